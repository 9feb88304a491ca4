// Host-only check of sfm_amd/csrc/match_plan.h, built with -fsanitize=address,undefined by tests/test_host_logic.py.
// Random segment tables -> plan_segments: every (query row, train row) of every segment must be covered by exactly one
// piece, pieces stay inside their segment, splits are whole 128-row chunks except the last, output rows are the
// segment's query rows in order; pick_nsplit respects its limits; match_u8_kernel picks the expected uint8 kernel, filter
// and split weights on each side of its thresholds.  The rest of the header, which is the whole host side of match.hip:
// the workspace layout over a grid of sizes (aligned, ordered, disjoint, large enough, totals equal to those of the
// hand-carved layout it replaced), the sizing calls against the calls they size (for the same random segment tables and
// every admitted metric and dim), the route table, every branch of every argument check with its firing order, and the
// grid functions against the expressions they stand for.  Prints "ok <pieces>" or a diagnostic and exits 1.
#define SFM_MATCH_PLAN_STANDALONE 1
#include "match_plan.h"
#include <cstdio>
#include <random>

static int fail(const char* what, long a, long b) { std::printf("FAIL %s %ld %ld\n", what, a, b); return 1; }

// every (metric, dim) the checks admit
struct MetricDim { int metric, dim; };
static const MetricDim ADMITTED[] = {{SFM_METRIC_L2_U8, 32}, {SFM_METRIC_L2_U8, 64}, {SFM_METRIC_L2_U8, 128}, {SFM_METRIC_L2_F32, 32}, {SFM_METRIC_L2_F32, 64},
                                     {SFM_METRIC_L2_F32, 128}, {SFM_METRIC_HAMMING, 16}, {SFM_METRIC_HAMMING, 32}, {SFM_METRIC_HAMMING, 64}};
static const int64_t ROWS[] = {1, 2, 127, 128, 129, 255, 256, 257, 1 << 20, 0x7FFFFF00LL};

// ---- layout: offsets aligned, regions in the declared order and disjoint, each as large as what is written into it
static int check_layout() {
  for (int64_t n_out : ROWS) for (int64_t nt : ROWS) for (int64_t nq : ROWS) for (int64_t plan_bytes : {(int64_t)0, (int64_t)1237}) for (int bits = 0; bits < 2; ++bits) {
    const MatchLayout L = match_layout(n_out, nt, nq, plan_bytes, bits != 0);
    const int64_t row = bits ? MATCH_BITS_ROW_BYTES : MATCH_ROW_BYTES;
    const int64_t tiled_rows = (nt + 31) / 32 * 32;                         // k_train_tile_u8 writes whole 32-row tiles, k_train_prep_u8 nt + 1 rows
    if (tiled_rows > nt + MATCH_PAD_ROWS || nt + 1 > nt + MATCH_PAD_ROWS) return fail("padding rows", (long)nt, (long)tiled_rows);
    if (tiled_rows / 32 * 2 > nt + 1) return fail("parity words of the tiles", (long)nt, 0);
    struct Region { const char* name; int64_t at, size; };
    const Region regions[] = {
        {"part", L.part, MATCH_MAX_SPLITS * n_out * MATCH_TOP * MATCH_CAND_BYTES},
        {"tf", L.tf, (nt + MATCH_PAD_ROWS) * row},
        {"qbits", L.qbits, nq * MATCH_BITS_ROW_BYTES},
        {"tbits", L.tbits, nt * MATCH_BITS_ROW_BYTES},
        {"th", L.th, (nt + MATCH_PAD_ROWS) * 4},
        {"par", L.par, (nt + 1) * 4},
        {"qn", L.qn, nq * 4},
        {"u2", L.u2, (n_out + MATCH_U2_SLACK) * 4},
        {"ratio", L.ratio, (n_out + MATCH_BLOCK - 1) / MATCH_BLOCK * 8 + 64},
        {"fix_list", L.fix_list, n_out * 4},
        {"fix_cnt", L.fix_cnt, 4},
        {"plan", L.plan, plan_bytes},
    };
    int64_t end = 0;
    for (const Region& r : regions) {
      const bool bit_region = r.name[1] == 'b';                            // qbits, tbits
      if (bit_region && !bits) { if (r.at != -1) return fail("bit region without bits", (long)r.at, 0); continue; }
      if (r.at < 0 || r.at % 256 != 0) return fail(r.name, (long)r.at, 256);
      if (r.at < end) return fail("regions overlap or out of order", (long)r.at, (long)end);
      if (r.size < 0) return fail("region size", (long)r.size, 0);
      end = r.at + r.size;
    }
    if (L.part != 0) return fail("first region", (long)L.part, 0);
    if (L.bytes < end || L.bytes <= 0) return fail("bytes", (long)L.bytes, (long)end);
    if (match_ratio_scratch_bytes(n_out, true) != regions[8].size || match_ratio_scratch_bytes(n_out) != regions[8].size - 64) return fail("ratio scratch", (long)n_out, 0);
    if (match_part_bytes(n_out) != regions[0].size || match_u2_count(n_out) * 4 != regions[7].size) return fail("part / u2", (long)n_out, 0);
  }
  // totals of the hand-carved layout this header replaced (computed with that function, not with this header)
  struct Total { int64_t n_out, nt, nq; int plan_bytes; bool bits; int64_t bytes; };
  const Total totals[] = {
      {1LL, 2LL, 1LL, 0, false, 7936LL},
      {1LL, 2LL, 1LL, 0, true, 13056LL},
      {257LL, 1025LL, 257LL, 0, false, 183040LL},
      {257LL, 1025LL, 257LL, 0, true, 646400LL},
      {127LL, 129LL, 255LL, 1237, false, 44032LL},
      {128LL, 256LL, 257LL, 1237, true, 229632LL},
      {1048576LL, 1048576LL, 1048576LL, 0, false, 289446400LL},
      {1048576LL, 1048576LL, 1048576LL, 1237, true, 960540416LL},
      {2147483392LL, 2147483392LL, 2147483392LL, 0, false, 592772531712LL},
      {2147483392LL, 2147483392LL, 2147483392LL, 1237, true, 1967161907968LL},
      {256LL, 1LL, 2LL, 0, false, 41984LL},
      {2LL, 2147483392LL, 129LL, 1237, false, 292057750784LL},
      {255LL, 127LL, 1048576LL, 0, true, 272741120LL},
  };
  for (const Total& e : totals)
    if (match_layout(e.n_out, e.nt, e.nq, e.plan_bytes, e.bits).bytes != e.bytes) return fail("total", (long)e.n_out, (long)e.bytes);
  return 0;
}

// ---- the plan region holds n_wgs records and the four segment arrays, inside plan_bytes
static int check_plan_region(int64_t n_wgs, int64_t n_seg) {
  const MatchPlanLayout P = match_plan_layout(n_wgs, n_seg);
  if (P.wg != 0 || P.wg_bytes != n_wgs * (int64_t)sizeof(MatchWG) || P.in_bytes != n_seg * 8 || P.out_bytes != (n_seg + 1) * 8) return fail("plan sizes", (long)n_wgs, (long)n_seg);
  if (P.q_beg < P.wg + P.wg_bytes || P.q_beg % 8 != 0) return fail("plan q_beg", (long)P.q_beg, (long)P.wg_bytes);
  if (P.t_beg < P.q_beg + P.out_bytes || P.t_end < P.t_beg + P.out_bytes || P.out_ptr < P.t_end + P.out_bytes) return fail("plan segment arrays", (long)n_wgs, (long)n_seg);
  if (P.out_ptr + P.out_bytes > P.bytes || match_plan_bytes(n_wgs, n_seg) != P.bytes) return fail("plan bytes", (long)P.bytes, (long)P.out_ptr);
  return 0;
}

// ---- sizing covers the call: one segment table, every admitted (metric, dim); nq_rows / nt_rows = rows of the two arrays
static int check_sizing_covers(int n_seg, const int64_t* qb, const int64_t* qe, const int64_t* tb, const int64_t* te, int64_t n_rows) {
  for (const MetricDim& m : ADMITTED) {
    const MatchRoute worst = match_route_largest(m.metric), r = match_route(m.metric, m.dim);
    std::vector<MatchWG> sized, called; std::vector<int64_t> sized_out, called_out;
    plan_segments(worst.metric, worst.dim, n_seg, qb, qe, tb, te, &sized, &sized_out);
    plan_segments(r.metric, r.dim, n_seg, qb, qe, tb, te, &called, &called_out);
    const int64_t n_out = called_out[n_seg];
    if (sized_out[n_seg] != n_out) return fail("output rows of the two plans", (long)sized_out[n_seg], (long)n_out);
    if (sized.size() < called.size()) return fail("the sized plan is shorter", (long)sized.size(), (long)called.size());
    if (check_plan_region((int64_t)called.size(), n_seg) || check_plan_region((int64_t)sized.size(), n_seg)) return 1;
    const int64_t reported = match_layout(n_out > 0 ? n_out : 1, n_rows, n_rows, match_plan_bytes((int64_t)sized.size(), n_seg), worst.bits).bytes;
    if (n_out < 1) continue;                                               // the call is refused (no query rows)
    const MatchPlanLayout P = match_plan_layout((int64_t)called.size(), n_seg);
    const MatchLayout L = match_layout(n_out, n_rows, n_rows, P.bytes, r.bits);
    if (reported < L.bytes) return fail("sizing below the call", (long)reported, (long)L.bytes);
    if (L.plan + P.bytes > L.bytes) return fail("plan region outside the layout", (long)L.plan, (long)P.bytes);
    if (worst.bits < r.bits) return fail("sized without the bit regions", m.metric, m.dim);
    // (sfm_match_workspace_bytes is told the dim: it and sfm_match_knn2 evaluate one expression, match_layout under
    // match_route(metric, dim), so there is nothing to compare for the single call; check_layout covers that layout)
  }
  return 0;
}

// ---- route: written out for every admitted pair
static int check_route() {
  struct Row { int metric, dim, to_metric, to_dim; bool bits; };
  const Row rows[] = {{SFM_METRIC_L2_U8, 32, SFM_METRIC_L2_U8, 32, false},     {SFM_METRIC_L2_U8, 64, SFM_METRIC_L2_U8, 64, false},
                      {SFM_METRIC_L2_U8, 128, SFM_METRIC_L2_U8, 128, false},   {SFM_METRIC_L2_F32, 32, SFM_METRIC_L2_F32, 32, false},
                      {SFM_METRIC_L2_F32, 64, SFM_METRIC_L2_F32, 64, false},   {SFM_METRIC_L2_F32, 128, SFM_METRIC_L2_F32, 128, false},
                      {SFM_METRIC_HAMMING, 16, SFM_METRIC_L2_U8, 128, true},   {SFM_METRIC_HAMMING, 32, SFM_METRIC_L2_U8, 256, true},
                      {SFM_METRIC_HAMMING, 64, SFM_METRIC_HAMMING, 64, false}};
  if (sizeof(rows) / sizeof(rows[0]) != sizeof(ADMITTED) / sizeof(ADMITTED[0])) return fail("route table size", 0, 0);
  for (const Row& e : rows) {
    const MatchRoute r = match_route(e.metric, e.dim);
    if (r.metric != e.to_metric || r.dim != e.to_dim || r.bits != e.bits || match_unpacks_bits(e.metric, e.dim) != e.bits) return fail("route", e.metric, e.dim);
    if (match_check_metric(e.metric, e.dim) != MATCH_FINE) return fail("admitted pair refused", e.metric, e.dim);
    if (match_check_route(r) != MATCH_FINE) return fail("Hamming other than 64 bytes on the popcount kernel", e.metric, e.dim);
    const MatchRoute worst = match_route_largest(e.metric);
    if (worst.metric != e.metric || worst.bits != (e.metric == SFM_METRIC_HAMMING)) return fail("largest route", e.metric, worst.bits);
  }
  // a Hamming width that reached the popcount kernel without being 64 bytes would be refused; no other route is
  for (int dim : {16, 32, 48, 128})
    if (match_check_route(MatchRoute{SFM_METRIC_HAMMING, dim, false}) != MATCH_WHY_POPCOUNT_DIM) return fail("popcount dim", dim, 0);
  if (match_check_route(MatchRoute{SFM_METRIC_L2_U8, 256, true}) != MATCH_FINE || match_check_route(MatchRoute{SFM_METRIC_L2_F32, 32, false}) != MATCH_FINE)
    return fail("route check on the other kernels", 0, 0);
  return 0;
}

// ---- checks: every branch once, from a valid call with one argument made bad
struct Knn2Args { int metric; const void* q; int64_t nq; const void* t; int64_t nt; int dim; const void *idx1, *idx2, *d1, *d2, *ws; };
static int run(const Knn2Args& a) { return match_check_knn2(a.metric, a.q, a.nq, a.t, a.nt, a.dim, a.idx1, a.idx2, a.d1, a.d2, a.ws); }
struct BatchArgs {
  int metric; const void* q; int64_t nq_rows; const void* t; int64_t nt_rows; int dim; int32_t n_seg;
  const int64_t *q_beg, *q_end, *t_beg, *t_end; const void *idx1, *idx2, *d1, *d2, *ws;
};
static int run(const BatchArgs& a) {
  return match_check_batched(a.metric, a.q, a.nq_rows, a.t, a.nt_rows, a.dim, a.n_seg, a.q_beg, a.q_end, a.t_beg, a.t_end, a.idx1, a.idx2, a.d1, a.d2, a.ws);
}
static int check_checks() {
  static char mem[8];
  const void* p = mem;
  for (int i = 1; i < MATCH_WHY_COUNT; ++i)
    if (!MATCH_WHY[i] || !MATCH_WHY[i][0]) return fail("empty text", i, 0);
  if (MATCH_WHY[MATCH_FINE][0]) return fail("text of 0", 0, 0);
  for (int i = 0; i < MATCH_WHY_COUNT; ++i)
    if (match_why_code(i) != (i == MATCH_FINE ? SFM_OK : i == MATCH_WHY_WORKSPACE ? SFM_ERR_WORKSPACE : SFM_ERR_ARG)) return fail("code", i, match_why_code(i));
  // metric / dim
  const int bad_dims[] = {0, 8, 16, 31, 33, 48, 63, 65, 96, 127, 129, 256, -32};
  for (int d : bad_dims) {
    if (d != 16 && match_check_metric(SFM_METRIC_HAMMING, d) != MATCH_WHY_DIM_HAMMING) return fail("hamming dim", d, 0);
    if (match_check_metric(SFM_METRIC_L2_U8, d) != MATCH_WHY_DIM_U8 || match_check_metric(SFM_METRIC_L2_F32, d) != MATCH_WHY_DIM_F32) return fail("l2 dim", d, 0);
  }
  if (match_check_metric(3, 32) != MATCH_WHY_METRIC || match_check_metric(-1, 32) != MATCH_WHY_METRIC) return fail("unknown metric", 0, 0);
  if (match_check_metric(3, 7) != MATCH_WHY_METRIC) return fail("unknown metric before its dim", 0, 0);
  // sfm_match_knn2
  const Knn2Args ok = {SFM_METRIC_L2_U8, p, 1, p, 2, 128, p, p, p, p, p};
  if (run(ok) != MATCH_FINE) return fail("valid knn2", run(ok), 0);
  for (int k = 0; k < 7; ++k) {
    Knn2Args a = ok;
    const void** ptrs[] = {&a.q, &a.t, &a.idx1, &a.idx2, &a.d1, &a.d2, &a.ws};
    *ptrs[k] = nullptr;
    if (run(a) != MATCH_WHY_NULL) return fail("knn2 null", k, run(a));
  }
  { Knn2Args a = ok; a.nq = 0; if (run(a) != MATCH_WHY_FEW_ROWS) return fail("nq 0", run(a), 0); }
  { Knn2Args a = ok; a.nt = 1; if (run(a) != MATCH_WHY_FEW_ROWS) return fail("nt 1", run(a), 0); }
  { Knn2Args a = ok; a.nq = 0x7FFFFF01LL; if (run(a) != MATCH_WHY_MANY_ROWS) return fail("nq many", run(a), 0); }
  { Knn2Args a = ok; a.nt = 0x7FFFFF01LL; if (run(a) != MATCH_WHY_MANY_ROWS) return fail("nt many", run(a), 0); }
  { Knn2Args a = ok; a.nq = a.nt = 0x7FFFFF00LL; if (run(a) != MATCH_FINE) return fail("most rows", run(a), 0); }
  { Knn2Args a = ok; a.dim = 96; if (run(a) != MATCH_WHY_DIM_U8) return fail("knn2 dim", run(a), 0); }
  { Knn2Args a = ok; a.metric = 7; if (run(a) != MATCH_WHY_METRIC) return fail("knn2 metric", run(a), 0); }
  // firing order: pointers, then too few rows, then too many, then the metric
  { Knn2Args a = ok; a.q = nullptr; a.nq = 0; a.metric = 7; if (run(a) != MATCH_WHY_NULL) return fail("order null", run(a), 0); }
  { Knn2Args a = ok; a.nq = 0; a.nt = 0x7FFFFF01LL; a.dim = 5; if (run(a) != MATCH_WHY_FEW_ROWS) return fail("order few", run(a), 0); }
  { Knn2Args a = ok; a.nt = 0x7FFFFF01LL; a.dim = 5; if (run(a) != MATCH_WHY_MANY_ROWS) return fail("order many", run(a), 0); }
  if (match_check_workspace(99, 100) != MATCH_WHY_WORKSPACE || match_check_workspace(100, 100) != MATCH_FINE) return fail("workspace", 0, 0);
  // sfm_match_knn2_batched: rows 0 .. 9 of either array, a segment without queries and two with
  const int64_t qb[3] = {4, 0, 4}, qe[3] = {4, 4, 10}, tb[3] = {0, 4, 0}, te[3] = {4, 10, 2};
  const BatchArgs okb = {SFM_METRIC_HAMMING, p, 10, p, 10, 32, 3, qb, qe, tb, te, p, p, p, p, p};
  if (run(okb) != MATCH_FINE) return fail("valid batch", run(okb), 0);
  for (int k = 0; k < 11; ++k) {
    BatchArgs a = okb;
    const void** ptrs[] = {&a.q, &a.t, &a.idx1, &a.idx2, &a.d1, &a.d2, &a.ws};
    const int64_t** segs[] = {&a.q_beg, &a.q_end, &a.t_beg, &a.t_end};
    if (k < 7) *ptrs[k] = nullptr; else *segs[k - 7] = nullptr;
    if (run(a) != MATCH_WHY_NULL_OR_NO_SEGMENTS) return fail("batch null", k, run(a));
  }
  { BatchArgs a = okb; a.n_seg = 0; if (run(a) != MATCH_WHY_NULL_OR_NO_SEGMENTS) return fail("n_seg 0", run(a), 0); }
  { BatchArgs a = okb; a.dim = 48; if (run(a) != MATCH_WHY_DIM_HAMMING) return fail("batch dim", run(a), 0); }
  { BatchArgs a = okb; a.metric = 9; if (run(a) != MATCH_WHY_METRIC) return fail("batch metric", run(a), 0); }
  { BatchArgs a = okb; a.nq_rows = 0x7FFFFF01LL; if (run(a) != MATCH_WHY_MANY_ROWS) return fail("batch nq many", run(a), 0); }
  { BatchArgs a = okb; a.nt_rows = 0x7FFFFF01LL; if (run(a) != MATCH_WHY_MANY_ROWS) return fail("batch nt many", run(a), 0); }
  for (int side = 0; side < 5; ++side) {
    int64_t b[4][3];
    for (int s = 0; s < 3; ++s) { b[0][s] = qb[s]; b[1][s] = qe[s]; b[2][s] = tb[s]; b[3][s] = te[s]; }
    if (side == 0) b[0][1] = -1;            // q_beg < 0
    if (side == 1) b[1][2] = 11;            // q_end > nq_rows
    if (side == 2) b[2][1] = -1;            // t_beg < 0
    if (side == 3) b[3][1] = 11;            // t_end > nt_rows
    if (side == 4) b[1][1] = -1;            // q_end < q_beg
    BatchArgs a = okb; a.q_beg = b[0]; a.q_end = b[1]; a.t_beg = b[2]; a.t_end = b[3];
    if (run(a) != MATCH_WHY_SEGMENT_OUTSIDE) return fail("segment outside", side, run(a));
  }
  { const int64_t te1[3] = {4, 10, 1}; BatchArgs a = okb; a.t_end = te1; if (run(a) != MATCH_WHY_SEGMENT_TRAIN_ROWS) return fail("one train row", run(a), 0); }
  { const int64_t te1[3] = {1, 10, 2}; BatchArgs a = okb; a.t_end = te1; if (run(a) != MATCH_FINE) return fail("one train row, no queries", run(a), 0); }
  { BatchArgs a = okb; a.n_seg = 1; if (run(a) != MATCH_WHY_NO_QUERIES) return fail("no queries", run(a), 0); }
  // firing order: pointers / n_seg, the metric, the row counts, the segments in turn, the empty batch
  { BatchArgs a = okb; a.q = nullptr; a.dim = 48; if (run(a) != MATCH_WHY_NULL_OR_NO_SEGMENTS) return fail("batch order null", run(a), 0); }
  { BatchArgs a = okb; a.dim = 48; a.nq_rows = 0x7FFFFF01LL; if (run(a) != MATCH_WHY_DIM_HAMMING) return fail("batch order metric", run(a), 0); }
  { const int64_t te1[3] = {4, 10, 1}; BatchArgs a = okb; a.t_end = te1; a.nt_rows = 0x7FFFFF01LL; if (run(a) != MATCH_WHY_MANY_ROWS) return fail("batch order rows", run(a), 0); }
  { const int64_t qb1[3] = {4, -1, 4}, te1[3] = {4, 10, 1}; BatchArgs a = okb; a.q_beg = qb1; a.t_end = te1; if (run(a) != MATCH_WHY_SEGMENT_OUTSIDE) return fail("batch order segments", run(a), 0); }
  { const int64_t qb1[3] = {4, 0, -1}, te1[3] = {4, 1, 2}; BatchArgs a = okb; a.q_beg = qb1; a.t_end = te1; if (run(a) != MATCH_WHY_SEGMENT_TRAIN_ROWS) return fail("batch order segments 2", run(a), 0); }
  // the ratio calls and the conversion
  if (match_check_ratio(1, p, p, p, p, p, p, p, p) != MATCH_FINE) return fail("valid ratio", 0, 0);
  for (int k = 0; k < 8; ++k) {
    const void* a[8] = {p, p, p, p, p, p, p, p};
    a[k] = nullptr;
    if (match_check_ratio(1, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]) != MATCH_WHY_BAD_ARGUMENT) return fail("ratio null", k, 0);
  }
  if (match_check_ratio(0, p, p, p, p, p, p, p, p) != MATCH_WHY_BAD_ARGUMENT) return fail("ratio nq 0", 0, 0);
  if (match_check_ratio_batched(1, p, p) != MATCH_FINE || match_check_ratio_batched(0, p, p) != MATCH_WHY_BAD_ARGUMENT ||
      match_check_ratio_batched(1, nullptr, p) != MATCH_WHY_BAD_ARGUMENT || match_check_ratio_batched(1, p, nullptr) != MATCH_WHY_BAD_ARGUMENT)
    return fail("ratio batched", 0, 0);
  if (match_check_f32_to_u8(p, 1, p, p) != MATCH_FINE || match_check_f32_to_u8(nullptr, 1, p, p) != MATCH_WHY_BAD_ARGUMENT ||
      match_check_f32_to_u8(p, 1, nullptr, p) != MATCH_WHY_BAD_ARGUMENT || match_check_f32_to_u8(p, 1, p, nullptr) != MATCH_WHY_BAD_ARGUMENT ||
      match_check_f32_to_u8(p, 0, p, p) != MATCH_WHY_BAD_ARGUMENT)
    return fail("f32_to_u8", 0, 0);
  return 0;
}

// ---- geometry: the grid functions against the expressions they replaced in match.hip
static unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }
static int check_geometry() {
  for (int64_t n : ROWS) {
    if (match_blocks(n) != cdiv(n, 256)) return fail("blocks", (long)n, 0);
    if (match_rerank_grid(n) != (n < 2048 ? (unsigned)n : 2048u)) return fail("rerank grid", (long)n, 0);
    if (match_ratio_scratch_bytes(n) != (int64_t)cdiv(n, 256) * 8 || match_ratio_scratch_bytes(n, true) != (int64_t)cdiv(n, 256) * 8 + 64) return fail("ratio bytes", (long)n, 0);
    for (int dim : {16, 32}) if (match_packed_bytes(n, dim) != n * dim) return fail("packed bytes", (long)n, dim);
    for (int dim : {32, 64, 128, 256}) {
      if (match_prep_grid(n, dim) != cdiv((n + 1) * (dim >> 4), 256)) return fail("prep grid", (long)n, dim);
      if (match_norm_grid(n, dim) != cdiv(n * (dim >> 4), 256)) return fail("norm grid", (long)n, dim);
    }
    for (int64_t m : ROWS) {
      const unsigned tb = (unsigned)((n + 31) >> 5);
      const MatchPrepass p4 = match_prepass(n, m, false), p8 = match_prepass(n, m, true);
      if (p4.tile_blocks != tb || p4.threads != 256 || p4.grid != tb + cdiv(m * 8, 256)) return fail("pre-pass dim 128", (long)n, (long)m);
      if (p8.tile_blocks != tb || p8.threads != 512 || p8.grid != tb + cdiv(m * 16, 512)) return fail("pre-pass dim 256", (long)n, (long)m);
      for (int64_t qpw : {(int64_t)256, (int64_t)512}) for (int nsplit = 1; nsplit <= 8; ++nsplit)
        if (match_grid(n, qpw, nsplit) != cdiv(n, qpw) * nsplit) return fail("grid", (long)n, nsplit);
    }
  }
  const int64_t tb[4] = {0, 5, 100, 7}, te[4] = {0, 9, 3000, 7};
  if (match_longest_segment(4, tb, te) != 2900 || match_longest_segment(2, tb, te) != 4 || match_longest_segment(1, tb, te) != 0) return fail("longest segment", 0, 0);
  return 0;
}

int main(int argc, char** argv) {
  if (check_layout() || check_route() || check_checks() || check_geometry()) return 1;
  std::mt19937_64 rng(argc > 1 ? std::atoll(argv[1]) : 1);
  long total_pieces = 0;
  for (int round = 0; round < 200; ++round) {
    const int n_seg = 1 + (int)(rng() % 40);
    const int metric = (int)(rng() % 3);
    const int dim = metric == SFM_METRIC_HAMMING ? 32 : (int[]){32, 64, 128}[rng() % 3];
    std::vector<int64_t> img_ptr(1, 0);
    const int n_img = 2 + (int)(rng() % 12);
    for (int i = 0; i < n_img; ++i) {
      const int kind = (int)(rng() % 5);
      const int64_t sz = kind == 0 ? 0 : kind == 1 ? 2 + (int64_t)(rng() % 40) : kind == 2 ? 200 + (int64_t)(rng() % 3000)
                                                   : kind == 3 ? 2048 + (int64_t)(rng() % 9000) : 511 + (int64_t)(rng() % 3);
      img_ptr.push_back(img_ptr.back() + sz);
    }
    std::vector<int64_t> qb(n_seg), qe(n_seg), tb(n_seg), te(n_seg);
    for (int s = 0; s < n_seg; ++s) {
      const int i = (int)(rng() % n_img), j = (int)(rng() % n_img);
      qb[s] = img_ptr[i]; qe[s] = img_ptr[i + 1]; tb[s] = img_ptr[j]; te[s] = img_ptr[j + 1];
    }
    std::vector<MatchWG> wgs; std::vector<int64_t> out_ptr;
    plan_segments(metric, dim, n_seg, qb.data(), qe.data(), tb.data(), te.data(), &wgs, &out_ptr);
    total_pieces += (long)wgs.size();
    if (check_sizing_covers(n_seg, qb.data(), qe.data(), tb.data(), te.data(), img_ptr.back())) return 1;
    size_t k = 0;
    for (int s = 0; s < n_seg; ++s) {
      const int64_t nq = qe[s] - qb[s], nt = te[s] - tb[s];
      if (out_ptr[s + 1] - out_ptr[s] != nq) return fail("out_ptr", s, (long)nq);
      if (nq <= 0) continue;
      const int64_t qpw = match_qpw(metric, dim, nq, true);
      for (int64_t q0 = 0; q0 < nq; q0 += qpw) {
        int64_t covered = 0; int split = 0;
        while (k < wgs.size() && wgs[k].q_first == qb[s] + q0 && wgs[k].t_seg == tb[s] && wgs[k].out_first == out_ptr[s] + q0) {
          const MatchWG& r = wgs[k];
          if (r.q_end != qe[s] || r.split != split) return fail("piece header", s, split);
          if (r.t_first != tb[s] + covered) return fail("split start", (long)r.t_first, (long)(tb[s] + covered));
          if (r.t_end > te[s] || r.t_end < r.t_first) return fail("split end", (long)r.t_end, (long)te[s]);
          if (r.t_end != te[s] && metric == SFM_METRIC_L2_U8 && (r.t_end - r.t_first) % 128 != 0) return fail("chunk multiple", s, split);
          covered += r.t_end - r.t_first; ++split; ++k;
          if (split > 8) return fail("more than 8 splits", s, split);
          if (covered == nt) break;
        }
        if (covered != nt && nt > 0) return fail("train rows covered", (long)covered, (long)nt);
        if (nt <= 0 && split != 1) return fail("empty train set pieces", s, split);
      }
    }
    if (k != wgs.size()) return fail("stray pieces", (long)k, (long)wgs.size());
  }
  for (int64_t nt : {2L, 511L, 512L, 1024L, 4095L, 50000L, 1000000L})
    for (int64_t nqb : {1L, 7L, 98L, 196L, 4000L}) {
      const int ns = pick_nsplit(nt, nqb);
      if (ns < 1 || ns > 8 || (ns > 1 && nt / ns < 512)) return fail("pick_nsplit", (long)nt, ns);
    }
  // the uint8 distance kernel on each side of every threshold of match_u8_kernel, for one pair planned as sfm_match_knn2
  // plans it (nsplit / grid checked where given: they decide the split weights)
  struct KernelCase { int64_t nq, nt; int dim; MatchU8Kernel kernel; bool filter; int w_first, w_second, nsplit; int64_t grid; };
  const KernelCase cases[] = {
      {50000, 50000, 128, MATCH_U8_DIRECT4, false, MATCH_W_FIRST, MATCH_W_SECOND, 5, 490},   // one round of two workgroups per CU
      {50000, 10240, 128, MATCH_U8_DIRECT4, false, MATCH_W_FIRST, MATCH_W_SECOND, 5, 490},   // 2,048 train rows per split
      {131072, 8192, 128, MATCH_U8_DIRECT4, false, MATCH_W_FIRST, MATCH_W_SECOND, 2, 512},   // 512 workgroups, two splits
      {50000, 10000, 128, MATCH_U8_DIRECT4, false, 0, 0, 5, 490},                            // 2,000 per split: even
      {150000, 600, 128, MATCH_U8_DIRECT4, false, 0, 0, 1, 293},                             // one split: even
      {28672, 2000, 128, MATCH_U8_DIRECT4, false, 0, 0, 3, 168},                             // 256 workgroups or fewer: even
      {300000, 50000, 128, MATCH_U8_DIRECT4, false, 0, 0, 6, 3516},                          // more than 512 workgroups: even
      {28671, 2000, 128, MATCH_U8_DIRECT2, false, 0, 0, 0, 0},                               // below 28,672 queries: two query blocks
      {20000, 20000, 128, MATCH_U8_DIRECT2, false, 0, 0, 6, 474},                            // weights only for four query blocks
      {20000, 400, 128, MATCH_U8_DIRECT2, false, 0, 0, 0, 0},                                // 8e6 distances
      {20000, 399, 128, MATCH_U8_LDS, false, 0, 0, 0, 0},                                    // below 8e6: the LDS kernel
      {20001, 3, 128, MATCH_U8_LDS, false, 0, 0, 0, 0},
      {2000, 2300, 128, MATCH_U8_LDS, true, 0, 0, 0, 0},                                     // the filter from 2,048 train rows
      {2000, 2048, 128, MATCH_U8_LDS, true, 0, 0, 0, 0},
      {2000, 2047, 128, MATCH_U8_LDS, false, 0, 0, 0, 0},
      {30000, 30000, 256, MATCH_U8_DIRECT2_KS8, false, 0, 0, 0, 0},                          // dim 256 (ORB over unpacked bits)
      {2000, 4000, 256, MATCH_U8_DIRECT2_KS8, false, 0, 0, 0, 0},
      {2000, 3999, 256, MATCH_U8_LDS, true, 0, 0, 0, 0},
      {30000, 30000, 64, MATCH_U8_LDS, true, 0, 0, 0, 0},                                    // dims below 128: always the LDS kernel
      {30000, 30000, 32, MATCH_U8_LDS, true, 0, 0, 0, 0},
  };
  for (const KernelCase& e : cases) {
    const int64_t qpw = match_qpw(SFM_METRIC_L2_U8, e.dim, e.nq, false);
    int nsplit; int64_t rps;
    match_tiling(SFM_METRIC_L2_U8, e.nq, qpw, e.nt, &nsplit, &rps);
    const int64_t grid = (e.nq + qpw - 1) / qpw * nsplit;
    const MatchU8Choice c = match_u8_kernel(e.dim, e.nq, e.nt, qpw, false, e.nt, grid, nsplit);
    if (c.kernel != e.kernel || c.filter != e.filter) return fail("kernel", (long)e.nq, (long)e.nt);
    if (c.w_first != e.w_first || c.w_second != e.w_second) return fail("split weights", (long)e.nq, (long)e.nt);
    if (e.nsplit && (nsplit != e.nsplit || grid != e.grid)) return fail("tiling", nsplit, (long)grid);
  }
  // a batched plan takes the LDS kernel whatever its size; the filter follows the longest segment
  for (int64_t longest : {2047L, 2048L, 30000L}) {
    const int64_t qb[2] = {0, 30000}, qe[2] = {30000, 60000}, tb[2] = {0, 1000}, te[2] = {1000, 1000 + longest};
    std::vector<MatchWG> wgs; std::vector<int64_t> out_ptr;
    plan_segments(SFM_METRIC_L2_U8, 128, 2, qb, qe, tb, te, &wgs, &out_ptr);
    const MatchU8Choice c = match_u8_kernel(128, 60000, 1000 + longest, 256, true, longest, (int64_t)wgs.size(), 1);
    if (c.kernel != MATCH_U8_LDS || c.filter != (longest >= 2048) || c.w_first || c.w_second) return fail("batched kernel", (long)longest, c.kernel);
  }
  std::printf("ok %ld\n", total_pieces);
  return 0;
}
