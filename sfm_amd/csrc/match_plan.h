// The whole host side of the matcher (match.hip) but the launches themselves: which kernels a call is routed to
// (match_route), the argument checks of every entry point (match_check_*, an index into MATCH_WHY), the layout of the
// caller's workspace (match_layout, match_plan_layout), how a (query set, train set) pair - or a batch of image pairs - is
// cut into workgroup-sized pieces (match_qpw, match_tiling, plan_segments) and the grids of the launches.  Plain C++ (no
// HIP): included by match.hip, and compiled on its own with the address and undefined-behaviour sanitizers by
// tests/test_host_logic.py (tests/native/match_plan_check.cpp, which defines SFM_MATCH_PLAN_STANDALONE).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

#ifdef SFM_MATCH_PLAN_STANDALONE
enum { SFM_METRIC_L2_U8 = 0, SFM_METRIC_L2_F32 = 1, SFM_METRIC_HAMMING = 2 };      // as in include/sfm_amd.h
enum { SFM_OK = 0, SFM_ERR_ARG = -1, SFM_ERR_WORKSPACE = -3 };
#endif

// Batched (segmented) matching: one launch covers every image pair of a preprocessing step
// (find_matches.py:329-350 calls match_features once per pair, serially).  A segment = one pair = a range of query
// rows against a range of train rows; the host cuts the segments into workgroup-sized pieces (plan_segments) and
// every workgroup of the distance kernels reads its piece from this record.  wg == nullptr = one segment covering
// the whole arrays, pieces computed from blockIdx.
struct MatchWG {
  int64_t q_first, q_end;     // query rows of this workgroup: [q_first, min(q_first + rows per workgroup, q_end))
  int64_t t_first, t_end;     // train rows of this workgroup's split
  int64_t t_seg;              // first train row of the segment: train indices are reported relative to it
  int64_t out_first;          // output row of q_first
  int32_t split, pad;
};
static inline int64_t plan_align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
static inline unsigned plan_cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

static inline int pick_nsplit(int64_t nt, int64_t n_qblocks) {
  // Splits of the train set buy parallelism (workgroups = query blocks x splits; the splits of one query block run side
  // by side and share their candidate threshold, so they do not loosen the filter).  The distance kernel holds two
  // workgroups per CU: take the split count (<= 8, splits of at least 512 rows) whose LAST round of 512 workgroups is
  // fullest - at 50k x 50k, 196 query blocks: 5 splits = 1.9 rounds against 8 = 3.06, 10 % of the launch.
  int best = 1;
  double best_cost = 1e30;
  for (int ns = 1; ns <= 8; ++ns) {
    const int64_t wgs = n_qblocks * ns, rounds = (wgs + 511) / 512;
    const double cost = (double)rounds / ns;             // time ~ rounds x rows per split
    if (cost < best_cost * 0.98) { best_cost = cost; best = ns; }
  }
  while (best > 1 && nt / best < 512) --best;
  return best;
}

// queries one workgroup of the distance kernel takes
static inline int64_t match_qpw(int metric, int dim, int64_t nq, bool batched) {
  // k_knn2_u8_direct with four query blocks per wave (512 queries per workgroup: half the train bytes per pair) once there
  // are enough queries to fill the chip that way; single segment, dim 128.  SFM_MATCH_QB = 2 / 4 forces either: a test hook
  // that lets the kernel-edge tests drive both direct instantiations at every size.
  const char* qb_env = getenv("SFM_MATCH_QB");
  // measured crossover (round 3, 20 calls each, us per call, 4 blocks / 2 blocks per wave): 12,288 queries 82 / 74,
  // 16,384: 98 / 89, 24,576: 166 / 146 (square sets; against 50,000 train rows 267 / 260), 32,768: 223 / 228 (301 / 317),
  // 40,960: 312 / 332, 50,000: 418 / 451 - two blocks (three waves per SIMD) win up to ~28k queries
  const bool qb4 = !batched && metric == SFM_METRIC_L2_U8 && dim == 128 && (qb_env ? qb_env[0] == '4' : nq >= 28672);
  return qb4 ? 512 : 256;
}

// rows of train data per split, and how many splits
static inline void match_tiling(int metric, int64_t nq, int64_t qpw, int64_t nt, int* nsplit, int64_t* rps) {
  int ns = pick_nsplit(nt, (nq + qpw - 1) / qpw);
  int64_t r = (nt + ns - 1) / ns;
  if (r < 1) r = 1;                                        // an empty train set: one (empty) piece, not a division by zero
  if (metric == SFM_METRIC_L2_U8) r = plan_align_up(r, 128);
  *nsplit = nt > 0 ? (int)((nt + r - 1) / r) : 1;
  *rps = r;
}

// the distance kernel of a uint8 launch (match.hip: match_launch)
enum MatchU8Kernel {
  MATCH_U8_LDS,            // k_knn2_u8<dim / 32, filter>: train rows staged through LDS
  MATCH_U8_DIRECT2,        // k_knn2_u8_direct<2>
  MATCH_U8_DIRECT4,        // k_knn2_u8_direct<4>
  MATCH_U8_DIRECT2_KS8     // k_knn2_u8_direct<2, 8>: dim 256 (ORB over unpacked bits)
};
struct MatchU8Choice {
  MatchU8Kernel kernel;
  bool filter;             // the LDS kernel's candidate filter (the direct kernels always filter)
  int w_first, w_second;   // the direct kernels' split weights (see MATCH_W_FIRST); 0 : 0 = even splits
};

// train rows per workgroup, first : second on a CU (k_knn2_u8_direct).  Measured at 50k x 50k, distance kernel by HIP events:
// even 378 us, 128:100 370, 135:100 367-368, 150:100 367 (the wave end stamps then lie within 306-354 us instead of 283-375)
constexpr int MATCH_W_FIRST = 135, MATCH_W_SECOND = 100;

// nq x nt rows of dim bytes in grid workgroups of qpw queries (match_qpw) and nsplit train splits; batched = a plan of
// segments (plan_segments), the longest of them with longest_nt train rows (nt for one pair)
static inline MatchU8Choice match_u8_kernel(int dim, int64_t nq, int64_t nt, int64_t qpw, bool batched, int64_t longest_nt,
                                            int64_t grid, int nsplit) {
  MatchU8Choice c = {MATCH_U8_LDS, false, 0, 0};
  // one pair at dim 128: the LDS-free kernel, with 4 query blocks per wave from 28,672 queries on and 2 below (8-20 % faster
  // than the LDS kernel at 2,000 .. 11,000 queries against 4,000 .. 50,000 train rows); dim 256 (ORB over unpacked bits):
  // two query blocks per wave, eight MFMAs per step.  Below 8e6 distances a call is launch-bound and the LDS kernel's lighter
  // pre-pass wins by ~3 us; the LDS kernel also serves the batched form and the smaller dims.
  if (qpw == 512) {
    c.kernel = MATCH_U8_DIRECT4;
    // uneven train splits for the two workgroups of a CU (see the kernel): grids of one round at two workgroups per CU
    // only, splits long enough to cut
    if (grid > 256 && grid <= 512 && nsplit > 1 && nt / nsplit >= 2048) { c.w_first = MATCH_W_FIRST; c.w_second = MATCH_W_SECOND; }
  } else if (!batched && (dim == 128 || dim == 256) && (double)nq * (double)nt >= 8e6) {
    c.kernel = dim == 256 ? MATCH_U8_DIRECT2_KS8 : MATCH_U8_DIRECT2;
  } else {
    // the candidate filter pays once the queries see a few thousand train rows (see k_knn2_u8); below that it is 10
    // operations per tile for nothing
    c.filter = longest_nt >= 2048;
  }
  return c;
}

static inline void plan_segments(int metric, int dim, int32_t n_seg, const int64_t* q_beg, const int64_t* q_end, const int64_t* t_beg,
                          const int64_t* t_end, std::vector<MatchWG>* wgs, std::vector<int64_t>* out_ptr) {
  out_ptr->assign((size_t)n_seg + 1, 0);
  int64_t all_queries = 0;                           // parallelism comes from all segments together
  for (int s = 0; s < n_seg; ++s) all_queries += (q_end[s] - q_beg[s] + 255) / 256 * 256;
  for (int s = 0; s < n_seg; ++s) {
    const int64_t nq = q_end[s] - q_beg[s], nt = t_end[s] - t_beg[s];
    (*out_ptr)[s + 1] = (*out_ptr)[s] + nq;
    if (nq <= 0) continue;
    int nsplit; int64_t rps;
    match_tiling(metric, all_queries, 256, nt, &nsplit, &rps);
    for (int64_t qb = 0; qb < nq; qb += match_qpw(metric, dim, nq, true))
      for (int sp = 0; sp < nsplit; ++sp) {          // consecutive workgroups = consecutive splits: one XCD per split as in the single-pair launch
        MatchWG r;
        r.q_first = q_beg[s] + qb; r.q_end = q_end[s];
        r.t_first = t_beg[s] + sp * rps; r.t_end = (r.t_first + rps) < t_end[s] ? (r.t_first + rps) : t_end[s];
        r.t_seg = t_beg[s]; r.out_first = (*out_ptr)[s] + qb; r.split = sp; r.pad = 0;
        wgs->push_back(r);
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------- route
// Hamming over 128- and 256-bit strings is unpacked to one byte per bit (k_unpack_bits) and runs as exact uint8 L2 on the
// int8 kernels at dim 128 / 256; the merge then reports d^2 itself, which is the popcount.  512 bits stay on the popcount
// kernel.
static inline bool match_unpacks_bits(int metric, int dim) { return metric == SFM_METRIC_HAMMING && dim <= 32; }

struct MatchRoute {
  int metric, dim;         // what the distance kernels see
  bool bits;               // the rows are unpacked first: two more workspace regions, no root in the merge
};
static inline MatchRoute match_route(int metric, int dim) {
  const bool bits = match_unpacks_bits(metric, dim);
  return bits ? MatchRoute{SFM_METRIC_L2_U8, dim * 8, true} : MatchRoute{metric, dim, false};
}
// sfm_match_batched_workspace_bytes is not told the dim and sizes for whichever route of the metric needs most.  Two
// things grow a batch's workspace.  The unpacked rows: some dim of the metric is unpacked <=> the smallest (16) is.  The
// number of plan records: every metric but L2_U8 cuts the train rows into splits that are not rounded up to 128 rows
// (match_tiling), so the plan under the caller's own metric is never shorter than under the route's, and the dim does not
// enter a batched plan at all (match_qpw).  Hence: planned as the caller's metric, laid out as the unpacked route.
static inline MatchRoute match_route_largest(int metric) { return MatchRoute{metric, 32, match_unpacks_bits(metric, 16)}; }

// --------------------------------------------------------------------------------------------------------------- layout
constexpr int64_t MATCH_BLOCK = 256;           // threads of every one-thread-per-item kernel; one count per block in the ratio scan
constexpr int64_t MATCH_MAX_SPLITS = 8;        // nsplit <= 8 (pick_nsplit)
constexpr int64_t MATCH_TOP = 2;               // candidates per query and split: the two nearest
constexpr int64_t MATCH_CAND_BYTES = 8;        // Cand { float d; int i; } (match.hip asserts it)
constexpr int64_t MATCH_PAD_ROWS = 32;         // padding rows behind the int8 copy of the train rows and their thresholds: one 32-row tile
constexpr int64_t MATCH_ROW_BYTES = 128;       // int8 copy of the train rows: dim <= 128 ...
constexpr int64_t MATCH_BITS_ROW_BYTES = 256;  // ... 256 for unpacked bits (one byte per bit, <= 256 bits)
constexpr int64_t MATCH_U2_SLACK = 128;        // shared candidate thresholds come in whole 128-query wave blocks
constexpr int64_t MATCH_WS_TAIL = 1024;        // slack behind the last region
constexpr int64_t MATCH_ROWS_MAX = 0x7FFFFF00LL;   // rows of either side: row indices and the padded counts stay in int32

static inline unsigned match_blocks(int64_t n) { return plan_cdiv(n, MATCH_BLOCK); }

// scratch of sfm_match_ratio (a count and an offset per block of 256 rows) and of sfm_match_ratio_batched (+ 64: the
// total, an int64 behind them)
static inline int64_t match_ratio_scratch_bytes(int64_t n, bool batched = false) {
  return (int64_t)match_blocks(n) * 8 + (batched ? 64 : 0);
}

static inline int64_t match_part_bytes(int64_t n_out) { return MATCH_MAX_SPLITS * n_out * MATCH_TOP * MATCH_CAND_BYTES; }
static inline int64_t match_u2_count(int64_t n_out) { return n_out + MATCH_U2_SLACK; }

// The plan region of a batch, as the kernels read it: workgroup records, then q_beg | t_beg | t_end | out_ptr, each of
// n_seg + 1 int64 (the three inputs fill n_seg of them).  Offsets are relative to MatchLayout::plan.
struct MatchPlanLayout {
  int64_t wg, q_beg, t_beg, t_end, out_ptr;
  int64_t wg_bytes, in_bytes, out_bytes;       // bytes copied: the records, one input array, out_ptr
  int64_t bytes;
};
static inline MatchPlanLayout match_plan_layout(int64_t n_wgs, int64_t n_seg) {
  MatchPlanLayout P;
  P.wg_bytes = n_wgs * (int64_t)sizeof(MatchWG);
  P.in_bytes = n_seg * 8;
  P.out_bytes = (n_seg + 1) * 8;
  P.wg = 0;
  P.q_beg = plan_align_up(P.wg_bytes, 256);
  P.t_beg = P.q_beg + P.out_bytes;
  P.t_end = P.t_beg + P.out_bytes;
  P.out_ptr = P.t_end + P.out_bytes;
  P.bytes = P.wg_bytes + 4 * P.out_bytes + 256;     // 256: what aligning the segment arrays can cost
  return P;
}
static inline int64_t match_plan_bytes(int64_t n_wgs, int64_t n_seg) { return match_plan_layout(n_wgs, n_seg).bytes; }

// byte offsets into the workspace of sfm_match_knn2 (plan_bytes = 0, nq_rows = n_out) and sfm_match_knn2_batched
struct MatchLayout {
  int64_t part;            // Cand [MATCH_MAX_SPLITS][n_out][MATCH_TOP]: per-split candidates
  int64_t tf;              // int8 copy of the train rows + padding, in the distance kernel's order
  int64_t qbits, tbits;    // bits only (else -1): the query / train rows unpacked to one byte per bit
  int64_t th;              // int32 [nt_rows + padding]: train norms (TN >> 1, SENT_TH for padding)
  int64_t par;             // int32 [nt_rows + 1]: their parity bits
  int64_t qn;              // int32 [nq_rows]: query norms
  int64_t u2;              // int32 [n_out + slack]: shared candidate thresholds
  int64_t ratio;           // reserved: room for sfm_match_ratio_batched's scratch.  No caller in this tree uses it (matcher.py
                           // hands the ratio call the base of the workspace, after the kNN is done with it); it stays
                           // because callers may have cached the byte counts
  int64_t fix_list;        // int32 [n_out]: queries to re-rank on the float32 value
  int64_t fix_cnt;         // int32: how many
  int64_t plan;            // batched only: MatchPlanLayout
  int64_t bytes;
};
static inline MatchLayout match_layout(int64_t n_out, int64_t nt_rows, int64_t nq_rows, int64_t plan_bytes, bool bits) {
  MatchLayout L;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { const int64_t at = off; off += plan_align_up(bytes, 256); return at; };
  L.part = take(match_part_bytes(n_out));
  L.tf = take((nt_rows + MATCH_PAD_ROWS) * (bits ? MATCH_BITS_ROW_BYTES : MATCH_ROW_BYTES));
  L.qbits = bits ? take(nq_rows * MATCH_BITS_ROW_BYTES) : -1;
  L.tbits = bits ? take(nt_rows * MATCH_BITS_ROW_BYTES) : -1;
  L.th = take((nt_rows + MATCH_PAD_ROWS) * 4);
  L.par = take((nt_rows + 1) * 4);
  L.qn = take(nq_rows * 4);
  L.u2 = take(match_u2_count(n_out) * 4);
  L.ratio = take(match_ratio_scratch_bytes(n_out, true));
  L.fix_list = take(n_out * 4);
  L.fix_cnt = take(256);
  L.plan = take(plan_bytes);
  L.bytes = off + MATCH_WS_TAIL;
  return L;
}

// --------------------------------------------------------------------------------------------------------------- checks
// 0 = fine, otherwise an index into MATCH_WHY; match_why_code gives the return code that goes with it
enum MatchWhy {
  MATCH_FINE = 0, MATCH_WHY_NULL, MATCH_WHY_FEW_ROWS, MATCH_WHY_MANY_ROWS, MATCH_WHY_DIM_U8, MATCH_WHY_DIM_F32, MATCH_WHY_DIM_HAMMING,
  MATCH_WHY_METRIC, MATCH_WHY_POPCOUNT_DIM, MATCH_WHY_WORKSPACE, MATCH_WHY_NULL_OR_NO_SEGMENTS, MATCH_WHY_SEGMENT_OUTSIDE,
  MATCH_WHY_SEGMENT_TRAIN_ROWS, MATCH_WHY_NO_QUERIES, MATCH_WHY_BAD_ARGUMENT, MATCH_WHY_COUNT
};
static const char* const MATCH_WHY[MATCH_WHY_COUNT] = {
    "", "null pointer", "needs nq >= 1 and nt >= 2", "too many rows", "L2_U8 needs dim 32, 64 or 128", "L2_F32 supports dim 32, 64, 128",
    "HAMMING supports dim 16, 32, 64 bytes", "unknown metric", "HAMMING on the popcount kernel needs dim 64", "workspace too small",
    "null pointer / no segments", "segment outside the descriptor arrays", "a segment with queries needs at least 2 train rows",
    "no query rows", "bad argument"};
static inline int match_why_code(int bad) { return bad == MATCH_FINE ? SFM_OK : bad == MATCH_WHY_WORKSPACE ? SFM_ERR_WORKSPACE : SFM_ERR_ARG; }

static inline int match_check_workspace(int64_t have, int64_t need) { return have < need ? MATCH_WHY_WORKSPACE : MATCH_FINE; }

// The popcount kernel (k_knn2_valu<2, 16>) exists for 64-byte rows only.  With the dims admitted below every other Hamming
// call is unpacked, so this cannot fire today; it stands between a Hamming width admitted later without a route and a
// kernel that would read its rows as 64 bytes.
static inline int match_check_route(const MatchRoute& r) {
  return r.metric == SFM_METRIC_HAMMING && r.dim != 64 ? MATCH_WHY_POPCOUNT_DIM : MATCH_FINE;
}
static inline int match_check_metric(int metric, int dim) {
  const bool sift_dim = dim == 32 || dim == 64 || dim == 128;
  if (metric == SFM_METRIC_L2_U8) return sift_dim ? MATCH_FINE : MATCH_WHY_DIM_U8;
  if (metric == SFM_METRIC_L2_F32) return sift_dim ? MATCH_FINE : MATCH_WHY_DIM_F32;
  if (metric != SFM_METRIC_HAMMING) return MATCH_WHY_METRIC;
  if (dim != 16 && dim != 32 && dim != 64) return MATCH_WHY_DIM_HAMMING;
  return match_check_route(match_route(metric, dim));
}

static inline int match_check_knn2(int metric, const void* q, int64_t nq, const void* t, int64_t nt, int dim, const void* idx1,
                                   const void* idx2, const void* d1, const void* d2, const void* workspace) {
  if (!q || !t || !idx1 || !idx2 || !d1 || !d2 || !workspace) return MATCH_WHY_NULL;
  if (nq < 1 || nt < 2) return MATCH_WHY_FEW_ROWS;
  if (nt > MATCH_ROWS_MAX || nq > MATCH_ROWS_MAX) return MATCH_WHY_MANY_ROWS;
  return match_check_metric(metric, dim);
}

static inline int match_check_batched(int metric, const void* q, int64_t nq_rows, const void* t, int64_t nt_rows, int dim, int32_t n_seg,
                                      const int64_t* q_beg, const int64_t* q_end, const int64_t* t_beg, const int64_t* t_end,
                                      const void* idx1, const void* idx2, const void* d1, const void* d2, const void* workspace) {
  if (!q || !t || !idx1 || !idx2 || !d1 || !d2 || !workspace || !q_beg || !q_end || !t_beg || !t_end || n_seg < 1)
    return MATCH_WHY_NULL_OR_NO_SEGMENTS;
  if (const int bad = match_check_metric(metric, dim)) return bad;
  if (nq_rows > MATCH_ROWS_MAX || nt_rows > MATCH_ROWS_MAX) return MATCH_WHY_MANY_ROWS;
  bool queries = false;
  for (int s = 0; s < n_seg; ++s) {
    if (q_beg[s] < 0 || q_end[s] < q_beg[s] || q_end[s] > nq_rows || t_beg[s] < 0 || t_end[s] > nt_rows) return MATCH_WHY_SEGMENT_OUTSIDE;
    if (q_end[s] > q_beg[s] && t_end[s] - t_beg[s] < 2) return MATCH_WHY_SEGMENT_TRAIN_ROWS;
    queries = queries || q_end[s] > q_beg[s];
  }
  return queries ? MATCH_FINE : MATCH_WHY_NO_QUERIES;
}

static inline int match_check_ratio(int64_t nq, const void* idx1, const void* d1, const void* d2, const void* query_idx,
                                    const void* train_idx, const void* dist, const void* n_matches, const void* workspace) {
  return (!idx1 || !d1 || !d2 || !query_idx || !train_idx || !dist || !n_matches || !workspace || nq < 1) ? MATCH_WHY_BAD_ARGUMENT : MATCH_FINE;
}
// the arrays it hands on are checked by sfm_match_ratio, which it calls
static inline int match_check_ratio_batched(int32_t n_seg, const void* out_ptr, const void* seg_match_ptr) {
  return (!out_ptr || !seg_match_ptr || n_seg < 1) ? MATCH_WHY_BAD_ARGUMENT : MATCH_FINE;
}
static inline int match_check_f32_to_u8(const void* src, int64_t n_elems, const void* dst, const void* all_integral) {
  return (!src || !dst || !all_integral || n_elems < 1) ? MATCH_WHY_BAD_ARGUMENT : MATCH_FINE;
}

// ------------------------------------------------------------------------------------------------------------- geometry
// workgroups of one pair: query blocks x train splits
static inline unsigned match_grid(int64_t nq, int64_t qpw, int nsplit) { return plan_cdiv(nq, qpw) * nsplit; }

// train rows of a batch's longest segment: they decide the candidate filter (match_u8_kernel)
static inline int64_t match_longest_segment(int32_t n_seg, const int64_t* t_beg, const int64_t* t_end) {
  int64_t longest = 0;
  for (int s = 0; s < n_seg; ++s) longest = (t_end[s] - t_beg[s]) > longest ? (t_end[s] - t_beg[s]) : longest;
  return longest;
}

// The direct kernels' pre-pass (k_train_tile_u8<4> at dim 128, <8> at dim 256): one workgroup per 32-row train tile, then
// workgroups that take the query norms 16 bytes per thread.
struct MatchPrepass { unsigned tile_blocks, grid, threads; };
static inline MatchPrepass match_prepass(int64_t nt_rows, int64_t nq_rows, bool dim256) {
  MatchPrepass p;
  p.tile_blocks = (unsigned)((nt_rows + 31) >> 5);
  p.threads = dim256 ? 512 : 256;
  p.grid = p.tile_blocks + plan_cdiv(nq_rows * (dim256 ? 16 : 8), p.threads);
  return p;
}
// the LDS kernel's pre-pass: k_train_prep_u8 (train rows + the sentinel row) and k_row_norm_u8, 16 bytes per thread
static inline unsigned match_prep_grid(int64_t nt_rows, int dim) { return match_blocks((nt_rows + 1) * (dim >> 4)); }
static inline unsigned match_norm_grid(int64_t nq_rows, int dim) { return match_blocks(nq_rows * (dim >> 4)); }
// k_unpack_bits: one thread per packed byte
static inline int64_t match_packed_bytes(int64_t rows, int dim) { return rows * dim; }
// k_knn2_u8_rerank: workgroups stride over the listed queries
static inline unsigned match_rerank_grid(int64_t n_out) { return n_out < 2048 ? (unsigned)n_out : 2048u; }
