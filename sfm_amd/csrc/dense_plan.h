// Planning of the dense solver (dense.hip): the workspace layout, the map between a workgroup and its tile, the schedule of
// a factorisation launch by launch, the placement of the triangular solves and the two switches.  Plain C++17 for host and
// device, no HIP types and no launches: dense.hip executes it, tests/native/dense_plan_check.cpp (which defines
// SFM_DENSE_PLAN_STANDALONE) replays it tile by tile on the CPU under the sanitizers (tests/test_host_logic.py).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>

#if defined(__HIPCC__)
#define DENSE_HD __host__ __device__ __forceinline__
#else
#define DENSE_HD inline
#endif

#ifdef SFM_DENSE_PLAN_STANDALONE
static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }      // as in common.h
#endif

// ---- the switches.  Read per call of dense_cholesky / dense_trsv, never cached: tests switch them within one process.
constexpr int CHOL_STRIP_MIN_N = 4096;       // systems at least this large use the two-level (strip + rank-256 update) scheme
constexpr int TRSV_FLOW_MAX_BLOCKS = 128;    // 128-row blocks up to which a triangular solve is one launch (k_trsv_flow)
struct DenseSwitches {
  int strip_min_n;     // SFM_CHOL_STRIP_MIN_N: a TEST knob - the two-level scheme from this size on
  bool trsv_flow;      // SFM_TRSV_FLOW=0: one launch per block (the path taken for n > 16384)
};
static inline DenseSwitches dense_switches_from_env() {
  DenseSwitches s;
  const char* strip = getenv("SFM_CHOL_STRIP_MIN_N");
  s.strip_min_n = strip ? atoi(strip) : CHOL_STRIP_MIN_N;
  const char* flow = getenv("SFM_TRSV_FLOW");
  s.trsv_flow = !(flow && flow[0] == '0');
  return s;
}

// ---- workspace: offsets in doubles of the regions of DenseWs (dense.h), in this order, and their sum
struct DenseWsLayout { int64_t Ld, Dinv, DinvT, inv64, flag, Lm, LmT, total; };
static inline DenseWsLayout dense_ws_layout(int n) {
  const int64_t nb = (n + 127) / 128;
  DenseWsLayout l;
  int64_t p = 0;
  l.Ld = p; p += 2 * 64 * 64;
  l.Dinv = p; p += nb * 128 * 128;
  l.DinvT = p; p += nb * 128 * 128;
  l.inv64 = p; p += nb * 2 * 64 * 64;                      // an odd count of 64-blocks leaves room for the identity partner
  l.flag = p; p += 32;
  l.Lm = p; p += align_up((int64_t)(n + 1) * n, 32);
  l.LmT = p; p += (int64_t)n * n;
  l.total = p;
  return l;
}

// ---- 1-D order over the lower-triangular tiles: b -> (ti, tj), tj <= ti, b = ti (ti + 1) / 2 + tj.  The float seed is
// exact while 8 b + 1 < 2^24; the two loops correct it beyond that.
DENSE_HD unsigned tri_count(unsigned T) { return T * (T + 1) / 2; }
struct TileIJ { int ti, tj; };
DENSE_HD TileIJ tri_tile(int b) {
  int ti = (int)((sqrtf(8.0f * (float)b + 1.0f) - 1.0f) * 0.5f);
  while ((ti + 1) * (ti + 2) / 2 <= b) ++ti;
  while (ti * (ti + 1) / 2 > b) --ti;
  return {ti, b - ti * (ti + 1) / 2};
}

// ---- one 64-column step of the factorisation (k_chol_step): the panel at j0, the trailing columns [j1, col_end) it
// updates (col_end = n, or the end of the current 256-column strip), in 64x64 tiles (ti, tj) counted from (j1, j1)
struct CholStep {
  int nb;              // columns of the panel (64, fewer in the last one)
  int j1;              // first row and column behind the panel
  int rem_r, rem_c;    // rows [j1, nrows) and columns [j1, col_end) behind it; rem_c <= 0: panel solve only
  int T, tcols;        // tile rows; tile columns (the strip case enumerates tcols of them)
  bool whole;          // col_end >= n, the last or only strip: the whole trailing triangle
};
DENSE_HD CholStep chol_step(int n, int nrows, int j0, int col_end) {
  CholStep s;
  s.nb = (n - j0) < 64 ? (n - j0) : 64;
  s.j1 = j0 + s.nb;
  s.rem_r = nrows - s.j1;
  s.rem_c = col_end - s.j1;
  s.T = (s.rem_r + 63) / 64;
  s.tcols = ((s.rem_c > 0 ? s.rem_c : 0) + 63) / 64;
  s.whole = col_end >= n;
  return s;
}
// workgroups of the step (rem_r > 0) ...
DENSE_HD unsigned chol_step_grid(const CholStep& s) {
  const unsigned T = (unsigned)s.T;
  if (s.rem_c <= 0) return T;                              // panel solve only (strip end / bordered row)
  if (s.whole) return tri_count(T);
  unsigned grid = 0;
  for (int c = 0; c < s.tcols; ++c) grid += T - c;
  return grid;
}
// ... and the tile of workgroup b among them
DENSE_HD TileIJ chol_step_tile(int b, const CholStep& s) {
  TileIJ t;
  if (s.rem_c <= 0) {                   // no columns to update: one tile per 64 rows
    t.ti = b; t.tj = 0;
  } else if (s.whole) {
    t = tri_tile(b);
  } else {
    // strip: column tj holds the tiles ti = tj .. T - 1, columns one after the other (at most 4 of them)
    t.tj = 0;
    int rest = b;
    while (rest >= s.T - t.tj) { rest -= s.T - t.tj; ++t.tj; }
    t.ti = t.tj + rest;
  }
  return t;
}
// Every tile with tj == 0 writes its panel rows X_I to Lm.  The transposed copy LmT of those rows comes from the same
// tile, except for the rows of tile (0,0) - the workgroup that carries the serial chain: tile (1,0), where the launch has
// one, holds the same rows as its X_J and writes them instead.
DENSE_HD bool chol_has_tile10(const CholStep& s) { return s.rem_c > 0 && s.rem_r > 64; }
DENSE_HD bool chol_tile_writes_own_lmt(const CholStep& s, int ti, int tj) { return tj == 0 && !(ti == 0 && chol_has_tile10(s)); }
DENSE_HD bool chol_tile_writes_lmt_of_tile00(int ti, int tj) { return ti == 1 && tj == 0; }      // asked where ti != tj, rem_c > 0
// LOOK-AHEAD: tile (0,0) of a step with columns left factors the next diagonal block; only then are the step's Dn and
// inv64_next written (a step without them is still handed both pointers, the second possibly one past the end)
DENSE_HD bool chol_step_looks_ahead(const CholStep& s) { return s.rem_c > 0; }

// ---- the schedule of dense_cholesky.  Strips of 256 columns from strip_min_n unknowns on, else one strip; per strip
// k_chol_diag on its first block, one k_chol_step per 64 columns while rows are left, k_syrk_lower on what lies behind
// the strip; at the end the block inverses for the solves.  `step` counts the k_chol_step launches: launch `step` reads
// the step data in slot step & 1 of Ld and its look-ahead leaves the next block's in the other one, where launch
// step + 1 reads; a strip's k_chol_diag writes the slot its first step reads.
enum CholLaunchKind { CHOL_DIAG, CHOL_STEP, CHOL_SYRK, CHOL_INV64_FIX, CHOL_IDENTITY, CHOL_MERGE };
struct CholLaunch {
  CholLaunchKind kind;
  int j0, col_end;         // DIAG: the block at j0; STEP: the panel at j0, columns up to col_end; SYRK: the strip [j0, col_end)
  unsigned grid;
  int ld_read, ld_write;   // slots of Ld handed to the kernel as D / Dn (-1: none)
  int inv64_block;         // 64x64 block of inv64 handed to the kernel (DIAG: written; STEP: written by the look-ahead;
                           // IDENTITY: the partner of an odd last block), else -1: INV64_FIX and MERGE take the whole array
  int R, Cn, K;            // SYRK: rows, columns, inner dimension
  int64_t c_off, x_off;    // SYRK: offsets of C inside A and of X inside Lm (doubles)
};
template <class F>
static inline void for_each_chol_launch(int n, int nrows, int strip_min_n, F&& f) {
  const int strip = n >= strip_min_n ? 256 : n;
  int step = 0;
  for (int jb = 0; jb < n; jb += strip) {
    const int je = (jb + strip) < n ? (jb + strip) : n;            // columns [jb, je) form this strip
    f(CholLaunch{CHOL_DIAG, jb, je, 1u, -1, step & 1, jb / 64, 0, 0, 0, 0, 0});
    for (int j0 = jb; j0 < je; j0 += 64, ++step) {
      const CholStep s = chol_step(n, nrows, j0, je);
      if (s.rem_r <= 0) break;
      f(CholLaunch{CHOL_STEP, j0, je, chol_step_grid(s), step & 1, (step + 1) & 1, s.j1 / 64, 0, 0, 0, 0, 0});
    }
    if (je < n) {
      const int R = nrows - je, Cn = n - je;
      f(CholLaunch{CHOL_SYRK, jb, je, tri_count((unsigned)((R + 127) / 128)), -1, -1, -1, R, Cn, je - jb,
                   (int64_t)je * n + je, (int64_t)je * n + jb});
    }
  }
  // 64x64 and then 128x128 diagonal-block inverses for the triangular solves
  const unsigned nb64 = (unsigned)((n + 63) / 64), nb128 = (unsigned)((n + 127) / 128);
  f(CholLaunch{CHOL_INV64_FIX, 0, n, nb64, -1, -1, -1, 0, 0, 0, 0, 0});
  if ((nb64 & 1u) != 0)             // odd number of 64-blocks: the partner of the last one is an identity block
    f(CholLaunch{CHOL_IDENTITY, 0, n, 1u, -1, -1, (int)nb64, 0, 0, 0, 0, 0});
  f(CholLaunch{CHOL_MERGE, 0, n, nb128, -1, -1, -1, 0, 0, 0, 0, 0});
}

// ---- triangular solves over nblk = ceil(n / 128) blocks
static inline bool trsv_takes_flow(int nblk, const DenseSwitches& sw) { return nblk <= TRSV_FLOW_MAX_BLOCKS && sw.trsv_flow; }
// k_trsv_flow: every working workgroup must be resident at once, one per CU.  Workgroups go round-robin over the 8 XCDs,
// so worker p (its position in the dependency order) sits at blockIdx 8 p + xcd(p) with 32 consecutive workers per XCD
// (32 CUs each): hand-offs between neighbours stay inside one L2.  The other seven of every eight workgroups exit at once.
DENSE_HD unsigned trsv_flow_grid(int nblk) { return 8u * (unsigned)nblk; }
DENSE_HD bool trsv_flow_worker(int block_idx, int& p) {    // false: a workgroup that exits
  p = block_idx >> 3;
  return (block_idx & 7) == ((p >> 5) & 7);
}
// the block of worker p: the backward solve walks the blocks from the last one
DENSE_HD int trsv_flow_block(int p, int nblk, bool transpose) { return transpose ? nblk - 1 - p : p; }
// k_trsv_step, one launch per block: forward, 32 of the rows behind block blk per workgroup; backward, 256 of the rows
// before it; one workgroup (for the block's own solve) where none are left
DENSE_HD unsigned trsv_step_grid_forward(int n, int blk) {
  const int after = n - (blk * 128 + 128);
  return after > 0 ? (unsigned)((after + 31) / 32) : 1u;
}
DENSE_HD unsigned trsv_step_grid_backward(int blk) {
  const int before = blk * 128;
  return before > 0 ? (unsigned)((before + 255) / 256) : 1u;
}
