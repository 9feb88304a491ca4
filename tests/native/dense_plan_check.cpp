// Host-only check of sfm_amd/csrc/dense_plan.h, built with -fsanitize=address,undefined by tests/test_host_logic.py.
// Replays the schedule of the factorisation (for_each_chol_launch) and the decode of every workgroup of every launch - the
// functions dense.hip itself runs - at 64x64 tile granularity, and asserts what the kernels rely on: every workgroup has a
// tile and no two share one, every row tile below a panel is solved once, every trailing tile receives every earlier panel's
// update once (from a step of the panel's strip or from the strip's k_syrk_lower), a step reads the step data the previous
// producer wrote, every block inverse and every tile row of the transposed copy is written once.  Then the triangular decode,
// the workspace layout against the formulas written out, the placement of k_trsv_flow and the grids of k_trsv_step.
// Prints "ok <tiles visited> tiles, <idle> idle" or a diagnostic and exits 1.
#define SFM_DENSE_PLAN_STANDALONE 1
#include "dense_plan.h"
#include <cstdio>
#include <vector>

static int fail(const char* what, long n, long nrows, long a, long b) {
  std::printf("FAIL %s: n %ld nrows %ld: %ld %ld\n", what, n, nrows, a, b);
  return 1;
}
#define CHECK(cond, what, a, b) do { if (!(cond)) return fail(what, n, nrows, (long)(a), (long)(b)); } while (0)

static long tiles_visited = 0, idle_tiles = 0;

// One factorisation.  full: with the bookkeeping of solves, updates and the transposed copy (small n); without it the grids
// and the decode only.
static int check_factorisation(int n, int nrows, int strip_min_n, bool full) {
  std::vector<CholLaunch> launches;
  for_each_chol_launch(n, nrows, strip_min_n, [&](const CholLaunch& l) { launches.push_back(l); });

  const int nb64 = (n + 63) / 64, nb128 = (n + 127) / 128;
  const int G = (nrows + 63) / 64;                      // 64-row tiles of the matrix, the bordered row's included
  // upd[(k * G + gi) * G + gj]: updates of panel k received by the tile at rows 64 gi, columns 64 gj
  std::vector<unsigned char> upd(full ? (size_t)nb64 * G * G : 0, 0);
  std::vector<int> inv_written(2 * nb128 + 1, 0), panel_steps(nb64, 0);
  std::vector<unsigned char> seen;
  std::vector<int> solved, lmt;
  int ld_valid = -1;                                    // the slot of Ld that holds the step data of the next panel
  int next_j0 = 0;                                      // the panel the next DIAG or STEP launch must be about
  size_t at = 0;
  for (; at < launches.size() && launches[at].kind <= CHOL_SYRK; ++at) {
    const CholLaunch& l = launches[at];
    if (l.kind == CHOL_DIAG) {
      // the head of a strip: the producer of its first step's data and of its first block's inverse
      CHECK(l.j0 == next_j0 && l.j0 % 64 == 0 && l.grid == 1, "diag block", l.j0, next_j0);
      CHECK(l.ld_write == 0 || l.ld_write == 1, "diag slot", l.ld_write, 0);
      CHECK(l.inv64_block == l.j0 / 64 && l.inv64_block < nb64, "diag inv64 block", l.inv64_block, nb64);
      ++inv_written[l.inv64_block];
      ld_valid = l.ld_write;
      continue;
    }
    if (l.kind == CHOL_SYRK) {
      // rank-K update of everything behind the strip [j0, col_end): 128x128 tiles, rows from je to nrows, columns from je to n
      const int jb = l.j0, je = l.col_end;
      CHECK(je == next_j0 && je < n && je % 64 == 0 && l.K == je - jb, "syrk strip", je, next_j0);
      CHECK(l.R == nrows - je && l.Cn == n - je, "syrk shape", l.R, l.Cn);
      CHECK(l.c_off == (int64_t)je * n + je && l.x_off == (int64_t)je * n + jb, "syrk offsets", l.c_off, l.x_off);
      const int T2 = (l.R + 127) / 128;
      CHECK(l.grid == (unsigned)(T2 * (T2 + 1) / 2), "syrk grid", l.grid, T2);
      seen.assign((size_t)T2 * T2, 0);
      for (unsigned b = 0; b < l.grid; ++b) {
        const TileIJ t = tri_tile((int)b);
        const int ti = t.ti, tj = t.tj;
        CHECK(0 <= tj && tj <= ti && ti < T2, "syrk decode range", ti, tj);
        CHECK(!seen[(size_t)ti * T2 + tj]++, "syrk tile twice", ti, tj);
        ++tiles_visited;
        if (!full) continue;
        for (int di = 0; di < 2; ++di)
          for (int dj = 0; dj < 2; ++dj) {
            const int gi = je / 64 + 2 * ti + di, gj = je / 64 + 2 * tj + dj;      // the kernel's guards: gr < R, gc < Cn, gc <= gr
            if (gi * 64 >= nrows || gj * 64 >= n || gj > gi) continue;
            for (int k = jb / 64; k < je / 64; ++k) ++upd[((size_t)k * G + gi) * G + gj];
          }
      }
      continue;
    }
    // ---- a step
    const CholStep s = chol_step(n, nrows, l.j0, l.col_end);
    const int T = s.T;
    CHECK(l.j0 == next_j0 && l.j0 % 64 == 0 && l.j0 < n, "step panel", l.j0, next_j0);
    CHECK(s.rem_r > 0 && T == (nrows - s.j1 + 63) / 64, "step rows", s.rem_r, T);
    ++panel_steps[l.j0 / 64];
    next_j0 = s.j1;
    // step data: read where the previous producer (k_chol_diag, or the look-ahead of the step before) wrote
    CHECK(l.ld_read == ld_valid && ld_valid >= 0, "step data slot", l.ld_read, ld_valid);
    CHECK(l.ld_write == 1 - l.ld_read, "step data: written where the other tiles still read", l.ld_write, l.ld_read);
    const bool ahead = chol_step_looks_ahead(s);
    CHECK(ahead == (s.rem_c > 0), "look-ahead", ahead, s.rem_c);
    ld_valid = ahead ? l.ld_write : -1;
    // the block inverse handed along: dereferenced by the look-ahead only, then the block at j1; otherwise at most one past the end
    CHECK(l.inv64_block == s.j1 / 64 && l.inv64_block <= 2 * nb128, "step inv64 block", l.inv64_block, 2 * nb128);
    if (ahead) {
      CHECK(s.j1 % 64 == 0 && s.j1 < n && l.inv64_block < nb64, "look-ahead block", s.j1, l.inv64_block);
      ++inv_written[l.inv64_block];
    }
    // the grid and the set of tiles
    const bool panel_only = s.rem_c <= 0, whole = l.col_end >= n;
    CHECK(s.tcols == ((s.rem_c > 0 ? s.rem_c : 0) + 63) / 64 && s.whole == whole, "step geometry", s.tcols, s.whole);
    const long expect_grid = panel_only ? T : whole ? (long)T * (T + 1) / 2 : (long)s.tcols * T - (long)s.tcols * (s.tcols - 1) / 2;
    CHECK((long)l.grid == expect_grid, "step grid", l.grid, expect_grid);
    CHECK(panel_only || whole || (l.col_end % 64 == 0 && s.tcols <= 4 && s.tcols <= T), "strip columns", l.col_end, s.tcols);
    seen.assign((size_t)T * T, 0);
    solved.assign(T, 0);
    lmt.assign(T, 0);
    bool tile10 = false;
    for (unsigned b = 0; b < l.grid; ++b) {
      const TileIJ t = chol_step_tile((int)b, s);
      const int ti = t.ti, tj = t.tj;
      CHECK(0 <= tj && tj <= ti && ti < T, "decode range", ti, tj);
      CHECK(!seen[(size_t)ti * T + tj]++, "tile twice", ti, tj);
      // with the grid's size and no tile twice, membership makes the set the expected one
      CHECK(panel_only ? tj == 0 : (whole || tj < s.tcols), "tile outside the expected set", ti, tj);
      ++tiles_visited;
      const bool idle = !panel_only && tj * 64 >= s.rem_c;      // columns begin behind the last one: solves its rows, writes nothing
      if (idle) ++idle_tiles;
      if (!full) continue;
      if (tj == 0) ++solved[ti];
      if (chol_tile_writes_own_lmt(s, ti, tj)) ++lmt[ti];
      if (panel_only) continue;                                 // the kernel returns here
      if (ti != tj && chol_tile_writes_lmt_of_tile00(ti, tj)) { ++lmt[0]; tile10 = true; }
      if (idle) continue;
      ++upd[((size_t)(l.j0 / 64) * G + s.j1 / 64 + ti) * G + s.j1 / 64 + tj];
    }
    if (!full) continue;
    CHECK(tile10 == chol_has_tile10(s) && tile10 == (!panel_only && T > 1), "tile (1,0)", tile10, T);
    for (int t = 0; t < T; ++t) {
      CHECK(solved[t] == 1, "panel rows solved", t, solved[t]);
      CHECK(lmt[t] == 1, "LmT tile rows written", t, lmt[t]);
    }
    CHECK(chol_tile_writes_own_lmt(s, 0, 0) == !tile10, "LmT rows of tile (0,0)", tile10, 0);
  }
  // every panel with rows below it had its step
  for (int k = 0; k < nb64; ++k) {
    const int j1 = (k + 1) * 64 < n ? (k + 1) * 64 : n;
    CHECK(panel_steps[k] == (nrows - j1 > 0 ? 1 : 0), "steps of a panel", k, panel_steps[k]);
  }
  // the block inverses: all written once by the factorisation, the partner of an odd last one by k_set_identity64
  CHECK(at < launches.size() && launches[at].kind == CHOL_INV64_FIX && launches[at].grid == (unsigned)nb64, "inv64 fix", at, nb64);
  ++at;
  if (nb64 & 1) {
    CHECK(at < launches.size() && launches[at].kind == CHOL_IDENTITY && launches[at].grid == 1, "identity partner", at, nb64);
    CHECK(launches[at].inv64_block == nb64 && nb64 < 2 * nb128, "identity partner block", launches[at].inv64_block, nb64);
    ++inv_written[nb64];
    ++at;
  }
  CHECK(at + 1 == launches.size() && launches[at].kind == CHOL_MERGE && launches[at].grid == (unsigned)nb128, "merge", at, nb128);
  for (int b = 0; b < 2 * nb128; ++b) CHECK(inv_written[b] == 1, "inv64 block written", b, inv_written[b]);       // k_inv_merge reads 2 b, 2 b + 1
  CHECK(inv_written[2 * nb128] == 0, "inv64 block past the end", 2 * nb128, 0);
  if (!full) return 0;
  for (int gi = 0; gi < G; ++gi)
    for (int gj = 0; gj <= gi && gj * 64 < n; ++gj)
      for (int k = 0; k < nb64; ++k)
        CHECK(upd[((size_t)k * G + gi) * G + gj] == (k < gj ? 1 : 0), "updates of a tile", gi * 1000 + gj, k);
  return 0;
}

static int check_tri_tile() {
  const int n = 0, nrows = 0, T = 1024;
  int b = 0;
  for (int ti = 0; ti < T; ++ti)
    for (int tj = 0; tj <= ti; ++tj, ++b) {           // the inverse of b = ti (ti + 1) / 2 + tj, tile by tile
      const TileIJ t = tri_tile(b);
      CHECK(t.ti == ti && t.tj == tj, "tri_tile", b, t.ti);
    }
  CHECK((unsigned)b == tri_count(T), "tri_count", b, tri_count(T));
  return 0;
}

static int check_layout(int n) {
  const int nrows = n;
  const DenseWsLayout l = dense_ws_layout(n);
  const int64_t nb = (n + 127) / 128;
  // the formulas dense_ws_doubles and dense_ws_lm_offset have always had, written out
  const int64_t doubles = 2 * 64 * 64 + 2 * nb * 128 * 128 + nb * 2 * 64 * 64 + 32 + ((int64_t)(n + 1) * n + 31) / 32 * 32 + (int64_t)n * n;
  const int64_t lm_offset = 2 * 64 * 64 + 2 * nb * 128 * 128 + nb * 2 * 64 * 64 + 32;
  CHECK(l.total == doubles, "workspace doubles", l.total, doubles);
  CHECK(l.Lm == lm_offset, "offset of Lm", l.Lm, lm_offset);
  CHECK(l.Ld == 0 && l.Dinv - l.Ld == 2 * 64 * 64, "Ld", l.Ld, l.Dinv);
  CHECK(l.DinvT - l.Dinv == nb * 128 * 128 && l.inv64 - l.DinvT == nb * 128 * 128, "Dinv, DinvT", l.DinvT, l.inv64);
  CHECK(l.flag - l.inv64 == 2 * nb * 64 * 64, "inv64", l.inv64, l.flag);
  CHECK(l.Lm - l.flag == 32, "flag", l.flag, l.Lm);
  CHECK(l.LmT - l.Lm >= (int64_t)(n + 1) * n && (l.LmT - l.Lm) % 32 == 0 && l.LmT - l.Lm < (int64_t)(n + 1) * n + 32, "Lm", l.Lm, l.LmT);
  CHECK(l.total - l.LmT == (int64_t)n * n, "LmT", l.LmT, l.total);
  return 0;
}

static int check_trsv(int n) {
  const int nrows = n, nblk = (n + 127) / 128;
  for (int blk = 0; blk < nblk; ++blk) {
    const long after = n - 128L * (blk + 1), before = 128L * blk;
    const long gf = trsv_step_grid_forward(n, blk), gb = trsv_step_grid_backward(blk);
    CHECK(gf >= 1 && 32 * gf >= after && (after <= 0 ? gf == 1 : 32 * (gf - 1) < after), "k_trsv_step forward grid", blk, gf);
    CHECK(gb >= 1 && 256 * gb >= before && (before <= 0 ? gb == 1 : 256 * (gb - 1) < before), "k_trsv_step backward grid", blk, gb);
  }
  return 0;
}

static int check_trsv_flow() {
  const int n = 0, nrows = 0;
  for (int nblk = 1; nblk <= 128; ++nblk) {
    const int grid = (int)trsv_flow_grid(nblk);
    CHECK(grid == 8 * nblk, "k_trsv_flow grid", nblk, grid);
    std::vector<int> at(nblk, -1);
    for (int b = 0; b < grid; ++b) {
      int p = -1;
      const bool works = trsv_flow_worker(b, p);
      CHECK(works == (b == 8 * (b >> 3) + (((b >> 3) >> 5) & 7)), "k_trsv_flow worker", b, works);
      if (!works) continue;
      CHECK(p >= 0 && p < nblk && at[p] < 0, "k_trsv_flow position", b, p);
      at[p] = b;
    }
    for (int p = 0; p < nblk; ++p) {
      CHECK(at[p] == 8 * p + ((p >> 5) & 7), "k_trsv_flow placement", p, at[p]);
      CHECK(trsv_flow_block(p, nblk, false) == p && trsv_flow_block(p, nblk, true) == nblk - 1 - p, "k_trsv_flow block", p, nblk);
    }
  }
  // the switches, through the environment
  unsetenv("SFM_TRSV_FLOW");
  unsetenv("SFM_CHOL_STRIP_MIN_N");
  DenseSwitches sw = dense_switches_from_env();
  CHECK(sw.strip_min_n == 4096 && sw.strip_min_n == CHOL_STRIP_MIN_N && sw.trsv_flow, "default switches", sw.strip_min_n, sw.trsv_flow);
  CHECK(trsv_takes_flow(1, sw) && trsv_takes_flow(128, sw) && !trsv_takes_flow(129, sw), "flow up to 128 blocks", TRSV_FLOW_MAX_BLOCKS, 0);
  setenv("SFM_TRSV_FLOW", "0", 1);
  setenv("SFM_CHOL_STRIP_MIN_N", "256", 1);
  sw = dense_switches_from_env();
  CHECK(sw.strip_min_n == 256 && !sw.trsv_flow, "switches set", sw.strip_min_n, sw.trsv_flow);
  CHECK(!trsv_takes_flow(1, sw) && !trsv_takes_flow(128, sw), "SFM_TRSV_FLOW=0", 0, 0);
  setenv("SFM_TRSV_FLOW", "1", 1);
  CHECK(trsv_takes_flow(128, dense_switches_from_env()), "SFM_TRSV_FLOW=1", 0, 0);
  unsetenv("SFM_TRSV_FLOW");
  unsetenv("SFM_CHOL_STRIP_MIN_N");
  return 0;
}

int main() {
  static const int LARGE[] = {2047, 2048, 2049, 4095, 4096, 4097, 10000, 16384, 16640};
  static const int STRIP_MIN_N[] = {4096, 256, 1};
  for (int n = 1; n <= 1400; ++n) {
    for (int nrows = n; nrows <= n + 1; ++nrows) {
      const long idle_before = idle_tiles;
      for (int strip_min_n : STRIP_MIN_N)
        if (check_factorisation(n, nrows, strip_min_n, true)) return 1;
      if (nrows == n && idle_tiles != idle_before) return fail("idle tiles without a bordered row", n, nrows, idle_tiles - idle_before, 0);
    }
    if (check_layout(n) || check_trsv(n)) return 1;
  }
  // the workgroups of a bordered system with n a multiple of 64 whose columns begin at n (last strip: the grid is the full
  // triangle over the tile rows, the bordered row's tile row included).  Harmless; the number pins the grids as they are.
  const long idle_small = idle_tiles;
  if (idle_small != 270) return fail("idle tiles over the sweep", 1400, 0, idle_small, 270);
  for (int n : LARGE) {
    for (int nrows = n; nrows <= n + 1; ++nrows)
      for (int strip_min_n : STRIP_MIN_N)
        if (check_factorisation(n, nrows, strip_min_n, false)) return 1;
    if (check_layout(n) || check_trsv(n)) return 1;
  }
  if (check_tri_tile() || check_trsv_flow()) return 1;
  std::printf("ok %ld tiles, %ld idle in n <= 1400 (%ld with the large sizes)\n", tiles_visited, idle_small, idle_tiles);
  return 0;
}
