// Host-only check of sfm_amd/csrc/ba_plan.h, built with -fsanitize=address,undefined by tests/test_host_logic.py.
// The route table of the camera solve, cell by cell on each side of every size threshold and with the switches set through the
// environment (so the real parsing runs); what the build may fuse; the invariant the build and the solve rely on (S~ is left or
// produced as a lower triangle iff the tile-streaming CG consumes it); the assembler shapes; the predictor of hopeless systems
// against verdicts computed by hand from its defining expressions.  Prints "ok <plans checked>" or a diagnostic and exits 1.
#define SFM_BA_PLAN_STANDALONE 1
#include "ba_plan.h"
#include <cstdio>
#include <cstring>
#include <initializer_list>

static int fail(const char* what, const char* row, long a, long b) { std::printf("FAIL %s [%s] %ld %ld\n", what, row, a, b); return 1; }

static const char* const SWITCH_NAMES[] = {"SFM_CGS_PERSIST", "SFM_CGS_BIG", "SFM_CGS_BIG_FROM", "SFM_CGS_BIG_BUDGET", "SFM_CGS_PREDICT",
                                           "SFM_SCHUR_FUSE_SCALE"};
// "NAME=value NAME=value" -> the environment holds exactly these of the six switches
static BaSwitches switches(const char* settings) {
  for (const char* name : SWITCH_NAMES) unsetenv(name);
  char buf[320];
  std::strncpy(buf, settings, sizeof(buf) - 1); buf[sizeof(buf) - 1] = 0;
  for (char* tok = std::strtok(buf, " "); tok; tok = std::strtok(nullptr, " ")) {
    char* eq = std::strchr(tok, '=');
    *eq = 0;
    setenv(tok, eq + 1, 1);
  }
  return ba_switches_from_env();
}

// a cell of the table: "P>I" persistent launch, k_cgs_iter if abandoned; "P>T" persistent, tile-streaming if abandoned; "I" k_cgs_iter;
// "T*" tile-streaming (the build may fuse the scaling, the solve uses the lower triangle); "F" factorisation
static bool cell_matches(const char* cell, const CamPlan& pl) {
  if (!std::strcmp(cell, "F")) return pl.route == CAM_FACTOR && !pl.lower_only;
  if (!std::strcmp(cell, "I")) return pl.route == CAM_CG_ITER && pl.per_launch == CAM_CG_ITER && !pl.lower_only;
  if (!std::strcmp(cell, "T*")) return pl.route == CAM_CG_TILES && pl.per_launch == CAM_CG_TILES && pl.lower_only;
  if (!std::strcmp(cell, "P>I")) return pl.route == CAM_CG_PERSIST && pl.per_launch == CAM_CG_ITER && !pl.lower_only;
  if (!std::strcmp(cell, "P>T")) return pl.route == CAM_CG_PERSIST && pl.per_launch == CAM_CG_TILES && !pl.lower_only;
  return false;
}

struct Row {
  const char* settings;
  bool persist_off;                  // the handle has given the persistent kernel up
  const char* cell[7];               // n = 250, 256 | 258, 1000 | 2046, 2048 | 2050 | 3000 | 4096 | 4098, 10000
  int budget[7];                     // with big = the tile-streaming budget (400, or SFM_CGS_BIG_BUDGET)
};
constexpr int BIG = -1;
static const Row ROWS[] = {
    {"", false, {"P>I", "P>I", "P>I", "T*", "T*", "T*", "T*"}, {160, 160, 160, BIG, BIG, BIG, BIG}},
    {"SFM_CGS_PERSIST=0", false, {"I", "I", "I", "T*", "T*", "T*", "T*"}, {160, 160, 160, BIG, BIG, BIG, BIG}},
    {"", true, {"I", "I", "I", "T*", "T*", "T*", "T*"}, {160, 160, 160, BIG, BIG, BIG, BIG}},
    {"SFM_CGS_BIG=0", false, {"P>I", "P>I", "P>I", "I", "I", "I", "F"}, {160, 160, 160, 160, 160, 160, 160}},
    {"SFM_CGS_PERSIST=0 SFM_CGS_BIG=0", false, {"I", "I", "I", "I", "I", "I", "F"}, {160, 160, 160, 160, 160, 160, 160}},
    {"SFM_CGS_BIG_FROM=257", false, {"P>I", "P>T", "P>T", "T*", "T*", "T*", "T*"}, {160, BIG, BIG, BIG, BIG, BIG, BIG}},
    {"SFM_CGS_BIG_FROM=256", false, {"P>I", "P>T", "P>T", "T*", "T*", "T*", "T*"}, {160, BIG, BIG, BIG, BIG, BIG, BIG}},
    {"SFM_CGS_BIG_FROM=0", false, {"P>I", "P>T", "P>T", "T*", "T*", "T*", "T*"}, {160, BIG, BIG, BIG, BIG, BIG, BIG}},
    {"SFM_CGS_PERSIST=0 SFM_CGS_BIG_FROM=257", false, {"I", "T*", "T*", "T*", "T*", "T*", "T*"}, {160, BIG, BIG, BIG, BIG, BIG, BIG}},
    {"SFM_CGS_PERSIST=0 SFM_CGS_BIG_FROM=100", false, {"I", "T*", "T*", "T*", "T*", "T*", "T*"}, {160, BIG, BIG, BIG, BIG, BIG, BIG}},
    {"SFM_CGS_PERSIST=0 SFM_CGS_BIG_FROM=256", false, {"I", "T*", "T*", "T*", "T*", "T*", "T*"}, {160, BIG, BIG, BIG, BIG, BIG, BIG}},
    {"SFM_CGS_BIG_FROM=257", true, {"I", "T*", "T*", "T*", "T*", "T*", "T*"}, {160, BIG, BIG, BIG, BIG, BIG, BIG}},
    {"SFM_CGS_BIG_FROM=3000", false, {"P>I", "P>I", "P>I", "I", "T*", "T*", "T*"}, {160, 160, 160, 160, BIG, BIG, BIG}},
};
static const int COLUMN_N[7][2] = {{250, 256}, {258, 1000}, {2046, 2048}, {2050, 2050}, {3000, 3000}, {4096, 4096}, {4098, 10000}};
static int column_of(int n) { return n <= 256 ? 0 : n <= 2048 ? (n <= 1000 ? 1 : 2) : n <= 2050 ? 3 : n <= 3000 ? 4 : n <= 4096 ? 5 : 6; }

static long plans = 0;

// one row under one setting of SFM_CGS_BIG_BUDGET ("" = unset): the cells, the fusion, the odd sizes, Cholesky
static int check_row(const Row& row, const char* budget_setting, int big_budget) {
  char settings[256];
  std::snprintf(settings, sizeof(settings), "%s %s", row.settings, budget_setting);
  for (int col = 0; col < 7; ++col)
    for (int k = 0; k < 2; ++k) {
      const int n = COLUMN_N[col][k];
      const int budget = row.budget[col] == BIG ? big_budget : row.budget[col];
      for (int solver : {SFM_CAMERA_SOLVER_AUTO, SFM_CAMERA_SOLVER_CG}) {
        const CamPlan pl = cam_plan(n, solver, row.persist_off, switches(settings));
        ++plans;
        if (!cell_matches(row.cell[col], pl)) return fail("route", settings, n, pl.route);
        if (pl.budget != budget) return fail("budget", settings, n, pl.budget);
      }
      const CamPlan chol = cam_plan(n, SFM_CAMERA_SOLVER_CHOLESKY, row.persist_off, switches(settings));
      if (!cell_matches("F", chol) || chol.budget != budget) return fail("cholesky", settings, n, chol.route);
      // what the build may fuse: the scaling on "*" cells only, there only if unsharded, not Cholesky and not switched off
      const bool star = std::strchr(row.cell[col], '*') != nullptr;
      for (const char* fs : {"", "SFM_SCHUR_FUSE_SCALE=0", "SFM_SCHUR_FUSE_SCALE=1"})
        for (int sharded = 0; sharded < 2; ++sharded)
          for (int solver : {SFM_CAMERA_SOLVER_AUTO, SFM_CAMERA_SOLVER_CHOLESKY, SFM_CAMERA_SOLVER_CG}) {
            char with_fs[320];
            std::snprintf(with_fs, sizeof(with_fs), "%s %s", settings, fs);
            const BaSwitches sw = switches(with_fs);
            const BuildFusion f = build_fusion(cam_plan(n, solver, row.persist_off, sw), sharded != 0, solver, n, sw);
            const bool may = !sharded && solver != SFM_CAMERA_SOLVER_CHOLESKY;
            if (f.einv != may) return fail("fuse_einv", with_fs, n, solver);
            if (f.scale != (star && may && std::strcmp(fs, "SFM_SCHUR_FUSE_SCALE=0") != 0)) return fail("fuse_scale", with_fs, n, solver);
            if (f.scale && !f.einv) return fail("fuse_scale without fuse_einv", with_fs, n, solver);
          }
    }
  // odd n: the factorisation, nothing fused - with the budget of its size all the same
  for (int n : {251, 1001, 2047, 2049, 3001, 4097, 9999}) {
    const BaSwitches sw = switches(settings);
    const CamPlan pl = cam_plan(n, SFM_CAMERA_SOLVER_AUTO, row.persist_off, sw);
    const int col = column_of(n + 1);
    if (!cell_matches("F", pl)) return fail("odd n", settings, n, pl.route);
    if (pl.budget != (row.budget[col] == BIG ? big_budget : row.budget[col])) return fail("odd n budget", settings, n, pl.budget);
    const BuildFusion f = build_fusion(pl, false, SFM_CAMERA_SOLVER_AUTO, n, sw);
    if (f.einv || f.scale) return fail("odd n fusion", settings, n, f.einv);
  }
  // every size: S~ is a lower triangle iff the tile-streaming CG is what consumes it - never under a persistent launch, whose
  // kernel reads the full matrix (the tile-streaming CG it may be abandoned for then reads a subset of that)
  for (int n = 2; n <= 4100; ++n) {
    const BaSwitches sw = switches(settings);
    for (int solver : {SFM_CAMERA_SOLVER_AUTO, SFM_CAMERA_SOLVER_CHOLESKY, SFM_CAMERA_SOLVER_CG}) {
      const CamPlan pl = cam_plan(n, solver, row.persist_off, sw);
      ++plans;
      if (pl.lower_only != (pl.route == CAM_CG_TILES)) return fail("lower_only", settings, n, pl.route);
      if (pl.per_launch != CAM_CG_ITER && pl.per_launch != CAM_CG_TILES) return fail("per_launch", settings, n, pl.per_launch);
      if ((pl.route == CAM_CG_ITER || pl.route == CAM_CG_TILES) && pl.route != pl.per_launch) return fail("route vs per_launch", settings, n, pl.route);
      if (pl.route != CAM_FACTOR && ((n & 1) || solver == SFM_CAMERA_SOLVER_CHOLESKY)) return fail("CG on an odd or Cholesky system", settings, n, pl.route);
      if (pl.route == CAM_CG_PERSIST && (n > PR_MAX_N || row.persist_off)) return fail("persistent launch", settings, n, pl.route);
      if (pl.route == CAM_CG_ITER && n > CGS_MAX_N) return fail("k_cgs_iter beyond its size", settings, n, pl.route);
      const BuildFusion f = build_fusion(pl, false, solver, n, sw);
      if (f.scale && !(pl.lower_only && f.einv)) return fail("S~ left for a route that does not take it", settings, n, pl.route);
    }
  }
  return 0;
}

static int check_predictor() {
  const CgPredictor none = {0.0, {0.0, 0.0}, {0, 0}};
  for (double arel : {1e-12, 1e-6, 1.0})
    if (none.hopeless(arel, 160) || none.hopeless(arel, 3)) return fail("hopeless without history", "", 0, 0);
  CgPredictor q = none;
  q.fail_rel = 1e-6;                                             // at or below 4 x the failure bound
  if (!q.hopeless(3e-6, 160) || q.hopeless(5e-6, 160)) return fail("failure bound", "", 0, 0);
  q = none; q.ok_rel[0] = 1e-3; q.ok_its[0] = 100;               // one record: slope 0.2
  if (!q.hopeless(1e-5, 160)) return fail("one record, 218.8 > 200", "", 0, 0);
  if (q.hopeless(1e-4, 160)) return fail("one record, 147.9", "", 0, 0);
  if (q.hopeless(2e-3, 160)) return fail("above the record", "", 0, 0);
  q = {0.0, {1e-4, 1e-2}, {120, 60}};                            // two records: slope log 2 / log 100
  if (!q.hopeless(1e-6, 160)) return fail("two records, 216.3 > 200", "", 0, 0);
  if (q.hopeless(1e-6, 400)) return fail("two records, budget 400", "", 0, 0);
  q = {0.0, {1e-4, 1e-2}, {10, 100}};                            // a negative raw slope clamps to 0
  if (q.hopeless(1e-8, 160)) return fail("slope clamped to 0", "", 0, 0);
  q = {0.0, {1e-4, 1e-3}, {150, 10}};                            // a raw slope above 0.5 clamps to 0.5
  if (!q.hopeless(1e-10, 160)) return fail("slope clamped to 0.5", "", 0, 0);

  q = none;
  q.note_ok(1e-3, 0);                                            // its <= 0: nothing
  if (q.ok_its[0] != 0 || q.ok_rel[0] != 0.0) return fail("note_ok with no iterations", "", 0, 0);
  const double base = 0x1p-10;                                   // (a power of two: the ratios below are exact)
  q.note_ok(base, 40);
  if (q.ok_its[0] != 40 || q.ok_rel[0] != base || q.ok_its[1] != 0) return fail("first record", "", q.ok_its[0], q.ok_its[1]);
  q.note_ok(1.4 * base, 35);                                     // within 1.5 x: replaces [0] only
  if (q.ok_its[0] != 35 || q.ok_rel[0] != 1.4 * base || q.ok_its[1] != 0) return fail("1.4 x replaces", "", q.ok_its[0], q.ok_its[1]);
  q = none; q.note_ok(base, 40);
  q.note_ok(1.5 * base, 30);                                     // at 1.5 x: [0] shifts to [1]
  if (q.ok_its[0] != 30 || q.ok_rel[0] != 1.5 * base || q.ok_its[1] != 40 || q.ok_rel[1] != base) return fail("1.5 x shifts", "", q.ok_its[0], q.ok_its[1]);
  q = none; q.note_ok(base, 40);
  q.note_ok(base / 1.5, 50);                                     // and at 1 / 1.5
  if (q.ok_its[0] != 50 || q.ok_its[1] != 40 || q.ok_rel[1] != base) return fail("1 / 1.5 shifts", "", q.ok_its[0], q.ok_its[1]);
  const CgPredictor before = q;
  q.note_ok(5e-4, 0);
  if (std::memcmp(&before, &q, sizeof(q)) != 0) return fail("note_ok with no iterations changes nothing", "", 0, 0);
  q.fail_rel = 1e-5;
  q.note_ok(2e-5, 90);                                           // above the failure bound: it stays
  if (q.fail_rel != 1e-5) return fail("fail_rel kept", "", 0, 0);
  q.note_ok(1e-5, 120);                                          // converged at the bound after all: halved
  if (q.fail_rel != 0.5 * 1e-5) return fail("fail_rel halved", "", 0, 0);

  q = none; q.fail_rel = 1e-6;
  q.note_out_of_budget(1e-5, 159, 160);
  if (q.fail_rel != 1e-6) return fail("budget - 1 iterations", "", 0, 0);
  q.note_out_of_budget(1e-7, 160, 160);
  if (q.fail_rel != 1e-6) return fail("out of budget below the bound", "", 0, 0);
  q.note_out_of_budget(1e-5, 160, 160);
  if (q.fail_rel != 1e-5) return fail("out of budget above the bound", "", 0, 0);
  q.note_out_of_budget(1e-4, 3, 3);                              // (SFM_CGS_BIG_BUDGET=3)
  if (q.fail_rel != 1e-4) return fail("out of a budget of 3", "", 0, 0);
  return 0;
}

int main() {
  for (const Row& row : ROWS) {
    if (check_row(row, "", 400)) return 1;
    if (check_row(row, "SFM_CGS_BIG_BUDGET=3", 3)) return 1;           // the tile-streaming budget alone: 160 stays
    if (check_row(row, "SFM_CGS_BIG_BUDGET=0", 400)) return 1;
    if (check_row(row, "SFM_CGS_BIG_BUDGET=-5", 400)) return 1;
  }
  // SFM_CGS_PREDICT is parsed like the other on / off switches
  if (!switches("").predict || switches("SFM_CGS_PREDICT=0").predict || !switches("SFM_CGS_PREDICT=1").predict) return fail("predict switch", "", 0, 0);

  struct Shape { int C, nb; bool rounds; int scaled_nb; };
  for (const Shape& e : {Shape{1, 2, false, 2}, Shape{127, 2, false, 2}, Shape{128, 8, false, 4}, Shape{511, 8, false, 4}, Shape{512, 8, true, 4},
                         Shape{5000, 8, true, 4}}) {
    const AsmShape s = schur_assemble_shape(e.C);
    if (s.nb != e.nb || s.rounds != e.rounds) return fail("assembler shape", "", e.C, s.nb);
    if (schur_assemble_scaled_nb(e.C) != e.scaled_nb) return fail("scaled assembler shape", "", e.C, schur_assemble_scaled_nb(e.C));
  }
  if (check_predictor()) return 1;
  std::printf("ok %ld\n", plans);
  return 0;
}
