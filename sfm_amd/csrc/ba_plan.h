// Host-side planning of the bundle adjustment's camera solve: which route forms and solves the reduced camera system of a
// damped solve, which assembler shape a camera count takes, and the prediction of systems the CG cannot finish.  Plain C++
// (no HIP): included by ba_internal.h, executed by sfm_ba_schur_build (ba.hip) / sfm_ba_schur_solve / sfm_ba_finish_solve (ba_camera_cg.hip), and
// compiled on its own with the address and undefined-behaviour sanitizers by tests/test_host_logic.py
// (tests/native/ba_plan_check.cpp, which defines SFM_BA_PLAN_STANDALONE).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>

#ifdef SFM_BA_PLAN_STANDALONE
enum { SFM_CAMERA_SOLVER_AUTO = 0, SFM_CAMERA_SOLVER_CHOLESKY = 1, SFM_CAMERA_SOLVER_CG = 2 };      // as in include/sfm_amd.h
#endif

// ---- sizes of the routes (the kernels size their arrays by them)
constexpr int PR_MAX_N = 2048;          // k_cgs_persist: 8 rows x 2048 columns per workgroup in registers; grid = n / 8 <= 256
constexpr int CGS_MAX_N = 4096;         // k_cgs_iter: the direction vector lives in LDS (32 KB); larger systems use the factorisation
constexpr int CGS_MAX_ITER = 160;       // iterations of k_cgs_persist / k_cgs_iter before a system falls back to the factorisation
constexpr int CGS_BIG_MAX_ITER = 400;   // the same for the tile-streaming route (cgs_solve_big)
constexpr int ASM_ROUNDS_FROM = 512;    // cameras from which k_schur_assemble walks its item tiles round by round (strip_item_sums)
constexpr int ASM_WIDE_FROM = 128;      // cameras from which the assemblers take more blocks per workgroup (schur_assemble_shape)

// ---- the switches of the camera solve.  Read per call of the three entry points, never cached: tests switch them within
// one process.
struct BaSwitches {
  bool persist;        // SFM_CGS_PERSIST=0: one launch per CG iteration instead of the persistent kernel
  bool big;            // SFM_CGS_BIG=0: no tile-streaming route; systems beyond CGS_MAX_N then take the factorisation
  int big_from;        // SFM_CGS_BIG_FROM: unknowns from which the launch-per-iteration CG is the tile-streaming one (at least 257)
  int big_budget;      // SFM_CGS_BIG_BUDGET: a TEST knob - a budget of a few iterations makes a system fall back to the factorisation
  bool predict;        // SFM_CGS_PREDICT=0: no prediction of hopeless systems (CgPredictor)
  bool fuse_scale;     // SFM_SCHUR_FUSE_SCALE=0: S first, then k_scale_system_lower, on the tile-streaming route
};
static inline bool ba_switch_on(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }
static inline BaSwitches ba_switches_from_env() {
  BaSwitches s;
  s.persist = ba_switch_on("SFM_CGS_PERSIST");
  s.big = ba_switch_on("SFM_CGS_BIG");
  const char* f = getenv("SFM_CGS_BIG_FROM");
  s.big_from = f ? (atoi(f) > 256 ? atoi(f) : 257) : PR_MAX_N + 1;
  const char* b = getenv("SFM_CGS_BIG_BUDGET");
  const int v = b ? atoi(b) : 0;
  s.big_budget = v > 0 ? v : CGS_BIG_MAX_ITER;
  s.predict = ba_switch_on("SFM_CGS_PREDICT");
  s.fuse_scale = ba_switch_on("SFM_SCHUR_FUSE_SCALE");
  return s;
}

// ---- the route of a camera system of n unknowns
enum CamRoute {
  CAM_FACTOR,          // bordered Cholesky + triangular solves
  CAM_CG_PERSIST,      // k_cgs_persist: one launch per system (n <= PR_MAX_N)
  CAM_CG_ITER,         // cgs_solve: k_cgs_iter, one launch per iteration (n <= CGS_MAX_N)
  CAM_CG_TILES         // cgs_solve_big: the tile-streaming CG over the lower triangle, two launches per iteration
};
struct CamPlan {
  CamRoute route;      // what the solve tries first (before the prediction of hopeless systems, which needs the problem's history)
  CamRoute per_launch; // CAM_CG_ITER or CAM_CG_TILES: the launch-per-iteration CG of this size - the route itself unless that is
                       // CAM_CG_PERSIST, whose systems take it when the persistent launch was abandoned
  bool lower_only;     // S~ is consumed as its lower triangle (+ the diagonal tiles) only: k_scale_system_lower or
                       // k_schur_assemble_scaled may produce it.  True iff route == CAM_CG_TILES: a persistent launch reads the
                       // full matrix, and the tile-streaming CG it may be abandoned for then reads a subset of that
  int budget;          // the iteration budget the predictor and the fall-back record compare against; cgs_solve_big's own budget
};
// The launch-per-iteration CG is the tile-streaming one from SFM_CGS_BIG_FROM unknowns on, k_cgs_iter below.  Default:
// everything beyond the persistent kernel's 2,048 - measured at n = 3,000 / 4,000: camera-solve slots 392 + 356 -> 329 + 290 us
// and 583 + 520 -> 422 + 348 us per damped solve against k_cgs_iter<8, 4> (half the bytes per iteration outweigh two more
// launches).  persist_off: the handle has given the persistent kernel up (a launch was abandoned).
// Two oddities are kept as they have always been:
//   * the budget follows the size alone, so under SFM_CGS_BIG_FROM=257 a persistent solve of n <= 2,048 is judged by the
//     predictor against the tile-streaming budget although k_cgs_persist itself stops at CGS_MAX_ITER;
//   * a CAM_FACTOR plan carries a budget too: with SFM_CAMERA_SOLVER_AUTO the predictor runs, and counts a fall-back when it
//     says "hopeless", even where no CG was possible anyway (odd n, or n > CGS_MAX_N under SFM_CGS_BIG=0).
static inline CamPlan cam_plan(int n, int camera_solver, bool persist_off, const BaSwitches& sw) {
  const bool even = (n & 1) == 0;                        // every CG kernel handles its unknowns in pairs
  const bool big = sw.big && n >= sw.big_from;
  CamPlan pl;
  pl.per_launch = big ? CAM_CG_TILES : CAM_CG_ITER;
  pl.budget = big ? sw.big_budget : CGS_MAX_ITER;
  if (camera_solver == SFM_CAMERA_SOLVER_CHOLESKY || !even || (n > CGS_MAX_N && !big)) pl.route = CAM_FACTOR;
  else if (n <= PR_MAX_N && !persist_off && sw.persist) pl.route = CAM_CG_PERSIST;
  else pl.route = pl.per_launch;
  pl.lower_only = pl.route == CAM_CG_TILES;
  return pl;
}

// What sfm_ba_schur_build leaves for the solve besides (or instead of) S.
struct BuildFusion {
  bool einv;           // the diagonal blocks' factors E_c, E_c^-1 for the camera CG come out of the assembler (unsharded problems
                       // whose camera system may go to the CG: a rank's S is a partial sum until the exchange)
  bool scale;          // ... and the scaled system S~ itself, INSTEAD of S (k_schur_diag + k_schur_assemble_scaled): only where the
                       // solve will take the tile-streaming CG - it alone consumes a lower-triangle S~
};
static inline BuildFusion build_fusion(const CamPlan& plan, bool sharded, int camera_solver, int n, const BaSwitches& sw) {
  BuildFusion f;
  f.einv = !sharded && camera_solver != SFM_CAMERA_SOLVER_CHOLESKY && (n & 1) == 0;
  f.scale = sw.fuse_scale && f.einv && plan.lower_only;
  return f;
}

// ---- assembler shapes
// k_schur_assemble<D, nb, rounds>: 8 blocks per workgroup (640-byte rows) from 128 cameras on; 2 below - a thread sums its
// element of every block of the workgroup in turn, and with few cameras a block holds many items (50 cameras / 200k
// observations: 4 per block) while the grid is small: at cfg3 eight blocks per workgroup cost 11 us more than they saved
struct AsmShape { int nb; bool rounds; };
static inline AsmShape schur_assemble_shape(int C) {
  if (C >= ASM_ROUNDS_FROM) return {8, true};
  if (C >= ASM_WIDE_FROM) return {8, false};
  return {2, false};
}
// k_schur_assemble_scaled<D, nb> (blocks per workgroup at >= 128 cameras, us per launch at 1000: 2: 397, 4: 277-285, 8: 299)
static inline int schur_assemble_scaled_nb(int C) { return C >= ASM_WIDE_FROM ? 4 : 2; }

// ---- Camera CG, SFM_CAMERA_SOLVER_AUTO: what a problem has taught about where the iteration budget runs out.
// A system the CG cannot finish within its budget costs the budget (160 iterations = 0.77 ms at n = 2000) AND the factorisation
// (0.9 ms).  SciPy's More' iteration resets alpha to 0.001 alpha_upper whenever the carried-over value falls outside its bracket
// (common.py:117-118) - on the spatially coherent scene that is one hopeless system every third outer iteration, seven in the
// first.  Whether a system is hopeless is predicted from the problem's own history (alpha relative to max diag H): the largest
// alpha at which CG ran out of iterations (forgotten by 20 % per linearisation), and the last two converged step systems at
// different alpha, whose iteration counts give the local exponent of iterations ~ alpha^-s (measured: s ~ 0.4 on the spatially
// coherent scene, ~ 0.2 on the random one, falling towards alpha -> 0).  A damped solve at or below 4 x the failure bound, or for
// which that power law - with 0.85 s - predicts more than 1.25 x the budget, goes to the factorisation at once.  The prediction
// depends on replicated quantities only (alpha, max diag H, iteration counts), so every rank of a sharded solve decides alike:
// the expressions below keep their operand order.
struct CgPredictor {
  double fail_rel, ok_rel[2];    // [0] the latest converged system, [1] the one before it at an alpha at least 1.5 x away
  int ok_its[2];

  bool hopeless(double arel, int budget) const {
    if (fail_rel > 0.0 && arel <= 4.0 * fail_rel) return true;
    if (ok_its[0] > 0 && arel < ok_rel[0]) {
      double slope = 0.2;                            // one record only: the flatter of the two measured exponents
      if (ok_its[1] > 0) {
        slope = -std::log((double)ok_its[0] / ok_its[1]) / std::log(ok_rel[0] / ok_rel[1]);
        slope = slope < 0.0 ? 0.0 : (slope > 0.5 ? 0.5 : slope);
      }
      if (ok_its[0] * std::pow(ok_rel[0] / arel, 0.85 * slope) > 1.25 * budget) return true;
    }
    return false;
  }
  // a converged step system joins the record
  void note_ok(double arel, int its) {
    if (its <= 0) return;
    if (ok_its[0] > 0) {
      const double r = arel / ok_rel[0];
      if (r >= 1.5 || r <= 1.0 / 1.5) { ok_rel[1] = ok_rel[0]; ok_its[1] = ok_its[0]; }
    }
    ok_rel[0] = arel; ok_its[0] = its;
    if (arel <= fail_rel) fail_rel = 0.5 * arel;     // it does converge here after all
  }
  // a system the CG did not finish: out of iterations (not: broken) raises the failure bound
  void note_out_of_budget(double arel, int its, int budget) {
    if (its >= budget && arel > fail_rel) fail_rel = arel;
  }
};
