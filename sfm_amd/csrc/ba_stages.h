// What the bundle-adjustment units (ba*.hip) share on the host side (included by ba_internal.h): the words of the camera CG's status block
// (Lay::cg_scal) and the functions one unit calls in another - a kernel is launched only by the unit that defines it.  Every launch_* /
// ba_* function enqueues on h->stream and leaves the launch check to the calling stage.
#pragma once
// cg_scal as the CG on the formed system uses it (ba_camera_cg.hip; k_schur_assemble / k_schur_diag in ba.hip raise CGS_FAIL for a bad block)
enum { CGS_RR0 = 0, CGS_RR = 1, CGS_ITER = 2, CGS_FAIL = 3, CGS_DONE = 4,
       CGS_RR_SLOT = 5 };   // [5], [6]: ||r||^2 handed from launch to launch; launch `it` reads slot (it + 1) & 1, writes slot it & 1
enum { CGB_PAIR = 5 };     // scal[5 + 2 (it & 1)], scal[6 + 2 (it & 1)]: alpha and gamma of launch `it`, read by launch it + 1
// ... and as the implicit-Schur PCG uses it (ba_pcg.hip)
enum { CG_RZ = 0, CG_RR = 1, CG_RR0 = 2, CG_ITER = 3, CG_FAIL = 4, CG_DOT = 5 };
#pragma GCC visibility push(hidden)      // (build.py sets no -fvisibility, and the library's exported symbols are to stay what they were)
// ---- ba.hip
int check_problem(sfm_ctx* h, sfm_ba_problem p, Lay* L);                  // argument check of every stage; *L = the problem's layout
bool ba_wait_for_word(sfm_ctx* h, const volatile double* word, double want);   // spins on a pinned word (publish_word) until it reads `want`: true; false: the stream drained first
void ba_copy_neg(sfm_ctx* h, const double* src, double* dst, int n, double sgn);                // k_copy_neg: dst = sgn * src
void ba_add_vec(sfm_ctx* h, const double* a, const double* b, double* dst, int n);              // k_add_vec: dst = a + b
void ba_dot(sfm_ctx* h, int n, const double* a, const double* b, double* out);                  // k_dot: *out = a . b
void ba_sum_partials(sfm_ctx* h, const double* part, int nblk, int cnt, double* dst);           // k_sum_partials: dst[0..cnt) = column sums
void launch_build_G(sfm_ctx* h, sfm_ba_problem p, const Lay& L, double alpha, double* cg_scal);  // k_build_G: G, eobs, Linv, e; clears cg_scal if given
void launch_obs_Gtp(sfm_ctx* h, sfm_ba_problem p, const Lay& L, const double* vc);                // k_obs_Gtp: tmp3[k] = G_k^T vc_cam(k)
void launch_backsub_points(sfm_ctx* h, sfm_ba_problem p, const Lay& L);                           // k_backsub: pp, v, part_pt from tmp3
void launch_cam_reduce_chunks(sfm_ctx* h, sfm_ba_problem p, const Lay& L, const double* vec);     // k_cam_reduce_chunks (if any chunk): cch_part = G vec
// k_cam_reduce_final: out = base (may be null) - the chunk sums per camera; point_sums: one workgroup more sums part_pt into red_q[n..n+2)
void launch_cam_reduce_final(sfm_ctx* h, sfm_ba_problem p, const Lay& L, const double* base, double* out, bool point_sums);
void launch_backsub(sfm_ctx* h, sfm_ba_problem p, const Lay& L, int want_q);    // the point step pp for the p_c in pc; want_q: rhs2 pieces in red_q
int schur_materialise_S(sfm_ctx* h, sfm_ba_problem p, const Lay& L);           // S into red_S from the item tiles if the build left S~ only
// ---- ba_camera_cg.hip
// k_finish_solve_pcg: PNORM2, PQ (from *dotp), CHOL_FAIL (from *failp) into the scalars, with a new ticket
void launch_finish_solve_pcg(sfm_ctx* h, sfm_ba_problem p, const Lay& L, int want_q, const double* dotp, const double* failp);
int cgs_second_system_verdict(sfm_ctx* h, sfm_ba_problem p, const Lay& L);    // the persistent CG sfm_ba_finish_solve left in flight, once the stream is past it: redoes the q term if it must
#pragma GCC visibility pop
