/* sfm_amd.h - C-ABI of libsfm_amd.so (MI355X / gfx950 hot path of Sovik-Ghosh/SFM).
 *
 * The reference has no FFI layer: its hot path is two Python methods,
 *   ImageMatcher.match_features          /root/reference/utils/find_matches.py:141-155
 *   StructureFromMotion.bundle_adjust    /root/reference/utils/sfm_reconstruction.py:401-549
 * (plus compute_reconstruction_stats :582-631, a by-product of the residual kernel).
 * This header is what a ctypes binding for those two methods binds instead of
 * cv2.BFMatcher.knnMatch (find_matches.py:144-147) and scipy.optimize.least_squares
 * (sfm_reconstruction.py:506-514).  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: every data pointer is a DEVICE pointer (HBM resident, caller-allocated,
 * caller-owned) unless its name ends in _host.  All work is enqueued on the handle's
 * HIP stream (sfm_set_stream; default = the null stream); functions return without
 * synchronising unless stated.  Return value 0 = OK, <0 = error (sfm_last_error).
 * One handle per (process, device); a handle is not thread-safe.
 */
#ifndef SFM_AMD_H
#define SFM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfm_ctx* sfm_handle;

enum { SFM_OK = 0, SFM_ERR_ARG = -1, SFM_ERR_HIP = -2, SFM_ERR_WORKSPACE = -3, SFM_ERR_NUMERIC = -4 };

int         sfm_create(int device, sfm_handle* out);
void        sfm_destroy(sfm_handle h);
const char* sfm_last_error(sfm_handle h);
int         sfm_set_stream(sfm_handle h, void* hip_stream);
int         sfm_synchronize(sfm_handle h);
const char* sfm_version(void);
/* Stream-ordered copy of device memory the library owns (e.g. sfm_ba_get_structure) to the host; synchronises. */
int         sfm_copy_to_host(sfm_handle h, void* dst_host, const void* src_device, int64_t bytes);

/* The persistent conjugate-gradient kernel of the camera solve (SFM_CAMERA_SOLVER_CG, n <= 2048) needs its n / 8 workgroups
 * co-resident.  A launch whose workgroups give up waiting for each other (bounded spins; e.g. the CUs are shared with another
 * process) is abandoned, the solve falls back to one launch per iteration and the handle stops using the persistent kernel.
 * sfm_cgs_persist_enable switches it back on (or off); sfm_cgs_persist_enabled reports the state. */
int sfm_cgs_persist_enable(sfm_handle h, int enabled);
int sfm_cgs_persist_enabled(sfm_handle h);

/* Per-kernel device timing with HIP events recorded on the handle's stream (what bench.py's
 * roofline numbers are computed from).  Off by default.  sfm_profile_read synchronises the stream,
 * returns the accumulated milliseconds and launch count of one slot and resets it. */
enum { SFM_PROF_LIN_OBS = 0,   /* k_lin_obs: residual + Jacobian + Huber scaling, one launch per linearisation */
       SFM_PROF_LIN_REST = 1,  /* per-point / per-camera block sums of a linearisation */
       SFM_PROF_BUILD_G = 2,   /* point factors + G = W L^-T */
       SFM_PROF_SCHUR = 3,     /* reduced camera system S, r */
       SFM_PROF_CHOL = 4,      /* camera solve for the step: CG on the scaled system, or the bordered Cholesky of S */
       SFM_PROF_TRSV = 5,      /* second system (q term) by CG, or the triangular solves with the factor */
       SFM_PROF_BACKSUB = 6,   /* point back-substitution and the q pieces */
       SFM_PROF_STEP = 7,      /* trial step: x + s, predicted reduction sums, cost(x + s) */
       SFM_PROF_KNN = 8,       /* matcher distance + top-2 kernel */
       SFM_PROF_SCHUR_ITEMS = 9, /* k_schur_items alone (inside SFM_PROF_SCHUR) */
       SFM_PROF_FUND_HYP = 10, /* k_fund_hypotheses alone (inside sfm_fund_ransac) */
       SFM_PROF_PNP_HYP = 11,  /* k_pnp_hypotheses alone (inside sfm_pnp_ransac) */
       SFM_PROF_POSE_VOTE = 12, /* k_pose_vote alone (inside sfm_pose_recover) */
       SFM_PROF_FEAT_SCORE = 13,    /* k_feat_score alone (inside sfm_features_detect) */
       SFM_PROF_FEAT_SELECT = 14,   /* suppression, cut, ties and the row scan (the rest of sfm_features_detect) */
       SFM_PROF_FEAT_SCATTER = 15,  /* k_feat_scatter (inside sfm_features_describe) */
       SFM_PROF_FEAT_BLUR = 16,     /* k_feat_blur */
       SFM_PROF_FEAT_DESCRIBE = 17, /* k_feat_describe */
       SFM_PROF_ESS_SOLVE = 18,     /* k_ess_solve alone (inside sfm_ess_ransac) */
       SFM_PROF_ESS_SCORE = 19,     /* k_ess_score alone (inside sfm_ess_ransac) */
       SFM_PROF_HOM_HYP = 20,       /* k_hom_hypotheses alone (inside sfm_hom_ransac) */
       SFM_PROF_COUNT = 21 };
int sfm_set_profiling(sfm_handle h, int enabled);
int sfm_profile_read(sfm_handle h, int slot, double* total_ms_host, int64_t* count_host);

/* ------------------------------------------------------------------ matcher
 * Replaces cv2.BFMatcher(norm).knnMatch(desc1, desc2, k=2) + the ratio loop
 * (find_matches.py:144-153).  Distances are float32 as OpenCV's DMatch.distance.
 *
 * Non-finite distances (SFM_METRIC_L2_F32 only: a float32 sum that overflows, a NaN or infinite input value; the uint8
 * and Hamming distances are always finite).  Rows are ranked by (float32 distance, train index).  +inf is a distance
 * like any other and ranks after every finite one, by index.  A NaN distance never enters the top-2.  A slot with no
 * rankable row reports index -1 and distance +inf.  The ratio test then drops a query with no neighbour
 * (inf < r * inf is false) and keeps a query with exactly one (d1 < r * inf): no match ever carries train index -1.
 */
enum {
  SFM_METRIC_L2_U8   = 0,  /* uint8 [n,dim], dim % 32 == 0 (SIFT: 128): exact integer d^2 on i8 MFMA */
  SFM_METRIC_L2_F32  = 1,  /* float32 [n,dim]: sequential float32 sum of (a-b)^2 (general floats)   */
  SFM_METRIC_HAMMING = 2   /* uint8 [n,dim] bit strings, dim 16 / 32 (ORB) / 64 bytes: popcount distance;
                              128 / 256 bits run as exact uint8 L2 over unpacked bits on the i8 MFMA path       */
};

int sfm_match_workspace_bytes(int metric, int64_t nq, int64_t nt, int dim, int64_t* bytes_host);

/* Per query row: two nearest train rows (idx1/d1 nearest), ties -> lower train index.
 * d1/d2: L2 = sqrtf(d^2), Hamming = bit count.  Needs nt >= 2. */
int sfm_match_knn2(sfm_handle h, int metric, const void* q, int64_t nq, const void* t, int64_t nt,
                   int dim, int32_t* idx1, int32_t* idx2, float* d1, float* d2,
                   void* workspace, int64_t workspace_bytes);

/* Lowe ratio test `(double)d1 < ratio * (double)d2` (find_matches.py:152) and compaction in
 * query order.  query_idx/train_idx/dist have room for nq entries; *n_matches is a device int64. */
int sfm_match_ratio(sfm_handle h, int64_t nq, const int32_t* idx1, const float* d1, const float* d2,
                    double ratio, int32_t* query_idx, int32_t* train_idx, float* dist,
                    int64_t* n_matches, void* workspace, int64_t workspace_bytes);

/* Batched form: every image pair of a preprocessing step in ONE call.  The reference calls match_features once per
 * pair in a serial loop (find_matches.py:329-350, call at :272) on sets of a few hundred to a few thousand
 * descriptors, where a launch per pair is all overhead.  Segment s (= one pair) matches the query rows
 * [q_beg[s], q_end[s]) of q against the train rows [t_beg[s], t_end[s]) of t (q and t may be the same array holding
 * the descriptors of all images back to back).  Output row out_ptr[s] + i belongs to query row q_beg[s] + i;
 * out_ptr = exclusive prefix sum of the query counts, n_out = out_ptr[n_seg].  idx1 / idx2 are train indices
 * RELATIVE to t_beg[s] (what DMatch.trainIdx is for that pair).  Results per segment are bit-identical to a
 * sfm_match_knn2 call on that pair.  The four segment arrays are HOST pointers (the caller knows its image sizes);
 * out_ptr_device (optional, [n_seg+1] device int64) receives out_ptr for sfm_match_ratio_batched. */
int sfm_match_batched_workspace_bytes(int metric, int32_t n_seg, const int64_t* q_beg_host, const int64_t* q_end_host,
                                      const int64_t* t_beg_host, const int64_t* t_end_host, int64_t nq_rows,
                                      int64_t nt_rows, int64_t* n_out_host, int64_t* bytes_host);
int sfm_match_knn2_batched(sfm_handle h, int metric, const void* q, int64_t nq_rows, const void* t, int64_t nt_rows,
                           int dim, int32_t n_seg, const int64_t* q_beg_host, const int64_t* q_end_host,
                           const int64_t* t_beg_host, const int64_t* t_end_host, int32_t* idx1, int32_t* idx2,
                           float* d1, float* d2, int64_t* out_ptr_device, void* workspace, int64_t workspace_bytes);
/* Ratio test + compaction over all n_out rows of a batch: the matches of segment s are entries
 * [seg_match_ptr[s], seg_match_ptr[s+1]) (device int64 [n_seg+1]) of query_idx / train_idx / dist, query indices
 * relative to the segment (DMatch.queryIdx), in query order.  workspace: ceil(n_out / 256) * 8 + 64 bytes. */
int sfm_match_ratio_batched(sfm_handle h, int64_t n_out, int32_t n_seg, const int64_t* out_ptr_device, const int32_t* idx1,
                            const float* d1, const float* d2, double ratio, int32_t* query_idx, int32_t* train_idx,
                            float* dist, int64_t* seg_match_ptr_device, void* workspace, int64_t workspace_bytes);

/* float32 descriptors whose every value is an integer in [0,255] (what SIFT emits) -> uint8 copy;
 * *all_integral (device int32) is 0 if any value is not such an integer. */
int sfm_match_f32_to_u8(sfm_handle h, const float* src, int64_t n_elems, uint8_t* dst, int32_t* all_integral);

/* ------------------------------------------------------------------ guided matching
 * Matching again under each pair's fundamental matrix: a query q of image i is compared only with
 * C(q) = { t of image j : both point-line distances of (q, t) under F are <= gate_px } (the rule of
 * sfm_amd/csrc/guided_rule.h, float64 without FMA contraction, image i always in its first slot).  best = the minimum
 * over C(q) of (distance, t), second = the minimum of the rest; distances as in the matcher (popcount, or sqrtf of the
 * integer d^2, float32).  q is kept iff |C(q)| >= 1, (double)d1 <= max_distance (max_distance < 0: no such test),
 * |C(q)| == 1 or (double)d1 < ratio * (double)d2, and - with cross_check - q is the (distance, q') minimum over
 * { q' : gate(q', best) }.  Ratio and max_distance apply in the forward direction only.
 *
 * desc uint8 [n_rows, dim] and xy float32 [n_rows, 2] describe the same rows (the keypoints of all images back to back);
 * segment s (= one pair, described as for sfm_match_knn2_batched, HOST arrays) takes its queries from rows
 * [q_beg[s], q_end[s]) and its candidates from [t_beg[s], t_end[s]); either may be empty, and a single candidate row is
 * legal.  F: device double [n_seg, 9], row-major, x_j^T F x_i = 0.  Supported: SFM_METRIC_HAMMING with dim 16 / 32 / 64
 * bytes, SFM_METRIC_L2_U8 with dim 32 / 64 / 128; anything else is SFM_ERR_ARG.
 * Outputs (device): query_idx / train_idx / distance with room for n_out entries (sfm_guided_workspace_bytes reports
 * n_out = all query rows), the matches of segment s at [seg_ptr[s], seg_ptr[s+1]) (int64 [n_seg+1]), indices relative
 * to the segment, in query order; train_idx may repeat without cross_check.  n_candidates (optional, int32 [n_out]):
 * |C(q)| of every query row.  The output bytes are a function of the inputs alone. */
int sfm_guided_workspace_bytes(int metric, int32_t n_seg, const int64_t* q_beg_host, const int64_t* q_end_host,
                               const int64_t* t_beg_host, const int64_t* t_end_host, int64_t* n_out_host, int64_t* bytes_host);
int sfm_guided_match(sfm_handle h, int metric, const void* desc, int64_t n_rows, int dim, const float* xy, int32_t n_seg,
                     const int64_t* q_beg_host, const int64_t* q_end_host, const int64_t* t_beg_host, const int64_t* t_end_host,
                     const double* F, double gate_px, double ratio, double max_distance, int cross_check, int32_t* query_idx,
                     int32_t* train_idx, float* distance, int32_t* n_candidates, int64_t* seg_ptr, void* workspace,
                     int64_t workspace_bytes);

/* ------------------------------------------------------------------ bundle adjustment
 * Replaces what scipy.optimize.least_squares does for bundle_adjust: evaluation of the
 * closure `objective` (sfm_reconstruction.py:472-501), its Jacobian, the Huber scaling
 * (scipy _lsq/common.py:720-731), the damped step (H + alpha I) p = -g of the exact
 * trust-region solver (scipy _lsq/common.py:57-168), done block-sparse with a Schur complement,
 * and the trust-region loop itself (scipy _lsq/trf.py:401-560): sfm_ba_run_trf is the single call
 * that stands where `optimize.least_squares(...)` stands at sfm_reconstruction.py:506-514.
 * The stages are exported too: a multi-rank host (points sharded over GPUs, cameras replicated)
 * all-reduces the regions named `reduce_*` between them, either itself (sfm_amd/ba.py) or through
 * the sfm_reduce_fn hook of the trust-region loop.
 *
 * Parameter vector x = [cams (n_cams*cam_dim) | pts (n_pts*3)] float64, camera block
 * [rvec(3), t(3), fx, fy, cx, cy] for cam_dim 10 (reference, :416-427) or [rvec, t] for 6.
 * Observations are in the reference's point-major order (:430-435): pt_idx non-decreasing.
 */

/* What bundle_adjust packs before it calls SciPy (sfm_reconstruction.py:409-451) - nothing kernel-specific.
 * cam_idx / pt_idx / uv may be host or device pointers; sfm_ba_create_problem copies them. */
enum { SFM_CAMERA_SOLVER_AUTO = 0,       /* CG on the block-scaled system (n = n_cams * cam_dim even), the factorisation as its fallback (default) */
       SFM_CAMERA_SOLVER_CHOLESKY = 1,   /* bordered dense Cholesky + triangular solves */
       SFM_CAMERA_SOLVER_CG = 2 };       /* conjugate gradients on the block-scaled system, relative residual 1e-13 (~25 iterations
                                            at 200 cameras, ~40 at 1000): ONE persistent launch per system for n <= 2048 (the
                                            matrix rows in registers, the product all-gathered between workgroups through
                                            self-validating 8-byte granules); beyond, three launches per iteration that stream
                                            the 128 x 128 tiles of the LOWER triangle only (a tile serves both products it takes
                                            part in; partial sums added in fixed order); falls back to the factorisation when it
                                            does not converge (160 / 400 iterations) or meets non-positive curvature */
enum { SFM_BA_FP64 = 0,    /* every intermediate in float64 (default; the reference's arithmetic) */
       SFM_BA_MIXED = 1 }; /* Jacobian rows (and scaled residuals) stored in float32; every sum, W L^-T, S and the solve in float64 */
enum { SFM_UV_AS_GIVEN = 0,           /* observation k is compared with uv[k] */
       SFM_UV_REFERENCE_PAIRING = 1 }; /* the reference's own residual (sfm_reconstruction.py:480-486): projections are stacked camera
                                          by camera, `points2D` stays point-major, so the q-th observation in stable camera-sorted
                                          order meets uv[q].  Applied on the device from the camera-sorted list the problem builds
                                          anyway.  The pairing is a permutation of ALL observations: a sharded host applies it
                                          before it shards (sfm_amd.reconstruction.reference_pairing) and passes SFM_UV_AS_GIVEN */
typedef struct {
  int32_t n_cams, n_pts, cam_dim, apply_reg;   /* apply_reg: add the 4 regulariser rows per camera (:489-499); rank 0 only */
  int64_t n_obs;
  const int32_t* cam_idx;    /* [n_obs] */
  const int32_t* pt_idx;     /* [n_obs] non-decreasing */
  const double*  uv;         /* [n_obs*2] pixel each observation is compared with */
  double fx0, fy0, cx0, cy0; /* pre-BA self.K (:492-497); intrinsics of every camera when cam_dim == 6 */
  double width, height, reg_weight;
  int32_t precision;         /* SFM_BA_FP64 | SFM_BA_MIXED */
  int32_t camera_solver;     /* how sfm_ba_schur_solve solves the formed n x n camera system: SFM_CAMERA_SOLVER_* */
  int32_t uv_pairing;        /* SFM_UV_AS_GIVEN | SFM_UV_REFERENCE_PAIRING */
  int32_t reserved;          /* 0 */
} sfm_ba_desc;

typedef struct sfm_ba_prob* sfm_ba_problem;    /* opaque; owns its index structure (device memory) */

/* Multi-rank hook (points sharded over GPUs, cameras replicated): all-reduce `count` doubles at device pointer
 * `data` (inside the bound workspace) in place across the ranks: op 0 = SUM, 1 = MAX.  Return 0 on success.
 * NULL = single rank. */
typedef int (*sfm_reduce_fn)(void* user, void* data, int64_t count, int op);

/* ---- collectives inside the library (multi-rank: points sharded over GPUs, cameras replicated - SURVEY.md section 8e).
 * RCCL (= NCCL's API over xGMI) is dlopen'ed on first use, so nothing here is needed on one GPU.  One communicator per
 * handle; sfm_comm_allreduce enqueues ncclAllReduce (float64, in place, op 0 = SUM / 1 = MAX) on the handle's stream: no
 * host synchronisation.  sfm_comm_reduce_hook IS an sfm_reduce_fn: pass it as `reduce` with the handle as `reduce_user`
 * and every exchange of the trust-region loop / of sfm_ba_solve_pcg runs on the stream between the stages.
 * Bootstrap like any NCCL program: rank 0 calls sfm_comm_unique_id and ships the 128 bytes to the other ranks by whatever
 * the host has (MPI, a file, torch.distributed), then every rank calls sfm_comm_init_rank (collective).  A host that
 * already owns an ncclComm_t for the handle's device hands it over with sfm_comm_adopt (not destroyed by the library). */
enum { SFM_COMM_ID_BYTES = 128 };
int sfm_comm_unique_id(sfm_handle h, void* id_host);
int sfm_comm_init_rank(sfm_handle h, const void* id_host, int32_t n_ranks, int32_t rank);
int sfm_comm_adopt(sfm_handle h, void* nccl_comm, int32_t n_ranks, int32_t rank);
int sfm_comm_destroy(sfm_handle h);
int sfm_comm_info(sfm_handle h, int32_t* n_ranks_host, int32_t* rank_host);      /* 0 ranks: no communicator */
int sfm_comm_allreduce(sfm_handle h, double* data, int64_t count, int op);
int sfm_comm_reduce_hook(void* handle_as_user, void* data, int64_t count, int op);

/* Validates the indices and builds, ON THE DEVICE, everything the kernels need besides the arrays above:
 * per-point / per-camera observation lists, the camera-pair lists of the Schur complement and their split
 * into work items (sfm_ba_structure shows them).  Synchronises the stream (sizes are data-dependent).
 * SFM_ERR_ARG for out-of-range or non point-major indices. */
int  sfm_ba_create_problem(sfm_handle h, const sfm_ba_desc* desc, sfm_ba_problem* out);
void sfm_ba_destroy_problem(sfm_ba_problem p);

/* The index structure as built (device pointers, int32), for inspection and tests; sfm_amd/structure.py is
 * its host-side mirror and produces bit-identical arrays. */
typedef struct {
  int64_t n_obs, n_pairs, n_items, n_cchunks, xcd_max_items;
  const int32_t* pt_ptr;     /* [n_pts+1]  obs range of each point (track) */
  const int32_t* cam_ptr;    /* [n_cams+1] ranges into cam_obs */
  const int32_t* cam_obs;    /* [n_obs] observation ids grouped by camera, ascending inside a camera */
  const int32_t* blk_ptr;    /* [n_cams*(n_cams+1)/2 + 1] ranges into pair_k/pair_k2, block (c<=c2) at c*n_cams - c*(c-1)/2 + (c2-c) */
  const int32_t* pair_k;     /* [n_pairs] observation of camera c  on a shared track */
  const int32_t* pair_k2;    /* [n_pairs] observation of camera c2 on the same track */
  const int32_t* item_ptr;   /* [n_blocks+1] work items per block: each <= 256 consecutive pairs of ONE block */
  const int32_t* item_beg;   /* [n_items] ranges into pair_k / pair_k2 */
  const int32_t* item_end;   /* [n_items] */
  const int32_t* xcd_ptr;    /* [9]  item ids of block rows c = x (mod 8): xcd_items[xcd_ptr[x] .. xcd_ptr[x+1]) */
  const int32_t* xcd_items;  /* [n_items] (workgroup b of the Schur kernel serves group b % 8: XCD-local L2 reuse of G) */
  const int32_t* cch_ptr;    /* [n_cams+1] chunks per camera: each <= 256 consecutive entries of cam_obs of ONE camera */
  const int32_t* cch_beg;    /* [n_cchunks] ranges into cam_obs */
  const int32_t* cch_end;    /* [n_cchunks] */
} sfm_ba_structure;
int sfm_ba_get_structure(sfm_ba_problem p, sfm_ba_structure* out_host);
/* How the Schur kernel walks a work item (device pointers, int32 [n_items]; inspection and tests): item i of block b takes
 * pairs first[i] + j * stride[i], j < count[i] <= 256.  The n items of a block partition its range of pair_k / pair_k2: blocks
 * of n <= 2 items by the contiguous stretches item_beg / item_end (stride 1), blocks of n >= 3 items interleaved - item i takes
 * pairs blk_ptr[b] + i + j n (stride n), so that every item of a block row walks its camera's observation list at one pace. */
int sfm_ba_get_item_descriptors(sfm_ba_problem p, const int32_t** first, const int32_t** stride, const int32_t** count);

/* Byte offsets into the workspace of the regions the host reads or all-reduces. */
typedef struct {
  int64_t total_bytes;
  int64_t rec_off, rec_stride;      /* per observation: Jc~ [2][cam_dim] (robust-scaled), doubles; stride in bytes */
  int64_t recB_off;                 /* per observation: Jp~ [2][3], f~ [2] (8 doubles) */
  int64_t B_off, gc_off;            /* [n_cams][cam_dim][cam_dim], [n_cams][cam_dim]   (this rank's partial sums) */
  int64_t Cp_off, gp_off;           /* [n_pts][6] (xx,xy,xz,yy,yz,zz), [n_pts][3] */
  int64_t reduce_lin_off, reduce_lin_count;     /* doubles: [gc copy (n) | cost | ||gp||^2 | diag(B) (n)], n = n_cams*cam_dim  SUM */
  int64_t gmax_off;                              /* 2 doubles: max |gp|, max diag(C_j)                       MAX */
  int64_t reduce_S_off, reduce_S_count;         /* doubles: [S (n x n, n = n_cams*cam_dim) | r (n)]          SUM */
  int64_t reduce_Sp_off, reduce_Sp_count;       /* doubles: lower triangle of S by rows, then r: n(n+1)/2 + n - what
                                                   sfm_ba_pack_system fills and sfm_ba_unpack_system reads (the factorisation
                                                   only reads the lower triangle, so ranks exchange half the bytes) SUM */
  int64_t reduce_q_off, reduce_q_count;         /* doubles: [q_c (n) | ||p_pts||^2 | p_pts^T C_a^-1 p_pts]   SUM
                                                   q_c = -W C_a^-1 p_pts, the point part of rhs2 = p_c + q_c (sfm_ba_finish_solve adds p_c);
                                                   q_c is written only when want_q, the two sums always */
  int64_t reduce_step_off, reduce_step_count;   /* doubles: [||J~ s||^2 | f~^T J~ s | cost(x+s) | ||s_pts||^2 | ||x_pts+s_pts||^2 ] SUM */
  int64_t pc_off, pp_off;           /* camera / point part of p = -(H + alpha I)^-1 g */
  int64_t scalars_off;              /* 16 doubles, see SFM_SC_* */
  int64_t G_off;                    /* [n_obs][G stride]: [3][cam_dim] doubles per observation, padded to 32 doubles (256 B = two whole
                                       128-byte lines) for cam_dim 10, 18 for cam_dim 6 */
  int64_t cg_Ap_off, cg_M_off;      /* sfm_ba_solve_pcg: S p [n] and the block-Jacobi blocks [n_cams][cam_dim][cam_dim] (this rank's partial sums) SUM */
} sfm_ba_layout;

enum { SFM_SC_COST = 0, SFM_SC_GNORM2 = 1, SFM_SC_GINF = 2, SFM_SC_PNORM2 = 3, SFM_SC_PQ = 4,
       SFM_SC_JS2 = 5, SFM_SC_GTS = 6, SFM_SC_COST_NEW = 7, SFM_SC_SNORM2 = 8, SFM_SC_XNEW_NORM2 = 9,
       SFM_SC_CHOL_FAIL = 10 /* 0 ok, 1 not positive definite, 2 triangular solve stalled, 3 step not finite */,
       SFM_SC_HDIAG = 11 /* max diag(H) */, SFM_SC_COUNT = 16 };

/* Layout of the workspace of a problem.  The workspace (total_bytes, device memory) is the caller's: bind it
 * before the first stage; workspace == NULL makes the library allocate (and own) one.  rec / recB hold
 * float32 values when the problem was created with SFM_BA_MIXED (rec_stride is in bytes); G is always float64. */
int sfm_ba_get_layout(sfm_ba_problem p, sfm_ba_layout* out_host);
int sfm_ba_bind_workspace(sfm_handle h, sfm_ba_problem p, void* workspace, int64_t workspace_bytes);

/* cost(x) = 1/2 sum rho(f_i^2) (Huber, per scalar) -> partial into reduce_step[2] (this rank's observations). */
int sfm_ba_cost(sfm_handle h, sfm_ba_problem p, const double* x);
/* per-observation reprojection error ||proj - uv||_2.  shared_k != 0: ONE shared K = (fx0,fy0,cx0,cy0)
 * for every camera (compute_reconstruction_stats, :582-631); shared_k == 0: each camera's own
 * intrinsics when cam_dim == 10 (the reprojection rows of `objective`, :478-486). */
int sfm_ba_reproj_errors(sfm_handle h, sfm_ba_problem p, const double* x, int shared_k, double* err_out);

/* sum over the problem's observations of ||proj - uv||^2 at x, to the host (synchronises): the reprojection part of the
 * ||objective(x)||_2 that bundle_adjust logs before and after the solve (:522-524). */
int sfm_ba_residual_norm2(sfm_handle h, sfm_ba_problem p, const double* x, int shared_k, double* out_host);

/* The same without a problem object (nothing but the three packed arrays is needed): what
 * compute_reconstruction_stats (:582-631) computes per observation.  All pointers are device pointers; indices
 * must be in range (the caller's responsibility: there is no structure pass here). */
int sfm_reproj_errors(sfm_handle h, int32_t n_cams, int32_t cam_dim, int64_t n_obs, const int32_t* cam_idx,
                      const int32_t* pt_idx, const double* uv, const double* x, double fx, double fy, double cx,
                      double cy, int shared_k, double* err_out);

/* Linearise at x: records, B, gc, Cp, gp, cost -> reduce_lin region (+ gmax). */
int sfm_ba_linearize(sfm_handle h, sfm_ba_problem p, const double* x);
/* After the host has (all-)reduced reduce_lin and gmax: scalars COST, GNORM2, GINF, HDIAG. */
int sfm_ba_finish_linearize(sfm_handle h, sfm_ba_problem p);

/* Damped solve in three stages around two reductions. */
int sfm_ba_schur_build(sfm_handle h, sfm_ba_problem p, double alpha);          /* -> reduce_S (partial) */
/* Multi-rank only: reduce_S (lower triangle + r) -> reduce_Sp before the all-reduce, and back after it. */
int sfm_ba_pack_system(sfm_handle h, sfm_ba_problem p);
int sfm_ba_unpack_system(sfm_handle h, sfm_ba_problem p);
int sfm_ba_schur_solve(sfm_handle h, sfm_ba_problem p, double alpha, int want_q); /* chol, p_c, p_p; -> reduce_q (partial) */
int sfm_ba_finish_solve(sfm_handle h, sfm_ba_problem p, int want_q);              /* scalars PNORM2 (and PQ) */

/* The same damped solve WITHOUT forming or factoring S: conjugate gradients on the implicit Schur complement
 * S v = (B + alpha I) v - W (C + alpha I)^-1 W^T v (two passes over G per product), preconditioned with the exact
 * d x d diagonal blocks of S.  One call = schur_build + schur_solve + finish_solve: afterwards pc / pp hold the step
 * and the scalars PNORM2 (and PQ when want_q) are set; SFM_SC_CHOL_FAIL != 0 when S or a block is not positive
 * definite.  A system that has not reached rtol after max_iter iterations (measured: near convergence of the outer loop,
 * alpha ~ 1e-3, S nearly singular along the gauge directions, block-Jacobi PCG stalls at 1e-2 .. 1e-4) is never accepted:
 * the damped solve is then redone by the formed-S route (schur_build / schur_solve / finish_solve, reductions through the
 * same hook) and counted (sfm_ba_pcg_stats) - an inexact p would silently steer the alpha iteration.  Stops when ||r|| <= rtol ||r_0|| (checked every 8 iterations) or after max_iter iterations per system
 * (want_q solves two).  Multi-rank: `reduce` sums, per call, the right-hand side and the diagonal blocks once and
 * ONE vector of n doubles per iteration - against n(n+1)/2 + n doubles and a replicated factorisation on the dense
 * route; meant for many cameras (BASELINE config 5) and for scaling over GPUs.  iters_host: CG iterations spent. */
int sfm_ba_solve_pcg(sfm_handle h, sfm_ba_problem p, double alpha, int want_q, double rtol, int32_t max_iter,
                     sfm_reduce_fn reduce, void* reduce_user, int32_t* iters_host);

/* s = scale * p;  x_new = x + s;  partial sums for the predicted reduction and cost(x_new) -> reduce_step. */
int sfm_ba_step(sfm_handle h, sfm_ba_problem p, const double* x, double scale, double* x_new);
int sfm_ba_finish_step(sfm_handle h, sfm_ba_problem p, const double* x, double scale, const double* x_new);

/* Copy the SFM_SC_COUNT scalars to the host.  Waits for the FINISHING call of the stage enqueued last (sfm_ba_finish_linearize /
 * _finish_solve / _finish_step, sfm_ba_solve_pcg, the trust-region loop's own stages): its kernel publishes a ticket behind the
 * scalars in a pinned page and this call spins on it, so it returns as soon as the scalars are there - everything enqueued BEFORE
 * that kernel has completed by then (stream order), but the call is not a full stream synchronisation: work enqueued after a
 * finishing call is not waited for (SFM_POLL_SCALARS=0 restores the synchronisation).  This is also where a damped solve COMPLETES: the
 * persistent conjugate-gradient launch of the second camera system (sfm_ba_finish_solve with want_q) is not waited for
 * there - its verdict arrives with this synchronisation, and if it did not converge the q term is redone from the
 * factorisation here (no exchange between ranks is involved).  Read the scalars through this call, not from the workspace. */
int sfm_ba_read_scalars(sfm_handle h, sfm_ba_problem p, double* out_host);
/* Tell the library that this problem is ONE RANK'S SHARD of a multi-rank solve (points sharded, cameras replicated: SURVEY.md
 * section 8e; the reference has no counterpart - its solve is single-process, /root/reference/utils/sfm_reconstruction.py:506-514).
 * Every rank must then take the same route through the replicated camera solve, because the routes sum in different orders:
 * a persistent-CG launch that had to be abandoned on one rank is launched again instead of being replaced by the
 * launch-per-iteration route on that rank alone, and if it cannot run the solve fails with SFM_ERR_HIP (set SFM_CGS_PERSIST=0
 * on all ranks).  Implied by a non-null reduce hook in sfm_ba_trf_begin / sfm_ba_run_trf / sfm_ba_solve_pcg; a host that
 * drives the stages itself and reduces between them calls this once after sfm_ba_create_problem. */
int sfm_ba_set_sharded(sfm_handle h, sfm_ba_problem p, int sharded);
/* SFM_CAMERA_SOLVER_CG bookkeeping since the problem was created: CG iterations spent, solves that fell back. */
int sfm_ba_solver_stats(sfm_ba_problem p, int64_t* cg_iters_host, int64_t* cg_fallbacks_host);

/* sfm_ba_solve_pcg bookkeeping since the problem was created: damped solves that were handed to the formed-S route
 * because a system ran out of iterations above rtol, and the worst relative residual ||r|| / ||r_0|| PCG had reached there. */
int sfm_ba_pcg_stats(sfm_ba_problem p, int64_t* fallbacks_host, double* worst_relres_host);

/* ---- the trust-region loop (scipy _lsq/trf.py:401-560 trf_no_bounds + common.py:57-168,222-248,705-717),
 * control flow on the host, every data-parallel stage above on the device.  Same state machine as
 * sfm_amd/trf.py (the host-language mirror the multi-rank CPU tests drive). */
enum { SFM_SOLVER_DENSE = 0, SFM_SOLVER_PCG = 1 };
typedef struct {
  double ftol, xtol, gtol;        /* the reference passes ftol = xtol = 1e-4 (:512-513); SciPy's default gtol = 1e-8 */
  int32_t max_nfev;               /* 100 (:511) */
  int32_t max_outer;              /* < 0: no limit; otherwise stop after this many outer iterations (fixed schedules) */
  int32_t check_tolerances;       /* 0 turns the gtol / ftol / xtol tests off (throughput runs) */
  int32_t solver;                 /* SFM_SOLVER_DENSE: Schur complement + dense Cholesky; SFM_SOLVER_PCG: sfm_ba_solve_pcg */
  double  pcg_rtol;               /* SFM_SOLVER_PCG: relative residual (<= 0: 1e-13) */
  int32_t pcg_max_iter;           /* SFM_SOLVER_PCG: iterations per system before the formed-S fallback (<= 0: 400) */
  int32_t reserved;
} sfm_trf_options;
typedef struct {
  double cost, optimality;        /* 1/2 sum rho(f^2) and ||g||_inf at the returned x */
  int32_t nfev, njev, status;     /* SciPy's counters and termination status (0: max_nfev, 1 gtol, 2 ftol, 3 xtol, 4 both) */
  int32_t n_solves, n_outer;
  int32_t cg_iters;               /* SFM_SOLVER_PCG: conjugate-gradient iterations over all damped solves */
} sfm_trf_result;
typedef struct sfm_trf_state_s* sfm_trf_state;
/* x: [n_cams*cam_dim + 3*n_pts] device doubles, start point in, current iterate out (after every sfm_ba_trf_outer).
 * x_norm_pts_only_local: nothing to set - with a reduce hook the point part of ||x|| is summed over the ranks. */
int  sfm_ba_trf_begin(sfm_handle h, sfm_ba_problem p, double* x, const sfm_trf_options* opt,
                      sfm_reduce_fn reduce, void* reduce_user, sfm_trf_state* out);
/* One outer iteration: the trial steps of the current linearisation up to the accepted one, then the next
 * linearisation.  *more = 0 once the loop has ended (status set, max_nfev or max_outer reached). */
int  sfm_ba_trf_outer(sfm_trf_state st, int* more);
int  sfm_ba_trf_result(sfm_trf_state st, sfm_trf_result* out);
/* (alpha, Delta, ||step||, accepted) of every trial so far, 4 doubles each; returns the number of trials. */
int  sfm_ba_trf_trace(sfm_trf_state st, double* out_host, int32_t capacity_trials);
void sfm_ba_trf_end(sfm_trf_state st);
/* begin + outer until done + result + end. SFM_ERR_NUMERIC when a damped system is not positive definite or a
 * step is not finite (x then holds the last accepted iterate). */
int  sfm_ba_run_trf(sfm_handle h, sfm_ba_problem p, double* x, const sfm_trf_options* opt,
                    sfm_reduce_fn reduce, void* reduce_user, sfm_trf_result* out);

/* Dense SPD helpers used by the solve, exported for tests: in-place lower Cholesky of a [n][n]
 * row-major matrix and solves with the factor.  fail_flag: device int32, set when a pivot <= 0. */
int sfm_dense_cholesky(sfm_handle h, double* a, int32_t n, int32_t* fail_flag);
int sfm_dense_trsv(sfm_handle h, const double* l, int32_t n, double* b, int transpose);
/* Test helpers: the solve's own path on a workspace the caller owns.  offsets_host [8]: the offsets, in doubles, of the
 * regions Ld, Dinv, DinvT, inv64, flag, Lm, LmT and their total.  sfm_dense_factor_ws clears the flag word, factors
 * a (device [nrows][n], nrows = n or n + 1: a last row leaves as L^-1 of it; a is consumed) into ws and synchronises;
 * sfm_dense_trsv_ws solves L y = b (transpose 0) or L^T x = b (1) with what ws holds: b is destroyed, the flag is left
 * as it is (1: a pivot was not positive, 2: a solve stalled). */
int sfm_dense_ws_layout(int32_t n, int64_t* offsets_host);
int sfm_dense_factor_ws(sfm_handle h, double* a, int32_t n, int32_t nrows, double* ws);
int sfm_dense_trsv_ws(sfm_handle h, int32_t n, double* ws, double* b, double* xout, int transpose);

/* ------------------------------------------------------------------ driver-side rows either side of the path
 * (SURVEY.md section 8f).  All three are batched over "segments" (one segment = one image pair), so the
 * per-pair Python loops of the reference become one launch.  seg pointers are DEVICE int64 arrays.
 */

/* Replaces the dense [T,M,2] broadcast + np.where of find_2d3d_matches
 * (/root/reference/utils/sfm_reconstruction.py:209-218): for every segment s, all pairs
 * (track row i in [t_ptr[s], t_ptr[s+1]), correspondence m in [m_ptr[s], m_ptr[s+1])) with
 * sqrt(dx*dx + dy*dy) < radius in float64, emitted segment-major, row-major (np.where order).
 * track_xy [T][2], corr_xy [M][2] float64 (float32 pixels widened exactly, as NumPy's broadcast does).
 * out_row / out_col: global row / correspondence indices, room for `capacity` pairs; pairs beyond the
 * capacity are counted but not written.  *n_pairs: device int64 total.  workspace from
 * sfm_assoc_workspace_bytes. */
int sfm_assoc_workspace_bytes(int64_t n_rows, int64_t* bytes_host);
int sfm_assoc_radius(sfm_handle h, const double* track_xy, const int64_t* t_ptr, const double* corr_xy,
                     const int64_t* m_ptr, int32_t n_seg, int64_t n_rows, double radius,
                     int32_t* out_row, int32_t* out_col, int64_t capacity, int64_t* n_pairs,
                     void* workspace, int64_t workspace_bytes);

/* Replaces the per-track cv2.triangulatePoints call + reprojection gate of triangulate_point
 * (sfm_reconstruction.py:287-307) inside add_new_matches' loop (:381-385): two-view DLT (null vector of
 * the 4x4 system x*P[2]-P[0], y*P[2]-P[1], by one-sided Jacobi SVD in float64), X = v[:3]/v[3], and
 * valid[i] = 0 when either view reprojects further than max_err px (comparison `err > max_err`, so NaN
 * passes exactly as in the reference).  proj [n_cams][12] row-major 3x4 K[R|t]; cam0/cam1 [n] index it;
 * x0/x1 [n][2] float64 pixels.  X [n][3]; err [n][2] (optional, may be NULL). */
int sfm_triangulate2(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam0, const int32_t* cam1,
                     const double* x0, const double* x1, int64_t n, double max_err,
                     double* X, int32_t* valid, double* err);

/* Replaces the per-match arithmetic of geometric_verification
 * (/root/reference/utils/find_matches.py:160-174): epilines as cv2.computeCorrespondEpilines forms them
 * (float64 accumulate, a^2+b^2 = 1, stored float32), the float32 symmetric epipolar distance and
 * mask = err < threshold.  F [n_seg][9] float64; seg_ptr [n_seg+1]; pts1/pts2 [n][2] float32. */
int sfm_epipolar_errors(sfm_handle h, const double* F, const int64_t* seg_ptr, int32_t n_seg,
                        const float* pts1, const float* pts2, int64_t n, float threshold,
                        float* err, uint8_t* mask);

/* ------------------------------------------------------------------ fundamental-matrix RANSAC, batched over pairs
 * The step between match_features and geometric_verification in the reference's pair loop
 * (cv2.findFundamentalMat with cv2.FM_RANSAC, /root/reference/utils/find_matches.py:282), for every pair of a
 * driver step in one call.  Structure as OpenCV's FM_RANSAC is recalled (not pinned): samples of 7, the 7-point
 * solver (up to three real solutions), error = the larger of the two squared point-to-epipolar-line distances,
 * inlier when error <= threshold^2, best model = most inliers (ties: lowest hypothesis index), F scaled to
 * F[2][2] = 1.  Deviations: every one of the n_hyp hypotheses runs (no early exit on confidence), and the samples
 * are data: drawn by a stateless integer hash of (seed, segment, hypothesis, draw) written out in
 * sfm_amd/csrc/twoview.hip, or supplied by the caller.  The result is a function of (points, samples) alone.
 * All arithmetic float64.  seg_ptr [n_seg+1] device int64; pts1 / pts2 [n][2] float32 pixels.  A match with a NaN
 * or infinite coordinate is never an inlier; a sample index outside its segment voids that hypothesis.
 *
 * samples [n_seg][n_hyp][7] int32, segment-local indices, 7 distinct per hypothesis (-1 for segments with fewer
 * than 7 points).  status [n_seg]: 0 ok, 1 fewer than 7 points, 2 no sample gave a model; status 1 / 2 segments get
 * F = 0, an all-zero mask and count 0.  hyp_count [n_seg][n_hyp] (may be NULL): per hypothesis the best inlier count
 * of its candidates.  refine != 0: normalised 8-point least squares over the winner's inliers, rank 2 enforced,
 * re-scored with the same error; it replaces the winner only if its count is not lower (refined[s] = 1 then;
 * refined may be NULL).  Everything runs on the handle's stream without host synchronisation. */
int sfm_fund_workspace_bytes(int64_t n_points, int32_t n_seg, int32_t n_hyp, int64_t* bytes_host);
int sfm_fund_draw_samples(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, int32_t n_hyp, uint64_t seed,
                          int32_t* samples);
int sfm_fund_ransac(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, const float* pts1, const float* pts2,
                    int64_t n, const int32_t* samples, int32_t n_hyp, double threshold, int32_t refine,
                    double* F, uint8_t* mask, int32_t* n_inliers, int32_t* status, int32_t* hyp_count,
                    int32_t* refined, void* workspace, int64_t workspace_bytes);

/* ------------------------------------------------------------------ PnP RANSAC, batched over candidate images
 * The camera-registration step of the reference's add_new_image (`pnp_ransac`: cv2.solvePnPRansac with 1,000
 * iterations, 8 px, SOLVEPNP_ITERATIVE), for every candidate image of a step in one call; one segment = one image.
 * Structure as OpenCV's solvePnPRansac is recalled (not pinned): EPnP on samples of 5 inside the loop, reprojection
 * error against the threshold, most inliers wins, then the ITERATIVE (Levenberg-Marquardt) solver on the inliers.
 * Deviations, on purpose: minimal samples of 3 solved by closed-form P3P with all of its (up to four) roots scored;
 * every one of the n_hyp hypotheses runs (no early exit on confidence); the samples are data, drawn by the stateless
 * integer hash of sfm_fund_draw_samples with 3 slots, or supplied by the caller.  The result is a function of
 * (points, K, samples) alone, bitwise.
 * All arithmetic float64.  seg_ptr [n_seg+1] device int64; X [n][3] float64 world points; uv [n][2] float32 pixels;
 * Kseg [n_seg][4] float64 (fx, fy, cx, cy).  Inlier rule, without division: p = K [R|t] [X; 1], inlier when p2 > 0
 * and (p0 - u p2)^2 + (p1 - v p2)^2 <= threshold^2 p2^2; best model = most inliers (ties: lowest hypothesis index,
 * then lowest root slot).  A point with a NaN or infinite coordinate is never an inlier; a sample that holds one, or
 * whose three world points span no area (|d1 x d2|^2 <= 1e-20 |d1|^2 |d2|^2), gives no model; a sample index
 * outside its segment voids that hypothesis.
 *
 * samples [n_seg][n_hyp][3] int32, segment-local indices, 3 distinct per hypothesis (-1 for segments with fewer
 * than 4 points).  status [n_seg]: 0 ok, 1 fewer than 4 points, 2 no sample gave a model; status 1 / 2 segments get
 * Rt = 0, an all-zero mask and count 0.  Rt [n_seg][12]: row-major 3 x 4 [R|t].  hyp_count [n_seg][n_hyp] (may be
 * NULL): per hypothesis the best inlier count of its candidates.  refine != 0: Levenberg-Marquardt on (rvec, t) -
 * the rotation vector taken about the current rotation - over the winner's inliers, at most 30 steps, re-scored
 * over all points with the same rule; it replaces the winner only if its count is not lower (refined[s] = 1 then;
 * refined may be NULL).  Everything runs on the handle's stream without host synchronisation. */
int sfm_pnp_workspace_bytes(int64_t n_points, int32_t n_seg, int32_t n_hyp, int64_t* bytes_host);
int sfm_pnp_draw_samples(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, int32_t n_hyp, uint64_t seed,
                         int32_t* samples);
int sfm_pnp_ransac(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, const double* X, const float* uv, int64_t n,
                   const double* Kseg, const int32_t* samples, int32_t n_hyp, double threshold, int32_t refine,
                   double* Rt /* [n_seg][12], row-major [R|t] */, uint8_t* mask, int32_t* n_inliers, int32_t* status,
                   int32_t* hyp_count /* may be NULL */, int32_t* refined /* may be NULL */, void* workspace,
                   int64_t workspace_bytes);

/* ------------------------------------------------------------------ essential-matrix RANSAC, batched over pairs
 * cv2.findEssentialMat(pts1, pts2, K, cv2.RANSAC, threshold) for every pair of a step in one call: the calibrated
 * counterpart of sfm_fund_ransac, for callers that go on to a pose (sfm_pose_recover with is_fundamental = 0).
 * E = K^T F K of a 7-point F is not an essential matrix, and the pose taken from it leaves errors of many pixels.
 * Structure as OpenCV's is recalled (not pinned): samples of 5, Nister's five-point solver (up to 10 real solutions;
 * its steps are listed in sfm_amd/csrc/essential_solve.h), most inliers wins (ties: lowest hypothesis index, then
 * lowest root slot).  Deviations, on purpose: the error rule is sfm_fund_ransac's, in pixels on F = K^-T E K^-1 (the
 * larger of the two squared point-to-epipolar-line distances <= threshold^2); every one of the n_hyp hypotheses runs;
 * the samples are data, drawn by the stateless integer hash of sfm_fund_draw_samples with 5 slots, or supplied by the
 * caller.  The result is a function of (points, K, samples) alone, bitwise, run to run and independent of the batch.
 * All arithmetic float64.  seg_ptr [n_seg+1] device int64; pts1 / pts2 [n][2] float32 pixels; Kseg [n_seg][4] float64
 * (fx, fy, cx, cy).  A match with a NaN or infinite coordinate is never an inlier.  A hypothesis gives no model if its
 * sample holds such a match or an index outside its segment, or if two matches of its sample share a pixel in image 1
 * or share a pixel in image 2 (float32 == on both coordinates: a doubled match leaves the 5 x 9 system with rank 4).
 *
 * samples [n_seg][n_hyp][5] int32, segment-local indices, 5 distinct per hypothesis (-1 for segments with fewer than
 * 5 matches).  status [n_seg]: 0 ok, 1 fewer than 5 matches, 2 no hypothesis gave an inlier; status 1 / 2 segments get
 * E = 0, an all-zero mask and count 0.  E [n_seg][9] row-major, in normalised coordinates (x2^T E x1 = 0 for
 * x = K^-1 [u, v, 1]), |E|_F = sqrt(2), its entry of largest magnitude (the first on a tie) positive.  hyp_count
 * [n_seg][n_hyp] (may be NULL): per hypothesis the best inlier count of its candidates.  refine != 0: the same solver
 * over all inliers of the winner (the four eigenvectors of the smallest eigenvalues of A^T A in place of the null
 * space), every candidate re-scored with the same rule; the best replaces the winner only if its count is not lower
 * (refined[s] = 1 then; refined may be NULL).  Everything runs on the handle's stream without host synchronisation. */
int sfm_ess_workspace_bytes(int64_t n_points, int32_t n_seg, int32_t n_hyp, int64_t* bytes_host);
int sfm_ess_draw_samples(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, int32_t n_hyp, uint64_t seed,
                         int32_t* samples);
int sfm_ess_ransac(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, const float* pts1, const float* pts2, int64_t n,
                   const double* Kseg /* [n_seg][4] */, const int32_t* samples /* [n_seg][n_hyp][5] */, int32_t n_hyp,
                   double threshold /* pixels */, int32_t refine, double* E /* [n_seg][9] */, uint8_t* mask,
                   int32_t* n_inliers, int32_t* status, int32_t* hyp_count /* may be NULL */,
                   int32_t* refined /* may be NULL */, void* workspace, int64_t workspace_bytes);

/* ------------------------------------------------------------------ homography RANSAC, batched over pairs
 * cv2.findHomography(pts1, pts2, cv2.RANSAC, threshold) for every pair of a step in one call: x2 ~ H x1.  A pair whose
 * matches lie on a plane, or whose cameras share a centre, has no defined F, and an H explains nearly all of its
 * matches: the ratio of this call's inlier count to sfm_fund_ransac's (or sfm_ess_ransac's) tells such a pair apart.
 * Structure as OpenCV's is recalled (not pinned): samples of 4, a subset check, the DLT on normalised coordinates, the
 * forward transfer error against threshold^2, most inliers wins (ties: lowest hypothesis index), H scaled to
 * H[2][2] = 1.  Deviations, on purpose: every one of the n_hyp hypotheses runs; the samples are data, drawn by the
 * stateless integer hash of sfm_fund_draw_samples with 4 slots, or supplied by the caller; the refit is linear and NO
 * Levenberg-Marquardt step follows it.  The result is a function of (points, samples) alone, bitwise, run to run and
 * independent of the batch.
 * All arithmetic float64.  seg_ptr [n_seg+1] device int64; pts1 / pts2 [n][2] float32 pixels.
 * Sample rule, on the float32 pixels widened to double: for each of the triples (i, j, k) = (0,1,2), (0,1,3), (0,2,3),
 * (1,2,3) and each image, a = (xj - xi)(yk - yi) - (yj - yi)(xk - xi), d1 = |pj - pi|^2, d2 = |pk - pi|^2; the sample
 * gives no model unless a^2 > 1e-6 d1 d2 in both images (collinear or repeated points), and none if (a1 > 0) != (a2 > 0)
 * for any triple (the sample reverses an orientation).  A sample that holds a NaN or infinite coordinate, or an index
 * outside its segment, gives no model either.
 * Solve: on the segment's Hartley-normalised coordinates (the transforms of sfm_fund_ransac, over the finite matches),
 * the 8 x 9 system with the rows [x, y, 1, 0, 0, 0, -u x, -u y, -u] and [0, 0, 0, x, y, 1, -v x, -v y, -v] per match;
 * its null vector by Givens rotations of column pairs (sfm_amd/csrc/homography_solve.h); H = T2^-1 Hn T1; a
 * non-finite H is no model.
 * Inlier rule, without division (sfm_amd/csrc/homography_rule.h): X = (h0 x + h1 y) + h2, Y = (h3 x + h4 y) + h5,
 * W = (h6 x + h7 y) + h8; inlier when W != 0 and (X - u W)^2 + (Y - v W)^2 <= threshold^2 W^2.  A match with a NaN or
 * infinite coordinate is never an inlier.
 *
 * samples [n_seg][n_hyp][4] int32, segment-local indices, 4 distinct per hypothesis (-1 for segments with fewer than
 * 4 matches).  status [n_seg]: 0 ok, 1 fewer than 4 matches, 2 no hypothesis gave an inlier; status 1 / 2 segments get
 * H = 0, an all-zero mask and count 0.  H [n_seg][9] row-major.  hyp_count [n_seg][n_hyp] (may be NULL): per hypothesis
 * its inlier count.  refine != 0, with at least 4 inliers: the normalised DLT over the winner's inliers (smallest
 * eigenvector of the 9 x 9 normal matrix), re-scored with the same rule; it replaces the winner only if its count is not
 * lower (refined[s] = 1 then; refined may be NULL).  Argument checks and return codes are those of sfm_fund_ransac.
 * Everything runs on the handle's stream without host synchronisation. */
int sfm_hom_workspace_bytes(int64_t n_points, int32_t n_seg, int32_t n_hyp, int64_t* bytes_host);
int sfm_hom_draw_samples(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, int32_t n_hyp, uint64_t seed,
                         int32_t* samples);
int sfm_hom_ransac(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, const float* pts1, const float* pts2,
                   int64_t n, const int32_t* samples, int32_t n_hyp, double threshold, int32_t refine,
                   double* H, uint8_t* mask, int32_t* n_inliers, int32_t* status, int32_t* hyp_count,
                   int32_t* refined, void* workspace, int64_t workspace_bytes);

/* ------------------------------------------------------------- relative-pose recovery, batched over image pairs
 * The cv2.recoverPose(E, pts1, pts2, K) call of the reference's find_best_initial_pair / initialize_reconstruction, for
 * every pair of a data set in one call; one segment = one pair.  opencv-python 4.11's recoverPose and
 * decomposeEssentialMat as recalled (not pinned; the reference's shipped run pins this row, tests/pose_reference.py):
 * float32 pixels widened to double and normalised as (u - cx) / fx, (v - cy) / fy; E = U S V^T with both determinants
 * +1, R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2]; the candidates [R1|t], [R2|t], [R1|-t], [R2|-t] each triangulate every
 * point against [I|0] by the DLT of sfm_triangulate2; a point is good when Q.z Q.w > 0, X.z < dist and 0 < z2 < dist
 * (X = Q / Q.w, z2 its depth in the second camera) and its byte of mask_in is not zero; a point with a NaN or infinite
 * coordinate is never good.  The winner is the FIRST candidate with the largest count.  The order of the four
 * candidates follows the sign choices of this library's own decomposition, not cv2's: a tie may go to another
 * candidate than cv2's.
 *
 * seg_ptr [n_seg+1] device int64; pts1 / pts2 [n][2] float32 pixels; EorF [n_seg][9] float64 row-major: essential
 * matrices, or with is_fundamental != 0 fundamental matrices (E = K^T F K is formed on the device); Kseg [n_seg][4]
 * float64 (fx, fy, cx, cy).  Outputs: R [n_seg][9], t [n_seg][3], n_good [n_seg], status [n_seg] (0 ok, 1 empty
 * segment, 2 no model: E not finite or its second singular value not > 0; status 1 / 2 get R = t = 0, n_good = 0),
 * mask_out [n] (255 / 0: the winner's good points), X [n][3] (may be NULL): the winner's good points triangulated again
 * in PIXEL coordinates with K [I|0], K [R|t] - what initialize_reconstruction stores - and NaN elsewhere.  Debug
 * outputs, each may be NULL: cand_count [n_seg][4], cand_pose [n_seg][4][12] (row-major [R|t]; NaN without a model),
 * winner [n_seg].  Everything runs on the handle's stream without host synchronisation. */
int sfm_pose_workspace_bytes(int64_t n_points, int32_t n_seg, int64_t* bytes_host);
int sfm_pose_recover(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, const float* pts1, const float* pts2,
                     int64_t n, const double* EorF /* [n_seg][9] */, int32_t is_fundamental,
                     const double* Kseg /* [n_seg][4] */, const uint8_t* mask_in /* may be NULL */, double dist,
                     double* R, double* t, int32_t* n_good, int32_t* status, uint8_t* mask_out,
                     double* X /* [n][3], may be NULL */, int32_t* cand_count /* [n_seg][4], may be NULL */,
                     double* cand_pose /* [n_seg][4][12], may be NULL */, int32_t* winner /* may be NULL */,
                     void* workspace, int64_t workspace_bytes);

/* ------------------------------------------------------------- multi-view feature tracks from pairwise matches
 * One call joins the matches of all image pairs of a data set into tracks in CSR form.  A node is one keypoint of one
 * image: id = kp_ptr[image] + keypoint with kp_ptr [n_img+1] device int64 ascending from 0 to n_nodes < 2^31.  Segment s of
 * seg_ptr [n_seg+1] (device int64, ascending from 0 to n_edges) is the image pair pair_img[s] = (i, j) ([n_seg][2] int32);
 * edge e of segment s joins (i, query_idx[e]) and (j, train_idx[e]) (int32).  An edge whose byte of mask (may be NULL) is 0
 * is skipped.  An edge is counted in n_bad_edges, skipped and never followed when i == j, when an image is out of range,
 * when a keypoint index is outside its image's range, or when it lies in no segment.  Duplicate edges are harmless.
 *
 * A track is a connected component with at least min_len (>= 2) nodes.  A component that holds two nodes of one image is
 * conflicting: policy 0 (drop) removes it, policy 1 (keep) keeps it with track_conflict = 1.  Tracks are numbered by their
 * smallest node id and the observations of a track ascend by node id: the outputs do not depend on the order of the edges
 * or of the pairs, bit for bit.
 *
 * Outputs (device): track_ptr [cap_tracks+1] int64, obs_image / obs_kp [cap_obs] int32, track_conflict [cap_tracks] uint8,
 * node_track [n_nodes] int32 (track id; -1 unmatched keypoint; -2 component shorter than min_len; -3 dropped for a
 * conflict), counts [5] int64: n_tracks, n_obs, n_conflicting (components of at least min_len, whatever the policy),
 * n_bad_edges, status.  cap_tracks >= n_nodes / 2 and cap_obs >= n_nodes are required (SFM_ERR_ARG otherwise).  Without
 * nodes or without edges there are no tracks and every node_track entry is -1.  The kernels run on the handle's stream and
 * nothing is read back between them; the call then waits for the stream and reads the status word once: it is nonzero
 * only if the union loop exhausted its step budget, which the algorithm excludes, and gives SFM_ERR_NUMERIC. */
int sfm_tracks_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t* bytes_host);
int sfm_tracks_build(sfm_handle h, const int64_t* kp_ptr, int32_t n_img, int64_t n_nodes, const int64_t* seg_ptr,
                     int32_t n_seg, const int32_t* pair_img /* [n_seg][2] */, const int32_t* query_idx,
                     const int32_t* train_idx, const uint8_t* mask /* may be NULL */, int64_t n_edges, int32_t min_len,
                     int32_t policy, int64_t* track_ptr, int32_t* obs_image, int32_t* obs_kp, uint8_t* track_conflict,
                     int32_t* node_track, int64_t* counts, int64_t cap_tracks, int64_t cap_obs, void* workspace,
                     int64_t workspace_bytes);

/* ------------------------------------------------------------------- N-view triangulation of multi-view tracks
 * One call turns the tracks of sfm_tracks_build plus the registered cameras into 3-D points, one thread per track.
 * proj [n_cams][12] row-major 3 x 4 K[R|t]; cam_of_image [n_img] int32 gives the camera of an image position or -1 when
 * the image is not registered; kp_ptr [n_img+1] and kp_xy [n_nodes][2] (float64 pixels by node id = kp_ptr[image] +
 * keypoint) locate the pixels; track_ptr [n_tracks+1], obs_image / obs_kp [n_obs] are the CSR arrays as they are.  A used
 * observation is one whose image is registered (an image or camera index out of range counts as not registered; a
 * keypoint outside its image reads as a NaN pixel).  Per track, over its used observations in their order
 * (sfm_amd/csrc/triangulate_solve.h):
 *   linear stage: the rows x P[2] - P[0], y P[2] - P[1] are folded by Givens rotations into a 4 x 4 triangular factor
 *   whose null vector (the Jacobi iteration of sfm_triangulate2) is the homogeneous point; a track of exactly two used
 *   observations takes the DLT of sfm_triangulate2 itself and gives its bits.  Then exactly refine_iters Gauss-Newton steps
 *   on the sum of squared reprojection errors (3 x 3 Cholesky; the loop ends early only at a pivot that is not positive or
 *   a step that is not finite); the linear point is returned when the refined one costs more.
 * status [n_tracks], the first failing gate in this order: */
enum { SFM_TRI_OK = 0,
       SFM_TRI_TOO_FEW_VIEWS = 1,  /* fewer than min_views (>= 2) used observations */
       SFM_TRI_DEGENERATE = 2,     /* a non-finite input of a used observation, v[3] == 0, or a non-finite X */
       SFM_TRI_BEHIND = 3,         /* P[2].(X,1) <= 0 in some used view */
       SFM_TRI_LOW_ANGLE = 4,      /* min_angle_deg > 0 and no pair of used views has cos(d_i, d_j) <= cos(min_angle), d = X - C */
       SFM_TRI_HIGH_ERROR = 5,     /* some used view reprojects further than max_error px (`err > max_error`) */
       SFM_TRI_STATUS_COUNT = 6 };
/* X [n_tracks][3] and max_err [n_tracks] (the largest reprojection error of a used view) are NaN for status 1 and 2 and
 * written for every other status; n_views [n_tracks] is the number of used observations; counts [6] int64 tracks by
 * status.  The outputs of a track depend on its used observations in their order and on nothing else.  The workspace
 * holds the camera centres C = -M^-1 p4 (a prologue kernel, one thread per camera).  n_tracks == 0 only zeroes counts.
 * Everything runs on the handle's stream without host synchronisation. */
int sfm_triangulate_tracks_workspace_bytes(int32_t n_cams, int64_t* bytes_host);
int sfm_triangulate_tracks(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam_of_image, int32_t n_img,
                           const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes, const int64_t* track_ptr,
                           int64_t n_tracks, const int32_t* obs_image, const int32_t* obs_kp, int64_t n_obs,
                           int32_t min_views, int32_t refine_iters, double max_error, double min_angle_deg, double* X,
                           int32_t* status, int32_t* n_views, double* max_err, int64_t* counts /* [6] by status */,
                           void* workspace, int64_t workspace_bytes);

/* ------------------------------------------------------------------- the gates at points that are given
 * sfm_triangulate_tracks can only recompute a point; after a bundle adjustment the cameras and the points have moved and
 * the point to judge is the adjusted one.  Same arrays, same observation source and same camera-centre prologue (the
 * workspace is that of sfm_triangulate_tracks_workspace_bytes), one thread per track, X [n_tracks][3] and has_point
 * [n_tracks] uint8 given.  A track with has_point == 0 gets status SFM_EVAL_NO_POINT, its n_views is still counted, its
 * max_err is NaN and it is left out of counts.  Every other track is judged at X by the gates of sfm_triangulate_tracks in
 * their order (SFM_TRI_*; DEGENERATE: a non-finite input of a used observation or a non-finite X); max_err is NaN for
 * status 1 and 2, else the largest reprojection error of a used view.  obs_err [n_obs] (may be NULL): the reprojection
 * error of every observation at its track's X, NaN when the observation's image is not registered or the track has no
 * point.  counts [6] int64: the tracks that have a point, by status.  Fed the X of sfm_triangulate_tracks with the same
 * cameras and gates, a track of status 0, 3, 4 or 5 gets the same status, the same n_views and the same max_err bits.
 * Everything runs on the handle's stream without host synchronisation. */
enum { SFM_EVAL_NO_POINT = -1 };
int sfm_tracks_evaluate(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam_of_image, int32_t n_img,
                        const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes, const int64_t* track_ptr,
                        int64_t n_tracks, const int32_t* obs_image, const int32_t* obs_kp, int64_t n_obs,
                        const double* X, const uint8_t* has_point, int32_t min_views, double max_error,
                        double min_angle_deg, int32_t* status, int32_t* n_views, double* max_err,
                        double* obs_err /* [n_obs], may be NULL */, int64_t* counts /* [6] */,
                        void* workspace, int64_t workspace_bytes);

/* ------------------------------------------------------------------- robust triangulation: drop observations, not points
 * Tracks are connected components of pairwise matches, so one wrong match puts a foreign keypoint into a good track, and
 * sfm_triangulate_tracks then fails the whole track.  sfm_triangulate_tracks_robust takes the arguments of
 * sfm_triangulate_tracks and adds a per-observation inlier flag (sfm_amd/csrc/triangulate_robust.h).  For one track, with
 * its used observations in track order: an observation is sound when its pixel, P and C are finite; it agrees with a
 * point X when it is sound, its depth P[2].(X,1) > 0 and its reprojection error e <= max_error.
 *   Step 1: the rule of sfm_triangulate_tracks over all used observations.  Status 0 is returned as it is - X, max_err
 *   and n_views are the bits of sfm_triangulate_tracks - with obs_inlier = 1 for every used observation and n_inliers =
 *   n_views.  A failing track with fewer than 4 sound observations is returned as it is too, with obs_inlier = 0
 *   everywhere and n_inliers = 0: two or three views cannot tell which one is wrong, a pair always fits itself and a
 *   consensus needs a third, confirming view.
 *   Step 2: with s sound observations and M = s (s - 1) / 2 pairs (a, b), a < b, over them in lexicographic order,
 *   hypothesis h (0 <= h < min(M, H), H = SFM_TRI_ROBUST_PAIRS) uses pair number h when M <= H and pair number
 *   (h * M) / H in 64-bit integers otherwise.  Its point is the DLT of sfm_triangulate2 of the two observations.  It is
 *   void when v[3] == 0, the point is not finite, either depth is <= 0, or min_angle_deg > 0 and the two rays do not pass
 *   the angle gate.  Its score is the number of used observations that agree with its point.  The winner has the highest
 *   score; ties go to the lowest h.  When no hypothesis scores at least max(min_views, 3) the failing result of step 1
 *   is returned as above.
 *   Step 3: the rule of sfm_triangulate_tracks over the observations that agree with the winner's point, with min_views
 *   = max(min_views, 3) and the caller's refine_iters and gates.  A status other than 0 returns the failing result of
 *   step 1.  Otherwise status is 0, X is the refit point, obs_inlier [n_obs] uint8 is 1 exactly for the used observations
 *   that agree with X (a superset of the refit's own set), n_inliers counts them, max_err is their largest error and
 *   n_views stays the number of used observations.
 * obs_inlier is 0 for unused observations, for tracks without a point and for an observation that no track covers (the
 * call zeroes the array first).  counts [6] int64: tracks by status.  Two passes: one thread per track runs step 1 and
 * appends the failing tracks with at least 4 sound observations to a work list in the workspace (a wavefront ballot and
 * one integer atomic add per wavefront); then one wavefront per entry runs hypothesis h on lane h, takes the winner by an integer wave
 * reduction on (score, -lane) and refits once.  The second launch does not depend on the length of the list, nothing is
 * read back and the outputs do not depend on the order of the list: a track's outputs depend on its used observations
 * in their order and on nothing else.  Argument checks, return codes and n_tracks == 0 as sfm_triangulate_tracks.
 * The workspace holds, each rounded up to 256 bytes: the camera centres [n_cams][3] float64, the work list [n_tracks]
 * int32 (track indices in no particular order) and its length, one int32 - after the call the number of tracks that went
 * through the second pass, which a caller may read.
 *
 * sfm_tracks_classify is sfm_tracks_evaluate over the observations that agree with the given X: same arguments, the
 * workspace of sfm_triangulate_tracks_workspace_bytes, one thread per track.  A track with has_point == 0 gets
 * SFM_EVAL_NO_POINT, its n_views is still counted, n_inliers = 0, max_err NaN, and it is left out of counts.  Every other
 * track: n_views used observations, n_inliers of them agree with X, obs_inlier flags them, and status is
 * SFM_TRI_TOO_FEW_VIEWS (n_inliers < min_views; a non-finite X lands here; max_err NaN), SFM_TRI_LOW_ANGLE (no pair of
 * inliers passes the angle gate) or 0; max_err is the largest error of an inlier.  obs_err as sfm_tracks_evaluate.  Fed
 * the X of sfm_triangulate_tracks_robust with the same cameras and gates, a track of status 0 gets status 0, the same
 * flags, the same n_inliers and the same max_err bits.  obs_inlier is zeroed first here too.  Both calls run on the
 * handle's stream without host synchronisation. */
enum { SFM_TRI_ROBUST_PAIRS = 64 };
int sfm_triangulate_tracks_robust_workspace_bytes(int32_t n_cams, int64_t n_tracks, int64_t* bytes_host);
int sfm_triangulate_tracks_robust(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam_of_image,
                                  int32_t n_img, const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes,
                                  const int64_t* track_ptr, int64_t n_tracks, const int32_t* obs_image,
                                  const int32_t* obs_kp, int64_t n_obs, int32_t min_views, int32_t refine_iters,
                                  double max_error, double min_angle_deg, double* X, int32_t* status, int32_t* n_views,
                                  int32_t* n_inliers, double* max_err, uint8_t* obs_inlier /* [n_obs] */,
                                  int64_t* counts /* [6] by status */, void* workspace, int64_t workspace_bytes);
int sfm_tracks_classify(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam_of_image, int32_t n_img,
                        const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes, const int64_t* track_ptr,
                        int64_t n_tracks, const int32_t* obs_image, const int32_t* obs_kp, int64_t n_obs,
                        const double* X, const uint8_t* has_point, int32_t min_views, double max_error,
                        double min_angle_deg, int32_t* status, int32_t* n_views, int32_t* n_inliers, double* max_err,
                        uint8_t* obs_inlier /* [n_obs] */, double* obs_err /* [n_obs], may be NULL */,
                        int64_t* counts /* [6] */, void* workspace, int64_t workspace_bytes);

/* ------------------------------------------------------------------- 2D-3D correspondences of the unregistered images
 * What sfm_pnp_ransac consumes, taken from the tracks by index.  Node n of image i (kp_ptr[i] <= n < kp_ptr[i+1]) is
 * listed when cam_of_image[i] < 0, 0 <= node_track[n] < n_tracks and has_point[node_track[n]] != 0: integers only, so a
 * non-finite X or pixel is still listed (the PnP stage never counts such a point as an inlier).  A node that lies in no
 * image is not listed.  The listed nodes are written in ascending node id, so the lists of all images are contiguous
 * segments: seg_ptr[i] (device int64 [n_img+1]) is the number of listed nodes below kp_ptr[i] (segments of registered
 * images are empty) and *total (device int64) = seg_ptr[n_img].  For entry k < min(total, cap_corr): corr_node[k],
 * corr_track[k], corr_X[k] = X[track] (a bit copy), corr_uv[k] = (float)kp_xy[node] (round to nearest).  Nothing is
 * written at or beyond cap_corr; seg_ptr and total are always complete, so the caller can retry with a larger buffer.
 * seg_ptr, corr_X and corr_uv are the first arguments of sfm_pnp_ransac as they are.  Flag, exclusive scan and scatter
 * over the nodes in integers: the output bytes are a function of the inputs alone.  SFM_ERR_ARG for n_nodes >= 2^31, a
 * negative size, a NULL required pointer or a workspace that is too small; n_nodes == 0 writes seg_ptr = 0 and total = 0.
 * Everything runs on the handle's stream; nothing is read back and the stream is not synchronised. */
int sfm_resection_workspace_bytes(int64_t n_nodes, int64_t* bytes_host);
int sfm_tracks_resection(sfm_handle h, const int64_t* kp_ptr, int32_t n_img, int64_t n_nodes, const double* kp_xy,
                         const int32_t* node_track, const int32_t* cam_of_image, const double* X /* [n_tracks][3] */,
                         const uint8_t* has_point /* [n_tracks] */, int64_t n_tracks,
                         int64_t* seg_ptr /* [n_img+1] */, int32_t* corr_node, int32_t* corr_track,
                         double* corr_X /* [cap][3] */, float* corr_uv /* [cap][2] */, int64_t cap_corr,
                         int64_t* total, void* workspace, int64_t workspace_bytes);

/* ------------------------------------------------------------------- feature detection and description, batched
 * The detect_features step of the reference (find_matches.py:74-139: FAST with threshold 20, ORB descriptors, the
 * silhouette-mask filter) for all images of a data set in two calls with one read-back between them.  The detector is
 * FAST-9/16 to its published definition.  The descriptor is this library's own steered binary descriptor - OpenCV's
 * learned sampling table is not part of this project - specified here completely; every step is integer arithmetic.
 *
 * Input: n_img gray uint8 images, each with its own height and width, rows contiguous, all in one device buffer; image i
 * starts at img_off[i] and ends at or before img_off[i+1].  masks (may be NULL) has the same layout: a keypoint is kept
 * only where mask[y, x] > 0.  img_off [n_img+1] int64, heights / widths [n_img] int32 are HOST arrays (the calls size
 * their launches from them and check them before any device work).  An image with h < 2 edge + 1 or w < 2 edge + 1 has
 * no keypoints; no kernel reads outside an image.
 *
 * FAST-9/16: the circle is (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) (2,-2) (1,-3) (0,-3) (-1,-3) (-2,-2) (-3,-1) (-3,0)
 *   (-3,1) (-2,2) (-1,3) as (dx, dy); d_i = I(circle_i) - I(p); b = the maximum, over the 16 arcs of 9 contiguous circle
 *   pixels and both polarities, of the smallest +d_i (or the smallest -d_i) on the arc.  p is a corner iff b > threshold
 *   (1 <= threshold <= 254); its score is b - 1, the largest threshold at which it still passes (uint8); a non-corner
 *   and every pixel closer than 3 to the image border score 0.
 * Suppression: a corner is kept iff its score is strictly greater than the scores of all 8 neighbours (two equal adjacent
 *   maxima both go), taken from the whole image: a corner outside the gate or under the mask still suppresses its
 *   neighbour.  Then the gate edge <= x < w - edge, edge <= y < h - edge (edge >= 16), then the mask.
 * Selection: max_features = 0 keeps all.  An image with more than max_features survivors gets the cut score s with
 *   #(score > s) < max_features <= #(score >= s) from a 256-bin histogram; all above s stay, and of those equal to s the
 *   first max_features - #(score > s) in row-major order.  Nothing is sorted.
 * Order: the keypoints of an image are row-major (y ascending, then x); image i owns kp_ptr[i] .. kp_ptr[i+1].  The
 *   output bytes are the same from run to run and do not depend on the launch geometry or on the other images.
 * Orientation: m10 = sum dx I, m01 = sum dy I over the disc dx^2 + dy^2 <= 225 of the unblurred image (exact in int32);
 *   a = atan2((double)m01, (double)m10), 0 when both are 0; bin = ((int)floor(a * 15 / pi + 0.5) mod 30 + 30) mod 30;
 *   the angle is 12 bin degrees.
 * Blur: separable 7-tap, weights (18, 33, 49, 56, 49, 33, 18) (sum 256), borders reflect-101,
 *   B = (sum_y sum_x w_y w_x I + 32768) >> 16: exact in int32, rounded once.
 * Descriptor: rot [30][256][4] int8 holds (ax, ay, bx, by) per bin; bit k = B(p + a_k) < B(p + b_k) with the table of
 *   the keypoint's bin, stored in byte k / 8 at bit position k % 8: 32 bytes in the layout of cv2.ORB.
 * Pattern (host only): sfm_orb_default_pattern writes this library's base table - 256 pairs from a splitmix64 stream
 *   with a fixed seed, coordinates centre-weighted, every endpoint within x^2 + y^2 <= 169, no pair with two equal
 *   endpoints, no pair twice.  sfm_orb_rotate_pattern turns a base table by 12 bin degrees: x' = round(x cos - y sin),
 *   y' = round(x sin + y cos) in double, rounding half away from zero; bin 0 is the identity and bins 15 .. 29 are the
 *   exact negatives of bins 0 .. 14.  A base table with an endpoint outside radius 13 is refused (SFM_ERR_ARG): with it
 *   every rotated sample plus the 3-pixel blur support stays within 16 pixels of the keypoint, hence edge >= 16.
 *
 * sfm_features_detect: score map, suppression with gate and mask, histogram and cut, keypoints per row and their scan;
 *   writes kp_ptr (device int64 [n_img+1]) on the handle's stream; nothing is read back.  The caller reads kp_ptr and
 *   sizes the outputs exactly: n_kp = kp_ptr[n_img].
 * sfm_features_describe: the ordered scatter (xy int32 [n_kp][2] as (x, y), score uint8), the blur, the moments
 *   (angle_bin uint8) and the descriptor (desc uint8 [n_kp][32]), with the SAME images, sizes and workspace, untouched
 *   since detect.  blurred_out (may be NULL) receives the blurred images in the layout of `images`.  n_kp == 0 with
 *   blurred_out == NULL returns at once.
 * The workspace holds the image table, one uint8 map of the scores after suppression, one uint8 map that is the raw score
 * during detect and the blurred image during describe, three int32 per row of an image at least 33 wide, the histograms
 * and the cuts; its size depends on img_off alone.  SFM_ERR_ARG before any device work for a null handle, an argument
 * out of range, an img_off that does not ascend, an image larger than its slot or a workspace that is too small. */
int sfm_orb_default_pattern(int8_t base[256][4]);
int sfm_orb_rotate_pattern(const int8_t base[256][4], int8_t rot[30][256][4]);
int sfm_features_workspace_bytes(int32_t n_img, const int64_t* img_off_host, int64_t* bytes_host);
int sfm_features_detect(sfm_handle h, const uint8_t* images, const uint8_t* masks /* may be NULL */,
                        const int64_t* img_off /* host */, const int32_t* heights /* host */,
                        const int32_t* widths /* host */, int32_t n_img, int32_t threshold, int32_t edge,
                        int32_t max_features, int64_t* kp_ptr /* device int64 [n_img+1] */, void* workspace,
                        int64_t workspace_bytes);
int sfm_features_describe(sfm_handle h, const uint8_t* images, const int64_t* img_off /* host */,
                          const int32_t* heights /* host */, const int32_t* widths /* host */, int32_t n_img,
                          const int64_t* kp_ptr /* device */, int64_t n_kp, const int8_t* rot_pattern /* device */,
                          int32_t* xy /* int32 [n_kp][2] */, uint8_t* score, uint8_t* angle_bin,
                          uint8_t* desc /* uint8 [n_kp][32] */, uint8_t* blurred_out /* may be NULL */, void* workspace,
                          int64_t workspace_bytes);

/* ---- multi-scale features: an image pyramid in front of detect and describe (sfm_amd/csrc/features_pyramid.hip,
 * features_pyramid_plan.h) ----
 * The two calls above take a batch of images of different sizes, so a pyramid is such a batch with n_img * n_levels
 * entries, and they run on it unchanged.  The calls here build that batch and join the keypoints of an image's levels
 * into one list in level-0 coordinates under one max_features budget.  Every byte is integer arithmetic (the coordinate
 * map is one double division, rounded once); the outputs are the same from run to run and do not depend on the launch
 * geometry or on the other images of the batch.
 *
 * Scale and levels: the scale is a rational num / den with den < num <= 2 den, num <= 16 and 8 num >= 9 den (default
 *   6/5); 2 <= n_levels <= 16.
 * Level sizes, chained, heights and widths alike: n_l = max(1, (2 n_{l-1} den + num) / (2 num)) in integer division (the
 *   half-up rounding of n_{l-1} den / num); a side of 0 stays 0.  n_l <= n_{l-1} always, and a side of at least 33
 *   strictly shrinks; a small side may repeat - such an image is not eligible for keypoints anyway.
 * Level batch: image-major; slot i * n_levels + l holds level l of image i in exactly h_l * w_l bytes, the slots back to
 *   back from offset 0 (lvl_off ascends).  Level 0 is a copy of the image; its mask a copy of the mask.
 * Resampling level l from level l - 1: for the destination pixel x of a row of wd pixels over a source row of ws, in int64
 *   ux = (2x + 1) ws - wd,  x0 = ux / (2 wd),  fx = ((ux % (2 wd)) * 256) / (2 wd),  x1 = min(x0 + 1, ws - 1); the same in
 *   y.  The value is ((256-fx)(256-fy) I[y0,x0] + fx (256-fy) I[y0,x1] + (256-fx) fy I[y1,x0] + fx fy I[y1,x1] + 32768)
 *   >> 16: pixel-centre aligned, 8-bit weights, exact in int32, rounded once.
 * Masks: the mask of a level is 1 exactly where all four of those source mask pixels are > 0, else 0 - whatever their
 *   weights.  Conservative: a keypoint of a coarse level never sits on a pixel that drew on a masked one.
 * Each level is detected and described by the rule above, with the call's threshold, edge and pattern.
 * Joining: the keypoints of image i are those of its levels in (level ascending, row-major) order - the segment
 *   lvl_kp_ptr[i n_levels] .. lvl_kp_ptr[(i + 1) n_levels] of the level batch's list.  With max_features = M > 0 and more
 *   than M of them the cut is the one above, over the union: the score s with #(score > s) < M <= #(score >= s) from a
 *   256-bin histogram; all above s stay, of those equal to s the first M - #(score > s) in that order.  Nothing is
 *   sorted; the survivors keep their order.  The level batch may be detected with the same M per level first: a keypoint
 *   in the union's top M is in its level's top M, and both tie rules take prefixes of the same order, so the result is
 *   the same.
 * Outputs per kept keypoint: xy float32 in level-0 pixels, X = ((double)(2x + 1) * (double)w0) / (double)(2 w_l) - 0.5 and
 *   Y likewise with the heights, without FMA contraction, rounded once to float32 - exactly (x, y) at level 0; level
 *   uint8; score, angle_bin and desc copied; src int32, its index in the level batch's keypoint list.
 * Limits: a keypoint of level l is located to about (num/den)^l / 2 pixels of level 0; one global score cut, not a quota
 *   per level; the levels are chained bilinear resamplings, not area averages, and each is blurred by the fixed 7-tap rule.
 *
 * sfm_features_pyramid_sizes (host only): the tables of the level batch - lvl_off int64 [n_img n_levels + 1], lvl_heights
 *   / lvl_widths int32 [n_img n_levels] - which go straight into sfm_features_workspace_bytes / _detect / _describe with
 *   n_img n_levels images.  SFM_ERR_ARG for an option out of range, a negative size or more than 2^32 pixels.
 * sfm_features_pyramid: builds the level batch into lvl_images (and lvl_masks; NULL iff masks is NULL) on the handle's
 *   stream: one launch copies level 0, then one launch per level (and one more for the masks) resamples level l from
 *   level l - 1.  img_off / heights / widths are HOST arrays as above.  No kernel reads outside an image or writes outside
 *   a level's slot.  The workspace holds the tile table.
 * sfm_features_merge_count: from lvl_kp_ptr (device, what detect wrote for the level batch) and lvl_score (what describe
 *   wrote), writes kp_ptr (device int64 [n_img+1]) on the stream.  The caller reads kp_ptr[n_img] back - one more
 *   read-back, as between detect and describe.
 * sfm_features_merge_gather: with the same workspace, untouched since merge_count, writes xy float32 [n_kp][2], level,
 *   score, angle_bin, desc [n_kp][32] (4-byte aligned) and src; nothing at or beyond n_kp.  lvl_heights / lvl_widths are
 *   the HOST tables of sfm_features_pyramid_sizes.
 * SFM_ERR_ARG before any device work, with the rule's text in sfm_last_error, for a null handle, an option out of range,
 * a null pointer, masks without lvl_masks or the reverse, or a workspace that is too small. */
int sfm_features_pyramid_sizes(int32_t n_img, const int32_t* heights, const int32_t* widths, int32_t n_levels, int32_t num,
                               int32_t den, int64_t* lvl_off /* [n_img n_levels + 1] */, int32_t* lvl_heights,
                               int32_t* lvl_widths);
int sfm_features_pyramid_workspace_bytes(int32_t n_img, int32_t n_levels, int64_t* bytes_host);
int sfm_features_pyramid(sfm_handle h, const uint8_t* images, const uint8_t* masks /* may be NULL */,
                         const int64_t* img_off /* host */, const int32_t* heights /* host */,
                         const int32_t* widths /* host */, int32_t n_img, int32_t n_levels, int32_t num, int32_t den,
                         uint8_t* lvl_images, uint8_t* lvl_masks /* NULL iff masks is */, void* workspace,
                         int64_t workspace_bytes);
int sfm_features_merge_workspace_bytes(int32_t n_img, int32_t n_levels, int64_t* bytes_host);
int sfm_features_merge_count(sfm_handle h, const int64_t* lvl_kp_ptr /* device [n_img n_levels + 1] */,
                             const uint8_t* lvl_score, int32_t n_img, int32_t n_levels, int32_t max_features,
                             int64_t* kp_ptr /* device int64 [n_img+1] */, void* workspace, int64_t workspace_bytes);
int sfm_features_merge_gather(sfm_handle h, const int64_t* lvl_kp_ptr, const int32_t* lvl_xy, const uint8_t* lvl_score,
                              const uint8_t* lvl_angle_bin, const uint8_t* lvl_desc, const int32_t* lvl_heights /* host */,
                              const int32_t* lvl_widths /* host */, int32_t n_img, int32_t n_levels,
                              const int64_t* kp_ptr /* device */, int64_t n_kp, float* xy /* float32 [n_kp][2] */,
                              uint8_t* level, uint8_t* score, uint8_t* angle_bin, uint8_t* desc /* uint8 [n_kp][32] */,
                              int32_t* src, void* workspace, int64_t workspace_bytes);

/* ---- dense depth maps by plane-sweep stereo (sfm_amd/csrc/depth.hip, depth_rule.h, depth_plan.h) ----
 * From n_img gray uint8 images in the layout of sfm_features_detect (one device buffer, img_off [n_img+1] int64, heights /
 * widths [n_img] int32 as HOST arrays), registered cameras and a list of plane depths per reference view: per reference
 * pixel the plane with the lowest aggregated census cost, that cost, a depth refined between planes, and after a
 * cross-view check a keep flag and the 3-D point.  Fronto-parallel planes of the reference camera only.  All floating
 * point is float64 without FMA contraction; everything else is integer: the output bytes are a function of the inputs
 * alone, the same from run to run, and independent of the launch geometry and of the other views of the batch.
 *
 * Views: n_ref reference views, ref_image [n_ref] (each image at most once); view r has the sources
 *   src_image[src_ptr[r] .. src_ptr[r+1]) (at most 8, none equal to ref_image[r]; ref_image, src_ptr, src_image are HOST
 *   arrays) and the plane depths plane_depth[plane_ptr[r] .. plane_ptr[r+1]) (plane_ptr a HOST array, plane_depth float64 on
 *   the device; 1 .. 1024 planes, every depth finite and > 0).  Entry e of src_image has the warp warps[e] = [A | b], 12
 *   float64 row-major 3 x 4 on the device; the caller forms A = K_s R_s R_r^T K_r^-1, b = K_s (t_s - R_s R_r^T t_r), so
 *   that with the last row of K_s = (0, 0, 1) q2 below is the depth along the source's optical axis.  The maps of view r
 *   are the elements out_off[r] .. out_off[r] + h w (row-major) of every output, out_off[r] = sum over r' < r of h w.
 * Census: cen(p) is 48 bits in a uint64; for the offsets (dy, dx), dy, dx in -3 .. 3 in row-major order with the centre
 *   skipped, bit k = I(clamp(p + o_k)) < I(p), coordinates clamped to the image.  census has img_off[n_img] elements, the
 *   word of pixel (x, y) of image i at img_off[i] + y w + x; elements of a slot behind h w are not written.
 * Sample: for the reference pixel (x, y), a depth d and a source of w_s x h_s pixels with warp [A | b]:
 *   a_i = (A_i0 * x + A_i1 * y) + A_i2,  q_i = d * a_i + b_i,  u = q0 / q2,  v = q1 / q2;  valid iff q2 > 0 and
 *   u >= -0.5 and u < w_s - 0.5 and v >= -0.5 and v < h_s - 0.5, each comparison false on NaN;  xi = (int)floor(u + 0.5),
 *   yi likewise (never above w_s - 1, h_s - 1: the rounded sum can reach the size only for a size of 1, and is then cut).
 *   c = popcount(cen_r(p) ^ cen_s(yi, xi)); an invalid sample costs 24, what two unrelated census words are expected to give.
 * Aggregate: c_k(p) = sum of c over the sources at plane k;  S_k(p) = sum of c_k(clamp(p + o)) over the (2 radius + 1)^2
 *   window, 0 <= radius <= 4, coordinates clamped to the reference image.  S <= 48 * 8 * 81 = 31,104.
 * Winner: best = the lowest k that minimises S_k.  plane (int32) = best, cost (uint16) = S_best, depth (float32): with D
 *   planes, if 0 < best < D - 1 and den = S_{best-1} - 2 S_best + S_{best+1} > 0 (integers), off = (double)(S_{best-1} -
 *   S_{best+1}) / (double)(2 * den), j = best + 1 if off >= 0 else best - 1, f = fabs(off),
 *   w = 1 / d_best + f * (1 / d_j - 1 / d_best), depth = (float)(1 / w); otherwise depth = (float)d_best.  A view without a
 *   source still gets its maps: S_k = 0, best = 0.
 * Filter: for a reference pixel whose depth is finite, d = that float32 widened to double goes through the sample rule
 *   against every source that has a depth map of its own (it is itself a reference view of the call); the pixel agrees
 *   with the source iff the sample is valid, ds = depth_s(yi, xi) is finite and fabs(ds - q2) <= rel_tol * q2.
 *   n_consistent (uint8) counts the agreeing sources; keep (uint8) = 1 iff cost <= max_cost[r] (a HOST int32 [n_ref], NULL:
 *   no limit) and n_consistent >= min_consistent.  xyz (float64 x 3) for every pixel: with backproj[r] = [M | c], 12 float64
 *   row-major 3 x 4 on the device, M = R_r^T K_r^-1, c = -R_r^T t_r: xyz_i = d * ((M_i0 * x + M_i1 * y) + M_i2) + c_i.
 *   A pixel whose depth is not finite has n_consistent = 0, keep = 0 and xyz = NaN.
 * The workspace (sfm_depth_workspace_bytes; n_entries = src_ptr[n_ref]) holds the tables of a call only; one workspace
 * sized for the sweep serves the census and the filter of the same images too.  SFM_ERR_ARG before any device work for a
 * null handle, an img_off that does not ascend, an image larger than its slot, a reference or source index out of range, a
 * reference listed twice, a source equal to its reference, more than 8 sources, a radius above 4, fewer than 1 or more than
 * 1024 planes, or a workspace that is missing or too small.  No kernel reads outside an image. */
int sfm_depth_workspace_bytes(int32_t n_img, int32_t n_ref, int64_t n_entries, int64_t* bytes_host);
int sfm_depth_census(sfm_handle h, const uint8_t* images, const int64_t* img_off /* host */, const int32_t* heights /* host */,
                     const int32_t* widths /* host */, int32_t n_img, uint64_t* census /* device [img_off[n_img]] */,
                     void* workspace, int64_t workspace_bytes);
int sfm_depth_sweep(sfm_handle h, const uint64_t* census, const int64_t* img_off /* host */, const int32_t* heights /* host */,
                    const int32_t* widths /* host */, int32_t n_img, int32_t n_ref, const int32_t* ref_image /* host */,
                    const int64_t* src_ptr /* host [n_ref+1] */, const int32_t* src_image /* host */,
                    const double* warps /* device [n_entries][12] */, const int64_t* plane_ptr /* host [n_ref+1] */,
                    const double* plane_depth /* device */, int32_t radius, int32_t* plane, uint16_t* cost, float* depth,
                    void* workspace, int64_t workspace_bytes);
int sfm_depth_filter(sfm_handle h, const int64_t* img_off /* host */, const int32_t* heights /* host */,
                     const int32_t* widths /* host */, int32_t n_img, int32_t n_ref, const int32_t* ref_image /* host */,
                     const int64_t* src_ptr /* host [n_ref+1] */, const int32_t* src_image /* host */,
                     const double* warps /* device [n_entries][12] */, const double* backproj /* device [n_ref][12] */,
                     const float* depth, const uint16_t* cost, const int32_t* max_cost /* host [n_ref] or NULL */,
                     double rel_tol, int32_t min_consistent, uint8_t* n_consistent, uint8_t* keep,
                     double* xyz /* device [n_out][3] */, void* workspace, int64_t workspace_bytes);

/* ---- fusion of the depth maps into one cloud with normals (sfm_amd/csrc/depth_fuse.hip, depth_rule.h, depth_plan.h) ----
 * From the inputs of sfm_depth_filter and its outputs depth, keep and xyz (on the device): every surface point once, as
 * the mean of the views that agree on it, with a normal.  A pure function of those arrays: no visit order, no atomics on
 * memory, no randomness.  All floating point is float64 without FMA contraction, everything else is integer, so the
 * output bytes are the same from run to run.  Parameters: rel_tol >= 0, normal_step t in 1 .. 4, normal_jump j >= 0.
 * "Position" of a view is its index in ref_image.  X(x, y) is the xyz of a pixel, d its float32 depth widened to double.
 *
 * 1. Normal map per view (normal_map, float32 [n_out][3]; keep plays no part).  With the neighbours at clamp(x +- t) and
 *    clamp(y +- t), coordinates clamped to the view's image:  a = X(x+t, y) - X(x-t, y),  b = X(x, y+t) - X(x, y-t),
 *    n = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0),  l2 = (n0*n0 + n1*n1) + n2*n2.  The normal is valid iff the centre
 *    depth d is finite, each of the four neighbour depths dn is finite with fabs(dn - d) <= j * d, and l2 is finite and
 *    > 0.  Then n_i = n_i / sqrt(l2), and n is negated when ((n0*c0 + n1*c1) + n2*c2) < 0 with c = C - X, C the view's
 *    centre (elements 3, 7, 11 of backproj[r]).  Rounded to float32; an invalid normal is (0, 0, 0).  An image one pixel
 *    wide or high has no valid normal (a or b is zero).
 * 2. Partners.  For a pixel p of view v with keep = 1, entry s (0 .. 7) of the view's sources agrees iff the source has
 *    maps of its own, the sample rule at the pixel's depth d is valid, ds = the source's depth at (yi, xi) is finite,
 *    fabs(ds - q2) <= rel_tol * q2, and keep of that source pixel is 1.  agree_mask (uint8 [n_out]) has bit s set for
 *    each agreeing entry and is 0 where keep = 0;  n_views = 1 + popcount(agree_mask).
 * 3. Owner (uint8 [n_out]) = keep and no agreeing partner lies in a view of lower position.  A pixel is dropped only in
 *    favour of a kept pixel of an earlier view: by induction over the positions every kept pixel is an owner or reaches
 *    one through a chain of agreeing partners, and view 0 loses nothing.
 * 4. Fused point and normal, owners only.  acc = X(p); for the agreeing entries in entry order acc_i = acc_i + X_s_i with
 *    X_s the xyz of the partner pixel; point_i = acc_i / (double)n_views.  The normal is the same sum over the float32
 *    normals of the normal maps widened to double, the pixel's own first, invalid ones adding zero; l2 as above; when l2
 *    is finite and > 0 each sum is divided by sqrt(l2), otherwise the normal is (0, 0, 0); rounded to float32.
 * 5. Output order: the owners in (view position, row-major) order.  points float64 [m][3], normals float32 [m][3],
 *    n_views uint8 [m], index int32 [m][3] as (view position, y, x); pt_ptr int64 [n_ref+1] on the device, the owners of
 *    view v are the points pt_ptr[v] .. pt_ptr[v+1], m = pt_ptr[n_ref].
 * Limits.  Agreement is not transitive: several pixels of a close view can fall on one pixel of a farther, earlier view
 *    and are all dropped, so the earlier view's resolution wins.  No forward-backward check is added: the partner need
 *    not project back onto p.  Sources without maps of their own never count.
 * Two calls.  sfm_depth_fuse_mark writes normal_map, agree_mask, owner and pt_ptr and leaves the first output slot of
 *    every block of 256 pixels in the workspace; the caller reads pt_ptr[n_ref] (after a synchronisation of the stream),
 *    allocates the outputs and hands the same workspace, untouched, with the same views to sfm_depth_fuse_gather, which
 *    returns at once for n_points == 0.  n_points is the capacity of the outputs: a value between 0 and the number of
 *    pixels cannot be checked against the device's count on the host and is NOT checked; the gather writes no slot at or
 *    above it, nor outside pt_ptr's range of the pixel's view, so a wrong value loses points but writes nothing outside.
 * The workspace (sfm_depth_fuse_workspace_bytes; n_out = the pixels of all views) is larger than that of
 *    sfm_depth_workspace_bytes and may be the same buffer.  SFM_ERR_ARG before any device work for what
 *    sfm_depth_filter refuses, a normal_step outside 1 .. 4, a negative or NaN normal_jump or rel_tol, a negative n_points
 *    or one above the number of pixels.  No kernel reads outside a map. */
int sfm_depth_fuse_workspace_bytes(int32_t n_img, int32_t n_ref, int64_t n_entries, int64_t n_out, int64_t* bytes_host);
int sfm_depth_fuse_mark(sfm_handle h, const int64_t* img_off /* host */, const int32_t* heights /* host */,
                        const int32_t* widths /* host */, int32_t n_img, int32_t n_ref, const int32_t* ref_image /* host */,
                        const int64_t* src_ptr /* host [n_ref+1] */, const int32_t* src_image /* host */,
                        const double* warps /* device [n_entries][12] */, const double* backproj /* device [n_ref][12] */,
                        const float* depth, const uint8_t* keep, const double* xyz, double rel_tol, int32_t normal_step,
                        double normal_jump, float* normal_map /* device [n_out][3] */, uint8_t* agree_mask, uint8_t* owner,
                        int64_t* pt_ptr /* device [n_ref+1] */, void* workspace, int64_t workspace_bytes);
int sfm_depth_fuse_gather(sfm_handle h, const int64_t* img_off /* host */, const int32_t* heights /* host */,
                          const int32_t* widths /* host */, int32_t n_img, int32_t n_ref, const int32_t* ref_image /* host */,
                          const int64_t* src_ptr /* host [n_ref+1] */, const int32_t* src_image /* host */,
                          const double* warps /* device [n_entries][12] */, const float* depth, const double* xyz,
                          const float* normal_map, const uint8_t* agree_mask, const uint8_t* owner,
                          const int64_t* pt_ptr /* device [n_ref+1] */, int64_t n_points, double* points /* [n_points][3] */,
                          float* normals /* [n_points][3] */, uint8_t* n_views, int32_t* index /* [n_points][3] */,
                          void* workspace, int64_t workspace_bytes);

/* ---- a surface from the depth maps: TSDF volume and marching tetrahedra (sfm_amd/csrc/tsdf.hip, mesh.hip, tsdf_rule.h,
 *      mesh_rule.h, mesh_plan.h) ----
 * Two stages, each a pure function of its inputs: float64 without FMA contraction, everything else integer, no visit
 * order, no atomics on memory, so the output bytes are the same from run to run.
 * Grid: nx x ny x nz NODES, each dimension 2 .. 1024; node (i, j, k) has the index n = (k ny + j) nx + i and the position
 *   X_a = origin_a + voxel * (double)index_a, origin (3 float64, HOST) finite, voxel finite and > 0.  tsdf is float32
 *   [n_nodes], weight uint16 [n_nodes], both on the device.
 *
 * sfm_tsdf_integrate.  The depth maps in the layout of sfm_depth_filter: heights / widths per image and ref_image per view
 *   (HOST), view r at out_off[r] = sum over r' < r of h w in depth (float32) and keep (uint8, or NULL: every finite depth
 *   counts).  proj (device, float64 [n_ref][12]) is the row-major [P | p] of a view, P = K R, p = K t; with the last row of
 *   K = (0, 0, 1) q2 below is the depth along the optical axis.  For the node X and the views in position order:
 *   q_i = ((P_i0 * X0 + P_i1 * X1) + P_i2 * X2) + p_i,  u = q0 / q2,  v = q1 / q2;  validity and the nearest pixel (xi, yi)
 *   are those of the sample rule above (q2 > 0, the half-open bounds, floor(u + 0.5) with the cut);  ds = the float32 depth
 *   at (yi, xi) widened.  The view is skipped unless the projection is valid, ds is finite and keep != 0;  sdf = ds - q2,
 *   and the view is skipped if sdf < -trunc;  otherwise acc = acc + (sdf < trunc ? sdf : trunc) / trunc and w = w + 1.
 *   After all views weight = w and tsdf = (float)(acc / (double)w); for w = 0 tsdf has the bit pattern 0x7FC00000.
 *   Every view weighs the same.  A pixel without a depth carries no evidence, so free space outside every silhouette stays
 *   unknown (w = 0).  The workspace (sfm_tsdf_workspace_bytes) holds the view table.  SFM_ERR_ARG before any device work
 *   for a null handle, a negative image size, a reference index out of range, a reference listed twice, n_ref > n_img or
 *   > 65,535, a dimension out of range, a non-finite origin or voxel, voxel <= 0, trunc not > 0, a null pointer, or a
 *   workspace that is missing or too small.  No kernel reads outside a map.
 *
 * sfm_mesh_mark / sfm_mesh_emit.  Marching tetrahedra over the Kuhn split of every cell.
 *   Known, inside, active: a node is known iff weight >= min_weight and tsdf is finite, and inside iff tsdf < 0.  Cell
 *   (i, j, k), each index below its dimension - 1, is active iff its 8 corners are known; its index is that of its node.
 *   Split: every cell has 6 tetrahedra, numbered by the permutations of the axes in lexicographic order xyz, xzy, yxz, yzx,
 *   zxy, zyx; the tetrahedron of (a, b, c) has the local nodes v0 = (0,0,0), v1 = v0 + e_a, v2 = v1 + e_b, v3 = (1,1,1).
 *   Every edge of every tetrahedron runs from a node in one of the directions 0 .. 6 = (1,0,0), (0,1,0), (0,0,1), (1,1,0),
 *   (1,0,1), (0,1,1), (1,1,1) and is owned by that node.  The split is the same in every cell: faces match.
 *   Vertices: direction d of node N carries a vertex iff B = N + d is in the grid, N and B differ in "inside", and at least
 *   one active cell contains the edge (the cells N - (a, b, c), each component 0 where that of d is 1 and 0 or 1 otherwise).
 *   Vertices come in (node index, direction) order.  With fa, fb the values at N and B widened, t = fa / (fa - fb) and
 *   V_a = XA_a + t * (XB_a - XA_a), float64.  Normal: per node and axis the gradient is 0.5 * (f(+) - f(-)) when both
 *   neighbours are in the grid and known, else f(+) - f or f - f(-) with the usable one, else 0;  g_a = gA_a + t * (gB_a -
 *   gA_a), l2 = (g0*g0 + g1*g1) + g2*g2; when l2 is finite and > 0 each g_a is divided by sqrt(l2), otherwise the normal
 *   is (0, 0, 0); rounded to float32.  It points to the outside.
 *   Triangles: in (cell index, tetrahedron number) order, active cells only.  Name an edge by its two local nodes.  One
 *   node p on one side and a < b < c on the other (either way round): (pa, pb, pc).  Inside p < q and outside r < s:
 *   (pr, ps, qs), then (pr, qs, qr).  Orientation: with m(e) the sum of the two local node offsets of edge e,
 *   n = (m1 - m0) x (m2 - m0) and D = |I| * sum(outside offsets) - |O| * sum(inside offsets), all integers and n . D never
 *   0, the second and third vertex are exchanged iff n . D < 0: the normal of a triangle points from inside to outside.
 *   Zero-area triangles (a node that holds exactly 0) are kept.  mesh_rule.h has the 6 x 16 cases as a table.
 *   Limits: no hole filling; about 2.3 x the triangles of marching cubes.  Colour comes afterwards: one per vertex from
 *   sfm_mesh_colors, a texture atlas from sfm_mesh_texture, both below.
 * Two calls.  sfm_mesh_mark writes counts (device int64 [2]: vertices, triangles) and leaves in the workspace
 *    (sfm_mesh_workspace_bytes) per node its flags and one record - the 7-bit vertex mask, the node's first vertex slot and
 *    the cell's first triangle slot relative to its block of 256 nodes, the cell's activity - and the first slots of every
 *    block through a two-level scan.  The caller reads counts (after a synchronisation of the stream), allocates and hands
 *    the same workspace, untouched, with the same grid to sfm_mesh_emit, which writes vertices float64 [nv][3], normals
 *    float32 [nv][3] and triangles int32 [nt][3]; a triangle finds a vertex as the slot of the owning node plus the
 *    popcount of the mask below the direction.  n_vertices / n_triangles are the capacities of the outputs: emit writes
 *    nothing at or above them and returns at once when both are 0.  SFM_ERR_ARG before any device work for a null handle,
 *    a dimension out of range, a negative min_weight, a non-finite origin or voxel, voxel <= 0, a capacity below 0 or above
 *    2^31 - 1, a null pointer, or a workspace that is missing or too small. */
int sfm_tsdf_workspace_bytes(int32_t n_ref, int64_t* bytes_host);
int sfm_tsdf_integrate(sfm_handle h, const int32_t* heights /* host */, const int32_t* widths /* host */, int32_t n_img,
                       int32_t n_ref, const int32_t* ref_image /* host */, const double* proj /* device [n_ref][12] */,
                       const float* depth, const uint8_t* keep /* or NULL */, const double* origin /* host [3] */,
                       double voxel, int32_t nx, int32_t ny, int32_t nz, double trunc, float* tsdf, uint16_t* weight,
                       void* workspace, int64_t workspace_bytes);
int sfm_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t* bytes_host);
int sfm_mesh_mark(sfm_handle h, const float* tsdf, const uint16_t* weight, int32_t nx, int32_t ny, int32_t nz,
                  int32_t min_weight, int64_t* counts /* device [2] */, void* workspace, int64_t workspace_bytes);
int sfm_mesh_emit(sfm_handle h, const float* tsdf, int32_t nx, int32_t ny, int32_t nz, const double* origin /* host [3] */,
                  double voxel, int64_t n_vertices, int64_t n_triangles, double* vertices, float* normals,
                  int32_t* triangles, void* workspace, int64_t workspace_bytes);

/* ---- connected components of a mesh and the removal of the small ones (sfm_amd/csrc/mesh_clean.hip, mesh_clean_rule.h,
 *      mesh_clean_plan.h) ----
 * Integers only: every output byte is a function of the inputs, the same from run to run, and NumPy / SciPy reproduce it
 * (tests/mesh_clean_reference.py).  Nothing depends on the order of the triangles, of the indices within a triangle, or of
 * the lanes.
 *
 * Input.  n_vertices, 0 .. 2^31 - 1, and triangles int32 [n_triangles][3] with n_triangles 0 .. 2^31 - 1.
 * Sound triangles.  A triangle is sound iff its three indices lie in [0, n_vertices).  An unsound triangle joins nothing:
 *   its component is -1, it is counted in counts[1], it is never kept, and no kernel uses its indices as addresses.  A
 *   repeated index inside a triangle is allowed, and a zero-area triangle is a triangle like any other.
 * Components.  The vertices are the nodes and every sound triangle joins its three vertices.  A vertex in no sound triangle
 *   is a component of its own with 0 triangles.  Components are numbered in ascending order of their smallest vertex index,
 *   comp_root.  sfm_mesh_components writes vertex_component int32 [n_vertices], triangle_component int32 [n_triangles] (the
 *   component of its vertices, -1 when unsound), the first n_components entries of comp_root, comp_vertices and
 *   comp_triangles (int32; the caller provides n_vertices entries of each; comp_triangles counts sound triangles), and
 *   counts, device int64 [3]: components, unsound triangles, status.  Status is 0; it is 1 when a walk towards a root ran
 *   out of its step budget (4 n_vertices + 1024 steps, which no input reaches), and the call then returns SFM_ERR_NUMERIC
 *   instead of spinning.  The call reads the status behind its last launch, so it returns with the stream synchronised.
 * Selection.  min_triangles >= 0 and keep_largest >= 0, where 0 means no limit.  Component c is a candidate iff
 *   comp_triangles[c] >= min_triangles.  With keep_largest = k > 0 and more than k candidates the cut of the feature
 *   selection applies to the candidates' triangle counts: the size s with #(size > s) < k <= #(size >= s); all candidates
 *   above s are kept, and of those at s the first k - #(size > s) in component order.  Nothing is sorted.  Otherwise every
 *   candidate is kept.  The result is comp_keep, uint8 [n_components], 1 = kept.  mesh_clean_rule.h holds this rule in plain
 *   C++ for host and device: four passes of 8-bit histograms over the sizes, most significant byte first, then the ties.
 * Compaction.  A vertex is kept iff its component is kept; a triangle is kept iff it is sound and its component is kept.
 *   Kept vertices and kept triangles stay in their old order.  vertex_map int32 [nv'] is the old index of each new vertex,
 *   ascending, triangle_map int32 [nt'] likewise; the new triangles int32 [nt'][3] hold, for every index, the rank of its
 *   vertex among the kept ones; vertices (float64 x 3) and normals (float32 x 3) are copied bit for bit.  A mesh of which
 *   everything is kept comes out byte for byte as it went in.
 * Limits: no threshold as a fraction of the largest component, no components by area or bounding box, no removal of
 *   zero-area triangles or non-manifold edges, no hole filling, decimation by clustering only: see Decimation.
 *
 * Calls, in the shape of sfm_mesh_mark / sfm_mesh_emit: the host reads a count between them and allocates.
 * sfm_mesh_components: the labels, the per-component tables and counts.  Union-find with "the larger root goes under the
 *   smaller id", one lane per triangle and two unions each, every find halving the path it walks, and one more find per
 *   lane from its largest vertex, so that chains hooked at the same moment are shortened at once; the roots are numbered
 *   by the block counts and the two-level scan of every compaction here, the per-component counts are integer atomic adds,
 *   one per run of equal components within a wavefront.
 * sfm_mesh_clean_mark: takes the labels and comp_triangles of that call with the two parameters, writes comp_keep and
 *   counts, device int64 [3]: kept components, kept vertices, kept triangles, and leaves the first slots of every block of
 *   both compactions in the workspace (sfm_mesh_clean_workspace_bytes).  The selection is one workgroup: serial in the number
 *   of components.
 * sfm_mesh_clean_emit: takes the same workspace, untouched, with the same labels and comp_keep, and the capacities of the
 *   outputs; it writes nothing at or above the capacities and returns at once when both are 0.
 * sfm_mesh_gather_rows: dst row i = src row map[i], i < n, rows of row_bytes bytes; it applies vertex_map to any per-vertex
 *   array (vertex_colors, n_views, best_view).  Every map[i] must be a row of src; a negative one leaves its row untouched.
 * Every call returns SFM_ERR_ARG before any device work for a null handle, a count or a capacity below 0 or above 2^31 - 1,
 * n_components outside 0 .. n_vertices, a negative min_triangles or keep_largest, row_bytes < 1, a null pointer (allowed
 * only where its count is 0), or a workspace that is missing or too small. */
int sfm_mesh_components_workspace_bytes(int64_t n_vertices, int64_t* bytes_host);
int sfm_mesh_components(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const int32_t* triangles,
                        int32_t* vertex_component, int32_t* triangle_component, int32_t* comp_root, int32_t* comp_vertices,
                        int32_t* comp_triangles, int64_t* counts /* device [3] */, void* workspace, int64_t workspace_bytes);
int sfm_mesh_clean_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int64_t* bytes_host);
int sfm_mesh_clean_mark(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t n_components,
                        const int32_t* vertex_component, const int32_t* triangle_component, const int32_t* comp_triangles,
                        int64_t min_triangles, int64_t keep_largest, uint8_t* comp_keep, int64_t* counts /* device [3] */,
                        void* workspace, int64_t workspace_bytes);
int sfm_mesh_clean_emit(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t n_components,
                        const int32_t* vertex_component, const int32_t* triangle_component, const uint8_t* comp_keep,
                        const int32_t* triangles, const double* vertices, const float* normals, int64_t cap_vertices,
                        int64_t cap_triangles, int32_t* vertex_map, int32_t* triangle_map, int32_t* triangles_out,
                        double* vertices_out, float* normals_out, void* workspace, int64_t workspace_bytes);
int sfm_mesh_gather_rows(sfm_handle h, const void* src, int64_t row_bytes, const int32_t* map, int64_t n, void* dst);

/* ---- the edge table of a mesh, its boundary loops and the filling of the small holes (sfm_amd/csrc/mesh_fill.hip,
 *      mesh_fill_rule.h, mesh_fill_plan.h) ----
 * Integers except for the new vertices and their normals; every output byte is a function of the inputs, the same from run
 * to run, and NumPy reproduces it (tests/mesh_fill_reference.py).
 *
 * Input.  n_vertices, 0 .. 2^31 - 1, and triangles int32 [n_triangles][3] with n_triangles 0 .. (2^31 - 1) / 3.
 * Half-edges.  Half-edge h = 3 t + k of triangle t runs from a_h = tri[t][k] to b_h = tri[t][(k + 1) % 3].  It is live iff
 *   the triangle is sound (all three indices in [0, n_vertices), as for sfm_mesh_components) and a_h != b_h.
 * Uses and twin.  uses[h] is the number of live half-edges on the same unordered pair {a, b}, itself included, and 0 for a
 *   half-edge that is not live.  twin[h] is the other half-edge of the pair iff uses == 2 and the two run in opposite
 *   directions, otherwise -1.  An edge is boundary when uses == 1, inconsistent when uses == 2 without a twin, non-manifold
 *   when uses > 2.
 * Successor.  For a boundary half-edge h rotate about b_h inside the surface: g = the next half-edge of h's triangle; while
 *   g is live and not boundary: stop with -1 if it has no twin, otherwise g = the next half-edge of the triangle of
 *   twin[g].  next[h] = g if the walk ended on a boundary half-edge, otherwise -1 (a half-edge that is not live, or an
 *   inconsistent or non-manifold edge in the fan); -1 for every h that is not boundary.  The walk visits each triangle of
 *   the fan once; it has a budget of n_triangles + 1 steps, which no valid twin table exhausts, and raises the status word
 *   when it runs out.  Rotation through twins is reversible, so next is injective where it is defined.
 * Loops.  From a boundary half-edge follow next for at most 64 steps.  If the walk returns to h, h lies on a short loop of
 *   that length, named by its smallest half-edge, its leader; otherwise on none (the walk met -1, or the cycle is longer
 *   than 64: the wavefront).  Short loops are numbered in ascending order of their leaders; a loop has at least 3 edges, so
 *   there are at most n_triangles.
 * Sub-loops.  Where two holes touch in a vertex the surface about it is two fans, and one loop passes that vertex twice.
 *   Walk the loop from its leader in next order with a stack: push h; if some stack entry p has a_p == b_h, the entries
 *   p .. top are a sub-loop: emit and pop them.  At most one p can match (the start vertices on the stack are distinct at
 *   all times) and the stack is empty when the walk ends.  A sub-loop has distinct vertices and at least 3 edges; it is
 *   named by its smallest half-edge and is filled iff 3 <= n <= max_edges, 1 <= max_edges <= 64.
 * Fill.  The filled sub-loops in ascending order of their names get the new vertices n_vertices + r.  Walk the sub-loop from
 *   its name in its own cyclic order (the stack order): c = (((v[a_0] + v[a_1]) + ...)) / (double)n per coordinate, in
 *   float64, sequentially, without FMA.  The new normal is unit(sum over the same order of cross(v[a_h] - v[b_h],
 *   c - v[b_h])): every product and sum rounds on its own, l2 = (x x + y y) + z z, each component is divided by sqrt(l2) and
 *   rounded once to float32; (0, 0, 0) when l2 is 0 or not finite.  Every half-edge h of a filled sub-loop gives one
 *   triangle (b_h, a_h, n_vertices + r), the triangles in ascending order of h.  Old vertices, normals and triangles are not
 *   touched: the new ones are to be appended.  NaN and infinite coordinates propagate; no input bit pattern changes an
 *   address.
 * Limits: boundary cycles of more than 64 edges - an outline is one - and the holes that touch them stay open and are only
 *   counted by their edges; the centroid fan is the only patch, without a planarity test and without refinement of large
 *   patches; non-manifold and inconsistent edges are reported, not repaired, and a hole whose fan holds one stays open; the
 *   outline of a lone fragment of at most max_edges edges is a short loop too and is filled: clean first.
 *
 * sfm_mesh_edges: halfedge_uses, halfedge_twin, halfedge_next and halfedge_loop (the number of the short loop or -1), int32
 *   [3 n_triangles]; the first n_loops entries of loop_leader and loop_edges (int32; the caller provides n_triangles entries
 *   of each); counts, device int64 [8]: distinct live edges, boundary edges, inconsistent edges, non-manifold edges, short
 *   loops, boundary half-edges on no short loop, unsound triangles, status (0; 1 when a rotation ran out of its budget: the
 *   table is then not to be used).  uses and twin come out of one stable radix sort of (key, h) with the key (min(a, b) <<
 *   32) | max(a, b), all ones for a half-edge that is not live, and one lane per sorted slot that finds the ends of its run
 *   of equal keys: near-linear on a fan about one vertex.  The workspace holds the sort's temporary storage, which the
 *   library measures on the handle's device: sfm_mesh_edges_workspace_bytes takes the handle.
 * sfm_mesh_fill_mark: takes halfedge_next, n_loops and loop_leader of that call with max_edges; writes halfedge_fill, int32
 *   [3 n_triangles]: the rank r of the filled sub-loop the half-edge belongs to, or -1; counts, device int64 [4]: filled
 *   sub-loops, fill triangles, sub-loops left open, status (1 when the tables are not those of sfm_mesh_edges for these
 *   triangles: such a loop is left alone); and leaves the first slot of every block's fill triangles in the workspace
 *   (sfm_mesh_fill_workspace_bytes).  One wavefront per short loop.
 * sfm_mesh_fill_emit: takes the same workspace, untouched, with the same tables and halfedge_fill, the vertices (float64
 *   [n_vertices][3]) and the capacities of the outputs: fill_vertices float64 [cap_fill][3], fill_normals float32
 *   [cap_fill][3], fill_name int32 [cap_fill] (the name of sub-loop r), fill_triangles int32 [cap_triangles][3] and
 *   fill_triangle_halfedge int32 [cap_triangles] (the h of each).  It writes nothing at or above the capacities and returns
 *   at once when both are 0.
 * Every call returns SFM_ERR_ARG before any device work for a null handle, n_vertices outside 0 .. 2^31 - 1, n_triangles
 * outside 0 .. (2^31 - 1) / 3, n_loops outside 0 .. n_triangles, max_edges outside 1 .. 64, a capacity below 0 or above
 * 2^31 - 1, a null pointer (allowed only where its count is 0), or a workspace that is missing or too small. */
int sfm_mesh_edges_workspace_bytes(sfm_handle h, int64_t n_triangles, int64_t* bytes_host);
int sfm_mesh_edges(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const int32_t* triangles, int32_t* halfedge_uses,
                   int32_t* halfedge_twin, int32_t* halfedge_next, int32_t* halfedge_loop, int32_t* loop_leader,
                   int32_t* loop_edges, int64_t* counts /* device [8] */, void* workspace, int64_t workspace_bytes);
int sfm_mesh_fill_workspace_bytes(int64_t n_triangles, int64_t* bytes_host);
int sfm_mesh_fill_mark(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const int32_t* triangles,
                       const int32_t* halfedge_next, int64_t n_loops, const int32_t* loop_leader, int64_t max_edges,
                       int32_t* halfedge_fill, int64_t* counts /* device [4] */, void* workspace, int64_t workspace_bytes);
int sfm_mesh_fill_emit(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const int32_t* triangles,
                       const int32_t* halfedge_next, int64_t n_loops, const int32_t* loop_leader, const int32_t* halfedge_fill,
                       const double* vertices, int64_t cap_fill, int64_t cap_triangles, double* fill_vertices,
                       float* fill_normals, int32_t* fill_name, int32_t* fill_triangles, int32_t* fill_triangle_halfedge,
                       void* workspace, int64_t workspace_bytes);

/* ---- smoothing of a mesh: the vertex adjacency, Taubin steps over it, area-weighted vertex normals
 *      (sfm_amd/csrc/mesh_smooth.hip, mesh_smooth_rule.h, mesh_smooth_plan.h) ----
 * Taubin's lambda | mu smoothing with uniform weights.  float64 without FMA contraction, every sum in one stated order, no
 * float atomics and no order decided by an atomic: every output byte is a function of the inputs, the same from run to run,
 * and NumPy reproduces it (tests/mesh_smooth_reference.py).
 *
 * Adjacency (integers only).  Half-edge h = 3 t + k runs from a = tri[t][k] to b = tri[t][(k + 1) % 3].  A triangle is sound
 *   iff its three indices lie in [0, n_vertices); a half-edge is live iff its triangle is sound and a != b.  uses(a, b) is
 *   the number of live half-edges on the unordered pair.  The neighbours of v are the distinct other ends of its live
 *   half-edges in ascending index: index[ptr[v] .. ptr[v + 1]).  vertex_flags bit 0 (boundary) is set iff some neighbour j
 *   has uses(v, j) != 2 - boundary, non-manifold and doubled edges alike -, bit 1 (isolated) iff v has no neighbour.
 * State (uint8 per vertex, fixed before the first step).  Bit 0: boundary and pin_boundary.  Bit 1: pinned[v] != 0.  Bit 2:
 *   unsound, a coordinate of the INPUT is not finite.  Bit 3: isolated.
 * Step with factor f.  A vertex whose state is not 0 keeps its bytes.  Otherwise, over its neighbours j in ascending order
 *   whose state has bit 2 clear, per axis s = ((0 + x_j1) + x_j2) + ..., n their number; n == 0 keeps the bytes; otherwise
 *   m = s / (double)n and x' = x + f * (m - x), the product and the two sums rounding on their own.  Every step reads the
 *   vertices of the step before only (Jacobi, two buffers).  One iteration is a step with lam, then, when has_mu, one with
 *   mu; without mu the steps are plain Laplacian.  An unsound vertex is never read as a neighbour and never moves, so one
 *   NaN does not spread; values that overflow during the steps propagate.  No bit pattern of a coordinate becomes an
 *   address.
 * Normals.  The corners of v are the h = 3 t + k of the sound triangles with tri[t][k] == v, in ascending h.  Each adds the
 *   face normal of its triangle, with p0, p1, p2 its vertices in its own order whatever k is: e1 = p1 - p0, e2 = p2 - p0,
 *   n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), not normalised, so a triangle weighs with its area; per
 *   axis ns = ((0 + n_1) + n_2) + ...; l2 = (x x + y y) + z z; each component is divided by sqrt(l2) and rounded once to
 *   float32; zeros when l2 is 0 or not finite.  A triangle (a, a, b) is sound and adds a zero; the bytes depend on the order
 *   of the triangles, the direction does not.
 * Limits: uniform weights - no cotangent or bilateral weights, no feature preservation; a pinned outline stays jagged; a
 *   vertex of degree d costs its lane d dependent additions, and a run of r equal entries its head lane r steps; the
 *   normals' bytes depend on the order of the triangles.
 *
 * Calls.  Each has a workspace of its own (the _workspace_bytes functions take the handle because two of them size the
 * library's radix sorts on its device); nothing is read back inside a call.
 * sfm_mesh_adjacency: the symmetrised keys (a << 32) | b, two per live half-edge and all ones otherwise, ONE keys-only radix
 *   sort over the 32 + bits(n_vertices) bits they need, run heads, block counts and the two-level scan, a scatter of the
 *   heads and one lane per vertex.  Writes ptr int32 [n_vertices + 1], of index (int32; the caller provides 6 n_triangles
 *   elements, the upper bound) the first counts[0], vertex_flags uint8 [n_vertices]; counts, device int64 [4]: entries,
 *   boundary vertices, isolated vertices, unsound triangles.
 * sfm_mesh_smooth: takes those tables and n_index, the number of elements of index that may be read (the entries, or the
 *   capacity).  Enqueues the state kernel and one launch per step back to back on the handle's stream.  Writes vertices_out
 *   float64 [n_vertices][3] (not vertices_in; with iterations = 0 a copy of it) and vertex_state uint8 [n_vertices];
 *   counts, device int64 [5]: vertices pinned as boundary, pinned by the caller, unsound, isolated, status.  The status is
 *   1 when ptr decreases or leaves [0, n_index] or an entry lies outside [0, n_vertices): such a table is not of these
 *   triangles; the entry is skipped, the vertex with such a ptr keeps its bytes, and neither is ever an address.  The
 *   workspace holds the second buffer.
 * sfm_mesh_vertex_normals: one stable sort of (vertex, h) over the bits n_vertices needs, then one lane per vertex.  Writes
 *   normals float32 [n_vertices][3].
 * Every call returns SFM_ERR_ARG before any device work for a null handle, n_vertices outside 0 .. 2^31 - 1, n_triangles
 * outside 0 .. (2^31 - 1) / 6, n_index outside 0 .. 2^31 - 1, iterations outside 0 .. 1000, lam not finite in (0, 1], mu
 * (when has_mu) not finite in [-2, -lam), vertices_out == vertices_in, a null pointer (allowed only where its count is 0;
 * pinned may always be NULL), or a workspace that is missing or too small. */
int sfm_mesh_adjacency_workspace_bytes(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t* bytes_host);
int sfm_mesh_adjacency(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const int32_t* triangles, int32_t* ptr,
                       int32_t* index /* capacity 6 n_triangles */, uint8_t* vertex_flags, int64_t* counts /* device [4] */,
                       void* workspace, int64_t workspace_bytes);
int sfm_mesh_smooth_workspace_bytes(sfm_handle h, int64_t n_vertices, int64_t* bytes_host);
int sfm_mesh_smooth(sfm_handle h, int64_t n_vertices, const double* vertices_in, const int32_t* ptr, const int32_t* index,
                    int64_t n_index, const uint8_t* vertex_flags, const uint8_t* pinned /* or NULL */, int pin_boundary,
                    double lam, double mu, int has_mu, int64_t iterations, double* vertices_out, uint8_t* vertex_state,
                    int64_t* counts /* device [5] */, void* workspace, int64_t workspace_bytes);
int sfm_mesh_vertex_normals_workspace_bytes(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t* bytes_host);
int sfm_mesh_vertex_normals(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const double* vertices,
                            const int32_t* triangles, float* normals, void* workspace, int64_t workspace_bytes);

/* ---- decimation of a mesh: vertex clustering on a uniform grid with a quadric-optimal vertex per cell
 *      (sfm_amd/csrc/mesh_decimate.hip, mesh_decimate_rule.h, mesh_decimate_plan.h) ----
 * Rossignac-Borrel clustering with Lindstrom's placement.  float64 without FMA contraction, every sum in one stated order,
 * no float atomics and no order decided by an atomic: every output byte is a function of the inputs, the same from run to
 * run, and NumPy reproduces it (tests/mesh_decimate_reference.py).
 *
 * Input.  n_vertices, 0 .. 2^31 - 1, with vertices float64 [n_vertices][3] and normals float32 [n_vertices][3] or NULL;
 *   triangles int32 [n_triangles][3] with n_triangles 0 .. (2^31 - 1) / 3; origin, host [3], finite; cell, finite and > 0;
 *   placement, 0 for the mean and 1 for the quadric.
 * Cell of a vertex.  Per axis q_a = floor((v_a - origin_a) / cell) in float64.  The vertex is sound iff its three
 *   coordinates are finite and 0 <= q_a < 2^21 on every axis; its key is then (iz << 42) | (iy << 21) | ix.  An unsound
 *   vertex has no cell and vertex_cluster = -1.  The comparisons are made on the double: no bit pattern of a coordinate
 *   becomes an address.
 * Clusters.  The distinct keys in ascending order are the clusters 0 .. nc - 1, so the order is z-major.  The members of a
 *   cluster are its vertices in ascending index; cluster_first[c] is the smallest member, so sfm_mesh_gather_rows carries any
 *   per-vertex array across; cluster_size[c] is the member count.
 * Mean.  Per coordinate m = (((v_0 + v_1) + ...)) / (double)n over the members in that order.
 * Normal (when normals are given).  The float32 normals of the members, widened, are summed in the same order; l2 = (x x +
 *   y y) + z z; each component is divided by sqrt(l2) and rounded once to float32; zeros when l2 is 0 or not finite.
 * Sound triangle.  Its three indices lie in [0, n_vertices) and its three vertices are sound.
 * Quadric (placement = 1).  The corners of a cluster c are the h = 3 t + k of sound triangles with
 *   vertex_cluster[tri[t][k]] == c, in ascending h; a triangle with two corners in the cell counts twice.  For each corner,
 *   with p0, p1, p2 the triangle's vertices in its own order, whatever k is: e1 = p1 - p0, e2 = p2 - p0, n = (e1y e2z - e1z
 *   e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), r = p0 - m, s = (nx rx + ny ry) + nz rz; then A00 += nx nx, A01 += nx ny,
 *   A02 += nx nz, A11 += ny ny, A12 += ny nz, A22 += nz nz and g_a += n_a s, every product rounding on its own.  tr = (A00 +
 *   A11) + A22, lambda = tr * 2^-6, B = A with lambda added to its diagonal.  B y = g is solved in this order: d0 = B00, l10
 *   = B01 / d0, l20 = B02 / d0, d1 = B11 - l10 B01, u = B12 - l20 B01, l21 = u / d1, d2 = (B22 - l20 B02) - l21 u, z1 = g1
 *   - l10 g0, z2 = (g2 - l20 g0) - l21 z1, y2 = z2 / d2, y1 = z1 / d1 - l21 y2, y0 = (g0 / d0 - l10 y1) - l20 y2.  x = m +
 *   y.  The position is x iff tr > 0, d0 > 0, d1 > 0, d2 > 0, x is finite and lo_a <= x_a <= hi_a on every axis, with lo_a
 *   = origin_a + cell * (double)i_a and hi_a = origin_a + cell * (double)(i_a + 1); otherwise it is m.  cluster_placed[c]
 *   (uint8) says which was taken.  The regularisation pulls towards the mean, so a flat cell moves along its normal only
 *   and no eigen-decomposition is needed.
 * New triangles.  A sound triangle maps to (c0, c1, c2); it is degenerate when two of them are equal.  The others are
 *   grouped by their sorted triple; within a group E are those whose order is an even permutation of the sorted triple and
 *   O the odd ones.  If |E| > |O| the first of E in old triangle order is kept, if |O| > |E| the first of O, if |E| == |O|
 *   none: clustering folds small fins flat, and two triangles on one triple with opposite orientation cancel.  Kept triangles
 *   stay in old order; triangle_map[t'] is the old index.  Every cluster is an output vertex, referenced or not.
 * Limits: decimation by clustering only.  The grid is uniform: no adaptation to curvature, no target triangle count;
 *   features thinner than a cell pinch into non-manifold edges, which sfm_mesh_edges reports; unreferenced clusters stay as
 *   vertices until the mesh is cleaned; boundaries shrink towards the cell means; a run of r equal triples costs its head
 *   lane r steps; there is no edge-collapse refinement afterwards.
 *
 * Calls, in the shape of sfm_mesh_fill_mark / sfm_mesh_fill_emit: the host reads a count between them and allocates.  ONE
 * workspace (sfm_mesh_decimate_workspace_bytes, which takes the handle because it sizes the library's radix sorts on its
 * device) goes through the three calls untouched: it carries the vertices sorted by cell, the corners sorted by cluster and
 * the first slots of every block of kept triangles from one call to the next.
 * sfm_mesh_decimate_cluster: keys, one stable sort of (key, vertex) - over 64 bits: the 64th keeps the vertices without a
 *   cell apart from the last cell of the grid -, run heads, block counts and the two-level scan; writes vertex_cluster int32
 *   [n_vertices], and of cluster_start (int32; the caller provides n_vertices + 1 entries; positions in the sorted vertex
 *   list) the first nc + 1 entries, of cluster_first and cluster_size (int32; n_vertices entries each) the first nc; counts,
 *   device int64 [2]: clusters, unsound vertices.
 * sfm_mesh_decimate_mark: takes n_clusters and vertex_cluster of that call; a stable sort of (cluster, h) over the bits
 *   n_clusters needs gives the corner list of every cluster; the non-degenerate triangles are sorted by (triple, t), in one
 *   pass when three cluster numbers fit 63 bits and in two stable passes otherwise, the output bytes being the same either
 *   way; the head of every run of equal triples applies the duplicate rule.  Writes triangle_keep uint8 [n_triangles];
 *   counts, device int64 [5]: kept triangles, unsound triangles, degenerate triangles, triangles dropped by the duplicate
 *   rule, status (1 when vertex_cluster holds a number outside -1 .. n_clusters - 1: such a triangle counts as unsound).
 * sfm_mesh_decimate_emit: takes the same tables and the capacities of the outputs: new_vertices float64 [cap_clusters][3],
 *   new_normals float32 [cap_clusters][3] (not written, and may be NULL, when normals is NULL), cluster_placed uint8
 *   [cap_clusters], new_triangles int32 [cap_triangles][3] and triangle_map int32 [cap_triangles].  One lane per cluster
 *   walks its members and its corners in the rule's order.  It writes nothing at or above the capacities and returns at once
 *   when both are 0.
 * Every call returns SFM_ERR_ARG before any device work for a null handle, n_vertices outside 0 .. 2^31 - 1, n_triangles
 * outside 0 .. (2^31 - 1) / 3, n_clusters outside 0 .. n_vertices, a capacity below 0 or above 2^31 - 1, placement outside
 * 0 .. 1, an origin that is not finite, a cell that is not finite or <= 0, a null pointer (allowed only where its count is
 * 0), or a workspace that is missing or too small. */
int sfm_mesh_decimate_workspace_bytes(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t* bytes_host);
int sfm_mesh_decimate_cluster(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const double* vertices,
                              const double* origin /* host [3] */, double cell, int32_t* vertex_cluster, int32_t* cluster_start,
                              int32_t* cluster_first, int32_t* cluster_size, int64_t* counts /* device [2] */, void* workspace,
                              int64_t workspace_bytes);
int sfm_mesh_decimate_mark(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t n_clusters, const int32_t* triangles,
                           const int32_t* vertex_cluster, uint8_t* triangle_keep, int64_t* counts /* device [5] */,
                           void* workspace, int64_t workspace_bytes);
int sfm_mesh_decimate_emit(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t n_clusters, const double* vertices,
                           const float* normals, const int32_t* triangles, const int32_t* vertex_cluster,
                           const int32_t* cluster_start, const uint8_t* triangle_keep, const double* origin /* host [3] */,
                           double cell, int placement, int64_t cap_clusters, int64_t cap_triangles, double* new_vertices,
                           float* new_normals, uint8_t* cluster_placed, int32_t* new_triangles, int32_t* triangle_map,
                           void* workspace, int64_t workspace_bytes);

/* ---- colours of the mesh: per vertex a blend over the views that see it (sfm_amd/csrc/mesh_color.hip,
 *      mesh_color_rule.h, mesh_color_plan.h) ----
 * A pure function of its inputs: float64 without FMA contraction, no visit order, no atomics, no randomness, so NumPy
 * reproduces every output byte (tests/mesh_color_reference.py).
 * Inputs.  The vertex X (float64 [3]) and its normal n (float32 [3], widened to double) as sfm_mesh_emit wrote them.  The
 *   views in the layout of sfm_tsdf_integrate: heights / widths per image and ref_image per view (HOST), proj (device,
 *   float64 [n_ref][12]), depth (float32) and keep (uint8, or NULL: every finite depth counts) back to back at out_off[r].
 *   centres (device, float64 [n_ref][3]): the camera centres.  pixels (device, uint8 [n_out][channels]): the views' images
 *   back to back in the layout of depth, channels interleaved, channels 1 or 3, their order untouched.
 * Per vertex acc_k = 0, W = 0, m = 0, best = -1, bw = 0, then the views in position order:
 *   1. q_i, u = q0 / q2, v = q1 / q2, validity and the nearest pixel (yi, xi) as in sfm_tsdf_integrate; skipped unless
 *      valid (a NaN vertex never is).
 *   2. ds = the float32 depth at (yi, xi) widened; skipped unless ds is finite and keep there != 0; d = ds - q2; skipped
 *      unless d >= -tol && d <= tol.  This is the occlusion test: the view's own depth map says that it sees this surface
 *      and not one in front of it.
 *   3. g_a = C_a - X_a, l2 = (g0 g0 + g1 g1) + g2 g2; skipped unless l2 is finite and > 0.  c = 1 when n is all zeros,
 *      otherwise c = ((n0 g0 + n1 g1) + n2 g2) / sqrt(l2); skipped unless c >= min_cos (false on NaN).  wgt = c * c.
 *   4. Bilinear sample at (u, v): x0 = floor(u), fx = u - x0, the columns clamp((int)x0, 0, w - 1) and
 *      clamp((int)x0 + 1, 0, w - 1), the rows likewise from v with fy.  With the four pixel values of channel k widened to
 *      double as a, b (upper row) and e, f (lower row): top = a + fx * (b - a), bot = e + fx * (f - e),
 *      s_k = top + fy * (bot - top).
 *   5. acc_k = acc_k + wgt * s_k;  W = W + wgt;  m = m + 1;  if wgt > bw then bw = wgt and best = v (ties go to the
 *      earlier view).
 * After the views colors[k] = (uint8) min(floor(acc_k / W + 0.5), 255) when m > 0 && W > 0, otherwise fill;
 *   n_views = min(m, 255) (uint8); best_view = best (int32, -1 for none).  colors is uint8 [n_vertices][channels].
 * Limits: one colour per vertex (sfm_mesh_texture below gives every triangle a patch of texels by the same rule), no
 *   exposure compensation; a vertex that no view sees gets fill and is not filled from its neighbours; every view that
 *   passes weighs by its angle only.  (Gains per view are estimated and applied in front of this call: "exposure of the
 *   views" below.)
 * The workspace (sfm_mesh_colors_workspace_bytes) holds the view table.  Nothing is written at or above n_vertices, and
 *   the call returns at once for n_vertices == 0.  SFM_ERR_ARG before any device work for a null handle, what
 *   sfm_tsdf_integrate refuses about the views, channels not 1 or 3, n_vertices below 0 or above 2^31 - 1, tol not finite or
 *   below 0, min_cos not finite, not > 0 or above 1, fill outside 0 .. 255, a null pointer (keep excepted; depth / pixels
 *   may be null only when there is no pixel, vertices / normals / the outputs only when n_vertices is 0), or a workspace
 *   that is missing or too small.  No kernel reads outside a map or an image. */
int sfm_mesh_colors_workspace_bytes(int32_t n_ref, int64_t* bytes_host);
int sfm_mesh_colors(sfm_handle h, const int32_t* heights /* host */, const int32_t* widths /* host */, int32_t n_img,
                    int32_t n_ref, const int32_t* ref_image /* host */, const double* proj /* device [n_ref][12] */,
                    const double* centres /* device [n_ref][3] */, const float* depth, const uint8_t* keep /* or NULL */,
                    const uint8_t* pixels, int32_t channels, int64_t n_vertices, const double* vertices, const float* normals,
                    double tol, double min_cos, int32_t fill, uint8_t* colors, uint8_t* n_views, int32_t* best_view,
                    void* workspace, int64_t workspace_bytes);

/* ---- exposure of the views: one gain per view and channel, estimated from the mesh (sfm_amd/csrc/mesh_exposure.hip,
 *      mesh_exposure_rule.h, mesh_exposure_plan.h) ----
 * sfm_mesh_colors, sfm_mesh_texture and sfm_render_score assume that every photograph of a surface point holds the same
 * value.  Where the exposure drifts between the shots, this stage estimates one gain per view and channel from the vertices
 * that several views see and applies it to the images BEFORE they go to those calls, which do not change.  The device makes
 * bytes and integer sums; the gains are solved on the host (sfm_amd/exposure.py, solve_gains).  NumPy reproduces every
 * output byte (tests/mesh_exposure_reference.py).
 * Sample (sfm_mesh_exposure_sample).  The views, the vertices, tol and min_cos are those of sfm_mesh_colors.  For vertex X
 *   with the normal n and view v, steps 1 to 4 of sfm_mesh_colors unchanged: the view SEES the vertex iff it passes steps 1
 *   to 3, and then q_k = (uint8) min(floor(s_k + 0.5), 255.0) with s_k the bilinear sample of step 4, float64 without FMA
 *   contraction.  seen is uint8 [n_ref][n_vertices] holding 0 or 1, samples uint8 [n_ref][channels][n_vertices], 0 where the
 *   view does not see the vertex.  Every element of both is written.
 * Tables (sfm_mesh_exposure_gram).  With f_i(x) = (seen[i][x] != 0):
 *     overlap[i][j]  = #{x : f_i(x) and f_j(x)}                             int64 [n_ref][n_ref]
 *     sums[i][j][k]  = sum of samples[i][k][x] over those x                 int64 [n_ref][n_ref][channels]
 *   the diagonal included: what view i sees at all.  Both are INTEGER sums, so no order of summation exists and the tables
 *   are the same bytes whatever the launch geometry.  The call clears its outputs itself.  On the device they are the
 *   products F F^T and Q_k F^T over the vertex axis on the i8 matrix cores, Q - 128 where seen as the signed operand and
 *   sums = product + 128 * overlap; a workgroup takes a tile of 32 x 32 view pairs and a chunk of vertices
 *   (sfm_mesh_exposure_plan: out[0], out[1] the tile sides, out[2] the chunk length, out[3] the workgroups of the launch),
 *   accumulates in int32 - 128 * chunk < 2^31 - and adds its tile to the tables with integer atomics.
 * Gains (host, float64; not part of this library).  Per channel k: a view with sum over j != i of overlap[i][j] == 0 (pairs
 *   below min_overlap count as 0) gets the gain 1 and leaves the system.  For every ordered pair i != j with
 *   N = overlap[i][j] > 0, a = sums[i][j][k] / N and b = sums[j][i][k] / N:
 *     A[i][i] += N (a a / sigma_n^2 + 1 / sigma_g^2),  A[j][j] += N b b / sigma_n^2,  A[i][j] -= N a b / sigma_n^2,
 *     A[j][i] -= N a b / sigma_n^2,  rhs[i] += N / sigma_g^2,   and g = solve(A, rhs).
 *   This is the gain compensation of panorama stitching (Brown and Lowe 2007) with the mesh's vertices in the place of the
 *   image overlaps: it minimises sum N ((g_i a - g_j b)^2 / sigma_n^2 + (1 - g_i)^2 / sigma_g^2).
 * Apply (sfm_images_gain).  n_img images back to back, uint8 [h][w][channels]; gains HOST float64 [n_img][channels], each
 *   finite and >= 0.  out = (uint8) min(floor((double)in * g + 0.5), 255.0) per pixel and channel: the product is rounded,
 *   then the sum (no FMA contraction).  pixels_out may be pixels_in.
 * Limits: one gain per view and channel - no offsets, no per-channel curves, no vignetting; no seam levelling inside the atlas;
 *   the gains are not applied inside the blend kernels and not estimated from the render's residuals; the solve is plain
 *   least squares, a wrong sample (a highlight, an occlusion the depth test missed) is not down-weighted; n_ref <= 1024.
 * The workspace (sfm_mesh_exposure_workspace_bytes) holds the view table of the sample call; the gram call takes the same
 *   workspace and leaves it alone.  Nothing is written outside the outputs.  SFM_ERR_ARG before any device work for a null
 *   handle, n_ref above 1024, whatever sfm_mesh_colors refuses about the views, channels, n_vertices, tol and min_cos, a gain
 *   that is negative or not finite, an image side outside 0 .. 32768, a null pointer (keep excepted; depth / pixels may be
 *   null only when there is no pixel, vertices / normals only when n_vertices is 0, seen / samples only without a vertex or
 *   a view, the tables only without a view, gains only without an image), or a workspace that is missing or too small. */
int sfm_mesh_exposure_workspace_bytes(int32_t n_ref, int32_t channels, int64_t n_vertices, int64_t* bytes_host);
int sfm_mesh_exposure_plan(int32_t n_ref, int32_t channels, int64_t n_vertices, int32_t* out_host /* [4] */);
int sfm_mesh_exposure_sample(sfm_handle h, const int32_t* heights /* host */, const int32_t* widths /* host */, int32_t n_img,
                             int32_t n_ref, const int32_t* ref_image /* host */, const double* proj /* device [n_ref][12] */,
                             const double* centres /* device [n_ref][3] */, const float* depth, const uint8_t* keep /* or NULL */,
                             const uint8_t* pixels, int32_t channels, int64_t n_vertices, const double* vertices,
                             const float* normals, double tol, double min_cos, uint8_t* seen /* [n_ref][n_vertices] */,
                             uint8_t* samples /* [n_ref][channels][n_vertices] */, void* workspace, int64_t workspace_bytes);
int sfm_mesh_exposure_gram(sfm_handle h, int32_t n_ref, int32_t channels, int64_t n_vertices, const uint8_t* seen,
                           const uint8_t* samples, int64_t* overlap /* [n_ref][n_ref] */,
                           int64_t* sums /* [n_ref][n_ref][channels] */, void* workspace, int64_t workspace_bytes);
int sfm_images_gain(sfm_handle h, const int32_t* heights /* host */, const int32_t* widths /* host */, int32_t n_img,
                    int32_t channels, const double* gains /* host [n_img][channels] */, const uint8_t* pixels_in,
                    uint8_t* pixels_out);

/* ---- texture of the mesh: a patch of texels per triangle in one atlas, every texel blended over the views that see it
 *      (sfm_amd/csrc/mesh_texture.hip, mesh_texture_rule.h, mesh_texture_plan.h) ----
 * A pure function of its inputs: float64 without FMA contraction and integers, no visit order, no atomics, no randomness,
 * so NumPy reproduces every output byte (tests/mesh_texture_reference.py).
 * Layout, a pure function of (n_triangles, texels, cells_per_row).  s = texels, 1 <= s <= 64, and P = s + 3.  Triangle t
 *   lives in cell c = t >> 1, half t & 1; cell c starts at texel (x0, y0) = ((c % cells_per_row) * P, (c / cells_per_row) * P).
 *   The atlas is W = cells_per_row * P wide and H = ceil(ceil(n_triangles / 2) / cells_per_row) * P high, W, H <= 32768
 *   (sfm_mesh_texture_size).  Local coordinates (i, j) of a triangle run over i, j >= 0, i + j <= s + 1; half 0 puts (i, j)
 *   at texel (x0 + i, y0 + j), half 1 at (x0 + P - 1 - i, y0 + P - 1 - j): a point reflection, so the orientation is kept.
 *   The corners sit on texel centres: corner 0 at (0, 0), corner 1 at (s, 0), corner 2 at (0, s).
 *   The inverse map takes a texel (x, y) with lx = x % P, ly = y % P: lx + ly <= s + 1 is half 0 with (i, j) = (lx, ly);
 *   lx + ly >= s + 3 is half 1 with (i, j) = (P - 1 - lx, P - 1 - ly); lx + ly == s + 2 belongs to no triangle, and so does
 *   a half whose t >= n_triangles.
 * Barycentric numerators over 2 s.  Interior texels (i + j <= s): n1 = 2 i, n2 = 2 j, n0 = 2 s - n1 - n2.  The diagonal
 *   i + j == s + 1 is the gutter: n1 = clamp(2 i - 1, 0, 2 s), n2 = 2 s - n1, n0 = 0 - the texel centre moved onto the
 *   hypotenuse.  With the corners on texel centres and this gutter a bilinear lookup at any point inside a triangle takes
 *   non-zero weight only from that triangle's own texels; the sides i = -1 and j = -1 need no gutter.
 * Point and normal of a texel.  V0, V1, V2 the triangle's vertices (float64), m0, m1, m2 their normals (float32 widened),
 *   the numerators converted to double:  X_a = ((n0 * V0_a + n1 * V1_a) + n2 * V2_a) / (double)(2 s), g_a the same expression
 *   of the normals, l2 = (g0 g0 + g1 g1) + g2 g2; the normal is g_a / sqrt(l2) when l2 is finite and > 0, else zeros.  It is
 *   used in double and not rounded to float32.
 * Colour.  Steps 1 to 5 of sfm_mesh_colors and its finish, applied to (X, normal) with the same views, tol, min_cos and
 *   fill: texture[y][x][k] is that colour, views[y][x] = min(m, 255).  A triangle with a vertex index outside
 *   [0, n_vertices) is seen by no view - fill and 0, and nothing is read through the bad index.  Texels that belong to no
 *   triangle get fill and 0.  Every texel of the H x W atlas is written and nothing outside it.
 * uv (float32 [n_triangles][3][2]): for corner k at texel (x, y) it is ((x + 0.5) / W, (y + 0.5) / H), computed in double
 *   and rounded once; v counts downwards from the top row (writers flip it where a format wants that).  Written for every
 *   triangle, those with bad indices included.
 * Limits: one patch size for all triangles (the triangles of marching tetrahedra are all voxel-sized; slivers waste
 *   texels), no chart merging (triangles that share an edge share no texel), no view culling per triangle, no exposure
 *   compensation, no fill-in of unseen texels, no mip levels.  (Gains per view are estimated and applied in front of this
 *   call: "exposure of the views" above.)
 * The workspace (sfm_mesh_texture_workspace_bytes) holds the view table.  The call returns at once for n_triangles == 0.
 *   SFM_ERR_ARG before any device work for a null handle, what sfm_mesh_colors refuses about the views and the scalars
 *   (channels, n_vertices, tol, min_cos, fill), texels outside 1 .. 64, cells_per_row < 1, W or H above 32768, n_triangles
 *   below 0 or above 2^31 - 1, a null pointer (keep excepted; depth / pixels may be null only when there is no pixel,
 *   vertices / normals only when n_vertices is 0, triangles and the outputs only when n_triangles is 0), or a workspace that
 *   is missing or too small.  sfm_mesh_texture_size refuses the same layouts and a null output.  No kernel reads outside a
 *   map, an image or the mesh. */
int sfm_mesh_texture_size(int64_t n_triangles, int32_t texels, int32_t cells_per_row, int32_t* width_host, int32_t* height_host);
int sfm_mesh_texture_workspace_bytes(int32_t n_ref, int64_t* bytes_host);
int sfm_mesh_texture(sfm_handle h, const int32_t* heights /* host */, const int32_t* widths /* host */, int32_t n_img,
                     int32_t n_ref, const int32_t* ref_image /* host */, const double* proj /* device [n_ref][12] */,
                     const double* centres /* device [n_ref][3] */, const float* depth, const uint8_t* keep /* or NULL */,
                     const uint8_t* pixels, int32_t channels, int64_t n_vertices, const double* vertices, const float* normals,
                     int64_t n_triangles, const int32_t* triangles, int32_t texels, int32_t cells_per_row, double tol,
                     double min_cos, int32_t fill, uint8_t* texture /* [H][W][channels] */, uint8_t* views /* [H][W] */,
                     float* uv /* [n_triangles][3][2] */, void* workspace, int64_t workspace_bytes);

/* ---- render of the mesh: depth, triangle, barycentrics and colour per pixel of any camera (sfm_amd/csrc/mesh_render.hip,
 *      mesh_render_rule.h, mesh_render_plan.h) ----
 * A pure function of its inputs: float64 without FMA contraction and integers, no floating-point atomics, no randomness;
 * the only atomic is an integer minimum, which has no order, so NumPy reproduces every output byte
 * (tests/mesh_render_reference.py).
 * Inputs.  n_cam cameras: heights / widths (HOST, 0 .. 32768 each; a camera with a side of 0 has no pixel) and proj (device,
 *   float64 [n_cam][12], row-major [K R | K t], world to pixels, as sfm_tsdf_integrate takes it).  The outputs of camera c
 *   start at pixel off[c] = sum over c' < c of heights[c'] * widths[c'].  vertices float64 [n_vertices][3] and triangles int32
 *   [n_triangles][3] as sfm_mesh_emit wrote them.  color_mode 0: no colour; 1: vertex_colors uint8 [n_vertices][channels]
 *   (what sfm_mesh_colors made); 2: the atlas uint8 [atlas_h][atlas_w][channels] with uv float32 [n_triangles][3][2] (what
 *   sfm_mesh_texture made).  channels 1 or 3.
 * Per camera P with an image of w x h pixels, pixel (x, y) having its centre at (x, y):
 *   1. Project, per vertex: q_i = ((P_i0 X0 + P_i1 X1) + P_i2 X2) + P_i3, u = q0 / q2, v = q1 / q2.  A vertex is usable iff
 *      q2 > 0 and u, v, q2 are finite.  A triangle with a corner that is not usable, or with an index outside [0, n_vertices),
 *      draws nothing; it is not clipped against the near plane, and nothing is read through a bad index.
 *   2. Bounding box, per triangle with the corners a, b, c: columns ceil(min u) .. floor(max u), rows ceil(min v) ..
 *      floor(max v), both cut to the image.  An empty box draws nothing.
 *   3. Inside test at (x, y): w0 = (ub - x)(vc - y) - (vb - y)(uc - x), w1 = (uc - x)(va - y) - (vc - y)(ua - x),
 *      w2 = (ua - x)(vb - y) - (va - y)(ub - x), A = (w0 + w1) + w2.  Inside iff A != 0 and (w0, w1, w2 all >= 0 or all <= 0).
 *      Both orientations draw (the mesh is open; no back-face culling).  A pixel on a shared edge is claimed by both
 *      triangles, and step 5 decides.
 *   4. Depth: r_k = w_k / q2_k, s = (r0 + r1) + r2, depth = (float)(A / s): 1 / z is linear on the screen.  The pixel is
 *      skipped unless that float32 is finite and > 0.
 *   5. Winner: the smallest (depth as float32, triangle index) in lexicographic order over the triangles that claim the
 *      pixel.  A positive float32 orders like its bits, so this is the minimum of one 64-bit unsigned key per pixel, the
 *      depth's bits in the high word and the index in the low word, whatever the visit order.
 *   6. Outputs per pixel.  triangle (int32): the winner, -1 where nothing draws.  depth (float32): the winner's, the quiet
 *      NaN 0x7FC00000 where nothing draws.  bary (float32 [3]): b_k = r_k / s of the winner, recomputed, kept in double for the
 *      shading and rounded once for the output; zeros where nothing draws.  color (uint8 [channels], color_mode != 0): fill
 *      where nothing draws, else with round(x) = min(max(floor(x + 0.5), 0), 255)
 *      - vertex colours: round((b0 c_a + b1 c_b) + b2 c_c) per channel, c the colours of the winner's corners;
 *      - atlas: px = ((b0 U_a + b1 U_b) + b2 U_c) * atlas_w - 0.5 with U the float32 uv column of the winner's corners
 *        widened to double, py likewise from the uv row with atlas_h; x0 = floor(px), fx = px - x0, the columns x0 and x0 + 1
 *        clamped to 0 .. atlas_w - 1, rows likewise; the bilinear sample of step 4 of sfm_mesh_colors over the four texels,
 *        rounded by round.  uv is used as it is: the atlas rule keeps the taps that weigh inside the triangle's own patch.
 * Limits: no clipping against the near plane (a triangle with a corner behind the camera is dropped whole), no culling, one
 *   sample per pixel and so no anti-aliasing, no mip levels, the nearest depth wins alone (no blending, no transparency).
 * The workspace (sfm_mesh_render_workspace_bytes; mesh_render_plan.h has the layout) holds at byte 0 one uint64, after the
 *   call the number of (camera, triangle) boxes of more than 64 pixels, then the camera table, one 64-bit key per pixel, the
 *   projected vertices of every camera and the list of those boxes.  Nothing is written at or above the sizes given.
 *   SFM_ERR_ARG before any device work for a null handle, n_cam outside 0 .. 65535, a side outside 0 .. 32768, n_vertices or
 *   n_triangles below 0 or above 2^31 - 1, color_mode not 0, 1 or 2, channels not 1 or 3 with a colour, fill outside
 *   0 .. 255, an atlas side outside 1 .. 32768 when there is a triangle, a null pointer (heights / widths / proj may be null
 *   only without a camera, vertices without a vertex, triangles without a triangle, the outputs without a pixel, color and
 *   the colour sources where color_mode does not ask for them), or a workspace that is missing or too small. */
int sfm_mesh_render_workspace_bytes(int32_t n_cam, const int32_t* heights /* host */, const int32_t* widths /* host */,
                                    int64_t n_vertices, int64_t n_triangles, int64_t* bytes_host);
int sfm_mesh_render(sfm_handle h, int32_t n_cam, const int32_t* heights /* host */, const int32_t* widths /* host */,
                    const double* proj /* device [n_cam][12] */, int64_t n_vertices, const double* vertices, int64_t n_triangles,
                    const int32_t* triangles, int32_t color_mode, int32_t channels, const uint8_t* vertex_colors /* or NULL */,
                    const float* uv /* or NULL */, const uint8_t* atlas /* or NULL */, int32_t atlas_w, int32_t atlas_h,
                    int32_t fill, float* depth /* [n_pix] */, int32_t* triangle /* [n_pix] */, float* bary /* [n_pix][3] */,
                    uint8_t* color /* [n_pix][channels], or NULL */, void* workspace, int64_t workspace_bytes);

/* ---- score of a render against the photographs: error, PSNR and SSIM sums and the distance to the views' own depth
 *      (sfm_amd/csrc/render_score.hip, render_score_rule.h, render_score_plan.h) ----
 * A pure function of its inputs.  Every statistic is an INTEGER sum, so no order of summation exists and NumPy reproduces
 * every output byte whatever the launch geometry (tests/render_score_reference.py); the two quotients are float64 without
 * FMA contraction.
 * Inputs.  n_view views in the order of the render: heights / widths (HOST, 0 .. 32768 each); the arrays of view v start at
 *   pixel off[v] = sum over v' < v of heights[v'] * widths[v'] (times channels for the colour arrays).  channels c is 1 or 3.
 *   From the render (sfm_mesh_render): render_color uint8 [h][w][c], render_triangle int32 [h][w], render_depth float32 [h][w].
 *   photos uint8 [h][w][c].  Optional: photo_mask uint8 [h][w]; view_depth float32 [h][w] with view_keep uint8 [h][w], the
 *   view's own depth map and what sfm_depth_filter kept of it (both or neither).
 * Per view of w x h pixels:
 *   1. A pixel is covered iff triangle >= 0, and compared iff it is covered and the mask, if given, is > 0.  Per channel k
 *      with e = render - photo in integers: sad[k] += |e| and sse[k] += e e over the compared pixels; abs_error is |e| there
 *      and 0 elsewhere.
 *   2. SSIM over a uniform W x W window, W = window odd in 3 .. 11, n = W W.  A pixel has a window iff all n pixels of the
 *      window centred on it are inside the image and compared.  Per channel over the window in int64, x the render and y the
 *      photograph: Sx, Sy, Sxx, Syy, Sxy;  a = 2 Sx Sy,  b = Sx Sx + Sy Sy,  cv = 2 (n Sxy - Sx Sy),
 *      vr = (n Sxx - Sx Sx) + (n Syy - Sy Sy),  c1 = (double)(n n) * 6.5025,  c2 = (double)(n n) * 58.5225 (the usual
 *      (0.01 * 255)^2 and (0.03 * 255)^2 scaled by n^2),
 *        s_k = (((double)a + c1) * ((double)cv + c2)) / (((double)b + c1) * ((double)vr + c2)).
 *      This is the population covariance (divisor n), not the sample covariance (n - 1).  The denominator is positive, so
 *      no NaN arises.  s = s_0, or ((s_0 + s_1) + s_2) / 3.0 for three channels.  ssim_map = (float)s, the quiet NaN
 *      0x7FC00000 where there is no window.  n_ssim += 1 and q_ssim += (int64)floor(s * 16777216.0 + 0.5), a signed sum.
 *   3. Depth, only with view_depth.  A pixel is seen iff keep != 0 and dv = view_depth is finite.  n_both counts covered and
 *      seen pixels; there r = |(double)dr - (double)dv| with dr = render_depth.  When r is a NaN nothing more is counted.
 *      Otherwise n_agree += (r <= rel_tol * (double)dv) and q_rel += (int64)floor(t * 16777216.0 + 0.5), where
 *      t = min(r / (double)dv, 1.0) for dv > 0; for dv <= 0, where r / dv is no relative error, t = 0.0 when r == 0 and 1.0
 *      otherwise (such a pixel agrees only when dr == dv == 0).  n_render_only counts covered pixels that are not seen,
 *      n_view_only seen pixels that are not covered.
 *   4. stats int64 [n_view][16]: n_pixels (h w), n_compared, sad[3], sse[3], n_ssim, q_ssim, n_both, n_agree, q_rel,
 *      n_render_only, n_view_only, 0.  The columns of channels that are not there are 0, and so are the depth columns
 *      without view_depth.  The call clears the table itself.  Means, PSNR = 10 log10(255^2 n_compared c / sum sse) and the
 *      mean SSIM q_ssim / (2^24 n_ssim) are formed by the caller in double from these integers; pooled figures come from the
 *      summed integers.
 * Limits: a uniform window only (no Gaussian weights), one scale, no learned metric; no exposure compensation is estimated;
 *   pixels the mesh does not cover are counted (n_view_only) and not penalised in the error.  (Gains per view come from the
 *   mesh, not from these residuals: "exposure of the views" above.)
 * abs_error (uint8 [h][w][c]) and ssim_map (float32 [h][w]) may each be NULL: statistics only.  The workspace
 *   (sfm_render_score_workspace_bytes; render_score_plan.h has the layout) holds the table of the views.
 *   sfm_render_score_tile gives the sides of the tile one workgroup takes.  Nothing is written outside the pixels of the
 *   views and the n_view rows of stats.  SFM_ERR_ARG before any device work for a null handle, n_view outside 0 .. 65535, a
 *   side outside 0 .. 32768, channels not 1 or 3, window even or outside 3 .. 11, rel_tol not finite or negative, view_keep
 *   without view_depth or the reverse, a null pointer (heights / widths / stats may be null only without a view, the four
 *   images only without a pixel), or a workspace that is missing or too small. */
int sfm_render_score_tile(int32_t* tile_w, int32_t* tile_h);
int sfm_render_score_workspace_bytes(int32_t n_view, const int32_t* heights /* host */, const int32_t* widths /* host */,
                                     int64_t* bytes_host);
int sfm_render_score(sfm_handle h, int32_t n_view, const int32_t* heights /* host */, const int32_t* widths /* host */,
                     int32_t channels, const uint8_t* render_color, const int32_t* render_triangle, const float* render_depth,
                     const uint8_t* photos, const uint8_t* photo_mask /* or NULL */, const float* view_depth /* or NULL */,
                     const uint8_t* view_keep /* or NULL */, int32_t window, double rel_tol, int64_t* stats /* [n_view][16] */,
                     uint8_t* abs_error /* or NULL */, float* ssim_map /* or NULL */, void* workspace, int64_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
