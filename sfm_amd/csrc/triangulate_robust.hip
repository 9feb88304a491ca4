// Robust N-view triangulation of tracks (sfm_triangulate_tracks_robust, sfm_tracks_classify of include/sfm_amd.h; the
// rule is triangulate_robust.h), gfx950 only.  The work is bimodal: most tracks pass step 1, which costs what
// k_tri_tracks costs, and a failing one then costs up to 64 two-view Jacobi solves plus 64 passes over its observations,
// so with one thread per track a few lanes of a wavefront would hold the others for about 60 times as long.  Two passes:
//   k_robust_first    one thread per track: tri::solve over all used observations, every output of the track, and a
//                     failing track with at least 4 sound observations is appended to the work list: a ballot over the
//                     wavefront, one atomic add of its population count by the first flagged lane, and each flagged
//                     lane's slot is the base plus the count of flagged lanes below it.  Nothing depends on the list's
//                     order.
//   k_robust_rescue   persistent wavefronts over the work list, one entry at a time: lane h runs hypothesis h (H = 64 is
//                     the wavefront size on purpose), all lanes read the same observation so the gathers of P and C are
//                     broadcasts, the winner comes from an integer wave reduction on (score, -lane), its point is
//                     broadcast, every lane runs the same refit on the same numbers (one refit's time, no divergence),
//                     the flags are written with the lanes striding over the observations and lane 0 writes the
//                     track's outputs and moves it from its failing status to OK in counts.  The launch is sized by
//                     n_tracks alone: the list's length is read on the device.
//   k_tri_classify    one thread per track: tri::classify at a point that is given, the flags and the errors
// No FMA contraction anywhere in this file.
#include "common.h"
#include "triangulate_robust.h"
#include "triangulate_source.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ void track_range(const int64_t* __restrict__ track_ptr, int64_t t, int64_t n_obs, int64_t& lo,
                                            int& n_raw) {
  // the track's range, clamped into [0, n_obs] (track_ptr is trusted to ascend)
  int64_t hi = track_ptr[t + 1];
  lo = track_ptr[t];
  hi = hi < 0 ? 0 : (hi > n_obs ? n_obs : hi);
  lo = lo < 0 ? 0 : (lo > hi ? hi : lo);
  const int64_t len = hi - lo;
  n_raw = (int)(len > 0x7fffffffLL ? 0x7fffffffLL : len);
}

__global__ __launch_bounds__(256) void k_robust_first(TrackSrc src, const int64_t* __restrict__ track_ptr, int64_t n_tracks,
                                                      int64_t n_obs, int min_views, int refine_iters, double max_error,
                                                      int check_angle, double cos_min_angle, double* __restrict__ X,
                                                      int* __restrict__ status, int* __restrict__ n_views,
                                                      int* __restrict__ n_inliers, double* __restrict__ max_err,
                                                      uint8_t* __restrict__ obs_inlier, unsigned long long* __restrict__ counts,
                                                      int* __restrict__ list, int* __restrict__ list_count) {
  __shared__ int s_cnt[SFM_TRI_STATUS_COUNT];
  if (threadIdx.x < SFM_TRI_STATUS_COUNT) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool push = false;
  if (t < n_tracks) {
    int64_t lo;
    int n_raw;
    track_range(track_ptr, t, n_obs, lo, n_raw);
    src.b = lo;
    double Xt[3], me;
    int nv;
    const int st = tri::solve(src, n_raw, min_views, refine_iters, max_error, check_angle != 0, cos_min_angle, Xt, nv, me);
    X[3 * t] = Xt[0]; X[3 * t + 1] = Xt[1]; X[3 * t + 2] = Xt[2];
    status[t] = st;
    n_views[t] = nv;
    n_inliers[t] = st == SFM_TRI_OK ? nv : 0;
    max_err[t] = me;
    if (st == SFM_TRI_OK) {                                       // the call zeroed the flags
      int img;
      for (int k = 0; k < n_raw; ++k)
        if (src.camera(k, img) >= 0) obs_inlier[lo + k] = 1;
    }
    if (st != SFM_TRI_OK) {
      int n_used, s;
      tri::count_views(src, n_raw, n_used, s);
      push = s >= 4;
    }
    atomicAdd(&s_cnt[st], 1);
  }
  // every lane of the wavefront is here again.  Every track is pushed at most once: a slot stays below n_tracks.
  const unsigned long long flagged = __ballot(push);
  if (flagged) {
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)flagged) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(list_count, __popcll(flagged));
    base = __shfl(base, leader, 64);
    if (push) list[base + __popcll(flagged & ((1ull << lane) - 1ull))] = (int)t;
  }
  __syncthreads();
  if (threadIdx.x < SFM_TRI_STATUS_COUNT && s_cnt[threadIdx.x])
    atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_robust_rescue(TrackSrc src, const int64_t* __restrict__ track_ptr, int64_t n_tracks,
                                                       int64_t n_obs, int min_views, int refine_iters, double max_error,
                                                       int check_angle, double cos_min_angle, double* __restrict__ X,
                                                       int* __restrict__ status, int* __restrict__ n_inliers,
                                                       double* __restrict__ max_err, uint8_t* __restrict__ obs_inlier,
                                                       unsigned long long* __restrict__ counts, const int* __restrict__ list,
                                                       const int* __restrict__ list_count) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  int64_t n_list = *list_count;
  n_list = n_list < 0 ? 0 : (n_list > n_tracks ? n_tracks : n_list);
  for (int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_list; e += n_waves) {
    const int64_t t = list[e];
    if (t < 0 || t >= n_tracks) continue;                          // the same in every lane
    int64_t lo;
    int n_raw;
    track_range(track_ptr, t, n_obs, lo, n_raw);
    src.b = lo;
    int n_used, s;
    tri::count_views(src, n_raw, n_used, s);
    const int n_hyp = tri::hypotheses(s);
    double Xh[3] = {NAN, NAN, NAN};
    int score = 0;
    if (lane < n_hyp) score = tri::hypothesis(src, n_raw, s, max_error, check_angle != 0, cos_min_angle, lane, Xh);
    // the winner: highest score, ties to the lowest lane
    long long key = ((long long)score << 6) | (long long)(63 - lane);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const long long other = __shfl_xor(key, d, 64);
      key = other > key ? other : key;
    }
    const int best = (int)(key >> 6), winner = 63 - (int)(key & 63);
    if (best < (min_views < 3 ? 3 : min_views)) continue;
    const double Xw[3] = {__shfl(Xh[0], winner, 64), __shfl(Xh[1], winner, 64), __shfl(Xh[2], winner, 64)};
    double Xr[3], me;
    int ni;
    if (!tri::finish(src, n_raw, min_views, refine_iters, max_error, check_angle != 0, cos_min_angle, Xw, Xr, ni, me)) continue;
    tri::Obs o;
    for (int k = lane; k < n_raw; k += 64) {
      double err;
      obs_inlier[lo + k] = (src.get(k, o) && tri::agrees(o, Xr, max_error, err)) ? 1 : 0;
    }
    if (lane == 0) {
      const int full = status[t];
      X[3 * t] = Xr[0]; X[3 * t + 1] = Xr[1]; X[3 * t + 2] = Xr[2];
      n_inliers[t] = ni;
      max_err[t] = me;
      status[t] = SFM_TRI_OK;
      if ((unsigned)full < (unsigned)SFM_TRI_STATUS_COUNT) atomicAdd(&counts[full], ~0ull);     // minus one
      atomicAdd(&counts[SFM_TRI_OK], 1ull);
    }
  }
}

// The gates over the observations that agree with the caller's points.  A track without a point only counts its views.
__global__ __launch_bounds__(256) void k_tri_classify(TrackSrc src, const int64_t* __restrict__ track_ptr, int64_t n_tracks,
                                                      int64_t n_obs, int min_views, double max_error, int check_angle,
                                                      double cos_min_angle, const double* __restrict__ X,
                                                      const uint8_t* __restrict__ has_point, int* __restrict__ status,
                                                      int* __restrict__ n_views, int* __restrict__ n_inliers,
                                                      double* __restrict__ max_err, uint8_t* __restrict__ obs_inlier,
                                                      double* __restrict__ obs_err, unsigned long long* __restrict__ counts) {
  __shared__ int s_cnt[SFM_TRI_STATUS_COUNT];
  if (threadIdx.x < SFM_TRI_STATUS_COUNT) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n_tracks) {
    int64_t lo;
    int n_raw;
    track_range(track_ptr, t, n_obs, lo, n_raw);
    src.b = lo;
    const bool has = has_point[t] != 0;
    const double Xt[3] = {X[3 * t], X[3 * t + 1], X[3 * t + 2]};
    double me = NAN;
    int ni = 0, st = SFM_EVAL_NO_POINT;
    if (has) st = tri::classify(src, n_raw, min_views, Xt, max_error, check_angle != 0, cos_min_angle, ni, me);
    int nv = 0;
    tri::Obs o;
    for (int k = 0; k < n_raw; ++k) {
      double e = NAN;
      bool in = false;
      if (src.get(k, o)) {
        ++nv;
        if (has) {                                                  // tri::agrees, with the error kept as k_tri_evaluate gives it
          double hw, e2;
          e = tri::reproj(o, Xt, hw, e2);
          in = tri::sound(o) && hw > 0.0 && e <= max_error;
        }
      }
      obs_inlier[lo + k] = in ? 1 : 0;
      if (obs_err) obs_err[lo + k] = e;
    }
    status[t] = st;
    n_views[t] = nv;
    n_inliers[t] = ni;
    max_err[t] = me;
    if (has) atomicAdd(&s_cnt[st], 1);
  }
  __syncthreads();
  if (threadIdx.x < SFM_TRI_STATUS_COUNT && s_cnt[threadIdx.x])
    atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

TrackSrc track_source(const double* proj, const double* centres, const int32_t* cam_of_image, const int64_t* kp_ptr,
                      const double* kp_xy, const int32_t* obs_image, const int32_t* obs_kp, int64_t n_nodes, int32_t n_cams,
                      int32_t n_img) {
  TrackSrc src;
  src.proj = proj; src.centres = centres; src.cam_of_image = cam_of_image; src.kp_ptr = kp_ptr;
  src.kp_xy = (const double2*)kp_xy; src.obs_image = obs_image; src.obs_kp = obs_kp;
  src.n_nodes = n_nodes; src.b = 0; src.n_cams = n_cams; src.n_img = n_img;
  return src;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_triangulate_tracks_robust_workspace_bytes(int32_t n_cams, int64_t n_tracks, int64_t* bytes_host) {
  if (!bytes_host || n_cams < 0 || n_tracks < 0 || n_tracks > 0x3fffffffLL) return SFM_ERR_ARG;
  ws_carve ws{nullptr};
  ws.take<double>(3 * (int64_t)n_cams);
  ws.take<int>(n_tracks);
  ws.take<int>(1);
  *bytes_host = ws.bytes();
  return SFM_OK;
}

extern "C" int sfm_triangulate_tracks_robust(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam_of_image,
                                             int32_t n_img, const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes,
                                             const int64_t* track_ptr, int64_t n_tracks, const int32_t* obs_image,
                                             const int32_t* obs_kp, int64_t n_obs, int32_t min_views, int32_t refine_iters,
                                             double max_error, double min_angle_deg, double* X, int32_t* status,
                                             int32_t* n_views, int32_t* n_inliers, double* max_err, uint8_t* obs_inlier,
                                             int64_t* counts, void* workspace, int64_t workspace_bytes) {
  const char* me = "sfm_triangulate_tracks_robust";
  if (!h) return SFM_ERR_ARG;
  if (n_cams < 0 || n_img < 0 || n_nodes < 0 || n_tracks < 0 || n_obs < 0 || n_tracks > 0x3fffffffLL)
    return sfm_fail(h, SFM_ERR_ARG, me, "bad argument");
  if (min_views < 2) return sfm_fail(h, SFM_ERR_ARG, me, "min_views must be at least 2");
  if (refine_iters < 0) return sfm_fail(h, SFM_ERR_ARG, me, "refine_iters must not be negative");
  if (!(max_error >= 0.0) || !(min_angle_deg >= 0.0) || !(min_angle_deg <= 180.0))
    return sfm_fail(h, SFM_ERR_ARG, me, "max_error / min_angle_deg out of range");
  if (!counts) return sfm_fail(h, SFM_ERR_ARG, me, "null pointer");
  SFM_HIP(h, hipMemsetAsync(counts, 0, SFM_TRI_STATUS_COUNT * sizeof(int64_t), h->stream));
  if (n_tracks == 0) return SFM_OK;
  if (!track_ptr || !X || !status || !n_views || !n_inliers || !max_err || !workspace || (n_obs > 0 && !obs_inlier) ||
      (n_obs > 0 && (!obs_image || !obs_kp || !kp_ptr)) || (n_cams > 0 && !proj) || (n_img > 0 && !cam_of_image) ||
      (n_nodes > 0 && !kp_xy))
    return sfm_fail(h, SFM_ERR_ARG, me, "null pointer");
  int64_t need = 0;
  sfm_triangulate_tracks_robust_workspace_bytes(n_cams, n_tracks, &need);
  if (workspace_bytes < need) return sfm_fail(h, SFM_ERR_WORKSPACE, me, "workspace too small");
  ws_carve ws{(char*)workspace};
  double* centres = ws.take<double>(3 * (int64_t)n_cams);
  int* list = ws.take<int>(n_tracks);
  int* list_count = ws.take<int>(1);
  SFM_HIP(h, hipMemsetAsync(list_count, 0, sizeof(int), h->stream));
  if (n_obs > 0) SFM_HIP(h, hipMemsetAsync(obs_inlier, 0, (size_t)n_obs, h->stream));      // also where no track covers an observation
  if (n_cams > 0)
    hipLaunchKernelGGL(k_camera_centres, dim3(cdiv(n_cams, 256)), dim3(256), 0, h->stream, proj, n_cams, centres);
  const TrackSrc src = track_source(proj, centres, cam_of_image, kp_ptr, kp_xy, obs_image, obs_kp, n_nodes, n_cams, n_img);
  const double cos_min = cos(min_angle_deg * (3.14159265358979323846 / 180.0));
  const int check_angle = min_angle_deg > 0.0 ? 1 : 0;
  hipLaunchKernelGGL(k_robust_first, dim3(cdiv(n_tracks, 256)), dim3(256), 0, h->stream, src, track_ptr, n_tracks, n_obs,
                     (int)min_views, (int)refine_iters, max_error, check_angle, cos_min, X, status, n_views, n_inliers, max_err,
                     obs_inlier, (unsigned long long*)counts, list, list_count);
  // four wavefronts per workgroup, at most one wavefront per track, and no more than fill the device several times over
  const unsigned blocks = cdiv(n_tracks, 4) < 2048u ? cdiv(n_tracks, 4) : 2048u;
  hipLaunchKernelGGL(k_robust_rescue, dim3(blocks), dim3(256), 0, h->stream, src, track_ptr, n_tracks, n_obs, (int)min_views,
                     (int)refine_iters, max_error, check_angle, cos_min, X, status, n_inliers, max_err, obs_inlier,
                     (unsigned long long*)counts, (const int*)list, (const int*)list_count);
  SFM_LAUNCH_CHECK(h, me);
  return SFM_OK;
}

extern "C" int sfm_tracks_classify(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam_of_image, int32_t n_img,
                                   const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes, const int64_t* track_ptr,
                                   int64_t n_tracks, const int32_t* obs_image, const int32_t* obs_kp, int64_t n_obs,
                                   const double* X, const uint8_t* has_point, int32_t min_views, double max_error,
                                   double min_angle_deg, int32_t* status, int32_t* n_views, int32_t* n_inliers,
                                   double* max_err, uint8_t* obs_inlier, double* obs_err, int64_t* counts, void* workspace,
                                   int64_t workspace_bytes) {
  const char* me = "sfm_tracks_classify";
  if (!h) return SFM_ERR_ARG;
  if (n_cams < 0 || n_img < 0 || n_nodes < 0 || n_tracks < 0 || n_obs < 0 || n_tracks > 0x3fffffffLL)
    return sfm_fail(h, SFM_ERR_ARG, me, "bad argument");
  if (min_views < 2) return sfm_fail(h, SFM_ERR_ARG, me, "min_views must be at least 2");
  if (!(max_error >= 0.0) || !(min_angle_deg >= 0.0) || !(min_angle_deg <= 180.0))
    return sfm_fail(h, SFM_ERR_ARG, me, "max_error / min_angle_deg out of range");
  if (!counts) return sfm_fail(h, SFM_ERR_ARG, me, "null pointer");
  SFM_HIP(h, hipMemsetAsync(counts, 0, SFM_TRI_STATUS_COUNT * sizeof(int64_t), h->stream));
  if (n_tracks == 0) return SFM_OK;
  if (!track_ptr || !X || !has_point || !status || !n_views || !n_inliers || !max_err || !workspace ||
      (n_obs > 0 && !obs_inlier) || (n_obs > 0 && (!obs_image || !obs_kp || !kp_ptr)) || (n_cams > 0 && !proj) ||
      (n_img > 0 && !cam_of_image) || (n_nodes > 0 && !kp_xy))
    return sfm_fail(h, SFM_ERR_ARG, me, "null pointer");
  int64_t need = 0;
  sfm_triangulate_tracks_workspace_bytes(n_cams, &need);
  if (workspace_bytes < need) return sfm_fail(h, SFM_ERR_WORKSPACE, me, "workspace too small");
  ws_carve ws{(char*)workspace};
  double* centres = ws.take<double>(3 * (int64_t)n_cams);
  if (n_obs > 0) SFM_HIP(h, hipMemsetAsync(obs_inlier, 0, (size_t)n_obs, h->stream));
  if (n_cams > 0)
    hipLaunchKernelGGL(k_camera_centres, dim3(cdiv(n_cams, 256)), dim3(256), 0, h->stream, proj, n_cams, centres);
  const TrackSrc src = track_source(proj, centres, cam_of_image, kp_ptr, kp_xy, obs_image, obs_kp, n_nodes, n_cams, n_img);
  const double cos_min = cos(min_angle_deg * (3.14159265358979323846 / 180.0));
  hipLaunchKernelGGL(k_tri_classify, dim3(cdiv(n_tracks, 256)), dim3(256), 0, h->stream, src, track_ptr, n_tracks, n_obs,
                     (int)min_views, max_error, min_angle_deg > 0.0 ? 1 : 0, cos_min, X, has_point, status, n_views, n_inliers,
                     max_err, obs_inlier, obs_err, (unsigned long long*)counts);
  SFM_LAUNCH_CHECK(h, me);
  return SFM_OK;
}
