// N-view triangulation of the tracks of sfm_tracks_build (include/sfm_amd.h), gfx950 only:
//   k_camera_centres   prologue, one thread per camera: C = -M^-1 p4 into the workspace (triangulate_source.h, with TrackSrc)
//   k_tri_tracks       one thread per track: tri::solve of triangulate_solve.h over the track's CSR range
//   k_tri_evaluate     one thread per track: tri::judge at a point that is given (sfm_tracks_evaluate), plus the
//                      reprojection error of every observation
// One thread per track keeps every sum in observation order, so a track's outputs do not depend on its place in the
// batch.  The kernel is gather- and latency-bound: per observation it streams 8 B of CSR indices and 16 B of pixels and
// gathers 96 B of P and 24 B of C from tables that stay in cache (n_cams x 120 B); the passes of the refinement re-read
// the same lines.  No FMA contraction anywhere in this file: a two-view track gives the bits of sfm_triangulate2.
#include "common.h"
#include "triangulate_source.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void k_tri_tracks(TrackSrc src, const int64_t* __restrict__ track_ptr, int64_t n_tracks,
                                                    int64_t n_obs, int min_views, int refine_iters, double max_error,
                                                    int check_angle, double cos_min_angle, double* __restrict__ X,
                                                    int* __restrict__ status, int* __restrict__ n_views,
                                                    double* __restrict__ max_err, unsigned long long* __restrict__ counts) {
  __shared__ int s_cnt[SFM_TRI_STATUS_COUNT];
  if (threadIdx.x < SFM_TRI_STATUS_COUNT) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n_tracks) {
    // the track's range, clamped into [0, n_obs] (track_ptr is trusted to ascend)
    int64_t lo = track_ptr[t], hi = track_ptr[t + 1];
    hi = hi < 0 ? 0 : (hi > n_obs ? n_obs : hi);
    lo = lo < 0 ? 0 : (lo > hi ? hi : lo);
    const int64_t len = hi - lo;
    src.b = lo;
    double Xt[3], me;
    int nv;
    const int st = tri::solve(src, (int)(len > 0x7fffffffLL ? 0x7fffffffLL : len), min_views, refine_iters, max_error,
                              check_angle != 0, cos_min_angle, Xt, nv, me);
    X[3 * t] = Xt[0]; X[3 * t + 1] = Xt[1]; X[3 * t + 2] = Xt[2];
    status[t] = st;
    n_views[t] = nv;
    max_err[t] = me;
    atomicAdd(&s_cnt[st], 1);
  }
  __syncthreads();
  if (threadIdx.x < SFM_TRI_STATUS_COUNT && s_cnt[threadIdx.x])
    atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// The gates at the caller's points: same source, same prologue, no solve.  A track without a point only counts its views.
__global__ __launch_bounds__(256) void k_tri_evaluate(TrackSrc src, const int64_t* __restrict__ track_ptr, int64_t n_tracks,
                                                      int64_t n_obs, int min_views, double max_error, int check_angle,
                                                      double cos_min_angle, const double* __restrict__ X,
                                                      const uint8_t* __restrict__ has_point, int* __restrict__ status,
                                                      int* __restrict__ n_views, double* __restrict__ max_err,
                                                      double* __restrict__ obs_err, unsigned long long* __restrict__ counts) {
  __shared__ int s_cnt[SFM_TRI_STATUS_COUNT];
  if (threadIdx.x < SFM_TRI_STATUS_COUNT) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n_tracks) {
    int64_t lo = track_ptr[t], hi = track_ptr[t + 1];
    hi = hi < 0 ? 0 : (hi > n_obs ? n_obs : hi);
    lo = lo < 0 ? 0 : (lo > hi ? hi : lo);
    const int64_t len = hi - lo;
    const int n_raw = (int)(len > 0x7fffffffLL ? 0x7fffffffLL : len);
    src.b = lo;
    const bool has = has_point[t] != 0;
    const double Xt[3] = {X[3 * t], X[3 * t + 1], X[3 * t + 2]};
    double me = NAN;
    int nv = 0, st = SFM_EVAL_NO_POINT;
    if (has) {
      st = tri::judge(src, n_raw, min_views, Xt, max_error, check_angle != 0, cos_min_angle, nv, me);
    } else {
      int img;
      for (int k = 0; k < n_raw; ++k) nv += src.camera(k, img) >= 0;
    }
    status[t] = st;
    n_views[t] = nv;
    max_err[t] = me;
    if (obs_err) {
      tri::Obs o;
      for (int k = 0; k < n_raw; ++k) {
        double e = NAN, hw, e2;
        if (has && src.get(k, o)) e = tri::reproj(o, Xt, hw, e2);
        obs_err[lo + k] = e;
      }
    }
    if (has) atomicAdd(&s_cnt[st], 1);
  }
  __syncthreads();
  if (threadIdx.x < SFM_TRI_STATUS_COUNT && s_cnt[threadIdx.x])
    atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_triangulate_tracks_workspace_bytes(int32_t n_cams, int64_t* bytes_host) {
  if (!bytes_host || n_cams < 0) return SFM_ERR_ARG;
  ws_carve ws{nullptr};
  ws.take<double>(3 * (int64_t)n_cams);
  *bytes_host = ws.bytes();
  return SFM_OK;
}

extern "C" int sfm_triangulate_tracks(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam_of_image,
                                      int32_t n_img, const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes,
                                      const int64_t* track_ptr, int64_t n_tracks, const int32_t* obs_image,
                                      const int32_t* obs_kp, int64_t n_obs, int32_t min_views, int32_t refine_iters,
                                      double max_error, double min_angle_deg, double* X, int32_t* status, int32_t* n_views,
                                      double* max_err, int64_t* counts, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  if (n_cams < 0 || n_img < 0 || n_nodes < 0 || n_tracks < 0 || n_obs < 0 || n_tracks > 0x3fffffffLL)
    return sfm_fail(h, SFM_ERR_ARG, "sfm_triangulate_tracks", "bad argument");
  if (min_views < 2) return sfm_fail(h, SFM_ERR_ARG, "sfm_triangulate_tracks", "min_views must be at least 2");
  if (refine_iters < 0) return sfm_fail(h, SFM_ERR_ARG, "sfm_triangulate_tracks", "refine_iters must not be negative");
  if (!(max_error >= 0.0) || !(min_angle_deg >= 0.0) || !(min_angle_deg <= 180.0))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_triangulate_tracks", "max_error / min_angle_deg out of range");
  if (!counts) return sfm_fail(h, SFM_ERR_ARG, "sfm_triangulate_tracks", "null pointer");
  SFM_HIP(h, hipMemsetAsync(counts, 0, SFM_TRI_STATUS_COUNT * sizeof(int64_t), h->stream));
  if (n_tracks == 0) return SFM_OK;
  if (!track_ptr || !X || !status || !n_views || !max_err || !workspace ||
      (n_obs > 0 && (!obs_image || !obs_kp || !kp_ptr)) || (n_cams > 0 && !proj) || (n_img > 0 && !cam_of_image) ||
      (n_nodes > 0 && !kp_xy))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_triangulate_tracks", "null pointer");
  int64_t need = 0;
  sfm_triangulate_tracks_workspace_bytes(n_cams, &need);
  if (workspace_bytes < need) return sfm_fail(h, SFM_ERR_WORKSPACE, "sfm_triangulate_tracks", "workspace too small");
  ws_carve ws{(char*)workspace};
  double* centres = ws.take<double>(3 * (int64_t)n_cams);
  if (n_cams > 0)
    hipLaunchKernelGGL(k_camera_centres, dim3(cdiv(n_cams, 256)), dim3(256), 0, h->stream, proj, n_cams, centres);
  TrackSrc src;
  src.proj = proj; src.centres = centres; src.cam_of_image = cam_of_image; src.kp_ptr = kp_ptr;
  src.kp_xy = (const double2*)kp_xy; src.obs_image = obs_image; src.obs_kp = obs_kp;
  src.n_nodes = n_nodes; src.b = 0; src.n_cams = n_cams; src.n_img = n_img;
  const double cos_min = cos(min_angle_deg * (3.14159265358979323846 / 180.0));
  hipLaunchKernelGGL(k_tri_tracks, dim3(cdiv(n_tracks, 256)), dim3(256), 0, h->stream, src, track_ptr, n_tracks, n_obs,
                     (int)min_views, (int)refine_iters, max_error, min_angle_deg > 0.0 ? 1 : 0, cos_min, X, status, n_views,
                     max_err, (unsigned long long*)counts);
  SFM_LAUNCH_CHECK(h, "sfm_triangulate_tracks");
  return SFM_OK;
}

extern "C" int sfm_tracks_evaluate(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam_of_image, int32_t n_img,
                                   const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes, const int64_t* track_ptr,
                                   int64_t n_tracks, const int32_t* obs_image, const int32_t* obs_kp, int64_t n_obs,
                                   const double* X, const uint8_t* has_point, int32_t min_views, double max_error,
                                   double min_angle_deg, int32_t* status, int32_t* n_views, double* max_err, double* obs_err,
                                   int64_t* counts, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  if (n_cams < 0 || n_img < 0 || n_nodes < 0 || n_tracks < 0 || n_obs < 0 || n_tracks > 0x3fffffffLL)
    return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_evaluate", "bad argument");
  if (min_views < 2) return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_evaluate", "min_views must be at least 2");
  if (!(max_error >= 0.0) || !(min_angle_deg >= 0.0) || !(min_angle_deg <= 180.0))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_evaluate", "max_error / min_angle_deg out of range");
  if (!counts) return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_evaluate", "null pointer");
  SFM_HIP(h, hipMemsetAsync(counts, 0, SFM_TRI_STATUS_COUNT * sizeof(int64_t), h->stream));
  if (n_tracks == 0) return SFM_OK;
  if (!track_ptr || !X || !has_point || !status || !n_views || !max_err || !workspace ||
      (n_obs > 0 && (!obs_image || !obs_kp || !kp_ptr)) || (n_cams > 0 && !proj) || (n_img > 0 && !cam_of_image) ||
      (n_nodes > 0 && !kp_xy))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_evaluate", "null pointer");
  int64_t need = 0;
  sfm_triangulate_tracks_workspace_bytes(n_cams, &need);
  if (workspace_bytes < need) return sfm_fail(h, SFM_ERR_WORKSPACE, "sfm_tracks_evaluate", "workspace too small");
  ws_carve ws{(char*)workspace};
  double* centres = ws.take<double>(3 * (int64_t)n_cams);
  if (n_cams > 0)
    hipLaunchKernelGGL(k_camera_centres, dim3(cdiv(n_cams, 256)), dim3(256), 0, h->stream, proj, n_cams, centres);
  TrackSrc src;
  src.proj = proj; src.centres = centres; src.cam_of_image = cam_of_image; src.kp_ptr = kp_ptr;
  src.kp_xy = (const double2*)kp_xy; src.obs_image = obs_image; src.obs_kp = obs_kp;
  src.n_nodes = n_nodes; src.b = 0; src.n_cams = n_cams; src.n_img = n_img;
  const double cos_min = cos(min_angle_deg * (3.14159265358979323846 / 180.0));
  hipLaunchKernelGGL(k_tri_evaluate, dim3(cdiv(n_tracks, 256)), dim3(256), 0, h->stream, src, track_ptr, n_tracks, n_obs,
                     (int)min_views, max_error, min_angle_deg > 0.0 ? 1 : 0, cos_min, X, has_point, status, n_views, max_err,
                     obs_err, (unsigned long long*)counts);
  SFM_LAUNCH_CHECK(h, "sfm_tracks_evaluate");
  return SFM_OK;
}
