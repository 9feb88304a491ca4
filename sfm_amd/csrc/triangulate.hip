// N-view triangulation of the tracks of sfm_tracks_build and the gates at points that are given (include/sfm_amd.h; the
// rules are triangulate_solve.h and triangulate_robust.h), gfx950 only:
//   k_camera_centres      prologue, one thread per camera: C = -M^-1 p4 into the workspace
//   k_tri_tracks<false>   one thread per track: tri::solve of triangulate_solve.h over the track's CSR range
//   k_tri_tracks<true>    the first pass of sfm_triangulate_tracks_robust: the same, plus the flags, and a failing track
//                         with at least 4 sound observations is appended to the work list: a ballot over the wavefront,
//                         one atomic add of its population count by the first flagged lane, and each flagged lane's slot
//                         is the base plus the count of flagged lanes below it.  Nothing depends on the list's order.
//   k_robust_rescue       persistent wavefronts over the work list, one entry at a time: lane h runs hypothesis h (H = 64
//                         is the wavefront size on purpose), all lanes read the same observation so the gathers of P and C
//                         are broadcasts, the winner comes from an integer wave reduction on (score, -lane), its point is
//                         broadcast, every lane runs the same refit on the same numbers (one refit's time, no
//                         divergence), the flags are written with the lanes striding over the observations and lane 0
//                         writes the track's outputs and moves it from its failing status to OK in counts.  The launch is
//                         sized by n_tracks alone: the list's length is read on the device.
//   k_tri_evaluate        one thread per track: tri::judge at a point that is given (sfm_tracks_evaluate), plus the
//                         reprojection error of every observation
//   k_tri_classify        one thread per track: tri::classify at a point that is given, the flags and the errors
// One thread per track keeps every sum in observation order, so a track's outputs do not depend on its place in the
// batch.  The kernels are gather- and latency-bound: per observation a track streams 8 B of CSR indices and 16 B of pixels
// and gathers 96 B of P and 24 B of C from tables that stay in cache (n_cams x 120 B); the passes of the refinement
// re-read the same lines.  The robust work is bimodal: most tracks pass the first pass, and a failing one then costs up to
// 64 two-view Jacobi solves plus 64 passes over its observations, so with one thread per track a few lanes of a wavefront
// would hold the others for about 60 times as long: hence the second pass.
// No FMA contraction anywhere in this file: a two-view track gives the bits of sfm_triangulate2.
#include "common.h"
#include "triangulate_robust.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void k_camera_centres(const double* __restrict__ proj, int n_cams,
                                                        double* __restrict__ centres) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cams) return;
  double P[12], C[3];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = proj[12 * (int64_t)c + k];
  tri::camera_centre(P, C);
  centres[3 * (int64_t)c] = C[0]; centres[3 * (int64_t)c + 1] = C[1]; centres[3 * (int64_t)c + 2] = C[2];
}

// the observations [b, b + n_raw) of one track; every index is checked before it is used as one
struct TrackSrc {
  const double* __restrict__ proj;
  const double* __restrict__ centres;
  const int32_t* __restrict__ cam_of_image;
  const int64_t* __restrict__ kp_ptr;
  const double2* __restrict__ kp_xy;
  const int32_t* __restrict__ obs_image;
  const int32_t* __restrict__ obs_kp;
  int64_t n_nodes, b;
  int n_cams, n_img;

  __device__ __forceinline__ int camera(int k, int& img) const {
    img = obs_image[b + k];
    if ((unsigned)img >= (unsigned)n_img) return -1;
    const int cam = cam_of_image[img];
    return ((unsigned)cam >= (unsigned)n_cams) ? -1 : cam;
  }
  __device__ __forceinline__ bool centre(int k, double (&C)[3]) const {
    int img;
    const int cam = camera(k, img);
    if (cam < 0) return false;
    const double* c = centres + 3 * (int64_t)cam;
    C[0] = c[0]; C[1] = c[1]; C[2] = c[2];
    return true;
  }
  __device__ __forceinline__ bool get(int k, tri::Obs& o) const {
    int img;
    const int cam = camera(k, img);
    if (cam < 0) return false;
    const double* p = proj + 12 * (int64_t)cam;
    const double* c = centres + 3 * (int64_t)cam;
#pragma unroll
    for (int e = 0; e < 12; ++e) o.P[e] = p[e];
    o.C[0] = c[0]; o.C[1] = c[1]; o.C[2] = c[2];
    const int kp = obs_kp[b + k];
    const int64_t lo = kp_ptr[img], hi = kp_ptr[img + 1];
    const int64_t node = lo + kp;
    o.x = NAN; o.y = NAN;                        // a keypoint outside its image: a non-finite input (DEGENERATE)
    if (kp >= 0 && lo >= 0 && node < hi && node < n_nodes) {
      const double2 xy = kp_xy[node];
      o.x = xy.x; o.y = xy.y;
    }
    return true;
  }
};

// the options of a call as the kernels take them (refine_iters is 0 in the calls that judge a given point)
struct Gates {
  double max_error, cos_min_angle;
  int min_views, refine_iters, check_angle;
};

// the track's range, clamped into [0, n_obs] (track_ptr is trusted to ascend)
__device__ __forceinline__ void track_range(const int64_t* __restrict__ track_ptr, int64_t t, int64_t n_obs, int64_t& lo,
                                            int& n_raw) {
  int64_t hi = track_ptr[t + 1];
  lo = track_ptr[t];
  hi = hi < 0 ? 0 : (hi > n_obs ? n_obs : hi);
  lo = lo < 0 ? 0 : (lo > hi ? hi : lo);
  const int64_t len = hi - lo;
  n_raw = (int)(len > 0x7fffffffLL ? 0x7fffffffLL : len);
}

// The tracks of a workgroup by status: cleared, counted in LDS, then one atomic per status that occurred into counts.
__device__ __forceinline__ void tally_clear(int (&s_cnt)[SFM_TRI_STATUS_COUNT]) {
  if (threadIdx.x < SFM_TRI_STATUS_COUNT) s_cnt[threadIdx.x] = 0;
  __syncthreads();
}
__device__ __forceinline__ void tally_add(int (&s_cnt)[SFM_TRI_STATUS_COUNT], int st) { atomicAdd(&s_cnt[st], 1); }
__device__ __forceinline__ void tally_flush(int (&s_cnt)[SFM_TRI_STATUS_COUNT], unsigned long long* __restrict__ counts) {
  __syncthreads();
  if (threadIdx.x < SFM_TRI_STATUS_COUNT && s_cnt[threadIdx.x])
    atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// Robust = false: n_inliers, obs_inlier, list and list_count are not used (the plain call passes null).
template <bool Robust>
__global__ __launch_bounds__(256) void k_tri_tracks(TrackSrc src, const int64_t* __restrict__ track_ptr, int64_t n_tracks,
                                                    int64_t n_obs, Gates g, double* __restrict__ X, int* __restrict__ status,
                                                    int* __restrict__ n_views, int* __restrict__ n_inliers,
                                                    double* __restrict__ max_err, uint8_t* __restrict__ obs_inlier,
                                                    unsigned long long* __restrict__ counts, int* __restrict__ list,
                                                    int* __restrict__ list_count) {
  __shared__ int s_cnt[SFM_TRI_STATUS_COUNT];
  tally_clear(s_cnt);
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool push = false;
  if (t < n_tracks) {
    int64_t lo;
    int n_raw;
    track_range(track_ptr, t, n_obs, lo, n_raw);
    src.b = lo;
    double Xt[3], me;
    int nv;
    const int st = tri::solve(src, n_raw, g.min_views, g.refine_iters, g.max_error, g.check_angle != 0, g.cos_min_angle, Xt,
                              nv, me);
    X[3 * t] = Xt[0]; X[3 * t + 1] = Xt[1]; X[3 * t + 2] = Xt[2];
    status[t] = st;
    n_views[t] = nv;
    max_err[t] = me;
    if constexpr (Robust) {
      n_inliers[t] = st == SFM_TRI_OK ? nv : 0;
      if (st == SFM_TRI_OK) {                                     // the call zeroed the flags
        int img;
        for (int k = 0; k < n_raw; ++k)
          if (src.camera(k, img) >= 0) obs_inlier[lo + k] = 1;
      } else {
        int n_used, s;
        tri::count_views(src, n_raw, n_used, s);
        push = s >= 4;
      }
    }
    tally_add(s_cnt, st);
  }
  if constexpr (Robust) {
    // every lane of the wavefront is here again.  Every track is pushed at most once: a slot stays below n_tracks.
    const unsigned long long flagged = __ballot(push);
    if (flagged) {
      const int lane = threadIdx.x & 63, leader = __ffsll((long long)flagged) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(list_count, __popcll(flagged));
      base = __shfl(base, leader, 64);
      if (push) list[base + __popcll(flagged & ((1ull << lane) - 1ull))] = (int)t;
    }
  }
  tally_flush(s_cnt, counts);
}

__global__ __launch_bounds__(256) void k_robust_rescue(TrackSrc src, const int64_t* __restrict__ track_ptr, int64_t n_tracks,
                                                       int64_t n_obs, Gates g, double* __restrict__ X,
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
    if (lane < n_hyp) score = tri::hypothesis(src, n_raw, s, g.max_error, g.check_angle != 0, g.cos_min_angle, lane, Xh);
    // the winner: highest score, ties to the lowest lane
    long long key = ((long long)score << 6) | (long long)(63 - lane);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const long long other = __shfl_xor(key, d, 64);
      key = other > key ? other : key;
    }
    const int best = (int)(key >> 6), winner = 63 - (int)(key & 63);
    if (best < (g.min_views < 3 ? 3 : g.min_views)) continue;
    const double Xw[3] = {__shfl(Xh[0], winner, 64), __shfl(Xh[1], winner, 64), __shfl(Xh[2], winner, 64)};
    double Xr[3], me;
    int ni;
    if (!tri::finish(src, n_raw, g.min_views, g.refine_iters, g.max_error, g.check_angle != 0, g.cos_min_angle, Xw, Xr, ni, me))
      continue;
    tri::Obs o;
    for (int k = lane; k < n_raw; k += 64) {
      double err;
      obs_inlier[lo + k] = (src.get(k, o) && tri::agrees(o, Xr, g.max_error, err)) ? 1 : 0;
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

// The gates at the caller's points: same source, same prologue, no solve.  A track without a point only counts its views.
__global__ __launch_bounds__(256) void k_tri_evaluate(TrackSrc src, const int64_t* __restrict__ track_ptr, int64_t n_tracks,
                                                      int64_t n_obs, Gates g, const double* __restrict__ X,
                                                      const uint8_t* __restrict__ has_point, int* __restrict__ status,
                                                      int* __restrict__ n_views, double* __restrict__ max_err,
                                                      double* __restrict__ obs_err, unsigned long long* __restrict__ counts) {
  __shared__ int s_cnt[SFM_TRI_STATUS_COUNT];
  tally_clear(s_cnt);
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n_tracks) {
    int64_t lo;
    int n_raw;
    track_range(track_ptr, t, n_obs, lo, n_raw);
    src.b = lo;
    const bool has = has_point[t] != 0;
    const double Xt[3] = {X[3 * t], X[3 * t + 1], X[3 * t + 2]};
    double me = NAN;
    int nv = 0, st = SFM_EVAL_NO_POINT;
    if (has) {
      st = tri::judge(src, n_raw, g.min_views, Xt, g.max_error, g.check_angle != 0, g.cos_min_angle, nv, me);
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
    if (has) tally_add(s_cnt, st);
  }
  tally_flush(s_cnt, counts);
}

// The gates over the observations that agree with the caller's points.  A track without a point only counts its views.
__global__ __launch_bounds__(256) void k_tri_classify(TrackSrc src, const int64_t* __restrict__ track_ptr, int64_t n_tracks,
                                                      int64_t n_obs, Gates g, const double* __restrict__ X,
                                                      const uint8_t* __restrict__ has_point, int* __restrict__ status,
                                                      int* __restrict__ n_views, int* __restrict__ n_inliers,
                                                      double* __restrict__ max_err, uint8_t* __restrict__ obs_inlier,
                                                      double* __restrict__ obs_err, unsigned long long* __restrict__ counts) {
  __shared__ int s_cnt[SFM_TRI_STATUS_COUNT];
  tally_clear(s_cnt);
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
    if (has) st = tri::classify(src, n_raw, g.min_views, Xt, g.max_error, g.check_angle != 0, g.cos_min_angle, ni, me);
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
          in = tri::sound(o) && hw > 0.0 && e <= g.max_error;
        }
      }
      obs_inlier[lo + k] = in ? 1 : 0;
      if (obs_err) obs_err[lo + k] = e;
    }
    status[t] = st;
    n_views[t] = nv;
    n_inliers[t] = ni;
    max_err[t] = me;
    if (has) tally_add(s_cnt, st);
  }
  tally_flush(s_cnt, counts);
}

// What track_call_begin leaves to the entry point: the source, the gates and the workspace behind the camera centres.
struct TrackCall {
  TrackSrc src;
  Gates g;
  ws_carve ws;
};

// The frame of the four entry points below, in the order their callers rely on: sizes and options (SFM_ERR_ARG, nothing
// touched), counts zeroed, n_tracks == 0 (SFM_OK: the entry point returns), pointers (own_ok: the entry point's own),
// workspace (need_bytes: what its *_workspace_bytes reports), then the camera centres are on their way and c is filled.
// A call that judges a given point has no refine_iters and passes 0.
int track_call_begin(sfm_handle h, const char* name, const double* proj, int32_t n_cams, const int32_t* cam_of_image,
                     int32_t n_img, const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes, const int64_t* track_ptr,
                     int64_t n_tracks, const int32_t* obs_image, const int32_t* obs_kp, int64_t n_obs, int32_t min_views,
                     int32_t refine_iters, double max_error, double min_angle_deg, int64_t* counts, bool own_ok,
                     void* workspace, int64_t workspace_bytes, int64_t need_bytes, TrackCall& c) {
  if (!h) return SFM_ERR_ARG;
  if (n_cams < 0 || n_img < 0 || n_nodes < 0 || n_tracks < 0 || n_obs < 0 || n_tracks > 0x3fffffffLL)
    return sfm_fail(h, SFM_ERR_ARG, name, "bad argument");
  if (min_views < 2) return sfm_fail(h, SFM_ERR_ARG, name, "min_views must be at least 2");
  if (refine_iters < 0) return sfm_fail(h, SFM_ERR_ARG, name, "refine_iters must not be negative");
  if (!(max_error >= 0.0) || !(min_angle_deg >= 0.0) || !(min_angle_deg <= 180.0))
    return sfm_fail(h, SFM_ERR_ARG, name, "max_error / min_angle_deg out of range");
  if (!counts) return sfm_fail(h, SFM_ERR_ARG, name, "null pointer");
  SFM_HIP(h, hipMemsetAsync(counts, 0, SFM_TRI_STATUS_COUNT * sizeof(int64_t), h->stream));
  if (n_tracks == 0) return SFM_OK;
  if (!track_ptr || !own_ok || !workspace || (n_obs > 0 && (!obs_image || !obs_kp || !kp_ptr)) || (n_cams > 0 && !proj) ||
      (n_img > 0 && !cam_of_image) || (n_nodes > 0 && !kp_xy))
    return sfm_fail(h, SFM_ERR_ARG, name, "null pointer");
  if (workspace_bytes < need_bytes) return sfm_fail(h, SFM_ERR_WORKSPACE, name, "workspace too small");
  c.ws = ws_carve{(char*)workspace};
  double* centres = c.ws.take<double>(3 * (int64_t)n_cams);
  if (n_cams > 0)
    hipLaunchKernelGGL(k_camera_centres, dim3(cdiv(n_cams, 256)), dim3(256), 0, h->stream, proj, n_cams, centres);
  c.src.proj = proj; c.src.centres = centres; c.src.cam_of_image = cam_of_image; c.src.kp_ptr = kp_ptr;
  c.src.kp_xy = (const double2*)kp_xy; c.src.obs_image = obs_image; c.src.obs_kp = obs_kp;
  c.src.n_nodes = n_nodes; c.src.b = 0; c.src.n_cams = n_cams; c.src.n_img = n_img;
  c.g.max_error = max_error;
  c.g.cos_min_angle = cos(min_angle_deg * (3.14159265358979323846 / 180.0));
  c.g.min_views = min_views; c.g.refine_iters = refine_iters; c.g.check_angle = min_angle_deg > 0.0 ? 1 : 0;
  return SFM_OK;
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

extern "C" int sfm_triangulate_tracks_robust_workspace_bytes(int32_t n_cams, int64_t n_tracks, int64_t* bytes_host) {
  if (!bytes_host || n_cams < 0 || n_tracks < 0 || n_tracks > 0x3fffffffLL) return SFM_ERR_ARG;
  ws_carve ws{nullptr};
  ws.take<double>(3 * (int64_t)n_cams);
  ws.take<int>(n_tracks);
  ws.take<int>(1);
  *bytes_host = ws.bytes();
  return SFM_OK;
}

extern "C" int sfm_triangulate_tracks(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam_of_image,
                                      int32_t n_img, const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes,
                                      const int64_t* track_ptr, int64_t n_tracks, const int32_t* obs_image,
                                      const int32_t* obs_kp, int64_t n_obs, int32_t min_views, int32_t refine_iters,
                                      double max_error, double min_angle_deg, double* X, int32_t* status, int32_t* n_views,
                                      double* max_err, int64_t* counts, void* workspace, int64_t workspace_bytes) {
  const char* me = "sfm_triangulate_tracks";
  int64_t need = 0;
  sfm_triangulate_tracks_workspace_bytes(n_cams, &need);
  TrackCall c;
  const int rc = track_call_begin(h, me, proj, n_cams, cam_of_image, n_img, kp_ptr, kp_xy, n_nodes, track_ptr, n_tracks,
                                  obs_image, obs_kp, n_obs, min_views, refine_iters, max_error, min_angle_deg, counts,
                                  X && status && n_views && max_err, workspace, workspace_bytes, need, c);
  if (rc != SFM_OK || n_tracks == 0) return rc;
  hipLaunchKernelGGL(k_tri_tracks<false>, dim3(cdiv(n_tracks, 256)), dim3(256), 0, h->stream, c.src, track_ptr, n_tracks,
                     n_obs, c.g, X, status, n_views, (int*)nullptr, max_err, (uint8_t*)nullptr, (unsigned long long*)counts,
                     (int*)nullptr, (int*)nullptr);
  SFM_LAUNCH_CHECK(h, me);
  return SFM_OK;
}

extern "C" int sfm_tracks_evaluate(sfm_handle h, const double* proj, int32_t n_cams, const int32_t* cam_of_image, int32_t n_img,
                                   const int64_t* kp_ptr, const double* kp_xy, int64_t n_nodes, const int64_t* track_ptr,
                                   int64_t n_tracks, const int32_t* obs_image, const int32_t* obs_kp, int64_t n_obs,
                                   const double* X, const uint8_t* has_point, int32_t min_views, double max_error,
                                   double min_angle_deg, int32_t* status, int32_t* n_views, double* max_err, double* obs_err,
                                   int64_t* counts, void* workspace, int64_t workspace_bytes) {
  const char* me = "sfm_tracks_evaluate";
  int64_t need = 0;
  sfm_triangulate_tracks_workspace_bytes(n_cams, &need);
  TrackCall c;
  const int rc = track_call_begin(h, me, proj, n_cams, cam_of_image, n_img, kp_ptr, kp_xy, n_nodes, track_ptr, n_tracks,
                                  obs_image, obs_kp, n_obs, min_views, 0, max_error, min_angle_deg, counts,
                                  X && has_point && status && n_views && max_err, workspace, workspace_bytes, need, c);
  if (rc != SFM_OK || n_tracks == 0) return rc;
  hipLaunchKernelGGL(k_tri_evaluate, dim3(cdiv(n_tracks, 256)), dim3(256), 0, h->stream, c.src, track_ptr, n_tracks, n_obs,
                     c.g, X, has_point, status, n_views, max_err, obs_err, (unsigned long long*)counts);
  SFM_LAUNCH_CHECK(h, me);
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
  int64_t need = 0;
  sfm_triangulate_tracks_robust_workspace_bytes(n_cams, n_tracks, &need);
  TrackCall c;
  const int rc = track_call_begin(h, me, proj, n_cams, cam_of_image, n_img, kp_ptr, kp_xy, n_nodes, track_ptr, n_tracks,
                                  obs_image, obs_kp, n_obs, min_views, refine_iters, max_error, min_angle_deg, counts,
                                  X && status && n_views && n_inliers && max_err && (n_obs == 0 || obs_inlier), workspace,
                                  workspace_bytes, need, c);
  if (rc != SFM_OK || n_tracks == 0) return rc;
  int* list = c.ws.take<int>(n_tracks);
  int* list_count = c.ws.take<int>(1);
  SFM_HIP(h, hipMemsetAsync(list_count, 0, sizeof(int), h->stream));
  if (n_obs > 0) SFM_HIP(h, hipMemsetAsync(obs_inlier, 0, (size_t)n_obs, h->stream));      // also where no track covers an observation
  hipLaunchKernelGGL(k_tri_tracks<true>, dim3(cdiv(n_tracks, 256)), dim3(256), 0, h->stream, c.src, track_ptr, n_tracks,
                     n_obs, c.g, X, status, n_views, n_inliers, max_err, obs_inlier, (unsigned long long*)counts, list,
                     list_count);
  // four wavefronts per workgroup, at most one wavefront per track, and no more than fill the device several times over
  const unsigned blocks = cdiv(n_tracks, 4) < 2048u ? cdiv(n_tracks, 4) : 2048u;
  hipLaunchKernelGGL(k_robust_rescue, dim3(blocks), dim3(256), 0, h->stream, c.src, track_ptr, n_tracks, n_obs, c.g, X, status,
                     n_inliers, max_err, obs_inlier, (unsigned long long*)counts, (const int*)list, (const int*)list_count);
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
  int64_t need = 0;
  sfm_triangulate_tracks_workspace_bytes(n_cams, &need);
  TrackCall c;
  const int rc = track_call_begin(h, me, proj, n_cams, cam_of_image, n_img, kp_ptr, kp_xy, n_nodes, track_ptr, n_tracks,
                                  obs_image, obs_kp, n_obs, min_views, 0, max_error, min_angle_deg, counts,
                                  X && has_point && status && n_views && n_inliers && max_err && (n_obs == 0 || obs_inlier),
                                  workspace, workspace_bytes, need, c);
  if (rc != SFM_OK || n_tracks == 0) return rc;
  if (n_obs > 0) SFM_HIP(h, hipMemsetAsync(obs_inlier, 0, (size_t)n_obs, h->stream));
  hipLaunchKernelGGL(k_tri_classify, dim3(cdiv(n_tracks, 256)), dim3(256), 0, h->stream, c.src, track_ptr, n_tracks, n_obs,
                     c.g, X, has_point, status, n_views, n_inliers, max_err, obs_inlier, obs_err, (unsigned long long*)counts);
  SFM_LAUNCH_CHECK(h, me);
  return SFM_OK;
}
