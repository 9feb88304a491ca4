// What the triangulation kernels share (triangulate.hip, triangulate_robust.hip), gfx950 only:
//   k_camera_centres   prologue, one thread per camera: C = -M^-1 p4 into the workspace
//   TrackSrc           the observation source of tri::solve over one track's CSR range
// Each translation unit gets its own copy (anonymous namespace).  No FMA contraction, as in triangulate_solve.h.
#pragma once
#include "common.h"
#include "triangulate_solve.h"

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

}  // namespace
