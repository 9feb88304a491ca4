// The 2D-3D correspondences of every unregistered image, taken from the tracks by index (sfm_tracks_resection of
// include/sfm_amd.h, gfx950 only): what the PnP stage consumes, and its per-image counts are the next-best-view score.
// A stream compaction over the nodes, integers only, so the output has one byte pattern:
//   k_resect_flag      one lane per node: the listing rule; the ballot of each wavefront (one 64-bit word) and the number
//                      of listed nodes of each workgroup go to the workspace
//   k_resect_scan      exclusive scan in place of the workgroup sums by one workgroup (scan_counts of block_scan.h); the total
//   k_resect_scatter   one lane per node: slot = workgroup offset + popcounts of the ballots of the wavefronts before it
//                      + popcount of its own ballot below its lane; entries below cap_corr are written
//   k_resect_segments  one lane per image boundary: seg_ptr[i] = listed nodes below kp_ptr[i], from the same words
// Nothing is read back between the launches and the stream is not synchronised.
#include "common.h"
#include "resection_plan.h"
#include "block_scan.h"

namespace {

// largest s in [0, n) with ptr[s] <= i (skips empty ranges); the caller checks i against ptr[s] and ptr[s + 1]
__device__ __forceinline__ int range_of(const int64_t* __restrict__ ptr, int n, int64_t i) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(RESECT_BLOCK) void k_resect_flag(const int64_t* __restrict__ kp_ptr, int n_img, int64_t n_nodes,
                                                              const int32_t* __restrict__ node_track,
                                                              const int32_t* __restrict__ cam_of_image,
                                                              const uint8_t* __restrict__ has_point, int64_t n_tracks,
                                                              unsigned long long* __restrict__ mask, int* __restrict__ blk) {
  __shared__ int s_w[RESECT_WAVES];
  const int64_t n = (int64_t)blockIdx.x * RESECT_BLOCK + threadIdx.x;
  bool f = false;
  if (n < n_nodes) {
    const int i = range_of(kp_ptr, n_img, n);
    if (kp_ptr[i] <= n && n < kp_ptr[i + 1] && cam_of_image[i] < 0) {
      const int t = node_track[n];
      f = t >= 0 && t < n_tracks && has_point[t] != 0;
    }
  }
  const unsigned long long word = __ballot(f);
  if ((threadIdx.x & 63) == 0) mask[(int64_t)blockIdx.x * RESECT_WAVES + (threadIdx.x >> 6)] = word;
  const int sum = block_flag_count<RESECT_BLOCK>(f, s_w);
  if (threadIdx.x == 0) blk[blockIdx.x] = sum;
}

// exclusive scan in place of the n workgroup sums by one workgroup; blk[n] and *total get the sum
__global__ __launch_bounds__(256) void k_resect_scan(int n, int* blk, int64_t* __restrict__ total) {
  __shared__ int64_t s_wave[4];
  int64_t sum;
  scan_counts<256>(n, blk, blk, s_wave, &sum);
  if (threadIdx.x == 0) { blk[n] = (int)sum; *total = sum; }
}

// listed nodes below node p (0 <= p <= n_nodes), from the scanned workgroup sums and the ballots
__device__ __forceinline__ int64_t listed_below(const unsigned long long* __restrict__ mask, const int* __restrict__ blk,
                                                int64_t n_nodes, int64_t p) {
  if (p >= n_nodes) return blk[(n_nodes + RESECT_BLOCK - 1) / RESECT_BLOCK];
  const int64_t b = p / RESECT_BLOCK;
  const int w = (int)(p % RESECT_BLOCK) >> 6, lane = (int)(p & 63);
  int64_t k = blk[b];
  for (int q = 0; q < w; ++q) k += __popcll(mask[b * RESECT_WAVES + q]);
  return k + __popcll(mask[b * RESECT_WAVES + w] & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(RESECT_BLOCK) void k_resect_scatter(int64_t n_nodes, const double2* __restrict__ kp_xy,
                                                                 const int32_t* __restrict__ node_track,
                                                                 const unsigned long long* __restrict__ X,
                                                                 const unsigned long long* __restrict__ mask,
                                                                 const int* __restrict__ blk, int32_t* __restrict__ corr_node,
                                                                 int32_t* __restrict__ corr_track,
                                                                 unsigned long long* __restrict__ corr_X,
                                                                 float2* __restrict__ corr_uv, int64_t cap_corr) {
  const int64_t n = (int64_t)blockIdx.x * RESECT_BLOCK + threadIdx.x;
  if (n >= n_nodes) return;
  if (!((mask[n >> 6] >> (n & 63)) & 1ull)) return;
  const int64_t k = listed_below(mask, blk, n_nodes, n);
  if (k >= cap_corr) return;
  const int t = node_track[n];                      // in [0, n_tracks): the flag says so
  corr_node[k] = (int32_t)n;
  corr_track[k] = t;
  corr_X[3 * k] = X[3 * (int64_t)t]; corr_X[3 * k + 1] = X[3 * (int64_t)t + 1]; corr_X[3 * k + 2] = X[3 * (int64_t)t + 2];
  const double2 xy = kp_xy[n];
  corr_uv[k] = make_float2((float)xy.x, (float)xy.y);
}

__global__ __launch_bounds__(256) void k_resect_segments(const int64_t* __restrict__ kp_ptr, int n_img, int64_t n_nodes,
                                                         const unsigned long long* __restrict__ mask,
                                                         const int* __restrict__ blk, int64_t* __restrict__ seg_ptr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n_img) return;
  int64_t p = i == n_img ? n_nodes : kp_ptr[i];
  p = p < 0 ? 0 : (p > n_nodes ? n_nodes : p);
  seg_ptr[i] = listed_below(mask, blk, n_nodes, p);
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_resection_workspace_bytes(int64_t n_nodes, int64_t* bytes_host) {
  if (!bytes_host || n_nodes < 0 || n_nodes >= ((int64_t)1 << 31)) return SFM_ERR_ARG;
  *bytes_host = resect_plan_layout(n_nodes).bytes;
  return SFM_OK;
}

extern "C" int sfm_tracks_resection(sfm_handle h, const int64_t* kp_ptr, int32_t n_img, int64_t n_nodes, const double* kp_xy,
                                    const int32_t* node_track, const int32_t* cam_of_image, const double* X,
                                    const uint8_t* has_point, int64_t n_tracks, int64_t* seg_ptr, int32_t* corr_node,
                                    int32_t* corr_track, double* corr_X, float* corr_uv, int64_t cap_corr, int64_t* total,
                                    void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  static const char* const rule[] = {"", "negative size", "n_nodes must be below 2^31", "nodes without images"};
  const int why = resect_check_sizes(n_img, n_nodes, n_tracks, cap_corr);
  if (why) return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_resection", rule[why]);
  if (!seg_ptr || !total) return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_resection", "null pointer");
  if (n_nodes == 0) {
    SFM_HIP(h, hipMemsetAsync(seg_ptr, 0, ((size_t)n_img + 1) * sizeof(int64_t), h->stream));
    SFM_HIP(h, hipMemsetAsync(total, 0, sizeof(int64_t), h->stream));
    return SFM_OK;
  }
  if (!kp_ptr || !node_track || !cam_of_image || !workspace || (n_tracks > 0 && (!has_point || !X)) ||
      (cap_corr > 0 && (!kp_xy || !corr_node || !corr_track || !corr_X || !corr_uv)))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_resection", "null pointer");
  const resect_layout L = resect_plan_layout(n_nodes);
  if (workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_resection", "workspace too small");
  unsigned long long* mask = (unsigned long long*)((char*)workspace + L.mask);
  int* blk = (int*)((char*)workspace + L.blk);
  const int64_t blocks = resect_blocks(n_nodes);
  const dim3 tb(RESECT_BLOCK), gn((unsigned)blocks);
  hipLaunchKernelGGL(k_resect_flag, gn, tb, 0, h->stream, kp_ptr, (int)n_img, n_nodes, node_track, cam_of_image, has_point,
                     n_tracks, mask, blk);
  hipLaunchKernelGGL(k_resect_scan, dim3(1), dim3(256), 0, h->stream, (int)blocks, blk, total);
  if (cap_corr > 0)
    hipLaunchKernelGGL(k_resect_scatter, gn, tb, 0, h->stream, n_nodes, (const double2*)kp_xy, node_track,
                       (const unsigned long long*)X, (const unsigned long long*)mask, (const int*)blk, corr_node, corr_track,
                       (unsigned long long*)corr_X, (float2*)corr_uv, cap_corr);
  hipLaunchKernelGGL(k_resect_segments, dim3(cdiv((int64_t)n_img + 1, 256)), dim3(256), 0, h->stream, kp_ptr, (int)n_img,
                     n_nodes, (const unsigned long long*)mask, (const int*)blk, seg_ptr);
  SFM_LAUNCH_CHECK(h, "sfm_tracks_resection");
  return SFM_OK;
}
