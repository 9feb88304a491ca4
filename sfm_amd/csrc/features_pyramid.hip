// Multi-scale features (gfx950 only): the device code on either side of sfm_features_detect / sfm_features_describe when
// they run on a pyramid.  One side builds the level batch - every level of every image as one more image of the batch, by
// the chained 8-bit bilinear rule of include/sfm_amd.h; the other joins the keypoints of an image's levels into one list
// in level-0 coordinates under one max_features cut.  Every byte is integer arithmetic (the coordinate map is one double
// division, rounded once), so the outputs have ONE byte pattern; the order of the survivors comes from a workgroup scan,
// never from an atomic counter.
//
// sfm_features_pyramid
//   k_pyr_copy       level 0: images (and masks) into their slots, 4096 bytes per workgroup
//   k_pyr_level      level l from level l - 1, one launch per level over the tiles of all images: a thread produces 4
//                    adjacent pixels of 4 rows and stores each 4 as one dword; their source pixels, at most 8 per source
//                    row, are one unaligned 8-byte load per row and go through the cache (neighbouring lanes share their
//                    lines; there is no reuse an LDS stage would add to that).
//                    <true> is the mask rule: 1 where all four source pixels are > 0
// sfm_features_merge_count
//   k_merge_cut      per image: 256-bin histogram of the scores of its levels' keypoints, the cut (s, quota), its count
//   k_merge_scan     exclusive scan of the counts over the images -> kp_ptr
// sfm_features_merge_gather
//   k_merge_rank     per image: walks its keypoints in pieces of 1024 with a running carry; the keypoints above s and at s
//                    in front of each come from ONE scan of two packed counters -> src
//   k_merge_gather   8 lanes per kept keypoint: the coordinate map, level, score, angle bin, and the descriptor as 8 dwords
#include "common.h"
#include "features_pyramid_plan.h"
#include "block_scan.h"

namespace {

constexpr int MERGE_ITEMS = 4;                     // consecutive keypoints per thread of k_merge_rank
constexpr int MERGE_PIECE = 256 * MERGE_ITEMS;

// largest i in [0, n) with key(i) <= v
template <typename F> __device__ __forceinline__ int pyr_find(int n, int64_t v, F key) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (key(mid) <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------------ the levels
// blockIdx.y = 0: images, 1: masks
__global__ __launch_bounds__(256) void k_pyr_copy(const pyr_entry* __restrict__ T, int n_img, const uint8_t* __restrict__ images,
                                                  const uint8_t* __restrict__ masks, uint8_t* __restrict__ lvl_images,
                                                  uint8_t* __restrict__ lvl_masks) {
  const int img = pyr_find(n_img, (int64_t)blockIdx.x, [&](int i) { return (int64_t)T[i].tile0; });
  const pyr_entry e = T[img];
  const int64_t n = (int64_t)e.hd * e.wd;
  const int64_t at = (int64_t)((int)blockIdx.x - e.tile0) * PYR_COPY_CHUNK + 16 * (int64_t)threadIdx.x;
  if (at >= n) return;
  const uint8_t* s = (blockIdx.y ? masks : images) + e.src + at;
  uint8_t* d = (blockIdx.y ? lvl_masks : lvl_images) + e.dst + at;
  if (at + 16 <= n && (((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
    *(uint4*)d = *(const uint4*)s;
  } else {
    const int len = (int)min((int64_t)16, n - at);
    for (int k = 0; k < len; ++k) d[k] = s[k];
  }
}

template <bool MASK>
__global__ __launch_bounds__(256) void k_pyr_level(const pyr_entry* __restrict__ T, int n_img, uint8_t* __restrict__ lvl) {
  const int img = pyr_find(n_img, (int64_t)blockIdx.x, [&](int i) { return (int64_t)T[i].tile0; });
  const pyr_entry e = T[img];
  const int t = (int)blockIdx.x - e.tile0;
  const int tx0 = (t % e.tiles_x) * PYR_TILE_W, ty0 = (t / e.tiles_x) * PYR_TILE_H;
  const int x = tx0 + PYR_PX * (int)(threadIdx.x & 63);
  if (x >= e.wd) return;
  const uint8_t* src = lvl + e.src;      // level l - 1: written by the launch before, never by this one
  uint8_t* dst = lvl + e.dst;
  int x0[PYR_PX], x1[PYR_PX], fx[PYR_PX];
#pragma unroll
  for (int q = 0; q < PYR_PX; ++q) pyr_tap(min(x + q, e.wd - 1), e.wd, e.ws, &x0[q], &x1[q], &fx[q]);      // inside the source
  // The scale is at most 2, so the four pixels' taps span at most 8 source pixels (x1[3] <= x0[0] + 7).  Where those 8
  // lie inside the source row they are read as one unaligned 8-byte word per row; at the row's end, byte by byte.
  const bool wide = x0[0] + 8 <= e.ws && x1[PYR_PX - 1] - x0[0] <= 7;
#pragma unroll
  for (int r = 0; r < PYR_TILE_H / 4; ++r) {
    const int y = ty0 + (int)(threadIdx.x >> 6) + 4 * r;
    if (y >= e.hd) break;
    int y0, y1, fy;
    pyr_tap(y, e.hd, e.hs, &y0, &y1, &fy);
    const uint8_t* r0 = src + (int64_t)y0 * e.ws;
    const uint8_t* r1 = src + (int64_t)y1 * e.ws;
    unsigned packed = 0;
    if (wide) {
      uint64_t w0, w1;                    // source pixels x0[0] .. x0[0] + 7 of both rows: two loads instead of sixteen
      __builtin_memcpy(&w0, r0 + x0[0], 8);
      __builtin_memcpy(&w1, r1 + x0[0], 8);
#pragma unroll
      for (int q = 0; q < PYR_PX; ++q) {
        const int s0 = 8 * (x0[q] - x0[0]), s1 = 8 * (x1[q] - x0[0]);
        const int a00 = (int)(w0 >> s0) & 255, a01 = (int)(w0 >> s1) & 255, a10 = (int)(w1 >> s0) & 255, a11 = (int)(w1 >> s1) & 255;
        const int v = MASK ? (int)(a00 > 0 && a01 > 0 && a10 > 0 && a11 > 0) : pyr_blend(fx[q], fy, a00, a01, a10, a11);
        packed |= (unsigned)v << (8 * q);
      }
    } else {
#pragma unroll
      for (int q = 0; q < PYR_PX; ++q) {
        const int a00 = r0[x0[q]], a01 = r0[x1[q]], a10 = r1[x0[q]], a11 = r1[x1[q]];
        const int v = MASK ? (int)(a00 > 0 && a01 > 0 && a10 > 0 && a11 > 0) : pyr_blend(fx[q], fy, a00, a01, a10, a11);
        packed |= (unsigned)v << (8 * q);
      }
    }
    uint8_t* o = dst + (int64_t)y * e.wd + x;
    if (((uintptr_t)o & 3) == 0 && x + PYR_PX <= e.wd) {
      *(unsigned*)o = packed;
    } else {
      for (int q = 0; q < PYR_PX; ++q)
        if (x + q < e.wd) o[q] = (uint8_t)(packed >> (8 * q));
    }
  }
}

// -------------------------------------------------------------------------------------------------------- the merge
struct merge_dev {
  int* dims;
  int* cut;
  int* cnt;
};

// The keypoints of image i are the segment lvl_kp_ptr[i L] .. lvl_kp_ptr[(i + 1) L] of the level batch's list: level
// ascending, row-major within a level - the order of the contract already.  cut[i] = (s, quota) by k_feat_cut's rule over
// that segment; cnt[i] = what stays.
__global__ __launch_bounds__(256) void k_merge_cut(merge_dev w, const int64_t* __restrict__ lvl_kp_ptr,
                                                   const uint8_t* __restrict__ lvl_score, int n_levels, int max_features) {
  __shared__ unsigned hist[256];
  const int img = blockIdx.x;
  const int64_t a = lvl_kp_ptr[(int64_t)img * n_levels], b = lvl_kp_ptr[(int64_t)(img + 1) * n_levels];
  hist[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t k = a + threadIdx.x; k < b; k += 256) atomicAdd(&hist[lvl_score[k]], 1u);      // counts: the order is immaterial
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int64_t total = b - a;
  int s = 0, quota = 0;
  int64_t kept = total;
  if (max_features > 0 && total > max_features) {
    int64_t above = 0;
    for (int v = 255; v >= 1; --v) {
      if (above + hist[v] >= max_features) { s = v; quota = (int)(max_features - above); break; }
      above += hist[v];
    }
    kept = max_features;
  }
  w.cut[2 * img] = s;
  w.cut[2 * img + 1] = quota;
  w.cnt[img] = (int)kept;
}

__global__ __launch_bounds__(256) void k_merge_scan(merge_dev w, int n_img, int64_t* __restrict__ kp_ptr) {
  __shared__ int64_t part[4];
  int64_t total;
  scan_counts<256>(n_img, w.cnt, w.cnt, part, &total);
  __syncthreads();                        // the bases this workgroup wrote are visible to all of its threads
  for (int i = threadIdx.x; i <= n_img; i += 256) kp_ptr[i] = i < n_img ? (int64_t)w.cnt[i] : total;
}

__global__ __launch_bounds__(256) void k_merge_rank(merge_dev w, const int64_t* __restrict__ lvl_kp_ptr,
                                                    const uint8_t* __restrict__ lvl_score, int n_levels,
                                                    const int64_t* __restrict__ kp_ptr, int64_t n_kp, int32_t* __restrict__ src) {
  __shared__ int64_t part[4];
  const int img = blockIdx.x;
  const int64_t a = lvl_kp_ptr[(int64_t)img * n_levels], b = lvl_kp_ptr[(int64_t)(img + 1) * n_levels];
  const int s = w.cut[2 * img], quota = w.cut[2 * img + 1];
  const int64_t out0 = kp_ptr[img];
  int64_t carry = 0;                      // high half: keypoints above s so far, low half: keypoints at s so far
  for (int64_t base = a; base < b; base += MERGE_PIECE) {        // uniform over the workgroup: every thread meets the scan
    const int64_t k0 = base + MERGE_ITEMS * (int64_t)threadIdx.x;
    int v[MERGE_ITEMS];
    int64_t mine = 0;
#pragma unroll
    for (int j = 0; j < MERGE_ITEMS; ++j) {
      v[j] = k0 + j < b ? (int)lvl_score[k0 + j] : 0;          // a keypoint's score is at least 1: 0 is neither above nor a tie
      mine += v[j] > s ? ((int64_t)1 << 32) : (v[j] == s && s > 0) ? (int64_t)1 : (int64_t)0;
    }
    int64_t total;
    int64_t before = carry + block_exclusive_scan<256, int64_t>(mine, part, &total);
#pragma unroll
    for (int j = 0; j < MERGE_ITEMS; ++j) {
      const int64_t above = before >> 32, ties = before & 0xffffffff;
      const bool tie = v[j] == s && s > 0;
      const bool keep = v[j] > s || (tie && ties < quota);
      const int64_t p = out0 + above + min(ties, (int64_t)quota);
      if (keep && p < n_kp) src[p] = (int32_t)(k0 + j);
      before += v[j] > s ? ((int64_t)1 << 32) : tie ? (int64_t)1 : (int64_t)0;
    }
    carry += total;
  }
}

__global__ __launch_bounds__(256) void k_merge_gather(merge_dev w, const int64_t* __restrict__ lvl_kp_ptr,
                                                      const int32_t* __restrict__ lvl_xy, const uint8_t* __restrict__ lvl_score,
                                                      const uint8_t* __restrict__ lvl_bin, const uint32_t* __restrict__ lvl_desc,
                                                      int n_img, int n_levels, const int64_t* __restrict__ kp_ptr, int64_t n_kp,
                                                      const int32_t* __restrict__ src, float* __restrict__ xy,
                                                      uint8_t* __restrict__ level, uint8_t* __restrict__ score,
                                                      uint8_t* __restrict__ bin, uint32_t* __restrict__ desc) {
  const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int part = threadIdx.x & 7;
  if (p >= n_kp) return;
  const int64_t k = src[p];
  desc[p * 8 + part] = lvl_desc[k * 8 + part];
  if (part != 0) return;
  const int img = pyr_find(n_img, p, [&](int i) { return kp_ptr[i]; });
  const int64_t* lp = lvl_kp_ptr + (int64_t)img * n_levels;
  const int l = pyr_find(n_levels, k, [&](int i) { return lp[i]; });
  const int* d0 = w.dims + 2 * ((int64_t)img * n_levels);
  const int* dl = d0 + 2 * l;
  xy[2 * p] = pyr_map(lvl_xy[2 * k], d0[1], dl[1]);
  xy[2 * p + 1] = pyr_map(lvl_xy[2 * k + 1], d0[0], dl[0]);
  level[p] = (uint8_t)l;
  score[p] = lvl_score[k];
  bin[p] = lvl_bin[k];
}

merge_dev merge_carve(void* workspace, const merge_layout& L) {
  char* p = (char*)workspace;
  merge_dev w;
  w.dims = (int*)(p + L.dims);
  w.cut = (int*)(p + L.cut);
  w.cnt = (int*)(p + L.cnt);
  return w;
}

int merge_check(int64_t n_img, int64_t n_levels) {
  if (n_levels < 2 || n_levels > PYR_MAX_LEVELS) return 1;
  if (n_img < 0 || n_img * n_levels >= (1 << 24)) return 5;
  return 0;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_features_pyramid_sizes(int32_t n_img, const int32_t* heights, const int32_t* widths, int32_t n_levels,
                                          int32_t num, int32_t den, int64_t* lvl_off, int32_t* lvl_heights,
                                          int32_t* lvl_widths) {
  return pyr_plan_sizes(n_img, heights, widths, n_levels, num, den, lvl_off, lvl_heights, lvl_widths) ? SFM_ERR_ARG : SFM_OK;
}

extern "C" int sfm_features_pyramid_workspace_bytes(int32_t n_img, int32_t n_levels, int64_t* bytes_host) {
  if (!bytes_host || merge_check(n_img, n_levels)) return SFM_ERR_ARG;
  *bytes_host = pyr_plan_layout(n_img, n_levels).bytes;
  return SFM_OK;
}

extern "C" int sfm_features_pyramid(sfm_handle h, const uint8_t* images, const uint8_t* masks, const int64_t* img_off,
                                    const int32_t* heights, const int32_t* widths, int32_t n_img, int32_t n_levels,
                                    int32_t num, int32_t den, uint8_t* lvl_images, uint8_t* lvl_masks, void* workspace,
                                    int64_t workspace_bytes) {
  static const char* const fn = "sfm_features_pyramid";
  if (!h) return SFM_ERR_ARG;
  int why = pyr_check_options(n_levels, num, den);
  if (why) return sfm_fail(h, SFM_ERR_ARG, fn, pyr_rule_text(why));
  why = feat_check_images(n_img, img_off, heights, widths);
  if (why) return sfm_fail(h, SFM_ERR_ARG, fn, feat_rule_text(why));
  if ((int64_t)n_img * n_levels >= (1 << 24)) return sfm_fail(h, SFM_ERR_ARG, fn, pyr_rule_text(5));
  if ((masks == nullptr) != (lvl_masks == nullptr))
    return sfm_fail(h, SFM_ERR_ARG, fn, "masks and lvl_masks must both be given or both be null");
  if (n_img == 0) return SFM_OK;
  const size_t slots = (size_t)n_img * (size_t)n_levels;
  std::vector<int64_t> lvl_off(slots + 1);
  std::vector<int32_t> lvl_h(slots), lvl_w(slots);
  why = pyr_plan_sizes(n_img, heights, widths, n_levels, num, den, lvl_off.data(), lvl_h.data(), lvl_w.data());
  if (why) return sfm_fail(h, SFM_ERR_ARG, fn, pyr_rule_text(why));
  const pyr_plan P = pyr_plan_tiles(n_img, img_off, n_levels, lvl_off.data(), lvl_h.data(), lvl_w.data());
  const pyr_layout L = pyr_plan_layout(n_img, n_levels);
  if (!workspace || workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_ARG, fn, "workspace too small");
  if (P.pixels > 0 && (!images || !lvl_images)) return sfm_fail(h, SFM_ERR_ARG, fn, "null pointer");
  if (P.pixels == 0) return SFM_OK;
  const pyr_entry* T = (const pyr_entry*)((char*)workspace + L.table);
  SFM_HIP(h, hipMemcpyAsync((void*)T, P.entry.data(), P.entry.size() * sizeof(pyr_entry), hipMemcpyHostToDevice, h->stream));
  if (P.tiles[0] > 0)
    hipLaunchKernelGGL(k_pyr_copy, dim3((unsigned)P.tiles[0], masks ? 2 : 1), dim3(256), 0, h->stream, T, (int)n_img, images,
                       masks, lvl_images, lvl_masks);
  for (int l = 1; l < n_levels; ++l) {
    if (P.tiles[(size_t)l] == 0) continue;
    const pyr_entry* Tl = T + (size_t)l * (size_t)n_img;
    hipLaunchKernelGGL(k_pyr_level<false>, dim3((unsigned)P.tiles[(size_t)l]), dim3(256), 0, h->stream, Tl, (int)n_img, lvl_images);
    if (masks)
      hipLaunchKernelGGL(k_pyr_level<true>, dim3((unsigned)P.tiles[(size_t)l]), dim3(256), 0, h->stream, Tl, (int)n_img, lvl_masks);
  }
  SFM_LAUNCH_CHECK(h, fn);
  return SFM_OK;
}

extern "C" int sfm_features_merge_workspace_bytes(int32_t n_img, int32_t n_levels, int64_t* bytes_host) {
  if (!bytes_host || merge_check(n_img, n_levels)) return SFM_ERR_ARG;
  *bytes_host = merge_plan_layout(n_img, n_levels).bytes;
  return SFM_OK;
}

extern "C" int sfm_features_merge_count(sfm_handle h, const int64_t* lvl_kp_ptr, const uint8_t* lvl_score, int32_t n_img,
                                        int32_t n_levels, int32_t max_features, int64_t* kp_ptr, void* workspace,
                                        int64_t workspace_bytes) {
  static const char* const fn = "sfm_features_merge_count";
  if (!h) return SFM_ERR_ARG;
  const int why = merge_check(n_img, n_levels);
  if (why) return sfm_fail(h, SFM_ERR_ARG, fn, pyr_rule_text(why));
  if (max_features < 0) return sfm_fail(h, SFM_ERR_ARG, fn, feat_rule_text(3));
  if (!kp_ptr || (n_img > 0 && !lvl_kp_ptr)) return sfm_fail(h, SFM_ERR_ARG, fn, "null pointer");
  if (n_img == 0) {
    SFM_HIP(h, hipMemsetAsync(kp_ptr, 0, sizeof(int64_t), h->stream));
    return SFM_OK;
  }
  const merge_layout L = merge_plan_layout(n_img, n_levels);
  if (!workspace || workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_ARG, fn, "workspace too small");
  const merge_dev w = merge_carve(workspace, L);
  // lvl_score may be null only when the level batch has no keypoint: then no thread of k_merge_cut reads it
  hipLaunchKernelGGL(k_merge_cut, dim3((unsigned)n_img), dim3(256), 0, h->stream, w, lvl_kp_ptr, lvl_score, (int)n_levels,
                     (int)max_features);
  hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(256), 0, h->stream, w, (int)n_img, kp_ptr);
  SFM_LAUNCH_CHECK(h, fn);
  return SFM_OK;
}

extern "C" int sfm_features_merge_gather(sfm_handle h, const int64_t* lvl_kp_ptr, const int32_t* lvl_xy,
                                         const uint8_t* lvl_score, const uint8_t* lvl_angle_bin, const uint8_t* lvl_desc,
                                         const int32_t* lvl_heights, const int32_t* lvl_widths, int32_t n_img,
                                         int32_t n_levels, const int64_t* kp_ptr, int64_t n_kp, float* xy, uint8_t* level,
                                         uint8_t* score, uint8_t* angle_bin, uint8_t* desc, int32_t* src, void* workspace,
                                         int64_t workspace_bytes) {
  static const char* const fn = "sfm_features_merge_gather";
  if (!h) return SFM_ERR_ARG;
  const int why = merge_check(n_img, n_levels);
  if (why) return sfm_fail(h, SFM_ERR_ARG, fn, pyr_rule_text(why));
  if (n_kp < 0 || n_kp >= ((int64_t)1 << 31)) return sfm_fail(h, SFM_ERR_ARG, fn, "n_kp out of range");
  if (n_kp == 0) return SFM_OK;
  if (n_img == 0 || !lvl_kp_ptr || !lvl_xy || !lvl_score || !lvl_angle_bin || !lvl_desc || !lvl_heights || !lvl_widths ||
      !kp_ptr || !xy || !level || !score || !angle_bin || !desc || !src)
    return sfm_fail(h, SFM_ERR_ARG, fn, "null pointer");
  const size_t slots = (size_t)n_img * (size_t)n_levels;
  for (size_t s = 0; s < slots; ++s)
    if (lvl_heights[s] < 0 || lvl_widths[s] < 0) return sfm_fail(h, SFM_ERR_ARG, fn, pyr_rule_text(7));
  const merge_layout L = merge_plan_layout(n_img, n_levels);
  if (!workspace || workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_ARG, fn, "workspace too small");
  const merge_dev w = merge_carve(workspace, L);
  std::vector<int32_t> dims(2 * slots);
  for (size_t s = 0; s < slots; ++s) { dims[2 * s] = lvl_heights[s]; dims[2 * s + 1] = lvl_widths[s]; }
  SFM_HIP(h, hipMemcpyAsync(w.dims, dims.data(), dims.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_merge_rank, dim3((unsigned)n_img), dim3(256), 0, h->stream, w, lvl_kp_ptr, lvl_score, (int)n_levels,
                     kp_ptr, n_kp, src);
  hipLaunchKernelGGL(k_merge_gather, dim3(cdiv(n_kp * 8, 256)), dim3(256), 0, h->stream, w, lvl_kp_ptr, lvl_xy, lvl_score,
                     lvl_angle_bin, (const uint32_t*)lvl_desc, (int)n_img, (int)n_levels, kp_ptr, n_kp, (const int32_t*)src,
                     xy, level, score, angle_bin, (uint32_t*)desc);
  SFM_LAUNCH_CHECK(h, fn);
  return SFM_OK;
}
