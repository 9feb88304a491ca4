// Dense depth maps by plane-sweep stereo for gfx950 (MI355X): census transform, plane sweep with winner-take-all and a
// sub-plane step, cross-view consistency filter with back-projection.  include/sfm_amd.h states the rule; depth_rule.h
// holds its floating-point pieces (float64, no FMA contraction), depth_plan.h the tables, tiles and checks.
//
// k_depth_sweep is the hot kernel: pixels x planes x sources samples, each a 3 x 4 warp, two float64 divisions, one
// gathered 8-byte census word and a popcount.  One workgroup of 256 threads owns a tile of 32 x 16 reference pixels.  Per
// plane every thread fills its slots of tile plus halo with c_k (uint16) in LDS, the workgroup meets at ONE barrier, and
// every thread box-sums the windows of its two vertically adjacent pixels from LDS: the 2r + 2 row sums they share are
// formed once.  The two LDS planes alternate, so the writes of plane k + 1 cannot reach a buffer that a slower thread
// still reads for plane k - 1: that thread has not passed barrier k yet, and no thread starts plane k + 1 before all have.
// The running minimum, its plane and the sums of the two planes beside it stay in registers; the cost volume never goes
// to memory.  Reference census words and clamped coordinates of a thread's slots are loaded once and kept in registers;
// the warps and source tables of the view sit in LDS and are read at one address by all lanes (a broadcast).
#include "common.h"
#include "depth_rule.h"
#include "depth_plan.h"

#pragma clang fp contract(off)

namespace {

// bit k of the census word, k counting the 7 x 7 offsets row-major with the centre skipped: I(clamp(p + o_k)) < I(p)
__global__ __launch_bounds__(DEPTH_PIXEL_BLOCK) void k_depth_census(const uint8_t* __restrict__ images, const DepthImage* __restrict__ tab,
                                                                    int n_img, int64_t n_elem, uint64_t* __restrict__ census) {
  const int64_t e = (int64_t)blockIdx.x * DEPTH_PIXEL_BLOCK + threadIdx.x;
  if (e >= n_elem) return;
  const DepthImage im = tab[depth_find_image(tab, n_img, e)];
  const int64_t p = e - im.off;
  if (p < 0 || p >= (int64_t)im.h * im.w) return;             // slack of a slot: not a pixel
  const int y = (int)(p / im.w), x = (int)(p % im.w);
  const uint8_t* __restrict__ img = images + im.off;
  const int c = img[p];
  uint64_t word = 0;
  int k = 0;
#pragma unroll
  for (int dy = -3; dy <= 3; ++dy) {
    const int64_t row = (int64_t)depth_clamp(y + dy, im.h - 1) * im.w;
#pragma unroll
    for (int dx = -3; dx <= 3; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const int v = img[row + depth_clamp(x + dx, im.w - 1)];
      word |= (uint64_t)(v < c ? 1 : 0) << k;
      ++k;
    }
  }
  census[e] = word;
}

template <int R>
__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_sweep(const uint64_t* __restrict__ census, const DepthImage* __restrict__ images,
                                                               const DepthView* __restrict__ views, int n_ref,
                                                               const int32_t* __restrict__ src_image, const double* __restrict__ warps,
                                                               const double* __restrict__ planes, int32_t* __restrict__ plane_out,
                                                               uint16_t* __restrict__ cost_out, float* __restrict__ depth_out) {
  constexpr int HW = DEPTH_TW + 2 * R, HH = DEPTH_TH + 2 * R, COUNT = HW * HH;
  constexpr int ROUNDS = (COUNT + DEPTH_THREADS - 1) / DEPTH_THREADS;
  __shared__ uint16_t s_c[2][COUNT];
  __shared__ double s_warp[DEPTH_MAX_SOURCES][12];
  __shared__ int64_t s_off[DEPTH_MAX_SOURCES];
  __shared__ int s_w[DEPTH_MAX_SOURCES], s_h[DEPTH_MAX_SOURCES];
  const int tid = threadIdx.x;
  const DepthView view = views[depth_find_view(views, n_ref, blockIdx.x, DEPTH_BY_TILE)];
  const DepthImage ref = images[view.image];
  const int tile = (int)((int64_t)blockIdx.x - view.tile_first);
  const int x0 = (tile % view.tiles_x) * DEPTH_TW, y0 = (tile / view.tiles_x) * DEPTH_TH;
  const int n_src = view.n_src, n_planes = view.n_planes;
  if (tid < n_src * 12) s_warp[tid / 12][tid % 12] = warps[(int64_t)view.src_first * 12 + tid];
  if (tid < n_src) {
    const DepthImage s = images[src_image[view.src_first + tid]];
    s_off[tid] = s.off; s_w[tid] = s.w; s_h[tid] = s.h;
  }
  // this thread's slots of tile plus halo: the census word and the (clamped) pixel of each, for every plane
  uint64_t cen[ROUNDS];
  double fx[ROUNDS], fy[ROUNDS];
#pragma unroll
  for (int j = 0; j < ROUNDS; ++j) {
    const int slot = tid + j * DEPTH_THREADS;
    cen[j] = 0; fx[j] = 0.0; fy[j] = 0.0;
    if (slot < COUNT) {
      int px, py;
      depth_halo_pixel(slot, R, x0, y0, ref.w, ref.h, &px, &py);
      cen[j] = census[ref.off + (int64_t)py * ref.w + px];
      fx[j] = (double)px; fy[j] = (double)py;
    }
  }
  __syncthreads();

  const int tx = tid % DEPTH_TW, ty = 2 * (tid / DEPTH_TW);      // the upper of this thread's two pixels, in the tile
  int best_k[2] = {0, 0}, best_s[2] = {0x7FFFFFFF, 0x7FFFFFFF}, best_m[2] = {0, 0}, best_p[2] = {0, 0}, prev[2] = {0, 0};
  const double* __restrict__ dk = planes + view.plane_first;
  for (int k = 0; k < n_planes; ++k) {
    const double d = dk[k];
    uint16_t* __restrict__ buf = s_c[k & 1];
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
      const int slot = tid + j * DEPTH_THREADS;
      if (slot < COUNT) {
        int c = 0;
        for (int s = 0; s < n_src; ++s) {
          const depth::Sample smp = depth::sample(s_warp[s], fx[j], fy[j], d, s_w[s], s_h[s]);
          int cs = DEPTH_ABSENT_COST;
          if (smp.valid) cs = depth::cost(cen[j], census[s_off[s] + (int64_t)smp.yi * s_w[s] + smp.xi]);
          c += cs;
        }
        buf[slot] = (uint16_t)c;
      }
    }
    __syncthreads();
    int rows[2 * R + 2];
#pragma unroll
    for (int ry = 0; ry < 2 * R + 2; ++ry) {
      int acc = 0;
#pragma unroll
      for (int dx = 0; dx <= 2 * R; ++dx) acc += buf[(ty + ry) * HW + tx + dx];
      rows[ry] = acc;
    }
    int mid = 0;
#pragma unroll
    for (int ry = 1; ry <= 2 * R; ++ry) mid += rows[ry];
    const int S[2] = {mid + rows[0], mid + rows[2 * R + 1]};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (best_k[q] == k - 1) best_p[q] = S[q];               // the plane behind the running best
      if (S[q] < best_s[q]) { best_s[q] = S[q]; best_k[q] = k; best_m[q] = prev[q]; }
      prev[q] = S[q];
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int x = x0 + tx, y = y0 + ty + q;
    if (x < ref.w && y < ref.h) {
      const int b = best_k[q];
      const double dm = b > 0 ? dk[b - 1] : 0.0, dp = b < n_planes - 1 ? dk[b + 1] : 0.0;
      const int64_t o = view.out_off + (int64_t)y * ref.w + x;
      plane_out[o] = b;
      cost_out[o] = (uint16_t)best_s[q];
      depth_out[o] = depth::refine(b, n_planes, best_m[q], best_s[q], best_p[q], dm, dk[b], dp);
    }
  }
}

__global__ __launch_bounds__(DEPTH_PIXEL_BLOCK) void k_depth_filter(const DepthImage* __restrict__ images, const DepthView* __restrict__ views,
                                                                    int n_ref, const int32_t* __restrict__ src_image,
                                                                    const int32_t* __restrict__ ref_of_image, const double* __restrict__ warps,
                                                                    const double* __restrict__ backproj, const float* __restrict__ depth_in,
                                                                    const uint16_t* __restrict__ cost_in, const int32_t* __restrict__ max_cost,
                                                                    double rel_tol, int min_consistent, uint8_t* __restrict__ n_consistent,
                                                                    uint8_t* __restrict__ keep, double* __restrict__ xyz) {
  const int v = depth_find_view(views, n_ref, blockIdx.x, DEPTH_BY_PIXEL_BLOCK);
  const DepthView view = views[v];
  const DepthImage ref = images[view.image];
  const int64_t p = ((int64_t)blockIdx.x - view.pix_block_first) * DEPTH_PIXEL_BLOCK + threadIdx.x;
  if (p >= (int64_t)ref.h * ref.w) return;
  const double x = (double)(int)(p % ref.w), y = (double)(int)(p / ref.w);
  const int64_t o = view.out_off + p;
  const double d = (double)depth_in[o];
  const bool finite = d - d == 0.0;
  int n = 0;
  if (finite) {
    for (int s = 0; s < view.n_src; ++s) {
      const int e = view.src_first + s;
      const int si = src_image[e];
      const int rs = ref_of_image[si];
      if (rs < 0) continue;                                   // a source without a depth map of its own does not count
      const DepthImage src = images[si];
      const depth::Sample smp = depth::sample(warps + (int64_t)e * 12, x, y, d, src.w, src.h);
      if (!smp.valid) continue;
      const double ds = (double)depth_in[views[rs].out_off + (int64_t)smp.yi * src.w + smp.xi];
      n += depth::agrees(ds, smp.q2, rel_tol);
    }
  }
  n_consistent[o] = (uint8_t)n;
  const bool cost_ok = !max_cost || (int)cost_in[o] <= max_cost[v];
  keep[o] = (finite && cost_ok && n >= min_consistent) ? 1 : 0;
  const double* __restrict__ M = backproj + (int64_t)v * 12;
  const double nan = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < 3; ++i) xyz[o * 3 + i] = finite ? depth::backproject(M + 4 * i, x, y, d) : nan;
}

// the tables of a call -> the workspace; the host vectors are pageable, so the copies must have left them on return
int depth_upload(sfm_ctx* h, const DepthPlan& p, const DepthLayout& L, char* ws, const int32_t* src_image, int64_t n_entries,
                 const int32_t* max_cost, int64_t n_ref) {
  SFM_HIP(h, hipMemcpyAsync(ws + L.images, p.images.data(), p.images.size() * sizeof(DepthImage), hipMemcpyHostToDevice, h->stream));
  SFM_HIP(h, hipMemcpyAsync(ws + L.views, p.views.data(), p.views.size() * sizeof(DepthView), hipMemcpyHostToDevice, h->stream));
  if (n_entries > 0) SFM_HIP(h, hipMemcpyAsync(ws + L.src_image, src_image, (size_t)n_entries * 4, hipMemcpyHostToDevice, h->stream));
  if (!p.ref_of_image.empty())
    SFM_HIP(h, hipMemcpyAsync(ws + L.ref_of_image, p.ref_of_image.data(), p.ref_of_image.size() * 4, hipMemcpyHostToDevice, h->stream));
  if (max_cost && n_ref > 0) SFM_HIP(h, hipMemcpyAsync(ws + L.max_cost, max_cost, (size_t)n_ref * 4, hipMemcpyHostToDevice, h->stream));
  SFM_HIP(h, hipStreamSynchronize(h->stream));
  return SFM_OK;
}

}  // namespace

extern "C" int sfm_depth_workspace_bytes(int32_t n_img, int32_t n_ref, int64_t n_entries, int64_t* bytes_host) {
  if (!bytes_host || n_img < 0 || n_ref < 0 || n_ref > n_img || n_entries < 0 || n_entries > (int64_t)n_ref * DEPTH_MAX_SOURCES)
    return SFM_ERR_ARG;
  *bytes_host = depth_layout(n_img, n_ref, n_entries).bytes;
  return SFM_OK;
}

extern "C" int sfm_depth_census(sfm_handle h, const uint8_t* images, const int64_t* img_off, const int32_t* heights, const int32_t* widths,
                                int32_t n_img, uint64_t* census, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const int bad = depth_check_images(n_img, img_off, heights, widths);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_census", DEPTH_WHY[bad]);
  const DepthLayout L = depth_layout(n_img, 0, 0);
  if (!workspace || workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_census", "workspace missing or too small");
  const int64_t n_elem = img_off[n_img];
  if (cdiv(n_elem, DEPTH_PIXEL_BLOCK) > 0x7FFFFFFFu) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_census", "too many pixels for one call");
  if (n_elem == 0) return SFM_OK;
  if (!images || !census) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_census", "null pointer");
  const DepthPlan p = depth_plan(n_img, img_off, heights, widths, 0, nullptr, nullptr, nullptr);
  char* ws = (char*)workspace;
  const int rc = depth_upload(h, p, L, ws, nullptr, 0, nullptr, 0); if (rc) return rc;
  hipLaunchKernelGGL(k_depth_census, dim3(cdiv(n_elem, DEPTH_PIXEL_BLOCK)), dim3(DEPTH_PIXEL_BLOCK), 0, h->stream, images,
                     (const DepthImage*)(ws + L.images), n_img, n_elem, census);
  SFM_LAUNCH_CHECK(h, "sfm_depth_census");
  return SFM_OK;
}

extern "C" int sfm_depth_sweep(sfm_handle h, const uint64_t* census, const int64_t* img_off, const int32_t* heights, const int32_t* widths,
                               int32_t n_img, int32_t n_ref, const int32_t* ref_image, const int64_t* src_ptr, const int32_t* src_image,
                               const double* warps, const int64_t* plane_ptr, const double* plane_depth, int32_t radius,
                               int32_t* plane, uint16_t* cost, float* depth, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  int bad = depth_check_images(n_img, img_off, heights, widths);
  if (!bad) bad = depth_check_views(n_img, n_ref, ref_image, src_ptr, src_image, plane_ptr, radius);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_sweep", DEPTH_WHY[bad]);
  const int64_t n_entries = src_ptr[n_ref];
  const DepthLayout L = depth_layout(n_img, n_ref, n_entries);
  if (!workspace || workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_sweep", "workspace missing or too small");
  const DepthPlan p = depth_plan(n_img, img_off, heights, widths, n_ref, ref_image, src_ptr, plane_ptr);
  if (p.n_tiles > 0x7FFFFFFFLL) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_sweep", "too many tiles for one call");
  if (p.n_tiles == 0) return SFM_OK;
  if (!census || !plane_depth || !plane || !cost || !depth || (n_entries > 0 && !warps))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_sweep", "null pointer");
  char* ws = (char*)workspace;
  const int rc = depth_upload(h, p, L, ws, src_image, n_entries, nullptr, 0); if (rc) return rc;
  const DepthImage* d_img = (const DepthImage*)(ws + L.images);
  const DepthView* d_view = (const DepthView*)(ws + L.views);
  const int32_t* d_src = (const int32_t*)(ws + L.src_image);
#define DEPTH_SWEEP(RR) hipLaunchKernelGGL((k_depth_sweep<RR>), dim3((unsigned)p.n_tiles), dim3(DEPTH_THREADS), 0, h->stream, census, d_img, \
                                           d_view, n_ref, d_src, warps, plane_depth, plane, cost, depth)
  switch (radius) {
    case 0: DEPTH_SWEEP(0); break;
    case 1: DEPTH_SWEEP(1); break;
    case 2: DEPTH_SWEEP(2); break;
    case 3: DEPTH_SWEEP(3); break;
    default: DEPTH_SWEEP(4); break;
  }
#undef DEPTH_SWEEP
  SFM_LAUNCH_CHECK(h, "sfm_depth_sweep");
  return SFM_OK;
}

extern "C" int sfm_depth_filter(sfm_handle h, const int64_t* img_off, const int32_t* heights, const int32_t* widths, int32_t n_img,
                                int32_t n_ref, const int32_t* ref_image, const int64_t* src_ptr, const int32_t* src_image,
                                const double* warps, const double* backproj, const float* depth, const uint16_t* cost,
                                const int32_t* max_cost, double rel_tol, int32_t min_consistent, uint8_t* n_consistent, uint8_t* keep,
                                double* xyz, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  int bad = depth_check_images(n_img, img_off, heights, widths);
  std::vector<int64_t> one((size_t)(n_ref > 0 ? n_ref : 0) + 1);      // the filter has no planes: one per view stands in for them
  for (size_t r = 0; r < one.size(); ++r) one[r] = (int64_t)r;
  if (!bad) bad = depth_check_views(n_img, n_ref, ref_image, src_ptr, src_image, one.data(), 0);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_filter", DEPTH_WHY[bad]);
  if (!(rel_tol >= 0.0)) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_filter", "rel_tol must be a number >= 0");
  const int64_t n_entries = src_ptr[n_ref];
  const DepthLayout L = depth_layout(n_img, n_ref, n_entries);
  if (!workspace || workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_filter", "workspace missing or too small");
  const DepthPlan p = depth_plan(n_img, img_off, heights, widths, n_ref, ref_image, src_ptr, one.data());
  if (p.n_pix_blocks > 0x7FFFFFFFLL) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_filter", "too many pixels for one call");
  if (p.n_pix_blocks == 0) return SFM_OK;
  if (!backproj || !depth || !cost || !n_consistent || !keep || !xyz || (n_entries > 0 && !warps))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_filter", "null pointer");
  char* ws = (char*)workspace;
  const int rc = depth_upload(h, p, L, ws, src_image, n_entries, max_cost, n_ref); if (rc) return rc;
  hipLaunchKernelGGL(k_depth_filter, dim3((unsigned)p.n_pix_blocks), dim3(DEPTH_PIXEL_BLOCK), 0, h->stream,
                     (const DepthImage*)(ws + L.images), (const DepthView*)(ws + L.views), n_ref, (const int32_t*)(ws + L.src_image),
                     (const int32_t*)(ws + L.ref_of_image), warps, backproj, depth, cost,
                     max_cost ? (const int32_t*)(ws + L.max_cost) : nullptr, rel_tol, min_consistent, n_consistent, keep, xyz);
  SFM_LAUNCH_CHECK(h, "sfm_depth_filter");
  return SFM_OK;
}
