// The render of a mesh scored against the photographs it was built from: absolute error, squared error, SSIM over a uniform
// window and the distance to the view's own depth, per view, for gfx950 (MI355X).  include/sfm_amd.h states the rule;
// render_score_rule.h holds its arithmetic (integers, and float64 without FMA contraction for the two quotients),
// render_score_plan.h the argument checks, the tiles, the workspace and the grid.
//
//   k_render_score  one workgroup per tile of 32 x 8 pixels of one view, one thread per pixel.  The workgroup stages the tile
//                   and a halo of window / 2 pixels of the render, the photograph and the flags in LDS, one 32-bit word per
//                   pixel and image; a thread takes the five sums of every channel over its W x W window straight from LDS
//                   (the direct loop; no separable variant was built), writes its pixel of abs_error and ssim_map, and
//                   the fourteen counts are reduced over the wavefront in 32-bit integers, over the four wavefronts through
//                   LDS in 64-bit, and added to the view's row of `stats` with one integer atomicAdd per column that is
//                   not zero.
// Every statistic is an integer sum: no order of the workgroups can change a byte.  No floating-point atomics, no kernel
// waits on another workgroup, every loop is bounded by the staged tile or the window, and nothing is written outside the
// pixels of a view or its row of the table.
#include <vector>

#include "common.h"
#include "render_score_rule.h"
#include "render_score_plan.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;                                                        // the whole sum in lane 0
}
__device__ __forceinline__ int wave_count(bool b) { return (int)__popcll(__ballot(b)); }

template <int CH, int W>
__global__ __launch_bounds__(RENDER_SCORE_BLOCK) void k_render_score(const TsdfView* __restrict__ views, const uint8_t* __restrict__ color,
                                                                     const int32_t* __restrict__ triangle, const float* __restrict__ depth,
                                                                     const uint8_t* __restrict__ photos, const uint8_t* __restrict__ mask,
                                                                     const float* __restrict__ view_depth, const uint8_t* __restrict__ view_keep,
                                                                     double rel_tol, unsigned long long* __restrict__ stats,
                                                                     uint8_t* __restrict__ abs_error, uint32_t* __restrict__ ssim_map) {
  __shared__ uint32_t s_render[RENDER_SCORE_STAGE_WORDS], s_photo[RENDER_SCORE_STAGE_WORDS];
  __shared__ long long s_sum[RENDER_SCORE_BLOCK / 64][RENDER_SCORE_STATS];
  const TsdfView view = views[blockIdx.y];
  const int w = view.w, h = view.h;
  if ((int64_t)blockIdx.x >= render_score_tiles(h, w)) return;     // the same in every thread
  const RenderScoreTile T = render_score_tile(blockIdx.x, w, W);
  constexpr int R = W / 2, SW = RENDER_SCORE_TILE_W + 2 * R, SH = RENDER_SCORE_TILE_H + 2 * R;
  static_assert(SW * SH <= RENDER_SCORE_STAGE_WORDS, "the staged tile fits");
  for (int i = threadIdx.x; i < SW * SH; i += RENDER_SCORE_BLOCK) {
    const int x = T.sx0 + i % SW, y = T.sy0 + i / SW;
    uint32_t r = 0, p = 0;
    if (x >= 0 && x < w && y >= 0 && y < h) {
      const int64_t at = view.out_off + (int64_t)y * w + x;
      const int covered = triangle[at] >= 0;
      const int compared = covered && (!mask || mask[at] > 0);
      const uint8_t* c = color + at * CH;
      const uint8_t* q = photos + at * CH;
      r = render_score::pack(c[0], CH == 3 ? c[CH - 2] : 0, CH == 3 ? c[CH - 1] : 0,
                             (compared ? RENDER_SCORE_COMPARED : 0) | (covered ? RENDER_SCORE_COVERED : 0));
      p = render_score::pack(q[0], CH == 3 ? q[CH - 2] : 0, CH == 3 ? q[CH - 1] : 0, 0);
    }
    s_render[i] = r;
    s_photo[i] = p;
  }
  __syncthreads();

  const int lx = threadIdx.x % RENDER_SCORE_TILE_W, ly = threadIdx.x / RENDER_SCORE_TILE_W;
  const int x = T.x0 + lx, y = T.y0 + ly;
  int sad[3] = {0, 0, 0}, sse[3] = {0, 0, 0}, q_ssim = 0, q_rel = 0;
  bool compared = false, has_ssim = false, both = false, agree = false, render_only = false, view_only = false;
  if (x < w && y < h) {
    const int64_t at = view.out_off + (int64_t)y * w + x;
    const uint32_t rc = s_render[(ly + R) * SW + lx + R], pc = s_photo[(ly + R) * SW + lx + R];
    const int f = render_score::flags(rc);
    compared = (f & RENDER_SCORE_COMPARED) != 0;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int e = render_score::channel(rc, k) - render_score::channel(pc, k);
      const int a = compared ? (e < 0 ? -e : e) : 0;
      sad[k] = a;
      sse[k] = a * a;
      if (abs_error) abs_error[at * CH + k] = (uint8_t)a;
    }
    uint32_t bits = RENDER_SCORE_NAN_BITS;
    if (compared && x >= R && x + R < w && y >= R && y + R < h) {
      double s;
      if (render_score::window_ssim<CH, W>(s_render, s_photo, SW, ly * SW + lx, &s)) {
        has_ssim = true;
        q_ssim = (int)render_score::quantise(s);
        bits = __float_as_uint((float)s);
      }
    }
    if (ssim_map) ssim_map[at] = bits;
    if (view_depth) {
      const float dv = view_depth[at];
      const bool covered = (f & RENDER_SCORE_COVERED) != 0, seen = render_score::seen(view_keep[at], dv) != 0;
      both = covered && seen;
      render_only = covered && !seen;
      view_only = seen && !covered;
      if (both) {
        int ag;
        int64_t q;
        render_score::depth_term(depth[at], dv, rel_tol, &ag, &q);
        agree = ag != 0;
        q_rel = (int)q;
      }
    }
  }
  // every thread of the workgroup is here again
  int part[RENDER_SCORE_STATS];
  part[RS_N_COMPARED - 1] = wave_count(compared);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    part[RS_SAD - 1 + k] = k < CH ? wave_sum(sad[k]) : 0;
    part[RS_SSE - 1 + k] = k < CH ? wave_sum(sse[k]) : 0;
  }
  part[RS_N_SSIM - 1] = wave_count(has_ssim);
  part[RS_Q_SSIM - 1] = wave_sum(q_ssim);
  part[RS_N_BOTH - 1] = wave_count(both);
  part[RS_N_AGREE - 1] = wave_count(agree);
  part[RS_Q_REL - 1] = wave_sum(q_rel);
  part[RS_N_RENDER_ONLY - 1] = wave_count(render_only);
  part[RS_N_VIEW_ONLY - 1] = wave_count(view_only);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < RENDER_SCORE_STATS; ++k) s_sum[wave][k] = (long long)part[k];
  }
  __syncthreads();
  unsigned long long* row = stats + (int64_t)blockIdx.y * RENDER_SCORE_COLUMNS;
  if (threadIdx.x < RENDER_SCORE_STATS) {
    long long t = 0;
#pragma unroll
    for (int v = 0; v < RENDER_SCORE_BLOCK / 64; ++v) t += s_sum[v][threadIdx.x];
    if (t != 0) atomicAdd(row + 1 + threadIdx.x, (unsigned long long)t);         // two's complement: a negative q_ssim adds as it should
  }
  if (blockIdx.x == 0 && threadIdx.x == RENDER_SCORE_STATS) row[RS_N_PIXELS] = (unsigned long long)((int64_t)h * w);
}

}  // namespace

extern "C" int sfm_render_score_tile(int32_t* tile_w, int32_t* tile_h) {
  if (!tile_w || !tile_h) return SFM_ERR_ARG;
  *tile_w = RENDER_SCORE_TILE_W;
  *tile_h = RENDER_SCORE_TILE_H;
  return SFM_OK;
}

extern "C" int sfm_render_score_workspace_bytes(int32_t n_view, const int32_t* heights, const int32_t* widths, int64_t* bytes_host) {
  if (!bytes_host) return SFM_ERR_ARG;
  if (render_score_check_views(n_view, heights, widths, nullptr, nullptr, nullptr)) return SFM_ERR_ARG;
  *bytes_host = render_score_layout(n_view).bytes;
  return SFM_OK;
}

extern "C" int sfm_render_score(sfm_handle h, int32_t n_view, const int32_t* heights, const int32_t* widths, int32_t channels,
                                const uint8_t* render_color, const int32_t* render_triangle, const float* render_depth, const uint8_t* photos,
                                const uint8_t* photo_mask, const float* view_depth, const uint8_t* view_keep, int32_t window, double rel_tol,
                                int64_t* stats, uint8_t* abs_error, float* ssim_map, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_render_score";
  std::vector<TsdfView> views((size_t)(n_view > 0 && n_view <= RENDER_SCORE_MAX_VIEWS ? n_view : 0) + 1);
  int64_t n_pix = 0, max_tiles = 0;
  int bad = render_score_check_views(n_view, heights, widths, views.data(), &n_pix, &max_tiles);
  if (!bad) bad = render_score_check_options(channels, window, rel_tol, view_depth, view_keep);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, RENDER_SCORE_WHY[bad]);
  const RenderScoreLayout L = render_score_layout(n_view);
  bad = render_score_check_buffers(n_view, n_pix, L.bytes, render_color, render_triangle, render_depth, photos, stats, workspace, workspace_bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, RENDER_SCORE_WHY[bad]);
  if (n_view == 0) return SFM_OK;
  SFM_HIP(h, hipMemsetAsync(stats, 0, (size_t)n_view * RENDER_SCORE_COLUMNS * sizeof(int64_t), h->stream));
  if (n_pix == 0) return SFM_OK;                                   // no pixel: every count is 0
  char* ws = (char*)workspace;
  // the view table is pageable host memory: the copy must have left it on return
  SFM_HIP(h, hipMemcpyAsync(ws + L.views, views.data(), views.size() * sizeof(TsdfView), hipMemcpyHostToDevice, h->stream));
  SFM_HIP(h, hipStreamSynchronize(h->stream));
  const TsdfView* d_views = (const TsdfView*)(ws + L.views);
  const dim3 grid((unsigned)max_tiles, (unsigned)n_view), block(RENDER_SCORE_BLOCK);
#define SFM_RENDER_SCORE(CH, W)                                                                                                                  \
  hipLaunchKernelGGL((k_render_score<CH, W>), grid, block, 0, h->stream, d_views, render_color, render_triangle, render_depth, photos, photo_mask, \
                     view_depth, view_keep, rel_tol, (unsigned long long*)stats, abs_error, (uint32_t*)ssim_map)
#define SFM_RENDER_SCORE_WINDOWS(CH)                                                                                                             \
  switch (window) {                                                                                                                              \
    case 3: SFM_RENDER_SCORE(CH, 3); break;                                                                                                      \
    case 5: SFM_RENDER_SCORE(CH, 5); break;                                                                                                      \
    case 7: SFM_RENDER_SCORE(CH, 7); break;                                                                                                      \
    case 9: SFM_RENDER_SCORE(CH, 9); break;                                                                                                      \
    default: SFM_RENDER_SCORE(CH, 11); break;                                                                                                    \
  }
  if (channels == 1) { SFM_RENDER_SCORE_WINDOWS(1) } else { SFM_RENDER_SCORE_WINDOWS(3) }
#undef SFM_RENDER_SCORE_WINDOWS
#undef SFM_RENDER_SCORE
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}
