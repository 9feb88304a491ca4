// Exposure compensation between the views of a mesh, for gfx950 (MI355X): what every view sees of every vertex as one byte per
// channel, the two integer tables the gain solve needs, and the gains applied to the images.  include/sfm_amd.h states the
// rule; mesh_exposure_rule.h holds its arithmetic (float64 without FMA contraction, integers), mesh_color_rule.h the sample,
// mesh_exposure_plan.h the argument checks, the workspace, the grids and the split of the vertex range.
//
//   k_exposure_sample  one thread per vertex, the views in batches of MESH_COLOR_BATCH exactly as k_mesh_colors walks them
//                      (all depths of a batch, then all pixels); per view one flag and `channels` bytes, written along the
//                      vertex axis, so a wavefront writes 64 consecutive bytes per row.
//   k_exposure_gram    overlap = F F^T and sums_k = Q_k F^T over the vertex axis on the matrix cores
//                      (v_mfma_i32_32x32x32_i8): F the flags as 0 / 1, Q - 128 where seen as the signed operand, and
//                      sums = product + 128 * overlap.  Operands come straight from global memory, 16 bytes of one row per
//                      lane: both operands of a product take their k from the same 16 vertices, so no staging is needed.
//                      A step is one round trip to memory and little else, so a wavefront asks for the operands of
//                      MESH_EXPOSURE_AHEAD steps before it multiplies the first (0.037 against 0.065 ms with one step at a
//                      time and chunks twice as long: README, "Exposure").  A workgroup adds the tiles of its four
//                      wavefronts in LDS (int32) and then adds what is not zero to the int64 tables with integer atomics;
//                      k_exposure_clear zeroes both tables in one launch in front of it.
//   k_images_gain      one thread per 16-byte window of the source: a vector load and store where the window is whole and the
//                      destination is aligned like the source, bytes otherwise.
// The tables are integer sums: no order of the workgroups can change a byte.  No floating-point atomics, no kernel waits on
// another workgroup, every loop is bounded by the chunk or the batch, and nothing is written outside the outputs.
#include <vector>

#include "common.h"
#include "mesh_exposure_rule.h"
#include "mesh_exposure_plan.h"
#include "view_table.h"

#pragma clang fp contract(off)

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

template <int CH, int BATCH>
__global__ __launch_bounds__(MESH_BLOCK) void k_exposure_sample(const TsdfView* __restrict__ views, int n_ref, const double* __restrict__ proj,
                                                                const double* __restrict__ centres, const float* __restrict__ depth_in,
                                                                const uint8_t* __restrict__ keep, const uint8_t* __restrict__ pixels,
                                                                int64_t n_vertices, const double* __restrict__ vertices,
                                                                const float* __restrict__ normals, double tol, double min_cos,
                                                                uint8_t* __restrict__ seen, uint8_t* __restrict__ samples) {
  const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const double X[3] = {vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]};
  const double n[3] = {(double)normals[3 * i], (double)normals[3 * i + 1], (double)normals[3 * i + 2]};
  for (int v0 = 0; v0 < n_ref; v0 += BATCH) {
    TsdfView view[BATCH];
    mesh_color::Projection p[BATCH];
    float ds[BATCH];
    uint8_t kept[BATCH];
    // round trip one: the depth and the keep flag of every view of the batch
#pragma unroll
    for (int b = 0; b < BATCH; ++b) {
      const int v = v0 + b;
      p[b].valid = 0;
      ds[b] = 0.0f;
      kept[b] = 1;
      if (v < n_ref) {                                           // wave-uniform
        view[b] = views[v];
        p[b] = mesh_color::project(proj + (int64_t)v * 12, X[0], X[1], X[2], view[b].w, view[b].h);
        if (p[b].valid) {                                        // never valid in a view without a pixel
          const int64_t e = view[b].out_off + (int64_t)p[b].yi * view[b].w + p[b].xi;
          ds[b] = depth_in[e];
          if (keep) kept[b] = keep[e];
        }
      }
    }
    // round trip two: the four pixels of every view that sees the vertex
    mesh_color::Taps t[BATCH];
    uint8_t px[BATCH][4 * CH];
    bool use[BATCH];
#pragma unroll
    for (int b = 0; b < BATCH; ++b) {
      double wgt;
      use[b] = p[b].valid && mesh_color::sees((double)ds[b], kept[b] != 0, p[b].q2, tol) &&
               mesh_color::weight(centres + (int64_t)(v0 + b) * 3, X, n, min_cos, &wgt);
      if (use[b]) {
        t[b] = mesh_color::taps(p[b].u, p[b].v, view[b].w, view[b].h);
        const uint8_t* img = pixels + view[b].out_off * CH;
        const int64_t r0 = (int64_t)t[b].y0 * view[b].w, r1 = (int64_t)t[b].y1 * view[b].w;
        const int64_t at[4] = {(r0 + t[b].x0) * CH, (r0 + t[b].x1) * CH, (r1 + t[b].x0) * CH, (r1 + t[b].x1) * CH};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int k = 0; k < CH; ++k) px[b][c * CH + k] = img[at[c] + k];
      }
    }
#pragma unroll
    for (int b = 0; b < BATCH; ++b) {
      const int v = v0 + b;
      if (v >= n_ref) break;                                     // wave-uniform
      seen[(int64_t)v * n_vertices + i] = use[b] ? 1 : 0;
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        uint8_t q = 0;
        if (use[b])
          q = mesh_exposure::quantise(mesh_color::bilinear((double)px[b][k], (double)px[b][CH + k], (double)px[b][2 * CH + k],
                                                           (double)px[b][3 * CH + k], t[b].fx, t[b].fy));
        samples[((int64_t)v * CH + k) * n_vertices + i] = q;
      }
    }
  }
}

// the 16 bytes of a row of n bytes from byte v on; zeros past the row's end
__device__ __forceinline__ v4i load16(const uint8_t* __restrict__ row, int64_t n, int64_t v) {
  v4i r = {0, 0, 0, 0};
  if (v + 16 <= n) {
    __builtin_memcpy(&r, row + v, 16);
  } else if (v < n) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (v + k < n) w[k >> 2] |= (uint32_t)row[v + k] << (8 * (k & 3));
    r = v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
  }
  return r;
}

// both tables to zero in one launch: n_sums >= n_overlap entries
__global__ __launch_bounds__(MESH_EXPOSURE_GRAM_BLOCK) void k_exposure_clear(int64_t n_overlap, int64_t n_sums, unsigned long long* __restrict__ overlap,
                                                                             unsigned long long* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * MESH_EXPOSURE_GRAM_BLOCK + threadIdx.x;
  if (i < n_overlap) overlap[i] = 0;
  if (i < n_sums) sums[i] = 0;
}

template <int CH>
__global__ __launch_bounds__(MESH_EXPOSURE_GRAM_BLOCK) void k_exposure_gram(int n_ref, int64_t n_vertices, const uint8_t* __restrict__ seen,
                                                                            const uint8_t* __restrict__ samples,
                                                                            unsigned long long* __restrict__ overlap,
                                                                            unsigned long long* __restrict__ sums) {
  constexpr int T = MESH_EXPOSURE_TILE, CELLS = T * T, WAVES = MESH_EXPOSURE_GRAM_BLOCK / 64;
  static_assert(T == 32 && MESH_EXPOSURE_STEP == 32, "one v_mfma_i32_32x32x32_i8 per table and step");
  __shared__ int s_tile[(1 + CH) * CELLS];
  const int tiles = (n_ref + T - 1) / T;
  const int ti = (int)blockIdx.y / tiles, tj = (int)blockIdx.y % tiles;
  for (int e = threadIdx.x; e < (1 + CH) * CELLS; e += MESH_EXPOSURE_GRAM_BLOCK) s_tile[e] = 0;
  __syncthreads();

  // lane l holds, of row l & 31 of its tile, the 16 vertices of half l >> 5 of the step: the A operand (view i, rows of the
  // result) and the B operand (view j, columns of the result) alike, so both take their k from the same vertices
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, half = lane >> 5;
  const int vi = ti * T + r, vj = tj * T + r;
  const int64_t c0 = (int64_t)blockIdx.x * MESH_EXPOSURE_CHUNK;
  const int64_t c1 = c0 + MESH_EXPOSURE_CHUNK < n_vertices ? c0 + MESH_EXPOSURE_CHUNK : n_vertices;
  // a row ends with the chunk; one that is not there reads as one of no length: all zeros, and nothing is read through it
  const int64_t ni = vi < n_ref ? c1 : 0, nj = vj < n_ref ? c1 : 0;
  const uint8_t* fi = seen + (vi < n_ref ? (int64_t)vi * n_vertices : 0);
  const uint8_t* fj = seen + (vj < n_ref ? (int64_t)vj * n_vertices : 0);
  const uint8_t* qi = samples + (vi < n_ref ? (int64_t)vi * CH * n_vertices : 0);
  v16i acc[1 + CH];
#pragma unroll
  for (int a = 0; a < 1 + CH; ++a)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[a][g] = 0;
  // a wavefront's steps are WAVES apart; it asks for the operands of MESH_EXPOSURE_AHEAD of them before it multiplies the
  // first, because a step is one round trip to memory and little else.  A step past the chunk's end reads as zeros.
  constexpr int U = MESH_EXPOSURE_AHEAD;
  for (int64_t v0 = c0 + wave * MESH_EXPOSURE_STEP; v0 < c1; v0 += U * WAVES * MESH_EXPOSURE_STEP) {   // the same in a wavefront
    v4i si[U], sj[U], q[U][CH];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = v0 + (int64_t)u * WAVES * MESH_EXPOSURE_STEP + 16 * half;
      si[u] = load16(fi, ni, v);
      sj[u] = load16(fj, nj, v);
#pragma unroll
      for (int k = 0; k < CH; ++k) q[u][k] = load16(qi + (int64_t)k * n_vertices, ni, v);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v4i a01, b01;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        a01[w] = (int)mesh_exposure::flags01((uint32_t)si[u][w]);
        b01[w] = (int)mesh_exposure::flags01((uint32_t)sj[u][w]);
      }
      acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a01, b01, acc[0], 0, 0, 0);
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        v4i s;
#pragma unroll
        for (int w = 0; w < 4; ++w) s[w] = (int)mesh_exposure::signed4((uint32_t)q[u][k][w], (uint32_t)a01[w]);
        acc[1 + k] = __builtin_amdgcn_mfma_i32_32x32x32_i8(s, b01, acc[1 + k], 0, 0, 0);
      }
    }
  }
  // register g of lane l is row (g & 3) + 8 (g >> 2) + 4 (l >> 5), column l & 31 of the 32 x 32 result
#pragma unroll
  for (int a = 0; a < 1 + CH; ++a)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int row = (g & 3) + 8 * (g >> 2) + 4 * half;
      if (acc[a][g] != 0) atomicAdd(&s_tile[a * CELLS + row * T + r], acc[a][g]);
    }
  __syncthreads();
  for (int e = threadIdx.x; e < CELLS; e += MESH_EXPOSURE_GRAM_BLOCK) {
    const int gi = ti * T + e / T, gj = tj * T + e % T;
    if (gi >= n_ref || gj >= n_ref) continue;
    const long long o = (long long)s_tile[e];
    const int64_t cell = (int64_t)gi * n_ref + gj;
    if (o != 0) atomicAdd(overlap + cell, (unsigned long long)o);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const long long s = (long long)s_tile[(1 + k) * CELLS + e] + 128LL * o;      // >= 0: a sum of bytes
      if (s != 0) atomicAdd(sums + cell * CH + k, (unsigned long long)s);
    }
  }
}

// a batch of images for k_images_gain: the first byte of each within the arrays, one more that closes the list, and the gains
struct GainBatch {
  int64_t byte0[MESH_EXPOSURE_GAIN_BATCH + 1];
  double gain[MESH_EXPOSURE_GAIN_BATCH][3];
};

template <int CH>
__global__ __launch_bounds__(MESH_EXPOSURE_GAIN_BLOCK) void k_images_gain(const GainBatch B, int mis, int same_alignment,
                                                                          const uint8_t* in, uint8_t* out) {       // may be one array
  const int img = blockIdx.y;
  const int64_t b0 = B.byte0[img], b1 = B.byte0[img + 1];
  const int64_t t = (int64_t)blockIdx.x * MESH_EXPOSURE_GAIN_BLOCK + threadIdx.x;
  if (t >= mesh_exposure_windows(b0, b1, mis)) return;
  const MeshExposureWindow W = mesh_exposure_window(b0, b1, mis, t);
  double g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = B.gain[img][k < CH ? k : 0];
  int ph = (int)((W.lo - b0) % CH);                                // the channel of the window's first byte
  if (W.hi - W.lo == 16 && same_alignment) {
    const uint4 x = *(const uint4*)(in + W.lo);
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
    uint32_t yw[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      uint32_t y = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double gk = CH == 1 ? g[0] : (ph == 0 ? g[0] : (ph == 1 ? g[1] : g[2]));
        y |= (uint32_t)mesh_exposure::gain((uint8_t)((xw[w] >> (8 * j)) & 255u), gk) << (8 * j);
        ph = ph + 1 == CH ? 0 : ph + 1;
      }
      yw[w] = y;
    }
    *(uint4*)(out + W.lo) = uint4{yw[0], yw[1], yw[2], yw[3]};
  } else {
    for (int64_t b = W.lo; b < W.hi; ++b) {
      const double gk = CH == 1 ? g[0] : (ph == 0 ? g[0] : (ph == 1 ? g[1] : g[2]));
      out[b] = mesh_exposure::gain(in[b], gk);
      ph = ph + 1 == CH ? 0 : ph + 1;
    }
  }
}

}  // namespace

extern "C" int sfm_mesh_exposure_workspace_bytes(int32_t n_ref, int32_t channels, int64_t n_vertices, int64_t* bytes_host) {
  if (!bytes_host || mesh_exposure_check(n_ref, channels, n_vertices)) return SFM_ERR_ARG;
  *bytes_host = mesh_exposure_workspace_bytes(n_ref);
  return SFM_OK;
}

extern "C" int sfm_mesh_exposure_plan(int32_t n_ref, int32_t channels, int64_t n_vertices, int32_t* out) {
  if (!out || mesh_exposure_check(n_ref, channels, n_vertices)) return SFM_ERR_ARG;
  mesh_exposure_plan(n_ref, n_vertices, out);
  return SFM_OK;
}

extern "C" int sfm_mesh_exposure_sample(sfm_handle h, const int32_t* heights, const int32_t* widths, int32_t n_img, int32_t n_ref,
                                        const int32_t* ref_image, const double* proj, const double* centres, const float* depth,
                                        const uint8_t* keep, const uint8_t* pixels, int32_t channels, int64_t n_vertices, const double* vertices,
                                        const float* normals, double tol, double min_cos, uint8_t* seen, uint8_t* samples, void* workspace,
                                        int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_exposure_sample";
  int bad = mesh_exposure_check(n_ref < 0 ? 0 : n_ref, channels, n_vertices);        // a negative n_ref is the view check's to name
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_EXPOSURE_WHY[bad]);
  ViewTable views;
  bad = view_table_build(n_img, heights, widths, n_ref, ref_image, &views);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_WHY[bad]);
  bad = mesh_color_check(channels, n_vertices, tol, min_cos, 0);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_COLOR_WHY[bad]);
  bad = mesh_exposure_check_sample_buffers(n_ref, views.n_out, n_vertices, proj, centres, depth, pixels, vertices, normals, seen, samples,
                                           workspace, workspace_bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_EXPOSURE_WHY[bad]);
  if (n_vertices == 0 || n_ref == 0) return SFM_OK;
  if (const int rc = sfm_put_views(h, views, workspace)) return rc;
  const dim3 grid((unsigned)mesh_color_blocks(n_vertices)), block(MESH_BLOCK);
  if (channels == 1)
    hipLaunchKernelGGL((k_exposure_sample<1, MESH_COLOR_BATCH>), grid, block, 0, h->stream, (const TsdfView*)workspace, n_ref, proj, centres, depth,
                       keep, pixels, n_vertices, vertices, normals, tol, min_cos, seen, samples);
  else
    hipLaunchKernelGGL((k_exposure_sample<3, MESH_COLOR_BATCH>), grid, block, 0, h->stream, (const TsdfView*)workspace, n_ref, proj, centres, depth,
                       keep, pixels, n_vertices, vertices, normals, tol, min_cos, seen, samples);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}

extern "C" int sfm_mesh_exposure_gram(sfm_handle h, int32_t n_ref, int32_t channels, int64_t n_vertices, const uint8_t* seen,
                                      const uint8_t* samples, int64_t* overlap, int64_t* sums, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_exposure_gram";
  int bad = mesh_exposure_check(n_ref, channels, n_vertices);
  if (!bad) bad = mesh_exposure_check_gram_buffers(n_ref, n_vertices, seen, samples, overlap, sums, workspace, workspace_bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_EXPOSURE_WHY[bad]);
  if (n_ref == 0) return SFM_OK;
  const int64_t cells = (int64_t)n_ref * n_ref;
  hipLaunchKernelGGL(k_exposure_clear, dim3(cdiv(cells * channels, MESH_EXPOSURE_GRAM_BLOCK)), dim3(MESH_EXPOSURE_GRAM_BLOCK), 0, h->stream, cells,
                     cells * channels, (unsigned long long*)overlap, (unsigned long long*)sums);
  SFM_LAUNCH_CHECK(h, what);
  if (n_vertices == 0) return SFM_OK;                              // no vertex: every count is 0
  const int64_t tiles = mesh_exposure_tiles(n_ref);
  const dim3 grid((unsigned)mesh_exposure_chunks(n_vertices), (unsigned)(tiles * tiles)), block(MESH_EXPOSURE_GRAM_BLOCK);
  if (channels == 1)
    hipLaunchKernelGGL((k_exposure_gram<1>), grid, block, 0, h->stream, (int)n_ref, n_vertices, seen, samples, (unsigned long long*)overlap,
                       (unsigned long long*)sums);
  else
    hipLaunchKernelGGL((k_exposure_gram<3>), grid, block, 0, h->stream, (int)n_ref, n_vertices, seen, samples, (unsigned long long*)overlap,
                       (unsigned long long*)sums);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}

extern "C" int sfm_images_gain(sfm_handle h, const int32_t* heights, const int32_t* widths, int32_t n_img, int32_t channels, const double* gains,
                               const uint8_t* pixels_in, uint8_t* pixels_out) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_images_gain";
  std::vector<int64_t> off((size_t)(n_img > 0 ? n_img : 0) + 1);
  int bad = mesh_exposure_check_images(n_img, heights, widths, channels, gains, off.data());
  if (!bad && off[(size_t)n_img] > 0 && (!pixels_in || !pixels_out)) bad = 5;
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_EXPOSURE_WHY[bad]);
  const int mis = (int)((uintptr_t)pixels_in % 16), same = (uintptr_t)pixels_out % 16 == (uintptr_t)mis;
  for (int64_t first = 0; first < n_img; first += MESH_EXPOSURE_GAIN_BATCH) {
    const int n = (int)(n_img - first < MESH_EXPOSURE_GAIN_BATCH ? n_img - first : MESH_EXPOSURE_GAIN_BATCH);
    GainBatch B = {};
    int64_t most = 0;
    for (int b = 0; b <= n; ++b) B.byte0[b] = off[(size_t)(first + b)] * channels;
    for (int b = 0; b < n; ++b) {
      for (int k = 0; k < channels; ++k) B.gain[b][k] = gains[(first + b) * channels + k];
      const int64_t w = mesh_exposure_windows(B.byte0[b], B.byte0[b + 1], mis);
      most = w > most ? w : most;
    }
    if (most == 0) continue;                                       // no pixel in the batch
    const dim3 grid((unsigned)mesh_exposure_gain_blocks(most), (unsigned)n), block(MESH_EXPOSURE_GAIN_BLOCK);
    if (channels == 1)
      hipLaunchKernelGGL((k_images_gain<1>), grid, block, 0, h->stream, B, mis, (int)same, pixels_in, pixels_out);
    else
      hipLaunchKernelGGL((k_images_gain<3>), grid, block, 0, h->stream, B, mis, (int)same, pixels_in, pixels_out);
  }
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}
