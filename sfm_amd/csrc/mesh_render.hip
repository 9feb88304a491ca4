// The mesh drawn through a batch of cameras: depth, triangle, barycentrics and colour per pixel, for gfx950 (MI355X).
// include/sfm_amd.h states the rule; mesh_render_rule.h holds its floating point (float64, no FMA contraction) and the key,
// mesh_render_plan.h the argument checks, the workspace and the grids.
//
//   k_render_clear         the keys to all ones, the length of the list to 0
//   k_render_project       one thread per (camera, vertex): u, v, q2 into the workspace, q2 = 0 for an unusable vertex
//   k_render_raster        one thread per (camera, triangle): the box cut to the image; a box of at most
//                          MESH_RENDER_SMALL_BOX pixels is walked by the thread, a larger one is appended to the list - a
//                          ballot over the wavefront, one integer atomic add of its population count by the first flagged
//                          lane, each flagged lane's slot the base plus the flagged lanes below it
//   k_render_raster_large  a fixed grid over the list, one workgroup per entry at a time, its threads the box's pixels
//   k_render_resolve       one thread per pixel: the winner out of the key, its barycentrics again, the four outputs
// A pixel's winner is the minimum of a 64-bit unsigned key (depth bits, triangle) taken with atomicMin in global memory: an
// integer minimum has no order, so neither the visit order nor the order of the list can change a byte.  No floating-point
// atomics, no kernel waits on another workgroup, nothing spins, every loop is bounded by a box that was cut to the image
// or by the list's capacity.  The marching-tetrahedra triangles are voxel-sized, about a fifth of a pixel centre each at the
// image sizes of the sweep, so the thread-per-triangle pass carries the work and the list stays empty unless a camera is close.
#include <vector>

#include "common.h"
#include "mesh_render_rule.h"
#include "mesh_render_plan.h"

#pragma clang fp contract(off)

namespace {

using mesh_render::Vertex;

__global__ __launch_bounds__(MESH_BLOCK) void k_render_clear(unsigned long long* __restrict__ keys, int64_t n_pix,
                                                             unsigned long long* __restrict__ count) {
  const int64_t stride = (int64_t)gridDim.x * MESH_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x; i < n_pix; i += stride) keys[i] = MESH_RENDER_NO_KEY;
  if (blockIdx.x == 0 && threadIdx.x == 0) *count = 0ull;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_render_project(const double* __restrict__ proj, int64_t n_vertices,
                                                               const double* __restrict__ vertices, double* __restrict__ projected) {
  const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const int64_t cam = blockIdx.y;
  const Vertex p = mesh_render::project(proj + cam * 12, vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]);
  double* out = projected + (cam * n_vertices + i) * 3;
  out[0] = p.u; out[1] = p.v; out[2] = p.q2;
}

__device__ __forceinline__ Vertex load_vertex(const double* __restrict__ projected, int64_t i) {
  Vertex p;
  p.u = projected[3 * i]; p.v = projected[3 * i + 1]; p.q2 = projected[3 * i + 2];
  return p;
}

// the corners of triangle t as camera `cam` sees them and its box; false when it draws nothing
__device__ __forceinline__ bool load_triangle(const int32_t* __restrict__ triangles, int64_t t, int64_t n_vertices,
                                              const double* __restrict__ cam_projected, int w, int h, Vertex& a, Vertex& b, Vertex& c,
                                              mesh_render::Box& bx) {
  const int64_t c0 = triangles[3 * t], c1 = triangles[3 * t + 1], c2 = triangles[3 * t + 2];
  if (!(c0 >= 0 && c0 < n_vertices && c1 >= 0 && c1 < n_vertices && c2 >= 0 && c2 < n_vertices)) return false;   // nothing read through it
  a = load_vertex(cam_projected, c0);
  b = load_vertex(cam_projected, c1);
  c = load_vertex(cam_projected, c2);
  if (!mesh_render::usable(a, b, c)) return false;
  bx = mesh_render::box(a, b, c, w, h);
  return !bx.empty;
}

__device__ __forceinline__ void draw(const Vertex& a, const Vertex& b, const Vertex& c, int x, int y, int64_t t,
                                     unsigned long long* __restrict__ cam_keys, int w) {
  const uint64_t k = mesh_render::claim(a, b, c, x, y, t);
  if (k != MESH_RENDER_NO_KEY) atomicMin(cam_keys + ((int64_t)y * w + x), (unsigned long long)k);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_render_raster(const TsdfView* __restrict__ cams, int64_t n_vertices, int64_t n_triangles,
                                                              const int32_t* __restrict__ triangles, const double* __restrict__ projected,
                                                              unsigned long long* __restrict__ keys, unsigned long long* __restrict__ list,
                                                              unsigned long long* __restrict__ list_count) {
  const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  const int64_t cam = blockIdx.y;
  const TsdfView view = cams[cam];
  bool push = false;
  if (t < n_triangles) {
    Vertex a, b, c;
    mesh_render::Box bx;
    if (load_triangle(triangles, t, n_vertices, projected + cam * n_vertices * 3, view.w, view.h, a, b, c, bx)) {
      if (mesh_render::box_pixels(bx) > MESH_RENDER_SMALL_BOX) {
        push = true;
      } else {
        unsigned long long* cam_keys = keys + view.out_off;
        for (int y = bx.y0; y <= bx.y1; ++y)
          for (int x = bx.x0; x <= bx.x1; ++x) draw(a, b, c, x, y, t, cam_keys, view.w);
      }
    }
  }
  // every lane of the wavefront is here again.  A (camera, triangle) pair is pushed at most once: a slot stays below
  // n_cam * n_triangles, the capacity of the list.
  const unsigned long long flagged = __ballot(push);
  if (flagged) {
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)flagged) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(list_count, (unsigned long long)__popcll(flagged));
    base = __shfl(base, leader, 64);
    if (push) list[base + (unsigned long long)__popcll(flagged & ((1ull << lane) - 1ull))] = ((unsigned long long)cam << 32) | (unsigned long long)t;
  }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_render_raster_large(const TsdfView* __restrict__ cams, int64_t n_cam, int64_t n_vertices,
                                                                    int64_t n_triangles, const int32_t* __restrict__ triangles,
                                                                    const double* __restrict__ projected, unsigned long long* __restrict__ keys,
                                                                    const unsigned long long* __restrict__ list,
                                                                    const unsigned long long* __restrict__ list_count, int64_t capacity) {
  const unsigned long long counted = *list_count;
  const int64_t n_list = counted > (unsigned long long)capacity ? capacity : (int64_t)counted;
  for (int64_t e = blockIdx.x; e < n_list; e += gridDim.x) {
    const unsigned long long entry = list[e];
    const int64_t cam = (int64_t)(entry >> 32), t = (int64_t)(entry & 0xFFFFFFFFull);
    if (cam >= n_cam || t >= n_triangles) continue;                // the same in every thread
    const TsdfView view = cams[cam];
    Vertex a, b, c;
    mesh_render::Box bx;
    if (!load_triangle(triangles, t, n_vertices, projected + cam * n_vertices * 3, view.w, view.h, a, b, c, bx)) continue;
    const int bw = bx.x1 - bx.x0 + 1;
    const int64_t n = mesh_render::box_pixels(bx);
    unsigned long long* cam_keys = keys + view.out_off;
    for (int64_t p = threadIdx.x; p < n; p += MESH_BLOCK) draw(a, b, c, bx.x0 + (int)(p % bw), bx.y0 + (int)(p / bw), t, cam_keys, view.w);
  }
}

template <int MODE, int CH>
__global__ __launch_bounds__(MESH_BLOCK) void k_render_resolve(const TsdfView* __restrict__ cams, int64_t n_vertices, int64_t n_triangles,
                                                               const int32_t* __restrict__ triangles, const double* __restrict__ projected,
                                                               const unsigned long long* __restrict__ keys,
                                                               const uint8_t* __restrict__ vertex_colors, const float* __restrict__ uv,
                                                               const uint8_t* __restrict__ atlas, int atlas_w, int atlas_h, int fill,
                                                               uint32_t* __restrict__ depth, int32_t* __restrict__ triangle,
                                                               float* __restrict__ bary, uint8_t* __restrict__ color) {
  const int64_t cam = blockIdx.y;
  const TsdfView view = cams[cam];
  const int64_t p = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (p >= (int64_t)view.h * view.w) return;
  const int64_t at = view.out_off + p;
  const uint64_t k = keys[at];
  int64_t t = -1;
  int64_t c0 = 0, c1 = 0, c2 = 0;
  if (k != MESH_RENDER_NO_KEY) {
    t = mesh_render::key_triangle(k);
    if (t < n_triangles) {
      c0 = triangles[3 * t]; c1 = triangles[3 * t + 1]; c2 = triangles[3 * t + 2];
    }
    // only a triangle that passed these checks in the raster pass can be in a key
    if (!(t < n_triangles && c0 >= 0 && c0 < n_vertices && c1 >= 0 && c1 < n_vertices && c2 >= 0 && c2 < n_vertices)) t = -1;
  }
  if (t < 0) {
    depth[at] = MESH_RENDER_NAN_BITS;
    triangle[at] = -1;
    bary[3 * at] = 0.0f; bary[3 * at + 1] = 0.0f; bary[3 * at + 2] = 0.0f;
    if (MODE != MESH_RENDER_NONE) {
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) color[at * CH + ch] = (uint8_t)fill;
    }
    return;
  }
  const double* cam_projected = projected + cam * n_vertices * 3;
  const Vertex a = load_vertex(cam_projected, c0), b = load_vertex(cam_projected, c1), c = load_vertex(cam_projected, c2);
  double bk[3];
  mesh_render::bary(a, b, c, (int)(p % view.w), (int)(p / view.w), bk);
  depth[at] = mesh_render::key_depth_bits(k);
  triangle[at] = (int32_t)t;
  bary[3 * at] = (float)bk[0]; bary[3 * at + 1] = (float)bk[1]; bary[3 * at + 2] = (float)bk[2];
  if (MODE == MESH_RENDER_VERTEX) {
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
      color[at * CH + ch] = mesh_render::shade(bk, (double)vertex_colors[c0 * CH + ch], (double)vertex_colors[c1 * CH + ch],
                                               (double)vertex_colors[c2 * CH + ch]);
  }
  if (MODE == MESH_RENDER_ATLAS) {
    const float* q = uv + 6 * t;
    const double px = mesh_render::atlas_pos(bk, q[0], q[2], q[4], atlas_w), py = mesh_render::atlas_pos(bk, q[1], q[3], q[5], atlas_h);
    const mesh_color::Taps tp = mesh_render::taps(px, py, atlas_w, atlas_h);
    const int64_t r0 = (int64_t)tp.y0 * atlas_w, r1 = (int64_t)tp.y1 * atlas_w;
    const int64_t e[4] = {(r0 + tp.x0) * CH, (r0 + tp.x1) * CH, (r1 + tp.x0) * CH, (r1 + tp.x1) * CH};
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
      color[at * CH + ch] = mesh_render::sample((double)atlas[e[0] + ch], (double)atlas[e[1] + ch], (double)atlas[e[2] + ch],
                                                (double)atlas[e[3] + ch], tp);
  }
}

}  // namespace

extern "C" int sfm_mesh_render_workspace_bytes(int32_t n_cam, const int32_t* heights, const int32_t* widths, int64_t n_vertices,
                                               int64_t n_triangles, int64_t* bytes_host) {
  if (!bytes_host) return SFM_ERR_ARG;
  int64_t n_pix = 0;
  if (mesh_render_check_cameras(n_cam, heights, widths, nullptr, &n_pix, nullptr) || mesh_render_check_mesh(n_vertices, n_triangles)) return SFM_ERR_ARG;
  *bytes_host = mesh_render_layout(n_cam, n_pix, n_vertices, n_triangles).bytes;
  return SFM_OK;
}

extern "C" int sfm_mesh_render(sfm_handle h, int32_t n_cam, const int32_t* heights, const int32_t* widths, const double* proj, int64_t n_vertices,
                               const double* vertices, int64_t n_triangles, const int32_t* triangles, int32_t color_mode, int32_t channels,
                               const uint8_t* vertex_colors, const float* uv, const uint8_t* atlas, int32_t atlas_w, int32_t atlas_h, int32_t fill,
                               float* depth, int32_t* triangle, float* bary, uint8_t* color, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_render";
  std::vector<TsdfView> cams((size_t)(n_cam > 0 && n_cam <= MESH_RENDER_MAX_CAMERAS ? n_cam : 0) + 1);
  int64_t n_pix = 0, max_pix = 0;
  int bad = mesh_render_check_cameras(n_cam, heights, widths, cams.data(), &n_pix, &max_pix);
  if (!bad) bad = mesh_render_check_mesh(n_vertices, n_triangles);
  if (!bad) bad = mesh_render_check_color(color_mode, channels, fill, n_triangles, atlas_w, atlas_h);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_RENDER_WHY[bad]);
  const MeshRenderLayout L = mesh_render_layout(n_cam, n_pix, n_vertices, n_triangles);
  bad = mesh_render_check_buffers(n_cam, n_pix, n_vertices, n_triangles, color_mode, L.bytes, proj, vertices, triangles, vertex_colors, uv, atlas, depth,
                                  triangle, bary, color, workspace, workspace_bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_RENDER_WHY[bad]);
  char* ws = (char*)workspace;
  unsigned long long* count = (unsigned long long*)(ws + L.count);
  const TsdfView* d_cams = (const TsdfView*)(ws + L.cameras);
  unsigned long long* keys = (unsigned long long*)(ws + L.keys);
  double* projected = (double*)(ws + L.projected);
  unsigned long long* list = (unsigned long long*)(ws + L.list);
  const dim3 block(MESH_BLOCK);
  hipLaunchKernelGGL(k_render_clear, dim3((unsigned)mesh_render_clear_groups(n_pix)), block, 0, h->stream, keys, n_pix, count);
  SFM_LAUNCH_CHECK(h, what);
  if (n_pix == 0) return SFM_OK;                                   // no pixel: nothing to draw and nothing to write
  // the camera table is pageable host memory: the copy must have left it on return
  SFM_HIP(h, hipMemcpyAsync(ws + L.cameras, cams.data(), cams.size() * sizeof(TsdfView), hipMemcpyHostToDevice, h->stream));
  SFM_HIP(h, hipStreamSynchronize(h->stream));
  if (n_triangles > 0 && n_vertices > 0) {
    hipLaunchKernelGGL(k_render_project, dim3((unsigned)mesh_render_blocks(n_vertices), (unsigned)n_cam), block, 0, h->stream, proj, n_vertices,
                       vertices, projected);
    SFM_LAUNCH_CHECK(h, what);
    hipLaunchKernelGGL(k_render_raster, dim3((unsigned)mesh_render_blocks(n_triangles), (unsigned)n_cam), block, 0, h->stream, d_cams, n_vertices,
                       n_triangles, triangles, projected, keys, list, count);
    SFM_LAUNCH_CHECK(h, what);
    hipLaunchKernelGGL(k_render_raster_large, dim3(MESH_RENDER_LARGE_GROUPS), block, 0, h->stream, d_cams, (int64_t)n_cam, n_vertices, n_triangles,
                       triangles, projected, keys, list, count, L.list_capacity);
    SFM_LAUNCH_CHECK(h, what);
  }
  const dim3 grid((unsigned)mesh_render_blocks(max_pix), (unsigned)n_cam);
#define SFM_RENDER_RESOLVE(MODE, CH)                                                                                                              \
  hipLaunchKernelGGL((k_render_resolve<MODE, CH>), grid, block, 0, h->stream, d_cams, n_vertices, n_triangles, triangles, projected, keys,       \
                     vertex_colors, uv, atlas, (int)atlas_w, (int)atlas_h, (int)fill, (uint32_t*)depth, triangle, bary, color)
  if (color_mode == MESH_RENDER_NONE) SFM_RENDER_RESOLVE(MESH_RENDER_NONE, 1);
  else if (color_mode == MESH_RENDER_VERTEX && channels == 1) SFM_RENDER_RESOLVE(MESH_RENDER_VERTEX, 1);
  else if (color_mode == MESH_RENDER_VERTEX) SFM_RENDER_RESOLVE(MESH_RENDER_VERTEX, 3);
  else if (channels == 1) SFM_RENDER_RESOLVE(MESH_RENDER_ATLAS, 1);
  else SFM_RENDER_RESOLVE(MESH_RENDER_ATLAS, 3);
#undef SFM_RENDER_RESOLVE
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}
