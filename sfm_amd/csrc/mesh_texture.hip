// A texture atlas for a mesh: one patch of texels per triangle, every texel blended over the views that see its point, for
// gfx950 (MI355X).  include/sfm_amd.h states the rule; mesh_texture_rule.h holds the layout and the point of a texel,
// mesh_color_rule.h the per-view floating point (float64, no FMA contraction), mesh_texture_plan.h the size of the atlas,
// the argument checks and the grid.
//
// One thread per texel over tiles of 64 x 4 texels: a wavefront is 64 neighbouring texels of one row, so its stores are
// contiguous and its lanes are texels of the same or the next triangles - which come in (cell, tetrahedron) order, so they
// project to neighbouring pixels.  The three corners of a texel's triangle are read by every lane that shares it (one
// request per distinct address; they stay in L1/L2) and are not staged in LDS.  The view record, the 12 numbers of its
// projection and its centre are wave-uniform reads.  The launch has a thread per texel - 1e7 for a mesh of 2e5 triangles -
// so occupancy hides the two dependent round trips per view and the thread takes MESH_TEXTURE_BATCH = 1 view at a time; the
// batch is a template parameter as in k_mesh_colors, and the sums stay strictly in view order whatever it is.  The walk over
// the views stands here as it does in k_mesh_colors, on the same functions of mesh_color_rule.h: moved into one inlined
// function for both kernels it cost the colouring 4.5 % (tools/experiments/README.md).  k_exposure_sample
// (mesh_exposure.hip) is the third place where the walk stands; what the host does around the three is spelt once
// (ViewTable in mesh_plan.h, view_table.h).
// A pure function of its inputs: no atomics, no visit order.
#include "common.h"
#include "mesh_texture_rule.h"
#include "mesh_texture_plan.h"
#include "view_table.h"

#pragma clang fp contract(off)

namespace {

template <int CH, int BATCH>
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_texture(const TsdfView* __restrict__ views, int n_ref, const double* __restrict__ proj,
                                                             const double* __restrict__ centres, const float* __restrict__ depth_in,
                                                             const uint8_t* __restrict__ keep, const uint8_t* __restrict__ pixels,
                                                             int64_t n_vertices, const double* __restrict__ vertices,
                                                             const float* __restrict__ normals, int64_t n_triangles,
                                                             const int32_t* __restrict__ triangles, int s, int cells_per_row, int W, int H,
                                                             double tol, double min_cos, int fill, uint8_t* __restrict__ texture,
                                                             uint8_t* __restrict__ n_views) {
  const int x = (int)blockIdx.x * MESH_TEXTURE_TILE_X + (int)(threadIdx.x % MESH_TEXTURE_TILE_X);
  const int y = (int)blockIdx.y * MESH_TEXTURE_TILE_Y + (int)(threadIdx.x / MESH_TEXTURE_TILE_X);
  if (x >= W || y >= H) return;
  const int64_t at_texel = (int64_t)y * W + x;
  double acc[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) acc[k] = 0.0;
  mesh_color::Tally tally = mesh_color::empty_tally();
  const mesh_texture::Texel tx = mesh_texture::texel_of(x, y, s, cells_per_row, n_triangles);
  bool owned = tx.tri >= 0;
  int64_t c0 = 0, c1 = 0, c2 = 0;
  if (owned) {
    c0 = triangles[3 * tx.tri]; c1 = triangles[3 * tx.tri + 1]; c2 = triangles[3 * tx.tri + 2];
    owned = c0 >= 0 && c0 < n_vertices && c1 >= 0 && c1 < n_vertices && c2 >= 0 && c2 < n_vertices;      // a bad index: no view, nothing read
  }
  if (owned) {
    double V[3][3], m[3][3], X[3], n[3];
    const int64_t corner[3] = {c0, c1, c2};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        V[k][a] = vertices[3 * corner[k] + a];
        m[k][a] = (double)normals[3 * corner[k] + a];
      }
    mesh_texture::point_and_normal(mesh_texture::numerators(tx.i, tx.j, s), V[0], V[1], V[2], m[0], m[1], m[2], s, X, n);
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
        if (v < n_ref) {                                         // wave-uniform
          view[b] = views[v];
          p[b] = mesh_color::project(proj + (int64_t)v * 12, X[0], X[1], X[2], view[b].w, view[b].h);
          if (p[b].valid) {                                      // never valid in a view without a pixel
            const int64_t e = view[b].out_off + (int64_t)p[b].yi * view[b].w + p[b].xi;
            ds[b] = depth_in[e];
            if (keep) kept[b] = keep[e];
          }
        }
      }
      // round trip two: the four pixels of every view that counts
      double wgt[BATCH];
      mesh_color::Taps t[BATCH];
      uint8_t px[BATCH][4 * CH];
      bool use[BATCH];
#pragma unroll
      for (int b = 0; b < BATCH; ++b) {
        use[b] = p[b].valid && mesh_color::sees((double)ds[b], kept[b] != 0, p[b].q2, tol) &&
                 mesh_color::weight(centres + (int64_t)(v0 + b) * 3, X, n, min_cos, &wgt[b]);
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
      // the sums, in view order
#pragma unroll
      for (int b = 0; b < BATCH; ++b) {
        if (!use[b]) continue;
#pragma unroll
        for (int k = 0; k < CH; ++k) {
          const double smp = mesh_color::bilinear((double)px[b][k], (double)px[b][CH + k], (double)px[b][2 * CH + k], (double)px[b][3 * CH + k],
                                                  t[b].fx, t[b].fy);
          acc[k] = mesh_color::add_sample(acc[k], wgt[b], smp);
        }
        mesh_color::add_view(&tally, wgt[b], v0 + b);
      }
    }
  }
  // a texel of no triangle, or of one with a bad index, has an empty tally: fill and 0
#pragma unroll
  for (int k = 0; k < CH; ++k) texture[at_texel * CH + k] = mesh_color::finish(acc[k], tally, fill);
  n_views[at_texel] = mesh_color::finish_views(tally);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_texture_uv(int64_t n_triangles, int s, int cells_per_row, int W, int H, float* __restrict__ uv) {
  const int64_t t = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (t >= n_triangles) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float q[2];
    mesh_texture::corner_uv(t, k, s, cells_per_row, W, H, q);
    uv[6 * t + 2 * k] = q[0];
    uv[6 * t + 2 * k + 1] = q[1];
  }
}

}  // namespace

extern "C" int sfm_mesh_texture_size(int64_t n_triangles, int32_t texels, int32_t cells_per_row, int32_t* width_host, int32_t* height_host) {
  if (!width_host || !height_host) return SFM_ERR_ARG;
  return mesh_texture_size(n_triangles, texels, cells_per_row, width_host, height_host) ? SFM_ERR_ARG : SFM_OK;
}

extern "C" int sfm_mesh_texture_workspace_bytes(int32_t n_ref, int64_t* bytes_host) {
  if (!bytes_host || n_ref < 0 || n_ref > TSDF_MAX_VIEWS) return SFM_ERR_ARG;
  *bytes_host = mesh_texture_workspace_bytes(n_ref);
  return SFM_OK;
}

extern "C" int sfm_mesh_texture(sfm_handle h, const int32_t* heights, const int32_t* widths, int32_t n_img, int32_t n_ref, const int32_t* ref_image,
                                const double* proj, const double* centres, const float* depth, const uint8_t* keep, const uint8_t* pixels,
                                int32_t channels, int64_t n_vertices, const double* vertices, const float* normals, int64_t n_triangles,
                                const int32_t* triangles, int32_t texels, int32_t cells_per_row, double tol, double min_cos, int32_t fill,
                                uint8_t* texture, uint8_t* views_out, float* uv, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_texture";
  ViewTable views;
  int bad = view_table_build(n_img, heights, widths, n_ref, ref_image, &views);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_WHY[bad]);
  bad = mesh_color_check(channels, n_vertices, tol, min_cos, fill);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_COLOR_WHY[bad]);
  int32_t W = 0, H = 0;
  bad = mesh_texture_size(n_triangles, texels, cells_per_row, &W, &H);
  if (!bad) bad = mesh_texture_check_buffers(n_ref, views.n_out, n_vertices, n_triangles, proj, centres, depth, pixels, vertices, normals,
                                             triangles, texture, views_out, uv, workspace, workspace_bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_TEXTURE_WHY[bad]);
  if (n_triangles == 0) return SFM_OK;
  if (const int rc = sfm_put_views(h, views, workspace)) return rc;
  const dim3 grid((unsigned)mesh_texture_tiles_x(W), (unsigned)mesh_texture_tiles_y(H)), block(MESH_BLOCK);
  if (channels == 1)
    hipLaunchKernelGGL((k_mesh_texture<1, MESH_TEXTURE_BATCH>), grid, block, 0, h->stream, (const TsdfView*)workspace, n_ref, proj, centres, depth,
                       keep, pixels, n_vertices, vertices, normals, n_triangles, triangles, (int)texels, (int)cells_per_row, (int)W, (int)H, tol,
                       min_cos, (int)fill, texture, views_out);
  else
    hipLaunchKernelGGL((k_mesh_texture<3, MESH_TEXTURE_BATCH>), grid, block, 0, h->stream, (const TsdfView*)workspace, n_ref, proj, centres, depth,
                       keep, pixels, n_vertices, vertices, normals, n_triangles, triangles, (int)texels, (int)cells_per_row, (int)W, (int)H, tol,
                       min_cos, (int)fill, texture, views_out);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_mesh_texture_uv, dim3((unsigned)mesh_texture_uv_blocks(n_triangles)), block, 0, h->stream, n_triangles, (int)texels,
                     (int)cells_per_row, (int)W, (int)H, uv);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}
