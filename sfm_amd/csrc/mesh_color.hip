// Per-vertex colours of a mesh, blended over the views that see the vertex, for gfx950 (MI355X).
// include/sfm_amd.h states the rule; mesh_color_rule.h holds its floating point (float64, no FMA contraction),
// mesh_color_plan.h the argument checks and the workspace, mesh_plan.h the view table.
//
// One thread per vertex, MESH_BLOCK consecutive vertices per workgroup; the vertices come in (node, direction) order, so
// neighbouring lanes project to neighbouring pixels.  The view record, the 12 numbers of its projection and its centre are
// wave-uniform reads.  Per view a thread has two dependent round trips - the depth and the keep flag at the nearest pixel,
// then the 4 x channels bytes around (u, v) - and a mesh of 1e5 vertices is under two waves per SIMD, so nothing hides
// them: the thread takes MESH_COLOR_BATCH views at a time, asks for all their depths, then for all their pixels, and only
// then adds them up, strictly in view order, so that the bytes are those of the one-view-at-a-time loop.
// A pure function of its inputs: no atomics, no visit order.
#include "common.h"
#include "mesh_color_rule.h"
#include "mesh_color_plan.h"
#include "view_table.h"

#pragma clang fp contract(off)

namespace {

template <int CH, int BATCH>
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_colors(const TsdfView* __restrict__ views, int n_ref, const double* __restrict__ proj,
                                                            const double* __restrict__ centres, const float* __restrict__ depth_in,
                                                            const uint8_t* __restrict__ keep, const uint8_t* __restrict__ pixels,
                                                            int64_t n_vertices, const double* __restrict__ vertices,
                                                            const float* __restrict__ normals, double tol, double min_cos, int fill,
                                                            uint8_t* __restrict__ colors, uint8_t* __restrict__ n_views,
                                                            int32_t* __restrict__ best_view) {
  const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (i >= n_vertices) return;
  const double X[3] = {vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]};
  const double n[3] = {(double)normals[3 * i], (double)normals[3 * i + 1], (double)normals[3 * i + 2]};
  double acc[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) acc[k] = 0.0;
  mesh_color::Tally tally = mesh_color::empty_tally();
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
        const double s = mesh_color::bilinear((double)px[b][k], (double)px[b][CH + k], (double)px[b][2 * CH + k], (double)px[b][3 * CH + k],
                                              t[b].fx, t[b].fy);
        acc[k] = mesh_color::add_sample(acc[k], wgt[b], s);
      }
      mesh_color::add_view(&tally, wgt[b], v0 + b);
    }
  }
#pragma unroll
  for (int k = 0; k < CH; ++k) colors[i * CH + k] = mesh_color::finish(acc[k], tally, fill);
  n_views[i] = mesh_color::finish_views(tally);
  best_view[i] = tally.best;
}

}  // namespace

extern "C" int sfm_mesh_colors_workspace_bytes(int32_t n_ref, int64_t* bytes_host) {
  if (!bytes_host || n_ref < 0 || n_ref > TSDF_MAX_VIEWS) return SFM_ERR_ARG;
  *bytes_host = mesh_color_workspace_bytes(n_ref);
  return SFM_OK;
}

extern "C" int sfm_mesh_colors(sfm_handle h, const int32_t* heights, const int32_t* widths, int32_t n_img, int32_t n_ref,
                               const int32_t* ref_image, const double* proj, const double* centres, const float* depth, const uint8_t* keep,
                               const uint8_t* pixels, int32_t channels, int64_t n_vertices, const double* vertices, const float* normals,
                               double tol, double min_cos, int32_t fill, uint8_t* colors, uint8_t* n_views, int32_t* best_view,
                               void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_colors";
  ViewTable views;
  int bad = view_table_build(n_img, heights, widths, n_ref, ref_image, &views);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_WHY[bad]);
  bad = mesh_color_check(channels, n_vertices, tol, min_cos, fill);
  if (!bad) bad = mesh_color_check_buffers(n_ref, views.n_out, n_vertices, proj, centres, depth, pixels, vertices, normals, colors, n_views,
                                           best_view, workspace, workspace_bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_COLOR_WHY[bad]);
  if (n_vertices == 0) return SFM_OK;
  if (const int rc = sfm_put_views(h, views, workspace)) return rc;
  const dim3 grid((unsigned)mesh_color_blocks(n_vertices)), block(MESH_BLOCK);
  if (channels == 1)
    hipLaunchKernelGGL((k_mesh_colors<1, MESH_COLOR_BATCH>), grid, block, 0, h->stream, (const TsdfView*)workspace, n_ref, proj, centres, depth,
                       keep, pixels, n_vertices, vertices, normals, tol, min_cos, (int)fill, colors, n_views, best_view);
  else
    hipLaunchKernelGGL((k_mesh_colors<3, MESH_COLOR_BATCH>), grid, block, 0, h->stream, (const TsdfView*)workspace, n_ref, proj, centres, depth,
                       keep, pixels, n_vertices, vertices, normals, tol, min_cos, (int)fill, colors, n_views, best_view);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}
