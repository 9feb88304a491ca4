// Integration of the depth maps of a call into a truncated signed distance volume for gfx950 (MI355X).
// include/sfm_amd.h states the rule; tsdf_rule.h holds its floating point (float64, no FMA contraction), mesh_plan.h the
// view table, the workspace and the argument checks.
//
// One thread per node, x fastest, MESH_BLOCK consecutive nodes per workgroup.  The views are walked in position order by
// every thread alike: the view record and the 12 numbers of its projection are wave-uniform reads, the depth and the keep
// flag at the node's pixel are the gather.  A pure function of its inputs: no atomics, no visit order.
#include "common.h"
#include "tsdf_rule.h"
#include "mesh_plan.h"
#include "view_table.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(MESH_BLOCK) void k_tsdf_integrate(const TsdfView* __restrict__ views, int n_ref, const double* __restrict__ proj,
                                                               const float* __restrict__ depth_in, const uint8_t* __restrict__ keep,
                                                               double o0, double o1, double o2, double voxel, int nx, int ny, int nz,
                                                               double trunc, uint32_t* __restrict__ tsdf_bits, uint16_t* __restrict__ weight) {
  const int64_t n = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (n >= mesh_nodes(nx, ny, nz)) return;
  const int i = (int)(n % nx), j = (int)((n / nx) % ny), k = (int)(n / ((int64_t)nx * ny));
  const double X0 = tsdf::node_coord(o0, voxel, i), X1 = tsdf::node_coord(o1, voxel, j), X2 = tsdf::node_coord(o2, voxel, k);
  double acc = 0.0;
  int w = 0;
  for (int v = 0; v < n_ref; ++v) {
    const TsdfView view = views[v];
    const tsdf::Projection p = tsdf::project(proj + (int64_t)v * 12, X0, X1, X2, view.w, view.h);
    if (!p.valid) continue;                                    // never valid in a view without a pixel
    const int64_t e = view.out_off + (int64_t)p.yi * view.w + p.xi;
    w += tsdf::add_view((double)depth_in[e], keep ? keep[e] != 0 : 1, p.q2, trunc, &acc);
  }
  tsdf_bits[n] = tsdf::finish_bits(acc, w);
  weight[n] = (uint16_t)w;
}

}  // namespace

extern "C" int sfm_tsdf_workspace_bytes(int32_t n_ref, int64_t* bytes_host) {
  if (!bytes_host || n_ref < 0 || n_ref > TSDF_MAX_VIEWS) return SFM_ERR_ARG;
  *bytes_host = tsdf_workspace_bytes(n_ref);
  return SFM_OK;
}

extern "C" int sfm_tsdf_integrate(sfm_handle h, const int32_t* heights, const int32_t* widths, int32_t n_img, int32_t n_ref,
                                  const int32_t* ref_image, const double* proj, const float* depth, const uint8_t* keep, const double* origin,
                                  double voxel, int32_t nx, int32_t ny, int32_t nz, double trunc, float* tsdf, uint16_t* weight,
                                  void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_tsdf_integrate";
  ViewTable views;
  int bad = view_table_build(n_img, heights, widths, n_ref, ref_image, &views);
  if (!bad) bad = mesh_check_grid(nx, ny, nz);
  if (!bad) bad = mesh_check_frame(origin, voxel);
  if (!bad) bad = tsdf_check_trunc(trunc);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_WHY[bad]);
  if (!workspace || workspace_bytes < tsdf_workspace_bytes(n_ref)) return sfm_fail(h, SFM_ERR_ARG, what, "workspace missing or too small");
  if (!tsdf || !weight || (n_ref > 0 && !proj) || (views.n_out > 0 && !depth)) return sfm_fail(h, SFM_ERR_ARG, what, "null pointer");
  if (const int rc = sfm_put_views(h, views, workspace)) return rc;
  const int64_t n_nodes = mesh_nodes(nx, ny, nz);
  hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)mesh_blocks(n_nodes)), dim3(MESH_BLOCK), 0, h->stream, (const TsdfView*)workspace, n_ref,
                     proj, depth, keep, origin[0], origin[1], origin[2], voxel, nx, ny, nz, trunc, (uint32_t*)tsdf, weight);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}
