// The one host step the four per-view calls share after their checks (sfm_tsdf_integrate, sfm_mesh_colors, sfm_mesh_texture,
// sfm_mesh_exposure_sample): the ViewTable of mesh_plan.h goes to the start of the workspace, where the kernels read it.
#pragma once
#include "common.h"
#include "mesh_plan.h"

// The table is pageable host memory that dies with the caller's frame: the copy must have left it on return, hence the
// synchronise.  The workspace holds tsdf_workspace_bytes(n_ref) bytes or more; the caller has checked that.
static inline int sfm_put_views(sfm_ctx* h, const ViewTable& views, void* workspace) {
  SFM_HIP(h, hipMemcpyAsync(workspace, views.views.data(), views.views.size() * sizeof(TsdfView), hipMemcpyHostToDevice, h->stream));
  SFM_HIP(h, hipStreamSynchronize(h->stream));
  return SFM_OK;
}
