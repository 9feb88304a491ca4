// Fusion of the depth maps of a call into one cloud with normals for gfx950 (MI355X): a normal map per view, the agreeing
// partners and the owner of every kept pixel, a two-level exclusive scan of the owner counts, and the gather of the fused
// points.  include/sfm_amd.h states the rule; depth_rule.h holds its floating-point pieces (float64, no FMA contraction),
// depth_plan.h the block counts and the workspace layout; count, scan and rank are those of block_scan.h / scan_plan.h.
//
// Every kernel is one thread per pixel over the pixel blocks of the filter (DEPTH_PIXEL_BLOCK pixels of one view).  The
// rule is a pure function of the filter's outputs: no visit order, no global atomics, nothing waits on another workgroup.
// k_depth_fuse_mark counts the owners of its block with one ballot per wavefront; the scan turns the
// counts into the first output slot of every block; k_depth_fuse_gather ranks an owner inside its block by the ballots
// of the wavefronts in front of it and the lanes below it, and re-reads the partners that agree_mask names through the
// sample rule: partner coordinates are never stored.
#include "common.h"
#include "depth_rule.h"
#include "depth_plan.h"
#include "block_scan.h"

#pragma clang fp contract(off)

namespace {

constexpr int FUSE_WAVES = DEPTH_PIXEL_BLOCK / 64;

struct FusePixel { int v; int64_t p, o; int x, y; bool in; };

// the pixel of this thread: view, index in the view, element of the outputs; in = false behind the view's last pixel
__device__ __forceinline__ FusePixel fuse_pixel(const DepthImage* __restrict__ images, const DepthView* __restrict__ views, int n_ref,
                                                DepthView* view, DepthImage* ref) {
  FusePixel q;
  q.v = depth_find_view(views, n_ref, blockIdx.x, DEPTH_BY_PIXEL_BLOCK);
  *view = views[q.v];
  *ref = images[view->image];
  q.p = ((int64_t)blockIdx.x - view->pix_block_first) * DEPTH_PIXEL_BLOCK + threadIdx.x;
  q.in = q.p < (int64_t)ref->h * ref->w;
  q.o = view->out_off + q.p;
  q.x = q.in ? (int)(q.p % ref->w) : 0;
  q.y = q.in ? (int)(q.p / ref->w) : 0;
  return q;
}

__global__ __launch_bounds__(DEPTH_PIXEL_BLOCK) void k_depth_normals(const DepthImage* __restrict__ images, const DepthView* __restrict__ views,
                                                                     int n_ref, const double* __restrict__ backproj,
                                                                     const float* __restrict__ depth_in, const double* __restrict__ xyz,
                                                                     int step, double jump, float* __restrict__ normal_map) {
  DepthView view; DepthImage ref;
  const FusePixel q = fuse_pixel(images, views, n_ref, &view, &ref);
  if (!q.in) return;
  // the neighbours at clamp(x +- t), clamp(y +- t), in the order of depth::view_normal
  const int64_t nb[4] = {view.out_off + (int64_t)q.y * ref.w + depth_clamp(q.x + step, ref.w - 1),
                         view.out_off + (int64_t)q.y * ref.w + depth_clamp(q.x - step, ref.w - 1),
                         view.out_off + (int64_t)depth_clamp(q.y + step, ref.h - 1) * ref.w + q.x,
                         view.out_off + (int64_t)depth_clamp(q.y - step, ref.h - 1) * ref.w + q.x};
  double dn[4], P[4][3], X[3], C[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    dn[k] = (double)depth_in[nb[k]];
#pragma unroll
    for (int i = 0; i < 3; ++i) P[k][i] = xyz[nb[k] * 3 + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) { X[i] = xyz[q.o * 3 + i]; C[i] = backproj[(int64_t)q.v * 12 + 4 * i + 3]; }
  float n[3];
  depth::view_normal((double)depth_in[q.o], X, dn, P[0], P[1], P[2], P[3], C, jump, n);
#pragma unroll
  for (int i = 0; i < 3; ++i) normal_map[q.o * 3 + i] = n[i];
}

// where entry e of a view's sources lands for the pixel (x, y) at depth d: the element of the outputs of the source's own
// maps, or -1 when the source has none or the sample is not valid; q2 is the depth in the source
__device__ __forceinline__ int64_t fuse_partner(const DepthImage* __restrict__ images, const DepthView* __restrict__ views,
                                                const int32_t* __restrict__ src_image, const int32_t* __restrict__ ref_of_image,
                                                const double* __restrict__ warps, int e, double x, double y, double d, int* rs_out,
                                                double* q2) {
  const int si = src_image[e];
  const int rs = ref_of_image[si];
  *rs_out = rs;
  if (rs < 0) return -1;
  const DepthImage src = images[si];
  const depth::Sample smp = depth::sample(warps + (int64_t)e * 12, x, y, d, src.w, src.h);
  *q2 = smp.q2;
  if (!smp.valid) return -1;
  return views[rs].out_off + (int64_t)smp.yi * src.w + smp.xi;
}

__global__ __launch_bounds__(DEPTH_PIXEL_BLOCK) void k_depth_fuse_mark(const DepthImage* __restrict__ images, const DepthView* __restrict__ views,
                                                                       int n_ref, const int32_t* __restrict__ src_image,
                                                                       const int32_t* __restrict__ ref_of_image, const double* __restrict__ warps,
                                                                       const float* __restrict__ depth_in, const uint8_t* __restrict__ keep,
                                                                       double rel_tol, uint8_t* __restrict__ agree_mask,
                                                                       uint8_t* __restrict__ owner, uint32_t* __restrict__ blk) {
  __shared__ int s_wave[FUSE_WAVES];
  DepthView view; DepthImage ref;
  const FusePixel q = fuse_pixel(images, views, n_ref, &view, &ref);
  unsigned mask = 0;
  bool own = false;
  if (q.in && keep[q.o] != 0) {
    own = true;
    const double d = (double)depth_in[q.o];
    for (int s = 0; s < view.n_src; ++s) {
      int rs; double q2;
      const int64_t po = fuse_partner(images, views, src_image, ref_of_image, warps, view.src_first + s, (double)q.x, (double)q.y, d, &rs, &q2);
      if (po < 0) continue;
      if (!depth::agrees((double)depth_in[po], q2, rel_tol) || keep[po] == 0) continue;
      mask |= 1u << s;
      if (rs < q.v) own = false;                               // a kept partner in an earlier view owns the point
    }
  }
  if (q.in) { agree_mask[q.o] = (uint8_t)mask; owner[q.o] = own ? 1 : 0; }
  const int owners = block_flag_count<DEPTH_PIXEL_BLOCK>(own, s_wave);
  if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)owners;
}

__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_fuse_scan_chunks(uint32_t* __restrict__ blk, int64_t n_blocks, int64_t* __restrict__ chunk_sum) {
  __shared__ int64_t s_wave[FUSE_WAVES];
  const int64_t total = scan_chunk_counts(blk, n_blocks, s_wave);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_fuse_scan_top(int64_t* __restrict__ chunk_sum, int64_t n_chunks, const uint32_t* __restrict__ blk,
                                                                       int64_t n_blocks, const DepthView* __restrict__ views, int n_ref,
                                                                       int64_t* __restrict__ pt_ptr) {
  __shared__ int64_t s_wave[FUSE_WAVES];
  const int64_t all = scan_chunk_totals(chunk_sum, n_chunks, 1, s_wave);
  __syncthreads();                                             // the bases of this workgroup's own stores, read below
  for (int v = threadIdx.x; v <= n_ref; v += DEPTH_THREADS) {
    const int64_t b = views[v].pix_block_first;
    pt_ptr[v] = b < n_blocks ? depth_scan_base(chunk_sum, blk, b) : all;
  }
}

__global__ __launch_bounds__(DEPTH_PIXEL_BLOCK) void k_depth_fuse_gather(const DepthImage* __restrict__ images, const DepthView* __restrict__ views,
                                                                         int n_ref, const int32_t* __restrict__ src_image,
                                                                         const int32_t* __restrict__ ref_of_image, const double* __restrict__ warps,
                                                                         const float* __restrict__ depth_in, const double* __restrict__ xyz,
                                                                         const float* __restrict__ normal_map, const uint8_t* __restrict__ agree_mask,
                                                                         const uint8_t* __restrict__ owner, const uint32_t* __restrict__ blk,
                                                                         const int64_t* __restrict__ chunk_base, const int64_t* __restrict__ pt_ptr,
                                                                         int64_t n_points, double* __restrict__ points, float* __restrict__ normals,
                                                                         uint8_t* __restrict__ n_views_out, int32_t* __restrict__ index) {
  __shared__ int s_wave[FUSE_WAVES];
  DepthView view; DepthImage ref;
  const FusePixel q = fuse_pixel(images, views, n_ref, &view, &ref);
  const bool own = q.in && owner[q.o] != 0;
  const int rank = block_flag_rank<DEPTH_PIXEL_BLOCK>(own, s_wave);
  if (!own) return;
  const int64_t slot = depth_scan_base(chunk_base, blk, blockIdx.x) + rank;
  // a workspace or a pt_ptr that is not the mark call's, or an n_points below the truth, writes nothing outside the outputs
  if (slot < pt_ptr[q.v] || slot >= pt_ptr[q.v + 1] || slot >= n_points) return;
  const unsigned mask = agree_mask[q.o];
  const double d = (double)depth_in[q.o];
  double acc[3], nacc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { acc[i] = xyz[q.o * 3 + i]; nacc[i] = (double)normal_map[q.o * 3 + i]; }
  int n_views = 1;
  for (int s = 0; s < view.n_src; ++s) {
    if (!((mask >> s) & 1u)) continue;
    int rs; double q2;
    const int64_t po = fuse_partner(images, views, src_image, ref_of_image, warps, view.src_first + s, (double)q.x, (double)q.y, d, &rs, &q2);
    if (po < 0) continue;                                      // not with the agree_mask of the mark call
#pragma unroll
    for (int i = 0; i < 3; ++i) { acc[i] = acc[i] + xyz[po * 3 + i]; nacc[i] = nacc[i] + (double)normal_map[po * 3 + i]; }
    ++n_views;
  }
  float n[3];
  depth::fused_normal(nacc, n);
#pragma unroll
  for (int i = 0; i < 3; ++i) { points[slot * 3 + i] = depth::fused_mean(acc[i], n_views); normals[slot * 3 + i] = n[i]; }
  n_views_out[slot] = (uint8_t)n_views;
  index[slot * 3 + 0] = q.v; index[slot * 3 + 1] = q.y; index[slot * 3 + 2] = q.x;
}

// the checks the two calls share; on success the plan of the call and its layout
int fuse_prepare(sfm_ctx* h, const char* what, const int64_t* img_off, const int32_t* heights, const int32_t* widths, int32_t n_img,
                 int32_t n_ref, const int32_t* ref_image, const int64_t* src_ptr, const int32_t* src_image, double rel_tol,
                 int32_t normal_step, double normal_jump, const void* workspace, int64_t workspace_bytes, DepthPlan* p, DepthFuseLayout* L) {
  int bad = depth_check_images(n_img, img_off, heights, widths);
  std::vector<int64_t> one((size_t)(n_ref > 0 ? n_ref : 0) + 1);      // as in the filter: one plane per view stands in
  for (size_t r = 0; r < one.size(); ++r) one[r] = (int64_t)r;
  if (!bad) bad = depth_check_views(n_img, n_ref, ref_image, src_ptr, src_image, one.data(), 0);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, DEPTH_WHY[bad]);
  bad = depth_check_fuse(rel_tol, normal_step, normal_jump);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, DEPTH_FUSE_WHY[bad]);
  *p = depth_plan(n_img, img_off, heights, widths, n_ref, ref_image, src_ptr, one.data());
  *L = depth_fuse_layout(n_img, n_ref, src_ptr[n_ref], p->n_pix_blocks);
  if (!workspace || workspace_bytes < L->bytes) return sfm_fail(h, SFM_ERR_ARG, what, "workspace missing or too small");
  if (p->n_pix_blocks > 0x7FFFFFFFLL) return sfm_fail(h, SFM_ERR_ARG, what, "too many pixels for one call");
  return SFM_OK;
}

// the tables of a call -> the workspace; the host vectors are pageable, so the copies must have left them on return
int fuse_upload(sfm_ctx* h, const DepthPlan& p, const DepthLayout& T, char* ws, const int32_t* src_image, int64_t n_entries) {
  SFM_HIP(h, hipMemcpyAsync(ws + T.images, p.images.data(), p.images.size() * sizeof(DepthImage), hipMemcpyHostToDevice, h->stream));
  SFM_HIP(h, hipMemcpyAsync(ws + T.views, p.views.data(), p.views.size() * sizeof(DepthView), hipMemcpyHostToDevice, h->stream));
  if (n_entries > 0) SFM_HIP(h, hipMemcpyAsync(ws + T.src_image, src_image, (size_t)n_entries * 4, hipMemcpyHostToDevice, h->stream));
  SFM_HIP(h, hipMemcpyAsync(ws + T.ref_of_image, p.ref_of_image.data(), p.ref_of_image.size() * 4, hipMemcpyHostToDevice, h->stream));
  SFM_HIP(h, hipStreamSynchronize(h->stream));
  return SFM_OK;
}

}  // namespace

extern "C" int sfm_depth_fuse_workspace_bytes(int32_t n_img, int32_t n_ref, int64_t n_entries, int64_t n_out, int64_t* bytes_host) {
  if (!bytes_host || n_img < 0 || n_ref < 0 || n_ref > n_img || n_entries < 0 || n_entries > (int64_t)n_ref * DEPTH_MAX_SOURCES || n_out < 0)
    return SFM_ERR_ARG;
  *bytes_host = depth_fuse_layout(n_img, n_ref, n_entries, depth_max_pixel_blocks(n_out, n_ref)).bytes;
  return SFM_OK;
}

extern "C" int sfm_depth_fuse_mark(sfm_handle h, const int64_t* img_off, const int32_t* heights, const int32_t* widths, int32_t n_img,
                                   int32_t n_ref, const int32_t* ref_image, const int64_t* src_ptr, const int32_t* src_image,
                                   const double* warps, const double* backproj, const float* depth, const uint8_t* keep, const double* xyz,
                                   double rel_tol, int32_t normal_step, double normal_jump, float* normal_map, uint8_t* agree_mask,
                                   uint8_t* owner, int64_t* pt_ptr, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  DepthPlan p; DepthFuseLayout L;
  const int rc = fuse_prepare(h, "sfm_depth_fuse_mark", img_off, heights, widths, n_img, n_ref, ref_image, src_ptr, src_image, rel_tol,
                              normal_step, normal_jump, workspace, workspace_bytes, &p, &L);
  if (rc) return rc;
  if (!pt_ptr) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_fuse_mark", "null pointer");
  const int64_t n_entries = src_ptr[n_ref], nb = p.n_pix_blocks;
  if (nb == 0) {                                               // no pixel: no owner
    SFM_HIP(h, hipMemsetAsync(pt_ptr, 0, ((size_t)n_ref + 1) * 8, h->stream));
    return SFM_OK;
  }
  if (!backproj || !depth || !keep || !xyz || !normal_map || !agree_mask || !owner || (n_entries > 0 && !warps))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_fuse_mark", "null pointer");
  char* ws = (char*)workspace;
  const DepthLayout& T = L.tables;
  const int up = fuse_upload(h, p, T, ws, src_image, n_entries); if (up) return up;
  const DepthImage* d_img = (const DepthImage*)(ws + T.images);
  const DepthView* d_view = (const DepthView*)(ws + T.views);
  uint32_t* d_blk = (uint32_t*)(ws + L.blk);
  int64_t* d_chunk = (int64_t*)(ws + L.chunk_base);
  const int64_t n_chunks = scan_chunks(nb);
  hipLaunchKernelGGL(k_depth_normals, dim3((unsigned)nb), dim3(DEPTH_PIXEL_BLOCK), 0, h->stream, d_img, d_view, n_ref, backproj, depth, xyz,
                     normal_step, normal_jump, normal_map);
  SFM_LAUNCH_CHECK(h, "sfm_depth_fuse_mark");
  hipLaunchKernelGGL(k_depth_fuse_mark, dim3((unsigned)nb), dim3(DEPTH_PIXEL_BLOCK), 0, h->stream, d_img, d_view, n_ref,
                     (const int32_t*)(ws + T.src_image), (const int32_t*)(ws + T.ref_of_image), warps, depth, keep, rel_tol, agree_mask,
                     owner, d_blk);
  SFM_LAUNCH_CHECK(h, "sfm_depth_fuse_mark");
  hipLaunchKernelGGL(k_depth_fuse_scan_chunks, dim3((unsigned)n_chunks), dim3(DEPTH_THREADS), 0, h->stream, d_blk, nb, d_chunk);
  SFM_LAUNCH_CHECK(h, "sfm_depth_fuse_mark");
  hipLaunchKernelGGL(k_depth_fuse_scan_top, dim3(1), dim3(DEPTH_THREADS), 0, h->stream, d_chunk, n_chunks, (const uint32_t*)d_blk, nb, d_view,
                     n_ref, pt_ptr);
  SFM_LAUNCH_CHECK(h, "sfm_depth_fuse_mark");
  return SFM_OK;
}

extern "C" int sfm_depth_fuse_gather(sfm_handle h, const int64_t* img_off, const int32_t* heights, const int32_t* widths, int32_t n_img,
                                     int32_t n_ref, const int32_t* ref_image, const int64_t* src_ptr, const int32_t* src_image,
                                     const double* warps, const float* depth, const double* xyz, const float* normal_map,
                                     const uint8_t* agree_mask, const uint8_t* owner, const int64_t* pt_ptr, int64_t n_points, double* points,
                                     float* normals, uint8_t* n_views, int32_t* index, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  DepthPlan p; DepthFuseLayout L;
  const int rc = fuse_prepare(h, "sfm_depth_fuse_gather", img_off, heights, widths, n_img, n_ref, ref_image, src_ptr, src_image, 0.0, 1,
                              0.0, workspace, workspace_bytes, &p, &L);
  if (rc) return rc;
  if (n_points < 0 || n_points > p.n_out) return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_fuse_gather", "n_points must be 0 .. the number of pixels");
  if (n_points == 0 || p.n_pix_blocks == 0) return SFM_OK;
  const int64_t n_entries = src_ptr[n_ref];
  if (!depth || !xyz || !normal_map || !agree_mask || !owner || !pt_ptr || !points || !normals || !n_views || !index || (n_entries > 0 && !warps))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_depth_fuse_gather", "null pointer");
  char* ws = (char*)workspace;
  const DepthLayout& T = L.tables;
  const int up = fuse_upload(h, p, T, ws, src_image, n_entries); if (up) return up;      // the tables again: only the scan is carried over
  hipLaunchKernelGGL(k_depth_fuse_gather, dim3((unsigned)p.n_pix_blocks), dim3(DEPTH_PIXEL_BLOCK), 0, h->stream,
                     (const DepthImage*)(ws + T.images), (const DepthView*)(ws + T.views), n_ref, (const int32_t*)(ws + T.src_image),
                     (const int32_t*)(ws + T.ref_of_image), warps, depth, xyz, normal_map, agree_mask, owner,
                     (const uint32_t*)(ws + L.blk), (const int64_t*)(ws + L.chunk_base), pt_ptr, n_points, points, normals, n_views, index);
  SFM_LAUNCH_CHECK(h, "sfm_depth_fuse_gather");
  return SFM_OK;
}
