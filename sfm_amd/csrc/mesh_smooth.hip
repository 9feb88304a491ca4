// The vertex adjacency of a triangle mesh, Taubin / Laplacian smoothing steps over it and area-weighted vertex normals, for
// gfx950 (MI355X).  include/sfm_amd.h states the rule; mesh_smooth_rule.h holds the keys, the state of a vertex, the step and
// the normal, mesh_smooth_plan.h the argument checks, the workspace layouts and the grids; the scans are those of
// block_scan.h / scan_plan.h.  Every output byte is a function of the inputs: the sums walk their members in one stated
// order, one lane per vertex.
//
// sfm_mesh_adjacency
//   k_adj_keys        one lane per half-edge: the two entries (a, b) and (b, a) of a live one, all ones otherwise
//   rocprim           one keys-only radix sort over the bits n_vertices needs, the only part that is not hand-written
//   k_adj_heads       one lane per sorted slot: the heads of the runs of equal keys per block
//   k_adj_scan_*      the two-level scan of the heads -> counts[0]
//   k_adj_scatter     a head at its rank: the neighbour -> index, its key and the length of its run behind it
//   k_adj_vertices    one lane per vertex: ptr from the compacted keys, the flags from the run lengths
// sfm_mesh_smooth
//   k_smo_state       one lane per vertex: its state byte, the counts, the soundness of ptr
//   k_smo_step        THE HOT PATH, one launch per step: one lane per vertex gathers its neighbours' float64 rows
// sfm_mesh_vertex_normals
//   k_nrm_keys        one lane per corner: (vertex, corner), all ones for a corner of an unsound triangle
//   rocprim           one stable radix sort of the pairs over the bits n_vertices needs
//   k_nrm_vertices    one lane per vertex: the face normals of its corners in ascending corner, the unit of their sum
// Nothing waits on another workgroup; the only atomics are integer adds and a status flag in the counts.  A vertex of degree
// d costs its lane d dependent additions: a fan about one vertex is sequential.
#include "common.h"
#include "mesh_smooth_rule.h"
#include "mesh_smooth_plan.h"
#include "block_scan.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

__device__ __forceinline__ void add64(int64_t* p, int64_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// *p += the set flags of the wavefront, in one add; every lane of the wavefront must call
__device__ __forceinline__ void wave_count(int64_t* p, bool flag) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && m) add64(p, __popcll(m));
}

__device__ __forceinline__ void load_triangle(const int32_t* __restrict__ triangles, int64_t t, int32_t* v) {
  v[0] = triangles[3 * t]; v[1] = triangles[3 * t + 1]; v[2] = triangles[3 * t + 2];
}

// ------------------------------------------------------------------------------------------------ adjacency
__global__ __launch_bounds__(SMO_BLOCK) void k_adj_keys(const int32_t* __restrict__ triangles, int64_t n_halfedges, int64_t n_vertices,
                                                        uint64_t* __restrict__ keys, int64_t* __restrict__ counts) {
  const int64_t h = (int64_t)blockIdx.x * SMO_BLOCK + threadIdx.x;
  bool unsound = false;
  if (h < n_halfedges) {
    const int64_t t = h / 3;
    const int k = (int)(h - 3 * t);
    int32_t v[3], a, b;
    load_triangle(triangles, t, v);
    const int live = mesh_smooth::halfedge(v, k, n_vertices, &a, &b);
    keys[2 * h] = live ? mesh_smooth::edge_key(a, b) : MESH_ADJ_DEAD_KEY;
    keys[2 * h + 1] = live ? mesh_smooth::edge_key(b, a) : MESH_ADJ_DEAD_KEY;
    unsound = k == 0 && !mesh_clean::sound(v[0], v[1], v[2], n_vertices);
  }
  wave_count(&counts[ADJ_UNSOUND], unsound);
}

__device__ __forceinline__ bool is_head(const uint64_t* __restrict__ keys, int64_t s, int64_t n) {
  if (s >= n) return false;
  const uint64_t key = keys[s];
  return key != MESH_ADJ_DEAD_KEY && (s == 0 || keys[s - 1] != key);
}

__global__ __launch_bounds__(SMO_BLOCK) void k_adj_heads(const uint64_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ blk) {
  __shared__ int s_wave[SMO_WAVES];
  const int64_t s = (int64_t)blockIdx.x * SMO_BLOCK + threadIdx.x;
  const int all = block_flag_count<SMO_BLOCK>(is_head(keys, s, n), s_wave);
  if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)all;
}

__global__ __launch_bounds__(SMO_BLOCK) void k_adj_scan_chunks(uint32_t* __restrict__ blk, int64_t n_blocks, int64_t* __restrict__ chunk_sum) {
  __shared__ int64_t s_wave[SMO_WAVES];
  const int64_t total = scan_chunk_counts(blk, n_blocks, s_wave);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(SMO_BLOCK) void k_adj_scan_top(int64_t* __restrict__ chunk_sum, int64_t n_chunks, int64_t* __restrict__ count) {
  __shared__ int64_t s_wave[SMO_WAVES];
  const int64_t all = scan_chunk_totals(chunk_sum, n_chunks, 1, s_wave);
  if (threadIdx.x == 0) *count = all;
}

// A run of r equal keys costs its head r steps; r is the uses of the edge, 2 inside a manifold surface.
__global__ __launch_bounds__(SMO_BLOCK) void k_adj_scatter(const uint64_t* __restrict__ keys, int64_t n, const uint32_t* __restrict__ blk,
                                                           const int64_t* __restrict__ chunk_base, int32_t* __restrict__ index,
                                                           uint64_t* __restrict__ entry_key, int32_t* __restrict__ entry_uses) {
  __shared__ int s_wave[SMO_WAVES];
  const int64_t s = (int64_t)blockIdx.x * SMO_BLOCK + threadIdx.x;
  const bool head = is_head(keys, s, n);
  const int rank = block_flag_rank<SMO_BLOCK>(head, s_wave);
  if (!head) return;
  const int64_t e = scan_base(chunk_base, 1, 0, blockIdx.x, (int64_t)blk[blockIdx.x]) + rank;
  if (e < 0 || e >= n) return;                                     // never so: there are no more heads than slots
  const uint64_t key = keys[s];
  int64_t r = 1;
  for (int64_t j = s + 1; j < n && keys[j] == key; ++j) ++r;
  index[e] = mesh_smooth::key_neighbour(key);
  entry_key[e] = key;
  entry_uses[e] = (int32_t)r;
}

// the first of the n sorted entries whose key is >= key
__device__ __forceinline__ int64_t entry_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// lanes 0 .. n_vertices: ptr; lanes below n_vertices the flags too
__global__ __launch_bounds__(SMO_BLOCK) void k_adj_vertices(int64_t n_vertices, int64_t capacity, const uint64_t* __restrict__ entry_key,
                                                            const int32_t* __restrict__ entry_uses, int32_t* __restrict__ ptr,
                                                            uint8_t* __restrict__ vertex_flags, int64_t* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * SMO_BLOCK + threadIdx.x;
  bool boundary = false, isolated = false;
  if (v <= n_vertices) {
    int64_t n = counts[ADJ_ENTRIES];
    n = n < 0 ? 0 : (n > capacity ? capacity : n);
    const int64_t lo = entry_bound(entry_key, n, (uint64_t)v << 32);
    ptr[v] = (int32_t)lo;
    if (v < n_vertices) {
      const int64_t hi = entry_bound(entry_key, n, (uint64_t)(v + 1) << 32);
      bool odd = false;
      for (int64_t e = lo; e < hi; ++e) odd = odd || entry_uses[e] != 2;
      const uint8_t f = mesh_smooth::vertex_flags(hi - lo, odd);
      vertex_flags[v] = f;
      boundary = (f & MESH_ADJ_BOUNDARY) != 0;
      isolated = (f & MESH_ADJ_ISOLATED) != 0;
    }
  }
  wave_count(&counts[ADJ_BOUNDARY], boundary);
  wave_count(&counts[ADJ_ISOLATED], isolated);
}

// ------------------------------------------------------------------------------------------------ smoothing
// the entries [*lo, *hi) of vertex v when ptr is sound there: 0 <= lo <= hi <= n_index
__device__ __forceinline__ bool entries_of(const int32_t* __restrict__ ptr, int64_t v, int64_t n_index, int64_t* lo, int64_t* hi) {
  *lo = ptr[v];
  *hi = ptr[v + 1];
  return *lo >= 0 && *lo <= *hi && *hi <= n_index;
}

__global__ __launch_bounds__(SMO_BLOCK) void k_smo_state(int64_t n_vertices, int64_t n_index, const double* __restrict__ vertices,
                                                         const int32_t* __restrict__ ptr, const uint8_t* __restrict__ vertex_flags,
                                                         const uint8_t* __restrict__ pinned, int pin_boundary, uint8_t* __restrict__ state,
                                                         int64_t* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * SMO_BLOCK + threadIdx.x;
  uint8_t st = 0;
  bool foreign = false;
  if (v < n_vertices) {
    const double x[3] = {vertices[3 * v], vertices[3 * v + 1], vertices[3 * v + 2]};
    st = mesh_smooth::vertex_state(vertex_flags[v], pinned && pinned[v] != 0, pin_boundary != 0, x);
    state[v] = st;
    int64_t lo, hi;
    foreign = !entries_of(ptr, v, n_index, &lo, &hi);
  }
  wave_count(&counts[SMO_PINNED_BOUNDARY], (st & MESH_SMOOTH_PIN_BOUNDARY) != 0);
  wave_count(&counts[SMO_PINNED_GIVEN], (st & MESH_SMOOTH_PIN_GIVEN) != 0);
  wave_count(&counts[SMO_UNSOUND], (st & MESH_SMOOTH_UNSOUND) != 0);
  wave_count(&counts[SMO_ISOLATED], (st & MESH_SMOOTH_ISOLATED) != 0);
  if (foreign) counts[SMO_STATUS] = 1;
}

// One Jacobi step with factor f: src -> dst, every row written.  The neighbours are taken four at a time - their indices,
// then their states and rows, then the additions in ascending order - so that the loads of a group are in flight together;
// the order of the additions is that of the rule.  No index is an address before it is checked.
#define SMO_GROUP 4
__global__ __launch_bounds__(SMO_BLOCK) void k_smo_step(int64_t n_vertices, int64_t n_index, const double* __restrict__ src,
                                                        const int32_t* __restrict__ ptr, const int32_t* __restrict__ index,
                                                        const uint8_t* __restrict__ state, double f, double* __restrict__ dst,
                                                        int64_t* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * SMO_BLOCK + threadIdx.x;
  if (v >= n_vertices) return;
  const double x[3] = {src[3 * v], src[3 * v + 1], src[3 * v + 2]};
  double out[3] = {x[0], x[1], x[2]};
  bool foreign = false;
  if (state[v] == 0) {
    int64_t lo, hi;
    if (entries_of(ptr, v, n_index, &lo, &hi)) {
      double s[3] = {0.0, 0.0, 0.0};
      int64_t n = 0;
      for (int64_t e = lo; e < hi; e += SMO_GROUP) {
        int32_t j[SMO_GROUP];
        bool use[SMO_GROUP];
        double xj[SMO_GROUP][3];
#pragma unroll
        for (int u = 0; u < SMO_GROUP; ++u) j[u] = e + u < hi ? index[e + u] : -1;
#pragma unroll
        for (int u = 0; u < SMO_GROUP; ++u) {
          const bool inside = j[u] >= 0 && (int64_t)j[u] < n_vertices;
          if (e + u < hi && !inside) foreign = true;
          use[u] = inside && (state[j[u]] & MESH_SMOOTH_UNSOUND) == 0;
        }
#pragma unroll
        for (int u = 0; u < SMO_GROUP; ++u) {
          const int64_t row = use[u] ? (int64_t)j[u] : v;          // a row that exists; it is not added
          xj[u][0] = src[3 * row]; xj[u][1] = src[3 * row + 1]; xj[u][2] = src[3 * row + 2];
        }
#pragma unroll
        for (int u = 0; u < SMO_GROUP; ++u)
          if (use[u]) { mesh_smooth::add_neighbour(xj[u], s); ++n; }
      }
      if (n > 0) mesh_smooth::move(x, s, n, f, out);
    } else {
      foreign = true;
    }
  }
  dst[3 * v] = out[0]; dst[3 * v + 1] = out[1]; dst[3 * v + 2] = out[2];
  if (foreign) counts[SMO_STATUS] = 1;
}

// ------------------------------------------------------------------------------------------------ normals
__global__ __launch_bounds__(SMO_BLOCK) void k_nrm_keys(const int32_t* __restrict__ triangles, int64_t n_corners, int64_t n_vertices,
                                                        uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int64_t h = (int64_t)blockIdx.x * SMO_BLOCK + threadIdx.x;
  if (h >= n_corners) return;
  const int64_t t = h / 3;
  const int k = (int)(h - 3 * t);
  int32_t v[3];
  load_triangle(triangles, t, v);
  keys[h] = mesh_clean::sound(v[0], v[1], v[2], n_vertices) ? (uint32_t)(k == 0 ? v[0] : (k == 1 ? v[1] : v[2])) : MESH_ADJ_DEAD_CORNER;
  vals[h] = (int32_t)h;
}

// the first slot of the sorted corner keys that holds a key >= c
__device__ __forceinline__ int64_t corner_bound(const uint32_t* __restrict__ keys, int64_t n, uint32_t c) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(SMO_BLOCK) void k_nrm_vertices(int64_t n_vertices, int64_t n_corners, const double* __restrict__ vertices,
                                                            const int32_t* __restrict__ triangles, const uint32_t* __restrict__ corner_key,
                                                            const int32_t* __restrict__ corner_val, float* __restrict__ normals) {
  const int64_t v = (int64_t)blockIdx.x * SMO_BLOCK + threadIdx.x;
  if (v >= n_vertices) return;
  double ns[3] = {0.0, 0.0, 0.0};
  const int64_t cb = corner_bound(corner_key, n_corners, (uint32_t)v), ce = corner_bound(corner_key, n_corners, (uint32_t)v + 1u);
  for (int64_t i = cb; i < ce; ++i) {
    const int64_t h = corner_val[i];
    if (h < 0 || h >= n_corners) continue;                        // never so with the pairs of k_nrm_keys
    int32_t w[3];
    load_triangle(triangles, h / 3, w);
    if (!mesh_clean::sound(w[0], w[1], w[2], n_vertices)) continue;
    double n[3];
    mesh_smooth::face_normal(vertices + 3 * (int64_t)w[0], vertices + 3 * (int64_t)w[1], vertices + 3 * (int64_t)w[2], n);
    mesh_smooth::add_face(n, ns);
  }
  float out[3];
  mesh_smooth::unit_normal(ns, out);
  normals[3 * v] = out[0]; normals[3 * v + 1] = out[1]; normals[3 * v + 2] = out[2];
}

// ------------------------------------------------------------------------------------------------ host
hipError_t adj_sort_room(int64_t n_vertices, int64_t n_triangles, hipStream_t stream, size_t* room) {
  *room = 0;
  if (n_triangles == 0) return hipSuccess;
  return rocprim::radix_sort_keys(nullptr, *room, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)(6 * n_triangles), 0u,
                                  (unsigned)smo_key_bits(n_vertices), stream);
}

hipError_t nrm_sort_room(int64_t n_vertices, int64_t n_triangles, hipStream_t stream, size_t* room) {
  *room = 0;
  if (n_triangles == 0) return hipSuccess;
  return rocprim::radix_sort_pairs(nullptr, *room, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)(3 * n_triangles),
                                   0u, (unsigned)smo_vertex_bits(n_vertices), stream);
}

}  // namespace

extern "C" int sfm_mesh_adjacency_workspace_bytes(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t* bytes_host) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_adjacency_workspace_bytes";
  if (!bytes_host) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[2]);
  if (smo_check_counts(n_vertices, n_triangles)) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[1]);
  size_t room = 0;
  SFM_HIP(h, adj_sort_room(n_vertices, n_triangles, h->stream, &room));
  *bytes_host = adj_layout(n_triangles, (int64_t)room).bytes;
  return SFM_OK;
}

extern "C" int sfm_mesh_adjacency(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const int32_t* triangles, int32_t* ptr, int32_t* index,
                                  uint8_t* vertex_flags, int64_t* counts, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_adjacency";
  int bad = smo_check_adjacency(n_vertices, n_triangles, triangles, ptr, index, vertex_flags, counts);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[bad]);
  size_t room = 0;
  SFM_HIP(h, adj_sort_room(n_vertices, n_triangles, h->stream, &room));
  const AdjLayout L = adj_layout(n_triangles, (int64_t)room);
  bad = smo_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[bad]);
  SFM_HIP(h, hipMemsetAsync(counts, 0, ADJ_COUNTS * sizeof(int64_t), h->stream));
  char* ws = (char*)workspace;
  uint64_t* d_keys_in = (uint64_t*)(ws + L.key_in);
  uint64_t* d_keys = (uint64_t*)(ws + L.key_out);
  int32_t* d_uses = (int32_t*)(ws + L.uses);
  uint32_t* d_blk = (uint32_t*)(ws + L.blk);
  int64_t* d_chunk = (int64_t*)(ws + L.chunk);
  const int64_t n = 6 * n_triangles;
  const dim3 tb(SMO_BLOCK);
  if (n > 0) {
    const int64_t nb = smo_blocks(n), n_chunks = scan_chunks(nb);
    hipLaunchKernelGGL(k_adj_keys, dim3((unsigned)smo_blocks(3 * n_triangles)), tb, 0, h->stream, triangles, 3 * n_triangles, n_vertices, d_keys_in, counts);
    SFM_LAUNCH_CHECK(h, what);
    size_t sort_bytes = room;
    SFM_HIP(h, rocprim::radix_sort_keys(ws + L.sort, sort_bytes, d_keys_in, d_keys, (size_t)n, 0u, (unsigned)smo_key_bits(n_vertices), h->stream));
    hipLaunchKernelGGL(k_adj_heads, dim3((unsigned)nb), tb, 0, h->stream, (const uint64_t*)d_keys, n, d_blk);
    SFM_LAUNCH_CHECK(h, what);
    hipLaunchKernelGGL(k_adj_scan_chunks, dim3((unsigned)n_chunks), tb, 0, h->stream, d_blk, nb, d_chunk);
    SFM_LAUNCH_CHECK(h, what);
    hipLaunchKernelGGL(k_adj_scan_top, dim3(1), tb, 0, h->stream, d_chunk, n_chunks, counts + ADJ_ENTRIES);
    SFM_LAUNCH_CHECK(h, what);
    // the compacted keys take the place of the sort's input
    hipLaunchKernelGGL(k_adj_scatter, dim3((unsigned)nb), tb, 0, h->stream, (const uint64_t*)d_keys, n, (const uint32_t*)d_blk, (const int64_t*)d_chunk,
                       index, d_keys_in, d_uses);
    SFM_LAUNCH_CHECK(h, what);
  }
  hipLaunchKernelGGL(k_adj_vertices, dim3((unsigned)smo_blocks(n_vertices + 1)), tb, 0, h->stream, n_vertices, n, (const uint64_t*)d_keys_in,
                     (const int32_t*)d_uses, ptr, vertex_flags, counts);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}

extern "C" int sfm_mesh_smooth_workspace_bytes(sfm_handle h, int64_t n_vertices, int64_t* bytes_host) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_smooth_workspace_bytes";
  if (!bytes_host) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[2]);
  if (smo_check_counts(n_vertices, 0)) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[1]);
  *bytes_host = smo_layout_bytes(n_vertices);
  return SFM_OK;
}

extern "C" int sfm_mesh_smooth(sfm_handle h, int64_t n_vertices, const double* vertices_in, const int32_t* ptr, const int32_t* index, int64_t n_index,
                               const uint8_t* vertex_flags, const uint8_t* pinned, int pin_boundary, double lam, double mu, int has_mu,
                               int64_t iterations, double* vertices_out, uint8_t* vertex_state, int64_t* counts, void* workspace,
                               int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_smooth";
  int bad = smo_check_smooth(n_vertices, n_index, iterations, lam, mu, has_mu, vertices_in, ptr, index, vertex_flags, vertices_out, vertex_state, counts);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[bad]);
  bad = smo_check_workspace(workspace, workspace_bytes, smo_layout_bytes(n_vertices));
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[bad]);
  SFM_HIP(h, hipMemsetAsync(counts, 0, SMO_COUNTS * sizeof(int64_t), h->stream));
  if (n_vertices == 0) return SFM_OK;
  const dim3 tb(SMO_BLOCK), grid((unsigned)smo_blocks(n_vertices));
  hipLaunchKernelGGL(k_smo_state, grid, tb, 0, h->stream, n_vertices, n_index, vertices_in, ptr, vertex_flags, pinned, pin_boundary, vertex_state, counts);
  SFM_LAUNCH_CHECK(h, what);
  const int64_t n_steps = smo_steps(iterations, has_mu);
  if (n_steps == 0) {
    SFM_HIP(h, hipMemcpyAsync(vertices_out, vertices_in, (size_t)n_vertices * 3 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return SFM_OK;
  }
  double* second = (double*)workspace;
  const double* src = vertices_in;
  for (int64_t i = 0; i < n_steps; ++i) {
    double* dst = smo_step_writes_out(n_steps, i) ? vertices_out : second;
    hipLaunchKernelGGL(k_smo_step, grid, tb, 0, h->stream, n_vertices, n_index, src, ptr, index, (const uint8_t*)vertex_state,
                       smo_step_factor(i, lam, mu, has_mu), dst, counts);
    SFM_LAUNCH_CHECK(h, what);
    src = dst;
  }
  return SFM_OK;
}

extern "C" int sfm_mesh_vertex_normals_workspace_bytes(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t* bytes_host) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_vertex_normals_workspace_bytes";
  if (!bytes_host) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[2]);
  if (smo_check_counts(n_vertices, n_triangles)) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[1]);
  size_t room = 0;
  SFM_HIP(h, nrm_sort_room(n_vertices, n_triangles, h->stream, &room));
  *bytes_host = nrm_layout(n_triangles, (int64_t)room).bytes;
  return SFM_OK;
}

extern "C" int sfm_mesh_vertex_normals(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const double* vertices, const int32_t* triangles,
                                       float* normals, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_vertex_normals";
  int bad = smo_check_normals(n_vertices, n_triangles, vertices, triangles, normals);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[bad]);
  size_t room = 0;
  SFM_HIP(h, nrm_sort_room(n_vertices, n_triangles, h->stream, &room));
  const NrmLayout L = nrm_layout(n_triangles, (int64_t)room);
  bad = smo_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, SMO_WHY[bad]);
  if (n_vertices == 0) return SFM_OK;
  char* ws = (char*)workspace;
  uint32_t* d_key_in = (uint32_t*)(ws + L.key_in);
  uint32_t* d_key = (uint32_t*)(ws + L.key_out);
  int32_t* d_val_in = (int32_t*)(ws + L.val_in);
  int32_t* d_val = (int32_t*)(ws + L.val_out);
  const int64_t n = 3 * n_triangles;
  const dim3 tb(SMO_BLOCK);
  if (n > 0) {
    hipLaunchKernelGGL(k_nrm_keys, dim3((unsigned)smo_blocks(n)), tb, 0, h->stream, triangles, n, n_vertices, d_key_in, d_val_in);
    SFM_LAUNCH_CHECK(h, what);
    size_t sort_bytes = room;
    SFM_HIP(h, rocprim::radix_sort_pairs(ws + L.sort, sort_bytes, d_key_in, d_key, d_val_in, d_val, (size_t)n, 0u, (unsigned)smo_vertex_bits(n_vertices),
                                         h->stream));
  }
  hipLaunchKernelGGL(k_nrm_vertices, dim3((unsigned)smo_blocks(n_vertices)), tb, 0, h->stream, n_vertices, n, vertices, triangles, (const uint32_t*)d_key,
                     (const int32_t*)d_val, normals);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}
