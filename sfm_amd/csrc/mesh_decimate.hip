// Decimation of a triangle mesh by vertex clustering on a uniform grid, with a quadric-optimal vertex per cell, for gfx950
// (MI355X).  include/sfm_amd.h states the rule; mesh_decimate_rule.h holds the cell of a vertex, the placement and the
// duplicate rule, mesh_decimate_plan.h the argument checks, the workspace layout and the grids; the scans are those of
// block_scan.h / scan_plan.h.  Every output byte is a function of the inputs: the sums walk their members in one stated
// order, one lane per cluster.
//
// sfm_mesh_decimate_cluster
//   k_dec_vertex_keys    one lane per vertex: the key of its cell (all ones when it has none), the unsound vertices
//   rocprim              one stable radix sort of (key, vertex) over 64 bits, the only part that is not hand-written
//   k_dec_heads          one lane per sorted slot: the heads of the runs of equal keys per block
//   k_dec_scan_*         the two-level scan of the heads -> counts[0]
//   k_dec_number         the cluster of every slot from the heads in front of it -> vertex_cluster, cluster_start, cluster_first
//   k_dec_sizes          one lane per cluster: cluster_size from cluster_start
// sfm_mesh_decimate_mark
//   k_dec_corner_keys    one lane per corner: the cluster of the corner (all ones for an unsound triangle); lane k = 0 also the
//                        key of the triangle's sorted cluster triple (all ones when unsound or degenerate)
//   rocprim              (cluster, corner) over the bits n_clusters needs; (triple, triangle) in one pass over three such fields,
//                        or by the largest cluster first and the other two (k_dec_pair_keys) second when they pass 63 bits
//   k_dec_duplicates     one lane per sorted slot: the head of a run of equal triples counts its even and odd members and keeps
//                        the first of the majority, none on a tie -> triangle_keep
//   k_dec_keep_count     kept triangles per block; k_dec_scan_* their scan -> counts[0]
// sfm_mesh_decimate_emit
//   k_dec_place          one lane per cluster: the mean and the normal over its members, the quadric over its corners, the solve
//                        and the box test
//   k_dec_emit_triangles one lane per triangle: a kept one at its rank, with the clusters of its vertices
// Nothing waits on another workgroup; the only atomics are integer adds and a status flag in the counts.
#include "common.h"
#include "mesh_decimate_rule.h"
#include "mesh_decimate_plan.h"
#include "block_scan.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

struct Grid3 { double origin[3]; double cell; };

__device__ __forceinline__ void add64(int64_t* p, int64_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// *p += the set flags of the wavefront, in one add; every lane of the wavefront must call
__device__ __forceinline__ void wave_count(int64_t* p, bool flag) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && m) add64(p, __popcll(m));
}

// ------------------------------------------------------------------------------------------------ clusters
__global__ __launch_bounds__(DEC_BLOCK) void k_dec_vertex_keys(const double* __restrict__ vertices, int64_t n, Grid3 g, uint64_t* __restrict__ keys,
                                                               int32_t* __restrict__ vals, int64_t* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  bool unsound = false;
  if (v < n) {
    const double p[3] = {vertices[3 * v], vertices[3 * v + 1], vertices[3 * v + 2]};
    int64_t idx[3];
    const uint64_t key = mesh_decimate::vertex_key(p, g.origin, g.cell, idx);
    keys[v] = key;
    vals[v] = (int32_t)v;
    unsound = key == MESH_DEC_DEAD_KEY;
  }
  wave_count(&counts[DEC_UNSOUND_VERTICES], unsound);
}

__device__ __forceinline__ bool is_head(const uint64_t* __restrict__ keys, int64_t s, int64_t n) {
  if (s >= n) return false;
  const uint64_t key = keys[s];
  return key != MESH_DEC_DEAD_KEY && (s == 0 || keys[s - 1] != key);
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_heads(const uint64_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ blk) {
  __shared__ int s_wave[DEC_WAVES];
  const int64_t s = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  const int all = block_flag_count<DEC_BLOCK>(is_head(keys, s, n), s_wave);
  if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)all;
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_scan_chunks(uint32_t* __restrict__ blk, int64_t n_blocks, int64_t* __restrict__ chunk_sum) {
  __shared__ int64_t s_wave[DEC_WAVES];
  const int64_t total = scan_chunk_counts(blk, n_blocks, s_wave);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_scan_top(int64_t* __restrict__ chunk_sum, int64_t n_chunks, int64_t* __restrict__ count) {
  __shared__ int64_t s_wave[DEC_WAVES];
  const int64_t all = scan_chunk_totals(chunk_sum, n_chunks, 1, s_wave);
  if (threadIdx.x == 0) *count = all;
}

// The cluster of a live slot is the number of heads at or in front of it, less one.  cluster_start[n_clusters], the end of
// the live slots, has one writer: the first dead slot, or the last slot when it is live.
__global__ __launch_bounds__(DEC_BLOCK) void k_dec_number(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n,
                                                          const uint32_t* __restrict__ blk, const int64_t* __restrict__ chunk_base,
                                                          const int64_t* __restrict__ counts, int32_t* __restrict__ vertex_cluster,
                                                          int32_t* __restrict__ cluster_start, int32_t* __restrict__ cluster_first) {
  __shared__ int s_wave[DEC_WAVES];
  const int64_t s = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  const bool head = is_head(keys, s, n);
  const int rank = block_flag_rank<DEC_BLOCK>(head, s_wave);
  if (s >= n) return;
  const int32_t v = vals[s];
  const int64_t nc = counts[DEC_CLUSTERS];
  if (keys[s] == MESH_DEC_DEAD_KEY) {
    vertex_cluster[v] = -1;
    if (s == 0 || keys[s - 1] != MESH_DEC_DEAD_KEY) cluster_start[nc] = (int32_t)s;
    return;
  }
  const int64_t c = scan_base(chunk_base, 1, 0, blockIdx.x, (int64_t)blk[blockIdx.x]) + rank + (head ? 1 : 0) - 1;
  vertex_cluster[v] = (int32_t)c;
  if (head) { cluster_start[c] = (int32_t)s; cluster_first[c] = v; }
  if (s == n - 1) cluster_start[nc] = (int32_t)n;
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_sizes(int64_t n, const int64_t* __restrict__ counts, const int32_t* __restrict__ cluster_start,
                                                         int32_t* __restrict__ cluster_size) {
  const int64_t c = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (c < n && c < counts[DEC_CLUSTERS]) cluster_size[c] = cluster_start[c + 1] - cluster_start[c];
}

// ------------------------------------------------------------------------------------------------ triangles
__device__ __forceinline__ void load_triangle(const int32_t* __restrict__ triangles, int64_t t, int32_t* v) {
  v[0] = triangles[3 * t]; v[1] = triangles[3 * t + 1]; v[2] = triangles[3 * t + 2];
}

// The clusters of the triangle's vertices: 1 when it is sound (three indices in 0 .. nv - 1, three vertices with a cell).
// No index and no table entry is an address before it is checked; *foreign is set when vertex_cluster holds a number that is
// not -1 .. n_clusters - 1, which sfm_mesh_decimate_cluster never writes.
__device__ __forceinline__ int triangle_clusters(const int32_t* __restrict__ triangles, int64_t t, int64_t n_vertices, int64_t n_clusters,
                                                 const int32_t* __restrict__ vertex_cluster, int32_t* c, bool* foreign) {
  int32_t v[3];
  load_triangle(triangles, t, v);
  if (!mesh_clean::sound(v[0], v[1], v[2], n_vertices)) return 0;
  int ok = 1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = vertex_cluster[v[k]];
    if (c[k] < -1 || c[k] >= n_clusters) { *foreign = true; ok = 0; }
    if (c[k] < 0) ok = 0;
  }
  return ok;
}

// the sorted triple of a live triangle - sound and with three different clusters - and its parity; 0 when it is not live
__device__ __forceinline__ int live_triple(const int32_t* __restrict__ triangles, int64_t t, int64_t n_vertices, int64_t n_clusters,
                                           const int32_t* __restrict__ vertex_cluster, int32_t* s, int* odd) {
  int32_t c[3];
  bool foreign = false;
  if (!triangle_clusters(triangles, t, n_vertices, n_clusters, vertex_cluster, c, &foreign)) return 0;
  return mesh_decimate::sort_triple(c[0], c[1], c[2], s, odd);
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_corner_keys(const int32_t* __restrict__ triangles, int64_t n, int64_t n_vertices, int64_t n_clusters,
                                                               const int32_t* __restrict__ vertex_cluster, int bits, int passes,
                                                               uint32_t* __restrict__ ckeys, int32_t* __restrict__ cvals, uint64_t* __restrict__ tkeys,
                                                               uint32_t* __restrict__ tlow, int32_t* __restrict__ tvals, int64_t* __restrict__ counts) {
  const int64_t h = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  bool unsound = false, degenerate = false, foreign = false;
  if (h < n) {
    const int64_t t = h / 3;
    const int k = (int)(h - 3 * t);
    int32_t c[3];
    const int ok = triangle_clusters(triangles, t, n_vertices, n_clusters, vertex_cluster, c, &foreign);
    ckeys[h] = ok ? (uint32_t)(k == 0 ? c[0] : (k == 1 ? c[1] : c[2])) : MESH_DEC_DEAD_CORNER;
    cvals[h] = (int32_t)h;
    if (k == 0) {
      int32_t s[3];
      int odd;
      const int live = ok && mesh_decimate::sort_triple(c[0], c[1], c[2], s, &odd);
      unsound = !ok;
      degenerate = ok && !live;
      if (passes == 1) tkeys[t] = live ? dec_triple_key(s[0], s[1], s[2], bits) : MESH_DEC_DEAD_KEY;
      else tlow[t] = live ? (uint32_t)s[2] : MESH_DEC_DEAD_CORNER;
      tvals[t] = (int32_t)t;
    } else {
      foreign = false;                                     // lane k = 0 reports it
    }
  }
  wave_count(&counts[DEC_UNSOUND], unsound);
  wave_count(&counts[DEC_DEGENERATE], degenerate);
  if (foreign) counts[DEC_STATUS] = 1;
}

// the second of two passes: the two smaller clusters of the triangle in slot s of the first pass
__global__ __launch_bounds__(DEC_BLOCK) void k_dec_pair_keys(const int32_t* __restrict__ vals, int64_t n, const int32_t* __restrict__ triangles,
                                                             int64_t n_vertices, int64_t n_clusters, const int32_t* __restrict__ vertex_cluster,
                                                             uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (i >= n) return;
  int32_t s[3];
  int odd;
  keys[i] = live_triple(triangles, vals[i], n_vertices, n_clusters, vertex_cluster, s, &odd) ? dec_pair_key(s[0], s[1]) : MESH_DEC_DEAD_KEY;
}

// vals holds the triangles in (triple, triangle) order, the ones that are not live behind the others.  A run of r equal
// triples costs its head r steps; every other lane of the run stops after looking at the slot in front of it.
__global__ __launch_bounds__(DEC_BLOCK) void k_dec_duplicates(const int32_t* __restrict__ vals, int64_t n, const int32_t* __restrict__ triangles,
                                                              int64_t n_vertices, int64_t n_clusters, const int32_t* __restrict__ vertex_cluster,
                                                              uint8_t* __restrict__ keep, int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (i >= n) return;
  int32_t mine[3], other[3];
  int odd;
  const int32_t t = vals[i];
  if (!live_triple(triangles, t, n_vertices, n_clusters, vertex_cluster, mine, &odd)) return;
  if (i > 0) {
    int o;
    if (live_triple(triangles, vals[i - 1], n_vertices, n_clusters, vertex_cluster, other, &o) && other[0] == mine[0] && other[1] == mine[1] &&
        other[2] == mine[2])
      return;
  }
  int64_t n_even = odd ? 0 : 1, n_odd = odd ? 1 : 0, first_even = odd ? -1 : t, first_odd = odd ? t : -1;
  for (int64_t j = i + 1; j < n; ++j) {
    int o;
    const int32_t u = vals[j];
    if (!live_triple(triangles, u, n_vertices, n_clusters, vertex_cluster, other, &o) || other[0] != mine[0] || other[1] != mine[1] || other[2] != mine[2])
      break;
    if (o) { if (n_odd++ == 0) first_odd = u; } else { if (n_even++ == 0) first_even = u; }
  }
  const int64_t pick = mesh_decimate::duplicate_pick(n_even, n_odd, first_even, first_odd);
  if (pick >= 0) keep[pick] = 1;
  const int64_t dropped = n_even + n_odd - (pick >= 0 ? 1 : 0);
  if (dropped > 0) add64(&counts[DEC_DROPPED], dropped);
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_keep_count(const uint8_t* __restrict__ keep, int64_t n, uint32_t* __restrict__ blk) {
  __shared__ int s_wave[DEC_WAVES];
  const int64_t t = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  const int all = block_flag_count<DEC_BLOCK>(t < n && keep[t] != 0, s_wave);
  if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)all;
}

// ------------------------------------------------------------------------------------------------ emit
// the first slot of the sorted corner keys that holds a key >= c
__device__ __forceinline__ int64_t corner_bound(const uint32_t* __restrict__ keys, int64_t n, uint32_t c) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_place(int64_t n_out, int64_t n_vertices, int64_t n_corners, const double* __restrict__ vertices,
                                                         const float* __restrict__ normals, const int32_t* __restrict__ triangles,
                                                         const int32_t* __restrict__ cluster_start, const int32_t* __restrict__ sorted_vertex,
                                                         const uint32_t* __restrict__ corner_key, const int32_t* __restrict__ corner_val, Grid3 g,
                                                         int placement, double* __restrict__ new_vertices, float* __restrict__ new_normals,
                                                         uint8_t* __restrict__ placed) {
  const int64_t c = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  if (c >= n_out) return;
  double x[3] = {0.0, 0.0, 0.0}, ns[3] = {0.0, 0.0, 0.0};
  int took = 0;
  const int64_t beg = cluster_start[c], end = cluster_start[c + 1];
  // always so with the arrays of sfm_mesh_decimate_cluster; anything else writes zeros and reads nothing
  if (beg >= 0 && beg < end && end <= n_vertices) {
    double s[3] = {0.0, 0.0, 0.0}, m[3];
    int64_t members = 0, first = -1;
    for (int64_t i = beg; i < end; ++i) {
      const int64_t v = sorted_vertex[i];
      if (v < 0 || v >= n_vertices) continue;
      if (first < 0) first = v;
      mesh_decimate::add_member(members++, vertices + 3 * v, normals ? normals + 3 * v : nullptr, s, ns);
    }
    if (members > 0) {
      mesh_decimate::mean(s, members, m);
      x[0] = m[0]; x[1] = m[1]; x[2] = m[2];
      int64_t idx[3];
      const double p[3] = {vertices[3 * first], vertices[3 * first + 1], vertices[3 * first + 2]};
      if (placement == 1 && n_corners > 0 && mesh_decimate::vertex_key(p, g.origin, g.cell, idx) != MESH_DEC_DEAD_KEY) {
        double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0}, lo[3], hi[3];
        const int64_t cb = corner_bound(corner_key, n_corners, (uint32_t)c), ce = corner_bound(corner_key, n_corners, (uint32_t)c + 1u);
        for (int64_t i = cb; i < ce; ++i) {
          const int64_t h = corner_val[i];
          if (h < 0 || h >= n_corners) continue;                  // never so with the workspace of sfm_mesh_decimate_mark
          const int64_t t = h / 3;
          int32_t w[3];
          load_triangle(triangles, t, w);
          if (!mesh_clean::sound(w[0], w[1], w[2], n_vertices)) continue;
          mesh_decimate::add_corner(vertices + 3 * (int64_t)w[0], vertices + 3 * (int64_t)w[1], vertices + 3 * (int64_t)w[2], m, A, q);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          lo[a] = mesh_decimate::cell_lo(g.origin[a], g.cell, idx[a]);
          hi[a] = mesh_decimate::cell_hi(g.origin[a], g.cell, idx[a]);
        }
        took = mesh_decimate::place(A, q, m, lo, hi, x);
      }
    }
  }
  new_vertices[3 * c] = x[0]; new_vertices[3 * c + 1] = x[1]; new_vertices[3 * c + 2] = x[2];
  placed[c] = (uint8_t)took;
  if (normals) {
    float out[3];
    mesh_decimate::unit_normal(ns, out);
    new_normals[3 * c] = out[0]; new_normals[3 * c + 1] = out[1]; new_normals[3 * c + 2] = out[2];
  }
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_emit_triangles(int64_t n, int64_t n_vertices, int64_t n_clusters, const int32_t* __restrict__ triangles,
                                                                  const int32_t* __restrict__ vertex_cluster, const uint8_t* __restrict__ keep,
                                                                  const uint32_t* __restrict__ blk, const int64_t* __restrict__ chunk_base, int64_t cap,
                                                                  int32_t* __restrict__ new_triangles, int32_t* __restrict__ triangle_map) {
  __shared__ int s_wave[DEC_WAVES];
  const int64_t t = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
  const bool kept = t < n && keep[t] != 0;
  const int rank = block_flag_rank<DEC_BLOCK>(kept, s_wave);
  if (!kept) return;
  const int64_t slot = scan_base(chunk_base, 1, 0, blockIdx.x, (int64_t)blk[blockIdx.x]) + rank;
  if (slot < 0 || slot >= cap) return;
  // always live with the flags of sfm_mesh_decimate_mark
  int32_t c[3] = {-1, -1, -1};
  bool foreign = false;
  const int ok = triangle_clusters(triangles, t, n_vertices, n_clusters, vertex_cluster, c, &foreign);
  new_triangles[3 * slot] = ok ? c[0] : -1;
  new_triangles[3 * slot + 1] = ok ? c[1] : -1;
  new_triangles[3 * slot + 2] = ok ? c[2] : -1;
  triangle_map[slot] = (int32_t)t;
}

// ------------------------------------------------------------------------------------------------ host
template <typename K>
hipError_t sort_pairs(void* tmp, size_t& tmp_bytes, K* keys_in, K* keys_out, int32_t* vals_in, int32_t* vals_out, int64_t n, int end_bit,
                      hipStream_t stream) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, (unsigned)end_bit, stream);
}

// the most temporary storage any sort of the three calls asks for: the vertex sort, the corner sort and the triple sorts at
// their widest cuts
hipError_t sort_room(int64_t n_vertices, int64_t n_triangles, hipStream_t stream, size_t* room) {
  size_t most = 0, b = 0;
  hipError_t e = hipSuccess;
  if (n_vertices > 0) {
    e = sort_pairs<uint64_t>(nullptr, b, nullptr, nullptr, nullptr, nullptr, n_vertices, 64, stream);
    if (e != hipSuccess) return e;
    most = b > most ? b : most;
  }
  if (n_triangles > 0) {
    e = sort_pairs<uint32_t>(nullptr, b, nullptr, nullptr, nullptr, nullptr, 3 * n_triangles, 32, stream);
    if (e != hipSuccess) return e;
    most = b > most ? b : most;
    e = sort_pairs<uint64_t>(nullptr, b, nullptr, nullptr, nullptr, nullptr, n_triangles, 64, stream);
    if (e != hipSuccess) return e;
    most = b > most ? b : most;
    e = sort_pairs<uint32_t>(nullptr, b, nullptr, nullptr, nullptr, nullptr, n_triangles, 32, stream);
    if (e != hipSuccess) return e;
    most = b > most ? b : most;
  }
  *room = most;
  return hipSuccess;
}

Grid3 grid_of(const double* origin, double cell) {
  Grid3 g;
  g.origin[0] = origin[0]; g.origin[1] = origin[1]; g.origin[2] = origin[2];
  g.cell = cell;
  return g;
}

}  // namespace

extern "C" int sfm_mesh_decimate_workspace_bytes(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t* bytes_host) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_decimate_workspace_bytes";
  if (!bytes_host) return sfm_fail(h, SFM_ERR_ARG, what, DEC_WHY[5]);
  if (dec_check_counts(n_vertices, n_triangles)) return sfm_fail(h, SFM_ERR_ARG, what, DEC_WHY[1]);
  size_t room = 0;
  SFM_HIP(h, sort_room(n_vertices, n_triangles, h->stream, &room));
  *bytes_host = dec_layout(n_vertices, n_triangles, (int64_t)room).bytes;
  return SFM_OK;
}

extern "C" int sfm_mesh_decimate_cluster(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const double* vertices, const double* origin, double cell,
                                         int32_t* vertex_cluster, int32_t* cluster_start, int32_t* cluster_first, int32_t* cluster_size,
                                         int64_t* counts, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_decimate_cluster";
  int bad = dec_check_cluster(n_vertices, n_triangles, vertices, origin, cell, vertex_cluster, cluster_start, cluster_first, cluster_size, counts);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, DEC_WHY[bad]);
  size_t room = 0;
  SFM_HIP(h, sort_room(n_vertices, n_triangles, h->stream, &room));
  const DecLayout L = dec_layout(n_vertices, n_triangles, (int64_t)room);
  bad = dec_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, DEC_WHY[bad]);
  SFM_HIP(h, hipMemsetAsync(counts, 0, DEC_CLUSTER_COUNTS * sizeof(int64_t), h->stream));
  const int64_t n = n_vertices;
  if (n == 0) {
    SFM_HIP(h, hipMemsetAsync(cluster_start, 0, sizeof(int32_t), h->stream));
    return SFM_OK;
  }
  char* ws = (char*)workspace;
  uint64_t* d_keys_in = (uint64_t*)(ws + L.vkey_in);
  uint64_t* d_keys = (uint64_t*)(ws + L.vkey_out);
  int32_t* d_vals_in = (int32_t*)(ws + L.vval_in);
  int32_t* d_vals = (int32_t*)(ws + L.sorted_vertex);
  uint32_t* d_blk = (uint32_t*)(ws + L.vblk);
  int64_t* d_chunk = (int64_t*)(ws + L.vchunk);
  const int64_t nb = dec_blocks(n), n_chunks = scan_chunks(nb);
  const dim3 tb(DEC_BLOCK), grid((unsigned)nb);
  hipLaunchKernelGGL(k_dec_vertex_keys, grid, tb, 0, h->stream, vertices, n, grid_of(origin, cell), d_keys_in, d_vals_in, counts);
  SFM_LAUNCH_CHECK(h, what);
  size_t sort_bytes = room;
  SFM_HIP(h, sort_pairs<uint64_t>(ws + L.sort, sort_bytes, d_keys_in, d_keys, d_vals_in, d_vals, n, 64, h->stream));
  hipLaunchKernelGGL(k_dec_heads, grid, tb, 0, h->stream, (const uint64_t*)d_keys, n, d_blk);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_dec_scan_chunks, dim3((unsigned)n_chunks), tb, 0, h->stream, d_blk, nb, d_chunk);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_dec_scan_top, dim3(1), tb, 0, h->stream, d_chunk, n_chunks, counts + DEC_CLUSTERS);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_dec_number, grid, tb, 0, h->stream, (const uint64_t*)d_keys, (const int32_t*)d_vals, n, (const uint32_t*)d_blk,
                     (const int64_t*)d_chunk, (const int64_t*)counts, vertex_cluster, cluster_start, cluster_first);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_dec_sizes, grid, tb, 0, h->stream, n, (const int64_t*)counts, (const int32_t*)cluster_start, cluster_size);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}

extern "C" int sfm_mesh_decimate_mark(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t n_clusters, const int32_t* triangles,
                                      const int32_t* vertex_cluster, uint8_t* triangle_keep, int64_t* counts, void* workspace,
                                      int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_decimate_mark";
  int bad = dec_check_mark(n_vertices, n_triangles, n_clusters, triangles, vertex_cluster, triangle_keep, counts);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, DEC_WHY[bad]);
  size_t room = 0;
  SFM_HIP(h, sort_room(n_vertices, n_triangles, h->stream, &room));
  const DecLayout L = dec_layout(n_vertices, n_triangles, (int64_t)room);
  bad = dec_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, DEC_WHY[bad]);
  SFM_HIP(h, hipMemsetAsync(counts, 0, DEC_MARK_COUNTS * sizeof(int64_t), h->stream));
  const int64_t nt = n_triangles, n = 3 * n_triangles;
  if (nt == 0) return SFM_OK;
  char* ws = (char*)workspace;
  uint32_t* d_ckey_in = (uint32_t*)(ws + L.ckey_in);
  uint32_t* d_ckey = (uint32_t*)(ws + L.corner_key);
  int32_t* d_cval_in = (int32_t*)(ws + L.cval_in);
  int32_t* d_cval = (int32_t*)(ws + L.corner_val);
  uint64_t* d_tkey_in = (uint64_t*)(ws + L.tkey_in);
  uint64_t* d_tkey = (uint64_t*)(ws + L.tkey_out);
  uint32_t* d_tlow_in = (uint32_t*)(ws + L.tlow_in);
  uint32_t* d_tlow = (uint32_t*)(ws + L.tlow_out);
  int32_t* d_tval_a = (int32_t*)(ws + L.tval_a);
  int32_t* d_tval_b = (int32_t*)(ws + L.tval_b);
  uint32_t* d_blk = (uint32_t*)(ws + L.tri_blk);
  int64_t* d_chunk = (int64_t*)(ws + L.tri_chunk);
  const int bits = dec_cluster_bits(n_clusters), passes = dec_triple_passes(n_clusters);
  const int64_t cb = dec_blocks(n), nb = dec_blocks(nt), n_chunks = scan_chunks(nb);
  const dim3 tb(DEC_BLOCK), grid((unsigned)nb);
  SFM_HIP(h, hipMemsetAsync(triangle_keep, 0, (size_t)nt, h->stream));
  hipLaunchKernelGGL(k_dec_corner_keys, dim3((unsigned)cb), tb, 0, h->stream, triangles, n, n_vertices, n_clusters, vertex_cluster, bits, passes,
                     d_ckey_in, d_cval_in, d_tkey_in, d_tlow_in, d_tval_a, counts);
  SFM_LAUNCH_CHECK(h, what);
  size_t sort_bytes = room;
  SFM_HIP(h, sort_pairs<uint32_t>(ws + L.sort, sort_bytes, d_ckey_in, d_ckey, d_cval_in, d_cval, n, bits, h->stream));
  const int32_t* d_order = d_tval_b;
  if (passes == 1) {
    sort_bytes = room;
    SFM_HIP(h, sort_pairs<uint64_t>(ws + L.sort, sort_bytes, d_tkey_in, d_tkey, d_tval_a, d_tval_b, nt, 3 * bits, h->stream));
  } else {
    sort_bytes = room;
    SFM_HIP(h, sort_pairs<uint32_t>(ws + L.sort, sort_bytes, d_tlow_in, d_tlow, d_tval_a, d_tval_b, nt, bits, h->stream));
    hipLaunchKernelGGL(k_dec_pair_keys, grid, tb, 0, h->stream, (const int32_t*)d_tval_b, nt, triangles, n_vertices, n_clusters, vertex_cluster,
                       d_tkey_in);
    SFM_LAUNCH_CHECK(h, what);
    sort_bytes = room;
    SFM_HIP(h, sort_pairs<uint64_t>(ws + L.sort, sort_bytes, d_tkey_in, d_tkey, d_tval_b, d_tval_a, nt, 32 + bits, h->stream));
    d_order = d_tval_a;
  }
  hipLaunchKernelGGL(k_dec_duplicates, grid, tb, 0, h->stream, d_order, nt, triangles, n_vertices, n_clusters, vertex_cluster, triangle_keep, counts);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_dec_keep_count, grid, tb, 0, h->stream, (const uint8_t*)triangle_keep, nt, d_blk);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_dec_scan_chunks, dim3((unsigned)n_chunks), tb, 0, h->stream, d_blk, nb, d_chunk);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_dec_scan_top, dim3(1), tb, 0, h->stream, d_chunk, n_chunks, counts + DEC_KEPT);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}

extern "C" int sfm_mesh_decimate_emit(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t n_clusters, const double* vertices,
                                      const float* normals, const int32_t* triangles, const int32_t* vertex_cluster, const int32_t* cluster_start,
                                      const uint8_t* triangle_keep, const double* origin, double cell, int placement, int64_t cap_clusters,
                                      int64_t cap_triangles, double* new_vertices, float* new_normals, uint8_t* cluster_placed,
                                      int32_t* new_triangles, int32_t* triangle_map, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_decimate_emit";
  int bad = dec_check_emit_counts(n_vertices, n_triangles, n_clusters, cap_clusters, cap_triangles, placement, origin, cell);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, DEC_WHY[bad]);
  size_t room = 0;
  SFM_HIP(h, sort_room(n_vertices, n_triangles, h->stream, &room));
  const DecLayout L = dec_layout(n_vertices, n_triangles, (int64_t)room);
  bad = dec_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, DEC_WHY[bad]);
  if (cap_clusters == 0 && cap_triangles == 0) return SFM_OK;
  bad = dec_check_emit_pointers(n_triangles, cap_clusters, cap_triangles, vertices, normals, triangles, vertex_cluster, cluster_start, triangle_keep,
                                new_vertices, new_normals, cluster_placed, new_triangles, triangle_map);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, DEC_WHY[bad]);
  char* ws = (char*)workspace;
  const dim3 tb(DEC_BLOCK);
  const int64_t n_out = n_clusters < cap_clusters ? n_clusters : cap_clusters;
  if (n_out > 0) {
    hipLaunchKernelGGL(k_dec_place, dim3((unsigned)dec_blocks(n_out)), tb, 0, h->stream, n_out, n_vertices, 3 * n_triangles, vertices, normals, triangles,
                       cluster_start, (const int32_t*)(ws + L.sorted_vertex), (const uint32_t*)(ws + L.corner_key),
                       (const int32_t*)(ws + L.corner_val), grid_of(origin, cell), placement, new_vertices, new_normals, cluster_placed);
    SFM_LAUNCH_CHECK(h, what);
  }
  if (cap_triangles > 0 && n_triangles > 0) {
    hipLaunchKernelGGL(k_dec_emit_triangles, dim3((unsigned)dec_blocks(n_triangles)), tb, 0, h->stream, n_triangles, n_vertices, n_clusters, triangles,
                       vertex_cluster, triangle_keep, (const uint32_t*)(ws + L.tri_blk), (const int64_t*)(ws + L.tri_chunk), cap_triangles,
                       new_triangles, triangle_map);
    SFM_LAUNCH_CHECK(h, what);
  }
  return SFM_OK;
}
