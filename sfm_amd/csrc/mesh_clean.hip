// The connected components of a triangle mesh and the removal of the small ones, for gfx950 (MI355X).  include/sfm_amd.h
// states the rule; mesh_clean_rule.h holds the selection, mesh_clean_plan.h the argument checks, the workspace layouts and
// the grids; the scans are those of block_scan.h / scan_plan.h.  Integers only: every output byte is a function of the
// inputs, whatever the order of the triangles, of the indices within one or of the lanes.
//
// sfm_mesh_components
//   k_cc_init          parent[v] = v, the counts to zero
//   k_cc_hook          one lane per triangle, two unions: "the larger root goes under the smaller id" (atomicCAS on a root
//                      only); every find halves the path it walks (atomicMin towards the grandparent), and every lane ends
//                      with one more find from its largest vertex
//   k_cc_flatten       one lane per vertex: find with halving, then parent[v] = root; the roots of the block are counted
//   k_cc_scan_*        the two-level scan of the root counts -> counts[0]
//   k_cc_number        a root takes its number (block base + rank), writes comp_root and zeroes its two counts
//   k_cc_label         vertex_component, triangle_component and the per-component counts: one integer atomicAdd per run of
//                      equal components within a wavefront
// sfm_mesh_clean_mark
//   k_clean_select     ONE workgroup: the candidates, the radix select of the cut, the ties with a running carry -> comp_keep
//   k_clean_count      kept vertices and kept triangles per block, packed; k_clean_scan_* their two-level scan -> counts
// sfm_mesh_clean_emit
//   k_clean_emit_vertices   vertex_map, the copied rows, the new index of every vertex
//   k_clean_emit_triangles  triangle_map and the renumbered triangles
// sfm_mesh_gather_rows      k_gather_rows
// Nothing waits on another workgroup; no atomic decides an order.
#include "common.h"
#include "mesh_clean_rule.h"
#include "mesh_clean_plan.h"
#include "block_scan.h"

namespace {

constexpr int CLEAN_WAVES = CLEAN_BLOCK / 64;
static_assert(CLEAN_BLOCK == MESH_CLEAN_RADIX_BINS, "a thread of the selection clears one bin");

__device__ __forceinline__ void add64(int64_t* p, int64_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// tracks.hip explains it: the 8 XCDs have private L2s and every CU its own L1, so while `parent` is being written (the hook
// and the flatten kernel) it is only read with agent-scope atomic loads, and written by atomics.
__device__ __forceinline__ int parent_of(const int* parent, int v) {
  return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above v, halving the path on the way.  Invariant of `parent`: parent[v] <= v, and parent[v] is a node of v's
// tree.  A root is re-parented by the CAS of the hook alone; a node that is NOT a root only ever sees atomicMin with one of
// its ancestors at the time of the read, which is smaller than its parent: the pointer moves to a smaller node of the same
// tree or stays, whatever other lanes do in between, so chains keep descending strictly and end.  A non-root never becomes
// a root again, so the halving never touches a word a CAS expects to be a root's.  Every step lowers v; *budget counts them.
__device__ __forceinline__ int find_halving(int* parent, int v, int64_t* budget) {
  for (;;) {
    const int p = parent_of(parent, v);
    if (p == v) return v;
    const int g = parent_of(parent, p);
    if (g == p) return p;
    atomicMin(&parent[v], g);
    v = g;
    if (--*budget < 0) return v;
  }
}

// true when the budget ran out
__device__ __forceinline__ bool unite(int* parent, int a, int b, int64_t* budget) {
  int ra = a, rb = b;
  for (;;) {
    ra = find_halving(parent, ra, budget);
    rb = find_halving(parent, rb, budget);
    if (*budget < 0) return true;
    if (ra == rb) return false;
    const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    const int old = atomicCAS(&parent[hi], hi, lo);
    if (old == hi) return false;
    ra = old; rb = lo;                                   // from what the atomic returned, never from a plain re-read
    if (--*budget < 0) return true;
  }
}

__global__ __launch_bounds__(CLEAN_BLOCK) void k_cc_init(int64_t n_vertices, int* __restrict__ parent, int64_t* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
  if (v < n_vertices) parent[v] = (int)v;
  if (v < CC_COUNTS) counts[v] = 0;
}

__global__ __launch_bounds__(CLEAN_BLOCK) void k_cc_hook(const int32_t* __restrict__ triangles, int64_t n_triangles, int64_t n_vertices,
                                                         int* parent, int64_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
  const bool in = t < n_triangles;
  int a = 0, b = 0, c = 0;
  if (in) { a = triangles[3 * t]; b = triangles[3 * t + 1]; c = triangles[3 * t + 2]; }
  const bool ok = in && mesh_clean::sound(a, b, c, n_vertices);
  // the unsound triangles of the wavefront in one add
  const unsigned long long bad = __ballot(in && !ok);
  if ((threadIdx.x & 63) == 0 && bad) add64(&counts[CC_UNSOUND], __popcll(bad));
  if (!ok) return;
  int64_t budget = cc_budget(n_vertices);
  bool out = false;
  if (a != b) out = unite(parent, a, b, &budget);
  if (!out && c != a && c != b) out = unite(parent, a, c, &budget);     // a repeated index is joined already
  // One more find, from the lane's largest vertex.  The lanes of a wavefront hooked their roots at the same moment, which on
  // a path builds a chain as long as the lanes in flight; walking it now, in step with the neighbours, halves it everywhere
  // at once - pointer doubling - before a later wavefront has to walk it alone.  On a triangle strip the second union does
  // this already; on a path given as one-edge triangles (i, i + 1, i + 1) nothing else does: 147 ms without, 2 ms with, at
  // 2^20 vertices.
  if (!out) {
    const int top = a > b ? (a > c ? a : c) : (b > c ? b : c);
    find_halving(parent, top, &budget);
    out = budget < 0;
  }
  if (out) counts[CC_STATUS] = 1;
}

// A launch of its own: every link is in place, no root changes any more.  The halving goes on beside the other lanes' finds.
__global__ __launch_bounds__(CLEAN_BLOCK) void k_cc_flatten(int64_t n_vertices, int* parent, uint32_t* __restrict__ blk,
                                                            int64_t* __restrict__ counts) {
  __shared__ int s_wave[CLEAN_WAVES];
  const int64_t v = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
  bool root = false;
  if (v < n_vertices) {
    int64_t budget = cc_budget(n_vertices);
    const int r = find_halving(parent, (int)v, &budget);
    if (budget < 0) counts[CC_STATUS] = 1;
    root = r == (int)v;
    if (!root) atomicMin(&parent[v], r);
  }
  const int all = block_flag_count<CLEAN_BLOCK>(root, s_wave);
  if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)all;
}

__global__ __launch_bounds__(CLEAN_BLOCK) void k_cc_scan_chunks(uint32_t* __restrict__ blk, int64_t n_blocks, int64_t* __restrict__ chunk_sum) {
  __shared__ int64_t s_wave[CLEAN_WAVES];
  const int64_t total = scan_chunk_counts(blk, n_blocks, s_wave);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(CLEAN_BLOCK) void k_cc_scan_top(int64_t* __restrict__ chunk_sum, int64_t n_chunks, int64_t* __restrict__ counts) {
  __shared__ int64_t s_wave[CLEAN_WAVES];
  const int64_t all = scan_chunk_totals(chunk_sum, n_chunks, 1, s_wave);
  if (threadIdx.x == 0) counts[CC_COMPONENTS] = all;
}

__global__ __launch_bounds__(CLEAN_BLOCK) void k_cc_number(int64_t n_vertices, const int* __restrict__ parent, const uint32_t* __restrict__ blk,
                                                           const int64_t* __restrict__ chunk_base, int* __restrict__ number,
                                                           int32_t* __restrict__ comp_root, int32_t* __restrict__ comp_vertices,
                                                           int32_t* __restrict__ comp_triangles) {
  __shared__ int s_wave[CLEAN_WAVES];
  const int64_t v = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
  const bool root = v < n_vertices && parent[v] == (int)v;
  const int rank = block_flag_rank<CLEAN_BLOCK>(root, s_wave);
  if (v >= n_vertices) return;
  if (!root) { number[v] = -1; return; }
  const int64_t c = scan_base(chunk_base, 1, 0, blockIdx.x, (int64_t)blk[blockIdx.x]) + rank;
  number[v] = (int)c;
  comp_root[c] = (int32_t)v;
  comp_vertices[c] = 0;
  comp_triangles[c] = 0;
}

// table[c] += 1 for every lane with c >= 0, as one add per run of equal c over consecutive lanes: a mesh that is one
// component costs one add per wavefront, not one per lane on one word.  Every lane of the wavefront must call.
__device__ __forceinline__ void add_runs(int32_t* table, int c) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(c, 1, 64);
  const bool head = lane == 0 || prev != c;
  const unsigned long long heads = __ballot(head);
  if (head && c >= 0) {
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    atomicAdd(&table[c], after ? (int)__ffsll((unsigned long long)after) : 64 - lane);
  }
}

__global__ __launch_bounds__(CLEAN_BLOCK) void k_cc_label(int64_t n_vertices, int64_t n_triangles, const int32_t* __restrict__ triangles,
                                                          const int* __restrict__ parent, const int* __restrict__ number,
                                                          int32_t* __restrict__ vertex_component, int32_t* __restrict__ triangle_component,
                                                          int32_t* comp_vertices, int32_t* comp_triangles) {
  const int64_t i = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
  // parent[] holds the roots, whose numbers are set; after a failed call (the status word) it may hold another vertex, whose
  // number is -1: nothing is added then
  int cv = -1, ct = -1;
  if (i < n_vertices) {
    cv = number[parent[i]];
    vertex_component[i] = cv;
  }
  if (i < n_triangles) {
    const int a = triangles[3 * i], b = triangles[3 * i + 1], c = triangles[3 * i + 2];
    if (mesh_clean::sound(a, b, c, n_vertices)) ct = number[parent[a]];
    triangle_component[i] = ct;
  }
  add_runs(comp_vertices, cv);
  add_runs(comp_triangles, ct);
}

// ------------------------------------------------------------------------------------------------ selection
// ONE workgroup, serial in the number of components: six walks over comp_triangles when the cut applies, two otherwise.
__global__ __launch_bounds__(CLEAN_BLOCK) void k_clean_select(int64_t n_components, const int32_t* __restrict__ comp_triangles, int64_t min_triangles,
                                                              int64_t keep_largest, uint8_t* __restrict__ comp_keep, int64_t* __restrict__ counts,
                                                              int64_t* __restrict__ sel) {
  __shared__ int64_t s_wave[CLEAN_WAVES];
  __shared__ int32_t s_hist[MESH_CLEAN_RADIX_BINS];
  __shared__ mesh_clean::Cut s_cut;
  int64_t mine = 0;
  for (int64_t c = threadIdx.x; c < n_components; c += CLEAN_BLOCK) mine += mesh_clean::candidate(comp_triangles[c], min_triangles) ? 1 : 0;
  int64_t n_cand;
  block_exclusive_scan<CLEAN_BLOCK, int64_t>(mine, s_wave, &n_cand);
  const bool cutting = keep_largest > 0 && n_cand > keep_largest;
  if (threadIdx.x == 0) s_cut = mesh_clean::Cut{0u, keep_largest};
  if (cutting)
    for (int pass = 0; pass < MESH_CLEAN_RADIX_PASSES; ++pass) {
      s_hist[threadIdx.x] = 0;
      __syncthreads();
      const uint32_t prefix = s_cut.prefix;
      for (int64_t c = threadIdx.x; c < n_components; c += CLEAN_BLOCK) {
        const int32_t size = comp_triangles[c];
        if (mesh_clean::candidate(size, min_triangles) && mesh_clean::radix_match((uint32_t)size, prefix, pass))
          atomicAdd(&s_hist[mesh_clean::radix_bin((uint32_t)size, pass)], 1);
      }
      __syncthreads();
      if (threadIdx.x == 0) mesh_clean::radix_step(s_hist, pass, &s_cut);
      __syncthreads();
    }
  __syncthreads();
  const uint32_t s = s_cut.prefix;
  const int64_t ties_kept = s_cut.left;
  int64_t carry = 0, kept = 0;
  for (int64_t first = 0; first < n_components; first += CLEAN_BLOCK) {
    const int64_t c = first + threadIdx.x;
    const bool in = c < n_components;
    const int32_t size = in ? comp_triangles[c] : 0;
    const bool tie = in && cutting && mesh_clean::candidate(size, min_triangles) && (uint32_t)size == s;
    int64_t ties;
    const int64_t before = block_exclusive_scan<CLEAN_BLOCK, int64_t>(tie ? 1 : 0, s_wave, &ties);
    if (in) {
      const bool keep = mesh_clean::keeps(size, min_triangles, cutting, s, carry + before, ties_kept);
      comp_keep[c] = keep ? 1 : 0;
      kept += keep ? 1 : 0;
    }
    carry += ties;
  }
  int64_t all;
  block_exclusive_scan<CLEAN_BLOCK, int64_t>(kept, s_wave, &all);
  if (threadIdx.x == 0) {
    counts[CLEAN_COMPONENTS] = all;
    sel[0] = n_cand; sel[1] = cutting ? 1 : 0; sel[2] = (int64_t)s; sel[3] = ties_kept;
  }
}

__device__ __forceinline__ bool kept_component(const uint8_t* __restrict__ comp_keep, int64_t n_components, int c) {
  return c >= 0 && c < n_components && comp_keep[c] != 0;
}

__global__ __launch_bounds__(CLEAN_BLOCK) void k_clean_count(int64_t n_vertices, int64_t n_triangles, int64_t n_components,
                                                             const int32_t* __restrict__ vertex_component, const int32_t* __restrict__ triangle_component,
                                                             const uint8_t* __restrict__ comp_keep, uint64_t* __restrict__ blk) {
  __shared__ int s_v[CLEAN_WAVES], s_t[CLEAN_WAVES];
  const int64_t i = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
  const bool fv = i < n_vertices && kept_component(comp_keep, n_components, vertex_component[i]);
  const bool ft = i < n_triangles && kept_component(comp_keep, n_components, triangle_component[i]);
  const int nv = block_flag_count<CLEAN_BLOCK>(fv, s_v);
  const int nt = block_flag_count<CLEAN_BLOCK>(ft, s_t);
  if (threadIdx.x == 0) blk[blockIdx.x] = clean_count_pack((uint32_t)nv, (uint32_t)nt);
}

__global__ __launch_bounds__(CLEAN_BLOCK) void k_clean_scan_chunks(uint64_t* __restrict__ blk, int64_t n_blocks, int64_t* __restrict__ chunk_sum) {
  __shared__ int64_t s_wave[CLEAN_WAVES];
  const int64_t total = scan_chunk_counts(blk, n_blocks, s_wave);   // neither half leaves its 32 bits within a chunk
  if (threadIdx.x == 0) {
    chunk_sum[2 * (int64_t)blockIdx.x] = total & 0xFFFFFFFFll;
    chunk_sum[2 * (int64_t)blockIdx.x + 1] = total >> 32;
  }
}

__global__ __launch_bounds__(CLEAN_BLOCK) void k_clean_scan_top(int64_t* __restrict__ chunk_sum, int64_t n_chunks, int64_t* __restrict__ counts) {
  __shared__ int64_t s_wave[CLEAN_WAVES];
  for (int half = 0; half < 2; ++half) {
    const int64_t all = scan_chunk_totals(chunk_sum + half, n_chunks, 2, s_wave);
    if (threadIdx.x == 0) counts[CLEAN_VERTICES + half] = all;
  }
}

// ------------------------------------------------------------------------------------------------ emit
// The rows are copied as integers: bit for bit, whatever they hold.
__global__ __launch_bounds__(CLEAN_BLOCK) void k_clean_emit_vertices(int64_t n_vertices, int64_t n_components, const int32_t* __restrict__ vertex_component,
                                                                     const uint8_t* __restrict__ comp_keep, const uint64_t* __restrict__ blk,
                                                                     const int64_t* __restrict__ chunk_base, const uint64_t* __restrict__ vertices,
                                                                     const uint32_t* __restrict__ normals, int64_t cap_vertices,
                                                                     int32_t* __restrict__ new_index, int32_t* __restrict__ vertex_map,
                                                                     uint64_t* __restrict__ vertices_out, uint32_t* __restrict__ normals_out) {
  __shared__ int s_wave[CLEAN_WAVES];
  const int64_t v = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
  const bool in = v < n_vertices;
  const bool keep = in && kept_component(comp_keep, n_components, vertex_component[v]);
  const int rank = block_flag_rank<CLEAN_BLOCK>(keep, s_wave);
  if (!in) return;
  const int64_t slot = clean_vertex_base(chunk_base, blk, blockIdx.x) + rank;
  new_index[v] = keep ? (int32_t)slot : -1;
  // a workspace that is not the mark call's, or a capacity below the truth, writes nothing outside the outputs
  if (!keep || slot < 0 || slot >= cap_vertices) return;
  vertex_map[slot] = (int32_t)v;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    vertices_out[slot * 3 + a] = vertices[v * 3 + a];
    normals_out[slot * 3 + a] = normals[v * 3 + a];
  }
}

__global__ __launch_bounds__(CLEAN_BLOCK) void k_clean_emit_triangles(int64_t n_vertices, int64_t n_triangles, int64_t n_components,
                                                                      const int32_t* __restrict__ triangle_component, const uint8_t* __restrict__ comp_keep,
                                                                      const uint64_t* __restrict__ blk, const int64_t* __restrict__ chunk_base,
                                                                      const int32_t* __restrict__ triangles, const int32_t* __restrict__ new_index,
                                                                      int64_t cap_triangles, int32_t* __restrict__ triangle_map,
                                                                      int32_t* __restrict__ triangles_out) {
  __shared__ int s_wave[CLEAN_WAVES];
  const int64_t t = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
  const bool in = t < n_triangles;
  const bool keep = in && kept_component(comp_keep, n_components, triangle_component[t]);
  const int rank = block_flag_rank<CLEAN_BLOCK>(keep, s_wave);
  if (!keep) return;
  const int64_t slot = clean_triangle_base(chunk_base, blk, blockIdx.x) + rank;
  if (slot < 0 || slot >= cap_triangles) return;
  const int a = triangles[3 * t], b = triangles[3 * t + 1], c = triangles[3 * t + 2];
  // always sound with the labels of sfm_mesh_components; an index is never an address otherwise
  const bool ok = mesh_clean::sound(a, b, c, n_vertices);
  triangle_map[slot] = (int32_t)t;
  triangles_out[slot * 3] = ok ? new_index[a] : -1;
  triangles_out[slot * 3 + 1] = ok ? new_index[b] : -1;
  triangles_out[slot * 3 + 2] = ok ? new_index[c] : -1;
}

// ------------------------------------------------------------------------------------------------ gather
// dst row i = src row map[i], U bytes per thread in a grid-stride loop over the units of dst
template <typename U>
__global__ __launch_bounds__(CLEAN_BLOCK) void k_gather_rows(const U* __restrict__ src, int64_t row_units, const int32_t* __restrict__ map, int64_t n,
                                                             U* __restrict__ dst) {
  const int64_t total = n * row_units, stride = (int64_t)gridDim.x * CLEAN_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x; i < total; i += stride) {
    const int64_t row = i / row_units, u = i - row * row_units;
    const int64_t from = map[row];
    if (from >= 0) dst[i] = src[from * row_units + u];
  }
}

template <typename U>
void launch_gather(sfm_ctx* h, const void* src, int64_t row_bytes, const int32_t* map, int64_t n, void* dst) {
  const int64_t row_units = row_bytes / (int64_t)sizeof(U);
  hipLaunchKernelGGL(k_gather_rows<U>, dim3((unsigned)clean_gather_blocks(n * row_units)), dim3(CLEAN_BLOCK), 0, h->stream, (const U*)src, row_units,
                     map, n, (U*)dst);
}

}  // namespace

extern "C" int sfm_mesh_components_workspace_bytes(int64_t n_vertices, int64_t* bytes_host) {
  if (!bytes_host || n_vertices < 0 || n_vertices > CLEAN_MAX_COUNT) return SFM_ERR_ARG;
  *bytes_host = cc_layout(n_vertices).bytes;
  return SFM_OK;
}

extern "C" int sfm_mesh_components(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const int32_t* triangles, int32_t* vertex_component,
                                   int32_t* triangle_component, int32_t* comp_root, int32_t* comp_vertices, int32_t* comp_triangles,
                                   int64_t* counts, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_components";
  int bad = cc_check(n_vertices, n_triangles, triangles, vertex_component, triangle_component, comp_root, comp_vertices, comp_triangles, counts);
  const CcLayout L = cc_layout(bad ? 0 : n_vertices);
  if (!bad) bad = clean_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, CLEAN_WHY[bad]);
  char* ws = (char*)workspace;
  int* d_parent = (int*)(ws + L.parent);
  int* d_number = (int*)(ws + L.number);
  uint32_t* d_blk = (uint32_t*)(ws + L.blk);
  int64_t* d_chunk = (int64_t*)(ws + L.chunk_base);
  const int64_t nbv = clean_blocks(n_vertices), nbt = clean_blocks(n_triangles), n_chunks = scan_chunks(nbv);
  const dim3 tb(CLEAN_BLOCK);
  hipLaunchKernelGGL(k_cc_init, dim3((unsigned)clean_max(nbv, 1)), tb, 0, h->stream, n_vertices, d_parent, counts);
  SFM_LAUNCH_CHECK(h, what);
  if (n_triangles > 0) {
    hipLaunchKernelGGL(k_cc_hook, dim3((unsigned)nbt), tb, 0, h->stream, triangles, n_triangles, n_vertices, d_parent, counts);
    SFM_LAUNCH_CHECK(h, what);
  }
  if (n_vertices > 0) {
    hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)nbv), tb, 0, h->stream, n_vertices, d_parent, d_blk, counts);
    SFM_LAUNCH_CHECK(h, what);
    hipLaunchKernelGGL(k_cc_scan_chunks, dim3((unsigned)n_chunks), tb, 0, h->stream, d_blk, nbv, d_chunk);
    SFM_LAUNCH_CHECK(h, what);
    hipLaunchKernelGGL(k_cc_scan_top, dim3(1), tb, 0, h->stream, d_chunk, n_chunks, counts);
    SFM_LAUNCH_CHECK(h, what);
    hipLaunchKernelGGL(k_cc_number, dim3((unsigned)nbv), tb, 0, h->stream, n_vertices, (const int*)d_parent, (const uint32_t*)d_blk,
                       (const int64_t*)d_chunk, d_number, comp_root, comp_vertices, comp_triangles);
    SFM_LAUNCH_CHECK(h, what);
  }
  if (n_vertices > 0 || n_triangles > 0) {
    hipLaunchKernelGGL(k_cc_label, dim3((unsigned)clean_max(nbv, nbt)), tb, 0, h->stream, n_vertices, n_triangles, triangles, (const int*)d_parent,
                       (const int*)d_number, vertex_component, triangle_component, comp_vertices, comp_triangles);
    SFM_LAUNCH_CHECK(h, what);
  }
  // the status word, once, behind the last launch
  int64_t* status = (int64_t*)(h->pinned + SFM_PIN_MESH_CC);
  SFM_HIP(h, hipMemcpyAsync(status, counts + CC_STATUS, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  SFM_HIP(h, hipStreamSynchronize(h->stream));
  if (*status != 0) return sfm_fail(h, SFM_ERR_NUMERIC, what, "a walk towards a root ran out of its step budget");
  return SFM_OK;
}

extern "C" int sfm_mesh_clean_workspace_bytes(int64_t n_vertices, int64_t n_triangles, int64_t* bytes_host) {
  if (!bytes_host || clean_check_counts(n_vertices, n_triangles)) return SFM_ERR_ARG;
  *bytes_host = clean_layout(n_vertices, n_triangles).bytes;
  return SFM_OK;
}

extern "C" int sfm_mesh_clean_mark(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t n_components, const int32_t* vertex_component,
                                   const int32_t* triangle_component, const int32_t* comp_triangles, int64_t min_triangles, int64_t keep_largest,
                                   uint8_t* comp_keep, int64_t* counts, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_clean_mark";
  int bad = clean_check_mark(n_vertices, n_triangles, n_components, min_triangles, keep_largest, vertex_component, triangle_component, comp_triangles,
                             comp_keep, counts);
  const CleanLayout L = bad ? clean_layout(0, 0) : clean_layout(n_vertices, n_triangles);
  if (!bad) bad = clean_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, CLEAN_WHY[bad]);
  char* ws = (char*)workspace;
  uint64_t* d_blk = (uint64_t*)(ws + L.blk);
  int64_t* d_chunk = (int64_t*)(ws + L.chunk_base);
  const int64_t nb = clean_scan_blocks(n_vertices, n_triangles), n_chunks = scan_chunks(nb);
  const dim3 tb(CLEAN_BLOCK);
  hipLaunchKernelGGL(k_clean_select, dim3(1), tb, 0, h->stream, n_components, comp_triangles, min_triangles, keep_largest, comp_keep, counts,
                     (int64_t*)(ws + L.sel));
  SFM_LAUNCH_CHECK(h, what);
  if (nb > 0) {
    hipLaunchKernelGGL(k_clean_count, dim3((unsigned)nb), tb, 0, h->stream, n_vertices, n_triangles, n_components, vertex_component,
                       triangle_component, (const uint8_t*)comp_keep, d_blk);
    SFM_LAUNCH_CHECK(h, what);
    hipLaunchKernelGGL(k_clean_scan_chunks, dim3((unsigned)n_chunks), tb, 0, h->stream, d_blk, nb, d_chunk);
    SFM_LAUNCH_CHECK(h, what);
  }
  hipLaunchKernelGGL(k_clean_scan_top, dim3(1), tb, 0, h->stream, d_chunk, n_chunks, counts);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}

extern "C" int sfm_mesh_clean_emit(sfm_handle h, int64_t n_vertices, int64_t n_triangles, int64_t n_components, const int32_t* vertex_component,
                                   const int32_t* triangle_component, const uint8_t* comp_keep, const int32_t* triangles, const double* vertices,
                                   const float* normals, int64_t cap_vertices, int64_t cap_triangles, int32_t* vertex_map, int32_t* triangle_map,
                                   int32_t* triangles_out, double* vertices_out, float* normals_out, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_clean_emit";
  int bad = clean_check_emit_counts(n_vertices, n_triangles, n_components, cap_vertices, cap_triangles);
  const CleanLayout L = bad ? clean_layout(0, 0) : clean_layout(n_vertices, n_triangles);
  if (!bad) bad = clean_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, CLEAN_WHY[bad]);
  if (cap_vertices == 0 && cap_triangles == 0) return SFM_OK;
  bad = clean_check_emit_pointers(n_vertices, n_triangles, n_components, cap_vertices, cap_triangles, vertex_component, triangle_component, comp_keep,
                                  triangles, vertices, normals, vertex_map, triangle_map, triangles_out, vertices_out, normals_out);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, CLEAN_WHY[bad]);
  char* ws = (char*)workspace;
  int32_t* d_new = (int32_t*)(ws + L.new_index);
  const uint64_t* d_blk = (const uint64_t*)(ws + L.blk);
  const int64_t* d_chunk = (const int64_t*)(ws + L.chunk_base);
  const dim3 tb(CLEAN_BLOCK);
  if (n_vertices > 0) {
    hipLaunchKernelGGL(k_clean_emit_vertices, dim3((unsigned)clean_blocks(n_vertices)), tb, 0, h->stream, n_vertices, n_components, vertex_component,
                       comp_keep, d_blk, d_chunk, (const uint64_t*)vertices, (const uint32_t*)normals, cap_vertices, d_new, vertex_map,
                       (uint64_t*)vertices_out, (uint32_t*)normals_out);
    SFM_LAUNCH_CHECK(h, what);
  }
  if (n_triangles > 0 && cap_triangles > 0) {
    hipLaunchKernelGGL(k_clean_emit_triangles, dim3((unsigned)clean_blocks(n_triangles)), tb, 0, h->stream, n_vertices, n_triangles, n_components,
                       triangle_component, comp_keep, d_blk, d_chunk, triangles, (const int32_t*)d_new, cap_triangles, triangle_map, triangles_out);
    SFM_LAUNCH_CHECK(h, what);
  }
  return SFM_OK;
}

extern "C" int sfm_mesh_gather_rows(sfm_handle h, const void* src, int64_t row_bytes, const int32_t* map, int64_t n, void* dst) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_gather_rows";
  const int bad = clean_check_gather(row_bytes, n, src, map, dst);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, CLEAN_WHY[bad]);
  if (n == 0) return SFM_OK;
  switch (clean_gather_unit(row_bytes, (uintptr_t)src, (uintptr_t)dst)) {
    case 16: launch_gather<uint4>(h, src, row_bytes, map, n, dst); break;
    case 8: launch_gather<uint64_t>(h, src, row_bytes, map, n, dst); break;
    case 4: launch_gather<uint32_t>(h, src, row_bytes, map, n, dst); break;
    default: launch_gather<uint8_t>(h, src, row_bytes, map, n, dst); break;
  }
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}
