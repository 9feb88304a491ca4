// The edge table of a triangle mesh, its boundary loops and the filling of the small holes, for gfx950 (MI355X).
// include/sfm_amd.h states the rule; mesh_fill_rule.h holds the keys, the stack that splits a loop and the centroid fan,
// mesh_fill_plan.h the argument checks, the workspace layouts and the grids; the scans are those of block_scan.h /
// scan_plan.h.  Integers apart from the new vertices and their normals; every output byte is a function of the inputs.
//
// sfm_mesh_edges
//   k_edges_keys       one lane per half-edge: the key of its unordered pair (all ones when it is not live), the unsound triangles
//   rocprim            one stable radix sort of (key, half-edge), the only part that is not hand-written
//   k_edges_twin       one lane per sorted slot: the ends of its run of equal keys -> uses, twin and the four edge counts
//   k_edges_next       one lane per half-edge, only boundary ones walk: the rotation about b through the twins -> next
//   k_edges_loops      one lane per boundary half-edge: at most 64 steps along next -> its leader, the leaders of the block
//   k_edges_scan_*     the two-level scan of the leader counts -> counts[4]
//   k_edges_number     a leader takes its number, writes loop_leader / loop_edges and the number of every half-edge of its loop
// sfm_mesh_fill_mark
//   k_fill_init        sub_name = -1
//   k_fill_split       ONE wavefront per short loop: lane i holds the i-th half-edge, lane 0 runs the stack -> sub_name, open loops
//   k_fill_count       names of filled sub-loops and fill triangles per block, packed; k_fill_scan_* their scan -> counts
//   k_fill_rank        the rank of every name; k_fill_flags halfedge_fill = the rank of the half-edge's name
// sfm_mesh_fill_emit
//   k_fill_emit_vertices   one wavefront per short loop again; the lane that holds a filled sub-loop's name sums its vertex
//   k_fill_emit_triangles  one lane per half-edge: its fill triangle at its rank among the marked ones
// Nothing waits on another workgroup; the only atomics are integer adds into the counts.
#include "common.h"
#include "mesh_fill_rule.h"
#include "mesh_fill_plan.h"
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

// ------------------------------------------------------------------------------------------------ the table
__global__ __launch_bounds__(FILL_BLOCK) void k_edges_keys(const int32_t* __restrict__ triangles, int64_t n, int64_t n_vertices,
                                                           uint64_t* __restrict__ keys, int32_t* __restrict__ vals, int64_t* __restrict__ counts) {
  const int64_t h = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
  const bool in = h < n;
  bool unsound = false;
  if (in) {
    const int64_t t = h / 3;
    const int k = (int)(h - 3 * t);
    int32_t v[3];
    load_triangle(triangles, t, v);
    keys[h] = mesh_fill::edge_key(v[0], v[1], v[2], k, n_vertices);
    vals[h] = (int32_t)h;
    unsound = k == 0 && !mesh_clean::sound(v[0], v[1], v[2], n_vertices);
  }
  wave_count(&counts[EDGES_UNSOUND], unsound);
}

// the first slot of the run of `key` that holds slot s, and the slot behind its last: the neighbours first, a binary search
// only for a run of more than two in front of or behind s (an edge used more than twice)
__device__ __forceinline__ int64_t run_begin(const uint64_t* __restrict__ keys, int64_t s, uint64_t key) {
  if (s == 0 || keys[s - 1] != key) return s;
  if (s == 1 || keys[s - 2] != key) return s - 1;
  int64_t lo = 0, hi = s - 2;                              // keys[hi] == key; the first slot with keys[slot] >= key
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int64_t run_end(const uint64_t* __restrict__ keys, int64_t n, int64_t s, uint64_t key) {
  if (s + 1 >= n || keys[s + 1] != key) return s + 1;
  if (s + 2 >= n || keys[s + 2] != key) return s + 2;
  int64_t lo = s + 3, hi = n;                              // the first slot with keys[slot] > key
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(FILL_BLOCK) void k_edges_twin(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n,
                                                           const int32_t* __restrict__ triangles, int32_t* __restrict__ uses,
                                                           int32_t* __restrict__ twin, int64_t* __restrict__ counts) {
  const int64_t s = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
  bool first = false, boundary = false, inconsistent = false, nonmanifold = false;
  if (s < n) {
    const uint64_t key = keys[s];
    const int32_t h = vals[s];
    int32_t u = 0, tw = -1;
    if (key != MESH_FILL_DEAD_KEY) {
      const int64_t lo = run_begin(keys, s, key), hi = run_end(keys, n, s, key);
      u = (int32_t)(hi - lo);
      first = s == lo;
      if (u == 2) {
        const int32_t o = vals[lo + (hi - 1 - s)];
        // the same unordered pair with a != b: opposite iff the other one starts where this one ends
        int32_t v[3], w[3], a, b, oa, ob;
        load_triangle(triangles, h / 3, v);
        load_triangle(triangles, o / 3, w);
        mesh_fill::ends(v[0], v[1], v[2], h % 3, &a, &b);
        mesh_fill::ends(w[0], w[1], w[2], o % 3, &oa, &ob);
        if (oa == b) tw = o;
      }
      boundary = first && u == 1;
      inconsistent = first && u == 2 && tw < 0;
      nonmanifold = first && u > 2;
    }
    uses[h] = u;
    twin[h] = tw;
  }
  wave_count(&counts[EDGES_DISTINCT], first);
  wave_count(&counts[EDGES_BOUNDARY], boundary);
  wave_count(&counts[EDGES_INCONSISTENT], inconsistent);
  wave_count(&counts[EDGES_NONMANIFOLD], nonmanifold);
}

// A launch of its own: uses and twin are complete.  Only the boundary lanes walk; a rotation passes each triangle of the fan
// about b once, so the budget of n_triangles + 1 steps cannot run out on a valid twin table.
__global__ __launch_bounds__(FILL_BLOCK) void k_edges_next(int64_t n, int64_t n_triangles, const int32_t* __restrict__ uses,
                                                           const int32_t* __restrict__ twin, int32_t* __restrict__ next, int64_t* __restrict__ counts) {
  const int64_t h = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
  if (h >= n) return;
  int32_t out = -1;
  if (uses[h] == 1) {
    int g = mesh_fill::next_in_triangle((int)h);
    int64_t budget = edges_budget(n_triangles);
    for (;;) {
      const int32_t u = uses[g];
      if (u == 1) { out = g; break; }
      if (u == 0) break;                                   // not live
      const int32_t tw = twin[g];
      if (tw < 0) break;                                   // inconsistent or non-manifold
      g = mesh_fill::next_in_triangle(tw);
      if (--budget < 0) { counts[EDGES_STATUS] = 1; break; }
    }
  }
  next[h] = out;
}

__global__ __launch_bounds__(FILL_BLOCK) void k_edges_loops(int64_t n, const int32_t* __restrict__ uses, const int32_t* __restrict__ next,
                                                            int32_t* __restrict__ lead, uint32_t* __restrict__ blk, int64_t* __restrict__ counts) {
  __shared__ int s_wave[FILL_WAVES];
  const int64_t h = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
  const bool boundary = h < n && uses[h] == 1;
  int32_t leader = -1;
  if (boundary) {
    int g = (int)h, low = (int)h;
    for (int i = 0; i < MESH_FILL_WAVE; ++i) {
      g = next[g];
      if (g < 0) break;
      if (g == (int)h) { leader = low; break; }
      low = g < low ? g : low;
    }
  }
  if (h < n) lead[h] = leader;
  wave_count(&counts[EDGES_LONG], boundary && leader < 0);
  const int all = block_flag_count<FILL_BLOCK>(boundary && leader == (int)h, s_wave);
  if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)all;
}

__global__ __launch_bounds__(FILL_BLOCK) void k_edges_scan_chunks(uint32_t* __restrict__ blk, int64_t n_blocks, int64_t* __restrict__ chunk_sum) {
  __shared__ int64_t s_wave[FILL_WAVES];
  const int64_t total = scan_chunk_counts(blk, n_blocks, s_wave);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(FILL_BLOCK) void k_edges_scan_top(int64_t* __restrict__ chunk_sum, int64_t n_chunks, int64_t* __restrict__ counts) {
  __shared__ int64_t s_wave[FILL_WAVES];
  const int64_t all = scan_chunk_totals(chunk_sum, n_chunks, 1, s_wave);
  if (threadIdx.x == 0) counts[EDGES_LOOPS] = all;
}

// Every slot of halfedge_loop has one writer: the half-edge itself when it is on no short loop, its leader otherwise.
__global__ __launch_bounds__(FILL_BLOCK) void k_edges_number(int64_t n, const int32_t* __restrict__ next, const int32_t* __restrict__ lead,
                                                             const uint32_t* __restrict__ blk, const int64_t* __restrict__ chunk_base,
                                                             int32_t* __restrict__ loop, int32_t* __restrict__ loop_leader,
                                                             int32_t* __restrict__ loop_edges) {
  __shared__ int s_wave[FILL_WAVES];
  const int64_t h = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
  const int32_t leader = h < n ? lead[h] : -1;
  const bool leads = h < n && leader == (int32_t)h;
  const int rank = block_flag_rank<FILL_BLOCK>(leads, s_wave);
  if (h >= n) return;
  if (leader < 0) { loop[h] = -1; return; }
  if (!leads) return;
  const int64_t number = scan_base(chunk_base, 1, 0, blockIdx.x, (int64_t)blk[blockIdx.x]) + rank;
  int g = (int)h, edges = 0;
  for (int i = 0; i < MESH_FILL_WAVE; ++i) {
    loop[g] = (int32_t)number;
    ++edges;
    g = next[g];
    if (g == (int)h || g < 0) break;
  }
  loop_leader[number] = (int32_t)h;
  loop_edges[number] = edges;
}

// ------------------------------------------------------------------------------------------------ the holes
// What one wavefront holds of its loop in LDS: the ends and the number of the i-th half-edge, and what the stack makes of them.
struct LoopLds { int32_t a[MESH_FILL_WAVE], b[MESH_FILL_WAVE], h[MESH_FILL_WAVE], stack[MESH_FILL_WAVE], name[MESH_FILL_WAVE], len[MESH_FILL_WAVE], succ[MESH_FILL_WAVE]; int32_t ok; };

// The loop of this wavefront from its leader: every lane follows `next` in step (one address, at most 64 dependent loads),
// lane i keeps the i-th half-edge and loads its ends; lane 0 runs the stack of the rule.  Returns the edges of the loop, 0
// when `loop` is past the last one, -1 when the tables are not those of sfm_mesh_edges for these triangles: a leader or a
// successor outside the half-edges, a walk that does not close within 64 steps, a half-edge that is not live.  No table
// entry is an address before it is checked.  Two workgroup barriers: every wavefront of the workgroup must call.
__device__ __forceinline__ int load_loop(int64_t loop, int64_t n_loops, const int32_t* __restrict__ loop_leader, const int32_t* __restrict__ next,
                                         const int32_t* __restrict__ triangles, int64_t n, int64_t n_vertices, LoopLds* L, int32_t* mine) {
  const int lane = threadIdx.x & 63;
  int count = 0;
  bool closed = false;
  *mine = -1;
  if (loop < n_loops) {
    const int32_t leader = loop_leader[loop];
    if (leader >= 0 && leader < n) {
      int g = leader;
      for (int i = 0; i < MESH_FILL_WAVE; ++i) {
        if (lane == i) *mine = g;
        count = i + 1;
        const int32_t nx = next[g];
        if (nx == leader) { closed = true; break; }
        if (nx < 0 || nx >= n) break;
        g = nx;
      }
    }
  }
  bool dead = false;
  if (closed && lane < count) {
    int32_t v[3], a, b;
    load_triangle(triangles, *mine / 3, v);
    mesh_fill::ends(v[0], v[1], v[2], *mine % 3, &a, &b);
    dead = !mesh_clean::sound(v[0], v[1], v[2], n_vertices) || a == b;
    L->a[lane] = a; L->b[lane] = b; L->h[lane] = *mine;
  }
  closed = closed && __ballot(dead) == 0ull;
  __syncthreads();
  if (lane == 0) L->ok = closed ? mesh_fill::split(count, L->a, L->b, L->h, L->stack, L->name, L->len, L->succ) : 0;
  __syncthreads();
  if (loop >= n_loops) return 0;
  return L->ok ? count : -1;
}

__global__ __launch_bounds__(FILL_BLOCK) void k_fill_init(int64_t n, int32_t* __restrict__ sub_name) {
  const int64_t h = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
  if (h < n) sub_name[h] = -1;
}

__global__ __launch_bounds__(FILL_BLOCK) void k_fill_split(int64_t n_vertices, int64_t n, const int32_t* __restrict__ triangles,
                                                           const int32_t* __restrict__ next, int64_t n_loops, const int32_t* __restrict__ loop_leader,
                                                           int max_edges, int32_t* __restrict__ sub_name, int64_t* __restrict__ counts) {
  __shared__ LoopLds s_loop[FILL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  LoopLds* L = &s_loop[wave];
  int32_t mine;
  const int count = load_loop((int64_t)blockIdx.x * FILL_WAVES + wave, n_loops, loop_leader, next, triangles, n, n_vertices, L, &mine);
  if (count < 0 && lane == 0) counts[FILL_STATUS] = 1;
  bool open = false;
  if (lane < count) {
    const bool fills = mesh_fill::filled(L->len[lane], max_edges);
    sub_name[mine] = fills ? L->name[lane] : -1;
    open = !fills && L->name[lane] == mine;
  }
  wave_count(&counts[FILL_OPEN], open);
}

__global__ __launch_bounds__(FILL_BLOCK) void k_fill_count(int64_t n, const int32_t* __restrict__ sub_name, uint64_t* __restrict__ blk) {
  __shared__ int s_n[FILL_WAVES], s_t[FILL_WAVES];
  const int64_t h = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
  const int32_t name = h < n ? sub_name[h] : -1;
  const int names = block_flag_count<FILL_BLOCK>(name >= 0 && name == (int32_t)h, s_n);
  const int tris = block_flag_count<FILL_BLOCK>(name >= 0, s_t);
  if (threadIdx.x == 0) blk[blockIdx.x] = fill_count_pack((uint32_t)names, (uint32_t)tris);
}

__global__ __launch_bounds__(FILL_BLOCK) void k_fill_scan_chunks(uint64_t* __restrict__ blk, int64_t n_blocks, int64_t* __restrict__ chunk_sum) {
  __shared__ int64_t s_wave[FILL_WAVES];
  const int64_t total = scan_chunk_counts(blk, n_blocks, s_wave);   // neither half leaves its 32 bits within a chunk
  if (threadIdx.x == 0) {
    chunk_sum[2 * (int64_t)blockIdx.x] = total & 0xFFFFFFFFll;
    chunk_sum[2 * (int64_t)blockIdx.x + 1] = total >> 32;
  }
}

__global__ __launch_bounds__(FILL_BLOCK) void k_fill_scan_top(int64_t* __restrict__ chunk_sum, int64_t n_chunks, int64_t* __restrict__ counts) {
  __shared__ int64_t s_wave[FILL_WAVES];
  for (int half = 0; half < 2; ++half) {
    const int64_t all = scan_chunk_totals(chunk_sum + half, n_chunks, 2, s_wave);
    if (threadIdx.x == 0) counts[FILL_FILLED + half] = all;
  }
}

__global__ __launch_bounds__(FILL_BLOCK) void k_fill_rank(int64_t n, const int32_t* __restrict__ sub_name, const uint64_t* __restrict__ blk,
                                                          const int64_t* __restrict__ chunk_base, int32_t* __restrict__ rank) {
  __shared__ int s_wave[FILL_WAVES];
  const int64_t h = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
  const bool names = h < n && sub_name[h] == (int32_t)h;
  const int r = block_flag_rank<FILL_BLOCK>(names, s_wave);
  if (names) rank[h] = (int32_t)(fill_name_base(chunk_base, blk, blockIdx.x) + r);
}

// a launch of its own: the rank of every name is in place
__global__ __launch_bounds__(FILL_BLOCK) void k_fill_flags(int64_t n, const int32_t* __restrict__ sub_name, const int32_t* __restrict__ rank,
                                                           int32_t* __restrict__ halfedge_fill) {
  const int64_t h = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
  if (h >= n) return;
  const int32_t name = sub_name[h];
  halfedge_fill[h] = name >= 0 ? rank[name] : -1;
}

// ------------------------------------------------------------------------------------------------ emit
__global__ __launch_bounds__(FILL_BLOCK) void k_fill_emit_vertices(int64_t n_vertices, int64_t n, const int32_t* __restrict__ triangles,
                                                                   const int32_t* __restrict__ next, int64_t n_loops,
                                                                   const int32_t* __restrict__ loop_leader, const int32_t* __restrict__ halfedge_fill,
                                                                   const double* __restrict__ vertices, int64_t cap_fill,
                                                                   double* __restrict__ fill_vertices, float* __restrict__ fill_normals,
                                                                   int32_t* __restrict__ fill_name) {
  __shared__ LoopLds s_loop[FILL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  LoopLds* L = &s_loop[wave];
  int32_t mine;
  const int count = load_loop((int64_t)blockIdx.x * FILL_WAVES + wave, n_loops, loop_leader, next, triangles, n, n_vertices, L, &mine);
  if (lane >= count || L->name[lane] != mine) return;
  // the lane of a sub-loop's name; a fill flag that is not the mark call's, or a capacity below the truth, writes nothing
  // outside the outputs
  const int64_t r = halfedge_fill[mine];
  if (r < 0 || r >= cap_fill) return;
  double c[3];
  float normal[3];
  mesh_fill::patch(L->len[lane], lane, L->succ, L->a, vertices, c, normal);
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    fill_vertices[3 * r + x] = c[x];
    fill_normals[3 * r + x] = normal[x];
  }
  fill_name[r] = mine;
}

__global__ __launch_bounds__(FILL_BLOCK) void k_fill_emit_triangles(int64_t n_vertices, int64_t n, const int32_t* __restrict__ triangles,
                                                                    const int32_t* __restrict__ halfedge_fill, const uint64_t* __restrict__ blk,
                                                                    const int64_t* __restrict__ chunk_base, int64_t cap_fill, int64_t cap_triangles,
                                                                    int32_t* __restrict__ fill_triangles, int32_t* __restrict__ fill_triangle_halfedge) {
  __shared__ int s_wave[FILL_WAVES];
  const int64_t h = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
  const int64_t r = h < n ? (int64_t)halfedge_fill[h] : -1;
  const bool marked = r >= 0;
  const int rank = block_flag_rank<FILL_BLOCK>(marked, s_wave);
  if (!marked) return;
  const int64_t slot = fill_triangle_base(chunk_base, blk, blockIdx.x) + rank;
  if (slot < 0 || slot >= cap_triangles) return;
  const int64_t t = h / 3;
  int32_t v[3], a, b;
  load_triangle(triangles, t, v);
  mesh_fill::ends(v[0], v[1], v[2], (int)(h - 3 * t), &a, &b);
  // always sound and within the capacity with the flags of sfm_mesh_fill_mark
  const bool ok = mesh_clean::sound(v[0], v[1], v[2], n_vertices) && r < cap_fill && n_vertices + r <= 0x7FFFFFFFll;
  fill_triangles[3 * slot] = ok ? b : -1;
  fill_triangles[3 * slot + 1] = ok ? a : -1;
  fill_triangles[3 * slot + 2] = ok ? (int32_t)(n_vertices + r) : -1;
  fill_triangle_halfedge[slot] = (int32_t)h;
}

// the bits of the key that the sort looks at: those of (min << 32) | max with max < n_vertices.  The all-ones key of a
// half-edge that is not live stays above every live one under this cut, since min <= n_vertices - 2 < 2^bits - 1.
int sort_end_bit(int64_t n_vertices) {
  int bits = 1;
  while (bits < 32 && (1ll << bits) <= n_vertices) ++bits;
  return 32 + bits;
}

hipError_t sort_pairs(void* tmp, size_t& tmp_bytes, uint64_t* keys_in, uint64_t* keys_out, int32_t* vals_in, int32_t* vals_out, int64_t n,
                      int64_t n_vertices, hipStream_t stream) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, (unsigned)sort_end_bit(n_vertices), stream);
}

}  // namespace

extern "C" int sfm_mesh_edges_workspace_bytes(sfm_handle h, int64_t n_triangles, int64_t* bytes_host) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_edges_workspace_bytes";
  if (!bytes_host) return sfm_fail(h, SFM_ERR_ARG, what, FILL_WHY[4]);
  if (fill_check_counts(0, n_triangles)) return sfm_fail(h, SFM_ERR_ARG, what, FILL_WHY[1]);
  size_t sort_bytes = 0;
  // the widest cut of the key: the storage does not depend on the bits, and is measured for the most it could be
  if (n_triangles > 0)
    SFM_HIP(h, sort_pairs(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, 3 * n_triangles, FILL_MAX_VERTICES, h->stream));
  *bytes_host = edges_layout(n_triangles, (int64_t)sort_bytes).bytes;
  return SFM_OK;
}

extern "C" int sfm_mesh_edges(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const int32_t* triangles, int32_t* halfedge_uses,
                              int32_t* halfedge_twin, int32_t* halfedge_next, int32_t* halfedge_loop, int32_t* loop_leader, int32_t* loop_edges,
                              int64_t* counts, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_edges";
  int bad = edges_check(n_vertices, n_triangles, triangles, halfedge_uses, halfedge_twin, halfedge_next, halfedge_loop, loop_leader, loop_edges, counts);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, FILL_WHY[bad]);
  const int64_t n = 3 * n_triangles;
  // the layout is that of sfm_mesh_edges_workspace_bytes, measured for the widest cut; the sort is told what its own cut needs
  size_t sort_room = 0, sort_bytes = 0;
  if (n > 0) {
    SFM_HIP(h, sort_pairs(nullptr, sort_room, nullptr, nullptr, nullptr, nullptr, n, FILL_MAX_VERTICES, h->stream));
    SFM_HIP(h, sort_pairs(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, n_vertices, h->stream));
    if (sort_bytes > sort_room) sort_room = sort_bytes;
  }
  const EdgesLayout L = edges_layout(n_triangles, (int64_t)sort_room);
  bad = fill_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, FILL_WHY[bad]);
  SFM_HIP(h, hipMemsetAsync(counts, 0, EDGES_COUNTS * sizeof(int64_t), h->stream));
  if (n == 0) return SFM_OK;
  char* ws = (char*)workspace;
  uint64_t* d_keys_in = (uint64_t*)(ws + L.keys_in);
  uint64_t* d_keys = (uint64_t*)(ws + L.keys_out);
  int32_t* d_vals_in = (int32_t*)(ws + L.vals_in);
  int32_t* d_vals = (int32_t*)(ws + L.vals_out);
  int32_t* d_lead = (int32_t*)(ws + L.lead);
  uint32_t* d_blk = (uint32_t*)(ws + L.blk);
  int64_t* d_chunk = (int64_t*)(ws + L.chunk_base);
  const int64_t nb = fill_blocks(n), n_chunks = scan_chunks(nb);
  const dim3 tb(FILL_BLOCK), grid((unsigned)nb);
  hipLaunchKernelGGL(k_edges_keys, grid, tb, 0, h->stream, triangles, n, n_vertices, d_keys_in, d_vals_in, counts);
  SFM_LAUNCH_CHECK(h, what);
  SFM_HIP(h, sort_pairs(ws + L.sort, sort_bytes, d_keys_in, d_keys, d_vals_in, d_vals, n, n_vertices, h->stream));
  hipLaunchKernelGGL(k_edges_twin, grid, tb, 0, h->stream, (const uint64_t*)d_keys, (const int32_t*)d_vals, n, triangles, halfedge_uses,
                     halfedge_twin, counts);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_edges_next, grid, tb, 0, h->stream, n, n_triangles, (const int32_t*)halfedge_uses, (const int32_t*)halfedge_twin,
                     halfedge_next, counts);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_edges_loops, grid, tb, 0, h->stream, n, (const int32_t*)halfedge_uses, (const int32_t*)halfedge_next, d_lead, d_blk, counts);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_edges_scan_chunks, dim3((unsigned)n_chunks), tb, 0, h->stream, d_blk, nb, d_chunk);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_edges_scan_top, dim3(1), tb, 0, h->stream, d_chunk, n_chunks, counts);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_edges_number, grid, tb, 0, h->stream, n, (const int32_t*)halfedge_next, (const int32_t*)d_lead, (const uint32_t*)d_blk,
                     (const int64_t*)d_chunk, halfedge_loop, loop_leader, loop_edges);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}

extern "C" int sfm_mesh_fill_workspace_bytes(int64_t n_triangles, int64_t* bytes_host) {
  if (!bytes_host || fill_check_counts(0, n_triangles)) return SFM_ERR_ARG;
  *bytes_host = fill_layout(n_triangles).bytes;
  return SFM_OK;
}

extern "C" int sfm_mesh_fill_mark(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const int32_t* triangles, const int32_t* halfedge_next,
                                  int64_t n_loops, const int32_t* loop_leader, int64_t max_edges, int32_t* halfedge_fill, int64_t* counts,
                                  void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_fill_mark";
  int bad = fill_check_mark(n_vertices, n_triangles, n_loops, max_edges, triangles, halfedge_next, loop_leader, halfedge_fill, counts);
  const FillLayout L = fill_layout(bad ? 0 : n_triangles);
  if (!bad) bad = fill_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, FILL_WHY[bad]);
  SFM_HIP(h, hipMemsetAsync(counts, 0, FILL_COUNTS * sizeof(int64_t), h->stream));
  const int64_t n = 3 * n_triangles;
  if (n == 0) return SFM_OK;
  char* ws = (char*)workspace;
  int32_t* d_name = (int32_t*)(ws + L.sub_name);
  int32_t* d_rank = (int32_t*)(ws + L.rank);
  uint64_t* d_blk = (uint64_t*)(ws + L.blk);
  int64_t* d_chunk = (int64_t*)(ws + L.chunk_base);
  const int64_t nb = fill_blocks(n), n_chunks = scan_chunks(nb);
  const dim3 tb(FILL_BLOCK), grid((unsigned)nb);
  hipLaunchKernelGGL(k_fill_init, grid, tb, 0, h->stream, n, d_name);
  SFM_LAUNCH_CHECK(h, what);
  if (n_loops > 0) {
    hipLaunchKernelGGL(k_fill_split, dim3((unsigned)fill_loop_blocks(n_loops)), tb, 0, h->stream, n_vertices, n, triangles, halfedge_next, n_loops,
                       loop_leader, (int)max_edges, d_name, counts);
    SFM_LAUNCH_CHECK(h, what);
  }
  hipLaunchKernelGGL(k_fill_count, grid, tb, 0, h->stream, n, (const int32_t*)d_name, d_blk);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_fill_scan_chunks, dim3((unsigned)n_chunks), tb, 0, h->stream, d_blk, nb, d_chunk);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_fill_scan_top, dim3(1), tb, 0, h->stream, d_chunk, n_chunks, counts);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_fill_rank, grid, tb, 0, h->stream, n, (const int32_t*)d_name, (const uint64_t*)d_blk, (const int64_t*)d_chunk, d_rank);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_fill_flags, grid, tb, 0, h->stream, n, (const int32_t*)d_name, (const int32_t*)d_rank, halfedge_fill);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}

extern "C" int sfm_mesh_fill_emit(sfm_handle h, int64_t n_vertices, int64_t n_triangles, const int32_t* triangles, const int32_t* halfedge_next,
                                  int64_t n_loops, const int32_t* loop_leader, const int32_t* halfedge_fill, const double* vertices,
                                  int64_t cap_fill, int64_t cap_triangles, double* fill_vertices, float* fill_normals, int32_t* fill_name,
                                  int32_t* fill_triangles, int32_t* fill_triangle_halfedge, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_fill_emit";
  int bad = fill_check_emit_counts(n_vertices, n_triangles, n_loops, cap_fill, cap_triangles);
  const FillLayout L = fill_layout(bad ? 0 : n_triangles);
  if (!bad) bad = fill_check_workspace(workspace, workspace_bytes, L.bytes);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, FILL_WHY[bad]);
  if (cap_fill == 0 && cap_triangles == 0) return SFM_OK;
  bad = fill_check_emit_pointers(n_vertices, n_triangles, n_loops, cap_fill, cap_triangles, triangles, halfedge_next, loop_leader, halfedge_fill,
                                 vertices, fill_vertices, fill_normals, fill_name, fill_triangles, fill_triangle_halfedge);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, FILL_WHY[bad]);
  const int64_t n = 3 * n_triangles;
  if (n == 0) return SFM_OK;
  char* ws = (char*)workspace;
  const uint64_t* d_blk = (const uint64_t*)(ws + L.blk);
  const int64_t* d_chunk = (const int64_t*)(ws + L.chunk_base);
  const dim3 tb(FILL_BLOCK);
  if (n_loops > 0 && cap_fill > 0) {
    hipLaunchKernelGGL(k_fill_emit_vertices, dim3((unsigned)fill_loop_blocks(n_loops)), tb, 0, h->stream, n_vertices, n, triangles, halfedge_next,
                       n_loops, loop_leader, halfedge_fill, vertices, cap_fill, fill_vertices, fill_normals, fill_name);
    SFM_LAUNCH_CHECK(h, what);
  }
  if (cap_triangles > 0) {
    hipLaunchKernelGGL(k_fill_emit_triangles, dim3((unsigned)fill_blocks(n)), tb, 0, h->stream, n_vertices, n, triangles, halfedge_fill, d_blk,
                       d_chunk, cap_fill, cap_triangles, fill_triangles, fill_triangle_halfedge);
    SFM_LAUNCH_CHECK(h, what);
  }
  return SFM_OK;
}
