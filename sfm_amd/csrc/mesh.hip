// A triangle mesh of the zero level of a TSDF volume by marching tetrahedra over the Kuhn split, for gfx950 (MI355X):
// the flags of every node, the vertex mask of every node and the triangle count of every cell with their ranks inside
// the block, a two-level exclusive scan of the block counts, and the two emitting kernels.  include/sfm_amd.h states the
// rule; mesh_rule.h holds the case table and the floating point (float64, no FMA contraction), mesh_plan.h the node
// record, the packed counts and the workspace layout; the scans are those of block_scan.h / scan_plan.h.
//
// Every kernel is one thread per node, x fastest, MESH_BLOCK consecutive nodes per workgroup; the thread of a node also
// handles the cell whose lowest node it is.  The rule is a pure function of the field: no visit order, no global atomics,
// nothing waits on another workgroup.  A triangle finds a vertex as the first slot of the owning node - the base of that
// node's block plus the node's rank in it - plus the set bits of the node's mask below the direction: vertex numbers are
// never stored.
#include "common.h"
#include "tsdf_rule.h"
#include "mesh_rule.h"
#include "mesh_plan.h"
#include "block_scan.h"

#pragma clang fp contract(off)

namespace {

constexpr int MESH_WAVES = MESH_BLOCK / 64;

struct Grid { int nx, ny, nz; };
struct NodeOfThread { int64_t n; int i, j, k; bool in; };

__device__ __forceinline__ NodeOfThread node_of_thread(Grid g) {
  NodeOfThread q;
  q.n = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  q.in = q.n < mesh_nodes(g.nx, g.ny, g.nz);
  q.i = q.in ? (int)(q.n % g.nx) : 0;
  q.j = q.in ? (int)((q.n / g.nx) % g.ny) : 0;
  q.k = q.in ? (int)(q.n / ((int64_t)g.nx * g.ny)) : 0;
  return q;
}

// the flags of node (i, j, k); 0 - not known, not inside - outside the grid
__device__ __forceinline__ int flags_at(const uint8_t* __restrict__ flags, Grid g, int i, int j, int k) {
  if ((unsigned)i >= (unsigned)g.nx || (unsigned)j >= (unsigned)g.ny || (unsigned)k >= (unsigned)g.nz) return 0;
  return flags[mesh_node(i, j, k, g.nx, g.ny)];
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_classify(const float* __restrict__ tsdf, const uint16_t* __restrict__ weight,
                                                              int64_t n_nodes, int min_weight, uint8_t* __restrict__ flags) {
  const int64_t n = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (n < n_nodes) flags[n] = (uint8_t)mesh::node_flags(tsdf[n], (int)weight[n], min_weight);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_mark(const uint8_t* __restrict__ flags, Grid g, uint32_t* __restrict__ record,
                                                          uint64_t* __restrict__ blk) {
  __shared__ int s_wave[MESH_WAVES];
  const NodeOfThread q = node_of_thread(g);
  int mask = 0, triangles = 0, active = 0;
  if (q.in) {
    // the known bits of the 27 nodes around this one, bit (dx + 1) + 3 (dy + 1) + 9 (dz + 1), and the inside bits of the
    // 8 corners of this node's cell
    uint32_t known = 0;
    int inside8 = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int f = flags_at(flags, g, q.i + dx, q.j + dy, q.k + dz);
          known |= (uint32_t)(f & mesh::KNOWN) << ((dx + 1) + 3 * (dy + 1) + 9 * (dz + 1));
          if (dx >= 0 && dy >= 0 && dz >= 0) inside8 |= ((f & mesh::INSIDE) ? 1 : 0) << (dx + 2 * dy + 4 * dz);
        }
    // bit c: the cell of which this node is corner c is active (a cell that leaves the grid has an unknown corner)
    int active8 = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      uint32_t need = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        need |= 1u << (((e & 1) - (c & 1) + 1) + 3 * (((e >> 1) & 1) - ((c >> 1) & 1) + 1) + 9 * (((e >> 2) & 1) - ((c >> 2) & 1) + 1));
      active8 |= ((known & need) == need ? 1 : 0) << c;
    }
#pragma unroll
    for (int d = 0; d < MESH_DIRS; ++d) {
      const int differ = (inside8 ^ (inside8 >> MESH_DIR_CORNER(d))) & 1;
      mask |= (differ && (active8 & mesh::edge_cells(d))) ? (1 << d) : 0;
    }
    active = active8 & 1;
    triangles = active ? mesh::cell_triangles(inside8) : 0;
  }
  // both counts of a block stay below 2^16: one scan of the packed pair
  const int v = __popc((unsigned)mask) | (triangles << 16);
  int all;
  const int rank = block_exclusive_scan<MESH_BLOCK, int>(v, s_wave, &all);
  if (q.in) record[q.n] = mesh_record(mask, rank & 0xFFFF, rank >> 16, active);
  if (threadIdx.x == 0) blk[blockIdx.x] = mesh_count_pack((uint32_t)(all & 0xFFFF), (uint32_t)(all >> 16));
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_scan_chunks(uint64_t* __restrict__ blk, int64_t n_blocks, int64_t* __restrict__ chunk_sum) {
  __shared__ int64_t s_wave[MESH_WAVES];
  const int64_t total = scan_chunk_counts(blk, n_blocks, s_wave);   // neither half leaves its 32 bits within a chunk
  if (threadIdx.x == 0) {
    chunk_sum[2 * (int64_t)blockIdx.x] = total & 0xFFFFFFFFll;
    chunk_sum[2 * (int64_t)blockIdx.x + 1] = total >> 32;
  }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_scan_top(int64_t* __restrict__ chunk_sum, int64_t n_chunks, int64_t* __restrict__ counts) {
  __shared__ int64_t s_wave[MESH_WAVES];
  for (int half = 0; half < 2; ++half) {
    const int64_t all = scan_chunk_totals(chunk_sum + half, n_chunks, 2, s_wave);
    if (threadIdx.x == 0) counts[half] = all;
  }
}

// the gradient of the field at the known node (i, j, k)
__device__ __forceinline__ void gradient_at(const float* __restrict__ tsdf, const uint8_t* __restrict__ flags, Grid g, int i, int j, int k,
                                            double* out) {
  const double f0 = (double)tsdf[mesh_node(i, j, k, g.nx, g.ny)];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int di = a == 0, dj = a == 1, dk = a == 2;
    const int kp = flags_at(flags, g, i + di, j + dj, k + dk) & mesh::KNOWN;
    const int km = flags_at(flags, g, i - di, j - dj, k - dk) & mesh::KNOWN;
    const double fp = kp ? (double)tsdf[mesh_node(i + di, j + dj, k + dk, g.nx, g.ny)] : 0.0;
    const double fm = km ? (double)tsdf[mesh_node(i - di, j - dj, k - dk, g.nx, g.ny)] : 0.0;
    out[a] = mesh::gradient(f0, fp, fm, kp, km);
  }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_emit_vertices(const float* __restrict__ tsdf, const uint8_t* __restrict__ flags,
                                                                   const uint32_t* __restrict__ record, const uint64_t* __restrict__ blk,
                                                                   const int64_t* __restrict__ chunk_base, Grid g, double o0, double o1,
                                                                   double o2, double voxel, int64_t n_vertices,
                                                                   double* __restrict__ vertices, float* __restrict__ normals) {
  const NodeOfThread q = node_of_thread(g);
  if (!q.in) return;
  const int mask = mesh_record_mask(record[q.n]);
  if (!mask) return;
  int64_t slot = mesh_vertex_base(chunk_base, blk, blockIdx.x) + mesh_record_vrank(record[q.n]);
  const double fa = (double)tsdf[q.n];
  const double XA[3] = {tsdf::node_coord(o0, voxel, q.i), tsdf::node_coord(o1, voxel, q.j), tsdf::node_coord(o2, voxel, q.k)};
  double gA[3];
  gradient_at(tsdf, flags, g, q.i, q.j, q.k, gA);
#pragma unroll
  for (int d = 0; d < MESH_DIRS; ++d) {
    if (!((mask >> d) & 1)) continue;
    const int c = MESH_DIR_CORNER(d);
    const int ib = q.i + (c & 1), jb = q.j + ((c >> 1) & 1), kb = q.k + ((c >> 2) & 1);
    // a workspace that is not the mark call's, or an n_vertices below the truth, writes nothing outside the outputs and
    // reads nothing outside the grid
    if (ib >= g.nx || jb >= g.ny || kb >= g.nz || slot < 0 || slot >= n_vertices) { ++slot; continue; }
    const double t = mesh::cut(fa, (double)tsdf[mesh_node(ib, jb, kb, g.nx, g.ny)]);
    const double XB[3] = {tsdf::node_coord(o0, voxel, ib), tsdf::node_coord(o1, voxel, jb), tsdf::node_coord(o2, voxel, kb)};
    double gB[3];
    gradient_at(tsdf, flags, g, ib, jb, kb, gB);
    float nrm[3];
    mesh::normal(gA, gB, t, nrm);
#pragma unroll
    for (int a = 0; a < 3; ++a) { vertices[slot * 3 + a] = mesh::lerp(XA[a], XB[a], t); normals[slot * 3 + a] = nrm[a]; }
    ++slot;
  }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_emit_triangles(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ record,
                                                                    const uint64_t* __restrict__ blk, const int64_t* __restrict__ chunk_base,
                                                                    Grid g, int64_t n_triangles, int32_t* __restrict__ triangles) {
  const NodeOfThread q = node_of_thread(g);
  if (!q.in) return;
  const uint32_t rec = record[q.n];
  // the last test is always false with the record of the mark call
  if (!mesh_record_active(rec) || q.i >= g.nx - 1 || q.j >= g.ny - 1 || q.k >= g.nz - 1) return;
  int64_t slot = mesh_triangle_base(chunk_base, blk, blockIdx.x) + mesh_record_trank(rec);
  int inside8 = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    inside8 |= ((flags[mesh_node(q.i + (c & 1), q.j + ((c >> 1) & 1), q.k + ((c >> 2) & 1), g.nx, g.ny)] & mesh::INSIDE) ? 1 : 0) << c;
  for (int T = 0; T < 6; ++T) {
    const uint8_t* row = MESH_CASE[T][mesh::tet_case(T, inside8)];
    for (int t = 0; t < row[0]; ++t, ++slot) {
      if (slot < 0 || slot >= n_triangles) continue;
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const int code = row[1 + 3 * t + v], c = code >> 3, d = code & 7;
        const int64_t owner = mesh_node(q.i + (c & 1), q.j + ((c >> 1) & 1), q.k + ((c >> 2) & 1), g.nx, g.ny);
        const uint32_t ro = record[owner];
        const int64_t id = mesh_vertex_base(chunk_base, blk, owner / MESH_BLOCK) + mesh_record_vrank(ro) +
                           __popc((unsigned)mesh_record_mask(ro) & ((1u << d) - 1u));
        triangles[slot * 3 + v] = (int32_t)id;
      }
    }
  }
}

}  // namespace

extern "C" int sfm_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t* bytes_host) {
  if (!bytes_host || mesh_check_grid(nx, ny, nz)) return SFM_ERR_ARG;
  *bytes_host = mesh_layout(mesh_nodes(nx, ny, nz)).bytes;
  return SFM_OK;
}

extern "C" int sfm_mesh_mark(sfm_handle h, const float* tsdf, const uint16_t* weight, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                             int64_t* counts, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_mark";
  int bad = mesh_check_grid(nx, ny, nz);
  if (!bad && min_weight < 0) bad = 11;
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_WHY[bad]);
  const int64_t n_nodes = mesh_nodes(nx, ny, nz), nb = mesh_blocks(n_nodes), n_chunks = scan_chunks(nb);
  const MeshLayout L = mesh_layout(n_nodes);
  if (!workspace || workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_ARG, what, "workspace missing or too small");
  if (!tsdf || !weight || !counts) return sfm_fail(h, SFM_ERR_ARG, what, "null pointer");
  char* ws = (char*)workspace;
  uint8_t* d_flags = (uint8_t*)(ws + L.flags);
  uint64_t* d_blk = (uint64_t*)(ws + L.blk);
  int64_t* d_chunk = (int64_t*)(ws + L.chunk_base);
  const Grid g{nx, ny, nz};
  hipLaunchKernelGGL(k_mesh_classify, dim3((unsigned)nb), dim3(MESH_BLOCK), 0, h->stream, tsdf, weight, n_nodes, min_weight, d_flags);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_mesh_mark, dim3((unsigned)nb), dim3(MESH_BLOCK), 0, h->stream, (const uint8_t*)d_flags, g, (uint32_t*)(ws + L.record), d_blk);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_mesh_scan_chunks, dim3((unsigned)n_chunks), dim3(MESH_BLOCK), 0, h->stream, d_blk, nb, d_chunk);
  SFM_LAUNCH_CHECK(h, what);
  hipLaunchKernelGGL(k_mesh_scan_top, dim3(1), dim3(MESH_BLOCK), 0, h->stream, d_chunk, n_chunks, counts);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}

extern "C" int sfm_mesh_emit(sfm_handle h, const float* tsdf, int32_t nx, int32_t ny, int32_t nz, const double* origin, double voxel,
                             int64_t n_vertices, int64_t n_triangles, double* vertices, float* normals, int32_t* triangles, void* workspace,
                             int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const char* what = "sfm_mesh_emit";
  int bad = mesh_check_grid(nx, ny, nz);
  if (!bad) bad = mesh_check_frame(origin, voxel);
  if (bad) return sfm_fail(h, SFM_ERR_ARG, what, MESH_WHY[bad]);
  if (n_vertices < 0 || n_triangles < 0 || n_vertices > 0x7FFFFFFFLL || n_triangles > 0x7FFFFFFFLL)
    return sfm_fail(h, SFM_ERR_ARG, what, "n_vertices and n_triangles must be 0 .. 2^31 - 1");
  const int64_t n_nodes = mesh_nodes(nx, ny, nz), nb = mesh_blocks(n_nodes);
  const MeshLayout L = mesh_layout(n_nodes);
  if (!workspace || workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_ARG, what, "workspace missing or too small");
  if (n_vertices == 0 && n_triangles == 0) return SFM_OK;
  if (!tsdf || (n_vertices > 0 && (!vertices || !normals)) || (n_triangles > 0 && !triangles)) return sfm_fail(h, SFM_ERR_ARG, what, "null pointer");
  char* ws = (char*)workspace;
  const uint8_t* d_flags = (const uint8_t*)(ws + L.flags);
  const uint32_t* d_record = (const uint32_t*)(ws + L.record);
  const uint64_t* d_blk = (const uint64_t*)(ws + L.blk);
  const int64_t* d_chunk = (const int64_t*)(ws + L.chunk_base);
  const Grid g{nx, ny, nz};
  if (n_vertices > 0) {
    hipLaunchKernelGGL(k_mesh_emit_vertices, dim3((unsigned)nb), dim3(MESH_BLOCK), 0, h->stream, tsdf, d_flags, d_record, d_blk, d_chunk, g,
                       origin[0], origin[1], origin[2], voxel, n_vertices, vertices, normals);
    SFM_LAUNCH_CHECK(h, what);
  }
  if (n_triangles > 0) {
    hipLaunchKernelGGL(k_mesh_emit_triangles, dim3((unsigned)nb), dim3(MESH_BLOCK), 0, h->stream, d_flags, d_record, d_blk, d_chunk, g,
                       n_triangles, triangles);
    SFM_LAUNCH_CHECK(h, what);
  }
  return SFM_OK;
}
