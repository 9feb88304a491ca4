// Multi-view feature tracks from the pairwise matches of a data set (gfx950 only): the join between the pair loop and the
// reconstruction.  A node is one keypoint of one image (id = kp_ptr[image] + keypoint), a match is an edge, a track is a
// connected component with at least min_len nodes; a component that holds two keypoints of one image is conflicting and
// is dropped (as OpenMVG's track filter does) or kept and flagged.  The result is in CSR form and has ONE byte pattern:
//   tracks are numbered by their smallest node id, the observations of a track ascend by node id,
// so nothing depends on the order of the edges, of the pairs or of the lanes.  Integers only: no float atomics.
//
//   k_tracks_init      parent[v] = v, the counters to zero
//   k_tracks_hook      one lane per edge: union by "the larger root goes under the smaller id" (atomicCAS on a root only)
//   k_tracks_flatten   label[v] = root of v, size[root] += 1 (integer atomicAdd)
//   scan (mode 0)      roots with size >= min_len get a candidate number and an offset into `members` (multi-block scan)
//   k_tracks_claim     every node of a candidate takes a slot of it (any order); the others get their node_track code
//   k_tracks_sort_*    the slots of each candidate ascend afterwards: one lane per short candidate, a workgroup per long one
//   k_tracks_conflict  equal images on adjacent sorted members mark the candidate
//   scan (mode 1)      kept candidates get their track number and their observation offset
//   k_tracks_emit      obs_image / obs_kp / node_track
// Nothing is read back between the launches; the status word counts[4] is read once behind the last one.
#include "common.h"
#include "tracks_plan.h"
#include "block_scan.h"

namespace {

// largest s in [0, n) with ptr[s] <= i (skips empty ranges); the caller checks i against ptr[s + 1]
__device__ __forceinline__ int range_of(const int64_t* __restrict__ ptr, int n, int64_t i) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void add64(int64_t* p, int64_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// The 8 XCDs have private L2s and every CU its own L1: a plain load of `parent` may return a value another workgroup
// has replaced since.  Inside the hook kernel `parent` is only read with agent-scope atomic loads (and by the CAS itself).
__device__ __forceinline__ int parent_of(const int* parent, int v) {
  return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_tracks_init(int n_nodes, int* __restrict__ parent, int* __restrict__ size,
                                                     int64_t* __restrict__ counts, int64_t* __restrict__ ctr) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n_nodes) { parent[v] = (int)v; size[v] = 0; }
  if (v < 5) counts[v] = 0;
  if (v < TRACKS_CTR_COUNT) ctr[v] = 0;
}

// ---------------------------------------------------------------------------------------------------- hook
// One lane per edge.  Both ends are followed to their roots; while the roots differ, the larger one is put under the
// smaller one with old = atomicCAS(&parent[hi], hi, lo).  Only a ROOT is ever re-parented (the CAS expects hi), and always
// under a smaller id, so parent[v] is written at most once and every chain of parents descends strictly: it ends, and the
// only node of a component that can remain a root is its smallest.  A failed CAS returns the value that won; the lane goes
// on from (old, lo) - from what the atomic returned, never from a plain re-read.  Every step lowers a candidate, so the
// walk is bounded by 2 n_nodes steps; the budget below is twice that and only guards against a defect: exhausting it sets
// counts[4] and the call fails instead of spinning.
__global__ __launch_bounds__(256) void k_tracks_hook(const int64_t* __restrict__ kp_ptr, int n_img, int n_nodes,
                                                     const int64_t* __restrict__ seg_ptr, int n_seg,
                                                     const int32_t* __restrict__ pair_img,
                                                     const int32_t* __restrict__ query_idx,
                                                     const int32_t* __restrict__ train_idx,
                                                     const uint8_t* __restrict__ mask, int64_t n_edges, int* parent,
                                                     int64_t* __restrict__ counts) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  if (mask && mask[e] == 0) return;
  const int s = range_of(seg_ptr, n_seg, e);
  bool bad = !(seg_ptr[s] <= e && e < seg_ptr[s + 1]);
  int64_t a = 0, b = 0;
  if (!bad) {
    const int i = pair_img[2 * (int64_t)s], j = pair_img[2 * (int64_t)s + 1];
    const int q = query_idx[e], t = train_idx[e];
    bad = i == j || i < 0 || j < 0 || i >= n_img || j >= n_img || q < 0 || t < 0;
    if (!bad) {
      const int64_t bi = kp_ptr[i], bj = kp_ptr[j];
      a = bi + q; b = bj + t;
      bad = a >= kp_ptr[i + 1] || b >= kp_ptr[j + 1] || bi < 0 || bj < 0 || a >= n_nodes || b >= n_nodes;
    }
  }
  if (bad) { add64(&counts[3], 1); return; }
  int64_t budget = 4 * (int64_t)n_nodes + 1024;
  int ra = (int)a, rb = (int)b;
  for (;;) {
    for (;;) {
      const int p = parent_of(parent, ra);
      if (p == ra) break;
      ra = p;
      if (--budget < 0) break;
    }
    for (;;) {
      const int p = parent_of(parent, rb);
      if (p == rb) break;
      rb = p;
      if (--budget < 0) break;
    }
    if (ra == rb) return;
    if (--budget < 0) break;
    const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    const int old = atomicCAS(&parent[hi], hi, lo);
    if (old == hi) return;
    ra = old; rb = lo;
  }
  counts[4] = 1;
}

// ------------------------------------------------------------------------------------------------- flatten
// A launch of its own: every link is in place and visible.  Chains descend, so the walk ends.
__global__ __launch_bounds__(256) void k_tracks_flatten(int n_nodes, const int* __restrict__ parent,
                                                        int* __restrict__ label, int* __restrict__ size) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n_nodes) return;
  int r = (int)v;
  for (;;) {
    const int p = parent[r];
    if (p == r) break;
    r = p;
  }
  label[v] = r;
  atomicAdd(&size[r], 1);
}

// ---------------------------------------------------------------------------------------------------- scans
// A (flag, length) pair goes through block_exclusive_scan as one 64-bit value, the flag in the low half: a workgroup's
// flags sum to at most 256 and its lengths to at most n_nodes < 2^31, so neither half leaves its 32 bits.
__device__ __forceinline__ int64_t pair_pack(int a, int b) { return (int64_t)a | ((int64_t)b << 32); }
__device__ __forceinline__ int pair_a(int64_t v) { return (int)(v & 0xFFFFFFFFll); }
__device__ __forceinline__ int pair_b(int64_t v) { return (int)(v >> 32); }

struct tracks_dev {
  int64_t* ctr;
  int *parent, *label, *size, *cidx, *members;
  int *cand_root, *cand_off, *cand_len, *cand_cur, *cand_conf, *cand_tid, *cand_obs;
  int* long_list;
  int *blk_a, *blk_b;
};

// the pair (flag, length) an item contributes.  MODE 0: item = node, flag = root of a component with >= min_len nodes.
// MODE 1: item = candidate, flag = kept under the policy.
template <int MODE>
__device__ __forceinline__ void tracks_item(const tracks_dev& w, int64_t item, int n_nodes, int min_len, int policy, int& a,
                                          int& b) {
  a = 0; b = 0;
  if (MODE == 0) {
    if (item < n_nodes && w.label[item] == (int)item && w.size[item] >= min_len) { a = 1; b = w.size[item]; }
  } else {
    if (item < w.ctr[TRACKS_CTR_CAND] && !(policy == TRACKS_POLICY_DROP && w.cand_conf[item] != 0)) {
      a = 1; b = w.cand_len[item];
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_tracks_scan_reduce(tracks_dev w, int n_nodes, int min_len, int policy) {
  __shared__ int64_t s_w[4];
  int a, b;
  tracks_item<MODE>(w, (int64_t)blockIdx.x * 256 + threadIdx.x, n_nodes, min_len, policy, a, b);
  int64_t total;
  (void)block_exclusive_scan<256, int64_t>(pair_pack(a, b), s_w, &total);
  if (threadIdx.x == 0) { w.blk_a[blockIdx.x] = pair_a(total); w.blk_b[blockIdx.x] = pair_b(total); }
}

// exclusive scan in place of the n block sums of both quantities by one workgroup; the totals go to two counters
__global__ __launch_bounds__(256) void k_tracks_scan_sums(int n, int* blk_a, int* blk_b, int64_t* __restrict__ total_a,
                                                          int64_t* __restrict__ total_b) {
  __shared__ int64_t s_wave[4];
  int64_t ta, tb;
  scan_counts<256>(n, blk_a, blk_a, s_wave, &ta);
  scan_counts<256>(n, blk_b, blk_b, s_wave, &tb);
  if (threadIdx.x == 0) { *total_a = ta; *total_b = tb; }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_tracks_scan_apply(tracks_dev w, int n_nodes, int min_len, int policy,
                                                           int64_t* __restrict__ track_ptr,
                                                           uint8_t* __restrict__ track_conflict,
                                                           int64_t* __restrict__ counts) {
  __shared__ int64_t s_w[4];
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int a, b;
  tracks_item<MODE>(w, item, n_nodes, min_len, policy, a, b);
  int64_t total;
  const int64_t before = block_exclusive_scan<256, int64_t>(pair_pack(a, b), s_w, &total);
  const int num = w.blk_a[blockIdx.x] + pair_a(before), off = w.blk_b[blockIdx.x] + pair_b(before);
  if (MODE == 0) {
    if (a) {
      w.cidx[item] = num;
      w.cand_root[num] = (int)item; w.cand_off[num] = off; w.cand_len[num] = b;
      w.cand_cur[num] = 0; w.cand_conf[num] = 0;
    }
  } else {
    if (item < w.ctr[TRACKS_CTR_CAND]) {
      w.cand_tid[item] = a ? num : -1;
      w.cand_obs[item] = off;
      if (a) { track_ptr[num] = off; track_conflict[num] = w.cand_conf[item] != 0 ? 1 : 0; }
    }
    if (item == 0) {
      const int64_t n_tracks = w.ctr[TRACKS_CTR_KEPT], n_obs = w.ctr[TRACKS_CTR_KEPT_OBS];
      counts[0] = n_tracks; counts[1] = n_obs;
      track_ptr[n_tracks] = n_obs;
    }
  }
}

// --------------------------------------------------------------------------------------------------- claim
__global__ __launch_bounds__(256) void k_tracks_claim(tracks_dev w, int n_nodes, int min_len,
                                                      int32_t* __restrict__ node_track) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n_nodes) return;
  const int r = w.label[v], s = w.size[r];
  if (s >= min_len) {
    const int c = w.cidx[r];
    const int slot = atomicAdd(&w.cand_cur[c], 1);
    w.members[(int64_t)w.cand_off[c] + slot] = (int)v;
  } else {
    node_track[v] = s == 1 ? -1 : -2;
  }
}

// ---------------------------------------------------------------------------------------------------- sort
// One lane per candidate: a short one is sorted where it lies (insertion sort: the mean track has 4 views), a long one
// is put on the list of the workgroup kernel (the order of that list does not matter: each entry is sorted on its own).
__global__ __launch_bounds__(256) void k_tracks_sort_short(tracks_dev w) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= w.ctr[TRACKS_CTR_CAND]) return;
  const int len = w.cand_len[c];
  if (len > TRACKS_SHORT_MAX) {
    const unsigned long long k = atomicAdd((unsigned long long*)&w.ctr[TRACKS_CTR_LONG], 1ull);
    w.long_list[k] = (int)c;
    return;
  }
  int* m = w.members + w.cand_off[c];
  for (int i = 1; i < len; ++i) {
    const int x = m[i];
    int j = i - 1;
    while (j >= 0 && m[j] > x) { m[j + 1] = m[j]; --j; }
    m[j + 1] = x;
  }
}

// The network of tracks_plan.h run by a whole workgroup: one barrier per step.
__device__ void wg_bitonic(int* a, unsigned len) {
  const unsigned lp = tracks_bitonic_levels(len);
  const unsigned half = 1u << (lp - 1);
  for (unsigned lk = 1; lk <= lp; ++lk) {
    for (unsigned t = threadIdx.x; t < half; t += 256) {
      unsigned i, j;
      tracks_bitonic_mirror(t, lk, i, j);
      if (j < len) {
        const int x = a[i], y = a[j];
        if (x > y) { a[i] = y; a[j] = x; }
      }
    }
    __syncthreads();
    for (unsigned ld = lk - 1; ld-- > 0;) {            // distances 2^(lk-2) ... 1
      for (unsigned t = threadIdx.x; t < half; t += 256) {
        unsigned i, j;
        tracks_bitonic_step(t, ld, i, j);
        if (j < len) {
          const int x = a[i], y = a[j];
          if (x > y) { a[i] = y; a[j] = x; }
        }
      }
      __syncthreads();
    }
  }
}

// Workgroups share the list of long candidates.  Up to TRACKS_LDS_MAX members are sorted in LDS, longer ones in global
// memory (the workgroup is the only reader and writer of that range; __syncthreads orders its waves' accesses).
__global__ __launch_bounds__(256) void k_tracks_sort_long(tracks_dev w) {
  __shared__ int s_m[TRACKS_LDS_MAX];
  const int64_t n_long = w.ctr[TRACKS_CTR_LONG];
  for (int64_t k = blockIdx.x; k < n_long; k += gridDim.x) {
    const int c = w.long_list[k];
    const unsigned len = (unsigned)w.cand_len[c];
    int* m = w.members + w.cand_off[c];
    if (len <= (unsigned)TRACKS_LDS_MAX) {
      for (unsigned i = threadIdx.x; i < len; i += 256) s_m[i] = m[i];
      __syncthreads();
      wg_bitonic(s_m, len);
      for (unsigned i = threadIdx.x; i < len; i += 256) m[i] = s_m[i];
      __syncthreads();
    } else {
      wg_bitonic(m, len);
    }
  }
}

// ------------------------------------------------------------------------------------- conflict, emit
// One lane per slot of `members`: a member of the image of its sorted predecessor marks the candidate (node ids are
// image-major, so two nodes of one image are adjacent once sorted).
__global__ __launch_bounds__(256) void k_tracks_conflict(tracks_dev w, const int64_t* __restrict__ kp_ptr, int n_img,
                                                         int64_t* __restrict__ counts) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= w.ctr[TRACKS_CTR_CAND_OBS]) return;
  const int v = w.members[p];
  const int c = w.cidx[w.label[v]];
  if (p == w.cand_off[c]) return;
  const int u = w.members[p - 1];
  if (range_of(kp_ptr, n_img, u) != range_of(kp_ptr, n_img, v)) return;
  if (atomicExch(&w.cand_conf[c], 1) == 0) add64(&counts[2], 1);
}

__global__ __launch_bounds__(256) void k_tracks_emit(tracks_dev w, const int64_t* __restrict__ kp_ptr, int n_img,
                                                     int32_t* __restrict__ obs_image, int32_t* __restrict__ obs_kp,
                                                     int32_t* __restrict__ node_track) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= w.ctr[TRACKS_CTR_CAND_OBS]) return;
  const int v = w.members[p];
  const int c = w.cidx[w.label[v]];
  const int t = w.cand_tid[c];
  if (t < 0) { node_track[v] = -3; return; }
  const int64_t o = (int64_t)w.cand_obs[c] + (p - w.cand_off[c]);
  const int img = range_of(kp_ptr, n_img, v);
  obs_image[o] = img;
  obs_kp[o] = (int32_t)(v - kp_ptr[img]);
  node_track[v] = t;
}

tracks_dev tracks_carve(void* workspace, const tracks_layout& L) {
  char* p = (char*)workspace;
  tracks_dev w;
  w.ctr = (int64_t*)(p + L.ctr);
  w.parent = (int*)(p + L.parent); w.label = (int*)(p + L.label); w.size = (int*)(p + L.size);
  w.cidx = (int*)(p + L.cidx); w.members = (int*)(p + L.members);
  w.cand_root = (int*)(p + L.cand_root); w.cand_off = (int*)(p + L.cand_off); w.cand_len = (int*)(p + L.cand_len);
  w.cand_cur = (int*)(p + L.cand_cur); w.cand_conf = (int*)(p + L.cand_conf); w.cand_tid = (int*)(p + L.cand_tid);
  w.cand_obs = (int*)(p + L.cand_obs);
  w.long_list = (int*)(p + L.long_list);
  w.blk_a = (int*)(p + L.blk_a); w.blk_b = (int*)(p + L.blk_b);
  return w;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_tracks_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t* bytes_host) {
  if (!bytes_host || n_nodes < 0 || n_edges < 0 || n_nodes >= ((int64_t)1 << 31)) return SFM_ERR_ARG;
  *bytes_host = tracks_plan_layout(n_nodes).bytes;
  return SFM_OK;
}

extern "C" int sfm_tracks_build(sfm_handle h, const int64_t* kp_ptr, int32_t n_img, int64_t n_nodes, const int64_t* seg_ptr,
                                int32_t n_seg, const int32_t* pair_img, const int32_t* query_idx, const int32_t* train_idx,
                                const uint8_t* mask, int64_t n_edges, int32_t min_len, int32_t policy, int64_t* track_ptr,
                                int32_t* obs_image, int32_t* obs_kp, uint8_t* track_conflict, int32_t* node_track,
                                int64_t* counts, int64_t cap_tracks, int64_t cap_obs, void* workspace,
                                int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  static const char* const rule[] = {"", "negative size", "n_nodes must be below 2^31", "min_len must be at least 2",
                                     "policy must be 0 (drop) or 1 (keep)",
                                     "cap_tracks / cap_obs below n_nodes / 2 / n_nodes", "nodes without images"};
  const int why = tracks_check_sizes(n_img, n_nodes, n_seg, n_edges, min_len, policy, cap_tracks, cap_obs);
  if (why) return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_build", rule[why]);
  if (!track_ptr || !counts || (n_nodes > 0 && (!node_track || !obs_image || !obs_kp)) || (n_nodes > 1 && !track_conflict))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_build", "null pointer");
  if (n_nodes == 0 || n_edges == 0 || n_seg == 0) {      // no tracks, every keypoint unmatched
    SFM_HIP(h, hipMemsetAsync(counts, 0, 5 * sizeof(int64_t), h->stream));
    SFM_HIP(h, hipMemsetAsync(track_ptr, 0, sizeof(int64_t), h->stream));
    if (n_nodes > 0) SFM_HIP(h, hipMemsetAsync(node_track, 0xff, (size_t)n_nodes * sizeof(int32_t), h->stream));
    return SFM_OK;
  }
  if (!kp_ptr || !seg_ptr || !pair_img || !query_idx || !train_idx || !workspace)
    return sfm_fail(h, SFM_ERR_ARG, "sfm_tracks_build", "null pointer");
  const tracks_layout L = tracks_plan_layout(n_nodes);
  if (workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_WORKSPACE, "sfm_tracks_build", "workspace too small");
  const tracks_dev w = tracks_carve(workspace, L);
  const int N = (int)n_nodes;
  const dim3 tb(256), gn(cdiv(n_nodes, 256)), gc(cdiv(tracks_cap_tracks(n_nodes) + 1, 256));
  hipLaunchKernelGGL(k_tracks_init, gn, tb, 0, h->stream, N, w.parent, w.size, counts, w.ctr);
  hipLaunchKernelGGL(k_tracks_hook, dim3(cdiv(n_edges, 256)), tb, 0, h->stream, kp_ptr, (int)n_img, N, seg_ptr, (int)n_seg,
                     pair_img, query_idx, train_idx, mask, n_edges, w.parent, counts);
  hipLaunchKernelGGL(k_tracks_flatten, gn, tb, 0, h->stream, N, (const int*)w.parent, w.label, w.size);
  hipLaunchKernelGGL(k_tracks_scan_reduce<0>, gn, tb, 0, h->stream, w, N, (int)min_len, (int)policy);
  hipLaunchKernelGGL(k_tracks_scan_sums, dim3(1), tb, 0, h->stream, (int)gn.x, w.blk_a, w.blk_b, w.ctr + TRACKS_CTR_CAND,
                     w.ctr + TRACKS_CTR_CAND_OBS);
  hipLaunchKernelGGL(k_tracks_scan_apply<0>, gn, tb, 0, h->stream, w, N, (int)min_len, (int)policy, track_ptr,
                     track_conflict, counts);
  hipLaunchKernelGGL(k_tracks_claim, gn, tb, 0, h->stream, w, N, (int)min_len, node_track);
  hipLaunchKernelGGL(k_tracks_sort_short, gc, tb, 0, h->stream, w);
  hipLaunchKernelGGL(k_tracks_sort_long, dim3(TRACKS_LONG_GRID), tb, 0, h->stream, w);
  hipLaunchKernelGGL(k_tracks_conflict, gn, tb, 0, h->stream, w, kp_ptr, (int)n_img, counts);
  hipLaunchKernelGGL(k_tracks_scan_reduce<1>, gc, tb, 0, h->stream, w, N, (int)min_len, (int)policy);
  hipLaunchKernelGGL(k_tracks_scan_sums, dim3(1), tb, 0, h->stream, (int)gc.x, w.blk_a, w.blk_b, w.ctr + TRACKS_CTR_KEPT,
                     w.ctr + TRACKS_CTR_KEPT_OBS);
  hipLaunchKernelGGL(k_tracks_scan_apply<1>, gc, tb, 0, h->stream, w, N, (int)min_len, (int)policy, track_ptr,
                     track_conflict, counts);
  hipLaunchKernelGGL(k_tracks_emit, gn, tb, 0, h->stream, w, kp_ptr, (int)n_img, obs_image, obs_kp, node_track);
  SFM_LAUNCH_CHECK(h, "sfm_tracks_build");
  // the status word, once, behind the last launch
  int64_t* status = (int64_t*)(h->pinned + SFM_PIN_TRACKS);
  SFM_HIP(h, hipMemcpyAsync(status, counts + 4, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  SFM_HIP(h, hipStreamSynchronize(h->stream));
  if (*status != 0) return sfm_fail(h, SFM_ERR_NUMERIC, "sfm_tracks_build", "the union loop ran out of its step budget");
  return SFM_OK;
}
