// Guided matching for gfx950 (MI355X): nearest neighbour + ratio test among the keypoints near the epipolar line only.
//
// Once a pair (i, j) has a fundamental matrix, a query q of image i is compared with C(q) = { t of image j : gate(q, t) }
// (guided_rule.h: both point-line distances within `gate_px` pixels) instead of with the whole image, so a descriptor
// that repeats elsewhere in the image no longer fails the ratio test.  Per query: best = min over C(q) of (distance, t),
// second = min of the rest; kept iff |C(q)| >= 1, d1 <= max_distance (when given), |C(q)| == 1 or (double)d1 < ratio *
// (double)d2, and - with cross_check - q is the (distance, q') minimum over { q' : gate(q', best) }.  Distances are the
// matcher's: the popcount, or sqrtf of the integer d^2, as float32.
//
// The gate is the hot loop (at 3 px about 1 % of the combinations pass), the descriptor distance the rare one, so they
// are kept apart.  One workgroup of 4 wavefronts takes a tile of GUIDED_QT queries of one pair and stages the other
// image's per-point half of the rule through LDS, GUIDED_CHUNK points at a time.  A wavefront walks its GUIDED_QW queries
// one at a time: the query's half of the rule is wave-uniform, lane = point.  The __ballot of the gate is compacted with
// mbcnt into the query's candidate queue in LDS; whenever GUIDED_DRAIN candidates are queued, and once more at the end,
// the queue drains with lane = candidate: each lane gathers its row, computes the distance and the 64-bit key
// (float32 distance bits << 32 | index), and a butterfly reduction merges the wave's two smallest keys into the query's
// running two.  Keys are distinct, so the result does not depend on the order candidates are met in.  Nothing but one
// row of results per query reaches memory; the kept matches are compacted by count / scan / scatter without atomics.
// The cross-check is the same kernel with the roles swapped (image i stays in slot one of the rule) and a join.
#include "common.h"
#include "guided_rule.h"
#include "guided_plan.h"
#include "block_scan.h"

namespace {

constexpr unsigned long long KEY_NONE = ~0ull;

__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }      // correctly rounded (see match.hip)

// distance between the descriptor rows qr and tr of DIMV 16-byte pieces
template <int METRIC, int DIMV>
__device__ __forceinline__ float row_distance(const uint4* __restrict__ qr, const uint4* __restrict__ tr) {
  int acc = 0;
#pragma unroll
  for (int v = 0; v < DIMV; ++v) {
    const uint4 a = qr[v], b = tr[v];
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (METRIC == SFM_METRIC_HAMMING) {
        acc += __popc(aw[k] ^ bw[k]);
      } else {
#pragma unroll
        for (int sh = 0; sh < 32; sh += 8) {
          const int df = (int)((aw[k] >> sh) & 0xFFu) - (int)((bw[k] >> sh) & 0xFFu);
          acc += df * df;
        }
      }
    }
  }
  return METRIC == SFM_METRIC_HAMMING ? (float)acc : sqrt_rn((float)acc);      // d^2 <= 128 * 255^2 < 2^24: exact in float32
}

__device__ __forceinline__ unsigned long long umin64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a < b ? b : a; }
// the two smallest of {k1 <= k2} and {o1 <= o2}
__device__ __forceinline__ void merge2(unsigned long long& k1, unsigned long long& k2, unsigned long long o1, unsigned long long o2) {
  const unsigned long long lo = umin64(k1, o1), hi = umax64(k1, o1);
  k2 = umin64(hi, umin64(k2, o2));
  k1 = lo;
}

// REV = false: queries are image i's rows, candidates image j's.  REV = true (cross-check): queries are image j's rows,
// candidates image i's, and only the best is wanted.  idx1 / d1 / d2 / ncand are indexed by output row (REV: reverse row).
template <int METRIC, int DIMV, bool REV>
__global__ __launch_bounds__(64 * GUIDED_WAVES) void k_guided(const uint8_t* __restrict__ desc, const float2* __restrict__ xy,
                                                              const GuidedSeg* __restrict__ segs, int n_seg,
                                                              const double* __restrict__ Fs, double thr2, int* __restrict__ idx1,
                                                              float* __restrict__ d1, float* __restrict__ d2, int* __restrict__ ncand) {
  __shared__ double s_p[4][GUIDED_CHUNK];                               // the staged half of the rule, one array per value
  __shared__ int s_ring[GUIDED_WAVES][GUIDED_QW][GUIDED_RING];          // candidate queue of every query
  __shared__ unsigned long long s_key[GUIDED_WAVES][GUIDED_QW][2];      // running best two
  __shared__ double s_q[GUIDED_WAVES][GUIDED_QW][4];                    // the query's half of the rule
  __shared__ int s_rc[GUIDED_WAVES][GUIDED_QW], s_nc[GUIDED_WAVES][GUIDED_QW];      // queued / drained candidates
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int s = guided_find(segs, n_seg, blockIdx.x, REV ? GUIDED_BY_REV_TILE : GUIDED_BY_TILE);
  const GuidedSeg seg = segs[s];
  const int64_t tile = (int64_t)blockIdx.x - (REV ? seg.rev_tile_first : seg.tile_first);
  const int64_t qb = REV ? seg.t_beg : seg.q_beg, qe = REV ? seg.t_end : seg.q_end;      // query rows
  const int64_t lb = REV ? seg.q_beg : seg.t_beg, le = REV ? seg.q_end : seg.t_end;      // rows of the lane side
  const int64_t out0 = REV ? seg.rev_first : seg.out_first;
  double f[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) f[k] = Fs[(int64_t)s * 9 + k];

  const int64_t q_wave = qb + tile * GUIDED_QT + (int64_t)w * GUIDED_QW;     // first query of this wavefront
  const int64_t left = qe - q_wave;
  const int nqw = left <= 0 ? 0 : (left < GUIDED_QW ? (int)left : GUIDED_QW);
  if (lane < GUIDED_QW) {
    s_key[w][lane][0] = KEY_NONE; s_key[w][lane][1] = KEY_NONE;
    s_rc[w][lane] = 0; s_nc[w][lane] = 0;
    if (lane < nqw) {
      const float2 p = xy[q_wave + lane];
      if (REV) {
        const guided::Side2 v = guided::side2(f, p.x, p.y);
        s_q[w][lane][0] = v.x; s_q[w][lane][1] = v.y; s_q[w][lane][2] = v.den; s_q[w][lane][3] = 0.0;
      } else {
        const guided::Side1 v = guided::side1(f, p.x, p.y);
        s_q[w][lane][0] = v.a; s_q[w][lane][1] = v.b; s_q[w][lane][2] = v.c; s_q[w][lane][3] = v.den;
      }
    }
  }

  // candidates [0, n) of query qi's queue -> distances -> the query's running best two
  auto drain = [&](int qi, int n) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    unsigned long long k1 = KEY_NONE, k2 = KEY_NONE;
    if (lane < n) {
      const int t = s_ring[w][qi][lane];
      const float dist = row_distance<METRIC, DIMV>((const uint4*)desc + (q_wave + qi) * DIMV, (const uint4*)desc + (lb + t) * DIMV);
      k1 = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)t;      // dist >= 0: its bits order as its value
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long o1 = __shfl_xor(k1, o, 64), o2 = __shfl_xor(k2, o, 64);
      merge2(k1, k2, o1, o2);
    }
    merge2(k1, k2, s_key[w][qi][0], s_key[w][qi][1]);
    const int nc = s_nc[w][qi] + n;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (lane == 0) { s_key[w][qi][0] = k1; s_key[w][qi][1] = k2; s_nc[w][qi] = nc; }
  };

  for (int64_t cb = lb; cb < le; cb += GUIDED_CHUNK) {
    const int cnt = (le - cb) < GUIDED_CHUNK ? (int)(le - cb) : GUIDED_CHUNK;
    __syncthreads();                                        // the previous chunk has been read by every wavefront
    for (int i = tid; i < cnt; i += 64 * GUIDED_WAVES) {
      const float2 p = xy[cb + i];
      if (REV) {
        const guided::Side1 v = guided::side1(f, p.x, p.y);
        s_p[0][i] = v.a; s_p[1][i] = v.b; s_p[2][i] = v.c; s_p[3][i] = v.den;
      } else {
        const guided::Side2 v = guided::side2(f, p.x, p.y);
        s_p[0][i] = v.x; s_p[1][i] = v.y; s_p[2][i] = v.den;
      }
    }
    __syncthreads();
    const int t0 = (int)(cb - lb);                          // index inside the pair of the chunk's first point
    for (int qi = 0; qi < nqw; ++qi) {
      const double q0 = s_q[w][qi][0], q1 = s_q[w][qi][1], q2 = s_q[w][qi][2], q3 = s_q[w][qi][3];
      int rc = s_rc[w][qi];
      for (int base = 0; base < cnt; base += 64) {
        const int j = base + lane;
        bool g = false;
        if (j < cnt) {
          g = REV ? guided::gate(s_p[0][j], s_p[1][j], s_p[2][j], s_p[3][j], q0, q1, q2, thr2)
                  : guided::gate(q0, q1, q2, q3, s_p[0][j], s_p[1][j], s_p[2][j], thr2);
        }
        const unsigned long long m = __ballot(g);
        if (m == 0ull) continue;                            // wave-uniform: most steps end here
        const int pos = rc + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (g) s_ring[w][qi][pos] = t0 + j;                 // rc < GUIDED_DRAIN here, so pos < GUIDED_RING
        rc += __popcll(m);
        if (rc >= GUIDED_DRAIN) {
          drain(qi, GUIDED_DRAIN);
          rc -= GUIDED_DRAIN;                               // < GUIDED_DRAIN left: move them to the front
          int keep = 0;
          if (lane < rc) keep = s_ring[w][qi][GUIDED_DRAIN + lane];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          if (lane < rc) s_ring[w][qi][lane] = keep;
        }
      }
      if (lane == 0) s_rc[w][qi] = rc;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int qi = 0; qi < nqw; ++qi) {
    const int rc = s_rc[w][qi];
    if (rc > 0) drain(qi, rc);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < nqw) {
    const unsigned long long k1 = s_key[w][lane][0], k2 = s_key[w][lane][1];
    const int64_t o = out0 + (q_wave - qb) + lane;
    idx1[o] = k1 == KEY_NONE ? -1 : (int)(unsigned)k1;
    if (!REV) {
      d1[o] = k1 == KEY_NONE ? 0.0f : __uint_as_float((unsigned)(k1 >> 32));
      d2[o] = k2 == KEY_NONE ? __builtin_huge_valf() : __uint_as_float((unsigned)(k2 >> 32));
      ncand[o] = s_nc[w][lane];
    }
  }
}

// ------------------------------------------------------------------------------------ which queries are kept
__device__ __forceinline__ bool guided_keeps(int64_t o, const GuidedSeg* __restrict__ segs, int n_seg, const int* __restrict__ idx1,
                                             const float* __restrict__ d1, const float* __restrict__ d2, const int* __restrict__ ncand,
                                             const int* __restrict__ rev, double ratio, double max_distance, int cross_check) {
  const int nc = ncand[o];
  if (nc < 1) return false;
  const double a = (double)d1[o];
  if (max_distance >= 0.0 && !(a <= max_distance)) return false;
  if (nc > 1 && !(a < ratio * (double)d2[o])) return false;
  if (cross_check) {
    const GuidedSeg r = segs[guided_find(segs, n_seg, o, GUIDED_BY_OUT)];
    if ((int64_t)rev[r.rev_first + idx1[o]] != o - r.out_first) return false;
  }
  return true;
}

__global__ __launch_bounds__(256) void k_guided_count(int64_t n_out, const GuidedSeg* __restrict__ segs, int n_seg,
                                                      const int* __restrict__ idx1, const float* __restrict__ d1,
                                                      const float* __restrict__ d2, const int* __restrict__ ncand,
                                                      const int* __restrict__ rev, double ratio, double max_distance, int cross_check,
                                                      uint8_t* __restrict__ keep, int* __restrict__ blk_cnt) {
  __shared__ int s_c[4];
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool k = o < n_out && guided_keeps(o, segs, n_seg, idx1, d1, d2, ncand, rev, ratio, max_distance, cross_check);
  if (o < n_out) keep[o] = k ? 1 : 0;
  const int kept = block_flag_count(k, s_c);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = kept;
}

// exclusive scan of the per-block counts by one workgroup; one entry past the last block: the total
__global__ __launch_bounds__(256) void k_guided_scan(int nblk, const int* __restrict__ blk_cnt, int* __restrict__ blk_off) {
  __shared__ int64_t s_wave[4];
  int64_t total;
  scan_counts<256>(nblk, blk_cnt, blk_off, s_wave, &total);
  if (threadIdx.x == 0) blk_off[nblk] = (int)total;
}

__global__ __launch_bounds__(256) void k_guided_scatter(int64_t n_out, const GuidedSeg* __restrict__ segs, int n_seg,
                                                        const uint8_t* __restrict__ keep, const int* __restrict__ blk_off,
                                                        const int* __restrict__ idx1, const float* __restrict__ d1,
                                                        int* __restrict__ query_idx, int* __restrict__ train_idx, float* __restrict__ dist) {
  __shared__ int s_c[4];
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool k = o < n_out && keep[o] != 0;
  const int off = blk_off[blockIdx.x] + block_flag_rank(k, s_c);
  if (k) {
    const int s = guided_find(segs, n_seg, o, GUIDED_BY_OUT);
    query_idx[off] = (int)(o - segs[s].out_first);
    train_idx[off] = idx1[o];
    dist[off] = d1[o];
  }
}

// seg_ptr[s] = kept rows in front of the segment's first output row (s = n_seg: all of them)
__global__ __launch_bounds__(256) void k_guided_seg_ptr(int64_t n_out, const GuidedSeg* __restrict__ segs, int n_seg,
                                                        const uint8_t* __restrict__ keep, const int* __restrict__ blk_off,
                                                        int64_t* __restrict__ seg_ptr) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s > n_seg) return;
  const int64_t row = segs[s].out_first;                    // record n_seg holds n_out
  const int64_t blk = row >> 8;
  int64_t v = blk_off[blk];                                 // blk_off has one entry past the last block: the total
  for (int64_t o = blk << 8; o < row; ++o) v += keep[o];
  seg_ptr[s] = v;
}

int guided_check_metric(sfm_ctx* h, int metric, int dim) {
  if (metric == SFM_METRIC_HAMMING) {
    if (dim != 16 && dim != 32 && dim != 64) return sfm_fail(h, SFM_ERR_ARG, "sfm_guided_match", "HAMMING supports dim 16, 32, 64 bytes");
  } else if (metric == SFM_METRIC_L2_U8) {
    if (dim != 32 && dim != 64 && dim != 128) return sfm_fail(h, SFM_ERR_ARG, "sfm_guided_match", "L2_U8 needs dim 32, 64 or 128");
  } else {
    return sfm_fail(h, SFM_ERR_ARG, "sfm_guided_match", "metric must be SFM_METRIC_HAMMING or SFM_METRIC_L2_U8 (uint8 descriptors)");
  }
  return SFM_OK;
}

template <bool REV>
void guided_launch(sfm_ctx* h, int metric, int dim, unsigned grid, const uint8_t* desc, const float2* xy, const GuidedSeg* segs, int n_seg,
                   const double* F, double thr2, int* idx1, float* d1, float* d2, int* ncand) {
#define GUIDED_LAUNCH(M, V) hipLaunchKernelGGL((k_guided<M, V, REV>), dim3(grid), dim3(64 * GUIDED_WAVES), 0, h->stream, desc, xy, segs, n_seg, F, thr2, idx1, d1, d2, ncand)
  if (metric == SFM_METRIC_HAMMING) {
    if (dim == 16) GUIDED_LAUNCH(SFM_METRIC_HAMMING, 1); else if (dim == 32) GUIDED_LAUNCH(SFM_METRIC_HAMMING, 2); else GUIDED_LAUNCH(SFM_METRIC_HAMMING, 4);
  } else {
    if (dim == 32) GUIDED_LAUNCH(SFM_METRIC_L2_U8, 2); else if (dim == 64) GUIDED_LAUNCH(SFM_METRIC_L2_U8, 4); else GUIDED_LAUNCH(SFM_METRIC_L2_U8, 8);
  }
#undef GUIDED_LAUNCH
}

}  // namespace

extern "C" int sfm_guided_workspace_bytes(int metric, int32_t n_seg, const int64_t* q_beg_host, const int64_t* q_end_host,
                                          const int64_t* t_beg_host, const int64_t* t_end_host, int64_t* n_out_host, int64_t* bytes_host) {
  if (!n_out_host || !bytes_host) return SFM_ERR_ARG;
  if (metric != SFM_METRIC_HAMMING && metric != SFM_METRIC_L2_U8) return SFM_ERR_ARG;
  if (guided_check_segments(n_seg, q_beg_host, q_end_host, t_beg_host, t_end_host, 0x7FFFFF00LL)) return SFM_ERR_ARG;
  const GuidedPlan p = guided_plan(n_seg, q_beg_host, q_end_host, t_beg_host, t_end_host);
  *n_out_host = p.n_out;
  *bytes_host = guided_layout(n_seg, p.n_out, p.n_rev).bytes;
  return SFM_OK;
}

extern "C" int sfm_guided_match(sfm_handle h, int metric, const void* desc, int64_t n_rows, int dim, const float* xy, int32_t n_seg,
                                const int64_t* q_beg_host, const int64_t* q_end_host, const int64_t* t_beg_host, const int64_t* t_end_host,
                                const double* F, double gate_px, double ratio, double max_distance, int cross_check, int32_t* query_idx,
                                int32_t* train_idx, float* distance, int32_t* n_candidates, int64_t* seg_ptr, void* workspace,
                                int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  int rc = guided_check_metric(h, metric, dim); if (rc) return rc;
  const int bad = guided_check_segments(n_seg, q_beg_host, q_end_host, t_beg_host, t_end_host, n_rows);
  if (bad) {
    static const char* const why[] = {"", "negative number of segments", "negative or too many rows", "null segment array",
                                      "query range outside the rows", "train range outside the rows"};
    return sfm_fail(h, SFM_ERR_ARG, "sfm_guided_match", why[bad]);
  }
  if (!seg_ptr || !workspace) return sfm_fail(h, SFM_ERR_ARG, "sfm_guided_match", "null pointer");
  if (!(gate_px >= 0.0)) return sfm_fail(h, SFM_ERR_ARG, "sfm_guided_match", "gate_px must be a number >= 0");
  const GuidedPlan p = guided_plan(n_seg, q_beg_host, q_end_host, t_beg_host, t_end_host);
  const GuidedLayout L = guided_layout(n_seg, p.n_out, p.n_rev);
  if (workspace_bytes < L.bytes) return sfm_fail(h, SFM_ERR_WORKSPACE, "sfm_guided_match", "workspace too small");
  if (p.n_out == 0) {                                       // no query anywhere: every segment is empty
    SFM_HIP(h, hipMemsetAsync(seg_ptr, 0, ((size_t)n_seg + 1) * 8, h->stream));
    return SFM_OK;
  }
  if (!desc || !xy || !F || !query_idx || !train_idx || !distance) return sfm_fail(h, SFM_ERR_ARG, "sfm_guided_match", "null pointer");
  char* ws = (char*)workspace;
  GuidedSeg* segs = (GuidedSeg*)(ws + L.segs);
  int* idx1 = (int*)(ws + L.idx1); float* d1 = (float*)(ws + L.d1); float* d2 = (float*)(ws + L.d2);
  int* ncand = n_candidates ? n_candidates : (int*)(ws + L.ncand);
  int* rev = (int*)(ws + L.rev);
  uint8_t* keep = (uint8_t*)(ws + L.keep);
  int* blk_cnt = (int*)(ws + L.blk_cnt); int* blk_off = (int*)(ws + L.blk_off);
  SFM_HIP(h, hipMemcpyAsync(segs, p.segs.data(), p.segs.size() * sizeof(GuidedSeg), hipMemcpyHostToDevice, h->stream));
  SFM_HIP(h, hipStreamSynchronize(h->stream));              // the table is pageable host memory: the copy must have left it
  const double thr2 = gate_px * gate_px;
  const uint8_t* d8 = (const uint8_t*)desc;
  const float2* xy2 = (const float2*)xy;
  guided_launch<false>(h, metric, dim, (unsigned)p.n_tiles, d8, xy2, segs, n_seg, F, thr2, idx1, d1, d2, ncand);
  if (cross_check && p.n_rev_tiles > 0)
    guided_launch<true>(h, metric, dim, (unsigned)p.n_rev_tiles, d8, xy2, segs, n_seg, F, thr2, rev, nullptr, nullptr, nullptr);
  const int nblk = (int)guided_blocks(p.n_out);
  hipLaunchKernelGGL(k_guided_count, dim3(nblk), dim3(256), 0, h->stream, p.n_out, segs, n_seg, idx1, d1, d2, ncand, rev, ratio,
                     max_distance, cross_check ? 1 : 0, keep, blk_cnt);
  hipLaunchKernelGGL(k_guided_scan, dim3(1), dim3(256), 0, h->stream, nblk, blk_cnt, blk_off);
  hipLaunchKernelGGL(k_guided_scatter, dim3(nblk), dim3(256), 0, h->stream, p.n_out, segs, n_seg, keep, blk_off, idx1, d1, query_idx,
                     train_idx, distance);
  hipLaunchKernelGGL(k_guided_seg_ptr, dim3(cdiv((int64_t)n_seg + 1, 256)), dim3(256), 0, h->stream, p.n_out, segs, n_seg, keep, blk_off,
                     seg_ptr);
  SFM_LAUNCH_CHECK(h, "sfm_guided_match");
  return SFM_OK;
}
