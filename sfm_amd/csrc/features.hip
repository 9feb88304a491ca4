// Feature detection and description, batched over the images of a data set (gfx950 only): the FAST-9/16 corner score,
// 3x3 non-maximum suppression with the border gate and the mask, an optional cut to max_features by a 256-bin
// histogram, and a steered binary descriptor of 256 bits over an integer-blurred image.  The arithmetic is the contract
// in include/sfm_amd.h; every step is integer, so the outputs have ONE byte pattern: keypoints come out row-major by
// construction (ballot + popcount prefix inside a row, an exclusive scan over the rows), never through an atomic counter.
//
// sfm_features_detect
//   k_feat_score     a 128 x 32 tile with a 3-pixel halo in LDS; branch-free segment test, exact score only for corners
//   k_feat_nms       one wavefront per image row: strict 3x3 maximum, gate, mask -> nms map, keypoints per row, histogram
//   k_feat_cut       per image: the cut score s and how many keypoints of score s stay          (max_features only)
//   k_feat_ties      one wavefront per row: keypoints above s and at s                          (max_features only)
//   k_feat_tie_scan  per image: ties before each row -> keypoints per row after the cut         (max_features only)
//   k_feat_scan      exclusive scan of the keypoints per row over all rows of all images -> row_off, kp_ptr
// sfm_features_describe
//   k_feat_scatter   the walk of k_feat_nms again: xy and score to their row-major positions
//   k_feat_blur      separable 7-tap integer blur, both passes in one kernel (uint16 intermediate in LDS)
//   k_feat_describe  one wavefront per keypoint: moments -> angle bin, 256 comparisons -> four ballots = the 32 bytes
#include "common.h"
#include "features_plan.h"
#include "block_scan.h"

namespace {

constexpr int SCORE_LDS_STRIDE = 160;      // 16 (alignment shift) + 128 + 6 rounded up to a multiple of 16
constexpr int SCORE_LDS_ROWS = FEAT_SCORE_TILE_H + 6;
constexpr int SCORE_CHUNKS = SCORE_LDS_STRIDE / 16;
constexpr int BLUR_IN_W = FEAT_TILE_W + 6, BLUR_IN_H = FEAT_BLUR_TILE_H + 6;

struct feat_dev {
  const feat_image* table;
  uint8_t* raw;
  uint8_t* nms;
  int* row_cnt;
  int* row_off;
  int* row_tie;
  unsigned* hist;
  int* cut;
  int* hdr;          // [0]: the edge of the detect call, read again by the scatter
};

// largest i in [0, n) with key(table[i]) <= v
template <typename F> __device__ __forceinline__ int table_find(int n, int v, F key) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (key(mid) <= v) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int popc_below(unsigned long long m) {
  return __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// ------------------------------------------------------------------------------------------------------ score

// b - 1 of the contract for the pixel whose circle differences are d[16]; 0 for a non-corner
__device__ __forceinline__ int fast_score(const int (&d)[16], int threshold) {
  unsigned hi = 0, lo = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    hi |= (unsigned)(d[i] > threshold) << i;
    lo |= (unsigned)(d[i] < -threshold) << i;
  }
  unsigned pass = 0;
#pragma unroll
  for (int pol = 0; pol < 2; ++pol) {
    const unsigned m0 = pol ? (lo | (lo << 16)) : (hi | (hi << 16));
    unsigned m = m0;
    m &= m >> 1; m &= m >> 2; m &= m >> 4; m &= m0 >> 8;      // a run of 9 in the doubled mask
    pass |= m;
  }
  if (pass == 0) return 0;
  int b = -255;
#pragma unroll
  for (int a = 0; a < 16; ++a) {
    int mn = 255, mx = -255;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int v = d[(a + j) & 15];
      mn = min(mn, v); mx = max(mx, v);
    }
    b = max(b, max(mn, -mx));
  }
  return b - 1;
}

__global__ __launch_bounds__(256) void k_feat_score(feat_dev w, int n_img, const uint8_t* __restrict__ images,
                                                    int threshold) {
  __shared__ __align__(16) uint8_t tile[SCORE_LDS_ROWS * SCORE_LDS_STRIDE];
  const feat_image* T = w.table;
  const int img = table_find(n_img, (int)blockIdx.x, [&](int i) { return T[i].score_tile0; });
  const feat_image m = T[img];
  const int t = (int)blockIdx.x - m.score_tile0;
  const int tx0 = (t % m.score_tiles_x) * FEAT_TILE_W, ty0 = (t / m.score_tiles_x) * FEAT_SCORE_TILE_H;
  const uint8_t* src = images + m.off;
  const int xs = max(tx0 - 3, 0), xe = min(tx0 + FEAT_TILE_W + 3, m.w), len = xe - xs;
  // the address of tile row 0 (image row ty0 - 3, which may lie above the image: only its low bits are used) mod 16
  const int sh_top = (int)(((uintptr_t)src + (uintptr_t)((int64_t)(ty0 - 3) * m.w + xs)) & 15);
  // Row r of the tile holds pixels [xs, xe) of image row ty0 - 3 + r, shifted by the low four bits of the row's global
  // address: a 16-byte chunk of LDS then maps to an aligned 16-byte chunk of global memory.  Only chunks that lie wholly
  // inside [xs, xe) are read as one vector; the rest goes byte by byte, so nothing outside the row is touched.
  for (int i = threadIdx.x; i < SCORE_LDS_ROWS * SCORE_CHUNKS; i += 256) {
    const int r = i / SCORE_CHUNKS, c = i % SCORE_CHUNKS, gy = ty0 - 3 + r;
    uint8_t* dst = tile + r * SCORE_LDS_STRIDE + 16 * c;
    if (gy < 0 || gy >= m.h) { *(uint4*)dst = make_uint4(0, 0, 0, 0); continue; }
    const uint8_t* row = src + (int64_t)gy * m.w + xs;
    const int sh = (sh_top + r * (m.w & 15)) & 15, lo = 16 * c - sh;  // sh = address of `row` mod 16; lo: this chunk's offset from `row`
    if (lo >= 0 && lo + 16 <= len) {
      *(uint4*)dst = *(const uint4*)(row + lo);
    } else {
      for (int k = 0; k < 16; ++k) dst[k] = (lo + k >= 0 && lo + k < len) ? row[lo + k] : (uint8_t)0;
    }
  }
  __syncthreads();
  // a thread takes 4 adjacent pixels of every 8th row
  const int px = (threadIdx.x & 31) * 4;
  uint8_t* out = w.raw + m.off;
  for (int ry = threadIdx.x >> 5; ry < FEAT_SCORE_TILE_H; ry += 8) {
    const int y = ty0 + ry;
    if (y >= m.h || tx0 + px >= m.w) continue;
    int rowpos[7];                      // where image rows y - 3 .. y + 3 start in the tile, their shifts included
#pragma unroll
    for (int j = 0; j < 7; ++j) rowpos[j] = (ry + j) * SCORE_LDS_STRIDE + ((sh_top + (ry + j) * (m.w & 15)) & 15);
    unsigned packed = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = tx0 + px + q;
      int s = 0;
      if (x >= 3 && y >= 3 && x < m.w - 3 && y < m.h - 3) {
        constexpr int CX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
        constexpr int CY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
        int d[16];
        const int centre = tile[rowpos[3] + (x - xs)];
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = (int)tile[rowpos[3 + CY[i]] + (x + CX[i] - xs)] - centre;
        s = fast_score(d, threshold);
      }
      packed |= (unsigned)s << (8 * q);
    }
    uint8_t* o = out + (int64_t)y * m.w + tx0 + px;
    if (((uintptr_t)o & 3) == 0 && tx0 + px + 3 < m.w) {
      *(unsigned*)o = packed;
    } else {
      for (int q = 0; q < 4; ++q)
        if (tx0 + px + q < m.w) o[q] = (uint8_t)(packed >> (8 * q));
    }
  }
}

// ------------------------------------------------------------------------------------------- suppression and counts
// the image and the row of entry R of the row list
__device__ __forceinline__ int row_image(const feat_image* T, int n_img, int R) {
  return table_find(n_img, R, [&](int i) { return T[i].row0; });
}

__global__ __launch_bounds__(256) void k_feat_nms(feat_dev w, int n_img, int n_rows, const uint8_t* __restrict__ masks,
                                                  int edge, int want_hist) {
  const int R = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (R >= n_rows) return;
  const int img = row_image(w.table, n_img, R);
  const feat_image m = w.table[img];
  const int y = R - m.row0;
  int kept = 0;
  if (y >= edge && y < m.h - edge) {
    const uint8_t* s = w.raw + m.off + (int64_t)y * m.w;
    uint8_t* o = w.nms + m.off + (int64_t)y * m.w;
    const uint8_t* mk = masks ? masks + m.off + (int64_t)y * m.w : nullptr;
    for (int x0 = edge; x0 < m.w - edge; x0 += 64) {
      const int x = x0 + lane;
      bool keep = false;
      int v = 0;
      if (x < m.w - edge) {          // the gate keeps x - 1, x + 1, y - 1, y + 1 inside the image
        v = s[x];
        if (v > 0) {
          const uint8_t *up = s - m.w, *dn = s + m.w;
          const int nb = max(max(max((int)up[x - 1], (int)up[x]), max((int)up[x + 1], (int)s[x - 1])),
                             max(max((int)s[x + 1], (int)dn[x - 1]), max((int)dn[x], (int)dn[x + 1])));
          keep = v > nb && (!mk || mk[x] > 0);
        }
        o[x] = keep ? (uint8_t)v : (uint8_t)0;
      }
      if (keep && want_hist) atomicAdd(&w.hist[(int64_t)img * 256 + v], 1u);
      kept += __popcll(__ballot(keep));
    }
  }
  if (lane == 0) { w.row_cnt[R] = kept; w.row_tie[R] = 0; }
}

// cut[img] = (s, quota): with more than max_features keypoints, s is the score with #(> s) < max_features <= #(>= s) and
// quota = max_features - #(> s) of the keypoints at s stay; otherwise (0, 0): every keypoint stays.
__global__ void k_feat_cut(feat_dev w, int n_img, int max_features, int edge) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= n_img) return;
  if (img == 0) w.hdr[0] = edge;
  const unsigned* hs = w.hist + (int64_t)img * 256;
  int64_t total = 0;
  for (int b = 1; b < 256; ++b) total += hs[b];
  int s = 0, quota = 0;
  if (max_features > 0 && total > max_features) {
    int64_t above = 0;
    for (int b = 255; b >= 1; --b) {
      if (above + hs[b] >= max_features) { s = b; quota = (int)(max_features - above); break; }
      above += hs[b];
    }
  }
  w.cut[2 * img] = s;
  w.cut[2 * img + 1] = quota;
}

__global__ __launch_bounds__(256) void k_feat_ties(feat_dev w, int n_img, int n_rows, int edge) {
  const int R = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (R >= n_rows) return;
  const int img = row_image(w.table, n_img, R);
  const int s = w.cut[2 * img];
  if (s == 0) return;
  const feat_image m = w.table[img];
  const int y = R - m.row0;
  if (y < edge || y >= m.h - edge) return;          // row_cnt and row_tie are 0 already
  const uint8_t* o = w.nms + m.off + (int64_t)y * m.w;
  int above = 0, ties = 0;
  for (int x0 = edge; x0 < m.w - edge; x0 += 64) {
    const int x = x0 + lane;
    const int v = x < m.w - edge ? o[x] : 0;
    above += __popcll(__ballot(v > s));
    ties += __popcll(__ballot(v == s));
  }
  if (lane == 0) { w.row_cnt[R] = above; w.row_tie[R] = ties; }
}

// row_tie[R]: ties of the image before row R; row_cnt[R] += the ties of the row that stay
__global__ __launch_bounds__(256) void k_feat_tie_scan(feat_dev w) {
  __shared__ int part[4];
  const int img = blockIdx.x;
  const int s = w.cut[2 * img], quota = w.cut[2 * img + 1];
  if (s == 0) return;
  const feat_image m = w.table[img];
  int carry = 0;
  for (int base = 0; base < m.rows; base += 256) {
    const int r = base + threadIdx.x;
    const int ties = r < m.rows ? w.row_tie[m.row0 + r] : 0;
    int total;
    const int before = carry + block_exclusive_scan<256, int>(ties, part, &total);
    if (r < m.rows) {
      w.row_tie[m.row0 + r] = before;
      w.row_cnt[m.row0 + r] += min(max(quota - before, 0), ties);
    }
    carry += total;
  }
}

// One workgroup walks the row list in pieces of 4096 (4 rows per thread) with a running carry: the list has one entry per
// image row (tens of thousands for a data set), a few pieces.  Then kp_ptr[i] = row_off[first row of image i].
__global__ __launch_bounds__(1024) void k_feat_scan(feat_dev w, int n_img, int n_rows, int64_t* __restrict__ kp_ptr) {
  __shared__ int part[16];
  int carry = 0;
  for (int base = 0; base < n_rows; base += 4096) {
    const int r = base + 4 * threadIdx.x;
    int c[4], sum = 0;
    for (int k = 0; k < 4; ++k) { c[k] = r + k < n_rows ? w.row_cnt[r + k] : 0; sum += c[k]; }
    int total;
    int at = carry + block_exclusive_scan<1024, int>(sum, part, &total);
    for (int k = 0; k < 4; ++k) {
      if (r + k < n_rows) w.row_off[r + k] = at;
      at += c[k];
    }
    carry += total;
  }
  if (threadIdx.x == 0) w.row_off[n_rows] = carry;
  __syncthreads();                        // the row_off values this workgroup wrote are visible to all of its threads
  for (int i = threadIdx.x; i <= n_img; i += 1024)
    kp_ptr[i] = i < n_img ? (int64_t)w.row_off[w.table[i].row0] : (int64_t)carry;
}

// ---------------------------------------------------------------------------------------------------- scatter
__global__ __launch_bounds__(256) void k_feat_scatter(feat_dev w, int n_img, int n_rows, int64_t n_kp,
                                                      int32_t* __restrict__ xy, uint8_t* __restrict__ score) {
  const int R = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (R >= n_rows) return;
  const int img = row_image(w.table, n_img, R);
  const feat_image m = w.table[img];
  const int y = R - m.row0;
  const int edge = max(w.hdr[0], FEAT_EDGE_MIN);      // as detect left it; never below the smallest gate
  if (y < edge || y >= m.h - edge) return;
  const int s = w.cut[2 * img], quota = w.cut[2 * img + 1];
  const uint8_t* o = w.nms + m.off + (int64_t)y * m.w;
  int64_t at = w.row_off[R];
  int tie_at = w.row_tie[R];
  for (int x0 = edge; x0 < m.w - edge; x0 += 64) {
    const int x = x0 + lane;
    const int v = x < m.w - edge ? o[x] : 0;
    const bool tie = v > 0 && v == s;
    const unsigned long long tb = __ballot(tie);
    const bool keep = v > s || (tie && tie_at + popc_below(tb) < quota);
    const unsigned long long kb = __ballot(keep);
    const int64_t p = at + popc_below(kb);
    if (keep && p < n_kp) {
      xy[2 * p] = x;
      xy[2 * p + 1] = y;
      score[p] = (uint8_t)v;
    }
    at += __popcll(kb);
    tie_at += __popcll(tb);
  }
}

// ------------------------------------------------------------------------------------------------------- blur
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

__global__ __launch_bounds__(256) void k_feat_blur(feat_dev w, int n_img, const uint8_t* __restrict__ images) {
  __shared__ uint8_t in[BLUR_IN_H * BLUR_IN_W];
  __shared__ uint16_t mid[BLUR_IN_H * FEAT_TILE_W];
  const feat_image* T = w.table;
  const int img = table_find(n_img, (int)blockIdx.x, [&](int i) { return T[i].blur_tile0; });
  const feat_image m = T[img];
  const int t = (int)blockIdx.x - m.blur_tile0;
  const int tx0 = (t % m.blur_tiles_x) * FEAT_TILE_W, ty0 = (t / m.blur_tiles_x) * FEAT_BLUR_TILE_H;
  const uint8_t* src = images + m.off;
  for (int i = threadIdx.x; i < BLUR_IN_H * BLUR_IN_W; i += 256) {
    const int r = i / BLUR_IN_W, c = i % BLUR_IN_W;
    // columns and rows past the image are not used by any output of this tile; reflecting them keeps the read inside
    const int gy = reflect101(min(ty0 - 3 + r, m.h + 2), m.h), gx = reflect101(min(tx0 - 3 + c, m.w + 2), m.w);
    in[i] = src[(int64_t)gy * m.w + gx];
  }
  __syncthreads();
  constexpr int W0 = FEAT_BLUR_W[0], W1 = FEAT_BLUR_W[1], W2 = FEAT_BLUR_W[2], W3 = FEAT_BLUR_W[3];
  for (int i = threadIdx.x; i < BLUR_IN_H * FEAT_TILE_W; i += 256) {
    const int r = i / FEAT_TILE_W, c = i % FEAT_TILE_W;
    const uint8_t* p = in + r * BLUR_IN_W + c;
    mid[i] = (uint16_t)(W0 * (p[0] + p[6]) + W1 * (p[1] + p[5]) + W2 * (p[2] + p[4]) + W3 * p[3]);
  }
  __syncthreads();
  uint8_t* out = w.raw + m.off;
  const int c = threadIdx.x & (FEAT_TILE_W - 1), x = tx0 + c;
  for (int r = threadIdx.x / FEAT_TILE_W; r < FEAT_BLUR_TILE_H; r += 256 / FEAT_TILE_W) {
    const int y = ty0 + r;
    if (x >= m.w || y >= m.h) continue;
    const uint16_t* p = mid + r * FEAT_TILE_W + c;
    const int v = W0 * (p[0] + p[6 * FEAT_TILE_W]) + W1 * (p[FEAT_TILE_W] + p[5 * FEAT_TILE_W]) +
                  W2 * (p[2 * FEAT_TILE_W] + p[4 * FEAT_TILE_W]) + W3 * p[3 * FEAT_TILE_W];
    out[(int64_t)y * m.w + x] = (uint8_t)((v + 32768) >> 16);
  }
}

// ---------------------------------------------------------------------------------------------------- describe
__device__ __forceinline__ int wave_sum(int v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// One wavefront per keypoint.  The gate (edge >= 16) keeps both patches inside the image.
__global__ __launch_bounds__(256) void k_feat_describe(feat_dev w, int n_img, const uint8_t* __restrict__ images,
                                                       const int64_t* __restrict__ kp_ptr, int64_t n_kp,
                                                       const int32_t* __restrict__ xy, const int8_t* __restrict__ rot,
                                                       uint8_t* __restrict__ angle_bin, uint8_t* __restrict__ desc) {
  __shared__ uint8_t soft[4][33 * 33 + 3];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = min((int64_t)blockIdx.x * 4 + wv, n_kp - 1);      // a wavefront past the end repeats the last keypoint
  int lo = 0, hi = n_img;                         // the image of keypoint k: largest i with kp_ptr[i] <= k
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (kp_ptr[mid] <= k) lo = mid; else hi = mid;
  }
  const feat_image m = w.table[lo];
  const int x = xy[2 * k], y = xy[2 * k + 1];
  const bool inside = x >= 16 && y >= 16 && x < m.w - 16 && y < m.h - 16;      // always, for the output of k_feat_scatter
  const uint8_t* src = images + m.off;
  const uint8_t* blr = w.raw + m.off;
  int m10 = 0, m01 = 0;
  // the 31 x 31 unblurred patch is used once, for the moments: it goes through registers.  The 33 x 33 blurred patch is
  // gathered from 512 times: it is staged in LDS, rows of 33 bytes read by adjacent lanes.
  for (int i = lane; i < 31 * 31 && inside; i += 64) {
    const int dy = i / 31 - 15, dx = i % 31 - 15;
    const int v = src[(int64_t)(y + dy) * m.w + (x + dx)];
    if (dx * dx + dy * dy <= 225) { m10 += dx * v; m01 += dy * v; }
  }
  for (int i = lane; i < 33 * 33; i += 64) {
    const int dy = i / 33 - 16, dx = i % 33 - 16;
    soft[wv][i] = inside ? blr[(int64_t)(y + dy) * m.w + (x + dx)] : (uint8_t)0;
  }
  m10 = wave_sum(m10);
  m01 = wave_sum(m01);
  const double a = (m10 == 0 && m01 == 0) ? 0.0 : atan2((double)m01, (double)m10);
  const int q = (int)floor(a * 15.0 / 3.14159265358979323846 + 0.5);
  const int bin = ((q % FEAT_BINS) + FEAT_BINS) % FEAT_BINS;
  __syncthreads();
  const int32_t* table = (const int32_t*)(rot + (int64_t)bin * FEAT_PAIRS * 4);      // one pair = four int8 = one dword
  unsigned long long bits[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int32_t p = table[64 * j + lane];       // bit 64 j + lane: the ballot puts it at byte (64 j + lane) / 8, bit % 8
    const int ax = (int8_t)p, ay = (int8_t)(p >> 8), bx = (int8_t)(p >> 16), by = (int8_t)(p >> 24);
    const int va = soft[wv][(ay + 16) * 33 + (ax + 16)], vb = soft[wv][(by + 16) * 33 + (bx + 16)];
    bits[j] = __ballot(va < vb);
  }
  if (lane < 4) {
    const unsigned long long mine = lane == 0 ? bits[0] : lane == 1 ? bits[1] : lane == 2 ? bits[2] : bits[3];
    *(unsigned long long*)(desc + k * 32 + 8 * lane) = mine;
  }
  if (lane == 0) angle_bin[k] = (uint8_t)bin;
}

feat_dev feat_carve(void* workspace, const feat_layout& L) {
  char* p = (char*)workspace;
  feat_dev w;
  w.table = (const feat_image*)(p + L.table);
  w.raw = (uint8_t*)(p + L.raw);
  w.nms = (uint8_t*)(p + L.nms);
  w.row_cnt = (int*)(p + L.row_cnt); w.row_off = (int*)(p + L.row_off); w.row_tie = (int*)(p + L.row_tie);
  w.hist = (unsigned*)(p + L.hist);
  w.cut = (int*)(p + L.cut);
  w.hdr = (int*)(p + L.hdr);
  return w;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_orb_default_pattern(int8_t base[256][4]) {
  if (!base) return SFM_ERR_ARG;
  feat_default_pattern(base);
  return SFM_OK;
}

extern "C" int sfm_orb_rotate_pattern(const int8_t base[256][4], int8_t rot[30][256][4]) {
  if (!base || !rot) return SFM_ERR_ARG;
  return feat_rotate_pattern(base, rot) ? SFM_OK : SFM_ERR_ARG;
}

extern "C" int sfm_features_workspace_bytes(int32_t n_img, const int64_t* img_off_host, int64_t* bytes_host) {
  if (!bytes_host || feat_check_offsets(n_img, img_off_host)) return SFM_ERR_ARG;
  *bytes_host = feat_plan_layout(n_img, n_img > 0 ? img_off_host[n_img] : 0).bytes;
  return SFM_OK;
}

extern "C" int sfm_features_detect(sfm_handle h, const uint8_t* images, const uint8_t* masks, const int64_t* img_off,
                                   const int32_t* heights, const int32_t* widths, int32_t n_img, int32_t threshold,
                                   int32_t edge, int32_t max_features, int64_t* kp_ptr, void* workspace,
                                   int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  int why = feat_check_options(threshold, edge, max_features);
  if (!why) why = feat_check_images(n_img, img_off, heights, widths);
  if (why) return sfm_fail(h, SFM_ERR_ARG, "sfm_features_detect", feat_rule_text(why));
  if (!kp_ptr) return sfm_fail(h, SFM_ERR_ARG, "sfm_features_detect", "null pointer");
  const feat_plan P = feat_plan_images(n_img, img_off, heights, widths);
  const feat_layout L = feat_plan_layout(n_img, P.pixels);
  if (n_img > 0 && (!workspace || workspace_bytes < L.bytes))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_features_detect", "workspace too small");
  if (P.pixels > 0 && !images) return sfm_fail(h, SFM_ERR_ARG, "sfm_features_detect", "null pointer");
  if (n_img == 0) {
    SFM_HIP(h, hipMemsetAsync(kp_ptr, 0, sizeof(int64_t), h->stream));
    return SFM_OK;
  }
  const feat_dev w = feat_carve(workspace, L);
  const int n_rows = (int)P.rows;
  SFM_HIP(h, hipMemcpyAsync((void*)w.table, P.img.data(), (size_t)n_img * sizeof(feat_image), hipMemcpyHostToDevice, h->stream));
  SFM_HIP(h, hipMemsetAsync(w.hist, 0, (size_t)n_img * 256 * sizeof(unsigned), h->stream));
  if (P.score_tiles > 0) {
    sfm_prof_begin(h, SFM_PROF_FEAT_SCORE);
    hipLaunchKernelGGL(k_feat_score, dim3((unsigned)P.score_tiles), dim3(256), 0, h->stream, w, (int)n_img, images, (int)threshold);
    sfm_prof_end(h, SFM_PROF_FEAT_SCORE);
  }
  sfm_prof_begin(h, SFM_PROF_FEAT_SELECT);
  if (n_rows > 0)
    hipLaunchKernelGGL(k_feat_nms, dim3(cdiv(n_rows, 4)), dim3(256), 0, h->stream, w, (int)n_img, n_rows, masks, (int)edge,
                       max_features > 0 ? 1 : 0);
  hipLaunchKernelGGL(k_feat_cut, dim3(cdiv(n_img, 64)), dim3(64), 0, h->stream, w, (int)n_img, (int)max_features,
                     (int)edge);
  if (max_features > 0 && n_rows > 0) {
    hipLaunchKernelGGL(k_feat_ties, dim3(cdiv(n_rows, 4)), dim3(256), 0, h->stream, w, (int)n_img, n_rows, (int)edge);
    hipLaunchKernelGGL(k_feat_tie_scan, dim3((unsigned)n_img), dim3(256), 0, h->stream, w);
  }
  hipLaunchKernelGGL(k_feat_scan, dim3(1), dim3(1024), 0, h->stream, w, (int)n_img, n_rows, kp_ptr);
  sfm_prof_end(h, SFM_PROF_FEAT_SELECT);
  SFM_LAUNCH_CHECK(h, "sfm_features_detect");
  return SFM_OK;
}

extern "C" int sfm_features_describe(sfm_handle h, const uint8_t* images, const int64_t* img_off, const int32_t* heights,
                                     const int32_t* widths, int32_t n_img, const int64_t* kp_ptr, int64_t n_kp,
                                     const int8_t* rot_pattern, int32_t* xy, uint8_t* score, uint8_t* angle_bin,
                                     uint8_t* desc, uint8_t* blurred_out, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const int why = feat_check_images(n_img, img_off, heights, widths);
  if (why) return sfm_fail(h, SFM_ERR_ARG, "sfm_features_describe", feat_rule_text(why));
  if (n_kp < 0 || n_kp >= ((int64_t)1 << 31)) return sfm_fail(h, SFM_ERR_ARG, "sfm_features_describe", "n_kp out of range");
  const feat_plan P = feat_plan_images(n_img, img_off, heights, widths);
  const feat_layout L = feat_plan_layout(n_img, P.pixels);
  if (n_img > 0 && (!workspace || workspace_bytes < L.bytes))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_features_describe", "workspace too small");
  if (n_kp > 0 && (!images || !kp_ptr || !rot_pattern || !xy || !score || !angle_bin || !desc || n_img == 0))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_features_describe", "null pointer");
  if (P.pixels > 0 && blurred_out && !images) return sfm_fail(h, SFM_ERR_ARG, "sfm_features_describe", "null pointer");
  if (n_kp == 0 && !blurred_out) return SFM_OK;
  if (n_img == 0) return SFM_OK;
  const feat_dev w = feat_carve(workspace, L);
  const int n_rows = (int)P.rows;
  if (n_kp > 0 && n_rows > 0) {
    sfm_prof_begin(h, SFM_PROF_FEAT_SCATTER);
    hipLaunchKernelGGL(k_feat_scatter, dim3(cdiv(n_rows, 4)), dim3(256), 0, h->stream, w, (int)n_img, n_rows, n_kp, xy, score);
    sfm_prof_end(h, SFM_PROF_FEAT_SCATTER);
  }
  if (P.blur_tiles > 0) {
    sfm_prof_begin(h, SFM_PROF_FEAT_BLUR);
    hipLaunchKernelGGL(k_feat_blur, dim3((unsigned)P.blur_tiles), dim3(256), 0, h->stream, w, (int)n_img, images);
    sfm_prof_end(h, SFM_PROF_FEAT_BLUR);
    if (blurred_out)
      SFM_HIP(h, hipMemcpyAsync(blurred_out, w.raw, (size_t)P.pixels, hipMemcpyDeviceToDevice, h->stream));
  }
  if (n_kp > 0) {
    sfm_prof_begin(h, SFM_PROF_FEAT_DESCRIBE);
    hipLaunchKernelGGL(k_feat_describe, dim3(cdiv(n_kp, 4)), dim3(256), 0, h->stream, w, (int)n_img, images, kp_ptr, n_kp,
                       (const int32_t*)xy, rot_pattern, angle_bin, desc);
    sfm_prof_end(h, SFM_PROF_FEAT_DESCRIBE);
  }
  SFM_LAUNCH_CHECK(h, "sfm_features_describe");
  return SFM_OK;
}
