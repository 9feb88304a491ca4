// The device side of every compaction ("Compaction"): count, scan and rank over one workgroup of whole
// wavefronts, for gfx950.  __device__ functions only; every kernel stays in its stage's source.  scan_plan.h holds the
// integer plan they walk.
//
// The barrier discipline of the scan: barrier, write the wave partials to s_wave, barrier, read them.  The first barrier
// closes the reads of the call before, so block_exclusive_scan and what is built on it may be called again on the same
// s_wave at once and in a loop.  The two flag functions are called once per kernel, on LDS words nothing has touched: they
// write, meet ONE barrier and read, as the count and scatter kernels always did; a second use of their s_wave needs a
// barrier in between.  Every thread of the workgroup must call.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "scan_plan.h"

// exclusive prefix of v over the NT threads of the workgroup, and the workgroup's total; s_wave has NT / 64 elements
template <int NT, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* s_wave, T* total) {
  static_assert(NT % 64 == 0 && NT <= 1024, "a workgroup of whole wavefronts");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const T t = s_wave[w];
    if (w < wave) before += t;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

// the set flags of the workgroup from one ballot per wavefront; s_wave has NT / 64 elements, untouched since the last barrier
template <int NT = 256>
__device__ __forceinline__ int block_flag_count(bool flag, int* s_wave) {
  const unsigned long long word = __ballot(flag);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(word);
  __syncthreads();
  int all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) all += s_wave[w];
  return all;
}

// the set flags of the workgroup in front of this thread, from the same ballots
template <int NT = 256>
__device__ __forceinline__ int block_flag_rank(bool flag, int* s_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long word = __ballot(flag);
  if (lane == 0) s_wave[wave] = __popcll(word);
  __syncthreads();
  int rank = __popcll(word & ((1ull << lane) - 1ull));
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) rank += w < wave ? s_wave[w] : 0;
  return rank;
}

// Exclusive scan of n block counts by ONE workgroup of NT threads: out[i] = the sum of in[0 .. i), *total = the sum of
// all, in every thread.  A thread holds the run scan_run gives it and reads each count before it writes that slot, so out
// may be in (the pair is not __restrict__).  Sums are 64-bit; a base is stored as the int its stage's outputs can hold.
template <int NT>
__device__ __forceinline__ void scan_counts(int n, const int* in, int* out, int64_t* s_wave, int64_t* total) {
  int64_t beg, end;
  scan_run(n, (int)threadIdx.x, NT, &beg, &end);
  int64_t mine = 0;
  for (int64_t i = beg; i < end; ++i) mine += in[i];
  int64_t run = block_exclusive_scan<NT, int64_t>(mine, s_wave, total);
  for (int64_t i = beg; i < end; ++i) {
    const int c = in[i];
    out[i] = (int)run;
    run += c;
  }
}

// Level one of the two-level scan, workgroup blockIdx.x of SCAN_THREADS threads on its chunk: blk[i] becomes the sum of the
// counts in front of it within the chunk; returns the chunk's total.  C is uint32_t, or uint64_t holding two packed 32-bit
// halves whose sums within a chunk both stay below 2^32 (the caller's static_assert): one 64-bit add then scans both.
template <typename C>
__device__ __forceinline__ int64_t scan_chunk_counts(C* blk, int64_t n_blocks, int64_t* s_wave) {
  C c[SCAN_ITEMS];
  int64_t sum = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const int64_t i = scan_item(blockIdx.x, threadIdx.x, j);
    c[j] = i < n_blocks ? blk[i] : (C)0;
    sum += (int64_t)c[j];
  }
  int64_t total;
  int64_t run = block_exclusive_scan<SCAN_THREADS, int64_t>(sum, s_wave, &total);
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const int64_t i = scan_item(blockIdx.x, threadIdx.x, j);
    if (i < n_blocks) blk[i] = (C)run;
    run += (int64_t)c[j];
  }
  return total;
}

// Level two by ONE workgroup of SCAN_THREADS threads: the totals chunk_sum[stride * i], i < n_chunks, walked in tiles with
// a running carry, each replaced by the sum of those in front of it; returns the sum of all, in every thread
__device__ __forceinline__ int64_t scan_chunk_totals(int64_t* chunk_sum, int64_t n_chunks, int stride, int64_t* s_wave) {
  int64_t carry = 0;
  for (int64_t first = 0; first < n_chunks; first += SCAN_THREADS) {
    const int64_t i = first + threadIdx.x;
    const int64_t v = i < n_chunks ? chunk_sum[stride * i] : 0;
    int64_t total;
    const int64_t before = block_exclusive_scan<SCAN_THREADS, int64_t>(v, s_wave, &total);
    if (i < n_chunks) chunk_sum[stride * i] = carry + before;
    carry += total;
  }
  return carry;
}
