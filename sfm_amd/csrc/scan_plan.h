// The integer side of every compaction ("Compaction"): which counts a thread of a scanning workgroup holds and
// where the first slot of a block is found afterwards.  Plain C++: it compiles for the host too
// (tests/native/scan_plan_check.cpp replays it under the sanitizers); block_scan.h holds the device side.
//
// One-workgroup scan (scan_counts of block_scan.h): thread t of n_threads holds the contiguous run scan_run gives it.
// Two-level scan: a chunk is SCAN_CHUNK consecutive block counts.  Level one, one workgroup of SCAN_THREADS threads per
// chunk, replaces every count by the sum of the counts in front of it within its chunk and hands out the chunk's total;
// thread t holds the SCAN_ITEMS consecutive counts from scan_item(chunk, t, 0).  Level two, ONE workgroup, walks the chunk
// totals in tiles of SCAN_THREADS with a running carry and replaces every total by the sum in front of its chunk.  The
// first slot of block b is then scan_base: its chunk's base plus its own value within the chunk.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SCAN_PLAN_HD __host__ __device__ __forceinline__
#else
#define SCAN_PLAN_HD inline
#endif

#define SCAN_THREADS 256
#define SCAN_ITEMS 4
#define SCAN_CHUNK (SCAN_THREADS * SCAN_ITEMS)

// the run [*beg, *end) of n counts that thread tid of n_threads holds: ceil(n / n_threads) each, the last ones short or
// empty; beg <= end <= n always, and the runs of all threads tile [0, n)
SCAN_PLAN_HD void scan_run(int64_t n, int tid, int n_threads, int64_t* beg, int64_t* end) {
  const int64_t per = (n + n_threads - 1) / n_threads;
  const int64_t b = (int64_t)tid * per, e = b + per;
  *beg = b < n ? b : n;
  *end = e < n ? e : n;
}

SCAN_PLAN_HD int64_t scan_chunks(int64_t n_blocks) { return (n_blocks + SCAN_CHUNK - 1) / SCAN_CHUNK; }
SCAN_PLAN_HD int64_t scan_item(int64_t chunk, int tid, int j) { return chunk * SCAN_CHUNK + (int64_t)tid * SCAN_ITEMS + j; }
// the first slot of block b: chunk_base holds `stride` sums per chunk, this one at `part`; `within` is the block's own
// value after level one
SCAN_PLAN_HD int64_t scan_base(const int64_t* chunk_base, int stride, int part, int64_t b, int64_t within) {
  return chunk_base[stride * (b / SCAN_CHUNK) + part] + within;
}
