// The scans of sfm_amd/csrc/block_scan.h on the host, walked as the kernels walk them: the same functions of scan_plan.h say
// which thread holds which count, the threads run one after the other, and block_exclusive_scan is the running sum over
// the threads in their order.  Shared by scan_plan_check.cpp, depth_fuse_check.cpp and mesh_check.cpp.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scan_plan.h"

#define SCAN_REPLAY_REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

namespace scan_replay {

// scan_counts<n_threads>: out[i] = in[0] + .. + in[i - 1], returns the sum of all; out may be in.  Requires that the runs
// of the threads tile [0, n) in thread order.
inline int64_t counts(int n_threads, int64_t n, const int* in, int* out) {
  std::vector<int64_t> before((size_t)n_threads);
  int64_t next = 0, all = 0;
  for (int tid = 0; tid < n_threads; ++tid) {
    int64_t beg, end;
    scan_run(n, tid, n_threads, &beg, &end);
    SCAN_REPLAY_REQUIRE(beg == next && beg <= end && end <= n);
    next = end;
    before[(size_t)tid] = all;
    for (int64_t i = beg; i < end; ++i) all += in[i];
  }
  SCAN_REPLAY_REQUIRE(next == n);
  for (int tid = 0; tid < n_threads; ++tid) {
    int64_t beg, end, run = before[(size_t)tid];
    scan_run(n, tid, n_threads, &beg, &end);
    for (int64_t i = beg; i < end; ++i) {
      const int c = in[i];                                       // read before the slot is written
      out[i] = (int)run;
      run += c;
    }
  }
  return all;
}

// scan_chunk_counts, one workgroup per chunk: blk holds the counts on entry and the sums in front within the chunk on
// return; chunk_total gets one total per chunk (packed as the counts are).  Requires that every count is in one thread's
// hands, that a uint32 sum stays in 32 bits and that the low half of a packed uint64 sum never carries into the high one.
template <typename C>
inline void chunk_counts(std::vector<C>& blk, std::vector<int64_t>& chunk_total) {
  const int64_t nb = (int64_t)blk.size(), n_chunks = scan_chunks(nb);
  SCAN_REPLAY_REQUIRE(n_chunks * SCAN_CHUNK >= nb && (n_chunks == 0 || (n_chunks - 1) * SCAN_CHUNK < nb));
  chunk_total.assign((size_t)n_chunks, 0);
  std::vector<char> seen((size_t)nb, 0);
  for (int64_t c = 0; c < n_chunks; ++c) {
    uint64_t run = 0;
    for (int tid = 0; tid < SCAN_THREADS; ++tid)
      for (int j = 0; j < SCAN_ITEMS; ++j) {
        const int64_t i = scan_item(c, tid, j);
        SCAN_REPLAY_REQUIRE(i >= c * SCAN_CHUNK && i < (c + 1) * SCAN_CHUNK);
        if (i >= nb) continue;
        SCAN_REPLAY_REQUIRE(!seen[(size_t)i]);
        seen[(size_t)i] = 1;
        const uint64_t count = blk[(size_t)i];
        SCAN_REPLAY_REQUIRE(sizeof(C) == 8 || run <= 0xFFFFFFFFull);
        SCAN_REPLAY_REQUIRE((run & 0xFFFFFFFFull) + (count & 0xFFFFFFFFull) <= 0xFFFFFFFFull || sizeof(C) == 4);
        blk[(size_t)i] = (C)run;
        run += count;
      }
    chunk_total[(size_t)c] = (int64_t)run;
  }
  for (int64_t i = 0; i < nb; ++i) SCAN_REPLAY_REQUIRE(seen[(size_t)i]);
}

// scan_chunk_totals, one workgroup: the totals chunk_sum[stride * i] in tiles of SCAN_THREADS with a carry; returns the sum
inline int64_t chunk_totals(int64_t* chunk_sum, int64_t n_chunks, int stride) {
  int64_t carry = 0;
  for (int64_t first = 0; first < n_chunks; first += SCAN_THREADS) {
    int64_t total = 0;
    for (int tid = 0; tid < SCAN_THREADS; ++tid) {
      const int64_t i = first + tid;
      if (i >= n_chunks) continue;
      const int64_t v = chunk_sum[stride * i];
      chunk_sum[stride * i] = carry + total;
      total += v;
    }
    carry += total;
  }
  return carry;
}

}  // namespace scan_replay
