// Host build of the fusion's rule and scan plan (sfm_amd/csrc/depth_rule.h, depth_plan.h) for tests/test_depth_fuse_reference.py.
//   depth_fuse_check normal IN OUT   IN: int64 n, then n records of { double d, X[3], dn[4], P[4][3], C[3], jump }
//                                    OUT: n records of { int32 valid; float n[3] }
//   depth_fuse_check fused IN OUT    IN: int64 n, then n records of { double acc[3], nacc[3]; int32 n_views, pad }
//                                    OUT: n records of { double X[3]; float n[3]; int32 pad }
//   depth_fuse_check scan SEED       the two-level scan as the kernels walk it (scan_replay.h: scan_item, chunks, tiles of the top
//                                    level with their carry, depth_scan_base) against a running sum, for block counts
//                                    around the chunk size and above DEPTH_THREADS chunks; pt_ptr from the views of random
//                                    batches; the layout; the parameter checks; prints "ok <cases>"
// Build with -ffp-contract=off (the header's pragma is clang's).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "depth_plan.h"
#include "depth_rule.h"
#include "scan_replay.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct NormalIn { double d, X[3], dn[4], P[4][3], C[3], jump; };
struct NormalOut { int32_t valid; float n[3]; };
struct FusedIn { double acc[3], nacc[3]; int32_t n_views, pad; };
struct FusedOut { double X[3]; float n[3]; int32_t pad; };

template <typename In, typename Out, typename F>
static int run_records(const char* in, const char* out, F f) {
  std::FILE* fi = std::fopen(in, "rb");
  REQUIRE(fi);
  int64_t n = 0;
  REQUIRE(std::fread(&n, 8, 1, fi) == 1 && n >= 0);
  std::vector<In> rec((size_t)n);
  REQUIRE(n == 0 || std::fread(rec.data(), sizeof(In), (size_t)n, fi) == (size_t)n);
  std::fclose(fi);
  std::vector<Out> res((size_t)n);
  for (int64_t i = 0; i < n; ++i) res[(size_t)i] = f(rec[(size_t)i]);
  std::FILE* fo = std::fopen(out, "wb");
  REQUIRE(fo);
  REQUIRE(n == 0 || std::fwrite(res.data(), sizeof(Out), (size_t)n, fo) == (size_t)n);
  std::fclose(fo);
  return 0;
}

static uint64_t rng_state;
static uint64_t rnd() {
  rng_state += 0x9E3779B97F4A7C15ull;
  uint64_t z = rng_state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// k_depth_fuse_scan_chunks and k_depth_fuse_scan_top on the host (the shared replay of scan_replay.h): blk holds the counts
// on entry and the bases within a chunk on return, chunk_base one sum per chunk; returns the grand total
static int64_t fuse_scan(std::vector<uint32_t>& blk, std::vector<int64_t>& chunk_base) {
  scan_replay::chunk_counts(blk, chunk_base);
  return scan_replay::chunk_totals(chunk_base.data(), (int64_t)chunk_base.size(), 1);
}

static int check_scan(uint64_t seed) {
  rng_state = seed;
  int cases = 0;
  const int64_t sizes[] = {0, 1, 2, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 3 * SCAN_CHUNK + 7,
                           (int64_t)DEPTH_THREADS * SCAN_CHUNK + 5, (int64_t)(DEPTH_THREADS + 1) * SCAN_CHUNK + 1};
  for (int64_t nb : sizes) {
    for (int full = 0; full < 2; ++full) {
      std::vector<uint32_t> blk((size_t)nb), counts;
      for (auto& c : blk) c = full ? DEPTH_PIXEL_BLOCK : (uint32_t)(rnd() % (DEPTH_PIXEL_BLOCK + 1));
      counts = blk;
      std::vector<int64_t> chunk_base;
      const int64_t total = fuse_scan(blk, chunk_base);
      int64_t run = 0;
      for (int64_t b = 0; b < nb; ++b) {
        REQUIRE(depth_scan_base(chunk_base.data(), blk.data(), b) == run);
        run += counts[(size_t)b];
      }
      REQUIRE(total == run);
      ++cases;
    }
  }
  // pt_ptr of random batches: the base of a view's first block, the grand total where no block follows
  for (int rep = 0; rep < 40; ++rep) {
    const int n_img = 1 + (int)(rnd() % 6);
    std::vector<int64_t> off((size_t)n_img + 1, 0), src_ptr, plane_ptr;
    std::vector<int32_t> hs((size_t)n_img), ws((size_t)n_img), refs;
    for (int i = 0; i < n_img; ++i) {
      const int kind = (int)(rnd() % 5);
      hs[(size_t)i] = kind == 0 ? 0 : 1 + (int)(rnd() % 40);
      ws[(size_t)i] = kind == 1 ? 0 : (kind == 2 ? DEPTH_PIXEL_BLOCK : 1 + (int)(rnd() % 40));
      off[(size_t)i + 1] = off[(size_t)i] + (int64_t)hs[(size_t)i] * ws[(size_t)i] + (int64_t)(rnd() % 3);
    }
    for (int i = n_img - 1; i >= 0; --i) if (rnd() % 4) refs.push_back(i);      // not in image order
    const int n_ref = (int)refs.size();
    src_ptr.assign((size_t)n_ref + 1, 0);
    for (int r = 0; r <= n_ref; ++r) plane_ptr.push_back(r);
    REQUIRE(depth_check_images(n_img, off.data(), hs.data(), ws.data()) == 0);
    REQUIRE(depth_check_views(n_img, n_ref, refs.data(), src_ptr.data(), nullptr, plane_ptr.data(), 0) == 0);
    const DepthPlan p = depth_plan(n_img, off.data(), hs.data(), ws.data(), n_ref, refs.data(), src_ptr.data(), plane_ptr.data());
    REQUIRE(p.n_pix_blocks <= depth_max_pixel_blocks(p.n_out, n_ref));
    std::vector<uint32_t> blk((size_t)p.n_pix_blocks);
    std::vector<int64_t> want((size_t)n_ref + 1, 0), chunk_base;
    for (int r = 0; r < n_ref; ++r) {
      const int64_t n = (int64_t)hs[(size_t)refs[(size_t)r]] * ws[(size_t)refs[(size_t)r]];
      const int64_t first = p.views[(size_t)r].pix_block_first;
      REQUIRE(p.views[(size_t)r + 1].pix_block_first - first == depth_pixel_blocks(n));
      int64_t owners = 0;
      for (int64_t b = 0; b < depth_pixel_blocks(n); ++b) {
        const int64_t in_block = n - b * DEPTH_PIXEL_BLOCK < DEPTH_PIXEL_BLOCK ? n - b * DEPTH_PIXEL_BLOCK : DEPTH_PIXEL_BLOCK;
        blk[(size_t)(first + b)] = (uint32_t)(rnd() % (uint64_t)(in_block + 1));
        owners += blk[(size_t)(first + b)];
      }
      want[(size_t)r + 1] = want[(size_t)r] + owners;
    }
    const int64_t total = fuse_scan(blk, chunk_base);
    for (int r = 0; r <= n_ref; ++r) {
      const int64_t b = p.views[(size_t)r].pix_block_first;
      REQUIRE((b < p.n_pix_blocks ? depth_scan_base(chunk_base.data(), blk.data(), b) : total) == want[(size_t)r]);
    }
    // the layout: the tables of the filter first, then the counts and the chunk bases, nothing overlapping, all inside
    const DepthFuseLayout L = depth_fuse_layout(n_img, n_ref, 0, p.n_pix_blocks);
    const DepthFuseLayout most = depth_fuse_layout(n_img, n_ref, 0, depth_max_pixel_blocks(p.n_out, n_ref));
    REQUIRE(L.blk >= L.tables.bytes && L.blk % 256 == 0 && L.chunk_base % 256 == 0);
    REQUIRE(L.chunk_base >= L.blk + p.n_pix_blocks * 4);
    REQUIRE(L.bytes >= L.chunk_base + scan_chunks(p.n_pix_blocks) * 8 && most.bytes >= L.bytes);
    ++cases;
  }
  const double nan = std::nan("");
  REQUIRE(depth_check_fuse(0.0, 1, 0.0) == 0 && depth_check_fuse(0.02, DEPTH_MAX_NORMAL_STEP, 0.05) == 0);
  REQUIRE(depth_check_fuse(-1e-9, 2, 0.05) == 1 && depth_check_fuse(nan, 2, 0.05) == 1);
  REQUIRE(depth_check_fuse(0.02, 0, 0.05) == 2 && depth_check_fuse(0.02, DEPTH_MAX_NORMAL_STEP + 1, 0.05) == 2 && depth_check_fuse(0.02, -3, 0.05) == 2);
  REQUIRE(depth_check_fuse(0.02, 2, -0.5) == 3 && depth_check_fuse(0.02, 2, nan) == 3);
  REQUIRE(std::strlen(DEPTH_FUSE_WHY[1]) && std::strlen(DEPTH_FUSE_WHY[2]) && std::strlen(DEPTH_FUSE_WHY[3]));
  std::printf("ok %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "normal"))
    return run_records<NormalIn, NormalOut>(argv[2], argv[3], [](const NormalIn& r) {
      NormalOut o;
      o.valid = depth::view_normal(r.d, r.X, r.dn, r.P[0], r.P[1], r.P[2], r.P[3], r.C, r.jump, o.n);
      return o;
    });
  if (argc == 4 && !std::strcmp(argv[1], "fused"))
    return run_records<FusedIn, FusedOut>(argv[2], argv[3], [](const FusedIn& r) {
      FusedOut o;
      for (int i = 0; i < 3; ++i) o.X[i] = depth::fused_mean(r.acc[i], r.n_views);
      depth::fused_normal(r.nacc, o.n);
      o.pad = 0;
      return o;
    });
  if (argc == 3 && !std::strcmp(argv[1], "scan")) return check_scan(std::strtoull(argv[2], nullptr, 10));
  std::fprintf(stderr, "usage: depth_fuse_check normal|fused IN OUT | scan SEED\n");
  return 2;
}
