// The tracers' launch plan of ragged restricted ensembles (csrc/rr_plan.h) checked on its own, on the host: a stand-alone
// program for a sanitizer build.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rr_plan_check.cpp -o rr_plan_check
//   ./rr_plan_check
//
// It lays out the plan and the work-item table of (a) the sizes at every boundary of a launch class crossed with the tracer
// counts at every boundary of a tile (0, 1, 511, 512, 513, 1025, ...), in a seeded shuffle, (b) 10^5 worlds of seeded random
// sizes and counts, a third of them without tracers, (c) worlds that are all without tracers, one world, 2^26 tracers in one
// world and in 2^26 / 512 worlds, and checks that every tracer row is in exactly one item, that a world's items are contiguous in
// its launch with ascending tracer_row0 and count and the world's body_row0 and n, that a launch holds one class under the LDS of
// the largest of its worlds that have tracers, that a world without tracers has launch -1 and block -1 and no item, and that
// invalid sizes or counts are refused with nothing written.  Every case runs under both LDS functions the plan is used with:
// ensemble_lds_bytes (nbody_rr_*) and ensemble64_lds_bytes (nbody_rr64_*), the latter also with the worlds on either side of
// 64 KB of LDS (3272 / 3273 bodies).  Exit status 0 and "ok" when all of it holds.
// A tool, not a test: nothing here touches a device.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../nbody-simulation_amd/csrc/rr_plan.h"

using namespace nbody;

static int g_failed = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      ++g_failed;                                                         \
    }                                                                     \
  } while (0)

struct Precision {
  const char* name;
  RaggedLdsFn lds;
};
static const Precision kPrecisions[] = {{"f32", ensemble_lds_bytes}, {"f64", ensemble64_lds_bytes}};

static void check(const std::vector<int64_t>& sizes, const std::vector<int64_t>& counts, const char* what, const Precision& pr) {
  const int64_t b = (int64_t)sizes.size();
  EXPECT(counts.size() == sizes.size());
  RrPlan plan;
  std::vector<int32_t> launch((size_t)b, -7);
  std::vector<int64_t> first((size_t)b, -7);
  EXPECT(rr_plan(b, sizes.data(), counts.data(), &plan, launch.data(), first.data(), pr.lds) == kRaggedOk);
  EXPECT(plan.n_launches >= 0 && plan.n_launches <= kRaggedMaxLaunches);
  std::vector<RrItem> items((size_t)plan.total_blocks);
  int64_t first_item[kRaggedMaxLaunches];
  rr_items(b, sizes.data(), counts.data(), plan, items.data(), first_item);

  int64_t body_rows = 0, tracer_rows = 0, blocks = 0;
  int max_n[kRaggedMaxLaunches] = {}, cls_of[kRaggedMaxLaunches] = {-1, -1, -1, -1, -1, -1};
  int64_t next_in[kRaggedMaxLaunches] = {};
  std::vector<char> seen(items.size(), 0);
  for (int64_t k = 0; k < b; ++k) {
    const int n = (int)sizes[(size_t)k];
    const int64_t m = counts[(size_t)k], tiles = rr_tiles(m);
    const int l = launch[(size_t)k];
    if (!m) {
      EXPECT(l == -1 && first[(size_t)k] == -1 && tiles == 0);
    } else {
      EXPECT(l >= 0 && l < plan.n_launches);
      if (l < 0 || l >= plan.n_launches) continue;
      EXPECT(first[(size_t)k] == next_in[l]);  // worlds follow one another in world order, without gaps
      EXPECT(first[(size_t)k] + tiles <= plan.blocks[l]);
      next_in[l] += tiles;
      if (cls_of[l] < 0) cls_of[l] = ragged_class(n);
      EXPECT(cls_of[l] == ragged_class(n));
      if (n > max_n[l]) max_n[l] = n;
      int64_t covered = 0;
      for (int64_t t = 0; t < tiles; ++t) {
        const size_t at = (size_t)(first_item[l] + first[(size_t)k] + t);
        EXPECT(at < items.size());
        if (at >= items.size()) continue;
        EXPECT(!seen[at]);
        seen[at] = 1;
        const RrItem& it = items[at];
        EXPECT(it.body_row0 == (uint32_t)body_rows && it.n == (uint32_t)n);
        EXPECT(it.tracer_row0 == (uint32_t)(tracer_rows + covered));  // ascending, no gap, no overlap
        EXPECT(it.count >= 1 && it.count <= (uint32_t)kRrTile && (t + 1 == tiles || it.count == (uint32_t)kRrTile));
        EXPECT((int64_t)it.body_row0 + it.n <= kEnsembleMaxRows && (int64_t)it.tracer_row0 + it.count <= tracer_rows + m);
        covered += it.count;
      }
      EXPECT(covered == m);
    }
    body_rows += n;
    tracer_rows += m;
    blocks += tiles;
  }
  for (size_t i = 0; i < seen.size(); ++i) EXPECT(seen[i]);
  EXPECT(body_rows == plan.body_rows && tracer_rows == plan.tracer_rows && blocks == plan.total_blocks);
  int64_t sum = 0;
  for (int l = 0; l < kRaggedMaxLaunches; ++l) {
    if (l < plan.n_launches) {
      EXPECT(plan.blocks[l] >= 1 && plan.blocks[l] == next_in[l]);
      EXPECT(plan.lds_bytes[l] == (int32_t)pr.lds(max_n[l]) && first_item[l] == sum);
      EXPECT((size_t)plan.lds_bytes[l] <= pr.lds(kEnsembleMaxBodies));
      EXPECT(l == 0 || cls_of[l] > cls_of[l - 1]);
      sum += plan.blocks[l];
    } else {
      EXPECT(plan.lds_bytes[l] == 0 && plan.blocks[l] == 0);
    }
  }
  EXPECT(sum == plan.total_blocks && sum <= kEnsembleMaxRows);
  std::printf("%s %-40s %8lld worlds %10lld rows %10lld tracers %9lld blocks %d launches\n", pr.name, what, (long long)b, (long long)body_rows,
              (long long)tracer_rows, (long long)blocks, plan.n_launches);
}

static void check(const std::vector<int64_t>& sizes, const std::vector<int64_t>& counts, const char* what) {
  for (const Precision& pr : kPrecisions) check(sizes, counts, what, pr);
}

int main() {
  EXPECT(ensemble64_lds_bytes(3272) == 65440 && ensemble64_lds_bytes(3273) == 65600 && ensemble64_lds_bytes(4096) == 81920);
  const int64_t ns[] = {1, 2, 7, 65, 128, 129, 256, 257, 512, 513, 1000, 1024, 1025, 2048, 2049, 3272, 3273, 4096};
  const int64_t ms[] = {0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049};
  std::mt19937_64 rng(20261020);
  std::vector<int64_t> sizes, counts;
  for (int64_t n : ns)
    for (int64_t m : ms) sizes.push_back(n), counts.push_back(m);
  for (size_t i = sizes.size(); i > 1; --i) {
    const size_t j = (size_t)(rng() % i);
    std::swap(sizes[i - 1], sizes[j]);
    std::swap(counts[i - 1], counts[j]);
  }
  check(sizes, counts, "class x tile boundaries, shuffled");

  sizes.clear(), counts.clear();
  for (int k = 0; k < 100000; ++k) {
    sizes.push_back(1 + (int64_t)(rng() % 600));
    counts.push_back(rng() % 3 ? (int64_t)(rng() % 600) : 0);
  }
  check(sizes, counts, "10^5 random sizes and counts");

  // the LDS of a launch is that of the largest world WITH tracers: 200 has none, so the class of 129 .. 256 launches under 150
  check({200, 150, 130}, {0, 5, 700}, "largest member without tracers");
  {
    RrPlan plan;
    const int64_t n3[] = {200, 150, 130}, m3[] = {0, 5, 700};
    EXPECT(rr_plan(3, n3, m3, &plan, nullptr, nullptr) == kRaggedOk && plan.n_launches == 1);
    EXPECT(plan.lds_bytes[0] == (int32_t)ensemble_lds_bytes(150) && plan.blocks[0] == 3);
    EXPECT(rr_plan(3, n3, m3, &plan, nullptr, nullptr, ensemble64_lds_bytes) == kRaggedOk && plan.n_launches == 1);
    EXPECT(plan.lds_bytes[0] == (int32_t)ensemble64_lds_bytes(150) && plan.blocks[0] == 3);
    // f64: the last class on either side of 64 KB, by which of its worlds have tracers
    const int64_t n4[] = {4096, 3273, 3272, 7}, below[] = {0, 0, 513, 1}, above[] = {0, 1, 513, 1};
    EXPECT(rr_plan(4, n4, below, &plan, nullptr, nullptr, ensemble64_lds_bytes) == kRaggedOk && plan.n_launches == 2);
    EXPECT(plan.lds_bytes[0] == 160 && plan.lds_bytes[1] == 65440 && plan.blocks[1] == 2);
    EXPECT(rr_plan(4, n4, above, &plan, nullptr, nullptr, ensemble64_lds_bytes) == kRaggedOk && plan.n_launches == 2);
    EXPECT(plan.lds_bytes[1] == 65600 && plan.blocks[1] == 3);
  }
  check({4096, 3273, 3272, 7}, {0, 1, 513, 1}, "either side of 64 KB in f64");
  check({300, 7, 4096}, {0, 0, 0}, "no tracers at all");
  check({1}, {1}, "one body, one tracer");
  check({4096}, {kEnsembleMaxRows}, "2^26 tracers in one world");
  check(std::vector<int64_t>((size_t)1 << 14, 4096), std::vector<int64_t>((size_t)1 << 14, 4096), "2^14 x (4096 bodies, 4096 tracers)");
  check(std::vector<int64_t>((size_t)1 << 17, 3), std::vector<int64_t>((size_t)1 << 17, 512), "2^17 x (3 bodies, 512 tracers)");

  // refusals: nothing is written
  RrPlan plan;
  int32_t launch[2] = {-7, -7};
  int64_t first[2] = {-7, -7};
  const int64_t ok_n[] = {5, 9}, ok_m[] = {3, 0}, zero[] = {5, 0}, big[] = {4097, 1}, neg[] = {3, -1};
  const int64_t over[] = {kEnsembleMaxRows, 1}, huge[] = {INT64_MAX, INT64_MAX};
  for (const Precision& pr : kPrecisions) {
    launch[0] = launch[1] = -7;
    first[0] = first[1] = -7;
    EXPECT(rr_plan(2, zero, ok_m, &plan, launch, first, pr.lds) == kRaggedBadSize);
    EXPECT(rr_plan(2, big, ok_m, &plan, launch, first, pr.lds) == kRaggedBadSize);
    EXPECT(rr_plan(0, ok_n, ok_m, &plan, launch, first, pr.lds) == kRaggedNoWorld);
    EXPECT(rr_plan(2, nullptr, ok_m, &plan, launch, first, pr.lds) == kRaggedNoWorld);
    EXPECT(rr_plan(2, ok_n, nullptr, &plan, launch, first, pr.lds) == kRrNoCounts);
    EXPECT(rr_plan(2, ok_n, neg, &plan, launch, first, pr.lds) == kRrBadCount);
    EXPECT(rr_plan(2, ok_n, over, &plan, launch, first, pr.lds) == kRrTooManyTracers);
    EXPECT(rr_plan(2, ok_n, huge, &plan, launch, first, pr.lds) == kRrTooManyTracers);  // (no overflow on the way)
    EXPECT(plan.n_launches == 0 && plan.tracer_rows == 0 && plan.body_rows == 0);
    EXPECT(launch[0] == -7 && launch[1] == -7 && first[0] == -7 && first[1] == -7);
    EXPECT(rr_plan(2, ok_n, ok_m, nullptr, launch, first, pr.lds) == kRaggedOk);
    EXPECT(launch[0] == 0 && launch[1] == -1 && first[0] == 0 && first[1] == -1);
  }

  std::puts(g_failed ? "FAILED" : "ok");
  return g_failed ? 1 : 0;
}
