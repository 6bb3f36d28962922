// The launch plan of ragged ensembles (csrc/ragged_plan.h) checked on its own, on the host: a stand-alone program for a
// sanitizer build.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ragged_plan_check.cpp -o ragged_plan_check
//   ./ragged_plan_check
//
// It lays out the plan and the work-item table of (a) the sizes at every boundary of a lane split and of a launch class, three
// times over in a seeded shuffle, (b) 10^5 worlds of seeded random sizes, (c) one world of 1 body, one of 4096, and equal sizes,
// and checks that every (world, tile) is exactly one item, that a world's items are contiguous in its launch with the right row0
// and size, that a launch holds one class under the LDS of its largest member, and that invalid sizes are refused with nothing
// written — all of it once under the f32 LDS function (ensemble_lds_bytes, the plan's default) and once under the f64 one
// (ensemble64_lds_bytes), whose six class caps must come out as 2 560 .. 81 920 B.  Exit status 0 and "ok" when all of it holds.
// A tool, not a test: nothing here touches a device.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../nbody-simulation_amd/csrc/ragged_plan.h"

using namespace nbody;

static int g_failed = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      ++g_failed;                                                         \
    }                                                                     \
  } while (0)

static RaggedLdsFn g_lds = ensemble_lds_bytes;  // the precision under check
static const char* g_precision = "f32";

static void check(const std::vector<int64_t>& sizes, const char* what) {
  const int64_t b = (int64_t)sizes.size();
  RaggedPlan plan;
  std::vector<int32_t> launch((size_t)b, -1);
  std::vector<int64_t> first((size_t)b, -1);
  EXPECT(ragged_plan(b, sizes.data(), &plan, launch.data(), first.data(), g_lds) == kRaggedOk);
  if (g_lds == ensemble_lds_bytes) {  // the default is the f32 plan, field for field
    RaggedPlan dflt;
    EXPECT(ragged_plan(b, sizes.data(), &dflt, nullptr, nullptr) == kRaggedOk && dflt.n_launches == plan.n_launches);
    for (int l = 0; l < kRaggedMaxLaunches; ++l) EXPECT(dflt.lds_bytes[l] == plan.lds_bytes[l] && dflt.blocks[l] == plan.blocks[l]);
  }
  EXPECT(plan.n_launches >= 1 && plan.n_launches <= kRaggedMaxLaunches);
  std::vector<RaggedItem> items((size_t)plan.total_blocks);
  int64_t first_item[kRaggedMaxLaunches];
  ragged_items(b, sizes.data(), plan, items.data(), first_item);

  int64_t rows = 0, blocks = 0;
  int max_n[kRaggedMaxLaunches] = {}, cls_of[kRaggedMaxLaunches] = {-1, -1, -1, -1, -1, -1};
  std::vector<char> seen(items.size(), 0);
  for (int64_t k = 0; k < b; ++k) {
    const int n = (int)sizes[(size_t)k], l = launch[(size_t)k], tiles = ragged_tiles(n);
    EXPECT(l >= 0 && l < plan.n_launches);
    EXPECT(first[(size_t)k] >= 0 && first[(size_t)k] + tiles <= plan.blocks[l]);
    if (cls_of[l] < 0) cls_of[l] = ragged_class(n);
    EXPECT(cls_of[l] == ragged_class(n));
    if (n > max_n[l]) max_n[l] = n;
    for (int t = 0; t < tiles; ++t) {
      const size_t at = (size_t)(first_item[l] + first[(size_t)k] + t);
      EXPECT(at < items.size());
      if (at >= items.size()) continue;
      EXPECT(!seen[at]);
      seen[at] = 1;
      EXPECT(items[at].row0 == (uint32_t)rows && (items[at].n_tile & 0xffffu) == (uint32_t)n && (items[at].n_tile >> 16) == (uint32_t)t);
    }
    EXPECT((int64_t)tiles * (kEnsembleBlock / ensemble_split(n)) >= n && tiles <= 16);
    rows += n;
    blocks += tiles;
  }
  for (size_t i = 0; i < seen.size(); ++i) EXPECT(seen[i]);
  EXPECT(rows == plan.rows && blocks == plan.total_blocks);
  int64_t sum = 0;
  for (int l = 0; l < kRaggedMaxLaunches; ++l) {
    if (l < plan.n_launches) {
      EXPECT(plan.lds_bytes[l] == (int32_t)g_lds(max_n[l]) && first_item[l] == sum);
      for (int64_t k = 0; k < b; ++k) EXPECT(launch[(size_t)k] != l || (size_t)plan.lds_bytes[l] >= g_lds((int)sizes[(size_t)k]));
      EXPECT(l == 0 || cls_of[l] > cls_of[l - 1]);
      sum += plan.blocks[l];
    } else {
      EXPECT(plan.lds_bytes[l] == 0 && plan.blocks[l] == 0);
    }
  }
  EXPECT(sum == plan.total_blocks);
  std::printf("%-28s %s %8lld worlds %10lld rows %9lld blocks %d launches\n", what, g_precision, (long long)b, (long long)rows, (long long)blocks, plan.n_launches);
}

static void check_all();

int main() {
  check_all();
  g_lds = ensemble64_lds_bytes;
  g_precision = "f64";
  check_all();
  // the f64 class caps, and either side of the 64 KiB dynamic-LDS limit
  const int64_t caps[] = {128, 256, 512, 1024, 2048, 4096};
  const int32_t want[] = {2560, 5120, 10240, 20480, 40960, 81920};
  RaggedPlan plan;
  EXPECT(ragged_plan(6, caps, &plan, nullptr, nullptr, ensemble64_lds_bytes) == kRaggedOk && plan.n_launches == 6);
  for (int l = 0; l < 6; ++l) EXPECT(plan.lds_bytes[l] == want[l]);
  EXPECT(ensemble64_lds_bytes(3272) == 65440 && ensemble64_lds_bytes(3273) == 65600 && ensemble64_lds_bytes(1) == 160);
  std::puts(g_failed ? "FAILED" : "ok");
  return g_failed ? 1 : 0;
}

static void check_all() {
  const int64_t edge[] = {1, 2, 3, 7, 12, 24, 50, 100, 128, 129, 256, 257, 300, 512, 513, 1000, 1024, 1025, 2048, 2049, 4096};
  std::mt19937_64 rng(20261019);
  std::vector<int64_t> sizes;
  for (int r = 0; r < 3; ++r) sizes.insert(sizes.end(), std::begin(edge), std::end(edge));
  for (size_t i = sizes.size(); i > 1; --i) std::swap(sizes[i - 1], sizes[(size_t)(rng() % i)]);
  check(sizes, "boundary sizes, shuffled");

  sizes.clear();
  for (int k = 0; k < 100000; ++k) sizes.push_back(1 + (int64_t)(rng() % 4096));  // ~2^27.6 rows would be too many: see below
  int64_t rows = 0;
  size_t keep = 0;
  while (keep < sizes.size() && rows + sizes[keep] <= kEnsembleMaxRows) rows += sizes[keep++];
  {
    RaggedPlan untouched;
    std::vector<int32_t> launch(sizes.size(), -7);
    EXPECT(keep == sizes.size() || ragged_plan((int64_t)sizes.size(), sizes.data(), &untouched, launch.data(), nullptr, g_lds) == kRaggedTooManyRows);
    EXPECT(untouched.n_launches == 0 && launch[0] == -7);
  }
  sizes.resize(keep);  // the longest prefix within 2^26 rows
  check(sizes, "random sizes 1 .. 4096");
  sizes.clear();
  for (int k = 0; k < 100000; ++k) sizes.push_back(1 + (int64_t)(rng() % 600));
  check(sizes, "10^5 random sizes 1 .. 600");

  check({1}, "one body");
  check({4096}, "4096 bodies");
  check(std::vector<int64_t>(5, 300), "5 x 300");
  check(std::vector<int64_t>((size_t)1 << 14, 4096), "2^14 x 4096 (2^26 rows)");

  RaggedPlan plan;
  const int64_t zero[] = {5, 0}, big[] = {4097}, neg[] = {-3};
  EXPECT(ragged_plan(2, zero, &plan, nullptr, nullptr, g_lds) == kRaggedBadSize);
  EXPECT(ragged_plan(1, big, &plan, nullptr, nullptr, g_lds) == kRaggedBadSize);
  EXPECT(ragged_plan(1, neg, &plan, nullptr, nullptr, g_lds) == kRaggedBadSize);
  EXPECT(ragged_plan(0, zero, &plan, nullptr, nullptr, g_lds) == kRaggedNoWorld);
  EXPECT(ragged_plan(1, nullptr, &plan, nullptr, nullptr, g_lds) == kRaggedNoWorld);
  EXPECT(plan.n_launches == 0 && plan.rows == 0);
  EXPECT(ragged_plan(1, big + 0, nullptr, nullptr, nullptr, g_lds) == kRaggedBadSize && ragged_plan(2, edge, nullptr, nullptr, nullptr, g_lds) == kRaggedOk);
}
