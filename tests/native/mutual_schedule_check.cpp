// The mutual main pass's schedule (csrc/mutual_schedule.h), enumerated on the CPU exactly as direct_mutual.hip runs it:
//   1. a diagonal item: lane by lane and step by step, every ordered pair of couples of the slice is summed exactly once (a mutual
//      evaluation serves both orders, a one-sided one the target's), and the eight waves run the same number of steps;
//   2. for every slice count up to the 2^22-body bound: the units cover every slice pair s < b once and every diagonal once,
//      and cut into strips of whole rounds they take ceil(units / CUs) rounds (32 at 2^20 bodies on 256 CUs).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../nbody-simulation_amd/csrc/mutual_schedule.h"

using namespace nbody::mutual_schedule;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("MISMATCH %s:%d %s\n", __FILE__, __LINE__, #c); \
      if (++fails > 20) return;                                   \
    }                                                             \
  } while (0)

static void check_diagonal() {
  const int kCouples = 4096;  // a slice of 8192 bodies in couples
  std::vector<uint8_t> cnt((size_t)kCouples * kCouples, 0);
  int steps[8] = {0};
  for (int w = 0; w < 8; ++w)
    for (int p = 0; p < kDiagPhases; ++p) {
      const int u = diag_block(w, p), r0 = diag_first_step(w, p), n = diag_steps(p);
      for (int j = 0; j < 8; ++j) {
        for (int i = 0; i < n; ++i) {
          const int r = r0 + i;
          const bool one = diag_one_sided(p, i);
          for (int a = 0; a < 64; ++a)
            for (int k = 0; k < 8; ++k) {
              const int t = 512 * w + 8 * a + k, s = 512 * u + 8 * ((a - r) & 63) + j;
              ++cnt[(size_t)t * kCouples + s];  // the target side: t receives from s
              if (!one) ++cnt[(size_t)s * kCouples + t];
            }
        }
        steps[w] += n;
      }
    }
  for (int w = 0; w < 8; ++w) CHECK(steps[w] == 2056);
  for (size_t q = 0; q < cnt.size(); ++q) {
    CHECK(cnt[q] == 1);
    if (fails) return;
  }
}

static void check_units() {
  for (int nb = 1; nb <= 512; ++nb) {
    std::vector<uint8_t> seen((size_t)nb * nb, 0);
    const int64_t U = units(nb);
    for (int64_t q = 0; q < U; ++q) {
      int s, b;
      unit_slices(q, nb, s, b);
      CHECK(0 <= s && s <= b && b < nb);
      if (s < b) {
        CHECK(item_of(s, b, nb) == q);
        ++seen[(size_t)s * nb + b];
      } else {
        CHECK(diag_unit(s, nb) == q && s % 2 == 0);
        ++seen[(size_t)s * nb + s];
        if (s + 1 < nb) {
          CHECK(diag_unit(s + 1, nb) == q);
          ++seen[(size_t)(s + 1) * nb + s + 1];
        }
      }
    }
    for (int s = 0; s < nb; ++s)
      for (int b = s; b < nb; ++b) CHECK(seen[(size_t)s * nb + b] == 1);
    for (int cus : {32, 80, 104, 255, 256}) {
      const int S = strip_units(cus, 256);
      CHECK(S % cus == 0 && S <= 256);
      int64_t rounds = 0;
      for (int64_t lo = 0; lo < U; lo += S) rounds += ((U - lo < S ? U - lo : S) + cus - 1) / cus;
      CHECK(rounds == (U + cus - 1) / cus);
    }
    if (fails) return;
  }
  CHECK(units(128) == 32 * 256);
}

int main() {
  check_diagonal();
  check_units();
  std::printf(fails ? "FAILED\n" : "OK\n");
  return fails ? 1 : 0;
}
