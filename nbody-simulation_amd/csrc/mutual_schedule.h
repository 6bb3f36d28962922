// The schedule of the mutual main pass (direct_mutual.hip): which slice pairs a unit of work covers, and how a diagonal item
// splits its slice over the eight waves of a work-group.  Plain integer functions, host and device alike, so that the CPU test
// (tests/native/mutual_schedule_check.cpp) enumerates exactly what the kernels run.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NB_HD __host__ __device__
#else
#define NB_HD
#endif

namespace nbody {
namespace mutual_schedule {

// ---- Units: the slice pairs (s, b) with s < b, row by row, then the diagonal items two by two.  A unit costs one off-diagonal
// item: a diagonal item evaluates each unordered pair of its slice once, half an item, and a unit holds two of them (the last
// unit one when the slice count is odd).  At 2^20 bodies (128 slices): 8128 + 64 = 8192 units, 32 rounds of 256 work-groups.
NB_HD inline int64_t off_items(int nb) { return (int64_t)nb * (nb - 1) / 2; }
NB_HD inline int64_t item_of(int s, int b, int nb) { return (int64_t)s * nb - (int64_t)s * (s + 1) / 2 + (b - s - 1); }
NB_HD inline int64_t units(int nb) { return off_items(nb) + (nb + 1) / 2; }
// unit -> (s, b): s < b for an off-diagonal item; s == b for a diagonal unit, whose slices are s and s + 1 (when s + 1 < nb)
NB_HD inline void unit_slices(int64_t unit, int nb, int& s, int& b) {
  const int64_t n_off = off_items(nb);
  if (unit < n_off) {
    s = 0;
    int64_t first = 0;
    while (first + (nb - 1 - s) <= unit) first += nb - 1 - s++;
    b = s + 1 + (int)(unit - first);
  } else {
    s = b = 2 * (int)(unit - n_off);
  }
}
// the diagonal unit of slice s and its half (0: the unit's first slice, 1: its second)
NB_HD inline int64_t diag_unit(int s, int nb) { return off_items(nb) + s / 2; }

// Units per launch: the largest multiple of the CU count that fits the strip area (capacity units), or the capacity itself when
// one round alone exceeds it.  Every strip but the last is then whole rounds, and the pass takes ceil(units / cus) rounds.
NB_HD inline int strip_units(int cus, int capacity) { return cus >= capacity ? capacity : capacity / cus * cus; }

// ---- A diagonal item.  Wave w (of 8) holds the slice's wave block w as targets: couple 512 w + 8 l + k in lane l, k < 8.  Its
// sources come in chunks (u, j) of 64 couples, lane l loading couple 512 u + 8 l + j.  During a chunk the couple moves one lane
// up per step, so at step r lane l pairs its targets with the couple loaded by lane l - r.  The block pairs are taken in five
// phases p, wave w working on block u = w + p (mod 8), eight chunks each:
//   p = 0, its own block: steps 0 .. 32, mutual but for steps 0 and 32, which are one-sided (target side only);
//   p = 1, 2, 3: all 64 steps, mutual (block pairs at distance 1 .. 3 once, from their lower wave mod 8);
//   p = 4, the block pair at distance 4, shared: waves 0 .. 3 take steps 0 .. 31, waves 4 .. 7 steps 1 .. 32.
// Every ordered pair of the slice is then summed exactly once, and every wave runs 8 (33 + 3 x 64 + 32) = 2056 steps, against
// 4096 for an off-diagonal item.  In phase p every block receives source sums from one wave only (w = u - p).
constexpr int kDiagPhases = 5;
NB_HD inline int diag_block(int w, int p) { return (w + p) & 7; }
NB_HD inline int diag_first_step(int w, int p) { return p == 4 && w >= 4 ? 1 : 0; }
NB_HD inline int diag_steps(int p) { return p == 0 ? 33 : p == 4 ? 32 : 64; }
// step index i of diag_steps(p) in the chunk: one-sided (target side only)?
NB_HD inline bool diag_one_sided(int p, int i) { return p == 0 && (i == 0 || i == 32); }

}  // namespace mutual_schedule
}  // namespace nbody

#undef NB_HD
