// A sequential floating-point sum, evaluated in parallel without changing one bit of it.  One text for f32 and f64.
//
// BVHTree::from folds `sum = sum + p.position` over the node's slice in slice order (the reference's
// src/bvh_tree.rs:58-61) and splits at `sum / len` (:67): the split, hence the whole tree, depends on every rounding of
// that chain.  The chain cannot be re-associated, but it can be scanned (f32 numbers; M = 23 mantissa bits):
//
//   while the running sum s stays inside one binade, s = S * ulp with S an integer in [2^M, 2^(M+1)), and
//   fl(s + x) = (S + r(x)) * ulp, where r(x) is x/ulp rounded to nearest; the only way the result depends on S is the
//   tie rule (x/ulp exactly half-way: round so that the new S is even), i.e. through the PARITY of S.
//
// So one addend is a map {parity of S} -> {integer increment}: a pair (a0, a1).  Maps compose associatively
// ((f then g)_p = f_p + g_[(p + f_p) & 1]), so a prefix scan of the addends gives every intermediate S exactly.  The scan
// is only valid while every intermediate stays strictly inside (2^M, 2^(M+1)); the first addend that leaves the binade
// (or is not finite, or is larger than the binade) is found by the same scan, added with a real add, and the scan
// restarts in the new binade.  For sums of same-signed numbers that happens once per binade (~20 times per f32 node).
//
// The f64 BVH (an extension: the reference is f32) folds the same chain with 53-bit significands (M = 52).  Increments
// are 64-bit: that is all it takes.  Traits<T> holds every constant in which the two precisions differ.
//
// Host + device: the device folds (bvh_fold.hip, bvh_build64.hip) and the CPU emulations the tests run
// (exact_sum_emulate.h, through `nbody_selftest_exact_sum*` of capi.hip) run the very same functions.
#pragma once
#include <stdint.h>
#include <string.h>

#include <type_traits>

#if defined(__HIPCC__)
#define NB_HD __host__ __device__ __forceinline__
#else
#define NB_HD inline
#endif

namespace nbody {
namespace xsum {

template <class T> struct Traits;
template <> struct Traits<float> {
  using U = uint32_t;  // the word S, the increments and the bit pattern live in
  using I = int32_t;   // a run's signed offsets
  static constexpr int kMantBits = 23;
  static constexpr U kExpMask = 255u;
  static constexpr U kPoison = 1u << 30;  // an increment no valid S survives
  static constexpr I kRunSat = 1 << 29;   // two saturated values still add without wrapping
};
template <> struct Traits<double> {
  using U = uint64_t;
  using I = int64_t;
  static constexpr int kMantBits = 52;
  static constexpr U kExpMask = 2047ull;
  static constexpr U kPoison = 1ull << 62;
  static constexpr I kRunSat = 1ll << 60;
};
template <class T> using Word = typename Traits<T>::U;
template <class T> using Offs = typename Traits<T>::I;
template <class T> constexpr int kMantBits = Traits<T>::kMantBits;
template <class T> constexpr Word<T> kExpMask = Traits<T>::kExpMask;
template <class T> constexpr Word<T> kPoison = Traits<T>::kPoison;
template <class T> constexpr Offs<T> kRunSat = Traits<T>::kRunSat;
template <class T> constexpr Word<T> kLo = Word<T>(1) << kMantBits<T>;
template <class T> constexpr Word<T> kHi = kLo<T> << 1;
template <class T> constexpr Word<T> kMant = kLo<T> - 1;
template <class T> constexpr int kSignBit = 8 * (int)sizeof(T) - 1;

template <class T> NB_HD Word<T> to_bits(T f) {
  Word<T> u;
  memcpy(&u, &f, sizeof u);
  return u;
}
template <class T> NB_HD T from_bits(Word<T> u) {
  T f;
  memcpy(&f, &u, sizeof f);
  return f;
}

// Running sum s = (-1)^sign * S * 2^(E - bias - M).  Usable iff s is normal (E >= 3 keeps the step's limit normal) and
// S > 2^M (at S == 2^M a subtraction would land in the finer binade below without S leaving the range).
template <class T> struct Chain {
  Word<T> sign, E, S;
};
template <class T> NB_HD bool chain_open(T s, Chain<T>& c) {
  const Word<T> b = to_bits(s), e = (b >> kMantBits<T>) & kExpMask<T>;
  c.sign = b >> kSignBit<T>;
  c.E = e;
  c.S = (b & kMant<T>) | kLo<T>;
  return e >= 3u && e != kExpMask<T> && c.S != kLo<T>;
}
template <class T> NB_HD T chain_value(const Chain<T>& c, Word<T> S) {
  return from_bits<T>((c.sign << kSignBit<T>) | (c.E << kMantBits<T>) | (S & kMant<T>));
}
template <class T> NB_HD bool in_binade(Word<T> S) { return S > kLo<T> && S < kHi<T>; }

// Increment of S caused by adding x, for S even (a0) / odd (a1).  Wrapping unsigned arithmetic.
// The FPU does the rounding: with C0 = 1.5 * 2^E (even) and C1 = C0 + ulp (odd), and |x| < 2^(E-2), C + x stays inside
// the binade, so fl(C + x) - C is x rounded to a multiple of ulp with ties going to the even/odd side exactly as they
// would from any S of the same parity; the difference of the bit patterns is that multiple as an integer.
template <class T> struct Step {
  Word<T> a0, a1;
};
template <class T> NB_HD Step<T> step_of(T x, Word<T> chain_sign, Word<T> E) {
  const Word<T> c0 = (E << kMantBits<T>) | (kLo<T> >> 1);
  const T xs = from_bits<T>(to_bits(x) ^ (chain_sign << kSignBit<T>));
  const T lim = from_bits<T>((E - 2u) << kMantBits<T>);  // chain_open guarantees E >= 3
  const T ax = from_bits<T>(to_bits(x) & ~(Word<T>(1) << kSignBit<T>));
  if (!(ax < lim)) return {kPoison<T>, kPoison<T>};  // too large for this binade, inf or NaN: a real add decides
  const T r0 = from_bits<T>(c0) + xs, r1 = from_bits<T>(c0 + 1u) + xs;
  return {to_bits(r0) - c0, to_bits(r1) - (c0 + 1u)};
}
template <class T> NB_HD Step<T> identity() { return {0u, 0u}; }
template <class T> NB_HD Word<T> apply(Word<T> S, Step<T> f) { return S + ((S & 1u) ? f.a1 : f.a0); }
// f first, then g
template <class T> NB_HD Step<T> compose(Step<T> f, Step<T> g) {
  Step<T> h;
  h.a0 = f.a0 + ((f.a0 & 1u) ? g.a1 : g.a0);
  h.a1 = f.a1 + (((f.a1 + 1u) & 1u) ? g.a1 : g.a0);
  return h;
}

// ---- whole runs of addends, so that a long chain can be cut into pieces that are prepared in parallel ------------------
// A run seen from a chain in one binade: the total increment of S and the extremes of every intermediate S, relative to
// the S the run starts from, for an even (index 0) / odd (1) start.  If S + lo > 2^M and S + hi < 2^(M+1) for the actual
// start, every add of the run stayed in the binade and S + a is the exact result.  Saturating at +-kRunSat: beyond that
// a run is unusable anyway (a poison step is twice or four times that, saturated on entry).
template <class T> struct Run {
  Offs<T> a0, a1, lo0, lo1, hi0, hi1;  // scalars: the compiler turns a select between two array elements into an indexed load from scratch
};
// The device builds lay these out by hand: six ints per f32 run, sizeof(Run) per f64 run, (sign << 32) | E from a Chain.
static_assert(sizeof(Step<float>) == 8 && sizeof(Step<double>) == 16 && sizeof(Run<float>) == 24 && sizeof(Run<double>) == 48, "");
static_assert(std::is_trivially_copyable<Step<float>>::value && std::is_trivially_copyable<Step<double>>::value, "");
static_assert(std::is_trivially_copyable<Run<float>>::value && std::is_trivially_copyable<Run<double>>::value, "");
static_assert(std::is_trivially_copyable<Chain<float>>::value && std::is_trivially_copyable<Chain<double>>::value, "");

template <class T> NB_HD Offs<T> run_sat(Offs<T> v) {
  return v > kRunSat<T> ? kRunSat<T> : (v < -kRunSat<T> ? -kRunSat<T> : v);
}
template <class T> NB_HD Run<T> run_of(Step<T> f) {
  Run<T> r;
  r.a0 = r.lo0 = r.hi0 = run_sat<T>((Offs<T>)f.a0);
  r.a1 = r.lo1 = r.hi1 = run_sat<T>((Offs<T>)f.a1);
  return r;
}
template <class T> NB_HD Run<T> run_none() { return Run<T>{0, 0, 0, 0, 0, 0}; }  // an open chain has S inside the binade: offsets 0 fit
// f first, then g.  All values travel as scalars: given `const Run&` the compiler fuses `q ? g.a1 : g.a0` into one load at a
// computed address before it has inlined the call, and the run then lives in scratch memory on the device.
template <class T>
NB_HD void run_then_from(int p, Offs<T> fa, Offs<T> flo, Offs<T> fhi, Offs<T> ga0, Offs<T> ga1, Offs<T> glo0, Offs<T> glo1, Offs<T> ghi0,
                         Offs<T> ghi1, Offs<T>& ha, Offs<T>& hlo, Offs<T>& hhi) {
  const bool q = (((int)(p + fa)) & 1) != 0;
  const Offs<T> ga = q ? ga1 : ga0, glo = q ? glo1 : glo0, ghi = q ? ghi1 : ghi0;
  ha = run_sat<T>(fa + ga);
  const Offs<T> gl = run_sat<T>(fa + glo), gh = run_sat<T>(fa + ghi);
  hlo = flo < gl ? flo : gl;
  hhi = fhi > gh ? fhi : gh;
}
template <class T> NB_HD Run<T> run_then(const Run<T>& f, const Run<T>& g) {
  const Offs<T> ga0 = g.a0, ga1 = g.a1, glo0 = g.lo0, glo1 = g.lo1, ghi0 = g.hi0, ghi1 = g.hi1;
  Run<T> h;
  run_then_from<T>(0, f.a0, f.lo0, f.hi0, ga0, ga1, glo0, glo1, ghi0, ghi1, h.a0, h.lo0, h.hi0);
  run_then_from<T>(1, f.a1, f.lo1, f.hi1, ga0, ga1, glo0, glo1, ghi0, ghi1, h.a1, h.lo1, h.hi1);
  return h;
}
template <class T> NB_HD bool run_fits(Word<T> S, const Run<T>& r) {
  const Offs<T> lo0 = r.lo0, lo1 = r.lo1, hi0 = r.hi0, hi1 = r.hi1;
  const bool p = (S & 1u) != 0u;
  return (int64_t)S + (p ? lo1 : lo0) > (int64_t)kLo<T> && (int64_t)S + (p ? hi1 : hi0) < (int64_t)kHi<T>;
}

// ---- what only one of the builds uses --------------------------------------------------------------------------------
// f32 only (bvh_chunk_runs of bvh_fold.hip): how close (relatively) to a power of two a predicted prefix may come and still
// be trusted.  The f32 chain drifts from the exact prefix by ~sqrt(n) half-ulps (worst case n): 2^-13 covers millions of
// addends; if it is ever too tight, the run's own bounds fail when it is applied and the scan takes over.  The addends inside
// the margin are added for real, so the margin also is 2 * margin * (addends so far) of serial work per crossing.
constexpr double kRunMargin = 1.0 / 8192.0;

// f64 only (b64_seg_runs of bvh_build64.hip): the binade a chain is predicted to be in over a segment whose exact prefix sums
// start at `p0` and end at `p1` (any evaluation of them: the prediction only has to be right often, the run's own bounds
// decide): both ends inside one binade and at least 2^-20 (relatively) away from its edges.  false: no run is prepared.
template <class T> NB_HD bool predict_binade(T p0, T p1, Chain<T>& c) {
  Chain<T> c1;
  if (!chain_open(p0, c) || !chain_open(p1, c1) || c.E != c1.E || c.sign != c1.sign) return false;
  constexpr Word<T> margin = kLo<T> >> 20;  // 2^-20 of the binade's 2^M steps
  return c.S > kLo<T> + margin && c.S < kHi<T> - margin && c1.S > kLo<T> + margin && c1.S < kHi<T> - margin;
}

}  // namespace xsum
}  // namespace nbody
