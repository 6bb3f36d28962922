// CPU emulations of the device folds' control flow over the functions of exact_sum.h, to check those functions against
// the plain loop.  Host only: test scaffolding behind `nbody_selftest_exact_sum*` (capi.hip) and the native check
// (tests/native/exact_sum_check.cpp); no device translation unit includes this.
#pragma once
#include "exact_sum.h"

namespace nbody {
namespace xsum {

// The scan of bvh_big_fold / b64_fold: `tile` addends scanned at once, `seq_run` real adds after a stop.  Returns the sum;
// *stops counts the restarts.
template <class T> inline T emulate_fold(const T* x, int64_t n, int tile, int seq_run, int64_t* stops) {
  T s = 0;
  int64_t pos = 0, nstop = 0;
  while (pos < n) {
    Chain<T> c;
    if (!chain_open(s, c)) {
      const int64_t cnt = (n - pos < seq_run) ? n - pos : seq_run;
      for (int64_t k = 0; k < cnt; ++k) s = s + x[pos + k];
      pos += cnt;
      ++nstop;
      continue;
    }
    const int64_t cnt = (n - pos < tile) ? n - pos : tile;
    // "scan": prefix compositions, then every element checks its own intermediate
    Step<T> acc = identity<T>();
    Word<T> S = c.S;
    int64_t bad = -1;
    for (int64_t k = 0; k < cnt; ++k) {
      const Step<T> f = step_of(x[pos + k], c.sign, c.E);
      const Word<T> before = apply(c.S, acc);  // what the scan hands to element k
      const Word<T> after = apply(before, f);
      if (!in_binade<T>(after)) { bad = k; S = before; break; }
      acc = compose(acc, f);
      S = after;
    }
    s = chain_value(c, S);
    if (bad < 0) { pos += cnt; continue; }
    ++nstop;
    pos += bad;
    const int64_t run = (n - pos < seq_run) ? n - pos : seq_run;
    for (int64_t k = 0; k < run; ++k) s = s + x[pos + k];
    pos += run;
  }
  if (stops) *stops = nstop;
  return s;
}

// f32, the chunked fold (bvh_fold.hip: bvh_chunk_sums / bvh_chunk_runs / the chunk walk of bvh_big_fold): every chunk's runs
// are prepared for the binades its start and end are PREDICTED to be in (from exact f64 partial sums); the walk uses a run
// only if the prediction and the bounds hold for the true state, and adds for real otherwise.  A chunk that contains a
// crossing is split three ways (bvh_chunk_runs' second form): thread segments of `seg` addends whose predicted prefix stays
// below (1 - kRunMargin) of the power of two form run A (old binade), those above (1 + kRunMargin) of it run B (new binade),
// the segments in between are added for real.
inline float emulate_fold_chunked2(const float* x, int64_t n, int chunk, int seg, int64_t* used_runs) {
  using Chain = xsum::Chain<float>;
  using Run = xsum::Run<float>;
  float s = 0.0f;
  double prefix = 0.0;
  int64_t used = 0;
  auto real = [&](int64_t b, int64_t e) { for (int64_t k = b; k < e; ++k) s = s + x[k]; };
  auto take = [&](const Run& r, uint32_t sign, uint32_t E, int64_t b, int64_t e) {
    Chain cur;
    if (e > b && chain_open(s, cur) && cur.E == E && cur.sign == sign && run_fits(cur.S, r)) {
      s = chain_value(cur, (uint32_t)((int64_t)cur.S + ((cur.S & 1u) ? r.a1 : r.a0)));
      ++used;
    } else {
      real(b, e);
    }
  };
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const int64_t c1 = c0 + chunk < n ? c0 + chunk : n;
    double total = 0.0;
    for (int64_t k = c0; k < c1; ++k) total += (double)x[k];
    Chain ca, cb;
    const bool have = c0 > 0 && chain_open((float)prefix, ca) && chain_open((float)(prefix + total), cb) && ca.sign == cb.sign &&
                      (cb.E == ca.E || cb.E == ca.E + 1);
    if (!have) {
      real(c0, c1);
    } else {
      const int64_t nseg = (c1 - c0 + seg - 1) / seg;
      if (nseg > (1 << 16)) { real(c0, c1); prefix += total; continue; }  // more segments than the scratch below holds
      const double sgn = ca.sign ? -1.0 : 1.0;
      double B = 1.0;
      for (int e = 127; e < (int)cb.E; ++e) B *= 2.0;
      for (int e = 127; e > (int)cb.E; --e) B *= 0.5;
      const double lo = B * (1.0 - kRunMargin), hi = B * (1.0 + kRunMargin);
      int64_t nA = 0, nB = 0;
      bool contiguous = true;
      {
        double run = prefix;
        // pass 1: classify
        static thread_local int cls[1 << 16];
        for (int64_t t = 0; t < nseg; ++t) {
          const int64_t b = c0 + t * seg, e = b + seg < c1 ? b + seg : c1;
          const double qs = sgn * run;
          for (int64_t k = b; k < e; ++k) run += (double)x[k];
          const double qe = sgn * run;
          int cl = 2;  // zone
          if (cb.E == ca.E) cl = 0;
          else if (qs < lo && qe < lo) cl = 0;
          else if (qs > hi && qe > hi) cl = 1;
          cls[t] = cl;
          nA += cl == 0;
          nB += cl == 1;
        }
        for (int64_t t = 0; t < nseg; ++t) {
          if (cls[t] == 0 && t >= nA) contiguous = false;
          if (cls[t] == 1 && t < nseg - nB) contiguous = false;
        }
      }
      if (!contiguous) {
        real(c0, c1);
      } else {
        const int64_t u0 = c0 + (nA * seg < c1 - c0 ? nA * seg : c1 - c0);
        const int64_t u1 = c0 + ((nseg - nB) * seg < c1 - c0 ? (nseg - nB) * seg : c1 - c0);
        Run ra = run_none<float>(), rb = run_none<float>();
        for (int64_t k = c0; k < u0; ++k) ra = run_then(ra, run_of(step_of(x[k], ca.sign, ca.E)));
        for (int64_t k = u1; k < c1; ++k) rb = run_then(rb, run_of(step_of(x[k], cb.sign, cb.E)));
        take(ra, ca.sign, ca.E, c0, u0);
        real(u0, u1);
        take(rb, cb.sign, cb.E, u1, c1);
      }
    }
    prefix += total;
  }
  if (used_runs) *used_runs = used;
  return s;
}

// f64, the segmented fold (bvh_build64.hip: b64_seg_sums / b64_seg_runs / the segment test of b64_fold): every `seg`-long
// segment's run is prepared for the binade its ends are PREDICTED to be in (from plain f64 partial sums); the walk uses a
// run only if the prediction and the run's bounds hold for the true state, and scans the segment otherwise.
inline double emulate_fold_segmented(const double* x, int64_t n, int seg, int64_t* used_runs) {
  double s = 0.0, prefix = 0.0;
  int64_t used = 0;
  for (int64_t c0 = 0; c0 < n; c0 += seg) {
    const int64_t c1 = c0 + seg < n ? c0 + seg : n;
    double total = 0.0;
    for (int64_t k = c0; k < c1; ++k) total += x[k];
    Chain<double> pred;
    const bool have = c1 - c0 == seg && predict_binade(prefix, prefix + total, pred);
    Run<double> r = run_none<double>();
    if (have)
      for (int64_t k = c0; k < c1; ++k) r = run_then(r, run_of(step_of(x[k], pred.sign, pred.E)));
    Chain<double> cur;
    if (have && chain_open(s, cur) && cur.E == pred.E && cur.sign == pred.sign && run_fits(cur.S, r)) {
      s = chain_value(cur, (uint64_t)((int64_t)cur.S + ((cur.S & 1ull) ? r.a1 : r.a0)));
      ++used;
    } else {
      for (int64_t k = c0; k < c1; ++k) s = s + x[k];
    }
    prefix += total;
  }
  if (used_runs) *used_runs = used;
  return s;
}

}  // namespace xsum
}  // namespace nbody
