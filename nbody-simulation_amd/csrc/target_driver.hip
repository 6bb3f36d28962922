// libnbody_hip — the direct sum at points that are not bodies: the probe call (nbody_accel_direct_at_f32 / _f64) and the tracers'
// share of a direct step (ctx.h, Tracers).  Kernels: target_kernels.hip, and the step's clamped FAST pass (direct_kernels.hip).
//
// Routing, per call or step, from the bodies and the params alone; per target, from its own coordinates alone (include/nbody_hip.h):
//   f32  EXACT, or a clamp below 2^-19, or AUTO with a body outside FAST's domain (what makes the step run direct_exact):
//        every target EXACT.  Otherwise FAST — under AUTO a target outside FAST's domain takes its EXACT value.
//   f64  EXACT unless FAST is asked for with a clamp > 0 and every body inside the f64 FAST domain; then FAST, a target
//        outside that domain EXACT.
// FAST f32 is the clamped packed pass of the step (direct_fast<1, *, false, 2>) over the bodies in row order, its source split
// fixed by the number of bodies (probe_gsplit_f32); the clamp is in every pair, so no near/far decision depends on the targets.
// Targets go through in batches: the workspace (ctx->probe_ws) is bounded whatever their number.
#include <algorithm>
#include <vector>

#include "direct_layout.h"
#include "driver.h"
#include "target_kernels.h"

using namespace nbody;

namespace {

constexpr size_t kTargetFlagBytes = 256;
constexpr int64_t kMaxPartialF32 = (int64_t)1 << 23, kMaxPartialF64 = (int64_t)1 << 22;  // entries of a batch's partial sums at most

// The workspace of a batch of targets: the flag words, `extra` per-target arrays (the probe call's targets and results; the
// tracers have their own), and — FAST only (`gsplit` > 0) — the batch's partial sums.  A batch holds at most 2^20 targets, and
// its partial sums at most `max_partial` entries.  *batch receives the batch size.
int target_workspace(nbody_ctx* c, int64_t n_targets, size_t elem, int64_t max_partial, int gsplit, int extra, int64_t* batch) {
  const int64_t b = std::min<int64_t>(1 << 20, max_partial / std::max(gsplit, 1)) / 256 * 256;
  *batch = std::min<int64_t>(n_targets, std::max<int64_t>(b, 256));
  const size_t need = kTargetFlagBytes + (size_t)*batch * elem * ((size_t)extra + (size_t)std::max(gsplit, 0));
  return ensure_dev_bytes(c, c->probe_ws, c->probe_ws_bytes, need);
}

// The f32 FAST main pass over a batch of targets: the step's packed pass through LDS, with the clamp, its targets (a.pos_all)
// and its sources (a.src_pos: the bodies `pos`, `mass`) in different arrays; the partial sums [probe_gsplit_f32(n)][nb] go to
// `partial`.  The pass runs when flags[kFlagState] == run_state (< 0: always).
hipError_t fast_pass_f32(nbody_ctx* c, const float2* pos, const float* mass, const float2* tgt, int64_t nb, float2* partial, const int* flags,
                         int run_state) {
  const State<float>& s = c->sf;
  DirectArgs a{};
  a.pos_all = tgt;  // the targets ...
  a.src_pos = pos;  // ... and the bodies
  a.mass_all = mass;
  a.n_src = (int)s.n;
  a.tgt_begin = 0;
  a.n_tgt = (int)nb;
  a.partial = partial;
  a.to_partial = 1;
  a.clamp = c->params.clamp;
  a.uniform_mass = s.uniform_mass > 0.f ? s.uniform_mass : 0.f;
  a.flags = flags;
  a.run_state = run_state;
  DirectConfig cfg;
  cfg.tpt = 1;
  cfg.gsplit = probe_gsplit_f32(s.n);
  cfg.use_asm = 2;
  cfg.nearfar = false;
  return launch_direct_fast(c->stream, a, cfg, false);
}

}  // namespace

// ---- tracers
// Routing as the probe call's (below), but nothing comes back to the host: tracer_mark reads the decision word the bodies' step has
// just written to the workspace and every tracer's pre-step position, and leaves one mark per tracer (which of the two finishing
// kernels integrates it) and a decision word of the tracers' own at the head of ctx->probe_ws, which gates the f32 FAST main pass
// (the f64 pass has no gate: it runs for nothing in a step whose bodies left the f64 FAST domain).
namespace nbody {

int tracers_direct_f32(nbody_ctx* c, const float2* pos, const float* mass, float delta) {
  const Tracers& tr = c->tracers;
  if (tr.m == 0) return NBODY_OK;
  const int64_t n = c->sf.n, m = tr.m;
  const float clamp = c->params.clamp;
  const int arith = direct_arith_f32(c->params.arith, clamp);
  float2 *tpos = (float2*)tr.pos, *tvel = (float2*)tr.vel;
  if (arith == NBODY_ARITH_EXACT || n == 0) {
    HIPCHK(c, launch_target_exact<float>(c->stream, pos, mass, n, tpos, m, clamp, StepTracer<float>{tpos, tvel, delta, nullptr, 1}));
    return NBODY_OK;
  }
  TracerRoute r;
  if (arith == NBODY_ARITH_AUTO) {  // the step's own decision (kFlagState == 2: a body outside FAST's domain), and the per-tracer exception
    r.word = direct_flags(c->workspace);
    r.word_kind = kTracerWordState;
    r.per_target = 1;
  }
  const int g = probe_gsplit_f32(n);
  int64_t batch = 0;
  int rc = target_workspace(c, m, sizeof(float2), kMaxPartialF32, g, 0, &batch);
  if (rc) return rc;
  int* state = (int*)c->probe_ws;
  float2* part = (float2*)((char*)c->probe_ws + kTargetFlagBytes);
  HIPCHK(c, launch_tracer_mark<float>(c->stream, tpos, m, r, tr.mark, state));
  for (int64_t b0 = 0; b0 < m; b0 += batch) {
    const int64_t nb = std::min<int64_t>(batch, m - b0);
    HIPCHK(c, fast_pass_f32(c, pos, mass, tpos + b0, nb, part, state, 1));  // (tracer_mark wrote 2 when the step-level route is EXACT: the pass returns at once)
    HIPCHK(c, launch_target_fold<float>(c->stream, part, g, nb, StepTracer<float>{tpos + b0, tvel + b0, delta, tr.mark + b0, 0}));
  }
  if (r.per_target)  // the fix-up pass
    HIPCHK(c, launch_target_exact<float>(c->stream, pos, mass, n, tpos, m, clamp, StepTracer<float>{tpos, tvel, delta, tr.mark, 1}));
  return NBODY_OK;
}

int tracers_direct_f64(nbody_ctx* c, const double2* pos, const double* mass, double delta) {
  const Tracers& tr = c->tracers;
  if (tr.m == 0) return NBODY_OK;
  const int64_t n = c->sd.n, m = tr.m;
  const double clamp = (double)c->params.clamp;  // as direct64_step
  double2 *tpos = (double2*)tr.pos, *tvel = (double2*)tr.vel;
  if (!direct_fast_f64(c->params.arith, clamp) || n == 0) {
    HIPCHK(c, launch_target_exact<double>(c->stream, pos, mass, n, tpos, m, clamp, StepTracer<double>{tpos, tvel, delta, nullptr, 1}));
    return NBODY_OK;
  }
  TracerRoute r;
  r.word = (const int*)c->workspace;  // the domain flag the f64 step has just scanned the bodies into
  r.word_kind = kTracerWordDomain64;
  r.per_target = 1;
  const int g = probe_gsplit_f64(n);
  int64_t batch = 0;
  int rc = target_workspace(c, m, sizeof(double2), kMaxPartialF64, g, 0, &batch);
  if (rc) return rc;
  double2* part = (double2*)((char*)c->probe_ws + kTargetFlagBytes);
  HIPCHK(c, launch_tracer_mark<double>(c->stream, tpos, m, r, tr.mark, (int*)c->probe_ws));
  for (int64_t b0 = 0; b0 < m; b0 += batch) {
    const int64_t nb = std::min<int64_t>(batch, m - b0);
    HIPCHK(c, launch_target_fast_pass_f64(c->stream, pos, mass, n, tpos + b0, nb, clamp, part));
    HIPCHK(c, launch_target_fold<double>(c->stream, part, g, nb, StepTracer<double>{tpos + b0, tvel + b0, delta, tr.mark + b0, 0}));
  }
  HIPCHK(c, launch_target_exact<double>(c->stream, pos, mass, n, tpos, m, clamp, StepTracer<double>{tpos, tvel, delta, tr.mark, 1}));  // the fix-up pass
  return NBODY_OK;
}

}  // namespace nbody

// ---- the probe call
namespace {

// The device flag word of a body scan, read back: 0 all inside the domain.
int read_flag(nbody_ctx* c, const int* flag_dev, int* out) {
  HIPCHK(c, hipMemcpyAsync(out, flag_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NBODY_OK;
}

// Runs `pass(d_tgt, n, d_out, d_partial)` over the targets `idx` (all of them when idx is null) batch by batch and scatters the
// results into acc.
template <class T2, class Pass>
int probe_batches(nbody_ctx* c, int64_t m, const T2* tgt, const std::vector<int64_t>* idx, T2* acc, int64_t batch, Pass pass) {
  char* ws = (char*)c->probe_ws;
  T2* d_tgt = (T2*)(ws + kTargetFlagBytes);
  T2* d_out = d_tgt + batch;
  T2* d_part = d_out + batch;
  std::vector<T2> gather, result;
  const int64_t total = idx ? (int64_t)idx->size() : m;
  for (int64_t b0 = 0; b0 < total; b0 += batch) {
    const int64_t nb = std::min<int64_t>(batch, total - b0);
    const T2* src = tgt + b0;
    T2* dst = acc + b0;
    if (idx) {
      gather.resize((size_t)nb);
      result.resize((size_t)nb);
      for (int64_t k = 0; k < nb; ++k) gather[(size_t)k] = tgt[(*idx)[(size_t)(b0 + k)]];
      src = gather.data();
      dst = result.data();
    }
    HIPCHK(c, hipMemcpyAsync(d_tgt, src, (size_t)nb * sizeof(T2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, pass(d_tgt, nb, d_out, d_part));
    HIPCHK(c, hipMemcpyAsync(dst, d_out, (size_t)nb * sizeof(T2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (idx)
      for (int64_t k = 0; k < nb; ++k) acc[(*idx)[(size_t)(b0 + k)]] = result[(size_t)k];
  }
  return NBODY_OK;
}

// The targets outside FAST's domain: under f32 AUTO and f64 FAST they take their EXACT values.
template <class T2> std::vector<int64_t> odd_targets(int64_t m, const T2* tgt) {
  std::vector<int64_t> odd;
  for (int64_t i = 0; i < m; ++i)
    if (outside_fast(tgt[i].x) || outside_fast(tgt[i].y)) odd.push_back(i);
  return odd;
}

int accel_at_f32(nbody_ctx* c, int64_t m, const float2* tgt, float2* acc) {
  State<float>& s = c->sf;
  const int64_t n = s.n;
  if (n == 0) {
    std::fill(acc, acc + m, make_float2(0.f, 0.f));
    return NBODY_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const float clamp = c->params.clamp;
  int arith = direct_arith_f32(c->params.arith, clamp);
  const int g = probe_gsplit_f32(n);
  auto& st = s.set[s.cur];
  int rc = NBODY_OK;
  if (arith == NBODY_ARITH_AUTO) {  // the step's hazard scan over the bodies
    rc = ensure_dev_bytes(c, c->probe_ws, c->probe_ws_bytes, kTargetFlagBytes);
    if (rc) return rc;
    int* flag = (int*)c->probe_ws;
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    HIPCHK(c, launch_hazard_scan(c->stream, (const float*)st.pos, 2 * n, flag));
    int bad = 0;
    rc = read_flag(c, flag, &bad);
    if (rc) return rc;
    if (bad) arith = NBODY_ARITH_EXACT;
  }
  int64_t batch = 0;
  rc = target_workspace(c, m, sizeof(float2), kMaxPartialF32, arith == NBODY_ARITH_EXACT ? 0 : g, 2, &batch);
  if (rc) return rc;
  const int* flag = (const int*)c->probe_ws;
  auto exact = [&](const float2* d_tgt, int64_t nb, float2* d_out, float2*) {
    return launch_target_exact<float>(c->stream, st.pos, st.mass, n, d_tgt, nb, clamp, StoreAcc<float>{d_out});
  };
  if (arith == NBODY_ARITH_EXACT) return probe_batches(c, m, tgt, nullptr, acc, batch, exact);
  auto fast = [&](const float2* d_tgt, int64_t nb, float2* d_out, float2* d_part) {
    hipError_t e = fast_pass_f32(c, st.pos, st.mass, d_tgt, nb, d_part, flag, -1);
    return e == hipSuccess ? launch_target_fold<float>(c->stream, d_part, g, nb, StoreAcc<float>{d_out}) : e;
  };
  rc = probe_batches(c, m, tgt, nullptr, acc, batch, fast);
  if (rc || arith != NBODY_ARITH_AUTO) return rc;
  const std::vector<int64_t> odd = odd_targets(m, tgt);
  return odd.empty() ? NBODY_OK : probe_batches(c, m, tgt, &odd, acc, batch, exact);
}

int accel_at_f64(nbody_ctx* c, int64_t m, const double2* tgt, double2* acc) {
  State<double>& s = c->sd;
  const int64_t n = s.n;
  if (n == 0) {
    std::fill(acc, acc + m, double2{0.0, 0.0});
    return NBODY_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const double clamp = (double)c->params.clamp;  // the f32 parameter widened, as direct64_step
  bool fast = direct_fast_f64(c->params.arith, clamp);
  auto& st = s.set[s.cur];
  int rc = NBODY_OK;
  if (fast) {  // the f64 step's domain scan over the bodies
    rc = ensure_dev_bytes(c, c->probe_ws, c->probe_ws_bytes, kTargetFlagBytes);
    if (rc) return rc;
    int* flag = (int*)c->probe_ws;
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    HIPCHK(c, launch_domain_scan_f64(c->stream, (const double*)st.pos, 2 * n, flag));
    int bad = 0;
    rc = read_flag(c, flag, &bad);
    if (rc) return rc;
    if (bad) fast = false;
  }
  const int g = probe_gsplit_f64(n);
  int64_t batch = 0;
  rc = target_workspace(c, m, sizeof(double2), kMaxPartialF64, fast ? g : 0, 2, &batch);
  if (rc) return rc;
  auto exact = [&](const double2* d_tgt, int64_t nb, double2* d_out, double2*) {
    return launch_target_exact<double>(c->stream, st.pos, st.mass, n, d_tgt, nb, clamp, StoreAcc<double>{d_out});
  };
  if (!fast) return probe_batches(c, m, tgt, nullptr, acc, batch, exact);
  rc = probe_batches(c, m, tgt, nullptr, acc, batch, [&](const double2* d_tgt, int64_t nb, double2* d_out, double2* d_part) {
    hipError_t e = launch_target_fast_pass_f64(c->stream, st.pos, st.mass, n, d_tgt, nb, clamp, d_part);
    return e == hipSuccess ? launch_target_fold<double>(c->stream, d_part, g, nb, StoreAcc<double>{d_out}) : e;
  });
  if (rc) return rc;
  const std::vector<int64_t> odd = odd_targets(m, tgt);
  return odd.empty() ? NBODY_OK : probe_batches(c, m, tgt, &odd, acc, batch, exact);
}

int accel_at_check(nbody_ctx* c, bool f64, int64_t m, const void* tgt, const void* acc) {
  const char* what = f64 ? "accel_direct_at_f64" : "accel_direct_at_f32";
  if (m < 0) return fail(c, NBODY_ERR_INVALID, std::string(what) + ": n_targets < 0");
  if (m > 0 && (!tgt || !acc)) return fail(c, NBODY_ERR_INVALID, std::string(what) + ": target_xy or acc_xy is NULL");
  if (f64 ? !c->has_f64 : !c->has_f32)
    return fail(c, NBODY_ERR_INVALID, std::string(what) + ((f64 ? c->has_f32 : c->has_f64)
                                                               ? ": the context holds particles of the other precision"
                                                               : ": no particles uploaded"));
  return NBODY_OK;
}

}  // namespace

namespace nbody {
int ctx_accel_direct_at(nbody_ctx* c, bool f64, int64_t n_targets, const void* target_xy, void* acc_xy) {
  if (n_targets == 0) return NBODY_OK;
  return f64 ? accel_at_f64(c, n_targets, (const double2*)target_xy, (double2*)acc_xy)
             : accel_at_f32(c, n_targets, (const float2*)target_xy, (float2*)acc_xy);
}
}  // namespace nbody

NB_API int nbody_accel_direct_at_f32(nbody_ctx* c, int64_t n_targets, const float* target_xy, float* acc_xy) {
  if (!c) return NBODY_ERR_INVALID;
  int rc = accel_at_check(c, false, n_targets, target_xy, acc_xy);
  if (rc || n_targets == 0) return rc;
  if (c->multi) return multi_accel_direct_at(c, false, n_targets, target_xy, acc_xy);
  return ctx_accel_direct_at(c, false, n_targets, target_xy, acc_xy);
}
NB_API int nbody_accel_direct_at_f64(nbody_ctx* c, int64_t n_targets, const double* target_xy, double* acc_xy) {
  if (!c) return NBODY_ERR_INVALID;
  int rc = accel_at_check(c, true, n_targets, target_xy, acc_xy);
  if (rc || n_targets == 0) return rc;
  if (c->multi) return multi_accel_direct_at(c, true, n_targets, target_xy, acc_xy);
  return ctx_accel_direct_at(c, true, n_targets, target_xy, acc_xy);
}
