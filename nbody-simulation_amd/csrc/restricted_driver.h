// libnbody_hip — restricted ensembles: the host driver behind nbody_restricted_* (restricted.hip) and nbody_restricted64_*
// (restricted64.hip), written once over a precision P as ensemble_driver.h is, and out of its parts: the bodies are the ensemble's
// — state, create / destroy, params, errors, upload, download and the *_with functions — stepped by the ensemble's own launch.
// Internal.  What differs: beside the bodies the handle keeps m tracers per world and steps them with P's tracer launch.  A step
// is the bodies' launch and then the tracers', both given the same P::Args: the tracers read the buffer the bodies' launch reads
// (pos_in, the pre-step positions — the bodies write the other buffer), and the next step's launches follow in stream order.
// Nothing is read back and nothing waits between the steps of a call.
//
// P supplies what ensemble_driver.h asks for (kWho "restricted") and, for the tracers:
//   Tracers                                          the tracer kernel's arguments (tpos, tvel, tacc_out, n_tracers);
//   launch_tracers(stream, n_worlds, args, tracers)  one step — without tvel, one force evaluation — of the tracers of all worlds.
#pragma once
#include "ensemble_driver.h"

namespace nbody {

template <class P> struct RestrictedState : EnsembleState<P> {
  int64_t n_tracers = 0;  // per world; 0: none
  typename P::Vec2* tpos = nullptr;
  typename P::Vec2* tvel = nullptr;
  typename P::Vec2* tacc = nullptr;
  ~RestrictedState() { drop_tracers(); }  // (ens_destroy has made the device current and drained the stream)
  void drop_tracers() {
    free_dev(tpos); free_dev(tvel); free_dev(tacc);
    n_tracers = 0;
    this->dtracers.release();  // (the tracers' delta streams start over with the next tracers)
  }
};

template <class P> int rst_fail(RestrictedState<P>* e, const char* msg) { return ens_fail<P>(e, NBODY_ERR_INVALID, msg); }
#define RST_HIPCHK(e, call)                                        \
  do {                                                             \
    hipError_t h__ = (call);                                       \
    if (h__ != hipSuccess) return ens_fail_hip<P>(e, h__, #call);  \
  } while (0)

template <class P> typename P::Tracers rst_tracers(const RestrictedState<P>* e) {
  typename P::Tracers t;
  t.tpos = e->tpos;
  t.n_tracers = e->n_tracers;
  return t;
}

// The ensemble's upload in its two halves.  Refused for its arguments, it leaves bodies and tracers as they were; past the check
// the tracers go, with the bodies where the store fails (it drains the stream before it frees) and as those of a new world where
// it succeeds.
template <class P>
int rst_upload(RestrictedState<P>* e, int64_t n_worlds, int64_t n_bodies, const typename P::Real* pos, const typename P::Real* vel,
               const uint32_t* weight) {
  if (int rc = ens_upload_check<P>(e, n_worlds, n_bodies, pos, vel)) return rc;
  const int rc = ens_upload_store<P>(e, n_worlds, n_bodies, pos, vel, weight);
  e->drop_tracers();
  return rc;
}

template <class P> int rst_tracers_upload(RestrictedState<P>* e, int64_t n_worlds, int64_t n_tracers, const typename P::Real* pos, const typename P::Real* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rst_fail(e, "restricted tracers_upload: nothing uploaded (the bodies come first)");
  if (n_worlds != e->n_worlds) return rst_fail(e, "restricted tracers_upload: n_worlds is not the number of worlds of the bodies");
  if (n_tracers < 0 || n_tracers > kEnsembleMaxRows / n_worlds)
    return rst_fail(e, "restricted tracers_upload: n_tracers must be >= 0 and n_worlds * n_tracers <= 2^26");
  if (n_tracers > 0 && (!pos || !vel)) return rst_fail(e, "restricted tracers_upload: pos_xy or vel_xy is NULL");
  RST_HIPCHK(e, hipSetDevice(e->device));
  RST_HIPCHK(e, hipStreamSynchronize(e->stream));
  e->drop_tracers();
  if (n_tracers == 0) return NBODY_OK;
  const size_t bytes = (size_t)(n_worlds * n_tracers) * sizeof(typename P::Vec2);
  hipError_t h = hipMalloc((void**)&e->tpos, bytes);
  if (h == hipSuccess) h = hipMalloc((void**)&e->tvel, bytes);
  if (h == hipSuccess) h = hipMemcpyAsync(e->tpos, pos, bytes, hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipMemcpyAsync(e->tvel, vel, bytes, hipMemcpyHostToDevice, e->stream);
  if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
  if (h != hipSuccess) {
    e->drop_tracers();
    return ens_fail_hip<P>(e, h, "upload of the tracers");
  }
  e->n_tracers = n_tracers;
  return NBODY_OK;
}

template <class P> int rst_tracers_download(RestrictedState<P>* e, typename P::Real* pos, typename P::Real* vel) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rst_fail(e, "restricted tracers_download: nothing uploaded");
  if (!e->n_tracers) return NBODY_OK;
  RST_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)(e->n_worlds * e->n_tracers) * sizeof(typename P::Vec2);
  if (pos) RST_HIPCHK(e, hipMemcpyAsync(pos, e->tpos, bytes, hipMemcpyDeviceToHost, e->stream));
  if (vel) RST_HIPCHK(e, hipMemcpyAsync(vel, e->tvel, bytes, hipMemcpyDeviceToHost, e->stream));
  RST_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

// One step of the bodies and then of the tracers, both given `a`.
template <class P> hipError_t rst_launch_step(RestrictedState<P>* e, const typename P::Args& a) {
  hipError_t h = P::launch(e->stream, e->n_worlds, a);
  if (h != hipSuccess || !e->n_tracers) return h;
  typename P::Tracers t = rst_tracers(e);
  t.tvel = e->tvel;
  return P::launch_tracers(e->stream, e->n_worlds, a, t);  // a.pos_in: what the bodies' launch above reads
}

template <class P> int rst_update(RestrictedState<P>* e, typename P::Real delta, int n_steps, nbody_counting* counter) {
  return ens_update_with<P>(e, delta, n_steps, counter, [e](const typename P::Args& a) { return rst_launch_step<P>(e, a); });
}

// A sweep: the tracers of world k follow its delta, clamp and steps (both launches read the same table).
template <class P>
int rst_sweep(RestrictedState<P>* e, const typename P::Real* delta, const float* clamp, const int32_t* steps, int n_steps, nbody_counting* counter) {
  return ens_sweep_with<P>(e, delta, clamp, steps, n_steps, counter, [e](const typename P::Args& a) { return rst_launch_step<P>(e, a); });
}

template <class P> int rst_accel(RestrictedState<P>* e, typename P::Real* acc_xy) { return ens_accel<P>(e, acc_xy); }

template <class P> int rst_tracers_accel(RestrictedState<P>* e, typename P::Real* acc_xy) {
  if (!e) return NBODY_ERR_INVALID;
  if (!e->n_worlds) return rst_fail(e, "restricted tracers_accel: nothing uploaded");
  if (!e->n_tracers) return NBODY_OK;
  if (!acc_xy) return rst_fail(e, "restricted tracers_accel: acc_xy is NULL");
  RST_HIPCHK(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)(e->n_worlds * e->n_tracers) * sizeof(typename P::Vec2);
  if (!e->tacc) RST_HIPCHK(e, hipMalloc((void**)&e->tacc, bytes));
  typename P::Tracers t = rst_tracers(e);
  t.tacc_out = e->tacc;
  RST_HIPCHK(e, P::launch_tracers(e->stream, e->n_worlds, ens_args<P>(e), t));
  RST_HIPCHK(e, hipMemcpyAsync(acc_xy, e->tacc, bytes, hipMemcpyDeviceToHost, e->stream));
  RST_HIPCHK(e, hipStreamSynchronize(e->stream));
  return NBODY_OK;
}

// Where the handle's rows are, for the observers (ensemble_observers.h); of no handle, nothing (they refuse it).  Without tracers
// the tracers' frames are the bodies', every world's tracer stream a header of 0 rows and its tracer records of rows == 0.
template <class P> WorldRows<P> rst_rows(const RestrictedState<P>* e) {
  WorldRows<P> rows;
  rows.has_tracer_calls = true;
  if (!e) return rows;
  rows.n_tracers = e->n_tracers;
  rows.tracer_rows = e->n_worlds * e->n_tracers;
  rows.tpos = e->tpos;
  rows.tvel = e->tvel;
  return rows;
}

template <class P> int64_t rst_num_tracers(const RestrictedState<P>* e) { return e ? e->n_tracers : 0; }

#undef RST_HIPCHK

}  // namespace nbody
