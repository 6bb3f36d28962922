// Internal: the phase clock of a tree step (tree_driver.hip) over the context's PhaseTiming (ctx.h): the three phases of Counting
// timed on the step's stream by events (PhaseEvents) or, for the steps enqueued ahead, by the kernels' own clock — no event
// records between the phases (every recorded event is a marker in the queue, ~6 us of idle stream).
#pragma once
#include "driver.h"

namespace nbody {

constexpr int kStampSlots = 256;  // (a ring: phase_backlog has the slots drained long before it comes round)
inline int close_open_stamp(nbody_ctx* c) {  // the last stamped step's end, when no stamped step follows it directly
  PhaseTiming& t = c->phases;
  if (t.stamp_open < 0) return NBODY_OK;
  HIPCHK(c, launch_stamp(c->stream, t.stamp_dev + 4 * (size_t)t.stamp_open + 3));
  t.stamp_open = -1;
  return NBODY_OK;
}

// One step's phases, in seconds, into the context's Counting and the caller's.
inline void book_phases(nbody_ctx* c, const double sec[3]) {
  for (nbody_counting* k : {&c->counting, c->phases.counter}) {
    if (!k) continue;
    k->build_bvh += sec[0];
    k->sum_gravity += sec[1];
    k->post_calculations += sec[2];
  }
}

// Reads every recorded step's phases into the context's (and the caller's) Counting.  Waits for them.
inline int phase_drain(nbody_ctx* c) {
  PhaseTiming& t = c->phases;
  if (int rc = close_open_stamp(c)) return rc;
  if (!t.stamp_pending.empty()) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> h((size_t)kStampSlots * 4);
    HIPCHK(c, hipMemcpy(h.data(), t.stamp_dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int slot : t.stamp_pending) {
      const unsigned long long* s = h.data() + 4 * (size_t)slot;
      const double sec[3] = {1e-8 * (double)(long long)(s[1] - s[0]), 1e-8 * (double)(long long)(s[2] - s[1]), 1e-8 * (double)(long long)(s[3] - s[2])};  // 100 MHz ticks
      book_phases(c, sec);
    }
    t.stamp_pending.clear();
  }
  for (auto& p : t.pending) {
    HIPCHK(c, hipEventSynchronize(p.e[3]));
    float ms[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) HIPCHK(c, hipEventElapsedTime(&ms[k], p.e[k], p.e[k + 1]));
    const double sec[3] = {1e-3 * ms[0], 1e-3 * ms[1], 1e-3 * ms[2]};
    book_phases(c, sec);
  }
  for (auto& p : t.pending)
    for (int k = p.borrowed ? 1 : 0; k < 4; ++k) t.free_events.push_back(p.e[k]);
  t.pending.clear();
  return NBODY_OK;
}
inline bool phase_backlog(const nbody_ctx* c) { return c->phases.pending.size() >= 64 || c->phases.stamp_pending.size() >= 64; }  // time to drain

// The clock one step holds: boundary k = 0 the build begins, 1 the walk, 2 the integration, 3 the step ends.
class StepClock {
 public:
  // `by_stamps`: the step's kernels write the boundaries themselves (stamp(k): where); otherwise mark(k) records an event.
  // `chain` (may be null): the step enqueued just before this one, with nothing in between, or an empty one; taken over — its
  // end event doubles as this step's start (two records back to back would be the largest gap of a step) — and left empty.
  int begin(nbody_ctx* c, bool by_stamps, PhaseEvents* chain = nullptr) {
    c_ = c;
    PhaseTiming& t = c->phases;
    const PhaseEvents prev = chain ? *chain : PhaseEvents{};
    if (chain) *chain = PhaseEvents{};
    if (by_stamps) {
      if (!t.stamp_dev) {
        HIPCHK(c, hipMalloc((void**)&t.stamp_dev, (size_t)kStampSlots * 4 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemsetAsync(t.stamp_dev, 0, (size_t)kStampSlots * 4 * sizeof(unsigned long long), c->stream));
      }
      slot_ = t.stamp_next;
      t.stamp_next = (t.stamp_next + 1) % kStampSlots;
      if (t.stamp_open >= 0) prev_end_ = t.stamp_dev + 4 * (size_t)t.stamp_open + 3;  // this step's first kernel closes the step before
      t.stamp_open = -1;
      return NBODY_OK;
    }
    if (int rc = close_open_stamp(c)) return rc;
    for (int k = prev.e[3] ? 1 : 0; k < 4; ++k) {
      if (t.free_events.empty()) HIPCHK(c, hipEventCreate(&ev_.e[k]));
      else { ev_.e[k] = t.free_events.back(); t.free_events.pop_back(); }
    }
    ev_.borrowed = prev.e[3] != nullptr;
    if (ev_.borrowed) ev_.e[0] = prev.e[3];
    else HIPCHK(c, hipEventRecord(ev_.e[0], c->stream));
    return NBODY_OK;
  }
  // Where the kernel at boundary k (0 .. 2) writes its stamp, and where the step's first kernel writes the end of the step
  // before; nullptr when timing by events (or nothing is open).
  unsigned long long* stamp(int k) const { return slot_ < 0 ? nullptr : c_->phases.stamp_dev + 4 * (size_t)slot_ + k; }
  unsigned long long* stamp_prev_end() const { return prev_end_; }
  int mark(int k) {  // boundary k (1, 2) is here on the stream: an event; nothing when the kernels stamp it
    if (slot_ < 0) HIPCHK(c_, hipEventRecord(ev_.e[k], c_->stream));
    return NBODY_OK;
  }
  // The step is enqueued to its end.  Stamps: its slot is booked and left open (its end: the next stamped step's first kernel,
  // or close_open_stamp).  Events: the last one is recorded, and `chain` (may be null) is where the next step starts.
  int close(PhaseEvents* chain = nullptr) {
    PhaseTiming& t = c_->phases;
    if (slot_ >= 0) {
      t.stamp_open = slot_;
      t.stamp_pending.push_back(slot_);
      return NBODY_OK;
    }
    HIPCHK(c_, hipEventRecord(ev_.e[3], c_->stream));
    t.pending.push_back(ev_);
    if (chain) *chain = ev_;
    return NBODY_OK;
  }
  // The step gave up half way and is done again by another clock's step: its events end here; a stamped slot is simply not booked.
  void give_up() { if (slot_ < 0) (void)close(); }

 private:
  nbody_ctx* c_ = nullptr;
  PhaseEvents ev_;  // timing by events
  int slot_ = -1;   // ... or by stamps: this step's slot, and where the end of the step before goes
  unsigned long long* prev_end_ = nullptr;
};

}  // namespace nbody
