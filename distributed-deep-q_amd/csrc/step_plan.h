// The plan of one training step: which launch applies, books, bumps, draws.
// Decided once (plan_step) from what the step is (StepFacts); every launch
// wrapper reads its own fields of the answer and decides nothing again.  Plain
// C++17, no HIP: cpu/step_plan_check.cpp enumerates every StepFacts and checks
// the step invariant on the plans (DESIGN.md "The step plan" has the table).
#pragma once

namespace ddq {

// The exchange a step really runs (cfg->exchange with no communicator is None).
enum class Exchange {
  None,
  AllReduce,          // one call on the ctx stream, or an in-process group's copies
  AllReduceOverlap,   // over a communicator, the fc4 bucket under the conv backward
  Sharded,
  Server,
  AsyncWorker,        // a gradient for the owners: no apply, no bookkeeping here
};

// A launch of the step, in launch order on the ctx stream.  Side: the side
// stream, forked before the step's first launch.  Apply and OwnerApply are
// alternatives at the same place.  (SlabReduce: K4 on the small path; Head:
// K1's book block there.)
enum class Site { Nobody, Side, Head, PrioCommit, SlabReduce, Apply, OwnerApply };
inline int site_order(Site s) { return s == Site::OwnerApply ? (int)Site::Apply : (int)s; }
inline bool on_ctx_stream(Site s) { return s != Site::Nobody && s != Site::Side; }

enum class ApplyRange {
  None,                     // gradient only
  AllInSlabReduce,          // fused apply (small path: fc4 in K2, the rest in K4)
  Fc4InSlabRestInApply,     // fused apply, ext: the rest after its all-reduce
  AllInApply,
  OwnerApply,               // the rank's shard
};

struct StepFacts {
  bool small = false;            // the S = 16 four-launch step, else the general kernels
  bool b_le_256 = true;
  bool prio = false;
  bool adam = false;
  Exchange ex = Exchange::None;
  bool fused_apply_ok = true;    // the layout allows it and the apply is no phase of its own
  bool no_grad_store = false;    // DDQ_STEP_NO_GRAD_STORE
  bool holds_counter = true;     // one-launch or prioritized draw: the step must advance the
                                 // counter; the two-launch draw advanced it already
  bool prefetch = false;         // the next step's set is drawn + gathered beside this step
  int book_period = 0;           // target period of the apply bookkeeping; < 0: no bookkeeping
  int book_step = 1;              // param-server iterations per apply (1, or W)
  bool fault_k2_short = false;   // ddq_inject_fault: this step's fc4 chain one workgroup short
};

struct StepPlan {
  ApplyRange apply = ApplyRange::None;   // which launch applies which parameter range
  bool store_grad = false;               // fused: fc4's weight gradient also to the buffer
  bool prio_commit = false;              // the |TD| commit launch runs (and there the counter
                                         // always moves: it must then be the bump site)
  Site bump = Site::Nobody;              // who advances the draw counter
  Site draw = Site::Nobody;              // who draws the next step's index set
  Site gather = Site::Nobody;            // who gathers it
  Site latch = Site::Nobody;             // who latches the apply flags first
  Site book = Site::Nobody;              // who does the apply bookkeeping (Apply: a launch of
                                         // its own before it, plan_apply_only)
  int book_period = 0, book_step = 1;
  bool k2_short = false;

  bool fused() const {
    return apply == ApplyRange::AllInSlabReduce || apply == ApplyRange::Fc4InSlabRestInApply;
  }
  bool ext() const { return apply == ApplyRange::Fc4InSlabRestInApply; }
  // the gather blocks find the set in idx already
  bool predrawn() const { return draw != gather && on_ctx_stream(draw) && on_ctx_stream(gather); }
};

// An update outside a step (ddq_apply_async): the apply launch, its
// bookkeeping as the one-thread launch before it.
inline StepPlan plan_apply_only() {
  StepPlan p;
  p.apply = ApplyRange::AllInApply;
  p.latch = p.book = Site::Apply;
  return p;
}

// Forward + backward alone (ddq_forward_backward): nobody does anything else.
inline StepPlan plan_grad_only() {
  StepPlan p;
  p.book_period = -1;
  return p;
}

// false (*why set): a combination the contract never produces.
inline bool plan_step(const StepFacts& f, StepPlan* p, const char** why) {
  *p = StepPlan{};
  auto no = [&](const char* w) {
    if (why) *why = w;
    return false;
  };
  const bool async = f.ex == Exchange::AsyncWorker;
  const bool owner = f.ex == Exchange::Sharded || f.ex == Exchange::Server;
  // exchange-free steps, and the overlapped all-reduce of the general kernels
  // (the small path applies fc4 inside K2, before a bucket could be summed);
  // Adam keeps two state words: its update is a launch of its own
  const bool fused = !f.adam && f.fused_apply_ok &&
                     (f.ex == Exchange::None || (f.ex == Exchange::AllReduceOverlap && !f.small));
  if (f.prio && (!(fused || f.adam) || !f.holds_counter))
    return no("a prioritized step without the fused apply or the draw counter");
  if (f.small && !f.b_le_256) return no("the small path with B > 256");
  if (f.holds_counter != f.b_le_256)
    return no("the one-launch draw is the draw of B <= 256, and leaves the counter to the step");
  if (f.prio && f.ex != Exchange::None) return no("a prioritized step with an exchange");
  if (f.adam && f.ex != Exchange::None && f.ex != Exchange::AllReduce)
    return no("Adam with an exchange other than the one-call all-reduce");
  if ((f.book_period < 0) != async) return no("bookkeeping is off for the async worker only");
  if (async && f.prefetch) return no("the async worker's next draw belongs to its tick");

  p->apply = async   ? ApplyRange::None
             : fused ? (f.ex == Exchange::None ? ApplyRange::AllInSlabReduce
                                               : ApplyRange::Fc4InSlabRestInApply)
             : owner ? ApplyRange::OwnerApply
                     : ApplyRange::AllInApply;
  p->store_grad = fused && (f.ex != Exchange::None || !f.no_grad_store);
  p->book = async ? Site::Nobody : Site::SlabReduce;
  p->latch = async ? Site::Nobody : fused ? Site::Head : Site::SlabReduce;
  p->prio_commit = f.prio;
  // once per step, and before the next draw
  p->bump = !f.holds_counter ? Site::Nobody
            : f.prio         ? Site::PrioCommit
            : fused || async ? Site::Head
                             : Site::SlabReduce;
  if (f.prefetch && !f.b_le_256) {
    p->draw = p->gather = Site::Side;   // the two-launch draw
  } else if (f.prefetch) {
    p->gather = fused ? Site::SlabReduce : owner ? Site::OwnerApply : Site::Apply;
    p->draw = f.prio ? Site::PrioCommit : fused ? Site::Head : p->gather;
  }
  p->book_period = f.book_period;
  p->book_step = f.book_step;
  p->k2_short = f.fault_k2_short;
  return true;
}

}  // namespace ddq
