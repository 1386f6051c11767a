// The step invariant, checked on every plan plan_step makes -- no GPU, no HIP:
// each step advances the device draw counter exactly once, applies the update
// exactly once and does the apply bookkeeping exactly once, and the next
// step's index set is drawn after the counter has moved.
//   g++ -std=c++17 cpu/step_plan_check.cpp -o step_plan_check && ./step_plan_check
// 1. every StepFacts combination: the invariant on each accepted plan, and
//    every combination the step body used to refuse is refused with a reason;
// 2. the plan of each regime the GPU tests run, against a literal table
//    written down from the launch wrappers' conditions before there was a plan.
#include "../csrc/step_plan.h"

#include <cstdio>
#include <string>

using namespace ddq;

static int g_failed = 0;
static std::string g_ctx;
#define CHECK(cond, what)                                                        \
  do {                                                                           \
    if (!(cond)) {                                                               \
      if (++g_failed <= 20) printf("FAILED [%s]: %s\n", g_ctx.c_str(), what);    \
    }                                                                            \
  } while (0)

static const char* kSite[] = {"Nobody", "Side", "Head", "PrioCommit", "SlabReduce", "Apply",
                              "OwnerApply"};
static const char* kEx[] = {"None", "AllReduce", "AllReduceOverlap", "Sharded", "Server",
                            "AsyncWorker"};
static const char* kApply[] = {"None", "AllInSlabReduce", "Fc4InSlabRestInApply", "AllInApply",
                               "OwnerApply"};

static std::string show(const StepFacts& f) {
  char b[256];
  snprintf(b, sizeof b, "small %d B<=256 %d prio %d adam %d ex %s fused_ok %d no_grad_store %d "
           "holds %d prefetch %d period %d inc %d fault %d", f.small, f.b_le_256, f.prio, f.adam,
           kEx[(int)f.ex], f.fused_apply_ok, f.no_grad_store, f.holds_counter, f.prefetch,
           f.book_period, f.book_step, f.fault_k2_short);
  return b;
}

static void check_invariant(const StepFacts& f, const StepPlan& p) {
  const bool async = f.ex == Exchange::AsyncWorker;
  const bool owner = f.ex == Exchange::Sharded || f.ex == Exchange::Server;
  const bool book_on = f.book_period >= 0;
  // the counter: one site if the caller holds it, none otherwise
  CHECK((p.bump != Site::Nobody) == f.holds_counter,
        "exactly one site advances the counter iff the caller holds it");
  CHECK(p.bump == Site::Nobody || p.bump == Site::Head || p.bump == Site::PrioCommit ||
            p.bump == Site::SlabReduce,
        "the counter advances in the head, the commit or the slab-reduce launch");
  CHECK(p.prio_commit == (p.bump == Site::PrioCommit),
        "the commit launch always advances the counter: it runs iff it is the one bump site");
  CHECK(p.prio_commit == f.prio, "the commit launch runs on prioritized steps only");
  CHECK(p.bump != Site::SlabReduce || p.book == Site::SlabReduce,
        "the slab reduce advances the counter inside its bookkeeping");
  CHECK(!(p.fused() && p.bump == Site::SlabReduce),
        "with the fused apply the slab reduce does not advance the counter (the head does, "
        "so the slab-reduce launch can carry the next gather)");
  // the next draw
  CHECK((p.draw != Site::Nobody) == f.prefetch && (p.gather != Site::Nobody) == f.prefetch,
        "a next set is drawn and gathered iff one is prefetched");
  CHECK(p.draw == Site::Nobody || p.bump == Site::Nobody ||
            site_order(p.draw) >= site_order(p.bump),
        "the next draw comes no earlier than the counter's advance");
  CHECK(site_order(p.gather) >= site_order(p.draw), "the gather comes no earlier than the draw");
  CHECK((p.draw == Site::Side) == (p.gather == Site::Side), "the side stream draws what it gathers");
  CHECK(p.draw != Site::PrioCommit || p.prio_commit, "the commit launch draws only when it runs");
  CHECK(p.draw != Site::Head || p.bump == Site::Head,
        "the head's draw block is the one that advances the counter");
  {
    const bool ctx_d = p.draw != Site::Nobody && p.draw != Site::Side;
    const bool ctx_g = p.gather != Site::Nobody && p.gather != Site::Side;
    CHECK(p.predrawn() == (p.draw != p.gather && ctx_d && ctx_g),
          "predrawn exactly when draw and gather are different ctx-stream launches");
  }
  CHECK(!(p.draw == Site::Side && f.b_le_256 && !async),
        "no side-stream draw at B <= 256 without the async exchange");
  // the apply: every range by one site (the enum), none without bookkeeping
  CHECK((p.apply == ApplyRange::None) == !book_on, "nothing is applied iff bookkeeping is off");
  CHECK((p.apply == ApplyRange::OwnerApply) == owner, "the owner apply is the sharded / server one");
  CHECK(p.gather != Site::OwnerApply || p.apply == ApplyRange::OwnerApply,
        "the owner apply gathers only where it runs");
  CHECK(p.gather != Site::Apply || p.apply == ApplyRange::AllInApply,
        "the apply launch gathers only where it applies everything");
  CHECK(!(p.fused() && f.adam), "the fused apply never occurs with Adam");
  CHECK(!p.ext() || (f.ex == Exchange::AllReduceOverlap && !f.small),
        "ext occurs only with the overlapped all-reduce on the general path");
  CHECK(!p.store_grad || p.fused(), "store_grad is a switch of the fused apply");
  CHECK(!p.ext() || p.store_grad, "ext: the all-reduce needs fc4's gradient in the buffer");
  // bookkeeping and latch: once, or not at all
  CHECK((p.book == Site::SlabReduce) == book_on && (p.book == Site::Nobody) == !book_on,
        "the bookkeeping happens once, in the slab reduce, or not at all");
  CHECK((p.latch == Site::Nobody) == !book_on, "the latch happens iff the bookkeeping does");
  CHECK(p.latch == (p.fused() ? Site::Head : p.book),
        "the flags are latched before the first launch that applies: the head when fused, the "
        "bookkeeping otherwise");
  CHECK(p.book_period == f.book_period && p.book_step == f.book_step && p.k2_short == f.fault_k2_short,
        "period, increment and the fault bit pass through");
}

// the refusal of the step body before there was a plan:
//   prio && (!(fa.on || adam) || !bump)
static bool old_guard_refuses(const StepFacts& f) {
  const bool ar_overlap = f.ex == Exchange::AllReduceOverlap;
  const bool fa_on = !f.adam && (f.ex == Exchange::None || (ar_overlap && !f.small)) &&
                     f.fused_apply_ok;
  return f.prio && (!(fa_on || f.adam) || !f.holds_counter);
}

static int enumerate() {
  int n = 0, ok = 0;
  const int periods[] = {-1, 0, 10}, incs[] = {1, 4};
  for (int bits = 0; bits < 512; ++bits)
    for (int ex = 0; ex < 6; ++ex)
      for (int period : periods)
        for (int inc : incs) {
          StepFacts f;
          f.small = bits & 1; f.b_le_256 = bits & 2; f.prio = bits & 4; f.adam = bits & 8;
          f.fused_apply_ok = bits & 16; f.no_grad_store = bits & 32; f.holds_counter = bits & 64;
          f.prefetch = bits & 128; f.fault_k2_short = bits & 256;
          f.ex = (Exchange)ex; f.book_period = period; f.book_step = inc;
          g_ctx = show(f);
          StepPlan p;
          const char* why = nullptr;
          const bool acc = plan_step(f, &p, &why);
          ++n;
          if (acc) {
            ++ok;
            check_invariant(f, p);
          } else {
            CHECK(why && *why, "a refusal gives its reason");
          }
          if (old_guard_refuses(f)) CHECK(!acc && why && *why, "the step body's old refusal is kept");
        }
  printf("%d combinations, %d accepted\n", n, ok);
  return ok;
}

// One regime: the facts, and the plan read off the parent's launch wrappers.
struct Row {
  const char* name;
  // facts: small, B <= 256, prio, adam, exchange, fused_apply_ok, no_grad_store, holds, prefetch,
  // period, inc
  bool small, b256, prio, adam;
  Exchange ex;
  bool fok, nogs, holds, prefetch;
  int period, inc;
  // plan
  ApplyRange apply;
  bool store_grad, commit;
  Site bump, draw, gather, latch, book;
  bool predrawn;
};

using E = Exchange;
using A = ApplyRange;
using S = Site;
static const Row kRows[] = {
    // name                                 sm b256 prio adam ex                  fok nogs holds pre  per inc  apply                    store commit bump           draw           gather         latch          book           predrawn
    {"plain fused eager B<=256",            0, 1,   0,   0,   E::None,             1,  0,   1,    0,   10, 1,   A::AllInSlabReduce,      1,    0,     S::Head,       S::Nobody,     S::Nobody,     S::Head,       S::SlabReduce, 0},
    {"plain fused eager, no grad store",    0, 1,   0,   0,   E::None,             1,  1,   1,    0,   10, 1,   A::AllInSlabReduce,      0,    0,     S::Head,       S::Nobody,     S::Nobody,     S::Head,       S::SlabReduce, 0},
    {"plain fused pipelined B<=256",        0, 1,   0,   0,   E::None,             1,  0,   1,    1,   10, 1,   A::AllInSlabReduce,      1,    0,     S::Head,       S::Head,       S::SlabReduce, S::Head,       S::SlabReduce, 1},
    {"B>256 eager",                         0, 0,   0,   0,   E::None,             1,  0,   0,    0,   10, 1,   A::AllInSlabReduce,      1,    0,     S::Nobody,     S::Nobody,     S::Nobody,     S::Head,       S::SlabReduce, 0},
    {"B>256 pipelined",                     0, 0,   0,   0,   E::None,             1,  0,   0,    1,   10, 1,   A::AllInSlabReduce,      1,    0,     S::Nobody,     S::Side,       S::Side,       S::Head,       S::SlabReduce, 0},
    {"prioritized rmsprop pipelined",       0, 1,   1,   0,   E::None,             1,  0,   1,    1,   10, 1,   A::AllInSlabReduce,      1,    1,     S::PrioCommit, S::PrioCommit, S::SlabReduce, S::Head,       S::SlabReduce, 1},
    {"prioritized Adam pipelined",          0, 1,   1,   1,   E::None,             1,  0,   1,    1,   10, 1,   A::AllInApply,           0,    1,     S::PrioCommit, S::PrioCommit, S::Apply,      S::SlabReduce, S::SlabReduce, 1},
    {"Adam with clipping, plain",           0, 1,   0,   1,   E::None,             1,  0,   1,    0,   10, 1,   A::AllInApply,           0,    0,     S::SlabReduce, S::Nobody,     S::Nobody,     S::SlabReduce, S::SlabReduce, 0},
    {"small path fused",                    1, 1,   0,   0,   E::None,             1,  0,   1,    0,   10, 1,   A::AllInSlabReduce,      1,    0,     S::Head,       S::Nobody,     S::Nobody,     S::Head,       S::SlabReduce, 0},
    {"small path fused pipelined",          1, 1,   0,   0,   E::None,             1,  0,   1,    1,   10, 1,   A::AllInSlabReduce,      1,    0,     S::Head,       S::Head,       S::SlabReduce, S::Head,       S::SlabReduce, 1},
    {"small path overlapped all-reduce",    1, 1,   0,   0,   E::AllReduceOverlap, 1,  0,   1,    1,   10, 1,   A::AllInApply,           0,    0,     S::SlabReduce, S::Apply,      S::Apply,      S::SlabReduce, S::SlabReduce, 0},
    {"general overlapped all-reduce",       0, 1,   0,   0,   E::AllReduceOverlap, 1,  1,   1,    1,   10, 1,   A::Fc4InSlabRestInApply, 1,    0,     S::Head,       S::Head,       S::SlabReduce, S::Head,       S::SlabReduce, 1},
    {"plain all-reduce pipelined",          0, 1,   0,   0,   E::AllReduce,        1,  0,   1,    1,   10, 1,   A::AllInApply,           0,    0,     S::SlabReduce, S::Apply,      S::Apply,      S::SlabReduce, S::SlabReduce, 0},
    {"sharded pipelined",                   0, 1,   0,   0,   E::Sharded,          1,  0,   1,    1,   10, 1,   A::OwnerApply,           0,    0,     S::SlabReduce, S::OwnerApply, S::OwnerApply, S::SlabReduce, S::SlabReduce, 0},
    {"server pipelined",                    0, 1,   0,   0,   E::Server,           1,  0,   1,    1,   10, 4,   A::OwnerApply,           0,    0,     S::SlabReduce, S::OwnerApply, S::OwnerApply, S::SlabReduce, S::SlabReduce, 0},
    {"async worker B<=256",                 0, 1,   0,   0,   E::AsyncWorker,      1,  0,   1,    0,   -1, 1,   A::None,                 0,    0,     S::Head,       S::Nobody,     S::Nobody,     S::Nobody,     S::Nobody,     0},
    {"async worker B>256",                  0, 0,   0,   0,   E::AsyncWorker,      1,  0,   0,    0,   -1, 1,   A::None,                 0,    0,     S::Nobody,     S::Nobody,     S::Nobody,     S::Nobody,     S::Nobody,     0},
    {"group step B<=256",                   0, 1,   0,   0,   E::Sharded,          0,  0,   1,    0,   10, 1,   A::OwnerApply,           0,    0,     S::SlabReduce, S::Nobody,     S::Nobody,     S::SlabReduce, S::SlabReduce, 0},
    {"group step B<=256, no exchange",      0, 1,   0,   0,   E::None,             0,  0,   1,    0,   10, 1,   A::AllInApply,           0,    0,     S::SlabReduce, S::Nobody,     S::Nobody,     S::SlabReduce, S::SlabReduce, 0},
    {"group step B>256",                    0, 0,   0,   0,   E::AllReduce,        0,  0,   0,    0,   10, 1,   A::AllInApply,           0,    0,     S::Nobody,     S::Nobody,     S::Nobody,     S::SlabReduce, S::SlabReduce, 0},
};

static void check_table() {
  for (const Row& r : kRows) {
    g_ctx = r.name;
    StepFacts f;
    f.small = r.small; f.b_le_256 = r.b256; f.prio = r.prio; f.adam = r.adam; f.ex = r.ex;
    f.fused_apply_ok = r.fok; f.no_grad_store = r.nogs; f.holds_counter = r.holds;
    f.prefetch = r.prefetch; f.book_period = r.period; f.book_step = r.inc;
    StepPlan p;
    const char* why = "";
    if (!plan_step(f, &p, &why)) {
      ++g_failed;
      printf("FAILED [%s]: refused: %s\n", r.name, why);
      continue;
    }
    const bool same = p.apply == r.apply && p.store_grad == r.store_grad &&
                      p.prio_commit == r.commit && p.bump == r.bump && p.draw == r.draw &&
                      p.gather == r.gather && p.latch == r.latch && p.book == r.book &&
                      p.predrawn() == r.predrawn && p.book_period == r.period &&
                      p.book_step == r.inc;
    if (!same) {
      ++g_failed;
      printf("FAILED [%s]: the plan differs from the table:\n"
             "  plan  apply %s store_grad %d commit %d bump %s draw %s gather %s latch %s book %s "
             "predrawn %d\n"
             "  table apply %s store_grad %d commit %d bump %s draw %s gather %s latch %s book %s "
             "predrawn %d\n",
             r.name, kApply[(int)p.apply], p.store_grad, p.prio_commit, kSite[(int)p.bump],
             kSite[(int)p.draw], kSite[(int)p.gather], kSite[(int)p.latch], kSite[(int)p.book],
             p.predrawn(), kApply[(int)r.apply], r.store_grad, r.commit, kSite[(int)r.bump],
             kSite[(int)r.draw], kSite[(int)r.gather], kSite[(int)r.latch], kSite[(int)r.book],
             r.predrawn);
    }
  }
  printf("%d table rows\n", (int)(sizeof kRows / sizeof kRows[0]));
}

int main() {
  const int ok = enumerate();
  if (ok < 100) {
    ++g_failed;
    printf("FAILED: only %d combinations accepted\n", ok);
  }
  check_table();
  // the plans outside a step
  g_ctx = "plan_apply_only";
  const StepPlan a = plan_apply_only();
  CHECK(a.apply == ApplyRange::AllInApply && a.book == Site::Apply && a.latch == Site::Apply &&
            a.bump == Site::Nobody && a.draw == Site::Nobody && !a.prio_commit,
        "an update outside a step: the apply launch and its own bookkeeping, nothing else");
  g_ctx = "plan_grad_only";
  const StepPlan g = plan_grad_only();
  CHECK(g.apply == ApplyRange::None && g.book == Site::Nobody && g.latch == Site::Nobody &&
            g.bump == Site::Nobody && g.draw == Site::Nobody && !g.prio_commit,
        "forward + backward alone: nobody applies, books, bumps or draws");
  if (g_failed) {
    printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("step plan ok\n");
  return 0;
}
