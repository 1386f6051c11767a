// The step layer's helpers that more than one host unit calls: what a step
// of (ctx, cfg) is, its checks, and the enqueue of its parts.  Each is defined
// once, without `static`, in the unit named; none is exported from the library.
#pragma once
#include <functional>

#include "ctx.h"

#pragma GCC visibility push(hidden)
namespace ddq {

// api.hip
int check_cfg(ddq_ctx* c, const ddq_update_cfg* u);
UpdateRule rule_of(const ddq_update_cfg& u, int period);
int enqueue_apply(ddq_ctx* c, const NetBuffers& nb, const StepLaunch& sl, Marks m = {});
int enqueue_fwd_bwd(ddq_ctx* c, const NetBuffers& nb, const StepLaunch& sl, Marks m = {},
                    Fc4Done fc4_done = {}, const NetBuffers* prio_next = nullptr,
                    uint64_t prio_seed = 0);
// api_step.hip
void count_steps(ddq_ctx* c, const ddq_step_cfg* cfg, int n);
bool is_async(const ddq_ctx* c, const ddq_step_cfg* cfg);
int check_not_async(ddq_ctx* c);
StepFacts step_facts(const ddq_ctx* c, const ddq_step_cfg* cfg);
int plan_launches(ddq_ctx* c, const ddq_step_cfg* cfg, const StepFacts& f, StepLaunch* sl);
int enqueue_draw(ddq_ctx* c, const NetBuffers& nb, uint64_t seed, hipStream_t stream, Marks m = {});
int enqueue_step(ddq_ctx* c, const ddq_step_cfg* cfg, Marks m = {}, bool fault = false);
int initial_target_sync(ddq_ctx* c, const ddq_step_cfg* cfg);
int check_step(ddq_ctx* c, const ddq_step_cfg* cfg);
int check_monitor_step(ddq_ctx* c, const ddq_step_cfg* cfg);
int capture_exec(ddq_ctx* c, hipGraphExec_t* out, const std::function<int()>& body,
                 const char* async_what = nullptr);
// api_exchange.hip: the async exchange's steps, for ddq_step_async and
// ddq_step_graph_async
int async_prepare(ddq_ctx* c, const ddq_step_cfg* cfg);
int async_round_eager(ddq_ctx* c, const ddq_step_cfg* cfg);
int async_graph_steps(ddq_ctx* c, const ddq_step_cfg* cfg, int nsteps);

}  // namespace ddq
#pragma GCC visibility pop
