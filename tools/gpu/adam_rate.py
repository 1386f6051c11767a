"""Updates per second of the training step under the Adam rule, with and without
gradient clipping, beside the default rmsprop step, in one process.

    python tools/gpu/adam_rate.py [--frames 64,16] [--batch 32] [--steps 2000]
                                  [--warmup 100] [--reps 3] [--out profiles/adam_rate.json]

Per frame size four contexts with the same weights and ring (bench.py's worker
and parameters; a 4096-slot ring of synthetic transitions), the chip preheated
as bench.py preheats it:

  rmsprop          the default step: every update inside the slab-reduce launch
  rmsprop_unfused  the same rule on the sequencing an Adam step takes: gradient
                   launches, then the apply launch (a world-1 all-reduce without
                   overlap; the one-rank all-reduce call is part of it)
  adam             DDQ_RULE_ADAM, clipping off
  adam_clip        DDQ_RULE_ADAM, max_grad_norm 10 ("grad_norm" launch added)

Each context runs a pipelined chain of ``--warmup`` steps, then ``--reps`` timed
chains of ``--steps`` steps with one synchronise at the end, the four alternated
within every repetition.  Recorded alongside: the eager per-kernel device times
of one profiled step (median of ``--profile-steps``).  fused - unfused rmsprop is
the step cost of leaving the fused path; the "adam_apply" launch against the
unfused "apply" launch of the same run is the cost of the rule itself (7 words
per parameter moved against 5).  Prints one JSON line and writes it to ``--out``.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "distributed-deep-q_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CAPACITY = 4096
CLIP = 10.0
CONFIGS = ("rmsprop", "rmsprop_unfused", "adam", "adam_clip")


def make_net(B, S, name):
    import numpy as np

    import ddq
    from ddq.expgain import synthetic_transitions
    from ddq.params import init_params_flat
    net = ddq.DeepQNet(batch=B, frame=S, device=0)
    theta = init_params_flat(S, seed=42)
    net.set_flat(0, theta)
    net.set_flat(1, theta)
    net.replay_create(CAPACITY)
    st, ac, rw, nt = synthetic_transitions(CAPACITY, S, seed=1000)
    net.replay_fill_tiled(st, ac, rw, nt.astype(np.uint8), 0, CAPACITY)
    if name == "rmsprop_unfused":
        net.comm_init(ddq.DeepQNet.comm_unique_id(), 1, 0)
    if name.startswith("adam"):
        net.set_adam(max_grad_norm=CLIP if name == "adam_clip" else 0.0)
    return net


def step_cfg(net, name):
    rule = "adam" if name.startswith("adam") else "rmsprop"
    ex = "allreduce" if name == "rmsprop_unfused" else "none"
    return net.step_cfg(rule, lr=1e-4, target_period=10, exchange=ex, overlap=False, seed=5)


def measure(S, args):
    import bench

    B = args.batch
    nets = {k: make_net(B, S, k) for k in CONFIGS}
    cfg = {k: step_cfg(net, k) for k, net in nets.items()}
    hot = bench.preheat(B, S, 0, args.preheat_ms)
    for k, net in nets.items():
        net.step_pipelined(cfg[k], args.warmup)
        net.synchronize()
    runs = {k: [] for k in nets}
    for _ in range(args.reps):
        for k, net in nets.items():
            t0 = time.perf_counter()
            net.step_pipelined(cfg[k], args.steps)
            net.synchronize()
            runs[k].append(args.steps / (time.perf_counter() - t0))
    out = {"frame": S, "batch": B, "capacity": CAPACITY, "small_path": nets["rmsprop"].small_path()[0],
           "preheat": hot[1] if hot is not None else None, "configs": {}}
    base = statistics.median(runs["rmsprop"])
    for k, net in nets.items():
        prof = [net.profile_step(cfg[k]) for _ in range(args.profile_steps)]
        names = [n for n, _ in prof[0]]
        us = [statistics.median(p[i][1] for p in prof) for i in range(len(names))]
        spread = [[round(min(p[i][1] for p in prof), 2), round(max(p[i][1] for p in prof), 2)]
                  for i in range(len(names))]
        med = statistics.median(runs[k])
        out["configs"][k] = {"value": round(med, 1), "runs": [round(v, 1) for v in runs[k]],
                             "vs_rmsprop": round(med / base, 4), "step_us": round(1e6 / med, 2),
                             "kernels": [[n, round(u, 2)] for n, u in zip(names, us)],
                             "kernel_spread": spread, "step_device_us": round(sum(us), 2)}
        net._check(net.lib.ddq_replay_status(net.ctx))
    if hot is not None:
        hot[0].close()
    for net in nets.values():
        net.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_rate.json"))
    args = ap.parse_args()
    out = {"metric": "adam_rate", "unit": "updates/s", "clip": CLIP,
           "steps_per_chain": args.steps, "warmup": args.warmup, "reps": args.reps,
           "mode": "ddq_step_pipelined_async, the four contexts alternated per repetition",
           "cases": [measure(int(s), args) for s in args.frames.split(",")]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
