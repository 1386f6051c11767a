"""Updates per second of the training step with soft target updates
(ddq_set_target_tau) beside the hard copy, in one process.

    python tools/gpu/soft_target_rate.py [--frames 64,16] [--batch 32] [--steps 2000]
                                         [--warmup 100] [--reps 3]
                                         [--out profiles/soft_target_rate.json]

Per frame size three contexts with the same weights and ring (bench.py's worker
and parameters; a 4096-slot ring of synthetic transitions), the chip preheated
as bench.py preheats it:

  hard_p10   tau = 1, target_period 10: the default step (a copy every tenth update)
  hard_p1    tau = 1, target_period 1: P <- Q after every update
  soft_p1    tau = 0.005, target_period 1: P <- P + tau (Q - P) after every update

hard_p1 against hard_p10 is the cost of writing P and its conv copies every
step; soft_p1 against hard_p1 is the cost of the blend itself: one more read of
every parameter's old P (17.5 MB at 64x64) and three flops.  Each context runs a
pipelined chain of ``--warmup`` steps, then ``--reps`` timed chains of
``--steps`` steps with one synchronise at the end, the three alternated within
every repetition.  Recorded alongside: the eager per-kernel device times of one
profiled step (median of ``--profile-steps``).  Prints one JSON line and writes
it to ``--out``.
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
TAU = 0.005
# name -> (tau, target_period)
CONFIGS = {"hard_p10": (1.0, 10), "hard_p1": (1.0, 1), "soft_p1": (TAU, 1)}


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
    net.set_target_tau(CONFIGS[name][0])
    return net


def measure(S, args):
    import bench

    B = args.batch
    nets = {k: make_net(B, S, k) for k in CONFIGS}
    cfg = {k: net.step_cfg("rmsprop", lr=1e-4, target_period=CONFIGS[k][1], seed=5)
           for k, net in nets.items()}
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
    out = {"frame": S, "batch": B, "capacity": CAPACITY, "small_path": nets["hard_p10"].small_path()[0],
           "preheat": hot[1] if hot is not None else None, "configs": {}}
    base = statistics.median(runs["hard_p10"])
    for k, net in nets.items():
        prof = [net.profile_step(cfg[k]) for _ in range(args.profile_steps)]
        names = [n for n, _ in prof[0]]
        us = [statistics.median(p[i][1] for p in prof) for i in range(len(names))]
        med = statistics.median(runs[k])
        out["configs"][k] = {"tau": CONFIGS[k][0], "target_period": CONFIGS[k][1],
                             "value": round(med, 1), "runs": [round(v, 1) for v in runs[k]],
                             "vs_hard_p10": round(med / base, 4), "step_us": round(1e6 / med, 2),
                             "kernels": [[n, round(u, 2)] for n, u in zip(names, us)],
                             "step_device_us": round(sum(us), 2)}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_target_rate.json"))
    args = ap.parse_args()
    out = {"metric": "soft_target_rate", "unit": "updates/s", "tau": TAU,
           "steps_per_chain": args.steps, "warmup": args.warmup, "reps": args.reps,
           "mode": "ddq_step_pipelined_async, the three contexts alternated per repetition",
           "cases": [measure(int(s), args) for s in args.frames.split(",")]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
