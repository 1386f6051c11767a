"""Updates per second of the training step at n-step lengths 1, 3 and 8
(ddq_replay_set_nstep), in one process.

    python tools/gpu/nstep_rate.py [--frames 64,16] [--batch 32] [--replay 30000]
                                   [--nsteps 1,3,8] [--steps 2000] [--warmup 100]
                                   [--reps 3] [--out profiles/nstep_rate.json]

Per frame size: one context per n with the same weights and ring (bench.py's
worker, rmsprop), the chip preheated as bench.py preheats it.  Each context
runs a pipelined chain of ``--warmup`` steps, then ``--reps`` timed chains of
``--steps`` steps with one synchronise at the end, the contexts alternated
within every repetition.  Recorded alongside: one profiled step's kernel list
per n (the launches that carry the draw and the gather are in it), so that a
cost above the n = 1 context's own spread can be placed.  Prints one JSON line
and writes it to ``--out``.
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


def measure(S, args, nsteps):
    import bench

    B = args.batch
    nets = {}
    for n in nsteps:
        net = bench.make_net(B, S, args.replay, 0, 0)
        if n != 1:
            net.replay_set_nstep(n)
        assert net.replay_nstep() == n
        nets[n] = net
    cfg = {n: net.step_cfg("rmsprop", lr=1e-4, target_period=10, exchange="none", seed=5)
           for n, net in nets.items()}
    hot = bench.preheat(B, S, 0, args.preheat_ms)
    for n, net in nets.items():
        net.step_pipelined(cfg[n], args.warmup)
        net.synchronize()
    runs = {n: [] for n in nsteps}
    for _ in range(args.reps):
        for n, net in nets.items():
            t0 = time.perf_counter()
            net.step_pipelined(cfg[n], args.steps)
            net.synchronize()
            runs[n].append(args.steps / (time.perf_counter() - t0))
    out = {"frame": S, "batch": B, "small_path": nets[nsteps[0]].small_path()[0],
           "preheat": hot[1] if hot is not None else None, "nstep": {}}
    base = statistics.median(runs[nsteps[0]])
    for n, net in nets.items():
        prof = [net.profile_step(cfg[n]) for _ in range(args.profile_steps)]
        names = [k for k, _ in prof[0]]
        us = [statistics.median(p[i][1] for p in prof) for i in range(len(names))]
        out["nstep"][str(n)] = {"value": round(statistics.median(runs[n]), 1),
                                "runs": [round(v, 1) for v in runs[n]],
                                "vs_n1": round(statistics.median(runs[n]) / base, 4),
                                "kernels": {k: round(u, 2) for k, u in zip(names, us)},
                                "step_device_us": round(sum(us), 2)}
        net._check(net.lib.ddq_replay_status(net.ctx))
    spread = runs[nsteps[0]]
    out["n1_spread"] = [round(min(spread), 1), round(max(spread), 1)]
    if hot is not None:
        hot[0].close()
    for net in nets.values():
        net.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--replay", type=int, default=30000)
    ap.add_argument("--nsteps", default="1,3,8")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nstep_rate.json"))
    args = ap.parse_args()
    nsteps = [int(n) for n in args.nsteps.split(",")]
    out = {"metric": "nstep_rate", "unit": "updates/s", "rule": "rmsprop",
           "steps_per_chain": args.steps, "warmup": args.warmup, "reps": args.reps,
           "mode": "ddq_step_pipelined_async, one context per n alternated per repetition",
           "frames": [measure(int(s), args, nsteps) for s in args.frames.split(",")]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
