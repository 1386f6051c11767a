"""Updates per second of the training step under each TD objective
(ddq_set_objective) against the default {MAX, EUCLIDEAN}, in one process.

    python tools/gpu/objective_rate.py [--frames 64,16] [--batch 32] [--replay 30000]
                                       [--steps 2000] [--warmup 100] [--reps 3]
                                       [--out profiles/objective_rate.json]

Per frame size: four contexts with the same weights and ring (bench.py's worker,
rmsprop), one per objective -- {max, double} x {euclidean, huber delta 1} -- the
chip preheated as bench.py preheats it.  Each context runs a pipelined chain of
``--warmup`` steps, then ``--reps`` timed chains of ``--steps`` steps with one
synchronise at the end, the four objectives alternated within every repetition.
Recorded alongside: one profiled step's kernel list per objective, the extra
forward's own device time (the sum of its "qn_" entries) and the wall time of a
synchronous ``ddq_forward_q`` (the same kernels plus one launch + synchronise
round trip of the host).  Prints one JSON line and writes it to ``--out``.
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

OBJECTIVES = [("max", "euclidean"), ("max", "huber"), ("double", "euclidean"), ("double", "huber")]


def measure(S, args):
    import bench

    B = args.batch
    nets = {}
    for obj in OBJECTIVES:
        net = bench.make_net(B, S, args.replay, 0, 0)
        if obj != OBJECTIVES[0]:
            net.set_objective(obj[0], obj[1], 1.0)
        nets[obj] = net
    cfg = {o: n.step_cfg("rmsprop", lr=1e-4, target_period=10, exchange="none", seed=5)
           for o, n in nets.items()}
    hot = bench.preheat(B, S, 0, args.preheat_ms)
    for o, n in nets.items():
        n.step_pipelined(cfg[o], args.warmup)
        n.synchronize()
    runs = {o: [] for o in OBJECTIVES}
    for _ in range(args.reps):
        for o, n in nets.items():
            t0 = time.perf_counter()
            n.step_pipelined(cfg[o], args.steps)
            n.synchronize()
            runs[o].append(args.steps / (time.perf_counter() - t0))
    out = {"frame": S, "batch": B, "small_path": nets[OBJECTIVES[0]].small_path()[0],
           "preheat": hot[1] if hot is not None else None, "objectives": {}}
    base = statistics.median(runs[OBJECTIVES[0]])
    for o, n in nets.items():
        prof = [n.profile_step(cfg[o]) for _ in range(args.profile_steps)]
        names = [k for k, _ in prof[0]]
        us = [statistics.median(p[i][1] for p in prof) for i in range(len(names))]
        qn = sum(u for k, u in zip(names, us) if k.startswith("qn_"))
        rec = {"value": round(statistics.median(runs[o]), 1),
               "runs": [round(v, 1) for v in runs[o]],
               "vs_default": round(statistics.median(runs[o]) / base, 4),
               "kernels": {k: round(u, 2) for k, u in zip(names, us)},
               "step_device_us": round(sum(us), 2),
               "extra_forward_us": round(qn, 2)}
        if o[0] == "double":
            k = 200
            n.forward_q()
            t0 = time.perf_counter()
            for _ in range(k):
                n.forward_q()
            rec["forward_q_wall_us"] = round((time.perf_counter() - t0) / k * 1e6, 2)
        out["objectives"]["%s+%s" % o] = rec
        n._check(n.lib.ddq_replay_status(n.ctx))
    spread = runs[OBJECTIVES[0]]
    out["default_spread"] = [round(min(spread), 1), round(max(spread), 1)]
    if hot is not None:
        hot[0].close()
    for n in nets.values():
        n.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--replay", type=int, default=30000)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objective_rate.json"))
    args = ap.parse_args()
    out = {"metric": "objective_rate", "unit": "updates/s", "rule": "rmsprop",
           "steps_per_chain": args.steps, "warmup": args.warmup, "reps": args.reps,
           "mode": "ddq_step_pipelined_async, four contexts alternated per repetition",
           "frames": [measure(int(s), args) for s in args.frames.split(",")]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
