"""Updates per second of the training step with prioritized replay on and off
(ddq_replay_set_priority), in one process.

    python tools/gpu/per_rate.py [--frames 64,16] [--batch 32] [--capacities 4096,1048576]
                                 [--steps 2000] [--warmup 100] [--reps 3]
                                 [--out profiles/per_rate.json]

Per frame size and ring capacity: two contexts with the same weights and ring
(bench.py's worker and parameters, rmsprop; the ring tiled on the device from
4096 synthetic transitions), one with prioritization on (alpha 0.6, beta 0.4,
eps 0.01), the chip preheated as bench.py preheats it.  Each context runs a
pipelined chain of ``--warmup`` steps, then ``--reps`` timed chains of
``--steps`` steps with one synchronise at the end, the two alternated within
every repetition.  Recorded alongside: the eager per-kernel device times of one
profiled step (median of ``--profile-steps``), which list the new launches
"prio_sample", "gather" and "prio_commit".  Prints one JSON line and writes it
to ``--out``.
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

PRIO = dict(alpha=0.6, beta=0.4, eps=0.01)


def make_net(B, S, capacity, prio):
    import numpy as np

    import ddq
    from ddq.expgain import synthetic_transitions
    from ddq.params import init_params_flat
    net = ddq.DeepQNet(batch=B, frame=S, device=0)
    theta = init_params_flat(S, seed=42)
    net.set_flat(0, theta)
    net.set_flat(1, theta)
    net.replay_create(capacity)
    st, ac, rw, nt = synthetic_transitions(min(capacity, 4096), S, seed=1000)
    net.replay_fill_tiled(st, ac, rw, nt.astype(np.uint8), 0, capacity)
    if prio:
        net.replay_set_priority(**PRIO)
    return net


def measure(S, capacity, args):
    import bench

    B = args.batch
    nets = {"off": make_net(B, S, capacity, False), "on": make_net(B, S, capacity, True)}
    cfg = {k: net.step_cfg("rmsprop", lr=1e-4, target_period=10, exchange="none", seed=5)
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
    out = {"frame": S, "batch": B, "capacity": capacity, "small_path": nets["off"].small_path()[0],
           "preheat": hot[1] if hot is not None else None, "priority": {}}
    base = statistics.median(runs["off"])
    for k, net in nets.items():
        prof = [net.profile_step(cfg[k]) for _ in range(args.profile_steps)]
        names = [n for n, _ in prof[0]]
        us = [statistics.median(p[i][1] for p in prof) for i in range(len(names))]
        out["priority"][k] = {"value": round(statistics.median(runs[k]), 1),
                              "runs": [round(v, 1) for v in runs[k]],
                              "vs_off": round(statistics.median(runs[k]) / base, 4),
                              "step_us": round(1e6 / statistics.median(runs[k]), 2),
                              "kernels": [[n, round(u, 2)] for n, u in zip(names, us)],
                              "step_device_us": round(sum(us), 2)}
        net._check(net.lib.ddq_replay_status(net.ctx))
    q, total, pmax = nets["on"].replay_priorities()
    out["priority"]["on"]["leaves_distinct"] = int(len(set(q.tolist())))
    out["priority"]["on"]["total"] = total
    out["priority"]["on"]["pmax"] = pmax
    out["off_spread"] = [round(min(runs["off"]), 1), round(max(runs["off"]), 1)]
    if hot is not None:
        hot[0].close()
    for net in nets.values():
        net.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--capacities", default="4096,1048576")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_rate.json"))
    args = ap.parse_args()
    out = {"metric": "per_rate", "unit": "updates/s", "rule": "rmsprop", "priority": PRIO,
           "steps_per_chain": args.steps, "warmup": args.warmup, "reps": args.reps,
           "mode": "ddq_step_pipelined_async, an enabled and a disabled context alternated per "
                   "repetition",
           "cases": [measure(int(s), int(c), args) for s in args.frames.split(",")
                     for c in args.capacities.split(",")]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
