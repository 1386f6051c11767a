"""Cost of parameter-space noise (ddq_set_param_noise), in one process.

    python tools/gpu/param_noise_rate.py [--frames 64,16] [--batch 32] [--replay 2000]
                                         [--calls 200] [--reps 5] [--moves 2000]
                                         [--out profiles/param_noise_rate.json]

Per frame size:
* a resample (one launch: theta~ and its split conv copies) against the
  two-launch baseline kept in this tool only -- an elementwise perturb
  (torch.randn_like, mul, add on the device) followed by launch_relayout, reached
  through ddq_set_params(on_dev=1) into a second context -- both timed per call
  with the synchronise each needs (one against two, plus torch's dispatch), in
  alternated pairs: a host-synced call cost, not a kernel time; and the
  resample's device time (``--calls`` enqueued, one synchronise), which the
  baseline has no counterpart of (ddq_set_params synchronises);
* the stream floor: 8 P bytes (P floats read, P written) at ``--hbm`` bytes/s;
* the device actor's moves per second with the feature off and with
  resample_every in {0, 1, 64}, contexts alternated within every repetition.
Prints one JSON line and writes it to ``--out``.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "distributed-deep-q_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e6


def measure(S, args):
    import torch

    import bench
    from ddq.actor import DeviceActor
    from ddq.snake import SnakeGame
    import random

    B = args.batch
    net, other = bench.make_net(B, S, args.replay, 0, 0), bench.make_net(B, S, args.replay, 0, 0)
    P = net.num_params
    net.set_param_noise(0.05, seed=1)
    theta = torch.from_numpy(net.get_flat(0)).cuda()

    def one_launch():
        net.param_noise_resample()
        net.synchronize()

    def two_launch():
        pert = theta + 0.05 * torch.randn_like(theta)
        torch.cuda.synchronize()
        other._check(other.lib.ddq_set_params(other.ctx, 0, ctypes.c_void_p(pert.data_ptr()), P, 1))

    for fn in (one_launch, two_launch):
        timed(fn, 20)
    pairs = [(timed(one_launch, args.calls), timed(two_launch, args.calls)) for _ in range(args.reps)]

    def chain():
        for _ in range(args.calls):
            net.param_noise_resample()
        net.synchronize()

    dev = [timed(chain, 1) / args.calls for _ in range(args.reps)]
    out = {"frame": S, "params": P,
           "resample_us_per_call_synced": [round(a, 2) for a, _ in pairs],
           "two_launch_us_per_call_synced": [round(b, 2) for _, b in pairs],
           "one_vs_two": round(statistics.median(a / b for a, b in pairs), 4),
           "resample_device_us": [round(v, 2) for v in dev],
           "stream_floor_us": round(8.0 * P / args.hbm * 1e6, 2)}
    net.close()
    other.close()
    # the device actor: moves / s
    init = SnakeGame(random.Random(0)).encode_state()
    modes = {"off": None, "every0": 0, "every1": 1, "every64": 64}
    nets = {}
    for name, k in modes.items():
        n = bench.make_net(B, S, args.replay, 0, 0)
        if k is not None:
            n.set_param_noise(0.05, seed=1, resample_every=k)
        DeviceActor(n, init, 21)
        n.actor_step(100, 60000)
        n.synchronize()
        nets[name] = n
    runs = {name: [] for name in modes}
    for _ in range(args.reps):
        for name, n in nets.items():
            t0 = time.perf_counter()
            n.actor_step(args.moves, 60000)
            n.synchronize()
            runs[name].append(args.moves / (time.perf_counter() - t0))
    base = statistics.median(runs["off"])
    out["actor_moves_per_s"] = {name: {"runs": [round(v, 1) for v in r],
                                       "vs_off": round(statistics.median(r) / base, 4)}
                                for name, r in runs.items()}
    for n in nets.values():
        n.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--replay", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--moves", type=int, default=2000)
    ap.add_argument("--hbm", type=float, default=8.0e12, help="HBM bytes/s of the stream floor")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_noise_rate.json"))
    args = ap.parse_args()
    out = {"metric": "param_noise_rate", "calls": args.calls, "reps": args.reps, "hbm": args.hbm,
           "frames": [measure(int(s), args) for s in args.frames.split(",")]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
