#!/usr/bin/env python3
"""Cost of the Munchausen / soft-Q target against the default and the double
target: updates/s of the bench's pipelined graph step (bench.py's worker, ring and
timing, driven through DeepQNet) at 64x64 B = 32 and deepq16, each variant on a
ctx of its own, the variants alternated over several rounds (median reported).

    python tools/munchausen_cost.py [--steps 2000] [--warmup 200] [--rounds 5]
        [--variants off,soft,munchausen,double] [--out FILE.json]

A tree without ddq_set_munchausen (the parent commit) runs ``--variants
off,double``.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distributed-deep-q_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SET = {"off": lambda net: None,
       "soft": lambda net: net.set_munchausen(alpha=0.0, tau=0.03),
       "munchausen": lambda net: net.set_munchausen(alpha=0.9, tau=0.03, clip=-1.0),
       "double": lambda net: net.set_objective("double")}


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default="off,soft,munchausen,double")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    variants = args.variants.split(",")
    res = {}
    for S, B, replay in ((64, 32, 30000), (16, 32, 30000)):
        nets = {}
        for v in variants:
            net = bench.make_net(B, S, replay, 0, 0)
            SET[v](net)
            cfg = net.step_cfg("rmsprop", lr=1e-4, target_period=10, seed=1234)
            net.step_prepare(cfg, "pipelined")
            net.step_pipelined(cfg, args.warmup)
            net.synchronize()
            nets[v] = (net, cfg)
        rates = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v in variants:
                net, cfg = nets[v]
                t0 = time.perf_counter()
                net.step_pipelined(cfg, args.steps)
                net.synchronize()
                rates[v].append(args.steps / (time.perf_counter() - t0))
        res["%dx%d B=%d" % (S, S, B)] = {
            v: {"updates_per_s": round(float(np.median(r)), 1),
                "min": round(min(r), 1), "max": round(max(r), 1)} for v, r in rates.items()}
        for net, _ in nets.values():
            net.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
