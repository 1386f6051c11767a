"""What the device-resident training monitor costs a pipelined training chain.

    python tools/gpu/monitor_rate.py [--frames 64,16] [--batch 32] [--steps 2000]
                                     [--reps 3] [--out profiles/monitor_rate.json]

One process, the chip preheated as bench.py preheats it.  Per frame size three
contexts with bench.py's seeded parameters and replay ring: the monitor off, on
with period 1 (a record every step) and on with period 100 (the launch every
step, its early exit on 99 of 100).  Each runs the shipped step path
(``step_pipelined``: 8-step graphs) for ``steps`` steps, alternated ``reps``
times after one warm-up chain of each; updates/s is steps over the wall time
between two synchronisations.

Also the monitor kernel's own device time inside an eager step
(``ddq_profile_step``, the dispatch's own timestamps; median of 7 steps), with a
record taken and on its early exit, next to its byte floor: the 3 P floats it
reads over the f32 copy rate and over the write-only rate of DESIGN.md's gather
section (4.85 / 6.83 TB/s).

Prints one JSON line.
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

COPY_TBS, WRITE_TBS = 4.85, 6.83     # DESIGN.md, large-batch replay gather


def measure(bench, S, B, steps, reps, preheat_ms):
    replay = 30000 if S >= 64 else 4096
    periods = {"off": None, "period_1": 1, "period_100": 100}
    nets, cfgs = {}, {}
    for k, period in periods.items():
        net = bench.make_net(B, S, replay, 0, 0)
        if period is not None:
            net.monitor_enable(4096, period)
        cfg = net.step_cfg("rmsprop", lr=1e-4, target_period=10, exchange="none", seed=1234)
        net.step_prepare(cfg, "pipelined")
        nets[k], cfgs[k] = net, cfg
    hot = bench.preheat(B, S, 0, preheat_ms)

    def chain(k, n):
        net = nets[k]
        net.synchronize()
        t0 = time.perf_counter()
        net.step_pipelined(cfgs[k], n)
        net.synchronize()
        return n / (time.perf_counter() - t0)

    for k in nets:                                   # warm-up: graphs uploaded, clocks up
        chain(k, 96)
    runs = {k: [] for k in nets}
    for _ in range(reps):
        for k in nets:
            runs[k].append(chain(k, steps))
    res = {k: {"updates_per_s": round(statistics.median(v), 1),
               "updates_per_s_runs": [round(x, 1) for x in v],
               "us_per_step": round(1e6 / statistics.median(v), 2)} for k, v in runs.items()}
    off = res["off"]["us_per_step"]
    for k in ("period_1", "period_100"):
        res[k]["slowdown_vs_off"] = round(res[k]["us_per_step"] / off, 4)
        res[k]["extra_us_per_step"] = round(res[k]["us_per_step"] - off, 2)
        total = nets[k].monitor_read(0, 0)[1]
        res[k]["records_taken"] = int(total)

    # the kernel's own time inside an eager step
    kern = {}
    for k in ("period_1", "period_100"):
        mon, step = [], []
        for _ in range(7):
            prof = nets[k].profile_step(cfgs[k])
            mon.append([us for name, us in prof if name == "monitor"][0])
            step.append(sum(us for _, us in prof))
        kern[k] = {"monitor_us": round(statistics.median(mon), 2),
                   "monitor_us_runs": [round(x, 2) for x in mon],
                   "step_kernels_us": round(statistics.median(step), 2)}
    nbytes = 3 * nets["off"].num_params * 4
    out = {"frame": S, "batch": B, "steps": steps, "reps": reps, "replay": replay,
           "chain": res, "in_step_kernel": kern,
           "bytes_read": nbytes,
           "floor_us_copy_rate": round(nbytes / (COPY_TBS * 1e6), 2),
           "floor_us_write_only_rate": round(nbytes / (WRITE_TBS * 1e6), 2),
           "preheat": hot[1] if hot is not None else None}
    for net in nets.values():
        net.synchronize()
        net.close()
    if hot is not None:
        hot[0].synchronize()
        hot[0].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,16")
    ap.add_argument("--frame", type=int, default=None, help="one frame size only")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import bench
    frames = [args.frame] if args.frame else [int(x) for x in args.frames.split(",")]
    out = {"metric": "monitor_rate",
           "frames": [measure(bench, S, args.batch, args.steps, args.reps, args.preheat_ms)
                      for S in frames]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
