"""Updates per second of the product loop "act once, add the transition, train
once" (main.py:61-103), host actor against device actor, in one process.

    python tools/gpu/acting_rate.py [--frame 64] [--batch 32] [--replay 30000]
                                    [--updates 2000] [--warmup 200] [--reps 3]

One context (64x64, B = 32, rmsprop, 30,000-slot ring filled as bench.py
fills it), the chip preheated as bench.py preheats it.  Two loops over the
same number of updates, each after a warm-up and with one synchronise at its
end, alternated ``reps`` times:

  (a) bench.py's ``acting_rate`` loop: eager step + batch-1 ``select_action``
      + ``replay_add`` per update (two stream synchronisations and the small
      copies per update);
  (b) ``DeviceActor.act_and_step``: ``ddq_actor_step_async`` + one graph step
      per update, nothing but enqueues.

Prints one JSON line: both rates (median of the repetitions, all of them
listed), their ratio, and for (b) the host time spent enqueueing per update
(the loop's wall time before its synchronise), which bounds it from below
when the host is the limit.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--replay", type=int, default=30000)
    ap.add_argument("--updates", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import bench
    from ddq.actor import DeviceActor
    from ddq.snake import SnakeGame

    S, B, n = args.frame, args.batch, args.updates
    net = bench.make_net(B, S, args.replay, 0, 0)
    cfg = net.step_cfg("rmsprop", lr=1e-4, target_period=10, exchange="none", seed=5)
    actor = DeviceActor(net, SnakeGame().encode_state(), seed=1)
    hot = bench.preheat(B, S, 0, args.preheat_ms)

    def host_loop():
        # bench.acting_rate warms itself up (5 updates) and synchronises once
        return bench.acting_rate(net, cfg, S, iters=n)["value"]

    it = [0]

    def device_loop():
        t0 = time.perf_counter()
        actor.act_and_step(cfg, n, it[0])
        t1 = time.perf_counter()
        net.synchronize()
        t2 = time.perf_counter()
        it[0] += n
        return n / (t2 - t0), (t1 - t0) / n * 1e6

    # warm-up of both shapes: code objects, the step graph's capture + upload
    bench.acting_rate(net, cfg, S, iters=args.warmup)
    actor.act_and_step(cfg, args.warmup, 0)
    net.synchronize()

    a, b, enq = [], [], []
    for _ in range(args.reps):
        a.append(host_loop())
        r, e = device_loop()
        b.append(r)
        enq.append(e)
    net._check(net.lib.ddq_replay_status(net.ctx))
    st = actor.stats()
    ra, rb = statistics.median(a), statistics.median(b)
    out = {
        "metric": "acting_rate", "unit": "updates/s", "frame": S, "batch": B,
        "replay": args.replay, "rule": "rmsprop", "updates_per_loop": n, "warmup": args.warmup,
        "host_actor": {"value": round(ra, 1), "runs": [round(v, 1) for v in a],
                       "loop": "eager step + batch-1 select_action + replay_add per update"},
        "device_actor": {"value": round(rb, 1), "runs": [round(v, 1) for v in b],
                         "enqueue_us_per_update": [round(v, 1) for v in enq],
                         "loop": "DeviceActor.act_and_step: actor_step(1) + step_graph(1)"},
        "ratio": round(rb / ra, 3),
        "actor": {k: st[k] for k in ("steps", "games", "reward_sum", "draws")},
        "preheat": hot[1] if hot is not None else None,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
