"""Updates per second of the product loop "act, add the transition, train" at an
act / train ratio of 1:1: the single device actor against the actor pool, in one
process.

    python tools/gpu/pool_rate.py [--frame 64] [--batch 32] [--games 32]
                                  [--replay 30000] [--updates 1920] [--warmup 192]
                                  [--reps 3] [--out FILE]

Two contexts with the same weights (64x64, B = 32, rmsprop), the chip preheated
as bench.py preheats it.  Two loops over the same number of updates, each after
a warm-up and with one synchronise at its end, alternated ``reps`` times:

  (b) ``DeviceActor.act_and_step`` on a ``--replay``-slot ring filled as
      bench.py fills it: ``ddq_actor_step_async(1)`` + one graph step per update
      (tools/gpu/acting_rate.py's leg (b));
  (c) ``DeviceActorPool.act_and_train`` at N = ``--games`` on a laned ring of
      the capacity nearest ``--replay`` that N divides (the larger one at a
      tie), filled with the same transitions: per round one lock-step move of N
      games (N transitions), then N updates as one pipelined chain.

``--updates`` is rounded down to a multiple of N.  Prints one JSON line: both
rates (median of the repetitions, all of them listed), (c)/(b), and per loop the
host time spent enqueueing per update.
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


def laned_capacity(replay, lanes):
    lo = replay // lanes * lanes
    return lo if replay - lo < lo + lanes - replay else lo + lanes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--games", type=int, default=32)
    ap.add_argument("--replay", type=int, default=30000)
    ap.add_argument("--updates", type=int, default=1920)
    ap.add_argument("--warmup", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--preheat-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np

    import bench
    import ddq
    from ddq.actor import DeviceActor, DeviceActorPool
    from ddq.params import init_params_flat
    from ddq.snake import SnakeGame

    S, B, N = args.frame, args.batch, args.games
    rounds, wrounds = args.updates // N, max(1, args.warmup // N)
    n = rounds * N
    init = SnakeGame().encode_state()

    single = bench.make_net(B, S, args.replay, 0, 0)
    actor = DeviceActor(single, init, seed=1)

    cap = laned_capacity(args.replay, N)
    laned = ddq.DeepQNet(batch=B, frame=S, device=0)
    theta = init_params_flat(S, seed=42)
    laned.set_flat(0, theta)
    laned.set_flat(1, theta)
    laned.replay_create(cap)
    laned.replay_set_lanes(N)
    st, ac, rw, nt = single.replay_export()
    slot = np.arange(cap) % args.replay
    laned.replay_import(st[slot], ac[slot], rw[slot], nt[slot].astype(np.uint8), 0, cap // N)
    del st
    pool = DeviceActorPool(laned, np.stack([init] * N), seed=1)

    cfgs = {net: net.step_cfg("rmsprop", lr=1e-4, target_period=10, exchange="none", seed=5)
            for net in (single, laned)}
    hot = bench.preheat(B, S, 0, args.preheat_ms)
    it = {single: 0, laned: 0}

    def timed(net, enqueue):
        t0 = time.perf_counter()
        enqueue(it[net])
        t1 = time.perf_counter()
        net.synchronize()
        t2 = time.perf_counter()
        it[net] += n
        return n / (t2 - t0), (t1 - t0) / n * 1e6

    def single_loop():
        return timed(single, lambda i0: actor.act_and_step(cfgs[single], n, i0))

    def pool_loop():
        return timed(laned, lambda i0: pool.act_and_train(cfgs[laned], rounds, i0))

    # warm-up of both shapes: code objects, the graphs' capture + upload
    actor.act_and_step(cfgs[single], wrounds * N, 0)
    pool.act_and_train(cfgs[laned], wrounds, 0)
    single.synchronize()
    laned.synchronize()

    b, c, enq_b, enq_c = [], [], [], []
    for _ in range(args.reps):
        r, e = single_loop()
        b.append(r)
        enq_b.append(e)
        r, e = pool_loop()
        c.append(r)
        enq_c.append(e)
    for net in (single, laned):
        net._check(net.lib.ddq_replay_status(net.ctx))
    sa, sp = actor.stats(), pool.stats()
    rb, rc = statistics.median(b), statistics.median(c)
    keys = ("steps", "games", "reward_sum", "draws")
    out = {
        "metric": "actor_pool_rate", "unit": "updates/s", "frame": S, "batch": B, "rule": "rmsprop",
        "updates_per_loop": n, "warmup": wrounds * N,
        "device_actor": {"value": round(rb, 1), "runs": [round(v, 1) for v in b],
                         "enqueue_us_per_update": [round(v, 1) for v in enq_b],
                         "replay": args.replay,
                         "loop": "DeviceActor.act_and_step: actor_step(1) + step_graph(1)",
                         "actor": {k: sa[k] for k in keys}},
        "actor_pool": {"value": round(rc, 1), "runs": [round(v, 1) for v in c],
                       "enqueue_us_per_update": [round(v, 1) for v in enq_c],
                       "games": N, "replay": cap, "lane_len": cap // N,
                       "loop": "DeviceActorPool.act_and_train: actors_step(1) + "
                               "step_pipelined(%d) per round" % N,
                       "actors": {k: sp[k] for k in keys}},
        "ratio": round(rc / rb, 3),
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
