"""The cost of a checkpoint: the section digest's read rate and a full save and
load, in one process.

    python tools/gpu/checkpoint_rate.py [--frame 64] [--batch 32] [--slots 30000]
                                        [--reps 20] [--dir /dev/shm] [--large-slots 330000]
                                        [--out profiles/checkpoint_rate.json]

* ``digest``: ``ddq_state_digest`` on ``ring_state`` of the bench ring (30,000
  slots at 64x64: 491 MB) and on ``theta_q``: the median host time of ``--reps``
  calls, each of which synchronises, runs the two digest launches and copies
  eight bytes back, so a small section's figure is the call's overhead, not a
  rate.  Beside it, in the same process, a read-only stream of torch's own
  (``sum`` of an int32 view of 2 GiB) and its copy: the ceiling the digest, a
  read-only stream with two 64-bit hashes per 16 bytes, is judged against.
* ``save`` / ``load``: ``save_checkpoint`` and ``ddq.checkpoint.restore`` of that
  net on ``--dir`` (a tmpfs path: the file system is not what is measured).
* ``large``: once, a ring past 4 GiB (``--large-slots`` slots filled by
  ``replay_fill_tiled`` from a pool of 1,000) must give the reference digest,
  computed here from the pool tile by tile in numpy; its time is the digest
  kernel's rate with the call's overhead amortised.  0 skips it.

Prints one JSON line and writes it to ``--out``.
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

POOL = 1000
GOLDEN = 0x9E3779B97F4A7C15


def make_net(B, S, slots, pool):
    import numpy as np

    import ddq
    from ddq.expgain import synthetic_transitions
    from ddq.params import init_params_flat
    net = ddq.DeepQNet(batch=B, frame=S, device=0)
    theta = init_params_flat(S, seed=42)
    net.set_flat(0, theta)
    net.set_flat(1, theta)
    net.replay_create(slots)
    st, ac, rw, nt = synthetic_transitions(pool, S, seed=1000)
    net.replay_fill_tiled(st, ac, rw, nt.astype(np.uint8), 0, slots)
    return net, np.ascontiguousarray(st, np.uint8)


def splitmix64(x):
    import numpy as np
    with np.errstate(over="ignore"):
        x = x + np.uint64(GOLDEN)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def tiled_digest(pool_bytes, slots, pool):
    """The digest of `slots` slots, slot i the pool's entry i % pool, without
    the tiled image: the pool's words meet another index term in every tile."""
    import numpy as np
    words = pool_bytes.reshape(-1).view("<u8").astype(np.uint64)       # whole words: 4 S^2 % 8 == 0
    per_slot = words.size // pool
    n_bytes = slots * per_slot * 8
    total = splitmix64(np.uint64(n_bytes))
    k1 = np.arange(1, words.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for t in range(0, slots, pool):
            m = min(pool, slots - t) * per_slot
            idx = (k1[:m] + np.uint64(t * per_slot)) * np.uint64(GOLDEN)
            total = total + np.add.reduce(splitmix64(words[:m] ^ idx), dtype=np.uint64)
    return int(total)


def time_digest(net, name, reps):
    from ddq import checkpoint
    checkpoint.state_digest(net, name)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        d = checkpoint.state_digest(net, name)
        ts.append(time.perf_counter() - t0)
    return d, statistics.median(ts), min(ts)


def torch_read_ceiling():
    import torch
    n = 1 << 29
    a = torch.ones(n, device="cuda", dtype=torch.int32)
    b = torch.empty_like(a)

    def t(fn, nbytes, it=10):
        fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(it):
            fn()
        e.record()
        torch.cuda.synchronize()
        return nbytes / (s.elapsed_time(e) * 1e-3 / it) / 1e12
    out = {"read_sum_int32_TBps": round(t(lambda: a.sum(), 4 * n), 3),
           "copy_int32_TBps": round(t(lambda: b.copy_(a), 8 * n), 3), "bytes": 4 * n}
    del a, b
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--slots", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--large-slots", type=int, default=330000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_rate.json"))
    args = ap.parse_args()
    from ddq import checkpoint
    if not os.access(args.dir, os.W_OK):      # no tmpfs there: the figure then includes the disk
        import tempfile
        args.dir = tempfile.gettempdir()
    S = args.frame
    out = {"metric": "checkpoint_rate", "frame": S, "batch": args.batch, "slots": args.slots,
           "reps": args.reps, "ceiling": torch_read_ceiling(), "digest": {}}
    net, pool = make_net(args.batch, S, args.slots, POOL)
    sizes = {n: b for n, b, _ in net.state_sections()}
    for name in ("ring_state", "theta_q"):
        d, med, best = time_digest(net, name, args.reps)
        out["digest"][name] = {"bytes": sizes[name], "median_us": round(med * 1e6, 1),
                               "min_us": round(best * 1e6, 1),
                               "GBps_median": round(sizes[name] / med / 1e9, 1),
                               "GBps_best": round(sizes[name] / best / 1e9, 1)}
        if name == "ring_state":
            want = tiled_digest(pool, args.slots, POOL)
            out["digest"][name]["equals_reference"] = d == want
            assert d == want, "ring_state digest %016x, reference %016x" % (d, want)
    path = os.path.join(args.dir, "ddq_checkpoint_rate.%d.ckpt" % os.getpid())
    try:
        t0 = time.perf_counter()
        net.save_checkpoint(path, meta={"tool": "checkpoint_rate"})
        t_save = time.perf_counter() - t0
        nbytes = os.path.getsize(path)
        net.close()
        t0 = time.perf_counter()
        net, _ = checkpoint.restore(path)
        t_load = time.perf_counter() - t0
    finally:
        if os.path.exists(path):
            os.unlink(path)
    out["file"] = {"dir": args.dir, "bytes": nbytes, "save_s": round(t_save, 3),
                   "load_s": round(t_load, 3), "save_GBps": round(nbytes / t_save / 1e9, 2),
                   "load_GBps": round(nbytes / t_load / 1e9, 2),
                   "load_includes": "ddq_create, ring allocation, write, commit, device digests"}
    net.close()
    if args.large_slots:
        big, pool = make_net(args.batch, S, args.large_slots, POOL)
        nb = args.large_slots * 4 * S * S
        d, med, best = time_digest(big, "ring_state", 3)
        t0 = time.perf_counter()
        want = tiled_digest(pool, args.large_slots, POOL)
        out["large"] = {"slots": args.large_slots, "bytes": nb, "past_4GiB": nb > (1 << 32),
                        "equals_reference": d == want, "median_us": round(med * 1e6, 1),
                        "GBps_median": round(nb / med / 1e9, 1), "GBps_best": round(nb / best / 1e9, 1),
                        "reference_s": round(time.perf_counter() - t0, 1)}
        big.close()
        assert d == want, "large ring digest %016x, reference %016x" % (d, want)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
