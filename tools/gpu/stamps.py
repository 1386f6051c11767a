"""Phase stamps of a DDQ_STAMPS variant build (common.h DDQ_STAMP): run a few
eager forward/backward passes at the given frame / batch and print, per stamp
slot, the median time since the workgroup's own slot 0 and since the earliest
slot-0 stamp of the launch (the launch's start).

Usage: DDQ_LIB_PATH=<variant .so> python tools/gpu/stamps.py [S] [B] [reps] [fb|step]
("step": the bench's pipelined graph step, rmsprop with the fused apply)"""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "distributed-deep-q_amd"))
import ddq  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 16
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
mode = sys.argv[4] if len(sys.argv) > 4 else "fb"
SLOTS, BLOCKS = 58, 640

net = ddq.DeepQNet(batch=B, frame=S)
rng = np.random.default_rng(0)
st = rng.integers(0, 256, (B, 4, S, S)).astype(np.float32)
ns = rng.integers(0, 256, (B, 4, S, S)).astype(np.float32)
act = np.eye(4, dtype=np.float32)[rng.integers(0, 4, B)].reshape(B, 4, 1, 1)
net.write_minibatch(st, act, rng.standard_normal((B, 1, 1, 1)).astype(np.float32), ns,
                    np.ones((B, 1, 1, 1), np.float32))
lib = net.lib
lib.ddq_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int64]
buf = np.zeros(SLOTS * BLOCKS, np.uint64)
runs = []
if mode == "step":
    from ddq.params import init_params_flat
    theta = init_params_flat(S, seed=42)
    net.set_flat(0, theta)
    net.set_flat(1, theta)
    N = 4096
    net.replay_create(N)
    net.replay_import(rng.integers(0, 256, (N, 4, S, S)).astype(np.uint8),
                      rng.integers(0, 4, N).astype(np.uint8), rng.integers(-1, 2, N).astype(np.int16),
                      (rng.random(N) > 0.05).astype(np.uint8), 0, N)
    cfg = net.step_cfg("rmsprop", lr=1e-4, target_period=10, seed=1234)
    net.step_prepare(cfg, "pipelined")
    net.step_pipelined(cfg, 20)
for r in range(reps + 2):
    if mode == "step":
        net.step_pipelined(cfg, 1)
        net.synchronize()
    else:
        net.forward_backward()
    assert lib.ddq_debug_stamps(buf.ctypes.data, buf.size) == 0
    if r >= 2:
        runs.append(buf.reshape(BLOCKS, SLOTS).astype(np.int64).copy())
for r, t in enumerate(runs):
    # kernels stamp disjoint slot ranges (small.h: K1 0..7, K3 8..15, K2
    # 16..23, K4 conv2 tiles 24..31, conv3 tiles 32..39)
    for lo in (0, 8, 16, 24, 32, 40, 42):
        tt = t[t[:, lo] > 0]
        if not len(tt):
            continue
        t0 = tt[:, lo].min()
        seq = [16, 17, 18, 19, 20, 44, 45, 46, 21, 22, 23] if lo == 16 else \
            ([lo, lo + 1, lo + 2, lo + 3, lo + 4, lo + 6, lo + 5] if lo in (24, 32) else
             range(lo, lo + (2 if lo >= 40 else 8)))
        used = [k for k in seq if (tt[:, k] > 0).any()]
        # each slot over the workgroups that wrote it (K2's P-tower workgroups
        # leave after slot 18; an unwritten slot is 0, not a time)
        rel = {}
        for k in used:
            w = tt[tt[:, k] > 0]
            rel[k] = (np.median(w[:, k] - w[:, lo]) * 10 / 1000, (w[:, k].max() - t0) * 10 / 1000)
        print("run %d slots %d+: %d blocks, span %.2f us; slot: median since own start / last "
              "since launch start (us): %s" % (r, lo, len(tt), (tt[:, used].max() - t0) * 10 / 1000,
                                            " ".join("%d:%.2f/%.2f" % (k, a, b) for k, (a, b) in rel.items())))
# the conv2 + conv3 weight-gradient pair (wgrads.h): per unit kind (conv2's
# slots 48..50, conv3's 51..53: entry, wave 0's last row done, exit; conv2's
# bias units 55, 56: entry, exit) the times
# since the launch's first entry, and from slot 54 (the hardware id) how the
# units share the CUs and how many waves a SIMD holds over the launch
for r, t in enumerate(runs):
    u = t.astype(np.uint64)
    kinds = [(name, lo, np.nonzero(t[:, lo] > 0)[0]) for name, lo in (("conv2", 48), ("conv3", 51))]
    if not any(len(b) for _, _, b in kinds):
        continue
    t0 = min(t[b, lo].min() for _, lo, b in kinds if len(b))
    t1 = max(max(t[b, lo + 2].max() for _, lo, b in kinds if len(b)), t[:, 56].max())
    us = lambda v: (v - t0) * 10 / 1000
    print("pair run %d: launch span %.2f us" % (r, us(t1)))
    for name, lo, b in kinds:
        if not len(b):
            continue
        e, d, x = us(t[b, lo]), us(t[b, lo + 1]), us(t[b, lo + 2])
        print("  %s: %d units; entry median %.2f max %.2f; rows done median %.2f max %.2f; "
              "exit min %.2f median %.2f max %.2f; own length median %.2f us"
              % (name, len(b), np.median(e), e.max(), np.median(d), d.max(), x.min(),
                 np.median(x), x.max(), np.median(x - e)))
    # conv2's units by tap row (block L: ky = ((L >> 3) % (2 * 5)) % 5): which of
    # them set the launch's end
    b2 = kinds[0][2]
    for ky in range(5 if len(b2) else 0):
        bk = b2[((b2 >> 3) % 10) % 5 == ky]
        d, x = us(t[bk, 49]), us(t[bk, 50])
        print("  conv2 ky %d: %d units; rows done median %.2f max %.2f; exit min %.2f median %.2f "
              "max %.2f" % (ky, len(bk), np.median(d), d.max(), x.min(), np.median(x), x.max()))
    # conv2's bias units (slots 55, 56: entry, exit), dispatched behind conv3's
    bb = np.nonzero(t[:, 55] > 0)[0]
    if len(bb):
        e, x = us(t[bb, 55]), us(t[bb, 56])
        print("  conv2 bias units: %d; entry min %.2f median %.2f max %.2f; exit min %.2f median "
              "%.2f max %.2f; own length median %.2f us"
              % (len(bb), e.min(), np.median(e), e.max(), x.min(), np.median(x), x.max(),
                 np.median(x - e)))
    hw = u[:, 54]
    has = np.nonzero((hw >> np.uint64(62)) & np.uint64(1))[0]
    if not len(has):
        continue
    # CU key: (xcc, se, sh, cu); a workgroup's waves spread over the CU's 4 SIMDs
    key = {int(b): (int(hw[b] >> np.uint64(32)) & 15, int(hw[b] >> np.uint64(13)) & 7,
                    int(hw[b] >> np.uint64(12)) & 1, int(hw[b] >> np.uint64(8)) & 15) for b in has}
    waves = {int(b): (int(hw[b] >> np.uint64(48)) & 63) for b in has}
    c2 = set(int(b) for b in kinds[0][2])
    per_cu = {}
    for b, k in key.items():
        per_cu.setdefault(k, []).append(b)
    h2 = np.bincount([sum(b in c2 for b in bl) for bl in per_cu.values()])
    ha = np.bincount([len(bl) for bl in per_cu.values()])
    print("  CUs used %d; CUs by conv2 units held: %s; by workgroups held: %s" % (
        len(per_cu), " ".join("%d:%d" % (i, n) for i, n in enumerate(h2) if n),
        " ".join("%d:%d" % (i, n) for i, n in enumerate(ha) if n)))
    # CU-time by resident waves per SIMD (workgroup waves / 4), entry to exit
    share = {}
    for bl in per_cu.values():
        ev = []
        for b in bl:
            ent = min(t[b, lo] for lo in (48, 51, 55) if t[b, lo] > 0)
            ext = max(t[b, lo + (1 if lo == 55 else 2)] for lo in (48, 51, 55) if t[b, lo] > 0)
            ev += [(ent, waves[b] / 4.0), (ext, -waves[b] / 4.0)]
        ev.sort()
        cur, last = 0.0, t0
        for when, dw in ev:
            share[cur] = share.get(cur, 0) + (when - last)
            cur, last = cur + dw, when
        share[0.0] = share.get(0.0, 0) + (t1 - last)
    tot = float(sum(share.values()))
    print("  used CUs' time by waves per SIMD: %s" % " ".join(
        "%g:%.1f%%" % (k, 100 * v / tot) for k, v in sorted(share.items())))
# the meeting tiles' arrival skew: per K4 block (conv2 24.., conv3 32..) the
# pre-meeting stamp since the launch's start, slowest first
for lo, name in ((24, "conv2"), (32, "conv3")):
    t = runs[-1]
    if not (t[:, lo] > 0).any():
        continue
    t0 = t[t[:, 16 if lo == 0 else 24] > 0][:, 24].min() if (t[:, 24] > 0).any() else 0
    sel = np.nonzero((t[:, lo] > 0) & (t[:, lo + 3] > 0))[0]
    arr = sorted(((t[b, lo + 3] - t0) * 10 / 1000, b, [(t[b, lo + k] - t[b, lo]) * 10 / 1000 for k in range(1, 6)])
                 for b in sel)[::-1]
    print("%s pre-meeting arrivals (us since launch), slowest 6: %s" % (
        name, "; ".join("blk %d at %.2f (own: %s)" % (b, a, " ".join("%.2f" % x for x in o)) for a, b, o in arr[:6])))
    print("  median %.2f, fastest %.2f" % (arr[len(arr) // 2][0], arr[-1][0]))
