"""Reference for the checkpoint tests: the section digest restated in numpy
uint64, an independent parser of the checkpoint file, and ``full_state``: every
piece of a net's training state the public getters reach, as bytes.
"""
import json
import struct

import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def splitmix64(x):
    """ddq.actor.splitmix64 on a uint64 array (arithmetic wraps mod 2^64)."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, np.uint64) + GOLDEN
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def digest(data):
    """splitmix64(n) + sum_k splitmix64(w_k ^ ((k + 1) * golden)) over the
    zero-padded little-endian uint64 words w_k of the n bytes."""
    b = np.ascontiguousarray(data).view(np.uint8).ravel()
    n = b.size
    K = (n + 7) // 8
    padded = np.zeros(K * 8, np.uint8)
    padded[:n] = b
    w = padded.view("<u8").astype(np.uint64)
    with np.errstate(over="ignore"):
        k1 = (np.arange(K, dtype=np.uint64) + np.uint64(1)) * GOLDEN
        total = np.add.reduce(splitmix64(w ^ k1), dtype=np.uint64) if K else np.uint64(0)
        return int(splitmix64(np.uint64(n)) + total)


def check_vectors():
    """The digest against ddq.actor.splitmix64, on the scalar definition."""
    from ddq.actor import splitmix64 as sm
    M = (1 << 64) - 1
    for data in (b"", b"\x01", bytes(range(8)), bytes(range(9)), bytes(range(23))):
        n = len(data)
        want = sm(n)
        for k in range((n + 7) // 8):
            w = int.from_bytes(data[8 * k:8 * k + 8].ljust(8, b"\0"), "little")
            want = (want + sm(w ^ (((k + 1) * 0x9E3779B97F4A7C15) & M))) & M
        assert digest(np.frombuffer(data, np.uint8)) == want, n


def parse(path):
    """(header dict, {name: uint8 array}) read with nothing of ddq.checkpoint."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"DDQCKPT1", raw[:8]
    (hlen,) = struct.unpack("<Q", raw[8:16])
    hdr = json.loads(raw[16:16 + hlen].decode())
    secs = {}
    end = 16 + hlen
    for e in hdr["sections"]:
        off, nb = e["offset"], e["bytes"]
        assert off % 64 == 0 and off >= end, e
        assert not any(raw[end:off]), "padding before %s is not zero" % e["name"]
        end = off + nb
        assert end <= len(raw), e
        secs[e["name"]] = np.frombuffer(raw[off:end], np.uint8)
    assert end == len(raw), "bytes after the last section"
    return hdr, secs


def full_state(net, adam=False, prio=False, actor=False, pool=False, device=True):
    """{name: array} of everything the getters reach.  device: the counters
    only the HIP library keeps (iteration through adam_state needs Adam)."""
    net.synchronize()
    out = {"theta_q": net.get_flat(0), "theta_p": net.get_flat(1), "opt": net.optimizer_state(),
           "steps": np.asarray([net.lib.ddq_step_count(net.ctx)], np.int64)}
    if adam:
        m, v, t = net.adam_state()
        out.update(adam_m=m, adam_v=v, adam_t=np.asarray([t], np.int64))
    if net.has_replay:
        st, ac, rw, nt = net.replay_export()
        out.update(ring_state=st, ring_action=ac, ring_reward=rw, ring_nonterm=nt.astype(np.uint8),
                   ring_info=np.asarray(net.replay_info(), np.int64))
        if device:
            out["draws"] = np.asarray([net.replay_draws()], np.int64)
    if prio:
        q, total, pmax = net.replay_priorities()
        out.update(prio_leaf=q, prio_total=np.asarray([total], np.uint64),
                   prio_pmax=np.asarray([pmax], np.uint32))
    if actor:
        boards, stats = net.actor_read()
        out.update(actor_boards=boards, actor_stats=stats)
    if pool:
        boards, stats, totals = net.actors_read()
        out.update(pool_boards=boards, pool_stats=stats, pool_totals=totals)
    # the library's own view: every section's size and digest
    for name, nbytes, dig in net.state_sections():
        out["section " + name] = np.asarray([nbytes, dig], np.uint64)
    return out


def assert_same_state(a, b, what):
    assert list(a) == list(b), "%s: %s vs %s" % (what, list(a), list(b))
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype and x.shape == y.shape, "%s: %s" % (what, name)
        assert x.tobytes() == y.tobytes(), \
            "%s: %s differs in %d of %d elements" % (what, name, int((x != y).sum()), x.size)
