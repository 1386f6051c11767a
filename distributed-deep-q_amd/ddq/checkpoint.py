"""Checkpoint and bit-exact resume of a DeepQNet (include/ddq_hip.h ddq_state_*).

A checkpoint is one file:

    b"DDQCKPT1"                      magic
    uint64 little-endian             length H of the header
    H bytes                          JSON header
    sections, raw                    each at a 64-byte aligned file offset

The header holds ``{"version": 1, "mode": "gpu" | "cpu", "meta": {...},
"sections": [{"name", "bytes", "digest", "offset"}, ...]}``; ``digest`` is the
library's section digest as a decimal string (a uint64 does not fit a JSON
number everywhere).  Sections are streamed through ``ddq_state_read`` /
``ddq_state_write`` in chunks of at most 64 MiB, so a ring of any size passes
through a small staging buffer.  A file is written to ``path + ".tmp"``,
fsynced and moved into place with ``os.replace``: a reader never sees a partial
file.  Files are portable between the HIP library and the CPU twin.
"""
from __future__ import annotations

import ctypes
import json
import os
import struct

import numpy as np

from . import _lib
from ._lib import ptr

MAGIC = b"DDQCKPT1"
VERSION = 1
ALIGN = 64
CHUNK = 64 << 20
MAX_SECTIONS = 16


class CheckpointError(RuntimeError):
    """A checkpoint could not be written, read or restored."""


def _align(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def state_sections(net):
    """[(name, bytes, digest)] of ``net``: every section the ctx has, in the
    library's fixed order, with its digest (ddq_state_sections)."""
    arr = (_lib.StateSection * MAX_SECTIONS)()
    n = _lib._i32()
    net._check(net.lib.ddq_state_sections(net.ctx, arr, MAX_SECTIONS, ctypes.byref(n)))
    return [(s.name.decode(), int(s.bytes), int(s.digest)) for s in arr[:n.value]]


def state_read(net, name, offset=0, nbytes=None):
    """Bytes [offset, offset + nbytes) of a section as a uint8 array."""
    if nbytes is None:
        sizes = {s[0]: s[1] for s in _sizes(net)}
        if name not in sizes:
            raise KeyError(name)
        nbytes = sizes[name] - offset
    out = np.empty(int(nbytes), np.uint8)
    net._check(net.lib.ddq_state_read(net.ctx, name.encode(), int(offset), ptr(out), out.size))
    return out


def state_write(net, name, data, offset=0):
    data = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray))
                                else data).view(np.uint8).ravel()
    net._check(net.lib.ddq_state_write(net.ctx, name.encode(), int(offset), ptr(data), data.size))


def state_commit(net):
    net._check(net.lib.ddq_state_commit(net.ctx))


def state_digest(net, name):
    d = _lib._u64()
    net._check(net.lib.ddq_state_digest(net.ctx, name.encode(), ctypes.byref(d)))
    return int(d.value)


def _sizes(net):
    """[(name, bytes)] (they come with the digests, which are cheap beside any file I/O)."""
    return [(s[0], s[1]) for s in state_sections(net)]


def save(net, path, meta=None):
    """Write ``net``'s whole training state to ``path`` (atomically)."""
    meta = {} if meta is None else meta
    try:
        secs = state_sections(net)
    except _lib.DDQError as e:
        raise CheckpointError("cannot read the state: %s" % e) from e
    entries = [{"name": n, "bytes": b, "digest": str(d), "offset": 0} for n, b, d in secs]

    def header(first):
        off = first
        for e in entries:
            e["offset"] = off
            off = _align(off + e["bytes"])
        return json.dumps({"version": VERSION, "mode": net.mode, "meta": meta,
                           "sections": entries}, sort_keys=True).encode()

    # the offsets are part of the header whose length decides them: iterate to a fixed point
    first = _align(len(MAGIC) + 8 + len(header(0)))
    while True:
        h = header(first)
        need = _align(len(MAGIC) + 8 + len(h))
        if need == first:
            break
        first = need
    tmp = path + ".tmp"
    buf = np.empty(min(CHUNK, max(b for _, b, _ in secs)), np.uint8)
    try:
        with open(tmp, "wb") as f:
            f.write(MAGIC)
            f.write(struct.pack("<Q", len(h)))
            f.write(h)
            for e in entries:
                f.write(b"\0" * (e["offset"] - f.tell()))
                done = 0
                while done < e["bytes"]:
                    k = min(buf.size, e["bytes"] - done)
                    net._check(net.lib.ddq_state_read(net.ctx, e["name"].encode(), done,
                                                      ptr(buf), k))
                    f.write(memoryview(buf[:k]))
                    done += k
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException as e:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        if isinstance(e, _lib.DDQError):
            raise CheckpointError("cannot read the state: %s" % e) from e
        raise
    return entries


def read_header(path):
    """(header dict, file size).  Checks the magic, the header and that every
    section lies inside the file, aligned and in order."""
    try:
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(len(MAGIC) + 8)
            if len(head) < len(MAGIC) + 8 or head[:len(MAGIC)] != MAGIC:
                raise CheckpointError("%s: not a checkpoint (bad magic)" % path)
            (hlen,) = struct.unpack("<Q", head[len(MAGIC):])
            if hlen > size - len(head):
                raise CheckpointError("%s: truncated header" % path)
            raw = f.read(hlen)
    except OSError as e:
        raise CheckpointError("%s: %s" % (path, e)) from e
    try:
        hdr = json.loads(raw.decode())
        secs = hdr["sections"]
        if hdr["version"] != VERSION:
            raise CheckpointError("%s: version %r (this reader: %d)" % (path, hdr["version"], VERSION))
        end = len(MAGIC) + 8 + hlen
        for e in secs:
            name, nb, off = e["name"], int(e["bytes"]), int(e["offset"])
            int(e["digest"])
            if not isinstance(name, str) or nb <= 0 or off % ALIGN or off < end:
                raise CheckpointError("%s: bad section entry %r" % (path, e))
            end = off + nb
            if end > size:
                raise CheckpointError("%s: truncated: section %s ends at byte %d of %d"
                                      % (path, name, end, size))
    except (KeyError, TypeError, ValueError, UnicodeDecodeError) as e:
        raise CheckpointError("%s: bad header (%s)" % (path, e)) from e
    return hdr, size


def read_section(path, hdr, name):
    """A section's bytes from the file (uint8 array)."""
    for e in hdr["sections"]:
        if e["name"] == name:
            with open(path, "rb") as f:
                f.seek(int(e["offset"]))
                return np.frombuffer(f.read(int(e["bytes"])), np.uint8)
    raise KeyError(name)


def load(net, path):
    """Restore ``net`` -- configured as the writer was -- from ``path``; returns
    the writer's ``meta``.  Raises CheckpointError; after a failure past the
    first section the net stays "restoring" (load again, or discard it)."""
    hdr, _ = read_header(path)
    try:
        mine = _sizes(net)
        theirs = [(e["name"], int(e["bytes"])) for e in hdr["sections"]]
        if not theirs or theirs[0][0] != "config":
            raise CheckpointError("%s: no config section" % path)
        net_cfg = read_section(path, hdr, "config")
        # the fingerprint first: it names what differs, the size list could only say that something does
        state_write(net, "config", net_cfg)
        if mine != theirs:
            raise CheckpointError("%s: the file's sections %r are not this net's %r"
                                  % (path, theirs, mine))
        buf = np.empty(min(CHUNK, max(b for _, b in theirs)), np.uint8)
        with open(path, "rb") as f:
            for e in hdr["sections"][1:]:
                f.seek(int(e["offset"]))
                done, total = 0, int(e["bytes"])
                while done < total:
                    k = min(buf.size, total - done)
                    if f.readinto(memoryview(buf[:k])) != k:
                        raise CheckpointError("%s: short read in section %s" % (path, e["name"]))
                    net._check(net.lib.ddq_state_write(net.ctx, e["name"].encode(), done,
                                                       ptr(buf), k))
                    done += k
        state_commit(net)
        got = {n: d for n, _, d in state_sections(net)}
    except _lib.DDQError as e:
        raise CheckpointError("%s: %s" % (path, e.msg)) from e
    for e in hdr["sections"]:
        if got[e["name"]] != int(e["digest"]):
            raise CheckpointError("%s: section %s is corrupt: digest %016x, the file's header says %016x"
                                  % (path, e["name"], got[e["name"]], int(e["digest"])))
    if getattr(net, "has_replay", None) is not None:
        net.has_replay = any(n == "ring_state" for n, _ in theirs)
    return hdr.get("meta", {})


def config_of(path):
    """The checkpoint's ``config`` section as a numpy record (STATE_CONFIG_DTYPE)."""
    hdr, _ = read_header(path)
    raw = read_section(path, hdr, "config")
    if raw.size != _lib.STATE_CONFIG_DTYPE.itemsize:
        raise CheckpointError("%s: config section of %d bytes" % (path, raw.size))
    return raw.view(_lib.STATE_CONFIG_DTYPE)[0], hdr


def restore(path, device=0, mode="gpu", setup=None):
    """Build a net from the checkpoint's ``config`` -- batch, frame, gamma, ring,
    lanes, n-step, priority, objective, Adam and tau through the usual setters
    --, call ``setup(net)`` (create the DeviceActor or DeviceActorPool the
    writer had there), load, and return ``(net, meta)``."""
    from .net import DeepQNet
    k, _ = config_of(path)
    gamma = float(np.array([k["gamma_bits"]], "<u4").view("<f4")[0])
    net = DeepQNet(batch=int(k["batch"]), frame=int(k["frame"]), device=device, gamma=gamma,
                   mode=mode)
    try:
        if k["capacity"]:
            net.replay_create(int(k["capacity"]))
            if k["lanes"] > 1:
                net.replay_set_lanes(int(k["lanes"]))
            if k["nstep"] > 1:
                net.replay_set_nstep(int(k["nstep"]))
            if k["prio_enabled"]:
                net.replay_set_priority(alpha=float(k["prio_alpha"]), beta=float(k["prio_beta"]),
                                        eps=float(k["prio_eps"]))
        if k["obj_target"] or k["obj_loss"]:
            names = lambda d, v: next(n for n, x in d.items() if x == v)  # noqa: E731
            net.set_objective(names(_lib.TARGETS, int(k["obj_target"])),
                              names(_lib.LOSSES, int(k["obj_loss"])),
                              float(k["huber_delta"]) if k["obj_loss"] else 1.0)
        if k["adam_on"]:
            net.set_adam(float(k["adam_beta1"]), float(k["adam_beta2"]), float(k["adam_eps"]),
                         float(k["adam_max_grad_norm"]))
        if float(k["target_tau"]) != 1.0:
            net.set_target_tau(float(k["target_tau"]))
        if setup is not None:
            setup(net)
        meta = load(net, path)
    except BaseException:
        net.close()
        raise
    return net, meta
