"""The full pass at the largest shapes ddq_create accepts, checked by an oracle
that sees only a few images.

The float64 oracle (oracle/ref_numpy.py) cannot run 1024 images of 128 x 128.
It does not have to: the minibatch is built so that all but k *live* images add
exactly zero to every gradient.

* In both towers Q_out's weight row and bias of action 3 are zero (``params``).
* A *silent* image has action 3, reward 0 and non_terminal 0: Q_sa = 0 and
  target_Q_sa = 0 exactly, so d = 0, dQ = 0 and every gradient term of the image
  is 0, on the device and in the oracle.
* A live image has an action in {0, 1, 2}, reward and non_terminal drawn as
  tests/test_gpu_parity.make_inputs draws them.
* All B + 1 frames are distinct seeded data, so a vector read from the wrong
  image, or from a halo that should be zero, is a wrong non-zero value.

With B / k a power of two the oracle's pass over the k live images is the
device's pass over all B after its gradients and loss are multiplied by B / k
(exact in fp32); the per-image blobs and the pool routing are compared at the
live rows.  ``LiveRows`` presents exactly that to tests/_parity.check_full_pass,
whose rules apply unchanged.

The frames travel as uint8: a (B + 1)-slot ring (``replay_import``) sampled with
the host indices 0 .. B-1, so image i has state = slot i, next_state = slot
i + 1 and the action, reward and flag of slot i + 1 (replay.py:159-183);
``ReplayRef.gather`` of the live indices is the oracle's view.

``EXTENTS`` lists every device tensor's bytes as a function of (S, B), and
``DESCRIPTORS`` the 32-bit buffer descriptors the general kernels build over
them, by reading csrc/api.hip ddq_create and the kernels.  A descriptor that is
read with the out-of-range offset kOOB = 2^31 (an out-of-image halo vector, a
vector past a row: it must read 0) is right only while its bytes are <= 2^31,
and no descriptor may reach 2^32.  ``accepted`` restates ddq_create's checks.
"""
import collections
import contextlib

import numpy as np

MAX_FRAME, MAX_BATCH = 128, 1024
KOOB = 1 << 31


# ------------------------------------------------------------------ the domain
def refusal(S, B):
    """Why ddq_create refuses (S, B): "range", "32-bit", "frame", or None."""
    if S < 16 or S % 8 or S > 1024 or B < 1 or B > MAX_BATCH:
        return "range"
    if 16 * B * S * S >= KOOB or 2048 * S * S >= KOOB:
        return "32-bit"
    if S > MAX_FRAME:
        return "frame"
    return None


def accepted(S, B):
    return refusal(S, B) is None


def dgrad2_tiles(S):
    """Tiles an image of conv2's data gradient (csrc/kernels.hip kConv2Dgrad
    through pick_tile): one conv1 weight-gradient slab each."""
    H = S // 2
    menu = [(8, 16, 4 * 32), (8, 20, 5 * 32), (12, 12, 5 * 32), (8, 8, 2 * 32)]   # ty, tx, rows

    def tiles(o):
        return -(-H // o[0]) * -(-H // o[1])
    cost = [tiles(o) * (o[2] + 32) for o in menu]
    best = 0
    for i in range(1, len(menu)):
        if 10 * cost[i] < 9 * cost[0] and cost[i] < cost[best]:
            best = i
    return tiles(menu[best])


def _bs2(f):
    return lambda S, B: f * B * S * S


# name -> bytes(S, B); in ddq_create's order.  S2 = S/2 ..: pool1 is
# (B, S2, S2, 32), pool2 (B, S3, S3, 64), pool3 (B, S4, S4, 64).
EXTENTS = collections.OrderedDict([
    ("state / next_state (fp32 NHWC, each)", _bs2(16)),
    ("pool3 (fp32, each tower)", _bs2(4)),
    ("theta = W4 + the rest (each tower)", lambda S, B: 2048 * S * S + 4 * 97060),
    ("pool1f: fp32 pool1 (each tower)", _bs2(32)),
    ("pool2f: fp32 pool2 (each tower)", _bs2(16)),
    ("pool1s: split pool1, three planes", _bs2(48)),
    ("pool2s: split pool2, three planes", _bs2(24)),
    ("mask1", _bs2(8)), ("mask2", _bs2(4)), ("mask3", _bs2(1)),
    ("dconv3: fp32 dpool3 (B, S4, S4, 64) routed to (B, S3, S3, 64)", _bs2(16)),
    ("dconv2s: split dpool2, three planes", _bs2(24)),
    ("dconv3s: split expanded dconv3, three planes", _bs2(24)),
    ("wpart[0]: conv1's weight-gradient slabs", lambda S, B: B * dgrad2_tiles(S) * 32 * 256 * 4),
    ("grad / optimizer state (each)", lambda S, B: 2048 * S * S + 4 * 97060),
    ("act_u8", _bs2(4)), ("act_in", _bs2(16)),
    ("act_p1s: the acting forward's fp32 pool1 (in a split-sized buffer)", _bs2(48)),
    ("act_p2s: the acting forward's fp32 pool2 (likewise)", _bs2(24)),
])

# (name, bytes(S, B), read with kOOB): the descriptors (num_records) of the
# general kernels.  Those of wgrads.h, small_bwd.h and fc.h cover one plane or
# one fp32 tensor each; split.h's rin / rx / rs cover several planes or slabs.
DESCRIPTORS = [
    ("conv2 fwd rin32: fp32 pool1", _bs2(32), True),
    ("conv3 fwd rin32: fp32 pool2", _bs2(16), True),
    ("conv2 fwd rx: split pool1, three planes (stores)", _bs2(48), False),
    ("conv3 fwd rx: split pool2, three planes (stores)", _bs2(24), False),
    ("conv1 / conv2 fwd ro: fp32 pool1 / pool2 (stores)", _bs2(32), False),
    ("conv2 dgrad rin: split dpool2, three planes", _bs2(24), True),
    ("conv2 dgrad rroute: mask2", _bs2(4), True),
    ("conv2 dgrad w1 rr: mask1", _bs2(8), True),
    ("conv2 dgrad w1 rs: conv1's slabs (stores)",
     lambda S, B: B * dgrad2_tiles(S) * 32 * 256 * 4, False),
    ("conv3 dgrad rx: split dconv3, three planes (stores)", _bs2(24), False),
    ("wgrads rin_g: one split pool1 plane", _bs2(16), True),
    ("wgrads rd_g: one split dpool2 / dconv3 plane", _bs2(8), True),
    ("wgrads rm_g: mask2", _bs2(4), True),
    ("fc4 rx: pool3", _bs2(4), True),
    ("fc4 rw: W4", lambda S, B: 2048 * S * S, True),
]


def extents(S, B):
    return collections.OrderedDict((k, f(S, B)) for k, f in EXTENTS.items())


def descriptor_faults(S, B):
    """The descriptors that are wrong at (S, B): [(name, bytes, why)]."""
    out = []
    for name, f, oob in DESCRIPTORS:
        n = f(S, B)
        if n >= 1 << 32:
            out.append((name, n, "num_records wraps 2^32"))
        elif oob and n > KOOB:
            out.append((name, n, "kOOB = 2^31 lies inside it"))
    return out


# ------------------------------------------------------------ the construction
def live_positions(S, B, k, seed):
    """k sorted batch positions for the live images: 0 and B - 1; the image
    holding byte 2^31 of fp32 pool1 and its successor, the image holding byte
    2^31 of the three split dpool2 planes (modulo a plane's B images), where
    they exist; seeded random positions for the rest."""
    assert 2 <= k <= B
    must = [0, B - 1]
    p1 = KOOB // (32 * S * S)                   # fp32 pool1: 32 S^2 bytes an image
    must += [p for p in (p1, p1 + 1) if p < B]
    if 24 * B * S * S > KOOB:                   # a dpool2 plane: 8 S^2 bytes an image
        must.append((KOOB // (8 * S * S)) % B)
    live = []
    for p in must:
        if p not in live and len(live) < k:
            live.append(p)
    rng = np.random.default_rng(seed)
    rest = [p for p in rng.permutation(B) if p not in live]
    live += [int(p) for p in rest[:k - len(live)]]
    return np.sort(np.asarray(live, np.int64))


def params(ref, rng, S):
    """make_params(..., "x3") with action 3 silenced in both towers."""
    from test_gpu_parity import make_params
    pQ, pP = make_params(ref, rng, S, "x3")
    for p, name in ((pQ, "Q_out"), (pP, "P_out")):
        p[name][0].reshape(4, -1)[3] = 0
        p[name][1].reshape(-1)[3] = 0
    return pQ, pP


def draw_frames(rng, n, S, frames):
    """n distinct uint8 frame stacks (n, 4, S, S)."""
    if frames == "uniform":
        return rng.integers(0, 256, (n, 4, S, S), dtype=np.uint8)
    assert frames == "snake"                    # sparse {0, 200, 255}, p = 0.9 / 0.08 / 0.02
    u = rng.integers(0, 100, (n, 4, S, S), dtype=np.uint8)
    lut = np.array([0] * 90 + [200] * 8 + [255] * 2, np.uint8)
    return lut[u]


Case = collections.namedtuple("Case", "S B k live pQ pP ring mb")


def make_case(ref, S, B, k, frames, seed=None):
    """The parameters, the (B + 1)-slot ring as replay_import takes it
    (state, action, reward, non_terminal) and the oracle's minibatch of the
    live rows.  B / k must be a power of two."""
    assert B % k == 0 and (B // k) & (B // k - 1) == 0, (B, k)
    seed = 4000 + S + B if seed is None else seed
    rng = np.random.default_rng(seed)
    pQ, pP = params(ref, rng, S)
    live = live_positions(S, B, k, seed + 1)
    st = draw_frames(rng, B + 1, S, frames)
    # transition i is stored in slot i + 1
    action = np.full(B + 1, 3, np.uint8)
    reward = np.zeros(B + 1, np.int16)
    nonterm = np.zeros(B + 1, np.uint8)
    action[live + 1] = rng.integers(0, 3, k)
    reward[live + 1] = rng.integers(-1, 2, k)
    nonterm[live + 1] = rng.random(k) > 0.2
    if not nonterm[live + 1].any():             # P_sa must not be all zero
        nonterm[live[0] + 1] = 1
    r = ref.ReplayRef((4, S, S), B + 1)
    r.state, r.action, r.reward, r.non_terminal = st, action, reward, nonterm.astype(bool)
    r.head, r.valid = 0, B + 1
    return Case(S, B, k, live, pQ, pP, (st, action, reward, nonterm), r.gather(live))


def full_minibatch(ref, case):
    """The oracle's view of all B rows (small cases only)."""
    st, action, reward, nonterm = case.ring
    r = ref.ReplayRef((4, case.S, case.S), case.B + 1)
    r.state, r.action, r.reward, r.non_terminal = st, action, reward, nonterm.astype(bool)
    r.head, r.valid = 0, case.B + 1
    return r.gather(np.arange(case.B))


def bind(net, case):
    """The case's parameters and minibatch on a DeepQNet of batch B."""
    p = dict(case.pQ)
    p.update(case.pP)
    net.set_params(p)
    net.replay_create(case.B + 1)
    net.replay_import(*case.ring, 0, case.B + 1)
    net.replay_sample(np.arange(case.B, dtype=np.int32))


# ------------------------------------------------------------------ the adapter
class LiveRows:
    """The live rows of a net of batch B as a net of batch k, for
    tests/_parity.check_full_pass: per-image blobs and pool routing at the live
    rows, the loss and the gradients multiplied by B / k."""

    def __init__(self, net, live):
        self.net, self.live = net, np.asarray(live)
        self.batch = len(self.live)
        self.scale = np.float32(net.batch // self.batch)
        assert net.batch % self.batch == 0 and float(self.scale) * self.batch == net.batch
        self.layout = net.layout

    def blob(self, name):
        v = np.asarray(self.net.blob(name))
        if name == "loss":
            return np.float32(v) * self.scale
        return v.reshape(self.net.batch, -1)[self.live]

    def pool_mask(self, layer):
        return self.net.pool_mask(layer)[self.live]

    def get_grads_flat(self):
        return self.net.get_grads_flat() * self.scale

    def split(self, flat, prefix="Q"):
        return self.net.split(flat, prefix)


class OracleNet:
    """A stand-in for a DeepQNet of batch B whose last forward_backward is the
    float64 oracle's pass rounded to fp32 -- or a mutant's, when built inside
    ``mutant(...)``."""

    def __init__(self, ref, pQ, pP, mb):
        self.batch = np.asarray(mb[0]).shape[0]
        S = np.asarray(mb[0]).shape[2]
        blobs, grads, cache = ref.full_pass(pQ, pP, *mb, return_cache=True)
        self.blobs = blobs
        self.masks = {i: ref.route_codes(cache["act%d" % i], cache["arg%d" % i]) for i in (1, 2, 3)}
        self.flat = ref.flatten(grads).astype(np.float32)
        self.layout, o = collections.OrderedDict(), 0
        for name, shapes in ref.param_shapes(S, "Q").items():
            self.layout[name] = []
            for s in shapes:
                n = int(np.prod(s))
                self.layout[name].append((tuple(s), o, n))
                o += n

    def blob(self, name):
        return np.asarray(self.blobs[name], np.float32)

    def pool_mask(self, layer):
        return self.masks[layer]

    def get_grads_flat(self):
        return self.flat.copy()

    def split(self, flat, prefix="Q"):
        return collections.OrderedDict(
            (prefix + name[1:], [flat[o:o + c].reshape(s) for (s, o, c) in blobs])
            for name, blobs in self.layout.items())


# ------------------------------------------------------------------ the mutants
def conv_with_border(x, W, b, pad, border):
    """ref.conv_forward with the padding of image n taken from ``border(n)``, a
    (C, H + 2 pad, W + 2 pad) array (zeros: the convolution itself)."""
    B, C, H, Wd = x.shape
    cout, _, k, _ = W.shape
    Wm = W.reshape(cout, -1)
    top = np.empty((B, cout, H, Wd), np.float64)
    for n in range(B):
        xp = np.array(border(n), np.float64)
        xp[:, pad:pad + H, pad:pad + Wd] = x[n]
        cols = np.empty((C, k, k, H, Wd), np.float64)
        for ky in range(k):
            for kx in range(k):
                cols[:, ky, kx] = xp[:, ky:ky + H, kx:kx + Wd]
        top[n] = (Wm @ cols.reshape(C * k * k, H * Wd)).reshape(cout, H, Wd)
    return top + np.asarray(b, np.float64).reshape(1, cout, 1, 1)


def data_gradient(top_diff, W, pad, border):
    """conv_backward's bottom diff in the gather form the device uses: the top
    diff, padded by ``border``, correlated with the transposed, flipped weights."""
    Wt = np.ascontiguousarray(W.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
    return conv_with_border(top_diff, Wt, np.zeros(Wt.shape[0]), pad, border)


def other_image(x, pad, src):
    """border(n): image src(n) of x, wrapped around: what a halo offset that
    lands inside the tensor returns."""
    return lambda n: np.pad(x[src(n)], ((0, 0), (pad, pad), (pad, pad)), mode="wrap")


@contextlib.contextmanager
def mutant(ref, kind, src):
    """The oracle with conv2 (the 5 x 5 layer) reading another image's values
    where it should read zero padding: kind "forward" in conv2's forward (both
    towers), "dgrad" in its data gradient.  src(n): the image whose values image
    n's halo gets."""
    fwd, bwd = ref.conv_forward, ref.conv_backward

    def conv_forward(x, W, b, pad):
        if W.shape[2] != 5:
            return fwd(x, W, b, pad)
        return conv_with_border(x, W, b, pad, other_image(x, pad, src))

    def conv_backward(x, W, top_diff, pad, need_bottom=True):
        dW, db, dx = bwd(x, W, top_diff, pad, need_bottom)
        if W.shape[2] == 5 and need_bottom:
            dx = data_gradient(top_diff, W, pad, other_image(top_diff, pad, src))
        return dW, db, dx

    if kind == "forward":
        ref.conv_forward = conv_forward
    else:
        assert kind == "dgrad"
        ref.conv_backward = conv_backward
    try:
        yield
    finally:
        ref.conv_forward, ref.conv_backward = fwd, bwd
