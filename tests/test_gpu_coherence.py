"""GPU: every update path must leave the derived weight copies coherent.

tests/_coherence.py's probe after 2, 3 and 4 updates (target_period 3: before
the first P <- Q sync, right after it, and with P one update behind) of every
update site of the step plan (csrc/step_plan.h): the separate apply launch under
every rule, the fused apply of the eager, graph and pipelined steps, Adam's own
launch inside a step, the Double + Huber objective, prioritized replay, the
in-process group's exchanges (both members), every exchange over a one-rank
communicator (the only way to ApplyRange::Fc4InSlabRestInApply), the async
exchange (group tickets and one-rank ticks) and the host paths.  One context per
probe point: the probe overwrites the minibatch set.

Shapes (S, B), the smallest at which each path exists: (16, 8) the small-map
step whose K2 applies fc4's bias and Q_out, (16, 40) the one whose K4 does (B >
32: K2 works in image chunks and K4 sums them),
(24, 4) the general kernels at their smallest frame, (16, 257) the general
kernels at S = 16 behind the two-launch draw (its ring has 512 slots: a 257-draw
does not fit 256).

Combinations plan_step refuses are left out: a prioritized step with an exchange,
Adam with an exchange other than the one-call all-reduce, the async exchange
with Adam.  DESIGN.md section 4 has the copy x site table with these ids.
"""
import pytest

import _coherence as co

pytestmark = pytest.mark.gpu

SMALL, SMALL40, GENERAL, DRAW2 = (16, 8), (16, 40), (24, 4), (16, 257)
FOUR = [SMALL, SMALL40, GENERAL, DRAW2]
TWO = [SMALL, GENERAL]
SEED = 11


def sid(shape):
    return "S%d-B%d" % shape


def cases(*groups):
    """[(regime name, shape, k)] with ids "regime-S16-B8-k2"."""
    out = []
    for names, shapes in groups:
        for name in names:
            for shape in shapes:
                for k in co.PROBES:
                    out.append(pytest.param(name, shape, k, id="%s-%s-k%d" % (name, sid(shape), k)))
    return out


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


def test_shapes_take_the_paths_they_stand_for(ddq):
    for (S, B), small in ((SMALL, True), (SMALL40, True), (GENERAL, False), (DRAW2, False)):
        net = ddq.DeepQNet(batch=B, frame=S)
        assert net.small_path()[0] == small, (S, B, net.small_path())
        net.close()


# ---------------------------------------------------------------- the separate apply launch
@pytest.mark.parametrize("rule,shape,k", cases((["rmsprop"], FOUR),
                                               ([r for r in co.APPLY_RULES if r != "rmsprop"], TWO)))
def test_apply(ddq, rule, shape, k):
    """set_grads_flat + apply: apply_elems in the AllInApply launch, and Adam's
    own launch without and with clipping.  (ddq_apply carries no target period:
    P, set to another initialisation, and its layouts must not move.)"""
    S, B = shape
    co.check_regime(ddq, "apply %s %s" % (rule, sid(shape)),
                    lambda n: co.run_apply(ddq, S, B, rule, n), k, p_fixed=co.theta0(S, seed=43))


# ---------------------------------------------------------------- single-context steps
# name -> (mode, keywords of run_step)
STEP = {
    "eager-rmsprop": ("eager", {}),
    # (the ring's Snake frames are sparse and the loss small: sgd's gradients are
    # about 1e-3, and below lr = 1e-2 a step can leave a conv blob's high terms alone)
    "eager-sgd": ("eager", dict(rule="sgd", lr=0.1)),
    "eager-nostore": ("eager", dict(store_grads=False)),
    "graph-rmsprop": ("graph", {}),
    "pipelined-rmsprop": ("pipelined", {}),
    # Adam moves every weight by about lr whatever the gradient's size
    "eager-adam": ("eager", dict(rule="adam", lr=1e-4)),
    "pipelined-adam": ("pipelined", dict(rule="adam", lr=1e-4)),
    "eager-double-huber": ("eager", dict(objective=("double", "huber", 0.5))),
    "pipelined-double-huber": ("pipelined", dict(objective=("double", "huber", 0.5))),
    "eager-prio": ("eager", dict(prio=True)),
    "pipelined-prio": ("pipelined", dict(prio=True)),
}
# over a one-rank communicator: all-reduce with overlap (general kernels: fc4 in
# the slab reduce, the rest in the apply launch after their all-reduce; small
# path: the whole all-reduce on the comm stream, then the apply launch) and
# without, and the owner apply of the sharded and server exchanges
for _mode in ("eager", "pipelined"):
    for _ex, _ov in (("allreduce", True), ("allreduce", False), ("sharded", False), ("server", False)):
        STEP["comm1-%s-%s%s" % (_mode, _ex, "-overlap" if _ov else "")] = (
            _mode, dict(comm=True, exchange=_ex, overlap=_ov))
COMM1 = [n for n in STEP if n.startswith("comm1-")]


def run_step(ddq, S, B, k, mode, rule="rmsprop", lr=co.LR, store_grads=True, objective=None,
             prio=False, comm=False, exchange="none", overlap=False):
    net = co.make_net(ddq, S, B)
    if objective:
        net.set_objective(*objective)
    if prio:
        net.replay_set_priority(alpha=0.6, beta=0.4, eps=0.01)
    if rule == "adam":
        net.set_adam()
    if comm:
        net.comm_init(ddq.DeepQNet.comm_unique_id(), 1, 0)
    cfg = net.step_cfg(rule, lr=lr, target_period=co.PERIOD, seed=SEED, store_grads=store_grads,
                       exchange=exchange, overlap=overlap)
    if mode == "eager":
        for _ in range(k):
            net.step(cfg)
    elif mode == "graph":
        net.step_graph(cfg, k)
    else:
        net.step_pipelined(cfg, k)     # two buffer sets; at B = 257 the draw on the side stream
    net.synchronize()
    assert net.replay_draws() == k
    return [net]


@pytest.mark.parametrize("name,shape,k", cases(
    (["eager-rmsprop", "graph-rmsprop", "pipelined-rmsprop"], FOUR),
    (["eager-sgd", "eager-nostore", "eager-adam", "pipelined-adam", "eager-double-huber",
      "pipelined-double-huber", "eager-prio", "pipelined-prio"], TWO),
    (COMM1, TWO)))
def test_step(ddq, name, shape, k):
    S, B = shape
    mode, kw = STEP[name]
    co.check_regime(ddq, "step %s %s" % (name, sid(shape)),
                    lambda n: run_step(ddq, S, B, n, mode, **kw), k)


# ---------------------------------------------------------------- in-process group of two
def run_group(ddq, S, B, k, exchange):
    """k group steps.  allreduce and sharded count one iteration a step, so the
    probes fall at iterations 2, 3 and 4.  server counts one per member
    (book_step = W = 2): iterations 4, 6 and 8 -- still none of 1..4 a multiple
    of the period but 6, so again no sync yet, a sync just run, and P one step
    behind."""
    nets = [co.make_net(ddq, S, B, ring_seed=r) for r in range(2)]
    arr = ddq.DeepQNet.group_init(nets)
    cfg = nets[0].step_cfg("rmsprop", lr=co.LR, target_period=co.PERIOD, seed=SEED, exchange=exchange)
    for _ in range(k):
        ddq.DeepQNet.group_step(nets, cfg, arr)
    return nets


@pytest.mark.parametrize("exchange,shape,k", cases((["allreduce", "sharded", "server"], TWO)))
def test_group(ddq, exchange, shape, k):
    """Both members: each applied another shard and copied the other's;
    refresh_kernel then runs over every parameter (the skip range of a rank's own
    shard exists over a communicator only)."""
    S, B = shape
    co.check_regime(ddq, "group %s %s" % (exchange, sid(shape)),
                    lambda n: run_group(ddq, S, B, n, exchange), k)


# ---------------------------------------------------------------- async exchange
def run_async1(ddq, S, B, k):
    """One rank: k ticket ticks are k plain steps (staleness 0,
    tests/test_gpu_async.py): the owner apply writes the mirror and, as
    RefreshOut modes 2 and 3, the worker's layouts."""
    net = co.make_net(ddq, S, B)
    net.comm_init(ddq.DeepQNet.comm_unique_id(), 1, 0)
    cfg = net.step_cfg("rmsprop", lr=co.LR, target_period=co.PERIOD, seed=SEED, exchange="async")
    net.async_begin(cfg)
    for _ in range(k):
        while not net.async_ready():
            pass
        net.async_tick(cfg, 0)
    net.synchronize()
    return [net]


@pytest.mark.parametrize("name,shape,k", cases((["async-world1"], TWO)))
def test_async_world1(ddq, name, shape, k):
    S, B = shape
    co.check_regime(ddq, "async world1 %s" % sid(shape), lambda n: run_async1(ddq, S, B, n), k)


@pytest.mark.parametrize("name,shape,k", cases((["async-group"], TWO)))
def test_async_group(ddq, name, shape, k):
    """group_async_run, two members, k pushes in ticket order: every push is one
    iteration of the central model, and only the pusher pulls (Q always; P when
    a multiple of the period lies in (its last pull, now]).  The order is the
    run's own, so tower 1 is told from it: no sync yet at 2 pushes; at 3 the
    third pusher holds P = its Q, the other the initial P; at 4 a fourth pusher
    other than the third pulls P = the central model of iteration 3, which is
    the third pusher's Q, and a fourth pusher that is the third again keeps the
    P it pulled then.  A member's Q is the model of its last pull."""
    S, B = shape
    nets = [co.make_net(ddq, S, B, ring_seed=r) for r in range(2)]
    try:
        arr = ddq.DeepQNet.group_init(nets)
        cfg = nets[0].step_cfg("rmsprop", lr=co.LR, target_period=co.PERIOD, seed=SEED,
                               exchange="async")
        order = [int(w) for w in ddq.DeepQNet.group_async_run(nets, cfg, k, arr)]
        th0 = co.theta0(S)
        q = [n.get_flat(0) for n in nets]
        want = [th0, th0]
        if k >= 3:
            want[order[2]] = q[order[2]]
        if k == 4 and order[3] != order[2]:
            want[order[3]] = q[order[2]]
        if k == 4 and order[3] == order[2]:
            want[order[3]] = nets[order[3]].get_flat(1)      # (its own: checked to lag below)
            assert want[order[3]].tobytes() not in (th0.tobytes(), q[order[3]].tobytes())
        for r, net in enumerate(nets):
            assert (r in order) == (q[r].tobytes() != th0.tobytes()), (r, order)
            co.check(ddq, net, want[r], "async group %s, %d pushes in order %s, member %d"
                     % (sid(shape), k, order, r))
    finally:
        co.close_all(nets)


# ---------------------------------------------------------------- host paths
@pytest.mark.parametrize("shape", TWO, ids=sid)
@pytest.mark.parametrize("path", co.HOST_PATHS)
def test_host_paths(ddq, path, shape):
    """relayout_kernel after ddq_set_params, and ddq_sync_target's copies, on a
    net that trained for four steps (P one update behind Q)."""
    S, B = shape
    net, = run_step(ddq, S, B, 4, "eager")
    try:
        co.check_host_path(ddq, net, path, "host %s %s" % (path, sid(shape)))
    finally:
        co.close_all([net])


@pytest.mark.parametrize("name,shape,k", cases((["host-loop"], TWO)))
def test_host_loop(ddq, name, shape, k):
    """Updates driven from the host: a host-drawn set, forward_backward, the
    apply launch, ddq_sync_target after every third."""
    S, B = shape
    co.check_regime(ddq, "host loop %s" % sid(shape), lambda n: co.run_host_loop(ddq, S, B, n), k)


# ---------------------------------------------------------------- the harness can fail
@pytest.mark.parametrize("shape", TWO, ids=sid)
def test_mutants_are_detected(ddq, shape):
    """Eight mutant contexts per shape, each with conv weights of one tower one
    update stale: the six single elements and, per tower, conv3's last float4.
    All of them must be told from the coherent context.

    Probe seed 0.  theta and theta_prev come from the host-driven updates
    (run_host_loop), not from ddq_step: in the eager rmsprop steps at (16, 8)
    the conv2 and conv3 weights of largest |delta| -- the ones rmsprop's lagged
    cache throws furthest -- lie in channels that the throw has killed, and no
    probe seed of 0..5 sees them (conv1's, and all eight at (24, 4), are seen at
    every seed).  The mutants test the probe and the fresh contexts, which are
    the same whatever produced the two thetas; the host-driven towers are seen
    at every seed 0..5, at both shapes."""
    S, B = shape
    co.check_mutants(ddq, "host loop %s" % sid(shape), lambda n: co.run_host_loop(ddq, S, B, n),
                     seed=0)
