"""GPU: data-parallel gradient exchanges (include/ddq_hip.h enum
ddq_exchange) against the param-server semantics of server.py:196-209.

* In-process groups (ddq_group_init / ddq_group_step): W ctxs on one GPU run
  the same kernels, shard layout and exchange arithmetic as RCCL ranks, with
  the collectives done as device copies -- the sharded and server exchanges
  are checked here against the oracle's update rules:
    server    : theta' = apply(...apply(apply(theta, g_0), g_1)..., g_{W-1})
                (each gradient applied on arrival, in rank order; rmsprop's
                lagged cache and first call carried across them; iteration
                += W per step, so the P <- Q pull check sees W-multiples);
    sharded / allreduce : theta' = apply(theta, sum_r g_r).
* RCCL with a 1-rank communicator: every exchange (incl. the overlapped
  all-reduce inside the step graph) equals the exchange-free step bit-exactly.

B = 8 here.  group_exchange_semantics and rccl_world1_exchange_equals_plain_step
take the batch and the ring size: tests/test_gpu_large_batch.py runs them at
B = 264, past the one-launch draw.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddq():
    import ddq as m
    return m


@pytest.fixture(scope="module")
def ref():
    from oracle import ref_numpy
    return ref_numpy


def apply_ref(ref, rule, theta, g, state, lr):
    if rule == "sgd":
        return ref.sgd_update(theta, g, lr), None
    if rule == "rmsprop":
        return ref.rmsprop_update(theta, g, state, lr)
    return ref.adagrad_update(theta, g, state, lr)


def close(a, b, scale, rtol=1e-5, what=""):
    err = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    tol = rtol * (np.abs(b) + scale)
    assert (err <= tol).all(), "%s: max err %.3g" % (what, err.max())


def make_group(ddq, ref, W, S=16, B=8, N=120, seed=0):
    theta = ref.flatten(ref.init_params(S, seed=21))
    theta = (theta * 3).astype(np.float32)
    nets = []
    for r in range(W):
        rng = np.random.default_rng(seed + r)
        n = ddq.DeepQNet(batch=B, frame=S)
        n.set_flat(0, theta)
        n.set_flat(1, theta)
        n.replay_create(N)
        n.replay_import(rng.integers(0, 256, (N, 4, S, S)).astype(np.uint8),
                        rng.integers(0, 4, N).astype(np.uint8),
                        rng.integers(-1, 2, N).astype(np.int16),
                        (rng.random(N) > 0.1).astype(np.uint8), 0, N)
        nets.append(n)
    arr = ddq.DeepQNet.group_init(nets)
    return nets, arr, theta


@pytest.mark.parametrize("exchange", ["server", "sharded", "allreduce"])
@pytest.mark.parametrize("rule", ["rmsprop", "adagrad", "sgd"])
def test_group_exchange_semantics(ddq, ref, exchange, rule):
    group_exchange_semantics(ddq, ref, exchange, rule)


def group_exchange_semantics(ddq, ref, exchange, rule, B=8, N=120):
    """(tests/test_gpu_large_batch.py runs it at B = 264 on 700-slot rings.)
    Returns the members' final theta_Q."""
    # Two steps: the second runs on the first's optimizer state.  (The lagged
    # rmsprop cache of server.py:86-105 lets a later gradient divide by an
    # earlier, tiny one -- steps of up to lr*|g|*1e4 -- so longer runs at
    # these raw-pixel gradient scales leave the finite range, in the
    # reference as here.)
    W, S, lr = 3, 16, 1e-4
    nets, arr, theta = make_group(ddq, ref, W, S, B, N)
    state = None
    for step in range(2):
        cfg = nets[0].step_cfg(rule, lr=lr, target_period=0, exchange=exchange, seed=40 + step)
        # one cfg (seed) for the group: the members' minibatches differ
        # through their own replay contents
        ddq.DeepQNet.group_step(nets, cfg, arr)
        # per-rank gradients at the common theta, from each rank's own minibatch
        grads = []
        for n in nets:
            st, ac, rw, ns, nt = n.read_minibatch()
            pq, pp = ref.unflatten(theta, S, "Q"), ref.unflatten(n.get_flat(1) if step else theta,
                                                               S, "P")
            _, g = ref.full_pass(pq, pp, st, ac, rw, ns, nt)
            grads.append(ref.flatten(g).astype(np.float32))
        if exchange != "allreduce":           # own gradient stays in the grad buffer
            for n, g in zip(nets, grads):
                close(n.get_grads_flat(), g, np.abs(g).max(), 1e-4, "grad")
        else:                                 # the buffer holds the sum on every rank
            gsum = np.sum(np.stack(grads).astype(np.float64), axis=0)
            for n in nets:
                close(n.get_grads_flat(), gsum, np.abs(gsum).max(), 1e-4, "grad sum")
        # the members agree bit-exactly
        th = [n.get_flat(0) for n in nets]
        for t in th[1:]:
            np.testing.assert_array_equal(t, th[0])
        # oracle apply with the GPU's own gradients where they are observable
        gpu_g = [n.get_grads_flat() for n in nets]
        if exchange == "server":
            want = theta.copy()
            for g in gpu_g:
                want, state = apply_ref(ref, rule, want, g, state, lr)
        elif exchange == "sharded":
            gs = np.sum(np.stack(gpu_g).astype(np.float64), axis=0).astype(np.float32)
            want, state = apply_ref(ref, rule, theta, gs, state, lr)
        else:
            want, state = apply_ref(ref, rule, theta, gpu_g[0], state, lr)
        close(th[0], want, np.abs(theta - want).max() + 1e-30, 1e-3, "theta step %d" % step)
        theta = th[0]
        if state is not None:
            state = np.asarray(state, np.float32)
    for n in nets:
        n.close()
    return theta


def test_group_server_iteration_and_target_sync(ddq, ref):
    """server mode counts W iterations per step; P <- Q when the pull after
    a step sees iteration % period == 0 (server.py:188-189)."""
    W, S = 3, 16
    nets, arr, theta = make_group(ddq, ref, W, S)
    cfg = nets[0].step_cfg("sgd", lr=1e-2, target_period=2, exchange="server", seed=3)
    ddq.DeepQNet.group_step(nets, cfg, arr)      # iteration 3: no sync
    for n in nets:
        assert not np.array_equal(n.get_flat(1), n.get_flat(0))
        np.testing.assert_array_equal(n.get_flat(1), theta)
    ddq.DeepQNet.group_step(nets, cfg, arr)      # iteration 6: sync
    for n in nets:
        np.testing.assert_array_equal(n.get_flat(1), n.get_flat(0))
    for n in nets:
        n.close()


@pytest.mark.parametrize("exchange,overlap", [("allreduce", False), ("allreduce", True),
                                              ("sharded", False), ("server", False)])
def test_rccl_world1_exchange_equals_plain_step(ddq, ref, exchange, overlap):
    rccl_world1_exchange_equals_plain_step(ddq, ref, exchange, overlap)


def rccl_world1_exchange_equals_plain_step(ddq, ref, exchange, overlap, B=8, N=96, lr=1e-3):
    """(tests/test_gpu_large_batch.py runs it at B = 264 on a 700-slot ring.)
    Returns (theta_0, the final theta_Q)."""
    S = 16
    rng = np.random.default_rng(4)
    theta = (ref.flatten(ref.init_params(S, seed=5)) * 3).astype(np.float32)
    st = rng.integers(0, 256, (N, 4, S, S)).astype(np.uint8)
    ac = rng.integers(0, 4, N).astype(np.uint8)
    rw = rng.integers(-1, 2, N).astype(np.int16)
    nt = (rng.random(N) > 0.1).astype(np.uint8)
    nets = [ddq.DeepQNet(batch=B, frame=S) for _ in range(2)]
    for n in nets:
        n.set_flat(0, theta)
        n.set_flat(1, theta)
        n.replay_create(N)
        n.replay_import(st, ac, rw, nt, 0, N)
    nets[0].comm_init(ddq.DeepQNet.comm_unique_id(), 1, 0)
    for i, n in enumerate(nets):
        cfg = n.step_cfg("rmsprop", lr=lr, target_period=3,
                         exchange=exchange if i == 0 else "none", overlap=overlap, seed=9)
        n.step_graph(cfg, 5)
        n.step(cfg)
        # pipelined chains: the next draw + gather on the apply (allreduce:
        # fused slab-reduce launch; sharded / server: the owner-apply launch)
        n.step_pipelined(cfg, 11)
        n.step(cfg)
        n.synchronize()
    for z in (0, 1):
        np.testing.assert_array_equal(nets[0].get_flat(z), nets[1].get_flat(z))
    np.testing.assert_array_equal(nets[0].optimizer_state(), nets[1].optimizer_state())
    out = nets[0].get_flat(0)
    for n in nets:
        n.close()
    return theta, out


def _owner_state(nets):
    """Optimizer state as the owners hold it (shard r on member r)."""
    P = nets[0].num_params
    L = -(-P // (64 * len(nets))) * 64
    out = np.empty(P, np.float32)
    for r, n in enumerate(nets):
        out[r * L:(r + 1) * L] = n.optimizer_state()[r * L:(r + 1) * L]
    return out


@pytest.mark.parametrize("rule", ["rmsprop", "sgd"])
def test_group_async_round_robin_semantics(ddq, ref, rule):
    """DDQ_EXCHANGE_ASYNC on an in-process group (W = 3, 4 rounds, special
    update every 4 iterations) against server.py replayed tick by tick: at
    tick w the central model applies worker w's gradient -- computed on the
    model w pulled one round earlier (staleness W-1) -- on arrival, worker w
    pulls it (and the central P when a special-update pull happened since its
    last pull: server.py:186-189) and computes its next gradient there.
    Round 0 starts from the oracle's own first gradients; later rounds are
    teacher-forced with the GPU's pushed gradients, central model and
    optimizer state, and every new gradient is checked against the oracle at
    the worker's pulled model (tests/_parity.py tolerances)."""
    from _parity import check_full_pass, close as pclose
    W, S, B, N, lr, period = 3, 16, 8, 120, 1e-4, 4
    nets, arr, theta0 = make_group(ddq, ref, W, S, B, N)
    # the bench initialisation (seed-42 fillers, zero biases): make_group's
    # x3 weights leave the finite range within a few lagged-rmsprop rounds
    from ddq.params import init_params_flat
    theta0 = init_params_flat(S, seed=42)
    for n in nets:
        n.set_flat(0, theta0)
        n.set_flat(1, theta0)
    for n in nets:
        n.index_log_enable(16)
    # the members' replay contents (make_group's generator)
    data = []
    for r in range(W):
        rng = np.random.default_rng(0 + r)
        data.append((rng.integers(0, 256, (N, 4, S, S)).astype(np.uint8),
                     rng.integers(0, 4, N).astype(np.uint8),
                     rng.integers(-1, 2, N).astype(np.int16),
                     (rng.random(N) > 0.1).astype(np.uint8)))

    def minibatch(r, draw):
        st, ac, rw, nt = data[r]
        idx = nets[r].index_log(draw, 1)[0].astype(np.int64)
        nx = np.where(idx + 1 == N, 0, idx + 1)
        a = np.zeros((B, 4, 1, 1), np.float32)
        a[np.arange(B), ac[nx], 0, 0] = 1
        return (st[idx].astype(np.float32), a, rw[nx].astype(np.float32).reshape(B, 1, 1, 1),
                st[nx].astype(np.float32), nt[nx].astype(np.float32).reshape(B, 1, 1, 1))

    def apply(th, g, st):
        return apply_ref(ref, rule, th, g, st, lr)

    cfg = nets[0].step_cfg(rule, lr=lr, target_period=period, exchange="async", seed=5)
    central, pc, state, it = theta0.copy(), theta0.copy(), None, 0
    last_pull = [0] * W
    for rnd in range(4):
        prev_p = [n.get_flat(1) for n in nets]
        ddq.DeepQNet.group_step(nets, cfg, arr)
        if rnd == 0:   # the first gradients (draw 0) are the oracle's, on the initial model
            pq, pp = ref.unflatten(theta0, S, "Q"), ref.unflatten(theta0, S, "P")
            pushed = [ref.flatten(ref.full_pass(pq, pp, *minibatch(r, 0))[1]).astype(np.float32)
                      for r in range(W)]
        views, pviews = [], []
        for w in range(W):
            central, state = apply(central, pushed[w], state)
            if state is not None:
                state = np.asarray(state, np.float32)
            it += 1
            if it % period == 0:
                pc = central.copy()
            pull_p = it // period > last_pull[w] // period
            last_pull[w] = it
            views.append(central.copy())
            pviews.append(pc.copy() if pull_p else None)
        # round 0 applied the oracle's first gradients, not the GPU's: rmsprop's
        # lagged cache divides a later gradient by an earlier one, so elements
        # whose first gradient is near 0 amplify that fp32-vs-fp64 difference
        # without bound (server.py:86-105); those rounds check sgd only
        exact_in = rnd > 0 or rule == "sgd"
        for w, n in enumerate(nets):
            gv, gp = n.get_flat(0), n.get_flat(1)
            if exact_in:
                pclose(gv, views[w], what="round %d view %d" % (rnd, w))
            if pviews[w] is not None and exact_in:
                pclose(gp, pviews[w], what="round %d P view %d" % (rnd, w))
            elif pviews[w] is not None:          # P pulled = the central model then
                np.testing.assert_array_equal(gp, nets[w].get_flat(0) if it - W + 1 + w ==
                                              (it - W + 1 + w) // period * period else gp)
            else:                                # no special update since its last pull
                np.testing.assert_array_equal(gp, prev_p[w])
            # the new gradient at the worker's pulled model, on its new minibatch
            check_full_pass(ref, n, ref.unflatten(gv, S, "Q"), ref.unflatten(gp, S, "P"),
                            minibatch(w, rnd + 1), quiet=True, what="round %d w%d " % (rnd, w))
        if state is not None and exact_in:
            pclose(_owner_state(nets), state, what="round %d opt state" % rnd)
        # teacher forcing: the next round starts from the GPU's state
        central = nets[W - 1].get_flat(0)
        pushed = [n.get_grads_flat() for n in nets]
        if state is not None:
            state = _owner_state(nets)
        m = (it // period) * period              # the last special update
        if m > it - W:                           # in this round: tick m - (it - W + 1)
            pc = nets[m - (it - W + 1)].get_flat(1)
    for n in nets:
        n.close()


@pytest.mark.parametrize("rule", ["rmsprop", "adagrad"])
def test_rccl_world1_async_equals_plain_steps(ddq, ref, rule):
    """The RCCL async exchange (point-to-point push / owner apply / pull on
    the comm stream, the gradient on the ctx stream) with one rank: staleness
    0, so R rounds are R plain steps -- bit-identical parameters, P tower
    (special updates every 3 iterations) and optimizer state."""
    S, B, N = 16, 8, 96
    rng = np.random.default_rng(6)
    from ddq.params import init_params_flat
    theta = init_params_flat(S, seed=42)
    st = rng.integers(0, 256, (N, 4, S, S)).astype(np.uint8)
    ac = rng.integers(0, 4, N).astype(np.uint8)
    rw = rng.integers(-1, 2, N).astype(np.int16)
    nt = (rng.random(N) > 0.1).astype(np.uint8)
    nets = [ddq.DeepQNet(batch=B, frame=S) for _ in range(2)]
    for n in nets:
        n.set_flat(0, theta)
        n.set_flat(1, theta)
        n.replay_create(N)
        n.replay_import(st, ac, rw, nt, 0, N)
    nets[0].comm_init(ddq.DeepQNet.comm_unique_id(), 1, 0)
    for i, n in enumerate(nets):
        cfg = n.step_cfg(rule, lr=1e-4, target_period=3, exchange="async" if i == 0 else "none",
                         seed=9)
        for _ in range(7):
            n.step(cfg)
        n.synchronize()
    for z in (0, 1):
        np.testing.assert_array_equal(nets[0].get_flat(z), nets[1].get_flat(z))
    np.testing.assert_array_equal(nets[0].optimizer_state(), nets[1].optimizer_state())
    for n in nets:
        n.close()
