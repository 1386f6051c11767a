"""Float64 restatement of parameter-space noise (include/ddq_hip.h): the normals
from the same 64-bit words, the softmax KL, the oracle forward, and the bounds."""
import numpy as np

from _actor_host import seeded_theta
from _parity import ELEM_ATOL, ELEM_FLOOR, NORM_RTOL, RTOL, error_figures

SALT, SEED = 0x8EBC6AF09C88C6E3, 0x5EED0123456789AB
EPS_REF, COEF = 0.05, 1.01
DELTA = float(-np.log(1.0 - EPS_REF + EPS_REF / 4.0))
U = np.uint64


def mix(x):
    x = x + U(0x9E3779B97F4A7C15)
    x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
    return x ^ (x >> U(31))


def eps(n, epoch, seed=SEED):
    """The n normals of (seed, epoch) in float64."""
    with np.errstate(over="ignore"):
        j = np.arange((n + 1) // 2, dtype=U)
        w = mix(U(seed ^ SALT) ^ mix(U(epoch) * U(0x100000001B3) + j * U(0x9E37)))
    u1 = ((w >> U(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = ((w >> U(16)) & U(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return np.stack([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], 1).ravel()[:n]


def check_draw(got, theta, sigma, epoch, what=""):
    """|theta~ - (theta + sigma eps)| <= sigma 1e-5 + 2^-23 |ref|: sqrt / log at <= 2 ulp and
    the fp32 angle are <= 7e-6 absolute on eps at r <= 5.8; 2^-23: the final add."""
    want = theta.astype(np.float64) + sigma * eps(theta.size, epoch)
    err = np.abs(got.astype(np.float64) - want)
    tol = sigma * 1e-5 + 2.0 ** -23 * np.abs(want)
    print("%s draw: max err / tol %.3g" % (what, float(np.max(err / tol))))
    assert np.all(err <= tol), (what, int(np.argmax(err / tol)))


def check_draws(net, theta, sigma, what):
    """Epochs 0 and 1 against the reference; they differ; epoch 0 again: the same bits."""
    net.set_param_noise(sigma, seed=SEED)
    e0 = net.param_noise_params()
    net.param_noise_resample()
    e1 = net.param_noise_params()
    check_draw(e0, theta, sigma, 0, what)
    check_draw(e1, theta, sigma, 1, what)
    assert np.mean(e0 != e1) > 0.99
    net.set_param_noise(sigma, seed=SEED)
    assert np.array_equal(net.param_noise_params(), e0)


def kl(q, qn):
    q, qn = (np.asarray(x, np.float64).reshape(-1, 4) for x in (q, qn))
    lp = q - q.max(1, keepdims=True)
    lp -= np.log(np.exp(lp).sum(1, keepdims=True))
    lq = qn - qn.max(1, keepdims=True)
    lq -= np.log(np.exp(lq).sum(1, keepdims=True))
    return (np.exp(lp) * (lp - lq)).sum(1)


def hold(got, want, what):
    """tests/_parity.py rules 2 and 3: the normwise and the floored elementwise bound."""
    nerr, rel_hi, abs_lo, _ = error_figures(got, np.asarray(want, np.float64).reshape(np.shape(got)),
                                            ELEM_FLOOR)
    print("%s normwise %.3g, rel above the floor %.3g, abs below %.3g" % (what, nerr, rel_hi, abs_lo))
    assert nerr <= NORM_RTOL and rel_hi <= RTOL and abs_lo <= ELEM_ATOL, what


def states_of(B, S, seed=11):
    return np.random.default_rng(seed).integers(0, 256, (B, 4, S, S)).astype(np.uint8)


def q_oracle(ref, flat, S, states):
    p = ref.unflatten(np.asarray(flat, np.float64), S, "Q")
    return ref.net_forward(states.astype(np.float64), p)["out"]


def make_net(ddq, ref, S, B, states=None, **kw):
    net = ddq.DeepQNet(batch=B, frame=S, **kw)
    th = seeded_theta(S)
    net.set_flat(0, th)
    net.set_flat(1, th)
    if states is not None:
        z = np.zeros(B, np.float32)
        net.write_minibatch(states, np.eye(4, dtype=np.float32)[np.arange(B) % 4], z, states, z + 1)
    return net, th


def check_adapt(net, ref, S, states, sigma):
    """One adapt at sigma: Qa_out against the oracle on theta~ read back, pn_kl
    against float64 on the two Q blobs, sigma's exact step, select_action on theta~."""
    B = len(states)
    net.set_param_noise(sigma, eps_ref=EPS_REF, adapt_coef=COEF, seed=SEED)
    net.forward_q()
    q = net.blob("Q_out").reshape(B, 4)
    net.param_noise_adapt()
    net.synchronize()
    qa = net.blob("Qa_out").reshape(B, 4)
    hold(qa, q_oracle(ref, net.param_noise_params(), S, states), "S%d B%d s%g Qa_out" % (S, B, sigma))
    got, want = net.blob("pn_kl").reshape(B).astype(np.float64), kl(q, qa)
    if want.mean() > 10 * DELTA:
        hold(got, want, "S%d B%d s%g pn_kl" % (S, B, sigma))
        step = np.float32(sigma) / np.float32(COEF)
    else:
        # far below delta the fp32 sum cancels to O(2^-24 |lp|) per term while KL is
        # O(dQ^2): the rounding of lp and lq, <= 2^-20 (1 + max|ln pi|), is the bound
        lp = q - q.max(1, keepdims=True)
        bound = 2.0 ** -20 * (1 + np.abs(lp).max() + np.log(4))
        print("S%d s%g pn_kl max |err| %.3g (bound %.3g)" % (S, sigma, np.abs(got - want).max(), bound))
        assert np.all(np.abs(got - want) <= bound) and got.mean() < DELTA / 10
        step = np.float32(sigma) * np.float32(COEF)
    assert net.blob("pn_sigma") == step and np.float32(net.param_noise["sigma"]) == step
    assert np.array_equal(net.select_action(states), qa.argmax(1))   # numpy argmax: first max
    return want.mean()
