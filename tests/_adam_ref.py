"""Float64 restatement of DDQ_RULE_ADAM (include/ddq_hip.h): Adam without
amsgrad or weight decay, eps outside the square root, under an optional
global-norm gradient clip.  The constants are taken as given: a caller that
compares with the fp32 library passes the values fp32 holds (``f32``)."""
import numpy as np

DEFAULTS = dict(beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=0.0)


def f32(x):
    """The double an fp32 field holds for x."""
    return float(np.float32(x))


def constants(**kw):
    """DEFAULTS overridden by kw, each as fp32 holds it."""
    d = dict(DEFAULTS)
    d.update(kw)
    return {k: f32(v) for k, v in d.items()}


def clip_scale(g, max_grad_norm):
    """(norm, s): the gradient's L2 norm and the factor the rule scales it by."""
    g = np.asarray(g, np.float64)
    nrm = float(np.sqrt(np.sum(g * g)))
    if max_grad_norm > 0 and nrm > max_grad_norm:
        return nrm, max_grad_norm / nrm
    return nrm, 1.0


def step(theta, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=0.0):
    """Update number t (1 for the first after a reset, where m = v = 0 go in).
    Returns (theta, m, v, norm): norm is the pre-clip gradient norm, None with
    clipping off."""
    theta = np.asarray(theta, np.float64)
    g = np.asarray(g, np.float64)
    m = np.zeros_like(theta) if m is None else np.asarray(m, np.float64)
    v = np.zeros_like(theta) if v is None else np.asarray(v, np.float64)
    nrm = None
    if max_grad_norm > 0:
        nrm, s = clip_scale(g, max_grad_norm)
        g = s * g
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * (g * g)
    c1 = 1.0 - beta1 ** t
    c2 = 1.0 - beta2 ** t
    theta = theta - (lr * (m / c1)) / (np.sqrt(v / c2) + eps)
    return theta, m, v, nrm
