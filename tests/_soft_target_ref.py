"""The soft target update in NumPy: P' = P + tau (Q - P).

Three fp32 array operations, each rounded on its own and none through float64:
what ``target_blend`` (csrc/kernels.hip) and the CPU twin's
``ddq_soft_sync_target`` compute, so the tests compare bytes.
"""
import numpy as np


def blend(p, q, tau):
    p = np.ascontiguousarray(p, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    t = np.float32(tau)
    d = np.subtract(q, p, dtype=np.float32)
    s = np.multiply(t, d, dtype=np.float32)
    return np.add(p, s, dtype=np.float32)


def targets(p0, qs, tau, period):
    """[P_1 .. P_k]: the target tower after each of the updates that left Q at
    qs[0] .. qs[k - 1], from P_0 = p0.  Update t (1-based) is a sync when
    t % period == 0 (tau = 1: the copy)."""
    out, p = [], np.ascontiguousarray(p0, np.float32)
    for t, q in enumerate(qs, 1):
        if period > 0 and t % period == 0:
            p = blend(p, q, tau) if tau < 1 else np.ascontiguousarray(q, np.float32).copy()
        out.append(p)
    return out
