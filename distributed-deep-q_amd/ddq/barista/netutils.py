"""barista/netutils.py (reference): the helpers the worker loop and the
evaluator use, the norm monitoring (netutils.py:7-36) and NetLogger
(netutils.py:72-96).

The reference computes the norms on the host from pycaffe's ``.data`` /
``.diff`` arrays after every step.  Here the default (``ord=None``, the RMS
``np.linalg.norm(ravel(x)) / sqrt(x.size)``) comes from one record of the
device-resident monitor (``DeepQNet.monitor_record``): one reduction launch on
the device, 160 bytes to the host, no copy of the parameters.  Any other
``ord`` is computed on the host from ``net.params`` as the reference does."""
from __future__ import annotations

import os
from datetime import datetime

import numpy as np

_MONITOR_RING = 16      # records of the ring the helpers enable on demand


def extract_net_data(net, blobs):
    """netutils.py:48-53: squeezed copies of the named blobs."""
    b = net.blobs
    return {name: np.squeeze(b[name].data) for name in blobs}


def set_net_params(net, params):
    """netutils.py:61-64: assign {name: [W, b]} into the network."""
    dq = getattr(net, "dqn", net)
    dq.set_params(params)


def _names(dq):
    return list(dq.q_names) + list(dq.p_names)


def take_record(net):
    """One explicit monitor record of ``net`` (a BaristaNet or a DeepQNet) as
    it is now.  Enables a small explicit-record ring when the monitor is off
    (that invalidates captured step graphs once)."""
    dq = getattr(net, "dqn", net)
    if not getattr(dq, "_monitor_cap", 0):
        dq.monitor_enable(_MONITOR_RING, 0)
    dq.monitor_record(0)
    _, total = dq.monitor_read(0, 0)
    recs, _ = dq.monitor_read(total - 1, 1)
    return recs[0]


def gradient_norms_of(net, rec):
    """{name: [w, b]} gradient RMS of a monitor record; the P tower's are 0
    (Caffe's P layers have no diff)."""
    dq = getattr(net, "dqn", net)
    out = {}
    for l, name in enumerate(dq.q_names):
        out[name] = [float(rec["grad_rms"][2 * l]), float(rec["grad_rms"][2 * l + 1])]
    for name in dq.p_names:
        out[name] = [0.0, 0.0]
    return out


def param_norms_of(net, rec):
    """{name: [w, b]} parameter RMS of a monitor record, Q and P towers."""
    dq = getattr(net, "dqn", net)
    out = {}
    for z, names in enumerate((dq.q_names, dq.p_names)):
        for l, name in enumerate(names):
            out[name] = [float(rec["param_rms"][z][2 * l]), float(rec["param_rms"][z][2 * l + 1])]
    return out


def _host_arrays(net, field):
    """{name: [w, b]} host arrays of every Q* / P* blob: ``.data`` or ``.diff``."""
    if hasattr(net, "params"):
        return {k: [getattr(b, field) for b in v] for k, v in net.params.items()}
    dq = getattr(net, "dqn", net)
    if field == "data":
        return dq.get_params()
    out = dq.split(dq.get_grads_flat(), "Q")
    out.update({k: [np.zeros_like(a) for a in v] for k, v in dq.split(dq.get_flat(1), "P").items()})
    return out


def _host_norms(net, field, params, ord):
    arrays = _host_arrays(net, field)
    norms = {}
    for name in params:
        norms[name] = []
        for a in arrays[name]:
            norm = float(np.linalg.norm(np.ravel(a).astype(np.float64), ord=ord))
            if ord != 0:
                norm /= np.sqrt(a.size)
            norms[name].append(norm)
    return norms


def compute_gradient_norms(net, params=None, ord=None):
    """netutils.py:7-20.  ord=None: from a device monitor record."""
    dq = getattr(net, "dqn", net)
    if not params:
        params = _names(dq)
    if ord is None:
        norms = gradient_norms_of(net, take_record(net))
        return {name: norms[name] for name in params}
    return _host_norms(net, "diff", params, ord)


def compute_param_norms(net, params=None, ord=None):
    """netutils.py:23-36.  ord=None: from a device monitor record."""
    dq = getattr(net, "dqn", net)
    if not params:
        params = _names(dq)
    if ord is None:
        norms = param_norms_of(net, take_record(net))
        return {name: norms[name] for name in params}
    return _host_norms(net, "data", params, ord)


def pretty_print(param_dict):
    """netutils.py:67-69."""
    for param in sorted(param_dict.keys()):
        print(param.ljust(19), param_dict[param])


def _fmt(x):
    return "%.9g" % float(x)     # nine digits: an fp32 value reads back exactly


class NetLogger:
    """netutils.py:72-96: per-step ``loss``, ``<name>.gradnorm`` and
    ``<name>.norm`` files under ``path + "-" + str(datetime.now())``, one line
    per step, each norm line ``"w,b"``, for the ten Q* and P* layer names."""

    def __init__(self, net, path, reset=False):
        self.path = path + "-" + str(datetime.now())
        if not os.path.isdir(self.path):
            os.makedirs(self.path)
        self.net = net

    def _append(self, rec):
        with open(os.path.join(self.path, "loss"), "a") as fp:
            print(_fmt(rec["loss"]), file=fp)
        grad_norms = gradient_norms_of(self.net, rec)
        for name in grad_norms:
            with open(os.path.join(self.path, name + ".gradnorm"), "a") as fp:
                print(",".join(_fmt(x) for x in grad_norms[name]), file=fp)
        param_norms = param_norms_of(self.net, rec)
        for name in param_norms:
            with open(os.path.join(self.path, name + ".norm"), "a") as fp:
                print(",".join(_fmt(x) for x in param_norms[name]), file=fp)

    def write(self):
        """One explicit record of the net as it is now, read and appended."""
        rec = take_record(self.net)
        self._append(rec)
        return rec

    def flush(self, records):
        """Append the same lines from records the steps took themselves
        (``monitor_enable(capacity, period)`` then ``monitor_read``): a graph
        chain is logged after the fact."""
        for rec in records:
            self._append(rec)
