"""BaristaNet: the worker's network wrapper (barista/baristanet.py, reference)
with the same constructor and methods, computing on the MI355X.

``BaristaNet(architecture, model, driver, dataset=None, logpath=None,
reset_log=False, objective=None, n_step=None, priority=None, target_tau=None,
checkpoint=None, checkpoint_every=0, resume=None)``:
* ``architecture`` -- the deepq ``train_val.prototxt`` (its MEMORY_DATA dims and
  the target coefficient are read from the text; the layer graph itself is the
  fixed deepq network implemented in libddq_hip.so) or a dict
  ``{"batch": B, "frame": S, "gamma": g}``;
* ``model`` -- ``.npz`` file of {name: W, name + "/1": b} blobs, or None for the
  prototxt fillers;
* ``driver`` -- "host:port" of the parameter server, or None (dummy pull/push,
  baristanet.py:99-103, :125-133);
* ``objective`` -- None (the reference's max target and Euclidean loss) or a dict
  of ``DeepQNet.set_objective`` arguments, e.g. ``{"target": "double", "loss":
  "huber", "huber_delta": 1.0}``;
* ``n_step`` -- None (the dataset's own n-step length, 1 unless it was made with
  ``ReplayDataset(n_step=)``) or the n of the n-step returns the minibatches are
  gathered for (``DeepQNet.replay_set_nstep``), set on every dataset added;
* ``priority`` -- None (the dataset's own setting, uniform unless it was made with
  ``ReplayDataset(priority=)``) or a dict ``{"alpha":, "beta":, "eps":}`` of
  proportional prioritized replay (``DeepQNet.replay_set_priority``), set on
  every dataset added.  With it ``load_minibatch`` takes the device's
  prioritized draw and ``full_pass`` is followed by the commit of the pass's
  |TD| to the drawn slots;
* ``target_tau`` -- None (hard target syncs) or the tau in (0, 1] of soft target
  updates (``DeepQNet.set_target_tau``), set on the net's context: every target
  sync of a step taken there (``DeviceActor.act_and_train``, an actor pool's
  steps) then blends, P <- P + tau (Q - P).  The construction's own P <- Q stays
  a copy (it defines P);
* ``checkpoint`` / ``checkpoint_every`` -- a file ``maybe_checkpoint()`` rewrites
  (atomically) whenever the iteration is a multiple of ``checkpoint_every``: the
  context's whole training state (``DeepQNet.save_checkpoint``) plus the
  worker's iteration and index-draw state;
* ``resume`` -- a checkpoint to continue from, loaded once the dataset is added
  (``load_checkpoint``); the net then steps exactly as its writer would have.

The input buffers ``state``, ``action``, ``reward``, ``next_state``,
``non_terminal`` have the reference's shapes (baristanet.py:30-34).  They are
bound to the device minibatch (the MEMORY_DATA zero-copy binding,
baristanet.py:41-43): ``load_minibatch`` gathers straight into device memory,
and ``sync_inputs()`` / ``push_inputs()`` move them host <-> device on demand.
"""
from __future__ import annotations

import os
import random
import re
import urllib.request

import numpy as np

from ..net import DeepQNet, GAMMA
from .. import params as P
from . import messaging, netutils


def parse_architecture(architecture):
    """Batch/frame/gamma of a deepq prototxt (train_val.prototxt:2-37, :465-476)."""
    if isinstance(architecture, dict):
        return (int(architecture.get("batch", 32)), int(architecture.get("frame", 16)),
                float(architecture.get("gamma", GAMMA)))
    with open(architecture) as fp:
        txt = fp.read()
    m = re.search(r"memory_data_param\s*:?\s*\{([^}]*)\}", txt)
    if not m:
        raise ValueError("no MEMORY_DATA layer in %s" % architecture)
    body = m.group(1)
    get = lambda key: int(re.search(r"%s\s*:\s*(\d+)" % key, body).group(1))
    batch, channels, h, w = get("batch_size"), get("channels"), get("height"), get("width")
    if channels != 4 or h != w:
        raise ValueError("deepq expects 4 square frames, got %dx%dx%d" % (channels, h, w))
    gamma = GAMMA
    t = re.search(r'name:\s*"target_Q_sa".*?coeff\s*:\s*([0-9.eE+-]+)', txt, re.S)
    if t:
        gamma = float(t.group(1))
    return batch, h, gamma


def step_cfg_dict(cfg):
    """A ``DeepQNet.step_cfg`` (or a dict) as a JSON-able dict."""
    if isinstance(cfg, dict):
        return dict(cfg)
    u = cfg.update
    return {"rule": int(u.rule), "lr": float(u.lr), "decay": float(u.decay), "eps": float(u.eps),
            "momentum": float(u.momentum), "weight_decay": float(u.weight_decay),
            "target_period": int(cfg.target_period), "exchange": int(cfg.exchange),
            "seed": int(cfg.seed), "overlap": int(cfg.overlap), "flags": int(cfg.flags)}


class _Blob:
    """pycaffe-like blob view: ``.data`` / ``.diff`` numpy arrays."""

    def __init__(self, data, diff):
        self.data, self.diff = data, diff


class BaristaNet:
    def __init__(self, architecture, model, driver, dataset=None, logpath=None,
                 reset_log=False, device=0, mode="gpu", objective=None, n_step=None,
                 priority=None, target_tau=None, checkpoint=None, checkpoint_every=0,
                 resume=None):
        batch, frame, gamma = parse_architecture(architecture)
        # mode: main.py:149-151 caffe.set_mode_gpu / set_mode_cpu
        self.mode = mode
        self.dqn = DeepQNet(batch=batch, frame=frame, device=device, gamma=gamma, mode=mode)
        if objective is not None:
            self.dqn.set_objective(**objective)
        if model is not None and os.path.exists(str(model)):
            with np.load(model, allow_pickle=False) as f:
                blobs = {k: f[k] for k in f.files}
            params = {}
            for name in self.dqn.q_names + self.dqn.p_names:
                if name in blobs:
                    params[name] = [blobs[name], blobs[name + "/1"]]
            self.dqn.set_params(params)
        else:
            self.dqn.set_flat(0, P.init_params_flat(frame))
        self.dqn.sync_target()
        self.target_tau = None if target_tau is None else float(target_tau)
        if self.target_tau is not None:
            self.dqn.set_target_tau(self.target_tau)
        self.dataset = None
        self.n_step = None if n_step is None else int(n_step)
        self.priority = priority
        self.per_seed = random.getrandbits(63)   # the prioritized draws' index stream
        self.driver = driver
        # logpath: the reference's per-step loss / norm files (baristanet.py:45-46,
        # netutils.NetLogger), from records of the device-resident monitor; None
        # (what main.py passes unless --logpath is given): log() does nothing
        self.logger = netutils.NetLogger(self, logpath, reset_log) if logpath else None
        B, S = batch, frame
        self.state = np.zeros((B, 4, S, S), np.float32)
        self.action = np.zeros((B, 4, 1, 1), np.float32)
        self.reward = np.zeros((B, 1, 1, 1), np.float32)
        self.next_state = np.zeros((B, 4, S, S), np.float32)
        self.non_terminal = np.zeros((B, 1, 1, 1), np.float32)
        self.batch_size = B
        self.iteration = 0
        self.checkpoint = checkpoint
        self.checkpoint_every = int(checkpoint_every or 0)
        self._resume = resume
        if dataset is not None:
            self.add_dataset(dataset)

    # ----------------------------------------------------------- net-like API
    @property
    def params(self):
        """OrderedDict name -> [blob(.data, .diff)] (pycaffe ``net.params``)."""
        data = self.dqn.split(self.dqn.get_flat(0), "Q")
        diff = self.dqn.split(self.dqn.get_grads_flat(), "Q")
        out = {k: [_Blob(d, g) for d, g in zip(data[k], diff[k])] for k in data}
        pdata = self.dqn.split(self.dqn.get_flat(1), "P")
        out.update({k: [_Blob(d, np.zeros_like(d)) for d in v] for k, v in pdata.items()})
        return out

    @property
    def blobs(self):
        class _B:
            def __init__(s, a):
                s.data = a
        return {name: _B(self.dqn.blob(name)) for name in
                ("Q_out", "P_out", "Q_sa", "P_sa", "target_Q_sa", "loss")}

    def add_dataset(self, dset):
        dset.attach(self.dqn)
        if self.n_step is not None:
            dset.set_n_step(self.n_step)
        if self.priority is not None:
            dset.set_priority(self.priority)
        self.dataset = dset
        if self._resume and not self._resume_deferred:
            self.load_checkpoint(self._resume)

    # ----------------------------------------------------------- checkpoints
    # ``resume=PATH`` loads at the first add_dataset: the ring must exist and be
    # configured as the writer's was.  A worker that also creates a device actor
    # or pool on the context (after the dataset: they need the ring) defers the
    # load with ``defer_resume()`` and calls ``load_checkpoint`` itself once the
    # actor exists, as barista/main.py does.
    _resume_deferred = False

    def defer_resume(self):
        self._resume_deferred = True

    def save_checkpoint(self, path=None, step_cfg=None):
        """The context's whole training state (``DeepQNet.save_checkpoint``) with
        the worker's own: the iteration, the prioritized draws' seed, Python's
        ``random`` state (the reference's host index draws) and, when given, the
        step cfg as a dict."""
        path = path or self.checkpoint
        if not path:
            raise ValueError("no checkpoint path")
        st = random.getstate()
        meta = {"iteration": int(self.iteration), "per_seed": int(self.per_seed),
                "py_random": [st[0], list(st[1]), st[2]]}
        if step_cfg is not None:
            meta["step_cfg"] = step_cfg_dict(step_cfg)
        self.dqn.save_checkpoint(path, meta)
        return path

    def load_checkpoint(self, path):
        """Restore the context from ``path`` and the worker's own state from its
        meta; returns the meta."""
        meta = self.dqn.load_checkpoint(path)
        self.iteration = int(meta.get("iteration", self.iteration))
        self.per_seed = int(meta.get("per_seed", self.per_seed))
        if "py_random" in meta:
            v, words, gauss = meta["py_random"]
            random.setstate((v, tuple(words), gauss))
        self._resume = None
        return meta

    def maybe_checkpoint(self, step_cfg=None):
        """Write ``checkpoint`` when the iteration is a multiple of
        ``checkpoint_every`` (the worker calls this once per step); True if it did."""
        if not self.checkpoint or self.checkpoint_every <= 0 or \
                self.iteration % self.checkpoint_every:
            return False
        self.save_checkpoint(step_cfg=step_cfg)
        return True

    # --------------------------------------------------------------- inputs
    def push_inputs(self):
        """Host input arrays -> device minibatch."""
        self.dqn.write_minibatch(self.state, self.action.reshape(self.batch_size, 4),
                                 self.reward, self.next_state, self.non_terminal)

    def sync_inputs(self):
        """Device minibatch -> host input arrays."""
        st, ac, rw, ns, nt = self.dqn.read_minibatch()
        self.state[...], self.action[...], self.reward[...] = st, ac, rw
        self.next_state[...], self.non_terminal[...] = ns, nt

    def load_minibatch(self):
        """baristanet.py:55-68: sample from the replay into the net inputs."""
        if self.dataset and self.dataset.priority is not None:
            # the device's prioritized draw (and its importance-sampling weights)
            self.dqn.replay_sample_device(self.per_seed)
        elif self.dataset:
            idx = self.dataset.draw_indices(self.batch_size)
            self.dqn.replay_sample(np.asarray(idx, np.int32))
        else:
            print("Warning: no dataset specified, using dummy data.")
            self.dummy_load_minibatch()

    def dummy_load_minibatch(self):
        """baristanet.py:70-83: uniform frames, one-hot actions, rewards in [-5,5]."""
        B = self.batch_size
        self.state[...] = np.random.randint(0, 256, size=self.state.shape)
        self.action[...] = 0
        self.action[np.arange(B), np.random.randint(0, 4, size=(B,))] = 1
        self.reward[...] = np.random.randint(-5, 6, size=self.reward.shape)
        self.next_state[...] = np.random.randint(0, 256, size=self.next_state.shape)
        self.non_terminal[...] = np.random.choice([True, False], size=self.non_terminal.shape)
        self.push_inputs()

    # --------------------------------------------------------- param server
    def fetch_model(self):
        """baristanet.py:85-97: GET latest_model, load it, return the iteration."""
        if self.driver is None:
            return self.dummy_fetch_model()
        req = urllib.request.Request("http://%s/api/v1/latest_model" % self.driver,
                                     headers={"Content-Type": "application/deepQ"})
        message = urllib.request.urlopen(req).read()
        self.iteration = messaging.load_model_message(message, self.dqn)
        return self.iteration

    def dummy_fetch_model(self):
        """baristanet.py:99-103 with the 'ii' header the loader expects (the
        reference's dummy path builds an 'i' message, messaging.py:72 vs :91)."""
        message = messaging.create_message(self.dqn.split(self.dqn.get_flat(0), "Q"),
                                           self.iteration)
        return messaging.load_model_message(message, self.dqn)

    def send_gradient_update(self):
        """baristanet.py:105-123: POST the Q gradients; returns the reply body."""
        if self.driver is None:
            return self.dummy_send_gradient_update()
        message = messaging.create_gradient_message(self.dqn)
        req = urllib.request.Request("http://%s/api/v1/update_model" % self.driver,
                                     headers={"Content-Type": "application/deepQ"},
                                     data=message)
        return urllib.request.urlopen(req).read()

    def dummy_send_gradient_update(self):
        messaging.create_gradient_message(self.dqn)
        return b"OK" if np.random.rand() < 0.98 else b"ERROR"

    # -------------------------------------------------------------- compute
    def forward(self, end=None):
        if end == "Q_out":
            self.dqn.forward_q()
        else:
            self.dqn.forward_backward()

    def full_pass(self):
        """baristanet.py:138-140: forward + backward on the bound minibatch; on
        a prioritized dataset the pass's |TD| then becomes the drawn slots'
        priorities."""
        loss = self.dqn.forward_backward()
        if self.dataset and self.dataset.priority is not None:
            self.dqn.replay_update_priorities()
        return loss

    def select_action(self, state, batch_size=1):
        """baristanet.py:142-146: argmax_a Q(s, a) (first max).  ``state`` is
        one (4,S,S) stack or a batch; only the n given states are evaluated."""
        s = np.asarray(state)
        n = 1 if s.ndim == 3 else s.shape[0]
        a = self.dqn.select_action(s.reshape(n, 4, self.dqn.frame, self.dqn.frame))
        return int(a[0]) if (batch_size == 1 and n == 1) else a[:max(batch_size, n)]

    def log(self):
        """baristanet.py:148-149: append this step's loss and the RMS of every
        blob's gradient and parameters to the log files (one device monitor
        record); nothing without a logpath.  Returns the record or None."""
        if self.logger is None:
            return None
        return self.logger.write()
