"""Parameter server with the semantics of param-server/server.py (reference),
its model and optimizer state resident on the GPU.

Endpoints (server.py:181-215) as methods -- ``get_model_params`` (GET
/api/v1/latest_model), ``update_params`` (POST /api/v1/update_model),
``clear_params`` (GET /api/v1/clear_model) -- plus ``serve(port)``, a stdlib
HTTP front end with the same routes and ``application/deepQ`` bodies, so an
unmodified reference worker can talk to it.

Semantics kept:
* the central model holds the ``Q*`` parameters; a pull at
  ``iteration % special_update_period == 0`` first copies Q -> P
  (server.py:127-137, :188-189), after which P* blobs are part of every
  model message (dict order: Q* then P*);
* a push increments ``iteration`` then applies the gradient with the selected
  rule -- sgd (:81-83), rmsprop with the one-step-lagged cache (:86-105,
  default), adagrad (:108-124), or (no reference counterpart) ``adam`` with the
  ``adam=dict(beta1, beta2, eps, max_grad_norm)`` constants -- each on arrival,
  i.e. with the reference's unbounded staleness;
* ``snapshot_frequency`` (:74-77): every that many iterations the model is
  handed to ``on_snapshot(name, params)`` (Celery's ``saveSnapshot`` in the
  reference; a callback here);
* ``stats_frequency`` (:203-204, "Monitoring stats not implemented" in the
  reference): with ``on_stats`` given, every that many iterations one record of
  the device-resident monitor (the RMS of every blob of the model just applied
  and of the gradient just pushed, tagged with the iteration) is handed to
  ``on_stats(iteration, record)``.
Beside the snapshots (theta_Q only), ``checkpoint_path`` / ``checkpoint_freq``
write the server's whole state -- both towers, the optimizer state, the
iteration (``DeepQNet.save_checkpoint``) -- every that many iterations, and
``resume=PATH`` continues from such a file bit for bit.
The apply runs in ``apply_kernel`` on the device (``ddq_set_grads`` +
``ddq_apply``), not in numpy.
"""
from __future__ import annotations

import pickle
import struct
import threading

import numpy as np

from . import params as P
from .barista import messaging
from .net import DeepQNet

MODEL_NAME = "centralModel"     # server.py:13


def get_snapshot_name(iteration):
    return MODEL_NAME + "-%06d" % iteration     # server.py:41-42


class ParamServer:
    def __init__(self, frame=16, batch=32, update="rmsprop", lr=1e-4, rmsprop_decay=0.9,
                 special_update=10, snapshot_freq=500, stats_freq=500, device=0,
                 on_snapshot=None, mode="gpu", on_stats=None, adam=None, target_tau=None,
                 checkpoint_path=None, checkpoint_freq=0, resume=None):
        if update not in ("sgd", "rmsprop", "adagrad", "adam"):
            raise ValueError("update must be one of adagrad, adam, rmsprop, sgd")
        self.net = DeepQNet(batch=batch, frame=frame, device=device, mode=mode)
        # no reference counterpart: Adam (optionally under a global gradient-norm
        # clip), adam = DeepQNet.set_adam's keywords
        if update == "adam":
            self.net.set_adam(**(adam or {}))
        # no reference counterpart: soft target updates.  With target_tau < 1 a
        # special update blends, P <- P + tau (Q - P), once a target exists (the
        # first one still copies, so that P is defined)
        if target_tau is not None:
            self.net.set_target_tau(target_tau)
        self.update = update
        self.learning_rate = float(lr)
        self.rmsprop_decay = float(rmsprop_decay)
        self.special_update_period = int(special_update)
        self.snapshot_frequency = int(snapshot_freq)
        self.stats_frequency = int(stats_freq)
        self.on_snapshot = on_snapshot
        # server.py:203-204 ("Monitoring stats not implemented" there): with a
        # callback, every stats_frequency-th push takes one device monitor
        # record after its apply; without one nothing is enabled
        self.on_stats = on_stats
        if on_stats is not None:
            self.net.monitor_enable(4, 0)
        self.iteration = 0
        self.has_model = False
        self.has_target = False
        self.model_lock = threading.Lock()
        # no reference counterpart (its snapshots keep theta_Q only): every
        # checkpoint_freq iterations the whole server state -- both towers, the
        # optimizer state, the iteration -- goes to checkpoint_path, atomically;
        # resume: continue from such a file, exactly
        self.checkpoint_path = checkpoint_path
        self.checkpoint_frequency = int(checkpoint_freq or 0)
        if resume:
            self.load_checkpoint(resume)

    def save_checkpoint(self, path=None):
        """The server's whole state to ``path`` (default: ``checkpoint_path``).
        The caller holds ``model_lock`` or is the only thread."""
        path = path or self.checkpoint_path
        if not path:
            raise ValueError("no checkpoint path")
        self.net.save_checkpoint(path, meta={
            "iteration": int(self.iteration), "has_model": bool(self.has_model),
            "has_target": bool(self.has_target),
            "step_cfg": {"rule": self.update, "lr": self.learning_rate,
                         "decay": self.rmsprop_decay,
                         "target_period": self.special_update_period}})
        return path

    def load_checkpoint(self, path):
        """Continue from a checkpoint written by a server configured like this
        one (frame, batch, update rule's Adam constants, target_tau)."""
        with self.model_lock:
            meta = self.net.load_checkpoint(path)
            self.iteration = int(meta.get("iteration", 0))
            self.has_model = bool(meta.get("has_model", True))
            self.has_target = bool(meta.get("has_target", False))
        return meta

    # server.py:218-257 initParams(reset=True)
    def init_params(self, params=None, seed=42):
        """Model from ``params`` ({Q*: [W, b]}) or the prototxt fillers."""
        with self.model_lock:
            if params is None:
                params = P.init_params(self.net.frame, seed=seed)
            self.net.set_flat(0, self.net.join(params, "Q"))
            self.net.reset_optimizer()
            self.iteration = 0
            self.has_model = True
            self.has_target = False

    def clear_params(self):
        """GET /api/v1/clear_model (server.py:212-215)."""
        with self.model_lock:
            self.has_model = False
            self.has_target = False
        return b"Cleared"

    def model_params(self):
        out = self.net.split(self.net.get_flat(0), "Q")
        if self.has_target:
            out.update(self.net.split(self.net.get_flat(1), "P"))
        return out

    def get_model_params(self):
        """GET /api/v1/latest_model (server.py:181-193) -> model message bytes."""
        with self.model_lock:
            if not self.has_model:
                return messaging.create_message({}, self.iteration)
            if self.iteration % self.special_update_period == 0:
                if self.has_target:
                    self.net.soft_sync_target()     # (tau = 1: the copy)
                else:
                    self.net.sync_target()
                self.has_target = True
            return messaging.create_message(self.model_params(), self.iteration)

    def update_params(self, message):
        """POST /api/v1/update_model (server.py:196-209) -> b"Updated"."""
        grads = messaging.load_gradient_message(message)
        missing = [k for k in self.net.q_names if k not in grads]
        if missing:
            # server.py:86-124 would touch only the received keys; workers
            # always send every Q blob (messaging.py:43-79), and the device
            # apply updates the whole tower -- a partial message is refused
            # rather than zero-filled (which would still decay the rmsprop
            # cache / consume adagrad's first call of the missing blobs)
            raise ValueError("gradient message lacks %s" % ", ".join(missing))
        with self.model_lock:
            self.iteration += 1
            flat = self.net.join({k: v for k, v in grads.items()}, "Q")
            self.net.set_grads_flat(flat)
            self.net.apply(self.update, lr=self.learning_rate, decay=self.rmsprop_decay)
            if self.snapshot_frequency and self.iteration % self.snapshot_frequency == 0 \
                    and self.on_snapshot is not None:
                self.on_snapshot(get_snapshot_name(self.iteration), self.model_params())
            if self.checkpoint_path and self.checkpoint_frequency and \
                    self.iteration % self.checkpoint_frequency == 0:
                self.save_checkpoint()
            if self.on_stats is not None and self.stats_frequency and \
                    self.iteration % self.stats_frequency == 0:
                self.net.monitor_record(self.iteration)
                _, total = self.net.monitor_read(0, 0)
                recs, _ = self.net.monitor_read(total - 1, 1)
                self.on_stats(self.iteration, recs[0])
        return b"Updated"

    # ---------------------------------------------------------------- HTTP
    def serve(self, port=5500, host="127.0.0.1"):
        """Blocking HTTP server with the reference's routes (server.py:165-215)."""
        from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

        ps = self

        class Handler(BaseHTTPRequestHandler):
            def _reply(self, body, status=200):
                self.send_response(status)
                self.send_header("Content-Type", "application/deepQ")
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                self.wfile.write(body)

            def do_GET(self):
                if self.path == "/api/v1/latest_model":
                    self._reply(ps.get_model_params())
                elif self.path == "/api/v1/clear_model":
                    self._reply(ps.clear_params())
                elif self.path == "/":
                    self._reply(b"Param Server")
                else:
                    self._reply(b"not found", 404)

            def do_POST(self):
                if self.path != "/api/v1/update_model":
                    return self._reply(b"not found", 404)
                n = int(self.headers.get("Content-Length", "0"))
                try:
                    body = ps.update_params(self.rfile.read(n))
                except (ValueError, KeyError, struct.error, pickle.UnpicklingError) as e:
                    return self._reply(("bad gradient message: %s" % e).encode(), 400)
                self._reply(body)

            def log_message(self, *args):
                pass

        httpd = ThreadingHTTPServer((host, port), Handler)
        self._httpd = httpd
        try:
            httpd.serve_forever()
        finally:
            httpd.server_close()

    def shutdown(self):
        if getattr(self, "_httpd", None) is not None:
            self._httpd.shutdown()
