"""Barista worker server (main.py, reference): a TCP loop on 127.0.0.1:port
where one request byte 'G' triggers one training step (main.py:37-112):
fetch the model from the param server, generate one experience (ε-greedy
acting through the GPU Q tower), sample a minibatch from the HBM replay, run
the forward/backward pass on the GPU, push the Q gradients, reply.

    python -m ddq.barista.main <train_val.prototxt> <model.npz|none>
        [--port 50001] [--driver 127.0.0.1:5500|None] [--dataset replay-dataset.hdf5]
        [--dset-size 1000] [--overwrite] [--debug] [--initial-replay 20000]
        [--device-actor [--actor-seed N]] [--logpath PREFIX]
        [--double-q] [--huber-delta D] [--target-tau T]

``--mode gpu`` (default) runs libddq_hip.so; ``--mode cpu`` runs the same
step on the host through the CPU twin libddq_cpu.so (main.py:128,149-151, the
reference's Caffe CPU mode: BASELINE configs[0]).

``--device-actor`` (off by default) replaces the host ``ExpGain`` by
``ddq.actor.DeviceActor``: the game, the preprocessing, the ε-greedy choice and
the replay add run inside the net's context (ddq_actor_step_async), so
``generate_experience`` only enqueues.

``--double-q`` and ``--huber-delta D`` (both off by default) select the TD
objective the gradients are computed for (``DeepQNet.set_objective``): the
Double-DQN target r + gamma P(s', argmax_a Q(s',a)) in place of the max, and the
Huber loss with band D in place of the Euclidean one.  Both work in either mode.

``--target-tau T`` (default: hard target syncs) sets soft target updates on the
net's context (``DeepQNet.set_target_tau``), T in (0, 1]: the training steps taken
there (``--device-actor``'s ``act_and_train``, an actor pool) blend P towards Q at
every target sync, P <- P + T (Q - P).  Either mode.

``--n-step N`` (default 1) gathers the minibatches for N-step returns
(``DeepQNet.replay_set_nstep``): the discounted sum of up to N rewards and
gamma^N P(s_{t+N}, .), cut at the first terminal step.  Either mode.

``--per-alpha A`` (off by default) turns on proportional prioritized replay
(``DeepQNet.replay_set_priority``) with exponent A in [0, 1]; ``--per-beta``
(default 0.4, in [0, 1]) is the importance-sampling exponent and ``--per-eps``
(default 0.01, > 0) the priority floor.  ``load_minibatch`` then takes the
device's prioritized draw and every ``full_pass`` commits its |TD|.  Either mode.

``--logpath PREFIX`` (off by default) makes ``net.log()`` append the step's loss
and every blob's gradient / parameter RMS to files under ``PREFIX-<date>``
(netutils.NetLogger), from one record of the device-resident monitor.
"""
from __future__ import annotations

import argparse
import os
import random
import socket
import time

from .. import expgain as eg
from .._lib import NSTEP_MAX
from ..replay import ReplayDataset
from ..snake import SnakeGame, gray_scale
from . import GRAD_UPDATE, DARWIN_UPDATE, MSG_LENGTH, netutils
from .baristanet import BaristaNet


def recv_all(sock, size):
    message = b""
    while len(message) < size:
        chunk = sock.recv(4096)
        if not chunk:
            break
        message += chunk
    return message


def process_connection(sock, net, exp_gain, debug=False):
    """main.py:37-58 / :61-112 (the non-debug handler's NameError at :46 is
    not reproduced; both modes run the same step)."""
    message = recv_all(sock, MSG_LENGTH)
    if message == GRAD_UPDATE:
        iteration_num = net.fetch_model()
        exp_gain.generate_experience(iteration_num)
        net.load_minibatch()
        tic = time.time()
        net.full_pass()
        toc = time.time()
        if debug:
            print("    * step took % 0.2f milliseconds." % (1000 * (toc - tic)))
            print("Loss:", netutils.extract_net_data(net, ("loss",))["loss"])
        response = net.send_gradient_update()
        net.log()
        net.maybe_checkpoint()
        sock.sendall(response if isinstance(response, bytes) else str(response).encode())
    elif message == DARWIN_UPDATE:
        raise NotImplementedError("Darwinian SGD not implemented")
    else:
        print("Unknown request:", message)
    sock.close()


def issue_ready_signal(idx):
    """main.py:115-120: flags/__BARISTA_READY__.<port>."""
    os.makedirs("flags", exist_ok=True)
    open("flags/__BARISTA_READY__.%d" % idx, "w").close()


def get_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("architecture")
    ap.add_argument("model")
    ap.add_argument("--solver", default=None)
    ap.add_argument("--mode", default="gpu", choices=["gpu", "cpu"])
    ap.add_argument("--port", type=int, default=50001)
    ap.add_argument("--driver", default="127.0.0.1:5500")
    ap.add_argument("--dataset", default="replay-dataset.hdf5")   # main.py:131
    ap.add_argument("--dset-size", dest="dset_size", type=int, default=1000)
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--debug", action="store_true")
    ap.add_argument("--initial-replay", type=int, default=20000)
    ap.add_argument("--max-requests", type=int, default=0, help="exit after N requests (tests)")
    ap.add_argument("--device-actor", dest="device_actor", action="store_true",
                    help="act on the device (ddq.actor.DeviceActor) instead of the host ExpGain")
    ap.add_argument("--actor-seed", dest="actor_seed", type=int, default=None,
                    help="seed of the device actor's random stream (default: random)")
    ap.add_argument("--logpath", default=None,
                    help="prefix of the per-step loss / norm log directory (default: no log)")
    ap.add_argument("--double-q", dest="double_q", action="store_true",
                    help="Double-DQN target: P at argmax_a Q(s',a) instead of max_a P")
    ap.add_argument("--huber-delta", dest="huber_delta", type=float, default=None,
                    help="Huber loss with this band instead of the Euclidean loss")
    ap.add_argument("--target-tau", dest="target_tau", type=float, default=None,
                    help="soft target updates: P <- P + T (Q - P) at every target sync, T in (0, 1]")
    ap.add_argument("--n-step", dest="n_step", type=int, default=1,
                    help="N-step returns: the replay gathers N-step windows (default 1)")
    ap.add_argument("--per-alpha", dest="per_alpha", type=float, default=None,
                    help="prioritized replay with this priority exponent in [0, 1] (default: off)")
    ap.add_argument("--per-beta", dest="per_beta", type=float, default=None,
                    help="prioritized replay: importance-sampling exponent in [0, 1] (default 0.4)")
    ap.add_argument("--per-eps", dest="per_eps", type=float, default=None,
                    help="prioritized replay: priority floor, > 0 (default 0.01)")
    ap.add_argument("--checkpoint", default=None,
                    help="file the whole training state is written to (atomically) every "
                         "--checkpoint-every steps")
    ap.add_argument("--checkpoint-every", dest="checkpoint_every", type=int, default=0,
                    help="steps between checkpoints (default 0: none)")
    ap.add_argument("--resume", default=None,
                    help="checkpoint to continue from; the worker must be started with the "
                         "options of the run that wrote it")
    args = ap.parse_args(argv)
    if args.checkpoint_every < 0:
        ap.error("--checkpoint-every must be >= 0")
    if args.checkpoint_every and not args.checkpoint:
        ap.error("--checkpoint-every needs --checkpoint")
    if args.per_alpha is None and (args.per_beta is not None or args.per_eps is not None):
        ap.error("--per-beta / --per-eps need --per-alpha")
    if args.per_alpha is not None and not 0.0 <= args.per_alpha <= 1.0:
        ap.error("--per-alpha must be in [0, 1]")
    if args.per_beta is not None and not 0.0 <= args.per_beta <= 1.0:
        ap.error("--per-beta must be in [0, 1]")
    if args.per_eps is not None and not args.per_eps > 0:
        ap.error("--per-eps must be > 0")
    if not 1 <= args.n_step <= NSTEP_MAX:
        ap.error("--n-step must be in [1, %d]" % NSTEP_MAX)
    if args.n_step >= args.dset_size:
        ap.error("--n-step must be below --dset-size (%d)" % args.dset_size)
    if args.target_tau is not None and not 0.0 < args.target_tau <= 1.0:
        ap.error("--target-tau must be in (0, 1]")
    if args.huber_delta is not None and not args.huber_delta > 0:
        ap.error("--huber-delta must be > 0")
    if args.driver == "None":
        args.driver = None
    return args


def objective_of(args):
    """BaristaNet's ``objective`` for --double-q / --huber-delta (None: neither)."""
    double, delta = getattr(args, "double_q", False), getattr(args, "huber_delta", None)
    if not double and delta is None:
        return None
    obj = {"target": "double" if double else "max",
           "loss": "euclidean" if delta is None else "huber"}
    if delta is not None:
        obj["huber_delta"] = delta
    return obj


def priority_of(args):
    """ReplayDataset's ``priority`` for --per-alpha / --per-beta / --per-eps (None: off)."""
    alpha = getattr(args, "per_alpha", None)
    if alpha is None:
        return None
    beta, eps = getattr(args, "per_beta", None), getattr(args, "per_eps", None)
    return {"alpha": alpha, "beta": 0.4 if beta is None else beta,
            "eps": 0.01 if eps is None else eps}


def build_worker(args):
    model = None if args.model in ("none", "None") else args.model
    net = BaristaNet(args.architecture, model, args.driver,
                     logpath=getattr(args, "logpath", None), mode=args.mode,
                     objective=objective_of(args), target_tau=getattr(args, "target_tau", None),
                     checkpoint=getattr(args, "checkpoint", None),
                     checkpoint_every=getattr(args, "checkpoint_every", 0))
    # --resume: loaded below, once everything the checkpoint holds exists on the
    # context (the ring, and the device actor when there is one); the initial
    # replay fill is the checkpoint's then
    resume = getattr(args, "resume", None)
    replay = ReplayDataset(args.dataset, net.state[0].shape, dset_size=args.dset_size,
                           overwrite=args.overwrite, batch_size=net.batch_size, mode=args.mode,
                           n_step=getattr(args, "n_step", 1), priority=priority_of(args))
    net.add_dataset(replay)
    game = SnakeGame()
    pre = eg.generate_preprocessor(net.state.shape[2:], gray_scale)
    if getattr(args, "device_actor", False):
        from ..actor import DeviceActor
        seed = args.actor_seed if args.actor_seed is not None else random.getrandbits(64)
        exp_gain = DeviceActor(net, game.encode_state(), seed, preprocessor=pre)
        if resume:                                      # the actor's game and stream too
            net.load_checkpoint(resume)
        elif args.overwrite:                            # main.py:176-178
            exp_gain.fill(min(args.initial_replay, args.dset_size))
        return net, replay, exp_gain
    exp_gain = eg.ExpGain(net, ["w", "a", "s", "d"], pre, game.cpu_play, replay,
                          game.encode_state())
    if resume:       # (the host ExpGain's game is not device state: it starts a new game)
        net.load_checkpoint(resume)
    elif args.overwrite:                                # main.py:176-178
        for _ in range(min(args.initial_replay, args.dset_size)):
            exp_gain.generate_experience(0)
    return net, replay, exp_gain


def main(argv=None):
    args = get_args(argv)
    net, replay, exp_gain = build_worker(args)
    server = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    server.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    server.bind(("127.0.0.1", args.port))
    server.listen(5)
    print("* Starting BARISTA server: listening on port %d." % args.port, flush=True)
    issue_ready_signal(args.port)
    served = 0
    try:
        while args.max_requests == 0 or served < args.max_requests:
            client, _ = server.accept()
            process_connection(client, net, exp_gain, args.debug)
            served += 1
    finally:
        server.close()
        replay.close()


if __name__ == "__main__":
    main()
