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
        [--munchausen-alpha A] [--munchausen-tau T] [--munchausen-clip L]
        [--acting-path batch|spread|auto]
        [--param-noise-sigma S] [--param-noise-eps E] [--param-noise-resample K]

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

``--munchausen-alpha A`` or ``--munchausen-tau T`` (off by default; either turns it
on) select the Munchausen-DQN target (``DeepQNet.set_munchausen``): the soft value
T logsumexp(P(s',.) / T) in the max's place and A clip(T ln pi(a | s), L, 0) added to
the reward, L = ``--munchausen-clip`` (default -1).  Defaults A 0.9, T 0.03;
``--munchausen-alpha 0 --munchausen-tau T`` is Soft-DQN.  Not with ``--double-q``.
Either mode.

``--param-noise-sigma S`` (off by default) turns on parameter-space noise
(``DeepQNet.set_param_noise``): every act runs on theta_Q + sigma eps, sigma starting
at S and adapted towards the KL distance of epsilon-greedy at ``--param-noise-eps``
(default 0.05); ``--param-noise-resample K`` (default 64) redraws the noise every K
moves.  Epsilon-greedy stays on top of it.  Either mode.

``--acting-path`` (default ``batch``) selects the kernels of every acting
forward of the net's context (``DeepQNet.set_acting_path``): ``spread`` runs a
worker's one-state acts (the host ``ExpGain`` and ``--device-actor`` alike) on
kernels that spread one image over the chip.  Stored without effect in cpu mode.

``--target-tau T`` (default: hard target syncs) sets soft target updates on the
net's context (``DeepQNet.set_target_tau``), T in (0, 1]: the training steps taken
there (``--device-actor``'s ``act_and_train``, an actor pool) blend P towards Q at
every target sync, P <- P + T (Q - P).  Either mode.

``--n-step N`` (default 1) gathers the minibatches for N-step returns
(``DeepQNet.replay_set_nstep``): the discounted sum of up to N rewards and
gamma^N P(s_{t+N}, .), cut at the first terminal step.  Either mode.

``--augment-pad P`` (default 0, off) shifts every device-drawn frame by a random
offset in [-P, P]^2 over a replicate-padded copy (``DeepQNet.replay_set_augment``);
it acts where the minibatch is drawn on the device (prioritized replay, the step
modes), not on ``sample_direct``'s host-index gather.  Either mode.

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
    ap.add_argument("--munchausen-alpha", dest="munchausen_alpha", type=float, default=None,
                    help="Munchausen-DQN target with this bonus scale in [0, 1] (0: Soft-DQN)")
    ap.add_argument("--munchausen-tau", dest="munchausen_tau", type=float, default=None,
                    help="Munchausen-DQN target with this temperature, > 0 (default 0.03)")
    ap.add_argument("--munchausen-clip", dest="munchausen_clip", type=float, default=None,
                    help="Munchausen-DQN: lower clip of the scaled log-policy, < 0 (default -1)")
    ap.add_argument("--param-noise-sigma", dest="param_noise_sigma", type=float, default=None,
                    help="parameter-space noise with this initial sigma, >= 0 (default: off)")
    ap.add_argument("--param-noise-eps", dest="param_noise_eps", type=float, default=None,
                    help="parameter-space noise: the epsilon whose KL distance sigma is adapted "
                         "to, in (0, 1) (default 0.05)")
    ap.add_argument("--param-noise-resample", dest="param_noise_resample", type=int, default=None,
                    help="parameter-space noise: moves between resamples, >= 0 (default 64)")
    ap.add_argument("--target-tau", dest="target_tau", type=float, default=None,
                    help="soft target updates: P <- P + T (Q - P) at every target sync, T in (0, 1]")
    ap.add_argument("--acting-path", dest="acting_path", default=None,
                    choices=("batch", "spread", "auto"),
                    help="kernels of the acting forward (default batch)")
    ap.add_argument("--n-step", dest="n_step", type=int, default=1,
                    help="N-step returns: the replay gathers N-step windows (default 1)")
    ap.add_argument("--augment-pad", dest="augment_pad", type=int, default=0,
                    help="random-shift augmentation of device-drawn minibatches, pad in [0, 8] "
                         "(default 0: off)")
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
    if not 0 <= args.augment_pad <= 8:
        ap.error("--augment-pad must be in [0, 8]")
    if args.n_step >= args.dset_size:
        ap.error("--n-step must be below --dset-size (%d)" % args.dset_size)
    if args.target_tau is not None and not 0.0 < args.target_tau <= 1.0:
        ap.error("--target-tau must be in (0, 1]")
    if args.huber_delta is not None and not args.huber_delta > 0:
        ap.error("--huber-delta must be > 0")
    if args.munchausen_alpha is not None and not 0.0 <= args.munchausen_alpha <= 1.0:
        ap.error("--munchausen-alpha must be in [0, 1]")
    if args.munchausen_tau is not None and not args.munchausen_tau > 0:
        ap.error("--munchausen-tau must be > 0")
    if args.munchausen_clip is not None:
        if args.munchausen_alpha is None and args.munchausen_tau is None:
            ap.error("--munchausen-clip needs --munchausen-alpha or --munchausen-tau")
        if not args.munchausen_clip < 0:
            ap.error("--munchausen-clip must be < 0")
    if args.param_noise_sigma is None and (args.param_noise_eps is not None or
                                           args.param_noise_resample is not None):
        ap.error("--param-noise-eps / --param-noise-resample need --param-noise-sigma")
    if args.param_noise_sigma is not None and not args.param_noise_sigma >= 0:
        ap.error("--param-noise-sigma must be >= 0")
    if args.param_noise_eps is not None and not 0.0 < args.param_noise_eps < 1.0:
        ap.error("--param-noise-eps must be in (0, 1)")
    if args.param_noise_resample is not None and args.param_noise_resample < 0:
        ap.error("--param-noise-resample must be >= 0")
    if args.double_q and munchausen_of(args) is not None:
        ap.error("--double-q and the Munchausen target exclude each other")
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


def munchausen_of(args):
    """BaristaNet's ``munchausen`` for --munchausen-alpha / -tau / -clip (None: off)."""
    alpha, tau = getattr(args, "munchausen_alpha", None), getattr(args, "munchausen_tau", None)
    if alpha is None and tau is None:
        return None
    clip = getattr(args, "munchausen_clip", None)
    return {"alpha": 0.9 if alpha is None else alpha, "tau": 0.03 if tau is None else tau,
            "clip": -1.0 if clip is None else clip}


def param_noise_of(args):
    """BaristaNet's ``param_noise`` for --param-noise-sigma / -eps / -resample (None: off)."""
    sigma = getattr(args, "param_noise_sigma", None)
    if sigma is None:
        return None
    eps, k = getattr(args, "param_noise_eps", None), getattr(args, "param_noise_resample", None)
    return {"sigma": sigma, "eps_ref": 0.05 if eps is None else eps,
            "resample_every": 64 if k is None else k}


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
                     checkpoint_every=getattr(args, "checkpoint_every", 0),
                     acting_path=getattr(args, "acting_path", None),
                     munchausen=munchausen_of(args), param_noise=param_noise_of(args))
    # --resume: loaded below, once everything the checkpoint holds exists on the
    # context (the ring, and the device actor when there is one); the initial
    # replay fill is the checkpoint's then
    resume = getattr(args, "resume", None)
    replay = ReplayDataset(args.dataset, net.state[0].shape, dset_size=args.dset_size,
                           overwrite=args.overwrite, batch_size=net.batch_size, mode=args.mode,
                           n_step=getattr(args, "n_step", 1), priority=priority_of(args),
                           augment_pad=getattr(args, "augment_pad", 0))
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
