"""Snapshots and policy evaluation -- host drivers over the
GPU network.

* ``save_snapshot(snapshot_name, model)``: tasks.py:25-34 (``saveSnapshot``):
  pickles ``dict(model)`` ({name: [W, b]}) to ``snapshot_name + str(now)``.
  The reference also mirrors it into a Redis dict; here the files are the
  store.  ``ParamServer(on_snapshot=save_snapshot)`` reproduces the
  server's every-``snapshot_freq``-iterations hook (server.py:74-77).
* ``load_snapshot(path)``: reads such a file with an unpickler that only
  admits numpy arrays and builtin containers (no code runs from the file).
* ``PolicyEvaluator(architecture_file, model_file).evaluate(model,
  num_trials)``: evaluation.py:10-51 -- batch_size Snake engines play
  greedily in lock step, one batched ``select_action`` (the GPU Q tower,
  ``ddq_select_action``) per move; a finished game adds its score and the
  engine restarts, until ``num_trials`` games are done; returns the average
  score.  ``max_moves`` (default None = the reference's unbounded games) ends
  a game that has not finished after that many moves, for drivers that
  cannot risk a policy that circles forever.
  ``streams="per_game"`` gives every engine its own game and random stream
  (the contract of ``ddq_eval_create``, include/ddq_hip.h).
* ``DevicePolicyEvaluator(...).evaluate(model, num_trials)``: that per-game
  evaluation with the games on the device (``ddq_eval_*``): no host copy and
  no synchronisation between moves, the same trials and the same average.
* ``evaluate_model(barista_net, model, num_batches)``: q_convergence.py:15-25
  -- mean of Q_out over ``num_batches`` minibatches sampled from the net's
  dataset.
* ``start(architecture_file, model_file, snapshots, ...)``: evaluation.py:
  54-72 over snapshot files instead of Redis keys; returns {name: average};
  ``device=True`` evaluates with ``DevicePolicyEvaluator``.
"""
from __future__ import annotations

import glob
import os
import pickle
import random
from datetime import datetime

import numpy as np

from .expgain import ExpGain, generate_preprocessor
from .snake import SnakeGame, gray_scale


def save_snapshot(snapshot_name, model, directory="."):
    """tasks.py:25-34.  Returns the file written."""
    filename = os.path.join(directory, snapshot_name + str(datetime.now()))
    snap = {k: [np.array(a, np.float32) for a in v] for k, v in dict(model).items()}
    with open(filename, "wb") as f:
        pickle.dump(snap, f, protocol=2)
    return filename


class _SafeUnpickler(pickle.Unpickler):
    _ALLOWED = {
        ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
        ("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.multiarray", "scalar"),
        ("numpy._core.multiarray", "scalar"), ("_codecs", "encode"),
        ("builtins", "dict"), ("builtins", "list"), ("collections", "OrderedDict"),
    }

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError("snapshot refers to %s.%s: not loaded" % (module, name))


def load_snapshot(path):
    """{name: [W, b]} from a snapshot file (numpy arrays and containers only)."""
    with open(path, "rb") as f:
        snap = _SafeUnpickler(f, encoding="latin1").load()
    if not isinstance(snap, dict):
        raise ValueError("%s: not a snapshot dict" % path)
    return {k: [np.asarray(a, np.float32) for a in v] for k, v in snap.items()}


ACTIONS = ["w", "a", "s", "d"]


def select_trials(logs, num_trials):
    """The trials of a per-game evaluation: ``logs[i]`` holds game i's records
    (end_move, score, moves, ended_by); all records sorted by (end_move, game
    index), the first ``num_trials`` of them -- the order in which
    ``PolicyEvaluator.evaluate`` counts finished games.  Returns a list of
    (end_move, game, score, moves, ended_by)."""
    recs = sorted((int(r[0]), i, int(r[1]), int(r[2]), int(r[3]))
                  for i, log in enumerate(logs) for r in log)
    if len(recs) < num_trials:
        raise ValueError("%d episodes logged, %d trials wanted" % (len(recs), num_trials))
    return recs[:num_trials]


def _start_boards(init_states, n, seed):
    """(n,10,10) start boards: the given one replicated, or one per game."""
    if init_states is None:
        init_states = SnakeGame(random.Random(seed)).encode_state()
    b = np.array(init_states, np.int64)
    if b.ndim == 2:
        b = np.repeat(b[None], n, axis=0)
    if b.shape != (n, 10, 10):
        raise ValueError("start boards %s for %d games" % (b.shape, n))
    return b


class PolicyEvaluator:
    """evaluation.py:10-51.

    ``streams="per_game"`` (with ``epsilon`` and ``init_states``, one board or
    one per engine) is the host form of ``DevicePolicyEvaluator``'s contract:
    engine i plays its own ``SnakeGame`` on ``ActorRng(game_seed(seed, i))``,
    explores with probability ``epsilon`` (no coin is drawn at 0), logs its
    episodes, and the trials are chosen by ``select_trials``.  The defaults
    are the reference's loop: one game object and one stream for all engines."""

    def __init__(self, architecture_file, model_file, net=None, seed=None, max_moves=None,
                 streams="shared", epsilon=0.0, init_states=None):
        from .barista.baristanet import BaristaNet
        if streams not in ("shared", "per_game"):
            raise ValueError("streams must be 'shared' or 'per_game', got %r" % (streams,))
        self.net = net if net is not None else BaristaNet(architecture_file, model_file, None)
        self.batch_size = self.net.batch_size
        self.max_moves = max_moves
        self.streams = streams
        self.epsilon = float(epsilon)
        self.episodes = []
        preprocessor = generate_preprocessor(self.net.state.shape[2:], gray_scale)
        if streams == "per_game":
            from .actor import ActorRng, game_seed
            if not 0.0 <= self.epsilon <= 1.0:
                raise ValueError("epsilon must be in [0,1], got %r" % (epsilon,))
            seed = 0 if seed is None else seed
            n = self.batch_size
            if init_states is not None and np.ndim(init_states) == 3:
                n = len(init_states)
            boards = _start_boards(init_states, n, seed)
            self.engines = []
            for i in range(n):
                game = SnakeGame(random.Random(0))      # (its start apple is never seen)
                game.rng = ActorRng(game_seed(seed, i))
                self.engines.append(ExpGain(self.net, ACTIONS, preprocessor, game.cpu_play,
                                            None, boards[i], rng=game.rng))
            return
        if epsilon != 0.0 or init_states is not None:
            raise ValueError("epsilon / init_states need streams='per_game'")
        game = SnakeGame(random.Random(seed))
        self.engines = [ExpGain(self.net, ACTIONS, preprocessor, game.cpu_play,
                                None, game.encode_state())
                        for _ in range(self.batch_size)]

    def evaluate(self, model, num_trials):
        """Runs ``num_trials`` games and returns the average score."""
        from .barista.netutils import set_net_params
        if model is not None:
            set_net_params(self.net, model)
        for eg in self.engines:
            eg.reset_game()
        if self.streams == "per_game":
            return self._evaluate_per_game(num_trials)
        total_score = 0
        trials_completed = 0
        scores = [0] * self.batch_size
        moves = [0] * self.batch_size
        while trials_completed < num_trials:
            states = np.stack([eg.get_preprocessed_state() for eg in self.engines])
            actions = self.net.select_action(states, batch_size=self.batch_size)
            for i, (action, eg) in enumerate(zip(actions, self.engines)):
                scores[i] += eg.play_action(eg.actions[int(action)])
                moves[i] += 1
                if eg.game_over or (self.max_moves is not None and moves[i] >= self.max_moves):
                    total_score += scores[i]
                    trials_completed += 1
                    if trials_completed == num_trials:
                        break
                    eg.reset_game()
                    scores[i] = 0
                    moves[i] = 0
        return float(total_score) / num_trials

    def _evaluate_per_game(self, num_trials):
        n = len(self.engines)
        for eg in self.engines:
            eg.rng.draws = 0                   # every evaluation starts the streams anew
        max_moves = self.max_moves or 0
        logs = [[] for _ in range(n)]
        scores, moves = [0] * n, [0] * n
        done = move = 0
        while done < num_trials:
            states = np.stack([eg.get_preprocessed_state() for eg in self.engines])
            actions = self.net.select_action(states, batch_size=n)
            for i, eg in enumerate(self.engines):
                if len(logs[i]) >= num_trials:  # a full log: the game is idle
                    continue
                act = int(actions[i])
                if self.epsilon > 0.0 and eg.rng.random() < self.epsilon:
                    act = eg.rng.randrange(len(eg.actions))
                scores[i] += eg.play_action(eg.actions[act])
                moves[i] += 1
                if eg.game_over or (max_moves > 0 and moves[i] >= max_moves):
                    logs[i].append((move, scores[i], moves[i], 0 if eg.game_over else 1))
                    done += 1
                    eg.reset_game()
                    scores[i] = moves[i] = 0
            move += 1
        self.episodes = select_trials(logs, num_trials)
        return float(sum(r[2] for r in self.episodes)) / num_trials


class DevicePolicyEvaluator:
    """``PolicyEvaluator(streams="per_game")`` with the games on the device
    (``ddq_eval_*``): ``games`` (default: the batch size) Snake games in lock
    step on the net's ctx, one batched Q forward and one environment kernel
    per move, nothing copied and nothing synchronised between moves.

    ``evaluate`` enqueues ``chunk`` moves at a time and reads the per-game
    episode counts after each chunk (one synchronise per chunk).  Without
    ``max_moves`` the games are unbounded, as in the reference; ``move_limit``
    raises once that many lock-step moves have not produced the trials."""

    def __init__(self, architecture_file, model_file, net=None, seed=0, max_moves=None,
                 epsilon=0.0, init_state=None, games=None, chunk=32, move_limit=None):
        from .actor import zoom_maps
        from .barista.baristanet import BaristaNet
        self.net = net if net is not None else BaristaNet(architecture_file, model_file, None)
        self.dqn = getattr(self.net, "dqn", self.net)
        self.batch_size = self.dqn.batch
        self.games = self.batch_size if games is None else int(games)
        self.seed = 0 if seed is None else int(seed)
        self.max_moves = max_moves
        self.epsilon = float(epsilon)
        self.chunk = int(chunk)
        if self.chunk < 1:
            raise ValueError("chunk must be >= 1, got %d" % self.chunk)
        self.move_limit = move_limit
        self.boards = _start_boards(init_state, self.games, self.seed)
        S = self.dqn.frame
        self.row_map, self.col_map = zoom_maps((S, S), S)
        self.episodes = []
        self.stats = None

    def evaluate(self, model, num_trials):
        """Runs ``num_trials`` games and returns the average score; the chosen
        records (end_move, game, score, moves, ended_by) stay in ``episodes``."""
        from .barista.netutils import set_net_params
        if model is not None:
            set_net_params(self.net, model)
        num_trials = int(num_trials)
        self.dqn.eval_create(self.boards, self.row_map, self.col_map, self.seed, self.epsilon,
                             self.max_moves or 0, num_trials)
        moves = 0
        while True:
            self.dqn.eval_run(self.chunk)
            moves += self.chunk
            if int(self.dqn.eval_read(full=False).sum()) >= num_trials:
                break
            if self.move_limit is not None and moves >= self.move_limit:
                raise RuntimeError("%d lock-step moves without %d finished games"
                                   % (moves, num_trials))
        out = self.dqn.eval_read()
        self.stats = out["stats"]
        logs = [out["log"][i, :k] for i, k in enumerate(out["episodes"])]
        self.episodes = select_trials(logs, num_trials)
        return float(sum(r[2] for r in self.episodes)) / num_trials


def evaluate_model(barista_net, model, num_batches):
    """q_convergence.py:15-25: average Q_out over ``num_batches`` minibatches."""
    from .barista.netutils import set_net_params
    if model is not None:
        set_net_params(barista_net, model)
    avg_q = 0.0
    for _ in range(num_batches):
        barista_net.load_minibatch()
        barista_net.forward(end="Q_out")
        avg_q += float(np.mean(barista_net.blobs["Q_out"].data))
    return avg_q / num_batches


def start(architecture_file, model_file, snapshots="centralModel-*", num_trials=32,
          results=None, recompute=False, evaluator=None, device=False):
    """evaluation.py:54-72 over snapshot files (a glob or a list) instead of
    Redis keys.  ``results`` (a dict) carries earlier averages; entries are
    recomputed only with ``recompute``.  ``device``: when no evaluator is
    passed, build a ``DevicePolicyEvaluator`` instead of the host one."""
    results = {} if results is None else results
    paths = sorted(glob.glob(snapshots)) if isinstance(snapshots, str) else list(snapshots)
    pe = evaluator
    for path in paths:
        key = os.path.basename(path)
        if key in results and not recompute:
            continue
        if pe is None:
            pe = (DevicePolicyEvaluator if device else PolicyEvaluator)(architecture_file,
                                                                        model_file)
        results[key] = pe.evaluate(load_snapshot(path), num_trials)
    return results
