"""GRU4Rec on MI355X: session-based next-item recommendation with one GRU layer (Hidasi, Karatzoglou, Baltrunas, Tikk, ICLR
2016; Hidasi and Karatzoglou, "Recurrent Neural Networks with Top-k Gains", CIKM 2018).

No reference counterpart.  Training is session-parallel: batch_size slots each walk one session, a slot that finishes takes the
next session of the epoch's permutation.  steps_per_call steps are queued by one imp_gru_steps call (gru_steps,
csrc/gru4rec.hip, which states the model).  The item side is W_out with the output bias as its last column, the "user" side
[h | 1] with h the state after a session's last item -- one user per training session -- so recommend / similar_items /
rank_items / diversify_items / save / load / pickling come from MatrixFactorizationBase; recommend_sessions serves sessions
the model never saw."""
import logging
import time

import numpy as np

import implicit_amd.gpu as gpu

from ..utils import check_random_state
from .als import _progress
from .matrix_factorization_base import MatrixFactorizationBase

log = logging.getLogger("implicit_amd")

LOSSES = ("cross-entropy", "bpr-max")


def as_sessions(sessions):
    """(indptr int64, items int32) of a sequence of 1-d integer arrays in event order, or of such a pair itself."""
    if isinstance(sessions, tuple) and len(sessions) == 2 and np.ndim(sessions[0]) == 1 and np.ndim(sessions[1]) == 1 and \
            len(sessions[0]) and np.asarray(sessions[0])[-1] == len(sessions[1]) and np.asarray(sessions[0])[0] == 0:
        indptr, items = np.asarray(sessions[0], dtype=np.int64), np.asarray(sessions[1])
    else:
        sessions = [np.asarray(s).reshape(-1) for s in sessions]
        indptr = np.concatenate([[0], np.cumsum([len(s) for s in sessions])]).astype(np.int64)
        items = np.concatenate(sessions) if sessions else np.zeros(0, dtype=np.int32)
    if items.size and items.dtype.kind not in "iu":
        raise ValueError("session items must be integers")
    if (np.diff(indptr) < 0).any():
        raise ValueError("indptr must not decrease")
    return indptr, np.ascontiguousarray(items, dtype=np.int32)


def session_parallel_schedule(indptr, items, order, batch_size):
    """Host only: the session-parallel schedule of one epoch.  Slot r starts with session order[r]; when its session has no
    pair left it takes the next unused session of `order` (slots served in ascending r), and goes idle for good once
    `order` is exhausted.  Every session of `order` must hold two items or more.  Returns (inputs, targets, reset), int32
    [steps x batch_size]: an idle slot holds (-1, -1, 0), reset is 1 at a session's first pair."""
    indptr, order, B = np.asarray(indptr, dtype=np.int64), np.asarray(order, dtype=np.int64), int(batch_size)
    session = np.full(B, -1, dtype=np.int64)
    n_first = min(B, len(order))
    session[:n_first] = order[:n_first]
    taken, pos = n_first, np.zeros(B, dtype=np.int64)
    inputs, targets, reset = [], [], []
    while (session >= 0).any():
        live = session >= 0
        at = np.where(live, indptr[np.maximum(session, 0)] + pos, 0)
        inputs.append(np.where(live, items[at], -1))
        targets.append(np.where(live, items[np.minimum(at + 1, len(items) - 1)], -1))
        reset.append((live & (pos == 0)).astype(np.int32))
        pos += 1
        done = np.nonzero(live & (indptr[np.maximum(session, 0)] + pos + 1 >= indptr[np.maximum(session, 0) + 1]))[0]
        fresh = order[taken:taken + len(done)]
        session[done] = -1
        session[done[:len(fresh)]] = fresh
        pos[done] = 0
        taken += len(fresh)
    shape = (len(inputs), B)
    return tuple(np.asarray(a, dtype=np.int32).reshape(shape) for a in (inputs, targets, reset))


class GRU4Rec(MatrixFactorizationBase):
    """hidden: width of the GRU, a multiple of 32 in 32 .. 512.  loss: "bpr-max" or "cross-entropy".  n_sample: extra negatives
    shared by a step's rows, a multiple of 64 in 0 .. 4096, drawn proportional to support ** sample_alpha.  bpreg: the score
    regularisation of bpr-max.  learning_rate: Adagrad.  batch_size: sessions walked in parallel, a multiple of 64 in 64 ..
    1024.  iterations: epochs.  steps_per_call: steps queued per library call.  random_state: int, numpy RandomState /
    Generator or None -- seeds the weights, the epochs' permutations and the negatives.  fit's `callback(epoch, elapsed,
    loss)`: the mean loss of the epoch's steps.  The defaults are placeholders: none was tuned on real data."""

    def __init__(self, hidden=128, loss="bpr-max", n_sample=2048, sample_alpha=0.75, bpreg=1.0, learning_rate=0.1, batch_size=64,
                 iterations=10, steps_per_call=64, random_state=None):
        super().__init__()
        if not gpu.HAS_CUDA:
            raise ValueError("No usable HIP device / extension, can't train on GPU.")
        if not 32 <= int(hidden) <= 512 or int(hidden) % 32:
            raise ValueError("hidden must be a multiple of 32 in 32 .. 512")
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}")
        if not 0 <= int(n_sample) <= 4096 or int(n_sample) % 64:
            raise ValueError("n_sample must be a multiple of 64 in 0 .. 4096")
        if not 64 <= int(batch_size) <= 1024 or int(batch_size) % 64:
            raise ValueError("batch_size must be a multiple of 64 in 64 .. 1024")
        if int(steps_per_call) < 1:
            raise ValueError("steps_per_call must be at least 1")
        self.hidden = int(hidden)
        self.loss = loss
        self.n_sample = int(n_sample)
        self.sample_alpha = sample_alpha
        self.bpreg = bpreg
        self.learning_rate = learning_rate
        self.batch_size = int(batch_size)
        self.iterations = iterations
        self.steps_per_call = int(steps_per_call)
        self.random_state = random_state
        self.W_x = self.W_h = self.b = None

    @property
    def factors(self):
        return self.hidden

    def fit(self, sessions, n_items=None, show_progress=True, callback=None):
        """Trains on sessions: a sequence of 1-d integer arrays in event order, or a pair (indptr, items).  Sessions shorter
        than two items are skipped for training (they still receive a row of user_factors)."""
        rs = check_random_state(self.random_state)
        indptr, items = as_sessions(sessions)
        if items.size and items.min() < 0:
            raise IndexError("a session item is negative")
        n_items = int(items.max()) + 1 if n_items is None else int(n_items)
        if items.size and items.max() >= n_items:
            raise IndexError("a session item is not below n_items")
        H, B, N = self.hidden, self.batch_size, self.n_sample
        if self.item_factors is None:  # uniform in +- sqrt(6 / (rows + columns)), zero biases
            def uniform(rows, cols):
                bound = np.sqrt(6.0 / (rows + cols))
                return rs.uniform(-bound, bound, size=(rows, cols)).astype(np.float32)

            self.W_x, self.W_h = gpu.Matrix(uniform(n_items, 3 * H)), gpu.Matrix(uniform(H, 3 * H))
            self.b = gpu.Matrix(np.zeros((1, 3 * H), dtype=np.float32))
            W_out = uniform(n_items, H + 1)
            W_out[:, H] = 0.0
            self.item_factors = gpu.Matrix(W_out)
        elif self.item_factors.shape[0] != n_items:
            raise ValueError("the model was fitted with another number of items")
        self._item_norms = self._user_norms = None
        self._item_norms_host = self._user_norms_host = None

        trainable = np.nonzero(np.diff(indptr) >= 2)[0]
        keep = np.concatenate([np.arange(indptr[s], indptr[s + 1]) for s in trainable]) if len(trainable) else np.zeros(0, dtype=np.int64)
        support = np.bincount(items[keep], minlength=n_items).astype(np.float64) ** self.sample_alpha
        params = (self.W_x, self.W_h, self.b, self.item_factors)
        accumulators = tuple(gpu.Matrix.zeros(*p.shape) for p in params)
        log.debug("Running %i GRU4Rec training epochs", self.iterations)
        progress = _progress(self.iterations, show_progress)
        for epoch in range(self.iterations):
            t0 = time.time()
            inputs, targets, reset = session_parallel_schedule(indptr, items, trainable[rs.permutation(len(trainable))], B)
            steps = len(inputs)
            negatives = np.zeros((steps, N), dtype=np.int32)
            if N and steps:
                negatives = rs.choice(n_items, size=(steps, N), p=support / support.sum()).astype(np.int32)
            h, losses = gpu.Matrix.zeros(B, H), []
            for t in range(0, steps, self.steps_per_call):
                cut = slice(t, t + self.steps_per_call)
                losses.append(gpu.gru_steps(params, accumulators, h, inputs[cut], targets[cut], reset[cut], negatives[cut], self.loss,
                                            self.bpreg, self.learning_rate))
            loss = float(np.mean(np.concatenate(losses))) if losses else 0.0
            progress.update(None)
            if progress.bar is not None:
                progress.bar.set_postfix({"loss": f"{loss:0.4f}"})
            if callback:
                callback(epoch, time.time() - t0, loss)
        progress.close()
        self.user_factors = gpu.gru_encode(indptr, items, self.W_x, self.W_h, self.b)
        self._check_fit_errors()

    def encode_sessions(self, sessions):
        """[h | 1] after the last item of each session, a device Matrix: the query rows against item_factors."""
        indptr, items = as_sessions(sessions)
        return gpu.gru_encode(indptr, items, self.W_x, self.W_h, self.b)

    def recommend_sessions(self, sessions, N=10, filter_seen=False):
        """The top N next items of sessions the model need not have seen: (ids, scores), [sessions x N].  filter_seen: a
        session's own items are not recommended to it."""
        indptr, items = as_sessions(sessions)
        query = gpu.gru_encode(indptr, items, self.W_x, self.W_h, self.b)
        seen = None
        if filter_seen and len(items):
            from scipy.sparse import csr_matrix

            seen = csr_matrix((np.ones(len(items), dtype=np.float32), items, indptr), shape=(len(indptr) - 1, self.item_factors.shape[0]))
            seen.sum_duplicates()
            seen = self._liked_filter(seen)
        return self.knn.topk(self.item_factors, query, N, query_filter=seen)

    def recalculate_user(self, userid, user_items):
        raise ValueError("GRU4Rec cannot recalculate a user from a CSR row, which has no order: use recommend_sessions(sessions)")

    _npz_keys = ("hidden", "loss", "n_sample", "sample_alpha", "bpreg", "learning_rate", "batch_size", "iterations", "steps_per_call",
                 "random_state")
    _npz_stale = ("dtype",)
    _npz_dtype = np.float32
    _weights = ("W_x", "W_h", "b")

    def save(self, fileobj_or_path):
        args = {"user_factors": self.user_factors, "item_factors": self.item_factors}
        args.update({name: getattr(self, name) for name in self._weights})
        args = {k: v.to_numpy() for k, v in args.items() if v is not None}
        args.update({key: getattr(self, key) for key in self._npz_keys})
        if not isinstance(self.random_state, (int, np.integer)):
            del args["random_state"]
        np.savez(fileobj_or_path, **args)

    @classmethod
    def load(cls, fileobj_or_path):
        model = super().load(fileobj_or_path)
        for name in cls._weights:
            if isinstance(getattr(model, name, None), np.ndarray):
                setattr(model, name, gpu.Matrix(np.ascontiguousarray(getattr(model, name), dtype=np.float32)))
        return model

    def __getstate__(self):
        state = super().__getstate__()
        for name in self._weights:
            state[name] = None if state[name] is None else state[name].to_numpy()
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        for name in self._weights:
            if getattr(self, name) is not None:
                setattr(self, name, gpu.Matrix(getattr(self, name)))
