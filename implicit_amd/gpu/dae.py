"""Mult-DAE on MI355X: the multinomial denoising autoencoder of Liang, Krishnan, Hoffman and Jebara, "Variational
Autoencoders for Collaborative Filtering" (WWW 2018), one tanh hidden layer.

No reference counterpart.  Training runs one imp_dae_step call per mini-batch (dae_step, csrc/mult_dae.hip, which states
the model): the batch x items logits are never stored.  The item side is W_out with the output bias as its last column, the
user side [h, 1] with h the encoder's output, so recommend / similar_* / rank_items / diversify_items / save / load / pickling
come from MatrixFactorizationBase unchanged; recalculate_user encodes the rows it is given, for users the model never saw.
"""
import logging
import time

import numpy as np

import implicit_amd.gpu as gpu

from ..utils import check_csr, check_random_state
from .als import _progress
from .matrix_factorization_base import MatrixFactorizationBase

log = logging.getLogger("implicit_amd")


def _pattern(user_items):
    """The matrix as the kernels read it: CSR, float32, every row strictly ascending.  The caller's matrix stays as it was."""
    user_items = check_csr(user_items)
    if user_items.dtype != np.float32:
        user_items = user_items.astype(np.float32)
    if not user_items.has_canonical_format:
        user_items = user_items.copy()
        user_items.sum_duplicates()
    return user_items


class MultDAE(MatrixFactorizationBase):
    """hidden: width of the hidden layer, a multiple of 32 in 32 .. 512.  dropout: share of a row's items dropped from the
    encoder's input in training.  learning_rate, beta1, beta2, eps: Adam, applied densely each step.  regularization: L2
    weight decay on the two weight matrices (not the biases).  batch_size: users per step, a multiple of 64.  iterations:
    epochs over the shuffled users.  random_state: int, numpy RandomState / Generator or None -- seeds the initial weights,
    the epochs' permutations and the dropout streams.  fit's `callback(epoch, elapsed, loss)`: the mean loss of the epoch's
    steps.  The defaults follow the paper where it gives one; none was tuned here."""

    def __init__(self, hidden=256, dropout=0.5, learning_rate=1e-3, regularization=0.0, batch_size=512, iterations=20,
                 beta1=0.9, beta2=0.999, eps=1e-8, random_state=None):
        super().__init__()
        if not gpu.HAS_CUDA:
            raise ValueError("No usable HIP device / extension, can't train on GPU.")
        if not 32 <= int(hidden) <= 512 or int(hidden) % 32:
            raise ValueError("hidden must be a multiple of 32 in 32 .. 512")
        if int(batch_size) < 64 or int(batch_size) % 64:
            raise ValueError("batch_size must be a multiple of 64")
        if not 0 <= dropout < 1:
            raise ValueError("dropout must lie in [0, 1)")
        self.hidden = int(hidden)
        self.dropout = dropout
        self.learning_rate = learning_rate
        self.regularization = regularization
        self.batch_size = int(batch_size)
        self.iterations = iterations
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        self.random_state = random_state
        self.W_in = self.b_in = None

    @property
    def factors(self):
        return self.hidden

    def fit(self, user_items, show_progress=True, callback=None):
        """Trains on a (users x items) CSR matrix; every stored entry is a positive, its value is ignored."""
        rs = check_random_state(self.random_state)
        user_items = _pattern(user_items)
        users, items = user_items.shape
        H, B = self.hidden, self.batch_size
        if self.item_factors is None:  # Glorot normal weights, zero biases
            std = np.sqrt(2.0 / (items + H))
            self.W_in = gpu.Matrix((rs.standard_normal((items, H)) * std).astype(np.float32))
            self.b_in = gpu.Matrix(np.zeros((1, H), dtype=np.float32))
            W_out = (rs.standard_normal((items, H + 1)) * std).astype(np.float32)
            W_out[:, H] = 0.0
            self.item_factors = gpu.Matrix(W_out)
        self._item_norms = self._user_norms = None
        self._item_norms_host = self._user_norms_host = None

        csr = gpu.CSRMatrix(user_items)
        params = (self.W_in, self.b_in, self.item_factors)
        moments = tuple(gpu.Matrix.zeros(*p.shape) for p in params for _ in range(2))
        log.debug("Running %i Mult-DAE training epochs", self.iterations)
        progress = _progress(self.iterations, show_progress)
        step = 0
        for epoch in range(self.iterations):
            t0 = time.time()
            order = rs.permutation(users).astype(np.int32)
            order = np.concatenate([order, np.full(-len(order) % B, -1, dtype=np.int32)])  # the last batch's padding: empty rows
            losses = []
            for b in range(0, len(order), B):
                step += 1
                losses.append(gpu.dae_step(csr, order[b:b + B], params, moments, self.dropout, rs.integers(2**31),
                                           self.learning_rate, step, self.regularization, self.beta1, self.beta2, self.eps))
            loss = float(np.mean(losses)) if losses else 0.0
            progress.update(None)
            if progress.bar is not None:
                progress.bar.set_postfix({"loss": f"{loss:0.4f}"})
            if callback:
                callback(epoch, time.time() - t0, loss)
        progress.close()
        self.user_factors = gpu.dae_encode(csr, np.arange(users, dtype=np.int32), self.W_in, self.b_in)
        self._check_fit_errors()

    def recalculate_user(self, userid, user_items):
        """[h, 1] of the rows of user_items, one per entry of userid -- whose values are not read: the rows need not belong
        to users the model was trained on."""
        user_items = _pattern(user_items)
        if user_items.shape[1] != self.item_factors.shape[0]:
            raise ValueError("user_items must have one column per item of the model")
        return gpu.dae_encode(gpu.CSRMatrix(user_items), np.arange(user_items.shape[0], dtype=np.int32), self.W_in, self.b_in)

    _npz_keys = ("hidden", "dropout", "learning_rate", "regularization", "batch_size", "iterations", "beta1", "beta2", "eps",
                 "random_state")
    _npz_stale = ("dtype",)
    _npz_dtype = np.float32

    def save(self, fileobj_or_path):
        args = {"user_factors": self.user_factors, "item_factors": self.item_factors, "W_in": self.W_in, "b_in": self.b_in}
        args = {k: v.to_numpy() for k, v in args.items() if v is not None}
        args.update({key: getattr(self, key) for key in self._npz_keys})
        if not isinstance(self.random_state, (int, np.integer)):
            del args["random_state"]
        np.savez(fileobj_or_path, **args)

    @classmethod
    def load(cls, fileobj_or_path):
        model = super().load(fileobj_or_path)
        for name in ("W_in", "b_in"):
            if isinstance(getattr(model, name, None), np.ndarray):
                setattr(model, name, gpu.Matrix(np.ascontiguousarray(getattr(model, name), dtype=np.float32)))
        return model

    def __getstate__(self):
        state = super().__getstate__()
        for name in ("W_in", "b_in"):
            state[name] = None if state[name] is None else state[name].to_numpy()
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        for name in ("W_in", "b_in"):
            if getattr(self, name) is not None:
                setattr(self, name, gpu.Matrix(getattr(self, name)))
