"""Mult-VAE on MI355X: the variational autoencoder of Liang, Krishnan, Hoffman and Jebara, "Variational Autoencoders for
Collaborative Filtering" (WWW 2018, Mult-VAE^PR), one tanh layer on either side of a Gaussian code.

No reference counterpart.  Training runs one imp_vae_step call per mini-batch (vae_step, csrc/mult_vae.hip, which states the
model); the KL weight of step t is anneal_cap * min(1, t / anneal_steps).  The item side is W_out with the output bias as its
last column, the user side [h2, 1] with h2 the decoder's hidden layer at z = mu, so serving, save / load and pickling come from
MultDAE and MatrixFactorizationBase; recalculate_user encodes the rows it is given, for users the model never saw.
"""
import logging
import time

import numpy as np

import implicit_amd.gpu as gpu

from ..utils import check_random_state
from .als import _progress
from .dae import MultDAE, _pattern

log = logging.getLogger("implicit_amd")

_EXTRA = ("W_lat", "b_lat", "W_dec", "b_dec")


class MultVAE(MultDAE):
    """hidden, dropout, learning_rate, beta1, beta2, eps, regularization (on the four weight matrices), batch_size, iterations,
    random_state: as MultDAE.  latent: width of the code, a multiple of 32 in 32 .. 256.  anneal_cap: the KL weight the ramp
    ends at.  anneal_steps: steps the ramp takes; None: the first fifth of all steps of this fit.  fit's `callback(epoch,
    elapsed, loss)`: the mean of NLL + beta KL over the epoch's steps.  hidden = 256 stands in for the paper's 600, which the
    decoder's LDS plan does not hold; anneal_cap is the paper's 0.2; the other defaults are placeholders, none was tuned here."""

    def __init__(self, hidden=256, latent=64, dropout=0.5, anneal_cap=0.2, anneal_steps=None, learning_rate=1e-3,
                 regularization=0.0, batch_size=512, iterations=20, beta1=0.9, beta2=0.999, eps=1e-8, random_state=None):
        super().__init__(hidden, dropout, learning_rate, regularization, batch_size, iterations, beta1, beta2, eps, random_state)
        if not 32 <= int(latent) <= 256 or int(latent) % 32:
            raise ValueError("latent must be a multiple of 32 in 32 .. 256")
        if not anneal_cap >= 0:
            raise ValueError("anneal_cap must not be negative")
        if anneal_steps is not None and int(anneal_steps) < 1:
            raise ValueError("anneal_steps must be at least 1")
        self.latent = int(latent)
        self.anneal_cap = anneal_cap
        self.anneal_steps = anneal_steps
        self.W_lat = self.b_lat = self.W_dec = self.b_dec = None

    def _encoder(self):
        return (self.W_in, self.b_in, self.W_lat, self.b_lat, self.W_dec, self.b_dec)

    def fit(self, user_items, show_progress=True, callback=None):
        """Trains on a (users x items) CSR matrix; every stored entry is a positive, its value is ignored."""
        rs = check_random_state(self.random_state)
        user_items = _pattern(user_items)
        users, items = user_items.shape
        H, L, B = self.hidden, self.latent, self.batch_size
        if self.item_factors is None:  # Glorot normal weights, zero biases, in the order of the parameters
            def glorot(rows, cols):
                return (rs.standard_normal((rows, cols)) * np.sqrt(2.0 / (rows + cols))).astype(np.float32)

            self.W_in = gpu.Matrix(glorot(items, H))
            self.b_in = gpu.Matrix(np.zeros((1, H), dtype=np.float32))
            self.W_lat = gpu.Matrix(glorot(H, 2 * L))
            self.b_lat = gpu.Matrix(np.zeros((1, 2 * L), dtype=np.float32))
            self.W_dec = gpu.Matrix(glorot(L, H))
            self.b_dec = gpu.Matrix(np.zeros((1, H), dtype=np.float32))
            W_out = (rs.standard_normal((items, H + 1)) * np.sqrt(2.0 / (items + H))).astype(np.float32)
            W_out[:, H] = 0.0
            self.item_factors = gpu.Matrix(W_out)
        self._item_norms = self._user_norms = None
        self._item_norms_host = self._user_norms_host = None

        csr = gpu.CSRMatrix(user_items)
        params = self._encoder() + (self.item_factors,)
        moments = tuple(gpu.Matrix.zeros(*p.shape) for p in params for _ in range(2))
        per_epoch = -(-users // B)
        ramp = self.anneal_steps if self.anneal_steps is not None else max(1, self.iterations * per_epoch // 5)
        log.debug("Running %i Mult-VAE training epochs", self.iterations)
        progress = _progress(self.iterations, show_progress)
        step = 0
        for epoch in range(self.iterations):
            t0 = time.time()
            order = rs.permutation(users).astype(np.int32)
            order = np.concatenate([order, np.full(-len(order) % B, -1, dtype=np.int32)])  # the last batch's padding: empty rows
            losses = []
            for b in range(0, len(order), B):
                step += 1
                beta = self.anneal_cap * min(1.0, step / ramp)
                nll, kl = gpu.vae_step(csr, order[b:b + B], params, moments, self.dropout, rs.integers(2**31), beta,
                                       self.learning_rate, step, self.regularization, self.beta1, self.beta2, self.eps)
                losses.append(nll + np.float32(beta) * kl)
            loss = float(np.mean(losses)) if losses else 0.0
            progress.update(None)
            if progress.bar is not None:
                progress.bar.set_postfix({"loss": f"{loss:0.4f}"})
            if callback:
                callback(epoch, time.time() - t0, loss)
        progress.close()
        self.user_factors = gpu.vae_encode(csr, np.arange(users, dtype=np.int32), self._encoder())
        self._check_fit_errors()

    def recalculate_user(self, userid, user_items):
        """[h2, 1] at z = mu of the rows of user_items, one per entry of userid -- whose values are not read: the rows need not
        belong to users the model was trained on."""
        user_items = _pattern(user_items)
        if user_items.shape[1] != self.item_factors.shape[0]:
            raise ValueError("user_items must have one column per item of the model")
        return gpu.vae_encode(gpu.CSRMatrix(user_items), np.arange(user_items.shape[0], dtype=np.int32), self._encoder())

    _npz_keys = MultDAE._npz_keys + ("latent", "anneal_cap", "anneal_steps")

    def save(self, fileobj_or_path):
        args = {"user_factors": self.user_factors, "item_factors": self.item_factors, "W_in": self.W_in, "b_in": self.b_in}
        args.update({name: getattr(self, name) for name in _EXTRA})
        args = {k: v.to_numpy() for k, v in args.items() if v is not None}
        args.update({key: getattr(self, key) for key in self._npz_keys if getattr(self, key) is not None})
        if not isinstance(self.random_state, (int, np.integer)):
            args.pop("random_state", None)
        np.savez(fileobj_or_path, **args)

    @classmethod
    def load(cls, fileobj_or_path):
        model = super().load(fileobj_or_path)
        for name in _EXTRA:
            if isinstance(getattr(model, name, None), np.ndarray):
                setattr(model, name, gpu.Matrix(np.ascontiguousarray(getattr(model, name), dtype=np.float32)))
        return model

    def __getstate__(self):
        state = super().__getstate__()
        for name in _EXTRA:
            state[name] = None if state[name] is None else state[name].to_numpy()
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        for name in _EXTRA:
            if getattr(self, name) is not None:
                setattr(self, name, gpu.Matrix(getattr(self, name)))
