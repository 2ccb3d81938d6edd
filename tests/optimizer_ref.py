"""The optimiser step of the device trainer (``evac_adam_step``; include/evac.h) in NumPy, operation for operation.

``clip_grad_norm_`` followed by ``torch.optim.Adam`` (no weight decay, no amsgrad), every operation rounded on its own in the
working dtype, except the three scalars formed in double and rounded once.  The bias corrections come from running products
``P1 = beta1 ** t``, ``P2 = beta2 ** t`` kept in double, so that the step count can live beside them on the device.  With
``dtype=np.float32`` this is what the kernel is held to bit for bit; with ``np.float64`` it is Adam to rounding."""
from __future__ import annotations

import numpy as np


class AdamRef:
    """State of one optimiser: ``t``, the running products, and one (exp_avg, exp_avg_sq) pair per tensor."""

    def __init__(self, params, dtype=np.float32, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5):
        self.dtype = np.dtype(dtype).type
        self.lr, self.betas, self.eps, self.max_grad_norm = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(max_grad_norm)
        self.t = 0
        self.P1 = 1.0
        self.P2 = 1.0
        self.exp_avg = [np.zeros_like(np.asarray(p), dtype=self.dtype) for p in params]
        self.exp_avg_sq = [np.zeros_like(np.asarray(p), dtype=self.dtype) for p in params]
        self.last_clip_coef = None

    def clip_coef(self, sumsq):
        """``clamp(max_norm / (total_norm + 1e-6), max=1)``; a NaN stays a NaN."""
        f = self.dtype
        with np.errstate(invalid="ignore", divide="ignore"):
            x = f(f(self.max_grad_norm) / f(np.sqrt(f(sumsq)) + f(1e-6)))
        return f(1.0) if x > f(1.0) else x

    def step(self, params, grads, sumsq=None):
        """One step in place on ``params`` (arrays of ``dtype``); ``grads`` are left clipped.  ``sumsq``: the sum of squares of
        all gradient entries (default: summed here in ``dtype``, tensor by tensor)."""
        f = self.dtype
        if sumsq is None:
            sumsq = f(0)
            for g in grads:
                sumsq = f(sumsq + np.sum(np.square(g, dtype=f), dtype=f))
        c = self.clip_coef(sumsq)
        self.last_clip_coef = c
        b1, b2 = self.betas
        self.t += 1
        self.P1 *= b1
        self.P2 *= b2
        a = f(-(self.lr / (1.0 - self.P1)))
        q = f(np.sqrt(1.0 - self.P2))
        w, b2f, u, e = f(1.0 - b1), f(b2), f(1.0 - b2), f(self.eps)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for p, g, m, v in zip(params, grads, self.exp_avg, self.exp_avg_sq):
                assert p.dtype == f and g.dtype == f, "optimizer_ref: arrays of the working dtype"
                g *= c
                m += w * (g - m)
                v *= b2f
                v += (u * g) * g
                p += (a * m) / (np.sqrt(v) / q + e)
