"""NumPy float64 restatement of the deep-sets leader's forward pass (evac_deepsets.h, include/evac.h evac_deepsets_t) -- the
yardstick of tests/test_gpu_deepsets.py, itself pinned to the reference's own module by the recorded outputs of
tests/golden/deepsets_forward.npz (tests/test_deepsets_cpu.py).  The actor-critic behind the encoder is tests/policy_ref.py's."""
from __future__ import annotations

import numpy as np

from tests import policy_ref as R

ENCODER_KEYS = ("deep_sets.transform_phi.0.weight", "deep_sets.transform_phi.0.bias", "deep_sets.transform_phi.2.weight",
                "deep_sets.transform_phi.2.bias", "deep_sets.transform_rho.0.weight", "deep_sets.transform_rho.0.bias")


def params64(net) -> dict:
    """The 19 tensors of a network with a set encoder as float64 arrays: policy_ref's dict plus ``enc`` (ENCODER_KEYS order)."""
    P = R.params64(net)
    sd = net.state_dict()
    P["enc"] = [sd[k].detach().cpu().double().numpy() for k in ENCODER_KEYS]
    return P


def encode(P, x):
    """y = W_r sum_i (W_b relu(W_a x_i + b_a) + b_b) + b_r of observations x [..., D] read as [..., S, ed] -- element by element,
    as the reference's module does it."""
    wa, ba, wb, bb, wr, br = P["enc"]
    x = np.asarray(x, dtype=np.float64)
    rows = x.reshape(x.shape[:-1] + (-1, wa.shape[1]))
    phi = np.maximum(rows @ wa.T + ba, 0.0) @ wb.T + bb
    return phi.sum(axis=-2) @ wr.T + br


def actor_mean(P, x):
    return R.actor_mean(P, encode(P, x))


def value(P, x):
    return R.value(P, encode(P, x))


def policy_step(P, x, z):
    """policy_ref.policy_step behind the encoder."""
    return R.policy_step(P, encode(P, x), z)
