"""NumPy float64 restatement of the transformer leader's forward pass (evac_transformer.h, include/evac.h evac_transformer_t) --
the yardstick of tests/test_gpu_transformer.py, itself pinned to the reference's own module by the recorded outputs of
tests/golden/transformer_forward.npz (tests/test_transformer_cpu.py).  Written from the function's description, index by index;
the actor-critic behind the encoder is tests/policy_ref.py's."""
from __future__ import annotations

import numpy as np

from tests import policy_ref as R

HEADS = 3
LN_EPS = 1e-5
BLOCK_KEYS = ("attention.Wq.weight", "attention.Wq.bias", "attention.Wk.weight", "attention.Wk.bias", "attention.Wv.weight",
              "attention.Wv.bias", "attention.dense.weight", "attention.dense.bias", "ff.0.weight", "ff.0.bias", "ff.3.weight",
              "ff.3.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def blocks64(sd: dict) -> list:
    """The encoder's tensors of a state dict as float64 arrays: one list of 16 (BLOCK_KEYS order) per block."""
    out, b = [], 0
    while f"embedding.{b}.{BLOCK_KEYS[0]}" in sd:
        out.append([np.asarray(sd[f"embedding.{b}.{k}"].detach().cpu().double().numpy() if hasattr(sd[f"embedding.{b}.{k}"], "detach")
                               else sd[f"embedding.{b}.{k}"], dtype=np.float64) for k in BLOCK_KEYS])
        b += 1
    return out


def params64(net, use_resid=None) -> dict:
    """The tensors of a network with an attention encoder as float64 arrays: policy_ref's dict plus ``blocks`` and ``use_resid``."""
    P = R.params64(net)
    P["blocks"] = blocks64(net.state_dict())
    P["use_resid"] = bool(net.embedding[0].use_resid if use_resid is None else use_resid)
    return P


def layer_norm(v, w, b, variances=None):
    mean = v.mean(axis=-1, keepdims=True)
    var = ((v - mean) ** 2).mean(axis=-1, keepdims=True)            # biased
    if variances is not None:
        variances.append(float(var.min()))
    return (v - mean) / np.sqrt(var + LN_EPS) * w + b


def block(T, x, use_resid, variances=None):
    """One block on tokens x [..., S, dm]; ``variances`` collects the smallest LayerNorm input variance of each norm."""
    wq, bq, wk, bk, wv, bv, wd, bd, w1, b1, w2, b2, n1w, n1b, n2w, n2b = T
    dm = x.shape[-1]
    lead = x.shape[:-1]
    # output index h dm + c  ->  [..., S, h, c]
    q = (x @ wq.T + bq).reshape(lead + (HEADS, dm))
    k = (x @ wk.T + bk).reshape(lead + (HEADS, dm))
    v = (x @ wv.T + bv).reshape(lead + (HEADS, dm))
    # per channel c, contracted over the heads
    score = np.einsum("...ihc,...jhc->...cij", q, k) / np.sqrt(dm)
    score = score - score.max(axis=-1, keepdims=True)
    w = np.exp(score)
    w = w / w.sum(axis=-1, keepdims=True)
    o = np.einsum("...cij,...jhc->...ich", w, v)                   # [..., S, c, h]
    a = o.reshape(lead + (dm * HEADS,)) @ wd.T + bd                # flattened as c H + h
    u = layer_norm(x + a if use_resid else a, n1w, n1b, variances)
    f = np.maximum(u @ w1.T + b1, 0.0) @ w2.T + b2
    return layer_norm(u + f if use_resid else f, n2w, n2b, variances)


def encode(P, x, variances=None):
    """The last block's output of observations x [..., D] read as [..., S, dm], flattened back to [..., D]."""
    x = np.asarray(x, dtype=np.float64)
    dm = P["blocks"][0][0].shape[1]
    t = x.reshape(x.shape[:-1] + (-1, dm))
    for T in P["blocks"]:
        t = block(T, t, P["use_resid"], variances)
    return t.reshape(x.shape)


def min_norm_variance(P, x) -> float:
    """The smallest LayerNorm input variance over the observations x, across both norms of every block."""
    variances = []
    encode(P, x, variances)
    return min(variances)


def actor_mean(P, x):
    return R.actor_mean(P, encode(P, x))


def value(P, x):
    return R.value(P, encode(P, x))


def policy_step(P, x, z):
    """policy_ref.policy_step behind the encoder."""
    return R.policy_step(P, encode(P, x), z)
