"""NumPy float64 restatement of the policy rollout's actor-critic and device noise (evac_policy.h, include/evac.h
evac_policy_rollout) -- the yardstick of tests/test_gpu_policy_rollout.py, itself pinned to torch on the CPU by
tests/test_policy_cpu.py.  The Philox words come from the oracle's philox4x32_10."""
from __future__ import annotations

import numpy as np

from oracle.philox import _key, philox4x32_10

STREAM_POLICY = 0x504F4C49   # 'POLI'
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def policy_normal(seed: int, env_gid, total):
    """The two N(0,1) draws of env ``env_gid`` at its overall step ``total`` (Box-Muller of Philox4x32-10 at counter
    (env, 0, total, 'POLI')), float64 [..., 2]."""
    w = philox4x32_10(env_gid, 0, total, STREAM_POLICY, *_key(seed))
    u1 = ((w[0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=-1)


def params64(net) -> dict:
    """The network's tensors as float64 arrays (RPOLinearNetwork's attribute names)."""
    def f(t):
        return t.detach().cpu().double().numpy()
    a, c = net.actor_mean, net.critic
    return {"aw": [f(a[i].weight) for i in (0, 2, 4)], "ab": [f(a[i].bias) for i in (0, 2, 4)],
            "cw": [f(c[i].weight) for i in (0, 2, 4)], "cb": [f(c[i].bias) for i in (0, 2, 4)],
            "logstd": f(net.actor_logstd).reshape(-1)}


def mlp(ws, bs, x):
    h = np.tanh(x @ ws[0].T + bs[0])
    h = np.tanh(h @ ws[1].T + bs[1])
    return h @ ws[2].T + bs[2]


def actor_mean(P, x):
    return mlp(P["aw"], P["ab"], np.asarray(x, dtype=np.float64))


def value(P, x):
    return mlp(P["cw"], P["cb"], np.asarray(x, dtype=np.float64))[..., 0]


def log_prob(P, mean, action):
    """Normal(mean, exp(logstd)).log_prob(action).sum(-1)."""
    ls = P["logstd"]
    sd = np.exp(ls)
    return (-((action - mean) ** 2) / (2.0 * sd ** 2) - ls - LOG_SQRT_2PI).sum(-1)


def policy_step(P, x, z):
    """mean, action = mean + sigma z, log-prob of the action, value -- of observations x [..., D] and draws z [..., 2]."""
    mean = actor_mean(P, x)
    action = mean + np.exp(P["logstd"]) * z
    return mean, action, log_prob(P, mean, action), value(P, x)
