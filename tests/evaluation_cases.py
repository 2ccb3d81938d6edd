"""Shared builders of the policy-evaluation tests (tests/test_evaluation_cpu.py, tests/test_gpu_policy_evaluate.py)."""
import os
import types

import numpy as np

from tests.test_gpu_policy_rollout import CASES, OFFSET, SEED, base, i32, make_net, raw   # noqa: F401  (re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agent_vacuum_cleaner.npz")
STATE = ("ped", "status", "agent", "clock", "acc")
N_KERNELS = 10     # policy agents: {gravity, generic} x {raw, frozen norm} x {generic, default-config} = 8; scripted: 2


def make_raw_env(ea, case, E, options=None, **cfg_over):
    """The case's env WITHOUT the normalisation wrapper (one-wave step kernels, as the evaluation's)."""
    from evacuation_amd.options import KernelOptions
    cfg_kw, wrap_kw, _ = CASES[case]
    return ea.BatchedEvacuationEnv(ea.EnvConfig(**{**cfg_kw, **cfg_over}), ea.EnvWrappersConfig(**wrap_kw), num_envs=E, seed=SEED,
                                   env_id_offset=OFFSET, options=options or KernelOptions().replace(subwave=0))


def state_of(env):
    return {k: getattr(base(env), k).clone() for k in STATE}


def set_state(env, s):
    for k in STATE:
        getattr(base(env), k).copy_(s[k])


def assert_state_equal(a, b, what):
    for k in STATE:
        assert raw(a[k]).equal(raw(b[k])), (what, k)


def spread_clocks(env, near_trunc=5):
    """Every `near_trunc`-th env one step before truncation, its neighbour two (as the policy rollout's tests start)."""
    b = base(env)
    st = b.get_state()
    now = st["now"].clone()
    now[::near_trunc] = b.env_config.max_timesteps - 1
    now[1::near_trunc] = b.env_config.max_timesteps - 2
    b.set_state(now=now)


def eval_net(ea, D, seed=0):
    """make_net's recipe with an output bias of (1.5, -1.2): no action of it comes out shorter than 0.1."""
    import torch
    net = make_net(ea, D, seed)
    with torch.no_grad():
        net.actor_mean[4].bias.copy_(torch.tensor([1.5, -1.2], device=net.actor_mean[4].bias.device))
    return net


def fake_env(width, height, step_size):
    """What WacuumCleaner reads of an env: area.width / height / step_size and area.exit.position."""
    area = types.SimpleNamespace(width=width, height=height, step_size=step_size,
                                 exit=types.SimpleNamespace(position=np.array([0, -1], dtype=np.float32)))
    return types.SimpleNamespace(area=area)


def run_until_done(env, agent, n_episodes, max_steps, **kw):
    """policy_evaluate repeated with `max_steps` per call until every env has finished.  Returns (progress, records, calls)."""
    progress = out = None
    calls = 0
    while True:
        progress, out = env.policy_evaluate(agent, n_episodes, max_steps, progress, out, **kw)
        calls += 1
        assert calls < 100000
        if int(progress[:, 0].min()) >= n_episodes:
            return progress, out, calls
