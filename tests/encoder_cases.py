"""What tests/test_gpu_deepsets.py and tests/test_gpu_transformer.py share in front of their tests: the ``ea`` fixture, the
error measure, the frozen statistics, and -- bound to a file's own case table, net recipe and rollout length by
``EncoderCases`` -- the envs of a case, the one shared rollout per (case, E), and the runs of the invariance and evaluation
tests.  Each file keeps its cases, its ``make_net``, its tests and their bounds."""
import numpy as np
import pytest

from tests.test_gpu_policy_rollout import OFFSET, SEED, base, snapshot, start


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import evacuation_amd
    from evacuation_amd import build
    build.build_library()
    return evacuation_amd


def rel_err(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _frozen(env, E):
    import torch
    g = torch.Generator().manual_seed(5)
    D = env.obs_dim
    ns = torch.zeros((E, 3 * D + 4), dtype=torch.float64)
    ns[:, :D] = torch.randn((E, D), generator=g, dtype=torch.float64) * 0.1
    ns[:, D:2 * D] = torch.rand((E, D), generator=g, dtype=torch.float64) + 0.05
    return ns.to(env.device)


class EncoderCases:
    """``cases``: name -> (EnvConfig kwargs, EnvWrappersConfig kwargs, normalised chain, KernelOptions overrides, ...);
    ``make_net(case)``: the file's network of a case; ``t_steps``: the length of the shared rollout."""

    def __init__(self, cases, make_net, t_steps):
        self.cases, self.make_net, self.t_steps = cases, make_net, t_steps
        self._runs = {}

    def make_env(self, ea, case, E, raw_env=False, **options):
        from evacuation_amd.options import KernelOptions
        cfg_kw, wrap_kw, norm, opts = self.cases[case][:4]
        opts = {**opts, **options}
        env = ea.BatchedEvacuationEnv(ea.EnvConfig(**cfg_kw), ea.EnvWrappersConfig(**wrap_kw), num_envs=E, seed=SEED, env_id_offset=OFFSET,
                                      options=KernelOptions().replace(**opts) if opts else None)
        return ea.NormalizedVectorEnv(env) if norm and not raw_env else env

    def rollout_of(self, ea, case, E):
        """One rollout of ``t_steps`` per (case, E), shared by the tests and left unchanged: (net, storage, start observation,
        the envs' step counts at the start, final snapshot, norm_state at the start or None)."""
        key = (case, E)
        if key not in self._runs:
            import torch
            env = self.make_env(ea, case, E)
            net = self.make_net(case)
            obs, done = start(env)
            ns0 = env.norm_state.clone() if hasattr(env, "norm_state") else None
            total0 = base(env).clock[:, 2].cpu().numpy().astype(np.int64)
            obs0 = obs.clone()
            ro = env.policy_rollout(net, self.t_steps, obs, done)
            torch.cuda.synchronize()
            assert ro["next_obs"] is obs and ro["next_done"] is done
            self._runs[key] = (net, {k: v.clone() for k, v in ro.items()}, obs0, total0, snapshot(env), ns0)
            env.close()
        return self._runs[key]

    def run(self, ea, case, E, T_split, net):
        env = self.make_env(ea, case, E)
        obs, done = start(env)
        outs = [{k: v.clone() for k, v in env.policy_rollout(net, T, obs, done).items()} for T in T_split]
        fin = snapshot(env)
        env.close()
        return outs, fin

    def twins(self, ea, case, E):
        a, b = self.make_env(ea, case, E, raw_env=True, subwave=0), self.make_env(ea, case, E, raw_env=True, subwave=0)
        a.reset()
        b.reset()
        for env in (a, b):
            st = env.get_state()
            now = st["now"].clone()
            now[::5] = env.env_config.max_timesteps - 1
            now[1::5] = env.env_config.max_timesteps - 2
            env.set_state(now=now)
        return a, b
