"""What tests/test_gpu_deepsets.py and tests/test_gpu_transformer.py share in front of their tests: the ``ea`` fixture, the
error measure, the frozen statistics, and -- bound to a file's own case table, net recipe and rollout length by
``EncoderCases`` -- the envs of a case, the one shared rollout per (case, E), and the runs of the invariance and evaluation
tests.  Each file keeps its cases, its ``make_net``, its tests and their bounds."""
import numpy as np
import pytest

from tests.test_gpu_policy_rollout import OFFSET, SEED, base, i32, raw, replay_env_side, snapshot, start


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
    ``make_net(case)``: the file's network of a case; ``t_steps``: the length of the shared rollout; ``cfg_over``: fields of
    every case's EnvConfig to replace (tests/test_gpu_policy_long.py: max_timesteps)."""

    def __init__(self, cases, make_net, t_steps, **cfg_over):
        self.cases, self.make_net, self.t_steps, self.cfg_over = cases, make_net, t_steps, cfg_over
        self._runs = {}

    def make_env(self, ea, case, E, raw_env=False, **options):
        from evacuation_amd.options import KernelOptions
        cfg_kw, wrap_kw, norm, opts = self.cases[case][:4]
        opts = {**opts, **options}
        cfg_kw = {**cfg_kw, **self.cfg_over}
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

    def policy_noise(self, total0, T):
        """The restated Philox draws of steps 0..T-1 of envs whose step counts start at ``total0``: float64 [T, E, 2]."""
        from tests import policy_ref as R
        gid = (OFFSET + np.arange(total0.shape[0])).astype(np.uint32)
        steps = np.arange(T, dtype=np.int64)
        return R.policy_normal(SEED, gid[None, :], (total0[None, :] + steps[:, None]).astype(np.uint32))

    def env_side_bit_for_bit(self, ea, case, E):
        """Test 2 of the two files: a twin handle (subwave = 0) replays the shared rollout's recorded actions through step()."""
        import torch
        net, ro, obs0, _, fin, ns0 = self.rollout_of(ea, case, E)
        twin = self.make_env(ea, case, E, subwave=0)
        obs_b, _ = start(twin)
        assert i32(obs0).equal(i32(obs_b))
        if ns0 is not None:
            twin.norm_state.copy_(ns0)
        n_done = replay_env_side(ea, twin, ro, obs0, self.t_steps, case)
        assert n_done >= E // 5                       # autoresets inside the call
        torch.cuda.synchronize()
        end = snapshot(twin)
        for k in fin:                                 # ped, status, agent, clock, acc (and norm_state)
            assert raw(fin[k]).equal(raw(end[k])), (case, k)
        twin.close()

    def run(self, ea, case, E, T_split, net):
        env = self.make_env(ea, case, E)
        obs, done = start(env)
        outs = [{k: v.clone() for k, v in env.policy_rollout(net, T, obs, done).items()} for T in T_split]
        fin = snapshot(env)
        env.close()
        return outs, fin

    def evaluation_is_the_rollout(self, ea, case, mode, E=48, T=40):
        """Test 4a of the two files: policy_evaluate(max_steps = T) against policy_rollout(T) on a twin handle -- in mean mode
        with the twin's actor_logstd at -inf (expf gives 0 exactly).  Returns the rollout's [T, E] episode ends."""
        import copy

        import torch
        a, b = self.twins(ea, case, E)
        net = self.make_net(case)
        twin_net = net
        if mode == "mean":
            twin_net = copy.deepcopy(net)
            with torch.no_grad():
                twin_net.actor_logstd.fill_(float("-inf"))
        obs = b.observe().clone()
        done = torch.zeros(E, dtype=torch.float32, device=b.device)
        ro = b.policy_rollout(twin_net, T, obs, done)
        progress, rec = a.policy_evaluate(net, T, T, deterministic=(mode == "mean"))
        torch.cuda.synchronize()
        for k in ("ped", "status", "agent", "clock", "acc"):
            assert raw(getattr(a, k)).equal(raw(getattr(b, k))), (case, mode, k)
        assert progress[:, 1].eq(T).all() and progress[:, 2:].eq(0).all()
        ended = torch.cat([ro["dones"][1:].bool(), ro["next_done"].bool()[None]], dim=0)
        assert int(ended.sum()) >= E // 5
        assert progress[:, 0].equal(ended.sum(0).to(torch.int32))
        for e in range(E):
            rows = ro["episode_stats"][ended[:, e], e]
            n = rows.shape[0]
            assert i32(rec[:n, e]).equal(i32(rows)), (case, mode, e)
            assert i32(rec[n:, e]).eq(0).all(), (case, mode, e)
        a.close(); b.close()
        return ended.cpu().numpy()

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
