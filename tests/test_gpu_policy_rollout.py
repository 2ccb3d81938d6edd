"""The policy rollout (evac_policy_rollout, BatchedEvacuationEnv / NormalizedVectorEnv.policy_rollout) on an MI355X.

1. Policy outputs, teacher-forced on the kernel's own inputs: every step's recorded observation gives mean, sigma, the restated
   Philox draw z, the action, its log-prob and the value in float64 (tests/policy_ref.py); z over >= 10^5 draws is N(0, 1).
2. The env side, bit for bit: a twin handle with the same seed and start state replays the recorded actions through step() of
   the one-wave family
   (fused chain with a cloned norm_state, or the raw step) -- observations, rewards, dones, norm_state, episode records and the
   final state are identical as int32 views.  Some envs start one step before truncation, so autoresets happen inside the call.
3. Invariance: T = 33 in one call == 7 + 26; kernel options and handle forms give the same bits.
4. Errors.  5. Capture into a graph: weights changed in place are read at replay."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, OFFSET = 20261016, 3

CASES = {
    # name: (EnvConfig kwargs, EnvWrappersConfig kwargs, normalised chain)
    "n60_grav_norm_clip": (dict(number_of_pedestrians=60, is_new_exiting_reward=True, max_timesteps=25, clip_action=True),
                           dict(positions="grav", alpha=3), True),
    "n60_rel_ohe_box_norm_clip": (dict(number_of_pedestrians=60, max_timesteps=25, clip_action=True),
                                  dict(positions="rel", statuses="ohe", type="Box"), True),
    "n10_grav_raw": (dict(number_of_pedestrians=10, max_timesteps=20, intrinsic_reward_coef=0.5), dict(positions="grav", alpha=2), False),
    "n32_abs_cat_dict_norm": (dict(number_of_pedestrians=32, max_timesteps=22, enslaving_degree=0.7, clip_action=True),
                              dict(positions="abs", statuses="cat"), True),
    "n64_grav_wallterm_noise_raw": (dict(number_of_pedestrians=64, max_timesteps=30, is_termination_agent_wall_collision=True,
                                         noise_coef=1.2, step_size=0.05), dict(positions="grav", alpha=3), False),
    "n64_abs_ohe_box_norm": (dict(number_of_pedestrians=64, max_timesteps=25, is_new_exiting_reward=True),
                             dict(positions="abs", statuses="ohe", type="Box"), True),
}


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import evacuation_amd
    from evacuation_amd import build
    build.build_library()
    return evacuation_amd


def make_env(ea, case, E, options=None, seed=SEED, **cfg_over):
    """The case's env; ``cfg_over`` replaces fields of its EnvConfig (tests/test_gpu_policy_long.py: max_timesteps)."""
    cfg_kw, wrap_kw, norm = CASES[case]
    env = ea.BatchedEvacuationEnv(ea.EnvConfig(**{**cfg_kw, **cfg_over}), ea.EnvWrappersConfig(**wrap_kw), num_envs=E, seed=seed,
                                  env_id_offset=OFFSET, options=options)
    return ea.NormalizedVectorEnv(env) if norm else env


def base(env):
    return getattr(env, "env", env)


def make_net(ea, D, seed=0):
    import torch
    from evacuation_amd.policy import LinearActorCritic
    torch.manual_seed(seed)
    net = LinearActorCritic(D)
    with torch.no_grad():       # visible actions and values: larger last layers, non-zero biases, two different sigmas
        net.actor_mean[4].weight.mul_(60.0)
        net.actor_logstd.copy_(torch.tensor([[-0.5, 0.3]]))
        for m in list(net.actor_mean) + list(net.critic):
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.2)
    return net.to("cuda:0")


def start(env, near_trunc=5):
    """reset; every `near_trunc`-th env one step before truncation.  Returns (next_obs, next_done)."""
    import torch
    obs, _ = env.reset()
    b = base(env)
    if near_trunc:
        st = b.get_state()
        now = st["now"].clone()
        now[::near_trunc] = b.env_config.max_timesteps - 1
        now[1::near_trunc] = b.env_config.max_timesteps - 2
        b.set_state(now=now)
    return obs.clone(), torch.zeros(b.num_envs, dtype=torch.float32, device=b.device)


def i32(t):
    import torch
    return t.contiguous().view(torch.int32)


def raw(t):
    import torch
    return t.contiguous().view(-1).view(torch.uint8)


def snapshot(env):
    b = base(env)
    s = {k: getattr(b, k).clone() for k in ("ped", "status", "agent", "clock", "acc")}
    if hasattr(env, "norm_state"):
        s["norm_state"] = env.norm_state.clone()
    return s


def restore(env, s):
    b = base(env)
    for k in ("ped", "status", "agent", "clock", "acc"):
        getattr(b, k).copy_(s[k])
    if "norm_state" in s:
        env.norm_state.copy_(s["norm_state"])


OUT_KEYS = ("obs", "actions", "logprobs", "values", "rewards", "dones", "next_value", "episode_stats", "next_obs", "next_done")


def assert_same(ro, rb, what):
    for k in OUT_KEYS:
        assert i32(ro[k]).equal(i32(rb[k])), (what, k)


def check_policy_outputs(ea, env, net, ro, total0, seed=SEED):
    """1. every step's policy outputs against the float64 restatement on the recorded observation"""
    from tests import policy_ref as R
    b = base(env)
    P = R.params64(net)
    E = b.num_envs
    gid = (OFFSET + np.arange(E)).astype(np.uint32)
    obs, act = ro["obs"].cpu().double().numpy(), ro["actions"].cpu().double().numpy()
    lp, val = ro["logprobs"].cpu().double().numpy(), ro["values"].cpu().double().numpy()
    sd = np.exp(P["logstd"])
    zs = []
    steps = np.arange(obs.shape[0], dtype=np.int64)
    z_all = R.policy_normal(seed, gid[None, :], (total0[None, :] + steps[:, None]).astype(np.uint32))     # [T, E, 2]: one Philox pass
    for t in range(obs.shape[0]):
        z = z_all[t]
        mean, a64, lp64, v64 = R.policy_step(P, obs[t], z)
        np.testing.assert_allclose(act[t], a64, rtol=1e-5, atol=1e-5, err_msg=f"actions, step {t}")
        np.testing.assert_allclose(lp[t], lp64, rtol=1e-5, atol=1e-5, err_msg=f"logprobs, step {t}")
        np.testing.assert_allclose(val[t], v64, rtol=1e-5, atol=1e-5, err_msg=f"values, step {t}")
        z_dev = (act[t] - mean) / sd
        np.testing.assert_allclose(z_dev, z, rtol=2e-6, atol=2e-6, err_msg=f"z, step {t}")
        zs.append(z_dev)
    nv = ro["next_value"].cpu().double().numpy()
    np.testing.assert_allclose(nv, R.value(P, ro["next_obs"].cpu().double().numpy()), rtol=1e-5, atol=1e-5)
    return np.concatenate(zs).reshape(-1)


def replay_env_side(ea, twin, ro, obs0, T, what):
    """2. the twin steps with the recorded actions: the env side must be bit for bit the policy rollout's"""
    import torch
    from evacuation_amd.vector_env import stats_int_view
    b = base(twin)
    obs = obs0.clone()
    done = torch.zeros(b.num_envs, dtype=torch.float32, device=b.device)
    n_done = 0
    for t in range(T):
        at = f"{what}, step {t}"
        assert i32(ro["obs"][t]).equal(i32(obs)), at
        assert ro["dones"][t].equal(done), at
        o, r, te, tr, info = twin.step(ro["actions"][t].clone())
        assert i32(ro["rewards"][t]).equal(i32(r)), at
        d = (te | tr).bool()
        if d.any():
            n_done += int(d.sum())
            assert i32(info["episode_stats"][d]).equal(i32(ro["episode_stats"][t][d])), at
            assert stats_int_view(info["episode_stats"][d]).equal(stats_int_view(ro["episode_stats"][t][d])), at
        obs = o.clone()
        done = d.float()
    assert i32(ro["next_obs"]).equal(i32(obs)), what
    assert ro["next_done"].equal(done), what
    return n_done


def teacher_forced_and_env_side_bit_for_bit(ea, case, E=64, T=40, seed=SEED, **cfg_over):
    """1. and 2. of one rollout of T steps.  Returns its storage and the twin's norm_state (or None)."""
    import torch
    # (the twin steps with the one-wave family the policy rollout runs for every N <= 64: the sub-wave step kernels of N <= 32
    # sum the exit distances of the intrinsic reward in another order, which may move episode_intrinsic_reward by an ulp)
    from evacuation_amd.options import KernelOptions
    a = make_env(ea, case, E, seed=seed, **cfg_over)
    b = make_env(ea, case, E, options=KernelOptions().replace(subwave=0), seed=seed, **cfg_over)
    D = base(a).obs_dim
    net = make_net(ea, D)
    obs_a, done_a = start(a)
    obs_b, _ = start(b)
    assert i32(obs_a).equal(i32(obs_b))
    if hasattr(a, "norm_state"):
        b.norm_state.copy_(a.norm_state)
    total0 = base(a).clock[:, 2].cpu().numpy().astype(np.int64)
    obs0 = obs_a.clone()
    ro = a.policy_rollout(net, T, obs_a, done_a)
    assert ro["next_obs"] is obs_a and ro["next_done"] is done_a
    n_done = replay_env_side(ea, b, ro, obs0, T, case)
    assert n_done >= E // 5                       # autoresets inside the call
    if hasattr(a, "norm_state"):
        assert i32(a.norm_state.view(torch.float32)).equal(i32(b.norm_state.view(torch.float32))), case
    sa, sb = base(a).get_state(), base(b).get_state()
    for k in sa:
        assert sa[k].view(torch.uint8).equal(sb[k].view(torch.uint8)), (case, k)
    assert base(a).clock.equal(base(b).clock) and i32(base(a).acc).equal(i32(base(b).acc)), case
    check_policy_outputs(ea, a, net, ro, total0, seed)
    out = {k: v.clone() for k, v in ro.items()}, (b.norm_state.clone() if hasattr(b, "norm_state") else None)
    a.close(); b.close()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_policy_rollout_teacher_forced_and_env_side_bit_for_bit(ea, case):
    teacher_forced_and_env_side_bit_for_bit(ea, case)


def test_policy_noise_is_standard_normal(ea):
    """>= 10^5 device draws (backed out of the actions): moments and the Kolmogorov-Smirnov statistic of N(0, 1)"""
    env = make_env(ea, "n60_grav_norm_clip", 1024)
    net = make_net(ea, 6)
    obs, done = start(env, near_trunc=0)
    total0 = base(env).clock[:, 2].cpu().numpy().astype(np.int64)
    ro = env.policy_rollout(net, 64, obs, done)
    z = np.sort(check_policy_outputs(ea, env, net, ro, total0))
    n = z.size
    assert n >= 100_000
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
    assert abs((z ** 3).mean()) < 0.03 and abs((z ** 4).mean() - 3.0) < 0.06
    cdf = 0.5 * (1.0 + np.vectorize(math.erf)(z / math.sqrt(2.0)))
    ks = max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(n) / n))
    assert ks < 1.63 / math.sqrt(n), ks           # the 1 % critical value
    env.close()


def _run(ea, case, E, T_split, options=None, net=None, **cfg_over):
    env = make_env(ea, case, E, options=options, **cfg_over)
    net = net or make_net(ea, base(env).obs_dim)
    obs, done = start(env)
    outs = [env.policy_rollout(net, T, obs, done) for T in T_split]
    fin = snapshot(env)
    env.close()
    return outs, fin


PER_STEP = ("obs", "actions", "logprobs", "values", "rewards", "dones", "episode_stats")


def assert_split_equals_one(one, f1, parts, f2, what):
    """The storage of one call against that of split calls joined along the step axis, the last call's next_* and the two final
    snapshots (norm_state among them), bit for bit."""
    import torch
    for k in PER_STEP:
        assert i32(one[k]).equal(i32(torch.cat([p[k] for p in parts]))), (what, k)
    for k in ("next_obs", "next_done", "next_value"):
        assert i32(one[k]).equal(i32(parts[-1][k])), (what, k)
    assert set(f1) == set(f2)
    for k in f1:
        assert raw(f1[k]).equal(raw(f2[k])), (what, k)


def test_split_calls_equal_one_call(ea):
    for case in ("n60_grav_norm_clip", "n32_abs_cat_dict_norm"):
        (one,), f1 = _run(ea, case, 48, [33])
        parts, f2 = _run(ea, case, 48, [7, 26])
        assert_split_equals_one(one, f1, parts, f2, case)


@pytest.mark.parametrize("case,opts", [
    ("n60_grav_norm_clip", dict(cu_wide=0)), ("n60_grav_norm_clip", dict(cu_wide=1)), ("n60_grav_norm_clip", dict(specialize=0)),
    ("n60_rel_ohe_box_norm_clip", dict(specialize=0)), ("n32_abs_cat_dict_norm", dict(subwave=0)),
    ("n10_grav_raw", dict(subwave=0)), ("n60_grav_norm_clip", dict(parts=2)), ("n60_grav_norm_clip", dict(chain=1)),
    ("n64_grav_wallterm_noise_raw", dict(parts=2)), ("n64_grav_wallterm_noise_raw", dict(chain=1)),
])
def test_options_and_forms_give_the_same_bits(ea, case, opts):
    from evacuation_amd.options import KernelOptions
    E = 64
    ref, fref = _run(ea, case, E, [12, 9])
    alt, falt = _run(ea, case, E, [12, 9], options=KernelOptions().replace(**opts))
    for r, a in zip(ref, alt):
        assert_same(r, a, (case, opts))
    for k in fref:
        assert raw(fref[k]).equal(raw(falt[k])), (case, opts, k)


def test_errors(ea):
    import torch
    from evacuation_amd import _lib
    from evacuation_amd.policy import LinearActorCritic
    env = ea.BatchedEvacuationEnv(ea.EnvConfig(number_of_pedestrians=65), ea.EnvWrappersConfig(positions="grav"), num_envs=16)
    obs, _ = env.reset()
    done = torch.zeros(16, device=env.device)
    net = make_net(ea, 6)
    with pytest.raises(NotImplementedError):
        env.policy_rollout(net, 4, obs, done)
    from evacuation_amd.policy import PolicyBinder
    st = PolicyBinder(6, env.device)(net)
    bufs = [torch.zeros(4 * 16 * 8, device=env.device) for _ in range(8)]
    ptr = [C.c_void_p(t.data_ptr()) for t in bufs]
    args = [ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ptr[6], ptr[7], ptr[0], None, None, 0.99, 1.0, 100.0, 1e-8, None]
    assert env.lib.evac_policy_rollout(env._h, 4, C.byref(st), *args) == _lib.ERR_UNSUPPORTED
    env.close()

    env = make_env(ea, "n60_grav_norm_clip", 16)
    obs, done = start(env, near_trunc=0)
    with pytest.raises(ValueError, match="hidden width 32"):
        env.policy_rollout(LinearActorCritic(6, hidden=32).cuda(), 4, obs, done)
    with pytest.raises(ValueError, match="observation dim"):
        env.policy_rollout(make_net(ea, 7), 4, obs, done)
    with pytest.raises(ValueError):
        env.policy_rollout(net, 4, obs[:, :5].contiguous(), done)
    h, lib = env.env._h, env.lib
    st = PolicyBinder(6, env.env.device)(net)
    args = [ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ptr[6], ptr[7], ptr[0], None, None, 0.99, 1.0, 100.0, 1e-8, None]
    for k in range(9):                                        # each buffer NULL in turn
        bad = list(args)
        bad[k] = None
        assert lib.evac_policy_rollout(h, 4, C.byref(st), *bad) == _lib.ERR_INVALID_ARGUMENT, k
    assert lib.evac_policy_rollout(h, 4, None, *args) == _lib.ERR_INVALID_ARGUMENT
    for field, value in (("critic_b2", None), ("hidden", 32), ("obs_dim", 7)):
        s2 = _lib.EvacMlpPolicy.from_buffer_copy(st)
        setattr(s2, field, value)
        assert lib.evac_policy_rollout(h, 4, C.byref(s2), *args) == _lib.ERR_INVALID_ARGUMENT, field
    assert lib.evac_policy_rollout(h, 0, C.byref(st), *args) == _lib.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    env.close()


def test_captured_call_reads_the_weights_in_place(ea):
    import torch
    env = make_env(ea, "n60_grav_norm_clip", 64)
    net = make_net(ea, 6)
    obs, done = start(env)
    out = env.policy_rollout(net, 8, obs, done)              # warm-up, allocates `out`
    torch.cuda.synchronize()
    s0, o0, d0 = snapshot(env), obs.clone(), done.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            env.policy_rollout(net, 8, obs, done, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    restore(env, s0); obs.copy_(o0); done.copy_(d0)
    g.replay()
    torch.cuda.synchronize()
    old_actions = out["actions"].clone()
    with torch.no_grad():                                     # an optimiser step: in place
        for prm in net.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    restore(env, s0); obs.copy_(o0); done.copy_(d0)
    out["episode_stats"].zero_()                              # (records are written only where an episode ended)
    g.replay()
    torch.cuda.synchronize()
    replayed = {k: v.clone() for k, v in out.items()}
    after = snapshot(env)
    restore(env, s0); obs.copy_(o0); done.copy_(d0)
    direct = env.policy_rollout(net, 8, obs, done)
    torch.cuda.synchronize()
    assert_same(replayed, direct, "graph replay vs direct call")
    fin = snapshot(env)
    for k in fin:
        assert raw(fin[k]).equal(raw(after[k])), k
    assert not torch.equal(old_actions, replayed["actions"])     # the replay did use the new weights
    env.close()
