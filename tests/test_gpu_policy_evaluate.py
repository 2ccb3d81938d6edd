"""The policy evaluation (evac_policy_evaluate, BatchedEvacuationEnv / NormalizedVectorEnv.policy_evaluate, PolicyEvaluator,
RPOTrainer.evaluate) on an MI355X.

1. Sample mode is the policy rollout, bit for bit (state and episode records).  2. Mean mode is the policy rollout with sigma = 0.
3. Episode bookkeeping.  4. max_steps = 17 repeated == one call.  5. / 6. The frozen normaliser: exact (power-of-two scalings) and
general (float64 restatement, teacher-forced).  7. The scripted baseline against host WacuumCleaner objects driving step().
8. PolicyEvaluator: every evaluation from the same start.  9. RPOTrainer.evaluate / learn(eval_every).  10. Errors.  11. Capture."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import evaluation_cases as EC
from tests.evaluation_cases import CASES, OFFSET, SEED, base, i32, make_net, raw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import evacuation_amd
    from evacuation_amd import build
    build.build_library()
    return evacuation_amd


def twins(ea, case, E, **cfg_over):
    """Two raw handles of the case with the same seed, offset and start state (some envs close to truncation)."""
    a, b = EC.make_raw_env(ea, case, E, **cfg_over), EC.make_raw_env(ea, case, E, **cfg_over)
    a.reset()
    b.reset()
    EC.spread_clocks(a)
    EC.set_state(b, EC.state_of(a))
    return a, b


def evaluation_is_the_policy_rollout(ea, case, mode, E=64, T=40, **cfg_over):
    """policy_evaluate(max_steps = T, n_episodes large) against policy_rollout(T) on a twin handle -- in mean mode with the twin's
    actor_logstd at -inf (expf gives 0 exactly, so mu + 0 z = mu).  Returns the rollout's [T, E] episode ends."""
    import torch
    a, b = twins(ea, case, E, **cfg_over)
    net = make_net(ea, a.obs_dim)
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
    EC.assert_state_equal(EC.state_of(a), EC.state_of(b), (case, mode))
    assert progress[:, 1].eq(T).all() and progress[:, 2:].eq(0).all()
    ended = torch.cat([ro["dones"][1:].bool(), ro["next_done"].bool()[None]], dim=0)        # [T, E]: an episode ended at step t
    assert int(ended.sum()) >= E // 5
    assert progress[:, 0].equal(ended.sum(0).to(torch.int32))
    for e in range(E):
        rows = ro["episode_stats"][ended[:, e], e]
        n = rows.shape[0]
        assert i32(rec[:n, e]).equal(i32(rows)), (case, mode, e)
        assert i32(rec[n:, e]).eq(0).all(), (case, mode, e)
    a.close(); b.close()
    return ended.cpu().numpy()


@pytest.mark.parametrize("mode", ["sample", "mean"])
@pytest.mark.parametrize("case", list(CASES))
def test_evaluation_is_the_policy_rollout(ea, case, mode):
    """1. / 2."""
    evaluation_is_the_policy_rollout(ea, case, mode)


def test_episode_bookkeeping(ea):
    """3."""
    import torch
    from evacuation_amd.vector_env import STATS_FIELDS, stats_int_view
    for case in ("n60_grav_norm_clip", "n32_abs_cat_dict_norm"):
        env = EC.make_raw_env(ea, case, 48)
        env.reset()
        EC.spread_clocks(env)
        total0 = env.clock[:, 2].clone()
        net = make_net(ea, env.obs_dim)
        out = torch.full((3, 48, 10), 12345.0, dtype=torch.float32, device=env.device)
        progress, out = env.policy_evaluate(net, 3, 10, None, out)        # a first, short call: most envs have not finished
        n = progress[:, 0].long()
        assert int(n.min()) < 3 and int(n.max()) >= 1 and progress[:, 1].eq(10).all()
        for k in range(3):                                                # record slots beyond an env's count are untouched
            assert out[k][n <= k].eq(12345.0).all(), (case, k)
            assert not out[k][n > k].eq(12345.0).all(dim=1).any(), (case, k)
        progress, out = env.policy_evaluate(net, 3, 4096, progress, out)
        assert progress[:, 0].eq(3).all()
        ints = stats_int_view(out)
        ot, ne = ints[..., 0], ints[..., 1]
        length = out[..., STATS_FIELDS.index("episode_length")]
        assert (ne[1] == ne[0] + 1).all() and (ne[2] == ne[0] + 2).all(), case
        assert (length <= env.env_config.max_timesteps).all() and (length >= 1).all(), case
        assert (ot[1] - ot[0]).float().equal(length[1]) and (ot[2] - ot[1]).float().equal(length[2]), case
        assert (ot[2] - total0).equal(progress[:, 1]), case               # steps taken = what the env's clock advanced by
        assert env.clock[:, 2].equal(ot[2]) and env.clock[:, 0].eq(0).all() and env.clock[:, 1].equal(ne[2] + 1), case
        before = EC.state_of(env)
        p2, o2 = env.policy_evaluate(net, 3, 50, progress.clone(), out.clone())       # every env is done: the call does nothing
        torch.cuda.synchronize()
        assert p2.equal(progress) and raw(o2).equal(raw(out))
        EC.assert_state_equal(before, EC.state_of(env), case)
        env.close()


@pytest.mark.parametrize("case,agent,frozen", [
    ("n60_grav_norm_clip", "net", True), ("n60_rel_ohe_box_norm_clip", "net", False), ("n64_grav_wallterm_noise_raw", "net_sample", False),
    ("n60_grav_norm_clip", "vacuum_cleaner", False), ("n32_abs_cat_dict_norm", "vacuum_cleaner", False),
])
def test_split_calls_equal_one_call(ea, case, agent, frozen):
    """4. max_steps = 17 repeated until every env is done == one long call: records, progress and final state as bytes"""
    import torch
    E = 48
    a, b = twins(ea, case, E)
    kw, who = {}, agent
    if agent != "vacuum_cleaner":
        who = EC.eval_net(ea, a.obs_dim)
        kw["deterministic"] = agent == "net"
        if frozen:
            g = torch.Generator().manual_seed(5)
            W = 3 * a.obs_dim + 4
            ns = torch.zeros((E, W), dtype=torch.float64)
            ns[:, :a.obs_dim] = torch.randn((E, a.obs_dim), generator=g, dtype=torch.float64) * 0.1
            ns[:, a.obs_dim:2 * a.obs_dim] = torch.rand((E, a.obs_dim), generator=g, dtype=torch.float64) + 0.05
            kw["_norm"] = (ns.to(a.device), 1.0, 1e-8)
    p1, r1, c1 = EC.run_until_done(a, who, 2, 100000, **kw)
    p2, r2, c2 = EC.run_until_done(b, who, 2, 17, **kw)
    torch.cuda.synchronize()
    assert c1 == 1 and c2 >= 2
    assert p1.equal(p2) and raw(r1).equal(raw(r2)), (case, agent)
    EC.assert_state_equal(EC.state_of(a), EC.state_of(b), (case, agent))
    assert p1[:, 0].eq(2).all() and p1[:, 2:].eq(0).all()        # (a scripted agent's words are cleared by the last autoreset)
    a.close(); b.close()


@pytest.mark.parametrize("case", ["n60_rel_ohe_box_norm_clip", "n60_grav_norm_clip", "n32_abs_cat_dict_norm"])
def test_frozen_normaliser_exact(ea, case):
    """5. mean 0, var_j = 4^k_j - eps (so sqrt(var_j + eps) = 2^k_j exactly), a huge clip, and W1's column j scaled by 2^k_j:
    byte-equal to the raw evaluation of the unscaled network; norm_state is only read."""
    import torch
    E, eps = 48, 1e-8
    a, b = twins(ea, case, E)
    D = a.obs_dim
    net = EC.eval_net(ea, D)
    k = torch.tensor([(3 * j + 1) % 7 - 3 for j in range(D)], dtype=torch.float64)           # -3 .. 3, different per feature
    var = 4.0 ** k - eps
    assert (torch.sqrt(var + eps) == 2.0 ** k).all() and ((var + eps) == 4.0 ** k).all()
    ns = torch.zeros((E, 3 * D + 4), dtype=torch.float64)
    ns[:, D:2 * D] = var
    ns[:, 2 * D:] = 7.0                                                                       # (counts: never read)
    ns = ns.to(a.device)
    ns0 = ns.clone()
    scaled = copy.deepcopy(net)
    with torch.no_grad():
        scaled.actor_mean[0].weight.mul_((2.0 ** k).float().to(a.device)[None, :])
    p1, r1, _ = EC.run_until_done(a, net, 2, 4096)
    p2, r2, _ = EC.run_until_done(b, scaled, 2, 4096, _norm=(ns, 1e30, eps))
    torch.cuda.synchronize()
    assert p1.equal(p2) and raw(r1).equal(raw(r2)), case
    EC.assert_state_equal(EC.state_of(a), EC.state_of(b), case)
    assert raw(ns).equal(raw(ns0))
    a.close(); b.close()


@pytest.mark.parametrize("case", ["n60_grav_norm_clip", "n60_rel_ohe_box_norm_clip", "n32_abs_cat_dict_norm", "n64_abs_ohe_box_norm"])
def test_frozen_normaliser_general(ea, case):
    """6. a NormalizedVectorEnv whose statistics have moved; max_steps = 1 calls, each checked against the float64 restatement:
    observe() (raw) -> the frozen formula -> tests/policy_ref.actor_mean -> the oracle's agent_step.  The leader's new position
    within 2e-4 x step_size: check_policy_outputs' 1e-5 on the action, carried through the normalisation of an action of norm
    >= 0.1 (shorter actions are left out: at most 5 % of the envs)."""
    import torch
    from oracle import evac_oracle as O
    from tests import policy_ref as R
    from tests.test_gpu_policy_rollout import make_env, start
    E = 64
    env = make_env(ea, case, E)
    b = base(env)
    D = b.obs_dim
    net = EC.eval_net(ea, D)
    obs, done = start(env, near_trunc=0)
    env.policy_rollout(net, 40, obs, done)                      # the statistics move
    ns_before = env.norm_state.clone()
    ns = env.norm_state.cpu().numpy()
    mean, var = ns[:, :D], ns[:, D:2 * D]
    assert np.abs(mean).max() > 1e-3
    P = R.params64(net)
    cfg = b.env_config
    op = O.OracleParams(number_of_pedestrians=cfg.number_of_pedestrians, width=cfg.width, height=cfg.height, step_size=cfg.step_size,
                        eps=cfg.eps, is_termination_agent_wall_collision=cfg.is_termination_agent_wall_collision)
    progress = out = None
    left_out = checked = 0
    for call in range(6):
        x = b.observe().cpu().double().numpy()
        xn = np.clip((x - mean) / np.sqrt(var + env.epsilon), -env.obs_clip, env.obs_clip)
        act = R.actor_mean(P, xn)
        pos0 = b.agent[:, :2].cpu().numpy().copy()
        n0 = None if progress is None else progress[:, 0].clone()
        progress, out = env.policy_evaluate(net, 1000, 1, progress, out)
        ended = (progress[:, 0] - (0 if n0 is None else n0)).bool().cpu().numpy()
        pos1 = b.agent[:, :2].cpu().numpy()
        for e in range(E):
            if ended[e]:                                        # (the env was reset: the leader is back at the origin)
                continue
            if np.linalg.norm(act[e]) < 0.1:
                left_out += 1
                continue
            a = act[e]
            if cfg.clip_action:
                a = np.clip(a, -1.0, 1.0)
            st = O.OracleState(pos=np.zeros((1, 2), np.float32), dir=np.zeros((1, 2), np.float32), status=np.ones(1, np.int8),
                               agent_pos=pos0[e].astype(np.float32), agent_dir=np.zeros(2, np.float32))
            O.agent_step(op, st, a.astype(np.float32))
            err = np.abs(st.agent_pos.astype(np.float64) - pos1[e].astype(np.float64)).max()
            assert err <= 2e-4 * cfg.step_size, (case, call, e, err)
            checked += 1
    share = left_out / max(1, left_out + checked)
    print(f"{case}: {checked} steps checked, {left_out} left out (action shorter than 0.1): share {share:.4f}")
    assert share <= 0.05 and checked >= 5 * E
    assert raw(env.norm_state).equal(raw(ns_before))            # frozen: only read
    env.close()


@pytest.mark.parametrize("cfg_kw,wrap_kw", [
    (dict(number_of_pedestrians=60, is_new_exiting_reward=True, clip_action=True), dict(positions="grav", alpha=3)),
    (dict(number_of_pedestrians=20, width=0.7, height=1.3, step_size=0.03), dict(positions="abs", statuses="cat")),
])
def test_scripted_baseline_against_host_agents(ea, cfg_kw, wrap_kw):
    """7. 16 envs, one whole episode each at the default max_timesteps: the device agent against a twin handle stepped with step()
    from sixteen host WacuumCleaner objects, each fresh per episode and reading agent[:, :2]."""
    import torch
    from evacuation_amd.options import KernelOptions
    E = 16
    mk = lambda: ea.BatchedEvacuationEnv(ea.EnvConfig(**cfg_kw), ea.EnvWrappersConfig(**wrap_kw), num_envs=E, seed=SEED,       # noqa: E731
                                         env_id_offset=OFFSET, options=KernelOptions().replace(subwave=0))
    a, b = mk(), mk()
    a.reset()
    b.reset()
    assert a.env_config.max_timesteps == 2000
    progress, rec, calls = EC.run_until_done(a, "vacuum_cleaner", 1, 4096)
    torch.cuda.synchronize()
    assert calls == 1 and progress[:, 0].eq(1).all() and progress[:, 2:].eq(0).all()
    fake = EC.fake_env(a.env_config.width, a.env_config.height, a.env_config.step_size)
    agents = [ea.WacuumCleaner(fake) for _ in range(E)]
    final, records, steps = {}, {}, {}
    phases = set()
    actions = torch.zeros((E, 2), dtype=torch.float32, device=b.device)
    for t in range(1, 2001):
        pos = b.agent[:, :2].cpu().numpy()
        act = np.stack([agents[e].act({"agent_position": pos[e]}) for e in range(E)])
        phases.update(ag.phase for ag in agents)
        actions.copy_(torch.from_numpy(act))
        _, _, te, tr, info = b.step(actions)
        d = (te | tr).bool().cpu().numpy()
        for e in np.nonzero(d)[0]:
            if e not in final:                                  # the env's FIRST episode: its record and the state after the autoreset
                records[e] = info["episode_stats"][e].clone()
                final[e] = {k: getattr(b, k)[e].clone() for k in EC.STATE}
                steps[e] = t
            agents[e] = ea.WacuumCleaner(fake)                  # fresh per episode
        if len(final) == E:
            break
    assert len(final) == E
    for e in range(E):
        assert i32(rec[0, e]).equal(i32(records[e])), e
        assert int(progress[e, 1]) == steps[e], e
        for k in EC.STATE:
            assert raw(getattr(a, k)[e]).equal(raw(final[e][k])), (e, k)
    assert {0, 1} <= phases
    a.close(); b.close()


def test_policy_evaluator_same_start_for_everybody(ea):
    """8."""
    import torch
    cfg_kw, wrap_kw, _ = CASES["n60_grav_norm_clip"]
    ev = ea.PolicyEvaluator(ea.EnvConfig(**cfg_kw), ea.EnvWrappersConfig(**wrap_kw), num_envs=48, seed=SEED)
    snap = {k: v.clone() for k, v in ev.snapshot.items()}
    net = EC.eval_net(ea, 6)
    W = 3 * 6 + 4
    ns = torch.zeros((5, W), dtype=torch.float64, device=ev.env.device)              # 5 rows for 48 envs: row e mod 5
    ns[:, 6:12] = torch.arange(1, 6, dtype=torch.float64, device=ev.env.device)[:, None]
    results = {}
    for name, agent, kw in (("net", net, {}), ("net again", net, {}), ("norm", net, dict(norm_state=ns)),
                            ("baseline", "vacuum_cleaner", {}), ("baseline again", "vacuum_cleaner", {})):
        res = ev.evaluate(agent, 2, max_steps_per_launch=17, **kw)
        assert ev.launches >= 2
        results[name] = res
        e = res.episodes
        assert tuple(e["episode_reward"].shape) == (2, 48)
        # the first episode started from the snapshot: its reset count, and the clock it started at
        assert e["n_episodes"][0].equal(snap["clock"][:, 1]), name
        assert (e["overall_timesteps"][0] - snap["clock"][:, 2]).float().equal(e["episode_length"][0]), name
        assert res.steps.equal(e["overall_timesteps"][1] - snap["clock"][:, 2]), name
        s = res.summary()
        assert s["episodes"] == 96 and 1 <= s["episode_length_mean"] <= 25 and 0.0 <= s["escaped_fraction_mean"] <= 1.0
    for k in snap:
        assert raw(ev.snapshot[k]).equal(raw(snap[k]))
    for x, y in (("net", "net again"), ("baseline", "baseline again")):
        for k in results[x].episodes:
            assert raw(results[x].episodes[k]).equal(raw(results[y].episodes[k])), (x, k)
    assert not results["net"].episodes["episode_reward"].equal(results["baseline"].episodes["episode_reward"])
    assert not results["net"].episodes["episode_reward"].equal(results["norm"].episodes["episode_reward"])
    # row e mod rows: the evaluation with the five rows expanded by hand gives the same bits
    ev.restore()
    rows = ns[torch.arange(48, device=ns.device) % 5].contiguous()
    p, r, _ = EC.run_until_done(ev.env, net, 2, 4096, _norm=(rows, 1.0, 1e-8))
    assert raw(r[..., 0]).equal(raw(results["norm"].episodes["episode_reward"]))
    ev.close()


def test_trainer_evaluate_leaves_training_untouched(ea):
    """9."""
    import torch
    from evacuation_amd.policy import LinearActorCritic
    from evacuation_amd.trainer import RPOTrainer, RPOTrainingConfig
    E, T = 64, 16
    cfg = RPOTrainingConfig(num_envs=E, num_steps=T, total_timesteps=E * T * 3, num_minibatches=4, update_epochs=2, seed=1)
    env = ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=60, max_timesteps=25, is_new_exiting_reward=True),
                                      ea.EnvWrappersConfig(positions="grav", alpha=3), num_envs=E, gamma=cfg.gamma, seed=1)
    torch.manual_seed(0)
    net = LinearActorCritic(env.obs_dim).to(env.env.device)
    tr = RPOTrainer(env, net, cfg)
    tr.update()
    torch.cuda.synchronize()
    before = EC.state_of(env)
    keep = {"next_obs": tr.next_obs.clone(), "next_done": tr.next_done.clone(), "norm_state": env.norm_state.clone(),
            "generator": tr.generator.get_state().clone(), "params": [p.detach().clone() for p in net.parameters()]}
    res = tr.evaluate(n_episodes=2, num_envs=32)
    torch.cuda.synchronize()
    assert tuple(res.episodes["episode_reward"].shape) == (2, 32) and res.summary()["episodes"] == 64
    res_det = tr.evaluate(n_episodes=2, num_envs=32)
    assert raw(res_det.episodes["episode_reward"]).equal(raw(res.episodes["episode_reward"]))
    res_smp = tr.evaluate(n_episodes=2, num_envs=32, deterministic=False)
    assert not res_smp.episodes["episode_reward"].equal(res.episodes["episode_reward"])
    torch.cuda.synchronize()
    EC.assert_state_equal(before, EC.state_of(env), "training env")
    assert raw(tr.next_obs).equal(raw(keep["next_obs"])) and raw(tr.next_done).equal(raw(keep["next_done"]))
    assert raw(env.norm_state).equal(raw(keep["norm_state"]))
    assert tr.generator.get_state().equal(keep["generator"])
    assert all(raw(p.detach()).equal(raw(q)) for p, q in zip(net.parameters(), keep["params"]))
    logs = tr.learn(total_timesteps=2 * cfg.batch_size, eval_every=1, eval_episodes=1)
    assert len(logs) == 2
    for log in logs:
        s = log["eval"]
        assert s["episodes"] == E and all(type(v) in (float, int) for v in s.values())
        assert {"episode_reward_mean", "episode_reward_std", "episode_length_mean", "escaped_fraction_mean", "all_escaped_share"} <= set(s)
    assert "eval" not in tr.learn(total_timesteps=cfg.batch_size)[0]
    tr.evaluator.close()
    env.close()


def test_errors(ea):
    """10."""
    import torch
    from evacuation_amd import _lib
    from evacuation_amd.policy import LinearActorCritic, PolicyBinder
    env = ea.BatchedEvacuationEnv(ea.EnvConfig(number_of_pedestrians=65), ea.EnvWrappersConfig(positions="grav"), num_envs=16)
    env.reset()
    net = make_net(ea, 6)
    for agent in (net, "vacuum_cleaner"):
        with pytest.raises(NotImplementedError):
            env.policy_evaluate(agent, 1, 4)
    st = PolicyBinder(6, env.device)(net)
    prog = torch.zeros((16, 4), dtype=torch.int32, device=env.device)
    out = torch.zeros((1, 16, 10), dtype=torch.float32, device=env.device)
    pp, po = C.c_void_p(prog.data_ptr()), C.c_void_p(out.data_ptr())
    assert env.lib.evac_policy_evaluate(env._h, 0, C.byref(st), 1, 4, pp, po, None, 1.0, 1e-8, None) == _lib.ERR_UNSUPPORTED
    assert env.lib.evac_policy_evaluate(env._h, 2, None, 1, 4, pp, po, None, 1.0, 1e-8, None) == _lib.ERR_UNSUPPORTED
    env.close()

    env = EC.make_raw_env(ea, "n60_grav_norm_clip", 16)
    env.reset()
    with pytest.raises(ValueError, match="hidden width 32"):
        env.policy_evaluate(LinearActorCritic(6, hidden=32).cuda(), 1, 4)
    with pytest.raises(ValueError, match="observation dim"):
        env.policy_evaluate(make_net(ea, 7), 1, 4)
    with pytest.raises(ValueError):
        env.policy_evaluate("rotating", 1, 4)
    with pytest.raises(ValueError):
        env.policy_evaluate(net, 0, 4)
    with pytest.raises(ValueError):
        env.policy_evaluate(net, 1, 0)
    with pytest.raises(ValueError):
        env.policy_evaluate(net, 1, 4, prog[:8])
    with pytest.raises(ValueError):
        env.policy_evaluate("vacuum_cleaner", 1, 4, _norm=(torch.zeros((16, 22), dtype=torch.float64, device=env.device), 1.0, 1e-8))
    h, lib = env._h, env.lib
    ns = torch.zeros((16, 22), dtype=torch.float64, device=env.device)
    pn = C.c_void_p(ns.data_ptr())
    before = EC.state_of(env)
    call = lambda agent, pol, n, t, p, o, s: lib.evac_policy_evaluate(h, agent, pol, n, t, p, o, s, 1.0, 1e-8, None)     # noqa: E731
    assert call(3, C.byref(st), 1, 4, pp, po, None) == _lib.ERR_INVALID_ARGUMENT
    assert call(-1, C.byref(st), 1, 4, pp, po, None) == _lib.ERR_INVALID_ARGUMENT
    assert call(0, C.byref(st), 1, 4, None, po, None) == _lib.ERR_INVALID_ARGUMENT
    assert call(0, C.byref(st), 1, 4, pp, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert call(0, C.byref(st), 0, 4, pp, po, None) == _lib.ERR_INVALID_ARGUMENT
    assert call(0, C.byref(st), 1, 0, pp, po, None) == _lib.ERR_INVALID_ARGUMENT
    assert call(0, None, 1, 4, pp, po, None) == _lib.ERR_INVALID_ARGUMENT
    assert call(1, None, 1, 4, pp, po, None) == _lib.ERR_INVALID_ARGUMENT
    assert call(2, None, 1, 4, pp, po, pn) == _lib.ERR_INVALID_ARGUMENT
    for field, value in (("actor_b2", None), ("hidden", 32), ("obs_dim", 7)):
        s2 = _lib.EvacMlpPolicy.from_buffer_copy(st)
        setattr(s2, field, value)
        assert call(0, C.byref(s2), 1, 4, pp, po, None) == _lib.ERR_INVALID_ARGUMENT, field
    torch.cuda.synchronize()
    EC.assert_state_equal(before, EC.state_of(env), "refused calls launch nothing")
    assert prog.eq(0).all() and out.eq(0).all()
    assert call(2, None, 1, 4, pp, po, None) == 0 and call(0, C.byref(st), 1, 4, pp, po, pn) == 0
    torch.cuda.synchronize()
    assert prog[:, 1].eq(8).all()
    env.close()


def test_captured_call_reads_the_weights_in_place(ea):
    """11."""
    import torch
    from tests.test_gpu_policy_rollout import make_env
    env = make_env(ea, "n60_grav_norm_clip", 64)
    b = base(env)
    net = EC.eval_net(ea, 6)
    obs, _ = env.reset()
    env.policy_rollout(net, 8, obs.clone(), torch.zeros(64, device=b.device))      # the statistics move
    EC.spread_clocks(env)                                                           # episodes end inside the captured call
    torch.cuda.synchronize()
    s0 = EC.state_of(env)
    progress, out = env.policy_evaluate(net, 8, 8)                                  # warm-up, allocates
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            env.policy_evaluate(net, 8, 8, progress, out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    def rewind():
        EC.set_state(env, s0)
        progress.zero_()
        out.zero_()
    rewind()
    g.replay()
    torch.cuda.synchronize()
    old_state = EC.state_of(env)
    with torch.no_grad():                                     # an optimiser step: in place
        for prm in net.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    rewind()
    g.replay()
    torch.cuda.synchronize()
    replayed = (progress.clone(), out.clone(), EC.state_of(env))
    rewind()
    p, o = env.policy_evaluate(net, 8, 8, progress, out)
    torch.cuda.synchronize()
    assert p.equal(replayed[0]) and raw(o).equal(raw(replayed[1]))
    EC.assert_state_equal(EC.state_of(env), replayed[2], "graph replay vs direct call")
    assert not raw(old_state["agent"]).equal(raw(replayed[2]["agent"]))           # the replay did use the new weights
    assert int(p[:, 0].sum()) >= 64 // 5
    env.close()
