"""Population evaluation (evac_policy_evaluate_population, BatchedEvacuationEnv.policy_evaluate_population, PopulationEvaluator,
PopulationTrainer.evaluate) on an MI355X: every learner's whole episodes in one launch, each BIT FOR BIT the learner alone.

1. / 2. Learner s's columns == evac_policy_evaluate of nets[s] on a handle of E_l envs, with shared ids (the handle's offset) and
with the collection's ids (offset + s E_l); sample mode with max_steps = T == policy_rollout_population(T).  3. Edge geometry.
4. max_steps = 17 repeated == one call; a finished batch; the sentinel.  5. Refusals.  6. PopulationEvaluator.
7. PopulationTrainer.evaluate / learn(eval_every).  8. Capture.

Equal means: the bytes of the state, of `progress` and of the records."""
import ctypes as C

import pytest

from tests import evaluation_cases as EC
from tests.evaluation_cases import CASES, OFFSET, SEED, i32, raw

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


def make_population(ea, D, S):
    from tests.test_gpu_population import make_population as make
    return make(ea, D, [11 + 7 * s for s in range(S)])


def raw_env_at(ea, case, E, offset, **cfg_over):
    """EC.make_raw_env with an env_id_offset of the caller's."""
    from evacuation_amd.options import KernelOptions
    cfg_kw, wrap_kw, _ = CASES[case]
    return ea.BatchedEvacuationEnv(ea.EnvConfig(**{**cfg_kw, **cfg_over}), ea.EnvWrappersConfig(**wrap_kw), num_envs=E, seed=SEED,
                                   env_id_offset=offset, options=KernelOptions().replace(subwave=0))


def start(ea, case, S, E_l, **cfg_over):
    """The population's handle, reset, with clocks spread over the WHOLE batch so that episodes end early."""
    env = EC.make_raw_env(ea, case, S * E_l, **cfg_over)
    env.reset()
    EC.spread_clocks(env)
    return env


def norm_rows(env, seed=5):
    """Frozen statistics that differ per env (so per learner too): [E, 3 D + 4] float64 on the device."""
    import torch
    E, D = env.num_envs, env.obs_dim
    g = torch.Generator().manual_seed(seed)
    ns = torch.zeros((E, 3 * D + 4), dtype=torch.float64)
    ns[:, :D] = torch.randn((E, D), generator=g, dtype=torch.float64) * 0.1
    ns[:, D:2 * D] = torch.rand((E, D), generator=g, dtype=torch.float64) + 0.05
    return ns.to(env.device)


def learner_alone(ea, case, pop, s, E_l, state0, shared, K, T, deterministic, ns, **cfg_over):
    """evac_policy_evaluate of learner s on a handle of E_l envs: the same seed, env_id_offset = OFFSET (+ s E_l when the ids are
    not shared), the state of the learner's share, its rows of norm_state.  Returns (progress, records, final state)."""
    import torch
    cols = slice(s * E_l, (s + 1) * E_l)
    twin = raw_env_at(ea, case, E_l, OFFSET + (0 if shared else s * E_l), **cfg_over)
    twin.reset()
    for k in EC.STATE:
        getattr(twin, k).copy_(state0[k][cols])
    norm = None if ns is None else (ns[cols].contiguous(), 1.0, 1e-8)
    progress, rec = twin.policy_evaluate(pop.nets[s], K, T, deterministic=deterministic, _norm=norm)
    torch.cuda.synchronize()
    fin = EC.state_of(twin)
    twin.close()
    return progress, rec, fin


def assert_learners_alone(ea, case, S, E_l, shared, deterministic, frozen, K=2, T=4096, **cfg_over):
    """One population call against S calls of the one-learner entry.  Returns (progress, records) of the population call."""
    import torch
    env = start(ea, case, S, E_l, **cfg_over)
    pop = make_population(ea, env.obs_dim, S)
    ns = norm_rows(env) if frozen else None
    ns0 = None if ns is None else ns.clone()
    state0 = EC.state_of(env)
    progress, rec = env.policy_evaluate_population(pop, K, T, deterministic=deterministic, shared_episodes=shared,
                                                   _norm=None if ns is None else (ns, 1.0, 1e-8))
    torch.cuda.synchronize()
    assert tuple(progress.shape) == (S * E_l, 4) and tuple(rec.shape) == (K, S * E_l, 10)
    fin = EC.state_of(env)
    for s in range(S):
        cols = slice(s * E_l, (s + 1) * E_l)
        p1, r1, f1 = learner_alone(ea, case, pop, s, E_l, state0, shared, K, T, deterministic, ns, **cfg_over)
        what = (case, S, E_l, s, shared, deterministic)
        assert raw(progress[cols]).equal(raw(p1)), what
        assert raw(rec[:, cols]).equal(raw(r1)), what
        for k in EC.STATE:
            assert raw(fin[k][cols]).equal(raw(f1[k])), (what, k)
    if ns is not None:
        assert raw(ns).equal(raw(ns0))                            # frozen: only read
    env.close()
    return progress, rec


FROZEN = {"n60_grav_norm_clip": True, "n32_abs_cat_dict_norm": True, "n64_grav_wallterm_noise_raw": False}


# ------------------------------------------------------------------------------------------------ 1. / 2. each learner is the learner alone
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("mode", ["mean", "sample"])
@pytest.mark.parametrize("case", list(FROZEN))
def test_each_learner_is_the_learner_alone(ea, case, mode, shared):
    """S = 3, E_l = 20: two workgroups per learner, the second with four working waves.  Two whole episodes per env."""
    S, E_l = 3, 20
    progress, rec = assert_learners_alone(ea, case, S, E_l, shared, mode == "mean", FROZEN[case])
    assert progress[:, 0].eq(2).all() and progress[:, 2:].eq(0).all()
    # one learner's weights for all would pass the comparison above only if the learners were alike: they are not
    differ = [not raw(rec[:, :E_l]).equal(raw(rec[:, s * E_l:(s + 1) * E_l])) for s in range(1, S)]
    assert any(differ), (case, mode, shared)


def test_unshared_sample_mode_is_the_population_rollout(ea):
    """2. sample mode, max_steps = T, ids not shared: the env side of policy_rollout_population(T) on a twin population handle --
    the relation tests/test_gpu_policy_evaluate.py::test_evaluation_is_the_policy_rollout pins for one learner."""
    import torch
    case, S, E_l, T = "n64_grav_wallterm_noise_raw", 3, 20, 40
    a, b = start(ea, case, S, E_l), EC.make_raw_env(ea, case, S * E_l)
    b.reset()
    EC.set_state(b, EC.state_of(a))
    pop = make_population(ea, a.obs_dim, S)
    obs = b.observe().clone()
    done = torch.zeros(S * E_l, dtype=torch.float32, device=b.device)
    ro = b.policy_rollout_population(pop, T, obs, done)
    progress, rec = a.policy_evaluate_population(pop, T, T, deterministic=False, shared_episodes=False)
    torch.cuda.synchronize()
    EC.assert_state_equal(EC.state_of(a), EC.state_of(b), case)
    assert progress[:, 1].eq(T).all() and progress[:, 2:].eq(0).all()
    ended = torch.cat([ro["dones"][1:].bool(), ro["next_done"].bool()[None]], dim=0)        # [T, E]: an episode ended at step t
    assert int(ended.sum()) >= (S * E_l) // 5
    assert progress[:, 0].equal(ended.sum(0).to(torch.int32))
    for e in range(S * E_l):
        rows = ro["episode_stats"][ended[:, e], e]
        n = rows.shape[0]
        assert i32(rec[:n, e]).equal(i32(rows)), e
        assert i32(rec[n:, e]).eq(0).all(), e
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 3. edge geometry
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("S,E_l", [(5, 1), (2, 16), (3, 17), (1, 48)])
def test_edge_geometry(ea, S, E_l, shared):
    """(5, 1): 15 idle waves per workgroup; (2, 16): an exact fit; (3, 17): one env in a learner's second workgroup; (1, 48): one
    learner -- which is also evac_policy_evaluate on the SAME handle."""
    import torch
    case = "n60_grav_norm_clip"
    progress, rec = assert_learners_alone(ea, case, S, E_l, shared, True, True)
    assert progress[:, 0].eq(2).all()
    if S == 1:
        env = start(ea, case, 1, E_l)
        pop = make_population(ea, env.obs_dim, 1)
        p1, r1 = env.policy_evaluate(pop.nets[0], 2, 4096, _norm=(norm_rows(env), 1.0, 1e-8))
        torch.cuda.synchronize()
        assert raw(p1).equal(raw(progress)) and raw(r1).equal(raw(rec))
        env.close()


# ------------------------------------------------------------------------------------------------ 4. split calls, finished batch, sentinel
def test_split_calls_equal_one_call(ea):
    import torch
    case, S, E_l, K = "n60_grav_norm_clip", 3, 20, 2
    a, b = start(ea, case, S, E_l), EC.make_raw_env(ea, case, S * E_l)
    b.reset()
    EC.set_state(b, EC.state_of(a))
    pop = make_population(ea, a.obs_dim, S)
    norm = (norm_rows(a), 1.0, 1e-8)
    p1, r1 = a.policy_evaluate_population(pop, K, 100000, _norm=norm)
    assert p1[:, 0].eq(K).all()
    sentinel = 12345.0
    p2 = None
    r2 = torch.full((K, S * E_l, 10), sentinel, dtype=torch.float32, device=b.device)
    calls = 0
    while True:
        p2, r2 = b.policy_evaluate_population(pop, K, 17, p2, r2, _norm=norm)
        calls += 1
        assert calls < 1000
        n = p2[:, 0].long()
        if calls == 1:                                                # most envs have not finished: their later slots are untouched
            assert int(n.min()) < K and int(n.max()) >= 1 and p2[:, 1].le(17).all()
            for k in range(K):
                assert r2[k][n <= k].eq(sentinel).all(), k
                assert not r2[k][n > k].eq(sentinel).all(dim=1).any(), k
        if int(n.min()) >= K:
            break
    torch.cuda.synchronize()
    assert calls >= 2
    assert raw(p1).equal(raw(p2)) and raw(r1).equal(raw(r2))
    EC.assert_state_equal(EC.state_of(a), EC.state_of(b), case)
    before = EC.state_of(b)
    p3, r3 = b.policy_evaluate_population(pop, K, 50, p2.clone(), r2.clone(), _norm=norm)      # every env is done: nothing happens
    torch.cuda.synchronize()
    assert raw(p3).equal(raw(p2)) and raw(r3).equal(raw(r2))
    EC.assert_state_equal(before, EC.state_of(b), "a finished batch")
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_launch_nothing(ea):
    import torch
    from evacuation_amd import _lib
    from evacuation_amd.policy import DeepSetsActorCritic
    case = "n60_grav_norm_clip"
    env = start(ea, case, 2, 24)                                      # 48 envs
    lib, h = env.lib, env._h
    pop = make_population(ea, env.obs_dim, 2)
    pol, strides = pop.policy_struct(), pop.strides
    prog = torch.zeros((49, 4), dtype=torch.int32, device=env.device)
    out = torch.zeros((1, 48, 10), dtype=torch.float32, device=env.device)
    pp, po = C.c_void_p(prog.data_ptr()), C.c_void_p(out.data_ptr())
    before = EC.state_of(env)

    def call(handle, S, st, agent, p=pp):
        return lib.evac_policy_evaluate_population(handle, S, C.byref(pol), st, agent, 1, 1, 4, p, po, None, 1.0, 1e-8, None)
    bad = _lib.ERR_INVALID_ARGUMENT
    assert call(h, 0, C.byref(strides), 0) == bad and call(h, 65, C.byref(strides), 0) == bad
    assert call(h, 5, C.byref(strides), 0) == bad                      # 48 envs, 5 learners
    assert call(h, 2, None, 0) == bad                                 # NULL strides
    zero = _lib.EvacMlpPolicyStrides.from_buffer_copy(strides)
    zero.actor_w2 = 0
    assert call(h, 2, C.byref(zero), 0) == bad                         # a stride smaller than its tensor
    assert call(h, 2, C.byref(strides), _lib.AGENT_VACUUM_CLEANER) == bad
    assert call(h, 2, C.byref(strides), 3) == bad
    assert call(h, 2, C.byref(strides), 0, C.c_void_p(prog.data_ptr() + 4)) == bad      # misaligned progress
    env50 = EC.make_raw_env(ea, case, 50)
    env50.reset()
    assert call(env50._h, 3, C.byref(strides), 0) == bad              # 50 envs, 3 learners
    with pytest.raises(ValueError, match="equal shares"):
        env50.policy_evaluate_population(make_population(ea, env.obs_dim, 3), 1, 4)
    env50.close()
    with pytest.raises(ValueError):
        env.policy_evaluate_population("vacuum_cleaner", 1, 4)
    with pytest.raises(ValueError, match="deep_sets"):
        env.policy_evaluate_population(DeepSetsActorCritic(124, 60), 1, 4)
    with pytest.raises(ValueError):
        env.policy_evaluate_population(pop, 0, 4)
    with pytest.raises(ValueError):
        env.policy_evaluate_population(pop, 1, 4, prog[:8])
    torch.cuda.synchronize()
    EC.assert_state_equal(before, EC.state_of(env), "refused calls launch nothing")
    assert prog.eq(0).all() and out.eq(0).all()
    assert call(h, 2, C.byref(strides), 0) == 0                        # ... and the good call runs
    torch.cuda.synchronize()
    steps = prog[:48, 1]                                               # (one episode: the envs next to truncation stop after 1 or 2 steps)
    assert steps.ge(1).all() and steps.le(4).all() and int(steps.eq(4).sum()) >= 24 and prog[48].eq(0).all()
    env.close()


# ------------------------------------------------------------------------------------------------ 6. PopulationEvaluator
def test_population_evaluator(ea):
    import torch
    from evacuation_amd.evaluation import EvaluationResult, PopulationEvaluator
    S, E_l, K = 3, 20, 2
    cfg_kw, wrap_kw, _ = CASES["n60_grav_norm_clip"]
    cfg, wrap = ea.EnvConfig(**cfg_kw), ea.EnvWrappersConfig(**wrap_kw)
    ev = PopulationEvaluator(cfg, wrap, num_learners=S, num_envs=E_l, seed=SEED)
    assert ev.env.num_envs == S * E_l and ev.num_envs == E_l and ev.num_learners == S
    pop = make_population(ea, 6, S)
    g = torch.Generator().manual_seed(9)
    ns = torch.zeros((S, 7, 22), dtype=torch.float64)                 # 7 rows for 20 envs: row i mod 7, different per learner
    ns[:, :, :6] = torch.randn((S, 7, 6), generator=g, dtype=torch.float64) * 0.1
    ns[:, :, 6:12] = torch.rand((S, 7, 6), generator=g, dtype=torch.float64) + 0.05
    ns = ns.to(ev.env.device)
    first = ev.evaluate(pop, K, norm_state=ns, max_steps_per_launch=17)
    assert ev.launches >= 2 and len(first) == S
    first = [{k: v.clone() for k, v in res.episodes.items()} for res in first]
    again = ev.evaluate(pop, K, norm_state=list(ns.unbind(0)), max_steps_per_launch=17)       # the same start: the same bytes
    for s in range(S):
        for k in first[s]:
            assert raw(first[s][k]).equal(raw(again[s].episodes[k])), (s, k)
    one = ea.PolicyEvaluator(cfg, wrap, num_envs=E_l, seed=SEED)
    for s in range(S):
        res = one.evaluate(pop.nets[s], K, norm_state=ns[s])
        assert set(res.episodes) == set(again[s].episodes)
        for k in res.episodes:
            assert tuple(again[s].episodes[k].shape) == (K, E_l)
            assert raw(res.episodes[k]).equal(raw(again[s].episodes[k])), (s, k)
        assert res.steps.equal(again[s].steps) and res.n_pedestrians == again[s].n_pedestrians
    assert not raw(again[0].episodes["episode_reward"]).equal(raw(again[1].episodes["episode_reward"]))
    assert EvaluationResult.summaries(again) == [res.summary() for res in again]
    assert again[0].episodes["episode_reward"].untyped_storage().data_ptr() == \
        again[S - 1].episodes["episode_reward"].untyped_storage().data_ptr()          # views of ONE records tensor
    with pytest.raises(ValueError):
        ev.evaluate(make_population(ea, 6, 2), K)                     # a population of another size
    one.close()
    ev.close()


# ------------------------------------------------------------------------------------------------ 7. PopulationTrainer
def test_population_trainer_evaluates_in_one_set_of_launches(ea):
    import torch
    from tests.test_gpu_population import make_population_trainer
    S, E_l = 3, 8
    ptr = make_population_trainer(ea, S, E_l, 32, [4, 5, 6])
    ptr.update()
    assert ptr.population_evaluator is None
    results = ptr.evaluate(n_episodes=2)
    torch.cuda.synchronize()
    assert len(results) == S and ptr.population_evaluator is not None and ptr.population_evaluator.launches >= 1
    assert ptr.population_evaluator.num_envs == E_l and ptr.population_evaluator.num_learners == S
    assert ptr.evaluator is None                                      # the per-learner evaluator was not needed
    for res in results:
        assert tuple(res.episodes["episode_reward"].shape) == (2, E_l)
    logs = ptr.learn(total_timesteps=ptr.cfg.batch_size, eval_every=1)
    assert len(logs) == 1 and len(logs[0]) == S
    now = [res.summary() for res in ptr.evaluate(n_episodes=1)]       # the weights are those of learn()'s last update
    for s in range(S):
        assert logs[0][s]["eval"] == now[s], s
        assert now[s]["episodes"] == E_l and all(type(v) in (float, int) for v in now[s].values())
    ptr.population_evaluator.close()
    ptr.env.close()


# ------------------------------------------------------------------------------------------------ 8. capture
def test_captured_call_reads_the_stacked_weights_in_place(ea):
    """tests/test_gpu_population.py::test_captured_collection_reads_the_weights_in_place for the evaluation entry."""
    import torch
    S, E_l = 2, 8
    env = start(ea, "n60_grav_norm_clip", S, E_l)
    pop = make_population(ea, env.obs_dim, S)
    norm = (norm_rows(env), 1.0, 1e-8)
    s0 = EC.state_of(env)
    progress, out = env.policy_evaluate_population(pop, 8, 8, _norm=norm)           # warm-up, allocates
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            env.policy_evaluate_population(pop, 8, 8, progress, out, _norm=norm)
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
    with torch.no_grad():                                             # an optimiser step on the stacks: in place
        for t in pop.tensors:
            t.add_(0.05 * torch.randn_like(t))
    rewind()
    g.replay()
    torch.cuda.synchronize()
    replayed = (progress.clone(), out.clone(), EC.state_of(env))
    rewind()
    p, o = env.policy_evaluate_population(pop, 8, 8, progress, out, _norm=norm)
    torch.cuda.synchronize()
    assert raw(p).equal(raw(replayed[0])) and raw(o).equal(raw(replayed[1]))
    EC.assert_state_equal(EC.state_of(env), replayed[2], "graph replay vs direct call")
    for s in range(S):                                                # the replay did use every learner's new weights
        cols = slice(s * E_l, (s + 1) * E_l)
        assert not raw(old_state["agent"][cols]).equal(raw(replayed[2]["agent"][cols])), s
    assert int(p[:, 0].sum()) >= (S * E_l) // 5
    env.close()
