"""Evaluation of a population of deep-sets leaders (evac_policy_evaluate_population_deepsets, policy_evaluate_population and
PopulationEvaluator with a DeepSetsPopulation, PopulationTrainer.evaluate) on an MI355X: every learner's whole episodes in one
launch, each BIT FOR BIT the learner alone (evac_policy_evaluate_deepsets, which tests/test_gpu_deepsets.py holds to float64).

1. Learner s's columns == policy_evaluate(nets[s]) on a handle of E_l envs, shared ids and the collection's ids.  2. Unshared
sample mode with max_steps = T == policy_rollout_population(T).  3. Edge geometry.  4. max_steps = 17 repeated == one call; the
sentinel; a finished batch.  5. Past the first 64-step noise block.  6. The C entry's refusals: code and text, in their order.
7. The Python faces.  8. PopulationTrainer.evaluate / learn(eval_every).

Equal means: the bytes of the state, of `progress` and of the records.  No tolerance anywhere."""
import ctypes as C
from types import SimpleNamespace

import pytest

from tests import evaluation_cases as EC
from tests.evaluation_cases import OFFSET, SEED, i32, raw
from tests.test_gpu_deepsets_population import CASES, training_cfg, training_env, visible
from tests.trainer_cases import DEV

pytestmark = pytest.mark.gpu

NAME = "evac_policy_evaluate_population_deepsets"
N60, N10, N64 = "n60_rel_ohe_box_norm_clip", "n10_abs_cat_box_raw", "n64_rel_ohe_box_norm_clip"


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import evacuation_amd
    from evacuation_amd import build
    build.build_library()
    return evacuation_amd


def raw_env_at(ea, case, E, offset=OFFSET, **cfg_over):
    """The case's env WITHOUT the normalisation wrapper, as tests/evaluation_cases.make_raw_env builds it."""
    from evacuation_amd.options import KernelOptions
    cfg_kw, wrap_kw, _ = CASES[case]
    return ea.BatchedEvacuationEnv(ea.EnvConfig(**{**cfg_kw, **cfg_over}), ea.EnvWrappersConfig(**wrap_kw), num_envs=E, seed=SEED,
                                   env_id_offset=offset, options=KernelOptions().replace(subwave=0))


def start(ea, case, S, E_l, spread=True, **cfg_over):
    """The population's handle, reset, with clocks spread over the WHOLE batch so that episodes end early."""
    env = raw_env_at(ea, case, S * E_l, **cfg_over)
    env.reset()
    if spread:
        EC.spread_clocks(env)
    return env


def make_population(env, S):
    from evacuation_amd.population import DeepSetsPopulation
    return visible(DeepSetsPopulation(env.obs_dim, env.n_ped, [11 + 7 * s for s in range(S)], DEV))


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
    """evac_policy_evaluate_deepsets of learner s on a handle of E_l envs: the same seed, env_id_offset = OFFSET (+ s E_l when the
    ids are not shared), the state of the learner's share, its rows of norm_state.  Returns (progress, records, final state)."""
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


def assert_learners_alone(ea, case, S, E_l, shared, deterministic, K=2, T=4096, spread=True, **cfg_over):
    """One population call against S calls of the one-learner entry.  Returns (progress, records) of the population call."""
    import torch
    env = start(ea, case, S, E_l, spread, **cfg_over)
    pop = make_population(env, S)
    ns = norm_rows(env) if CASES[case][2] else None
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


# ------------------------------------------------------------------------------------------------ 1. each learner is the learner alone
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("mode", ["mean", "sample"])
@pytest.mark.parametrize("case", [N60, N10, N64])
def test_each_learner_is_the_learner_alone(ea, case, mode, shared):
    """S = 3, E_l = 20: two workgroups per learner, the second with four working waves.  Two whole episodes per env."""
    S, E_l = 3, 20
    progress, rec = assert_learners_alone(ea, case, S, E_l, shared, mode == "mean")
    assert progress[:, 0].eq(2).all() and progress[:, 2:].eq(0).all()
    # one learner's weights for all would pass the comparison above only if the learners were alike: they are not
    differ = [not raw(rec[:, :E_l]).equal(raw(rec[:, s * E_l:(s + 1) * E_l])) for s in range(1, S)]
    assert any(differ), (case, mode, shared)


# ------------------------------------------------------------------------------------------------ 2. the population rollout
def test_unshared_sample_mode_is_the_population_rollout(ea):
    """Sample mode, max_steps = T, ids not shared: the env side of policy_rollout_population(T) on a twin population handle."""
    import torch
    case, S, E_l, T = N10, 3, 20, 40
    a, b = start(ea, case, S, E_l), raw_env_at(ea, case, S * E_l)
    b.reset()
    EC.set_state(b, EC.state_of(a))
    pop = make_population(a, S)
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
    learner -- which is also evac_policy_evaluate_deepsets on the SAME handle."""
    import torch
    case = N60
    progress, rec = assert_learners_alone(ea, case, S, E_l, shared, True)
    assert progress[:, 0].eq(2).all()
    if S == 1:
        env = start(ea, case, 1, E_l)
        pop = make_population(env, 1)
        p1, r1 = env.policy_evaluate(pop.nets[0], 2, 4096, _norm=(norm_rows(env), 1.0, 1e-8))
        torch.cuda.synchronize()
        assert raw(p1).equal(raw(progress)) and raw(r1).equal(raw(rec))
        env.close()


# ------------------------------------------------------------------------------------------------ 4. split calls, sentinel, finished batch
def test_split_calls_equal_one_call(ea):
    import torch
    case, S, E_l, K = N60, 3, 20, 2
    a, b = start(ea, case, S, E_l), raw_env_at(ea, case, S * E_l)
    b.reset()
    EC.set_state(b, EC.state_of(a))
    pop = make_population(a, S)
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


# ------------------------------------------------------------------------------------------------ 5. past the first noise block
def test_sample_mode_past_the_first_64_step_noise_block(ea):
    """Sample mode draws its z in blocks of 64 steps of a LAUNCH: three episodes of max_timesteps = 25 in one launch take an env
    that starts fresh to 75 steps, into the second block, whoever the learner is."""
    progress, rec = assert_learners_alone(ea, N60, 3, 20, True, False, K=3)
    assert progress[:, 0].eq(3).all()
    assert int(progress[:, 1].max()) > 64


# ------------------------------------------------------------------------------------------------ 6. the C entry's refusals
STRIDES_TEXT = ": an encoder stride is smaller than its tensor, or rho_w's is no multiple of 4 floats"
POLICY_STRIDE_TEXT = ": a learner stride is smaller than its tensor"
NULL_STRIDES_TEXT = ": strides / enc_strides is NULL"


def evaluate(lib, h, a):
    """The entry on handle `h` with the arguments `a` (Handle.valid, spoiled): its return code."""
    ref = lambda s: None if s is None else C.byref(s)
    return getattr(lib, NAME)(h, a["n_learners"], ref(a["policy"]), ref(a["strides"]), ref(a["encoder"]), ref(a["enc_strides"]),
                              a["agent"], a.get("shared", 1), a["n_episodes"], a["max_steps"], a["progress"], a["episodes_out"],
                              a["norm_state"], 1.0, 1e-8, None)


def test_entry_refusals_have_their_code_and_text_in_their_order_and_enqueue_nothing(ea):
    """tests/test_gpu_policy_refusals.py's table for the new entry, through ctypes on reset handles: the return code and the text
    of evac_last_error of every case, as literals; double faults pin the order -- unbound, NULL strides, the scripted agent, an
    unknown agent, the counts and buffers, the two networks, the learners, the one-wave limit.  Box rel + ohe at E = 4, N = 3
    (D = 30, six floats an element) and E = 1, N = 65.  What one learner cannot break -- its strides are never applied -- is accepted at
    S = 1: such a call is shown to pass the strides' check by the refusal behind it (the one-wave limit, on the N = 65 handle)."""
    import torch
    from evacuation_amd import _lib
    from evacuation_amd.config import to_c_config
    from evacuation_amd.population import DeepSetsPopulation
    from tests.test_gpu_policy_refusals import (BAD, COUNTS_TEXT, LEARNERS_TEXT, PROGRESS_TEXT, ROOMS_TEXT, SCRIPTED, SCRIPTED_TEXT,
                                                UNSUPPORTED, Handle, changed)
    box_wrap = dict(positions="rel", statuses="ohe", type="Box")
    box, big = Handle(ea, 3, box_wrap, 4, 6), Handle(ea, 65, box_wrap, 1, 6)
    D, ed = 30, 6
    assert box.env.obs_dim == D and big.env.obs_dim == 402
    least = dict(phi_w1=24 * ed, phi_b1=24, phi_w2=24 * 24, phi_b2=24, rho_w=D * 24, rho_b=D)
    fields = [f for f, _ in _lib.EvacDeepSetsStrides._fields_]
    assert fields == list(least)
    box.valid["enc_strides"] = _lib.EvacDeepSetsStrides(*least.values())
    big.valid["enc_strides"] = _lib.EvacDeepSetsStrides(*{**least, "rho_w": 402 * 24, "rho_b": 402}.values())
    zero = _lib.EvacDeepSetsStrides(0, 0, 0, 0, 2, 0)                # every stride 0, rho_w's neither a tensor nor a multiple of 4
    no_strides = _lib.EvacMlpPolicyStrides()
    rows = [  # (what, handle, the changes, code, the text after the entry's name)
        # NULL strides: first behind the handle
        ("strides NULL", box, lambda v: dict(strides=None), BAD, NULL_STRIDES_TEXT),
        ("enc_strides NULL", box, lambda v: dict(enc_strides=None), BAD, NULL_STRIDES_TEXT),
        ("enc_strides NULL, one learner", box, lambda v: dict(enc_strides=None, n_learners=1), BAD, NULL_STRIDES_TEXT),
        ("strides NULL and the scripted agent", box, lambda v: dict(strides=None, agent=SCRIPTED), BAD, NULL_STRIDES_TEXT),
        ("N = 65 and enc_strides NULL", big, lambda v: dict(enc_strides=None), BAD, NULL_STRIDES_TEXT),
        # the agent
        ("the scripted agent", box, lambda v: dict(agent=SCRIPTED), BAD, SCRIPTED_TEXT),
        ("the scripted agent and progress NULL", box, lambda v: dict(agent=SCRIPTED, progress=None), BAD, SCRIPTED_TEXT),
        ("the scripted agent and encoder NULL", box, lambda v: dict(agent=SCRIPTED, encoder=None, policy=None), BAD, SCRIPTED_TEXT),
        ("agent 7", box, lambda v: dict(agent=7), BAD, ": unknown agent 7"),
        ("agent 7 and n_episodes = 0", box, lambda v: dict(agent=7, n_episodes=0), BAD, ": unknown agent 7"),
        # evaluate_check's
        ("progress NULL", box, lambda v: dict(progress=None), BAD, PROGRESS_TEXT),
        ("episodes_out NULL", box, lambda v: dict(episodes_out=None), BAD, PROGRESS_TEXT),
        ("n_episodes = 0", box, lambda v: dict(n_episodes=0), BAD, COUNTS_TEXT),
        ("max_steps = 0", box, lambda v: dict(max_steps=0), BAD, COUNTS_TEXT),
        ("progress + 4 bytes", box, lambda v: dict(progress=v["progress"] + 4), BAD, ": progress must be 16-byte aligned"),
        ("progress NULL and policy NULL", box, lambda v: dict(progress=None, policy=None), BAD, PROGRESS_TEXT),
        ("N = 65 and n_episodes = 0", big, lambda v: dict(n_episodes=0), BAD, COUNTS_TEXT),
        # the two networks'
        ("policy NULL", box, lambda v: dict(policy=None), BAD, ": policy is NULL"),
        ("encoder NULL", box, lambda v: dict(encoder=None), BAD, ": encoder is NULL"),
        ("policy NULL and encoder NULL", box, lambda v: dict(policy=None, encoder=None), BAD, ": policy is NULL"),
        ("policy.actor_w1 NULL", box, lambda v: dict(policy=changed(v["policy"], "actor_w1", None)), BAD,
         ": a tensor pointer of the policy is NULL"),
        ("hidden = 32", box, lambda v: dict(policy=changed(v["policy"], "hidden", 32)), BAD, ": hidden must be 64"),
        ("obs_dim off by one", box, lambda v: dict(policy=changed(v["policy"], "obs_dim", 31)), BAD, ": policy obs_dim 31 != evac_obs_dim 30"),
        ("encoder.rho_b NULL", box, lambda v: dict(encoder=changed(v["encoder"], "rho_b", None)), BAD,
         ": a tensor pointer of the encoder is NULL"),
        ("encoder hidden = 16", box, lambda v: dict(encoder=changed(v["encoder"], "hidden", 16)), BAD, ": the encoder's hidden must be 24"),
        ("set_elem_dim = 5", box, lambda v: dict(encoder=changed(v["encoder"], "set_elem_dim", 5)), BAD,
         ": set_elem_dim 5 x (3 + 2) elements is not the observation's 30 floats (a Box observation is needed)"),
        ("rho_w + 4 bytes", box, lambda v: dict(encoder=changed(v["encoder"], "rho_w", v["encoder"].rho_w + 4)), BAD,
         ": rho_w must be 16-byte aligned"),
        ("encoder NULL and n_learners = 0", box, lambda v: dict(encoder=None, n_learners=0), BAD, ": encoder is NULL"),
        # the learners'
        ("n_learners = 0", box, lambda v: dict(n_learners=0), BAD, LEARNERS_TEXT),
        ("n_learners = EVAC_MAX_LEARNERS + 1", box, lambda v: dict(n_learners=65), BAD, LEARNERS_TEXT),
        ("3 learners on 4 envs", box, lambda v: dict(n_learners=3), BAD, ": the handle's 4 envs are not 3 learners' equal shares"),
        ("a policy stride smaller than the tensor, 2 learners", box, lambda v: dict(strides=changed(v["strides"], "critic_b3", 0)), BAD,
         POLICY_STRIDE_TEXT),
        ("a policy stride and an encoder stride, 2 learners", box,
         lambda v: dict(strides=changed(v["strides"], "actor_w1", 64 * D - 1), enc_strides=zero), BAD, POLICY_STRIDE_TEXT),
        ("rho_w stride + 2", box, lambda v: dict(enc_strides=changed(v["enc_strides"], "rho_w", least["rho_w"] + 2)), BAD, STRIDES_TEXT),
        ("every encoder stride 0, 2 learners", box, lambda v: dict(enc_strides=zero), BAD, STRIDES_TEXT),
        ("N = 65 and n_learners = 0", big, lambda v: dict(n_learners=0), BAD, LEARNERS_TEXT),
        ("N = 65 and 2 learners on 1 env", big, lambda v: dict(n_learners=2), BAD, ": the handle's 1 envs are not 2 learners' equal shares"),
        # last, the one-wave limit -- and the strides that ONE learner cannot break are accepted: the call gets to the check behind them
        ("N = 65", big, lambda v: {}, UNSUPPORTED, ROOMS_TEXT),
        ("N = 65, every encoder stride 0, 1 learner", big, lambda v: dict(enc_strides=zero), UNSUPPORTED, ROOMS_TEXT),
        ("N = 65, every policy stride 0 too, 1 learner", big, lambda v: dict(enc_strides=zero, strides=no_strides), UNSUPPORTED, ROOMS_TEXT),
    ]
    for f in fields:                                                 # each of the six, one below its tensor and 0, with 2 learners
        for value in (least[f] - 1, 0):
            rows.append((f"encoder stride {f} = {value}, 2 learners", box,
                         lambda v, f=f, value=value: dict(enc_strides=changed(v["enc_strides"], f, value)), BAD, STRIDES_TEXT))
    torch.cuda.synchronize()
    before = {id(hd): hd.snapshot() for hd in (box, big)}
    lib = box.env.lib
    # a handle whose state is not bound: refused before the strides are looked at
    c = to_c_config(ea.EnvConfig(number_of_pedestrians=3), ea.EnvWrappersConfig(**box_wrap))
    unbound = C.c_void_p()
    assert lib.evac_create(C.byref(c), 4, 0, 0, 0, C.byref(unbound)) == 0 and unbound.value
    for spoil in ({}, dict(strides=None), dict(agent=SCRIPTED)):
        rc = evaluate(lib, unbound, {**box.valid, **spoil})
        assert (rc, lib.evac_last_error(unbound).decode()) == (_lib.ERR_NOT_BOUND, NAME + ": call evac_bind_state first"), spoil
    lib.evac_destroy(unbound)
    for what, hd, spoil, code, text in rows:
        args = {**hd.valid, **spoil(hd.valid)}
        rc = evaluate(lib, hd.env._h, args)
        got = (lib.evac_last_error(hd.env._h) or b"").decode()
        assert rc != 0, what                                          # (a call that went through: stop before anything else is tried)
        assert (rc, got) == (code, NAME + text), what
    assert len(rows) == 40 + 12
    torch.cuda.synchronize()
    for hd in (box, big):
        for k, t in hd.snapshot().items():
            assert torch.equal(t, before[id(hd)][k]), k
        assert hd.progress.eq(0).all() and hd.records.eq(0).all()
    # ... and a good call runs: two real learners on the box handle's four envs, two steps each
    pop = visible(DeepSetsPopulation(D, 3, [1, 2], DEV))
    good = {**box.valid, "policy": pop.policy_struct(), "strides": pop.strides, "encoder": pop.encoder_struct(),
            "enc_strides": pop.encoder_strides}
    assert evaluate(lib, box.env._h, good) == 0
    torch.cuda.synchronize()
    assert box.progress[:, 1].eq(2).all() and box.progress[:, 0].eq(0).all()
    for hd in (box, big):
        hd.env.close()


# ------------------------------------------------------------------------------------------------ 7. the Python faces
def test_population_evaluator_and_the_python_refusals(ea):
    import torch
    from evacuation_amd.evaluation import PopulationEvaluator
    from evacuation_amd.policy import DeepSetsActorCritic, TransformerActorCritic
    from evacuation_amd.population import DeepSetsPopulation
    from tests.test_gpu_population import make_population as make_linear
    S, E_l, K = 3, 20, 2
    cfg_kw, wrap_kw, _ = CASES[N10]
    cfg, wrap = ea.EnvConfig(**cfg_kw), ea.EnvWrappersConfig(**wrap_kw)
    ev = PopulationEvaluator(cfg, wrap, num_learners=S, num_envs=E_l, seed=SEED)
    env = ev.env
    D, N = env.obs_dim, env.n_ped
    assert env.num_envs == S * E_l and N == 10
    g = torch.Generator().manual_seed(9)
    ns = torch.zeros((S, 7, 3 * D + 4), dtype=torch.float64)          # 7 rows for 20 envs: row i mod 7, different per learner
    ns[:, :, :D] = torch.randn((S, 7, D), generator=g, dtype=torch.float64) * 0.1
    ns[:, :, D:2 * D] = torch.rand((S, 7, D), generator=g, dtype=torch.float64) + 0.05
    ns = ns.to(env.device)
    one = ea.PolicyEvaluator(cfg, wrap, num_envs=E_l, seed=SEED)
    pops = {"deep_sets": visible(DeepSetsPopulation(D, N, [11 + 7 * s for s in range(S)], DEV)),
            "linear": make_linear(ea, D, [11 + 7 * s for s in range(S)])}        # (a PolicyPopulation on the same evaluator still works)
    for kind, pop in pops.items():
        results = ev.evaluate(pop, K, norm_state=ns, max_steps_per_launch=17)
        assert ev.launches >= 2 and len(results) == S
        for s in range(S):
            res = one.evaluate(pop.nets[s], K, norm_state=ns[s])
            assert set(res.episodes) == set(results[s].episodes)
            for k in res.episodes:
                assert tuple(results[s].episodes[k].shape) == (K, E_l)
                assert raw(res.episodes[k]).equal(raw(results[s].episodes[k])), (kind, s, k)
            assert res.steps.equal(results[s].steps) and res.n_pedestrians == results[s].n_pedestrians
        assert not raw(results[0].episodes["episode_reward"]).equal(raw(results[1].episodes["episode_reward"])), kind
    one.close()
    # what stays refused, with its message
    pop = pops["deep_sets"]
    bare, tf = DeepSetsActorCritic(D, N).to(DEV), TransformerActorCritic(D, N).to(DEV)
    two = DeepSetsPopulation(D, N, [1, 2], DEV)
    ev.restore()                                                      # (an evaluate() that gets as far as its launch restores first)
    before = EC.state_of(env)
    for call in (lambda: ev.evaluate(bare, 1), lambda: env.policy_evaluate_population(bare, 1, 4),
                 # set-encoder nets in an object that has no encoder strides
                 lambda: env.policy_evaluate_population(SimpleNamespace(num_learners=S, nets=pop.nets, strides=pop.strides), 1, 4)):
        with pytest.raises(ValueError, match="`deep_sets`"):
            call()
    shaped = SimpleNamespace(num_learners=S, nets=[tf] * S, strides=pop.strides, encoder_strides=pop.encoder_strides)
    for call in (lambda: ev.evaluate(tf, 1), lambda: ev.evaluate(shaped, 1), lambda: env.policy_evaluate_population(shaped, 1, 4)):
        with pytest.raises(ValueError, match="attention encoder"):
            call()
    with pytest.raises(ValueError, match="a capture cannot be given"):
        env.policy_evaluate_population(pop, 1, 4, capture={"frames": None, "starts": None})
    with pytest.raises(ValueError, match="a PolicyPopulation is expected"):
        env.policy_evaluate_population("vacuum_cleaner", 1, 4)
    with pytest.raises(ValueError, match="the population has 2 learners, the evaluator 3"):
        ev.evaluate(two, 1)
    env50 = raw_env_at(ea, N10, 50)
    env50.reset()
    with pytest.raises(ValueError, match="50 envs are not 3 learners' equal shares"):
        env50.policy_evaluate_population(pop, 1, 4)
    env50.close()
    torch.cuda.synchronize()
    EC.assert_state_equal(before, EC.state_of(env), "refused calls launch nothing")
    ev.close()


# ------------------------------------------------------------------------------------------------ 8. the trainer
def test_population_trainer_evaluates_in_one_set_of_launches(ea):
    """DESIGN.md 8.1's measurement decided for the one-launch path: evaluate() makes the population evaluator and leaves the
    per-learner one alone; the results are the per-learner loop's bit for bit."""
    import torch
    from evacuation_amd.population import DeepSetsPopulation, PopulationTrainer
    S, E_l, T, seeds = 3, 4, 16, [11, 18, 25]
    cfg = training_cfg(E_l, T, 0)
    env = training_env(ea, S * E_l, OFFSET, cfg.gamma)
    ptr = PopulationTrainer(env, DeepSetsPopulation(env.obs_dim, 10, seeds, DEV), cfg)
    assert ptr.deepsets
    ptr.update()
    assert ptr.population_evaluator is None and ptr.evaluator is None
    results = ptr.evaluate(1)
    torch.cuda.synchronize()
    assert len(results) == S and ptr.population_evaluator is not None and ptr.population_evaluator.launches >= 1
    assert ptr.population_evaluator.num_envs == E_l and ptr.population_evaluator.num_learners == S
    assert ptr.evaluator is None                                      # the per-learner evaluator was not needed
    ev = ptr.make_evaluator()
    assert ev.num_envs == E_l
    for s in range(S):
        with torch.no_grad():
            one = ev.evaluate(ptr.nets[s], 1, norm_state=ptr.env.norm_state[s * E_l:(s + 1) * E_l].clone(), obs_clip=ptr.env.obs_clip,
                              epsilon=ptr.env.epsilon)
        for k in one.episodes:
            assert raw(one.episodes[k]).equal(raw(results[s].episodes[k])), (s, k)
        assert one.steps.equal(results[s].steps) and results[s].summary()["episodes"] == E_l
    assert not raw(results[0].episodes["episode_reward"]).equal(raw(results[1].episodes["episode_reward"]))
    logs = ptr.learn(total_timesteps=ptr.cfg.batch_size, eval_every=1)
    assert len(logs) == 1 and len(logs[0]) == S
    now = [res.summary() for res in ptr.evaluate(1)]                  # the weights are those of learn()'s last update
    for s in range(S):
        assert logs[0][s]["eval"] == now[s], s
        assert now[s]["episodes"] == E_l and all(type(v) in (float, int) for v in now[s].values())
    ptr.evaluator.close()
    ptr.population_evaluator.close()
    ptr.env.close()
