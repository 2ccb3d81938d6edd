"""Evaluation of a population of transformer leaders (evac_policy_evaluate_population_transformer; policy_evaluate_population and
PopulationEvaluator with a TransformerPopulation) on an MI355X: every learner's whole episodes in one launch, each BIT FOR BIT the
learner alone (evac_policy_evaluate_transformer, which tests/test_gpu_transformer.py holds to the float64 restatement).

1. Learner s's columns == policy_evaluate(nets[s]) on a handle of E_l envs: both agents, shared ids and the collection's ids,
   frozen per-env statistics, the four geometries of tests/test_gpu_transformer_population.py.
2. Unshared sample mode with max_steps = T == the env side of policy_rollout_population(T).
3. max_steps = 17 repeated == one call; the records' sentinel; a finished batch does nothing.
4. The Python faces: PopulationEvaluator, what stays refused, and that refused calls touch nothing.
5. The C entry's refusals: code and text, in their order, nothing enqueued; what is accepted runs.

Equal means: the bytes of the state, of `progress` and of the records.  No tolerance anywhere."""
import ctypes as C
from types import SimpleNamespace

import pytest

from tests import evaluation_cases as EC
from tests import test_gpu_transformer as TF
from tests.encoder_cases import ea  # noqa: F401 (the fixture)
from tests.evaluation_cases import OFFSET, SEED, i32, raw
from tests.test_gpu_transformer_population import (ENC_STRIDE_TEXT, GEOMETRIES, N10, N62, NULL_STRIDES_TEXT, all_strides, block_least,
                                                    encoder_strides, make_env, make_population, merged, stride_changed)
from tests.trainer_cases import DEV

pytestmark = pytest.mark.gpu

NAME = "evac_policy_evaluate_population_transformer"


def raw_env_at(ea, case, E, offset=OFFSET, **cfg_over):
    """The case's env WITHOUT the normalisation wrapper, on the one-wave step kernels (as tests/evaluation_cases.make_raw_env)."""
    return make_env(ea, case, E, offset, raw_env=True, options=dict(subwave=0), **cfg_over)


def start(ea, case, S, E_l, **cfg_over):
    """The population's handle, reset, with clocks spread over the WHOLE batch so that episodes end early."""
    env = raw_env_at(ea, case, S * E_l, **cfg_over)
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


def learner_alone(ea, case, pop, s, E_l, state0, shared, K, T, deterministic, ns):
    """evac_policy_evaluate_transformer of learner s on a handle of E_l envs: the same seed, env_id_offset = OFFSET (+ s E_l when
    the ids are not shared), the state of the learner's share, its rows of norm_state.  Returns (progress, records, final state)."""
    import torch
    cols = slice(s * E_l, (s + 1) * E_l)
    twin = raw_env_at(ea, case, E_l, OFFSET + (0 if shared else s * E_l))
    twin.reset()
    for k in EC.STATE:
        getattr(twin, k).copy_(state0[k][cols])
    norm = None if ns is None else (ns[cols].contiguous(), 1.0, 1e-8)
    progress, rec = twin.policy_evaluate(pop.nets[s], K, T, deterministic=deterministic, _norm=norm)
    torch.cuda.synchronize()
    fin = EC.state_of(twin)
    twin.close()
    return progress, rec, fin


def assert_learners_alone(ea, case, S, E_l, shared, deterministic, K=2, T=4096):
    """One population call against S calls of the one-learner entry.  Returns (progress, records) of the population call."""
    import torch
    env = start(ea, case, S, E_l)
    pop = make_population(env, case, S)
    ns = norm_rows(env) if TF.CASES[case][2] else None
    ns0 = None if ns is None else ns.clone()
    state0 = EC.state_of(env)
    progress, rec = env.policy_evaluate_population(pop, K, T, deterministic=deterministic, shared_episodes=shared,
                                                   _norm=None if ns is None else (ns, 1.0, 1e-8))
    torch.cuda.synchronize()
    assert tuple(progress.shape) == (S * E_l, 4) and tuple(rec.shape) == (K, S * E_l, 10)
    fin = EC.state_of(env)
    for s in range(S):
        cols = slice(s * E_l, (s + 1) * E_l)
        p1, r1, f1 = learner_alone(ea, case, pop, s, E_l, state0, shared, K, T, deterministic, ns)
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
@pytest.mark.parametrize("case,S,E_l", GEOMETRIES)
def test_each_learner_is_the_learner_alone(ea, case, S, E_l, mode, shared):
    """1.  Two whole episodes per env."""
    progress, rec = assert_learners_alone(ea, case, S, E_l, shared, mode == "mean")
    assert progress[:, 0].eq(2).all() and progress[:, 2:].eq(0).all()
    # one learner's weights for all would pass the comparison above only if the learners were alike: they are not
    differ = [not raw(rec[:, :E_l]).equal(raw(rec[:, s * E_l:(s + 1) * E_l])) for s in range(1, S)]
    assert any(differ), (case, mode, shared)


# ------------------------------------------------------------------------------------------------ 2. the population rollout
def test_unshared_sample_mode_is_the_population_rollout(ea):
    """2.  Sample mode, max_steps = T, ids not shared: the env side of policy_rollout_population(T) on a twin population handle."""
    import torch
    case, S, E_l, T = N10, 2, 17, 40
    a, b = start(ea, case, S, E_l), raw_env_at(ea, case, S * E_l)
    b.reset()
    EC.set_state(b, EC.state_of(a))
    pop = make_population(a, case, S)
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


# ------------------------------------------------------------------------------------------------ 3. split calls, sentinel, finished batch
def test_split_calls_equal_one_call(ea):
    import torch
    case, S, E_l, K = N62, 3, 5, 2
    a, b = start(ea, case, S, E_l), raw_env_at(ea, case, S * E_l)
    b.reset()
    EC.set_state(b, EC.state_of(a))
    pop = make_population(a, case, S)
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


# ------------------------------------------------------------------------------------------------ 4. the Python faces
def test_population_evaluator_and_the_python_refusals(ea):
    import torch
    from evacuation_amd.evaluation import PopulationEvaluator
    from evacuation_amd.policy import TransformerActorCritic
    from evacuation_amd.population import PopulationAdam, PopulationTrainer, TransformerPopulation
    from evacuation_amd.trainer import RPOTrainingConfig
    S, E_l, K = 3, 6, 2
    cfg_kw, wrap_kw = TF.CASES[N10][:2]
    cfg, wrap = ea.EnvConfig(**cfg_kw), ea.EnvWrappersConfig(**wrap_kw)
    ev = PopulationEvaluator(cfg, wrap, num_learners=S, num_envs=E_l, seed=SEED)
    env = ev.env
    D, N = env.obs_dim, env.n_ped
    assert env.num_envs == S * E_l and N == 10
    g = torch.Generator().manual_seed(9)
    ns = torch.zeros((S, 4, 3 * D + 4), dtype=torch.float64)          # 4 rows for 6 envs: row i mod 4, different per learner
    ns[:, :, :D] = torch.randn((S, 4, D), generator=g, dtype=torch.float64) * 0.1
    ns[:, :, D:2 * D] = torch.rand((S, 4, D), generator=g, dtype=torch.float64) + 0.05
    ns = ns.to(env.device)
    one = ea.PolicyEvaluator(cfg, wrap, num_envs=E_l, seed=SEED)
    pop = make_population(env, N10, S)
    for deterministic in (True, False):
        results = ev.evaluate(pop, K, norm_state=ns, max_steps_per_launch=17, deterministic=deterministic)
        assert ev.launches >= 2 and len(results) == S
        for s in range(S):
            res = one.evaluate(pop.nets[s], K, norm_state=ns[s], deterministic=deterministic)
            assert set(res.episodes) == set(results[s].episodes)
            for k in res.episodes:
                assert tuple(results[s].episodes[k].shape) == (K, E_l)
                assert raw(res.episodes[k]).equal(raw(results[s].episodes[k])), (deterministic, s, k)
            assert res.steps.equal(results[s].steps) and res.n_pedestrians == results[s].n_pedestrians
        assert not raw(results[0].episodes["episode_reward"]).equal(raw(results[1].episodes["episode_reward"])), deterministic
    one.close()
    # what stays refused, with its message; nothing of it touches the handle's state
    tf = TransformerActorCritic(D, N, num_blocks=1).to(DEV)
    two = TransformerPopulation(D, N, [1, 2], DEV, num_blocks=1)
    ev.restore()                                                      # (an evaluate() that gets as far as its launch restores first)
    before = EC.state_of(env)
    obs = env.observe().clone()
    done = torch.zeros(S * E_l, dtype=torch.float32, device=env.device)
    shaped = SimpleNamespace(num_learners=S, nets=[tf] * S, strides=pop.strides, encoder_strides=pop.encoder_strides)
    views = SimpleNamespace(num_learners=S, nets=pop.nets, strides=pop.strides, encoder_strides=pop.encoder_strides,
                            encoder_struct=pop.encoder_struct, policy_struct=pop.policy_struct)
    for call in (lambda: ev.evaluate(tf, 1), lambda: ev.evaluate(shaped, 1), lambda: env.policy_evaluate_population(shaped, 1, 4),
                 lambda: env.policy_evaluate_population(views, 1, 4), lambda: env.policy_evaluate_population(tf, 1, 4),
                 lambda: env.policy_rollout_population(views, 4, obs, done),
                 lambda: env.policy_rollout_population(SimpleNamespace(num_learners=S, nets=[tf] * S), 4, obs, done)):
        with pytest.raises(ValueError, match="attention encoder"):
            call()
    with pytest.raises(ValueError, match="sweeps of transformer learners are not built"):
        env.policy_rollout_population(pop, 4, obs, done, gammas=[0.99, 0.9, 0.99])
    with pytest.raises(ValueError, match="18 envs are not 4 learners' equal shares"):
        env.policy_rollout_population(TransformerPopulation(D, N, list(range(4)), DEV, num_blocks=1), 4, obs, done)
    wet = TransformerPopulation(D, N, [1, 2, 3], DEV, num_blocks=1)
    for m in wet.nets[0].embedding.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1
    with pytest.raises(ValueError, match="dropout p = 0.1"):
        env.policy_rollout_population(wet, 4, obs, done)
    train_cfg = RPOTrainingConfig(num_envs=E_l, num_steps=8, total_timesteps=E_l * 8 * 2)
    for make in (lambda: PopulationTrainer(env, pop, train_cfg), lambda: PopulationAdam(pop)):
        with pytest.raises(ValueError, match="the update of transformer learners is not built"):
            make()
    with pytest.raises(ValueError, match="a capture cannot be given"):
        env.policy_evaluate_population(pop, 1, 4, capture={"frames": None, "starts": None})
    with pytest.raises(ValueError, match="the population has 2 learners, the evaluator 3"):
        ev.evaluate(two, 1)
    with pytest.raises(ValueError, match="18 envs are not 4 learners' equal shares"):
        env.policy_evaluate_population(TransformerPopulation(D, N, list(range(4)), DEV, num_blocks=1), 1, 4)
    torch.cuda.synchronize()
    EC.assert_state_equal(before, EC.state_of(env), "refused calls launch nothing")
    ev.close()


# ------------------------------------------------------------------------------------------------ 5. the C entry's refusals
def evaluate(lib, h, a):
    """The entry on handle `h` with the arguments `a` (Handle.valid, spoiled): its return code."""
    ref = lambda s: None if s is None else C.byref(s)
    return getattr(lib, NAME)(h, a["n_learners"], ref(a["policy"]), ref(a["strides"]), ref(a["transformer"]), ref(a["enc_strides"]),
                              a["agent"], a.get("shared", 1), a["n_episodes"], a["max_steps"], a["progress"], a["episodes_out"],
                              a["norm_state"], 1.0, 1e-8, None)


def test_entry_refusals_have_their_code_and_text_in_their_order_and_enqueue_nothing(ea):
    """5.  tests/test_gpu_policy_refusals.py's table for the new entry, through ctypes on reset handles: the return code and the
    text of evac_last_error of every case, as literals; double faults pin the order -- unbound, NULL strides, the scripted agent,
    an unknown agent, the counts and buffers, the two networks (the attention encoder's token limit among them: it answers N = 64
    and N = 65 alike), the learners.  Box rel + ohe at E = 4, N = 3 (D = 30, six floats a token, ONE block in use); gravity at
    E = 2; E = 1 at N = 64 and N = 65.  Nothing is refused behind the learners on this entry (the one-wave limit is looser than
    the encoder's), so what the strides' check ACCEPTS is shown by calls that run: zero strides with one learner, and short
    strides in a block that is not in use with two."""
    import torch
    from evacuation_amd import _lib
    from evacuation_amd.config import to_c_config
    from evacuation_amd.population import TransformerPopulation
    from tests.test_gpu_policy_refusals import (BAD, COUNTS_TEXT, LEARNERS_TEXT, PROGRESS_TEXT, SCRIPTED, SCRIPTED_TEXT, TOKENS_TEXT,
                                                UNSUPPORTED, Handle, block_changed, changed, two_blocks)
    from tests.test_gpu_transformer_population import visible
    box_wrap = dict(positions="rel", statuses="ohe", type="Box")
    box, grav = Handle(ea, 3, box_wrap, 4, 6), Handle(ea, 3, dict(positions="grav"), 2, 2)
    tokens, big = Handle(ea, 64, box_wrap, 1, 6), Handle(ea, 65, box_wrap, 1, 6)
    handles = (box, grav, tokens, big)
    D, dm = 30, 6
    assert [hd.env.obs_dim for hd in handles] == [D, 6, 396, 402]
    least = block_least(dm)
    fields = [f for f, _ in _lib.EvacTransformerBlockStrides._fields_]
    assert fields == list(least) and box.valid["transformer"].num_blocks == 1
    for hd in handles:
        hd.valid["enc_strides"] = encoder_strides(hd.valid["transformer"].elem_dim)
    POLICY_STRIDE_TEXT = ": a learner stride is smaller than its tensor"
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
        ("the scripted agent and encoder NULL", box, lambda v: dict(agent=SCRIPTED, transformer=None, policy=None), BAD, SCRIPTED_TEXT),
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
        ("encoder NULL", box, lambda v: dict(transformer=None), BAD, ": encoder is NULL"),
        ("policy NULL and encoder NULL", box, lambda v: dict(policy=None, transformer=None), BAD, ": policy is NULL"),
        ("policy.actor_w1 NULL", box, lambda v: dict(policy=changed(v["policy"], "actor_w1", None)), BAD,
         ": a tensor pointer of the policy is NULL"),
        ("hidden = 32", box, lambda v: dict(policy=changed(v["policy"], "hidden", 32)), BAD, ": hidden must be 64"),
        ("obs_dim off by one", box, lambda v: dict(policy=changed(v["policy"], "obs_dim", 31)), BAD, ": policy obs_dim 31 != evac_obs_dim 30"),
        ("num_heads = 2 and a NULL block pointer", box,
         lambda v: dict(transformer=block_changed(changed(v["transformer"], "num_heads", 2), 0, "wk", None)), UNSUPPORTED,
         ": num_heads 2 is not supported (the kernels take 3)"),
        ("num_blocks = 3", box, lambda v: dict(transformer=changed(v["transformer"], "num_blocks", 3)), UNSUPPORTED,
         ": num_blocks 3 is not supported (1 or 2)"),
        ("N = 64", tokens, lambda v: {}, UNSUPPORTED, TOKENS_TEXT % 64),
        ("N = 65", big, lambda v: {}, UNSUPPORTED, TOKENS_TEXT % 65),
        ("N = 64 and n_learners = 0", tokens, lambda v: dict(n_learners=0), UNSUPPORTED, TOKENS_TEXT % 64),
        ("gravity observations", grav, lambda v: {}, UNSUPPORTED,
         ": the gravity observation is not supported (a Box observation of tokens is needed)"),
        ("blocks[0].ff1_b NULL", box, lambda v: dict(transformer=block_changed(v["transformer"], 0, "ff1_b", None)), BAD,
         ": a tensor pointer of the encoder's block 0 is NULL"),
        ("two blocks, blocks[1].dense_w NULL", box, lambda v: dict(transformer=block_changed(two_blocks(v["transformer"]), 1, "dense_w", None)),
         BAD, ": a tensor pointer of the encoder's block 1 is NULL"),
        ("elem_dim = 5", box, lambda v: dict(transformer=changed(v["transformer"], "elem_dim", 5)), BAD,
         ": elem_dim 5 x (3 + 2) tokens is not the observation's 30 floats (a Box observation is needed)"),
        ("encoder NULL and n_learners = 0", box, lambda v: dict(transformer=None, n_learners=0), BAD, ": encoder is NULL"),
        # the learners'
        ("n_learners = 0", box, lambda v: dict(n_learners=0), BAD, LEARNERS_TEXT),
        ("n_learners = EVAC_MAX_LEARNERS + 1", box, lambda v: dict(n_learners=65), BAD, LEARNERS_TEXT),
        ("3 learners on 4 envs", box, lambda v: dict(n_learners=3), BAD, ": the handle's 4 envs are not 3 learners' equal shares"),
        ("a policy stride smaller than the tensor, 2 learners", box, lambda v: dict(strides=changed(v["strides"], "critic_b3", 0)), BAD,
         POLICY_STRIDE_TEXT),
        ("a policy stride and every encoder stride, 2 learners", box,
         lambda v: dict(strides=changed(v["strides"], "actor_w1", 64 * D - 1), enc_strides=all_strides(0)), BAD, POLICY_STRIDE_TEXT),
        ("every encoder stride 0, 2 learners", box, lambda v: dict(enc_strides=all_strides(0)), BAD, ENC_STRIDE_TEXT),
        ("two blocks in use, blocks[1].norm2_b one short, 2 learners", box,
         lambda v: dict(transformer=two_blocks(v["transformer"]),
                        enc_strides=stride_changed(encoder_strides(dm, 2), 1, "norm2_b", least["norm2_b"] - 1)), BAD, ENC_STRIDE_TEXT),
        ("two blocks in use, blocks[1] strides 0, 2 learners", box,
         lambda v: dict(transformer=two_blocks(v["transformer"]), enc_strides=encoder_strides(dm, 1)), BAD, ENC_STRIDE_TEXT),
    ]
    for f in fields:                                                 # each of the 16 of the block in use, one short and 0, two learners
        for value in (least[f] - 1, 0):
            rows.append((f"encoder stride blocks[0].{f} = {value}, 2 learners", box,
                         lambda v, f=f, value=value: dict(enc_strides=stride_changed(v["enc_strides"], 0, f, value)), BAD, ENC_STRIDE_TEXT))
    torch.cuda.synchronize()
    before = {id(hd): hd.snapshot() for hd in handles}
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
    assert len(rows) == 41 + 32
    torch.cuda.synchronize()
    for hd in handles:
        for k, t in hd.snapshot().items():
            assert torch.equal(t, before[id(hd)][k]), k
        assert hd.progress.eq(0).all() and hd.records.eq(0).all()
    # ... and what is accepted runs, on the box handle's four envs, two steps each: real learners with ONE block in use --
    # one learner whose every stride is 0, then two learners whose strides of blocks[1] are short (-5)
    one, two = (visible(TransformerPopulation(D, 3, seeds, DEV, num_blocks=1)) for seeds in ([1], [1, 2]))
    runs = (("every stride 0, 1 learner", one, 1, _lib.EvacMlpPolicyStrides(), all_strides(0)),
            ("blocks[1] strides -5, 2 learners", two, 2, two.strides, merged(two.encoder_strides, all_strides(-5, blocks=(1,)))))
    for what, pop, S, strides, enc_strides in runs:
        box.progress.zero_()
        good = {**box.valid, "n_learners": S, "policy": pop.policy_struct(), "strides": strides, "transformer": pop.encoder_struct(),
                "enc_strides": enc_strides}
        assert evaluate(lib, box.env._h, good) == 0, what
        torch.cuda.synchronize()
        assert box.progress[:, 1].eq(2).all() and box.progress[:, 0].eq(0).all(), what
    for hd in handles:
        hd.env.close()
