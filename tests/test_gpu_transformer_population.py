"""Collection of a population of transformer leaders on an MI355X (evac_policy_rollout_population_transformer;
policy_rollout_population with a TransformerPopulation): S attention-encoder learners in one launch, each BIT FOR BIT the learner
it would be alone (evac_policy_rollout_transformer, which tests/test_gpu_transformer.py holds to the float64 restatement).

1. Collection: policy_rollout_population(TransformerPopulation) == S policy_rollout calls on handles of E_l envs with env_id_offset
   further by s E_l -- storage, norm_state, records, the final state of env and handle.
2. The encoder's strides are used, block by block: learners that share their 13 actor-critic tensors and differ in the encoder,
   and learners that differ in the SECOND block's norm2_b alone, act differently and each as it does alone.
3. Invariance: two runs from the same state give the same bytes; T = 33 == 7 + 26.
4. Past the first 64-step noise block: T = 70 at max_timesteps = 70.
5. The collection entry's own refusals through ctypes: code and text, in their order, nothing enqueued.

Equal means: the float32 / int32 / float64 words are compared as integers.  No tolerance anywhere."""
import ctypes as C

import pytest

from tests import test_gpu_transformer as TF
from tests.encoder_cases import ea  # noqa: F401 (the fixture)
from tests.test_gpu_policy_rollout import OFFSET, SEED, assert_split_equals_one, base, i32, raw
from tests.test_gpu_population import STORAGE_E, STORAGE_TE, restore, snapshot, start_population
from tests.trainer_cases import DEV

pytestmark = pytest.mark.gpu

N62, N10, N31, N60G = "n62_rel_ohe_box_norm_clip", "n10_abs_cat_box_raw", "n31_rel_no_box_norm", "n60_rel_ohe_box_raw_resid_generic"
# (case, S, E_l) of tests 1 here and 1 of tests/test_gpu_transformer_population_evaluate.py
GEOMETRIES = [
    (N62, 3, 5),      # 64 tokens (the full wave), dm 6, two blocks, the DEF kernels, the chain, one partly filled workgroup a learner
    (N10, 2, 17),     # dm 3, one block, a second workgroup per learner that holds one env
    (N31, 4, 16),     # dm 2, 33 tokens, exactly full workgroups
    (N60G, 2, 3),     # use_resid, the non-DEF kernels, two idle lanes
]
ENC_STRIDE_TEXT = ": an encoder stride of a block in use is smaller than its tensor"
NULL_STRIDES_TEXT = ": strides / enc_strides is NULL"


def make_env(ea, case, E, offset, raw_env=False, options=None, **cfg_over):
    """The case's env of tests/test_gpu_transformer.py at `offset`, with the case's own kernel options."""
    from evacuation_amd.options import KernelOptions
    cfg_kw, wrap_kw, norm, opts = TF.CASES[case][:4]
    opts = {**opts, **(options or {})}
    env = ea.BatchedEvacuationEnv(ea.EnvConfig(**{**cfg_kw, **cfg_over}), ea.EnvWrappersConfig(**wrap_kw), num_envs=E, seed=SEED,
                                  env_id_offset=offset, options=KernelOptions().replace(**opts) if opts else None)
    return ea.NormalizedVectorEnv(env) if norm and not raw_env else env


def visible(pop):
    """Freshly seeded learners made visible by tests/test_gpu_transformer.make_net's recipe, each in its own way: a scaled last
    actor layer, sigmas and biases of its own, LayerNorm weights and biases away from 1 and 0."""
    import torch
    with torch.no_grad():
        for s, net in enumerate(pop.nets):
            g = torch.Generator().manual_seed(1000 + s)
            net.actor_mean[4].weight.mul_(60.0)
            net.actor_logstd.copy_(torch.tensor([[-0.5 + 0.1 * s, 0.3 - 0.05 * s]]))
            for m in list(net.actor_mean) + list(net.critic):
                if isinstance(m, torch.nn.Linear):
                    m.bias.copy_((0.2 * torch.randn(m.bias.shape, generator=g)).to(DEV))
            for m in net.embedding.modules():
                if isinstance(m, torch.nn.LayerNorm):
                    m.weight.copy_((0.5 + torch.rand(m.weight.shape, generator=g)).to(DEV))
                    m.bias.copy_((0.3 * torch.randn(m.bias.shape, generator=g)).to(DEV))
    return pop


def make_population(env, case, S, **net_over):
    from evacuation_amd.population import TransformerPopulation
    b = base(env)
    return visible(TransformerPopulation(b.obs_dim, b.n_ped, [11 + 7 * s for s in range(S)], DEV, **{**TF.CASES[case][4], **net_over}))


# ------------------------------------------------------------------------------------------------ 1. collection
def collection_equals_standalone_rollouts(ea, case, S, E_l, T=30, shape=None, net_over=None, **cfg_over):
    """Learner s's storage, norm_state, records and final state are those of policy_rollout(nets[s]) alone.  `shape(pop)`: what
    a test does to the population before the call.  Returns the population call's storage."""
    import torch
    pop_env = make_env(ea, case, S * E_l, OFFSET, **cfg_over)
    b = base(pop_env)
    pop = make_population(pop_env, case, S, **(net_over or {}))
    assert len(pop.tensors) == 13 + 16 * pop.num_blocks
    if shape is not None:
        shape(pop)
    obs, done, now = start_population(pop_env)
    obs0 = obs.clone()
    norm0 = pop_env.norm_state.clone() if hasattr(pop_env, "norm_state") else None
    ro = pop_env.policy_rollout_population(pop, T, obs, done)
    assert ro["next_obs"] is obs and ro["next_done"] is done
    torch.cuda.synchronize()
    ended = int(ro["dones"][1:].sum()) + int(ro["next_done"].sum())
    assert ended >= (S * E_l) // 5 and ended >= 1 and 5 * ended >= S * E_l          # at least a fifth autoreset inside the call
    fin = snapshot(pop_env)
    for s in range(S):
        cols = slice(s * E_l, (s + 1) * E_l)
        env = make_env(ea, case, E_l, OFFSET + s * E_l, **cfg_over)
        o, _ = env.reset()
        assert i32(o).equal(i32(obs0[cols])), (case, s, "the reset observation")       # the same start state
        base(env).set_state(now=now[cols].clone())
        if norm0 is not None:
            assert raw(env.norm_state).equal(raw(norm0[cols])), (case, s, "norm_state after reset")
        d = torch.zeros(E_l, dtype=torch.float32, device=DEV)
        alone = env.policy_rollout(pop.nets[s], T, o.clone(), d)
        torch.cuda.synchronize()
        for k in STORAGE_TE:
            assert i32(ro[k][:, cols]).equal(i32(alone[k])), (case, S, E_l, s, k)
        for k in STORAGE_E:
            assert i32(ro[k][cols]).equal(i32(alone[k])), (case, S, E_l, s, k)
        mine = snapshot(env)
        for k in mine:
            assert raw(fin[k][cols]).equal(raw(mine[k])), (case, S, E_l, s, k)
        sa, sb = b.get_state(), base(env).get_state()
        for k in sa:
            assert sa[k][cols].contiguous().view(torch.uint8).equal(sb[k].contiguous().view(torch.uint8)), (case, s, k)
        env.close()
    if S > 1:                                                        # the learners did act differently
        assert not i32(ro["actions"][:, :E_l]).equal(i32(ro["actions"][:, E_l:2 * E_l]))
    pop_env.close()
    return ro


@pytest.mark.parametrize("case,S,E_l", GEOMETRIES + [(N10, 1, 17)])
def test_collection_equals_standalone_rollouts(ea, case, S, E_l):
    """1.  T = 30 at max_timesteps of 20 to 25: every env autoresets inside the call."""
    assert 20 <= TF.CASES[case][0]["max_timesteps"] <= 25
    collection_equals_standalone_rollouts(ea, case, S, E_l)


# ------------------------------------------------------------------------------------------------ 2. the encoder's strides
def share_the_actor_critic(pop):
    import torch
    with torch.no_grad():
        for t in pop.tensors[:13]:
            t[1:] = t[0]
    assert all(i32(t[0]).equal(i32(t[1])) for t in pop.tensors[:13])
    assert not any(i32(t[0]).equal(i32(t[1])) for t in pop.tensors[13:])        # every encoder tensor differs


LAST_NORM2_B = 13 + 16 + 15


def differ_in_the_second_blocks_last_tensor(pop):
    import torch
    with torch.no_grad():
        for t in pop.tensors:
            t[1:] = t[0]
        pop.tensors[LAST_NORM2_B][1] += torch.tensor([0.4, -0.3, 0.2], device=DEV)
    assert [i for i, t in enumerate(pop.tensors) if not i32(t[0]).equal(i32(t[1]))] == [LAST_NORM2_B]
    assert pop.nets[1].embedding[1].norm2.bias.data_ptr() == pop.tensors[LAST_NORM2_B][1].data_ptr()


@pytest.mark.parametrize("shape", [share_the_actor_critic, differ_in_the_second_blocks_last_tensor])
def test_the_encoders_strides_are_used_block_by_block(ea, shape):
    """2.  n10-size rooms (3 floats a token) with TWO blocks, S = 2, E_l = 2: a kernel that read learner 0's encoder, or its
    second block, for learner 1 would give both the same actions (asserted different inside) or miss learner 1's lone rollout."""
    collection_equals_standalone_rollouts(ea, N10, 2, 2, shape=shape, net_over=dict(num_blocks=2))


# ------------------------------------------------------------------------------------------------ 3. invariance
def test_two_runs_and_split_calls_give_the_same_bytes(ea):
    """3.  The normalised chain at 33 tokens, S = 2, E_l = 5: T = 33 twice, and as 7 + 26."""
    import torch
    case, S, E_l = N31, 2, 5
    env = make_env(ea, case, S * E_l, OFFSET)
    pop = make_population(env, case, S)
    obs0, done0, _ = start_population(env)
    state0 = snapshot(env)

    def run(T_split):
        restore(env, state0)
        obs, done = obs0.clone(), done0.clone()
        outs = [{k: v.clone() for k, v in env.policy_rollout_population(pop, T, obs, done).items()} for T in T_split]
        torch.cuda.synchronize()
        return outs, snapshot(env)
    (one,), f1 = run([33])
    (again,), f2 = run([33])
    assert_split_equals_one(one, f1, [again], f2, "two runs")
    parts, f3 = run([7, 26])
    assert_split_equals_one(one, f1, parts, f3, "7 + 26")
    assert int(one["dones"][1:].sum()) >= 2
    env.close()


# ------------------------------------------------------------------------------------------------ 4. past the first noise block
def test_collection_past_the_first_64_step_noise_block(ea):
    """4.  tests/test_gpu_policy_long.py's rule: the policy's noise is drawn 64 steps at a time, so a launch of T = 70 reads its
    second block -- at max_timesteps = 70 the envs that start fresh end their episode at step 69 of the launch, inside it."""
    import torch
    T = 70
    ro = collection_equals_standalone_rollouts(ea, N10, 2, 3, T=T, max_timesteps=70)
    assert ro["obs"].shape[0] == T > 64
    ended = torch.cat([ro["dones"][1:].bool(), ro["next_done"].bool()[None]], dim=0)
    at = ended.any(1).nonzero().flatten().tolist()
    assert max(at) >= 64 and min(at) < 64, at


# ------------------------------------------------------------------------------------------------ 5. the C entry's refusals
NAME = "evac_policy_rollout_population_transformer"


def block_least(dm):
    """The sizes of a block's 16 tensors at token width dm, in evac_transformer_block_t's order."""
    return dict(wq=3 * dm * dm, bq=3 * dm, wk=3 * dm * dm, bk=3 * dm, wv=3 * dm * dm, bv=3 * dm, dense_w=3 * dm * dm, dense_b=dm,
                ff1_w=96 * dm, ff1_b=96, ff2_w=96 * dm, ff2_b=dm, norm1_w=dm, norm1_b=dm, norm2_w=dm, norm2_b=dm)


def encoder_strides(dm, blocks=1, **changes):
    """evac_transformer_strides_t with the first `blocks` blocks at their tensors' sizes (the others 0); `changes`: field -> value
    of block 0, or (block, field) pairs through ``stride_changed``."""
    from evacuation_amd import _lib
    st = _lib.EvacTransformerStrides()
    for b in range(blocks):
        st.blocks[b] = _lib.EvacTransformerBlockStrides(*block_least(dm).values())
    for f, v in changes.items():
        setattr(st.blocks[0], f, v)
    return st


def stride_changed(st, block, field, value):
    s2 = type(st).from_buffer_copy(st)
    setattr(s2.blocks[block], field, value)
    return s2


def all_strides(value, blocks=(0, 1)):
    from evacuation_amd import _lib
    st = _lib.EvacTransformerStrides()
    for b in blocks:
        st.blocks[b] = _lib.EvacTransformerBlockStrides(*[value] * 16)
    return st


def merged(first, second):
    """blocks[0] of `first`, blocks[1] of `second`."""
    out = type(first).from_buffer_copy(first)
    out.blocks[1] = type(second.blocks[1]).from_buffer_copy(second.blocks[1])
    return out


def collect(lib, h, a):
    """The entry on handle `h` with the arguments `a` (Handle.valid, spoiled): its return code."""
    from tests.test_gpu_policy_refusals import BUFFERS
    ref = lambda s: None if s is None else C.byref(s)
    bufs = [a[k] for k in BUFFERS] + [a["final_stats"], a["norm_state"], 0.99, 1.0, 100.0, 1e-8]
    return getattr(lib, NAME)(h, a["n_learners"], ref(a["policy"]), ref(a["strides"]), ref(a["transformer"]), ref(a["enc_strides"]),
                              a["n_steps"], *bufs, None)


def test_collection_entry_refusals_have_their_code_and_text_and_enqueue_nothing(ea):
    """5.  tests/test_gpu_policy_refusals.py's table for the new collection entry, through ctypes on reset handles: the return
    code and the text of evac_last_error of every case, as literals.  A refused call enqueues nothing: nothing is launched here
    but `reset`, and every handle's state is bit-equal before and after the table.  Box rel + ohe at E = 4, N = 3 (D = 30, six
    floats a token, ONE block in use); gravity at E = 2; E = 1 at N = 64 (one wave of pedestrians, but 66 tokens) and N = 65.
    What one learner cannot break -- its strides are never applied -- and what a block that is not in use holds are accepted:
    such a call is shown to pass the strides' check by the refusal that comes behind it (the alignment of actions_out), which
    two learners with a short stride in a block in use do not reach."""
    import torch
    from evacuation_amd import _lib
    from tests.test_gpu_policy_refusals import (BAD, ENCODER_BUFFERS_TEXT, LEARNERS_TEXT, ROOMS_TEXT, TOKENS_TEXT, UNSUPPORTED, Handle,
                                                block_changed, changed, two_blocks)
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
    misaligned = lambda v: v["actions_out"] + 4
    ALIGN_TEXT = ": actions_out must be 8-byte aligned"
    rows = [  # (what, handle, the changes, code, the text after the entry's name)
        ("strides NULL", box, lambda v: dict(strides=None), BAD, NULL_STRIDES_TEXT),
        ("enc_strides NULL", box, lambda v: dict(enc_strides=None), BAD, NULL_STRIDES_TEXT),
        ("enc_strides NULL, one learner", box, lambda v: dict(enc_strides=None, n_learners=1), BAD, NULL_STRIDES_TEXT),
        ("N = 65 and enc_strides NULL", big, lambda v: dict(enc_strides=None), BAD, NULL_STRIDES_TEXT),
        # what the siblings refuse, in their order
        ("N = 65", big, lambda v: {}, UNSUPPORTED, ROOMS_TEXT),
        ("N = 65 and n_steps = 0", big, lambda v: dict(n_steps=0), UNSUPPORTED, ROOMS_TEXT),
        ("n_steps = 0", box, lambda v: dict(n_steps=0), BAD, ": n_steps must be >= 1"),
        ("reward_out NULL", box, lambda v: dict(reward_out=None), BAD, ENCODER_BUFFERS_TEXT),
        ("policy NULL", box, lambda v: dict(policy=None), BAD, ": policy is NULL"),
        ("encoder NULL", box, lambda v: dict(transformer=None), BAD, ": encoder is NULL"),
        ("policy.critic_b3 NULL", box, lambda v: dict(policy=changed(v["policy"], "critic_b3", None)), BAD,
         ": a tensor pointer of the policy is NULL"),
        ("num_heads = 2", box, lambda v: dict(transformer=changed(v["transformer"], "num_heads", 2)), UNSUPPORTED,
         ": num_heads 2 is not supported (the kernels take 3)"),
        ("N = 64", tokens, lambda v: {}, UNSUPPORTED, TOKENS_TEXT % 64),
        ("gravity observations", grav, lambda v: {}, UNSUPPORTED,
         ": the gravity observation is not supported (a Box observation of tokens is needed)"),
        ("blocks[0].norm2_b NULL", box, lambda v: dict(transformer=block_changed(v["transformer"], 0, "norm2_b", None)), BAD,
         ": a tensor pointer of the encoder's block 0 is NULL"),
        ("elem_dim = 5", box, lambda v: dict(transformer=changed(v["transformer"], "elem_dim", 5)), BAD,
         ": elem_dim 5 x (3 + 2) tokens is not the observation's 30 floats (a Box observation is needed)"),
        ("encoder NULL and n_learners = 0", box, lambda v: dict(transformer=None, n_learners=0), BAD, ": encoder is NULL"),
        # the learners'
        ("n_learners = 0", box, lambda v: dict(n_learners=0), BAD, LEARNERS_TEXT),
        ("n_learners = EVAC_MAX_LEARNERS + 1", box, lambda v: dict(n_learners=65), BAD, LEARNERS_TEXT),
        ("3 learners on 4 envs", box, lambda v: dict(n_learners=3), BAD, ": the handle's 4 envs are not 3 learners' equal shares"),
        ("a policy stride smaller than the tensor, 2 learners", box, lambda v: dict(strides=changed(v["strides"], "critic_b3", 0)), BAD,
         ": a learner stride is smaller than its tensor"),
        ("a policy stride and every encoder stride, 2 learners", box,
         lambda v: dict(strides=changed(v["strides"], "actor_w1", 64 * D - 1), enc_strides=all_strides(0)), BAD,
         ": a learner stride is smaller than its tensor"),
        ("every encoder stride 0, 2 learners, actions_out + 4 bytes", box, lambda v: dict(enc_strides=all_strides(0), actions_out=misaligned(v)),
         BAD, ENC_STRIDE_TEXT),
        ("two blocks in use, blocks[1].ff1_w one short, 2 learners", box,
         lambda v: dict(transformer=two_blocks(v["transformer"]),
                        enc_strides=stride_changed(encoder_strides(dm, 2), 1, "ff1_w", least["ff1_w"] - 1)), BAD, ENC_STRIDE_TEXT),
        # ... and the same strides with ONE learner are accepted: the call gets to the check behind them
        ("every encoder stride 0, 1 learner, actions_out + 4 bytes", box,
         lambda v: dict(enc_strides=all_strides(0), n_learners=1, actions_out=misaligned(v)), BAD, ALIGN_TEXT),
        ("every policy stride 0 too, 1 learner, actions_out + 4 bytes", box,
         lambda v: dict(enc_strides=all_strides(0), strides=_lib.EvacMlpPolicyStrides(), n_learners=1, actions_out=misaligned(v)), BAD, ALIGN_TEXT),
        # ... and so is anything in a block that is not in use (num_blocks = 1), with two learners
        ("blocks[1] strides 0, one block in use, 2 learners, actions_out + 4 bytes", box,
         lambda v: dict(enc_strides=encoder_strides(dm, 1), actions_out=misaligned(v)), BAD, ALIGN_TEXT),
        ("blocks[1] strides -5, one block in use, 2 learners, actions_out + 4 bytes", box,
         lambda v: dict(enc_strides=merged(encoder_strides(dm, 1), all_strides(-5, blocks=(1,))), actions_out=misaligned(v)), BAD,
         ALIGN_TEXT),
        ("actions_out + 4 bytes", box, lambda v: dict(actions_out=misaligned(v)), BAD, ALIGN_TEXT),
    ]
    for f in fields:                                                 # each of the 16 of the block in use, one short and 0, two learners
        for value in (least[f] - 1, 0):
            rows.append((f"encoder stride blocks[0].{f} = {value}, 2 learners", box,
                         lambda v, f=f, value=value: dict(enc_strides=stride_changed(v["enc_strides"], 0, f, value)), BAD, ENC_STRIDE_TEXT))
    torch.cuda.synchronize()
    before = {id(hd): hd.snapshot() for hd in handles}
    lib = box.env.lib
    for what, hd, spoil, code, text in rows:
        args = {**hd.valid, **spoil(hd.valid)}
        rc = collect(lib, hd.env._h, args)
        got = (lib.evac_last_error(hd.env._h) or b"").decode()
        assert rc != 0, what                                          # (a call that went through: stop before anything else is tried)
        assert (rc, got) == (code, NAME + text), what
    assert len(rows) == 29 + 32
    torch.cuda.synchronize()
    for hd in handles:
        for k, t in hd.snapshot().items():
            assert torch.equal(t, before[id(hd)][k]), k
        hd.env.close()
