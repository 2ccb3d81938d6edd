"""What the nine entries that run a network on a handle's envs refuse, and in which order (include/evac.h: evac_policy_rollout,
_population, _sweep, _deepsets, _transformer; evac_policy_evaluate, _population, _deepsets, _transformer), through ctypes: the
return code and the text of evac_last_error of every case, as literals.  A refused call enqueues nothing: nothing is launched
here but `reset`, and every handle's state is bit-equal before and after the whole table.

Four handles: E = 4, N = 3, Box rel + ohe (D = 30; four envs are no three learners' shares); E = 2, N = 3, gravity (no set of
rows or tokens for an encoder); E = 1, N = 65 (more than one wave); E = 1, N = 63 (one wave, but N + 2 tokens are more than one:
the transformer entries alone).  Single faults first; the double faults pin the precedence: collection refuses a room of more
than 64 pedestrians first and evaluation last -- so the transformer's evaluation answers N = 65 with its own limit of 62 -- a
missing policy comes after the buffers, the encoder entries' evaluation refuses the scripted agent before anything else, and
the attention encoder's sizes are looked at before its pointers."""
import ctypes as C
import math

import pytest

pytestmark = pytest.mark.gpu

BAD, UNSUPPORTED = -1, -3
COLLECT = ("evac_policy_rollout", "evac_policy_rollout_population", "evac_policy_rollout_sweep", "evac_policy_rollout_deepsets",
           "evac_policy_rollout_transformer")
EVALUATE = ("evac_policy_evaluate", "evac_policy_evaluate_population", "evac_policy_evaluate_deepsets",
            "evac_policy_evaluate_transformer")
LEARNERS = ("evac_policy_rollout_population", "evac_policy_rollout_sweep", "evac_policy_evaluate_population")
DEEPSETS = ("evac_policy_rollout_deepsets", "evac_policy_evaluate_deepsets")
TRANSFORMER = ("evac_policy_rollout_transformer", "evac_policy_evaluate_transformer")
ENCODERS = DEEPSETS + TRANSFORMER
LINEAR_COLLECT, LINEAR_EVALUATE = COLLECT[:3], EVALUATE[:2]
EVERY = COLLECT + EVALUATE
STATE = ("ped", "status", "agent", "clock", "acc")
BUFFERS = ("next_obs", "next_done", "obs_out", "actions_out", "logprob_out", "value_out", "reward_out", "done_out", "next_value_out")
T = 2

BUFFERS_TEXT = ": policy and every output buffer but final_stats / norm_state must be non-NULL"
ENCODER_BUFFERS_TEXT = ": every output buffer but final_stats / norm_state must be non-NULL"
ROOMS_TEXT = ": rooms of more than 64 pedestrians are not supported (one wave per env)"
TOKENS_TEXT = ": N = %d pedestrians is not supported (one wave holds the N + 2 tokens: N <= 62)"
SCRIPTED_TEXT = ": the scripted agent has no network (use evac_policy_evaluate)"
LEARNERS_TEXT = ": n_learners must be in 1..64"
COUNTS_TEXT = ": n_episodes and max_steps must be >= 1"
PROGRESS_TEXT = ": progress / episodes_out is NULL"
HYPERS_TEXT = ": hypers is NULL or a learner's values are refused (see evac_learner_hyper_t)"


class Handle:
    """A reset env and the arguments of a call that every entry accepts on it (no such call is made)."""

    def __init__(self, ea, n_ped, wrap, E, elem_dim):
        import torch
        from evacuation_amd import _lib
        self.env = ea.BatchedEvacuationEnv(ea.EnvConfig(number_of_pedestrians=n_ped), ea.EnvWrappersConfig(**wrap), num_envs=E)
        self.env.reset()
        D, dev = self.env.obs_dim, self.env.device
        self.weights = torch.zeros(64 * D, device=dev)
        self.room = [torch.zeros(T * E * max(D, 10), device=dev) for _ in range(len(BUFFERS) + 1)]
        self.progress = torch.zeros((E, 4), dtype=torch.int32, device=dev)
        self.records = torch.zeros((1, E, 10), device=dev)
        self.norm_state = torch.zeros((E, 3 * D + 4), dtype=torch.float64, device=dev)
        w = self.weights.data_ptr()
        transformer = _lib.EvacTransformer(elem_dim, 1, 3, 96, 0, 1e-5)
        transformer.blocks[0] = _lib.EvacTransformerBlock(*[w] * 16)
        self.valid = dict(
            n_steps=T, policy=_lib.EvacMlpPolicy(D, 64, *[w] * 13), encoder=_lib.EvacDeepSets(elem_dim, 24, *[w] * 6),
            transformer=transformer,
            strides=_lib.EvacMlpPolicyStrides(64 * D, 64, 64 * 64, 64, 128, 2, 2, 64 * D, 64, 64 * 64, 64, 64, 1),
            n_learners=2 if E > 1 else 1, hypers=_lib.learner_hypers(64), final_stats=self.room[-1].data_ptr(), norm_state=None,
            agent=_lib.AGENT_POLICY_MEAN, n_episodes=1, max_steps=T, progress=self.progress.data_ptr(),
            episodes_out=self.records.data_ptr(), **{k: t.data_ptr() for k, t in zip(BUFFERS, self.room)})

    def snapshot(self):
        return {k: getattr(self.env, k).clone() for k in STATE}


def invoke(lib, entry, h, a):
    """`entry` on handle `h` with the arguments `a` (Handle.valid, spoiled): its return code."""
    ref = lambda s: None if s is None else C.byref(s)
    bufs = [a[k] for k in BUFFERS] + [a["final_stats"], a["norm_state"], 0.99, 1.0, 100.0, 1e-8]
    ev = [a["n_episodes"], a["max_steps"], a["progress"], a["episodes_out"], a["norm_state"], 1.0, 1e-8]
    pol, enc, tf, strides = ref(a["policy"]), ref(a["encoder"]), ref(a["transformer"]), ref(a["strides"])
    if entry == "evac_policy_rollout":
        return lib.evac_policy_rollout(h, a["n_steps"], pol, *bufs, None)
    if entry == "evac_policy_rollout_population":
        return lib.evac_policy_rollout_population(h, a["n_learners"], pol, strides, a["n_steps"], *bufs, None)
    if entry == "evac_policy_rollout_sweep":
        return lib.evac_policy_rollout_sweep(h, a["n_learners"], pol, strides, a["n_steps"], *bufs, a["hypers"], None)
    if entry == "evac_policy_rollout_deepsets":
        return lib.evac_policy_rollout_deepsets(h, a["n_steps"], pol, *bufs, enc, None)
    if entry == "evac_policy_evaluate":
        return lib.evac_policy_evaluate(h, a["agent"], pol, *ev, None)
    if entry == "evac_policy_evaluate_population":
        return lib.evac_policy_evaluate_population(h, a["n_learners"], pol, strides, a["agent"], 1, *ev, None)
    if entry == "evac_policy_evaluate_deepsets":
        return lib.evac_policy_evaluate_deepsets(h, a["agent"], pol, *ev, enc, None)
    if entry == "evac_policy_rollout_transformer":
        return lib.evac_policy_rollout_transformer(h, a["n_steps"], pol, *bufs, tf, None)
    assert entry == "evac_policy_evaluate_transformer"
    return lib.evac_policy_evaluate_transformer(h, a["agent"], pol, *ev, tf, None)


def changed(struct, field, value):
    s2 = type(struct).from_buffer_copy(struct)
    setattr(s2, field, value)
    return s2


def block_changed(transformer, block, field, value):
    t2 = type(transformer).from_buffer_copy(transformer)
    setattr(t2.blocks[block], field, value)
    return t2


def two_blocks(transformer):
    t2 = changed(transformer, "num_blocks", 2)
    t2.blocks[1] = type(t2.blocks[0]).from_buffer_copy(t2.blocks[0])
    return t2


def nan_gamma(hypers):
    out = type(hypers).from_buffer_copy(hypers)
    out[1].gamma = math.nan
    return out


SCRIPTED = 2        # EVAC_AGENT_VACUUM_CLEANER


def table(handles):
    """(what, handle, entries, spoil(valid arguments) -> the changes, code, the text after the entry's name or {entry: text})."""
    box, grav, big, tokens = handles["box"], handles["grav"], handles["big"], handles["tokens"]
    rows = []

    def add(what, entries, spoil, text, code=BAD, handle=box):
        rows.append((what, handle, entries, spoil, code, text))
    # ---- single faults ----
    add("n_steps = 0", COLLECT, lambda v: dict(n_steps=0), ": n_steps must be >= 1")
    for k in ("next_obs", "reward_out", "next_value_out"):
        add(f"{k} NULL", COLLECT, lambda v, k=k: {k: None}, {**{e: BUFFERS_TEXT for e in LINEAR_COLLECT},
                                                             "evac_policy_rollout_deepsets": ENCODER_BUFFERS_TEXT,
                                                             "evac_policy_rollout_transformer": ENCODER_BUFFERS_TEXT})
    add("policy NULL", EVERY, lambda v: dict(policy=None),
        {**{e: BUFFERS_TEXT for e in LINEAR_COLLECT}, **{e: ": a policy agent needs a policy" for e in LINEAR_EVALUATE},
         **{e: ": policy is NULL" for e in ENCODERS}})
    for f in ("actor_w1", "actor_logstd", "critic_b3"):
        add(f"policy.{f} NULL", EVERY, lambda v, f=f: dict(policy=changed(v["policy"], f, None)), ": a tensor pointer of the policy is NULL")
    add("hidden = 32", EVERY, lambda v: dict(policy=changed(v["policy"], "hidden", 32)), ": hidden must be 64")
    add("obs_dim off by one", EVERY, lambda v: dict(policy=changed(v["policy"], "obs_dim", 31)), ": policy obs_dim 31 != evac_obs_dim 30")
    add("actions_out + 4 bytes", COLLECT, lambda v: dict(actions_out=v["actions_out"] + 4), ": actions_out must be 8-byte aligned")
    add("strides NULL", LEARNERS, lambda v: dict(strides=None), ": strides is NULL")
    add("n_learners = 0", LEARNERS, lambda v: dict(n_learners=0), LEARNERS_TEXT)
    add("n_learners = EVAC_MAX_LEARNERS + 1", LEARNERS, lambda v: dict(n_learners=65), LEARNERS_TEXT)
    add("3 learners on 4 envs", LEARNERS, lambda v: dict(n_learners=3), ": the handle's 4 envs are not 3 learners' equal shares")
    for f, least in (("actor_w1", 64 * 30), ("critic_b3", 1)):
        add(f"stride of {f} smaller than the tensor, 2 learners", LEARNERS,
            lambda v, f=f, least=least: dict(strides=changed(v["strides"], f, least - 1)), ": a learner stride is smaller than its tensor")
    add("hypers NULL", COLLECT[2:3], lambda v: dict(hypers=None), HYPERS_TEXT)
    add("a NaN gamma", COLLECT[2:3], lambda v: dict(hypers=nan_gamma(v["hypers"])), HYPERS_TEXT)
    add("agent 7", EVALUATE, lambda v: dict(agent=7), ": unknown agent 7")
    add("the scripted agent with strides", EVALUATE[1:2], lambda v: dict(agent=SCRIPTED, policy=None),
        ": the scripted agent has no learners: evac_policy_evaluate runs it")
    add("the scripted agent with norm_state", EVALUATE[:1], lambda v: dict(agent=SCRIPTED, policy=None, norm_state=box.norm_state.data_ptr()),
        ": the scripted agent reads no observation: norm_state must be NULL")
    add("the scripted agent on the encoder entries", EVALUATE[2:], lambda v: dict(agent=SCRIPTED), SCRIPTED_TEXT)
    add("progress NULL", EVALUATE, lambda v: dict(progress=None), PROGRESS_TEXT)
    add("episodes_out NULL", EVALUATE, lambda v: dict(episodes_out=None), PROGRESS_TEXT)
    add("progress + 4 bytes", EVALUATE, lambda v: dict(progress=v["progress"] + 4), ": progress must be 16-byte aligned")
    add("n_episodes = 0", EVALUATE, lambda v: dict(n_episodes=0), COUNTS_TEXT)
    add("max_steps = 0", EVALUATE, lambda v: dict(max_steps=0), COUNTS_TEXT)
    add("encoder NULL", DEEPSETS, lambda v: dict(encoder=None), ": encoder is NULL")
    for f in ("phi_w1", "phi_b2", "rho_b"):
        add(f"encoder.{f} NULL", DEEPSETS, lambda v, f=f: dict(encoder=changed(v["encoder"], f, None)),
            ": a tensor pointer of the encoder is NULL")
    add("encoder hidden = 16", DEEPSETS, lambda v: dict(encoder=changed(v["encoder"], "hidden", 16)), ": the encoder's hidden must be 24")
    add("set_elem_dim = 5", DEEPSETS, lambda v: dict(encoder=changed(v["encoder"], "set_elem_dim", 5)),
        ": set_elem_dim 5 x (3 + 2) elements is not the observation's 30 floats (a Box observation is needed)")
    add("rho_w + 4 bytes", DEEPSETS, lambda v: dict(encoder=changed(v["encoder"], "rho_w", v["encoder"].rho_w + 4)),
        ": rho_w must be 16-byte aligned")
    add("gravity observations", DEEPSETS, lambda v: {},
        ": set_elem_dim 2 x (3 + 2) elements is not the observation's 6 floats (a Box observation is needed)", handle=grav)
    add("transformer NULL", TRANSFORMER, lambda v: dict(transformer=None), ": encoder is NULL")
    for f in ("wq", "ff1_b", "norm2_b"):
        add(f"transformer.blocks[0].{f} NULL", TRANSFORMER, lambda v, f=f: dict(transformer=block_changed(v["transformer"], 0, f, None)),
            ": a tensor pointer of the encoder's block 0 is NULL")
    add("two blocks, blocks[1].dense_w NULL", TRANSFORMER,
        lambda v: dict(transformer=block_changed(two_blocks(v["transformer"]), 1, "dense_w", None)),
        ": a tensor pointer of the encoder's block 1 is NULL")
    for f, value, text in (("num_heads", 2, ": num_heads 2 is not supported (the kernels take 3)"),
                           ("dim_feedforward", 64, ": dim_feedforward 64 is not supported (the kernels take 96)"),
                           ("num_blocks", 0, ": num_blocks 0 is not supported (1 or 2)"),
                           ("num_blocks", 3, ": num_blocks 3 is not supported (1 or 2)"),
                           ("ln_eps", 1e-6, ": ln_eps other than 1e-5 is not supported")):
        add(f"transformer.{f} = {value}", TRANSFORMER, lambda v, f=f, value=value: dict(transformer=changed(v["transformer"], f, value)),
            text, code=UNSUPPORTED)
    add("elem_dim = 5", TRANSFORMER, lambda v: dict(transformer=changed(v["transformer"], "elem_dim", 5)),
        ": elem_dim 5 x (3 + 2) tokens is not the observation's 30 floats (a Box observation is needed)")
    add("gravity observations, transformer", TRANSFORMER, lambda v: {},
        ": the gravity observation is not supported (a Box observation of tokens is needed)", code=UNSUPPORTED, handle=grav)
    add("N = 63", TRANSFORMER, lambda v: {}, TOKENS_TEXT % 63, code=UNSUPPORTED, handle=tokens)
    add("N = 65", EVERY, lambda v: {}, {**{e: ROOMS_TEXT for e in EVERY}, "evac_policy_evaluate_transformer": TOKENS_TEXT % 65},
        code=UNSUPPORTED, handle=big)
    # ---- double faults: the precedence ----
    two = ("evac_policy_rollout", "evac_policy_rollout_deepsets", "evac_policy_rollout_transformer")
    add("N = 65 and n_steps = 0", two, lambda v: dict(n_steps=0), ROOMS_TEXT, code=UNSUPPORTED, handle=big)
    add("policy NULL and a NULL buffer", two, lambda v: dict(policy=None, done_out=None),
        {two[0]: BUFFERS_TEXT, two[1]: ENCODER_BUFFERS_TEXT, two[2]: ENCODER_BUFFERS_TEXT})
    two = ("evac_policy_evaluate", "evac_policy_evaluate_deepsets", "evac_policy_evaluate_transformer")
    add("N = 65 and n_episodes = 0", two, lambda v: dict(n_episodes=0), COUNTS_TEXT, handle=big)
    add("policy NULL and progress NULL", two, lambda v: dict(policy=None, progress=None), PROGRESS_TEXT)
    add("the scripted agent and encoder NULL", two[1:], lambda v: dict(agent=SCRIPTED, encoder=None, transformer=None), SCRIPTED_TEXT)
    add("num_heads = 2 and a NULL block pointer", TRANSFORMER,
        lambda v: dict(transformer=block_changed(changed(v["transformer"], "num_heads", 2), 0, "wk", None)),
        ": num_heads 2 is not supported (the kernels take 3)", code=UNSUPPORTED)
    return rows


def test_every_refusal_has_its_code_and_text_and_enqueues_nothing():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import evacuation_amd as ea
    from evacuation_amd import build
    build.build_library()
    box_wrap = dict(positions="rel", statuses="ohe", type="Box")
    handles = {"box": Handle(ea, 3, box_wrap, 4, 6), "grav": Handle(ea, 3, dict(positions="grav"), 2, 2),
               "big": Handle(ea, 65, box_wrap, 1, 6), "tokens": Handle(ea, 63, box_wrap, 1, 6)}
    assert [handles[k].env.obs_dim for k in ("box", "grav", "big", "tokens")] == [30, 6, 402, 390]
    torch.cuda.synchronize()
    before = {k: hd.snapshot() for k, hd in handles.items()}
    lib = handles["box"].env.lib
    calls = 0
    for what, hd, entries, spoil, code, text in table(handles):
        args = {**hd.valid, **spoil(hd.valid)}
        for entry in entries:
            rc = invoke(lib, entry, hd.env._h, args)
            got = (lib.evac_last_error(hd.env._h) or b"").decode()
            assert rc != 0, (what, entry)                # (a call that went through: stop before anything else is tried)
            expected = entry + (text[entry] if isinstance(text, dict) else text)
            assert (rc, got) == (code, expected), (what, entry)
            calls += 1
    assert calls >= 190
    torch.cuda.synchronize()
    for k, hd in handles.items():
        for name, t in hd.snapshot().items():
            assert torch.equal(t, before[k][name]), (k, name)
        hd.env.close()
