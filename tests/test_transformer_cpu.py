"""CPU checks of the transformer leader (evacuation_amd/policy.py TransformerActorCritic, PolicyBinder.transformer,
evac_transformer_t, the routing and the refusals, trainer.autograd_minibatch_grad): the float64 yardstick of the GPU tests
(tests/transformer_ref.py) and the module reproduce the reference's own RPOTransformerEmbedding on the recorded fixture
(tests/golden/transformer_forward.npz, written by tests/golden/make_transformer_forward.py), the binder fills and refuses as
include/evac.h says, everything that cannot take the network says so before a device is looked for, and the compiled kernels
keep to their resources."""
import copy
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.policy import (DeepSetsActorCritic, LinearActorCritic, PolicyBinder, TransformerActorCritic, all_tensors,
                                   is_deepsets, is_transformer, mlp_tensors, transformer_tensors)
from evacuation_amd.trainer import RPOTrainingConfig, autograd_minibatch_grad
from tests import helpers as H
from tests import transformer_ref as TR
from tests.kernel_meta import kernel_resources

# (N, floats per token, use_resid, num_blocks, the actor-critic's width) of the fixture
CASES = ((10, 6, False, 2, 16), (6, 3, False, 1, 16), (4, 2, False, 2, 64), (10, 6, True, 2, 16))
CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(H.GOLDEN, "transformer_forward.npz"))


def state_dict_of(recorded, tag):
    return {k[len(tag) + 4:]: torch.from_numpy(recorded[k]) for k in recorded.files if k.startswith(tag + "/sd/")}


def load_case(recorded, n_ped, dm, use_resid, num_blocks, hidden, sd=None):
    tag = f"n{n_ped}_dm{dm}_r{int(use_resid)}_b{num_blocks}"
    net = TransformerActorCritic((n_ped + 2) * dm, n_ped, num_blocks=num_blocks, use_resid=use_resid, hidden=hidden)
    net.load_state_dict(state_dict_of(recorded, tag) if sd is None else sd, strict=True)     # the reference's attribute names, all of them
    return net, {k: recorded[f"{tag}/{k}"] for k in ("x", "value", "actor_mean", "encoded")}


@pytest.mark.parametrize("n_ped,dm,use_resid,num_blocks,hidden", CASES)
def test_module_reproduces_the_reference_forward(recorded, n_ped, dm, use_resid, num_blocks, hidden):
    """The same torch operations as the reference's module: 1e-6 absolute."""
    net, rec = load_case(recorded, n_ped, dm, use_resid, num_blocks, hidden)
    assert net.token_dim == dm and is_transformer(net) and not is_deepsets(net)
    assert len(all_tensors(net)) == 13 + 16 * num_blocks == len(list(net.parameters()))
    assert {id(t) for t in all_tensors(net)} == {id(t) for t in net.parameters()}
    x = torch.from_numpy(rec["x"])
    with torch.no_grad():
        assert np.abs(net.encode(x).numpy() - rec["encoded"]).max() <= 1e-6
        assert np.abs(net.get_value(x).numpy() - rec["value"]).max() <= 1e-6
        assert np.abs(net.actor_mean(net.encode(x)).numpy() - rec["actor_mean"]).max() <= 1e-6
        torch.manual_seed(0)
        a, lp, ent, v = net.get_action_and_value(x)
        assert a.shape == (8, 2) and lp.shape == (8,) and ent.shape == (8,) and np.abs(v.numpy() - rec["value"]).max() <= 1e-6
        _, lp2, _, _ = net.get_action_and_value(x, a)
        assert torch.equal(lp, lp2)


@pytest.mark.parametrize("n_ped,dm,use_resid,num_blocks,hidden", CASES)
def test_float64_restatement_agrees_to_float32_rounding(recorded, n_ped, dm, use_resid, num_blocks, hidden):
    """|float64 - recorded float32| <= 1e-5 relative to max(1, |v|): the reference module's own float32 error against float64
    on such inputs is at most 1.7e-5 in the encoder with medians at or below 3.6e-6, and at most 5.4e-6 at the outputs; the
    fixture's seeds keep every LayerNorm input variance above 5e-3 (asserted), where the error stays at the low end."""
    net, rec = load_case(recorded, n_ped, dm, use_resid, num_blocks, hidden)
    P = TR.params64(net)
    assert TR.min_norm_variance(P, rec["x"]) >= 5e-3
    for got, want in ((TR.encode(P, rec["x"]), rec["encoded"]), (TR.value(P, rec["x"]), rec["value"][:, 0]),
                      (TR.actor_mean(P, rec["x"]), rec["actor_mean"])):
        scale = max(1.0, float(np.abs(want).max()))
        assert np.abs(got - want).max() <= 1e-5 * scale


def test_the_fixture_sees_both_index_conventions(recorded):
    """Swapping `dense`'s flatten order (c H + h -> h dm + c) or the projections' output order (h dm + c -> c H + h) in a copy of
    the state dict changes the outputs far beyond rounding: the two conventions are visible to the tests above."""
    n_ped, dm, use_resid, num_blocks, hidden = CASES[0]
    tag = f"n{n_ped}_dm{dm}_r{int(use_resid)}_b{num_blocks}"
    net, rec = load_case(recorded, *CASES[0])
    # perm[c H + h] = h dm + c
    perm = torch.tensor([h * dm + c for c in range(dm) for h in range(3)])
    for swap in ("dense", "qkv"):
        sd = {k: v.clone() for k, v in state_dict_of(recorded, tag).items()}
        for b in range(num_blocks):
            if swap == "dense":
                key = f"embedding.{b}.attention.dense.weight"
                sd[key] = sd[key][:, perm].contiguous()
            else:
                for m in ("Wq", "Wk", "Wv"):
                    for part in ("weight", "bias"):
                        key = f"embedding.{b}.attention.{m}.{part}"
                        sd[key] = sd[key][perm].contiguous()
        other, _ = load_case(recorded, *CASES[0], sd=sd)
        P = TR.params64(other)
        assert np.abs(TR.encode(P, rec["x"]) - rec["encoded"]).max() > 1e-2
        assert np.abs(TR.actor_mean(P, rec["x"]) - rec["actor_mean"]).max() > 1e-3
        with torch.no_grad():
            assert np.abs(other.encode(torch.from_numpy(rec["x"])).numpy() - rec["encoded"]).max() > 1e-2


def test_default_encoder_init_is_torchs_and_dropout_defaults_to_zero():
    torch.manual_seed(5)
    net = TransformerActorCritic(72, 10)
    blk = net.embedding[0]
    assert len(net.embedding) == 2 and blk.attention.num_heads == 3 and blk.ff[0].out_features == 96 and not blk.use_resid
    assert blk.attention.Wq.bias.abs().max() > 0 and blk.ff[3].bias.abs().max() > 0         # layer_init would have zeroed them
    assert float(blk.ff[3].weight.detach().abs().max()) <= 1.0 / np.sqrt(96) + 1e-6        # kaiming_uniform(a = sqrt 5): U(+-1 / sqrt fan_in)
    assert net.actor_mean[0].bias.abs().max() == 0                                          # the actor-critic keeps layer_init
    assert [m.p for m in net.embedding.modules() if isinstance(m, torch.nn.Dropout)] == [0.0] * 4
    assert sum(p.numel() for p in blk.parameters()) == 1770
    with pytest.raises(ValueError, match="whole number"):
        TransformerActorCritic(73, 10)


def test_abi_struct_and_symbols():
    assert C.sizeof(_lib.EvacTransformerBlock) == 16 * 8
    assert [f for f, _ in _lib.EvacTransformerBlock._fields_] == ["wq", "bq", "wk", "bk", "wv", "bv", "dense_w", "dense_b", "ff1_w", "ff1_b",
                                                                  "ff2_w", "ff2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b"]
    assert C.sizeof(_lib.EvacTransformer) == 6 * 4 + 2 * 16 * 8
    assert [f for f, _ in _lib.EvacTransformer._fields_] == ["elem_dim", "num_blocks", "num_heads", "dim_feedforward", "use_resid", "ln_eps",
                                                             "blocks"]
    assert _lib.EvacTransformer.ln_eps.offset == 20 and _lib.EvacTransformer.blocks.offset == 24
    header = open(os.path.join(ROOT, "include", "evac.h")).read()
    fields = re.search(r"typedef struct evac_transformer \{(.*?)\} evac_transformer_t;", header, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"\b(\w+)\s*(?:\[2\])?;", fields) == [f for f, _ in _lib.EvacTransformer._fields_]
    for name in ("evac_policy_rollout_transformer", "evac_policy_evaluate_transformer"):
        assert re.search(rf"\bint {name}\(", header) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["evac_policy_rollout_transformer"][1][:-2] == _lib.SIGNATURES["evac_policy_rollout_deepsets"][1][:-2]
    assert _lib.SIGNATURES["evac_policy_evaluate_transformer"][1][:-2] == _lib.SIGNATURES["evac_policy_evaluate_deepsets"][1][:-2]
    assert os.path.join(build.CSRC, "evac_transformer_api.hip") in build.SOURCES
    assert _lib.VERSION == 150


def test_host_side_refusals_need_no_gpu():
    """A NULL handle is refused before anything else."""
    build.build_library()
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    pol, enc = _lib.EvacMlpPolicy(36, 64, *([0x1000] * 13)), _lib.EvacTransformer(3, 1, 3, 96, 0, 1e-5)
    assert lib.evac_policy_rollout_transformer(None, 4, C.byref(pol), *([p] * 11), 0.99, 1.0, 1.0, 1e-8, C.byref(enc), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.evac_policy_evaluate_transformer(None, 0, C.byref(pol), 1, 4, p, p, None, 1.0, 1e-8, C.byref(enc), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.evac_version() == 150


def test_binder_fills_the_struct():
    net = TransformerActorCritic(36, 10, use_resid=True)
    b = PolicyBinder(36, CPU, 10)
    st = b.transformer(net)
    assert (st.elem_dim, st.num_blocks, st.num_heads, st.dim_feedforward, st.use_resid) == (3, 2, 3, 96, 1)
    assert np.float32(st.ln_eps) == np.float32(1e-5)
    ts = transformer_tensors(net)
    assert len(ts) == 32
    for blk in range(2):
        assert [getattr(st.blocks[blk], f) for f, _ in _lib.EvacTransformerBlock._fields_] == [t.data_ptr() for t in ts[16 * blk:16 * blk + 16]]
    assert ts[6] is net.embedding[0].attention.dense.weight and ts[16 + 10] is net.embedding[1].ff[3].weight
    assert b.transformer(net) is st                      # cached by the tensors' identity
    assert b(net).actor_w1 == mlp_tensors(net)[0].data_ptr()
    with torch.no_grad():                                # new tensors are checked again
        net.embedding[1].norm2.bias = torch.nn.Parameter(torch.zeros(3))
    assert b.transformer(net) is not st and b.transformer(net).blocks[1].norm2_b == net.embedding[1].norm2.bias.data_ptr()
    one = TransformerActorCritic(36, 10, num_blocks=1)
    st1 = b.transformer(one)
    assert st1.num_blocks == 1 and st1.use_resid == 0 and st1.blocks[1].wq is None


def test_binder_refusals():
    with pytest.raises(ValueError, match="num_heads 2"):
        PolicyBinder(36, CPU, 10).transformer(TransformerActorCritic(36, 10, num_heads=2))
    with pytest.raises(ValueError, match="dim_feedforward 64"):
        PolicyBinder(36, CPU, 10).transformer(TransformerActorCritic(36, 10, dim_feedforward=64))
    with pytest.raises(ValueError, match="num_blocks 3"):
        PolicyBinder(36, CPU, 10).transformer(TransformerActorCritic(36, 10, num_blocks=3))
    with pytest.raises(ValueError, match="N = 63"):
        PolicyBinder(130, CPU, 63).transformer(TransformerActorCritic(130, 63))
    PolicyBinder(128, CPU, 62).transformer(TransformerActorCritic(128, 62))             # N = 62: the full wave
    with pytest.raises(ValueError, match="whole number of rows"):                       # 36 floats are 12 tokens of 3, not 11 + 2
        PolicyBinder(36, CPU, 11).transformer(TransformerActorCritic(36, 10))
    net = TransformerActorCritic(36, 10)
    net.embedding[1].norm1 = torch.nn.LayerNorm(3, eps=1e-6)
    with pytest.raises(ValueError, match="embedding\\[1\\].norm1` has eps"):
        PolicyBinder(36, CPU, 10).transformer(net)
    for name, owner in (("attention.Wk.weight", lambda blk: (blk.attention.Wk, "weight")), ("ff\\[3\\].bias", lambda blk: (blk.ff[3], "bias")),
                        ("norm2.weight", lambda blk: (blk.norm2, "weight"))):
        for how in ("dtype", "shape"):
            net = TransformerActorCritic(36, 10)
            mod, attr = owner(net.embedding[1])
            t = getattr(mod, attr).detach()
            bad = t.double() if how == "dtype" else torch.zeros(tuple(s + 1 for s in t.shape))
            setattr(mod, attr, torch.nn.Parameter(bad))
            with pytest.raises(ValueError, match="embedding\\[1\\]." + name):
                PolicyBinder(36, CPU, 10).transformer(net)
    with pytest.raises(ValueError, match="embedding\\[0\\].attention.Wq.weight"):      # another device than the binder's
        PolicyBinder(36, torch.device("meta"), 10).transformer(TransformerActorCritic(36, 10))
    net = TransformerActorCritic(36, 10)
    net.embedding = torch.nn.Sequential(torch.nn.Linear(36, 36))
    with pytest.raises(ValueError, match="embedding\\[0\\]` must have"):
        PolicyBinder(36, CPU, 10).transformer(net)


def test_the_reference_module_binds_and_its_state_dict_loads():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_transformer_forward", os.path.join(H.GOLDEN, "make_transformer_forward.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    if not os.path.isdir(gen.NETWORKS):
        pytest.skip("the reference is not present")
    net = gen.make_reference_net(gen.load_networks(), 10, 6, True, 2)
    b = PolicyBinder(72, CPU, 10)
    st = b.transformer(net)
    assert (st.elem_dim, st.num_blocks, st.use_resid) == (6, 2, 1) and b(net).obs_dim == 72
    ours = TransformerActorCritic(72, 10, use_resid=True)
    assert list(ours.state_dict()) == list(net.state_dict())
    ours.load_state_dict(net.state_dict(), strict=True)
    assert len(all_tensors(net)) == 45
    from evacuation_amd.policy import refuse_dropout
    with pytest.raises(ValueError, match="embedding.*dropout p = 0.1"):      # the reference's default dropout: not in collection
        refuse_dropout(net, "policy_rollout")


def _minibatch(D, B, M, seed):
    g = torch.Generator().manual_seed(seed)
    batch = {"b_obs": torch.randn(B, D, generator=g), "b_actions": torch.randn(B, 2, generator=g),
             "b_logprobs": -2.0 + 0.3 * torch.randn(B, generator=g), "b_advantages": torch.randn(B, generator=g),
             "b_returns": torch.randn(B, generator=g), "b_values": torch.randn(B, generator=g)}
    return batch, torch.randperm(B, generator=g)[:M], (torch.rand(M, 2, generator=g) * 2 - 1) * 0.5


def test_everything_that_cannot_take_the_network_says_so():
    """Before any device is looked for, and with `embedding` in the message."""
    from evacuation_amd import trainer as T
    from evacuation_amd.evaluation import PopulationEvaluator
    from evacuation_amd.population import PolicyPopulation, PopulationTrainer, sweep_configs
    from evacuation_amd.vector_env import BatchedEvacuationEnv
    net = TransformerActorCritic(36, 10)
    cfg = RPOTrainingConfig(num_envs=4, num_steps=8, num_minibatches=2)
    env = SimpleNamespace(num_envs=4)
    batch, inds, _ = _minibatch(36, 8, 4, 0)
    perms = torch.arange(8)[None]
    says = "`embedding`"
    calls = {
        "rpo_minibatch_grad": lambda: T.rpo_minibatch_grad(net, batch, inds, cfg),
        "rpo_minibatch_step": lambda: T.rpo_minibatch_step(net, batch, inds, cfg, None),
        "rpo_update": lambda: T.rpo_update(net, batch, perms, cfg, None),
        "deepsets_minibatch_grad": lambda: T.deepsets_minibatch_grad(net, batch, inds, cfg),
        "deepsets_minibatch_step": lambda: T.deepsets_minibatch_step(net, batch, inds, cfg, None),
        "deepsets_update": lambda: T.deepsets_update(net, batch, perms, cfg, None),
        "deepsets_kernel_grad": lambda: T.deepsets_kernel_grad(SimpleNamespace(net=net, cfg=cfg), batch, inds, None, 0, torch.zeros(8)),
        "DeviceAdam": lambda: T.DeviceAdam(net),
        "RPOTrainer device": lambda: T.RPOTrainer(env, net, cfg, optimizer="device"),
        "RPOTrainer device, explicit gradient": lambda: T.RPOTrainer(env, net, cfg, optimizer="device", grad_fn=autograd_minibatch_grad),
        "PolicyPopulation": lambda: PolicyPopulation(36, [1, 2], device="cpu", net=net),
        "PopulationTrainer": lambda: PopulationTrainer(env, net, cfg),
        "sweep_configs": lambda: sweep_configs(cfg, {"learning_rate": [1e-3, 3e-4]}, net=net),
        "policy_rollout_population": lambda: BatchedEvacuationEnv._policy_rollout(None, net, SimpleNamespace(num_learners=2), 4, None, None, None, None),
        "policy_evaluate_population": lambda: BatchedEvacuationEnv.policy_evaluate_population(None, net, 1, 4),
        "PopulationEvaluator": lambda: PopulationEvaluator.evaluate(None, net),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match=says):
            call()
    # the nets that could go there before still can, and still say what they said
    assert len(sweep_configs(cfg, {"learning_rate": [1e-3, 3e-4]}, net=LinearActorCritic(36))) == 2
    with pytest.raises(ValueError, match="`deep_sets`"):
        T.rpo_minibatch_grad(DeepSetsActorCritic(36, 10), batch, inds, cfg)


def test_the_dropout_rule():
    from evacuation_amd import trainer as T
    from evacuation_amd.vector_env import BatchedEvacuationEnv
    cfg = RPOTrainingConfig(num_envs=4, num_steps=8, num_minibatches=2)
    env = SimpleNamespace(num_envs=4)
    wet = TransformerActorCritic(36, 10, dropout=0.1)
    with pytest.raises(ValueError, match="`embedding` has dropout p = 0.1"):
        T.RPOTrainer(env, wet, cfg)
    with pytest.raises(ValueError, match="`embedding` has dropout p = 0.1"):
        BatchedEvacuationEnv._policy_rollout(None, wet, None, 4, None, None, None, None)
    one = TransformerActorCritic(36, 10)
    one.embedding[1].ff[1].p = 0.25                       # one module of the four is enough
    with pytest.raises(ValueError, match="dropout p = 0.25"):
        T.RPOTrainer(env, one, cfg)
    dry = T.RPOTrainer(env, TransformerActorCritic(36, 10), cfg)
    assert dry.grad_fn is autograd_minibatch_grad and isinstance(dry.optimizer, torch.optim.Adam) and len(dry.params) == 45
    # evaluation is eval mode: policy_evaluate's routing binds such a net (the binder has no dropout rule)
    assert PolicyBinder(36, CPU, 10).transformer(wet).num_blocks == 2


def test_kernel_resources():
    """8 kernels under the limits of one 16-wave workgroup per CU.  Scratch: the step's state takes the 128 registers that
    __launch_bounds__(1024) allows, and in two of the eight kernels the compiler keeps two or three loop-invariant dwords of it
    in scratch (8 B and 12 B, measured) -- stored before the step loop and reloaded in its rare reset branch, never inside the
    encoder's loops over j; the sizes are pinned."""
    kernels = kernel_resources("evac_transformer_api.hip")
    short = {re.sub(r"^void ", "", n.split("(")[0]).replace("evac::", "", 1): r for n, r in kernels.items()}
    assert sorted(short) == sorted(f"k_policy_{kind}_transformer<{a}, {b}>" for kind in ("rollout", "evaluate")
                                   for a in ("false", "true") for b in ("false", "true"))
    for name, r in short.items():
        assert r["vgpr_count"] <= 128, (name, r)
    scratch = {name: r["private_segment_fixed_size"] for name, r in short.items() if r["private_segment_fixed_size"]}
    assert scratch == {"k_policy_rollout_transformer<false, false>": 8, "k_policy_evaluate_transformer<true, false>": 12}
    assert len(kernel_resources("evac_deepsets_api.hip")) == 8            # evac_deepsets_api.hip's own kernels are as they were


def test_static_lds_fits_a_cu():
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "evac.s")
        flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
        subprocess.run([build.hipcc_path()] + flags + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "evac_transformer_api.hip"), "-o", out],
                       check=True, capture_output=True)
        sizes = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", open(out).read())]
    assert len(sizes) == 8 and max(sizes) <= 163840


def test_autograd_gradient_of_all_45_tensors_against_float64():
    """1e-4 of each tensor's largest gradient: LayerNorm over 6 values amplifies float32 rounding by 1 / sqrt(variance).
    The key bias `attention.Wk.bias` is the exception that the function itself makes: it adds the same number to every score of
    a softmax row, so its exact gradient is ZERO (float64 gives 1e-19) and float32 leaves the rounding of a sum of cancelling
    terms -- the terms of `attention.Wk.weight`'s gradient with the token's value replaced by 1.  Its scale is therefore that
    weight's largest gradient, and the test asserts that float64 finds the zero."""
    torch.manual_seed(2)
    net = TransformerActorCritic(72, 10)
    with torch.no_grad():
        net.actor_mean[4].weight.mul_(60.0)
        for m in net.embedding.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.3)
    cfg = RPOTrainingConfig(num_envs=4, num_steps=64, num_minibatches=4)
    batch, inds, z = _minibatch(72, 256, 64, 4)
    stats = autograd_minibatch_grad(SimpleNamespace(net=net, cfg=cfg), batch, inds, z, 0, torch.zeros(8))
    assert stats.shape == (8,) and torch.isfinite(stats).all()
    grads = [t.grad for t in all_tensors(net)]
    assert len(grads) == 45 and all(g is not None and torch.isfinite(g).all() for g in grads)
    assert sum(bool(g.abs().max() > 1e-8) for g in grads) == 43               # (all but the two key biases, below)
    assert abs(float(stats[7]) - sum(float((g.double() ** 2).sum()) for g in grads)) <= 1e-6 * float(stats[7])
    net64 = copy.deepcopy(net).double()
    for p in net64.parameters():
        p.grad = None
    batch64 = {k: v.double() for k, v in batch.items()}
    stats64 = autograd_minibatch_grad(SimpleNamespace(net=net64, cfg=cfg), batch64, inds, z.double(), 0, torch.zeros(8, dtype=torch.float64))
    assert torch.allclose(stats[:6].double(), stats64[:6], rtol=1e-4, atol=1e-5)
    grads64 = [t.grad for t in all_tensors(net64)]
    key_bias = [13 + 16 * blk + 3 for blk in range(2)]
    for i, (g, g64) in enumerate(zip(grads, grads64)):
        scale = float(g64.abs().max())
        if i in key_bias:
            assert all_tensors(net)[i] is net.embedding[(i - 13) // 16].attention.Wk.bias
            assert scale <= 1e-12 * float(grads64[i - 1].abs().max())
            scale = float(grads64[i - 1].abs().max())
        assert float((g.double() - g64).abs().max()) <= 1e-4 * scale, i
