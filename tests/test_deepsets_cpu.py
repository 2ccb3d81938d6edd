"""CPU checks of the deep-sets leader (evacuation_amd/policy.py DeepSetsActorCritic, PolicyBinder.encoder, evac_deepsets_t,
trainer.autograd_minibatch_grad): the module reproduces the reference's own RPODeepSetsEmbedding on the recorded fixture
(tests/golden/deepsets_forward.npz, written by tests/golden/make_deepsets_forward.py), the float64 yardstick of the GPU tests
(tests/deepsets_ref.py) agrees with it, the binder fills and refuses as include/evac.h says, and the autograd gradient agrees
with the trainer's yardstick (tests/trainer_ref.py) on the linear network."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.policy import (SET_HIDDEN, DeepSetsActorCritic, LinearActorCritic, PolicyBinder, all_tensors, deepsets_tensors,
                                   is_deepsets, mlp_tensors)
from evacuation_amd.trainer import RPOTrainingConfig, autograd_minibatch_grad
from tests import deepsets_ref as DR
from tests import helpers as H
from tests import trainer_ref as R

CASES = ((10, 6, 16), (6, 3, 16), (4, 2, 64))     # (N, floats per element, the actor-critic's width) of the fixture
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(H.GOLDEN, "deepsets_forward.npz"))


def load_case(recorded, n_ped, ed, hidden):
    tag = f"n{n_ped}_ed{ed}"
    net = DeepSetsActorCritic((n_ped + 2) * ed, n_ped, hidden=hidden)
    sd = {k[len(tag) + 4:]: torch.from_numpy(recorded[k]) for k in recorded.files if k.startswith(tag + "/sd/")}
    net.load_state_dict(sd, strict=True)           # the reference's attribute names, all of them
    return net, {k: recorded[f"{tag}/{k}"] for k in ("x", "value", "actor_mean", "encoded")}


@pytest.mark.parametrize("n_ped,ed,hidden", CASES)
def test_module_reproduces_the_reference_forward_exactly(recorded, n_ped, ed, hidden):
    net, rec = load_case(recorded, n_ped, ed, hidden)
    assert net.set_element_dim == ed and is_deepsets(net) and len(all_tensors(net)) == 19
    x = torch.from_numpy(rec["x"])
    with torch.no_grad():
        assert np.array_equal(net.encode(x).numpy(), rec["encoded"])
        assert np.array_equal(net.get_value(x).numpy(), rec["value"])
        assert np.array_equal(net.actor_mean(net.encode(x)).numpy(), rec["actor_mean"])
        torch.manual_seed(0)
        a, lp, ent, v = net.get_action_and_value(x)
        assert a.shape == (8, 2) and lp.shape == (8,) and ent.shape == (8,) and np.array_equal(v.numpy(), rec["value"])
        _, lp2, _, _ = net.get_action_and_value(x, a)
        assert torch.equal(lp, lp2)


@pytest.mark.parametrize("n_ped,ed,hidden", CASES)
def test_float64_restatement_agrees_to_float32_rounding(recorded, n_ped, ed, hidden):
    """|float64 - recorded float32|: the recorded sums have at most 66 x 24 terms of magnitude <= ~10; 1e-5 relative to the
    outputs' scale is some 50 float32 roundings of room."""
    net, rec = load_case(recorded, n_ped, ed, hidden)
    P = DR.params64(net)
    for got, want in ((DR.encode(P, rec["x"]), rec["encoded"]), (DR.value(P, rec["x"]), rec["value"][:, 0]),
                      (DR.actor_mean(P, rec["x"]), rec["actor_mean"])):
        scale = max(1.0, float(np.abs(want).max()))
        assert np.abs(got - want).max() <= 1e-5 * scale


def test_default_encoder_init_is_torchs_not_layer_init():
    torch.manual_seed(5)
    net = DeepSetsActorCritic(72, 10)
    phi = net.deep_sets.transform_phi
    assert phi[0].bias.abs().max() > 0 and phi[2].bias.abs().max() > 0             # layer_init would have zeroed them
    assert float(phi[2].weight.detach().abs().max()) <= 1.0 / np.sqrt(SET_HIDDEN) + 1e-6    # kaiming_uniform(a = sqrt 5): U(+-1 / sqrt fan_in)
    assert net.actor_mean[0].bias.abs().max() == 0                                  # the actor-critic keeps layer_init


def test_binder_fills_the_struct():
    assert C.sizeof(_lib.EvacDeepSets) == 8 + 6 * 8
    assert [f for f, _ in _lib.EvacDeepSets._fields_] == ["set_elem_dim", "hidden", "phi_w1", "phi_b1", "phi_w2", "phi_b2", "rho_w", "rho_b"]
    net = DeepSetsActorCritic(36, 10)
    b = PolicyBinder(36, CPU, 10)
    st = b.encoder(net)
    assert (st.set_elem_dim, st.hidden) == (3, 24)
    assert [getattr(st, f) for f, _ in _lib.EvacDeepSets._fields_[2:]] == [t.data_ptr() for t in deepsets_tensors(net)]
    assert b.encoder(net) is st                      # cached by the tensors' identity
    pol = b(net)
    assert (pol.obs_dim, pol.hidden, pol.actor_w1) == (36, 64, mlp_tensors(net)[0].data_ptr())
    with torch.no_grad():                            # new tensors are checked again
        net.deep_sets.transform_rho[0].weight = torch.nn.Parameter(torch.zeros(36, 24))
    assert b.encoder(net) is not st and b.encoder(net).rho_w == net.deep_sets.transform_rho[0].weight.data_ptr()


def test_binder_refusals():
    def fresh():
        return DeepSetsActorCritic(36, 10)
    with pytest.raises(ValueError, match="dim_hidden 16"):
        PolicyBinder(36, CPU, 10).encoder(DeepSetsActorCritic(36, 10, dim_hidden=16))
    with pytest.raises(ValueError, match="whole number"):
        DeepSetsActorCritic(37, 10)
    with pytest.raises(ValueError, match="whole number of rows"):        # 36 floats are 12 rows of 3, not 11 + 2
        PolicyBinder(36, CPU, 11).encoder(fresh())
    with pytest.raises(ValueError, match="whole number of rows"):        # the gravity observation's 6 floats under a 4-float element
        net = DeepSetsActorCritic(8, 0)
        PolicyBinder(6, CPU).encoder(net)
    for index, name in ((0, "transform_phi\\[0\\].weight"), (3, "transform_phi\\[2\\].bias"), (4, "transform_rho\\[0\\].weight"),
                        (5, "transform_rho\\[0\\].bias")):
        owner = [(0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"), (0, "weight"), (0, "bias")][index]
        seq = "transform_phi" if index < 4 else "transform_rho"
        for how in ("dtype", "shape", "contiguity"):
            net = fresh()
            mod = getattr(net.deep_sets, seq)[owner[0]]
            t = getattr(mod, owner[1]).detach()
            if how == "dtype":
                bad = t.double()
            elif how == "shape":
                bad = torch.zeros(tuple(s + 1 for s in t.shape))
            else:
                if t.dim() < 2:
                    continue
                bad = torch.zeros(t.shape[1], t.shape[0]).t()
            setattr(mod, owner[1], torch.nn.Parameter(bad))
            with pytest.raises(ValueError, match=name):
                PolicyBinder(36, CPU, 10).encoder(net)
    with pytest.raises(ValueError, match="transform_phi\\[0\\].weight"):       # another device than the binder's
        PolicyBinder(36, torch.device("meta"), 10).encoder(fresh())
    net = fresh()
    net.deep_sets.transform_phi = torch.nn.Sequential(torch.nn.Linear(3, 24), torch.nn.Tanh(), torch.nn.Linear(24, 24))
    with pytest.raises(ValueError, match="Sequential\\(Linear, ReLU, Linear\\)"):
        PolicyBinder(36, CPU, 10).encoder(net)


def test_the_reference_module_binds():
    path = "/root/reference/src/agents/networks"
    if not os.path.isdir(path):
        pytest.skip("the reference is not present")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_deepsets_forward", os.path.join(H.GOLDEN, "make_deepsets_forward.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    mods = gen.load_networks()
    lin, ds = mods["rpo_linear_agent_network"], mods["rpo_deep_sets_agent_network"]
    envs = SimpleNamespace(single_observation_space=SimpleNamespace(shape=(72,)), single_action_space=SimpleNamespace(shape=(2,)))
    net = ds.RPODeepSetsEmbedding(envs, 10, ds.RPODeepSetsEmbeddingConfig(network=lin.RPOLinearNetworkConfig()), CPU)
    b = PolicyBinder(72, CPU, 10)
    assert b.encoder(net).set_elem_dim == 6 and b(net).obs_dim == 72
    ours = DeepSetsActorCritic(72, 10)
    assert list(ours.state_dict()) == list(net.state_dict())


def test_host_side_refusals_need_no_gpu():
    """A NULL handle is refused before anything else; the symbols are bound with the existing entries' arguments plus one."""
    build.build_library()
    lib = _lib.load()
    assert len(lib.evac_policy_rollout_deepsets.argtypes) == len(lib.evac_policy_rollout.argtypes) + 1
    assert len(lib.evac_policy_evaluate_deepsets.argtypes) == len(lib.evac_policy_evaluate.argtypes) + 1
    p = C.c_void_p(0x1000)
    pol, enc = _lib.EvacMlpPolicy(36, 64, *([0x1000] * 13)), _lib.EvacDeepSets(3, 24, *([0x1000] * 6))
    assert lib.evac_policy_rollout_deepsets(None, 4, C.byref(pol), *([p] * 11), 0.99, 1.0, 1.0, 1e-8, C.byref(enc), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.evac_policy_evaluate_deepsets(None, 0, C.byref(pol), 1, 4, p, p, None, 1.0, 1e-8, C.byref(enc), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.evac_version() == 150


def test_device_optimiser_and_populations_refuse_the_encoder():
    from evacuation_amd.population import PolicyPopulation, PopulationTrainer, sweep_configs
    from evacuation_amd.trainer import RPOTrainer, rpo_minibatch_grad
    net = DeepSetsActorCritic(36, 10)
    cfg = RPOTrainingConfig(num_envs=4, num_steps=8, num_minibatches=2)
    env = SimpleNamespace(num_envs=4)
    says = "gradient and optimiser kernels are the linear network's"
    with pytest.raises(ValueError, match=says):
        RPOTrainer(env, net, cfg, optimizer="device")
    with pytest.raises(ValueError, match=says):
        PolicyPopulation(36, [1, 2], device="cpu", net=net)
    with pytest.raises(ValueError, match=says):
        PopulationTrainer(env, net, cfg)
    with pytest.raises(ValueError, match=says):
        sweep_configs(cfg, {"learning_rate": [1e-3, 3e-4]}, net=net)
    with pytest.raises(ValueError, match=says):
        rpo_minibatch_grad(net, {"b_obs": torch.zeros(8, 36)}, torch.arange(4), cfg)
    assert len(sweep_configs(cfg, {"learning_rate": [1e-3, 3e-4]}, net=LinearActorCritic(36))) == 2


def _minibatch(D, B, M, seed):
    g = torch.Generator().manual_seed(seed)
    batch = {"b_obs": torch.randn(B, D, generator=g), "b_actions": torch.randn(B, 2, generator=g),
             "b_logprobs": -2.0 + 0.3 * torch.randn(B, generator=g), "b_advantages": torch.randn(B, generator=g),
             "b_returns": torch.randn(B, generator=g), "b_values": torch.randn(B, generator=g)}
    return batch, torch.randperm(B, generator=g)[:M], (torch.rand(M, 2, generator=g) * 2 - 1) * 0.5


@pytest.mark.parametrize("clip_vloss,norm_adv", [(True, True), (False, False)])
def test_autograd_gradient_on_the_linear_network_against_the_yardstick(clip_vloss, norm_adv):
    """The bound is the yardstick's own error: trainer_ref in float32 against trainer_ref in float64 on the same minibatch, per
    tensor relative to the tensor's largest gradient entry (and per statistic, relative to max(1, |value|)); autograd on the
    module orders its sums differently, so it gets 4x that."""
    torch.manual_seed(11)
    net = LinearActorCritic(36)
    with torch.no_grad():
        net.actor_mean[4].weight.mul_(30.0)
        net.actor_logstd.copy_(torch.tensor([[-0.4, 0.2]]))
    cfg = RPOTrainingConfig(num_envs=4, num_steps=64, num_minibatches=4, clip_vloss=clip_vloss, norm_adv=norm_adv, ent_coef=0.01)
    batch, inds, z = _minibatch(36, 256, 64, 3)
    g32, s32, _ = R.minibatch_grad(net, batch, inds, cfg, z, torch.float32)
    g64, s64, _ = R.minibatch_grad(net, batch, inds, cfg, z, torch.float64)
    stats = torch.zeros(8)
    out = autograd_minibatch_grad(SimpleNamespace(net=net, cfg=cfg), batch, inds, z, 0, stats)
    assert out is stats
    own = [t.grad for t in mlp_tensors(net)]
    ref_err = got_err = 0.0
    for a, b32, b64 in zip(own, g32, g64):
        scale = float(b64.abs().max()) or 1.0
        ref_err = max(ref_err, float((b32.double() - b64).abs().max()) / scale)
        got_err = max(got_err, float((a.double() - b64).abs().max()) / scale)
    scale = torch.clamp(s64.abs(), min=1.0)
    ref_stat = float(((s32.double() - s64).abs() / scale).max())
    got_stat = float(((stats.double() - s64).abs() / scale).max())
    print(f"gradients: trainer_ref f32 vs f64 {ref_err:.3e}, autograd vs f64 {got_err:.3e}; "
          f"statistics: {ref_stat:.3e}, {got_stat:.3e}")
    assert ref_err > 0 and ref_stat > 0
    assert got_err <= 4 * ref_err and got_stat <= 4 * ref_stat
    # written, not accumulated; and the drawn perturbation is a function of (seed, draw counter)
    autograd_minibatch_grad(SimpleNamespace(net=net, cfg=cfg), batch, inds, z, 0, stats)
    assert all(torch.equal(a, t.grad) for a, t in zip(own, mlp_tensors(net)))
    t = SimpleNamespace(net=net, cfg=cfg)
    s1 = autograd_minibatch_grad(t, batch, inds, None, 7, torch.zeros(8)).clone()
    s2 = autograd_minibatch_grad(t, batch, inds, None, 7, torch.zeros(8))
    s3 = autograd_minibatch_grad(t, batch, inds, None, 8, torch.zeros(8))
    assert torch.equal(s1, s2) and not torch.equal(s1, s3)


def test_autograd_gradient_reaches_the_encoder():
    torch.manual_seed(2)
    net = DeepSetsActorCritic(36, 10)
    cfg = RPOTrainingConfig(num_envs=4, num_steps=64, num_minibatches=4)
    batch, inds, z = _minibatch(36, 256, 64, 4)
    stats = autograd_minibatch_grad(SimpleNamespace(net=net, cfg=cfg), batch, inds, z, 0, torch.zeros(8))
    assert torch.isfinite(stats).all()
    grads = [t.grad for t in all_tensors(net)]
    assert len(grads) == 19 and all(g is not None and g.abs().max() > 0 for g in grads)
    assert abs(float(stats[7]) - sum(float((g.double() ** 2).sum()) for g in grads)) <= 1e-6 * float(stats[7])
