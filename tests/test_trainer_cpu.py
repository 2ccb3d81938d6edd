"""CPU checks of the trainer's update (evac_gae, evac_rpo_minibatch_grad, evacuation_amd/trainer.py): the entry points are
exported, bound and validate their arguments on the host with no GPU present; the torch yardstick of the GPU tests
(tests/trainer_ref.py) agrees with the reference's own network where the reference is present; RPOTrainingConfig has the
reference's defaults and derived sizes."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import pytest
import torch

from evacuation_amd import _lib, build
from evacuation_amd.policy import LinearActorCritic
from evacuation_amd.trainer import RPOTrainingConfig
from tests import trainer_ref as R

REFERENCE = "/root/reference/src"


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_trainer_symbols_are_exported_and_bound(lib):
    for name, nargs in (("evac_gae", 12), ("evac_rpo_workspace_bytes", 2), ("evac_rpo_minibatch_grad", 18)):
        assert name in _lib.SIGNATURES
        assert len(getattr(lib, name).argtypes) == nargs
    assert C.sizeof(_lib.EvacRpoLossConfig) == 24 and C.sizeof(_lib.EvacMlpPolicyGrads) == 13 * 8
    assert [f for f, _ in _lib.EvacMlpPolicyGrads._fields_] == [f for f, _ in _lib.EvacMlpPolicy._fields_[2:]]


def test_host_side_validation_needs_no_gpu(lib):
    """Every refusal comes before anything touches a device (the pointers here are never followed)."""
    bad = _lib.ERR_INVALID_ARGUMENT
    p = 0x1000                       # a non-NULL address
    ok = [8, 4, p, p, p, p, p, 0.99, 0.95, p, p, None]
    for i in (2, 3, 4, 5, 6, 9, 10):
        a = list(ok)
        a[i] = None
        assert lib.evac_gae(*a) == bad, i
    assert lib.evac_gae(0, 4, *ok[2:]) == bad and lib.evac_gae(-1, 4, *ok[2:]) == bad and lib.evac_gae(8, 0, *ok[2:]) == bad
    assert lib.evac_gae(8, -4, *ok[2:]) == bad
    assert lib.evac_rpo_workspace_bytes(0, 64) == bad and lib.evac_rpo_workspace_bytes(397, 64) == bad
    assert lib.evac_rpo_workspace_bytes(6, 0) == bad and lib.evac_rpo_workspace_bytes(6, -1) == bad
    small, big = lib.evac_rpo_workspace_bytes(6, 64), lib.evac_rpo_workspace_bytes(396, 16384)
    assert 0 < small < big and big >= 2 * 16384 * 64 * 4

    def call(pol=None, cfg=None, grads=None, B=128, M=64, ptrs=None, inds=p, stats=p, ws=p):
        pol = pol or _lib.EvacMlpPolicy(6, 64, *([p] * 13))
        cfg = cfg or _lib.EvacRpoLossConfig(0.2, 0.0, 0.5, 0.5, 1, 1)
        grads = grads or _lib.EvacMlpPolicyGrads(*([p] * 13))
        ptrs = ptrs or [p] * 6
        return lib.evac_rpo_minibatch_grad(C.byref(pol), C.byref(cfg), B, *ptrs, M, inds, None, 0, 0, C.byref(grads), stats, ws, None)

    assert lib.evac_rpo_minibatch_grad(None, None, 1, *([None] * 6), 1, None, None, 0, 0, None, None, None, None) == bad
    assert call(pol=_lib.EvacMlpPolicy(6, 32, *([p] * 13))) == bad                      # hidden != 64
    assert call(pol=_lib.EvacMlpPolicy(0, 64, *([p] * 13))) == bad and call(pol=_lib.EvacMlpPolicy(397, 64, *([p] * 13))) == bad
    assert call(pol=_lib.EvacMlpPolicy(6, 64, *([p] * 12 + [None]))) == bad
    assert call(grads=_lib.EvacMlpPolicyGrads(*([None] + [p] * 12))) == bad
    assert call(M=1) == bad                                                             # norm_adv: the std of one sample
    assert call(M=0) == bad and call(M=-5) == bad and call(B=0) == bad and call(B=-1) == bad
    for i in range(6):
        ptrs = [p] * 6
        ptrs[i] = None
        assert call(ptrs=ptrs) == bad, i
    assert call(inds=None) == bad and call(stats=None) == bad and call(ws=None) == bad and call(ws=p + 4) == bad


def test_training_config_has_the_reference_defaults_and_sizes():
    c = RPOTrainingConfig()
    assert (c.seed, c.total_timesteps, c.learning_rate, c.num_envs, c.num_steps, c.anneal_lr) == (1, 80000000, 3e-4, 3, 2048, True)
    assert (c.gamma, c.gae_lambda, c.num_minibatches, c.update_epochs, c.norm_adv, c.clip_coef, c.clip_vloss) == (0.99, 0.95, 32, 10, True, 0.2, True)
    assert (c.ent_coef, c.vf_coef, c.max_grad_norm, c.target_kl, c.rpo_alpha) == (0.0, 0.5, 0.5, None, 0.5)
    assert (c.batch_size, c.minibatch_size, c.num_updates) == (6144, 192, 80000000 // 6144)
    src = os.path.join(REFERENCE, "agents", "rpo_agent.py")
    if os.path.exists(src):          # the reference's own defaults, read from its dataclass without importing its dependencies
        import ast
        cls = next(n for n in ast.parse(open(src).read()).body if isinstance(n, ast.ClassDef) and n.name == "RPOAgentTrainingConfig")
        ref = {n.target.id: ast.literal_eval(n.value) for n in cls.body if isinstance(n, ast.AnnAssign) and n.value is not None}
        assert len(ref) >= 20
        for f, v in ref.items():
            assert getattr(c, f) == v, f
    with pytest.raises(ValueError):
        RPOTrainingConfig(num_envs=1, num_steps=4, num_minibatches=4).check()           # minibatches of one sample with norm_adv
    RPOTrainingConfig(num_envs=1, num_steps=4, num_minibatches=4, norm_adv=False).check()
    lc = RPOTrainingConfig(ent_coef=0.01).loss_config()
    assert (round(lc.clip_coef, 6), round(lc.ent_coef, 6), lc.vf_coef, lc.rpo_alpha, lc.norm_adv, lc.clip_vloss) == (0.2, 0.01, 0.5, 0.5, 1, 1)


def _reference_network(obs_dim, alpha):
    path = os.path.join(REFERENCE, "agents", "networks", "rpo_linear_agent_network.py")
    if not os.path.exists(path):
        pytest.skip("the reference is not present")
    import importlib.util
    import types
    pkg = types.ModuleType("refnets")
    pkg.__path__ = [os.path.dirname(path)]
    sys.modules["refnets"] = pkg
    try:
        spec = importlib.util.spec_from_file_location("refnets.rpo_linear_agent_network", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
    finally:
        sys.modules.pop("refnets", None)
    envs = SimpleNamespace(single_observation_space=SimpleNamespace(shape=(obs_dim,)), single_action_space=SimpleNamespace(shape=(2,)))
    return mod.RPOLinearNetwork(envs, mod.RPOLinearNetworkConfig(rpo_alpha=alpha), torch.device("cpu"))


@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_yardstick_equals_the_reference_network(alpha):
    """get_action_and_value(x, action) of the reference under a seed == the yardstick with z drawn by the same call after the same
    seed, bit for bit on the CPU; and z is a constant for the gradient."""
    torch.manual_seed(3)
    net = _reference_network(6, alpha)
    with torch.no_grad():
        net.actor_logstd.uniform_(-0.5, 0.3)
    x, act = torch.randn(37, 6), torch.randn(37, 2)
    torch.manual_seed(11)
    _, lp_ref, ent_ref, v_ref = net.get_action_and_value(x, act)
    torch.manual_seed(11)
    z = torch.FloatTensor(37, 2).uniform_(-alpha, alpha)
    P = R.params_of(net)
    lp, ent, v = R.logprob_entropy_value(P, x, act, z)
    assert torch.equal(lp, lp_ref) and torch.equal(ent, ent_ref) and torch.equal(v, v_ref)
    assert alpha == 0.0 or float(z.abs().max()) > 0.1
    # the gradient with z a constant == the reference's (its z never required grad)
    w = torch.randn(37)
    g_ref = torch.autograd.grad((lp_ref * w).sum() + v_ref.sum(), list(R.mlp_tensors(net)))
    g = torch.autograd.grad((lp * w).sum() + v.sum(), P)
    for a, b in zip(g, g_ref):
        assert torch.equal(a, b)


def test_yardstick_gae_float32_against_float64():
    g = torch.Generator().manual_seed(5)
    T, E = 200, 50
    r, v = torch.randn(T, E, generator=g), torch.randn(T, E, generator=g)
    d = (torch.rand(T, E, generator=g) < 0.03).float()
    d[T // 2, 0] = 1.0
    d[T - 1, 1] = 1.0
    nv, nd = torch.randn(E, generator=g), torch.zeros(E)
    nd[2] = 1.0
    a32, r32 = R.gae(r, v, d, nv, nd, 0.99, 0.95)
    a64, r64 = R.gae(r.double(), v.double(), d.double(), nv.double(), nd.double(), 0.99, 0.95)
    assert a32.dtype == torch.float32 and a64.dtype == torch.float64
    assert float((a32 - a64).abs().max()) <= 1e-5 * float(a64.abs().max())
    assert float((r32 - r64).abs().max()) <= 1e-5 * float(r64.abs().max())
    # a done cuts the recursion: the advantage before it does not see what follows
    v2 = v.clone()
    v2[T // 2 + 1:, 0] += 7.0
    a2, _ = R.gae(r, v2, d, nv, nd, 0.99, 0.95)
    assert torch.equal(a2[:T // 2, 0], a32[:T // 2, 0])


def test_yardstick_loss_takes_every_branch():
    """The loss of LinearActorCritic through the yardstick == the same lines through the module's own get_action_and_value
    (alpha = 0), in float64, for all four switch combinations."""
    torch.manual_seed(0)
    net = LinearActorCritic(6).double()
    B = 256
    batch = {"b_obs": torch.randn(B, 6).double(), "b_actions": torch.randn(B, 2).double(), "b_logprobs": -2.0 + 0.3 * torch.randn(B).double(),
             "b_advantages": torch.randn(B).double(), "b_returns": torch.randn(B).double(), "b_values": torch.randn(B).double()}
    inds = torch.randperm(B)[:100]
    for norm_adv in (False, True):
        for clip_vloss in (False, True):
            cfg = SimpleNamespace(clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, norm_adv=norm_adv, clip_vloss=clip_vloss)
            t = R.loss_terms(R.params_of(net), batch, inds, cfg, torch.zeros(100, 2).double())
            _, lp, ent, val = net.get_action_and_value(batch["b_obs"][inds], batch["b_actions"][inds])
            ratio = (lp - batch["b_logprobs"][inds]).exp()
            assert torch.allclose(t.ratio, ratio.detach(), rtol=1e-12, atol=0)
            assert 0.0 < float(t.clipfrac) < 1.0 and torch.isfinite(t.loss)
            assert abs(float(t.entropy) - float(ent.mean())) < 1e-12
