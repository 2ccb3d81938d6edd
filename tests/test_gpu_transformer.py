"""The transformer leader (evac_policy_rollout_transformer, evac_policy_evaluate_transformer; policy.TransformerActorCritic through
BatchedEvacuationEnv / NormalizedVectorEnv.policy_rollout / policy_evaluate, PolicyEvaluator, RPOTrainer) on an MI355X.

1. Policy outputs, teacher-forced on the recorded observations, against the float64 restatement (tests/transformer_ref.py).  The
   bound of a case is 8 x the largest error of the module's OWN float32 torch forward (CPU) against float64 on those same
   observations, per quantity, with a floor of 1e-5 (test_gpu_deepsets.py's rule).  Both figures are printed.  Precondition,
   asserted on the recorded observations: the smallest LayerNorm input variance of the float64 restatement, across both norms of
   every block, is at least 1e-4 -- below that LayerNorm divides by nearly nothing and no float32 forward is comparable with
   another.  A case that misses it gets another net seed (NET_SEEDS), never another bound.
2. The env side, bit for bit: a twin handle (subwave = 0) replays the recorded actions through step().
3. Invariance: T = 33 == 7 + 26, two runs, E = 20 == the first 20 envs of E = 64.
4. Evaluation: sample mode == the rollout, mean mode == the rollout with sigma = 0, max_steps = 17 repeated == one call, a frozen
   norm_state is only read.
5. An encoder that matters: other outputs than the linear entry's on the same x; attention without positions is equivariant
   under a permutation of the pedestrian tokens (float64 restatement: the output rows permute; device: with an actor first layer
   whose weights repeat from token to token the mean action does not move, through policy_rollout and policy_evaluate).
6. RPOTrainer with the net.  7. The C ABI's refusals.  8. examples/train_rpo.py --network transformer."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.encoder_cases import EncoderCases, _frozen, ea, rel_err  # noqa: F401 (ea: the fixture)
from tests.test_gpu_policy_rollout import OFFSET, SEED, base, i32, raw, replay_env_side, snapshot, start

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {
    # name: (EnvConfig kwargs, EnvWrappersConfig kwargs, normalised chain, KernelOptions overrides, the net's keyword arguments)
    "n62_rel_ohe_box_norm_clip": (dict(number_of_pedestrians=62, max_timesteps=25, clip_action=True),
                                  dict(positions="rel", statuses="ohe", type="Box"), True, {}, {}),      # S = 64: the full wave
    "n60_rel_ohe_box_raw_resid": (dict(number_of_pedestrians=60, max_timesteps=25), dict(positions="rel", statuses="ohe", type="Box"),
                                  False, {}, dict(use_resid=True)),                                      # S = 62: two idle lanes
    "n60_rel_ohe_box_raw_resid_generic": (dict(number_of_pedestrians=60, max_timesteps=25),
                                          dict(positions="rel", statuses="ohe", type="Box"), False, dict(specialize=0),
                                          dict(use_resid=True)),                                         # the non-DEF kernels
    "n10_abs_cat_box_raw": (dict(number_of_pedestrians=10, max_timesteps=20, intrinsic_reward_coef=0.5),
                            dict(positions="abs", statuses="cat", type="Box"), False, {}, dict(num_blocks=1)),   # 3 floats per token
    "n31_rel_no_box_norm": (dict(number_of_pedestrians=31, max_timesteps=22, enslaving_degree=0.7),
                            dict(positions="rel", statuses="no", type="Box"), True, {}, {}),             # 2 floats, 33 tokens
}
# the seed of each case's net (make_net): one for which the recorded observations meet the variance precondition of test 1
NET_SEEDS = {"n62_rel_ohe_box_norm_clip": 0, "n60_rel_ohe_box_raw_resid": 0, "n60_rel_ohe_box_raw_resid_generic": 0,
             "n10_abs_cat_box_raw": 1, "n31_rel_no_box_norm": 1}
# ... and for the rollouts of tests/test_gpu_policy_long.py (150 steps at max_timesteps = 70; 3 envs x 2048 steps at 700)
LONG_NET_SEEDS = {"n62_rel_ohe_box_norm_clip": 0, "n10_abs_cat_box_raw": 1}
MIN_NORM_VARIANCE = 1e-4
T_STEPS = 40


def token_dim(case):
    return 2 + {"ohe": 4, "cat": 1, "no": 0}[CASES[case][1]["statuses"]]


def make_net(case, seed=None, device="cuda:0"):
    """A transformer leader with visible actions and values (test_gpu_policy_rollout.make_net's recipe) and LayerNorm weights
    and biases away from their defaults of 1 and 0."""
    import torch
    from evacuation_amd.policy import TransformerActorCritic
    N = CASES[case][0]["number_of_pedestrians"]
    torch.manual_seed(NET_SEEDS[case] if seed is None else seed)
    net = TransformerActorCritic((N + 2) * token_dim(case), N, **CASES[case][4])
    with torch.no_grad():
        net.actor_mean[4].weight.mul_(60.0)
        net.actor_logstd.copy_(torch.tensor([[-0.5, 0.3]]))
        for m in list(net.actor_mean) + list(net.critic):
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.2)
        for m in net.embedding.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.3)
    return net.to(device)


_cases = EncoderCases(CASES, make_net, T_STEPS)
make_env, rollout_of, _run, _twins = _cases.make_env, _cases.rollout_of, _cases.run, _cases.twins


def check_policy_outputs_teacher_forced(cases, ea, case, E):
    """Test 1 on the shared rollout of ``cases`` (an EncoderCases of this file's CASES and make_net)."""
    import torch
    from torch.distributions.normal import Normal
    from tests import policy_ref as R
    from tests import transformer_ref as TR
    net, ro, _, total0, _, _ = cases.rollout_of(ea, case, E)
    P = TR.params64(net)
    cpu = copy.deepcopy(net).to("cpu")
    obs, act = ro["obs"].cpu().double().numpy(), ro["actions"].cpu().double().numpy()
    lp, val = ro["logprobs"].cpu().double().numpy(), ro["values"].cpu().double().numpy()
    next_obs = ro["next_obs"].cpu().double().numpy()
    variances = []
    y64, next_y64 = TR.encode(P, obs, variances), TR.encode(P, next_obs, variances)     # (one float64 pass serves both uses)
    least = min(variances)
    print(f"\n{case} E={E}: smallest LayerNorm input variance {least:.3e}")
    assert least >= MIN_NORM_VARIANCE, (case, E, least)
    sd = np.exp(P["logstd"])
    T = obs.shape[0]
    z = cases.policy_noise(total0, T)
    mean64, act64, lp64, val64 = R.policy_step(P, y64, z)
    nv64 = R.value(P, next_y64)
    # the yardstick's own float32 error: the module's torch forward on the CPU, on the same observations (and, for the
    # log-probability, the same recorded actions)
    with torch.no_grad():
        x32 = ro["obs"].cpu().reshape(T * E, -1)
        y32 = cpu.encode(x32)
        m32 = cpu.actor_mean(y32)
        v32 = cpu.critic(y32)[:, 0].double().numpy().reshape(T, E)
        lp32 = Normal(m32, torch.exp(cpu.actor_logstd.expand_as(m32))).log_prob(ro["actions"].cpu().reshape(T * E, 2)).sum(1)
        nv32 = cpu.get_value(ro["next_obs"].cpu())[:, 0].double().numpy()
    m32 = m32.double().numpy().reshape(T, E, 2)
    lp_at_recorded = R.log_prob(P, mean64, act)
    own = {"actions": rel_err(m32 + sd * z, act64), "logprobs": rel_err(lp32.double().numpy().reshape(T, E), lp_at_recorded),
           "values": rel_err(v32, val64), "next_value": rel_err(nv32, nv64)}
    got = {"actions": rel_err(act, act64), "logprobs": rel_err(lp, lp64), "values": rel_err(val, val64),
           "next_value": rel_err(ro["next_value"].cpu().double().numpy(), nv64)}
    tol = {k: max(8.0 * v, 1e-5) for k, v in own.items()}
    z_dev = (act - mean64) / sd
    got["z"], tol["z"], own["z"] = float(np.max(np.abs(z_dev - z))), tol["actions"] * max(1.0, float(np.abs(act64).max())) / float(sd.min()), 0.0
    print(f"{case} E={E}: " + "; ".join(f"{k}: torch f32 {own[k]:.3e} kernel {got[k]:.3e} bound {tol[k]:.3e}" for k in got))
    for k in got:
        assert got[k] <= tol[k], (case, E, k, got[k], tol[k])


@pytest.mark.parametrize("E", [64, 20])
@pytest.mark.parametrize("case", list(CASES))
def test_policy_outputs_teacher_forced(ea, case, E):
    """1."""
    check_policy_outputs_teacher_forced(_cases, ea, case, E)


@pytest.mark.parametrize("E", [64, 20])
@pytest.mark.parametrize("case", list(CASES))
def test_env_side_bit_for_bit(ea, case, E):
    """2."""
    _cases.env_side_bit_for_bit(ea, case, E)


PER_STEP = ("obs", "actions", "logprobs", "values", "rewards", "dones", "episode_stats")


@pytest.mark.parametrize("case", ["n62_rel_ohe_box_norm_clip", "n60_rel_ohe_box_raw_resid", "n10_abs_cat_box_raw", "n31_rel_no_box_norm"])
def test_invariance(ea, case):
    """3."""
    import torch
    net = make_net(case)
    (one,), f1 = _run(ea, case, 64, [33], net)
    (p7, p26), f2 = _run(ea, case, 64, [7, 26], net)
    (again,), f3 = _run(ea, case, 64, [33], net)
    (small,), _ = _run(ea, case, 20, [33], net)
    for k in PER_STEP:
        assert i32(one[k]).equal(i32(torch.cat([p7[k], p26[k]]))), (case, k)
        assert i32(one[k]).equal(i32(again[k])), (case, k)
        assert i32(one[k][:, :20]).equal(i32(small[k])), (case, k)
    for k in ("next_obs", "next_done", "next_value"):
        assert i32(one[k]).equal(i32(p26[k])) and i32(one[k]).equal(i32(again[k])) and i32(one[k][:20]).equal(i32(small[k])), (case, k)
    for k in f1:
        assert raw(f1[k]).equal(raw(f2[k])) and raw(f1[k]).equal(raw(f3[k])), (case, k)


STATE = ("ped", "status", "agent", "clock", "acc")


@pytest.mark.parametrize("mode", ["sample", "mean"])
@pytest.mark.parametrize("case", ["n62_rel_ohe_box_norm_clip", "n10_abs_cat_box_raw", "n60_rel_ohe_box_raw_resid",
                                  "n60_rel_ohe_box_raw_resid_generic"])
def test_evaluation_is_the_rollout(ea, case, mode):
    """4a. policy_evaluate(max_steps = T) against policy_rollout(T) on a twin handle -- in mean mode with the twin's actor_logstd
    at -inf (expf gives 0 exactly)."""
    _cases.evaluation_is_the_rollout(ea, case, mode)


@pytest.mark.parametrize("case,frozen", [("n62_rel_ohe_box_norm_clip", True), ("n31_rel_no_box_norm", True), ("n10_abs_cat_box_raw", False)])
def test_evaluation_split_calls_and_frozen_statistics(ea, case, frozen):
    """4b. max_steps = 17 repeated until every env is done == one long call; norm_state is only read."""
    import torch
    from tests.evaluation_cases import run_until_done
    E = 48
    a, b = _twins(ea, case, E)
    net = make_net(case)
    kw = {"deterministic": not frozen}
    if frozen:
        ns = _frozen(a, E)
        keep = ns.clone()
        kw["_norm"] = (ns, 1.0, 1e-8)
    p1, r1, c1 = run_until_done(a, net, 2, 100000, **kw)
    p2, r2, c2 = run_until_done(b, net, 2, 17, **kw)
    torch.cuda.synchronize()
    assert c1 == 1 and c2 >= 2
    assert p1.equal(p2) and raw(r1).equal(raw(r2)), case
    for k in STATE:
        assert raw(getattr(a, k)).equal(raw(getattr(b, k))), (case, k)
    assert p1[:, 0].eq(2).all()
    if frozen:
        assert raw(ns).equal(raw(keep))
    if frozen and token_dim(case) > 2:
        # ... and it is read: the raw evaluation of the same start takes other steps.  (Not at 2 floats per token: LayerNorm
        # over two values leaves little more than the sign of their difference, which the statistics seldom change -- there the
        # records of the two evaluations can be, and for this net are, the same.)
        c, d = _twins(ea, case, E)
        p3, r3, _ = run_until_done(c, net, 2, 100000, deterministic=False)
        assert not raw(r1).equal(raw(r3))
        c.close(); d.close()
    a.close(); b.close()


def test_evaluation_takes_any_dropout_and_collection_refuses_it(ea):
    """Evaluation is eval mode: the same records whatever the modules' p.  Collection says no."""
    import torch
    from tests.evaluation_cases import run_until_done
    case, E = "n10_abs_cat_box_raw", 32
    a, b = _twins(ea, case, E)
    net = make_net(case)
    wet = copy.deepcopy(net)
    for m in wet.embedding.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1
    p1, r1, _ = run_until_done(a, net, 1, 100000)
    p2, r2, _ = run_until_done(b, wet, 1, 100000)
    assert p1.equal(p2) and raw(r1).equal(raw(r2))
    with pytest.raises(ValueError, match="dropout p = 0.1"):
        b.policy_rollout(wet, 4, b.observe().clone(), torch.zeros(E, device=b.device))
    a.close(); b.close()


def test_an_encoder_that_matters(ea):
    """5a. Same start, same x, same noise: other actions and values than the linear entry's."""
    from evacuation_amd.policy import LinearActorCritic
    case, E = "n10_abs_cat_box_raw", 32
    net = make_net(case)
    lin = LinearActorCritic(36).to("cuda:0")
    lin.load_state_dict({k: v for k, v in net.state_dict().items() if not k.startswith("embedding.")})

    def first_step(network):
        env = make_env(ea, case, E)
        obs, done = start(env, near_trunc=0)
        ro = {k: v.clone() for k, v in env.policy_rollout(network, 1, obs, done).items()}
        env.close()
        return ro
    d1, x1 = first_step(net), first_step(lin)
    assert i32(d1["obs"]).equal(i32(x1["obs"]))
    assert rel_err(d1["actions"].cpu().double().numpy(), x1["actions"].cpu().double().numpy()) > 1e-2
    assert rel_err(d1["values"].cpu().double().numpy(), x1["values"].cpu().double().numpy()) > 1e-3


def test_attention_without_positions_is_equivariant(ea):
    """5b. Permuting the pedestrian tokens of an observation permutes the encoder's output rows and nothing else (float64
    restatement, to its own rounding).  On the device: with an actor first layer whose weights repeat from token to token the
    mean action is a sum over the tokens and does not move under the permutation, while an ordinary first layer's does.
    The device's sums over the 36 inputs run in another order for the permuted observation: float32 rounding of 36 terms of
    magnitude <= ~1.5 in front of two tanh layers and a last layer scaled by 60 -- 1e-4 relative is some ten times that, and
    the control has to differ by ten times the bound."""
    import torch
    from tests import transformer_ref as TR
    case, E, N, dm = "n10_abs_cat_box_raw", 32, 10, 3
    net = make_net(case)
    env = make_env(ea, case, E)
    obs, done = start(env, near_trunc=0)
    g = torch.Generator().manual_seed(11)
    perm = torch.randperm(N, generator=g)
    assert not perm.equal(torch.arange(N))
    tokens = torch.cat([torch.tensor([0, 1]), 2 + perm]).to(obs.device)       # the Box rows: the leader, the exit, the pedestrians
    obs_p = obs.view(E, N + 2, dm)[:, tokens].reshape(E, -1).contiguous()
    assert not obs_p.equal(obs)
    # float64: rows permute with the tokens
    P = TR.params64(net)
    y, y_p = TR.encode(P, obs.cpu().double().numpy()), TR.encode(P, obs_p.cpu().double().numpy())
    assert np.abs(y.reshape(E, N + 2, dm)[:, tokens.cpu().numpy()] - y_p.reshape(E, N + 2, dm)).max() <= 1e-12
    assert np.abs(y - y_p).max() > 1e-3
    # device: a first layer that repeats over the pedestrian tokens (the leader's and the exit's columns keep their own weights)
    tiled = copy.deepcopy(net)
    with torch.no_grad():
        for seq in (tiled.actor_mean, tiled.critic):
            w = seq[0].weight.view(64, N + 2, dm)
            w[:, 2:] = w[:, 2:3]

    def first_step(network, x):
        ro = env.policy_rollout(network, 1, x.clone(), done.clone())
        torch.cuda.synchronize()
        restore_to_start()
        return ro["actions"][0].cpu().double().numpy(), ro["values"][0].cpu().double().numpy()
    from tests.test_gpu_policy_rollout import restore
    snap = snapshot(env)

    def restore_to_start():
        restore(env, snap)
    a, v = first_step(tiled, obs)
    a_p, v_p = first_step(tiled, obs_p)
    c, _ = first_step(net, obs)
    c_p, _ = first_step(net, obs_p)
    assert rel_err(a_p, a) <= 1e-4 and rel_err(v_p, v) <= 1e-4
    assert rel_err(c_p, c) > 1e-3                                   # the control: an ordinary first layer sees the order
    env.close()
    # ... and through policy_evaluate: envs whose pedestrians are stored in another order take the same first step of the leader
    a_env, b_env = make_env(ea, case, E, raw_env=True, subwave=0), make_env(ea, case, E, raw_env=True, subwave=0)
    a_env.reset()
    b_env.reset()
    st = a_env.get_state()
    pd = perm.to(st["pos"].device)
    b_env.set_state(pos=st["pos"][:, pd].contiguous(), dir=st["dir"][:, pd].contiguous(), status=st["status"][:, pd].contiguous())
    a_obs = a_env.observe().clone()
    assert b_env.observe().view(E, N + 2, dm).equal(a_obs.view(E, N + 2, dm)[:, tokens])      # the tokens permute, bit for bit
    assert not b_env.observe().equal(a_obs)
    before = st["agent_pos"].clone()
    a_env.policy_evaluate(tiled, 1, 1)
    b_env.policy_evaluate(tiled, 1, 1)
    torch.cuda.synchronize()
    pa, pb = a_env.get_state()["agent_pos"].cpu().double().numpy(), b_env.get_state()["agent_pos"].cpu().double().numpy()
    moved = np.abs(pa - before.cpu().double().numpy()).max()
    assert moved > 1e-3
    # the leader moves by step_size x mean / |mean|: a difference d of the two means (at most the 1e-4 of above) turns the unit
    # vector by at most 2 d / |mean|, with |mean| from the float64 restatement; 1e-7 for the float32 position itself
    m = np.linalg.norm(TR.actor_mean(TR.params64(tiled), a_obs.cpu().double().numpy()), axis=1)
    tol = a_env.env_config.step_size * 2.0 * 1e-4 / m + 1e-7
    worst = np.abs(pa - pb).max(axis=1)
    print(f"\nequivariance through policy_evaluate: |mean| {m.min():.3e} .. {m.max():.3e}, largest difference / bound {float((worst / tol).max()):.3f}")
    assert (worst <= tol).all()
    a_env.close(); b_env.close()


def test_trainer_with_the_transformer_net(ea):
    """6."""
    import torch
    from evacuation_amd.policy import TransformerActorCritic, all_tensors
    from evacuation_amd.trainer import RPOTrainer, RPOTrainingConfig, autograd_minibatch_grad
    cfg_env = ea.EnvConfig(number_of_pedestrians=10, max_timesteps=30)
    wrap = ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box")
    env = ea.NormalizedVectorEnv(ea.BatchedEvacuationEnv(cfg_env, wrap, num_envs=8, seed=3))
    torch.manual_seed(1)
    net = TransformerActorCritic(env.obs_dim, 10).to("cuda:0")
    cfg = RPOTrainingConfig(num_envs=8, num_steps=32, num_minibatches=4, update_epochs=2, total_timesteps=8 * 32 * 4)
    with pytest.raises(ValueError, match="`embedding`"):
        RPOTrainer(env, net, cfg, optimizer="device")
    tr = RPOTrainer(env, net, cfg)
    assert tr.grad_fn is autograd_minibatch_grad and len(tr.params) == 45
    before = [t.detach().clone() for t in all_tensors(net)]
    logs = [tr.update(), tr.update()]
    for log in logs:
        for k in ("loss", "value_loss", "policy_loss", "entropy", "approx_kl"):
            assert np.isfinite(log[k]), (k, log[k])
    # every tensor moves but the two key biases `attention.Wk.bias`: a key bias adds the same number to every score of a softmax
    # row, so the function does not depend on it and its exact gradient is zero (tests/test_transformer_cpu.py measures it)
    still = [i for i, (b, t) in enumerate(zip(before, all_tensors(net))) if torch.equal(b, t.detach())]
    assert set(still) <= {13 + 3, 13 + 16 + 3}, still             # (float32 leaves a rounding-sized gradient that may move one)
    assert all_tensors(net)[16] is net.embedding[0].attention.Wk.bias and all_tensors(net)[32] is net.embedding[1].attention.Wk.bias
    res = tr.evaluate(1)
    assert res.episodes["episode_reward"].shape == (1, 8) and res.steps.shape == (8,)
    assert bool((res.episodes["episode_length"] >= 1).all())
    tr.evaluator.close()
    env.close()


def test_c_abi_refusals(ea):
    """7."""
    import torch
    from evacuation_amd import _lib
    from evacuation_amd.policy import PolicyBinder, TransformerActorCritic
    bad, unsupported = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    case = "n10_abs_cat_box_raw"
    env = make_env(ea, case, 16)
    env.reset()
    net = make_net(case)
    two = TransformerActorCritic(36, 10).to("cuda:0")
    binder = PolicyBinder(36, env.device, 10)
    pol, enc, enc2 = binder(net), binder.transformer(net), binder.transformer(two)
    h, lib = env._h, env.lib
    bufs = [torch.zeros(4 * 16 * 40, device=env.device) for _ in range(9)]
    ptr = [C.c_void_p(t.data_ptr()) for t in bufs]
    prog, recs = torch.zeros((16, 4), dtype=torch.int32, device=env.device), torch.zeros((1, 16, 10), device=env.device)

    def rollout(policy=pol, encoder=enc, n_steps=4, drop=None, handle=h):
        args = list(ptr) + [None, None, 0.99, 1.0, 100.0, 1e-8]
        if drop is not None:
            args[drop] = None
        return lib.evac_policy_rollout_transformer(handle, n_steps, None if policy is None else C.byref(policy), *args,
                                                   None if encoder is None else C.byref(encoder), None)

    def evaluate(agent=0, policy=pol, encoder=enc, handle=h, progress=prog):
        return lib.evac_policy_evaluate_transformer(handle, agent, None if policy is None else C.byref(policy), 1, 4,
                                                    C.c_void_p(progress.data_ptr()), C.c_void_p(recs.data_ptr()), None, 1.0, 1e-8,
                                                    None if encoder is None else C.byref(encoder), None)

    def changed(st, field, value, block=None):
        s2 = type(st).from_buffer_copy(st)
        setattr(s2 if block is None else s2.blocks[block], field, value)
        return s2
    for call in (rollout, evaluate):
        for f, _ in _lib.EvacTransformerBlock._fields_:                                 # a NULL tensor of a block in use
            assert call(encoder=changed(enc, f, None, block=0)) == bad, f
            assert b"block 0" in lib.evac_last_error(h)
        assert call(encoder=changed(enc2, "norm2_b", None, block=1)) == bad and b"block 1" in lib.evac_last_error(h)
        assert call(encoder=changed(enc, "wq", None, block=1)) == 0                     # ... and none beyond num_blocks is read
        for ed in (2, 4, 6, 0, 36, 7):                                                  # 12 tokens of 3 floats
            assert call(encoder=changed(enc, "elem_dim", ed)) == bad, ed
        assert b"elem_dim" in lib.evac_last_error(h)
        for field, value in (("num_heads", 2), ("dim_feedforward", 64), ("num_blocks", 3), ("num_blocks", 0), ("ln_eps", 1e-6)):
            assert call(encoder=changed(enc, field, value)) == unsupported, field
            assert field.encode() in lib.evac_last_error(h), (field, lib.evac_last_error(h))
        assert call(encoder=None) == bad and call(policy=None) == bad
        for field, value in (("critic_b2", None), ("hidden", 32), ("obs_dim", 37)):   # what the existing entries refuse
            assert call(policy=changed(pol, field, value)) == bad, field
        assert call(handle=None) == bad
    for k in range(9):
        assert rollout(drop=k) == bad, k
    assert rollout(n_steps=0) == bad
    assert evaluate(agent=_lib.AGENT_VACUUM_CLEANER) == bad and b"scripted" in lib.evac_last_error(h)
    assert evaluate(agent=7) == bad
    assert evaluate(progress=prog.view(-1)[1:]) == bad                                  # misaligned
    assert rollout() == 0 and evaluate() == 0 and rollout(encoder=enc2) == 0            # the valid calls go through
    torch.cuda.synchronize()
    env.close()
    # the gravity observation: no Box of tokens
    g = ea.BatchedEvacuationEnv(ea.EnvConfig(number_of_pedestrians=1), ea.EnvWrappersConfig(positions="grav"), num_envs=16)
    g.reset()
    gnet = TransformerActorCritic(6, 1).to("cuda:0")
    gb = PolicyBinder(6, g.device)
    assert rollout(policy=gb(gnet), encoder=gb.transformer(gnet), handle=g._h) == unsupported and b"gravity" in lib.evac_last_error(g._h)
    assert evaluate(policy=gb(gnet), encoder=gb.transformer(gnet), handle=g._h) == unsupported
    with pytest.raises(_lib.EvacError, match="gravity"):    # (6 floats are 3 tokens of 2 for the binder: the library knows better)
        g.policy_rollout(gnet, 4, g.observe().clone(), torch.zeros(16, device=g.device))
    g.close()
    # N = 63, 64: a second pass of tokens that would also have to serve as keys
    for n_ped in (63, 64):
        big = ea.BatchedEvacuationEnv(ea.EnvConfig(number_of_pedestrians=n_ped), ea.EnvWrappersConfig(positions="rel", statuses="no", type="Box"),
                                      num_envs=16)
        obs, _ = big.reset()
        bnet = TransformerActorCritic(big.obs_dim, n_ped).to("cuda:0")
        bb = PolicyBinder(big.obs_dim, big.device)              # (no N: the binder's own refusal is tested on the CPU)
        assert rollout(policy=bb(bnet), encoder=bb.transformer(bnet), handle=big._h) == unsupported
        assert b"N = %d" % n_ped in lib.evac_last_error(big._h)
        assert evaluate(policy=bb(bnet), encoder=bb.transformer(bnet), handle=big._h) == unsupported
        with pytest.raises(ValueError, match=f"N = {n_ped}"):
            big.policy_rollout(bnet, 4, obs, torch.zeros(16, device=big.device))
        with pytest.raises(ValueError, match=f"N = {n_ped}"):
            big.policy_evaluate(bnet, 1, 4)
        big.close()


def test_example_trains_the_transformer_net(ea):
    """8."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_rpo.py"), "--network", "transformer", "--envs", "8", "--steps", "16",
           "--updates", "2", "--pedestrians", "10", "--minibatches", "2", "--epochs", "1", "--eval-every", "2"]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert proc.stdout.count("SPS:") == 2 and "eval policy (mean)" in proc.stdout
