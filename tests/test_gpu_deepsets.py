"""The deep-sets leader (evac_policy_rollout_deepsets, evac_policy_evaluate_deepsets; policy.DeepSetsActorCritic through
BatchedEvacuationEnv / NormalizedVectorEnv.policy_rollout / policy_evaluate, PolicyEvaluator, RPOTrainer) on an MI355X.

1. Policy outputs, teacher-forced on the recorded observations, against the float64 restatement (tests/deepsets_ref.py).  The
   bound of a case is 8 x the largest error of the module's OWN float32 torch forward (CPU) against float64 on those same
   observations, per quantity, with a floor of 1e-5 (the linear test's figure): the margin covers the kernel's summation order
   (pooling above the relu, fixed trees) and tanhf.  Both figures are printed.
2. The env side, bit for bit: a twin handle (subwave = 0) replays the recorded actions through step().
3. Invariance: T = 33 == 7 + 26, two runs, E = 20 == the first 20 envs of E = 64.
4. Evaluation: sample mode == the rollout, mean mode == the rollout with sigma = 0, max_steps = 17 repeated == one call, a frozen
   norm_state is only read.
5. An encoder that matters: rho = 0 gives the linear entry's outputs on an all-zero observation; the real weights do not give the
   linear entry's outputs on x.
6. RPOTrainer with the deep-sets net.  7. The C ABI's refusals."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests.encoder_cases import EncoderCases, _frozen, ea, rel_err  # noqa: F401 (ea: the fixture)
from tests.test_gpu_policy_rollout import OFFSET, SEED, base, i32, raw, replay_env_side, snapshot, start

pytestmark = pytest.mark.gpu

CASES = {
    # name: (EnvConfig kwargs, EnvWrappersConfig kwargs, normalised chain, KernelOptions overrides)
    "n64_rel_ohe_box_norm_clip": (dict(number_of_pedestrians=64, max_timesteps=25, clip_action=True),
                                  dict(positions="rel", statuses="ohe", type="Box"), True, {}),          # D = 396: 66 elements, two passes
    "n10_abs_cat_box_raw": (dict(number_of_pedestrians=10, max_timesteps=20, intrinsic_reward_coef=0.5),
                            dict(positions="abs", statuses="cat", type="Box"), False, {}),               # 3 floats per element
    "n31_rel_no_box_norm": (dict(number_of_pedestrians=31, max_timesteps=22, enslaving_degree=0.7),
                            dict(positions="rel", statuses="no", type="Box"), True, {}),                 # 2 floats, 33 elements
    "n60_rel_ohe_box_raw": (dict(number_of_pedestrians=60, max_timesteps=25), dict(positions="rel", statuses="ohe", type="Box"),
                            False, {}),
    "n60_rel_ohe_box_raw_generic": (dict(number_of_pedestrians=60, max_timesteps=25), dict(positions="rel", statuses="ohe", type="Box"),
                                    False, dict(specialize=0)),
}
T_STEPS = 40


def make_net(case, seed=0, device="cuda:0"):
    """A deep-sets leader with visible actions and values (test_gpu_policy_rollout.make_net's recipe) and an encoder whose output
    stays in the tanh layers' range whatever the number of elements."""
    import torch
    from evacuation_amd.policy import DeepSetsActorCritic
    cfg_kw, wrap_kw = CASES[case][:2]
    N = cfg_kw["number_of_pedestrians"]
    ed = 2 + {"ohe": 4, "cat": 1, "no": 0}[wrap_kw["statuses"]]
    torch.manual_seed(seed)
    net = DeepSetsActorCritic((N + 2) * ed, N)
    with torch.no_grad():
        net.actor_mean[4].weight.mul_(60.0)
        net.actor_logstd.copy_(torch.tensor([[-0.5, 0.3]]))
        for m in list(net.actor_mean) + list(net.critic):
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.2)
        net.deep_sets.transform_rho[0].weight.mul_(3.0 / (N + 2))
    return net.to(device)


_cases = EncoderCases(CASES, make_net, T_STEPS)
make_env, rollout_of, _run, _twins = _cases.make_env, _cases.rollout_of, _cases.run, _cases.twins


def check_policy_outputs_teacher_forced(cases, ea, case, E):
    """Test 1 on the shared rollout of ``cases`` (an EncoderCases of this file's CASES and make_net)."""
    import torch
    from torch.distributions.normal import Normal
    from tests import deepsets_ref as DR
    from tests import policy_ref as R
    net, ro, _, total0, _, _ = cases.rollout_of(ea, case, E)
    P = DR.params64(net)
    cpu = copy.deepcopy(net).to("cpu")
    obs, act = ro["obs"].cpu().double().numpy(), ro["actions"].cpu().double().numpy()
    lp, val = ro["logprobs"].cpu().double().numpy(), ro["values"].cpu().double().numpy()
    sd = np.exp(P["logstd"])
    T = obs.shape[0]
    z = cases.policy_noise(total0, T)
    mean64, act64, lp64, val64 = DR.policy_step(P, obs, z)
    nv64 = DR.value(P, ro["next_obs"].cpu().double().numpy())
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
    print(f"\n{case} E={E}: " + "; ".join(f"{k}: torch f32 {own[k]:.3e} kernel {got[k]:.3e} bound {tol[k]:.3e}" for k in got))
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


@pytest.mark.parametrize("case", ["n64_rel_ohe_box_norm_clip", "n10_abs_cat_box_raw", "n31_rel_no_box_norm"])
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
@pytest.mark.parametrize("case", ["n64_rel_ohe_box_norm_clip", "n10_abs_cat_box_raw", "n60_rel_ohe_box_raw", "n60_rel_ohe_box_raw_generic"])
def test_evaluation_is_the_rollout(ea, case, mode):
    """4a. policy_evaluate(max_steps = T) against policy_rollout(T) on a twin handle -- in mean mode with the twin's actor_logstd
    at -inf (expf gives 0 exactly)."""
    _cases.evaluation_is_the_rollout(ea, case, mode)


@pytest.mark.parametrize("case,frozen", [("n64_rel_ohe_box_norm_clip", True), ("n31_rel_no_box_norm", True), ("n10_abs_cat_box_raw", False)])
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
        # ... and it is read: the raw evaluation of the same start takes other steps
        c, d = _twins(ea, case, E)
        p3, r3, _ = run_until_done(c, net, 2, 100000, deterministic=False)
        assert not raw(r1).equal(raw(r3))
        c.close(); d.close()
    a.close(); b.close()


def test_an_encoder_that_matters(ea):
    """5."""
    import torch
    from evacuation_amd.policy import LinearActorCritic
    case, E = "n10_abs_cat_box_raw", 32
    net = make_net(case)
    lin = LinearActorCritic(36).to("cuda:0")
    lin.load_state_dict({k: v for k, v in net.state_dict().items() if not k.startswith("deep_sets.")})
    zero = copy.deepcopy(net)
    with torch.no_grad():
        zero.deep_sets.transform_rho[0].weight.zero_()
        zero.deep_sets.transform_rho[0].bias.zero_()

    def first_steps(network, T, zero_obs=False):
        env = make_env(ea, case, E)
        obs, done = start(env, near_trunc=0)
        if zero_obs:
            obs.zero_()
        ro = {k: v.clone() for k, v in env.policy_rollout(network, T, obs, done).items()}
        env.close()
        return ro
    z8, l1, d1, x1 = first_steps(zero, 8), first_steps(lin, 1, zero_obs=True), first_steps(net, 1), first_steps(lin, 1)
    bound = 1e-5            # test 1's floor: y = 0 exactly, so the two entries run the same forward pass on the same row
    for k in ("actions", "logprobs", "values"):
        got, want = z8[k][0].cpu().double().numpy(), l1[k][0].cpu().double().numpy()
        assert rel_err(got, want) <= bound, k
    v0 = z8["values"][0, 0].item()
    assert rel_err(z8["values"].cpu().double().numpy(), np.full((8, E), v0)) <= bound      # critic(0) at every step, for every env
    assert rel_err(z8["next_value"].cpu().double().numpy(), np.full(E, v0)) <= bound
    # the real encoder: same start, same x, same noise -- other actions and values than the linear entry's
    assert i32(d1["obs"]).equal(i32(x1["obs"]))
    assert rel_err(d1["actions"].cpu().double().numpy(), x1["actions"].cpu().double().numpy()) > 1e-2
    assert rel_err(d1["values"].cpu().double().numpy(), x1["values"].cpu().double().numpy()) > 1e-3


def test_trainer_with_the_deepsets_net(ea):
    """6."""
    import torch
    from evacuation_amd.policy import DeepSetsActorCritic, all_tensors
    from evacuation_amd.trainer import RPOTrainer, RPOTrainingConfig, autograd_minibatch_grad
    cfg_env = ea.EnvConfig(number_of_pedestrians=10, max_timesteps=30)
    wrap = ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box")
    env = ea.NormalizedVectorEnv(ea.BatchedEvacuationEnv(cfg_env, wrap, num_envs=16, seed=3))
    torch.manual_seed(1)
    net = DeepSetsActorCritic(env.obs_dim, 10).to("cuda:0")
    cfg = RPOTrainingConfig(num_envs=16, num_steps=32, num_minibatches=4, update_epochs=2, total_timesteps=16 * 32 * 4)
    with pytest.raises(ValueError, match="linear network's"):
        RPOTrainer(env, net, cfg, optimizer="device")
    tr = RPOTrainer(env, net, cfg)
    assert tr.grad_fn is autograd_minibatch_grad and len(tr.params) == 19
    before = [t.detach().clone() for t in all_tensors(net)]
    logs = [tr.update(), tr.update()]
    for log in logs:
        for k in ("loss", "value_loss", "policy_loss", "entropy", "approx_kl"):
            assert np.isfinite(log[k]), (k, log[k])
    for i, (b, t) in enumerate(zip(before, all_tensors(net))):
        assert not torch.equal(b, t.detach()), i
    res = tr.evaluate(1)
    assert res.episodes["episode_reward"].shape == (1, 16) and res.steps.shape == (16,)
    assert bool((res.episodes["episode_length"] >= 1).all())
    tr.evaluator.close()
    env.close()


def test_c_abi_refusals(ea):
    """7."""
    import torch
    from evacuation_amd import _lib
    from evacuation_amd.policy import PolicyBinder
    bad, unsupported = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    case = "n10_abs_cat_box_raw"
    env = make_env(ea, case, 16)
    env.reset()
    net = make_net(case)
    binder = PolicyBinder(36, env.device, 10)
    pol, enc = binder(net), binder.encoder(net)
    h, lib = env._h, env.lib
    bufs = [torch.zeros(4 * 16 * 40, device=env.device) for _ in range(9)]
    ptr = [C.c_void_p(t.data_ptr()) for t in bufs]
    prog, recs = torch.zeros((16, 4), dtype=torch.int32, device=env.device), torch.zeros((1, 16, 10), device=env.device)

    def rollout(policy=pol, encoder=enc, n_steps=4, drop=None, handle=h):
        args = list(ptr) + [None, None, 0.99, 1.0, 100.0, 1e-8]
        if drop is not None:
            args[drop] = None
        return lib.evac_policy_rollout_deepsets(handle, n_steps, None if policy is None else C.byref(policy), *args,
                                                None if encoder is None else C.byref(encoder), None)

    def evaluate(agent=0, policy=pol, encoder=enc, handle=h, progress=prog):
        return lib.evac_policy_evaluate_deepsets(handle, agent, None if policy is None else C.byref(policy), 1, 4,
                                                 C.c_void_p(progress.data_ptr()), C.c_void_p(recs.data_ptr()), None, 1.0, 1e-8,
                                                 None if encoder is None else C.byref(encoder), None)

    def changed(st, field, value):
        s2 = type(st).from_buffer_copy(st)
        setattr(s2, field, value)
        return s2
    for call in (rollout, evaluate):
        for f in ("phi_w1", "phi_b1", "phi_w2", "phi_b2", "rho_w", "rho_b"):          # a NULL tensor
            assert call(encoder=changed(enc, f, None)) == bad, f
            assert b"encoder" in lib.evac_last_error(h)
        assert call(encoder=changed(enc, "hidden", 16)) == bad and b"24" in lib.evac_last_error(h)
        for ed in (2, 4, 6, 0, 36):                                                    # 12 elements of 3 floats
            assert call(encoder=changed(enc, "set_elem_dim", ed)) == bad, ed
        assert b"set_elem_dim" in lib.evac_last_error(h)
        assert call(encoder=changed(enc, "rho_w", enc.rho_w + 4)) == bad and b"aligned" in lib.evac_last_error(h)
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
    assert rollout() == 0 and evaluate() == 0                                           # the valid calls go through
    torch.cuda.synchronize()
    env.close()
    # the gravity observation: 6 floats are no set of N + 2 elements
    g = ea.BatchedEvacuationEnv(ea.EnvConfig(number_of_pedestrians=1), ea.EnvWrappersConfig(positions="grav"), num_envs=16)
    g.reset()
    from evacuation_amd.policy import DeepSetsActorCritic
    gnet = DeepSetsActorCritic(6, 1).to("cuda:0")
    gb = PolicyBinder(6, g.device)
    assert rollout(policy=gb(gnet), encoder=gb.encoder(gnet), handle=g._h) == bad and b"Box" in lib.evac_last_error(g._h)
    assert evaluate(policy=gb(gnet), encoder=gb.encoder(gnet), handle=g._h) == bad
    with pytest.raises(_lib.EvacError, match="Box"):    # (6 floats are 3 rows of 2 for the binder: the library knows better)
        g.policy_rollout(gnet, 4, g.observe().clone(), torch.zeros(16, device=g.device))
    g.close()
    # N > 64
    big = ea.BatchedEvacuationEnv(ea.EnvConfig(number_of_pedestrians=65), ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box"),
                                  num_envs=16)
    obs, _ = big.reset()
    bnet = DeepSetsActorCritic(big.obs_dim, 65).to("cuda:0")
    bb = PolicyBinder(big.obs_dim, big.device, 65)
    assert rollout(policy=bb(bnet), encoder=bb.encoder(bnet), handle=big._h) == unsupported
    assert evaluate(policy=bb(bnet), encoder=bb.encoder(bnet), handle=big._h) == unsupported
    with pytest.raises(NotImplementedError):
        big.policy_rollout(bnet, 4, obs, torch.zeros(16, device=big.device))
    with pytest.raises(NotImplementedError):
        big.policy_evaluate(bnet, 1, 4)
    big.close()
