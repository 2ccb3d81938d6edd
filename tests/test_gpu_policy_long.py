"""The policy kernels past their first 64-step noise block, on an MI355X.

policy_rollout_body and policy_evaluate_body (sample mode) draw the policy's noise 64 steps at a time, one step per lane, at every
`t & 63 == 0` of a launch, from the env's step counter at that moment; step t reads lane t & 63.  The other files of the suite
stop at or before step 64 of a launch.  Here every family runs T = 150 steps in one launch (blocks drawn at t = 0, 64 and 128, the
third one partial) on E = 20 envs (one full workgroup of 16 envs and one of 4) at max_timesteps = 70 with shifted clocks, so that
autoresets fall before, inside and after the block edges -- and the checks are the existing ones with their existing bounds:

1. Collection, linear network: test_gpu_policy_rollout's teacher-forced float64 comparison (1e-5; z against the restated Philox
   stream at the env's own counter, 2e-6) of all 150 rows -- rows 63, 64, 65, 127, 128 and 149 among them -- and the twin's replay
   through step(), bit for bit.
2. One call of 150 == calls of [64, 86], [63, 87], [65, 85], [1, 149], [128, 22], bit for bit: a call redraws its block at its own
   t = 0, so the split calls' block phases differ from the single call's.
3. Collection, deep-sets and transformer: test 1 and test 2 of their files (8 x the module's own float32 error, floor 1e-5).
4. The reference's own collection shape, 3 envs x 2048 steps (32 blocks), max_timesteps = 700.
5. Populations and sweeps: learner s is policy_rollout(nets[s]) alone at T = 150.
6. Evaluation: against policy_rollout(150); episodes of 150 steps in calls of 17, 64 and 100; the population's shared-episode
   form; the recorded frames of episodes of up to 80 steps (rows up to 159).

Every part asserts on its own recorded episode ends that each env ends at least two episodes inside the call, that the ends fall
on at least three values of t mod 64 and that one lies at t >= 64."""
import numpy as np
import pytest

from tests import test_gpu_deepsets as DS
from tests import test_gpu_transformer as TF
from tests.encoder_cases import EncoderCases, _frozen, ea  # noqa: F401 (ea: the fixture)
from tests.test_gpu_policy_rollout import _run, assert_split_equals_one, base, make_env, make_net, raw, start, teacher_forced_and_env_side_bit_for_bit

pytestmark = pytest.mark.gpu

T, E, MAX_T = 150, 20, 70
SPLITS = ([64, 86], [63, 87], [65, 85], [1, 149], [128, 22])
REF_E, REF_T, REF_MAX_T = 3, 2048, 700        # RPOTrainingConfig's num_envs x num_steps


def transformer_net(case):
    return TF.make_net(case, seed=TF.LONG_NET_SEEDS[case])


ENCODERS = {
    "deepsets": (DS, EncoderCases(DS.CASES, DS.make_net, T, max_timesteps=MAX_T), EncoderCases(DS.CASES, DS.make_net, REF_T, max_timesteps=REF_MAX_T)),
    "transformer": (TF, EncoderCases(TF.CASES, transformer_net, T, max_timesteps=MAX_T),
                    EncoderCases(TF.CASES, transformer_net, REF_T, max_timesteps=REF_MAX_T)),
}


def episode_ends(dones, next_done):
    """[T, E] bool: step t of the call ended an episode of env e -- from the storage's dones (row t + 1 is step t's) and next_done"""
    d = np.concatenate([np.asarray(dones.cpu().numpy())[1:], np.asarray(next_done.cpu().numpy())[None]], axis=0)
    return d > 0


def assert_ends_cross_the_blocks(ended, what):
    """The preconditions of every part, on the call's own episode ends [T, E]"""
    per_env = ended.sum(0)
    assert (per_env >= 2).all(), (what, "episode ends per env", per_env.tolist())
    at = np.nonzero(ended.any(1))[0]
    assert len(set((at % 64).tolist())) >= 3, (what, "t mod 64 of the episode ends", sorted(set((at % 64).tolist())))
    assert at.max() >= 64, (what, at.max())


# ------------------------------------------------------------------------------------------------ 1. collection, linear
@pytest.mark.parametrize("case", ["n60_grav_norm_clip", "n60_rel_ohe_box_norm_clip", "n10_grav_raw", "n64_grav_wallterm_noise_raw"])
def test_linear_collection_teacher_forced_and_env_side(ea, case):
    """1. All 150 rows of the storage -- 63, 64, 65 (the first refill and its neighbours), 127, 128 (the second) and 149 (the last
    row, in the partial third block) among them -- against float64 on the recorded observation (1e-5), z against the restated
    Philox stream (2e-6), and the env side by the subwave = 0 twin's replay, bit for bit: observations, rewards, dones, episode
    records, norm_state, final state, clock and accumulators."""
    ro, _ = teacher_forced_and_env_side_bit_for_bit(ea, case, E=E, T=T, max_timesteps=MAX_T)
    assert all(ro[k].shape[0] == T for k in ("obs", "actions", "logprobs", "values", "rewards", "dones")) and T > 149
    assert_ends_cross_the_blocks(episode_ends(ro["dones"], ro["next_done"]), case)


# ------------------------------------------------------------------------------------------------ 2. split calls
def linear_runs(ea, case, T_split, net):
    outs, fin = _run(ea, case, E, T_split, net=net, max_timesteps=MAX_T)
    return [{k: v.clone() for k, v in o.items()} for o in outs], fin


@pytest.mark.parametrize("network,case", [("linear", "n60_grav_norm_clip"), ("linear", "n32_abs_cat_dict_norm"),
                                          ("deepsets", "n64_rel_ohe_box_norm_clip"), ("transformer", "n62_rel_ohe_box_norm_clip")])
def test_split_calls_across_the_block_edges_equal_one_call(ea, network, case):
    """2. Every storage key, next_*, the final snapshot and norm_state, bit for bit."""
    if network == "linear":
        env = make_env(ea, case, E)
        net = make_net(ea, base(env).obs_dim)
        env.close()
        run = lambda T_split: linear_runs(ea, case, T_split, net)                   # noqa: E731
    else:
        cases = ENCODERS[network][1]
        net = cases.make_net(case)
        run = lambda T_split: cases.run(ea, case, E, T_split, net)                  # noqa: E731
    (one,), f1 = run([T])
    assert "norm_state" in f1
    assert_ends_cross_the_blocks(episode_ends(one["dones"], one["next_done"]), (network, case))
    for split in SPLITS:
        assert sum(split) == T
        parts, f2 = run(list(split))
        assert_split_equals_one(one, f1, parts, f2, (network, case, split))


# ------------------------------------------------------------------------------------------------ 3. collection, encoders
ENCODER_CASES = [("deepsets", "n64_rel_ohe_box_norm_clip"), ("deepsets", "n10_abs_cat_box_raw"),
                 ("transformer", "n62_rel_ohe_box_norm_clip"), ("transformer", "n10_abs_cat_box_raw")]


@pytest.mark.parametrize("network,case", ENCODER_CASES)
def test_encoder_collection_teacher_forced(ea, network, case):
    """3a. Test 1 of the network's file on the 150-step rollout: its bound (8 x the module's own float32 CPU error on the same
    observations, floor 1e-5; z as there), and for the transformer its variance precondition."""
    module, cases, _ = ENCODERS[network]
    _, ro, _, _, _, _ = cases.rollout_of(ea, case, E)
    assert ro["obs"].shape[0] == T
    assert_ends_cross_the_blocks(episode_ends(ro["dones"], ro["next_done"]), (network, case))
    module.check_policy_outputs_teacher_forced(cases, ea, case, E)


@pytest.mark.parametrize("network,case", ENCODER_CASES)
def test_encoder_collection_env_side(ea, network, case):
    """3b. Test 2 of the network's file on the same rollout: the twin's replay of all 150 steps, bit for bit."""
    ENCODERS[network][1].env_side_bit_for_bit(ea, case, E)


# ------------------------------------------------------------------------------------------------ 4. the reference's shape
def test_the_shape_is_the_training_configs():
    from evacuation_amd.trainer import RPOTrainingConfig
    cfg = RPOTrainingConfig()
    assert (cfg.num_envs, cfg.num_steps) == (REF_E, REF_T)


def test_reference_shape_linear(ea):
    """4. 3 envs x 2048 steps, n60_grav_norm_clip: part 1's checks, and the normaliser's observation count of every env is its
    count at the start plus one per step plus one per episode end (the terminal observation is counted, then the reset's)."""
    case = "n60_grav_norm_clip"
    env = make_env(ea, case, REF_E, max_timesteps=REF_MAX_T)
    start(env)
    D = base(env).obs_dim
    count0 = env.norm_state[:, 2 * D:3 * D].cpu().numpy().copy()
    env.close()
    ro, ns = teacher_forced_and_env_side_bit_for_bit(ea, case, E=REF_E, T=REF_T, max_timesteps=REF_MAX_T)
    ended = episode_ends(ro["dones"], ro["next_done"])
    assert ro["obs"].shape[0] == REF_T
    assert_ends_cross_the_blocks(ended, case)
    want = count0.copy()
    updates = REF_T + ended.sum(0)                                # per env
    for n in range(int(updates.max())):                           # rms_update1's own arithmetic: count + 1.0, one update at a time
        want = np.where((n < updates)[:, None], want + 1.0, want)
    got = ns[:, 2 * D:3 * D].cpu().numpy()                        # the twin's, bit for bit the rollout's (asserted in part 1's body)
    assert np.array_equal(got, want), (got[:, 0], want[:, 0])
    assert np.allclose(got, count0 + updates[:, None], rtol=0, atol=1e-6)


@pytest.mark.parametrize("network", ["deepsets", "transformer"])
def test_reference_shape_encoders(ea, network):
    """4. 3 envs x 2048 steps, n10_abs_cat_box_raw: part 3's checks."""
    case = "n10_abs_cat_box_raw"
    module, _, cases = ENCODERS[network]
    _, ro, _, _, _, _ = cases.rollout_of(ea, case, REF_E)
    assert ro["obs"].shape[0] == REF_T
    assert_ends_cross_the_blocks(episode_ends(ro["dones"], ro["next_done"]), (network, case))
    module.check_policy_outputs_teacher_forced(cases, ea, case, REF_E)
    cases.env_side_bit_for_bit(ea, case, REF_E)


# ------------------------------------------------------------------------------------------------ 5. populations and sweeps
@pytest.mark.parametrize("S,E_l", [(3, 3), (2, 20)])
@pytest.mark.parametrize("kernel", ["population", "sweep", "deepsets_population"])
def test_population_collection_is_each_learner_alone(ea, kernel, S, E_l):
    """5. k_collect_population (gravity, normaliser), k_collect_sweep (two gammas) and k_collect_population_deepsets at T = 150:
    learner s's storage, norm_state, records and final state are policy_rollout(nets[s]) alone, which parts 1 and 3 hold to
    their references."""
    if kernel == "population":
        from tests.test_gpu_population import collection_equals_standalone_rollouts
        ro = collection_equals_standalone_rollouts(ea, "n60_grav_norm_clip", S, E_l, T=T, max_timesteps=MAX_T)
    elif kernel == "sweep":
        from tests.test_gpu_sweep import collection_normalises_rewards_with_each_learners_gamma
        ro = collection_normalises_rewards_with_each_learners_gamma(ea, "n60_grav_norm_clip", S, E_l, T=T, gammas=[0.99, 0.9, 0.99][:S],
                                                                    max_timesteps=MAX_T)
    else:
        from tests.test_gpu_deepsets_population import collection_equals_standalone_rollouts
        ro = collection_equals_standalone_rollouts(ea, "n60_rel_ohe_box_norm_clip", S, E_l, T=T, max_timesteps=MAX_T)
    assert ro["obs"].shape[0] == T
    assert_ends_cross_the_blocks(episode_ends(ro["dones"], ro["next_done"]), (kernel, S, E_l))


# ------------------------------------------------------------------------------------------------ 6. evaluation
@pytest.mark.parametrize("network,case,mode", [
    ("linear", "n60_grav_norm_clip", "sample"), ("linear", "n60_grav_norm_clip", "mean"), ("linear", "n64_grav_wallterm_noise_raw", "sample"),
    ("deepsets", "n10_abs_cat_box_raw", "sample"), ("transformer", "n62_rel_ohe_box_norm_clip", "sample")])
def test_evaluation_is_the_rollout_past_a_block(ea, network, case, mode):
    """6a. policy_evaluate(max_steps = 150) against policy_rollout(150) on the twin: state, progress and episode records."""
    if network == "linear":
        from tests.test_gpu_policy_evaluate import evaluation_is_the_policy_rollout
        ended = evaluation_is_the_policy_rollout(ea, case, mode, E=E, T=T, max_timesteps=MAX_T)
    else:
        ended = ENCODERS[network][1].evaluation_is_the_rollout(ea, case, mode, E=E, T=T)
    assert ended.shape == (T, E)
    assert_ends_cross_the_blocks(ended, (network, case, mode))


LONG_EPISODE = 150


@pytest.mark.parametrize("network,case,frozen", [("linear", "n10_grav_raw", False), ("linear", "n60_grav_norm_clip", True),
                                                 ("deepsets", "n10_abs_cat_box_raw", False), ("transformer", "n10_abs_cat_box_raw", False)])
def test_episodes_longer_than_a_block_in_split_calls(ea, network, case, frozen):
    """6b. max_timesteps = 150, two episodes, sample mode: one call == calls of 17 == calls of 64 == calls of 100 -- records,
    progress and state as bytes.  Every env has an episode of more than 64 steps."""
    import torch
    from tests.evaluation_cases import STATE, eval_net, run_until_done
    from tests.test_gpu_policy_evaluate import twins

    def handles():
        if network == "linear":
            return twins(ea, case, E, max_timesteps=LONG_EPISODE)
        return EncoderCases(ENCODERS[network][0].CASES, None, 0, max_timesteps=LONG_EPISODE).twins(ea, case, E)
    a, b = handles()
    c, d = handles()
    net = eval_net(ea, a.obs_dim) if network == "linear" else ENCODERS[network][1].make_net(case)
    kw = {"deterministic": False}
    if frozen:
        ns = _frozen(a, E)
        keep = ns.clone()
        kw["_norm"] = (ns, 1.0, 1e-8)
    p1, r1, c1 = run_until_done(a, net, 2, 100000, **kw)
    torch.cuda.synchronize()
    assert c1 == 1 and p1[:, 0].eq(2).all() and p1[:, 2:].eq(0).all()
    length = r1[..., 1].cpu().numpy()                              # STATS_FIELDS: episode_length
    assert (length.max(0) > 64).all(), length.max(0).tolist()
    assert int(p1[:, 1].max()) > 128                               # three noise blocks in the one call
    for env, max_steps in ((b, 17), (c, 64), (d, 100)):
        p2, r2, c2 = run_until_done(env, net, 2, max_steps, **kw)
        torch.cuda.synchronize()
        assert c2 >= 2
        assert p1.equal(p2) and raw(r1).equal(raw(r2)), (network, case, max_steps)
        for k in STATE:
            assert raw(getattr(a, k)).equal(raw(getattr(env, k))), (network, case, max_steps, k)
    if frozen:
        assert raw(ns).equal(raw(keep))
    for env in (a, b, c, d):
        env.close()


@pytest.mark.parametrize("shared", [True, False])
def test_population_evaluation_is_each_learner_alone_over_long_episodes(ea, shared):
    """6c. assert_learners_alone at max_timesteps = 150, sample mode, S = 3, E_l = 3 (shared episodes: the global id is the env's
    place less the learner's shift)."""
    from tests.test_gpu_population_evaluate import assert_learners_alone
    progress, rec = assert_learners_alone(ea, "n60_grav_norm_clip", 3, 3, shared, False, True, max_timesteps=LONG_EPISODE)
    assert progress[:, 0].eq(2).all() and progress[:, 2:].eq(0).all()
    length = rec[..., 1].cpu().numpy()
    assert (length.max(0) > 64).all(), length.max(0).tolist()


CAPTURE_MAX_T, CAPTURE_EPISODES = 80, 2


@pytest.mark.parametrize("kind", ["linear", "deepsets", "transformer_n62"])
def test_recorded_frames_past_row_64(ea, kind):
    """6d. Tests 7 and 12 of test_gpu_evaluate_capture.py with episodes of up to 80 steps, two per env: up to 160 frame rows, the
    buffers starting as NaN.  Sample-mode frames are the plain rollout's trajectory under policy_rollout's stored actions; calls
    of max_steps = 5 write the frames of the one call; rows past each env's last frame stay NaN."""
    import torch
    from tests import test_gpu_evaluate_capture as CAP
    run = CAP.sample_mode_frames_are_the_plain_rollouts(ea, kind, CAPTURE_EPISODES, CAPTURE_MAX_T)
    steps = run.progress[:, 1].cpu().numpy()
    assert tuple(run.frames.shape[:2]) == (CAPTURE_EPISODES * CAPTURE_MAX_T, CAP.K)
    assert int(steps[:CAP.K].max()) > 128 and int(steps[:CAP.K].min()) > 64       # frame rows past both block edges
    one = CAP.resumption_and_bounds(ea, kind, "sample", False, CAPTURE_EPISODES, CAPTURE_MAX_T)
    assert one is run
    for e in range(CAP.K):
        n = int(steps[e])
        assert not torch.isnan(run.frames[:n, e]).any() and torch.isnan(run.frames[n:, e]).all(), (kind, e)
