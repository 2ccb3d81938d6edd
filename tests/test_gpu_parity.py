"""GPU parity: the HIP step path (through the libevac C ABI) against the oracle on identical inputs.

The bar (BASELINE.json north_star): fp32 results within 1e-5 of the NumPy reference on identical
state / actions / noise; statuses, flags and counts exact.  The oracle runs in the REFERENCE's
precision (f64 pedestrians) from the same f32-representable inputs the GPU gets.  A threshold
comparison whose f64 margin is below 1e-6 may legitimately flip in f32 (SURVEY.md 7 'Parity
definition'); such envs are excluded from the element-wise check and counted.
"""
import os

import numpy as np
import pytest

from oracle import evac_oracle as O
from oracle import philox as P
from tests import helpers as H

pytestmark = pytest.mark.gpu

ATOL = 1e-5
TIE = 1e-6


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    import evacuation_amd
    from evacuation_amd import _lib
    _lib.load()
    return evacuation_amd


def cfg_from_params(ea, p: O.OracleParams, **kw):
    d = {k: getattr(p, k) for k in ("number_of_pedestrians", "width", "height", "step_size", "noise_coef", "eps",
                                    "enslaving_degree", "is_new_exiting_reward", "is_new_followers_reward",
                                    "intrinsic_reward_coef", "is_termination_agent_wall_collision",
                                    "init_reward_each_step", "max_timesteps")}
    d.update(kw)
    return ea.EnvConfig(**d)


def f32_state(st: O.OracleState) -> O.OracleState:
    """Round the pedestrian state to f32 (what the GPU holds) but keep the reference's f64 dtype."""
    s = st.copy()
    s.pos = s.pos.astype(np.float32).astype(np.float64)
    s.dir = s.dir.astype(np.float32).astype(np.float64)
    return s


def gpu_step_batch(ea, p, wrap, states, actions, noise, autoreset=False):
    """Each state is one env of a batch; ONE evac_step launch."""
    env = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=len(states), autoreset=autoreset)
    env.set_state(pos=np.stack([s.pos for s in states]).astype(np.float32),
                  dir=np.stack([s.dir for s in states]).astype(np.float32),
                  status=np.stack([s.status for s in states]).astype(np.uint8),
                  agent_pos=np.stack([s.agent_pos for s in states]).astype(np.float32),
                  agent_dir=np.stack([s.agent_dir for s in states]).astype(np.float32),
                  now=np.array([s.now for s in states], dtype=np.int32))
    obs, rew, term, trunc, _ = env.step(np.asarray(actions, dtype=np.float32), noise=np.asarray(noise, dtype=np.float32))
    st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    out = dict(obs=obs.cpu().numpy().copy(), reward=rew.cpu().numpy().copy(), terminated=term.cpu().numpy().astype(bool),
               truncated=trunc.cpu().numpy().astype(bool), **st)
    env.close()
    return out


def flat_oracle_obs(st, wrap, eps):
    o = O.observe(st, wrap.positions, wrap.statuses, wrap.type, alpha=wrap.alpha, eps=eps)
    if wrap.positions == "grav":
        return np.concatenate([o["agent_position"], o["grad_potential_exit"], o["grad_potential_pedestrians"]]).astype(np.float64)
    if wrap.type == "Box":
        return np.asarray(o, dtype=np.float64).reshape(-1)
    parts = [o["agent_position"], o["exit_position"], o["pedestrians_positions"].reshape(-1)]
    if "pedestrians_statuses" in o:
        parts.append(np.asarray(o["pedestrians_statuses"]).reshape(-1))
    return np.concatenate(parts).astype(np.float64)


def grav_tolerance(st, alpha, eps):
    """Absolute tolerance for the gravity sums: 1e-5 relative to the sum of |terms| (an f32 sum of
    terms up to alpha/0.2^(alpha+1) cannot be held to an absolute 1e-5)."""
    m = st.status == O.VISCEK
    r = st.agent_pos.astype(np.float64)[None, :] - st.pos[m]
    scale = 1.0
    if len(r):
        nrm = np.linalg.norm(r, axis=1) + eps
        scale += float(np.sum(alpha / nrm ** (alpha + 1)))
    re = st.agent_pos.astype(np.float64) - O.EXIT_POSITION
    nf = float(np.sum(st.status == O.FOLLOWER))
    scale_exit = 1.0 + nf * alpha / (np.linalg.norm(re) + eps) ** (alpha + 1)
    return 1e-5 * scale, 1e-5 * scale_exit


TIE_LOG = []      # (fixture or case, envs, envs with a near-tie, of them resolved either way, pedestrians excluded): printed at the end of the session (conftest)


def legal_statuses(p, pos_i, agent_pos):
    """The statuses pedestrian i may legally get when a threshold comparison of statuses.py:29-48 lies within TIE of its radius: each
    such comparison may come out either way in f32 (both are 'the reference's result up to rounding'); the others are fixed."""
    d_lead = float(np.linalg.norm(pos_i - np.asarray(agent_pos, dtype=np.float64)))
    d_exit = float(np.linalg.norm(pos_i - O.EXIT_POSITION.astype(np.float64)))
    opts = []
    for d, r in ((d_lead, O.R_LEADER), (d_exit, O.R_EXIT), (d_exit, O.R_ESCAPE)):
        opts.append((True, False) if abs(d - r) < TIE else ((d < r),))
    out = set()
    for f in opts[0]:
        for e1 in opts[1]:
            for e2 in opts[2]:
                out.add(O.ESCAPED if e2 else (O.EXITING if e1 else (O.FOLLOWER if f else O.VISCEK)))
    return out


def oracle_step(p, pre, action, noise):
    """The oracle's step from the f32-rounded pre-state: (post-state, env_step's dict, per-pedestrian near-tie mask, pre-step
    statuses, whether the post-state is finite) -- what compare_step holds a kernel's outputs against."""
    st = f32_state(pre)
    pre_pos = st.pos.copy()
    old_status = st.status.copy()
    with np.errstate(all="ignore"):
        out = O.env_step(p, st, np.asarray(action, dtype=np.float32), np.asarray(noise, dtype=np.float32).astype(np.float64))
    finite = np.isfinite(st.pos).all()
    tied = np.zeros(len(st.status), bool)
    if finite:
        tied = O.threshold_margins_per_pedestrian(st.pos, st.agent_pos, pre_pos, p.width, p.height, st.status) < TIE
    return st, out, tied, old_status, finite


def compare_step(p, wrap, pre_states, actions, noise, got, min_checked=1, label=None, oracle=None, reset=None, counts=None):
    """Oracle (reference precision) from the same f32-representable inputs vs the GPU outputs.  A comparison whose f64 margin is
    below TIE may legitimately flip in f32: the pedestrians it involves are left out of the element-wise comparison (positions,
    directions, statuses of every OTHER pedestrian of that env are still compared).  The env-level outputs of such an env (rewards,
    flags, observation sums -- they depend on every status) are checked EITHER WAY: when the tie is one of
    the status thresholds -- the pedestrian's position and direction agree with the oracle's, only its class is in question --
    the GPU's class must be one of the legal outcomes, and the oracle's reward / termination / observation are re-evaluated with it;
    only a tie that changed a pedestrian's MOTION (a pair of the neighbour test, a wall test) still skips the env-level outputs.
    All counts are returned and logged.

    `oracle`: the `oracle_step` of every env, computed beforehand (a caller that compares several kernels on the same inputs
    steps the oracle once).  `reset[e]`: env e autoreset in the same step (a rollout kernel), so its state and observation are
    the reset's and the caller checks them: only the flags and the reward are compared here, and a near-tie in that env skips
    them.  `counts` (a dict) accumulates the envs whose env-level outputs were checked and the pedestrians left out."""
    checked = ties = resolved = peds_out = 0
    worst = 0.0
    for e, pre in enumerate(pre_states):
        st, out, tied, old_status, finite = oracle[e] if oracle is not None else oracle_step(p, pre, actions[e], noise[e])
        st = st.copy()
        moved = reset is None or not reset[e]
        ok = ~tied
        if moved:
            np.testing.assert_array_equal(got["status"][e][ok], st.status[ok], err_msg=f"env {e} status")
            np.testing.assert_allclose(got["pos"][e][ok], st.pos[ok], rtol=0, atol=ATOL, equal_nan=True, err_msg=f"env {e} pos")
            np.testing.assert_allclose(got["dir"][e][ok], st.dir[ok], rtol=0, atol=ATOL, equal_nan=True, err_msg=f"env {e} dir")
            np.testing.assert_allclose(got["agent_pos"][e], st.agent_pos, rtol=0, atol=1e-7)
            # (1e-8, or 2.5 ulp of the step size where that is more -- from a step of 0.06 on: the kernel multiplies by a reciprocal
            # where area.py:190 divides, which may differ by 2 ulp of the direction)
            np.testing.assert_allclose(got["agent_dir"][e], st.agent_dir, rtol=0, atol=max(1e-8, 2.5 * float(np.spacing(np.float32(p.step_size)))))
            assert got["now"][e] == st.now
        assert bool(got["truncated"][e]) == out["truncated"], f"env {e} truncated"
        if moved and finite and ok.any():
            worst = max(worst, float(np.abs(got["pos"][e][ok] - st.pos[ok]).max()), float(np.abs(got["dir"][e][ok] - st.dir[ok]).max()))
        ref_reward, ref_term = out["reward"], out["terminated"]
        if tied.any():
            ties += 1
            peds_out += int(tied.sum())
            if not moved:
                continue                                                   # (the state is the reset's: the tie's outcome cannot be seen)
            # status-only ties: same motion, class in question -> take the GPU's class if it is a legal one and re-evaluate
            idx = np.nonzero(tied)[0]
            same_motion = (np.abs(got["pos"][e][idx] - st.pos[idx]).max() <= ATOL) and (np.abs(got["dir"][e][idx] - st.dir[idx]).max() <= ATOL)
            if not same_motion:
                continue                                                   # (a pair / wall tie moved the pedestrian elsewhere: no env-level check)
            alt = st.status.copy()
            for i in idx:
                g = int(got["status"][e][i])
                assert g in legal_statuses(p, st.pos[i], st.agent_pos), f"env {e} pedestrian {i}: status {g} is no legal outcome of its near-tie"
                alt[i] = g
            st.status = alt
            r_ped = O.status_reward(p, old_status, alt, st.now)
            ref_reward = out["reward_agent"] + r_ped + p.intrinsic_reward_coef * out["intrinsic"]
            term_agent = bool(out["reward_agent"] != 0.0 and p.is_termination_agent_wall_collision)     # area.py:196-199
            ref_term = bool(term_agent or np.all(alt == O.ESCAPED))                                      # area.py:175-178, env.py:171
            resolved += 1
        checked += 1
        np.testing.assert_allclose(got["reward"][e], ref_reward, rtol=1e-5, atol=1e-5, equal_nan=True, err_msg=f"env {e} reward")
        assert bool(got["terminated"][e]) == ref_term, f"env {e} terminated"
        if not moved:
            continue                                                       # (the observation is the reset's: the caller checks it)
        ref_obs = flat_oracle_obs(st, wrap, p.eps)
        if wrap.positions == "grav":
            tol_p, tol_e = grav_tolerance(st, wrap.alpha, p.eps)
            np.testing.assert_allclose(got["obs"][e][0:2], ref_obs[0:2], rtol=0, atol=1e-7, equal_nan=True)
            np.testing.assert_allclose(got["obs"][e][2:4], ref_obs[2:4], rtol=2e-5, atol=tol_e, equal_nan=True, err_msg=f"env {e} grad_exit")
            np.testing.assert_allclose(got["obs"][e][4:6], ref_obs[4:6], rtol=2e-5, atol=tol_p, equal_nan=True, err_msg=f"env {e} grad_ped")
        else:
            np.testing.assert_allclose(got["obs"][e], ref_obs, rtol=0, atol=ATOL, equal_nan=True, err_msg=f"env {e} obs")
    assert checked >= min_checked, (checked, ties)
    if counts is not None:
        counts["checked"] = counts.get("checked", 0) + checked
        counts["peds_out"] = counts.get("peds_out", 0) + peds_out
    if label is not None:
        TIE_LOG.append((label, len(pre_states), ties, resolved, peds_out))
    return checked, ties, worst


WRAPS = [dict(positions="grav", alpha=3), dict(positions="grav", alpha=2), dict(positions="grav", alpha=5),
         dict(positions="grav", alpha=2.5),
         dict(positions="abs"), dict(positions="rel"), dict(positions="abs", statuses="ohe"),
         dict(positions="rel", statuses="cat"), dict(positions="rel", statuses="ohe", type="Box"),
         dict(positions="abs", statuses="cat", type="Box"), dict(positions="rel", statuses="no", type="Box")]


@pytest.mark.parametrize("path", H.traj_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_teacher_forced_steps_match_reference_fixtures(ea, path):
    """Every recorded reference step becomes one env of a batch: same pre-state, action, noise."""
    d = np.load(path)
    p = H.load_params(d["params_json"])
    K = len(d["action"])
    pre = [H.state_at(d, k) for k in range(K)]
    # Steps with a near-tie somewhere: a status-threshold tie is checked either way, a tie that moved a pedestrian skips the env-level
    # outputs of that step (compare_step).  A follower that keeps its distance to the leader (enslaving_degree 1) carries the same
    # near-tie from step to step, so the bound scales with the fixture's length; the counts are printed at the end of the session
    # (TIE_LOG), so that a silent growth is visible.
    total_ties = 0
    for i, w in enumerate(WRAPS):
        wrap = ea.EnvWrappersConfig(**w)
        got = gpu_step_batch(ea, p, wrap, pre, d["action"], d["noise"])
        checked, ties, worst = compare_step(p, wrap, pre, d["action"], d["noise"], got, min_checked=max(1, K - max(4, K // 5)),
                                            label=os.path.basename(path)[:-4] if i == 0 else None)
        total_ties = max(total_ties, ties)
        assert worst < 2e-6, worst          # in practice a few f32 ulp
    assert total_ties <= max(4, K // 5)


@pytest.mark.parametrize("name,c", list(H.crafted_cases()), ids=[n for n, _ in H.crafted_cases()])
def test_crafted_edge_cases(ea, name, c):
    """Leader wall hit, corner reflection, landing on the exit, all-escaped termination, truncation,
    reward transitions, empty noise draw, NaN poisoning (area.py:101), zero action, zero mean heading."""
    p = H.load_params(c["params_json"])
    pre = O.OracleState(c["pre_pos"].copy(), c["pre_dir"].copy(), c["pre_status"].copy(), c["pre_agent_pos"].copy(),
                        c["pre_agent_dir"].copy(), int(c["pre_now"]))
    for w in (dict(positions="grav", alpha=3), dict(positions="rel", statuses="ohe", type="Box"), dict(positions="abs", statuses="cat")):
        wrap = ea.EnvWrappersConfig(**w)
        got = gpu_step_batch(ea, p, wrap, [pre], [c["action"]], [c["noise"]])
        compare_step(p, wrap, [pre], [c["action"]], [c["noise"]], got)
        # and against the reference's own recorded outputs
        np.testing.assert_array_equal(got["status"][0], c["post_status"])
        np.testing.assert_allclose(got["pos"][0], c["post_pos"], rtol=0, atol=ATOL, equal_nan=True)
        np.testing.assert_allclose(got["reward"][0], c["reward"], rtol=1e-5, atol=1e-5, equal_nan=True)
        assert bool(got["terminated"][0]) == bool(c["terminated"]) and bool(got["truncated"][0]) == bool(c["truncated"])


def test_nan_guard_is_opt_in(ea):
    c = dict(H.crafted_cases())["nan_poison_zero_heading"]
    p = H.load_params(c["params_json"])
    env = ea.BatchedEvacuationEnv(cfg_from_params(ea, p, nan_guard=True), ea.EnvWrappersConfig(), num_envs=1, autoreset=False)
    env.set_state(pos=c["pre_pos"][None].astype(np.float32), dir=c["pre_dir"][None].astype(np.float32),
                  status=c["pre_status"][None].astype(np.uint8), agent_pos=c["pre_agent_pos"][None],
                  agent_dir=c["pre_agent_dir"][None], now=np.array([int(c["pre_now"])], dtype=np.int32))
    env.step(c["action"][None].astype(np.float32), noise=c["noise"][None].astype(np.float32))
    st = env.get_state()
    assert np.isfinite(st["pos"].cpu().numpy()).all()


@pytest.mark.parametrize("path", H.traj_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_reset_from_injected_draws(ea, path):
    d = np.load(path)
    p = H.load_params(d["params_json"])
    draws = np.concatenate([d["draw_pos"], d["draw_dir"]], axis=1).astype(np.float32)[None]
    for w in (dict(positions="grav", alpha=3), dict(positions="rel", statuses="ohe", type="Box")):
        wrap = ea.EnvWrappersConfig(**w)
        env = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=1, autoreset=False)
        obs, _ = env.reset(draws=draws)
        obs = obs.cpu().numpy().copy()
        st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
        check_reset(p, wrap, draws[0], {k: v[0] for k, v in st.items()}, obs[0])
        env.close()


def check_reset(p, wrap, draws, st, obs, label=""):
    """One env's state `st` (get_state, one row) and observation `obs` after a reset from `draws` [N, 4] against O.env_reset:
    positions bit-equal, directions to 1e-6; statuses and the observation where no status threshold lies within TIE.
    Returns whether those were compared."""
    ref = O.env_reset(p, draws[:, 0:2].astype(np.float64), draws[:, 2:4].astype(np.float64))
    np.testing.assert_array_equal(st["pos"], ref.pos.astype(np.float32), err_msg=f"{label} reset pos")
    np.testing.assert_allclose(st["dir"], ref.dir, rtol=0, atol=1e-6, err_msg=f"{label} reset dir")
    compared = O.threshold_margin(ref.pos, ref.agent_pos, None, p.width, p.height) > TIE
    if compared:
        np.testing.assert_array_equal(st["status"], ref.status, err_msg=f"{label} reset status")
        ref_obs = flat_oracle_obs(ref, wrap, p.eps)
        if wrap.positions == "grav":
            tol_p, tol_e = grav_tolerance(ref, wrap.alpha, p.eps)
            np.testing.assert_allclose(obs[4:6], ref_obs[4:6], rtol=2e-5, atol=tol_p, err_msg=f"{label} reset obs")
            np.testing.assert_allclose(obs[0:4], ref_obs[0:4], rtol=2e-5, atol=tol_e, err_msg=f"{label} reset obs")
        else:
            np.testing.assert_allclose(obs, ref_obs, rtol=0, atol=ATOL, err_msg=f"{label} reset obs")
    assert (st["agent_pos"] == 0).all() and (st["agent_dir"] == 0).all() and st["now"] == 0, label
    return compared


@pytest.mark.parametrize("n", [1, 2, 33, 64, 65, 100, 256, 300, 512, 600, 1024])
def test_random_states_all_sizes(ea, n):
    """Kernel geometry edges (1 wave, 4/8/16-wave workgroups, ragged last wave) on oracle-generated
    states: random reset, a few oracle steps to mix statuses, then one teacher-forced step."""
    p, pre, acts, nzs = H.random_states(n)
    E = len(pre)
    for w in (dict(positions="grav", alpha=3), dict(positions="rel", statuses="ohe", type="Box")):
        wrap = ea.EnvWrappersConfig(**w)
        got = gpu_step_batch(ea, p, wrap, pre, acts, nzs)
        compare_step(p, wrap, pre, acts, nzs, got, min_checked=E - 2)


@pytest.mark.parametrize("n", [60, 256, 512, 600, 1024])
def test_late_episode_states_with_few_rows(ea, n):
    """Late in an episode most pedestrians have escaped, the crowd hangs on the leader and, under enslaving_degree 1, only
    the few VISCEK pedestrians need a row of the distance matrix: the kernels then compact rows and columns (all-pairs
    families) or deal the rows to the waves and sweep the tile with the lanes (cell-list family, N > 512).  Crafted states of
    that kind -- 80 % escaped, a flock around the leader, a handful of loners, one dense knot -- one teacher-forced step
    against the reference-precision oracle."""
    p, pre, acts, nzs = H.late_episode_states(n)
    for w in (dict(positions="grav", alpha=3), dict(positions="rel", statuses="ohe", type="Box")):
        wrap = ea.EnvWrappersConfig(**w)
        got = gpu_step_batch(ea, p, wrap, pre, acts, nzs)
        compare_step(p, wrap, pre, acts, nzs, got, min_checked=2)


@pytest.mark.parametrize("fixture", ["traj_n60_s1_noise05_ens05", "traj_n256_s5"])
def test_free_running_50_steps_vs_reference_fixture(ea, fixture):
    """Same reset draws, actions and per-pedestrian noise as the reference episode; free-running (N = 60: one wave per env;
    N = 256: four waves per env, the row-blocked all-pairs sweep)."""
    d = np.load(os.path.join(H.GOLDEN, fixture + ".npz"))
    p = H.load_params(d["params_json"])
    env = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), ea.EnvWrappersConfig(positions="grav", alpha=3), num_envs=1, autoreset=False)
    draws = np.concatenate([d["draw_pos"], d["draw_dir"]], axis=1).astype(np.float32)[None]
    env.reset(draws=draws)
    for k in range(50):
        obs, r, te, tr, _ = env.step(d["action"][k][None], noise=d["noise"][k][None].astype(np.float32))
        st = env.get_state()
        np.testing.assert_allclose(st["pos"].cpu().numpy()[0], d["pos"][k + 1], rtol=0, atol=ATOL, err_msg=f"step {k}")
        np.testing.assert_array_equal(st["status"].cpu().numpy()[0], d["status"][k + 1])
        np.testing.assert_allclose(float(r[0]), d["reward"][k], rtol=1e-5, atol=1e-4)
    env.close()


def test_philox_reset_and_noise_are_bit_exact(ea):
    """Device Philox streams == oracle/philox.py, for a handle with an env_id_offset."""
    n, E, seed, off = 60, 5, 0x5EED0001, 37
    p = O.OracleParams(number_of_pedestrians=n)
    env = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), ea.EnvWrappersConfig(positions="grav"), num_envs=E, seed=seed,
                                  env_id_offset=off, autoreset=False)
    env.reset()
    st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    draws = P.reset_draws(seed, off + np.arange(E), n, 0)
    np.testing.assert_array_equal(st["pos"], draws[..., 0:2])
    nrm = np.sqrt(draws[..., 2] ** 2 + draws[..., 3] ** 2)
    np.testing.assert_allclose(st["dir"], draws[..., 2:4] / nrm[..., None], rtol=0, atol=2e-7)
    # one Philox step == the same step with the oracle's noise injected
    act = np.tile(np.array([[0.3, -0.8]], dtype=np.float32), (E, 1))
    env2 = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), ea.EnvWrappersConfig(positions="grav"), num_envs=E, seed=seed,
                                   env_id_offset=off, autoreset=False)
    env2.reset()
    for t in range(6):       # crosses the 4-step Philox block boundary
        env.step(act)
        env2.step(act, noise=P.step_noise(seed, off + np.arange(E), n, t, p.noise_coef))
        a, b = env.get_state(), env2.get_state()
        for k in a:
            assert (a[k] == b[k]).all(), (t, k)
    env.close(); env2.close()


def test_rollout_equals_step_by_step_and_oracle(ea):
    """evac_rollout (T steps, one launch, RandomAgent actions on device) is bit-identical to T
    evac_step launches fed the same actions, and within 1e-5 of the oracle for the first steps."""
    n, E, T, seed = 60, 8, 40, 0x5EED0002
    p = O.OracleParams(number_of_pedestrians=n, is_new_exiting_reward=True, max_timesteps=25)   # truncation + autoreset inside
    wrap = ea.EnvWrappersConfig(positions="grav", alpha=3)
    a = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=E, seed=seed)
    b = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=E, seed=seed)
    a.reset(); b.reset()
    ro = a.rollout(T, record_actions=True)
    acts = ro["actions"].cpu().numpy()
    np.testing.assert_array_equal(acts[0], P.random_action(seed, np.arange(E), 0))
    np.testing.assert_array_equal(acts[7], P.random_action(seed, np.arange(E), 7))
    n_done = 0
    for t in range(T):
        obs, r, te, tr, info = b.step(ro["actions"][t].contiguous())
        assert (obs == ro["obs"][t]).all(), t
        assert (r == ro["reward"][t]).all() and (te == ro["terminated"][t]).all() and (tr == ro["truncated"][t]).all(), t
        done = (te | tr).bool()
        n_done += int(done.sum())
        if done.any():
            assert (info["episode_stats"][done] == ro["episode_stats"][t][done]).all()
    assert n_done >= E                                   # every env truncated at least once
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    # oracle free-run on env 3 with the same Philox draws
    e = 3
    dr = P.reset_draws(seed, [e], n, 0)[0]
    st = O.env_reset(p, dr[:, 0:2].astype(np.float64), dr[:, 2:4].astype(np.float64))
    rew = ro["reward"].cpu().numpy()
    for t in range(20):
        out = O.env_step(p, st, acts[t, e], P.step_noise(seed, [e], n, t, p.noise_coef)[0].astype(np.float64))
        np.testing.assert_allclose(rew[t, e], out["reward"], rtol=1e-5, atol=1e-4, err_msg=f"t={t}")
    a.close(); b.close()


def test_autoreset_semantics(ea):
    """Same-step autoreset (gymnasium 0.29 SyncVectorEnv, rpo_agent.py:193-203): obs is the reset
    obs, final_observation the terminal one, episode stats recorded, state re-drawn from Philox."""
    n, E, seed = 30, 4, 99
    p = O.OracleParams(number_of_pedestrians=n, max_timesteps=3)
    wrap = ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box")
    env = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=E, seed=seed)
    twin = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=E, seed=seed, autoreset=False)
    env.reset(); twin.reset()
    act = np.tile(np.array([[1.0, 0.5]], dtype=np.float32), (E, 1))
    ret = np.zeros(E)
    for t in range(3):
        obs, r, te, tr, info = env.step(act)
        o2, r2, _, tr2, _ = twin.step(act)
        ret += r.cpu().numpy()
        assert (r == r2).all() and (tr == tr2).all()
    assert tr.bool().all() and not te.bool().any()
    assert (info["final_observation"] == o2).all()              # terminal obs preserved
    stats = info["episode_stats"].cpu().numpy()
    np.testing.assert_allclose(stats[:, 0], ret, rtol=1e-6)
    assert (stats[:, 1] == 3).all() and (stats[:, 4:8].sum(axis=1) == n).all()
    fin = env.final_info_list(info)
    assert fin[0]["episode"]["l"] == 3 and abs(fin[0]["episode"]["r"] - ret[0]) < 1e-4
    st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    np.testing.assert_array_equal(st["pos"], P.reset_draws(seed, np.arange(E), n, 1)[..., 0:2])   # second reset of each env
    assert (st["now"] == 0).all() and (st["agent_pos"] == 0).all()
    assert (env.clock[:, 1] == 2).all() and (env.clock[:, 2] == 3).all()
    assert (env.observe(out=obs.clone()) == obs).all()          # returned obs == obs of the fresh state
    env.close(); twin.close()


def test_sharded_handles_reproduce_single_handle(ea):
    """env_id_offset keys the Philox streams by GLOBAL env id: 2 shards == 1 big batch, bit for bit."""
    n, E, seed, T = 60, 16, 5, 30
    p = O.OracleParams(number_of_pedestrians=n, max_timesteps=20)
    wrap = ea.EnvWrappersConfig(positions="grav", alpha=3)
    whole = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=E, seed=seed)
    lo = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=E // 2, seed=seed, env_id_offset=0)
    hi = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=E // 2, seed=seed, env_id_offset=E // 2)
    for e in (whole, lo, hi):
        e.reset()
    rw, rl, rh = whole.rollout(T), lo.rollout(T), hi.rollout(T)
    for k in ("obs", "reward", "terminated", "truncated"):
        assert (rw[k][:, :E // 2] == rl[k]).all() and (rw[k][:, E // 2:] == rh[k]).all(), k


@pytest.mark.parametrize("parts,E,n", [(2, 64, 60), (4, 64, 60), (2, 8, 256)])
def test_split_batch_equals_one_handle(ea, parts, E, n):
    """SplitBatchEnv: one batch as `parts` independent handles on streams of their own (env_id_offset keys the random streams by
    global env id): the concatenated outputs of several launches, an autoreset among them, equal the single handle's bit for bit."""
    import torch
    cfg = ea.EnvConfig(number_of_pedestrians=n, max_timesteps=25, is_new_exiting_reward=True, is_new_followers_reward=True)
    wrap = ea.EnvWrappersConfig(positions="grav", alpha=3)
    whole = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=9)
    split = ea.SplitBatchEnv(cfg, wrap, num_envs=E, parts=parts, seed=9)
    assert len(split.parts) == parts and len({s.cuda_stream for s in split.streams}) == parts
    whole.reset()
    split.reset()
    launch, outs = split.rollout_launcher(10)
    for j in range(4):                                  # 40 steps: every env is truncated and reset once
        ref = whole.rollout(10)
        launch()
        split.synchronize()
        torch.cuda.synchronize()
        got = torch.cat([o["slab"] for o in outs], dim=1)
        assert torch.equal(got, ref["slab"]), f"launch {j}"
        done = (ref["terminated"] != 0) | (ref["truncated"] != 0)           # (the records' rows are valid where an episode ended)
        assert torch.equal(torch.cat([o["episode_stats"] for o in outs], dim=1)[done], ref["episode_stats"][done]), f"launch {j}: episode records"
        assert j != 2 or bool(done.any())
    one = split.rollout(5)                              # the convenience form: joined on the current stream, concatenated
    assert torch.equal(one["slab"], whole.rollout(5)["slab"])
    with pytest.raises(ValueError):
        ea.SplitBatchEnv(cfg, wrap, num_envs=E + 1, parts=parts)
    split.close()
    whole.close()


@pytest.mark.parametrize("n,E,wrap_kw,parts", [
    (60, 512, dict(positions="grav", alpha=3), 2),                            # CU-wide one-wave envs, forced (the batch would not ask for it)
    (60, 4096, dict(positions="grav", alpha=3), -1),                          # BASELINE config 2: the automatic choice IS two parts
    (200, 64, dict(positions="grav", alpha=3), 2),                            # four-wave envs
    (60, 100, dict(positions="rel", statuses="ohe", type="Box"), 2),          # 256-thread workgroups, generic observation
    (20, 90, dict(positions="abs", statuses="cat", type="Dict"), 2),          # sub-wave kernels (their own rollout scaffolding)
])
def test_two_parts_on_the_handles_own_streams_equal_one_kernel(ea, n, E, wrap_kw, parts):
    """evac_options_t.parts = 2: ONE handle, ONE slab, evac_rollout issued as two half-batch kernels on two
    streams the handle owns; bit-identical to the single-kernel handle over several launches with an autoreset among them, with
    RandomAgent and with given actions; evac_join orders the caller's stream behind both; every other call joins by itself."""
    import torch
    cfg = ea.EnvConfig(number_of_pedestrians=n, max_timesteps=25, is_new_exiting_reward=True, is_new_followers_reward=True)
    wrap = ea.EnvWrappersConfig(**wrap_kw)
    one = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=9, options=ea.KernelOptions(parts=1))
    two = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=9, options=ea.KernelOptions(parts=parts))
    assert one.num_parts == 1 and one.part_streams() == [] and "streams" not in one.kernel_variant()
    assert two.num_parts == 2 and two.resolved_options().parts == 2 and two.kernel_variant().endswith("x 2 streams")
    s0, s1 = two.part_streams()
    assert s0.cuda_stream != s1.cuda_stream and torch.cuda.current_stream().cuda_stream not in (s0.cuda_stream, s1.cuda_stream)
    one.reset(); two.reset()
    T, D = 10, one.obs_dim
    out = {"slab": torch.empty((T, E, D + 3), device=two.device), "episode_stats": torch.zeros((T, E, two.stats_words), device=two.device)}
    launch = two.rollout_launcher(T, out)
    for j in range(4):                                   # 40 steps: every env is truncated and reset once
        ref = one.rollout(T)
        launch()                                         # (asynchronous to the current stream until join)
        two.join()
        torch.cuda.current_stream().synchronize()        # ONLY the caller's stream: it was made to wait for both parts
        assert torch.equal(out["slab"], ref["slab"]), f"launch {j}"
        done = (ref["terminated"] != 0) | (ref["truncated"] != 0)
        assert torch.equal(out["episode_stats"][done], ref["episode_stats"][done]), f"launch {j}: episode records"
        assert j != 2 or bool(done.any())
    acts = torch.rand((7, E, 2), device=two.device) * 2 - 1
    a, b = one.rollout(7, actions=acts), two.rollout(7, actions=acts)      # rollout() joins by itself
    assert torch.equal(a["slab"], b["slab"])
    # back-to-back launches without a join between them, then a call that is not a plain rollout: it joins by itself
    o3 = {"slab": torch.empty((3, E, D + 3), device=two.device)}
    l3 = two.rollout_launcher(3, o3)
    for _ in range(5):
        one.rollout(3)
        l3()
    sa, sb = one.get_state(), two.get_state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    # the per-step API and the diagnostic rollout face run as one kernel on the caller's stream, on the same state
    act1 = torch.rand((E, 2), device=two.device) * 2 - 1
    ra, rb = one.step(act1), two.step(act1)
    for x, y in zip(ra[:4], rb[:4]):
        assert torch.equal(x, y)
    ca, cb = one.rollout(4, record_actions=True, capture_envs=2), two.rollout(4, record_actions=True, capture_envs=2)
    assert torch.equal(ca["slab"], cb["slab"]) and torch.equal(ca["trajectory"], cb["trajectory"]) and torch.equal(ca["actions"], cb["actions"])
    assert torch.equal(one.rollout(6)["slab"], two.rollout(6)["slab"])
    one.close(); two.close()


def _where_slabs_differ(outs, refs, replay=None):
    """The failure message of the chained-launch comparison: which launches, steps, envs and slab columns differ -- and, given a
    replay of the same launches by a third handle (one launch at a time), which of the two sides left it."""
    import torch
    lines = []
    if replay is not None:
        R = len(outs)
        last = replay[-R:]
        for name, side in (("chained", outs), ("plain", refs)):
            off = [j for j, (a, b) in enumerate(zip(side, last)) if not torch.equal(a["slab"], b["slab"])]
            lines.append(f"{name} side differs from a serial replay in launches {off}")
            for j in off[:2]:          # ... at which granularity, and with what in them?
                a, b = side[j]["slab"].flatten(), last[j]["slab"].flatten()
                ne = (a != b).nonzero().flatten()
                addr = a.data_ptr() + 4 * ne
                line = torch.unique(addr // 128)
                in_wrong_lines = torch.isin((a.data_ptr() + 4 * torch.arange(a.numel(), device=a.device)) // 128, line)
                could = int((in_wrong_lines & (b != 0)).sum())          # floats of the wrong lines that would show if the line were zero
                zeros = int((a[ne] == 0).sum())
                import time
                time.sleep(0.3); torch.cuda.synchronize()
                healed = bool(torch.equal(side[j]["slab"], last[j]["slab"]))
                lines.append(f"  {name} launch {j}: {ne.numel()} wrong floats in {line.numel()} lines of 128 B ({zeros} of them read 0.0; a zeroed line would show {could}); "
                             f"tensor at {a.data_ptr():#x} ({a.numel() * 4} B); first wrong lines at +{[(int(x) * 128 - a.data_ptr()) for x in line[:6].tolist()]}; "
                             f"a few wrong values {[float(x) for x in a[ne][:6].tolist()]} for {[float(x) for x in b[ne][:6].tolist()]}; equal after 0.3 s: {healed}")
            for j in off[:4]:          # where do the wrong rows come from?  the same (step, env) row of which launch of the whole run
                bad = (side[j]["slab"] != last[j]["slab"]).any(dim=2)
                t, e = torch.nonzero(bad, as_tuple=True)
                src = {}
                for tt, ee in list(zip(t.tolist(), e.tolist()))[:40]:
                    row = side[j]["slab"][tt, ee]
                    hit = [k for k in range(len(replay)) if torch.equal(replay[k]["slab"][tt, ee], row)]
                    hit2 = [(k, t2) for k in range(len(replay)) for t2 in range(replay[k]["slab"].shape[0]) if t2 != tt and torch.equal(replay[k]["slab"][t2, ee], row)][:2] if not hit else []
                    key = str(hit) if hit else ("other step " + str(hit2) if hit2 else ("zeros" if not bool(row.any()) else "nowhere"))
                    src[key] = src.get(key, 0) + 1
                lines.append(f"  {name} launch {j} (run launch {len(replay) - R + j}): {int(bad.sum())} wrong rows; the same row of run launch -> {src}")
    for j, (o, r) in enumerate(zip(outs, refs)):
        ne = o["slab"] != r["slab"]
        ne |= torch.isnan(o["slab"]) != torch.isnan(r["slab"])
        if not bool(ne.any()):
            continue
        t, e, c = (x.unique().tolist() for x in torch.nonzero(ne, as_tuple=True))
        lines.append(f"launch {j}: {int(ne.sum())} values; steps {t[:12]}{'...' if len(t) > 12 else ''}; {len(e)} envs {e[:24]}{'...' if len(e) > 24 else ''}; "
                     f"{len(c)} columns {c[:8]}..{c[-1]}")
    return " | ".join(lines) if lines else "(equal apart from NaN payloads)"


@pytest.mark.parametrize("n,E,wrap_kw,T,wide,form", [
    (60, 4096, dict(positions="grav", alpha=3), 20, 1, 1),                    # BASELINE config 2 with the driver's launch length
    (60, 512, dict(positions="grav", alpha=3), 7, 1, 1),                       # CU-wide forced on a small batch, odd launch length
    (33, 64, dict(positions="rel", statuses="ohe", type="Box"), 10, 1, 1),      # generic observation, four workgroups
    (64, 160, dict(positions="abs", statuses="cat", type="Dict"), 5, 1, 1),     # the env fills its wave; generic kernels (not the default configuration)
    (256, 1024, dict(positions="grav", alpha=3), 20, 1, 1),                     # BASELINE config 3: four waves per env, four envs per CU-wide workgroup
    (200, 52, dict(positions="rel", statuses="ohe", type="Box"), 6, 1, 1),      # four-wave envs that do not fill their lanes, 13 workgroups, Box observation
    (60, 4096, dict(positions="grav", alpha=3), 20, 0, 1),                     # BASELINE config 2 in 256-thread workgroups (four envs each, no deal)
    (33, 36, dict(positions="rel", statuses="ohe", type="Box"), 9, 0, 1),     # ... a small batch of them, generic observation
    # chain = 2: ONE PERSISTENT KERNEL per join, every launch a command of its ring (the state stays in registers from call to call)
    (60, 4096, dict(positions="grav", alpha=3), 20, 1, 2),
    (33, 64, dict(positions="rel", statuses="ohe", type="Box"), 10, 1, 2),
    (256, 1024, dict(positions="grav", alpha=3), 20, 1, 2),
    (200, 52, dict(positions="rel", statuses="ohe", type="Box"), 6, 1, 2),
    # ... of TEAMS (one env on 8 / 16 CUs): the members of a team agree on every command (BASELINE config 5's shard; a gravity face)
    (1024, 32, dict(positions="rel", statuses="ohe", type="Box"), 6, -1, 2),
    (700, 11, dict(positions="grav", alpha=3), 9, -1, 2),
])
def test_chained_launches_equal_plain_launches(ea, n, E, wrap_kw, T, wide, form):
    """evac_options_t.chain = 1: consecutive rollout launches on two queues, ordered per env by generation
    words on the device.  Slabs, episode records and the final state of many back-to-back launches -- autoresets among them --
    equal the plain handle's bit for bit; calls that are not plain rollouts join and restart the chain behind them."""
    import torch
    cfg = ea.EnvConfig(number_of_pedestrians=n, max_timesteps=45, is_new_exiting_reward=True, is_new_followers_reward=True)
    wrap = ea.EnvWrappersConfig(**wrap_kw)
    one = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=11, options=ea.KernelOptions(cu_wide=wide))
    ch = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=11, options=ea.KernelOptions(cu_wide=wide, chain=form))
    assert ch.own_streams == 2 and ch.num_parts == 1 and ch.resolved_options().chain == form
    assert ("chained" if form == 1 else "persistent") in ch.kernel_variant()
    if wide >= 0:
        assert ("CU-wide" in ch.kernel_variant()) == bool(wide)
    else:
        assert "CUs/env" in ch.kernel_variant(), ch.kernel_variant()
    assert one.own_streams == 0
    one.reset(); ch.reset()
    D = one.obs_dim
    R = 12                                               # launches in flight back to back, each into a buffer of its own
    outs = [{"slab": torch.empty((T, E, D + 3), device=ch.device), "episode_stats": torch.zeros((T, E, ch.stats_words), device=ch.device)} for _ in range(R)]
    goes = [ch.rollout_launcher(T, o) for o in outs]
    for rep in range(3):
        refs = [one.rollout(T) for _ in range(R)]
        for g in goes:
            g()                                          # nothing waits between them: launch j + 1 overlaps launch j
        ch.join()
        torch.cuda.current_stream().synchronize()
        assert ch.team_error(sync=False) == 0
    # (the reference rollouts above reuse no buffer: compare the LAST repetition launch by launch)
    for j, (o, r) in enumerate(zip(outs, refs)):
        if not torch.equal(o["slab"], r["slab"]):
            third = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=11)            # which side is wrong?  the same launches, one at a time
            third.reset()
            replay = []
            for _ in range(3 * R):
                replay.append(third.rollout(T)); torch.cuda.synchronize()
            raise AssertionError(f"launch {j}: " + _where_slabs_differ(outs, refs, replay))
        done = (r["terminated"] != 0) | (r["truncated"] != 0)
        assert torch.equal(o["episode_stats"][done], r["episode_stats"][done]), f"launch {j}: episode records"
    sa, sb = one.get_state(), ch.get_state()             # (joins by itself)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    # a step in between (one kernel on the caller's stream), then the chain again: it restarts behind the step
    act1 = torch.rand((E, 2), device=ch.device) * 2 - 1
    for x, y in zip(one.step(act1)[:4], ch.step(act1)[:4]):
        assert torch.equal(x, y)
    for _ in range(5):
        one.rollout(T); goes[0]()
    assert torch.equal(one.rollout(T)["slab"], ch.rollout(T)["slab"])          # rollout() joins by itself
    acts = torch.rand((T, E, 2), device=ch.device) * 2 - 1
    assert torch.equal(one.rollout(T, actions=acts)["slab"], ch.rollout(T, actions=acts)["slab"])
    assert ch.team_error() == 0
    one.close(); ch.close()


def test_a_chained_launch_that_is_lost_is_reported(ea):
    """Fault injection (team_fault = 1: the last workgroup of the chain's second launch is never run): the third launch waits in
    vain for those envs, its bounded waits give up, the error word is raised and every later call returns ERR_TEAM_ABORTED until
    it is cleared; the handle then issues plain launches and works again after a reset."""
    import torch
    from evacuation_amd import _lib
    cfg = ea.EnvConfig(number_of_pedestrians=60, max_timesteps=100)
    wrap = ea.EnvWrappersConfig(positions="grav", alpha=3)
    ch = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=64, seed=3, options=ea.KernelOptions(cu_wide=1, chain=1, team_fault=1))
    ch.reset()
    out = {"slab": torch.empty((4, 64, ch.obs_dim + 3), device=ch.device)}
    go = ch.rollout_launcher(4, out)
    for _ in range(4):
        go()
    torch.cuda.synchronize()                            # (the waits are bounded: well under a second)
    assert ch.team_error() == 1
    with pytest.raises(_lib.EvacError) as ei:
        ch.get_state()
    assert ei.value.code == _lib.ERR_TEAM_ABORTED and "chained" in str(ei.value)
    ch.team_clear_error()
    assert ch.team_error() == 0 and "chained" not in ch.kernel_variant()
    ch.reset()
    ref = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=64, seed=3)
    ref.reset()
    # (the faulty handle has reset one more time: compare invariants, not bits -- it works and is finite)
    a = ch.rollout(6)
    torch.cuda.synchronize()
    assert torch.isfinite(a["slab"]).all() and a["slab"].shape == ref.rollout(6)["slab"].shape
    ch.close(); ref.close()


def test_a_persistent_kernel_left_without_commands_leaves_and_is_taken_up_again(ea):
    """evac_options_t.chain = 2: a resident kernel that finds no command for ~150 us stores every env's state and its place in the ring and
    ENDS -- a caller who pauses, waits for the device without joining, or turns to another handle never meets a hung or a starved device -- and
    the next call (or the join) starts a kernel that takes every env up where it stopped.  Same bits as plain launches throughout."""
    import time
    import torch
    wrap = ea.EnvWrappersConfig(positions="grav", alpha=3)
    for E, n in ((64, 60), (4096, 60), (24, 200), (12, 1024)):   # a corner of the device; every CU; four-wave envs; teams of 16 CUs
        cfg_ = ea.EnvConfig(number_of_pedestrians=n, max_timesteps=100, is_new_exiting_reward=True, is_new_followers_reward=True)
        cw = 1 if n <= 256 else -1
        one = ea.BatchedEvacuationEnv(cfg_, wrap, num_envs=E, seed=3, options=ea.KernelOptions(cu_wide=cw))
        ch = ea.BatchedEvacuationEnv(cfg_, wrap, num_envs=E, seed=3, options=ea.KernelOptions(cu_wide=cw, chain=2))
        other = ea.BatchedEvacuationEnv(cfg_, wrap, num_envs=E, seed=4, options=ea.KernelOptions(cu_wide=cw, chain=2))      # a second persistent handle
        assert "persistent" in ch.kernel_variant() and "persistent" in other.kernel_variant()
        one.reset(); ch.reset(); other.reset()
        T, R = 4, 9
        outs = [{"slab": torch.empty((T, E, ch.obs_dim + 3), device=ch.device)} for _ in range(R)]
        outs_other = [{"slab": torch.empty((T, E, ch.obs_dim + 3), device=ch.device)} for _ in range(R)]
        refs = [one.rollout(T) for _ in range(R)]
        torch.cuda.synchronize()
        goes = [ch.rollout_launcher(T, o) for o in outs]
        goes_other = [other.rollout_launcher(T, o) for o in outs_other]
        goes[0](); goes[1]()
        time.sleep(0.02)                                         # the kernel leaves for lack of commands ...
        goes[2]()                                                # ... and this call starts one that resumes
        torch.cuda.synchronize()                                 # a device-wide wait WITHOUT a join: returns (the kernel leaves again)
        goes[3](); goes_other[0](); goes[4](); goes_other[1]()   # two persistent handles in turn: neither starves the other for long
        time.sleep(0.005)
        for k in range(5, R):
            goes[k]()
        for k in range(2, R):
            goes_other[k]()
        other.join(); ch.join()
        torch.cuda.synchronize()
        assert ch.team_error(sync=False) == 0 and other.team_error(sync=False) == 0
        for j in range(R):
            assert torch.equal(outs[j]["slab"], refs[j]["slab"]), (E, n, j)
        sa, sb = one.get_state(), ch.get_state()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (E, n, k)
        assert torch.isfinite(outs_other[-1]["slab"]).all()
        one.close(); ch.close(); other.close()


def test_a_persistent_kernels_ring_may_be_lapped(ea):
    """More calls without a join than the command ring holds (1024): the library stops the kernel, waits for it on the host and starts the
    next one -- the results are those of as many plain launches."""
    import torch
    cfg = ea.EnvConfig(number_of_pedestrians=33, max_timesteps=45, is_new_exiting_reward=True, is_new_followers_reward=True)
    wrap = ea.EnvWrappersConfig(positions="grav", alpha=3)
    one = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=32, seed=5, options=ea.KernelOptions(cu_wide=1))
    ch = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=32, seed=5, options=ea.KernelOptions(cu_wide=1, chain=2))
    one.reset(); ch.reset()
    out = {"slab": torch.empty((1, 32, ch.obs_dim + 3), device=ch.device)}
    ref = {"slab": torch.empty((1, 32, ch.obs_dim + 3), device=ch.device)}
    go, go_ref = ch.rollout_launcher(1, out), one.rollout_launcher(1, ref)
    for _ in range(2300):
        go(); go_ref()
    ch.join()
    torch.cuda.synchronize()
    assert ch.team_error(sync=False) == 0
    assert torch.equal(out["slab"], ref["slab"])
    sa, sb = one.get_state(), ch.get_state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    one.close(); ch.close()


def test_full_size_invariants_c2(ea):
    """BASELINE config 2 (N=60 x 4096 envs, gravity obs): size-independent properties after a long
    on-device rollout -- walls, escaped pinned at the exit, status == classifier(position), step
    length, reward bounds, truncation bookkeeping."""
    import torch
    n, E, T = 60, 4096, 300
    cfg = ea.EnvConfig(number_of_pedestrians=n, is_new_exiting_reward=True, max_timesteps=200)
    env = ea.BatchedEvacuationEnv(cfg, ea.EnvWrappersConfig(positions="grav", alpha=3), num_envs=E, seed=0x5EED0001)
    env.reset()
    ro = env.rollout(T)
    torch.cuda.synchronize()
    st = env.get_state()
    pos, dr, status = st["pos"], st["dir"], st["status"]
    assert torch.isfinite(pos).all() and torch.isfinite(ro["obs"]).all() and torch.isfinite(ro["reward"]).all()
    assert (pos.abs() <= 1.0).all()
    esc = status == 4
    assert (pos[esc] == torch.tensor([0.0, -1.0], device=pos.device)).all() or (pos[esc] - torch.tensor([0.0, -1.0], device=pos.device)).norm(dim=-1).max() < 0.01
    # status is a pure function of the position (statuses.py:29-48): recompute with torch f32
    ap = st["agent_pos"][:, None, :]
    d_lead = (pos - ap).norm(dim=-1)
    d_exit = (pos - torch.tensor([0.0, -1.0], device=pos.device)).norm(dim=-1)
    want = torch.ones_like(status)
    want[d_lead < 0.2] = 2
    want[d_exit < 0.4] = 3
    want[d_exit < 0.01] = 4
    near_tie = ((d_lead - 0.2).abs() < 1e-6) | ((d_exit - 0.4).abs() < 1e-6) | ((d_exit - 0.01).abs() < 1e-6)
    assert ((want == status) | near_tie).all()
    assert set(torch.unique(status).tolist()) <= {1, 2, 3, 4}
    # Vicsek pedestrians move exactly one step length
    v = status == 1
    np.testing.assert_allclose(dr[v].norm(dim=-1).cpu().numpy(), cfg.step_size, rtol=1e-5)
    # rewards: -1 per step minus wall penalty plus at most N transition bonuses
    r = ro["reward"]
    assert r.min() >= -6.0 - 1e-4 and r.max() <= -1.0 + 25.0 * n
    # every env was truncated at t=199 (0-based) exactly once in the first 200 steps, then again later
    tr = ro["truncated"].bool()
    assert tr[199].all() and not tr[:199].any()
    stats = ro["episode_stats"][199]
    assert (stats[:, 1] == 200).all() and (stats[:, 4:8].sum(dim=1) == n).all()
    np.testing.assert_allclose(stats[:, 0].cpu().numpy(), r[:200].sum(dim=0).cpu().numpy(), rtol=1e-4)
    env.close()


def test_single_env_facade_matches_reference_surface(ea):
    """setup_env() / reset() / step() with NumPy in/out (src/env/__init__.py:18-21, README.md:69-91)."""
    d = np.load(os.path.join(H.GOLDEN, "traj_n60_s0.npz"))
    p = H.load_params(d["params_json"])
    env = ea.setup_env(cfg_from_params(ea, p), ea.EnvWrappersConfig(positions="abs", statuses="ohe"))
    draws = np.concatenate([d["draw_pos"], d["draw_dir"]], axis=1)
    obs, info = env.reset(options={"draws": draws})
    assert info == {} and set(obs) == {"agent_position", "exit_position", "pedestrians_positions", "pedestrians_statuses"}
    assert obs["pedestrians_positions"].shape == (60, 2) and obs["pedestrians_statuses"].shape == (60, 4)
    np.testing.assert_allclose(obs["pedestrians_positions"], d["obs_abs_ohe_dict__pedestrians_positions"][0], atol=1e-6)
    np.testing.assert_array_equal(obs["pedestrians_statuses"], d["obs_abs_ohe_dict__pedestrians_statuses"][0])
    obs, reward, terminated, truncated, info = env.step(d["action"][0], noise=d["noise"][0])
    assert isinstance(reward, float) and isinstance(terminated, bool) and isinstance(truncated, bool) and info == {}
    np.testing.assert_allclose(reward, d["reward"][0], rtol=1e-5)
    u = env.unwrapped
    np.testing.assert_allclose(u.pedestrians.positions, d["pos"][1], atol=ATOL)
    assert [s.value for s in u.pedestrians.statuses] == d["status"][1].tolist()
    assert u.area.exit.position.tolist() == [0.0, -1.0] and u.area.step_size == p.step_size and u.time.now == 1
    # what the reference's scripted agent reads off the env (baseline_wacuum_cleaner.py:14-28): exit position, step size, room half-widths
    assert env.area is u.area and env.area.width == p.width and env.area.height == p.height
    assert env.area.exit.position.dtype == np.float32 and env.area.exit.position.shape == (2,) and env.area.eps == p.eps
    # (the scripted agent's sweep tests -- baseline_wacuum_cleaner.py:17-29 -- compare the leader's coordinates with the room's half-widths
    # less half the leader radius plus a step; with the attributes above they can be evaluated: the leader starts in the middle of the room)
    reach = 0.2 / 2 - float(env.area.step_size)                                  # constants.py:35 (leader radius 0.2)
    ax, ay = (float(v) for v in obs["agent_position"])
    assert -float(env.area.width) + reach < ax < float(env.area.width) - reach and -float(env.area.height) + reach < ay < float(env.area.height) - reach
    with pytest.raises(TypeError):
        env.step([1, 0])                       # integer action: the reference raises too (area.py:190)
    agent = ea.RandomAgent(env.action_space)
    for _ in range(3):
        obs, reward, terminated, truncated, _ = env.step(agent.act(obs))
    env.close()
    with pytest.raises(NotImplementedError):
        ea.setup_env(cfg_from_params(ea, p), ea.EnvWrappersConfig(positions="grav", type="Box"))


def test_philox_rollouts_are_statistically_equivalent_to_the_reference_rng(ea):
    """trajectories diverge chaotically, so Philox-mode rollouts are compared with
    oracle episodes driven by NumPy's RNG (the reference's own noise / reset / RandomAgent distributions)
    through distributions: status counts and mean reward after 150 and 400 steps."""
    import torch
    n, E_gpu, E_cpu = 60, 2048, 48
    p = O.OracleParams(number_of_pedestrians=n, is_new_exiting_reward=True, max_timesteps=100000)
    env = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), ea.EnvWrappersConfig(positions="grav"), num_envs=E_gpu, seed=1234)
    env.reset()
    rng = np.random.default_rng(7)
    cpu = [O.env_reset(p, rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2))) for _ in range(E_cpu)]
    cpu_rew = np.zeros(E_cpu)
    t_prev = 0
    for t_check in (150, 400):
        ro = env.rollout(t_check - t_prev)
        gpu_rew = ro["reward"].mean().item()
        for e, st in enumerate(cpu):
            acc = 0.0
            for _ in range(t_check - t_prev):
                acc += O.env_step(p, st, rng.uniform(-1, 1, 2).astype(np.float32), O.draw_step_noise(p, st, rng))["reward"]
            cpu_rew[e] = acc / (t_check - t_prev)
        t_prev = t_check
        s = env.get_state()["status"]
        gpu_counts = torch.stack([(s == k).sum(dim=1).float() for k in (1, 2, 3, 4)], dim=1).cpu().numpy()   # [E,4]
        cpu_counts = np.array([[np.sum(st.status == k) for k in (1, 2, 3, 4)] for st in cpu], dtype=np.float64)
        for k, name in enumerate(("viscek", "follower", "exiting", "escaped")):
            g, c = gpu_counts[:, k], cpu_counts[:, k]
            se = np.sqrt(g.var() / len(g) + c.var() / len(c)) + 1e-9
            z = (g.mean() - c.mean()) / se
            assert abs(z) < 4.5, (t_check, name, g.mean(), c.mean(), z)
        se = cpu_rew.std() / np.sqrt(E_cpu) + 1e-9
        assert abs(gpu_rew - cpu_rew.mean()) < 5 * se + 0.02, (t_check, gpu_rew, cpu_rew.mean(), se)
    env.close()


@pytest.mark.parametrize("kw", [
    dict(noise_coef=2.5, step_size=0.03, enslaving_degree=0.3),                 # ocml sincosf regime
    dict(noise_coef=1.2, width=1.5, height=0.7, eps=1e-3),                      # long Taylor regime, non-unit room
    dict(noise_coef=0.05, step_size=0.1, intrinsic_reward_coef=2.0, init_reward_each_step=0.0,
         is_new_followers_reward=False, is_new_exiting_reward=True),
], ids=["big_noise", "mid_noise_room", "coarse_step"])
def test_unusual_parameters_take_the_rare_code_paths(ea, kw):
    """Teacher-forced parity on oracle-generated states for parameter values that select the kernel's
    rarely used branches (sincos regimes 0/1, powf for non-integer alpha, walls != 1, large eps)."""
    n, E = 47, 10
    rng = np.random.default_rng(int(1000 * kw["noise_coef"]) + 17)          # fixed per case (str hashes are salted)
    p = O.OracleParams(number_of_pedestrians=n, **kw)
    pre, acts, nzs = [], [], []
    for e in range(E):
        st = O.env_reset(p, rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2)))
        for _ in range(2 + 4 * e):
            O.env_step(p, st, rng.uniform(-1, 1, 2).astype(np.float32), rng.uniform(-p.noise_coef / 2, p.noise_coef / 2, n))
        pre.append(st)
        acts.append(rng.uniform(-1, 1, 2).astype(np.float32))
        nzs.append(rng.uniform(-p.noise_coef / 2, p.noise_coef / 2, n).astype(np.float32))
    for w in (dict(positions="grav", alpha=2.5), dict(positions="grav", alpha=7), dict(positions="rel", statuses="cat")):
        wrap = ea.EnvWrappersConfig(**w)
        got = gpu_step_batch(ea, p, wrap, pre, acts, nzs)
        compare_step(p, wrap, pre, acts, nzs, got, min_checked=E - 3)


def test_step_is_hipgraph_capturable(ea):
    """evac_step only enqueues work on the caller's stream (no sync, no allocation), so a trainer can
    capture `policy -> env.step` into a hipGraph; replays must equal eager steps bit for bit."""
    import torch
    n, E, seed = 60, 64, 11
    cfg = ea.EnvConfig(number_of_pedestrians=n, max_timesteps=9)
    wrap = ea.EnvWrappersConfig(positions="grav", alpha=3)
    a = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=seed)
    b = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=seed)
    a.reset(); b.reset()
    act = torch.zeros((E, 2), dtype=torch.float32, device=a.device)
    acts = torch.rand((20, E, 2), device=a.device) * 2 - 1
    act.copy_(acts[0])
    a.step(act)                                  # warm-up outside capture
    b.step(acts[0].contiguous())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        act.copy_(acts[1])
        with torch.cuda.graph(g, stream=s):
            a.step(act)
    torch.cuda.current_stream().wait_stream(s)
    b_out = []
    for t in range(1, 20):
        act.copy_(acts[t])
        g.replay()
        o, r, te, tr, _ = b.step(acts[t].contiguous())
        torch.cuda.synchronize()
        assert (a.obs == o).all() and (a.reward == r).all() and (a.terminated == te).all() and (a.truncated == tr).all(), t
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert (sa[k] == sb[k]).all(), k


def test_trajectory_capture_matches_stepwise_state(ea):
    """the rollout's capture buffer holds what Pedestrians.save / Agent.save would
    have stored after every step -- checked against get_state() of a twin env stepped one step at a time."""
    import torch
    n, E, T, K, seed = 60, 6, 12, 3, 77
    cfg = ea.EnvConfig(number_of_pedestrians=n, max_timesteps=1000)
    wrap = ea.EnvWrappersConfig(positions="grav")
    a = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=seed)
    b = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=seed)
    a.reset(); b.reset()
    ro = a.rollout(T, record_actions=True, capture_envs=K)
    assert ro["positions"].shape == (T, K, n, 2) and ro["statuses"].shape == (T, K, n) and ro["agent_positions"].shape == (T, K, 2)
    for t in range(T):
        b.step(ro["actions"][t].contiguous())
        st = b.get_state()
        assert (ro["positions"][t] == st["pos"][:K]).all(), t
        assert (ro["statuses"][t] == st["status"][:K].float()).all(), t
        assert (ro["agent_positions"][t] == st["agent_pos"][:K]).all(), t


def test_c_abi_error_codes(ea):
    """include/evac.h conventions: negative status + message, never a crash or a silent no-op."""
    import ctypes as C
    import torch
    from evacuation_amd import _lib
    from evacuation_amd.config import to_c_config
    lib = _lib.load()
    c = to_c_config(ea.EnvConfig(number_of_pedestrians=60), ea.EnvWrappersConfig(positions="grav"))
    h = C.c_void_p()
    assert lib.evac_create(C.byref(c), 0, 0, 0, 0, C.byref(h)) == _lib.ERR_INVALID_ARGUMENT          # num_envs < 1
    assert lib.evac_create(C.byref(c), 4, 99, 0, 0, C.byref(h)) == _lib.ERR_INVALID_ARGUMENT         # no such device
    assert lib.evac_create(C.byref(c), 4, 0, 0, 2**32 - 2, C.byref(h)) == _lib.ERR_INVALID_ARGUMENT  # env ids overflow
    assert lib.evac_create(C.byref(c), 4, 0, 7, 0, C.byref(h)) == 0 and h.value
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    u8 = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, q = C.c_void_p(buf.data_ptr()), C.c_void_p(u8.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.evac_step(h, p, None, p, p, q, q, 0, None, None, s) == _lib.ERR_NOT_BOUND
    assert b"evac_bind_state" in lib.evac_last_error(h)
    assert lib.evac_reset(h, None, None, None, s) == _lib.ERR_NOT_BOUND
    assert lib.evac_rollout(h, 1, None, None, p, None, 0, None, None, s) == _lib.ERR_NOT_BOUND
    assert lib.evac_bind_state(h, p, q, None, p, p) == _lib.ERR_INVALID_ARGUMENT                      # NULL buffer
    assert lib.evac_bind_state(h, C.c_void_p(buf.data_ptr() + 4), q, p, p, p) == _lib.ERR_INVALID_ARGUMENT   # alignment
    env = ea.BatchedEvacuationEnv(ea.EnvConfig(number_of_pedestrians=60), ea.EnvWrappersConfig(positions="grav"), num_envs=4)
    env.reset()
    hh = env._h
    assert lib.evac_step(hh, None, None, p, p, q, q, 0, None, None, s) == _lib.ERR_INVALID_ARGUMENT  # actions NULL
    assert lib.evac_rollout(hh, 0, None, None, p, None, 0, None, None, s) == _lib.ERR_INVALID_ARGUMENT      # n_steps < 1
    assert lib.evac_rollout(hh, 1, None, None, None, None, 0, None, None, s) == _lib.ERR_INVALID_ARGUMENT   # slab NULL
    assert lib.evac_rollout(hh, 1, None, None, p, None, 9, p, None, s) == _lib.ERR_INVALID_ARGUMENT         # capture_envs > E
    with pytest.raises(ValueError):
        env.step(torch.zeros((3, 2), device="cuda"))                                                  # wrong batch size
    with pytest.raises(_lib.EvacError):
        _lib.check(lib.evac_observe(hh, None, s), hh)
    assert lib.evac_status_string(-2) == b"state buffers not bound"
    torch.cuda.synchronize()
    lib.evac_destroy(h)
    env.close()


@pytest.mark.parametrize("n,E,T,wrap_kw", [
    (256, 1024, 120, dict(positions="grav", alpha=3)),                          # BASELINE config 3
    (1024, 32, 60, dict(positions="rel", statuses="ohe", type="Box")),          # one GPU's shard of config 5
], ids=["c3_n256x1024_grav", "c5_n1024x32_box_ohe"])
def test_full_size_invariants_large_envs(ea, n, E, T, wrap_kw):
    """Size-independent properties at the BASELINE shapes that use the multi-wave kernels."""
    import torch
    cfg = ea.EnvConfig(number_of_pedestrians=n, is_new_exiting_reward=True, max_timesteps=50)
    wrap = ea.EnvWrappersConfig(**wrap_kw)
    env = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=0x5EED0003)
    env.reset()
    ro = env.rollout(T)
    torch.cuda.synchronize()
    st = env.get_state()
    pos, dr, status = st["pos"], st["dir"], st["status"]
    assert torch.isfinite(ro["slab"]).all() and torch.isfinite(pos).all()
    assert (pos.abs() <= 1.0).all() and set(torch.unique(status).tolist()) <= {1, 2, 3, 4}
    exit_xy = torch.tensor([0.0, -1.0], device=pos.device)
    d_lead = (pos - st["agent_pos"][:, None, :]).norm(dim=-1)
    d_exit = (pos - exit_xy).norm(dim=-1)
    want = torch.ones_like(status)
    want[d_lead < 0.2] = 2
    want[d_exit < 0.4] = 3
    want[d_exit < 0.01] = 4
    near_tie = ((d_lead - 0.2).abs() < 1e-6) | ((d_exit - 0.4).abs() < 1e-6) | ((d_exit - 0.01).abs() < 1e-6)
    assert ((want == status) | near_tie).all()
    v = status == 1
    np.testing.assert_allclose(dr[v].norm(dim=-1).cpu().numpy(), cfg.step_size, rtol=1e-5)
    tr = ro["truncated"] != 0
    n_trunc = T // 50                                                             # truncation every 50 steps, autoreset in between
    assert all(tr[50 * k - 1].all() for k in range(1, n_trunc + 1)) and int(tr.sum()) == n_trunc * E
    stats = ro["episode_stats"][49]
    assert (stats[:, 1] == 50).all() and (stats[:, 4:8].sum(dim=1) == n).all()
    np.testing.assert_allclose(stats[:, 0].cpu().numpy(), ro["reward"][:50].sum(dim=0).cpu().numpy(), rtol=1e-4)
    obs = env.split_observation(ro["obs"][-1])                                   # last step's observation
    if wrap.type == "Box":
        assert obs.shape == (E, n + 2, 6)
        np.testing.assert_array_equal(obs[:, 0, 2:].cpu().numpy(), 0)            # agent row: status 0000
        np.testing.assert_array_equal(obs[:, 1, 2:].cpu().numpy(), np.tile([1, 0, 0, 0], (E, 1)))   # exit row
        assert (obs[:, 2:, 2:].sum(dim=-1) == 1).all()                           # one-hot rows
        code = obs[:, 2:, 2:].argmax(dim=-1)                                     # wrappers.py:49: 4 - Status.value
        assert ((4 - code) == status.long()).all()
        rel = (pos - st["agent_pos"][:, None, :]) * 0.70710678
        np.testing.assert_allclose(obs[:, 2:, 0:2].cpu().numpy(), rel.cpu().numpy(), atol=1e-6)
    else:
        np.testing.assert_array_equal(obs["agent_position"].cpu().numpy(), st["agent_pos"].cpu().numpy())
    env.close()


@pytest.mark.parametrize("n", [10, 20, 60, 100])
def test_masked_reset_touches_only_selected_envs(ea, n):
    import torch
    E, seed = 8, 5
    env = ea.BatchedEvacuationEnv(ea.EnvConfig(number_of_pedestrians=n), ea.EnvWrappersConfig(positions="grav"), num_envs=E,
                                  seed=seed, autoreset=False)
    env.reset()
    act = torch.rand((E, 2), device=env.device) * 2 - 1
    for _ in range(5):
        env.step(act)
    before = {k: v.clone() for k, v in env.get_state().items()}
    obs_before = env.obs.clone()
    mask = torch.tensor([0, 1, 0, 0, 1, 0, 0, 1], dtype=torch.uint8, device=env.device)
    obs, _ = env.reset(mask=mask)
    after = env.get_state()
    m = mask.bool()
    for k in before:
        assert (after[k][~m] == before[k][~m]).all(), k                          # untouched envs
    assert (after["now"][m] == 0).all() and (after["agent_pos"][m] == 0).all()
    np.testing.assert_array_equal(after["pos"][m].cpu().numpy(), P.reset_draws(seed, np.nonzero(m.cpu().numpy())[0], n, 1)[..., 0:2])
    assert (obs[~m] == obs_before[~m]).all()                                      # only rows of reset envs are rewritten
    assert (env.clock[:, 1].cpu() == torch.tensor([1, 2, 1, 1, 2, 1, 1, 2])).all()
    env.close()


def test_wrap_env_selects_the_observation_epilogue(ea):
    """EnvWrappersConfig.wrap_env(env) (wrappers/config.py:46-93) on the single-env facade."""
    cfg = ea.EnvConfig(number_of_pedestrians=12)
    env = ea.EvacuationEnv(cfg)
    o, _ = env.reset()
    assert set(o) == {"agent_position", "exit_position", "pedestrians_positions"}
    assert ea.EnvWrappersConfig().wrap_env(env) is env                            # abs / no / Dict: no wrapper
    g = ea.EnvWrappersConfig(positions="grav", alpha=2).wrap_env(env)
    o, _ = g.reset()
    assert set(o) == {"agent_position", "grad_potential_exit", "grad_potential_pedestrians"}
    assert list(g.observation_space.keys()) == sorted(g.observation_space.keys())
    b = ea.EnvWrappersConfig(positions="rel", statuses="cat", type="Box").wrap_env(g)
    o, _ = b.reset()
    assert o.shape == (14, 3) and b.observation_space.shape == (14, 3) and b.unwrapped is b
    with pytest.raises(NotImplementedError):
        ea.EnvWrappersConfig(positions="grav", type="Box").wrap_env(b)
    b.close()


def test_long_rollouts_cross_the_64_step_action_blocks(ea):
    """Actions are staged 64 steps at a time, one per lane: check T > 64 for given and for Philox actions."""
    import torch
    n, E, T, seed = 33, 5, 150, 0xABCDEF
    cfg = ea.EnvConfig(number_of_pedestrians=n, max_timesteps=70)
    wrap = ea.EnvWrappersConfig(positions="grav", alpha=3)
    a = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=seed)
    b = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=seed)
    c = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=seed)
    for e in (a, b, c):
        e.reset()
    ro = a.rollout(T, record_actions=True)                                        # Philox actions
    acts = ro["actions"]
    for t in (0, 63, 64, 65, 127, 128, 149):
        np.testing.assert_array_equal(acts[t].cpu().numpy(), P.random_action(seed, np.arange(E), t))
    rb = b.rollout(T, actions=acts)                                               # the same actions, provided
    assert (rb["slab"] == ro["slab"]).all()
    for t in range(T):                                                            # and one step at a time
        o, r, te, tr, _ = c.step(acts[t].contiguous())
        assert (o == ro["obs"][t]).all() and (r == ro["reward"][t]).all(), t
        assert (te == ro["terminated"][t]).all() and (tr == ro["truncated"][t]).all(), t
    assert int((ro["truncated"] != 0).sum()) == 2 * E
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("n", [3, 10, 16, 17, 31, 32])
@pytest.mark.parametrize("wrap_kw", [dict(positions="grav", alpha=3), dict(positions="rel", statuses="ohe", type="Box")],
                         ids=["grav", "box"])
def test_subwave_kernels_match_one_wave_per_env(ea, n, wrap_kw):
    """N <= 32 runs 2 (N <= 16: 4) envs per wave (csrc/evac_subwave.h).  Same arithmetic as the one-wave-per-env
    kernels; only the reduction trees differ, so the dynamics (positions, directions, statuses, flags) must be
    bit-identical and the summed quantities (reward with intrinsic term, gravity sums) equal to f32 rounding."""
    import torch
    E, T, seed = 11, 90, 2024                       # E not a multiple of the envs per wave / block
    cfg = ea.EnvConfig(number_of_pedestrians=n, max_timesteps=40, is_new_exiting_reward=True, intrinsic_reward_coef=0.5)
    wrap = ea.EnvWrappersConfig(**wrap_kw)
    a = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=seed, options=ea.KernelOptions(subwave=1))
    b = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=seed, options=ea.KernelOptions(subwave=0))
    oa, _ = a.reset(); ob, _ = b.reset()
    torch.testing.assert_close(oa, ob, rtol=2e-6, atol=1e-6)
    ra = a.rollout(T, record_actions=True, capture_envs=E)
    rb = b.rollout(T, record_actions=True, capture_envs=E)
    assert (ra["actions"] == rb["actions"]).all()
    assert (ra["trajectory"] == rb["trajectory"]).all()                      # positions + statuses, every step
    assert (ra["terminated"] == rb["terminated"]).all() and (ra["truncated"] == rb["truncated"]).all()
    torch.testing.assert_close(ra["reward"], rb["reward"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(ra["obs"], rb["obs"], rtol=2e-5, atol=1e-4 if wrap.positions == "grav" else 1e-6)
    torch.testing.assert_close(ra["episode_stats"], rb["episode_stats"], rtol=1e-5, atol=1e-4)
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    act = ra["actions"][0].contiguous()                                       # and the per-step kernel
    o1, r1, t1, u1, i1 = a.step(act)
    o2, r2, t2, u2, i2 = b.step(act)
    assert (t1 == t2).all() and (u1 == u2).all()
    torch.testing.assert_close(r1, r2, rtol=1e-5, atol=1e-5)
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert (sa[k] == sb[k]).all(), k
    a.close(); b.close()


def test_sharded_env_single_process_path(ea):
    """ShardedEvacuationEnv without a process group = one shard holding every env; the gathered slab is the
    packed [obs | reward | terminated | truncated] record in global env order."""
    import torch
    from evacuation_amd.distributed import ShardedEvacuationEnv, unpack_outputs
    cfg = ea.EnvConfig(number_of_pedestrians=40, max_timesteps=6)
    sh = ShardedEvacuationEnv(cfg, ea.EnvWrappersConfig(positions="grav"), total_envs=12, device="cuda:0", seed=3)
    ref = ea.BatchedEvacuationEnv(cfg, ea.EnvWrappersConfig(positions="grav"), num_envs=12, seed=3)
    assert (sh.rank, sh.world_size, sh.offset, sh.local_envs) == (0, 1, 0, 12)
    sh.reset(); ref.reset()
    act = torch.rand((12, 2), device="cuda") * 2 - 1
    obs, rew, te, tr, info, slab = sh.step(act)
    o2, r2, t2, u2, _ = ref.step(act)
    o, r, t, u = unpack_outputs(slab)
    assert (o == o2).all() and (r == r2).all() and (t == t2.bool()).all() and (u == u2.bool()).all()
    ro, pending = sh.rollout_gathered(10)
    full = sh.wait(pending)
    rr = ref.rollout(10)
    assert full.shape == (10, 12, 9) and (full == rr["slab"]).all() and (ro["slab"] == rr["slab"]).all()
    sh.close(); ref.close()


@pytest.mark.parametrize("case", range(16))
def test_randomized_configurations(ea, case):
    """Random (N, room, step, noise, enslaving, eps, rewards, alpha, observation mode): oracle-generated states,
    one teacher-forced step, reference-precision comparison.  Covers the sub-wave (N <= 32), one-wave and
    multi-wave kernels with parameter combinations no hand-written case uses."""
    rng = np.random.default_rng(9000 + case)
    n = int(rng.choice([rng.integers(1, 17), rng.integers(17, 33), rng.integers(33, 65), rng.integers(65, 200)]))
    kw = dict(number_of_pedestrians=n,
              width=float(rng.uniform(0.8, 1.6)), height=float(rng.uniform(0.8, 1.6)),
              step_size=float(rng.choice([0.005, 0.01, 0.03, 0.08])), noise_coef=float(rng.choice([0.0, 0.1, 0.2, 0.7, 1.9])),
              enslaving_degree=float(rng.choice([1.0, 0.6, 0.05])), eps=float(rng.choice([1e-8, 1e-4])),
              is_new_exiting_reward=bool(rng.integers(2)), is_new_followers_reward=bool(rng.integers(2)),
              intrinsic_reward_coef=float(rng.choice([0.0, 1.0, 3.0])), init_reward_each_step=float(rng.choice([-1.0, 0.0, 0.5])),
              is_termination_agent_wall_collision=bool(rng.integers(2)), max_timesteps=int(rng.choice([7, 2000])))
    p = O.OracleParams(**kw)
    wrap_kw = [dict(positions="grav", alpha=float(rng.choice([1, 2, 3, 4.5]))),
               dict(positions=str(rng.choice(["abs", "rel"])), statuses=str(rng.choice(["no", "ohe", "cat"])),
                    type=str(rng.choice(["Dict", "Box"])))][case % 2]
    wrap = ea.EnvWrappersConfig(**wrap_kw)
    E = 5
    pre, acts, nzs = [], [], []
    for e in range(E):
        st = O.env_reset(p, rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2)))
        for _ in range(int(rng.integers(0, 7))):
            with np.errstate(all="ignore"):
                O.env_step(p, st, rng.uniform(-1, 1, 2).astype(np.float32), rng.uniform(-p.noise_coef / 2, p.noise_coef / 2, n))
        if not np.isfinite(st.pos).all():
            continue
        pre.append(st)
        acts.append(rng.uniform(-1, 1, 2).astype(np.float32))
        nzs.append(rng.uniform(-p.noise_coef / 2, p.noise_coef / 2, n).astype(np.float32))
    got = gpu_step_batch(ea, p, wrap, pre, acts, nzs)
    compare_step(p, wrap, pre, acts, nzs, got, min_checked=max(1, len(pre) - 2))
