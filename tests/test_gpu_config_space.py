"""Every kernel family against the oracle off the default environment settings: rooms W != H, the three sin/cos regimes of the
noise, eps and step sizes of other orders, enslaving degrees 0 / 0.05, wall termination, other rewards.

a. Which kernel a handle runs: the default-configuration instantiations (evac_create's default_cfg, which then fixes several fields
   at compile time: default_config_constants) exactly when the rule restated here admits the configuration.
b. Every rollout face, teacher-forced for one step (test_gpu_rollout_teacher_forced.teacher_force_batch) on the recorded
   off-default trajectories of its room and on oracle-generated states of four regimes -- random resets and a wall set -- with
   every observation variant spread over them.
c. Every step family the same way, through step() with the device's own Philox noise.
d. rollout(T) == T x step(), bit for bit, in a wall-terminating non-unit room and in sin/cos regime 0.
e. The fused normalised step (evac_step_normalized) at N = 256 / 512 / 1024 against oracle/gym_wrappers.py, the reference's NaN
   poisoning included at N = 1024.
"""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import evac_oracle as O
from oracle import gym_wrappers as G
from tests import test_gpu_rollout_teacher_forced as TF
from tests.test_gpu_parity import WRAPS, ea  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

DEFAULT_WRAPS = (dict(positions="grav", alpha=3), dict(positions="rel", statuses="ohe", type="Box"))
VARIANTS = list(WRAPS) + [dict(positions="grav", alpha=a) for a in (1, 4.5, 7)]      # (grav alpha = 2.5 is one of WRAPS)


def _key(w):
    return tuple(sorted(w.items()))


def default_config_eligible(cfg, wrap, specialize=-1):
    """evac_create's rule (default_cfg), restated: the gravity observation with alpha + 2 == 5 in f32 or the relative / one-hot / Box
    one, |noise| / 2 <= 0.2 in f32 (sin/cos regime 2), an enslaving degree of exactly 1 in f32, no wall termination, no NaN guard.
    `cfg`: an EnvConfig or OracleParams; `wrap`: an EnvWrappersConfig or its keyword dict."""
    f = np.float32
    w = dict(dataclasses.asdict(wrap) if dataclasses.is_dataclass(wrap) else wrap)
    pos, stat, typ, alpha = w.get("positions", "abs"), w.get("statuses", "no"), w.get("type", "Dict"), w.get("alpha", 3)
    if specialize == 0:
        return False
    obs = f(alpha) + f(2.0) == f(5.0) if pos == "grav" else (pos, stat, typ) == ("rel", "ohe", "Box")
    return bool(obs and abs(f(cfg.noise_coef)) * f(0.5) <= f(0.2) and f(cfg.enslaving_degree) == f(1.0)
                and not cfg.is_termination_agent_wall_collision and not getattr(cfg, "nan_guard", False))


# one room of every family: (family, N, KernelOptions fields)
FAMILIES = [("sub16", 10, {}), ("sub32", 32, {}), ("wave1", 60, dict(cu_wide=0)), ("wave1_cu_wide", 60, dict(cu_wide=1)),
            ("wave2", 100, {}), ("wave4", 256, dict(cu_wide=0)), ("wave4_cu_wide", 256, dict(cu_wide=1)), ("wave8", 512, {}),
            ("wave16", 1024, dict(cells=0, team=0)), ("cells2", 100, dict(cells=1)), ("cells4", 256, dict(cells=1)),
            ("cells8", 512, dict(cells=1)), ("cells16", 1024, dict(team=0)), ("team2", 1024, dict(team=2)), ("team16", 1024, dict(team=16))]
CONFIGS = ([("default", {}, {})]
           + [(f"rule:{k}={v}", {k: v}, {}) for k, v in (("is_termination_agent_wall_collision", True), ("nan_guard", True),
                                                          ("noise_coef", 0.41), ("noise_coef", 0.6), ("noise_coef", 2.0), ("enslaving_degree", 0.999))]
           + [("rule:noise_coef=0.4", {"noise_coef": 0.4}, {})]
           + [(f"rule:{w}", {}, w) for w in [dict(positions="grav", alpha=2), dict(positions="grav", alpha=3.0001)]
              + [w for w in VARIANTS if w.get("positions") != "grav" and _key(w) != _key(DEFAULT_WRAPS[1])]]
           + [(f"run-time:{k}={v}", {k: v}, {}) for k, v in (("width", 1.6), ("height", 0.6), ("eps", 1e-3), ("step_size", 0.07),
                                                              ("init_reward_each_step", 0.5), ("intrinsic_reward_coef", 3.0),
                                                              ("is_new_exiting_reward", True), ("is_new_followers_reward", False),
                                                              ("clip_action", True), ("max_timesteps", 17))]
           + [("specialize=0", {}, {})])
SELECTION = []      # (family, configuration, eligible, step kernel, rollout kernel): the table of part a, printed with -s


@pytest.mark.parametrize("family,n,opts", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_default_config_kernels_are_chosen_by_the_rule(ea, family, n, opts):
    seen = set()
    for label, cfg_kw, wrap_kw in CONFIGS:
        for base in (DEFAULT_WRAPS if not wrap_kw else (wrap_kw,)):
            cfg = ea.EnvConfig(number_of_pedestrians=n, **cfg_kw)
            wrap = ea.EnvWrappersConfig(**base)
            spec = 0 if label == "specialize=0" else -1
            want = default_config_eligible(cfg, wrap, spec)
            assert want == (label in ("default",) or label.startswith("run-time:") or label == "rule:noise_coef=0.4"), (label, base)
            env = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=8, seed=1, options=ea.KernelOptions().replace(specialize=spec, **opts))
            step, roll = env.kernel_variant("step"), env.kernel_variant("rollout")
            env.close()
            SELECTION.append((family, f"{label} {base}", want, step, roll))
            assert ("_default_config<" in step) == want, (family, label, base, step)
            assert ("_default_config<" in roll) == want, (family, label, base, roll)
            assert (", grav obs>" in step) == (base.get("positions") == "grav"), step
            seen.add(want)
    assert seen == {True, False}
    print("\n".join(f"{f:14s} {'default ' if w else 'generic '} {c:70s} {r}" for f, c, w, s, r in SELECTION if f == family))


# ---- regimes off the default room ------------------------------------------------------------------------------------------------
REGIMES = {
    # H < 1 < W, sin/cos regime 0, eps 1e-3, wall termination, init reward 0.5
    "room16x06_noise25_wallterm": dict(width=1.6, height=0.6, noise_coef=2.5, eps=1e-3, is_termination_agent_wall_collision=True,
                                       init_reward_each_step=0.5, step_size=0.05, is_new_exiting_reward=True),
    # W < 1 < H, regime 1, enslaving degree 0, intrinsic reward 3, no followers' reward
    "room07x13_noise1_ens0": dict(width=0.7, height=1.3, noise_coef=1.0, eps=1e-3, enslaving_degree=0.0, step_size=0.03,
                                  intrinsic_reward_coef=3.0, is_new_followers_reward=False),
    # both > 1, regime 0, enslaving degree 0.05, step 0.08
    "room25_noise25_ens005": dict(width=2.5, height=2.5, noise_coef=2.5, eps=1e-4, enslaving_degree=0.05, step_size=0.08,
                                  init_reward_each_step=0.5, intrinsic_reward_coef=3.0, is_new_exiting_reward=True, is_new_followers_reward=False),
    # eligible for the default-configuration kernels, with a room, an eps and a step size they keep as run-time values
    "eligible_room16x06_eps1e4_step07": dict(width=1.6, height=0.6, eps=1e-4, step_size=0.07, init_reward_each_step=0.5,
                                             intrinsic_reward_coef=3.0, is_new_exiting_reward=True),
}


DYNAMICS = ("width", "height", "step_size", "noise_coef", "eps", "enslaving_degree", "is_termination_agent_wall_collision")


def off_default(p):
    """A recorded trajectory whose dynamics are not the default environment's: any of DYNAMICS differs from EnvConfig's default
    (the rewards, the room size N and max_timesteps aside)."""
    d = O.OracleParams()
    return any(getattr(p, k) != getattr(d, k) for k in DYNAMICS)


def mean_heading_conditioning(st):
    """The smallest |sum of unit headings| over the neighbourhood of a moving pedestrian (area.py:118-120).  Near 0 -- two neighbours
    almost exactly antiparallel -- the angle of the mean heading is ill-conditioned: f32 rounding alone moves the new direction by
    more than the 1e-5 bar (a generated N = 513 state with |sum| = 1.2e-4 moved one pedestrian by 8e-6 in the f32 oracle, by 2e-4 in
    the kernels' integer heading sums), which compare_step's threshold-tie model does not cover.  Generated states avoid it, as the
    crafted cases avoid their thresholds (make_golden.make_crafted)."""
    efv = np.isin(st.status, (O.EXITING, O.FOLLOWER, O.VISCEK))
    fv = np.isin(st.status, (O.FOLLOWER, O.VISCEK))
    with np.errstate(all="ignore"):
        u = st.dir / np.linalg.norm(st.dir, axis=1)[:, None]
    pos = st.pos[efv]
    worst = np.inf
    for i in np.nonzero(fv)[0]:
        m = np.linalg.norm(pos - st.pos[i], axis=1) < O.R_PEDESTRIAN
        worst = min(worst, float(np.hypot(*u[efv][m].sum(axis=0))))
    return worst


def regime_states(name, n):
    """(params, pre-states, actions) of one regime in room n: three random resets followed by 0 / 3 / 6 oracle steps, and a wall set --
    the leader within one step of +W, -W, +H, -H and of a corner, moving into it, with four pedestrians a third of a step inside the
    four corners heading out of them."""
    p = O.OracleParams(number_of_pedestrians=n, **REGIMES[name])
    rng = np.random.default_rng(1000 * list(REGIMES).index(name) + n)
    c, s, W, Hh = p.noise_coef, p.step_size, p.width, p.height
    pre, acts = [], []
    for e in range(3):
        while True:
            st = O.env_reset(p, rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2)))
            for _ in range(3 * e):
                with np.errstate(all="ignore"):
                    O.env_step(p, st, rng.uniform(-1, 1, 2).astype(np.float32), rng.uniform(-c / 2, c / 2, n))
            if mean_heading_conditioning(st) > 1e-3:
                break
        pre.append(st)
        acts.append(rng.uniform(-1, 1, 2).astype(np.float32))
    spots = [((W - s / 2, 0.1), (1.0, 0.2)), ((-W + s / 2, -0.2), (-1.0, 0.1)), ((0.15, Hh - s / 2), (0.1, 1.0)),
             ((-0.1, -Hh + s / 2), (-0.2, -1.0)), ((W - s / 2, Hh - s / 2), (1.0, 1.0))]
    for (ax, ay), a in spots:
        while True:
            st = O.env_reset(p, rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2)))
            for i, (sx, sy) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))[:n]):
                st.pos[i] = (sx * (W - s / 3), sy * (Hh - s / 3))
                st.dir[i] = np.array([sx, sy]) / np.sqrt(2.0) * np.linalg.norm(st.dir[i])
            st.agent_pos = np.array([ax, ay], np.float32)
            st.agent_dir = (np.array(a) / np.linalg.norm(a) * s).astype(np.float32)
            st.status = O.classify_statuses(st.pos, st.agent_pos, O.EXIT_POSITION, st.pos.dtype)
            st.now = 40
            if mean_heading_conditioning(st) > 1e-3:
                break
        pre.append(st)
        acts.append(np.array(a, np.float32))
    return p, pre, acts


@functools.lru_cache(maxsize=None)
def regime_batches(n):
    """The batches of room n off the default room: its recorded off-default trajectories, then every regime's generated states."""
    raw = TF.fixture_states(n, off_default)
    for name in REGIMES:
        p, pre, acts = regime_states(name, n)
        raw.append((f"{name}_n{n}", p, pre, acts))
    return [TF.pad_batch(n, label, p, pre, acts) for label, p, pre, acts in raw]


def _spread(n):
    """The observation variants of each batch of room n: VARIANTS dealt round the batches, so that every variant meets the face
    once; a batch the default-configuration kernels may take also runs their two observations."""
    bs = regime_batches(n)
    out = []
    for j, b in enumerate(bs):
        ws = [w for k, w in enumerate(VARIANTS) if k % len(bs) == j]
        if default_config_eligible(b[1], DEFAULT_WRAPS[0]):
            ws += [w for w in DEFAULT_WRAPS if _key(w) not in {_key(x) for x in ws}]
        out.append(ws)
    return out


def _group(label, n):
    """A batch's name in the summary: the regime, or the fixture without its room prefix."""
    return label.replace(f"traj_n{n}_", "").replace(f"_n{n}", "")


def run_regimes(ea, face, n, opts, want, absent, mode="rollout"):
    """Every batch of regime_batches(n) through teacher_force_batch with its share of the variants; asserts that the face met every
    (observation variant) of VARIANTS and both the default-configuration and the generic kernels.  Returns the counts per (kernel
    variant, regime or fixture)."""
    log, ran = {}, set()
    for i, (batch, ws) in enumerate(zip(regime_batches(n), _spread(n))):
        TF.teacher_force_batch(ea, batch, functools.partial(TF.expected, regime_batches, n, i), ws, opts, want, absent, log, mode=mode,
                               group=_group(batch[0], n))
        ran |= {_key(w) for w in ws}
    assert ran >= {_key(w) for w in VARIANTS}, (face, sorted({_key(w) for w in VARIANTS} - ran))
    assert any("_default_config<" in k for k, _ in log) and any("_default_config<" not in k for k, _ in log), list(log)
    return log


FACES_B = TF.CASES          # every rollout face in every room of the FACES table (partial waves, partial teams)


@pytest.mark.parametrize("face,n", FACES_B, ids=[f"{f}-n{n}" for f, n in FACES_B])
def test_rollout_faces_teacher_forced_in_regimes(ea, face, n):
    """Every (face, observation variant) pair runs: each face asserts that it met all of VARIANTS (run_regimes)."""
    _, _, opts, want, absent = TF.FACE[face]
    log = run_regimes(ea, face, n, opts, want, absent)
    TF.assert_floors(face, n, log, "one step in the off-default regimes")


# ---- c. step families, the device's own noise -------------------------------------------------------------------------------------
STEP_FAMILIES = [("sub16", 10, {}, "4 envs/wave"), ("sub32", 32, {}, "2 envs/wave"), ("wave1", 60, {}, "1 wave/env, all pairs"),
                 ("wave2", 100, {}, "2 waves/env, all pairs"), ("wave4", 256, {}, "4 waves/env, all pairs"),
                 ("wave8", 512, {}, "8 waves/env, all pairs"), ("wave16", 1024, dict(cells=0, team=0), "16 waves/env, all pairs"),
                 ("cells2", 100, dict(cells=1), "2 waves/env, cell list"), ("cells4", 256, dict(cells=1), "4 waves/env, cell list"),
                 ("cells8", 512, dict(cells=1), "8 waves/env, cell list"), ("cells16", 1024, dict(team=0), "16 waves/env, cell list")]


@pytest.mark.parametrize("family,n,opts,fam", STEP_FAMILIES, ids=[f[0] for f in STEP_FAMILIES])
def test_step_families_with_device_noise_in_regimes(ea, family, n, opts, fam):
    log = run_regimes(ea, family, n, opts, ("k_step", fam), ("persistent",), mode="step")
    TF.assert_floors(f"step {family}", n, log, "one step() with device noise in the off-default regimes")


# ---- d. rollout(T) == T x step() in regimes ---------------------------------------------------------------------------------------
LAUNCH_CASES = {
    # a wall-terminating room 1.6 x 0.25 (the leader reaches a wall within a few steps), Dict / cat observation, truncation at 17
    "wallterm_room16x025_dict_cat": (dict(width=1.6, height=0.25, step_size=0.06, eps=1e-3, is_termination_agent_wall_collision=True,
                                          is_new_exiting_reward=True, max_timesteps=17), dict(positions="rel", statuses="cat", type="Dict")),
    # sin/cos regime 0, enslaving degree 0, grav alpha 2.5
    "noise25_ens0_grav25": (dict(width=2.5, height=1.3, noise_coef=2.5, enslaving_degree=0.0, step_size=0.05, eps=1e-4,
                                 intrinsic_reward_coef=3.0, max_timesteps=17), dict(positions="grav", alpha=2.5)),
}


@pytest.mark.parametrize("case", list(LAUNCH_CASES))
@pytest.mark.parametrize("face,n", FACES_B, ids=[f"{f}-n{n}" for f, n in FACES_B])
def test_rollout_launch_equals_step_by_step_in_regimes(ea, face, n, case):
    kw, wrap_kw = LAUNCH_CASES[case]
    p = O.OracleParams(number_of_pedestrians=n, **kw)
    terms = TF.launch_equals_steps(ea, face, p, wrap_kw, 33, False)
    if p.is_termination_agent_wall_collision:
        assert sum(int(t.sum()) for t in terms) > 0, "no wall termination inside the launches"


# ---- e. the fused normalised step at large N ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 512, 1024])
def test_fused_normalised_step_matches_the_restated_chain_at_large_n(n):
    """evac_step_normalized against oracle/gym_wrappers.py (the tolerances of test_gpu_wrappers.
    test_normalized_vector_env_matches_the_restated_chain) in a 2.5 x 0.7 room, sin/cos regime 1, a generic observation.  At N = 1024
    env 0 meets the reference's NaN poisoning in its second episode: a pedestrian reset ESCAPED at the exit, outside this 0.7-high room,
    is reflected into it with its zero heading and becomes VISCEK, whose normalised heading is 0 / 0 (area.py:101).  The raw
    observation turns NaN, and the chain's np.clip keeps it NaN, as the kernel must."""
    import torch
    import evacuation_amd as ea
    E, T, gamma, seed = 6, 40, 0.97, 321
    cfg = ea.EnvConfig(number_of_pedestrians=n, width=2.5, height=0.7, noise_coef=1.0, eps=1e-4, step_size=0.05, max_timesteps=13,
                       is_new_exiting_reward=True, intrinsic_reward_coef=3.0)
    wrap = ea.EnvWrappersConfig(positions="abs", statuses="cat", type="Box")
    nenv = ea.NormalizedVectorEnv.make(cfg, wrap, num_envs=E, gamma=gamma, seed=seed)
    raw = ea.BatchedEvacuationEnv(dataclasses.replace(cfg, clip_action=True), wrap, num_envs=E, seed=seed)
    D = raw.obs_dim
    stats = [G.WrappedEnvStats(D, gamma=gamma) for _ in range(E)]
    o_n, _ = nenv.reset()
    o_r, _ = raw.reset()
    want = np.stack([stats[e].observation(o_r[e].cpu().numpy().astype(np.float64)) for e in range(E)])
    np.testing.assert_allclose(o_n.cpu().numpy(), want, rtol=0, atol=2e-6)
    rng = np.random.default_rng(n)
    n_done, saw_nan = 0, False
    for t in range(T):
        act = torch.as_tensor(rng.uniform(-1.6, 1.6, (E, 2)).astype(np.float32)).cuda()
        on, rn, ten, trn, infn = nenv.step(act, fused=True)
        orr, rr, ter, trr, infr = raw.step(act)
        assert (ten == ter).all() and (trn == trr).all()
        te, tr = ter.cpu().numpy(), trr.cpu().numpy()
        saw_nan |= bool(torch.isnan(orr).any())
        w_obs, w_fin, w_rew = G.vector_step(stats, orr.cpu().numpy().astype(np.float64),
                                            infr["final_observation"].cpu().numpy().astype(np.float64),
                                            rr.cpu().numpy().astype(np.float64), te, tr)
        np.testing.assert_allclose(on.cpu().numpy(), w_obs, rtol=0, atol=2e-6, equal_nan=True, err_msg=f"t={t} obs")
        np.testing.assert_allclose(rn.cpu().numpy(), w_rew, rtol=1e-5, atol=1e-6, err_msg=f"t={t} reward")
        done = (te | tr).astype(bool)
        n_done += int(done.sum())
        if done.any():
            np.testing.assert_allclose(infn["final_observation"].cpu().numpy()[done], w_fin[done], rtol=0, atol=2e-6, equal_nan=True)
    assert n_done >= 2 * E
    assert saw_nan or n != 1024, "the N = 1024 case no longer reaches the NaN poisoning"
    st = nenv.norm_state.cpu().numpy()
    for e in range(E):
        np.testing.assert_allclose(st[e, :D], stats[e].obs_rms.mean, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(st[e, D:2 * D], stats[e].obs_rms.var, rtol=1e-8, atol=1e-12)
        assert abs(st[e, 2 * D] - stats[e].obs_rms.count) < 1e-9
        np.testing.assert_allclose(st[e, 3 * D + 3], stats[e].returns[0], rtol=1e-6)
    o = on.cpu().numpy()
    assert (np.isnan(o) | (np.abs(o) <= 1.0)).all()
    nenv.close(); raw.close()
