"""Every rollout kernel and form, teacher-forced against the reference-precision oracle one step at a time, and each T-step
launch against T step launches, bit for bit.

Part A: a batch of recorded (tests/golden/traj_*.npz), crafted (crafted.npz, embedded in larger rooms) and oracle-generated
pre-states is set through the public surface (set_state, then a direct write of clock[:, 1:3] and acc), the PRODUCTION face runs
one step (rollout(1): no injected noise, no recorded actions, no capture), and the oracle steps the same f32 pre-states with the
action and the Philox noise the device used.  compare_step (tests/test_gpu_parity.py) holds slab[0] and the state to it with its
tie model; an env that finished is held to the oracle's reward and flags, to O.env_reset on its Philox reset draws and to the
oracle's episode record started from the seeded accumulators.  Every 8th env stands one step before truncation, so that every
face truncates and autoresets.

Part B: rollout(T) of each face == T calls of step() of the same family (teams == Cells<16>, CU-wide Wave<w, 1024> == Wave<w>),
fed the actions the rollout draws on device and then one shared action tensor, with truncations inside: observations, rewards,
flags, episode records, final state, clock and accumulators, as int32 views.
"""
import functools
import os

import numpy as np
import pytest

from oracle import evac_oracle as O
from oracle import philox as P
from tests import helpers as H
from tests.test_gpu_parity import cfg_from_params, check_reset, compare_step, ea, oracle_step  # noqa: F401  (fixture)
from tests.test_gpu_production_faces import FACE_LOG

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0x5EED00A7, 3000                # a shard of a larger job: global env ids from OFFSET
WRAPS = (dict(positions="grav", alpha=3), dict(positions="rel", statuses="ohe", type="Box"))

# (face, rooms, KernelOptions fields, substrings of kernel_variant("rollout"), substrings it must not have).  chain = 0 unless the
# face is a chained or persistent one: an automatic choice must not move a face to another form.
FACES = [
    ("sub16", (8, 10), dict(chain=0), ("4 envs/wave",), ()),
    ("sub32", (17, 32), dict(chain=0), ("2 envs/wave",), ()),
    ("wave1", (60,), dict(cu_wide=0, chain=0), ("1 wave/env, all pairs",), ("CU-wide",)),
    ("wave1_cu_wide", (60,), dict(cu_wide=1, chain=0), ("1 wave/env, all pairs, CU-wide",), ("chained", "persistent", "streams")),
    ("wave1_cu_wide_chained", (60,), dict(cu_wide=1, chain=1), ("1 wave/env, all pairs, CU-wide", "chained launches"), ()),
    ("wave1_cu_wide_persistent", (60,), dict(cu_wide=1, chain=2), ("1 wave/env, all pairs, CU-wide", "one persistent kernel"), ()),
    ("wave1_cu_wide_parts2", (60,), dict(cu_wide=1, chain=0, parts=2), ("1 wave/env, all pairs, CU-wide", "x 2 streams"), ()),
    ("wave2", (100,), dict(chain=0), ("2 waves/env, all pairs",), ()),
    ("wave8", (512,), dict(chain=0), ("8 waves/env, all pairs",), ()),
    ("wave4", (256,), dict(cu_wide=0, chain=0), ("4 waves/env, all pairs",), ("CU-wide",)),
    ("wave4_cu_wide", (256,), dict(cu_wide=1, chain=0), ("4 waves/env, all pairs, CU-wide",), ("chained", "persistent")),
    ("wave4_cu_wide_chained", (256,), dict(cu_wide=1, chain=1), ("4 waves/env, all pairs, CU-wide", "chained launches"), ()),
    ("wave4_cu_wide_persistent", (256,), dict(cu_wide=1, chain=2), ("4 waves/env, all pairs, CU-wide", "one persistent kernel"), ()),
    ("wave16", (600, 1024), dict(cells=0, team=0, chain=0), ("16 waves/env, all pairs",), ()),
    ("cells2", (100,), dict(cells=1, chain=0), ("2 waves/env, cell list",), ()),
    ("cells4", (256,), dict(cells=1, chain=0), ("4 waves/env, cell list",), ()),
    ("cells8", (512,), dict(cells=1, chain=0), ("8 waves/env, cell list",), ()),
    ("cells16", (1024,), dict(team=0, chain=0), ("16 waves/env, cell list",), ()),
] + [(f"team{k}" + ("_persistent" if c else ""), (513, 777, 1024), dict(team=k, chain=c), (f"{k} CUs/env",) + (("one persistent kernel",) if c else ()),
      () if c else ("persistent",)) for k in (2, 4, 8, 16) for c in (0, 2)]
FACE = {f[0]: f for f in FACES}
CASES = [(f[0], n) for f in FACES for n in f[1]]
CRAFTED_ROOMS = {f[1][0] for f in FACES}       # the crafted cases run in every face, in its first room


def _padded_len(n, k):
    """Envs in a batch of k states: whole CU-wide workgroups of one-wave envs (16, and >= 32 for the chained form), of four-wave
    envs (4); teams of up to 16 CUs per env in rows of 8 envs must fit 256 CUs (<= 16 envs)."""
    if n <= 64:
        return max(32, -(-k // 16) * 16)
    if n <= 512:
        return -(-k // 16) * 16
    assert k <= 16, k
    return k if k > 8 or k == 1 else 8


def _embed(c, n):
    """A crafted 8-pedestrian case in a room of n: the N - 8 others ESCAPED, pinned at the exit, heading nowhere."""
    k = len(c["pre_status"])
    pos = np.zeros((n, 2)); d = np.zeros((n, 2)); s = np.full(n, O.ESCAPED, np.int8)
    pos[:] = O.EXIT_POSITION
    pos[:k], d[:k], s[:k] = c["pre_pos"], c["pre_dir"], c["pre_status"]
    return O.OracleState(pos, d, s, np.array(c["pre_agent_pos"], np.float32), np.array(c["pre_agent_dir"], np.float32), int(c["pre_now"]))


def pad_batch(n, label, p, pre, acts):
    """A batch of room n from k pre-states and their actions: (label, params, states, actions, t_e, n_resets, acc), padded to what
    every face of room n can launch.  A repeated state gets another Philox step counter (other noise); every 8th env stands at
    max_timesteps - 1."""
    E = _padded_len(n, len(pre))
    states, actions = [], []
    for e in range(E):
        st = pre[e % len(pre)].copy()
        if e % 8 == 7:
            st.now = p.max_timesteps - 1
        states.append(st)
        actions.append(np.asarray(acts[e % len(pre)], np.float32))
    t_e = 1000 + 7 * np.arange(E) + 4099 * (np.arange(E) // len(pre))   # (a repeat: another step counter, other noise)
    r = 1 + np.arange(E) % 3
    acc = np.stack([-0.25 - np.arange(E) % 5, 0.125 * (np.arange(E) % 3), -0.5 * (np.arange(E) % 7), np.zeros(E)], 1).astype(np.float32)
    return (label, p, states, np.stack(actions), t_e, r, acc)


def fixture_states(n, keep=lambda p: True):
    """(name, params, pre-states, actions) of every recorded trajectory of room n whose parameters `keep` admits."""
    out = []
    for f in H.traj_files():
        d = np.load(f)
        p = H.load_params(d["params_json"])
        if p.number_of_pedestrians == n and keep(p):
            out.append((os.path.basename(f)[:-4], p, [H.state_at(d, k) for k in range(len(d["action"]))], list(d["action"])))
    return out


@functools.lru_cache(maxsize=None)
def batches(n):
    """The batches of room n: every recorded trajectory of the room, oracle-generated random (and, from N = 60 on, late-episode)
    states, and the crafted cases in the first room of every face."""
    raw = fixture_states(n)
    for name, gen in (("random", H.random_states), ("late", H.late_episode_states)):
        if n >= 2 and (name == "random" or n >= 60):
            p, pre, acts, _ = gen(n)
            raw.append((f"{name}_n{n}", p, pre, acts))
    if n in CRAFTED_ROOMS:
        groups = {}
        for name, c in H.crafted_cases():
            g = groups.setdefault(str(c["params_json"]), ("crafted", H.load_params(c["params_json"]), [], [], []))
            g[2].append(_embed(c, n)); g[3].append(np.asarray(c["action"], np.float32)); g[4].append(name)
        for i, (_, p, pre, acts, names) in enumerate(groups.values()):
            p.number_of_pedestrians = n
            raw.append((f"crafted[{','.join(names)}]_n{n}", p, pre, acts))
    return [pad_batch(n, label, p, pre, acts) for label, p, pre, acts in raw]


@functools.lru_cache(maxsize=None)
def expected(source_of_batches, n, i, source):
    """The oracle's step of batch i of room n (``source_of_batches(n)[i]``), per env: (oracle_step, action, noise, reset draws of
    the autoreset)."""
    label, p, states, actions, t_e, r, acc = source_of_batches(n)[i]
    gid = OFFSET + np.arange(len(states))
    acts = actions if source == "fixture" else P.random_action(SEED, gid, t_e)
    noise = P.step_noise(SEED, gid, n, t_e, p.noise_coef)
    draws = P.reset_draws(SEED, gid, n, r)
    return [oracle_step(p, states[e], acts[e], noise[e]) for e in range(len(states))], acts, noise, draws


def _options(ea, **kw):
    return ea.KernelOptions().replace(**kw)


def _check_variant(name, want, absent):
    for s in want:
        assert s in name, (s, name)
    for s in absent:
        assert s not in name, (s, name)


def teacher_force_batch(ea, batch, expect, wraps, opts, want, absent, log, mode="rollout", group=""):
    """One batch of pre-states, teacher-forced for one step through the production face that `opts` selects, once per observation
    variant of `wraps`: set_state, a direct write of clock[:, 1:3] and acc, then rollout(1) (mode "rollout": the fixture's actions,
    then the device's RandomAgent; the persistent form takes no actions) or step() without injected noise (mode "step": the
    fixture's actions, then the RandomAgent's, both given), each held to the oracle stepped on the same Philox noise
    (``expect(source)``, see `expected`).  Envs that finished are held to the oracle's reset, clock, accumulators and episode record.
    Adds (pedestrian-steps compared, of, env-steps whose rewards / flags were compared, of) to `log` per (kernel variant, `group`)."""
    import torch
    from evacuation_amd.vector_env import STATS_FIELDS, stats_int_view
    label, p, states, actions, t_e, r, acc = batch
    n, E = p.number_of_pedestrians, len(states)
    sources = ("device",) if opts.get("chain") == 2 and mode == "rollout" else ("fixture", "device")
    for w in wraps:
        wrap = ea.EnvWrappersConfig(**w)
        env = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=E, seed=SEED, env_id_offset=OFFSET, options=_options(ea, **opts))
        name = env.kernel_variant(mode)
        _check_variant(name, want, absent)
        D = env.obs_dim
        for source in sources:
            orc, acts, noise, draws = expect(source)
            env.set_state(pos=np.stack([s.pos for s in states]).astype(np.float32), dir=np.stack([s.dir for s in states]).astype(np.float32),
                          status=np.stack([s.status for s in states]).astype(np.uint8),
                          agent_pos=np.stack([s.agent_pos for s in states]).astype(np.float32),
                          agent_dir=np.stack([s.agent_dir for s in states]).astype(np.float32),
                          now=np.array([s.now for s in states], dtype=np.int32))
            env.clock[:, 1] = torch.as_tensor(r, dtype=torch.int32, device=env.device)
            env.clock[:, 2] = torch.as_tensor(t_e, dtype=torch.int32, device=env.device)
            env.acc.copy_(torch.as_tensor(acc, device=env.device))
            if mode == "rollout":
                ro = env.rollout(1, actions=acts[None].astype(np.float32) if source == "fixture" else None)
                slab_t, stats_t = ro["slab"][0], ro["episode_stats"][0]
            else:
                obs, rew, te, tr, info = env.step(torch.as_tensor(np.asarray(acts, np.float32), device=env.device))
                slab_t = torch.cat([obs, rew[:, None], te[:, None].float(), tr[:, None].float()], dim=1)
                stats_t = info["episode_stats"]
            fin = {k: v.cpu().numpy() for k, v in env.get_state().items()}
            torch.cuda.synchronize()
            assert env.team_error() == 0
            slab = slab_t.cpu().numpy()
            f_stats, i_stats = stats_t.cpu().numpy(), stats_int_view(stats_t).cpu().numpy()
            clock, gacc = env.clock.cpu().numpy(), env.acc.cpu().numpy()
            done = (slab[:, D + 1] != 0) | (slab[:, D + 2] != 0)
            got = dict(obs=slab[:, :D], reward=slab[:, D], terminated=slab[:, D + 1] != 0, truncated=slab[:, D + 2] != 0, **fin)
            where = f"{name} {label} {w} {source}"
            cnt = {}
            compare_step(p, wrap, states, acts, noise, got, min_checked=0, oracle=orc, reset=done, counts=cnt)
            peds = E * n - cnt["peds_out"]
            for e in range(E):
                st, out, tied, _, _ = orc[e]
                now, at = states[e].now, f"{where} env {e}"
                if not done[e]:
                    assert tuple(clock[e, :3]) == (now + 1, r[e], t_e[e] + 1), (at, clock[e])
                    if not tied.any():
                        np.testing.assert_allclose(gacc[e, :3], acc[e, :3] + [out["reward"], out["intrinsic"], out["reward_agent"] + out["reward_ped"]],
                                                   rtol=1e-5, atol=1e-5, err_msg=f"{at} acc")
                    continue
                assert tuple(clock[e, :3]) == (0, r[e] + 1, t_e[e] + 1), (at, clock[e])
                assert (gacc[e] == 0).all(), (at, gacc[e])
                if not check_reset(p, wrap, draws[e], {k: v[e] for k, v in fin.items()}, slab[e, :D], label=at):
                    peds -= n - int(tied.sum())                  # (a reset near a status threshold: statuses not compared)
                log_ = O.EpisodeLog(int(t_e[e]))
                log_.episode_reward, log_.episode_intrinsic_reward, log_.episode_status_reward = (float(a) for a in acc[e, :3])
                log_.after_step(out)
                rec = log_.record(st)
                assert int(i_stats[e, 0]) == rec["overall_timesteps"] and int(i_stats[e, 1]) == r[e], (at, i_stats[e])
                assert f_stats[e, STATS_FIELDS.index("episode_length")] == rec["episode_length"], at
                if tied.any():
                    continue                                     # (counts and sums depend on the tie's outcome)
                for j, k in enumerate(STATS_FIELDS):
                    if k.endswith("_pedestrians"):
                        assert f_stats[e, j] == rec[k], (at, k, f_stats[e, j], rec[k])
                    elif k != "episode_length":
                        np.testing.assert_allclose(f_stats[e, j], rec[k], rtol=1e-5, atol=1e-4, err_msg=f"{at} {k}")
            a = log.setdefault((name, group), [0, 0, 0, 0])
            a[0] += peds; a[1] += E * n; a[2] += cnt["checked"]; a[3] += E
        env.close()


def assert_floors(face, n, log, what):
    """Each variant's counts to FACE_LOG, and the per-face floors (rewards / flags, pedestrian-steps); measured on an MI355X:
    >= 98.2 % / 99.97 % of every variant at n <= 512, >= 87.5 % / 99.9 % at n > 512 (an N = 1024 env has ~5e5 pair distances:
    about one in eight meets a near-tie)."""
    for (name, group), (peds, all_peds, scalars, all_scalars) in log.items():
        if group:       # (the summary prints 96 characters: the face, the room, the group, which instantiation)
            kind = ("default-config" if "_default_config<" in name else "generic") + (" grav" if ", grav obs>" in name else " generic-obs")
            label = f"{face}, n = {n}, {group}: {kind}"
        else:
            label = f"{name} -- {what}, n = {n}"
        FACE_LOG.append((label, peds, all_peds, scalars, all_scalars))
    peds, all_peds, scalars, all_scalars = (sum(v[j] for v in log.values()) for j in range(4))
    lo_s, lo_p = (0.97, 0.995) if n <= 512 else (0.85, 0.99)
    assert scalars >= lo_s * all_scalars and peds >= lo_p * all_peds, (face, n, peds, all_peds, scalars, all_scalars)


@pytest.mark.parametrize("face,n", CASES, ids=[f"{f}-n{n}" for f, n in CASES])
def test_rollout_step_teacher_forced_vs_oracle(ea, face, n):
    _, _, opts, want, absent = FACE[face]
    log = {}
    for i, batch in enumerate(batches(n)):
        teacher_force_batch(ea, batch, functools.partial(expected, batches, n, i), WRAPS, opts, want, absent, log)
    assert_floors(face, n, log, "one step from recorded states")
    if n in CRAFTED_ROOMS:
        assert any("_default_config<" in k for k, _ in log) and any("_default_config<" not in k for k, _ in log), list(log)


def _step_family(rollout_name):
    """The step kernel a rollout face is specified to equal bit for bit: teams == Cells<16>, CU-wide Wave<w, 1024> == Wave<w>."""
    if "CUs/env" in rollout_name:
        return "16 waves/env, cell list"
    fam = rollout_name.split("<", 1)[1].split(", grav obs>")[0].split(", generic obs>")[0]
    return fam.replace(", CU-wide workgroups", "")


@pytest.mark.parametrize("T", [7, 33])
@pytest.mark.parametrize("face,n", CASES, ids=[f"{f}-n{n}" for f, n in CASES])
def test_rollout_launch_equals_step_by_step(ea, face, n, T):
    """rollout(T) == T x step(), bit for bit, from the same seeded reset: first the actions the rollout draws on device, then (where the
    form takes actions) one shared action tensor in a second launch that continues from the first.  T = 7 runs the default
    configuration with max_timesteps 5, T = 33 a generic one (enslaving_degree 0.7, intrinsic reward) with max_timesteps 17."""
    default = T == 7
    p = O.OracleParams(number_of_pedestrians=n, is_new_exiting_reward=True, max_timesteps=5 if default else 17,
                       enslaving_degree=1.0 if default else 0.7, intrinsic_reward_coef=0.0 if default else 0.5)
    launch_equals_steps(ea, face, p, WRAPS[0 if default else 1], T, default)


def launch_equals_steps(ea, face, p, wrap_kw, T, default):
    """rollout(T) of `face` == T x step() of its step family, bit for bit (see test_rollout_launch_equals_step_by_step), for the
    configuration `p` and the observation `wrap_kw`; `default`: whether the default-configuration kernels must run.  Returns the
    rollouts' terminated flags, one [T, E] array per launch."""
    import torch
    from evacuation_amd.vector_env import stats_int_view
    _, _, opts, want, absent = FACE[face]
    n = p.number_of_pedestrians
    wrap = ea.EnvWrappersConfig(**wrap_kw)
    E = 32 if n <= 64 else 16
    a = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=E, seed=SEED, env_id_offset=OFFSET, options=_options(ea, **opts))
    b = ea.BatchedEvacuationEnv(cfg_from_params(ea, p), wrap, num_envs=E, seed=SEED, env_id_offset=OFFSET,
                                options=_options(ea, **dict(opts, chain=0, parts=1)))
    name = a.kernel_variant("rollout")
    _check_variant(name, want, absent)
    assert ("_default_config<" in name) == default, name
    assert _step_family(name) in b.kernel_variant("step"), (name, b.kernel_variant("step"))
    a.reset(); b.reset()
    gid = OFFSET + np.arange(E)
    rng = np.random.default_rng(n + T)
    launches = [None] + ([] if opts.get("chain") == 2 else [rng.uniform(-1.2, 1.2, (T, E, 2)).astype(np.float32)])
    n_done, t0, terms = 0, 0, []
    for acts in launches:
        ro = a.rollout(T, actions=acts)
        terms.append(ro["terminated"].cpu().numpy() != 0)
        for t in range(T):
            act = acts[t] if acts is not None else P.random_action(SEED, gid, t0 + t)
            obs, r, te, tr, info = b.step(torch.as_tensor(act, device=b.device))
            at = f"{name} launch {'given' if acts is not None else 'device'} actions, step {t}"
            assert torch.equal(obs.view(torch.int32), ro["obs"][t].view(torch.int32)), at
            assert torch.equal(r.view(torch.int32), ro["reward"][t].view(torch.int32)), at
            assert (te == ro["terminated"][t]).all() and (tr == ro["truncated"][t]).all(), at
            done = (te | tr).bool()
            n_done += int(done.sum())
            if done.any():
                assert torch.equal(info["episode_stats"][done].view(torch.int32), ro["episode_stats"][t][done].view(torch.int32)), at
                assert torch.equal(stats_int_view(info["episode_stats"][done]), stats_int_view(ro["episode_stats"][t][done])), at
        t0 += T
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert torch.equal(sa[k].view(torch.uint8), sb[k].view(torch.uint8)), (name, k)
        assert torch.equal(a.clock, b.clock), name
        assert torch.equal(a.acc.view(torch.int32), b.acc.view(torch.int32)), name
    torch.cuda.synchronize()
    assert a.team_error() == 0
    assert n_done >= E
    a.close(); b.close()
    return terms
