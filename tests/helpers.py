"""Shared helpers for the oracle / parity tests (test infrastructure)."""
from __future__ import annotations

import glob
import json
import os

import numpy as np

from oracle import evac_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def traj_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "traj_*.npz")))


def load_params(js) -> O.OracleParams:
    return O.OracleParams(**json.loads(str(js)))


def state_at(d, k, dtype=np.float64) -> O.OracleState:
    return O.OracleState(np.array(d["pos"][k], dtype=dtype), np.array(d["dir"][k], dtype=dtype),
                         np.array(d["status"][k], dtype=np.int8), np.array(d["agent_pos"][k], dtype=np.float32),
                         np.array(d["agent_dir"][k], dtype=np.float32), int(d["now"][k]))


def episode_record_files():
    """Fixtures that end with the reference's own per-episode record (env.py:114-127, captured by make_golden.capture_episode_record):
    the trajectories that ran to truncation, and the crafted episode that terminates with every pedestrian escaped."""
    out = [f for f in traj_files() if "episode_record" in np.load(f).files]
    extra = os.path.join(GOLDEN, "episode_all_escaped.npz")
    return out + ([extra] if os.path.exists(extra) else [])


def crafted_cases():
    d = np.load(os.path.join(GOLDEN, "crafted.npz"))
    for name in d["names"]:
        name = str(name)
        yield name, {k[len(name) + 2:]: d[k] for k in d.files if k.startswith(name + "__")}


OBS_VARIANTS = [(p, s, t) for p in ("abs", "rel") for s in ("no", "ohe", "cat") for t in ("Box", "Dict")
                if not (p == "abs" and s == "no" and t == "Dict")]


def check_observations(get, st: O.OracleState, eps: float, tol=1e-12):
    """Compare every observation variant of the oracle with the fixture's (``get(key)``)."""
    for a in (2, 3, 5):
        o = O.observe(st, "grav", alpha=a, eps=eps)
        for k, v in o.items():
            ref = get(f"obs_grav_a{a}__{k}")
            np.testing.assert_allclose(v, ref, rtol=tol, atol=tol, equal_nan=True, err_msg=f"grav a={a} {k}")
            assert np.asarray(v).dtype == ref.dtype, (k, np.asarray(v).dtype, ref.dtype)
    for pos, stat, typ in OBS_VARIANTS:
        o = O.observe(st, pos, stat, typ)
        name = f"obs_{pos}_{stat}_{typ.lower()}"
        if typ == "Box":
            ref = get(name)
            np.testing.assert_allclose(o, ref, rtol=tol, atol=tol, equal_nan=True, err_msg=name)
            assert o.dtype == ref.dtype and o.shape == ref.shape, (name, o.dtype, ref.dtype)
        else:
            for k, v in o.items():
                ref = get(f"{name}__{k}")
                np.testing.assert_allclose(v, ref, rtol=tol, atol=tol, equal_nan=True, err_msg=f"{name} {k}")
                assert np.asarray(v).dtype == ref.dtype, (name, k, np.asarray(v).dtype, ref.dtype)


def random_states(n):
    """Oracle-generated states of every kernel geometry (tests/test_gpu_parity.py::test_random_states_all_sizes): a random reset,
    then e * 3 oracle steps to mix the statuses.  Returns (params, pre-states, actions, noise) of one teacher-forced step."""
    rng = np.random.default_rng(100 + n)
    p = O.OracleParams(number_of_pedestrians=n, is_new_exiting_reward=True, intrinsic_reward_coef=0.5, enslaving_degree=0.7)
    E = 6 if n <= 256 else 3
    pre, acts, nzs = [], [], []
    for e in range(E):
        st = O.env_reset(p, rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2)))
        for _ in range(e * 3):
            O.env_step(p, st, rng.uniform(-1, 1, 2).astype(np.float32), rng.uniform(-0.1, 0.1, n))
        pre.append(st)
        acts.append(rng.uniform(-1, 1, 2).astype(np.float32))
        nzs.append(rng.uniform(-0.1, 0.1, n).astype(np.float32))
    return p, pre, acts, nzs


def late_episode_states(n):
    """Crafted late-episode states (tests/test_gpu_parity.py::test_late_episode_states_with_few_rows): 80 % escaped, a flock
    around the leader, a handful of loners, one dense knot.  Returns (params, pre-states, actions, noise)."""
    rng = np.random.default_rng(7000 + n)
    p = O.OracleParams(number_of_pedestrians=n, is_new_exiting_reward=True, is_new_followers_reward=True, enslaving_degree=1.0)
    pre, acts, nzs = [], [], []
    for e in range(4):
        pos = rng.uniform(-1, 1, (n, 2))
        d = rng.uniform(-1, 1, (n, 2))
        agent = rng.uniform(-0.6, 0.6, 2).astype(np.float32)
        k_esc = int(n * (0.8 if e < 3 else 0.5))
        esc = rng.permutation(n)[:k_esc]
        rest = np.setdiff1d(np.arange(n), esc)
        flock = rest[: max(1, (2 * len(rest)) // 3)]                          # followers: inside the leader's radius
        pos[flock] = agent + rng.uniform(-0.12, 0.12, (len(flock), 2))
        knot = rest[len(flock):][: max(0, len(rest) // 6)]                    # loners that see each other
        pos[knot] = np.array([0.7, 0.6]) + rng.uniform(-0.05, 0.05, (len(knot), 2))
        pos[esc] = O.EXIT_POSITION
        d[esc] = 0.0
        with np.errstate(all="ignore"):
            st = O.env_reset(p, pos, d)               # (normalises the directions: 0 / 0 for the escaped, overwritten below)
        st.dir[esc] = 0.0
        st.agent_pos = agent.copy()
        st.agent_dir = (rng.uniform(-1, 1, 2) * 0.01).astype(np.float32)
        st.status = O.classify_statuses(st.pos, st.agent_pos, O.EXIT_POSITION, st.pos.dtype)
        st.now = 1200 + e
        assert (st.status == O.ESCAPED).sum() >= k_esc and (st.status == O.VISCEK).sum() <= max(8, n // 4)
        pre.append(st)
        acts.append(rng.uniform(-1, 1, 2).astype(np.float32))
        nzs.append(rng.uniform(-0.1, 0.1, n).astype(np.float32))
    return p, pre, acts, nzs
