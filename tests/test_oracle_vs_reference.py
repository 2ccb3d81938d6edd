"""The oracle side by side with the real reference, through the reference's own outputs recorded in
tests/golden/reference_runs.npz (tests/golden/make_golden.py, make_reference_runs).

Route 1 (stub-free, tests/golden/_reference_loader.load_core) executed the reference's own
area/pedestrians/statuses/distances/reward modules with nothing replaced; the oracle runs here on the
same draws of the global NumPy RNG and must reproduce every recorded step."""
import os

import numpy as np
import pytest

from oracle import evac_oracle as O

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_runs.npz")


@pytest.fixture(scope="module")
def ref():
    with np.load(FIXTURE) as z:
        return dict(z)


@pytest.mark.parametrize("n,seed,noise,ens", [(60, 11, 0.2, 1.0), (60, 12, 0.8, 0.5), (17, 13, 0.05, 0.1), (256, 14, 0.2, 1.0)])
def test_core_dynamics_free_running_same_global_rng(ref, n, seed, noise, ens):
    key = f"core_{n}_{seed}_"
    p = O.OracleParams(number_of_pedestrians=n, noise_coef=noise, enslaving_degree=ens,
                       is_new_exiting_reward=True, is_new_followers_reward=True)
    np.random.seed(seed)
    st = O.env_reset(p, *O.draw_reset(n))
    np.testing.assert_array_equal(st.pos, ref[key + "reset_pos"])
    act = np.random.Generator(np.random.PCG64(seed))
    steps = 150 if n <= 60 else 30
    assert ref[key + "pos"].shape == (steps, n, 2)
    for t in range(steps):
        a = act.uniform(-1, 1, 2).astype(np.float32)
        nz = O.draw_step_noise(p, st)                  # the global stream the reference's step consumed
        out = O.env_step(p, st, a, nz)
        np.testing.assert_allclose(st.pos, ref[key + "pos"][t], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(st.dir, ref[key + "dir"][t], rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(st.status, ref[key + "status"][t])
        np.testing.assert_array_equal(st.agent_pos, ref[key + "agent_pos"][t])
        np.testing.assert_allclose(out["reward_ped"], ref[key + "reward_ped"][t], rtol=1e-12)
        np.testing.assert_allclose(out["intrinsic"], ref[key + "intrinsic"][t], rtol=1e-9)
        assert out["reward_agent"] == ref[key + "reward_agent"][t]


def test_full_env_with_shells_matches_stub_free_core(ref):
    """The gymnasium/wandb shells used for fixture generation do not change the dynamics: the setup_env surface (route 2)
    and the stub-free core (route 1) recorded the same trajectory bit for bit -- and the oracle reproduces it."""
    np.testing.assert_array_equal(ref["full_pos"], ref["fullcore_pos"])
    np.testing.assert_array_equal(ref["full_reward"], ref["fullcore_reward"])
    p = O.OracleParams(number_of_pedestrians=30, is_new_exiting_reward=True)
    np.random.seed(5)
    st = O.env_reset(p, *O.draw_reset(30))
    for t, a in enumerate(ref["full_actions"]):
        out = O.env_step(p, st, a, O.draw_step_noise(p, st))
        np.testing.assert_allclose(st.pos, ref["full_pos"][t], rtol=1e-9, atol=1e-9)
        assert out["reward_agent"] + out["reward_ped"] == pytest.approx(ref["full_reward"][t], rel=1e-12, abs=1e-12)
