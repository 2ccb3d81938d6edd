"""The frame lists built by evacuation_amd.trajectory are the REFERENCE's own rendering memory (SURVEY.md 8(f)
row 4): a reference env run with draw=True filled ``pedestrians.memory`` / ``agent.memory`` through ITS Pedestrians.save /
Agent.save (pedestrians.py:33-35, area.py:32-33, env.py:137,153-155), recorded in tests/golden/reference_runs.npz
(memory_*: positions and the leader's positions with the reference's dtypes, statuses as codes); the same trajectory, laid
out like rollout(capture_envs=K)'s device record, must come out of capture_to_memory as the same lists -- lengths,
element types, dtypes, shapes and values.  (The reference's save_animation itself pins matplotlib 3.8.0 and does not
run under this image's 3.10, whatever the data.)"""
import os
import types

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_runs.npz")


def test_capture_to_memory_equals_the_reference_memory():
    from evacuation_amd.statuses import Status
    from evacuation_amd.trajectory import capture_to_memory, feed_reference_env
    with np.load(FIXTURE) as z:
        n, T = int(z["memory_n"]), int(z["memory_T"])
        ref_pos, ref_st, ref_ag = z["memory_positions"], z["memory_statuses"], z["memory_agent_position"]
    assert ref_pos.shape == (T + 1, n, 2) and ref_st.shape == (T + 1, n) and ref_ag.shape == (T, 2)
    initial = {"pos": ref_pos[0][None], "status": ref_st[0][None]}
    # the layout of rollout(capture_envs=1): [T, K, N, 2] / [T, K, N] (status codes as f32) / [T, K, 2]
    ro = {"positions": ref_pos[1:, None], "statuses": ref_st[1:, None].astype(np.float32), "agent_positions": ref_ag[:, None]}
    ped_mem, agent_mem = capture_to_memory(ro, 0, initial=initial, status_cls=Status)
    assert set(ped_mem) == {"positions", "statuses"} and set(agent_mem) == {"position"}
    assert len(ped_mem["positions"]) == len(ped_mem["statuses"]) == T + 1            # reset frame + one per step
    assert len(agent_mem["position"]) == T                                            # the leader has no reset frame
    for a, b in zip(ped_mem["positions"], ref_pos):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
    for a, b in zip(ped_mem["statuses"], ref_st):
        assert a.dtype == object and a.shape == b.shape and all(x is Status(int(c)) for x, c in zip(a, b))
    for a, b in zip(agent_mem["position"], ref_ag):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
    # and what save_animation reads survives the hand-over (pedestrians.memory, agent.memory and time.now only)
    fresh = types.SimpleNamespace(pedestrians=types.SimpleNamespace(memory=None), agent=types.SimpleNamespace(memory=None),
                                  time=types.SimpleNamespace(now=0))
    feed_reference_env(fresh, ped_mem, agent_mem)
    sel = fresh.pedestrians.memory["statuses"][T] == Status.VISCEK                    # env.py:303 does exactly this
    assert sel.dtype == bool and sel.shape == (n,) and fresh.time.now == T
    assert (sel == (ref_st[T] == Status.VISCEK.value)).all()
    assert fresh.pedestrians.memory["positions"][T][sel, 0].shape == (int(sel.sum()),)
