"""The recording evaluation (evac_policy_evaluate*_capture, policy_evaluate(capture=...), PolicyEvaluator.evaluate(capture_envs=),
EvaluationResult.episode_memory, RPOTrainer.evaluate(capture_envs=), examples/train_rpo.py --capture) on an MI355X.

E = 20 envs, K = 18 recorded (two workgroups of 16 envs, the second part-filled, the capture boundary inside it, envs 18 and 19
unrecorded), N = 10, max_timesteps = 12, three episodes: at most 36 steps per env; N = 64 for the linear network (a full wave: the
owner lane writes the leader's row too) and N = 62 for the transformer (all 64 token lanes).  Every buffer starts as NaN.  Every
comparison is bit for bit.

6. Recording changes nothing: records, progress and state against a twin handle without a capture.  7. Sample mode: the frames are
the plain rollout's trajectory under policy_rollout's stored actions.  8. Mean mode is sample mode with sigma = 0.  9. The scripted
agent: the host WacuumCleaner's actions from the recorded leader rows, replayed through the plain rollout.  10. Start frames.
11. Terminal frames against the episode records.  12. Resumption and bounds.  13. The C ABI's refusals.  14. The Python faces."""
import copy
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, OFFSET = 20261020, 5
E, K, EPISODES, MAX_T = 20, 18, 3, 12
FRAMES = EPISODES * MAX_T
STATE = ("ped", "status", "agent", "clock", "acc")
GRAV, BOX = dict(positions="grav", alpha=3), dict(positions="rel", statuses="ohe", type="Box")
KINDS = {
    # name: (network or None for the scripted agent, N, EnvConfig kwargs beside N and max_timesteps, EnvWrappersConfig kwargs)
    "linear": ("linear", 10, dict(is_new_exiting_reward=True), GRAV),
    "deepsets": ("deepsets", 10, {}, BOX),
    "transformer": ("transformer", 10, {}, BOX),
    "linear_n64": ("linear", 64, dict(is_new_exiting_reward=True), GRAV),
    "transformer_n62": ("transformer", 62, {}, BOX),
    "scripted": (None, 10, dict(width=0.7, height=0.6, step_size=0.1), GRAV),
}
NETWORKS = ("linear", "deepsets", "transformer")


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import evacuation_amd
    from evacuation_amd import build
    build.build_library()
    return evacuation_amd


def raw(t):
    import torch
    return t.contiguous().view(-1).view(torch.uint8)


def make_env(ea, kind, max_t=MAX_T):
    """A raw handle of the kind, reset, every fifth env one step before truncation and its neighbour two: every handle of a kind
    starts from the same state.  (One-wave step kernels for the plain rollout too, as the evaluation's.)  ``max_t``, ``episodes``
    of the helpers below: tests/test_gpu_policy_long.py runs them with longer episodes."""
    from evacuation_amd.options import KernelOptions
    _, N, cfg_kw, wrap_kw = KINDS[kind]
    env = ea.BatchedEvacuationEnv(ea.EnvConfig(number_of_pedestrians=N, max_timesteps=max_t, **cfg_kw), ea.EnvWrappersConfig(**wrap_kw),
                                  num_envs=E, seed=SEED, env_id_offset=OFFSET, options=KernelOptions().replace(subwave=0))
    env.reset()
    now = env.get_state()["now"].clone()
    now[::5] = max_t - 1
    now[1::5] = max_t - 2
    env.set_state(now=now)
    return env


_nets = {}


def make_net(ea, kind, sigma_zero=False):
    """The kind's network with visible actions (larger last layer, biases, two sigmas; LayerNorms off their defaults)."""
    import torch
    from evacuation_amd.policy import DeepSetsActorCritic, LinearActorCritic, TransformerActorCritic
    if (kind, sigma_zero) in _nets:
        return _nets[kind, sigma_zero]
    if sigma_zero:
        net = copy.deepcopy(make_net(ea, kind))
        with torch.no_grad():
            net.actor_logstd.fill_(float("-inf"))            # expf gives 0 exactly: mu + 0 z = mu
        _nets[kind, True] = net
        return net
    network, N, _, wrap_kw = KINDS[kind]
    D = 6 if wrap_kw is GRAV else (N + 2) * 6
    torch.manual_seed(3)
    net = {"linear": lambda: LinearActorCritic(D), "deepsets": lambda: DeepSetsActorCritic(D, N),
           "transformer": lambda: TransformerActorCritic(D, N)}[network]()
    with torch.no_grad():
        net.actor_mean[4].weight.mul_(60.0)
        net.actor_logstd.copy_(torch.tensor([[-0.5, 0.3]]))
        for m in list(net.actor_mean) + list(net.critic):
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.2)
        if network == "deepsets":
            net.deep_sets.transform_rho[0].weight.mul_(3.0 / (N + 2))
        if network == "transformer":
            for m in net.embedding.modules():
                if isinstance(m, torch.nn.LayerNorm):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.normal_(0.0, 0.3)
    _nets[kind, False] = net.to("cuda:0")
    return _nets[kind, False]


def frozen_statistics(env):
    import torch
    g = torch.Generator().manual_seed(5)
    D = env.obs_dim
    ns = torch.zeros((E, 3 * D + 4), dtype=torch.float64)
    ns[:, :D] = torch.randn((E, D), generator=g, dtype=torch.float64) * 0.1
    ns[:, D:2 * D] = torch.rand((E, D), generator=g, dtype=torch.float64) + 0.05
    return (ns.to(env.device), 1.0, 1e-8)


def nan_buffers(env, rows=FRAMES, episodes=EPISODES, k=K):
    import torch
    full = lambda n: torch.full((n, k, env.n_ped + 1, 3), float("nan"), dtype=torch.float32, device=env.device)       # noqa: E731
    return {"frames": full(rows), "starts": full(episodes)}


def agent_of(ea, kind, mode):
    if KINDS[kind][0] is None:
        return "vacuum_cleaner", {}
    return make_net(ea, kind, sigma_zero=(mode == "sample0")), {"deterministic": mode == "mean"}


def evaluate(ea, kind, mode, *, capture=True, norm=False, max_steps=100000, episodes=EPISODES, buffers=None, max_t=MAX_T):
    """One evaluation of a fresh handle of the kind until every env has finished ``episodes`` episodes.  ``mode``: "mean",
    "sample", "sample0" (sample mode of the network with sigma = 0); ignored by the scripted agent."""
    import torch
    env = make_env(ea, kind, max_t)
    agent, kw = agent_of(ea, kind, mode)
    if norm:
        kw["_norm"] = frozen_statistics(env)
    start = {k: v.clone() for k, v in env.get_state().items()}
    if capture:
        kw["capture"] = buffers if buffers is not None else nan_buffers(env, rows=episodes * max_t, episodes=episodes)
    progress = out = None
    calls = 0
    while progress is None or int(progress[:, 0].min()) < episodes:
        progress, out = env.policy_evaluate(agent, episodes, max_steps, progress, out, **kw)
        calls += 1
        assert calls <= episodes * max_t + 1
    torch.cuda.synchronize()
    run = types.SimpleNamespace(progress=progress, records=out, state={k: getattr(env, k).clone() for k in STATE}, start=start,
                                final=env.get_state(), calls=calls, n_ped=env.n_ped, **(kw.get("capture") or {}))
    env.close()
    return run


_runs = {}


def recorded(ea, kind, mode, norm=False, episodes=EPISODES, max_t=MAX_T):
    """The one long recorded evaluation per (kind, mode, norm, episodes, max_t), shared by the tests and left unchanged."""
    key = (kind, "" if KINDS[kind][0] is None else mode, norm, episodes, max_t)
    if key not in _runs:
        _runs[key] = evaluate(ea, kind, mode, norm=norm, episodes=episodes, max_t=max_t)
        run = _runs[key]
        assert run.calls == 1 and run.progress[:, 0].eq(episodes).all() and int(run.progress[:, 1].max()) <= episodes * max_t
        assert int(run.progress[:, 1].min()) < int(run.progress[:, 1].max())          # (the envs' episodes end at different frames)
    return _runs[key]


def episode_lengths(run):
    """[episodes, E]: the steps of each episode inside the evaluation -- the ``episode_length`` records, the first one less the
    clock the env started the evaluation with (make_env moves some clocks; an evaluator's reset leaves them at 0)."""
    lengths = run.records[..., 1].cpu().numpy().astype(np.int64)
    lengths[0] -= run.start["now"].cpu().numpy().astype(np.int64)
    assert (lengths >= 1).all() and (lengths.sum(0) == run.progress[:, 1].cpu().numpy()).all()
    return lengths


def replay(ea, kind, actions, max_t=MAX_T):
    """The plain rollout's trajectory of envs 0..K-1 under ``actions`` [T, E, 2], from the kind's start state."""
    import torch
    env = make_env(ea, kind, max_t)
    traj = env.rollout(int(actions.shape[0]), actions=actions, capture_envs=K)["trajectory"].clone()
    torch.cuda.synchronize()
    env.close()
    return traj


def assert_frames_are(run, traj, what, episodes=EPISODES):
    steps = run.progress[:, 1].cpu().numpy()
    for e in range(K):
        n = int(steps[e])
        assert n >= episodes and raw(run.frames[:n, e]).equal(raw(traj[:n, e])), (what, e)


CASES_6 = [(k, m, False) for k in NETWORKS for m in ("mean", "sample")] + [(k, "mean", True) for k in NETWORKS] + \
    [("scripted", "mean", False), ("linear_n64", "sample", True), ("transformer_n62", "mean", True)]


@pytest.mark.parametrize("kind,mode,norm", CASES_6)
def test_recording_changes_nothing(ea, kind, mode, norm):
    """6."""
    a, b = recorded(ea, kind, mode, norm), evaluate(ea, kind, mode, capture=False, norm=norm)
    assert raw(a.records).equal(raw(b.records)) and a.progress.equal(b.progress), (kind, mode, norm)
    for k in STATE:
        assert raw(a.state[k]).equal(raw(b.state[k])), (kind, mode, norm, k)
    for k in a.final:
        assert raw(a.final[k]).equal(raw(b.final[k])), (kind, mode, norm, k)


_replays = {}


def rollout_replay(ea, kind, sigma_zero, episodes=EPISODES, max_t=MAX_T):
    """policy_rollout's stored actions on a twin handle, replayed through the plain rollout's capture on a third."""
    import torch
    if (kind, sigma_zero, episodes, max_t) not in _replays:
        env = make_env(ea, kind, max_t)
        ro = env.policy_rollout(make_net(ea, kind, sigma_zero), episodes * max_t, env.observe().clone(), torch.zeros(E, dtype=torch.float32, device=env.device))
        actions = ro["actions"].clone()
        torch.cuda.synchronize()
        env.close()
        _replays[kind, sigma_zero, episodes, max_t] = replay(ea, kind, actions, max_t)
    return _replays[kind, sigma_zero, episodes, max_t]


def sample_mode_frames_are_the_plain_rollouts(ea, kind, episodes=EPISODES, max_t=MAX_T):
    """Test 7.  Returns the recorded run."""
    run = recorded(ea, kind, "sample", episodes=episodes, max_t=max_t)
    # all episode ends but the last inside every env's frames (two at three episodes)
    assert (episode_lengths(run)[:episodes - 1].sum(0) < run.progress[:, 1].cpu().numpy()).all()
    assert_frames_are(run, rollout_replay(ea, kind, False, episodes, max_t), kind, episodes)
    return run


@pytest.mark.parametrize("kind", [k for k in KINDS if KINDS[k][0] is not None])
def test_sample_mode_frames_are_the_plain_rollouts_under_the_policy_rollouts_actions(ea, kind):
    """7."""
    sample_mode_frames_are_the_plain_rollouts(ea, kind)


@pytest.mark.parametrize("kind", [k for k in KINDS if KINDS[k][0] is not None])
def test_mean_mode_frames_are_sample_mode_with_sigma_zero(ea, kind):
    """8."""
    zero, mean = recorded(ea, kind, "sample0"), recorded(ea, kind, "mean")
    assert_frames_are(zero, rollout_replay(ea, kind, True), kind)
    assert raw(mean.frames).equal(raw(zero.frames)) and raw(mean.starts).equal(raw(zero.starts)), kind
    assert not raw(mean.frames).equal(raw(recorded(ea, kind, "sample").frames)), kind       # (and sigma does move the leader)


def test_scripted_agent_frames_are_the_host_agents(ea):
    """9."""
    import torch
    run = recorded(ea, "scripted", "mean")
    _, N, cfg_kw, _ = KINDS["scripted"]
    area = types.SimpleNamespace(width=cfg_kw["width"], height=cfg_kw["height"], step_size=cfg_kw["step_size"],
                                 exit=types.SimpleNamespace(position=np.array([0, -1], dtype=np.float32)))
    fake = types.SimpleNamespace(area=area)
    frames, starts, lengths = run.frames.cpu().numpy(), run.starts.cpu().numpy(), episode_lengths(run)
    actions = np.zeros((FRAMES, E, 2), dtype=np.float32)
    actions[..., 1] = 1.0                                                       # (where no recorded step is replayed: straight up)
    phases = set()
    for e in range(K):
        f = 0
        for k in range(EPISODES):
            agent = ea.WacuumCleaner(fake)                                      # fresh at each episode start
            pos = starts[k, e, N, :2]
            for _ in range(int(lengths[k, e])):
                actions[f, e] = agent.act({"agent_position": pos})
                phases.add(agent.phase)
                pos = frames[f, e, N, :2]
                f += 1
        assert f == int(run.progress[e, 1])
    assert len(phases) >= 2
    assert_frames_are(run, replay(ea, "scripted", torch.from_numpy(actions).to(run.frames.device)), "scripted")


@pytest.mark.parametrize("kind,mode", [("linear", "mean"), ("transformer", "sample"), ("deepsets", "mean"), ("scripted", "mean"),
                                       ("linear_n64", "sample")])
def test_start_frames(ea, kind, mode):
    """10."""
    import torch
    run = recorded(ea, kind, mode)
    N = run.n_ped

    def assert_start(k, state):
        s = run.starts[k]
        assert raw(s[:, :N, :2]).equal(raw(state["pos"][:K])) and s[:, :N, 2].equal(state["status"][:K].float()), (kind, mode, k)
        assert raw(s[:, N, :2]).equal(raw(state["agent_pos"][:K])) and s[:, N, 2].eq(0).all(), (kind, mode, k)
    assert not torch.isnan(run.starts).any()
    assert_start(0, run.start)
    for k in (1, 2):
        assert_start(k, evaluate(ea, kind, mode, capture=False, episodes=k).final)      # (stops right after the reset into episode k)


@pytest.mark.parametrize("kind,mode,norm", CASES_6)
def test_terminal_frames_against_the_records(ea, kind, mode, norm):
    """11."""
    from evacuation_amd.vector_env import STATS_FIELDS
    run = recorded(ea, kind, mode, norm)
    N, lengths = run.n_ped, episode_lengths(run)
    rec = run.records.cpu().numpy()
    frames = run.frames.cpu().numpy()
    names = {1: "viscek_pedestrians", 2: "following_pedestrians", 3: "exiting_pedestrians", 4: "escaped_pedestrians"}
    for e in range(K):
        f = 0
        for k in range(EPISODES):
            f += int(lengths[k, e])
            status = frames[f - 1, e, :N, 2]
            assert frames[f - 1, e, N, 2] == 0.0
            for code, name in names.items():
                assert int((status == code).sum()) == int(rec[k, e, STATS_FIELDS.index(name)]), (kind, mode, e, k, name)


def resumption_and_bounds(ea, kind, mode, norm, episodes=EPISODES, max_t=MAX_T):
    """Test 12.  Returns the one-call run."""
    import torch
    one = recorded(ea, kind, mode, norm, episodes, max_t)
    many = evaluate(ea, kind, mode, norm=norm, max_steps=5, episodes=episodes, max_t=max_t)
    assert many.calls >= 6
    assert raw(many.frames).equal(raw(one.frames)) and raw(many.starts).equal(raw(one.starts)), (kind, mode)
    assert many.progress.equal(one.progress) and raw(many.records).equal(raw(one.records))
    steps = one.progress[:, 1].cpu().numpy()
    for e in range(K):
        n = int(steps[e])
        assert not torch.isnan(one.frames[:n, e]).any() and torch.isnan(one.frames[n:, e]).all(), (kind, mode, e)
    # max_frames = 7: the first 7 rows of a backing tensor of episodes x max_t (36)
    env = make_env(ea, kind, max_t)
    backing = nan_buffers(env, rows=episodes * max_t, episodes=episodes)
    env.close()
    short = evaluate(ea, kind, mode, norm=norm, buffers={"frames": backing["frames"][:7], "starts": backing["starts"]}, episodes=episodes,
                     max_t=max_t)
    assert torch.isnan(backing["frames"][7:]).all()
    assert raw(backing["frames"][:7]).equal(raw(one.frames[:7])) and raw(short.starts).equal(raw(one.starts)), (kind, mode)
    assert raw(short.records).equal(raw(one.records))
    return one


@pytest.mark.parametrize("kind,mode,norm", [("linear", "sample", False), ("deepsets", "mean", True), ("transformer_n62", "mean", True),
                                            ("scripted", "mean", False)])
def test_resumption_and_bounds(ea, kind, mode, norm):
    """12."""
    resumption_and_bounds(ea, kind, mode, norm)


def test_c_abi_refusals(ea):
    """13."""
    import torch
    from evacuation_amd import _lib
    for kind in NETWORKS:
        env = make_env(ea, kind)
        net = make_net(ea, kind)
        binder = env._binder()
        pol, enc = binder(net), binder.bind_encoder(net)
        entry = getattr(env.lib, "evac_policy_evaluate" + ("" if enc is None else enc[0]) + "_capture")
        prog = torch.zeros((E, 4), dtype=torch.int32, device=env.device)
        out = torch.zeros((EPISODES, E, 10), dtype=torch.float32, device=env.device)
        buf = nan_buffers(env)
        before = {k: getattr(env, k).clone() for k in STATE}
        good = dict(capture_envs=K, max_frames=FRAMES, frames=buf["frames"].data_ptr(), starts=buf["starts"].data_ptr())

        def call(agent=0, n_episodes=EPISODES, capture=good):
            cap = None if capture is None else C.byref(_lib.EvacEvalCapture(*[capture[f] for f, _ in _lib.EvacEvalCapture._fields_]))
            tail = (cap, None) if enc is None else (C.byref(enc[1]), cap, None)
            return entry(env._h, agent, C.byref(pol), n_episodes, 5, C.c_void_p(prog.data_ptr()), C.c_void_p(out.data_ptr()), None, 1.0, 1e-8,
                         *tail)
        refused = [dict(capture=None), dict(capture={**good, "capture_envs": 0}), dict(capture={**good, "capture_envs": E + 1}),
                   dict(capture={**good, "max_frames": 0}), dict(capture={**good, "frames": None}), dict(capture={**good, "starts": None}),
                   dict(agent=7), dict(n_episodes=0)]                                           # (the last two: the counterpart's own)
        for kw in refused:
            assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, (kind, kw)
        torch.cuda.synchronize()
        assert prog.eq(0).all() and out.eq(0).all() and torch.isnan(buf["frames"]).all() and torch.isnan(buf["starts"]).all(), kind
        for k in STATE:
            assert raw(getattr(env, k)).equal(raw(before[k])), (kind, k)
        assert call() == 0                                                                     # ... and the accepted call records
        torch.cuda.synchronize()
        assert prog[:, 1].eq(5).all() and not torch.isnan(buf["frames"][:5]).any() and torch.isnan(buf["frames"][5:]).all(), kind
        env.close()
    # the scripted agent goes through the linear entry; an encoder entry refuses it as its counterpart does
    env = make_env(ea, "scripted")
    prog = torch.zeros((E, 4), dtype=torch.int32, device=env.device)
    out = torch.zeros((1, E, 10), dtype=torch.float32, device=env.device)
    buf = nan_buffers(env, episodes=1)
    cap = _lib.EvacEvalCapture(K, FRAMES, buf["frames"].data_ptr(), buf["starts"].data_ptr())
    args = (1, 4, C.c_void_p(prog.data_ptr()), C.c_void_p(out.data_ptr()), None, 1.0, 1e-8)
    assert env.lib.evac_policy_evaluate_capture(env._h, 2, None, *args, None, None) == _lib.ERR_INVALID_ARGUMENT
    sets = _lib.EvacDeepSets(6, 24)
    assert env.lib.evac_policy_evaluate_deepsets_capture(env._h, 2, None, *args, C.byref(sets), C.byref(cap), None) == _lib.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert prog.eq(0).all() and torch.isnan(buf["frames"]).all()
    assert env.lib.evac_policy_evaluate_capture(env._h, 2, None, *args, C.byref(cap), None) == 0
    torch.cuda.synchronize()
    assert prog[:, 1].ge(1).all() and not torch.isnan(buf["starts"]).any() and not torch.isnan(buf["frames"][0]).any()
    env.close()


def test_python_faces(ea):
    """14."""
    import torch
    from evacuation_amd.policy import LinearActorCritic
    from evacuation_amd.trainer import RPOTrainer, RPOTrainingConfig
    cfg = ea.EnvConfig(number_of_pedestrians=10, max_timesteps=MAX_T, is_new_exiting_reward=True)
    ev = ea.PolicyEvaluator(cfg, ea.EnvWrappersConfig(**GRAV), num_envs=5, seed=SEED)
    res = ev.evaluate(make_net(ea, "linear"), 2, capture_envs=2)
    plain = ev.evaluate(make_net(ea, "linear"), 2)
    assert plain.capture is None and raw(plain.episodes["episode_reward"]).equal(raw(res.episodes["episode_reward"]))
    assert tuple(res.capture["frames"].shape) == (2 * MAX_T, 2, 11, 3) and tuple(res.capture["starts"].shape) == (2, 2, 11, 3)
    L = int(res.episodes["episode_length"][1, 1])
    ped, agent = res.episode_memory(1, 1)
    assert len(ped["positions"]) == len(ped["statuses"]) == L + 1 and len(agent["position"]) == L and 1 <= L <= MAX_T
    assert ped["positions"][0].tobytes() == res.capture["starts"][1, 1, :10, :2].cpu().numpy().astype(np.float64).tobytes()
    with pytest.raises(IndexError):
        res.episode_memory(2, 0)
    with pytest.raises(ValueError):
        ev.evaluate(make_net(ea, "linear"), 2, capture_envs=6)
    ev.close()
    # RPOTrainer.evaluate passes capture_envs through
    n = 8
    tcfg = RPOTrainingConfig(num_envs=n, num_steps=8, total_timesteps=n * 8, num_minibatches=2, update_epochs=1, seed=1)
    env = ea.NormalizedVectorEnv.make(cfg, ea.EnvWrappersConfig(**GRAV), num_envs=n, gamma=tcfg.gamma, seed=1)
    torch.manual_seed(0)
    tr = RPOTrainer(env, LinearActorCritic(env.obs_dim).to(env.env.device), tcfg)
    res = tr.evaluate(1, capture_envs=1)
    L = int(res.episodes["episode_length"][0, 0])
    ped, agent = res.episode_memory(0, 0)
    assert tuple(res.capture["frames"].shape) == (MAX_T, 1, 11, 3) and len(ped["positions"]) == L + 1 and len(agent["position"]) == L
    tr.evaluator.close()
    env.close()


def test_the_training_example_writes_the_episodes(ea, tmp_path):
    """14., examples/train_rpo.py --capture 2 --capture-out DIR in a fresh child process"""
    out = tmp_path / "episodes"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_rpo.py"), "--envs", "8", "--steps", "8", "--updates", "1", "--pedestrians", "10",
           "--minibatches", "2", "--epochs", "1", "--eval-episodes", "2", "--capture", "2", "--capture-out", str(out)]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert sorted(os.listdir(out)) == [f"env{e}_episode{k}.npz" for e in range(2) for k in range(2)]
    for name in os.listdir(out):
        f = np.load(out / name)
        L = f["agent_positions"].shape[0]
        assert L >= 1 and f["positions"].shape == (L + 1, 10, 2) and f["statuses"].shape == (L + 1, 10)
        assert f["positions"].dtype == np.float64 and f["agent_positions"].dtype == np.float32 and f["agent_positions"].shape == (L, 2)
        assert set(np.unique(f["statuses"])) <= {1, 2, 3, 4} and np.isfinite(f["positions"]).all()
