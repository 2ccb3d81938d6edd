"""A population of deep-sets leaders on an MI355X: S set-encoder learners in one set of launches, each BIT FOR BIT the learner it
would be alone (the lone entries are held to autograd and float64 by tests/test_gpu_deepsets*.py).

1. Collection: policy_rollout_population(DeepSetsPopulation) == S policy_rollout calls on handles of E_l envs with env_id_offset
   further by s E_l.
2. Update: evac_deepsets_update_population on one common batch == S deepsets_update calls on the learners' own rows.
3. target_kl: the learners stop at different epochs; a stopped learner's later rows are untouched while the others go on.
4. Determinism and graph capture.
5. Whole loop: PopulationTrainer == S RPOTrainer(grad_fn=deepsets_kernel_grad, optimizer="device") on twin handles; evaluate().
6. Refusals through the Python face.
7. The collection entry's own refusals through ctypes: code and text, nothing enqueued.

Equal means: the float32 / int64 / float64 words are compared as integers."""
import ctypes as C
import dataclasses
import time
from types import SimpleNamespace

import pytest

from tests import deepsets_grad_cases as DC
from tests.test_gpu_policy_rollout import OFFSET, SEED, base, i32, raw
from tests.test_gpu_population import (LOG_SCALARS, STORAGE_E, STORAGE_TE, interleave, same_number, same_records, snapshot,
                                       start_population)
from tests.trainer_cases import DEV, loss_cfg, same_bits

pytestmark = pytest.mark.gpu

CASES = {
    # name: (EnvConfig kwargs, EnvWrappersConfig kwargs, normalised chain)
    "n60_rel_ohe_box_norm_clip": (dict(number_of_pedestrians=60, max_timesteps=25, clip_action=True),
                                  dict(positions="rel", statuses="ohe", type="Box"), True),               # D = 372, ed = 6
    "n10_abs_cat_box_raw": (dict(number_of_pedestrians=10, max_timesteps=20, intrinsic_reward_coef=0.5),
                            dict(positions="abs", statuses="cat", type="Box"), False),                    # ed = 3, no chain
    "n64_rel_ohe_box_norm_clip": (dict(number_of_pedestrians=64, max_timesteps=25, clip_action=True),
                                  dict(positions="rel", statuses="ohe", type="Box"), True),               # D = 396: phase A's second pass
}


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import evacuation_amd
    from evacuation_amd import build
    build.build_library()
    return evacuation_amd


def make_env(ea, case, E, offset, **cfg_over):
    cfg_kw, wrap_kw, norm = CASES[case]
    env = ea.BatchedEvacuationEnv(ea.EnvConfig(**{**cfg_kw, **cfg_over}), ea.EnvWrappersConfig(**wrap_kw), num_envs=E, seed=SEED, env_id_offset=offset)
    return ea.NormalizedVectorEnv(env) if norm else env


def visible(pop):
    """Freshly seeded learners made visible as tests/test_gpu_deepsets.make_net does, each in its own way."""
    import torch
    N = pop.number_of_pedestrians
    with torch.no_grad():
        for s, net in enumerate(pop.nets):
            g = torch.Generator().manual_seed(1000 + s)
            net.actor_mean[4].weight.mul_(60.0)
            net.actor_logstd.copy_(torch.tensor([[-0.5 + 0.1 * s, 0.3 - 0.05 * s]]))
            for m in list(net.actor_mean) + list(net.critic):
                if isinstance(m, torch.nn.Linear):
                    m.bias.copy_((0.2 * torch.randn(m.bias.shape, generator=g)).to(DEV))
            net.deep_sets.transform_rho[0].weight.mul_(3.0 / (N + 2))
    return pop


def all_tensors(net):
    from evacuation_amd.policy import all_tensors as at
    return at(net)


# ------------------------------------------------------------------------------------------------ 1. collection
def collection_equals_standalone_rollouts(ea, case, S, E_l, T=30, **cfg_over):
    """Learner s's storage, norm_state, records and final state are those of policy_rollout(nets[s]) alone.  Returns the
    population call's storage."""
    import torch
    from evacuation_amd.population import DeepSetsPopulation
    pop_env = make_env(ea, case, S * E_l, OFFSET, **cfg_over)
    b = base(pop_env)
    pop = visible(DeepSetsPopulation(b.obs_dim, b.n_ped, [11 + 7 * s for s in range(S)], DEV))
    obs, done, now = start_population(pop_env)
    obs0 = obs.clone()
    norm0 = pop_env.norm_state.clone() if hasattr(pop_env, "norm_state") else None
    ro = pop_env.policy_rollout_population(pop, T, obs, done)
    assert ro["next_obs"] is obs and ro["next_done"] is done
    torch.cuda.synchronize()
    ended = int(ro["dones"][1:].sum()) + int(ro["next_done"].sum())
    assert ended >= (S * E_l) // 5 and ended >= 1                    # autoresets inside the call
    fin = snapshot(pop_env)
    for s in range(S):
        cols = slice(s * E_l, (s + 1) * E_l)
        env = make_env(ea, case, E_l, OFFSET + s * E_l, **cfg_over)
        o, _ = env.reset()
        assert i32(o).equal(i32(obs0[cols])), (case, s, "the reset observation")       # the same start state
        base(env).set_state(now=now[cols].clone())
        if norm0 is not None:
            assert raw(env.norm_state).equal(raw(norm0[cols])), (case, s, "norm_state after reset")
        d = torch.zeros(E_l, dtype=torch.float32, device=DEV)
        alone = env.policy_rollout(pop.nets[s], T, o.clone(), d)
        torch.cuda.synchronize()
        for k in STORAGE_TE:
            assert i32(ro[k][:, cols]).equal(i32(alone[k])), (case, S, E_l, s, k)
        for k in STORAGE_E:
            assert i32(ro[k][cols]).equal(i32(alone[k])), (case, S, E_l, s, k)
        mine = snapshot(env)
        for k in mine:
            assert raw(fin[k][cols]).equal(raw(mine[k])), (case, S, E_l, s, k)
        sa, sb = b.get_state(), base(env).get_state()
        for k in sa:
            assert sa[k][cols].contiguous().view(torch.uint8).equal(sb[k].contiguous().view(torch.uint8)), (case, s, k)
        env.close()
    if S > 1:                                                        # the learners did act differently
        assert not i32(ro["actions"][:, :E_l]).equal(i32(ro["actions"][:, E_l:2 * E_l]))
    pop_env.close()
    return ro


@pytest.mark.parametrize("case,S,E_l", [(c, S, E_l) for c in ("n60_rel_ohe_box_norm_clip", "n10_abs_cat_box_raw")
                                         for S, E_l in ((3, 3), (2, 40), (1, 17))] + [("n64_rel_ohe_box_norm_clip", 2, 5)])
def test_collection_equals_standalone_rollouts(ea, case, S, E_l):
    """(3, 3): thirteen of sixteen waves leave; (2, 40): three workgroups per learner, the last part-filled; (1, 17)."""
    collection_equals_standalone_rollouts(ea, case, S, E_l)


# ------------------------------------------------------------------------------------------------ 2. update
def random_batch(D, B, seed):
    """A learner's own batch of B rows: the oracle is the lone entry on the same rows, so any finite rows serve."""
    import torch
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    batch = {"b_obs": (0.6 * r(B, D)).clamp(-1, 1), "b_actions": r(B, 2), "b_logprobs": -2.0 + 0.3 * r(B), "b_advantages": r(B) + 0.3,
             "b_returns": r(B), "b_values": r(B)}
    return {k: v.to(DEV).contiguous() for k, v in batch.items()}


def learner_nets(N, ed, S, seed):
    """tests/deepsets_grad_cases.make_net per learner, each from its own seed and with its own sigmas."""
    import torch
    nets = []
    for s in range(S):
        net = DC.make_net(N, ed, seed=seed + s)
        with torch.no_grad():
            net.actor_logstd.copy_(torch.tensor([[-0.4 - 0.2 * s, 0.2 - 0.2 * s]]))
        nets.append(net)
    return nets


def load_population(N, ed, seeds, tensors):
    """A DeepSetsPopulation whose row s holds tensors[s] (19 tensors)."""
    import torch
    from evacuation_amd.population import DeepSetsPopulation
    pop = DeepSetsPopulation((N + 2) * ed, N, seeds, DEV)
    with torch.no_grad():
        for s, ts in enumerate(tensors):
            for p, q in zip(all_tensors(pop.nets[s]), ts):
                p.copy_(q)
    return pop


def fresh_learner(N, ed, start, lr):
    """A lone network holding `start` (19 tensors) and its DeviceAdam."""
    import torch
    from evacuation_amd import trainer
    net = DC.make_net(N, ed, seed=0)
    with torch.no_grad():
        for p, q in zip(all_tensors(net), start):
            p.copy_(q)
    return net, trainer.DeviceAdam(net, lr=lr)


def assert_learner_equals(pop, popt, s, net, opt, what):
    import torch
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(all_tensors(pop.nets[s]), all_tensors(net))):
        name = DC.NAMES[i]
        assert same_bits(p, q), (what, s, "param", name, float((p - q).abs().max()))
        assert same_bits(p.grad, q.grad), (what, s, "clipped grad", name)
        assert same_bits(popt.exp_avg[i][s], opt.exp_avg[i]), (what, s, "exp_avg", name)
        assert same_bits(popt.exp_avg_sq[i][s], opt.exp_avg_sq[i]), (what, s, "exp_avg_sq", name)
    assert same_bits(popt.headers[s], opt.header), (what, s, popt.learners[s].read_header(), opt.read_header())


def update_inputs(N, ed, S, B_l, n_epochs, seed):
    import torch
    D = (N + 2) * ed
    nets = learner_nets(N, ed, S, seed)
    batches = [random_batch(D, B_l, seed + 100 + s) for s in range(S)]
    gen = torch.Generator().manual_seed(seed + B_l)
    perms = torch.stack([torch.stack([torch.randperm(B_l, generator=gen) for _ in range(n_epochs)]) for _ in range(S)]).to(DEV)
    return D, nets, batches, perms


UPDATE_CASES = [  # N, ed, B_l, E_l, M, norm_adv
    (1, 2, 200, 4, 72, 1),          # minibatches of 72, 72 and a tail of 56: k_set_backward with P = 3 and a part-filled tile, 2 segments
    (10, 3, 200, 4, 72, 1),
    (64, 6, 200, 4, 72, 1),         # D = 396: the widest rho_w, more dynamic LDS than the default limit
    (10, 3, 8, 1, 8, 1),            # M = B_l = 8: one tile, one segment, one workgroup
    (10, 3, 200, 4, 72, 0),         # without norm_adv: six launches per step
    (10, 3, 200, 4, 72, -1),        # norm_adv, and the perturbation INJECTED: rpo_noise [S][steps][M][2], a learner's rows by its stride
]


@pytest.mark.parametrize("N,ed,B_l,E_l,M,norm_adv", UPDATE_CASES)
def test_update_equals_standalone_updates(ea, N, ed, B_l, E_l, M, norm_adv):
    import torch
    from evacuation_amd import population, trainer
    S, n_epochs, lr = 3, 2, 1e-3
    inject, norm_adv = norm_adv < 0, abs(norm_adv)
    cfg = loss_cfg(norm_adv, 1, 0.01, 0.5)
    seeds = [900 + 13 * s for s in range(S)]
    firsts = [1000 + 37 * s for s in range(S)]                      # every learner at a draw counter of its own
    D, nets, batches, perms = update_inputs(N, ed, S, B_l, n_epochs, seed=50 + N + B_l)
    common = interleave(batches, E_l)
    pop = load_population(N, ed, seeds, [all_tensors(n) for n in nets])
    popt = population.PopulationAdam(pop, lr=lr)
    assert len(popt.exp_avg) == 19 and popt.learners[0].deepsets
    steps = n_epochs * len(trainer.update_steps(B_l, M, bool(norm_adv)))
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_l, S)
    for s in range(S):                                               # the mapping: the learner's own row, in the common batch
        assert same_bits(common["b_obs"][rows[s, 0]], batches[s]["b_obs"][perms[s, 0]])
    stats = torch.full((S, steps, 8), -7.0, device=DEV)
    noise = None
    if inject:                                                       # (the tail step of 56 reads the first 56 of its M rows)
        gen = torch.Generator().manual_seed(N + M)
        noise = ((torch.rand(S, steps, M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV).contiguous()
    out, headers = population.deepsets_update_population(pop, common, rows, cfg, popt, minibatch_size=M, rpo_noise=noise, seeds=seeds,
                                                         first_draw_counters=firsts, stats=stats)
    assert out is stats and headers is popt.headers
    torch.cuda.synchronize()
    for s in range(S):
        opt = trainer.DeviceAdam(nets[s], lr=lr)
        alone = torch.full((steps, 8), -7.0, device=DEV)
        _, header = trainer.deepsets_update(nets[s], batches[s], perms[s].contiguous(), cfg, opt,
                                            rpo_noise=None if noise is None else noise[s], seed=seeds[s],
                                            first_draw_counter=firsts[s], stats=alone, minibatch_size=M)
        h = trainer.decode_header(header)
        assert (h["steps_run"], h["epochs_run"], h["stop"], h["t"]) == (steps, n_epochs, 0, steps), h
        assert_learner_equals(pop, popt, s, nets[s], opt, (N, ed, B_l, M))
        assert same_bits(stats[s], alone), (N, ed, B_l, M, s)
    assert not bool((stats == -7.0).any())
    assert not same_bits(stats[0], stats[1])


# ------------------------------------------------------------------------------------------------ 3. target_kl
def test_learners_stop_at_different_epochs(ea):
    """The threshold comes from the lone runs of the same inputs: between the calmest learner's largest closing approx_kl and what
    another learner exceeds before its last epoch (old log-probabilities that are the network's own under the zero perturbation,
    so approx_kl starts near zero and grows as the policy moves -- faster for a learner with a smaller sigma)."""
    import torch
    from evacuation_amd import population, trainer
    N, ed, B_l, E_l, M, n_epochs, lr, S = 10, 3, 144, 4, 72, 5, 1e-3, 3
    per_epoch = B_l // M
    steps = n_epochs * per_epoch
    cfg = loss_cfg(1, 1, 0.01, 0.0)
    seeds, firsts = [3, 4, 5], [0, 10, 20]
    D, nets, batches, perms = update_inputs(N, ed, S, B_l, n_epochs, seed=77)
    start = []
    for s, net in enumerate(nets):
        with torch.no_grad():
            net.actor_logstd.copy_(torch.tensor([[-0.4 - 0.7 * s, 0.2 - 0.7 * s]]))
            _, lp, _, _ = net.get_action_and_value(batches[s]["b_obs"], batches[s]["b_actions"])
            batches[s]["b_logprobs"] = lp.contiguous()
        start.append([p.detach().clone() for p in all_tensors(net)])

    def alone(s, stats):
        net, opt = fresh_learner(N, ed, start[s], lr)
        trainer.deepsets_update(net, batches[s], perms[s].contiguous(), cfg, opt, seed=seeds[s], first_draw_counter=firsts[s],
                                stats=stats, minibatch_size=M)
        torch.cuda.synchronize()
        return net, opt

    closing = []
    for s in range(S):
        stats = torch.zeros(steps, 8, device=DEV)
        alone(s, stats)
        closing.append([float(stats[(e + 1) * per_epoch - 1, 5]) for e in range(n_epochs)])
        print(f"\nlearner {s}: closing approx_kl per epoch:", " ".join(f"{x:.3e}" for x in closing[-1]))
    calm = min(range(S), key=lambda s: max(closing[s]))
    eager = max(range(S), key=lambda s: max(closing[s][:-1]))
    lo, hi = max(closing[calm]), max(closing[eager][:-1])
    assert lo < hi, closing                                          # (fails, not skips)
    cfg.target_kl = 0.5 * (lo + hi)
    pop = load_population(N, ed, seeds, start)
    popt = population.PopulationAdam(pop, lr=lr)
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_l, S)
    stats = torch.full((S, steps, 8), -7.0, device=DEV)
    population.deepsets_update_population(pop, interleave(batches, E_l), rows, cfg, popt, minibatch_size=M, seeds=seeds,
                                          first_draw_counters=firsts, stats=stats)
    torch.cuda.synchronize()
    epochs_run = []
    for s in range(S):
        mine = torch.full((steps, 8), -7.0, device=DEV)
        net, opt = alone(s, mine)
        h, hp = opt.read_header(), popt.learners[s].read_header()
        assert hp == h, (s, hp, h)
        assert_learner_equals(pop, popt, s, net, opt, "target_kl")
        assert same_bits(stats[s], mine), s
        ran = h["steps_run"]
        assert ran == h["epochs_run"] * per_epoch
        assert bool((stats[s, ran:] == -7.0).all()) and not bool((stats[s, :ran] == -7.0).any())      # rows beyond steps_run: untouched
        epochs_run.append(h["epochs_run"])
    print("epochs run with target_kl =", cfg.target_kl, ":", epochs_run)
    assert min(epochs_run) < n_epochs and max(epochs_run) == n_epochs, epochs_run
    assert epochs_run[calm] == n_epochs and epochs_run[eager] < n_epochs


# ------------------------------------------------------------------------------------------------ 4. determinism, capture
def test_two_calls_and_a_captured_replay_give_the_same_bits(ea):
    import torch
    from evacuation_amd import population, trainer
    N, ed, B_l, E_l, M, n_epochs, S = 10, 3, 100, 2, 40, 2, 3       # a tail of 20
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    seeds, firsts = [7, 8, 9], [5, 6, 7]
    D, nets, batches, perms = update_inputs(N, ed, S, B_l, n_epochs, seed=31)
    start = [[p.detach().clone() for p in all_tensors(n)] for n in nets]
    common = interleave(batches, E_l)
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_l, S)
    steps = n_epochs * len(trainer.update_steps(B_l, M, True))
    need = population.population_workspace_bytes(D, M, S, deepsets=True)

    def state_of(pop, popt, stats):
        torch.cuda.synchronize()
        return [t.clone() for t in pop.tensors + pop.grads + popt.exp_avg + popt.exp_avg_sq] + [popt.headers.clone(), stats.clone()]

    def run(capture):
        pop = load_population(N, ed, seeds, start)
        popt = population.PopulationAdam(pop, lr=1e-3)
        stats = torch.full((S, steps, 8), -7.0, device=DEV)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        call = lambda: population.deepsets_update_population(pop, common, rows, cfg, popt, minibatch_size=M, seeds=seeds,
                                                             first_draw_counters=firsts, stats=stats, workspace=ws)
        if not capture:
            call()
            return state_of(pop, popt, stats)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()                                   # one stream, no parallel branches
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                call()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert bool((stats == -7.0).all())                           # captured, not run
        g.replay()
        return state_of(pop, popt, stats)

    a, b, c = run(False), run(False), run(True)
    for i, (x, y, z) in enumerate(zip(a, b, c)):
        assert same_bits(x, y), ("two calls", i)
        assert same_bits(x, z), ("captured replay", i)
    assert not bool((a[-1] == -7.0).any())


# ------------------------------------------------------------------------------------------------ 5. the whole loop
def training_env(ea, E, offset, gamma):
    return ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=10, max_timesteps=40),
                                       ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box"), num_envs=E, gamma=gamma, seed=SEED,
                                       env_id_offset=offset)


def training_cfg(E_l, T, seed):
    from evacuation_amd.trainer import RPOTrainingConfig
    return RPOTrainingConfig(seed=seed, num_envs=E_l, num_steps=T, total_timesteps=E_l * T * 2, num_minibatches=2, update_epochs=2,
                             anneal_lr=True)


def test_population_trainer_equals_standalone_trainers(ea):
    import torch
    from evacuation_amd.policy import DeepSetsActorCritic
    from evacuation_amd.population import DeepSetsPopulation, PopulationTrainer
    from evacuation_amd.trainer import RPOTrainer, deepsets_kernel_grad
    S, E_l, T, seeds = 3, 4, 16, [11, 18, 25]
    cfg = training_cfg(E_l, T, 0)
    env = training_env(ea, S * E_l, OFFSET, cfg.gamma)
    ptr = PopulationTrainer(env, DeepSetsPopulation(env.obs_dim, 10, seeds, DEV), cfg)
    assert ptr.deepsets and not ptr.sweep
    alone = []
    for s in range(S):
        c = training_cfg(E_l, T, seeds[s])
        e = training_env(ea, E_l, OFFSET + s * E_l, c.gamma)
        torch.manual_seed(seeds[s])
        tr = RPOTrainer(e, DeepSetsActorCritic(e.obs_dim, 10).to(DEV), c, grad_fn=deepsets_kernel_grad, optimizer="device", one_call=True)
        obs, _ = e.reset()                                           # the handle's seed: _start would reseed the env with cfg.seed
        tr.next_obs, tr.next_done = obs.clone(), torch.zeros(E_l, dtype=torch.float32, device=DEV)
        tr.start_time = time.time()
        alone.append(tr)
    for u in range(2):
        logs = ptr.update()
        torch.cuda.synchronize()
        assert len(logs) == S
        for s, tr in enumerate(alone):
            log = tr.update()
            torch.cuda.synchronize()
            cols = slice(s * E_l, (s + 1) * E_l)
            for k in LOG_SCALARS:
                assert same_number(logs[s][k], log[k]), (u, s, k, logs[s][k], log[k])
            for k in log["episodes"]:
                assert same_records(logs[s]["episodes"][k], log["episodes"][k]), (u, s, k)
            for i, (p, q) in enumerate(zip(all_tensors(ptr.nets[s]), all_tensors(tr.net))):
                assert same_bits(p, q), (u, s, DC.NAMES[i])
                assert same_bits(ptr.optimizer.exp_avg[i][s], tr.optimizer.exp_avg[i]), (u, s, "exp_avg", DC.NAMES[i])
                assert same_bits(ptr.optimizer.exp_avg_sq[i][s], tr.optimizer.exp_avg_sq[i]), (u, s, "exp_avg_sq", DC.NAMES[i])
            assert raw(ptr.env.norm_state[cols]).equal(raw(tr.env.norm_state)), (u, s)
            assert ptr.minibatch_steps[s] == tr.minibatch_steps and same_bits(ptr.optimizer.headers[s], tr.optimizer.header)
    assert ptr.minibatch_steps == [2 * 2 * 2] * S
    assert not same_bits(ptr.population.tensors[17][0], ptr.population.tensors[17][1])       # (the learners are not copies)
    # evaluate(): per-learner results equal PolicyEvaluator on nets[s]
    results = ptr.evaluate(1)
    assert len(results) == S
    ev = ptr.make_evaluator()
    assert ev.num_envs == E_l
    for s in range(S):
        with torch.no_grad():
            one = ev.evaluate(ptr.nets[s], 1, norm_state=ptr.env.norm_state[s * E_l:(s + 1) * E_l].clone(), obs_clip=ptr.env.obs_clip,
                              epsilon=ptr.env.epsilon)
        for k in one.episodes:
            assert raw(one.episodes[k]).equal(raw(results[s].episodes[k])), (s, k)
        assert one.steps.equal(results[s].steps) and results[s].summary()["episodes"] == E_l
    ptr.evaluator.close()
    for tr in alone:
        tr.env.close()
    ptr.env.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_through_the_python_face(ea):
    import torch
    from evacuation_amd import population
    from evacuation_amd.policy import TransformerActorCritic
    from evacuation_amd.population import DeepSetsPopulation, PopulationAdam, PopulationTrainer
    env = make_env(ea, "n10_abs_cat_box_raw", 8, OFFSET)
    D = base(env).obs_dim
    obs, done, _ = start_population(env, near_trunc=0)
    three, two = DeepSetsPopulation(D, 10, [1, 2, 3], DEV), DeepSetsPopulation(D, 10, [1, 2], DEV)
    with pytest.raises(ValueError, match="equal shares"):           # envs that S does not divide
        env.policy_rollout_population(three, 4, obs, done)
    with pytest.raises(ValueError, match="sweeps of deep-sets learners are not built"):
        env.policy_rollout_population(two, 4, obs, done, gammas=[0.99, 0.9])
    cfg = training_cfg(4, 8, 0)
    with pytest.raises(ValueError, match="2 learners x cfg.num_envs"):
        PopulationTrainer(env, two, training_cfg(3, 8, 0))
    with pytest.raises(ValueError, match="sweeps of deep-sets learners are not built"):      # a list of differing configurations
        PopulationTrainer(env, two, [cfg, dataclasses.replace(cfg, learning_rate=1e-3)])
    batch = random_batch(D, 2 * 16, 5)
    rows = torch.arange(2 * 16, device=DEV).reshape(2, 1, 16).contiguous()
    with pytest.raises(ValueError, match="made for another population"):
        population.deepsets_update_population(two, batch, rows, loss_cfg(1, 1, 0.0, 0.5), PopulationAdam(three), minibatch_size=8)
    with pytest.raises(ValueError, match="sweeps of deep-sets learners are not built"):
        population.deepsets_update_population(two, batch, rows, [loss_cfg(1, 1, 0.0, 0.5)] * 2, PopulationAdam(two), minibatch_size=8)
    with pytest.raises(ValueError, match="deepsets_update_population"):
        population.rpo_update_population(two, batch, rows, loss_cfg(1, 1, 0.0, 0.5), PopulationAdam(two), minibatch_size=8)
    tf = TransformerActorCritic(D, 10).to(DEV)                       # a transformer stays refused everywhere
    for make in (lambda: population.PolicyPopulation(D, [1, 2], DEV, net=tf), lambda: PopulationTrainer(env, tf, cfg),
                 lambda: population.sweep_configs(cfg, {"learning_rate": [1e-3]}, net=tf),
                 lambda: env.policy_rollout_population(SimpleNamespace(num_learners=2, nets=[tf, tf]), 4, obs, done),
                 lambda: PopulationAdam(SimpleNamespace(num_learners=1, device=torch.device(DEV), tensors=[], nets=[tf]))):
        with pytest.raises(ValueError, match="attention encoder"):
            make()
    torch.cuda.synchronize()
    env.close()


# ------------------------------------------------------------------------------------------------ 7. the C entry's refusals
STRIDES_TEXT = ": an encoder stride is smaller than its tensor, or rho_w's is no multiple of 4 floats"


def collect(lib, h, a):
    """evac_policy_rollout_population_deepsets on handle `h` with the arguments `a` (Handle.valid, spoiled): its return code."""
    from tests.test_gpu_policy_refusals import BUFFERS
    ref = lambda s: None if s is None else C.byref(s)
    bufs = [a[k] for k in BUFFERS] + [a["final_stats"], a["norm_state"], 0.99, 1.0, 100.0, 1e-8]
    return lib.evac_policy_rollout_population_deepsets(h, a["n_learners"], ref(a["policy"]), ref(a["strides"]), ref(a["encoder"]),
                                                       ref(a["enc_strides"]), a["n_steps"], *bufs, None)


def test_collection_entry_refusals_have_their_code_and_text_and_enqueue_nothing(ea):
    """tests/test_gpu_policy_refusals.py's table for the new collection entry, through ctypes on reset handles: the return code and
    the text of evac_last_error of every case, as literals.  A refused call enqueues nothing: nothing is launched here but
    `reset`, and every handle's state is bit-equal before and after the table.  Box rel + ohe at E = 4, N = 3 (D = 30, six floats
    an element), and E = 1, N = 65 (more than one wave).  What one learner cannot break -- its strides are never applied -- is
    accepted at S = 1: such a call is shown to pass the strides' check by the refusal that comes behind it (the alignment of
    actions_out), which two learners with the same strides do not reach."""
    import torch
    from evacuation_amd import _lib
    from tests.test_gpu_policy_refusals import BAD, ENCODER_BUFFERS_TEXT, LEARNERS_TEXT, ROOMS_TEXT, UNSUPPORTED, Handle, changed
    name = "evac_policy_rollout_population_deepsets"
    box_wrap = dict(positions="rel", statuses="ohe", type="Box")
    box, big = Handle(ea, 3, box_wrap, 4, 6), Handle(ea, 65, box_wrap, 1, 6)
    D, ed = 30, 6
    assert box.env.obs_dim == D
    least = dict(phi_w1=24 * ed, phi_b1=24, phi_w2=24 * 24, phi_b2=24, rho_w=D * 24, rho_b=D)
    fields = [f for f, _ in _lib.EvacDeepSetsStrides._fields_]
    assert fields == list(least)
    for hd in (box, big):
        hd.valid["enc_strides"] = _lib.EvacDeepSetsStrides(*least.values())
    zero = _lib.EvacDeepSetsStrides(0, 0, 0, 0, 2, 0)                # every stride 0, rho_w's neither a tensor nor a multiple of 4
    misaligned = lambda v: v["actions_out"] + 4
    ALIGN_TEXT = ": actions_out must be 8-byte aligned"
    rows = [  # (what, handle, the changes, code, the text after the entry's name)
        ("strides NULL", box, lambda v: dict(strides=None), BAD, ": strides / enc_strides is NULL"),
        ("enc_strides NULL", box, lambda v: dict(enc_strides=None), BAD, ": strides / enc_strides is NULL"),
        ("enc_strides NULL, one learner", box, lambda v: dict(enc_strides=None, n_learners=1), BAD, ": strides / enc_strides is NULL"),
        ("n_learners = 0", box, lambda v: dict(n_learners=0), BAD, LEARNERS_TEXT),
        ("n_learners = EVAC_MAX_LEARNERS + 1", box, lambda v: dict(n_learners=65), BAD, LEARNERS_TEXT),
        ("3 learners on 4 envs", box, lambda v: dict(n_learners=3), BAD, ": the handle's 4 envs are not 3 learners' equal shares"),
        ("a policy stride smaller than the tensor, 2 learners", box, lambda v: dict(strides=changed(v["strides"], "critic_b3", 0)), BAD,
         ": a learner stride is smaller than its tensor"),
        ("rho_w stride + 2", box, lambda v: dict(enc_strides=changed(v["enc_strides"], "rho_w", least["rho_w"] + 2)), BAD, STRIDES_TEXT),
        ("every encoder stride 0, 2 learners, actions_out + 4 bytes", box, lambda v: dict(enc_strides=zero, actions_out=misaligned(v)),
         BAD, STRIDES_TEXT),
        # ... and the same strides with ONE learner are accepted: the call gets to the check behind them
        ("every encoder stride 0, 1 learner, actions_out + 4 bytes", box,
         lambda v: dict(enc_strides=zero, n_learners=1, actions_out=misaligned(v)), BAD, ALIGN_TEXT),
        ("every policy stride 0 too, 1 learner, actions_out + 4 bytes", box,
         lambda v: dict(enc_strides=zero, strides=_lib.EvacMlpPolicyStrides(), n_learners=1, actions_out=misaligned(v)), BAD, ALIGN_TEXT),
        # what both siblings refuse, in their order
        ("n_steps = 0", box, lambda v: dict(n_steps=0), BAD, ": n_steps must be >= 1"),
        ("reward_out NULL", box, lambda v: dict(reward_out=None), BAD, ENCODER_BUFFERS_TEXT),
        ("policy NULL", box, lambda v: dict(policy=None), BAD, ": policy is NULL"),
        ("encoder NULL", box, lambda v: dict(encoder=None), BAD, ": encoder is NULL"),
        ("encoder.rho_b NULL", box, lambda v: dict(encoder=changed(v["encoder"], "rho_b", None)), BAD,
         ": a tensor pointer of the encoder is NULL"),
        ("set_elem_dim = 5", box, lambda v: dict(encoder=changed(v["encoder"], "set_elem_dim", 5)), BAD,
         ": set_elem_dim 5 x (3 + 2) elements is not the observation's 30 floats (a Box observation is needed)"),
        ("rho_w + 4 bytes", box, lambda v: dict(encoder=changed(v["encoder"], "rho_w", v["encoder"].rho_w + 4)), BAD,
         ": rho_w must be 16-byte aligned"),
        ("actions_out + 4 bytes", box, lambda v: dict(actions_out=misaligned(v)), BAD, ALIGN_TEXT),
        ("N = 65", big, lambda v: {}, UNSUPPORTED, ROOMS_TEXT),
        ("N = 65 and enc_strides NULL", big, lambda v: dict(enc_strides=None), BAD, ": strides / enc_strides is NULL"),
    ]
    for f in fields:                                                 # each of the six, one below its tensor and 0, with 2 learners
        for value in (least[f] - 1, 0):
            rows.append((f"encoder stride {f} = {value}, 2 learners", box,
                         lambda v, f=f, value=value: dict(enc_strides=changed(v["enc_strides"], f, value)), BAD, STRIDES_TEXT))
    torch.cuda.synchronize()
    before = {id(hd): hd.snapshot() for hd in (box, big)}
    lib = box.env.lib
    for what, hd, spoil, code, text in rows:
        args = {**hd.valid, **spoil(hd.valid)}
        rc = collect(lib, hd.env._h, args)
        got = (lib.evac_last_error(hd.env._h) or b"").decode()
        assert rc != 0, what                                          # (a call that went through: stop before anything else is tried)
        assert (rc, got) == (code, name + text), what
    assert len(rows) == 21 + 12
    torch.cuda.synchronize()
    for hd in (box, big):
        for k, t in hd.snapshot().items():
            assert torch.equal(t, before[id(hd)][k]), k
        hd.env.close()
