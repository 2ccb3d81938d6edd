"""The update of a population of transformer leaders on an MI355X: S attention-encoder learners in one set of launches
(evac_transformer_update_population), each BIT FOR BIT the learner it would be alone (trainer.transformer_update, which
tests/test_gpu_transformer_update.py holds to the host loop and tests/test_gpu_transformer_grad.py to float64).

1. Update: one call on one common batch == S transformer_update calls on the learners' own rows, inside a workspace of exactly
   the sizer's bytes between canaries.
2. target_kl: the learners stop at different epochs; a stopped learner's later rows are untouched while the others go on.
3. Determinism and graph capture.
4. TransformerAdam(storage=): the state in the caller's tensors, between canaries.
5. Whole loop: PopulationTrainer(optimizer="device_transformer") == S RPOTrainer(grad_fn=transformer_kernel_grad,
   optimizer="device_transformer") on twin handles; evaluate(); state_dict(s).
6. examples/train_rpo.py --network transformer --gradient device --optimizer device --seeds.

Equal means: the float32 / int64 / float64 words are compared as integers."""
import os
import re
import subprocess
import sys
import time

import pytest

from tests import transformer_grad_cases as TC
from tests.test_gpu_policy_rollout import OFFSET, SEED, raw
from tests.test_gpu_population import LOG_SCALARS, interleave, same_number, same_records
from tests.trainer_cases import DEV, loss_cfg, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import evacuation_amd
    from evacuation_amd import build
    build.build_library()
    return evacuation_amd


def all_tensors(net):
    from evacuation_amd.policy import all_tensors as at
    return at(net)


def random_batch(D, B, seed):
    """A learner's own batch of B rows: the oracle is the lone entry on the same rows, so any finite rows serve."""
    import torch
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    batch = {"b_obs": (0.6 * r(B, D)).clamp(-1, 1), "b_actions": r(B, 2), "b_logprobs": -2.0 + 0.3 * r(B), "b_advantages": r(B) + 0.3,
             "b_returns": r(B), "b_values": r(B)}
    return {k: v.to(DEV).contiguous() for k, v in batch.items()}


def learner_nets(shape, S, seed):
    """tests/transformer_grad_cases.make_net per learner, each from its own seed and with its own sigmas."""
    import torch
    nets = []
    for s in range(S):
        net = TC.make_net(*shape, seed=seed + s)
        with torch.no_grad():
            net.actor_logstd.copy_(torch.tensor([[-0.4 - 0.2 * s, 0.2 - 0.2 * s]]))
        nets.append(net)
    return nets


def load_population(shape, seeds, tensors):
    """A TransformerPopulation whose row s holds tensors[s] (13 + 16 per block tensors)."""
    import torch
    from evacuation_amd.population import TransformerPopulation
    N, dm, blocks, resid = shape
    pop = TransformerPopulation((N + 2) * dm, N, seeds, DEV, num_blocks=blocks, use_resid=resid)
    assert len(pop.tensors) == 13 + 16 * blocks
    with torch.no_grad():
        for s, ts in enumerate(tensors):
            for p, q in zip(all_tensors(pop.nets[s]), ts):
                p.copy_(q)
    return pop


def fresh_learner(shape, start, lr):
    """A lone network holding `start` and its TransformerAdam."""
    import torch
    from evacuation_amd import trainer
    net = TC.make_net(*shape, seed=0)
    with torch.no_grad():
        for p, q in zip(all_tensors(net), start):
            p.copy_(q)
    return net, trainer.TransformerAdam(net, lr=lr)


def assert_learner_equals(pop, popt, s, net, opt, what):
    import torch
    torch.cuda.synchronize()
    names = TC.names(pop.num_blocks)
    mine, lone = all_tensors(pop.nets[s]), all_tensors(net)
    assert len(mine) == len(lone) == len(names) == len(popt.exp_avg)
    for i, (p, q) in enumerate(zip(mine, lone)):
        assert same_bits(p, q), (what, s, "param", names[i], float((p - q).abs().max()))
        assert same_bits(p.grad, q.grad), (what, s, "clipped grad", names[i])
        assert same_bits(popt.exp_avg[i][s], opt.exp_avg[i]), (what, s, "exp_avg", names[i])
        assert same_bits(popt.exp_avg_sq[i][s], opt.exp_avg_sq[i]), (what, s, "exp_avg_sq", names[i])
    assert same_bits(popt.headers[s], opt.header), (what, s, popt.learners[s].read_header(), opt.read_header())


def update_inputs(shape, S, B_l, n_epochs, seed):
    import torch
    D = (shape[0] + 2) * shape[1]
    nets = learner_nets(shape, S, seed)
    batches = [random_batch(D, B_l, seed + 100 + s) for s in range(S)]
    gen = torch.Generator().manual_seed(seed + B_l)
    perms = torch.stack([torch.stack([torch.randperm(B_l, generator=gen) for _ in range(n_epochs)]) for _ in range(S)]).to(DEV)
    return D, nets, batches, perms


def learner_index(S):
    import torch
    return torch.arange(S, device=DEV).reshape(S, 1, 1)


# ------------------------------------------------------------------------------------------------ 1. update
UPDATE_CASES = [  # N, dm, blocks, resid, B_l, E_l, M, norm_adv
    (1, 2, 1, False, 200, 4, 70, 1),    # 3 tokens; steps of 70, 70 and a tail of 60: k_tf_backward with P = 3 and an uneven last chunk, a
                                        # part-filled k_tf_dy tile; blocks[1] NULL in every struct and its strides -5
    (10, 3, 2, False, 200, 4, 70, 1),   # two blocks
    (62, 6, 2, True, 200, 4, 70, 1),    # 64 tokens; D = 384: more dynamic LDS in k_population_grad than the default limit
    (10, 3, 2, True, 8, 1, 8, 1),       # M = B_l = 8: one tile, one part, one workgroup
    (10, 3, 2, False, 200, 4, 70, 0),   # without norm_adv
    (10, 3, 2, False, 200, 4, 70, -1),  # norm_adv, and the perturbation INJECTED: rpo_noise [S][steps][M][2], a learner's rows by its stride
]


@pytest.mark.parametrize("N,dm,blocks,resid,B_l,E_l,M,norm_adv", UPDATE_CASES)
def test_update_equals_standalone_updates(ea, N, dm, blocks, resid, B_l, E_l, M, norm_adv):
    import torch
    from evacuation_amd import population, trainer
    S, n_epochs, lr = 3, 2, 1e-3
    shape = (N, dm, blocks, resid)
    inject, norm_adv = norm_adv < 0, abs(norm_adv)
    cfg = loss_cfg(norm_adv, 1, 0.01, 0.5)
    seeds = [900 + 13 * s for s in range(S)]
    firsts = [1000 + 37 * s for s in range(S)]                      # every learner at a draw counter of its own
    D, nets, batches, perms = update_inputs(shape, S, B_l, n_epochs, seed=50 + N + B_l)
    common = interleave(batches, E_l)
    pop = load_population(shape, seeds, [all_tensors(n) for n in nets])
    popt = population.TransformerPopulationAdam(pop, lr=lr)
    assert len(popt.exp_avg) == 13 + 16 * blocks and isinstance(popt.learners[0], trainer.TransformerAdam)
    assert popt.encoder_moment_strides is pop.encoder_strides
    if blocks == 1:                                                  # a block not in use: NULL everywhere, its strides never looked at
        for st in (pop.encoder_struct(), popt.learners[0].state_struct().enc_exp_avg, popt.learners[0].state_struct().enc_exp_avg_sq):
            assert all(getattr(st.blocks[1], f) is None for f in TC.BLOCK_NAMES) and st.blocks[0].wq
        for f in TC.BLOCK_NAMES:
            setattr(pop.encoder_strides.blocks[1], f, -5)
    steps = n_epochs * len(trainer.update_steps(B_l, M, bool(norm_adv)))
    rows = population.population_rows(perms, learner_index(S), E_l, S)
    for s in range(S):                                               # the mapping: the learner's own row, in the common batch
        assert same_bits(common["b_obs"][rows[s, 0]], batches[s]["b_obs"][perms[s, 0]])
    stats = torch.full((S, steps, 8), -7.0, device=DEV)
    noise = None
    if inject:                                                       # (the tail step of 60 reads the first 60 of its M rows)
        gen = torch.Generator().manual_seed(N + M)
        noise = ((torch.rand(S, steps, M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV).contiguous()
    # the workspace: a window of exactly `need` bytes, 16-byte aligned, inside a larger buffer of canaries
    need = population.population_workspace_bytes(D, min(M, B_l), S, transformer=True)
    lead = 272
    buffer = torch.full((lead + need + 4096,), CANARY, dtype=torch.uint8, device=DEV)
    window = buffer[lead:lead + need]
    assert window.data_ptr() % 16 == 0 and window.numel() == need
    out, headers = population.transformer_update_population(pop, common, rows, cfg, popt, minibatch_size=M, rpo_noise=noise, seeds=seeds,
                                                            first_draw_counters=firsts, stats=stats, workspace=window)
    assert out is stats and headers is popt.headers
    torch.cuda.synchronize()
    assert bool((buffer[:lead] == CANARY).all()) and bool((buffer[lead + need:] == CANARY).all()), "the workspace's canaries"
    for s in range(S):
        opt = trainer.TransformerAdam(nets[s], lr=lr)
        alone = torch.full((steps, 8), -7.0, device=DEV)
        _, header = trainer.transformer_update(nets[s], batches[s], perms[s].contiguous(), cfg, opt,
                                               rpo_noise=None if noise is None else noise[s], seed=seeds[s],
                                               first_draw_counter=firsts[s], stats=alone, minibatch_size=M)
        h = trainer.decode_header(header)
        assert (h["steps_run"], h["epochs_run"], h["stop"], h["t"]) == (steps, n_epochs, 0, steps), h
        assert_learner_equals(pop, popt, s, nets[s], opt, shape + (B_l, M))
        assert same_bits(stats[s], alone), (shape, B_l, M, s)
    assert not bool((stats == -7.0).any())
    assert not same_bits(stats[0], stats[1])                         # the learners differ from one another
    assert not same_bits(pop.tensors[13][0], pop.tensors[13][1])


# ------------------------------------------------------------------------------------------------ 2. target_kl
def test_learners_stop_at_different_epochs(ea):
    """The threshold comes from the lone runs of the same inputs: the midpoint between the calmest learner's largest closing
    approx_kl and what an eager learner exceeds before its last epoch (old log-probabilities that are the network's own under the
    zero perturbation, so approx_kl starts near zero and grows as the policy moves -- faster for a learner with a smaller sigma)."""
    import torch
    from evacuation_amd import population, trainer
    shape, B_l, E_l, M, n_epochs, lr, S = (10, 3, 2, False), 144, 4, 72, 5, 1e-3, 3
    per_epoch = B_l // M
    steps = n_epochs * per_epoch
    cfg = loss_cfg(1, 1, 0.01, 0.0)
    seeds, firsts = [3, 4, 5], [0, 10, 20]
    D, nets, batches, perms = update_inputs(shape, S, B_l, n_epochs, seed=77)
    start = []
    for s, net in enumerate(nets):
        with torch.no_grad():
            net.actor_logstd.copy_(torch.tensor([[-0.4 - 0.7 * s, 0.2 - 0.7 * s]]))
            _, lp, _, _ = net.get_action_and_value(batches[s]["b_obs"], batches[s]["b_actions"])
            batches[s]["b_logprobs"] = lp.contiguous()
        start.append([p.detach().clone() for p in all_tensors(net)])

    def alone(s, stats):
        net, opt = fresh_learner(shape, start[s], lr)
        trainer.transformer_update(net, batches[s], perms[s].contiguous(), cfg, opt, seed=seeds[s], first_draw_counter=firsts[s],
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
    pop = load_population(shape, seeds, start)
    popt = population.TransformerPopulationAdam(pop, lr=lr)
    rows = population.population_rows(perms, learner_index(S), E_l, S)
    stats = torch.full((S, steps, 8), -7.0, device=DEV)
    population.transformer_update_population(pop, interleave(batches, E_l), rows, cfg, popt, minibatch_size=M, seeds=seeds,
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


# ------------------------------------------------------------------------------------------------ 3. determinism, capture
def test_two_calls_and_a_captured_replay_give_the_same_bits(ea):
    import torch
    from evacuation_amd import population, trainer
    shape, B_l, E_l, M, n_epochs, S = (10, 3, 2, True), 100, 2, 40, 2, 3       # a tail of 20
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    seeds, firsts = [7, 8, 9], [5, 6, 7]
    D, nets, batches, perms = update_inputs(shape, S, B_l, n_epochs, seed=31)
    start = [[p.detach().clone() for p in all_tensors(n)] for n in nets]
    common = interleave(batches, E_l)
    rows = population.population_rows(perms, learner_index(S), E_l, S)
    steps = n_epochs * len(trainer.update_steps(B_l, M, True))
    need = population.population_workspace_bytes(D, M, S, transformer=True)

    def state_of(pop, popt, stats):
        torch.cuda.synchronize()
        return [t.clone() for t in pop.tensors + pop.grads + popt.exp_avg + popt.exp_avg_sq] + [popt.headers.clone(), stats.clone()]

    def run(capture):
        pop = load_population(shape, seeds, start)
        popt = population.TransformerPopulationAdam(pop, lr=1e-3)
        stats = torch.full((S, steps, 8), -7.0, device=DEV)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        call = lambda: population.transformer_update_population(pop, common, rows, cfg, popt, minibatch_size=M, seeds=seeds,
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


# ------------------------------------------------------------------------------------------------ 4. the optimiser's storage
def test_transformer_adam_keeps_its_state_in_the_callers_storage(ea):
    """TransformerAdam(storage=): header and moments carved out of one buffer each with canaries between them; one
    transformer_minibatch_step equals the step of an optimiser that owns its state, and the canaries are untouched."""
    import torch
    from evacuation_amd import trainer
    shape, M = (10, 3, 2, False), 37
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    net_a, net_b = TC.make_net(*shape, seed=5), TC.make_net(*shape, seed=5)
    D = (shape[0] + 2) * shape[1]
    batch = random_batch(D, 2 * M + 3, 9)
    g = torch.Generator().manual_seed(M)
    inds = torch.randint(0, 2 * M + 3, (M,), generator=g).to(DEV)
    z = ((torch.rand(M, 2, generator=g) * 2 - 1) * cfg.rpo_alpha).to(DEV).contiguous()
    params = all_tensors(net_b)
    gap = 8                                                          # floats of canary between (and around) the tensors
    total = gap + sum(p.numel() + gap for p in params)
    flat = [torch.full((total,), float("nan"), device=DEV) for _ in range(2)]
    headers = torch.full((3, 8), -1, dtype=torch.int64, device=DEV)
    headers[1].zero_()                                               # (all zero: a fresh optimiser)
    moments, used = [[], []], torch.zeros(total, dtype=torch.bool, device=DEV)
    at = gap
    for p in params:
        for k in range(2):
            view = flat[k][at:at + p.numel()].view(p.shape)
            view.zero_()
            moments[k].append(view)
        used[at:at + p.numel()] = True
        at += p.numel() + gap
    opt_a = trainer.TransformerAdam(net_a, lr=1e-3)
    opt_b = trainer.TransformerAdam(net_b, lr=1e-3, storage=(headers[1], moments[0], moments[1]))
    assert opt_b.header.data_ptr() == headers[1].data_ptr() and opt_b.exp_avg[20].data_ptr() == moments[0][20].data_ptr()
    for k in range(2):                                               # the second step from non-zero moments
        stats_a = trainer.transformer_minibatch_step(net_a, batch, inds, cfg, opt_a, rpo_noise=z)
        stats_b = trainer.transformer_minibatch_step(net_b, batch, inds, cfg, opt_b, rpo_noise=z)
        torch.cuda.synchronize()
        assert same_bits(stats_a, stats_b)
        for i, (p, q) in enumerate(zip(all_tensors(net_a), all_tensors(net_b))):
            assert same_bits(p, q), (k, i)
            assert same_bits(opt_a.exp_avg[i], moments[0][i]) and same_bits(opt_a.exp_avg_sq[i], moments[1][i]), (k, i)
        assert same_bits(opt_a.header, headers[1]) and opt_b.read_header()["t"] == k + 1
    assert bool((moments[1][13] != 0).any())                         # (the state did move)
    for k in range(2):
        assert bool(torch.isnan(flat[k][~used]).all()), "a canary between the moments"
    assert bool((headers[0] == -1).all()) and bool((headers[2] == -1).all()), "the canaries around the header"


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
    from evacuation_amd.policy import TransformerActorCritic
    from evacuation_amd.population import PopulationTrainer, TransformerPopulation, TransformerPopulationAdam
    from evacuation_amd.trainer import RPOTrainer, transformer_kernel_grad
    S, E_l, T, seeds = 3, 4, 16, [11, 18, 25]
    cfg = training_cfg(E_l, T, 0)
    env = training_env(ea, S * E_l, OFFSET, cfg.gamma)
    ptr = PopulationTrainer(env, TransformerPopulation(env.obs_dim, 10, seeds, DEV), cfg, optimizer="device_transformer")
    assert ptr.transformer and not ptr.deepsets and not ptr.sweep and isinstance(ptr.optimizer, TransformerPopulationAdam)
    names = TC.names(2)
    alone = []
    for s in range(S):
        c = training_cfg(E_l, T, seeds[s])
        e = training_env(ea, E_l, OFFSET + s * E_l, c.gamma)
        torch.manual_seed(seeds[s])
        tr = RPOTrainer(e, TransformerActorCritic(e.obs_dim, 10).to(DEV), c, grad_fn=transformer_kernel_grad,
                        optimizer="device_transformer", one_call=True)
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
                assert same_bits(p, q), (u, s, names[i])
                assert same_bits(ptr.optimizer.exp_avg[i][s], tr.optimizer.exp_avg[i]), (u, s, "exp_avg", names[i])
                assert same_bits(ptr.optimizer.exp_avg_sq[i][s], tr.optimizer.exp_avg_sq[i]), (u, s, "exp_avg_sq", names[i])
            assert raw(ptr.env.norm_state[cols]).equal(raw(tr.env.norm_state)), (u, s)
            assert ptr.minibatch_steps[s] == tr.minibatch_steps and same_bits(ptr.optimizer.headers[s], tr.optimizer.header)
    assert ptr.minibatch_steps == [2 * 2 * 2] * S
    assert logs[0]["learning_rate"] == 0.5 * cfg.learning_rate      # (annealed)
    assert not same_bits(ptr.population.tensors[13][0], ptr.population.tensors[13][1])       # (the learners are not copies)
    # evaluate(): S results, per learner PolicyEvaluator's on nets[s]
    results = ptr.evaluate(1)
    assert len(results) == S
    ev = ptr.make_evaluator()
    for s in range(S):
        with torch.no_grad():
            one = ev.evaluate(ptr.nets[s], 1, norm_state=ptr.env.norm_state[s * E_l:(s + 1) * E_l].clone(), obs_clip=ptr.env.obs_clip,
                              epsilon=ptr.env.epsilon)
        for k in one.episodes:
            assert raw(one.episodes[k]).equal(raw(results[s].episodes[k])), (s, k)
        assert results[s].summary()["episodes"] == E_l
    # state_dict(s) round-trips and touches no other learner
    opt = ptr.optimizer
    before = [t.clone() for t in opt.exp_avg + opt.exp_avg_sq] + [opt.headers.clone()]
    sd = opt.state_dict(1)
    assert len(sd["state"]) == 45 and float(sd["state"][44]["step"]) == 8.0
    with torch.no_grad():
        for m in opt.exp_avg + opt.exp_avg_sq:
            m[1].zero_()
        opt.headers[1].zero_()
    opt.load_state_dict(1, sd)
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(before[:-1], opt.exp_avg + opt.exp_avg_sq)):
        assert same_bits(x, y), ("state_dict round trip", i)
    # the header: t, P1, P2 are the state (what the last update ran -- steps_run, epochs_run -- is not, and reads 0 once loaded)
    assert same_bits(before[-1][1, :3], opt.headers[1, :3]) and not bool(opt.headers[1, 3:].any())
    assert same_bits(before[-1][0], opt.headers[0]) and same_bits(before[-1][2], opt.headers[2])
    ptr.evaluator.close()
    for tr in alone:
        tr.env.close()
    ptr.env.close()


# ------------------------------------------------------------------------------------------------ 6. the example
def test_train_rpo_example_trains_a_transformer_population(ea):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_rpo.py"), "--network", "transformer", "--gradient", "device", "--optimizer",
           "device", "--seeds", "1,2", "--envs", "4", "--steps", "16", "--updates", "2", "--pedestrians", "10", "--minibatches", "2",
           "--epochs", "2"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    lines = re.findall(r"^seed (\d+)\s+update\s+(\d+)", done.stdout, re.M)
    assert lines == [("1", "1"), ("2", "1"), ("1", "2"), ("2", "2")], done.stdout[-2000:]       # one line per learner and update
    assert done.stdout.count("SPS:") == 4
