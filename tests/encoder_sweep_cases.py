"""What tests/test_gpu_deepsets_sweep.py and tests/test_gpu_transformer_sweep.py share: the checks of a SWEEP of an encoder
population (evac_policy_rollout_sweep_*, evac_*_update_sweep, PopulationTrainer(encoder_sweep=True)), written once over a
description of the encoder (``Enc``).  Learner s is held, bit for bit, to the lone entries of this project with its own values
(``policy_rollout`` on a handle wrapped with its gamma, ``deepsets_update`` / ``transformer_update`` with its configuration and a
lone optimiser at its lr / max_grad_norm), which other test files hold to autograd and float64.  Equal means: the words are
compared as integers.  No tolerance anywhere."""
import dataclasses
import struct
import time

import pytest

from tests.test_gpu_policy_rollout import OFFSET, SEED, base, i32, raw
from tests.test_gpu_population import (LOG_SCALARS, STORAGE_E, STORAGE_TE, interleave, same_number, same_records, snapshot,
                                       start_population)
from tests.test_gpu_sweep import learner_cfg
from tests.trainer_cases import DEV, loss_cfg, same_bits
from tests.workspace_guard import WorkspaceGuard

NORM_CASE = (dict(number_of_pedestrians=60, max_timesteps=25, clip_action=True), dict(positions="rel", statuses="ohe", type="Box"))
RAW_CASE = (dict(number_of_pedestrians=10, max_timesteps=20, intrinsic_reward_coef=0.5), dict(positions="abs", statuses="cat", type="Box"))
GAMMAS = [0.99, 0.9, 0.999]
TABLE_BYTES = 1288                              # evac::LearnerSteps: 64 doubles, 64 doubles, 64 floats, one 64-bit mask
TABLE_SLOT = 1536                               # ... rounded up to whole 256-byte parts


@dataclasses.dataclass
class Enc:
    """One encoder leader, as the checks below need it.  A network's ``shape`` is (N, ed) for deep-sets and (N, dm, blocks, resid)
    for the transformer; H is the encoder's test module of its population's update, whose helpers are reused."""
    name: str
    H: object
    small: tuple                                # the smallest network
    middle: tuple                               # the network of the checks that need one shape only

    @property
    def transformer(self):
        return self.name == "transformer"

    def inputs(self, shape, S, B_l, n_epochs, seed):
        return self.H.update_inputs(shape, S, B_l, n_epochs, seed) if self.transformer else self.H.update_inputs(*shape, S, B_l, n_epochs, seed)

    def load(self, shape, seeds, tensors):
        return self.H.load_population(shape, seeds, tensors) if self.transformer else self.H.load_population(*shape, seeds, tensors)

    def fresh(self, shape, start, lr, max_grad_norm=0.5):
        """A lone network holding `start` and its lone optimiser at the learner's lr / max_grad_norm."""
        net, _ = self.H.fresh_learner(shape, start, lr) if self.transformer else self.H.fresh_learner(*shape, start, lr)
        return net, self.lone_adam(net, lr, max_grad_norm)

    def lone_adam(self, net, lr, max_grad_norm=0.5):
        from evacuation_amd import trainer
        return (trainer.TransformerAdam if self.transformer else trainer.DeviceAdam)(net, lr=lr, max_grad_norm=max_grad_norm)

    def pop_adam(self, pop, **kw):
        from evacuation_amd import population
        return (population.TransformerPopulationAdam if self.transformer else population.PopulationAdam)(pop, **kw)

    def lone_update(self, *a, **kw):
        from evacuation_amd import trainer
        return (trainer.transformer_update if self.transformer else trainer.deepsets_update)(*a, **kw)

    def sweep_update(self, *a, **kw):
        from evacuation_amd import population
        return (population.transformer_update_sweep if self.transformer else population.deepsets_update_sweep)(*a, **kw)

    def population_update(self, *a, **kw):
        from evacuation_amd import population
        return (population.transformer_update_population if self.transformer else population.deepsets_update_population)(*a, **kw)

    def workspace_bytes(self, D, M, S, sweep):
        from evacuation_amd import population
        return population.population_workspace_bytes(D, M, S, sweep=sweep, **{self.name: True})

    def collecting_population(self, env, S, blocks=2):
        """Freshly seeded learners on `env`'s observation, made visible as the encoder's own collection tests do."""
        from evacuation_amd import population
        from tests import test_gpu_deepsets_population as DP
        from tests import test_gpu_transformer_population as TP
        b, seeds = base(env), [11 + 7 * s for s in range(S)]
        if self.transformer:
            return TP.visible(population.TransformerPopulation(b.obs_dim, b.n_ped, seeds, DEV, num_blocks=blocks))
        return DP.visible(population.DeepSetsPopulation(b.obs_dim, b.n_ped, seeds, DEV))


def make_env(ea, case, E, offset, gamma=None, generic=False):
    """`gamma`: the wrapped env with that gamma; None: the raw env.  `generic`: the kernels that take the configuration at run time."""
    from evacuation_amd.options import KernelOptions
    cfg_kw, wrap_kw = case
    env = ea.BatchedEvacuationEnv(ea.EnvConfig(**cfg_kw), ea.EnvWrappersConfig(**wrap_kw), num_envs=E, seed=SEED, env_id_offset=offset,
                                  options=KernelOptions().replace(specialize=0) if generic else None)
    return env if gamma is None else ea.NormalizedVectorEnv(env, gamma=gamma)


def learner_index(S):
    import torch
    return torch.arange(S, device=DEV).reshape(S, 1, 1)


def state_of(pop, popt, stats):
    import torch
    torch.cuda.synchronize()
    return [t.clone() for t in pop.tensors + pop.grads + popt.exp_avg + popt.exp_avg_sq] + [popt.headers.clone(), stats.clone()]


# ------------------------------------------------------------------------------------------------ 1. collection
def check_collection(ea, enc, S, E_l, generic=False, T=30):
    """Learner s's storage, norm_state, records and final state are policy_rollout(nets[s])'s alone on a handle of E_l envs wrapped
    with gammas[s]; learner 0's rewards differ from a run with learner 1's gamma."""
    import torch
    gammas = GAMMAS[:S]
    pop_env = make_env(ea, NORM_CASE, S * E_l, OFFSET, gamma=0.75, generic=generic)       # (the env's own gamma is nobody's)
    pop = enc.collecting_population(pop_env, S)
    obs, done, now = start_population(pop_env)
    obs0, norm0 = obs.clone(), pop_env.norm_state.clone()
    ro = pop_env.policy_rollout_sweep(pop, T, obs, done, gammas)
    assert ro["next_obs"] is obs and ro["next_done"] is done
    torch.cuda.synchronize()
    ended = int(ro["dones"][1:].sum()) + int(ro["next_done"].sum())
    assert ended >= 1 and ended >= (S * E_l) // 5                     # autoresets, and the normaliser's terminal handling
    fin = snapshot(pop_env)
    alone_rewards = []
    for s in range(S):
        cols = slice(s * E_l, (s + 1) * E_l)
        env = make_env(ea, NORM_CASE, E_l, OFFSET + s * E_l, gamma=gammas[s], generic=generic)
        o, _ = env.reset()
        assert i32(o).equal(i32(obs0[cols])), (s, "the reset observation")
        base(env).set_state(now=now[cols].clone())
        assert raw(env.norm_state).equal(raw(norm0[cols])), (s, "norm_state after reset")
        alone = env.policy_rollout(pop.nets[s], T, o.clone(), torch.zeros(E_l, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize()
        for k in STORAGE_TE:
            assert i32(ro[k][:, cols]).equal(i32(alone[k])), (S, E_l, s, k)
        for k in STORAGE_E:
            assert i32(ro[k][cols]).equal(i32(alone[k])), (S, E_l, s, k)
        mine = snapshot(env)
        for k in mine:
            assert raw(fin[k][cols]).equal(raw(mine[k])), (S, E_l, s, k)
        sa, sb = base(pop_env).get_state(), base(env).get_state()
        for k in sa:
            assert sa[k][cols].contiguous().view(torch.uint8).equal(sb[k].contiguous().view(torch.uint8)), (s, k)
        alone_rewards.append(alone["rewards"].clone())
        env.close()
    pop_env.close()
    env = make_env(ea, NORM_CASE, E_l, OFFSET, gamma=gammas[1], generic=generic)
    o, _ = env.reset()
    base(env).set_state(now=now[:E_l].clone())
    other = env.policy_rollout(pop.nets[0], T, o.clone(), torch.zeros(E_l, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    assert i32(other["actions"][0]).equal(i32(ro["actions"][0, :E_l]))                   # the same first step ...
    assert not i32(other["rewards"]).equal(i32(alone_rewards[0]))                        # ... and other rewards
    env.close()


def _collect_twice(ea, enc, case, S, E_l, gamma, gammas, T=30, blocks=2):
    """The population entry's storage and the sweep entry's with `gammas`, each from the same start on an env of its own."""
    import torch
    runs = []
    for sweep in (False, True):
        env = make_env(ea, case, S * E_l, OFFSET, gamma=gamma)
        pop = enc.collecting_population(env, S, blocks)
        obs, done, _ = start_population(env)
        if sweep:
            ro = env.policy_rollout_sweep(pop, T, obs, done, gammas)
        else:
            ro = env.policy_rollout_population(pop, T, obs, done)
        torch.cuda.synchronize()
        runs.append(({k: ro[k].clone() for k in STORAGE_TE + STORAGE_E}, snapshot(env)))
        if sweep and gamma is None:                                  # a raw env: checked all the same
            with pytest.raises(ValueError):
                env.policy_rollout_sweep(pop, T, obs, done, gammas[:-1])
            with pytest.raises(ea._lib.EvacError):
                env.policy_rollout_sweep(pop, T, obs, done, [gammas[0], float("nan")] + list(gammas[2:]))
        env.close()
    (a, sa), (b, sb) = runs
    assert int(a["dones"].sum()) >= 1
    for k in a:
        assert i32(a[k]).equal(i32(b[k])), k
    for k in sa:
        assert raw(sa[k]).equal(raw(sb[k])), k


def check_equal_gammas_are_the_population_entry(ea, enc):
    _collect_twice(ea, enc, NORM_CASE, 3, 3, 0.99, [0.99] * 3)


def check_gammas_change_nothing_on_a_raw_env(ea, enc):
    _collect_twice(ea, enc, RAW_CASE, 3, 4, None, GAMMAS, blocks=1)


def check_a_policy_population_is_forwarded(ea):
    """policy_rollout_sweep(PolicyPopulation) is policy_rollout_population(gammas=)."""
    import torch
    from tests.test_gpu_population import make_population
    case = (dict(number_of_pedestrians=10, max_timesteps=20), dict(positions="grav"))
    runs = []
    for sweep in (False, True):
        env = make_env(ea, case, 6, OFFSET, gamma=0.75)
        pop = make_population(ea, base(env).obs_dim, [11, 18])
        obs, done, _ = start_population(env)
        ro = env.policy_rollout_sweep(pop, 30, obs, done, GAMMAS[:2]) if sweep else env.policy_rollout_population(pop, 30, obs, done, gammas=GAMMAS[:2])
        torch.cuda.synchronize()
        runs.append({k: ro[k].clone() for k in STORAGE_TE + STORAGE_E})
        env.close()
    for k in runs[0]:
        assert i32(runs[0][k]).equal(i32(runs[1][k])), k


# ------------------------------------------------------------------------------------------------ 2. update
def check_update(ea, enc, shape, B_l, E_l, M, norm_adv):
    """Every learner its own lr, clip, ent, vf, alpha and max_grad_norm (tests/test_gpu_sweep.learner_cfg), S = 3, two epochs, a draw
    counter of its own per learner; norm_adv < 0: with the perturbation injected."""
    import torch
    from evacuation_amd import trainer
    S, n_epochs = 3, 2
    inject, norm_adv = norm_adv < 0, abs(norm_adv)
    cfgs = [learner_cfg(s, norm_adv, 1) for s in range(S)]
    seeds = [900 + 13 * s for s in range(S)]
    firsts = [1000 + 37 * s for s in range(S)]
    D, nets, batches, perms = enc.inputs(shape, S, B_l, n_epochs, seed=50 + shape[0] + B_l)
    common = interleave(batches, E_l)
    pop = enc.load(shape, seeds, [enc.H.all_tensors(n) for n in nets])
    popt = enc.pop_adam(pop, lr=[c.learning_rate for c in cfgs], max_grad_norm=[c.max_grad_norm for c in cfgs])
    steps = n_epochs * len(trainer.update_steps(B_l, M, bool(norm_adv)))
    rows = pop_rows(perms, E_l, S)
    stats = torch.full((S, steps, 8), -7.0, device=DEV)
    noise = None
    if inject:
        gen = torch.Generator().manual_seed(shape[0] + M)
        noise = torch.stack([(torch.rand(steps, M, 2, generator=gen) * 2 - 1) * c.rpo_alpha for c in cfgs]).to(DEV).contiguous()
    out, headers = enc.sweep_update(pop, common, rows, cfgs, popt, minibatch_size=M, rpo_noise=noise, seeds=seeds,
                                    first_draw_counters=firsts, stats=stats)
    assert out is stats and headers is popt.headers
    torch.cuda.synchronize()
    for s in range(S):
        opt = enc.lone_adam(nets[s], cfgs[s].learning_rate, cfgs[s].max_grad_norm)
        alone = torch.full((steps, 8), -7.0, device=DEV)
        _, header = enc.lone_update(nets[s], batches[s], perms[s].contiguous(), cfgs[s], opt, rpo_noise=None if noise is None else noise[s],
                                    seed=seeds[s], first_draw_counter=firsts[s], stats=alone, minibatch_size=M)
        h = trainer.decode_header(header)
        assert (h["steps_run"], h["epochs_run"], h["stop"], h["t"]) == (steps, n_epochs, 0, steps), h
        enc.H.assert_learner_equals(pop, popt, s, nets[s], opt, shape + (B_l, M))
        assert same_bits(stats[s], alone), (shape, B_l, M, s)
    assert not bool((stats == -7.0).any())
    assert not same_bits(stats[0], stats[1])                         # learners 0 and 1 differ
    assert not same_bits(pop.tensors[13][0], pop.tensors[13][1])


def pop_rows(perms, E_l, S):
    from evacuation_amd import population
    return population.population_rows(perms, learner_index(S), E_l, S)


# ------------------------------------------------------------------------------------------------ 3. uniform values
def check_uniform_values_are_the_population_entry(ea, enc):
    import torch
    from evacuation_amd import trainer
    shape, B_l, E_l, M, n_epochs, S = enc.middle, 200, 4, 72, 2, 3
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    seeds, firsts = [7, 8, 9], [5, 6, 7]
    D, nets, batches, perms = enc.inputs(shape, S, B_l, n_epochs, seed=31)
    start = [[p.detach().clone() for p in enc.H.all_tensors(n)] for n in nets]
    common, rows = interleave(batches, E_l), pop_rows(perms, E_l, S)
    steps = n_epochs * len(trainer.update_steps(B_l, M, True))
    results = []
    for update, cfg_arg in ((enc.population_update, cfg), (enc.sweep_update, [cfg] * S), (enc.sweep_update, cfg)):
        pop = enc.load(shape, seeds, start)
        popt = enc.pop_adam(pop, lr=1e-3)
        stats = torch.full((S, steps, 8), -7.0, device=DEV)
        update(pop, common, rows, cfg_arg, popt, minibatch_size=M, seeds=seeds, first_draw_counters=firsts, stats=stats)
        results.append(state_of(pop, popt, stats))
    for i, (x, y, z) in enumerate(zip(*results)):
        assert same_bits(x, y), ("S equal configurations", i)
        assert same_bits(x, z), ("one configuration", i)
    assert not bool((results[0][-1] == -7.0).any())


# ------------------------------------------------------------------------------------------------ 4. target_kl
def check_target_kl_is_each_learners_own(ea, enc):
    """tests/test_gpu_sweep.py::test_target_kl_is_each_learners_own's construction: old log-probabilities that are the network's own
    and no perturbation, so approx_kl starts near zero and grows as the policy moves.  The thresholds come from the lone runs
    without a target: the learner whose first epoch closes with the largest approx_kl gets half of that as its target and stops
    after its first epoch; of its neighbours one has no target and one a target above everything it reaches."""
    import torch
    shape, B_l, E_l, M, n_epochs, lr, S = enc.middle, 144, 4, 72, 4, 1e-3, 3
    per_epoch = B_l // M
    steps = n_epochs * per_epoch
    cfg = loss_cfg(1, 1, 0.01, 0.0)
    seeds, firsts = [3, 4, 5], [0, 10, 20]
    D, nets, batches, perms = enc.inputs(shape, S, B_l, n_epochs, seed=77)
    start = []
    for s, net in enumerate(nets):
        with torch.no_grad():
            net.actor_logstd.copy_(torch.tensor([[-0.4 - 0.7 * s, 0.2 - 0.7 * s]]))
            _, lp, _, _ = net.get_action_and_value(batches[s]["b_obs"], batches[s]["b_actions"])
            batches[s]["b_logprobs"] = lp.contiguous()
        start.append([p.detach().clone() for p in enc.H.all_tensors(net)])

    def alone(s, c, stats):
        net, opt = enc.fresh(shape, start[s], lr)
        enc.lone_update(net, batches[s], perms[s].contiguous(), c, opt, seed=seeds[s], first_draw_counter=firsts[s], stats=stats,
                        minibatch_size=M)
        torch.cuda.synchronize()
        return net, opt

    closing = []
    for s in range(S):
        stats = torch.zeros(steps, 8, device=DEV)
        alone(s, cfg, stats)
        closing.append([float(stats[(e + 1) * per_epoch - 1, 5]) for e in range(n_epochs)])
        print(f"\nlearner {s}: closing approx_kl per epoch:", " ".join(f"{x:.3e}" for x in closing[-1]))
    eager = max(range(S), key=lambda s: closing[s][0])
    free, high = sorted({0, 1, 2} - {eager})
    assert closing[eager][0] > 0.0, closing                          # (fails, not skips)
    targets = {eager: 0.5 * closing[eager][0], free: None, high: 2.0 * max(closing[high]) + 1.0}
    cfgs = [dataclasses.replace(cfg, target_kl=targets[s]) for s in range(S)]
    pop = enc.load(shape, seeds, start)
    popt = enc.pop_adam(pop, lr=lr)
    stats = torch.full((S, steps, 8), -7.0, device=DEV)
    enc.sweep_update(pop, interleave(batches, E_l), pop_rows(perms, E_l, S), cfgs, popt, minibatch_size=M, seeds=seeds,
                     first_draw_counters=firsts, stats=stats)
    torch.cuda.synchronize()
    epochs_run = []
    for s in range(S):
        mine = torch.full((steps, 8), -7.0, device=DEV)
        net, opt = alone(s, cfgs[s], mine)
        h, hp = opt.read_header(), popt.learners[s].read_header()
        assert hp == h, (s, hp, h)
        enc.H.assert_learner_equals(pop, popt, s, net, opt, "target_kl per learner")
        assert same_bits(stats[s], mine), s
        ran = h["steps_run"]
        assert ran == h["epochs_run"] * per_epoch
        assert bool((stats[s, ran:] == -7.0).all()) and not bool((stats[s, :ran] == -7.0).any())      # later rows: untouched
        epochs_run.append(h["epochs_run"])
    print("epochs run with targets", targets, ":", epochs_run)
    assert epochs_run[eager] == 1 and epochs_run[free] == n_epochs and epochs_run[high] == n_epochs, epochs_run
    assert [h["stop"] for h in popt.read_headers()] == [int(s == eager) for s in range(S)]


# ------------------------------------------------------------------------------------------------ 5. the table and the mask at their ends
def check_the_table_and_the_mask_at_their_ends(ea, enc):
    """S = 64, the smallest network, B_l = M = 8, one epoch: learners 0, 31, 32 and 63 have lrs of their own, 32 and 63 a target
    that the one step exceeds (bits >= 32 of the mask): the four equal their lone runs, stop flag included."""
    import torch
    shape, B_l, E_l, M, S = enc.small, 8, 1, 8, 64
    watched = {0: 2e-3, 31: 5e-4, 32: 7e-4, 63: 3e-3}
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    cfgs = [dataclasses.replace(cfg, target_kl=1e-9 if s in (32, 63) else None) for s in range(S)]
    lrs = [watched.get(s, 1e-3) for s in range(S)]
    seeds, firsts = [100 + s for s in range(S)], [3 * s for s in range(S)]
    D, nets, batches, perms = enc.inputs(shape, S, B_l, 1, seed=9)
    pop = enc.load(shape, seeds, [enc.H.all_tensors(n) for n in nets])
    popt = enc.pop_adam(pop, lr=lrs)
    stats = torch.full((S, 1, 8), -7.0, device=DEV)
    enc.sweep_update(pop, interleave(batches, E_l), pop_rows(perms, E_l, S), cfgs, popt, minibatch_size=M, seeds=seeds,
                     first_draw_counters=firsts, stats=stats)
    torch.cuda.synchronize()
    for s in watched:
        opt = enc.lone_adam(nets[s], lrs[s])
        alone = torch.full((1, 8), -7.0, device=DEV)
        enc.lone_update(nets[s], batches[s], perms[s].contiguous(), cfgs[s], opt, seed=seeds[s], first_draw_counter=firsts[s], stats=alone,
                        minibatch_size=M)
        enc.H.assert_learner_equals(pop, popt, s, nets[s], opt, ("S = 64", s))
        assert same_bits(stats[s], alone), s
        assert float(alone[0, 5]) > 1e-9                             # the target is exceeded
        assert opt.read_header()["stop"] == int(s in (32, 63)), (s, opt.read_header())
    assert [h["stop"] for h in popt.read_headers()] == [int(s in (32, 63)) for s in range(S)]


# ------------------------------------------------------------------------------------------------ 6. the workspace
def check_the_workspace(ea, enc):
    """One update inside a workspace of exactly the sweep sizer's bytes between canaries; the table is its last 1536 bytes and holds
    the learners' values as evac::LearnerSteps lays them out."""
    import torch
    shape, B_l, E_l, M, S = enc.middle, 200, 4, 72, 3
    cfgs = [learner_cfg(s, 1, 1) for s in range(S)]
    cfgs[2] = dataclasses.replace(cfgs[2], target_kl=123.5)          # (never reached: bit 2 of the mask and its double)
    seeds, firsts = [7, 8, 9], [5, 6, 7]
    D, nets, batches, perms = enc.inputs(shape, S, B_l, 1, seed=12)
    need = enc.workspace_bytes(D, M, S, True)
    assert need == enc.workspace_bytes(D, M, S, False) + TABLE_SLOT
    pop = enc.load(shape, seeds, [enc.H.all_tensors(n) for n in nets])
    popt = enc.pop_adam(pop, lr=[c.learning_rate for c in cfgs], max_grad_norm=[c.max_grad_norm for c in cfgs])
    guard = WorkspaceGuard(need, fill=0x3C, offset=16)
    guard.snapshot()
    enc.sweep_update(pop, interleave(batches, E_l), pop_rows(perms, E_l, S), cfgs, popt, minibatch_size=M, seeds=seeds,
                     first_draw_counters=firsts, workspace=guard.slice)
    torch.cuda.synchronize()
    guard.assert_outside_unchanged(enc.name)
    tail = bytes(guard.slice[need - TABLE_SLOT:].cpu().tolist())
    lr = [c.learning_rate for c in cfgs] + [0.0] * (64 - S)
    kl = [0.0, 0.0, 123.5] + [0.0] * (64 - S)
    norm = [c.max_grad_norm for c in cfgs] + [0.0] * (64 - S)
    expected = struct.pack("<64d64d64fQ", *lr, *kl, *norm, 1 << 2)
    assert len(expected) == TABLE_BYTES and tail[:TABLE_BYTES] == expected, "the table: evac::LearnerSteps, word for word"
    assert tail[TABLE_BYTES:] == bytes([0x3C]) * (TABLE_SLOT - TABLE_BYTES), "behind the table: untouched"
    for s in range(S):                                               # and the update inside it is the lone one
        net, opt = nets[s], enc.lone_adam(nets[s], cfgs[s].learning_rate, cfgs[s].max_grad_norm)
        enc.lone_update(net, batches[s], perms[s].contiguous(), cfgs[s], opt, seed=seeds[s], first_draw_counter=firsts[s], minibatch_size=M)
        enc.H.assert_learner_equals(pop, popt, s, net, opt, "workspace")


# ------------------------------------------------------------------------------------------------ 7. determinism, capture
def check_determinism_and_capture(ea, enc):
    """Two calls give the same bits; a captured update replayed after the host changed a learner's lr runs with the captured values."""
    import torch
    from evacuation_amd import trainer
    shape, B_l, E_l, M, n_epochs, S = enc.middle, 100, 2, 40, 2, 3              # a tail of 20
    cfgs = [learner_cfg(s, 1, 1) for s in range(S)]
    seeds, firsts = [7, 8, 9], [5, 6, 7]
    D, nets, batches, perms = enc.inputs(shape, S, B_l, n_epochs, seed=31)
    start = [[p.detach().clone() for p in enc.H.all_tensors(n)] for n in nets]
    common, rows = interleave(batches, E_l), pop_rows(perms, E_l, S)
    steps = n_epochs * len(trainer.update_steps(B_l, M, True))
    need = enc.workspace_bytes(D, M, S, True)

    def run(capture):
        pop = enc.load(shape, seeds, start)
        popt = enc.pop_adam(pop, lr=[c.learning_rate for c in cfgs], max_grad_norm=[c.max_grad_norm for c in cfgs])
        stats = torch.full((S, steps, 8), -7.0, device=DEV)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        call = lambda: enc.sweep_update(pop, common, rows, cfgs, popt, minibatch_size=M, seeds=seeds, first_draw_counters=firsts,
                                        stats=stats, workspace=ws)
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
        popt.learners[1].param_groups[0]["lr"] = 123.0               # after the capture: not seen by the replay
        g.replay()
        return state_of(pop, popt, stats)

    a, b, c = run(False), run(False), run(True)
    for i, (x, y, z) in enumerate(zip(a, b, c)):
        assert same_bits(x, y), ("two calls", i)
        assert same_bits(x, z), ("captured replay", i)
    assert not bool((a[-1] == -7.0).any())


# ------------------------------------------------------------------------------------------------ 8. the whole loop
def training_env(ea, E, offset, gamma):
    return ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=10, max_timesteps=40),
                                       ea.EnvWrappersConfig(positions="rel", statuses="ohe", type="Box"), num_envs=E, gamma=gamma, seed=SEED,
                                       env_id_offset=offset)


def training_cfgs(E_l, T, seeds):
    from evacuation_amd.trainer import RPOTrainingConfig
    one = RPOTrainingConfig(num_envs=E_l, num_steps=T, total_timesteps=E_l * T * 2, num_minibatches=2, update_epochs=2, anneal_lr=True)
    return [dataclasses.replace(one, seed=seeds[0], learning_rate=3e-4, gamma=0.99, gae_lambda=0.95, ent_coef=0.0),
            dataclasses.replace(one, seed=seeds[1], learning_rate=1e-3, anneal_lr=False, gamma=0.9, gae_lambda=0.8, ent_coef=0.01),
            dataclasses.replace(one, seed=seeds[2], learning_rate=1e-4, gamma=0.999, gae_lambda=1.0, ent_coef=0.02)]


def check_sweep_trainer_equals_standalone_trainers(ea, enc):
    """The shapes of the encoder's own test_population_trainer_equals_standalone_trainers; the configurations differ in
    learning_rate, gamma, gae_lambda, ent_coef and anneal_lr."""
    import torch
    from evacuation_amd import policy, population, trainer
    S, E_l, T, seeds = 3, 4, 16, [11, 18, 25]
    cfgs = training_cfgs(E_l, T, seeds)
    env = training_env(ea, S * E_l, OFFSET, 0.75)                    # (the env's own gamma is nobody's)
    if enc.transformer:
        ptr = population.PopulationTrainer(env, population.TransformerPopulation(env.obs_dim, 10, seeds, DEV), cfgs,
                                           optimizer="device_transformer", encoder_sweep=True)
        lone = dict(grad_fn=trainer.transformer_kernel_grad, optimizer="device_transformer")
        make_net = lambda D: policy.TransformerActorCritic(D, 10)
    else:
        ptr = population.PopulationTrainer(env, population.DeepSetsPopulation(env.obs_dim, 10, seeds, DEV), cfgs, encoder_sweep=True)
        lone = dict(grad_fn=trainer.deepsets_kernel_grad, optimizer="device")
        make_net = lambda D: policy.DeepSetsActorCritic(D, 10)
    assert ptr.sweep and ptr.encoder_sweep
    alone = []
    for s, c in enumerate(cfgs):
        e = training_env(ea, E_l, OFFSET + s * E_l, c.gamma)         # the twin handle, wrapped with the learner's own gamma
        torch.manual_seed(seeds[s])
        tr = trainer.RPOTrainer(e, make_net(e.obs_dim).to(DEV), c, one_call=True, **lone)
        obs, _ = e.reset()                                           # the handle's seed: _start would reseed the env with cfg.seed
        tr.next_obs, tr.next_done = obs.clone(), torch.zeros(E_l, dtype=torch.float32, device=DEV)
        tr.start_time = time.time()
        alone.append(tr)
    rates = []
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
            for i, (p, q) in enumerate(zip(enc.H.all_tensors(ptr.nets[s]), enc.H.all_tensors(tr.net))):
                assert same_bits(p, q), (u, s, i)
                assert same_bits(ptr.optimizer.exp_avg[i][s], tr.optimizer.exp_avg[i]), (u, s, "exp_avg", i)
                assert same_bits(ptr.optimizer.exp_avg_sq[i][s], tr.optimizer.exp_avg_sq[i]), (u, s, "exp_avg_sq", i)
            for k in STORAGE_TE:
                assert i32(ptr.storage[k][:, cols]).equal(i32(tr.storage[k])), (u, s, k)
            for k in STORAGE_E:
                assert i32(ptr.storage[k][cols]).equal(i32(tr.storage[k])), (u, s, k)
            assert same_bits(ptr.advantages[:, cols], tr.advantages) and same_bits(ptr.returns[:, cols], tr.returns), (u, s)
            assert raw(ptr.env.norm_state[cols]).equal(raw(tr.env.norm_state)), (u, s)
            assert ptr.minibatch_steps[s] == tr.minibatch_steps and same_bits(ptr.optimizer.headers[s], tr.optimizer.header)
        rates.append([l["learning_rate"] for l in logs])
    assert rates[0] == [3e-4, 1e-3, 1e-4] and rates[1] == [0.5 * 3e-4, 1e-3, 0.5 * 1e-4]       # one does not anneal
    assert logs[0]["config"] == {} and logs[1]["config"] == {"learning_rate": 1e-3, "anneal_lr": False, "gamma": 0.9, "gae_lambda": 0.8,
                                                             "ent_coef": 0.01}
    assert ptr.minibatch_steps == [2 * 2 * 2] * S
    for tr in alone:
        tr.env.close()
    ptr.env.close()
