"""Population sweeps on an MI355X: learners that differ in their hyperparameters, in one set of launches, each BIT FOR BIT the
learner it would be alone with its own configuration.

1. GAE: evac_gae_learners == gae on each learner's own columns with its own (gamma, lambda); equal pairs == gae on the whole.
2. Collection: a NormalizeReward gamma per learner == policy_rollout on handles wrapped with that gamma.
3. Update: evac_rpo_update_sweep == S rpo_update calls, each with its own loss coefficients, learning rate and max_grad_norm;
   with equal values == evac_rpo_update_population.
4. target_kl per learner: one learner stops early, one has no target, one has a target it never reaches.
5. Whole loop: PopulationTrainer(cfgs) == S RPOTrainer(optimizer="device", one_call=True) on twin handles, update by update.
6. PopulationAdam: loading one learner's state_dict touches that learner alone.  A captured update freezes the learners' values.

Equal means: the float32 / int64 / float64 words are compared as integers."""
import dataclasses
import time

import pytest

from tests import trainer_ref as R
from tests.test_gpu_policy_rollout import CASES, OFFSET, SEED, base, i32, raw
from tests.test_gpu_population import (LOG_SCALARS, STORAGE_E, STORAGE_TE, assert_learner_equals, interleave, load_population,
                                       make_population, same_number, same_records, snapshot, start_population)
from tests.trainer_cases import DEV, build_case, loss_cfg, make_net, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import evacuation_amd
    from evacuation_amd import build
    build.build_library()
    return evacuation_amd


# ------------------------------------------------------------------------------------------------ 1. GAE
GAMMAS, LAMBDAS = [0.99, 0.9, 0.999], [0.95, 0.8, 1.0]


@pytest.mark.parametrize("S,E_l", [(3, 5), (3, 70)])
def test_gae_takes_each_learners_own_pair(ea, S, E_l):
    """E_l = 70: the learners' boundaries (env 70, 140) fall inside waves."""
    import torch
    from evacuation_amd import trainer
    T, E = 17, S * E_l
    g = torch.Generator().manual_seed(E)
    storage = {"rewards": torch.randn(T, E, generator=g), "values": torch.randn(T, E, generator=g),
               "dones": (torch.rand(T, E, generator=g) < 0.2).float(), "next_value": torch.randn(E, generator=g),
               "next_done": (torch.rand(E, generator=g) < 0.3).float()}
    storage = {k: v.to(DEV).contiguous() for k, v in storage.items()}
    assert 0 < float(storage["dones"].sum()) < T * E and 0 < float(storage["next_done"].sum()) < E
    adv, ret = trainer.gae(storage, GAMMAS, LAMBDAS, envs_per_learner=E_l)
    torch.cuda.synchronize()
    for s in range(S):
        cols = slice(s * E_l, (s + 1) * E_l)
        own = {k: v[..., cols].contiguous() for k, v in storage.items()}
        a, r = trainer.gae(own, GAMMAS[s], LAMBDAS[s])
        assert same_bits(adv[:, cols], a) and same_bits(ret[:, cols], r), (S, E_l, s)
    assert not same_bits(adv[:, :E_l], trainer.gae({k: v[..., :E_l].contiguous() for k, v in storage.items()}, GAMMAS[1], LAMBDAS[1])[0])
    # equal pairs: the existing kernel on the whole array
    a_all, r_all = trainer.gae(storage, 0.99, 0.95)
    a_eq, r_eq = trainer.gae(storage, [0.99] * S, [0.95] * S, envs_per_learner=E_l)
    assert same_bits(a_eq, a_all) and same_bits(r_eq, r_all)
    out = (torch.empty_like(adv), torch.empty_like(adv))
    assert trainer.gae(storage, GAMMAS, 0.95, out=out, envs_per_learner=E_l)[0] is out[0]      # one lambda for all, `out` reused
    with pytest.raises(ValueError, match="envs_per_learner"):
        trainer.gae(storage, GAMMAS, LAMBDAS)
    with pytest.raises(ValueError):
        trainer.gae(storage, GAMMAS[:2], LAMBDAS, envs_per_learner=E_l)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. collection
def sweep_gammas(S):
    return [0.99, 0.9, 0.5, 0.95, 0.8][:S]


def make_env(ea, case, E, offset, gamma=None, **cfg_over):
    cfg_kw, wrap_kw, norm = CASES[case]
    env = ea.BatchedEvacuationEnv(ea.EnvConfig(**{**cfg_kw, **cfg_over}), ea.EnvWrappersConfig(**wrap_kw), num_envs=E, seed=SEED, env_id_offset=offset)
    return (ea.NormalizedVectorEnv(env) if gamma is None else ea.NormalizedVectorEnv(env, gamma=gamma)) if norm else env


def collection_normalises_rewards_with_each_learners_gamma(ea, case, S, E_l, T=30, gammas=None, **cfg_over):
    """Learner s's storage, norm_state, records and final state are those of policy_rollout(nets[s]) alone on an env of the
    learner's own gamma.  Returns the sweep call's storage."""
    import torch
    gammas = gammas or sweep_gammas(S)
    pop_env = make_env(ea, case, S * E_l, OFFSET, gamma=0.75, **cfg_over)        # (the env's own gamma is nobody's: it must not be used)
    D = base(pop_env).obs_dim
    pop = make_population(ea, D, [11 + 7 * s for s in range(S)])
    obs, done, now = start_population(pop_env)
    obs0, norm0 = obs.clone(), pop_env.norm_state.clone()
    ro = pop_env.policy_rollout_population(pop, T, obs, done, gammas=gammas)
    assert ro["next_obs"] is obs and ro["next_done"] is done
    torch.cuda.synchronize()
    ended = int(ro["dones"][1:].sum()) + int(ro["next_done"].sum())
    assert ended >= 1 and ended >= (S * E_l) // 5                     # autoresets, and the normaliser's terminal handling
    fin = snapshot(pop_env)
    alone_rewards = []
    for s in range(S):
        cols = slice(s * E_l, (s + 1) * E_l)
        env = make_env(ea, case, E_l, OFFSET + s * E_l, gamma=gammas[s], **cfg_over)
        o, _ = env.reset()
        assert i32(o).equal(i32(obs0[cols])), (case, s, "the reset observation")
        base(env).set_state(now=now[cols].clone())
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
        sa, sb = base(pop_env).get_state(), base(env).get_state()
        for k in sa:
            assert sa[k][cols].contiguous().view(torch.uint8).equal(sb[k].contiguous().view(torch.uint8)), (case, s, k)
        alone_rewards.append(alone["rewards"].clone())
        env.close()
    pop_env.close()
    # gamma does enter: the same learner (net, envs, start state) under another learner's gamma gets other normalised rewards
    env = make_env(ea, case, E_l, OFFSET, gamma=gammas[1], **cfg_over)
    o, _ = env.reset()
    base(env).set_state(now=now[:E_l].clone())
    other = env.policy_rollout(pop.nets[0], T, o.clone(), torch.zeros(E_l, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    assert i32(other["actions"][0]).equal(i32(ro["actions"][0, :E_l]))                   # the same first step ...
    assert not i32(other["rewards"]).equal(i32(alone_rewards[0]))                        # ... and other rewards
    assert not i32(ro["rewards"][:, :E_l]).equal(i32(ro["rewards"][:, E_l:2 * E_l]))
    env.close()
    return ro


@pytest.mark.parametrize("S,E_l", [(3, 3), (4, 40)])
@pytest.mark.parametrize("case", ["n60_grav_norm_clip", "n60_rel_ohe_box_norm_clip"])
def test_collection_normalises_rewards_with_each_learners_gamma(ea, case, S, E_l):
    collection_normalises_rewards_with_each_learners_gamma(ea, case, S, E_l)


def test_equal_gammas_are_the_population_kernel(ea):
    import torch
    S, E_l, T, case = 3, 3, 30, "n60_grav_norm_clip"
    runs = []
    for gammas in (None, [0.99] * S):
        env = make_env(ea, case, S * E_l, OFFSET)                     # NormalizedVectorEnv's default gamma: 0.99
        pop = make_population(ea, 6, [11 + 7 * s for s in range(S)])
        obs, done, _ = start_population(env)
        kw = {} if gammas is None else {"gammas": gammas}
        ro = env.policy_rollout_population(pop, T, obs, done, **kw)
        torch.cuda.synchronize()
        runs.append(({k: ro[k].clone() for k in STORAGE_TE + STORAGE_E}, snapshot(env)))
        env.close()
    (a, sa), (b, sb) = runs
    for k in a:
        assert i32(a[k]).equal(i32(b[k])), k
    for k in sa:
        assert raw(sa[k]).equal(raw(sb[k])), k


def test_gammas_change_nothing_on_a_raw_env(ea):
    import torch
    S, E_l, T, case = 3, 4, 30, "n10_grav_raw"
    runs = []
    for gammas in (None, [0.99, 0.9, 0.5]):
        env = make_env(ea, case, S * E_l, OFFSET)
        pop = make_population(ea, base(env).obs_dim, [11 + 7 * s for s in range(S)])
        obs, done, _ = start_population(env)
        kw = {} if gammas is None else {"gammas": gammas}
        ro = env.policy_rollout_population(pop, T, obs, done, **kw)
        torch.cuda.synchronize()
        runs.append(({k: ro[k].clone() for k in STORAGE_TE + STORAGE_E}, snapshot(env)))
        if gammas is not None:
            with pytest.raises(ValueError):
                env.policy_rollout_population(pop, T, obs, done, gammas=[0.9, 0.8])      # checked all the same
            with pytest.raises(ea._lib.EvacError):
                env.policy_rollout_population(pop, T, obs, done, gammas=[0.9, float("nan"), 0.8])
        env.close()
    (a, sa), (b, sb) = runs
    assert int(a["dones"].sum()) >= 1
    for k in a:
        assert i32(a[k]).equal(i32(b[k])), k
    for k in sa:
        assert raw(sa[k]).equal(raw(sb[k])), k


# ------------------------------------------------------------------------------------------------ 3. update
SWEEP_UPDATE_CASES = [  # D, B_l, E_l, M, norm_adv, clip_vloss, injected noise, S: of tests/test_gpu_population.UPDATE_CASES
    (6, 1024, 4, 256, 1, 1, False, 3),
    (6, 1000, 4, 256, 1, 0, True, 4),           # the tail minibatch runs
    (396, 1024, 2, 256, 1, 1, False, 2),        # the widest observation
    (6, 192, 3, 48, 1, 1, False, 1),
]


def learner_cfg(s, norm_adv, clip_vloss):
    """Every learner its own learning rate, clip range, entropy and value coefficients, alpha and max_grad_norm.  Learner 0's
    max_grad_norm is far below any gradient norm of these cases (clip coefficient < 1) and learner 1's far above (== 1)."""
    cfg = loss_cfg(norm_adv, clip_vloss, ent_coef=0.01 * s, rpo_alpha=0.5 - 0.15 * s, clip_coef=0.2 + 0.05 * s, vf_coef=0.5 + 0.25 * s)
    cfg.learning_rate = 1e-3 / (s + 1)
    cfg.max_grad_norm = [1e-3, 1e6, 0.5, 2.0][s]
    return cfg


@pytest.mark.parametrize("D,B_l,E_l,M,norm_adv,clip_vloss,inject,S", SWEEP_UPDATE_CASES)
def test_update_equals_standalone_updates_with_each_learners_config(ea, D, B_l, E_l, M, norm_adv, clip_vloss, inject, S):
    import torch
    from evacuation_amd import population, trainer
    n_epochs = 3
    cfgs = [learner_cfg(s, norm_adv, clip_vloss) for s in range(S)]
    seeds = [900 + 13 * s for s in range(S)]
    firsts = [1000 + 37 * s for s in range(S)]
    nets, batches = [], []
    for s in range(S):
        net, batch, *_ = build_case(D, B_l, "repeat", cfgs[s], seed=50 + D + B_l + s)
        nets.append(net)
        batches.append(batch)
    start = [[p.detach().clone() for p in R.mlp_tensors(net)] for net in nets]
    common = interleave(batches, E_l)
    pop = load_population(ea, D, seeds, nets)
    popt = population.PopulationAdam(pop, lr=[c.learning_rate for c in cfgs], max_grad_norm=[c.max_grad_norm for c in cfgs])
    gen = torch.Generator().manual_seed(B_l + S)
    perms = torch.stack([torch.stack([torch.randperm(B_l, generator=gen) for _ in range(n_epochs)]) for _ in range(S)]).to(DEV)
    steps = n_epochs * len(trainer.update_steps(B_l, M, bool(norm_adv)))
    noise = None
    if inject:
        noise = torch.stack([(torch.rand(steps, M, 2, generator=gen) * 2 - 1) * c.rpo_alpha for c in cfgs]).to(DEV).contiguous()
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_l, S)
    stats = torch.full((S, steps, 8), -7.0, device=DEV)
    out, headers = population.rpo_update_population(pop, common, rows, cfgs, popt, minibatch_size=M, rpo_noise=noise, seeds=seeds,
                                                    first_draw_counters=firsts, stats=stats)
    assert out is stats and headers is popt.headers
    torch.cuda.synchronize()
    clip_coefs = []
    for s in range(S):
        opt = trainer.DeviceAdam(nets[s], lr=cfgs[s].learning_rate, max_grad_norm=cfgs[s].max_grad_norm)
        alone = torch.full((steps, 8), -7.0, device=DEV)
        _, header = trainer.rpo_update(nets[s], batches[s], perms[s].contiguous(), cfgs[s], opt,
                                       rpo_noise=None if noise is None else noise[s], seed=seeds[s], first_draw_counter=firsts[s],
                                       stats=alone, minibatch_size=M)
        h = trainer.decode_header(header)
        assert (h["steps_run"], h["epochs_run"], h["stop"], h["t"]) == (steps, n_epochs, 0, steps), h
        assert_learner_equals(pop, popt, s, nets[s], opt, (D, B_l, M, S))
        assert same_bits(stats[s], alone), (D, B_l, M, S, s)
        # the clip coefficient of every step, from the STANDALONE statistics: min(1, max_grad_norm / (|g| + 1e-6))
        norms = alone[:, 7].double().sqrt()
        clip_coefs.append((cfgs[s].max_grad_norm / (norms + 1e-6)).clamp(max=1.0))
    assert not bool((stats == -7.0).any())
    assert float(clip_coefs[0].max()) < 1.0, clip_coefs[0]           # learner 0: every step clipped
    if S > 1:
        assert float(clip_coefs[1].min()) == 1.0, clip_coefs[1]      # learner 1: never
        assert not same_bits(stats[0], stats[1])
    # all learners with learner 0's values: the sweep's kernels against the population's, from the same start
    c0 = cfgs[0]
    results = []
    for cfg_arg in (c0, [c0] * S):
        p2 = ea.PolicyPopulation(D, seeds, DEV)
        with torch.no_grad():
            for s in range(S):
                for p, q in zip(R.mlp_tensors(p2.nets[s]), start[s]):
                    p.copy_(q)
        o2 = population.PopulationAdam(p2, lr=c0.learning_rate, max_grad_norm=c0.max_grad_norm)
        st2 = torch.full((S, steps, 8), -7.0, device=DEV)
        population.rpo_update_population(p2, common, rows, cfg_arg, o2, minibatch_size=M, rpo_noise=noise, seeds=seeds,
                                         first_draw_counters=firsts, stats=st2)
        torch.cuda.synchronize()
        results.append((p2, o2, st2))
    (pa, oa, sa), (pb, ob, sb) = results
    assert same_bits(sa, sb) and same_bits(oa.headers, ob.headers)
    for i in range(13):
        assert same_bits(pa.tensors[i], pb.tensors[i]) and same_bits(pa.grads[i], pb.grads[i]), R.NAMES[i]
        assert same_bits(oa.exp_avg[i], ob.exp_avg[i]) and same_bits(oa.exp_avg_sq[i], ob.exp_avg_sq[i]), R.NAMES[i]


# ------------------------------------------------------------------------------------------------ 4. target_kl per learner
def test_target_kl_is_each_learners_own(ea):
    """tests/test_gpu_population.py::test_learners_stop_at_different_epochs's construction: old log-probabilities that are the
    network's own and no perturbation, so approx_kl starts at zero and grows as the policy moves.  The thresholds come from the
    standalone runs without a target: the eager learner gets a target it exceeds before its last epoch, the calm one NONE, the
    third a target above everything it reaches."""
    import torch
    from evacuation_amd import population, trainer
    D, B_l, E_l, M, n_epochs, lr, S = 6, 1024, 4, 256, 6, 1e-3, 3
    per_epoch = B_l // M
    steps = n_epochs * per_epoch
    cfg = loss_cfg(1, 1, 0.01, 0.0)
    seeds, firsts = [3, 4, 5], [0, 10, 20]
    start, batches = [], []
    for s in range(S):
        net, batch, *_ = build_case(D, B_l, "repeat", cfg, seed=77 + s)
        with torch.no_grad():
            net.actor_logstd.copy_(torch.tensor([[-0.4 - 0.7 * s, 0.2 - 0.7 * s]]))
            P = [p.detach() for p in R.mlp_tensors(net)]
            lp, _, _ = R.logprob_entropy_value(P, batch["b_obs"], batch["b_actions"], torch.zeros(B_l, 2, device=DEV))
            batch["b_logprobs"] = lp.contiguous()
        start.append([p.detach().clone() for p in R.mlp_tensors(net)])
        batches.append(batch)
    gen = torch.Generator().manual_seed(8)
    perms = torch.stack([torch.stack([torch.randperm(B_l, generator=gen) for _ in range(n_epochs)]) for _ in range(S)]).to(DEV)

    def alone(s, c, stats):
        net = make_net(D, seed=s)
        with torch.no_grad():
            for p, q in zip(R.mlp_tensors(net), start[s]):
                p.copy_(q)
        opt = trainer.DeviceAdam(net, lr=lr)
        trainer.rpo_update(net, batches[s], perms[s].contiguous(), c, opt, seed=seeds[s], first_draw_counter=firsts[s], stats=stats,
                           minibatch_size=M)
        torch.cuda.synchronize()
        return net, opt

    closing = []
    for s in range(S):
        stats = torch.zeros(steps, 8, device=DEV)
        alone(s, cfg, stats)
        closing.append([float(stats[(e + 1) * per_epoch - 1, 5]) for e in range(n_epochs)])
        print(f"\nlearner {s}: closing approx_kl per epoch:", " ".join(f"{x:.3e}" for x in closing[-1]))
    calm = min(range(S), key=lambda s: max(closing[s]))
    eager = max(range(S), key=lambda s: max(closing[s][:-1]))
    third = ({0, 1, 2} - {calm, eager}).pop()
    lo, hi = max(closing[calm]), max(closing[eager][:-1])
    assert lo < hi, closing                                          # (fails, not skips)
    targets = {eager: 0.5 * (lo + hi), calm: None, third: 2.0 * max(closing[third]) + 1.0}
    cfgs = [dataclasses.replace(cfg, target_kl=targets[s]) for s in range(S)]
    pop = ea.PolicyPopulation(D, seeds, DEV)
    with torch.no_grad():
        for s in range(S):
            for p, q in zip(R.mlp_tensors(pop.nets[s]), start[s]):
                p.copy_(q)
    popt = population.PopulationAdam(pop, lr=lr)
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_l, S)
    stats = torch.full((S, steps, 8), -7.0, device=DEV)
    population.rpo_update_population(pop, interleave(batches, E_l), rows, cfgs, popt, minibatch_size=M, seeds=seeds,
                                     first_draw_counters=firsts, stats=stats)
    torch.cuda.synchronize()
    epochs_run = []
    for s in range(S):
        mine = torch.full((steps, 8), -7.0, device=DEV)
        net, opt = alone(s, cfgs[s], mine)
        h, hp = opt.read_header(), popt.learners[s].read_header()
        assert hp == h, (s, hp, h)
        assert_learner_equals(pop, popt, s, net, opt, "target_kl per learner")
        assert same_bits(stats[s], mine), s
        ran = h["steps_run"]
        assert ran == h["epochs_run"] * per_epoch
        assert bool((stats[s, ran:] == -7.0).all()) and not bool((stats[s, :ran] == -7.0).any())      # rows beyond steps_run: untouched
        epochs_run.append(h["epochs_run"])
    print("epochs run with targets", targets, ":", epochs_run)
    assert epochs_run[eager] < n_epochs and epochs_run[calm] == n_epochs and epochs_run[third] == n_epochs, epochs_run
    assert [h["stop"] for h in popt.read_headers()] == [int(s == eager) for s in range(S)]


# ------------------------------------------------------------------------------------------------ 5. the whole loop
def training_env(ea, E, offset, gamma):
    return ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=10, max_timesteps=40), ea.EnvWrappersConfig(positions="grav"),
                                       num_envs=E, gamma=gamma, seed=SEED, env_id_offset=offset)


def sweep_cfgs(E_l, T, seeds):
    from evacuation_amd.trainer import RPOTrainingConfig
    one = RPOTrainingConfig(num_envs=E_l, num_steps=T, total_timesteps=E_l * T * 3, num_minibatches=4, update_epochs=4)
    return [dataclasses.replace(one, seed=seeds[0], learning_rate=3e-4, gamma=0.99, gae_lambda=0.95, ent_coef=0.0, target_kl=0.01),
            dataclasses.replace(one, seed=seeds[1], learning_rate=1e-3, anneal_lr=False, gamma=0.9, gae_lambda=0.8, ent_coef=0.01,
                                target_kl=None),
            dataclasses.replace(one, seed=seeds[2], learning_rate=1e-4, gamma=0.999, gae_lambda=1.0, ent_coef=0.02, target_kl=0.5)]


def make_sweep_trainer(ea, E_l, T, seeds):
    cfgs = sweep_cfgs(E_l, T, seeds)
    env = training_env(ea, len(cfgs) * E_l, OFFSET, 0.75)            # (the env's own gamma is nobody's)
    return ea.PopulationTrainer(env, ea.PolicyPopulation(env.obs_dim, seeds, DEV), cfgs)


def test_sweep_trainer_equals_standalone_trainers(ea):
    import torch
    from evacuation_amd.policy import LinearActorCritic
    from evacuation_amd.trainer import RPOTrainer
    S, E_l, T = 3, 3, 64
    seeds = [21 + 5 * s for s in range(S)]
    ptr = make_sweep_trainer(ea, E_l, T, seeds)
    alone = []
    for s, cfg in enumerate(sweep_cfgs(E_l, T, seeds)):
        env = training_env(ea, E_l, OFFSET + s * E_l, cfg.gamma)     # the twin handle, wrapped with the learner's own gamma
        torch.manual_seed(seeds[s])
        tr = RPOTrainer(env, LinearActorCritic(env.obs_dim).to(DEV), cfg, optimizer="device", one_call=True)
        obs, _ = env.reset()
        tr.next_obs, tr.next_done = obs.clone(), torch.zeros(E_l, dtype=torch.float32, device=DEV)
        tr.start_time = time.time()
        alone.append(tr)
    rates = []
    for u in range(3):
        logs = ptr.update()
        torch.cuda.synchronize()
        assert len(logs) == S
        for s, tr in enumerate(alone):
            log = tr.update()
            torch.cuda.synchronize()
            cols = slice(s * E_l, (s + 1) * E_l)
            for k in LOG_SCALARS:
                assert same_number(logs[s][k], log[k]), (u, s, k, logs[s][k], log[k])
            assert set(log) <= set(logs[s])
            for k in log["episodes"]:
                assert same_records(logs[s]["episodes"][k], log["episodes"][k]), (u, s, k)
            for i, (p, q) in enumerate(zip(R.mlp_tensors(ptr.nets[s]), R.mlp_tensors(tr.net))):
                assert same_bits(p, q), (u, s, R.NAMES[i])
            assert raw(ptr.env.norm_state[cols]).equal(raw(tr.env.norm_state)), (u, s)
            assert same_bits(ptr.last_permutations[s], torch.stack(tr.last_permutations)), (u, s)
            assert ptr.minibatch_steps[s] == tr.minibatch_steps and same_bits(ptr.optimizer.headers[s], tr.optimizer.header), (u, s)
        rates.append([l["learning_rate"] for l in logs])
        print(f"\nupdate {u}: learning rates {rates[-1]}, epochs run {[l['epochs_run'] for l in logs]}")
    assert rates[0] == [3e-4, 1e-3, 1e-4] and rates[2][1] == 1e-3 and rates[2][0] < 3e-4 and rates[2][2] < 1e-4       # one does not anneal
    assert logs[0]["config"] == {} and logs[1]["config"] == {"learning_rate": 1e-3, "anneal_lr": False, "gamma": 0.9, "gae_lambda": 0.8,
                                                             "ent_coef": 0.01, "target_kl": None}
    assert ptr.minibatch_steps[1] == 3 * 4 * 4                        # no target: every epoch of every update
    for tr in alone:
        tr.env.close()
    ptr.env.close()


def test_two_sweep_runs_give_the_same_bits(ea):
    import torch
    runs = []
    for _ in range(2):
        ptr = make_sweep_trainer(ea, 3, 64, [1, 2, 3])
        logs = ptr.learn()
        torch.cuda.synchronize()
        assert len(logs) == 3 and all(len(l) == 3 for l in logs)
        runs.append(([t.clone() for t in ptr.population.tensors], ptr.env.norm_state.clone(), ptr.optimizer.headers.clone(),
                     [[l[k] for k in LOG_SCALARS] for per in logs for l in per], list(ptr.minibatch_steps)))
        ptr.env.close()
    a, b = runs
    for x, y in zip(a[0], b[0]):
        assert same_bits(x, y)
    assert raw(a[1]).equal(raw(b[1])) and same_bits(a[2], b[2]) and a[4] == b[4]
    assert all(same_number(x, y) for la, lb in zip(a[3], b[3]) for x, y in zip(la, lb))


def test_loading_one_learners_state_dict_touches_that_learner_alone(ea):
    import torch
    from evacuation_amd import population
    pop = ea.PolicyPopulation(6, [1, 2, 3], DEV)
    popt = population.PopulationAdam(pop, lr=[1e-4, 2e-4, 3e-4])
    headers0 = popt.headers.clone()
    sd = popt.state_dict(1)
    assert sd["param_groups"][0]["lr"] == 2e-4
    sd["param_groups"][0]["lr"] = 5e-3
    sd["param_groups"][0]["max_grad_norm"] = 0.25
    for i in sd["state"]:
        sd["state"][i]["step"] = torch.tensor(7.0)
        sd["state"][i]["exp_avg"] = torch.full_like(sd["state"][i]["exp_avg"], 0.5)
    popt.load_state_dict(1, sd)
    torch.cuda.synchronize()
    assert [g["lr"] for g in popt.param_groups] == [1e-4, 5e-3, 3e-4]
    assert [g["max_grad_norm"] for g in popt.param_groups] == [0.5, 0.25, 0.5]
    assert popt.learners[1].read_header()["t"] == 7 and same_bits(popt.headers[0], headers0[0]) and same_bits(popt.headers[2], headers0[2])
    for m in popt.exp_avg:
        assert bool((m[1] == 0.5).all()) and bool((m[0] == 0).all()) and bool((m[2] == 0).all())
    assert popt.config(1).lr == 5e-3 and popt.config(0).lr == 1e-4 and not popt.uniform()


def test_a_captured_sweep_update_freezes_the_learners_values(ea):
    """evac_rpo_update_sweep captured once and replayed twice == two direct calls from the same start; the values travel in the
    kernel arguments, so changing a learner's rate after the capture changes nothing in the replays."""
    import torch
    from evacuation_amd import population, trainer
    D, B_l, E_l, M, S = 6, 192, 3, 48, 2
    cfgs = [learner_cfg(s, 1, 1) for s in range(S)]
    seeds, firsts = [5, 6], [100, 200]
    nets, batches = [], []
    for s in range(S):
        net, batch, *_ = build_case(D, B_l, "repeat", cfgs[s], seed=300 + s)
        nets.append(net)
        batches.append(batch)
    common = interleave(batches, E_l)
    gen = torch.Generator().manual_seed(4)
    perms = torch.stack([torch.stack([torch.randperm(B_l, generator=gen)]) for _ in range(S)]).to(DEV)
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_l, S)
    steps = len(trainer.update_steps(B_l, M, True))

    def make():
        pop = load_population(ea, D, seeds, nets)
        popt = population.PopulationAdam(pop, lr=[c.learning_rate for c in cfgs], max_grad_norm=[c.max_grad_norm for c in cfgs])
        stats = torch.zeros(S, steps, 8, device=DEV)
        ws = torch.empty(population.population_workspace_bytes(D, M, S), dtype=torch.uint8, device=DEV)
        call = lambda: population.rpo_update_population(pop, common, rows, cfgs, popt, minibatch_size=M, seeds=seeds,
                                                        first_draw_counters=firsts, stats=stats, workspace=ws)
        return pop, popt, stats, call

    pa, oa, sa, call_a = make()
    call_a()                                                         # warm-up, undone in place
    torch.cuda.synchronize()
    with torch.no_grad():
        for s in range(S):
            for p, q in zip(R.mlp_tensors(pa.nets[s]), R.mlp_tensors(nets[s])):
                p.copy_(q)
        for t in oa.exp_avg + oa.exp_avg_sq:
            t.zero_()
        oa.headers.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call_a()
    oa.learners[1].param_groups[0]["lr"] = 123.0                     # after the capture: not seen by the replays
    graph.replay()
    first = sa.clone()
    graph.replay()
    torch.cuda.synchronize()
    pb, ob, sb, call_b = make()
    call_b()
    torch.cuda.synchronize()
    assert same_bits(first, sb)
    call_b()
    torch.cuda.synchronize()
    assert same_bits(sa, sb) and same_bits(oa.headers, ob.headers) and not same_bits(first, sb)
    for i in range(13):
        assert same_bits(pa.tensors[i], pb.tensors[i]), R.NAMES[i]
        assert same_bits(oa.exp_avg[i], ob.exp_avg[i]) and same_bits(oa.exp_avg_sq[i], ob.exp_avg_sq[i]), R.NAMES[i]
    assert [h["t"] for h in oa.read_headers()] == [2 * steps] * S
