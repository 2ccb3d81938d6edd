"""Population training on an MI355X: S learners in one set of launches, each BIT FOR BIT the learner it would be alone.

1. Collection: policy_rollout_population == S policy_rollout calls on handles of E_l envs with env_id_offset further by s E_l.
2. Update: evac_rpo_update_population on one common batch == S rpo_update calls on the learners' own rows.
3. target_kl: the learners stop at different epochs; a stopped learner's later rows are untouched while the others go on.
4. Whole loop: PopulationTrainer == S RPOTrainer(optimizer="device") on twin handles, update by update.
5. Determinism, graph capture, evaluation.

Equal means: the float32 / int64 / float64 words are compared as integers."""
import time

import pytest

from tests import trainer_ref as R
from tests.test_gpu_policy_rollout import CASES, OFFSET, SEED, base, i32, raw
from tests.trainer_cases import DEV, build_case, loss_cfg, same_bits

pytestmark = pytest.mark.gpu

STORAGE_TE = ("obs", "actions", "logprobs", "values", "rewards", "dones", "episode_stats")      # [T, E, ...]
STORAGE_E = ("next_value", "next_obs", "next_done")                                             # [E, ...]
STATE = ("ped", "status", "agent", "clock", "acc")


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


def make_population(ea, D, seeds):
    """Freshly seeded learners made visible as tests/test_gpu_policy_rollout.make_net does, each in its own way."""
    import torch
    pop = ea.PolicyPopulation(D, seeds, DEV)
    with torch.no_grad():
        for s, net in enumerate(pop.nets):
            g = torch.Generator().manual_seed(1000 + s)
            net.actor_mean[4].weight.mul_(60.0)
            net.actor_logstd.copy_(torch.tensor([[-0.5 + 0.1 * s, 0.3 - 0.05 * s]]))
            for m in list(net.actor_mean) + list(net.critic):
                if isinstance(m, torch.nn.Linear):
                    m.bias.copy_((0.2 * torch.randn(m.bias.shape, generator=g)).to(DEV))
    return pop


def start_population(env, near_trunc=5):
    """reset; every `near_trunc`-th env of the WHOLE batch one step before truncation (the next one two).  Returns
    (next_obs, next_done, the `now` given to the env)."""
    import torch
    obs, _ = env.reset()
    b = base(env)
    now = b.get_state()["now"].clone()
    if near_trunc:
        now[::near_trunc] = b.env_config.max_timesteps - 1
        now[1::near_trunc] = b.env_config.max_timesteps - 2
        b.set_state(now=now)
    return obs.clone(), torch.zeros(b.num_envs, dtype=torch.float32, device=b.device), now


def snapshot(env):
    b = base(env)
    s = {k: getattr(b, k).clone() for k in STATE}
    if hasattr(env, "norm_state"):
        s["norm_state"] = env.norm_state.clone()
    return s


def restore(env, s):
    b = base(env)
    for k in STATE:
        getattr(b, k).copy_(s[k])
    if "norm_state" in s:
        env.norm_state.copy_(s["norm_state"])


# ------------------------------------------------------------------------------------------------ 1. collection
def collection_equals_standalone_rollouts(ea, case, S, E_l, T=30, **cfg_over):
    """The storage, norm_state, the episode records and the final state of learner s's envs are those of policy_rollout(nets[s])
    alone.  Returns the population call's storage."""
    import torch
    pop_env = make_env(ea, case, S * E_l, OFFSET, **cfg_over)
    D = base(pop_env).obs_dim
    pop = make_population(ea, D, [11 + 7 * s for s in range(S)])
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
        sa, sb = base(pop_env).get_state(), base(env).get_state()
        for k in sa:
            assert sa[k][cols].contiguous().view(torch.uint8).equal(sb[k].contiguous().view(torch.uint8)), (case, s, k)
        env.close()
    if S > 1:                                                        # the learners did act differently
        assert not i32(ro["actions"][:, :E_l]).equal(i32(ro["actions"][:, E_l:2 * E_l]))
    pop_env.close()
    return ro


@pytest.mark.parametrize("S,E_l", [(1, 48), (3, 3), (5, 16), (4, 40)])
@pytest.mark.parametrize("case", ["n60_grav_norm_clip", "n60_rel_ohe_box_norm_clip", "n32_abs_cat_dict_norm", "n10_grav_raw"])
def test_collection_equals_standalone_rollouts(ea, case, S, E_l):
    """Gravity D = 6, the generic "rel + ohe Box" observation at N = 60 and an N <= 32 room, with the normalisation chain, and a
    raw gravity env without it."""
    collection_equals_standalone_rollouts(ea, case, S, E_l)


def test_collection_errors(ea):
    import torch
    env = make_env(ea, "n60_grav_norm_clip", 12, OFFSET)
    obs, done, _ = start_population(env, near_trunc=0)
    with pytest.raises(ValueError, match="equal shares"):
        env.policy_rollout_population(make_population(ea, 6, list(range(5))), 4, obs, done)
    with pytest.raises(ValueError, match="observation dim"):
        env.policy_rollout_population(make_population(ea, 7, [1, 2, 3]), 4, obs, done)
    torch.cuda.synchronize()
    env.close()


# ------------------------------------------------------------------------------------------------ 2. update
def interleave(batches, E_l):
    """The learners' own batches ([B_l, ...] each, flattened [T, E_l]) as ONE common batch, flattened [T, S E_l]."""
    import torch
    S = len(batches)
    out = {}
    for k in batches[0]:
        parts = [b[k].reshape(-1, E_l, *b[k].shape[1:]) for b in batches]              # [T, E_l, ...]
        out[k] = torch.stack(parts, dim=1).reshape(-1, *batches[0][k].shape[1:]).contiguous()      # [T, S, E_l, ...] flattened
    assert out["b_obs"].shape[0] == S * batches[0]["b_obs"].shape[0]
    return out


def load_population(ea, D, seeds, nets):
    """A population whose row s holds the parameters of nets[s]."""
    import torch
    pop = ea.PolicyPopulation(D, seeds, DEV)
    with torch.no_grad():
        for s, net in enumerate(nets):
            for p, q in zip(R.mlp_tensors(pop.nets[s]), R.mlp_tensors(net)):
                p.copy_(q)
    return pop


def assert_learner_equals(pop, popt, s, net, opt, what):
    import torch
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(R.mlp_tensors(pop.nets[s]), R.mlp_tensors(net))):
        assert same_bits(p, q), (what, s, "param", R.NAMES[i], float((p - q).abs().max()))
        assert same_bits(p.grad, q.grad), (what, s, "clipped grad", R.NAMES[i])
        assert same_bits(popt.exp_avg[i][s], opt.exp_avg[i]), (what, s, "exp_avg", R.NAMES[i])
        assert same_bits(popt.exp_avg_sq[i][s], opt.exp_avg_sq[i]), (what, s, "exp_avg_sq", R.NAMES[i])
    assert same_bits(popt.headers[s], opt.header), (what, s, popt.learners[s].read_header(), opt.read_header())


UPDATE_CASES = [  # D, B_l, E_l, M, norm_adv, clip_vloss, injected noise, S
    (6, 1024, 4, 256, 1, 1, False, 3),
    (6, 1000, 4, 256, 1, 0, True, 4),           # B_l mod M = 232: the tail minibatch runs
    (124, 1000, 8, 256, 0, 1, False, 3),        # ... and without norm_adv
    (396, 1024, 2, 256, 1, 1, False, 2),        # the widest observation (more dynamic LDS than the default limit)
    (6, 1025, 5, 256, 1, 1, False, 5),          # B_l mod M = 1 with norm_adv: the tail is skipped
    (6, 1025, 5, 256, 0, 0, True, 2),           # ... and runs without it
    (6, 192, 3, 48, 1, 1, False, 1),            # one learner: the indirection alone
]


@pytest.mark.parametrize("D,B_l,E_l,M,norm_adv,clip_vloss,inject,S", UPDATE_CASES)
def test_update_equals_standalone_updates(ea, D, B_l, E_l, M, norm_adv, clip_vloss, inject, S):
    import torch
    from evacuation_amd import population, trainer
    cfg = loss_cfg(norm_adv, clip_vloss, 0.01, 0.5)
    n_epochs = 3
    seeds = [900 + 13 * s for s in range(S)]
    firsts = [1000 + 37 * s for s in range(S)]                      # every learner at a draw counter of its own
    nets, batches = [], []
    for s in range(S):
        net, batch, *_ = build_case(D, B_l, "repeat", cfg, seed=50 + D + B_l + s)
        nets.append(net)
        batches.append(batch)
    common = interleave(batches, E_l)
    pop = load_population(ea, D, seeds, nets)
    popt = population.PopulationAdam(pop, lr=1e-3)
    gen = torch.Generator().manual_seed(B_l + S)
    perms = torch.stack([torch.stack([torch.randperm(B_l, generator=gen) for _ in range(n_epochs)]) for _ in range(S)]).to(DEV)
    steps = n_epochs * len(trainer.update_steps(B_l, M, bool(norm_adv)))
    noise = ((torch.rand(S, steps, M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV).contiguous() if inject else None
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_l, S)
    for s in range(S):                                               # the mapping: the learner's own row, in the common batch
        assert same_bits(common["b_obs"][rows[s, 0]], batches[s]["b_obs"][perms[s, 0]])
    stats = torch.full((S, steps, 8), -7.0, device=DEV)
    out, headers = population.rpo_update_population(pop, common, rows, cfg, popt, minibatch_size=M, rpo_noise=noise, seeds=seeds,
                                                    first_draw_counters=firsts, stats=stats)
    assert out is stats and headers is popt.headers
    torch.cuda.synchronize()
    for s in range(S):
        opt = trainer.DeviceAdam(nets[s], lr=1e-3)
        alone = torch.full((steps, 8), -7.0, device=DEV)
        _, header = trainer.rpo_update(nets[s], batches[s], perms[s].contiguous(), cfg, opt, rpo_noise=None if noise is None else noise[s],
                                       seed=seeds[s], first_draw_counter=firsts[s], stats=alone, minibatch_size=M)
        h = trainer.decode_header(header)
        assert (h["steps_run"], h["epochs_run"], h["stop"], h["t"]) == (steps, n_epochs, 0, steps), h
        assert_learner_equals(pop, popt, s, nets[s], opt, (D, B_l, M, S))
        assert same_bits(stats[s], alone), (D, B_l, M, S, s)
    assert not bool((stats == -7.0).any())
    if S > 1:
        assert not same_bits(stats[0], stats[1])


@pytest.mark.parametrize("B_l,norm_adv,target_kl,per_epoch", [
    (37, 1, None, 5),                           # B_l mod M = 5: the tail runs
    (33, 1, None, 4),                           # B_l mod M = 1 with norm_adv: the tail is skipped
    (33, 0, None, 5),                           # ... and runs without it
    (37, 1, 1e-6, 5),                           # every learner stops at its first epoch's end
])
def test_the_three_update_entries_walk_the_same_steps(ea, B_l, norm_adv, target_kl, per_epoch):
    """evac_rpo_update, evac_rpo_update_population and evac_rpo_update_sweep share one step loop: from the same weights every
    learner ends with the same bits whichever entry ran it.  The perturbation is drawn on the device at non-zero draw counters
    that differ between the learners (the lone entry adds the counter on the host, the others in the kernel), and the shapes are
    the smallest with a tail, an epoch boundary and a stop."""
    import torch
    from evacuation_amd import population, trainer
    D, S, M, E_l, n_epochs, lr = 6, 2, 8, 1, 2, 1e-3
    cfg = loss_cfg(norm_adv, 1, 0.01, 0.5)
    cfg.target_kl = target_kl
    seeds, firsts = [21, 34], [3, 11]
    steps = n_epochs * per_epoch
    assert steps == n_epochs * len(trainer.update_steps(B_l, M, bool(norm_adv)))
    nets, batches = [], []
    for s in range(S):
        net, batch, *_ = build_case(D, B_l, "repeat", cfg, seed=400 + B_l + s)
        nets.append(net)
        batches.append(batch)
    common = interleave(batches, E_l)
    gen = torch.Generator().manual_seed(B_l)
    perms = torch.stack([torch.stack([torch.randperm(B_l, generator=gen) for _ in range(n_epochs)]) for _ in range(S)]).to(DEV)
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_l, S)
    runs = []
    for form in (cfg, [cfg] * S):                                    # one configuration: the population entry; a list: the sweep's
        pop = load_population(ea, D, seeds, nets)
        popt = population.PopulationAdam(pop, lr=lr)
        stats = torch.full((S, steps, 8), -7.0, device=DEV)
        population.rpo_update_population(pop, common, rows, form, popt, minibatch_size=M, seeds=seeds, first_draw_counters=firsts,
                                         stats=stats)
        runs.append((pop, popt, stats))
    torch.cuda.synchronize()
    ran = per_epoch if target_kl is not None else steps
    for s in range(S):
        opt = trainer.DeviceAdam(nets[s], lr=lr)
        alone = torch.full((steps, 8), -7.0, device=DEV)
        _, header = trainer.rpo_update(nets[s], batches[s], perms[s].contiguous(), cfg, opt, seed=seeds[s], first_draw_counter=firsts[s],
                                       stats=alone, minibatch_size=M)
        h = trainer.decode_header(header)
        assert (h["steps_run"], h["epochs_run"], h["t"]) == (ran, ran // per_epoch, ran), h
        assert not bool((alone[:ran] == -7.0).any()) and bool((alone[ran:] == -7.0).all())          # rows beyond steps_run: untouched
        for (pop, popt, stats), entry in zip(runs, ("population", "sweep")):
            hp = popt.learners[s].read_header()
            assert (hp["steps_run"], hp["epochs_run"], hp["t"]) == (h["steps_run"], h["epochs_run"], h["t"]), (entry, s, hp, h)
            assert_learner_equals(pop, popt, s, nets[s], opt, (entry, B_l, norm_adv, target_kl))
            assert same_bits(stats[s], alone), (entry, B_l, norm_adv, target_kl, s)
    assert not same_bits(runs[0][2][0, :ran], runs[0][2][1, :ran])


# ------------------------------------------------------------------------------------------------ 3. target_kl
def test_learners_stop_at_different_epochs(ea):
    """The inputs are chosen from the standalone runs: old log-probabilities that are the network's own and no perturbation, so
    approx_kl starts at zero and grows as the policy moves -- faster for a learner with a smaller sigma.  The target lies between
    the calmest learner's largest closing approx_kl and what another learner exceeds before its last epoch."""
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

    def fresh(s):
        from tests.trainer_cases import make_net
        net = make_net(D, seed=s)
        with torch.no_grad():
            for p, q in zip(R.mlp_tensors(net), start[s]):
                p.copy_(q)
        return net, trainer.DeviceAdam(net, lr=lr)

    def alone(s, stats):
        net, opt = fresh(s)
        trainer.rpo_update(net, batches[s], perms[s].contiguous(), cfg, opt, seed=seeds[s], first_draw_counter=firsts[s], stats=stats,
                           minibatch_size=M)
        torch.cuda.synchronize()
        return net, opt

    # 1. the standalone runs without a target: every epoch's closing approx_kl
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
    # 2. the standalone runs with the target, 3. the population
    pop = ea.PolicyPopulation(D, seeds, DEV)
    with torch.no_grad():
        for s in range(S):
            for p, q in zip(R.mlp_tensors(pop.nets[s]), start[s]):
                p.copy_(q)
    popt = population.PopulationAdam(pop, lr=lr)
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_l, S)
    stats = torch.full((S, steps, 8), -7.0, device=DEV)
    population.rpo_update_population(pop, interleave(batches, E_l), rows, cfg, popt, minibatch_size=M, seeds=seeds,
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
    # a later call clears every learner's flag and runs
    cfg.target_kl = None
    population.rpo_update_population(pop, interleave(batches, E_l), rows[:, :1].contiguous(), cfg, popt, minibatch_size=M, seeds=seeds)
    for s, h in enumerate(popt.read_headers()):
        assert (h["stop"], h["steps_run"], h["epochs_run"]) == (0, per_epoch, 1), (s, h)


# ------------------------------------------------------------------------------------------------ 4. the whole loop
LOG_SCALARS = ("update", "global_step", "learning_rate", "value_loss", "policy_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac",
               "explained_variance", "loss")


def training_env(ea, E, offset, gamma):
    return ea.NormalizedVectorEnv.make(ea.EnvConfig(number_of_pedestrians=10, max_timesteps=40), ea.EnvWrappersConfig(positions="grav"),
                                       num_envs=E, gamma=gamma, seed=SEED, env_id_offset=offset)


def training_cfg(E_l, T, seed, target_kl):
    from evacuation_amd.trainer import RPOTrainingConfig
    return RPOTrainingConfig(seed=seed, num_envs=E_l, num_steps=T, total_timesteps=E_l * T * 3, num_minibatches=4, update_epochs=4,
                             target_kl=target_kl)


def make_population_trainer(ea, S, E_l, T, seeds, target_kl=None):
    cfg = training_cfg(E_l, T, 0, target_kl)
    env = training_env(ea, S * E_l, OFFSET, cfg.gamma)
    return ea.PopulationTrainer(env, ea.PolicyPopulation(env.obs_dim, seeds, DEV), cfg)


def same_number(a, b):
    return a == b or (a != a and b != b)


def same_records(a, b):
    """Columns of the episode records, possibly empty (no episode ended in the update)."""
    return a.shape == b.shape and (a.numel() == 0 or raw(a).equal(raw(b)))


@pytest.mark.parametrize("S,E_l,T,target_kl", [(3, 3, 64, None), (4, 32, 32, 0.01)])
def test_population_trainer_equals_standalone_trainers(ea, S, E_l, T, target_kl):
    import torch
    from evacuation_amd.policy import LinearActorCritic
    from evacuation_amd.trainer import RPOTrainer
    seeds = [21 + 5 * s for s in range(S)]
    ptr = make_population_trainer(ea, S, E_l, T, seeds, target_kl)
    alone = []
    for s in range(S):
        cfg = training_cfg(E_l, T, seeds[s], target_kl)
        env = training_env(ea, E_l, OFFSET + s * E_l, cfg.gamma)
        torch.manual_seed(seeds[s])
        tr = RPOTrainer(env, LinearActorCritic(env.obs_dim).to(DEV), cfg, optimizer="device", one_call=True)
        obs, _ = env.reset()                                         # the handle's seed: _start would reseed the env with cfg.seed
        tr.next_obs, tr.next_done = obs.clone(), torch.zeros(E_l, dtype=torch.float32, device=DEV)
        tr.start_time = time.time()
        alone.append(tr)
    stopped_early = 0
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
            assert ptr.minibatch_steps[s] == tr.minibatch_steps and same_bits(ptr.optimizer.headers[s], tr.optimizer.header)
            stopped_early += logs[s]["epochs_run"] < ptr.cfg.update_epochs
        print(f"\nupdate {u}: epochs run {[l['epochs_run'] for l in logs]}, closing approx_kl {[round(l['approx_kl'], 4) for l in logs]}")
    print(f"\n(S, E_l, T) = ({S}, {E_l}, {T}), target_kl = {target_kl}: learner-updates that stopped early: {stopped_early} of {3 * S}; "
          f"minibatch steps {ptr.minibatch_steps}")
    if target_kl is None:
        assert stopped_early == 0 and ptr.minibatch_steps == [3 * 4 * 4] * S
    for tr in alone:
        tr.env.close()
    ptr.env.close()


# ------------------------------------------------------------------------------------------------ 5. determinism, capture, evaluation
def test_two_population_runs_give_the_same_bits(ea):
    import torch
    runs = []
    for _ in range(2):
        ptr = make_population_trainer(ea, 3, 3, 64, [1, 2, 3], target_kl=0.02)
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
    assert not same_bits(a[0][0][0], a[0][0][1])                      # (the learners are not copies of each other)


def test_captured_collection_reads_the_weights_in_place(ea):
    """tests/test_gpu_policy_rollout.py::test_captured_call_reads_the_weights_in_place for the population form."""
    import torch
    S, E_l = 4, 16
    env = make_env(ea, "n60_grav_norm_clip", S * E_l, OFFSET)
    pop = make_population(ea, 6, [1, 2, 3, 4])
    obs, done, _ = start_population(env)
    out = env.policy_rollout_population(pop, 8, obs, done)       # warm-up, allocates `out`
    torch.cuda.synchronize()
    s0, o0, d0 = snapshot(env), obs.clone(), done.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            env.policy_rollout_population(pop, 8, obs, done, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    restore(env, s0); obs.copy_(o0); done.copy_(d0)
    g.replay()
    torch.cuda.synchronize()
    old_actions = out["actions"].clone()
    with torch.no_grad():                                         # an optimiser step on the stacks: in place
        for t in pop.tensors:
            t.add_(0.05 * torch.randn_like(t))
    restore(env, s0); obs.copy_(o0); done.copy_(d0)
    out["episode_stats"].zero_()                                  # (records are written only where an episode ended)
    g.replay()
    torch.cuda.synchronize()
    replayed = {k: v.clone() for k, v in out.items()}
    after = snapshot(env)
    restore(env, s0); obs.copy_(o0); done.copy_(d0)
    direct = env.policy_rollout_population(pop, 8, obs, done)
    torch.cuda.synchronize()
    for k in STORAGE_TE + STORAGE_E:
        assert i32(replayed[k]).equal(i32(direct[k])), k
    fin = snapshot(env)
    for k in fin:
        assert raw(fin[k]).equal(raw(after[k])), k
    for s in range(S):                                            # the replay did use every learner's new weights
        cols = slice(s * E_l, (s + 1) * E_l)
        assert not torch.equal(old_actions[:, cols], replayed["actions"][:, cols]), s
    env.close()


def test_evaluate_returns_every_learners_result(ea):
    import torch
    S, E_l = 3, 8
    ptr = make_population_trainer(ea, S, E_l, 32, [4, 5, 6])
    ptr.update()
    results = ptr.evaluate(n_episodes=2)
    assert len(results) == S
    ev = ptr.make_evaluator()
    assert ev.num_envs == E_l
    for s in range(S):
        with torch.no_grad():
            one = ev.evaluate(ptr.nets[s], 2, norm_state=ptr.env.norm_state[s * E_l:(s + 1) * E_l].clone(), obs_clip=ptr.env.obs_clip,
                              epsilon=ptr.env.epsilon)
        assert set(one.episodes) == set(results[s].episodes)
        for k in one.episodes:
            assert raw(one.episodes[k]).equal(raw(results[s].episodes[k])), (s, k)
        assert one.steps.equal(results[s].steps) and one.n_pedestrians == results[s].n_pedestrians
        assert results[s].summary()["episodes"] == 2 * E_l
    assert not raw(results[0].episodes["episode_reward"]).equal(raw(results[1].episodes["episode_reward"]))
    ptr.evaluator.close()
    ptr.env.close()
