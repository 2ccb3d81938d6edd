"""The join contract of include/evac.h for every rollout form a handle can take (plain, parts = 2, chain = 1, chain = 2, and the team
kernels): after evac_join -- or any other call on the handle, which settles it by itself -- the caller's state arrays ARE the state.
A checkpoint copied into the bound tensors, state arrays rebound to fresh tensors, an evac_team_clear_error on a clean handle: each is
honoured by the next rollout, which gives the same bits as a plain handle that did the same."""
import pytest

from tests.test_gpu_variants_sweep import ea  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

STATE = ("ped", "status", "agent", "clock", "acc")
T, CALLS = 5, 3

# (name, N, E, options): the forms of one-wave envs on a batch the chained forms accept, and the team kernels (N > 512, few envs)
FORMS = [("plain", 60, 64, dict(parts=1, chain=0)),
         ("parts", 60, 64, dict(parts=2, chain=0)),
         ("chain", 60, 64, dict(cu_wide=1, chain=1)),
         ("persist", 60, 64, dict(cu_wide=1, chain=2)),
         ("team", 1024, 8, dict(team=8, chain=0)),
         ("team_persist", 1024, 8, dict(team=8, chain=2))]


def _pair(ea, n, E, opts):
    cfg = ea.EnvConfig(number_of_pedestrians=n, max_timesteps=40, is_new_exiting_reward=True)
    wrap = ea.EnvWrappersConfig(positions="grav", alpha=3)
    plain = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=11, options=ea.KernelOptions(cu_wide=0, team=0, workspace=False))
    env = ea.BatchedEvacuationEnv(cfg, wrap, num_envs=E, seed=11, options=ea.KernelOptions(**opts))
    ro = env.resolved_options()
    assert ro.parts == opts.get("parts", 1) and ro.chain == opts["chain"], ro
    if opts.get("team"):
        assert "CUs/env" in env.kernel_variant("rollout"), env.kernel_variant("rollout")
    plain.reset(); env.reset()
    return plain, env


def _calls(env, outs):
    """CALLS rollout launches with nothing waiting between them (in flight on the handle's own streams where it has them)."""
    for o in outs:
        env.rollout_launcher(T, o)()


def _outs(env, torch):
    return [{"slab": torch.empty((T, env.num_envs, env.obs_dim + 3), device=env.device)} for _ in range(CALLS)]


def _same(torch, a, b, what):
    for j, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x["slab"].view(torch.int32), y["slab"].view(torch.int32)), (what, j)


def _rebind(ea, env, fresh):
    """evac_bind_state to fresh tensors (the handle's own launches may still be in flight: the call settles them first)."""
    from evacuation_amd import _lib
    from evacuation_amd.vector_env import _ptr
    for k in STATE:
        setattr(env, k, fresh[k])
    _lib.check(env.lib.evac_bind_state(env._h, *[_ptr(fresh[k]) for k in STATE]), env._h)


@pytest.mark.parametrize("name,n,E,opts", FORMS, ids=[f[0] for f in FORMS])
def test_checkpoint_copied_after_join_is_the_state(ea, name, n, E, opts):
    import torch
    plain, env = _pair(ea, n, E, opts)
    ckpt = {k: getattr(plain, k).clone() for k in STATE}
    a, b = _outs(plain, torch), _outs(env, torch)
    _calls(plain, a); _calls(env, b)
    env.join()
    for e in (plain, env):                         # (after the join, on the stream the join made wait)
        for k in STATE:
            getattr(e, k).copy_(ckpt[k])
    c, d = _outs(plain, torch), _outs(env, torch)
    _calls(plain, c); _calls(env, d)
    env.join()
    torch.cuda.synchronize()
    assert env.team_error(sync=False) == 0
    _same(torch, a, b, "before the checkpoint")
    _same(torch, c, d, "after the checkpoint")
    _same(torch, a, d, "the checkpoint replayed")
    for k in STATE:
        assert torch.equal(getattr(plain, k), getattr(env, k)), k
    plain.close(); env.close()


@pytest.mark.parametrize("name,n,E,opts", FORMS, ids=[f[0] for f in FORMS])
def test_state_rebound_between_calls_is_the_state(ea, name, n, E, opts):
    import torch
    plain, env = _pair(ea, n, E, opts)
    ckpt = {k: getattr(plain, k).clone() for k in STATE}
    a, b = _outs(plain, torch), _outs(env, torch)
    _calls(plain, a); _calls(env, b)
    for e in (plain, env):                         # (no join: the rebind settles the launches in flight by itself)
        _rebind(ea, e, {k: v.clone() for k, v in ckpt.items()})
    c, d = _outs(plain, torch), _outs(env, torch)
    _calls(plain, c); _calls(env, d)
    env.join()
    torch.cuda.synchronize()
    assert env.team_error(sync=False) == 0
    _same(torch, a, b, "before the rebind")
    _same(torch, c, d, "after the rebind")
    _same(torch, a, d, "the checkpoint replayed")
    for k in STATE:
        assert torch.equal(getattr(plain, k), getattr(env, k)), k
    plain.close(); env.close()


@pytest.mark.parametrize("name,n,E,opts", FORMS, ids=[f[0] for f in FORMS])
def test_clear_error_on_a_clean_handle_between_calls_changes_nothing(ea, name, n, E, opts):
    import torch
    plain, env = _pair(ea, n, E, opts)
    own = env.own_streams
    variant = env.kernel_variant("rollout")
    a, b = _outs(plain, torch), _outs(env, torch)
    _calls(plain, a); _calls(env, b)
    env.team_clear_error()                         # (no error: the handle keeps its form and its streams)
    assert env.lib.evac_own_streams(env._h) == own and env.kernel_variant("rollout") == variant
    c, d = _outs(plain, torch), _outs(env, torch)
    _calls(plain, c); _calls(env, d)
    env.join()
    torch.cuda.synchronize()
    assert env.team_error(sync=False) == 0
    _same(torch, a + c, b + d, "around the clear")
    for k in STATE:
        assert torch.equal(getattr(plain, k), getattr(env, k)), k
    plain.close(); env.close()
