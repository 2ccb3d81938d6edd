"""GPU tests of the contract include/evac.h states for every training entry that takes a workspace -- "evac_*_workspace_bytes(..)
bytes, 16-byte aligned, contents irrelevant before and after" -- and of the memory behind the entries' outputs.

The workspace is a slice of EXACTLY the sizer's figure between two bands (tests/workspace_guard.WorkspaceGuard): a store past
the figure changes a band; a read before a write shows as a changed result once the slice is filled with 0xFF (NaN as float,
all-ones as ticket, -1 as index) or holds what an earlier, larger call left.  The outputs -- the parameters' ``.grad``, the
statistics rows, the optimiser's header and moments -- lie in buffers of canaries (``Guarded``).  Every comparison is bit for bit
against the same call on the product's own path (``trainer._call_buffers`` / ``population._update_population``: a ``torch.empty``
of the caching allocator).  The tests only make well-formed calls: no entry ever gets less than its sizer's figure.

  (a) the gradient entries of the three networks, five runs per shape (product path, 0x00, 0xFF, stale, 0xFF at the documented
      minimum alignment), at the smallest shapes at which the workspace's layout changes form;
  (b) the update entries (two epochs with a tail minibatch over the full one's layout) and, on the slice the update left, the
      one-step entries; the transformer's stopped epoch leaves the slice as the last running step left it;
  (c) the population, sweep and deep-sets population updates with ``workspace=`` the planted slice;
  (d) the linear gradient past kGradMaxParts x kGradSamplesPerWg samples against float64, by tests/test_gpu_trainer.py's method.

The layout figures every shape is there for (workgroups P, samples a workgroup, tiles, segments) are restated below from the
headers' constants and asserted per case."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import deepsets_grad_cases as DC
from tests import trainer_ref as R
from tests import transformer_grad_cases as TC
from tests.encoder_grad_cases import ROOT, all_tensors
from tests.test_gpu_deepsets_population import load_population as load_deepsets_population
from tests.test_gpu_deepsets_population import update_inputs
from tests.test_gpu_population import interleave, load_population
from tests.test_gpu_sweep import learner_cfg
from tests.test_gpu_trainer import assert_branch_shares, kernel_grad, stat_errors, tensor_errors
from tests.test_gpu_transformer_update import make_batch
from tests.trainer_cases import DEV, build_case, loss_cfg, make_net, same_bits
from tests.workspace_guard import Guarded, WorkspaceGuard

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ea():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import evacuation_amd
    return evacuation_amd


def kernel_constant(header, name):
    text = open(os.path.join(ROOT, "evacuation_amd", "csrc", header)).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


def ceil_div(a, b):
    return -(-a // b)


def parts_and_chunk(M, per_wg, most, tile=1):
    """P workgroups of ``chunk`` samples as rpo_shape / SetGrad::shape / TfGrad::shape cut a minibatch: one workgroup per
    ``per_wg`` samples, ``most`` at most, the samples spread evenly (the chunk rounded up to whole ``tile``s)."""
    p0 = min(max(ceil_div(M, per_wg), 1), most)
    chunk = ceil_div(ceil_div(M, p0), tile) * tile
    return ceil_div(M, chunk), chunk


def linear_layout(D, M):
    """evac_train.h: rpo_parts_upper and rpo_shape, the dW1 tiles and rpo_w1_segments."""
    c = lambda name: kernel_constant("evac_train.h", name)
    P, chunk = parts_and_chunk(M, c("kGradSamplesPerWg"), c("kGradMaxParts"))
    tiles = ceil_div(D, c("kW1Tile"))
    segments = max(1, min(128 // tiles, 32, ceil_div(M, 64)))
    return SimpleNamespace(P=P, chunk=chunk, last_wg=M - (P - 1) * chunk, tiles=tiles, last_tile=D - (tiles - 1) * c("kW1Tile"),
                           segments=segments, cap=c("kGradMaxParts") * c("kGradSamplesPerWg"))


def deepsets_layout(D, M):
    """evac_deepsets_train.h: set_parts, set_segments and SetGrad::shape, the dy tiles and the dW_r tiles."""
    c = lambda name: kernel_constant("evac_deepsets_train.h", name)
    P, chunk = parts_and_chunk(M, c("kSetSamplesPerWg"), c("kSetMaxParts"), c("kSetTile"))
    return SimpleNamespace(P=P, chunk=chunk, even_chunk=ceil_div(M, min(max(ceil_div(M, c("kSetSamplesPerWg")), 1), c("kSetMaxParts"))),
                           dy_tiles=ceil_div(M, c("kSetTile")), last_dy_tile=M - (ceil_div(M, c("kSetTile")) - 1) * c("kSetTile"),
                           r_tiles=ceil_div(D, c("kSetRTile")), segments=min(max(ceil_div(M, 64), 1), c("kSetMaxSegments")),
                           max_segments=c("kSetMaxSegments"), cap=c("kSetMaxParts") * c("kSetSamplesPerWg"))


def transformer_layout(D, dm, M):
    """evac_transformer_train.h: tfg_parts and TfGrad::shape."""
    c = lambda name: kernel_constant("evac_transformer_train.h", name)
    P, chunk = parts_and_chunk(M, c("kTfgSamplesPerWg"), c("kTfgMaxParts"))
    return SimpleNamespace(P=P, chunk=chunk, tokens=D // dm, cap=c("kTfgMaxParts") * c("kTfgSamplesPerWg"), max_parts=c("kTfgMaxParts"))


# ------------------------------------------------------------------------------------------------ the three networks
def _family(name, make, obs_dim, adam, plant_header):
    return SimpleNamespace(name=name, make=make, obs_dim=obs_dim, adam=adam, plant_header=plant_header,
                           sizer=f"evac_{name}_workspace_bytes", grad=f"{name}_minibatch_grad", step=f"{name}_minibatch_step",
                           update=f"{name}_update")


LINEAR = _family("rpo", lambda shape, seed: make_net(shape[0], seed=seed), lambda shape: shape[0], "DeviceAdam", True)
DEEPSETS = _family("deepsets", lambda shape, seed: DC.make_net(*shape, seed=seed), lambda shape: (shape[0] + 2) * shape[1], "DeviceAdam", True)
# (TransformerAdam takes no `storage`: its header and moments cannot be planted between canaries from a test, and are not)
TRANSFORMER = _family("transformer", lambda shape, seed: TC.make_net(*shape, seed=seed), lambda shape: (shape[0] + 2) * shape[1],
                      "TransformerAdam", False)


def workspace_bytes(fam, D, M):
    from evacuation_amd import _lib
    need = int(getattr(_lib.load(), fam.sizer)(D, M))
    assert need > 0, (fam.sizer, D, M, need)
    return need


def plant(net, guard):
    """``guard``'s slice as the workspace the trainer's entries keep for ``net`` (trainer._call_buffers takes one that is large
    enough as it is: asserted after the call by ``planted_still``)."""
    from evacuation_amd import trainer
    trainer._grad_state(net).workspace = guard.slice
    guard.snapshot()


def planted_still(net, guard):
    from evacuation_amd import trainer
    ws = trainer._grad_state(net).workspace
    return ws.data_ptr() == guard.slice.data_ptr() and ws.numel() == guard.n


def guard_outputs(net, stats_rows):
    """The parameters' ``.grad`` as views into one ``Guarded`` buffer, preset to 7.0 (trainer.ensure_grads keeps a contiguous
    float32 ``.grad`` of the right shape), and behind them ``stats_rows`` rows of 8 statistics preset to -7.0; returns (the
    buffer, the statistics [stats_rows, 8])."""
    ts = all_tensors(net)
    G = Guarded([np.full(tuple(p.shape), 7.0, np.float32) for p in ts] + [np.full(8 * stats_rows, -7.0, np.float32)])
    for p, v in zip(ts, G.views):
        p.grad = v.view(p.shape)
    return G, G.views[-1].view(stats_rows, 8)


# ------------------------------------------------------------------------------------------------ (a) the gradient entries
#             shape            M      norm_adv  the layout's figures the case is there for
GRAD_CASES = [
    (LINEAR, (1,), 1, 0, dict(P=1, chunk=1, tiles=1, last_tile=1, segments=1)),
    (LINEAR, (6,), 2, 1, dict(P=1, chunk=2, tiles=1, last_tile=6, segments=1)),
    (LINEAR, (13,), 63, 1, dict(P=1, tiles=2, last_tile=5, segments=1)),       # D a multiple of neither 4 nor 8; one segment
    # two workgroups: the samples are spread evenly (rpo_shape), 65 + 64 -- no minibatch leaves a workgroup one sample
    (LINEAR, (124,), 129, 1, dict(P=2, chunk=65, last_wg=64, tiles=16, segments=3)),
    (LINEAR, (396,), 65, 1, dict(P=1, tiles=50, last_tile=4, segments=2)),     # kTrainMaxObs
    (LINEAR, (6,), 16385, 1, dict(P=128, chunk=129, last_wg=2, segments=32)),  # P at its cap, 129 samples a workgroup
    (DEEPSETS, (1, 2), 1, 0, dict(P=1, chunk=8, dy_tiles=1, r_tiles=1, segments=1)),
    (DEEPSETS, (10, 3), 9, 1, dict(P=1, dy_tiles=2, last_dy_tile=1, segments=1)),          # one full dy tile plus one sample
    (DEEPSETS, (31, 2), 33, 1, dict(P=2, chunk=24, r_tiles=2, segments=1)),
    (DEEPSETS, (64, 6), 65, 1, dict(P=3, chunk=24, r_tiles=7, segments=2)),                # D = 396, seven dW_r tiles
    (DEEPSETS, (10, 3), 16385, 1, dict(P=410, even_chunk=33, chunk=40, segments=32)),      # the chunk rounded up to whole tiles
    (TRANSFORMER, (1, 2, 1, False), 1, 0, dict(P=1, chunk=1, tokens=3)),       # one block in a workspace sized for two
    (TRANSFORMER, (10, 3, 2, False), 33, 1, dict(P=2, chunk=17, tokens=12)),
    (TRANSFORMER, (62, 6, 2, True), 65, 1, dict(P=3, chunk=22, tokens=64)),
    (TRANSFORMER, (10, 3, 2, True), 16385, 1, dict(P=497, chunk=33, tokens=12)),
]
RUNS = ("0x00", "0xFF", "stale", "0xFF at offset 16")


def layout_of(fam, shape, M):
    D = fam.obs_dim(shape)
    if fam is LINEAR:
        return linear_layout(D, M)
    return deepsets_layout(D, M) if fam is DEEPSETS else transformer_layout(D, shape[1], M)


def test_the_gradient_cases_are_the_shapes_at_which_the_layout_changes_form():
    """Every figure of the table, from the headers' constants; and the reasons behind the largest shapes."""
    for fam, shape, M, norm_adv, figures in GRAD_CASES:
        L = layout_of(fam, shape, M)
        for k, v in figures.items():
            assert getattr(L, k) == v, (fam.name, shape, M, k, getattr(L, k), v)
        if M == 16385:
            assert M == L.cap + 1 and 2 * M + 7 > L.cap                       # past the cap, and so is the stale run's larger call
    assert kernel_constant("evac_train.h", "kTrainMaxObs") == 396 and kernel_constant("evac_train.h", "kGradMaxParts") == 128
    assert linear_layout(396, 65).tiles == (396 + 7) // 8 and linear_layout(13, 63).last_tile % 4 != 0
    assert deepsets_layout(396, 65).r_tiles == (396 + 63) // 64 and deepsets_layout(36, 16385).segments == deepsets_layout(36, 16385).max_segments
    assert deepsets_layout(36, 16385).P < kernel_constant("evac_deepsets_train.h", "kSetMaxParts")     # (whole tiles need fewer workgroups)
    assert transformer_layout(36, 3, 16385).P < transformer_layout(36, 3, 16385).max_parts == 512
    assert transformer_layout(384, 6, 65).tokens == 64
    assert [c[0].name for c in GRAD_CASES].count("rpo") == 6 and len(GRAD_CASES) == 15
    assert {(c[0].name, c[3]) for c in GRAD_CASES if c[2] == 1} == {("rpo", 0), ("deepsets", 0), ("transformer", 0)}


@pytest.mark.parametrize("case", range(len(GRAD_CASES)), ids=[f"{c[0].name}-{'x'.join(map(str, map(int, c[1])))}-M{c[2]}" for c in GRAD_CASES])
def test_gradient_entries_need_the_sizers_bytes_and_nothing_of_their_contents(ea, case):
    """One network and one batch per case, the perturbation injected in the even cases and drawn on the device in the odd ones;
    five runs.  Run 1 is the product path.  Runs 2-5 get a planted slice of exactly the sizer's figure -- filled with 0x00, with
    0xFF, STALE (a 0xFF slice sized for 2 M + 7 samples runs that larger call first; the case's own M then runs in a slice of its
    own exact size at the front of the same buffer, not refilled), and 0xFF starting 16 bytes past a 4096-byte boundary -- with
    the ``.grad`` tensors (preset to 7.0) and the statistics row in a buffer of canaries.  In every run: all gradients and the 8
    statistics are run 1's bits, nothing outside the slice changed, the canaries are intact, every gradient is finite."""
    import torch
    from evacuation_amd import trainer
    fam, shape, M, norm_adv, _ = GRAD_CASES[case]
    D = fam.obs_dim(shape)
    cfg = loss_cfg(norm_adv, 1, 0.01, 0.5)
    entry = getattr(trainer, fam.grad)
    net = fam.make(shape, seed=11 + case)
    B = M + 3
    batch = make_batch(net, B, seed=case)
    assert batch["b_obs"].shape == (B, D)
    gen = torch.Generator().manual_seed(100 + case)
    inds = torch.randint(0, B, (M,), generator=gen).to(DEV)
    larger = torch.randint(0, B, (2 * M + 7,), generator=gen).to(DEV)
    z = ((torch.rand(M, 2, generator=gen) * 2 - 1) * cfg.rpo_alpha).to(DEV).contiguous() if case % 2 == 0 else None
    kw = dict(rpo_noise=z, seed=0x1234567890ABCDEF, draw_counter=(7 << 32) + 5)
    tensors = all_tensors(net)
    if fam is TRANSFORMER and shape[2] == 1:                                  # the second block's gradient pointers stay NULL
        assert len(tensors) == 29
        assert all(getattr(trainer.ensure_encoder_grads(net).blocks[1], f) is None for f in TC.BLOCK_NAMES)
    # run 1: the product path
    stats = entry(net, batch, inds, cfg, **kw)
    torch.cuda.synchronize()
    want, want_stats = [p.grad.detach().clone() for p in tensors], stats.clone()
    assert all(bool(torch.isfinite(g).all()) for g in want) and bool(torch.isfinite(want_stats).all())
    assert any(float(g.abs().max()) > 0 for g in want)
    need, need_larger = workspace_bytes(fam, D, M), workspace_bytes(fam, D, 2 * M + 7)
    assert need_larger > need
    for run in RUNS:
        G, row = guard_outputs(net, 1)
        if run == "stale":
            guard = WorkspaceGuard(need_larger, fill=0xFF)
            plant(net, guard)
            entry(net, batch, larger, cfg, seed=3, draw_counter=9, stats=row[0])
            torch.cuda.synchronize()
            assert planted_still(net, guard)
            guard.assert_outside_unchanged((fam.name, shape, M, "the stale run's larger call"))
            assert G.canaries_intact()
            assert not bool((guard.slice == 0xFF).all())                      # dirtied
            guard.replant(need)
            for v in G.views:
                v.fill_(7.0)
        else:
            guard = WorkspaceGuard(need, fill=0x00 if run == "0x00" else 0xFF, offset=16 if run.endswith("16") else 0)
        assert guard.slice.numel() == need and guard.slice.data_ptr() % 32 == (16 if run.endswith("16") else 0)
        plant(net, guard)
        out = entry(net, batch, inds, cfg, stats=row[0], **kw)
        torch.cuda.synchronize()
        what = (fam.name, shape, M, run)
        assert planted_still(net, guard) and out.data_ptr() == row.data_ptr(), what
        assert not bool((guard.slice == (0x00 if run == "0x00" else 0xFF)).all()), what      # the kernels did work in the slice
        names = R.NAMES + tuple(f"encoder[{i}]" for i in range(len(tensors) - 13))
        for name, p, g, view in zip(names, tensors, want, G.views):
            assert p.grad.data_ptr() == view.data_ptr(), (what, name)
            assert bool(torch.isfinite(p.grad).all()), (what, name)
            assert same_bits(p.grad, g), (what, name, int((p.grad != g).sum()))
        assert same_bits(row[0], want_stats), (what, row[0].tolist(), want_stats.tolist())
        guard.assert_outside_unchanged(what)
        assert G.canaries_intact(), what


# ------------------------------------------------------------------------------------------------ (b) the step and update entries
UPDATE_SHAPES = [(LINEAR, (13,)), (DEEPSETS, (10, 3)), (TRANSFORMER, (10, 3, 2, False))]
B_UPDATE, M_UPDATE, EPOCHS = 70, 32, 2
HEADER = ("t", "P1", "P2", "stop", "steps_run", "epochs_run")


def make_adam(fam, net, lr=1e-3):
    """The family's optimiser; for ``DeviceAdam`` with the 64-byte header and both moments of every tensor in a ``Guarded`` buffer
    (``storage=``).  Returns (the optimiser, the buffer or None)."""
    import torch
    from evacuation_amd import trainer
    if not fam.plant_header:
        return getattr(trainer, fam.adam)(net, lr=lr), None
    ts = list(all_tensors(net))
    zeros = [np.zeros(tuple(p.shape), np.float32) for p in ts]
    G = Guarded([np.zeros(16, np.float32)] + zeros + zeros)
    n = len(ts)
    moments = [v.view(p.shape) for v, p in zip(G.views[1:], ts + ts)]
    opt = trainer.DeviceAdam(net, lr=lr, storage=(G.views[0].view(torch.int64), moments[:n], moments[n:]))
    assert opt.header.data_ptr() == G.ptrs()[0] and opt.header.numel() == 8
    return opt, G


def state_of(net, opt, stats):
    import torch
    torch.cuda.synchronize()
    ts = all_tensors(net)
    return SimpleNamespace(params=[p.detach().clone() for p in ts], grads=[p.grad.detach().clone() for p in ts],
                           m=[t.clone() for t in opt.exp_avg], v=[t.clone() for t in opt.exp_avg_sq], header=opt.read_header(),
                           stats=stats.clone())


def assert_same_state(a, b, what, header=HEADER):
    for name in ("params", "m", "v", "grads"):
        for i, (x, y) in enumerate(zip(getattr(a, name), getattr(b, name))):
            assert same_bits(x, y), (what, name, i, int((x != y).sum()))
    for k in header:
        assert a.header[k] == b.header[k], (what, k, a.header, b.header)
    assert same_bits(a.stats, b.stats), (what, a.stats.tolist(), b.stats.tolist())


def update_case(fam, shape, seed):
    import torch
    cfg = loss_cfg(1, 1, 0.01, 0.5)
    batch = make_batch(fam.make(shape, seed=seed), B_UPDATE, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    perms = torch.stack([torch.randperm(B_UPDATE, generator=gen) for _ in range(EPOCHS)]).to(DEV)
    return cfg, batch, perms


@pytest.mark.parametrize("fam,shape", UPDATE_SHAPES, ids=[f[0].name for f in UPDATE_SHAPES])
def test_update_and_step_entries_need_the_sizers_bytes_and_nothing_of_their_contents(ea, fam, shape):
    """B = 70, M = 32, two epochs, norm_adv: every epoch ends in a tail of 6 samples, whose layout (the offsets depend on m) lies
    over what the full minibatches left, and the second epoch's full minibatches over what the tail left.  Twin networks and twin
    optimisers from the same start: one run on the product path, then a 0x00 slice, a 0xFF slice and a 0xFF slice 16 bytes past a
    4096-byte boundary, each of exactly the sizer's figure at (D, 32).  After the update, one ``*_minibatch_step`` of 32 samples
    on the slice as the update left it.  The statistics [steps + 1][8], the ``.grad`` tensors and, for ``DeviceAdam``, the 64-byte
    header and the moments lie between canaries; ``TransformerAdam`` takes no ``storage``, so its header and moments are its own
    allocations and only compared.  Equal across the runs, after the update and after the step: parameters, both moments,
    clipped gradients, the header's six fields, the statistics."""
    import torch
    from evacuation_amd import trainer
    D = fam.obs_dim(shape)
    cfg, batch, perms = update_case(fam, shape, seed=31)
    sizes = trainer.update_steps(B_UPDATE, M_UPDATE, True)
    assert sizes == [32, 32, 6]
    steps = EPOCHS * len(sizes)
    need = workspace_bytes(fam, D, M_UPDATE)
    assert workspace_bytes(fam, D, 6) < need
    update, step = getattr(trainer, fam.update), getattr(trainer, fam.step)
    step_inds = perms[1, 3:3 + M_UPDATE].contiguous()
    want = start = None
    for run in ("product path", "0x00", "0xFF", "0xFF at offset 16"):
        net = fam.make(shape, seed=31)
        opt, opt_guard = make_adam(fam, net)
        start = start or [p.detach().clone() for p in all_tensors(net)]
        assert all(same_bits(p, q) for p, q in zip(all_tensors(net), start)) and opt.read_header()["t"] == 0     # twins
        if run == "product path":
            guard, G, rows = None, None, torch.full((steps + 1, 8), -7.0, device=DEV)
        else:
            guard = WorkspaceGuard(need, fill=0x00 if run == "0x00" else 0xFF, offset=16 if run.endswith("16") else 0)
            G, rows = guard_outputs(net, steps + 1)
            plant(net, guard)
        what = (fam.name, shape, run)
        out, header = update(net, batch, perms, cfg, opt, seed=11, first_draw_counter=1000, stats=rows[:steps], minibatch_size=M_UPDATE)
        after_update = state_of(net, opt, rows[:steps])
        assert out.data_ptr() == rows.data_ptr() and header is opt.header
        h = after_update.header
        assert (h["steps_run"], h["epochs_run"], h["stop"], h["t"]) == (steps, EPOCHS, 0, steps), (what, h)
        step(net, batch, step_inds, cfg, opt, seed=11, draw_counter=77, stats=rows[steps])
        after_step = state_of(net, opt, rows)
        assert after_step.header["t"] == steps + 1 and not bool((rows == -7.0).any()), what
        assert all(bool(torch.isfinite(p).all()) for p in after_step.params), what
        if guard is None:
            want = (after_update, after_step)
            continue
        assert planted_still(net, guard) and not bool((guard.slice == guard.slice[0]).all()), what
        guard.assert_outside_unchanged(what)
        assert G.canaries_intact() and (opt_guard is None or opt_guard.canaries_intact()), what
        assert_same_state(after_update, want[0], what + ("update",))
        assert_same_state(after_step, want[1], what + ("step",))


def test_a_stopped_epoch_leaves_the_workspace_as_the_last_running_step_left_it(ea):
    """transformer_update with target_kl = 0.0 on a 0xFF slice: approx_kl > 0 once a step has moved the parameters, so the call
    stops after its first epoch and every kernel of the second returns at its gate.  The whole buffer -- bands AND slice -- must
    then be, byte for byte, what a one-epoch update of a twin left in a buffer of its own; parameters, moments, clipped gradients
    and the statistics rows likewise, and the rows of the stopped epoch keep their sentinel."""
    import torch
    from evacuation_amd import trainer
    fam, shape = TRANSFORMER, (10, 3, 2, False)
    D = fam.obs_dim(shape)
    cfg, batch, perms = update_case(fam, shape, seed=32)
    stopping = loss_cfg(1, 1, 0.01, 0.5)
    stopping.target_kl = 0.0
    per_epoch = 3
    need = workspace_bytes(fam, D, M_UPDATE)
    ran = []
    for c, p in ((cfg, perms[:1].contiguous()), (stopping, perms)):
        net = fam.make(shape, seed=32)
        opt, _ = make_adam(fam, net)
        guard = WorkspaceGuard(need, fill=0xFF)
        G, rows = guard_outputs(net, EPOCHS * per_epoch)
        plant(net, guard)
        trainer.transformer_update(net, batch, p, c, opt, seed=11, first_draw_counter=1000, stats=rows[:p.shape[0] * per_epoch],
                                   minibatch_size=M_UPDATE)
        state = state_of(net, opt, rows[:per_epoch])
        assert planted_still(net, guard)
        guard.assert_outside_unchanged(("target_kl", c.target_kl))
        assert G.canaries_intact()
        ran.append((state, guard, rows.clone()))
    (one, guard_one, _), (stopped, guard_stopped, rows_stopped) = ran
    assert (one.header["steps_run"], one.header["epochs_run"], one.header["stop"]) == (per_epoch, 1, 0), one.header
    assert (stopped.header["steps_run"], stopped.header["epochs_run"], stopped.header["stop"]) == (per_epoch, 1, 1), stopped.header
    assert float(stopped.stats[per_epoch - 1, 5]) > 0.0
    assert_same_state(stopped, one, "stopped epoch", header=("t", "P1", "P2", "steps_run", "epochs_run"))
    assert bool((rows_stopped[per_epoch:] == -7.0).all())
    assert not bool((guard_one.slice == 0xFF).all())
    differs = torch.nonzero(guard_stopped.buf != guard_one.buf).reshape(-1)
    assert differs.numel() == 0, (int(differs.numel()), (differs[:16] - 4096).tolist())


# ------------------------------------------------------------------------------------------------ (c) the populations
def population_state(pop, popt, stats):
    import torch
    torch.cuda.synchronize()
    return SimpleNamespace(tensors=[t.clone() for t in pop.tensors], grads=[t.clone() for t in pop.grads],
                           m=[t.clone() for t in popt.exp_avg], v=[t.clone() for t in popt.exp_avg_sq], headers=popt.headers.clone(),
                           stats=stats.clone())


def assert_same_population(a, b, what):
    for name in ("tensors", "m", "v", "grads"):
        for i, (x, y) in enumerate(zip(getattr(a, name), getattr(b, name))):
            assert same_bits(x, y), (what, name, i, [int((x[s] != y[s]).sum()) for s in range(x.shape[0])])
    assert same_bits(a.headers, b.headers), what
    assert same_bits(a.stats, b.stats), what


POPULATION_RUNS = ((None, 0), (0x00, 0), (0xFF, 0), (0xFF, 16))
B_L, E_L, M_POP, POP_EPOCHS = 70, 2, 33, 2


def population_runs(make, update, cfg, common, rows, S, D, seeds, deepsets, what):
    """``update`` from the same start without ``workspace=`` and with a planted slice of exactly population_workspace_bytes per
    fill and offset of ``POPULATION_RUNS``: every learner's parameters, moments, clipped gradients, header and statistics rows
    equal, nothing outside the slice changed."""
    import torch
    from evacuation_amd import population, trainer
    sizes = trainer.update_steps(B_L, M_POP, True)
    assert sizes == [33, 33, 4]
    steps = POP_EPOCHS * len(sizes)
    need = population.population_workspace_bytes(D, M_POP, S, deepsets=deepsets)
    firsts = [1000 + 37 * s for s in range(S)]
    want = None
    for fill, offset in POPULATION_RUNS:
        pop, popt = make()
        stats = torch.full((S, steps, 8), -7.0, device=DEV)
        kw = {}
        if fill is not None:
            guard = WorkspaceGuard(need, fill=fill, offset=offset)
            assert guard.slice.numel() == need
            guard.snapshot()
            kw["workspace"] = guard.slice
        update(pop, common, rows, cfg, popt, minibatch_size=M_POP, seeds=seeds, first_draw_counters=firsts, stats=stats, **kw)
        got = population_state(pop, popt, stats)
        heads = popt.read_headers()
        assert all((h["steps_run"], h["epochs_run"], h["stop"], h["t"]) == (steps, POP_EPOCHS, 0, steps) for h in heads), heads
        assert not bool((stats == -7.0).any()) and all(bool(torch.isfinite(t).all()) for t in got.tensors)
        if fill is None:
            want = got
            assert not same_bits(got.stats[0], got.stats[1])
            continue
        guard.assert_outside_unchanged(what + (hex(fill), offset))
        assert not bool((guard.slice == fill).all()), what                    # the kernels did work in the slice
        assert_same_population(got, want, what + (hex(fill), offset))


@pytest.mark.parametrize("sweep", [False, True], ids=["rpo_update_population", "sweep"])
def test_linear_population_updates_need_the_sizers_bytes_and_nothing_of_their_contents(ea, sweep):
    """evac_rpo_update_population (one configuration) and evac_rpo_update_sweep (one per learner): S = 3, D = 13, B_l = 70 in
    minibatches of 33, 33 and a tail of 4, two epochs.  include/evac.h asks 16 bytes of alignment of both entries' workspace (the
    learners' slices are whole multiples of 128 bytes FROM the base), so the 0xFF slice is also run 16 bytes past a 4096-byte
    boundary.  The learners' slices are packed: a learner that writes into its neighbour's slice changes no band -- it shows only
    as a changed result of the neighbour, which the comparison with the run without ``workspace=`` holds bit for bit."""
    import torch
    from evacuation_amd import population
    S, D = 3, 13
    cfgs = [learner_cfg(s, 1, 1) for s in range(S)]
    cfg = cfgs if sweep else loss_cfg(1, 1, 0.01, 0.5)
    seeds = [900 + 13 * s for s in range(S)]
    nets = [make_net(D, seed=60 + s) for s in range(S)]
    batches = [make_batch(net, B_L, seed=70 + s) for s, net in enumerate(nets)]
    common = interleave(batches, E_L)
    gen = torch.Generator().manual_seed(5)
    perms = torch.stack([torch.stack([torch.randperm(B_L, generator=gen) for _ in range(POP_EPOCHS)]) for _ in range(S)]).to(DEV)
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_L, S)
    assert population.population_workspace_bytes(D, M_POP, S) >= S * workspace_bytes(LINEAR, D, M_POP)

    def make():
        pop = load_population(ea, D, seeds, nets)
        if sweep:
            return pop, population.PopulationAdam(pop, lr=[c.learning_rate for c in cfgs], max_grad_norm=[c.max_grad_norm for c in cfgs])
        return pop, population.PopulationAdam(pop, lr=1e-3)
    population_runs(make, population.rpo_update_population, cfg, common, rows, S, D, seeds, False, ("sweep" if sweep else "population",))


def test_deepsets_population_update_needs_the_sizers_bytes_and_nothing_of_their_contents(ea):
    """evac_deepsets_update_population: S = 2, (N, ed) = (10, 3), B_l = 70 in minibatches of 33, 33 and a tail of 4, two epochs.
    include/evac.h asks 16 bytes of alignment of this workspace too -- every part of a learner's slice is a multiple of 256 bytes
    from the BASE, "whatever the base's alignment" -- so the 0xFF slice is also run 16 bytes past a 4096-byte boundary.  The
    slices and the common encoded batch behind them are packed: a learner writing into its neighbour's part shows only as a
    changed result, which the comparison with the run without ``workspace=`` holds bit for bit."""
    import torch
    from evacuation_amd import population
    S, N, ed = 2, 10, 3
    D, nets, batches, perms = update_inputs(N, ed, S, B_L, POP_EPOCHS, seed=81)
    seeds = [900 + 13 * s for s in range(S)]
    common = interleave(batches, E_L)
    rows = population.population_rows(perms, torch.arange(S, device=DEV).reshape(S, 1, 1), E_L, S)
    start = [[p.detach().clone() for p in all_tensors(n)] for n in nets]
    assert population.population_workspace_bytes(D, M_POP, S, deepsets=True) >= S * workspace_bytes(DEEPSETS, D, M_POP)

    def make():
        pop = load_deepsets_population(N, ed, seeds, start)
        return pop, population.PopulationAdam(pop, lr=1e-3)
    population_runs(make, population.deepsets_update_population, loss_cfg(1, 1, 0.01, 0.5), common, rows, S, D, seeds, True,
                    ("deepsets population",))


# ------------------------------------------------------------------------------------------------ (d) the linear gradient past its cap
def test_linear_gradient_past_its_cap_against_the_float64_yardstick(ea):
    """(D, M) = (6, 20000), strided, norm_adv and clip_vloss: past kGradMaxParts x kGradSamplesPerWg = 16 384 samples, so each of
    the 128 workgroups per net takes 157.  tests/test_gpu_trainer.py's method and bound: per tensor err = max|g - g64| / max|g64|,
    e32(case) = torch float32's own largest error on the same case, measured here; the kernel within 4 x e32(case) + 1e-7, the
    statistics the same way.  The printed line is in DESIGN.md's table of that suite's cases."""
    D, M, mode, norm_adv, clip_vloss, ent, alpha = 6, 20000, "strided", 1, 1, 0.01, 0.5
    L = linear_layout(D, M)
    assert M > L.cap == 16384 and (L.P, L.chunk) == (128, 157) and L.chunk > kernel_constant("evac_train.h", "kGradSamplesPerWg")
    cfg = loss_cfg(norm_adv, clip_vloss, ent, alpha)
    net, batch, inds, z, g64, s64, t = build_case(D, M, mode, cfg, seed=D + M)
    assert_branch_shares(t, cfg, M)
    assert batch["b_obs"].shape[0] == 2 * M + 3
    g32, s32, _ = R.minibatch_grad(net, batch, inds, cfg, z)                  # torch, float32, on the GPU
    gk, sk = kernel_grad(net, batch, inds, cfg, z)
    e32, ek = tensor_errors(g32, g64), tensor_errors(gk, g64)
    se32, sek = stat_errors(s32, s64), stat_errors(sk, s64)
    bound, sbound = 4 * max(e32) + 1e-7, 4 * max(se32) + 1e-7
    print(f"\ncase D={D} M={M} {mode} norm_adv={norm_adv} clip_vloss={clip_vloss} ent={ent} alpha={alpha}: e32(case) = {max(e32):.2e}, "
          f"bound {bound:.2e}, kernel {max(ek):.2e}; statistics e32 = {max(se32):.2e}, bound {sbound:.2e}, kernel {max(sek):.2e}")
    for name, a, b in zip(R.NAMES, e32, ek):
        print(f"  {name:13s} torch f32 {a:.2e}   kernel {b:.2e}")
    for name, a, b in zip(R.STATS, se32, sek):
        print(f"  {name:13s} torch f32 {a:.2e}   kernel {b:.2e}")
    assert all(math.isfinite(x) for x in ek + sek)
    for name, b in zip(R.NAMES, ek):
        assert b <= bound, (name, b, bound)
    for name, b in zip(R.STATS, sek):
        assert b <= sbound, (name, b, sbound)
