"""What the tests of the deep-sets leader's gradient (tests/test_deepsets_grad_cpu.py, tests/test_gpu_deepsets_grad.py) build: the
yardstick and the branch-covering minibatch case.

The yardstick is the reference's minibatch loss on the module in a given dtype through torch autograd: tests/trainer_ref.py's
``loss_terms`` fed y = encode(x), the encoder element by element as tests/deepsets_ref.py states it (phi per element, then the
sum, then rho).  It runs in float64 (the truth) and in float32 (whose error against float64 sets every bound), on the device
the batch is on."""
from tests import encoder_grad_cases as G
from tests import trainer_ref as R
from tests.encoder_grad_cases import all_tensors, fake_trainer  # noqa: F401  (the test files reach them here)

DEV = "cuda:0"
ENCODER_NAMES = ("phi_w1", "phi_b1", "phi_w2", "phi_b2", "rho_w", "rho_b")
NAMES = R.NAMES + ENCODER_NAMES
RELU_MARGIN = 1e-5


def params_of(net, dtype=None, device=None):
    """The 19 tensors (``NAMES`` order) as fresh leaves that require grad."""
    return [t.detach().to(dtype=dtype or t.dtype, device=device or t.device).clone().requires_grad_(True) for t in all_tensors(net)]


def preact(P, x):
    """The encoder's first-layer pre-activations a_ik of observations x [M, D]: [M, S, 24]."""
    wa, ba = P[13], P[14]
    return x.reshape(x.shape[0], -1, wa.shape[1]) @ wa.T + ba


def encode(P, x):
    """tests/deepsets_ref.encode in torch: y = W_r sum_i (W_b relu(W_a x_i + b_a) + b_b) + b_r, element by element."""
    import torch
    wb, bb, wr, br = P[15:19]
    phi = torch.relu(preact(P, x)) @ wb.T + bb
    return phi.sum(dim=-2) @ wr.T + br


def loss_terms(P, batch, mb_inds, cfg, z):
    """trainer_ref.loss_terms with the network reading y = encode(x): the minibatch gathered first, then the linear network's
    loss on the encoded rows."""
    import torch
    gathered = {k: v[mb_inds] for k, v in batch.items()}
    gathered["b_obs"] = encode(P, gathered["b_obs"])
    return R.loss_terms(P[:13], gathered, torch.arange(mb_inds.shape[0], device=mb_inds.device), cfg, z)


def minibatch_grad(net, batch, mb_inds, cfg, z, dtype=None):
    """Gradients of the 19 tensors (list, ``NAMES`` order) and the 8 statistics of one minibatch, everything cast to ``dtype``
    (float32 by default) first, by autograd."""
    import torch
    dtype = dtype or torch.float32
    P = params_of(net, dtype)
    b = {k: v.to(dtype) for k, v in batch.items()}
    t = loss_terms(P, b, mb_inds, cfg, z.to(dtype))
    grads = torch.autograd.grad(t.loss, P)
    sumsq = sum((g.double() ** 2).sum() for g in grads).to(dtype)
    stats = torch.stack([t.loss.detach(), t.pg_loss.detach(), t.v_loss.detach(), t.entropy.detach(), t.old_approx_kl, t.approx_kl,
                         t.clipfrac, sumsq])
    return list(grads), stats, t


def make_net(N, ed, seed=0, device=DEV):
    """A deep-sets leader with visible means and values (tests/trainer_cases.make_net, tests/test_gpu_deepsets.make_net): the
    actor's head x 40, two different sigmas, non-zero biases, and an encoder whose output stays in the tanh layers' range
    whatever the number of elements (rho's weight x 3 / (N + 2))."""
    import torch
    from evacuation_amd.policy import DeepSetsActorCritic
    torch.manual_seed(seed)
    net = DeepSetsActorCritic((N + 2) * ed, N)
    with torch.no_grad():
        net.actor_mean[4].weight.mul_(40.0)
        net.actor_logstd.copy_(torch.tensor([[-0.4, 0.2]]))
        for seq in (net.actor_mean, net.critic):
            for i in (0, 2, 4):
                seq[i].bias.uniform_(-0.2, 0.2)
        net.deep_sets.transform_rho[0].weight.mul_(3.0 / (N + 2))
    return net.to(device)


def _encode_rows(P, obs, rows=4096):
    import torch
    with torch.no_grad():
        return torch.cat([encode(P, obs[i:i + rows]) for i in range(0, obs.shape[0], rows)])


def _near_relu(P, obs, rows=4096):
    """The batch rows with a first-layer pre-activation inside the margin of the relu's branch point."""
    import torch
    with torch.no_grad():
        return torch.cat([(preact(P, obs[i:i + rows]).abs() < RELU_MARGIN).flatten(1).any(dim=1) for i in range(0, obs.shape[0], rows)])


def build_case(N, ed, M, mode, cfg, seed, device=DEV, cache=True):
    """tests/trainer_cases.build_case's recipe behind the encoder: a batch whose minibatch takes every branch of the loss by a
    known share of its samples -- old log-probabilities and values set FROM the float64 forward pass (half of the rows inside
    each clip range, a quarter above, a quarter below), no sample within 1e-6 of a branch point of max / clamp -- and, the relu
    being a branch point too, no batch row with a first-layer pre-activation |a_ik| < 1e-5 in float64 (such rows are redrawn, at
    most 8 rounds; a flipped mask would move a dW_a entry by about 1 / (M S) of its scale).  Returns (net, batch, inds, z, the 19
    float64 gradients, the 8 float64 statistics, the yardstick's terms with ``relu_on``: the share of relu masks that are 1).
    ``cache``: the case is built once per process and shared (nobody changes it)."""
    import torch
    D = (N + 2) * ed

    def encode64(net, obs, g):
        P = [p.detach().cpu().double() for p in all_tensors(net)]
        G.redraw_rows(obs, g, lambda o: _near_relu(P, o.double()))          # the relu's branch point
        assert not bool(_near_relu(P, obs.double()).any()), "rows at the relu's branch point after 8 rounds"

        def attach(t, batch, inds):
            with torch.no_grad():
                P64 = [p.detach().double() for p in all_tensors(net)]
                t.relu_on = float((preact(P64, batch["b_obs"][inds].double()) > 0).double().mean())
        return P[:13], _encode_rows(P, obs.double()), attach
    return G.build_case(D, M, mode, cfg, seed, device, lambda: make_net(N, ed, seed=seed, device=device), encode64, minibatch_grad,
                        key=("deepsets", N, ed) if cache else None)


kernel_grad = G.kernel_grad_of("deepsets_minibatch_grad")
