"""Writes tests/golden/transformer_forward.npz: the reference's OWN RPOTransformerEmbedding (src/agents/networks/
rpo_transformer_agent_network.py) in eval mode, run on the CPU -- its state_dict, eight observations, and embedding(x),
actor_mean(embedding(x)) and get_value(x) of them, for the CASES below.  Build container only (the reference lies beside the
repository there): `python tests/golden/make_transformer_forward.py`.  The reference's modules are imported by file path under a
stub `envs` that carries the two shapes the constructors read.  Nothing of the reference's text is copied here."""
import importlib.util
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

REFERENCE_ROOT = os.environ.get("EVAC_REFERENCE_ROOT", "/root/reference")
NETWORKS = os.path.join(REFERENCE_ROOT, "src", "agents", "networks")
# (number_of_pedestrians, floats per token, use_resid, num_blocks, num_hidden of the actor-critic): the kernels' width of 64 once
CASES = ((10, 6, False, 2, 16), (6, 3, False, 1, 16), (4, 2, False, 2, 64), (10, 6, True, 2, 16))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "transformer_forward.npz")


def tag_of(n_ped, dm, use_resid, num_blocks):
    return f"n{n_ped}_dm{dm}_r{int(use_resid)}_b{num_blocks}"


def load_networks():
    pkg = types.ModuleType("refnets")
    pkg.__path__ = [NETWORKS]
    sys.modules["refnets"] = pkg
    mods = {}
    for name in ("utils", "rpo_linear_agent_network", "rpo_transformer_agent_network"):
        spec = importlib.util.spec_from_file_location(f"refnets.{name}", os.path.join(NETWORKS, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods


def make_reference_net(mods, n_ped, dm, use_resid, num_blocks, hidden=64, dropout=0.1):
    lin, tf = mods["rpo_linear_agent_network"], mods["rpo_transformer_agent_network"]
    D = (n_ped + 2) * dm
    envs = SimpleNamespace(single_observation_space=SimpleNamespace(shape=(D,)), single_action_space=SimpleNamespace(shape=(2,)))
    cfg = tf.RPOTransformerEmbeddingConfig(network=lin.RPOLinearNetworkConfig(num_hidden=hidden), num_blocks=num_blocks,
                                           use_resid=use_resid, dropout=dropout)
    return tf.RPOTransformerEmbedding(envs, n_ped, cfg, torch.device("cpu"))


def main():
    mods = load_networks()
    out = {}
    for n_ped, dm, use_resid, num_blocks, hidden in CASES:
        D = (n_ped + 2) * dm
        # (the seeds' base: LayerNorm over 2 to 6 values divides by the spread of its input, and a draw that puts one token's
        # spread near zero -- easy at 2 values, after a first block whose outputs are close to +-weight + bias -- makes float32
        # and float64 incomparable.  With this base the smallest input variance of any norm over the recorded samples is 5.5e-3.)
        torch.manual_seed(5000 + 10 * n_ped + int(use_resid))
        net = make_reference_net(mods, n_ped, dm, use_resid, num_blocks, hidden).eval()
        with torch.no_grad():      # visible actions (a larger last actor layer, non-zero biases) and a LayerNorm affine that shows
            net.actor_mean[4].weight.mul_(60.0)
            for m in list(net.actor_mean) + list(net.critic):
                if isinstance(m, torch.nn.Linear):
                    m.bias.normal_(0.0, 0.2)
            for m in net.embedding.modules():
                if isinstance(m, torch.nn.LayerNorm):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.normal_(0.0, 0.3)
            x = torch.empty(8, D).uniform_(-1.0, 1.0)
            value = net.get_value(x)
            y = net.embedding(x)
            mean = net.actor_mean(y)
        tag = tag_of(n_ped, dm, use_resid, num_blocks)
        for k, v in net.state_dict().items():
            out[f"{tag}/sd/{k}"] = v.numpy().copy()
        out[f"{tag}/x"], out[f"{tag}/value"], out[f"{tag}/actor_mean"], out[f"{tag}/encoded"] = x.numpy(), value.numpy(), mean.numpy(), y.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
