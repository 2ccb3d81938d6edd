"""Writes tests/golden/deepsets_forward.npz: the reference's OWN RPODeepSetsEmbedding (src/agents/networks/
rpo_deep_sets_agent_network.py), run on the CPU -- its state_dict, eight observations, and get_value / actor_mean(encoder(x)) of
them, for N = 10 with 6 floats per element, N = 6 with 3 and N = 4 with 2 (CASES).  Build container only (the reference lies beside the
repository there): `python tests/golden/make_deepsets_forward.py`.  The reference's modules are imported by file path -- the
package __init__ above them needs the whole `src` tree on the path -- under a stub `envs` that carries the two shapes the
constructors read.  Nothing of the reference's text is copied here."""
import importlib.util
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

REFERENCE_ROOT = os.environ.get("EVAC_REFERENCE_ROOT", "/root/reference")
NETWORKS = os.path.join(REFERENCE_ROOT, "src", "agents", "networks")
# (number_of_pedestrians, floats per element, num_hidden of the actor-critic): the kernels' width of 64 once, 16 for the others --
# orthogonal 64 x 64 matrices do not compress, and the encoder under test is the same
CASES = ((10, 6, 16), (6, 3, 16), (4, 2, 64))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "deepsets_forward.npz")


def load_networks():
    pkg = types.ModuleType("refnets")
    pkg.__path__ = [NETWORKS]
    sys.modules["refnets"] = pkg
    mods = {}
    for name in ("utils", "rpo_linear_agent_network", "rpo_deep_sets_agent_network"):
        spec = importlib.util.spec_from_file_location(f"refnets.{name}", os.path.join(NETWORKS, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods


def main():
    mods = load_networks()
    lin, ds = mods["rpo_linear_agent_network"], mods["rpo_deep_sets_agent_network"]
    out = {}
    for n_ped, ed, hidden in CASES:
        D = (n_ped + 2) * ed
        torch.manual_seed(1000 + n_ped)
        envs = SimpleNamespace(single_observation_space=SimpleNamespace(shape=(D,)), single_action_space=SimpleNamespace(shape=(2,)))
        net = ds.RPODeepSetsEmbedding(envs, n_ped, ds.RPODeepSetsEmbeddingConfig(network=lin.RPOLinearNetworkConfig(num_hidden=hidden)), torch.device("cpu"))
        with torch.no_grad():      # visible actions: a larger last actor layer and non-zero biases (layer_init leaves them 0)
            net.actor_mean[4].weight.mul_(60.0)
            for m in list(net.actor_mean) + list(net.critic):
                if isinstance(m, torch.nn.Linear):
                    m.bias.normal_(0.0, 0.2)
            x = torch.empty(8, D).uniform_(-1.0, 1.0)
            value = net.get_value(x)
            y = net.deep_sets(x.view(8, -1, net.set_element_dim)).view(x.shape)
            mean = net.actor_mean(y)
        tag = f"n{n_ped}_ed{ed}"
        for k, v in net.state_dict().items():
            out[f"{tag}/sd/{k}"] = v.numpy().copy()
        out[f"{tag}/x"], out[f"{tag}/value"], out[f"{tag}/actor_mean"], out[f"{tag}/encoded"] = x.numpy(), value.numpy(), mean.numpy(), y.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
