"""The one place that answers "which encoder?" (policy.ENCODER_KINDS, encoder_kind, PolicyBinder.bind_encoder) and the four
encoder entries' ctypes signatures, without a GPU: the signatures are the literal lists they were written as, and a linear, a
deep-sets and a transformer network -- and a module with both attributes, which `embedding` decides -- get the same answer from
every helper."""
import ctypes as C

import torch

from evacuation_amd import _lib
from evacuation_amd.policy import (ENCODER_KINDS, DeepSetsActorCritic, LinearActorCritic, PolicyBinder, TransformerActorCritic,
                                   all_tensors, deepsets_tensors, encode_observation, encoder_kind, is_deepsets, is_transformer,
                                   mlp_tensors, transformer_tensors)

N, D = 10, 36
_P = C.c_void_p


def test_the_encoder_entries_signatures_are_the_literal_lists():
    pol = C.POINTER(_lib.EvacMlpPolicy)
    for suffix, struct in (("_deepsets", _lib.EvacDeepSets), ("_transformer", _lib.EvacTransformer)):
        assert _lib.SIGNATURES["evac_policy_rollout" + suffix] == (
            C.c_int, [_P, C.c_int32, pol, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float,
                      C.POINTER(struct), _P])
        assert _lib.SIGNATURES["evac_policy_evaluate" + suffix] == (
            C.c_int, [_P, C.c_int32, pol, C.c_int32, C.c_int32, _P, _P, _P, C.c_float, C.c_float, C.POINTER(struct), _P])
    # ... and each is the linear entry's list with the struct in front of the stream
    for what in ("rollout", "evaluate"):
        linear = _lib.SIGNATURES["evac_policy_" + what][1]
        assert _lib.SIGNATURES[f"evac_policy_{what}_deepsets"][1] == linear[:-1] + [C.POINTER(_lib.EvacDeepSets), _P]


def test_every_helper_gives_the_same_answer_in_todays_precedence():
    assert [(k.attr, k.suffix) for k in ENCODER_KINDS] == [("embedding", "_transformer"), ("deep_sets", "_deepsets")]
    torch.manual_seed(0)
    linear, sets, tf = LinearActorCritic(D), DeepSetsActorCritic(D, N), TransformerActorCritic(D, N)
    both = TransformerActorCritic(D, N)
    both.deep_sets = DeepSetsActorCritic(D, N).deep_sets
    binder = PolicyBinder(D, torch.device("cpu"), N)
    x = torch.randn(4, D)
    cases = {  # net: (kind's attribute, is_deepsets, is_transformer, the encoder's tensors, the struct's type)
        "linear": (linear, None, False, False, (), None),
        "deep_sets": (sets, "deep_sets", True, False, deepsets_tensors(sets), _lib.EvacDeepSets),
        "embedding": (tf, "embedding", False, True, transformer_tensors(tf), _lib.EvacTransformer),
        "both": (both, "embedding", True, True, transformer_tensors(both), _lib.EvacTransformer),
    }
    for name, (net, attr, sets_too, tf_too, tensors, struct) in cases.items():
        kind = encoder_kind(net)
        assert (None if kind is None else kind.attr) == attr, name
        assert (is_deepsets(net), is_transformer(net)) == (sets_too, tf_too), name
        got = all_tensors(net)
        assert len(got) == 13 + len(tensors) and all(a is b for a, b in zip(got, mlp_tensors(net) + tuple(tensors))), name
        bound = binder.bind_encoder(net)
        if attr is None:
            assert bound is None and encode_observation(net, x) is x, name
            continue
        suffix, st = bound
        assert suffix == kind.suffix and type(st) is struct, name
        assert st is (binder.transformer(net) if attr == "embedding" else binder.encoder(net)), name      # (one cache entry)
        with torch.no_grad():
            want = net.embedding(x) if attr == "embedding" else net.deep_sets(x.view(4, N + 2, -1)).view(4, D)
            assert torch.equal(encode_observation(net, x), want), name
    assert binder.bind_encoder(both)[1].blocks[0].wq == transformer_tensors(both)[0].data_ptr()
