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


def test_the_gradient_entries_signatures_are_the_literal_lists():
    pol, lc, grads = C.POINTER(_lib.EvacMlpPolicy), C.POINTER(_lib.EvacRpoLossConfig), C.POINTER(_lib.EvacMlpPolicyGrads)
    sig = _lib.SIGNATURES
    for kind in ("rpo", "deepsets", "transformer"):
        assert sig[f"evac_{kind}_workspace_bytes"] == (C.c_int64, [C.c_int32, C.c_int64])
    assert sig["evac_rpo_minibatch_grad"] == (
        C.c_int, [pol, lc, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_uint64, C.c_uint64, grads, _P, _P, _P])
    assert sig["evac_deepsets_minibatch_grad"] == (
        C.c_int, [pol, C.POINTER(_lib.EvacDeepSets), lc, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_uint64, C.c_uint64,
                  grads, C.POINTER(_lib.EvacDeepSetsGrads), _P, _P, _P])
    assert sig["evac_transformer_minibatch_grad"] == (
        C.c_int, [pol, C.POINTER(_lib.EvacTransformer), lc, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_uint64, C.c_uint64,
                  grads, C.POINTER(_lib.EvacTransformerGrads), _P, _P, _P])
    assert sig["evac_rpo_minibatch_step"] == (
        C.c_int, [pol, lc, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_uint64, C.c_uint64, grads, _P, _P, _P, grads,
                  C.POINTER(_lib.EvacAdamState), C.POINTER(_lib.EvacAdamConfig)])
    assert sig["evac_deepsets_minibatch_step"] == (
        C.c_int, [pol, C.POINTER(_lib.EvacDeepSets), lc, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_uint64, C.c_uint64,
                  grads, C.POINTER(_lib.EvacDeepSetsGrads), _P, _P, _P, grads, C.POINTER(_lib.EvacDeepSetsGrads),
                  C.POINTER(_lib.EvacDeepSetsAdamState), C.POINTER(_lib.EvacAdamConfig)])
    # ... and an encoder's form is the linear form with the encoder after the policy and its gradients after the policy's
    linear = sig["evac_rpo_minibatch_grad"][1]
    for kind, enc, enc_grads in (("deepsets", _lib.EvacDeepSets, _lib.EvacDeepSetsGrads),
                                 ("transformer", _lib.EvacTransformer, _lib.EvacTransformerGrads)):
        assert sig[f"evac_{kind}_minibatch_grad"][1] == linear[:1] + [C.POINTER(enc)] + linear[1:15] + [C.POINTER(enc_grads)] + linear[15:]
    assert linear[0] == pol and linear[14] == grads


def test_the_kind_table_names_the_gradient_entries_and_structs_used_today():
    from evacuation_amd import trainer
    torch.manual_seed(0)
    both = TransformerActorCritic(D, N)
    both.deep_sets = DeepSetsActorCritic(D, N).deep_sets
    cases = {  # net: (the sizer, the gradient entry, the encoder's gradients' struct, its .grad tensors)
        "linear": (LinearActorCritic(D), "evac_rpo_workspace_bytes", "evac_rpo_minibatch_grad", None, None),
        "deep_sets": (DeepSetsActorCritic(D, N), "evac_deepsets_workspace_bytes", "evac_deepsets_minibatch_grad", _lib.EvacDeepSetsGrads,
                      deepsets_tensors),
        "embedding": (TransformerActorCritic(D, N, num_blocks=1), "evac_transformer_workspace_bytes", "evac_transformer_minibatch_grad",
                      _lib.EvacTransformerGrads, transformer_tensors),
        "both": (both, "evac_transformer_workspace_bytes", "evac_transformer_minibatch_grad", _lib.EvacTransformerGrads,
                 transformer_tensors),
    }
    for name, (net, sizer, entry, struct, tensors) in cases.items():
        kind = encoder_kind(net)
        assert trainer._entry_name(kind, "workspace_bytes") == sizer and trainer._entry_name(kind, "minibatch_grad") == entry, name
        assert sizer in _lib.SIGNATURES and entry in _lib.SIGNATURES, name
        if struct is None:
            assert kind is None, name
            continue
        st = trainer.ensure_encoder_grads(net)
        assert type(st) is struct and st is trainer.ensure_encoder_grads(net), name                        # (one cache slot, kept)
        ptrs = [t.grad.data_ptr() for t in tensors(net)]
        if struct is _lib.EvacDeepSetsGrads:
            assert [getattr(st, f) for f, _ in struct._fields_] == ptrs, name
        else:
            fields = [f for f, _ in _lib.EvacTransformerBlockGrads._fields_]
            blocks = len(ptrs) // 16
            assert [getattr(st.blocks[b], f) for b in range(blocks) for f in fields] == ptrs, name
            assert all(getattr(st.blocks[b], f) is None for b in range(blocks, 2) for f in fields), name  # (a block not in use: NULL)
    assert trainer._entry_name(encoder_kind(cases["deep_sets"][0]), "minibatch_step") == "evac_deepsets_minibatch_step"
    assert trainer._entry_name(encoder_kind(cases["deep_sets"][0]), "update") == "evac_deepsets_update"
    assert trainer._entry_name(None, "minibatch_step") == "evac_rpo_minibatch_step" and trainer._entry_name(None, "update") == "evac_rpo_update"
    # the three grad_fn stay three function objects: the one-call tables compare by identity
    fns = (trainer._kernel_grad, trainer.deepsets_kernel_grad, trainer.transformer_kernel_grad)
    assert len({id(f) for f in fns}) == 3
    assert [fn for fn, _ in trainer._STEP_OF] == [fn for fn, _ in trainer._UPDATE_OF] == list(fns[:2])
