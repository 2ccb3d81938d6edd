"""ctypes binding of libevac.so (include/evac.h).  There is NO CPU fallback: if the HIP library is
missing or cannot be loaded this module raises, and every op needs a visible MI355X."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# EVAC_LIB overrides the library path (builds of another tree for A/B runs: tools/ab_bench.sh, tools/chain_trace.sh)
LIB_PATH = os.environ.get("EVAC_LIB") or os.path.join(HERE, "libevac.so")

EVAC_OK = 0
ERR_INVALID_ARGUMENT, ERR_NOT_BOUND, ERR_UNSUPPORTED, ERR_HIP, ERR_NO_DEVICE, ERR_TEAM_ABORTED = -1, -2, -3, -4, -5, -6
POS = {"abs": 0, "rel": 1, "grav": 2}
STAT = {"no": 0, "ohe": 1, "cat": 2}
TYPE = {"Dict": 0, "Box": 1}
MAX_PEDESTRIANS = 1024
VERSION = 150
MAX_LEARNERS = 64              # EVAC_MAX_LEARNERS
EPISODE_STATS_WORDS = 10       # evac_episode_stats_t: 8 floats + 2 int32
AGENT_POLICY_MEAN, AGENT_POLICY_SAMPLE, AGENT_VACUUM_CLEANER = 0, 1, 2   # evac_policy_evaluate's agents


class EvacConfig(C.Structure):
    """evac_config_t"""
    _fields_ = [
        ("number_of_pedestrians", C.c_int32), ("width", C.c_float), ("height", C.c_float),
        ("step_size", C.c_float), ("noise_coef", C.c_float), ("eps", C.c_float),
        ("enslaving_degree", C.c_float), ("is_new_exiting_reward", C.c_int32),
        ("is_new_followers_reward", C.c_int32), ("intrinsic_reward_coef", C.c_float),
        ("is_termination_agent_wall_collision", C.c_int32), ("init_reward_each_step", C.c_float),
        ("max_timesteps", C.c_int32), ("positions", C.c_int32), ("statuses", C.c_int32),
        ("type", C.c_int32), ("alpha", C.c_float), ("nan_guard", C.c_int32), ("clip_action", C.c_int32),
    ]


class EvacOptions(C.Structure):
    """evac_options_t: which kernels a handle launches (never what they compute); -1 = automatic"""
    _fields_ = [(f, C.c_int32) for f in ("subwave", "cells", "cu_wide", "team", "specialize", "parts", "team_coop", "team_fault", "chain")]


class EvacMlpPolicy(C.Structure):
    """evac_mlp_policy_t: the actor-critic's tensors (torch layouts) for evac_policy_rollout"""
    _fields_ = [("obs_dim", C.c_int32), ("hidden", C.c_int32)] + [
        (f, C.c_void_p) for f in ("actor_w1", "actor_b1", "actor_w2", "actor_b2", "actor_w3", "actor_b3", "actor_logstd",
                                  "critic_w1", "critic_b1", "critic_w2", "critic_b2", "critic_w3", "critic_b3")]


class EvacDeepSets(C.Structure):
    """evac_deepsets_t: the set encoder's tensors (torch layouts) for evac_policy_rollout_deepsets / evac_policy_evaluate_deepsets"""
    _fields_ = [("set_elem_dim", C.c_int32), ("hidden", C.c_int32)] + [
        (f, C.c_void_p) for f in ("phi_w1", "phi_b1", "phi_w2", "phi_b2", "rho_w", "rho_b")]


class EvacTransformerBlock(C.Structure):
    """evac_transformer_block_t: one block's 16 tensors (torch layouts)"""
    _fields_ = [(f, C.c_void_p) for f in ("wq", "bq", "wk", "bk", "wv", "bv", "dense_w", "dense_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b",
                                          "norm1_w", "norm1_b", "norm2_w", "norm2_b")]


class EvacTransformer(C.Structure):
    """evac_transformer_t: the attention encoder for evac_policy_rollout_transformer / evac_policy_evaluate_transformer"""
    _fields_ = [(f, C.c_int32) for f in ("elem_dim", "num_blocks", "num_heads", "dim_feedforward", "use_resid")] + [
        ("ln_eps", C.c_float), ("blocks", EvacTransformerBlock * 2)]


class EvacEvalCapture(C.Structure):
    """evac_eval_capture_t: where evac_policy_evaluate*_capture record the frames of envs 0..capture_envs-1"""
    _fields_ = [("capture_envs", C.c_int32), ("max_frames", C.c_int32), ("frames", C.c_void_p), ("starts", C.c_void_p)]


class EvacDeepSetsGrads(C.Structure):
    """evac_deepsets_grads_t: where evac_deepsets_minibatch_grad writes the gradients of the encoder's six tensors"""
    _fields_ = [(f, C.c_void_p) for f, _ in EvacDeepSets._fields_[2:]]


class EvacTransformerBlockGrads(C.Structure):
    """evac_transformer_block_grads_t: where evac_transformer_minibatch_grad writes the gradients of one block's 16 tensors"""
    _fields_ = list(EvacTransformerBlock._fields_)


class EvacTransformerGrads(C.Structure):
    """evac_transformer_grads_t: the blocks' gradients (blocks at index num_blocks and above are never followed)"""
    _fields_ = [("blocks", EvacTransformerBlockGrads * 2)]


class EvacRpoLossConfig(C.Structure):
    """evac_rpo_loss_config_t"""
    _fields_ = [(f, C.c_float) for f in ("clip_coef", "ent_coef", "vf_coef", "rpo_alpha")] + [("norm_adv", C.c_int32), ("clip_vloss", C.c_int32)]


class EvacMlpPolicyGrads(C.Structure):
    """evac_mlp_policy_grads_t: where evac_rpo_minibatch_grad writes the gradients of the 13 tensors"""
    _fields_ = [(f, C.c_void_p) for f, _ in EvacMlpPolicy._fields_[2:]]


class EvacMlpPolicyStrides(C.Structure):
    """evac_mlp_policy_strides_t: floats from learner s to learner s + 1, per tensor of evac_mlp_policy_t"""
    _fields_ = [(f, C.c_int64) for f, _ in EvacMlpPolicy._fields_[2:]]


class EvacDeepSetsStrides(C.Structure):
    """evac_deepsets_strides_t: floats from learner s to learner s + 1, per tensor of evac_deepsets_t"""
    _fields_ = [(f, C.c_int64) for f, _ in EvacDeepSets._fields_[2:]]


class EvacTransformerBlockStrides(C.Structure):
    """evac_transformer_block_strides_t: floats from learner s to learner s + 1, per tensor of evac_transformer_block_t"""
    _fields_ = [(f, C.c_int64) for f, _ in EvacTransformerBlock._fields_]


class EvacTransformerStrides(C.Structure):
    """evac_transformer_strides_t: the blocks' strides (blocks at index num_blocks and above are never looked at)"""
    _fields_ = [("blocks", EvacTransformerBlockStrides * 2)]


class EvacAdamConfig(C.Structure):
    """evac_adam_config_t"""
    _fields_ = [(f, C.c_double) for f in ("lr", "beta1", "beta2", "eps", "max_grad_norm")]


class EvacAdamState(C.Structure):
    """evac_adam_state_t: the optimiser's header and moments (caller-owned device memory; all zero = a fresh optimiser)"""
    _fields_ = [("header", C.c_void_p), ("exp_avg", EvacMlpPolicyGrads), ("exp_avg_sq", EvacMlpPolicyGrads)]


class EvacDeepSetsAdamState(C.Structure):
    """evac_deepsets_adam_state_t: evac_adam_state_t with the set encoder's moments after the 13 tensors'"""
    _fields_ = EvacAdamState._fields_ + [("enc_exp_avg", EvacDeepSetsGrads), ("enc_exp_avg_sq", EvacDeepSetsGrads)]


class EvacTransformerAdamState(C.Structure):
    """evac_transformer_adam_state_t: evac_adam_state_t with the attention encoder's moments (16 per block) after the 13 tensors'"""
    _fields_ = EvacAdamState._fields_ + [("enc_exp_avg", EvacTransformerGrads), ("enc_exp_avg_sq", EvacTransformerGrads)]


class EvacLearnerHyper(C.Structure):
    """evac_learner_hyper_t: one learner's float-valued hyperparameters (a host array [S] for the sweep entries)"""
    _fields_ = [(f, C.c_double) for f in ("learning_rate", "target_kl", "gamma", "gae_lambda")] + [
        (f, C.c_float) for f in ("clip_coef", "ent_coef", "vf_coef", "rpo_alpha", "max_grad_norm")] + [("use_target_kl", C.c_int32)]


HYPER_DEFAULTS = {"learning_rate": 3e-4, "target_kl": None, "gamma": 0.99, "gae_lambda": 0.95, "clip_coef": 0.2, "ent_coef": 0.0,
                  "vf_coef": 0.5, "rpo_alpha": 0.5, "max_grad_norm": 0.5}   # RPOTrainingConfig's


def learner_hypers(n_learners: int, **columns):
    """``evac_learner_hyper_t[n_learners]`` (a host array) from columns named as ``HYPER_DEFAULTS``: each one value for all
    learners or a sequence of ``n_learners``; a ``target_kl`` of None means no target.  What is not given takes the default."""
    n = int(n_learners)
    unknown = set(columns) - set(HYPER_DEFAULTS)
    if unknown:
        raise ValueError(f"learner_hypers: unknown fields {sorted(unknown)}")
    if not 1 <= n <= MAX_LEARNERS:
        raise ValueError(f"learner_hypers: {n} learners; expected 1..{MAX_LEARNERS}")
    out = (EvacLearnerHyper * n)()
    for name, default in HYPER_DEFAULTS.items():
        col = columns.get(name, default)
        col = list(col) if isinstance(col, (list, tuple)) else [col] * n
        if len(col) != n:
            raise ValueError(f"learner_hypers: {name} has {len(col)} entries for {n} learners")
        for s, v in enumerate(col):
            if name == "target_kl":
                out[s].use_target_kl = int(v is not None)
                out[s].target_kl = float(v or 0.0)
            else:
                setattr(out[s], name, float(v))
    return out


class EvacError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libevac error {code}: {msg}")
        self.code = code


# Every symbol include/evac.h declares: name -> (restype, argtypes)
_P = C.c_void_p


def _grad_args(*encoder) -> list:
    """evac_rpo_minibatch_grad's arguments; with ``encoder`` = (its struct, its gradients' struct) an encoder's entry's."""
    enc, enc_grads = ([C.POINTER(s)] for s in encoder) if encoder else ([], [])
    return [C.POINTER(EvacMlpPolicy), *enc, C.POINTER(EvacRpoLossConfig), C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_uint64,
            C.c_uint64, C.POINTER(EvacMlpPolicyGrads), *enc_grads, _P, _P, _P]


SIGNATURES = {
    "evac_version": (C.c_int, []),
    "evac_status_string": (C.c_char_p, [C.c_int]),
    "evac_last_error": (C.c_char_p, [_P]),
    "evac_config_validate": (C.c_int, [C.POINTER(EvacConfig)]),
    "evac_config_obs_dim": (C.c_int64, [C.POINTER(EvacConfig)]),
    "evac_create": (C.c_int, [C.POINTER(EvacConfig), C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(_P)]),
    "evac_create_ex": (C.c_int, [C.POINTER(EvacConfig), C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(EvacOptions), C.POINTER(_P)]),
    "evac_get_options": (C.c_int, [_P, C.POINTER(EvacOptions)]),
    "evac_join": (C.c_int, [_P, _P]),
    "evac_order_next_rollout": (C.c_int, [_P]),
    "evac_num_parts": (C.c_int32, [_P]),
    "evac_own_streams": (C.c_int32, [_P]),
    "evac_part_stream": (_P, [_P, C.c_int32]),
    "evac_destroy": (C.c_int, [_P]),
    "evac_obs_dim": (C.c_int64, [_P]),
    "evac_num_envs": (C.c_int32, [_P]),
    "evac_kernel_variant": (C.c_char_p, [_P, C.c_int32]),
    "evac_bind_state": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "evac_workspace_bytes": (C.c_int64, [_P]),
    "evac_bind_workspace": (C.c_int, [_P, _P, C.c_int64]),
    "evac_reschedule": (C.c_int, [_P, _P]),
    "evac_schedule_generation": (C.c_int32, [_P]),
    "evac_team_error": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "evac_team_error_nosync": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "evac_team_clear_error": (C.c_int, [_P]),
    "evac_peer_gather": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "evac_reset": (C.c_int, [_P, _P, _P, _P, _P]),
    "evac_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P, _P]),
    "evac_rollout": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, _P]),
    "evac_get_state": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "evac_set_state": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "evac_observe": (C.c_int, [_P, _P, _P]),
    "evac_algorithmic_bytes_per_env_step": (C.c_int64, [_P]),
    "evac_norm_state_doubles": (C.c_int64, [_P]),
    "evac_step_normalized": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "evac_norm_init": (C.c_int, [_P, _P, _P]),
    "evac_norm_reset": (C.c_int, [_P, _P, _P, _P, C.c_float, C.c_float, _P]),
    "evac_norm_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "evac_policy_rollout": (C.c_int, [_P, C.c_int32, C.POINTER(EvacMlpPolicy), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                      C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "evac_policy_rollout_population": (C.c_int, [_P, C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacMlpPolicyStrides), C.c_int32,
                                                 _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "evac_policy_evaluate": (C.c_int, [_P, C.c_int32, C.POINTER(EvacMlpPolicy), C.c_int32, C.c_int32, _P, _P, _P, C.c_float, C.c_float, _P]),
    "evac_policy_evaluate_population": (C.c_int, [_P, C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacMlpPolicyStrides), C.c_int32,
                                                  C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_float, C.c_float, _P]),
    # the encoder entries: evac_policy_rollout's / evac_policy_evaluate's arguments with the encoder's struct in front of the stream
    **{f"evac_policy_{what}{suffix}": (C.c_int, front + [C.POINTER(struct), _P])
       for suffix, struct in (("_deepsets", EvacDeepSets), ("_transformer", EvacTransformer))
       for what, front in (("rollout", [_P, C.c_int32, C.POINTER(EvacMlpPolicy)] + [_P] * 11 + [C.c_float] * 4),
                           ("evaluate", [_P, C.c_int32, C.POINTER(EvacMlpPolicy), C.c_int32, C.c_int32, _P, _P, _P, C.c_float, C.c_float]))},
    # the recording evaluation: the counterpart's arguments with evac_eval_capture_t in front of the stream
    **{f"evac_policy_evaluate{suffix}_capture": (
        C.c_int, [_P, C.c_int32, C.POINTER(EvacMlpPolicy), C.c_int32, C.c_int32, _P, _P, _P, C.c_float, C.c_float] + encoder +
        [C.POINTER(EvacEvalCapture), _P])
       for suffix, encoder in (("", []), ("_deepsets", [C.POINTER(EvacDeepSets)]), ("_transformer", [C.POINTER(EvacTransformer)]))},
    "evac_gae": (C.c_int, [C.c_int32, C.c_int64, _P, _P, _P, _P, _P, C.c_double, C.c_double, _P, _P, _P]),
    # the gradient entries: the linear network's, and an encoder's with its struct after the policy and its gradients' after the
    # policy's; a step has the optimiser's arguments behind the gradient's
    **{f"evac_{kind}_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64]) for kind in ("rpo", "deepsets", "transformer")},
    "evac_rpo_minibatch_grad": (C.c_int, _grad_args()),
    "evac_deepsets_minibatch_grad": (C.c_int, _grad_args(EvacDeepSets, EvacDeepSetsGrads)),
    "evac_transformer_minibatch_grad": (C.c_int, _grad_args(EvacTransformer, EvacTransformerGrads)),
    "evac_rpo_minibatch_step": (C.c_int, _grad_args() + [C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacAdamState), C.POINTER(EvacAdamConfig)]),
    "evac_deepsets_minibatch_step": (C.c_int, _grad_args(EvacDeepSets, EvacDeepSetsGrads) + [
        C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacDeepSetsGrads), C.POINTER(EvacDeepSetsAdamState), C.POINTER(EvacAdamConfig)]),
    "evac_adam_step": (C.c_int, [C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacAdamState),
                                 C.POINTER(EvacAdamConfig), C.c_int32, _P, _P]),
    "evac_rpo_update": (C.c_int, [C.POINTER(EvacMlpPolicy), C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacMlpPolicyGrads),
                                  C.POINTER(EvacRpoLossConfig), C.POINTER(EvacAdamConfig), C.POINTER(EvacAdamState), C.c_int64,
                                  _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, _P, _P, C.c_uint64, C.c_uint64, C.c_int32,
                                  C.c_double, _P, _P, _P]),
    "evac_deepsets_adam_step": (C.c_int, [C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacDeepSetsGrads), C.POINTER(EvacMlpPolicyGrads),
                                          C.POINTER(EvacDeepSetsGrads), C.POINTER(EvacDeepSetsAdamState), C.POINTER(EvacAdamConfig),
                                          C.c_int32, C.c_int32, _P, _P]),
    "evac_deepsets_update": (C.c_int, [C.POINTER(EvacMlpPolicy), C.POINTER(EvacDeepSets), C.POINTER(EvacMlpPolicyGrads),
                                       C.POINTER(EvacDeepSetsGrads), C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacDeepSetsGrads),
                                       C.POINTER(EvacRpoLossConfig), C.POINTER(EvacAdamConfig), C.POINTER(EvacDeepSetsAdamState),
                                       C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, _P, _P, C.c_uint64, C.c_uint64,
                                       C.c_int32, C.c_double, _P, _P, _P]),
    # the transformer leader's three: the deep-sets forms with its structs (the step takes num_blocks after elem_dim)
    "evac_transformer_minibatch_step": (C.c_int, _grad_args(EvacTransformer, EvacTransformerGrads) + [
        C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacTransformerGrads), C.POINTER(EvacTransformerAdamState), C.POINTER(EvacAdamConfig)]),
    "evac_transformer_adam_step": (C.c_int, [C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacTransformerGrads), C.POINTER(EvacMlpPolicyGrads),
                                             C.POINTER(EvacTransformerGrads), C.POINTER(EvacTransformerAdamState),
                                             C.POINTER(EvacAdamConfig), C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "evac_transformer_update": (C.c_int, [C.POINTER(EvacMlpPolicy), C.POINTER(EvacTransformer), C.POINTER(EvacMlpPolicyGrads),
                                          C.POINTER(EvacTransformerGrads), C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacTransformerGrads),
                                          C.POINTER(EvacRpoLossConfig), C.POINTER(EvacAdamConfig), C.POINTER(EvacTransformerAdamState),
                                          C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, _P, _P, C.c_uint64, C.c_uint64,
                                          C.c_int32, C.c_double, _P, _P, _P]),
    "evac_rpo_population_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32]),
    "evac_rpo_update_population": (C.c_int, [C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacMlpPolicyGrads),
                                             C.POINTER(EvacMlpPolicyStrides), C.POINTER(EvacMlpPolicyStrides),
                                             C.POINTER(EvacMlpPolicyStrides), C.c_int64, C.POINTER(EvacRpoLossConfig),
                                             C.POINTER(EvacAdamConfig), C.POINTER(EvacAdamState), C.c_int64, _P, _P, _P, _P, _P, _P,
                                             C.c_int64, C.c_int64, C.c_int32, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.c_int32, C.c_double, _P, _P, _P]),
    # the population of deep-sets leaders: the linear population's arguments with the encoder's structs and strides beside the
    # policy's
    "evac_policy_rollout_population_deepsets": (C.c_int, [_P, C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacMlpPolicyStrides),
                                                          C.POINTER(EvacDeepSets), C.POINTER(EvacDeepSetsStrides), C.c_int32,
                                                          _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float,
                                                          C.c_float, _P]),
    "evac_policy_evaluate_population_deepsets": (C.c_int, [_P, C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacMlpPolicyStrides),
                                                           C.POINTER(EvacDeepSets), C.POINTER(EvacDeepSetsStrides), C.c_int32, C.c_int32,
                                                           C.c_int32, C.c_int32, _P, _P, _P, C.c_float, C.c_float, _P]),
    "evac_deepsets_population_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32]),
    "evac_deepsets_update_population": (C.c_int, [C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacDeepSets),
                                                  C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacDeepSetsGrads),
                                                  C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacDeepSetsGrads),
                                                  C.POINTER(EvacMlpPolicyStrides), C.POINTER(EvacDeepSetsStrides),
                                                  C.POINTER(EvacMlpPolicyStrides), C.POINTER(EvacDeepSetsStrides),
                                                  C.POINTER(EvacMlpPolicyStrides), C.POINTER(EvacDeepSetsStrides), C.c_int64,
                                                  C.POINTER(EvacRpoLossConfig), C.POINTER(EvacAdamConfig),
                                                  C.POINTER(EvacDeepSetsAdamState), C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64,
                                                  C.c_int64, C.c_int32, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                  C.c_int32, C.c_double, _P, _P, _P]),
    # the population of transformer leaders on a handle's envs: the deep-sets forms with the attention encoder's struct and strides
    "evac_policy_rollout_population_transformer": (C.c_int, [_P, C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacMlpPolicyStrides),
                                                             C.POINTER(EvacTransformer), C.POINTER(EvacTransformerStrides), C.c_int32,
                                                             _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float,
                                                             C.c_float, C.c_float, _P]),
    "evac_policy_evaluate_population_transformer": (C.c_int, [_P, C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacMlpPolicyStrides),
                                                              C.POINTER(EvacTransformer), C.POINTER(EvacTransformerStrides), C.c_int32,
                                                              C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_float, C.c_float, _P]),
    # its update: evac_deepsets_update_population's arguments with the attention encoder's structs
    "evac_transformer_population_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32]),
    "evac_transformer_update_population": (C.c_int, [C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacTransformer),
                                                     C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacTransformerGrads),
                                                     C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacTransformerGrads),
                                                     C.POINTER(EvacMlpPolicyStrides), C.POINTER(EvacTransformerStrides),
                                                     C.POINTER(EvacMlpPolicyStrides), C.POINTER(EvacTransformerStrides),
                                                     C.POINTER(EvacMlpPolicyStrides), C.POINTER(EvacTransformerStrides), C.c_int64,
                                                     C.POINTER(EvacRpoLossConfig), C.POINTER(EvacAdamConfig),
                                                     C.POINTER(EvacTransformerAdamState), C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64,
                                                     C.c_int64, C.c_int32, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                     C.c_int32, C.c_double, _P, _P, _P]),
    "evac_gae_learners": (C.c_int, [C.c_int32, C.c_int64, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.POINTER(EvacLearnerHyper),
                                    _P, _P, _P]),
    "evac_policy_rollout_sweep": (C.c_int, [_P, C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacMlpPolicyStrides), C.c_int32,
                                            _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float,
                                            C.POINTER(EvacLearnerHyper), _P]),
    "evac_rpo_update_sweep": (C.c_int, [C.c_int32, C.POINTER(EvacMlpPolicy), C.POINTER(EvacMlpPolicyGrads), C.POINTER(EvacMlpPolicyGrads),
                                        C.POINTER(EvacMlpPolicyStrides), C.POINTER(EvacMlpPolicyStrides),
                                        C.POINTER(EvacMlpPolicyStrides), C.c_int64, C.POINTER(EvacRpoLossConfig),
                                        C.POINTER(EvacAdamConfig), C.POINTER(EvacAdamState), C.c_int64, _P, _P, _P, _P, _P, _P,
                                        C.c_int64, C.c_int64, C.c_int32, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                        C.POINTER(EvacLearnerHyper), _P, _P, _P]),
}
# the sweeps of the encoder leaders: the population entries' arguments with evac_learner_hyper_t[S] in front of the stream
# (collection) or in place of use_target_kl, target_kl (the update); the sizers are the population's
for _enc in ("deepsets", "transformer"):
    _res, _args = SIGNATURES[f"evac_policy_rollout_population_{_enc}"]
    SIGNATURES[f"evac_policy_rollout_sweep_{_enc}"] = (_res, _args[:-1] + [C.POINTER(EvacLearnerHyper), _args[-1]])
    _res, _args = SIGNATURES[f"evac_{_enc}_update_population"]
    SIGNATURES[f"evac_{_enc}_update_sweep"] = (_res, _args[:-5] + [C.POINTER(EvacLearnerHyper)] + _args[-3:])
    SIGNATURES[f"evac_{_enc}_sweep_workspace_bytes"] = SIGNATURES[f"evac_{_enc}_population_workspace_bytes"]
del _enc, _res, _args

_lib = None


def load() -> C.CDLL:
    """Load libevac.so (built in-tree by evacuation_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m evacuation_amd.build` (needs hipcc). "
            "evacuation_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if os.environ.get("EVAC_LIB"):   # a profiling build of an older tree (A/B runs): entry points added since are absent
                continue
            raise AttributeError(f"{LIB_PATH} does not export {name}: stale build? (python -m evacuation_amd.build --force)")
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, handle=None):
    if rc != EVAC_OK:
        lib = load()
        msg = lib.evac_last_error(handle)
        text = msg.decode() if msg else ""
        raise EvacError(rc, text or lib.evac_status_string(rc).decode())
