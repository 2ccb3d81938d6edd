"""A sweep of a population of transformer leaders on an MI355X (evac_policy_rollout_sweep_transformer,
evac_transformer_update_sweep, PopulationTrainer(optimizer="device_transformer", encoder_sweep=True)): every learner its own
hyperparameters in the population's launches, each BIT FOR BIT the lone trainer it would be with its configuration
(policy_rollout on a handle wrapped with its gamma; trainer.transformer_update with a TransformerAdam at its lr / max_grad_norm,
which tests/test_gpu_transformer_update.py holds to the host loop).  The checks are tests/encoder_sweep_cases.py's, shared with
tests/test_gpu_deepsets_sweep.py.

1. Collection.  2. Update.  3. Uniform values.  4. target_kl per learner.  5. The table and the mask at their ends (S = 64).
6. The workspace.  7. Determinism and capture.  8. The whole loop."""
import pytest

from tests import encoder_sweep_cases as SC
from tests import test_gpu_transformer_population_update as TU
from tests.encoder_cases import ea  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

ENC = SC.Enc("transformer", TU, small=(1, 2, 1, False), middle=(10, 3, 2, False))

UPDATE_CASES = [  # N, dm, blocks, resid, B_l, E_l, M, norm_adv
    (1, 2, 1, False, 200, 4, 70, 1),    # 3 tokens, one block; steps of 70, 70 and a tail of 60
    (10, 3, 2, False, 200, 4, 70, 1),   # two blocks
    (62, 6, 2, True, 200, 4, 70, 1),    # 64 tokens; D = 384: more dynamic LDS in k_sweep_grad than the default limit
    (10, 3, 2, True, 8, 1, 8, 1),       # M = B_l = 8: one tile, one part, one workgroup
    (10, 3, 2, False, 200, 4, 70, -1),  # norm_adv, and the perturbation INJECTED with every learner's own alpha
]


@pytest.mark.parametrize("S,E_l,generic", [(3, 3, False), (2, 40, False), (3, 3, True)])
def test_collection_normalises_rewards_with_each_learners_gamma(ea, S, E_l, generic):
    """(3, 3): thirteen of sixteen waves leave; (2, 40): three workgroups per learner; generic: the other instantiation."""
    SC.check_collection(ea, ENC, S, E_l, generic)


def test_equal_gammas_are_the_population_entry(ea):
    SC.check_equal_gammas_are_the_population_entry(ea, ENC)


def test_gammas_change_nothing_on_a_raw_env(ea):
    SC.check_gammas_change_nothing_on_a_raw_env(ea, ENC)


@pytest.mark.parametrize("N,dm,blocks,resid,B_l,E_l,M,norm_adv", UPDATE_CASES)
def test_update_equals_standalone_updates_with_each_learners_config(ea, N, dm, blocks, resid, B_l, E_l, M, norm_adv):
    SC.check_update(ea, ENC, (N, dm, blocks, resid), B_l, E_l, M, norm_adv)


def test_uniform_values_are_the_population_entry(ea):
    SC.check_uniform_values_are_the_population_entry(ea, ENC)


def test_target_kl_is_each_learners_own(ea):
    SC.check_target_kl_is_each_learners_own(ea, ENC)


def test_the_table_and_the_mask_at_their_ends(ea):
    SC.check_the_table_and_the_mask_at_their_ends(ea, ENC)


def test_the_workspace_holds_the_update_and_ends_with_the_table(ea):
    SC.check_the_workspace(ea, ENC)


def test_two_calls_and_a_captured_replay_give_the_same_bits(ea):
    SC.check_determinism_and_capture(ea, ENC)


def test_sweep_trainer_equals_standalone_trainers(ea):
    SC.check_sweep_trainer_equals_standalone_trainers(ea, ENC)
