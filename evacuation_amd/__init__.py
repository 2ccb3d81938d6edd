"""evacuation_amd -- MI355X-native step path of the cinemere/evacuation environment.

Public surface = the reference's ``src.env`` exports (src/env/__init__.py:3-21):
``setup_env, EvacuationEnv, EnvConfig, EnvWrappersConfig, Status`` plus the batched form
``BatchedEvacuationEnv``, its SyncVectorEnv-shaped host face ``HostVectorEnv``, the sharded form ``ShardedEvacuationEnv`` (across GPUs) and ``SplitBatchEnv`` (across streams of one GPU), and the reference trainer's update on
the device (``RPOTrainer``, ``RPOTrainingConfig``, ``gae``, ``rpo_minibatch_grad``, and the optimiser
step ``DeviceAdam``, ``rpo_minibatch_step``, ``rpo_update``, and the deep-sets leader's gradient ``deepsets_minibatch_grad`` /
``deepsets_kernel_grad``: ``evacuation_amd.trainer``), and the evaluation of a fixed agent
over whole episodes (``PolicyEvaluator``, ``PopulationEvaluator``, ``EvaluationResult``, the scripted baseline ``WacuumCleaner``), and S independent
learners of one configuration in one set of launches (``PolicyPopulation``, ``PopulationAdam``, ``PopulationTrainer``,
``rpo_update_population``: ``evacuation_amd.population``).  The reference's three networks live in ``evacuation_amd.policy``
(``LinearActorCritic``, ``DeepSetsActorCritic``, ``TransformerActorCritic``): each collects and evaluates on the device.  Importing the package does
not touch the GPU; constructing an env loads libevac.so and fails loudly without it."""
from .config import EnvConfig, EnvWrappersConfig
from .statuses import Status

__all__ = ["EnvConfig", "EnvWrappersConfig", "Status", "setup_env", "EvacuationEnv", "BatchedEvacuationEnv",
           "ShardedEvacuationEnv", "SplitBatchEnv", "NormalizedVectorEnv", "HostVectorEnv", "RandomAgent", "KernelOptions", "kernel_options",
           "RPOTrainer", "RPOTrainingConfig", "gae", "rpo_minibatch_grad", "DeviceAdam", "rpo_minibatch_step", "rpo_update",
           "deepsets_minibatch_grad", "deepsets_kernel_grad", "WacuumCleaner", "PolicyEvaluator", "PopulationEvaluator", "EvaluationResult",
           "PolicyPopulation", "DeepSetsPopulation", "TransformerPopulation", "PopulationAdam", "TransformerPopulationAdam",
           "PopulationTrainer", "rpo_update_population", "deepsets_update_population", "transformer_update_population", "deepsets_update_sweep",
           "transformer_update_sweep",
           "episode_to_memory"]


def __getattr__(name):   # lazy: keeps `import evacuation_amd` light and torch-free for config users
    if name in ("setup_env", "EvacuationEnv"):
        from . import env as _env
        return getattr(_env, name)
    if name == "BatchedEvacuationEnv":
        from .vector_env import BatchedEvacuationEnv
        return BatchedEvacuationEnv
    if name == "ShardedEvacuationEnv":
        from .distributed import ShardedEvacuationEnv
        return ShardedEvacuationEnv
    if name == "SplitBatchEnv":
        from .split_env import SplitBatchEnv
        return SplitBatchEnv
    if name == "NormalizedVectorEnv":
        from .wrappers import NormalizedVectorEnv
        return NormalizedVectorEnv
    if name == "HostVectorEnv":
        from .host_env import HostVectorEnv
        return HostVectorEnv
    if name in ("KernelOptions", "kernel_options"):
        from . import options as _options
        return getattr(_options, name)
    if name in ("RandomAgent", "WacuumCleaner"):
        from . import agents as _agents
        return getattr(_agents, name)
    if name in ("PolicyEvaluator", "PopulationEvaluator", "EvaluationResult"):      # whole-episode evaluation of a fixed agent on the device
        from . import evaluation as _evaluation
        return getattr(_evaluation, name)
    if name in ("RPOTrainer", "RPOTrainingConfig", "gae", "rpo_minibatch_grad", "DeviceAdam", "rpo_minibatch_step", "rpo_update",
                "deepsets_minibatch_grad", "deepsets_kernel_grad"):   # the trainer's update on the device
        from . import trainer as _trainer
        return getattr(_trainer, name)
    if name in ("PolicyPopulation", "DeepSetsPopulation", "TransformerPopulation", "PopulationAdam", "TransformerPopulationAdam",
                "PopulationTrainer", "rpo_update_population", "deepsets_update_population", "transformer_update_population", "deepsets_update_sweep",
                "transformer_update_sweep"):   # S learners in one set of launches
        from . import population as _population
        return getattr(_population, name)
    if name == "episode_to_memory":      # one episode of a recorded evaluation in the reference's frame format
        from .trajectory import episode_to_memory
        return episode_to_memory
    raise AttributeError(name)
