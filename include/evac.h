/*
 * libevac -- MI355X (gfx950) implementation of the cinemere/evacuation env step path.
 *
 * C ABI: plain pointers and sizes, no C++/torch types.  This is the drop-in boundary: the
 * reference is pure Python and has no FFI of its own, so each entry point below names the
 * reference *Python* interface it replaces (file:line under /root/reference).  INTEGRATION.md
 * shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *  - every function returns 0 on success or a negative evac_status_t; nothing throws;
 *  - the CALLER owns every device buffer (PyTorch tensors in our host code); the library owns
 *    only a host-side copy of the config, the Philox key and the bound pointers;
 *  - all work is enqueued on the caller's stream (a hipStream_t passed as void*); no call
 *    synchronises or allocates device memory, so calls can be captured into a hipGraph;
 *  - one handle per (device, set of state buffers); a handle is not thread-safe, distinct
 *    handles are independent.
 *
 * Kernel-family selection is a CREATE-TIME OPTION (evac_options_t, evac_create_ex); every field defaults to -1 = automatic.  The
 * environment switches below are kept as DIAGNOSTIC OVERRIDES only (A/B runs of an unmodified caller): a variable that is set wins
 * over the option.  EVAC_SUBWAVE=0 selects the one-wave-per-env
 * kernels also for N <= 32 (default: 4 envs per wave for N <= 16, 2 for N <= 32; same results, see
 * tests/test_gpu_parity.py::test_subwave_kernels_match_one_wave_per_env); EVAC_CELLS=1 / 0 forces the cell-list
 * kernels on (for every N > 64) / off (default: N > 512; the all-pairs kernels give the same neighbour sets); EVAC_CU_WIDE=1 / 0
 * forces / forbids the CU-wide rollout workgroups of one-wave envs (default: batches of >= 16 envs per CU); EVAC_TEAM=0 / 2 / 4 / 8 / 16
 * forbids / forces the team rollout kernels of rooms of more than 512 pedestrians (default: as many CUs per env as the batch leaves
 * free; not under EVAC_CELLS); all of them give bit-identical results.
 * EVAC_SPECIALIZE=0 keeps handles of the reference's default configuration (enslaving_degree 1, |noise_coef| <= 0.4, alpha 3 gravity
 * observation or rel + ohe Box, no wall termination) on the generic kernels instead of the k_*_default_config instantiations in
 * which those uniform parameters are compile-time constants (bit-identical, tests/test_gpu_schedule.py).
 * The Python host honours EVAC_WORKSPACE=0 (no workspace) and
 * EVAC_LIB=<path> to load a profiling build of this library instead of evacuation_amd/libevac.so.
 *
 * Device layouts (row-major, E = num_envs, N = n_ped)
 *    ped    float [E][N][4]   (x, y, dir_x, dir_y)      pedestrians.py:17-19
 *    status uint8 [E][N]      1 VISCEK 2 FOLLOWER 3 EXITING 4 ESCAPED   statuses.py:16-27
 *    agent  float [E][4]      (x, y, dir_x, dir_y)      area.py:12-30
 *    clock  int32 [E][4]      (now, n_resets, total_steps, 0)           area.py:42-59
 *    acc    float [E][4]      (episode_reward, episode_intrinsic_reward, episode_status_reward, 0)
 *                                                                       env.py:65-67,168-170
 *    obs    float [E][D]      D = evac_obs_dim(); layout per observation mode below
 *
 * Observation layouts (all f32; D floats per env)
 *    positions=grav                  [agent(2), grad_potential_exit(2), grad_potential_pedestrians(2)]
 *                                    (gymnasium Dict key order, i.e. what FlattenObservation yields)
 *    type=Box                        [(N+2)][C] rows agent, exit, pedestrians; C = 2 / 3 (cat) / 6 (ohe)
 *    type=Dict, positions=abs|rel    [agent(2), exit(2), pedestrians_positions(2N), pedestrians_statuses(4N | N | 0)]
 */
#ifndef EVAC_H
#define EVAC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVAC_VERSION 150          /* 0.1.5: evac_options_t / evac_create_ex, rollouts of one handle as two concurrent kernels (parts), evac_join */
#define EVAC_MAX_PEDESTRIANS 1024 /* one workgroup (<=16 waves) per env */

typedef enum evac_status {
    EVAC_OK = 0,
    EVAC_ERR_INVALID_ARGUMENT = -1,
    EVAC_ERR_NOT_BOUND = -2,
    EVAC_ERR_UNSUPPORTED = -3, /* e.g. positions=grav with type=Box: wrappers/config.py:79-80 raises NotImplementedError */
    EVAC_ERR_HIP = -4,
    EVAC_ERR_NO_DEVICE = -5,
    EVAC_ERR_TEAM_ABORTED = -6 /* an earlier team rollout lost a member, or a chained rollout (evac_options_t.chain) waited in vain for an
                                  env's state: see evac_team_error / evac_team_clear_error */
} evac_status_t;

enum { EVAC_POS_ABS = 0, EVAC_POS_REL = 1, EVAC_POS_GRAV = 2 };   /* wrappers/config.py:19-24 */
enum { EVAC_STAT_NO = 0, EVAC_STAT_OHE = 1, EVAC_STAT_CAT = 2 };  /* wrappers/config.py:26-29 */
enum { EVAC_TYPE_DICT = 0, EVAC_TYPE_BOX = 1 };                   /* wrappers/config.py:31-33 */

/* Parameter block = the fields of EnvConfig (src/env/env/config.py:11-59) and EnvWrappersConfig
 * (src/env/wrappers/config.py:12-38) that enter the arithmetic.  Same names, same meaning. */
typedef struct evac_config {
    int32_t number_of_pedestrians;
    float width;
    float height;
    float step_size;
    float noise_coef;
    float eps;
    float enslaving_degree;
    int32_t is_new_exiting_reward;
    int32_t is_new_followers_reward;
    float intrinsic_reward_coef;
    int32_t is_termination_agent_wall_collision;
    float init_reward_each_step;
    int32_t max_timesteps;
    /* observation wrappers */
    int32_t positions; /* EVAC_POS_*  */
    int32_t statuses;  /* EVAC_STAT_* */
    int32_t type;      /* EVAC_TYPE_* */
    float alpha;       /* GravityEncoding alpha (gravity_encoding.py:41-57) */
    /* 0 (default): bit-faithful to the reference, where a zero heading (0/0, area.py:101) poisons every
     * FOLLOWER/VISCEK pedestrian with NaN.  1: a zero heading contributes nothing (non-reference). */
    int32_t nan_guard;
    /* gym.wrappers.ClipAction of the trainer's wrapper chain (rpo_agent.py:27): clip actions to [-1,1] first */
    int32_t clip_action;
} evac_config_t;

/* Written for envs whose episode ended this step: the nine keys of the reference's per-episode logging dict
 * (env.py:115-125) plus the episode counter Time.n_episodes (area.py:49-51).  Ten 4-byte words; the two
 * counters are integers (a float would lose steps beyond 2^24). */
typedef struct evac_episode_stats {
    float episode_reward;
    float episode_length;
    float episode_intrinsic_reward;
    float episode_status_reward;
    float escaped_pedestrians;
    float exiting_pedestrians;
    float following_pedestrians;
    float viscek_pedestrians;
    int32_t overall_timesteps; /* Time.overall_timesteps (area.py:47,55): steps of this env since creation */
    int32_t n_episodes;        /* Time.n_episodes when the episode ended (resets so far) */
} evac_episode_stats_t;
#define EVAC_EPISODE_STATS_WORDS 10

typedef struct evac_handle* evac_handle_t;

int evac_version(void);
const char* evac_status_string(int status);
/* Last error message of a handle (or of the last failed evac_create when h == NULL). */
const char* evac_last_error(evac_handle_t h);

/* Device-free helpers: validate a config (same errors as evac_create) / floats per env of its
 * observation.  Mirror the checks of wrappers/config.py:76-82. */
int evac_config_validate(const evac_config_t* cfg);
int64_t evac_config_obs_dim(const evac_config_t* cfg);

/* Replaces EvacuationEnv.__init__ + EnvWrappersConfig.wrap_env for a batch of `num_envs` independent
 * envs (env.py:41-84, wrappers/config.py:46-93, src/env/__init__.py:18-21).  `seed` keys the Philox
 * streams; env e uses stream id `env_id_offset + e`, so a sharded run reproduces the single-GPU run. */
int evac_create(const evac_config_t* cfg, int32_t num_envs, int32_t device, uint64_t seed,
                uint64_t env_id_offset, evac_handle_t* out);

/* Create-time options: WHICH kernels a handle launches, never WHAT they compute -- every combination gives bit-identical results
 * (tests/test_gpu_variants_sweep.py, tools/soak_variants.py).  No reference analogue (the reference steps its envs one after another
 * in Python, rpo_agent.py:123-126).  Every field: -1 = automatic (what evac_create does).
 *   subwave     0: one wave per env also for N <= 32; 1: 4 / 2 envs per wave for N <= 16 / 32 (automatic)
 *   cells       1 / 0: the 16 x 16 cell-list kernels for every N > 64 / never (automatic: N > 512)
 *   cu_wide     1 / 0: CU-wide rollout workgroups (16 one-wave or 4 four-wave envs per 1024-thread workgroup) always / never
 *               (automatic: batches of 16..64 one-wave envs, 4..16 four-wave envs per CU)
 *   team        0 / 2 / 4 / 8 / 16: workgroups (CUs) per env of the team rollout kernels, N > 512 (automatic: what the batch leaves free)
 *   specialize  0: never the k_*_default_config instantiations (automatic: when the configuration matches)
 *   parts       1 / 2: evac_rollout issues the batch as ONE kernel on the caller's stream / as TWO half-batch kernels on two streams
 *               the handle owns (see evac_join).  -1: 2 where it pays (CU-wide handles whose halves still fill their CUs), else 1.
 *               evac_create() -- the entry point existing callers use -- always takes 1: its stream contract is unchanged.
 *   team_coop   1: team grids are launched with hipLaunchCooperativeKernel (3-4 % slower; automatic: plain launches)
 *   team_fault  1: fault injection for tests (the team grid is launched one workgroup short; chained launches: the last env's
 *               generation word is never published)
 *   chain       1: CHAINED rollout launches (CU-wide handles with a bound workspace; see below); 0: never; -1: where it
 *               pays (those handles).  Wins over `parts`.  evac_create() always takes 0, like parts = 1.
 *               2: ONE PERSISTENT KERNEL PER JOIN (see below; on request only -- the kernel holds the device until evac_join);
 *               (the CU-wide kernels of one- and four-wave envs, and the team kernels of rooms of more than 512 pedestrians);
 *               where it cannot be had (no such family, a batch of more workgroups than the device has CUs, no large BAR) the
 *               handle falls back to 1, then 0: evac_get_options says what it became. */
typedef struct evac_options {
    int32_t subwave, cells, cu_wide, team, specialize, parts, team_coop, team_fault, chain;
} evac_options_t;
#define EVAC_OPTIONS_AUTO {-1, -1, -1, -1, -1, -1, -1, -1, -1}
/* evac_create with options (NULL: all automatic, parts = 1: exactly evac_create). */
int evac_create_ex(const evac_config_t* cfg, int32_t num_envs, int32_t device, uint64_t seed, uint64_t env_id_offset,
                   const evac_options_t* options_or_null, evac_handle_t* out);
/* The options a handle ended up with (automatic choices resolved, diagnostic environment overrides applied). */
int evac_get_options(evac_handle_t h, evac_options_t* out);
int evac_destroy(evac_handle_t h);

/* Handles created with parts = 2 (no reference analogue).  A rollout launch lasts as long as the heaviest env it carries, and
 * between two launches of one stream lie the queue's kernel boundary and the kernel's prologue; the envs of a batch do not depend
 * on each other, only consecutive launches of the SAME env do.  So such a handle keeps two streams of its own (on two hardware
 * queues) and evac_rollout enqueues envs [0, E/2) and [E/2, E) as two kernels, one per stream: each half waits only for ITS
 * heaviest workgroup and its boundary and prologue run under the other half's steps (N = 60 x 4096 envs, 20 steps per launch:
 * +3.4-5 %).  One call, one slab [T][E][D+3], the same bits as parts = 1 (the Philox streams are keyed by the
 * global env id).  Stream contract of such a handle:
 *   - evac_rollout(h, ..., stream): the kernels go to the handle's own streams, and `stream` does NOT wait for them --
 *     consecutive evac_rollout calls must not meet at a common point, or the halves would run in lock-step again.  The own
 *     streams are put behind what `stream` holds (an event recorded on it) at the FIRST evac_rollout after an evac_join or any
 *     other call on the handle, and at every call that passes `actions` (new inputs); a run of RandomAgent rollout calls
 *     without a join between them is ordered after the work `stream` held at its first call only (a wait per launch costs a
 *     barrier packet, more than the form gains) -- so: join before `stream` reuses or refills anything those launches touch;
 *   - evac_join(h, stream): `stream` waits for everything the handle's own streams have been given so far.  Call it before
 *     anything on `stream` (or the host, after synchronising `stream`) consumes a slab, and before ending a stream capture;
 *   - every other call on the handle (evac_reset, evac_step*, evac_observe, evac_get_state, evac_set_state, evac_reschedule,
 *     rollouts with capture / recorded actions / injected noise) joins first by itself and runs as one kernel on `stream`.
 * evac_num_parts: 1 or 2.  evac_part_stream: the hipStream_t of part k (for timing events and profilers; NULL if k is out of
 * range or the handle owns no streams).  evac_join on a handle that owns no streams is a no-op.
 *
 * CHAINED LAUNCHES (chain = 1; no reference analogue).  With the driver's 20 steps per call a launch lasts as long as its
 * heaviest env, and in the steady state of a batch -- episode phases spread out by early terminations -- every launch carries
 * freshly reset, dense envs: most CUs idle behind them for a quarter of every launch (tools/steady_probe.py: 49.6 us per
 * 4096-env round where the same kernel sustains 36 with every CU kept busy).  Only consecutive launches of the SAME env depend on
 * each other.  A chained handle therefore sends its rollout launches to its two streams ALTERNATELY (launch g to stream g & 1)
 * and orders them per env on the device: a generation word per env in the workspace -- launch g waits for ready[env] == g before
 * it loads the env's state and publishes g + 1 behind its state stores (device-scope accesses; bounded waits) -- so launch
 * g + 1's workgroups take the CUs launch g's light workgroups leave and each wave starts the moment ITS env is ready.  At most
 * two launches overlap (launch g + 2 follows launch g in its stream).  Same bits as every other form.  Stream contract: exactly
 * that of parts = 2 (evac_join; everything that is not a plain rollout joins by itself and restarts the chain behind it).  A wait
 * that times out (it cannot, unless a launch is lost: every launch a wave waits for was dispatched in full before its own) voids
 * the run like a lost team member: the handle's error word is raised, evac_* calls return EVAC_ERR_TEAM_ABORTED until
 * evac_team_clear_error(), and the handle issues plain launches from then on.
 *
 * ONE PERSISTENT KERNEL PER JOIN (chain = 2; no reference analogue).  What a launch adds to the heaviest env's sequence of steps --
 * the queue's boundary, the dispatch of a 1024-thread workgroup (3.4 us on a CU that has just become free), the prologue, the
 * state's way through memory -- is a fifth of a 20-step call even when launches are chained.  With chain = 2 the first evac_rollout
 * after a join starts the rollout kernel on the handle's stream and every call (that one included) becomes a 64-byte COMMAND
 * {steps, slab, episode records} that the host writes, through the PCIe BAR, into a ring in uncached device memory; the resident
 * kernel runs the call's steps into the call's slab and takes the next command with the state still in registers.  evac_join
 * posts STOP: the waves store their state and the kernel ends.  Every call still computes exactly its n_steps into its own
 * buffers; same bits as every other form.  Stream contract: that of parts = 2.  What is particular to this form:
 *   - while it has commands the kernel HOLDS the CUs it runs on (all of them for a batch that fills the device): other kernels of
 *     the process run when it has left;
 *   - a kernel that finds no command for ~150 us LEAVES by itself: every wave stores its env's state and the index of the command
 *     it was waiting for, and the next evac_rollout -- or the join -- starts a kernel that takes every env up where it stopped.
 *     So a caller may pause, wait for the device without having joined, or turn to another handle (also another one with
 *     chain = 2): nothing hangs and nothing starves, there is no bound to exceed and no error to raise; what a gap of more than
 *     ~150 us between two calls costs is a kernel start;
 *   - evac_join posts STOP and enqueues, behind the resident kernel, a FINISHER kernel that runs whatever an env has not run up to
 *     the STOP (nothing, normally: it ends at once) -- the join itself only enqueues, like every call;
 *   - calls with `actions` (and the diagnostic faces) join and run as one kernel on `stream`; more than ~1000 calls without a
 *     join make the library stop the kernel, wait for it on the host and start the next one.
 * evac_own_streams: 0, or 2 for handles with parts = 2, chain = 1 or chain = 2. */
int evac_join(evac_handle_t h, void* stream);
/* The NEXT evac_rollout call puts the handle's own streams behind what its `stream` holds at that moment, as the first call after a
 * join does: for a caller who, between two rollout calls and without a join, gave `stream` work the coming launches must follow -- a
 * freshly allocated or refilled output buffer (a stream-ordered allocator hands out memory that kernels still queued on `stream`
 * may be using), new workspace contents.  The Python host's rollout(), which allocates its outputs, calls it every time. */
int evac_order_next_rollout(evac_handle_t h);
int32_t evac_num_parts(evac_handle_t h);
int32_t evac_own_streams(evac_handle_t h);
void* evac_part_stream(evac_handle_t h, int32_t part);

/* Floats per env in the observation buffer for this handle's observation mode. */
int64_t evac_obs_dim(evac_handle_t h);
int32_t evac_num_envs(evac_handle_t h);
/* Name of the kernel instantiation this handle's evac_step (rollout == 0) / evac_rollout (rollout != 0) launches,
 * e.g. "k_rollout<1 wave/env, grav>": the label bench.py puts next to its roofline numbers (no reference analogue). */
const char* evac_kernel_variant(evac_handle_t h, int32_t rollout);

/* Bind the caller-owned state buffers (device pointers, layouts above). */
int evac_bind_state(evac_handle_t h, float* ped, uint8_t* status, float* agent, int32_t* clock, float* acc);

/* EvacuationEnv.reset (env.py:106-139) for every env, or for those with mask[e] != 0.
 * draws_or_null: float [E][N][4] of U(-1,1) values (pos.x, pos.y, dir.x, dir.y) replacing the Philox
 * draws (pedestrians.py:17-18) -- the injection mode used by the parity tests.
 * obs_out_or_null: reset observation, float [E][D] (only rows of reset envs are written). */
int evac_reset(evac_handle_t h, const uint8_t* mask_or_null, const float* draws_or_null,
               float* obs_out_or_null, void* stream);

/* EvacuationEnv.step + observation wrappers (env.py:141-171, area.py:76-210, statuses.py:29-48,
 * reward.py:19-47, gravity_encoding.py:8-81, wrappers.py:8-96) for the whole batch, one launch.
 *   actions            float [E][2]  (device)
 *   noise_or_null      float [E][N]  per-pedestrian angular noise (injection mode); NULL = Philox
 *   obs_out            float [E][D]
 *   reward_out         float [E];  terminated_out / truncated_out  uint8 [E]
 *   autoreset != 0     finished envs are reset in the same launch (gymnasium-0.29 SyncVectorEnv
 *                      semantics, rpo_agent.py:193-203): obs_out then holds the reset observation,
 *                      final_obs_or_null [E][D] the terminal one, final_stats_or_null [E] the episode record
 */
int evac_step(evac_handle_t h, const float* actions, const float* noise_or_null, float* obs_out,
              float* reward_out, uint8_t* terminated_out, uint8_t* truncated_out, int32_t autoreset,
              float* final_obs_or_null, evac_episode_stats_t* final_stats_or_null, void* stream);

/* T consecutive steps in ONE launch with the env state held in registers/LDS (the trainer's rollout
 * loop rpo_agent.py:180-203 with the policy replaced by caller-provided or RandomAgent actions,
 * random_agent.py:8-9).  Always autoresets.  Buffers are time-major:
 *   actions_or_null     float [T][E][2]   NULL = draw U(-1,1)^2 on device (Philox)
 *   actions_out_or_null float [T][E][2]   records the actions actually used
 *   slab_out            float [T][E][D+3] = [obs(D) | reward | terminated (0/1) | truncated (0/1)] per env-step:
 *                       one packed record (what the trainer's rollout buffers and the all-gather consume)
 *   final_stats_or_null [T][E] (rows of envs that finished at step t)
 *   noise_or_null       float [T][E][N]   per-pedestrian angular noise replacing the Philox draw (injection mode, as
 *                       evac_step's; served by the diagnostic kernel face, like capture / actions_out)
 *   capture_or_null     float [T][capture_envs][N+1][3]: trajectory capture for rendering (the memory that
 *                       Pedestrians.save / Agent.save keep, pedestrians.py:33-35, area.py:32-33, consumed by
 *                       save_animation env.py:241-324): rows 0..N-1 = (x, y, status) of every pedestrian of the
 *                       first `capture_envs` envs after the step (before an autoreset), row N = (leader x, y, 0) */
int evac_rollout(evac_handle_t h, int32_t n_steps, const float* actions_or_null, float* actions_out_or_null,
                 float* slab_out, evac_episode_stats_t* final_stats_or_null, int32_t capture_envs,
                 float* capture_or_null, const float* noise_or_null, void* stream);

/* Optional workspace of evac_rollout (no reference analogue: the reference steps its envs one after another,
 * rpo_agent.py:123-126).  `workspace`: evac_workspace_bytes(h) bytes on the device, 256-byte aligned, ZERO-INITIALISED by the
 * caller, alive and used on one stream at a time like the state buffers.  It holds
 *   - the rollout schedule of large batches of one-wave envs (>= 16 envs per CU; four-wave envs: >= 4 per CU):
 *     moving[2][E] | perm[2][E] int32 -- rollout launch g of the handle runs its envs in the order perm[g & 1], leaves the
 *     pedestrians still moving of each env in moving[g & 1] and, inside the same launch (its first workgroup, which carries the
 *     lightest envs, before it starts stepping), deals the envs to the SIMDs for launch g + 1 by the loads launch g - 1 left:
 *     perm[(g + 1) & 1].  evac_schedule_generation returns g (the number of such launches so far; -1: no schedule, or no deal
 *     yet).  A launch captured into a hipGraph runs under the deal at hand and deals nothing;
 *   - the exchange areas of the team kernels (513..1024 pedestrians, few envs: 2 / 4 / 8 / 16 workgroups per env).
 * Performance devices only: results are bit-identical with and without the workspace.  NULL unbinds.
 *
 * Team rollouts need every workgroup of their grid resident at once (the members of a team wait for each other).  evac_rollout
 * checks that with hipOccupancyMaxActiveBlocksPerMultiprocessor (a grid that does not fit runs one workgroup per env instead);
 * EVAC_TEAM_COOP=1 additionally launches with hipLaunchCooperativeKernel (3-4 % slower).  Should a team lose a member all the
 * same, its waits are bounded: the launch ends, that env's state is NOT written back, and the handle's error word -- 64 bytes of
 * host-mapped memory, the one thing besides the config the library allocates -- is raised.  Every later call on the handle
 * (evac_reset / evac_step* / evac_rollout / evac_observe / evac_get_state / evac_set_state) then returns EVAC_ERR_TEAM_ABORTED
 * without touching the device, until evac_team_clear_error(); the handle uses one workgroup per env from then on.
 * evac_team_error: synchronises the device, then reports the error word (non-zero: the outputs of an earlier launch are void).
 * evac_team_error_nosync: the same word as it stands, without synchronising -- for a caller that has just waited for its
 * stream itself (a pipelined consumer of rollout slabs: wait for the launch, read the word, THEN trust the slab; a launch
 * that aborts returns EVAC_OK when it is enqueued, and so do the launches queued behind it, and a hipGraph replay goes past
 * every host-side check).
 * Team grids of one device run ONE AT A TIME, whatever handles and streams they come from (a device-side wait on the previous
 * team launch's event): two grids in flight could each be resident in part and wait for CUs the other holds.  Launches under
 * stream capture cannot join that chain -- do not replay a graph with team launches beside another team launch; and another
 * PROCESS sharing the GPU is out of reach: run it with EVAC_TEAM=0. */
int64_t evac_workspace_bytes(evac_handle_t h);
int evac_bind_workspace(evac_handle_t h, void* workspace_or_null, int64_t bytes);
/* Deal the envs to the SIMDs NOW (a launch of its own) by the most recent loads the workspace holds, moving[(g - 1) & 1], into
 * the permutation the next rollout launch reads: for callers that restored a state + workspace snapshot and want the next
 * launch to run under that deal.  No-op without a schedule. */
int evac_reschedule(evac_handle_t h, void* stream);
int32_t evac_schedule_generation(evac_handle_t h);
int evac_team_error(evac_handle_t h, int32_t* out);
int evac_team_error_nosync(evac_handle_t h, int32_t* out);
int evac_team_clear_error(evac_handle_t h);

/* The all-gather of the returned observation batch across the ranks of an env-sharded run (BASELINE.json north_star; the
 * reference steps all envs in one process, src/agents/rpo_agent.py:123-126, and has no analogue) as PEER STORES over xGMI,
 * without a library collective: columns [0, take_words) of this rank's record slab src[rows][row_words] -- the rollout's
 * packed [obs | reward | terminated | truncated] records; take_words = obs_dim picks the observation -- are written to
 * slice my_rank of every rank's buffer peer_dst[r] = [world][rows][take_words] (r = my_rank: the local buffer; the others:
 * the peers' buffers mapped into this process, e.g. through hipIpcOpenMemHandle).  One launch on `stream`, all peers at once,
 * wgs_per_peer workgroups of 256 threads each (0: 8); compiled to fit beside a running rollout kernel (evac_gather.h).  A
 * consumer of a buffer needs every rank's launch to have completed (a rendezvous of the ranks).  No handle: any device
 * pointers.  EVAC_ERR_INVALID_ARGUMENT: NULL pointers, world > 16, rows * take_words >= 2^31. */
int evac_peer_gather(const float* src, int64_t rows, int32_t row_words, int32_t take_words, float* const* peer_dst, int32_t world,
                     int32_t my_rank, int32_t wgs_per_peer, void* stream);

/* State exchange in the reference's own shapes (needed for parity tests, checkpoints):
 * pos/dir float [E][N][2], status uint8 [E][N], agent_pos/agent_dir float [E][2], now int32 [E]. */
int evac_get_state(evac_handle_t h, float* pos, float* dir, uint8_t* status, float* agent_pos,
                   float* agent_dir, int32_t* now, void* stream);
int evac_set_state(evac_handle_t h, const float* pos, const float* dir, const uint8_t* status,
                   const float* agent_pos, const float* agent_dir, const int32_t* now, void* stream);

/* Observation of the current state without stepping (EvacuationEnv._get_observation through the
 * wrapper chain, env.py:98-104). */
int evac_observe(evac_handle_t h, float* obs_out, void* stream);

/* Algorithmic HBM bytes of one env-step for this handle (32N+62 for grav, 56N+86
 * for Box+ohe, ...).  Used by bench.py for roofline accounting. */
int64_t evac_algorithmic_bytes_per_env_step(evac_handle_t h);

/* ---- The trainer's per-env wrapper chain on device (rpo_agent.py:24-33) ----
 * NormalizeObservation -> clip(obs, +-obs_clip) -> NormalizeReward(gamma) -> clip(reward, +-reward_clip), one set
 * of running statistics per env (gymnasium wrappers/normalize.py RunningMeanStd, float64), applied IN PLACE to
 * the outputs of evac_step / evac_reset.  ClipAction is evac_config_t.clip_action; FlattenObservation is the
 * flat observation layout; RecordEpisodeStatistics is evac_episode_stats_t.
 *   norm_state  double [E][evac_norm_state_doubles(h)] = obs_mean[D] | obs_var[D] | obs_count[D] | ret_mean |
 *               ret_var | ret_count | returns   (caller-owned, initialise with evac_norm_init)
 * evac_norm_step: for envs that finished (terminated|truncated, same-step autoreset) final_obs (the terminal
 * observation, may be NULL) is normalised and counted first, then obs (the reset observation) -- the order in
 * which SyncVectorEnv calls the wrapped step() and reset(). */
int64_t evac_norm_state_doubles(evac_handle_t h);
/* evac_step with the chain FUSED into the step kernel (one launch; the form the trainer's loop uses): the outputs come
 * out normalised and clipped, norm_state is updated, final_obs (terminal observation of finished envs) is counted
 * before obs.  Same results as evac_step followed by evac_norm_step, bit for bit. */
int evac_step_normalized(evac_handle_t h, const float* actions, const float* noise_or_null, float* obs_out,
                         float* reward_out, uint8_t* terminated_out, uint8_t* truncated_out, int32_t autoreset,
                         float* final_obs_or_null, evac_episode_stats_t* final_stats_or_null, double* norm_state,
                         float gamma, float obs_clip, float reward_clip, float epsilon, void* stream);
int evac_norm_init(evac_handle_t h, double* norm_state, void* stream);
int evac_norm_reset(evac_handle_t h, const uint8_t* mask_or_null, float* obs, double* norm_state, float obs_clip,
                    float epsilon, void* stream);
int evac_norm_step(evac_handle_t h, float* obs, float* final_obs_or_null, float* reward, const uint8_t* terminated,
                   const uint8_t* truncated, double* norm_state, float gamma, float obs_clip, float reward_clip,
                   float epsilon, void* stream);

/* ---- Policy rollout: the trainer's collection loop inside ONE launch (rpo_agent.py:180-196) ----
 * The actor-critic of RPOLinearNetwork (rpo_linear_agent_network.py:19-61):
 *   actor_mean = Linear(D,64) Tanh Linear(64,64) Tanh Linear(64,2);  critic = Linear(D,64) Tanh Linear(64,64) Tanh Linear(64,1);
 *   actor_logstd [1][2].
 * Tensors in torch layouts (W [out][in] row-major, b [out], f32), read through the pointers WHEN THE KERNEL RUNS: a trainer that
 * updates its parameters in place (torch optimisers) can capture the call into a graph once and replay it across updates. */
typedef struct evac_mlp_policy {
    int32_t obs_dim, hidden;   /* obs_dim == evac_obs_dim(h); hidden == 64 (the reference's default num_hidden) */
    const float *actor_w1, *actor_b1, *actor_w2, *actor_b2, *actor_w3, *actor_b3, *actor_logstd;
    const float *critic_w1, *critic_b1, *critic_w2, *critic_b2, *critic_w3, *critic_b3;
} evac_mlp_policy_t;
/* n_steps iterations of rpo_agent.py:180-196, per env, with x = next_obs and d = next_done carried in and out:
 *   obs_out[t] = x; done_out[t] = d;
 *   mu = actor_mean(x), sigma = exp(actor_logstd), a = mu + sigma * z: z = Box-Muller of Philox4x32-10 at counter
 *   (env id, 0, total steps of the env, 'POLI'): u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24, r = sqrt(-2 ln u1),
 *   z = (r cos 2 pi u2, r sin 2 pi u2) -- statistically equivalent to Normal.sample, not bit-identical to torch;
 *   actions_out[t] = a (unclipped), logprob_out[t] = Normal(mu, sigma).log_prob(a).sum(), value_out[t] = critic(x);
 *   the env steps with a exactly as evac_step (norm_state NULL) / evac_step_normalized would (ClipAction, noise, autoreset,
 *   episode records; the terminal observation of a finished episode is always counted in the statistics);
 *   reward_out[t] = the (normalised) reward; d = terminated | truncated; x = the new (normalised, reset) observation;
 *   final_stats_or_null[t] = the episode record of envs that finished at step t.
 * Then next_obs = x, next_done = d, next_value_out = critic(x) (the bootstrap get_value(next_obs)).
 *   next_obs [E][D], next_done [E] (f32 0/1): in/out;  obs_out [T][E][D], actions_out [T][E][2], logprob_out / value_out /
 *   reward_out / done_out [T][E], next_value_out [E], final_stats_or_null [T][E].
 * One wave per env: EVAC_ERR_UNSUPPORTED for rooms of more than 64 pedestrians.  EVAC_ERR_INVALID_ARGUMENT for a NULL pointer,
 * hidden != 64 or obs_dim != evac_obs_dim(h).  Handles with parts = 2 or chain = 1 / 2 are joined first; the call is ONE kernel
 * on `stream`. */
int evac_policy_rollout(evac_handle_t h, int32_t n_steps, const evac_mlp_policy_t* policy,
                        float* next_obs, float* next_done,
                        float* obs_out, float* actions_out, float* logprob_out,
                        float* value_out, float* reward_out, float* done_out,
                        float* next_value_out, evac_episode_stats_t* final_stats_or_null,
                        double* norm_state_or_null, float gamma, float obs_clip, float reward_clip, float epsilon,
                        void* stream);

/* ---- Population: S independent learners of ONE configuration in one set of launches ----
 * What the reference's users run is a sweep: `for sweep in 1 .. 10` independent training processes per setting.  A population
 * is S learners whose 13 tensors are stacked (learner s's tensor = the base pointer + s x that tensor's stride, in floats) and
 * whose envs are the consecutive shares of ONE handle of S x E_l envs: learner s owns envs [s E_l, (s + 1) E_l).
 * EVAC_MAX_LEARNERS is set by the kernel-argument segment: evac_rpo_update_population passes every learner's seed and draw
 * counter by value (16 bytes a learner: 1 KiB of the 4 KiB a HIP launch takes, beside ~0.9 KiB of pointers and strides). */
#define EVAC_MAX_LEARNERS 64
typedef struct evac_mlp_policy_strides {   /* floats from learner s to learner s + 1, per tensor of evac_mlp_policy_t */
    int64_t actor_w1, actor_b1, actor_w2, actor_b2, actor_w3, actor_b3, actor_logstd;
    int64_t critic_w1, critic_b1, critic_w2, critic_b2, critic_w3, critic_b3;
} evac_mlp_policy_strides_t;
/* evac_policy_rollout_population: evac_policy_rollout for n_learners learners in ONE launch.  `policy` holds learner 0's
 * tensors; the storage is that of one evac_policy_rollout over the whole handle (time-major, E = S x E_l: obs_out [T][E][D] ...),
 * norm_state and the env state likewise.  EQUIVALENCE: the call writes, bit for bit, what S calls of evac_policy_rollout write
 * -- call s with learner s's tensors on a handle of E_l envs with the same seed, env_id_offset = this handle's + s E_l and
 * learner s's share of the state -- into the learner's columns [s E_l, (s + 1) E_l) of every array (envs are independent of
 * their neighbours in a batch).  ceil(E_l / 16) CU-wide workgroups per learner; a workgroup never mixes learners.
 * EVAC_ERR_INVALID_ARGUMENT: as evac_policy_rollout, and a NULL strides, n_learners outside 1..EVAC_MAX_LEARNERS, a number of
 * envs that n_learners does not divide, and with n_learners > 1 a stride smaller than its tensor (0 included). */
int evac_policy_rollout_population(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                   const evac_mlp_policy_strides_t* strides, int32_t n_steps,
                                   float* next_obs, float* next_done,
                                   float* obs_out, float* actions_out, float* logprob_out,
                                   float* value_out, float* reward_out, float* done_out,
                                   float* next_value_out, evac_episode_stats_t* final_stats_or_null,
                                   double* norm_state_or_null, float gamma, float obs_clip, float reward_clip, float epsilon,
                                   void* stream);

/* ---- Policy evaluation: whole episodes per env under a FIXED agent, one episode record per finished episode ----
 * What a user of the reference writes around a trained network or a scripted agent and EvacuationEnv.step / reset
 * (env.py:106-171): `obs = env.reset(); while not done: obs, r, term, trunc, _ = env.step(agent.act(obs))`, per env, with the
 * episode dict of env.py:115-125 kept at every episode end.  ONE kernel (evac_evaluate.h), geometry and step body of
 * evac_policy_rollout.  Per env e, with progress[e] = {episodes finished, steps taken so far, two words of the scripted agent's
 * state} carried in and out (zero it to begin):
 *   if progress[e][0] >= n_episodes at entry: nothing is read or written for this env;
 *   x = the observation of the current state (as evac_observe), computed in the kernel;
 *   at most max_steps times:
 *     the action a, by `agent`:
 *       EVAC_AGENT_POLICY_MEAN    a = actor_mean(x) (rpo_linear_agent_network.py:49-50: the mean of get_action_and_value); no
 *                                 noise is drawn
 *       EVAC_AGENT_POLICY_SAMPLE  a = mu + sigma z, z exactly evac_policy_rollout's draw (counter (env id, 0, total steps of the
 *                                 env, 'POLI')): same env, seed and network give the same actions as evac_policy_rollout
 *       EVAC_AGENT_VACUUM_CLEANER WacuumCleaner.act (baseline_wacuum_cleaner.py:36-82) on the leader's position: climb until
 *                                 y >= T_y, sweep right / left between +-T_x with, at every turn, one step down and then up to 25
 *                                 more as long as y > -T_y, and once a step of those finds y <= -T_y head for the exit with
 *                                 a = exit - position.  T = extent - SWITCH_DISTANCE_TO_LEADER / 2 + step_size (:18-28) in double,
 *                                 rounded to float32 once (NumPy 2 compares the float32 position with a Python float in float32);
 *                                 extent and step_size are taken as the shortest decimals that round to the float32 values of
 *                                 evac_config_t (1.3f -> 1.3: the Python floats of the caller's config).
 *                                 It reads no observation.  The reference's object is never reset and would head for the exit for
 *                                 ever after its first episode; here an agent is FRESH FOR EVERY EPISODE (the two state words are
 *                                 cleared at every autoreset)
 *     the env steps with a exactly as evac_step would (ClipAction, the pedestrians' Philox noise, autoreset); progress[e][1] += 1;
 *     when the episode ended: episodes_out[progress[e][0]][e] = its record (as final_stats of evac_step); progress[e][0] += 1;
 *     the env is reset with its next Philox reset draw; the scripted agent starts afresh; stop if progress[e][0] == n_episodes;
 *     x = the new observation.
 *   The state is stored back: the next call continues where this one stopped -- max_steps = 17 repeated until every env is done
 *   equals one long call bit for bit.
 * norm_state_or_null (policy agents): the trainer's observation statistics, FROZEN: x = clip((x - mean_j) / sqrt(var_j + epsilon),
 * +-obs_clip) with the env's own row of norm_state ([E][evac_norm_state_doubles(h)]), which is only read; nothing is counted,
 * rewards and records stay raw.
 *   progress int32 [E][4], 16-byte aligned; episodes_out [n_episodes][E] (slots beyond an env's count are left untouched).
 * One wave per env: EVAC_ERR_UNSUPPORTED for rooms of more than 64 pedestrians.  EVAC_ERR_INVALID_ARGUMENT, decided on the host
 * before anything is launched: an unknown agent, a NULL or misaligned progress, a NULL episodes_out, n_episodes < 1,
 * max_steps < 1, a policy agent with a NULL policy, a NULL tensor, hidden != 64 or obs_dim != evac_obs_dim(h), norm_state given
 * with the scripted agent.  Handles with parts = 2 or chain = 1 / 2 are joined first; the call is ONE kernel on `stream`, no host
 * synchronisation, capturable; the weights are read when the kernel runs. */
enum { EVAC_AGENT_POLICY_MEAN = 0, EVAC_AGENT_POLICY_SAMPLE = 1, EVAC_AGENT_VACUUM_CLEANER = 2 };
int evac_policy_evaluate(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy_or_null,
                         int32_t n_episodes, int32_t max_steps,
                         int32_t* progress,                   /* [E][4] in/out; zero it to begin */
                         evac_episode_stats_t* episodes_out,  /* [n_episodes][E] */
                         const double* norm_state_or_null, float obs_clip, float epsilon, void* stream);
/* evac_policy_evaluate_population: evac_policy_evaluate under the policy agents for n_learners learners in ONE launch.  `policy`
 * holds learner 0's tensors (the actor alone is read); learner s evaluates in envs [s E_l, (s + 1) E_l) of the handle, and
 * progress [S E_l][4], episodes_out [n_episodes][S E_l] and norm_state [S E_l][evac_norm_state_doubles(h)] are indexed by the
 * handle's env.  EQUIVALENCE: the call writes, bit for bit, what S calls of evac_policy_evaluate write -- call s with learner s's
 * tensors on a handle of E_l envs with the same seed, learner s's share of the state and its rows of norm_state -- into learner
 * s's columns of progress and episodes_out and its share of the state.  With shared_episodes != 0 that handle's env_id_offset is
 * this handle's: env i of EVERY learner has the global id of env i, so all learners meet the same reset draws and pedestrian noise
 * (and, in sample mode, the same z).  With shared_episodes == 0 it is this handle's + s E_l, the id convention of
 * evac_policy_rollout_population: sample mode with max_steps = T is then that call's env side bit for bit.
 * ceil(E_l / 16) CU-wide workgroups per learner; a workgroup never mixes learners; the launch lasts as long as its longest env.
 * EVAC_ERR_UNSUPPORTED / EVAC_ERR_INVALID_ARGUMENT, decided on the host before anything is launched: as evac_policy_evaluate, and
 * EVAC_AGENT_VACUUM_CLEANER (no learners: evac_policy_evaluate runs it), a NULL strides, n_learners outside
 * 1..EVAC_MAX_LEARNERS, a number of envs that n_learners does not divide, and with n_learners > 1 a stride smaller than its
 * tensor (0 included).  The handle is joined first; ONE kernel on `stream`, no host synchronisation, capturable. */
int evac_policy_evaluate_population(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                    const evac_mlp_policy_strides_t* strides, int32_t agent, int32_t shared_episodes,
                                    int32_t n_episodes, int32_t max_steps,
                                    int32_t* progress,                   /* [S E_l][4] in/out; zero it to begin */
                                    evac_episode_stats_t* episodes_out,  /* [n_episodes][S E_l] */
                                    const double* norm_state_or_null, float obs_clip, float epsilon, void* stream);

/* ---- The deep-sets leader: the reference's set encoder in front of the actor-critic (rpo_deep_sets_agent_network.py:25-90) ----
 * RPODeepSetsEmbedding reads the Box observation x [D] as a set of S = N + 2 rows (pedestrians, leader, exit) of
 * set_elem_dim = D / S floats (6: positions + one-hot status, 3: positions + categorical status, 2: positions only):
 *   phi(x_i) = phi_w2 . relu(phi_w1 x_i + phi_b1) + phi_b2     phi_w1 [24][set_elem_dim], phi_b1 [24], phi_w2 [24][24], phi_b2 [24]
 *   y = rho_w . sum_i phi(x_i) + rho_b                          rho_w [D][24], rho_b [D]
 * and actor_mean(y) / critic(y) of evac_mlp_policy_t.  One encoder serves actor and critic.  x is what evac_policy_rollout's
 * network reads -- after the normalisation chain when norm_state is given -- and what goes into obs_out: y is never stored.
 * The kernels pool above the relu, sum_i phi(x_i) = phi_w2 . (sum_i relu(phi_w1 x_i + phi_b1)) + S phi_b2: the same function,
 * rounded elsewhere; every sum has a fixed order (evac_deepsets.h), so results do not depend on the batch, the launch or the run.
 * Tensors in torch layouts, float32, read in place when the kernel runs; rho_w 16-byte aligned (its rows are read as vectors). */
typedef struct evac_deepsets {
    int32_t set_elem_dim;      /* set_elem_dim x (N + 2) == evac_obs_dim(h): a Box observation */
    int32_t hidden;            /* 24 (RPODeepSetsEmbeddingConfig.dim_hidden, the only width taken) */
    const float *phi_w1, *phi_b1, *phi_w2, *phi_b2;
    const float *rho_w, *rho_b;
} evac_deepsets_t;
/* evac_policy_rollout with the encoder run on x before every step's forward pass and before the bootstrap value: arguments,
 * storage, env side (bit for bit) and refusals are evac_policy_rollout's.  Further EVAC_ERR_INVALID_ARGUMENT: a NULL encoder or
 * tensor of it, hidden != 24, set_elem_dim x (N + 2) != evac_obs_dim(h) (the gravity observation included), a misaligned rho_w. */
int evac_policy_rollout_deepsets(evac_handle_t h, int32_t n_steps, const evac_mlp_policy_t* policy,
                                 float* next_obs, float* next_done,
                                 float* obs_out, float* actions_out, float* logprob_out,
                                 float* value_out, float* reward_out, float* done_out,
                                 float* next_value_out, evac_episode_stats_t* final_stats_or_null,
                                 double* norm_state_or_null, float gamma, float obs_clip, float reward_clip, float epsilon,
                                 const evac_deepsets_t* encoder, void* stream);
/* evac_policy_evaluate for the policy agents with the encoder run before the actor: a = actor_mean(y) (+ sigma z).  Sample mode
 * is evac_policy_rollout_deepsets bit for bit.  EVAC_ERR_INVALID_ARGUMENT as evac_policy_evaluate and as above, and for
 * EVAC_AGENT_VACUUM_CLEANER (no network: evac_policy_evaluate runs it). */
int evac_policy_evaluate_deepsets(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy,
                                  int32_t n_episodes, int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out,
                                  const double* norm_state_or_null, float obs_clip, float epsilon,
                                  const evac_deepsets_t* encoder, void* stream);

/* ---- The transformer leader: the reference's attention encoder in front of the actor-critic (rpo_transformer_agent_network.py) ----
 * RPOTransformerEmbedding reads the Box observation x [D] as S = N + 2 tokens of elem_dim = D / S floats (6, 3 or 2) and runs
 * num_blocks blocks [S][dm] -> [S][dm] (dm = elem_dim, H = num_heads = 3):
 *   Q = x wq^T + bq, K, V likewise                       wq, wk, wv [H dm][dm], output index h dm + c
 *   score[c][i][j] = sum_h Q[i][h dm + c] K[j][h dm + c] / sqrt(dm),  w = softmax_j(score)      per channel c, contracted over heads
 *   o[i][c][h] = sum_j w[c][i][j] V[j][h dm + c],  a_i = dense_w . o[i] (flattened as c H + h) + dense_b      dense_w [dm][H dm]
 *   u = LayerNorm1(use_resid ? x + a : a)                over the dm values of a token, biased variance, eps ln_eps, affine
 *   f = ff2_w relu(ff1_w u + ff1_b) + ff2_b              ff1_w [96][dm], ff2_w [dm][96]
 *   block output = LayerNorm2(use_resid ? u + f : f)
 * with every dropout the identity (the module's eval-mode function), and actor_mean / critic of evac_mlp_policy_t read the last
 * block's output flattened back to [D].  One encoder serves actor and critic; x is what goes into obs_out.  Every sum has a
 * fixed order (evac_transformer.h): results do not depend on the batch, the launch or the run.  Tensors in torch layouts,
 * float32, read in place when the kernel runs. */
typedef struct evac_transformer_block {
    const float *wq, *bq, *wk, *bk, *wv, *bv;
    const float *dense_w, *dense_b;
    const float *ff1_w, *ff1_b, *ff2_w, *ff2_b;
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} evac_transformer_block_t;
typedef struct evac_transformer {
    int32_t elem_dim;          /* elem_dim x (N + 2) == evac_obs_dim(h): a Box observation */
    int32_t num_blocks;        /* 1 or 2; blocks[num_blocks ..] are not read */
    int32_t num_heads;         /* 3 (RPOTransformerEmbeddingConfig.num_heads, the only count taken) */
    int32_t dim_feedforward;   /* 96 (likewise) */
    int32_t use_resid;         /* 0 / 1 */
    float ln_eps;              /* 1e-5f (nn.LayerNorm's default, the only value taken) */
    evac_transformer_block_t blocks[2];
} evac_transformer_t;
/* evac_policy_rollout with the encoder run on x before every step's forward pass and before the bootstrap value: arguments,
 * storage, env side (bit for bit) and refusals are evac_policy_rollout's.  Further EVAC_ERR_INVALID_ARGUMENT: a NULL encoder or
 * tensor of a block in use, elem_dim outside 1..6 or elem_dim x (N + 2) != evac_obs_dim(h).  EVAC_ERR_UNSUPPORTED, with the
 * field named by evac_last_error: num_heads != 3, dim_feedforward != 96, num_blocks outside 1..2, ln_eps != 1e-5f, N > 62 (one
 * wave holds the N + 2 tokens), the gravity observation (no Box of tokens). */
int evac_policy_rollout_transformer(evac_handle_t h, int32_t n_steps, const evac_mlp_policy_t* policy,
                                    float* next_obs, float* next_done,
                                    float* obs_out, float* actions_out, float* logprob_out,
                                    float* value_out, float* reward_out, float* done_out,
                                    float* next_value_out, evac_episode_stats_t* final_stats_or_null,
                                    double* norm_state_or_null, float gamma, float obs_clip, float reward_clip, float epsilon,
                                    const evac_transformer_t* encoder, void* stream);
/* evac_policy_evaluate for the policy agents with the encoder run before the actor.  Sample mode is
 * evac_policy_rollout_transformer bit for bit.  Refusals as evac_policy_evaluate_deepsets and as above. */
int evac_policy_evaluate_transformer(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy,
                                     int32_t n_episodes, int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out,
                                     const double* norm_state_or_null, float obs_clip, float epsilon,
                                     const evac_transformer_t* encoder, void* stream);

/* ---- Recording an evaluation: the episodes' frames for rendering (Pedestrians.save / Agent.save, pedestrians.py:33-35,
 * area.py:32-33) ----
 * The three entries below are evac_policy_evaluate, evac_policy_evaluate_deepsets and evac_policy_evaluate_transformer with
 * `capture` in front of the stream: arguments, contract, progress, records and state are the counterpart's bit for bit, and the
 * launch also writes, for the envs e < capture_envs of the handle (K = capture_envs, N pedestrians; rows 0..N-1 of a frame hold
 * (x, y, status) as floats, row N holds (leader x, leader y, 0) -- evac_rollout's capture layout):
 *   frames[f][e]  the state after the env's step f and BEFORE any reset, f counted from the env's first step of the evaluation:
 *                 the step a launch takes as its t-th (t = 0, 1, ...) has f = progress[e][1] at the launch's entry + t.  A frame
 *                 with f >= max_frames is not written; n_episodes x max_timesteps frames hold every env.
 *   starts[k][e]  the state episode k begins with, k < n_episodes: the state the launch finds when progress[e][0] == 0 and
 *                 progress[e][1] == 0 (k = 0), and the state after the reset that ends episode k - 1.
 * Rows that no step reached are left untouched.  Episode k of env e, with L_k its record's episode_length and s = L_0 + ... +
 * L_{k-1}: what the reference's Pedestrians.memory holds is starts[k][e] and then frames[s .. s + L_k - 1][e]; the leader's
 * memory is row N of those L_k frames (an evaluation that begins at a reset, as above: an env that begins it t steps into an
 * episode takes L_0 - t steps in episode 0).  max_steps = 5 repeated equals one long call, frames included: the index comes
 * from the progress word.
 * Refusals, decided on the host before anything is launched: the counterpart's own, in its order, then
 * EVAC_ERR_INVALID_ARGUMENT for a NULL capture, capture_envs outside 1..num_envs, max_frames < 1, a NULL frames or starts.
 * ONE kernel on `stream` (k_evaluate_capture*, evac_capture_api.hip), no host synchronisation, capturable.  A diagnostic face:
 * the generic configuration's kernels only, and no population form. */
typedef struct evac_eval_capture {
    int32_t capture_envs;   /* K: envs 0..K-1 of the handle, 1..num_envs */
    int32_t max_frames;     /* F >= 1 */
    float*  frames;         /* [F][K][N+1][3] */
    float*  starts;         /* [n_episodes][K][N+1][3] */
} evac_eval_capture_t;
int evac_policy_evaluate_capture(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy_or_null,
                                 int32_t n_episodes, int32_t max_steps,
                                 int32_t* progress,                   /* [E][4] in/out; zero it to begin */
                                 evac_episode_stats_t* episodes_out,  /* [n_episodes][E] */
                                 const double* norm_state_or_null, float obs_clip, float epsilon,
                                 const evac_eval_capture_t* capture, void* stream);
int evac_policy_evaluate_deepsets_capture(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy,
                                          int32_t n_episodes, int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out,
                                          const double* norm_state_or_null, float obs_clip, float epsilon,
                                          const evac_deepsets_t* encoder, const evac_eval_capture_t* capture, void* stream);
int evac_policy_evaluate_transformer_capture(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy,
                                             int32_t n_episodes, int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out,
                                             const double* norm_state_or_null, float obs_clip, float epsilon,
                                             const evac_transformer_t* encoder, const evac_eval_capture_t* capture, void* stream);

/* ---- The trainer's update: the other half of RPOAgent.learn() (rpo_agent.py:205-283) for the network above ----
 * No handle: buffers, sizes and a stream; arguments are validated on the host before anything touches a device, and errors
 * come back through the return code alone (evac_last_error keeps its meaning for handles).
 *
 * evac_gae: rpo_agent.py:205-220 in one launch, one lane per env, time walked backwards, in float32 and operation for operation
 * as torch evaluates the reference's lines (every product and sum rounded, no fma):
 *   nonterminal = 1 - done_next;  delta = (r + (gamma * v_next) * nonterminal) - v;
 *   adv = delta + ((float)(gamma * gae_lambda) * nonterminal) * adv_next;  returns = adv + v
 * gamma and gae_lambda are doubles because the reference's are Python floats: gamma is rounded to float32 where it meets a
 * tensor, the product gamma * gae_lambda is formed in double and rounded once.  The result is bit-equal to the reference's loop
 * under torch float32 on the CPU.  rewards / values / dones / advantages_out / returns_out [T][E], next_value / next_done [E]
 * (the outputs must not overlap the inputs).  EVAC_ERR_INVALID_ARGUMENT: a NULL pointer, n_steps < 1, n_envs < 1. */
int evac_gae(int32_t n_steps, int64_t n_envs, const float* rewards, const float* values, const float* dones,
             const float* next_value, const float* next_done, double gamma, double gae_lambda, float* advantages_out,
             float* returns_out, void* stream);

/* evac_rpo_minibatch_grad: rpo_agent.py:239-277 for ONE minibatch, up to and including loss.backward(): the forward pass of
 * actor and critic on b_obs[mb_inds] with the recorded actions, the RPO perturbation of the mean
 * (rpo_linear_agent_network.py:55-59), the loss as the reference composes it, and its gradient with respect to all 13 tensors,
 * WRITTEN (not accumulated: the reference calls zero_grad() first) into grads_out in the parameters' own layouts.
 *   mean = actor_mean(x) + z: z = the row of rpo_noise, or, when it is NULL, rpo_alpha * (2 u - 1) with u the 24-bit uniform of
 *   words 0 and 1 of Philox4x32-10 at counter (position in the minibatch, draw_counter low, draw_counter high, 'RPOZ') keyed by
 *   seed -- statistically equivalent to torch's uniform_, not bit-identical (as the policy noise above).  z is a constant for
 *   the gradient.
 *   newlogprob, entropy of Normal(mean, exp(logstd)); ratio = exp(newlogprob - b_logprobs); with norm_adv the advantages are
 *   normalised over THIS minibatch with the unbiased std and + 1e-8 (:250-251); pg_loss = mean(max(-A ratio, -A clamp(ratio,
 *   1 - clip, 1 + clip))) (:254-256); v_loss clipped or not (:260-271); loss = pg_loss - ent_coef * entropy + vf_coef * v_loss.
 *   Sub-gradients as torch takes them: clamp passes 1 on the closed interval, max splits a tie half and half.
 *   stats_out [8] = loss, pg_loss, v_loss, entropy, old_approx_kl, approx_kl, clipfrac, sum of squares of all gradient entries
 *   (what clip_grad_norm_ needs).
 * b_obs [B][D], b_actions [B][2], b_logprobs / b_advantages / b_returns / b_values [B]; mb_inds int64 [M] in DEVICE memory, values
 * in [0, B) (an index outside is clamped into the batch, never followed); rpo_noise [M][2] or NULL; workspace: 16-byte aligned,
 * evac_rpo_workspace_bytes(obs_dim, M) bytes, contents irrelevant before and after.
 * At most three launches on `stream`, no host synchronisation, capturable into a graph; the parameters are read when the kernels
 * run.  DETERMINISTIC: every gradient and statistic is a fixed-order sum (no floating-point atomics), the same bits on every run
 * and stream.  EVAC_ERR_INVALID_ARGUMENT: a NULL pointer (rpo_noise excepted), hidden != 64, obs_dim outside 1..396,
 * batch_size < 1, n_minibatch < 1 (< 2 with norm_adv: the unbiased std of one sample does not exist), a misaligned workspace. */
typedef struct evac_rpo_loss_config {
    float clip_coef, ent_coef, vf_coef, rpo_alpha;
    int32_t norm_adv, clip_vloss;
} evac_rpo_loss_config_t;
typedef struct evac_mlp_policy_grads {   /* the 13 tensors of evac_mlp_policy_t, writable, same layouts */
    float *actor_w1, *actor_b1, *actor_w2, *actor_b2, *actor_w3, *actor_b3, *actor_logstd;
    float *critic_w1, *critic_b1, *critic_w2, *critic_b2, *critic_w3, *critic_b3;
} evac_mlp_policy_grads_t;
/* bytes of workspace for a minibatch of M samples (EVAC_ERR_INVALID_ARGUMENT for obs_dim outside 1..396 or M outside 1..2^31-1) */
int64_t evac_rpo_workspace_bytes(int32_t obs_dim, int64_t n_minibatch);
int evac_rpo_minibatch_grad(const evac_mlp_policy_t* policy, const evac_rpo_loss_config_t* cfg, int64_t batch_size,
                            const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                            const float* b_returns, const float* b_values, int64_t n_minibatch, const int64_t* mb_inds,
                            const float* rpo_noise_or_null, uint64_t seed, uint64_t draw_counter,
                            const evac_mlp_policy_grads_t* grads_out, float* stats_out, void* workspace, void* stream);

/* The same gradient for the deep-sets leader, all 19 tensors: the contract above word for word (the loss, the sub-gradients, the
 * clamped indices, the Philox draw of z when rpo_noise is NULL, written not accumulated), with the network reading y = encode(x)
 * of evac_deepsets_t where the linear one reads x = b_obs[mb_inds[m]].  The 13 gradients go to grads_out, the encoder's six to
 * encoder_grads_out; stats_out[0..6] keep their meaning and stats_out[7] is the sum of squares of the gradient over all 19
 * tensors.  relu' is 1 where the pre-activation is > 0 and 0 otherwise (torch's convention).  The forward pass is the pooled
 * form of the kernels above, the same order of sums.  Six launches on `stream` (five without norm_adv): the encoder forwards, the
 * three of the call above on the encoded observations, the encoder backwards, its finish.  No host synchronisation, capturable;
 * the parameters are read when the kernels run.  DETERMINISTIC: every sum has a fixed order, no floating-point atomics, the same
 * bits on every run and stream.  workspace: 16-byte aligned, evac_deepsets_workspace_bytes(obs_dim, M) bytes (that is an error
 * code for the arguments the other size function refuses), contents irrelevant before and after.
 * EVAC_ERR_INVALID_ARGUMENT, before anything touches a device: everything the call above refuses; a NULL encoder, a NULL
 * encoder-gradient struct or a NULL tensor in either; hidden != 24; set_elem_dim outside 1..6; obs_dim not a multiple of
 * set_elem_dim or fewer than 3 rows; a rho_w that is not 16-byte aligned; a misaligned workspace. */
typedef struct evac_deepsets_grads {      /* the six tensors of evac_deepsets_t, writable, same layouts */
    float *phi_w1, *phi_b1, *phi_w2, *phi_b2, *rho_w, *rho_b;
} evac_deepsets_grads_t;
int64_t evac_deepsets_workspace_bytes(int32_t obs_dim, int64_t n_minibatch);
int evac_deepsets_minibatch_grad(const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder,
                                 const evac_rpo_loss_config_t* cfg, int64_t batch_size,
                                 const float* b_obs, const float* b_actions, const float* b_logprobs,
                                 const float* b_advantages, const float* b_returns, const float* b_values,
                                 int64_t n_minibatch, const int64_t* mb_inds, const float* rpo_noise_or_null,
                                 uint64_t seed, uint64_t draw_counter,
                                 const evac_mlp_policy_grads_t* grads_out, const evac_deepsets_grads_t* encoder_grads_out,
                                 float* stats_out, void* workspace, void* stream);

/* The same gradient for the transformer leader, all 13 + 16 num_blocks tensors (45 with two blocks): evac_rpo_minibatch_grad's
 * contract word for word (the loss, the sub-gradients, the clamped indices, the Philox draw of z when rpo_noise is NULL, written
 * not accumulated), with the network reading y = encode(x) of evac_transformer_t -- the eval-mode function the entries above
 * compute, the same formulas in the same order of sums -- where the linear one reads x = b_obs[mb_inds[m]].  The 13 gradients go
 * to grads_out, a block's 16 to encoder_grads_out->blocks[b]; blocks at index num_blocks and above are neither read nor written
 * (their pointers may be NULL).  stats_out[0..6] keep their meaning and stats_out[7] is the sum of squares of the gradient over
 * all 13 + 16 num_blocks tensors.  relu' is 1 where the pre-activation is > 0 and 0 otherwise (torch's convention).  wk's bias has
 * the exact gradient zero (a shift of every score of a row); it is computed like every other tensor and holds rounding.
 * 5 + num_blocks + norm_adv launches on `stream`: the encoder forwards, the three of evac_rpo_minibatch_grad on the encoded
 * observations, the gradient of the encoder's output, one launch per block backwards (the last block first), the finish.  No
 * host synchronisation, capturable; the parameters are read when the kernels run.  DETERMINISTIC: every sum has a fixed order, no
 * floating-point atomics, the same bits on every run and stream.  workspace: 16-byte aligned,
 * evac_transformer_workspace_bytes(obs_dim, M) bytes (sized for two blocks; an error code for the arguments
 * evac_rpo_workspace_bytes refuses), contents irrelevant before and after.
 * Refusals, before anything touches a device and through the return code alone; the encoder's sizes are looked at before its
 * pointers.  EVAC_ERR_INVALID_ARGUMENT: everything evac_rpo_minibatch_grad refuses; a NULL encoder or encoder-gradient struct; a
 * NULL tensor of a block in use, in either; elem_dim outside 1..6; obs_dim not a multiple of elem_dim or fewer than 3 tokens; a
 * misaligned workspace.  EVAC_ERR_UNSUPPORTED: num_heads != 3, dim_feedforward != 96, num_blocks outside 1..2, ln_eps != 1e-5f,
 * more than 64 tokens (N > 62). */
typedef struct evac_transformer_block_grads {   /* the 16 tensors of evac_transformer_block_t, writable, same order and layouts */
    float *wq, *bq, *wk, *bk, *wv, *bv, *dense_w, *dense_b, *ff1_w, *ff1_b, *ff2_w, *ff2_b, *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} evac_transformer_block_grads_t;
typedef struct evac_transformer_grads { evac_transformer_block_grads_t blocks[2]; } evac_transformer_grads_t;
int64_t evac_transformer_workspace_bytes(int32_t obs_dim, int64_t n_minibatch);
int evac_transformer_minibatch_grad(const evac_mlp_policy_t* policy, const evac_transformer_t* encoder,
                                    const evac_rpo_loss_config_t* cfg, int64_t batch_size,
                                    const float* b_obs, const float* b_actions, const float* b_logprobs,
                                    const float* b_advantages, const float* b_returns, const float* b_values,
                                    int64_t n_minibatch, const int64_t* mb_inds, const float* rpo_noise_or_null,
                                    uint64_t seed, uint64_t draw_counter,
                                    const evac_mlp_policy_grads_t* grads_out, const evac_transformer_grads_t* encoder_grads_out,
                                    float* stats_out, void* workspace, void* stream);

/* ---- The optimiser step: rpo_agent.py:278-279, clip_grad_norm_(max_grad_norm) and Adam(lr, eps = 1e-5).step(), on the device ----
 * Adam as torch.optim.Adam with betas, no weight decay, no amsgrad.  All in float32, EVERY OPERATION ROUNDED ON ITS OWN (no fused
 * multiply-add, IEEE division, correctly rounded sqrt), except the three scalars marked double, formed in double and rounded
 * once.  With s = the sum of squares of all gradient entries:
 *   x  = f32(max_grad_norm) / (sqrt(s) + f32(1e-6));  c = x > 1 ? 1 : x        (a NaN stays a NaN, as torch.clamp keeps it)
 *   t += 1;  P1 *= beta1;  P2 *= beta2                                         (int64 and two doubles; P1 = P2 = 1 at t = 0)
 *   a  = f32(-(lr / (1 - P1)));  q = f32(sqrt(1 - P2))                         (double, rounded once)
 *   w  = f32(1 - beta1);  b2 = f32(beta2);  u = f32(1 - beta2);  e = f32(eps)  ((1 - beta) formed in double)
 *   per element:  g' = g * c;  m' = m + w * (g' - m);  v' = v * b2 + (u * g') * g';  p' = p + (a * m') / (sqrt(v') / q + e)
 * The gradients are left holding g' (what clip_grad_norm_ leaves); m, v, p are updated in place.  This sequence in float64 is
 * torch's Adam to 1e-15; in float32 it is as accurate as torch's float32 Adam but NOT bit-equal to it (torch's kernels fuse
 * some of the products and differ between builds); the kernels are bit-equal to the sequence above.  P1, P2 are running
 * products (beta ** t to a few 1e-16) so that the step count lives on the device: a captured step counts when it is replayed.
 *
 * The optimiser's state is caller-owned device memory; all zero = a fresh optimiser.  The header's last 28 bytes are the
 * library's (an integer ticket of the running launch, zero between launches): keep them zero.  steps_run counts every step
 * since evac_rpo_update last cleared it; stop and epochs_run are written by evac_rpo_update's launches alone. */
typedef struct evac_adam_config { double lr, beta1, beta2, eps, max_grad_norm; } evac_adam_config_t;
typedef struct evac_adam_state {
    void* header;                         /* 64 bytes, 8-byte aligned: int64 t | double P1 | double P2 | int32 stop |
                                             int32 steps_run | int32 epochs_run | pad  (P1, P2 read as 1 while t == 0) */
    evac_mlp_policy_grads_t exp_avg, exp_avg_sq;     /* the 13 tensors' moments, the parameters' layouts */
} evac_adam_state_t;
/* evac_adam_step: the sequence above for gradients that are already in `grads` (a caller with its own backward pass).  `params`:
 * the 13 parameter tensors, writable (the tensors evac_mlp_policy_t names); grad_sumsq: one float in DEVICE memory, read when
 * the kernel runs.  ONE launch on `stream` (one element per thread; the last workgroup to finish, by an integer ticket, is the
 * one writer of the header), no host synchronisation, capturable; cfg's values are frozen by a capture (the step count is not).
 * EVAC_ERR_INVALID_ARGUMENT: a NULL pointer, obs_dim outside 1..396, a header that is not 8-byte aligned, lr not finite, a beta
 * outside [0, 1), eps <= 0, max_grad_norm <= 0. */
int evac_adam_step(const evac_mlp_policy_grads_t* params, const evac_mlp_policy_grads_t* grads, const evac_adam_state_t* state,
                   const evac_adam_config_t* cfg, int32_t obs_dim, const float* grad_sumsq, void* stream);
/* evac_rpo_minibatch_step: evac_rpo_minibatch_grad with the same arguments (same kernels, same bits in grads_out before the
 * clip and in stats_out: its sum of squares is that of the UNCLIPPED gradient), then evac_adam_step on `params` (the tensors of
 * `policy`, writable) from stats_out[7].  One launch more than evac_rpo_minibatch_grad, no host synchronisation, capturable:
 * replaying the captured call n times equals n calls with the same arguments (by-value arguments -- lr, draw_counter, seed --
 * are frozen by a capture, as for evac_rpo_minibatch_grad; mb_inds, rpo_noise and the step count are read on the device).
 * EVAC_ERR_INVALID_ARGUMENT: as evac_rpo_minibatch_grad and evac_adam_step. */
int evac_rpo_minibatch_step(const evac_mlp_policy_t* policy, const evac_rpo_loss_config_t* cfg, int64_t batch_size,
                            const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                            const float* b_returns, const float* b_values, int64_t n_minibatch, const int64_t* mb_inds,
                            const float* rpo_noise_or_null, uint64_t seed, uint64_t draw_counter,
                            const evac_mlp_policy_grads_t* grads_out, float* stats_out, void* workspace, void* stream,
                            const evac_mlp_policy_grads_t* params, const evac_adam_state_t* state,
                            const evac_adam_config_t* adam_cfg);
/* evac_rpo_update: rpo_agent.py:233-283 in ONE host call: for every epoch, for start in range(0, B, M), a minibatch step on
 * perms[epoch][start : start + M] (perms: int64 [n_epochs][B] in device memory).  Step k, counted over the whole call, draws its
 * RPO perturbation at first_draw_counter + k (or reads rpo_noise[k], [steps][M][2], the tail's rows first) and writes
 * stats_out[k] ([steps][8], steps = n_epochs * ceil(B / M) at most).  The tail minibatch of B mod M samples is run like the
 * others and skipped when it has fewer than 2 samples (1 without norm_adv).  `grads`: where the gradients live (they hold the
 * last step's clipped gradient afterwards).  target_kl WITHOUT THE HOST (use_target_kl != 0): the launch that finishes an
 * epoch's last minibatch sets header.stop when that minibatch's approx_kl > target_kl (:281-283); every later kernel of the
 * call returns at once when it sees the flag, touching nothing.  header.steps_run / epochs_run say what ran; rows of stats_out
 * beyond steps_run are left as they were.  The call clears stop, steps_run, epochs_run on the stream before its first step.
 * workspace: evac_rpo_workspace_bytes(obs_dim, M).  No host synchronisation; four launches per step.
 * EVAC_ERR_INVALID_ARGUMENT: as evac_rpo_minibatch_step, and n_epochs < 1. */
int evac_rpo_update(const evac_mlp_policy_t* policy, const evac_mlp_policy_grads_t* params, const evac_mlp_policy_grads_t* grads,
                    const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg, const evac_adam_state_t* state,
                    int64_t batch_size, const float* b_obs, const float* b_actions, const float* b_logprobs,
                    const float* b_advantages, const float* b_returns, const float* b_values, int64_t n_minibatch,
                    int32_t n_epochs, const int64_t* perms, const float* rpo_noise_or_null, uint64_t seed,
                    uint64_t first_draw_counter, int32_t use_target_kl, double target_kl, float* stats_out, void* workspace,
                    void* stream);

/* ---- The same three entries for the deep-sets leader: clip + Adam over all 19 tensors, the step, the whole update ----
 * The optimiser's sequence above runs over the 13 tensors of evac_mlp_policy_grads_t followed by the 6 of evac_deepsets_grads_t
 * with ONE clip coefficient c (from the sum of squares over all 19), ONE step count t and ONE header: what clip_grad_norm_ and
 * torch.optim.Adam do given all_tensors(net).  The state is evac_adam_state_t's with the encoder's moments after it; the
 * header is the same 64 bytes under the same rules. */
typedef struct evac_deepsets_adam_state {
    void* header;                                        /* evac_adam_state_t.header: same 64 bytes, same rules */
    evac_mlp_policy_grads_t exp_avg, exp_avg_sq;         /* the 13 tensors' moments */
    evac_deepsets_grads_t enc_exp_avg, enc_exp_avg_sq;   /* the encoder's six, the parameters' layouts */
} evac_deepsets_adam_state_t;
/* evac_deepsets_adam_step: evac_adam_step for 19 tensors.  params / enc_params: the parameter tensors, writable (the tensors
 * evac_mlp_policy_t and evac_deepsets_t name); the encoder's sizes follow evac_deepsets_t for (obs_dim, set_elem_dim): phi_w1
 * [24][set_elem_dim], phi_b1 [24], phi_w2 [24][24], phi_b2 [24], rho_w [obs_dim][24], rho_b [obs_dim].  grad_sumsq: one float
 * in DEVICE memory, the sum of squares over all 19 gradients (stats_out[7] of evac_deepsets_minibatch_grad), read when the
 * kernel runs.  ONE launch on `stream` (every tensor starts at a workgroup boundary, one element per thread; the last workgroup
 * to finish, by an integer ticket, is the one writer of the header), no host synchronisation, capturable.  The gradients are
 * left holding g * c; a NaN sum of squares makes every parameter and moment a NaN and still counts as a step.
 * EVAC_ERR_INVALID_ARGUMENT, before anything touches a device: everything evac_adam_step refuses; a NULL enc_params or
 * enc_grads or a NULL tensor in either or in the encoder's moments; set_elem_dim outside 1..6, not dividing obs_dim, or leaving
 * fewer than 3 rows. */
int evac_deepsets_adam_step(const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                            const evac_mlp_policy_grads_t* grads, const evac_deepsets_grads_t* enc_grads,
                            const evac_deepsets_adam_state_t* state, const evac_adam_config_t* cfg, int32_t obs_dim,
                            int32_t set_elem_dim, const float* grad_sumsq, void* stream);
/* evac_deepsets_minibatch_step: evac_deepsets_minibatch_grad with the same 20 arguments (same kernels, same bits in the
 * gradients before the clip and in stats_out: its sum of squares is that of the UNCLIPPED gradient over 19 tensors), then
 * evac_deepsets_adam_step on params / enc_params (the tensors of `policy` and `encoder`, writable) from stats_out[7].  One
 * launch more than the gradient (seven, six without norm_adv), no host synchronisation, capturable: replaying the captured call
 * n times equals n calls with the same arguments (what a capture freezes is what evac_rpo_minibatch_step's freezes).
 * EVAC_ERR_INVALID_ARGUMENT: as evac_deepsets_minibatch_grad and evac_deepsets_adam_step. */
int evac_deepsets_minibatch_step(const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder,
                                 const evac_rpo_loss_config_t* cfg, int64_t batch_size,
                                 const float* b_obs, const float* b_actions, const float* b_logprobs,
                                 const float* b_advantages, const float* b_returns, const float* b_values,
                                 int64_t n_minibatch, const int64_t* mb_inds, const float* rpo_noise_or_null,
                                 uint64_t seed, uint64_t draw_counter,
                                 const evac_mlp_policy_grads_t* grads_out, const evac_deepsets_grads_t* encoder_grads_out,
                                 float* stats_out, void* workspace, void* stream,
                                 const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                                 const evac_deepsets_adam_state_t* state, const evac_adam_config_t* adam_cfg);
/* evac_deepsets_update: evac_rpo_update's contract word for word for the deep-sets leader: perms [n_epochs][B]; step k draws at
 * first_draw_counter + k or reads rpo_noise[k]; stats_out[k]; the tail minibatch is run, or skipped below 2 samples (1 without
 * norm_adv); the call clears stop, steps_run, epochs_run on the stream before its first step; with use_target_kl the launch
 * that finishes an epoch's last minibatch sets header.stop when its approx_kl > target_kl, and every later kernel of the call
 * (the encoder's three as well) returns at once, touching nothing; rows of stats_out beyond steps_run are left as they were.
 * EQUIVALENCE: bit for bit the sequence of evac_deepsets_minibatch_step calls a host loop would make, with a break after an
 * epoch whose closing approx_kl > target_kl.  workspace: evac_deepsets_workspace_bytes(obs_dim, M).  No host synchronisation;
 * seven launches per step (six without norm_adv).
 * EVAC_ERR_INVALID_ARGUMENT: as evac_deepsets_minibatch_step, and n_epochs < 1. */
int evac_deepsets_update(const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder,
                         const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                         const evac_mlp_policy_grads_t* grads, const evac_deepsets_grads_t* enc_grads,
                         const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                         const evac_deepsets_adam_state_t* state, int64_t batch_size,
                         const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                         const float* b_returns, const float* b_values, int64_t n_minibatch, int32_t n_epochs,
                         const int64_t* perms, const float* rpo_noise_or_null, uint64_t seed, uint64_t first_draw_counter,
                         int32_t use_target_kl, double target_kl, float* stats_out, void* workspace, void* stream);

/* ---- The same three entries for the transformer leader: clip + Adam over all 13 + 16 num_blocks tensors, the step, the update ----
 * The optimiser's sequence above runs over the 13 tensors of evac_mlp_policy_grads_t followed by the 16 of every block in use in
 * evac_transformer_block_grads_t order, blocks[0] first (29 tensors with one block, 45 with two), with ONE clip coefficient c
 * (from the sum of squares over all 13 + 16 num_blocks), ONE step count t and ONE header: what clip_grad_norm_ and
 * torch.optim.Adam do given all_tensors(net).  The state is evac_adam_state_t's with the encoder's moments after it; the
 * header is the same 64 bytes under the same rules. */
typedef struct evac_transformer_adam_state {
    void* header;                                           /* evac_adam_state_t.header: same 64 bytes, same rules */
    evac_mlp_policy_grads_t exp_avg, exp_avg_sq;            /* the 13 tensors' moments */
    evac_transformer_grads_t enc_exp_avg, enc_exp_avg_sq;   /* the encoder's 16 per block, the parameters' layouts */
} evac_transformer_adam_state_t;
/* evac_transformer_adam_step: evac_adam_step for 13 + 16 num_blocks tensors.  params / enc_params: the parameter tensors,
 * writable (the tensors evac_mlp_policy_t and evac_transformer_t name); a block's sizes follow evac_transformer_block_t for
 * elem_dim = dm: wq, wk, wv [3 dm][dm], bq, bk, bv [3 dm], dense_w [dm][3 dm], dense_b [dm], ff1_w [96][dm], ff1_b [96],
 * ff2_w [dm][96], ff2_b, norm1_w, norm1_b, norm2_w, norm2_b [dm].  Blocks at index num_blocks and above are neither read nor
 * written (their pointers may be NULL everywhere).  grad_sumsq: one float in DEVICE memory, the sum of squares over all 13 + 16
 * num_blocks gradients (stats_out[7] of evac_transformer_minibatch_grad), read when the kernel runs.  ONE launch on `stream`
 * (every tensor starts at a workgroup boundary, one element per thread; the last workgroup to finish, by an integer ticket, is
 * the one writer of the header), no host synchronisation, capturable.  The gradients are left holding g * c; a NaN sum of
 * squares makes every parameter and moment a NaN and still counts as a step.
 * Refusals, before anything touches a device and through the return code alone; the encoder's sizes are looked at before its
 * pointers.  EVAC_ERR_INVALID_ARGUMENT: everything evac_adam_step refuses; a NULL enc_params or enc_grads; a NULL tensor of a
 * block in use in either or in the encoder's moments; elem_dim outside 1..6, not dividing obs_dim, or leaving fewer than 3
 * tokens.  EVAC_ERR_UNSUPPORTED: num_blocks outside 1..2, more than 64 tokens. */
int evac_transformer_adam_step(const evac_mlp_policy_grads_t* params, const evac_transformer_grads_t* enc_params,
                               const evac_mlp_policy_grads_t* grads, const evac_transformer_grads_t* enc_grads,
                               const evac_transformer_adam_state_t* state, const evac_adam_config_t* cfg, int32_t obs_dim,
                               int32_t elem_dim, int32_t num_blocks, const float* grad_sumsq, void* stream);
/* evac_transformer_minibatch_step: evac_transformer_minibatch_grad with the same 20 arguments (same kernels, same bits in the
 * gradients before the clip and in stats_out: its sum of squares is that of the UNCLIPPED gradient over 13 + 16 num_blocks
 * tensors), then evac_transformer_adam_step on params / enc_params (the tensors of `policy` and `encoder`, writable) from
 * stats_out[7].  One launch more than the gradient (6 + num_blocks + norm_adv), no host synchronisation, capturable: replaying
 * the captured call n times equals n calls with the same arguments (what a capture freezes is what evac_rpo_minibatch_step's
 * freezes).  Refusals: as evac_transformer_minibatch_grad, then as evac_transformer_adam_step, each with its own code. */
int evac_transformer_minibatch_step(const evac_mlp_policy_t* policy, const evac_transformer_t* encoder,
                                    const evac_rpo_loss_config_t* cfg, int64_t batch_size,
                                    const float* b_obs, const float* b_actions, const float* b_logprobs,
                                    const float* b_advantages, const float* b_returns, const float* b_values,
                                    int64_t n_minibatch, const int64_t* mb_inds, const float* rpo_noise_or_null,
                                    uint64_t seed, uint64_t draw_counter,
                                    const evac_mlp_policy_grads_t* grads_out, const evac_transformer_grads_t* encoder_grads_out,
                                    float* stats_out, void* workspace, void* stream,
                                    const evac_mlp_policy_grads_t* params, const evac_transformer_grads_t* enc_params,
                                    const evac_transformer_adam_state_t* state, const evac_adam_config_t* adam_cfg);
/* evac_transformer_update: evac_rpo_update's contract word for word for the transformer leader: perms [n_epochs][B]; step k
 * draws at first_draw_counter + k or reads rpo_noise[k]; stats_out[k]; the tail minibatch is run, or skipped below 2 samples (1
 * without norm_adv); the call clears stop, steps_run, epochs_run on the stream before its first step; with use_target_kl the
 * launch that finishes an epoch's last minibatch sets header.stop when its approx_kl > target_kl, and every later kernel of the
 * call (the encoder's as well) returns at once, touching nothing; rows of stats_out beyond steps_run are left as they were.
 * EQUIVALENCE: bit for bit the sequence of evac_transformer_minibatch_step calls a host loop would make, with a break after an
 * epoch whose closing approx_kl > target_kl.  workspace: evac_transformer_workspace_bytes(obs_dim, M).  No host
 * synchronisation; 6 + num_blocks + norm_adv launches per step.
 * Refusals: as evac_transformer_minibatch_step, and EVAC_ERR_INVALID_ARGUMENT for n_epochs < 1. */
int evac_transformer_update(const evac_mlp_policy_t* policy, const evac_transformer_t* encoder,
                            const evac_mlp_policy_grads_t* params, const evac_transformer_grads_t* enc_params,
                            const evac_mlp_policy_grads_t* grads, const evac_transformer_grads_t* enc_grads,
                            const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                            const evac_transformer_adam_state_t* state, int64_t batch_size,
                            const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                            const float* b_returns, const float* b_values, int64_t n_minibatch, int32_t n_epochs,
                            const int64_t* perms, const float* rpo_noise_or_null, uint64_t seed, uint64_t first_draw_counter,
                            int32_t use_target_kl, double target_kl, float* stats_out, void* workspace, void* stream);

/* evac_rpo_update_population: evac_rpo_update for n_learners learners in one set of launches: the learner is one more grid
 * dimension of each of the four kernels of a step, so the launch count per minibatch step is that of one learner.
 *   policy / params / grads / state: learner 0's tensors; learner s's are s x the strides further (param_strides for policy and
 *   params, grad_strides, moment_strides for exp_avg and exp_avg_sq, in floats) and its 64-byte header s x header_stride_bytes.
 *   The batch arrays are COMMON: batch_size rows, of which each learner reads its own through its index list.
 *   perms int64 [S][n_epochs][learner_batch_size] in device memory: learner s's minibatches are consecutive n_minibatch-long
 *   pieces of perms[s][epoch], exactly as evac_rpo_update cuts perms[epoch]; the VALUES are rows of the common arrays (an index
 *   outside [0, batch_size) is clamped into the batch, never followed).  For the storage of evac_policy_rollout_population,
 *   flattened, sample i of learner s is row (i / E_l) x (S x E_l) + s x E_l + i % E_l.
 *   rpo_noise_or_null [S][steps][M][2];  stats_out [S][steps][8];  seeds [S] and first_draw_counters [S]: HOST arrays, read
 *   during the call (learners that stopped early have run fewer steps, so their counters differ).
 *   workspace: evac_rpo_population_workspace_bytes(obs_dim, M, S) bytes, 16-byte aligned: S slices of
 *   evac_rpo_workspace_bytes(obs_dim, M) rounded up to 128 bytes each.
 * Every learner has its own workspace slice, ticket words, header and statistics rows: no learner reads another's and nothing
 * waits across learners.  A learner whose stop flag is set (target_kl) returns at once in every later kernel while the others go
 * on; header s says what learner s ran.  The call clears every learner's stop / steps_run / epochs_run on the stream before
 * its first step.  EQUIVALENCE: learner s's parameters, moments, header, gradients and statistics rows are, bit for bit, those
 * of evac_rpo_update called with learner s's tensors, perms[s], seeds[s], first_draw_counters[s] and the same common batch
 * (equivalently: with the learner's own rows gathered into a batch of learner_batch_size and its own positions as indices).
 * No host synchronisation, capturable (seeds and counters are frozen by a capture, as evac_rpo_update's).
 * EVAC_ERR_INVALID_ARGUMENT, decided on the host before anything touches a device: as evac_rpo_update (a NULL pointer, hidden
 * != 64, obs_dim outside 1..396, n_minibatch < 1 or < 2 with norm_adv, a misaligned workspace, ...), and n_learners outside
 * 1..EVAC_MAX_LEARNERS, a NULL strides / seeds / first_draw_counters, learner_batch_size < 1, and with n_learners > 1 a stride
 * smaller than its tensor (0 included) or a header stride that is below 64 or not a multiple of 8. */
int64_t evac_rpo_population_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners);
int evac_rpo_update_population(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_mlp_policy_grads_t* params,
                               const evac_mlp_policy_grads_t* grads, const evac_mlp_policy_strides_t* param_strides,
                               const evac_mlp_policy_strides_t* grad_strides, const evac_mlp_policy_strides_t* moment_strides,
                               int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg,
                               const evac_adam_config_t* adam_cfg, const evac_adam_state_t* state, int64_t batch_size,
                               const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                               const float* b_returns, const float* b_values, int64_t learner_batch_size, int64_t n_minibatch,
                               int32_t n_epochs, const int64_t* perms, const float* rpo_noise_or_null, const uint64_t* seeds,
                               const uint64_t* first_draw_counters, int32_t use_target_kl, double target_kl, float* stats_out,
                               void* workspace, void* stream);

/* ---- Sweeps: a population whose learners differ in their float-valued hyperparameters ----
 * evac_learner_hyper_t: one learner's values.  Callers pass a HOST array [n_learners], read during the call; the values travel
 * to the kernels by value in the kernel-argument segment (as the seeds and draw counters do), so the calls stay free of host
 * synchronisation and capturable, and a capture freezes them.  Number types are the lone trainer's: learning_rate and target_kl
 * are used as doubles, the loss coefficients and max_grad_norm as float32, and gamma / gae_lambda as evac_gae uses them
 * ((float)gamma, (float)(gamma * gae_lambda) with the product formed in double).  What fixes launch geometry or storage shape
 * (n_minibatch, n_epochs, norm_adv, clip_vloss, Adam's betas and eps) stays one value for all learners.
 * Every entry below refuses (EVAC_ERR_INVALID_ARGUMENT, on the host, before anything touches a device) a NULL hypers and, for
 * any learner: a non-finite learning_rate, gamma or gae_lambda; max_grad_norm <= 0 (or NaN); clip_coef < 0 or rpo_alpha < 0 (or
 * NaN); with use_target_kl, a NaN target_kl. */
typedef struct evac_learner_hyper {
    double learning_rate, target_kl, gamma, gae_lambda;
    float clip_coef, ent_coef, vf_coef, rpo_alpha, max_grad_norm;
    int32_t use_target_kl;                 /* 0: target_kl is ignored and the learner never stops early */
} evac_learner_hyper_t;

/* evac_gae_learners: evac_gae over the storage of a population: env e belongs to learner e / envs_per_learner and uses
 * hypers[that learner].gamma / gae_lambda.  EQUIVALENCE: learner s's columns are, bit for bit, evac_gae on those columns alone
 * with hypers[s].gamma and hypers[s].gae_lambda.  Refused as evac_gae, and envs_per_learner < 1, n_learners outside
 * 1..EVAC_MAX_LEARNERS, n_envs != n_learners x envs_per_learner, and the hypers as above. */
int evac_gae_learners(int32_t n_steps, int64_t n_envs, const float* rewards, const float* values, const float* dones,
                      const float* next_value, const float* next_done, int64_t envs_per_learner, int32_t n_learners,
                      const evac_learner_hyper_t* hypers, float* advantages_out, float* returns_out, void* stream);

/* evac_policy_rollout_sweep: evac_policy_rollout_population with a per-learner gamma of the reward normaliser (the reference
 * wraps a learner's env with its training gamma).  Of hypers only gamma is read: learner s's chain runs with (float)hypers[s].gamma;
 * the `gamma` argument is not used.  Without the chain (norm_state NULL) gamma does not enter collection and the call is
 * evac_policy_rollout_population.  EQUIVALENCE: learner s's columns are, bit for bit, evac_policy_rollout on a handle of its
 * envs with gamma = (float)hypers[s].gamma.  Refused as evac_policy_rollout_population, and the hypers as above. */
int evac_policy_rollout_sweep(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                              const evac_mlp_policy_strides_t* strides, int32_t n_steps, float* next_obs, float* next_done,
                              float* obs_out, float* actions_out, float* logprob_out, float* value_out, float* reward_out,
                              float* done_out, float* next_value_out, evac_episode_stats_t* final_stats_or_null,
                              double* norm_state_or_null, float gamma, float obs_clip, float reward_clip, float epsilon,
                              const evac_learner_hyper_t* hypers, void* stream);

/* evac_rpo_update_sweep: evac_rpo_update_population with hypers[s] in place of the one configuration: learner s's loss runs
 * with hypers[s].clip_coef / ent_coef / vf_coef / rpo_alpha and its optimiser with learning_rate / max_grad_norm / use_target_kl
 * / target_kl.  loss_cfg gives norm_adv and clip_vloss (its four coefficients are not used), adam_cfg the betas and eps (its lr
 * and max_grad_norm are not used, but must be valid).  A learner with use_target_kl == 0 never sets its stop flag, whatever its
 * neighbours do.  EQUIVALENCE: learner s is, bit for bit, evac_rpo_update with learner s's tensors, perms[s], seeds[s],
 * first_draw_counters[s], a loss_cfg and adam_cfg holding hypers[s]'s values, and hypers[s].use_target_kl / target_kl.  The
 * same number of launches as evac_rpo_update_population; no host synchronisation, capturable.  Refused as
 * evac_rpo_update_population, and the hypers as above. */
int evac_rpo_update_sweep(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_mlp_policy_grads_t* params,
                          const evac_mlp_policy_grads_t* grads, const evac_mlp_policy_strides_t* param_strides,
                          const evac_mlp_policy_strides_t* grad_strides, const evac_mlp_policy_strides_t* moment_strides,
                          int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg,
                          const evac_adam_config_t* adam_cfg, const evac_adam_state_t* state, int64_t batch_size,
                          const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                          const float* b_returns, const float* b_values, int64_t learner_batch_size, int64_t n_minibatch,
                          int32_t n_epochs, const int64_t* perms, const float* rpo_noise_or_null, const uint64_t* seeds,
                          const uint64_t* first_draw_counters, const evac_learner_hyper_t* hypers, float* stats_out,
                          void* workspace, void* stream);

/* ---- Populations of deep-sets leaders: S learners of ONE configuration, each with its own set encoder ----
 * The two population entries above for the network of evac_deepsets_t: 19 stacked tensors per learner.  evac_deepsets_strides_t
 * is evac_mlp_policy_strides_t's sibling for the encoder's six: floats from learner s to learner s + 1, per tensor.  The
 * one-launch evaluation of such learners is evac_policy_evaluate_population_deepsets, below.  Sweeps (per-learner
 * hyperparameters) of such learners do not exist. */
typedef struct evac_deepsets_strides {     /* floats from learner s to learner s + 1, per tensor of evac_deepsets_t */
    int64_t phi_w1, phi_b1, phi_w2, phi_b2, rho_w, rho_b;
} evac_deepsets_strides_t;
/* evac_policy_rollout_population_deepsets: evac_policy_rollout_population with the set encoder in front of every learner's
 * actor-critic.  `policy` / `encoder` hold learner 0's tensors, learner s's are s x strides / enc_strides further; storage,
 * norm_state and env state as evac_policy_rollout_population's.  EQUIVALENCE: the call writes, bit for bit, what S calls of
 * evac_policy_rollout_deepsets write -- call s with learner s's 19 tensors on a handle of E_l envs with the same seed,
 * env_id_offset = this handle's + s E_l and learner s's share of the state -- into the learner's columns [s E_l, (s + 1) E_l) of
 * every array.  ONE launch of ceil(E_l / 16) CU-wide workgroups per learner; a workgroup never mixes learners.
 * Refused as evac_policy_rollout_deepsets and as evac_policy_rollout_population (EVAC_ERR_UNSUPPORTED above 64 pedestrians;
 * EVAC_ERR_INVALID_ARGUMENT otherwise), and a NULL enc_strides, and with n_learners > 1 an encoder stride smaller than its
 * tensor (0 included) or a rho_w stride that is no multiple of 4 floats (its rows are read as 16-byte vectors). */
int evac_policy_rollout_population_deepsets(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                            const evac_mlp_policy_strides_t* strides, const evac_deepsets_t* encoder,
                                            const evac_deepsets_strides_t* enc_strides, int32_t n_steps,
                                            float* next_obs, float* next_done,
                                            float* obs_out, float* actions_out, float* logprob_out,
                                            float* value_out, float* reward_out, float* done_out,
                                            float* next_value_out, evac_episode_stats_t* final_stats_or_null,
                                            double* norm_state_or_null, float gamma, float obs_clip, float reward_clip,
                                            float epsilon, void* stream);
/* evac_policy_evaluate_population_deepsets: evac_policy_evaluate_population with the set encoder in front of every learner's
 * actor, i.e. evac_policy_evaluate_deepsets under the policy agents for n_learners learners in ONE launch.  `policy` / `encoder`
 * hold learner 0's tensors, learner s's are s x strides / enc_strides further (the actor and the encoder alone are read); learner s
 * evaluates in envs [s E_l, (s + 1) E_l) of the handle, and progress [S E_l][4], episodes_out [n_episodes][S E_l] and norm_state
 * [S E_l][evac_norm_state_doubles(h)] are indexed by the handle's env.  EQUIVALENCE: the call writes, bit for bit, what S calls of
 * evac_policy_evaluate_deepsets write -- call s with learner s's 19 tensors on a handle of E_l envs with the same seed, learner
 * s's share of the state and its rows of norm_state -- into learner s's columns of progress and episodes_out and its share of the
 * state.  With shared_episodes != 0 that handle's env_id_offset is this handle's: env i of EVERY learner has the global id of
 * env i, so all learners meet the same reset draws and pedestrian noise (and, in sample mode, the same z).  With
 * shared_episodes == 0 it is this handle's + s E_l, the id convention of evac_policy_rollout_population_deepsets: sample mode
 * with max_steps = T is then that call's env side bit for bit.
 * ceil(E_l / 16) CU-wide workgroups per learner; a workgroup never mixes learners; the launch lasts as long as its longest env.
 * EVAC_ERR_UNSUPPORTED / EVAC_ERR_INVALID_ARGUMENT, decided on the host before anything is launched, in this order: a NULL
 * strides / enc_strides; EVAC_AGENT_VACUUM_CLEANER (no network: evac_policy_evaluate runs it) and an unknown agent; as
 * evac_policy_evaluate_deepsets of the counts, the buffers and the two networks; n_learners outside 1..EVAC_MAX_LEARNERS, a
 * number of envs that n_learners does not divide, and with n_learners > 1 a policy or encoder stride smaller than its tensor
 * (0 included) or a rho_w stride that is no multiple of 4 floats; last, rooms of more than 64 pedestrians.  The handle is joined
 * first; ONE kernel on `stream`, no host synchronisation, capturable. */
int evac_policy_evaluate_population_deepsets(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                             const evac_mlp_policy_strides_t* strides, const evac_deepsets_t* encoder,
                                             const evac_deepsets_strides_t* enc_strides, int32_t agent, int32_t shared_episodes,
                                             int32_t n_episodes, int32_t max_steps,
                                             int32_t* progress,                   /* [S E_l][4] in/out; zero it to begin */
                                             evac_episode_stats_t* episodes_out,  /* [n_episodes][S E_l] */
                                             const double* norm_state_or_null, float obs_clip, float epsilon, void* stream);
/* evac_deepsets_update_population: evac_deepsets_update for n_learners learners in one set of launches, with
 * evac_rpo_update_population's argument list and contract: ONE common batch, perms [S][n_epochs][learner_batch_size] whose
 * values are rows of the common arrays, rpo_noise_or_null [S][steps][M][2], stats_out [S][steps][8], HOST seeds [S] and
 * first_draw_counters [S], the 64-byte headers header_stride_bytes apart.  It adds the encoder (learner 0's), its parameters,
 * gradients and moments (evac_deepsets_adam_state_t) and their strides: enc_param_strides for encoder and enc_params,
 * enc_grad_strides, enc_moment_strides for enc_exp_avg and enc_exp_avg_sq.
 *   workspace: evac_deepsets_population_workspace_bytes(obs_dim, M, S) bytes, 16-byte aligned: S slices of
 *   evac_deepsets_workspace_bytes(obs_dim, M) (a multiple of 256 bytes, every part of a slice a multiple of 256 bytes from the
 *   base: no two learners' ticket words or partials share a 128-byte line, whatever the base's alignment), then the learners'
 *   encoded observations, gathered columns and index lists as one common batch [S][M][..] that the actor-critic's kernels read with learner s's index list s M + m.
 * EQUIVALENCE: learner s's 19 parameters, 2 x 19 moments, 19 gradients, header and statistics rows are, bit for bit, those of
 * evac_deepsets_update called with learner s's tensors, perms[s], seeds[s], first_draw_counters[s] and the same common batch.
 * A learner whose stop flag is set (target_kl) returns at the top of every later kernel, the encoder's three included, touching
 * nothing, while the others go on.  No learner reads another's memory and nothing waits across learners: every ticket is an
 * integer atomicAdd whose result is compared, and no kernel spins.  Launches per minibatch step are those of one learner: seven
 * (six without norm_adv: the encoder forwards, the advantage statistics, the gradient, its finish, the encoder backwards, its
 * finish, the optimiser), plus one launch per call that clears every learner's stop / steps_run / epochs_run.  No host
 * synchronisation, capturable (seeds and counters are frozen by a capture).
 * EVAC_ERR_INVALID_ARGUMENT, decided on the host before anything touches a device: as evac_deepsets_update and as
 * evac_rpo_update_population, and a NULL encoder strides struct, and with n_learners > 1 an encoder stride smaller than its
 * tensor (0 included) or a rho_w stride that is no multiple of 4 floats.
 * evac_deepsets_population_workspace_bytes: the workspace's size, or EVAC_ERR_INVALID_ARGUMENT where
 * evac_deepsets_workspace_bytes gives it or n_learners is outside 1..EVAC_MAX_LEARNERS. */
int64_t evac_deepsets_population_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners);
int evac_deepsets_update_population(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder,
                                    const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                                    const evac_mlp_policy_grads_t* grads, const evac_deepsets_grads_t* enc_grads,
                                    const evac_mlp_policy_strides_t* param_strides, const evac_deepsets_strides_t* enc_param_strides,
                                    const evac_mlp_policy_strides_t* grad_strides, const evac_deepsets_strides_t* enc_grad_strides,
                                    const evac_mlp_policy_strides_t* moment_strides, const evac_deepsets_strides_t* enc_moment_strides,
                                    int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg,
                                    const evac_adam_config_t* adam_cfg, const evac_deepsets_adam_state_t* state, int64_t batch_size,
                                    const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                                    const float* b_returns, const float* b_values, int64_t learner_batch_size, int64_t n_minibatch,
                                    int32_t n_epochs, const int64_t* perms, const float* rpo_noise_or_null, const uint64_t* seeds,
                                    const uint64_t* first_draw_counters, int32_t use_target_kl, double target_kl, float* stats_out,
                                    void* workspace, void* stream);

/* ---- Populations of transformer leaders on a handle's envs: S learners, each with its own attention encoder ----
 * Collection and whole-episode evaluation for the network of evac_transformer_t: 13 + 16 num_blocks stacked tensors per learner
 * (45 with two blocks).  evac_transformer_strides_t is evac_mlp_policy_strides_t's sibling for the encoder's blocks: floats from
 * learner s to learner s + 1, per tensor of evac_transformer_block_t; the strides of a block at index num_blocks and above are
 * never looked at.  num_blocks, elem_dim and use_resid are one value per population.  The UPDATE of such a population (gradient
 * and optimiser with the learner as a grid dimension) is evac_transformer_update_population below, under one configuration for
 * all learners.  Sweeps (per-learner hyperparameters) of such learners do not exist. */
typedef struct evac_transformer_block_strides {   /* floats from learner s to learner s + 1, per tensor of evac_transformer_block_t */
    int64_t wq, bq, wk, bk, wv, bv, dense_w, dense_b, ff1_w, ff1_b, ff2_w, ff2_b, norm1_w, norm1_b, norm2_w, norm2_b;
} evac_transformer_block_strides_t;
typedef struct evac_transformer_strides { evac_transformer_block_strides_t blocks[2]; } evac_transformer_strides_t;
/* evac_policy_rollout_population_transformer: evac_policy_rollout_population with the attention encoder in front of every
 * learner's actor-critic.  `policy` / `encoder` hold learner 0's tensors, learner s's are s x strides / enc_strides further;
 * storage, norm_state and env state as evac_policy_rollout_population's.  EQUIVALENCE: the call writes, bit for bit, what S calls
 * of evac_policy_rollout_transformer write -- call s with learner s's tensors on a handle of E_l envs with the same seed,
 * env_id_offset = this handle's + s E_l and learner s's share of the state -- into the learner's columns [s E_l, (s + 1) E_l) of
 * every array.  ONE launch of ceil(E_l / 16) CU-wide workgroups per learner; a workgroup never mixes learners.
 * Refused as evac_policy_rollout_transformer and as evac_policy_rollout_population (EVAC_ERR_UNSUPPORTED for more than 62
 * pedestrians -- one wave holds the N + 2 tokens --, the gravity observation and the encoder's sizes; EVAC_ERR_INVALID_ARGUMENT
 * otherwise), and a NULL enc_strides, and with n_learners > 1 an encoder stride of a block in use smaller than its tensor (0
 * included).  No alignment is asked of the encoder's strides: its tensors are read as scalars. */
int evac_policy_rollout_population_transformer(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                               const evac_mlp_policy_strides_t* strides, const evac_transformer_t* encoder,
                                               const evac_transformer_strides_t* enc_strides, int32_t n_steps,
                                               float* next_obs, float* next_done,
                                               float* obs_out, float* actions_out, float* logprob_out,
                                               float* value_out, float* reward_out, float* done_out,
                                               float* next_value_out, evac_episode_stats_t* final_stats_or_null,
                                               double* norm_state_or_null, float gamma, float obs_clip, float reward_clip,
                                               float epsilon, void* stream);
/* evac_policy_evaluate_population_transformer: evac_policy_evaluate_population with the attention encoder in front of every
 * learner's actor, i.e. evac_policy_evaluate_transformer under the policy agents for n_learners learners in ONE launch.  `policy`
 * / `encoder` hold learner 0's tensors, learner s's are s x strides / enc_strides further (the actor and the encoder alone are
 * read); learner s evaluates in envs [s E_l, (s + 1) E_l) of the handle, and progress [S E_l][4], episodes_out [n_episodes][S E_l]
 * and norm_state [S E_l][evac_norm_state_doubles(h)] are indexed by the handle's env.  EQUIVALENCE: the call writes, bit for bit,
 * what S calls of evac_policy_evaluate_transformer write -- call s with learner s's tensors on a handle of E_l envs with the same
 * seed, learner s's share of the state and its rows of norm_state -- into learner s's columns of progress and episodes_out and its
 * share of the state.  With shared_episodes != 0 that handle's env_id_offset is this handle's: env i of EVERY learner has the
 * global id of env i, so all learners meet the same reset draws and pedestrian noise (and, in sample mode, the same z).  With
 * shared_episodes == 0 it is this handle's + s E_l, the id convention of evac_policy_rollout_population_transformer: sample mode
 * with max_steps = T is then that call's env side bit for bit.
 * ceil(E_l / 16) CU-wide workgroups per learner; a workgroup never mixes learners; the launch lasts as long as its longest env.
 * EVAC_ERR_UNSUPPORTED / EVAC_ERR_INVALID_ARGUMENT, decided on the host before anything is launched, in this order: a NULL
 * strides / enc_strides; EVAC_AGENT_VACUUM_CLEANER (no network: evac_policy_evaluate runs it) and an unknown agent; as
 * evac_policy_evaluate_transformer of the counts, the buffers and the two networks; n_learners outside 1..EVAC_MAX_LEARNERS, a
 * number of envs that n_learners does not divide, and with n_learners > 1 a policy stride, or an encoder stride of a block in use,
 * smaller than its tensor (0 included); last, rooms of more than 64 pedestrians.  The handle is joined first; ONE kernel on
 * `stream`, no host synchronisation, capturable. */
int evac_policy_evaluate_population_transformer(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                                const evac_mlp_policy_strides_t* strides, const evac_transformer_t* encoder,
                                                const evac_transformer_strides_t* enc_strides, int32_t agent, int32_t shared_episodes,
                                                int32_t n_episodes, int32_t max_steps,
                                                int32_t* progress,                   /* [S E_l][4] in/out; zero it to begin */
                                                evac_episode_stats_t* episodes_out,  /* [n_episodes][S E_l] */
                                                const double* norm_state_or_null, float obs_clip, float epsilon, void* stream);
/* evac_transformer_update_population: evac_transformer_update for n_learners learners in one set of launches, with
 * evac_deepsets_update_population's argument list and contract word for word, the attention encoder's types where the set
 * encoder's stood: ONE common batch, perms [S][n_epochs][learner_batch_size] whose values are rows of the common arrays,
 * rpo_noise_or_null [S][steps][M][2], stats_out [S][steps][8], HOST seeds [S] and first_draw_counters [S], the 64-byte headers
 * header_stride_bytes apart; the encoder (learner 0's), its parameters, gradients and moments (evac_transformer_adam_state_t)
 * and their strides: enc_param_strides for encoder and enc_params, enc_grad_strides, enc_moment_strides for enc_exp_avg and
 * enc_exp_avg_sq.
 *   workspace: evac_transformer_population_workspace_bytes(obs_dim, M, S) bytes, 16-byte aligned: S slices of
 *   evac_transformer_workspace_bytes(obs_dim, M) rounded up to whole 256-byte parts (every part of a slice a multiple of 256
 *   bytes from the base: no two learners' ticket words or partials share a 128-byte line, whatever the base's alignment), then
 *   the learners' encoded observations, gathered columns and index lists as one common batch [S][M][..] that the actor-critic's
 *   kernels read with learner s's index list s M + m.
 * EQUIVALENCE: learner s's 13 + 16 num_blocks parameters, twice as many moments, as many gradients, header and statistics rows
 * are, bit for bit, those of evac_transformer_update called with learner s's tensors, perms[s], seeds[s],
 * first_draw_counters[s] and the same common batch.  A learner whose stop flag is set (target_kl) returns at the top of every
 * later kernel, the encoder's four included (k_tf_encode then does not clear the finish's ticket either), touching nothing,
 * while the others go on.  No learner reads another's memory and nothing waits across learners: every ticket is an integer
 * atomicAdd whose result is compared, and no kernel spins.  Launches per minibatch step are those of one learner:
 * 6 + num_blocks + norm_adv (the encoder forwards, the advantage statistics, the gradient, its finish, dX, one launch per block
 * backwards, the encoder's finish, the optimiser), plus one launch per call that clears every learner's stop / steps_run /
 * epochs_run.  No host synchronisation, no device allocation, capturable (seeds and counters are frozen by a capture).
 * EVAC_ERR_INVALID_ARGUMENT / EVAC_ERR_UNSUPPORTED, decided on the host before anything touches a device, in this order: as
 * evac_transformer_minibatch_grad of the gradient's arguments; a NULL state; as evac_rpo_update_population; a NULL encoder
 * strides struct; with n_learners > 1 an encoder stride of a block in use smaller than its tensor (0 included; the strides of a
 * block not in use are never looked at, and no alignment is asked); as evac_transformer_adam_step.
 * evac_transformer_population_workspace_bytes: the workspace's size, or EVAC_ERR_INVALID_ARGUMENT where
 * evac_transformer_workspace_bytes gives it or n_learners is outside 1..EVAC_MAX_LEARNERS. */
int64_t evac_transformer_population_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners);
int evac_transformer_update_population(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_transformer_t* encoder,
                                       const evac_mlp_policy_grads_t* params, const evac_transformer_grads_t* enc_params,
                                       const evac_mlp_policy_grads_t* grads, const evac_transformer_grads_t* enc_grads,
                                       const evac_mlp_policy_strides_t* param_strides, const evac_transformer_strides_t* enc_param_strides,
                                       const evac_mlp_policy_strides_t* grad_strides, const evac_transformer_strides_t* enc_grad_strides,
                                       const evac_mlp_policy_strides_t* moment_strides, const evac_transformer_strides_t* enc_moment_strides,
                                       int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg,
                                       const evac_adam_config_t* adam_cfg, const evac_transformer_adam_state_t* state, int64_t batch_size,
                                       const float* b_obs, const float* b_actions, const float* b_logprobs, const float* b_advantages,
                                       const float* b_returns, const float* b_values, int64_t learner_batch_size, int64_t n_minibatch,
                                       int32_t n_epochs, const int64_t* perms, const float* rpo_noise_or_null, const uint64_t* seeds,
                                       const uint64_t* first_draw_counters, int32_t use_target_kl, double target_kl, float* stats_out,
                                       void* workspace, void* stream);

/* ---- SWEEPS OF THE ENCODER LEADERS: a population of deep-sets or transformer leaders with a configuration per learner ----
 * What evac_policy_rollout_sweep / evac_rpo_update_sweep are to the linear population's entries, for the two encoder leaders:
 * `hypers` is the HOST array evac_learner_hyper_t[n_learners] above, and learner s is, bit for bit, the lone learner with its
 * own values (evac_deepsets_update / evac_transformer_update with hypers[s]'s clip_coef, ent_coef, vf_coef, rpo_alpha,
 * target_kl and an optimiser at its learning_rate / max_grad_norm; collection on a handle wrapped with its gamma).  The number
 * types are the lone entries': learning_rate and target_kl double, the four coefficients and max_grad_norm float32, the reward
 * normaliser's gamma (float)gamma.  evac_gae_learners serves these populations as it serves the linear one.
 *   evac_policy_rollout_sweep_deepsets / _transformer: evac_policy_rollout_population_deepsets / _transformer's arguments with
 *   `hypers` in front of the stream; only gamma of it is read, in place of the argument `gamma`.  With a NULL norm_state gamma
 *   does not enter collection: `hypers` is checked all the same and the population's kernel runs.  Refusals: the population
 *   entry's in its order; behind the learners' strides a NULL `hypers` or values that evac_learner_hyper_t refuses
 *   (EVAC_ERR_INVALID_ARGUMENT), before the alignment of actions_out.
 *   evac_deepsets_update_sweep / evac_transformer_update_sweep: evac_*_update_population's arguments with `hypers` in place of
 *   use_target_kl, target_kl (loss_cfg's four coefficients and adam_cfg's lr / max_grad_norm are checked and then replaced per
 *   learner; norm_adv, clip_vloss, betas and eps are everybody's).  The launches are the population entry's, the gradient and
 *   its finish with every learner's coefficients in their arguments, plus ONE small launch per call that copies the learners'
 *   lr / max_grad_norm / target_kl into a table in the last bytes of the workspace, which the optimiser's kernel reads at its
 *   learner's index.  No host synchronisation, no device allocation, capturable (a capture freezes the learners' values as it
 *   freezes the seeds).  Refusals: the population entry's in its order, then a NULL `hypers` or refused values
 *   (EVAC_ERR_INVALID_ARGUMENT), all on the host before anything touches a device.
 *   workspace: evac_*_sweep_workspace_bytes(obs_dim, M, S) bytes, 16-byte aligned: the population entry's layout, unchanged,
 *   then the table (1288 bytes rounded up to whole 256-byte parts).  The sizers refuse what the population's refuse. */
int evac_policy_rollout_sweep_deepsets(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                       const evac_mlp_policy_strides_t* strides, const evac_deepsets_t* encoder,
                                       const evac_deepsets_strides_t* enc_strides, int32_t n_steps, float* next_obs, float* next_done,
                                       float* obs_out, float* actions_out, float* logprob_out, float* value_out, float* reward_out,
                                       float* done_out, float* next_value_out, evac_episode_stats_t* final_stats_or_null,
                                       double* norm_state_or_null, float gamma, float obs_clip, float reward_clip, float epsilon,
                                       const evac_learner_hyper_t* hypers, void* stream);
int evac_policy_rollout_sweep_transformer(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                          const evac_mlp_policy_strides_t* strides, const evac_transformer_t* encoder,
                                          const evac_transformer_strides_t* enc_strides, int32_t n_steps, float* next_obs,
                                          float* next_done, float* obs_out, float* actions_out, float* logprob_out, float* value_out,
                                          float* reward_out, float* done_out, float* next_value_out,
                                          evac_episode_stats_t* final_stats_or_null, double* norm_state_or_null, float gamma,
                                          float obs_clip, float reward_clip, float epsilon, const evac_learner_hyper_t* hypers,
                                          void* stream);
int64_t evac_deepsets_sweep_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners);
int64_t evac_transformer_sweep_workspace_bytes(int32_t obs_dim, int64_t n_minibatch, int32_t n_learners);
int evac_deepsets_update_sweep(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_deepsets_t* encoder,
                               const evac_mlp_policy_grads_t* params, const evac_deepsets_grads_t* enc_params,
                               const evac_mlp_policy_grads_t* grads, const evac_deepsets_grads_t* enc_grads,
                               const evac_mlp_policy_strides_t* param_strides, const evac_deepsets_strides_t* enc_param_strides,
                               const evac_mlp_policy_strides_t* grad_strides, const evac_deepsets_strides_t* enc_grad_strides,
                               const evac_mlp_policy_strides_t* moment_strides, const evac_deepsets_strides_t* enc_moment_strides,
                               int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                               const evac_deepsets_adam_state_t* state, int64_t batch_size, const float* b_obs, const float* b_actions,
                               const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
                               int64_t learner_batch_size, int64_t n_minibatch, int32_t n_epochs, const int64_t* perms,
                               const float* rpo_noise_or_null, const uint64_t* seeds, const uint64_t* first_draw_counters,
                               const evac_learner_hyper_t* hypers, float* stats_out, void* workspace, void* stream);
int evac_transformer_update_sweep(int32_t n_learners, const evac_mlp_policy_t* policy, const evac_transformer_t* encoder,
                                  const evac_mlp_policy_grads_t* params, const evac_transformer_grads_t* enc_params,
                                  const evac_mlp_policy_grads_t* grads, const evac_transformer_grads_t* enc_grads,
                                  const evac_mlp_policy_strides_t* param_strides, const evac_transformer_strides_t* enc_param_strides,
                                  const evac_mlp_policy_strides_t* grad_strides, const evac_transformer_strides_t* enc_grad_strides,
                                  const evac_mlp_policy_strides_t* moment_strides, const evac_transformer_strides_t* enc_moment_strides,
                                  int64_t header_stride_bytes, const evac_rpo_loss_config_t* loss_cfg, const evac_adam_config_t* adam_cfg,
                                  const evac_transformer_adam_state_t* state, int64_t batch_size, const float* b_obs,
                                  const float* b_actions, const float* b_logprobs, const float* b_advantages, const float* b_returns,
                                  const float* b_values, int64_t learner_batch_size, int64_t n_minibatch, int32_t n_epochs,
                                  const int64_t* perms, const float* rpo_noise_or_null, const uint64_t* seeds,
                                  const uint64_t* first_draw_counters, const evac_learner_hyper_t* hypers, float* stats_out,
                                  void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVAC_H */
