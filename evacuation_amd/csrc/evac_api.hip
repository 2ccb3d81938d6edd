// Host side of the libevac C ABI (include/evac.h): argument checking, kernel dispatch by env size,
// error reporting.  No device allocation, no synchronisation: every call only enqueues work on the
// caller's stream, so the step can be captured into a hipGraph by the caller.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "evac_device.h"
#include "evac_subwave.h"
#include "evac_team.h"
#include "evac_gather.h"
#include "evac_policy.h"
#include "evac_evaluate.h"
#include "evac_host.h"
#include "evac_handle_host.h"

namespace {

thread_local std::string g_create_error;

int validate(const evac_config_t* c, std::string& err) {
    if (!c) { err = "cfg is NULL"; return EVAC_ERR_INVALID_ARGUMENT; }
    if (c->number_of_pedestrians < 1 || c->number_of_pedestrians > EVAC_MAX_PEDESTRIANS) {
        err = "number_of_pedestrians must be in [1, " + std::to_string(EVAC_MAX_PEDESTRIANS) + "]";
        return EVAC_ERR_INVALID_ARGUMENT;
    }
    if (!(c->width > 0.f) || !(c->height > 0.f) || !(c->step_size > 0.f)) { err = "width, height, step_size must be > 0"; return EVAC_ERR_INVALID_ARGUMENT; }
    if (c->max_timesteps < 1) { err = "max_timesteps must be >= 1"; return EVAC_ERR_INVALID_ARGUMENT; }
    if (c->positions < EVAC_POS_ABS || c->positions > EVAC_POS_GRAV) { err = "positions must be abs|rel|grav"; return EVAC_ERR_INVALID_ARGUMENT; }
    if (c->statuses < EVAC_STAT_NO || c->statuses > EVAC_STAT_CAT) { err = "statuses must be no|ohe|cat"; return EVAC_ERR_INVALID_ARGUMENT; }
    if (c->type != EVAC_TYPE_DICT && c->type != EVAC_TYPE_BOX) { err = "type must be Dict|Box"; return EVAC_ERR_INVALID_ARGUMENT; }   // wrappers/config.py:81-82 ValueError
    if (c->positions == EVAC_POS_GRAV && c->type == EVAC_TYPE_BOX) {
        err = "positions='grav' with type='Box' is not implemented (reference wrappers/config.py:79-80 raises NotImplementedError)";
        return EVAC_ERR_UNSUPPORTED;
    }
    return EVAC_OK;
}

int64_t obs_dim_of(const evac_config_t* c) {
    const int64_t n = c->number_of_pedestrians;
    if (c->positions == EVAC_POS_GRAV) return 6;
    const int64_t sc = c->statuses == EVAC_STAT_OHE ? 4 : (c->statuses == EVAC_STAT_CAT ? 1 : 0);
    if (c->type == EVAC_TYPE_BOX) return (n + 2) * (2 + sc);
    return 4 + 2 * n + sc * n;
}

}  // namespace

enum class Form { Plain, Parts, Chain, Persist };   // how a handle issues its rollouts (include/evac.h, evac_options_t.parts / chain)

struct evac_handle {
    evac_config_t cfg;
    evac::Params p;
    int device;
    bool bound;
    int sub_lanes;      // 0: one wave (or more) per env; 16 / 32: sub-wave kernels (evac_subwave.h)
    bool cells;         // workgroup-per-env kernels with the cell list (N > 64) instead of all pairs
    bool cu_wide;       // rollouts of one-wave envs in CU-wide workgroups (the batch fills every CU with 16 envs)
    bool cu_wide4;      // the same for four-wave envs (4 envs per CU-wide workgroup)
    bool default_cfg;   // the configuration the specialised rollout kernels assume (k_rollout_default_config)
    int team_k;         // rollouts of 513..1024-pedestrian envs by teams of 2 / 4 / 8 / 16 workgroups per env (0: one workgroup per env)
    int32_t* sched;     // inside the caller's workspace (evac_bind_workspace): moving[2][E] | perm[2][E], or NULL
    int sched_gen = -1; // rollout launches under the schedule so far (< 0: no deal yet): launch g reads perm[g & 1], leaves its loads
                        // in moving[g & 1] and deals perm[(g + 1) & 1] from moving[(g - 1) & 1] (rollout_body)
    bool team_bound;    // the workspace holds the teams' exchange areas
    int team_fit = -1;  // -1: not checked yet; 1 / 0: the team grid fits the device at once (occupancy x CUs >= workgroups) or not
    size_t team_xchg_bytes;   // the teams' exchange area (records + tile slots), filled with 0xff (the tag of no round) before every team launch
    bool team_coop;     // EVAC_TEAM_COOP=1 (and the device supports it): team kernels are launched with hipLaunchCooperativeKernel
    int cus;            // compute units of the device
    bool team_fault;    // EVAC_TEAM_FAULT=1 (tests): launch the team grid one workgroup short
    // The teams' error word: 64 bytes of host-mapped memory owned by the handle.  A team that lost a member raises it from the
    // kernel (system-scope store); every later evac_* call of the handle reads it on the host, without synchronising.
    volatile unsigned* team_flag_host;
    unsigned* team_flag_dev;
    std::string err;
    std::string variant[4];   // evac_step | evac_rollout with one workgroup (or less) per env | evac_rollout by teams | ... in the handle's form
    evac_options_t opt;       // as resolved at creation (evac_get_options)
    // How the handle issues its rollouts, fixed at creation (evac_create_ex); evac_team_clear_error falls back to Plain after settling.
    // Every form but Plain runs on the two streams the handle owns (`own`); whatever is not a plain rollout settles them first (settle).
    Form form = Form::Plain;
    struct OwnStreams {
        hipStream_t s[2];
        hipEvent_t done[2], fork;
        bool pending;         // the own streams hold work the caller's stream has not been made to wait for (evac_join)
        bool forked;          // the own streams have been put behind the caller's stream since the last join (evac_rollout forks once per join)
    } own;
    // Form::Parts (evac_options_t.parts = 2): the handle's rollouts go out as two half-batch kernels on the own streams (include/evac.h,
    // evac_join).  part[k] is a complete handle of its own over envs [k E / 2, (k + 1) E / 2) of THIS handle's buffers (state
    // pointers and workspace slices offset, Params::slab_envs = E, env_id_offset + k E / 2: the same global env ids), so a part
    // launches exactly what a handle of that size launches -- schedule, in-kernel deal and generation counter of its own.
    evac_handle* part[2];
    // Form::Chain and Form::Persist: what the handle allocates itself besides its streams
    char* xchg;               // uncached device memory: Chain's [E] exchange records (evac_common.h); Persist's command ring (+ next_cmd[E], decision[E])
    size_t xchg_bytes;        // (what the pool handed out: given back with it)
    unsigned* abort_word;     // device word: a wait timed out (Chain: in the workspace, Persist: behind the ring)
    hipEvent_t last_ev;       // Chain: behind a restart's import; Persist: behind every persistent kernel (has it left?)
    // Form::Chain (evac_options_t.chain = 1): rollout launch g goes to own.s[g & 1] and waits PER ENV for launch g - 1 on the device
    // (include/evac.h, evac_common.h ChainArgs).  The schedule is four deep here: launch g reads perm[g & 3], leaves its loads in
    // moving[g & 3] and deals perm[(g + 2) & 3] -- read by the next launch of ITS stream -- from moving[(g - 2) & 3], the last
    // launch of its stream: everything a launch reads was written by a launch its queue has completed.
    struct ChainState {
        bool bound;           // the workspace is bound (chained launches need it; without it the handle issues plain launches)
        bool small;           // the chain's launches are the 256-thread workgroups of one-wave envs (four envs each: no deal, no pace keeping)
        bool restart = true;  // the state was written by something else than the chain's last launch: fill the generation words first
        bool dirty;           // the records are ahead of the caller's state arrays (k_chain_export at the next join)
        int gen = 1;          // rollout launches of the chain so far = the generation the next launch waits for
        int start = 1;        // the launch at which the chain (re)started: deals begin two launches later
                              // (never 0: a zero-filled workspace must not look like a published generation)
        int32_t* sched;       // moving[4][E] | perm[4][E]
        unsigned long long wgs;   // workgroups of the chain's launches enqueued since its last restart (the gate's target)
    } chain;
    // Form::Persist (evac_options_t.chain = 2): one persistent rollout kernel per join, every evac_rollout call a command of its ring
    struct PersistState {
        bool running;         // the kernel is resident (on own.s[0]) and reads commands
        int seq;              // the next command's index (its sequence number is index + 1; never reset)
        int first;            // the first command of the kernel that is running
    } persist;
};

namespace {

int fail(evac_handle_t h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

// A team rollout of this handle lost a member (evac_team.h), or a chained launch waited in vain: the outputs of that launch are void.
// Sticky until evac_team_clear_error, which settles the handle and leaves it on plain launches of one workgroup per env.
int team_aborted(evac_handle_t h, const char* what) {
    if (!h->team_flag_host || *h->team_flag_host == 0u) return EVAC_OK;
    if (h->form == Form::Chain)
        return fail(h, EVAC_ERR_TEAM_ABORTED,
                    std::string(what) + ": a chained rollout launch waited in vain for an env's state (a launch of the chain was lost); the "
                    "outputs since are void -- call evac_team_clear_error(), then reset or restore the batch; the handle issues plain launches from now on");
    return fail(h, EVAC_ERR_TEAM_ABORTED,
                std::string(what) + ": an earlier team rollout lost a member (the workgroups of a team were not resident together); "
                "the outputs of that launch are void and the env it carried kept its pre-launch state -- call "
                "evac_team_clear_error(), then reset or restore the batch; the handle uses one workgroup per env from now on");
}

int check_launch(evac_handle_t h, const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, EVAC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return EVAC_OK;
}

int waves_per_env(int n_ped) { return n_ped <= 64 ? 1 : (n_ped <= 128 ? 2 : (n_ped <= 256 ? 4 : (n_ped <= 512 ? 8 : 16))); }

// launch KERNEL<F, GRAV> for a Wave / Cells family F
#define EVAC_LAUNCH_F(h, KERNEL, F_, GRAV_, s_, ...)                                                                  \
    hipLaunchKernelGGL((evac::KERNEL<F_, GRAV_>), dim3((unsigned)(((h)->p.n_envs + F_::kEnvsPerBlock - 1) / F_::kEnvsPerBlock)), \
                       dim3(F_::kBlock), 0, s_, __VA_ARGS__)
#define EVAC_LAUNCH_SUB(h, KERNEL, G_, GRAV_, s_, ...)                                                              \
    hipLaunchKernelGGL((evac::KERNEL##_sub<G_, GRAV_>),                                                             \
                       dim3((unsigned)(((h)->p.n_envs + evac::Sub<G_>::kEnvsPerBlock - 1) / evac::Sub<G_>::kEnvsPerBlock)), \
                       dim3(evac::Sub<G_>::kBlock), 0, s_, __VA_ARGS__)
#define EVAC_LAUNCH_WPE(h, KERNEL, WPE_, s_, ...)                                                                   \
    do {                                                                                                            \
        if (WPE_ > 1 && (h)->cells) {                                                                               \
            using FC_ = evac::Cells<(WPE_ > 1 ? WPE_ : 2)>;                                                         \
            if (grav_) EVAC_LAUNCH_F(h, KERNEL, FC_, true, s_, __VA_ARGS__);                                        \
            else EVAC_LAUNCH_F(h, KERNEL, FC_, false, s_, __VA_ARGS__);                                             \
        } else {                                                                                                    \
            using FW_ = evac::Wave<WPE_>;                                                                           \
            if (grav_) EVAC_LAUNCH_F(h, KERNEL, FW_, true, s_, __VA_ARGS__);                                        \
            else EVAC_LAUNCH_F(h, KERNEL, FW_, false, s_, __VA_ARGS__);                                             \
        }                                                                                                           \
    } while (0)

// kernel variant = family (lanes or waves per env, all pairs | cell list) x (gravity observation | generic
// positions/statuses observation)
#define EVAC_DISPATCH(h, KERNEL, stream, ...)                                         \
    do {                                                                              \
        const int wpe_ = waves_per_env((h)->p.n_ped);                                 \
        const bool grav_ = (h)->p.obs_pos == EVAC_POS_GRAV;                           \
        hipStream_t s_ = (hipStream_t)(stream);                                       \
        if ((h)->sub_lanes == 16) {                                                   \
            if (grav_) EVAC_LAUNCH_SUB(h, KERNEL, 16, true, s_, __VA_ARGS__);         \
            else EVAC_LAUNCH_SUB(h, KERNEL, 16, false, s_, __VA_ARGS__);              \
        } else if ((h)->sub_lanes == 32) {                                            \
            if (grav_) EVAC_LAUNCH_SUB(h, KERNEL, 32, true, s_, __VA_ARGS__);         \
            else EVAC_LAUNCH_SUB(h, KERNEL, 32, false, s_, __VA_ARGS__);              \
        } else if (wpe_ == 1) EVAC_LAUNCH_WPE(h, KERNEL, 1, s_, __VA_ARGS__);         \
        else if (wpe_ == 2) EVAC_LAUNCH_WPE(h, KERNEL, 2, s_, __VA_ARGS__);           \
        else if (wpe_ == 4) EVAC_LAUNCH_WPE(h, KERNEL, 4, s_, __VA_ARGS__);           \
        else if (wpe_ == 8) EVAC_LAUNCH_WPE(h, KERNEL, 8, s_, __VA_ARGS__);           \
        else EVAC_LAUNCH_WPE(h, KERNEL, 16, s_, __VA_ARGS__);                         \
    } while (0)


// ---- team rollouts (evac_team.h): which kernel, how many workgroups, and do they all fit the device at once ----
// ONE team grid at a time per device, process-wide.  The members of a team wait for each other, and team_grid_fits only
// checks that ONE grid fits the device: two grids in flight (two handles on two streams -- train and eval envs --, a graph replay
// beside a live launch) can each be dispatched in part, every resident member polling in place on a CU the other grid's missing
// members need -- both time out.  So every team launch first waits (on the device, hipStreamWaitEvent) for the event the
// previous team launch on that device recorded behind itself, whatever stream or handle it came from.  A launch under stream
// capture cannot join the chain (an event recorded outside the capture); a graph holding team launches must not be replayed
// beside another team launch.  Other PROCESSES on the same GPU are out of reach: they need EVAC_TEAM=0.
constexpr int kMaxDevices = 64;
std::mutex g_team_chain_lock;
hipEvent_t g_team_chain[kMaxDevices] = {};

// The kernel of a pair -- KDEF specialised for the default configuration (k_rollout_default_config), KGEN generic -- of family F_ for this
// handle's configuration and observation (gravity or not).  Both kernels of a pair take the same arguments: launch it through the pointer.
#define EVAC_PICK(h, KDEF, KGEN, F_)                                                                                        \
    ((h)->default_cfg ? ((h)->p.obs_pos == EVAC_POS_GRAV ? &evac::KDEF<F_, true> : &evac::KDEF<F_, false>)                  \
                      : ((h)->p.obs_pos == EVAC_POS_GRAV ? &evac::KGEN<F_, true> : &evac::KGEN<F_, false>))
#define EVAC_PICK_TEAM(h, KDEF, KGEN)                                                                                       \
    ((h)->team_k == 16 ? (const void*)EVAC_PICK(h, KDEF, KGEN, evac::Team<16>) :                                             \
     (h)->team_k == 8 ? (const void*)EVAC_PICK(h, KDEF, KGEN, evac::Team<8>) :                                               \
     (h)->team_k == 4 ? (const void*)EVAC_PICK(h, KDEF, KGEN, evac::Team<4>) : (const void*)EVAC_PICK(h, KDEF, KGEN, evac::Team<2>))
const void* team_kernel(const evac_handle* h) { return EVAC_PICK_TEAM(h, k_rollout_default_config, k_rollout); }
const void* team_persist_kernel(const evac_handle* h) { return EVAC_PICK_TEAM(h, k_rollout_persist_default_config, k_rollout_persist); }
unsigned team_grid(const evac_handle* h) {
    // (EVAC_TEAM_FAULT=1, fault injection for tests/test_gpu_team.py: the last workgroup is never launched, so the team it
    // belongs to loses a member and must time out, flag the error and leave its env's state alone)
    return (unsigned)((h->p.n_envs + 7) / 8 * 8 * h->team_k) - (h->team_fault ? 1u : 0u);
}
// The members of a team wait for each other, so every workgroup of the grid needs a CU of its own at the same time.
bool team_grid_fits(evac_handle* h) {
    if (h->team_fit < 0) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, team_kernel(h), 1024, 0) != hipSuccess) {
            (void)hipGetLastError();
            per_cu = 0;
        }
        h->team_fit = (long long)per_cu * h->cus >= (long long)team_grid(h) ? 1 : 0;
    }
    return h->team_fit == 1;
}
// A team grid on `s`, behind the previous team grid of the device (g_team_chain; `in_chain` = false under stream capture).  coop:
// hipLaunchCooperativeKernel (EVAC_TEAM_COOP=1), falling back to a plain launch where it fails.
hipError_t launch_team_grid(evac_handle* h, const void* fn, void** argv, hipStream_t s, bool in_chain, bool coop) {
    const dim3 grid(team_grid(h)), block(1024);
    const bool chained = in_chain && h->device >= 0 && h->device < kMaxDevices;
    std::unique_lock<std::mutex> chain(g_team_chain_lock, std::defer_lock);
    if (chained) {                               // (see g_team_chain: the previous team grid of this device has drained)
        chain.lock();
        hipEvent_t& ev = g_team_chain[h->device];
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ev = nullptr; }
        if (ev && hipStreamWaitEvent(s, ev, 0) != hipSuccess) (void)hipGetLastError();      // (a never-recorded event: no wait)
    }
    hipError_t le = coop ? hipLaunchCooperativeKernel(fn, grid, block, argv, 0, s) : hipLaunchKernel(fn, grid, block, argv, 0, s);
    if (le != hipSuccess && coop) {              // (e.g. under stream capture): the occupancy check still holds for a plain launch
        (void)hipGetLastError();
        h->team_coop = false;
        le = hipLaunchKernel(fn, grid, block, argv, 0, s);
    }
    if (chained && g_team_chain[h->device] && le == hipSuccess && hipEventRecord(g_team_chain[h->device], s) != hipSuccess) (void)hipGetLastError();
    return le;
}

}  // namespace

extern "C" {

int evac_version(void) { return EVAC_VERSION; }

const char* evac_status_string(int s) {
    switch (s) {
        case EVAC_OK: return "ok";
        case EVAC_ERR_INVALID_ARGUMENT: return "invalid argument";
        case EVAC_ERR_NOT_BOUND: return "state buffers not bound";
        case EVAC_ERR_UNSUPPORTED: return "unsupported configuration";
        case EVAC_ERR_HIP: return "HIP error";
        case EVAC_ERR_NO_DEVICE: return "no HIP device";
        case EVAC_ERR_TEAM_ABORTED: return "a team rollout lost a member";
        default: return "unknown status";
    }
}

const char* evac_last_error(evac_handle_t h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int evac_config_validate(const evac_config_t* cfg) {
    std::string err;
    const int rc = validate(cfg, err);
    g_create_error = err;
    return rc;
}

int64_t evac_config_obs_dim(const evac_config_t* cfg) {
    std::string err;
    if (validate(cfg, err) != EVAC_OK) { g_create_error = err; return -1; }
    return obs_dim_of(cfg);
}

}  // extern "C"

namespace {
// A create-time option: the diagnostic environment variable wins when it is set (A/B runs of an unmodified caller), then the
// caller's evac_options_t field, then -1 = automatic.
int option_value(const char* env_name, int option) {
    const char* v = std::getenv(env_name);
    if (v && v[0]) return std::atoi(v);
    return option;
}

// ---- What a handle allocates from the device ITSELF -- its two streams, the chain's uncached exchange records, the host-mapped error
// word -- is taken from pools that live as long as the process and goes back to them when the handle is destroyed; nothing of it is
// ever given back to HIP.  Creating and freeing these per handle re-used device addresses (and hardware queues) at a high rate under
// whatever else the process runs, and on some MI355X boxes a process that did so read stale memory through OTHER allocations for a
// while afterwards (tests/test_gpu_parity.py's chained cases, in their first iterations only, serialised launches included:
// DESIGN.md "the pools").  A process that creates a thousand handles now makes one pair of streams.
struct PooledPair { int device; hipStream_t s[2]; };
struct PooledBuf { int device; size_t bytes; void* p; };
struct PooledWord { int device; void* host; void* dev; };
std::mutex g_pool_mu;
std::vector<PooledPair> g_pool_pairs;
std::vector<PooledBuf> g_pool_bufs;
std::vector<PooledWord> g_pool_words;
bool pools_on() { static const bool on = option_value("EVAC_DIAG_NO_POOLS", 0) == 0; return on; }

// 64 bytes of host memory the device can write (the error word of the team kernels and of the chain), zeroed
bool take_error_word(int device, void** host, void** dev) {
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t i = 0; i < g_pool_words.size(); ++i)
            if (g_pool_words[i].device == device) {
                *host = g_pool_words[i].host; *dev = g_pool_words[i].dev;
                g_pool_words.erase(g_pool_words.begin() + (long)i);
                std::memset(*host, 0, 64);
                return true;
            }
    }
    *host = *dev = nullptr;
    if (hipHostMalloc(host, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(dev, *host, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (*host) (void)hipHostFree(*host);
        *host = *dev = nullptr;
        return false;
    }
    std::memset(*host, 0, 64);
    return true;
}
void give_error_word(int device, void* host, void* dev) {
    if (!host) return;
    if (!pools_on()) { (void)hipHostFree(host); return; }
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool_words.push_back(PooledWord{device, host, dev});
}
// uncached device memory of at least `bytes` (the caller fills it)
void* take_uncached(int device, size_t bytes, size_t* got) {
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        size_t best = g_pool_bufs.size();
        for (size_t i = 0; i < g_pool_bufs.size(); ++i)
            if (g_pool_bufs[i].device == device && g_pool_bufs[i].bytes >= bytes && g_pool_bufs[i].bytes <= 2 * bytes + (1u << 16) &&
                (best == g_pool_bufs.size() || g_pool_bufs[i].bytes < g_pool_bufs[best].bytes)) best = i;
        if (best < g_pool_bufs.size()) {
            void* p = g_pool_bufs[best].p;
            *got = g_pool_bufs[best].bytes;
            g_pool_bufs.erase(g_pool_bufs.begin() + (long)best);
            return p;
        }
    }
    void* p = nullptr;
    if (hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    *got = bytes;
    return p;
}
void give_uncached(int device, void* p, size_t bytes) {
    if (!p) return;
    if (!pools_on()) { (void)hipFree(p); return; }
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool_bufs.push_back(PooledBuf{device, bytes, p});
}

int create_impl(const evac_config_t* cfg, int32_t num_envs, int32_t device, uint64_t seed, uint64_t env_id_offset,
                const evac_options_t& o, evac_handle_t* out) {
    if (!out) { g_create_error = "out is NULL"; return EVAC_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    std::string err;
    const int rc = validate(cfg, err);
    if (rc != EVAC_OK) { g_create_error = err; return rc; }
    if (num_envs < 1) { g_create_error = "num_envs must be >= 1"; return EVAC_ERR_INVALID_ARGUMENT; }
    if (env_id_offset + (uint64_t)num_envs > 0xffffffffull) { g_create_error = "env_id_offset + num_envs exceeds 2^32"; return EVAC_ERR_INVALID_ARGUMENT; }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        g_create_error = "no HIP device visible: libevac has no CPU path";
        return EVAC_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) { g_create_error = "device index out of range"; return EVAC_ERR_INVALID_ARGUMENT; }
    evac_handle* h = new (std::nothrow) evac_handle();   // (value-initialised: every field not set below is zero / as declared)
    if (!h) { g_create_error = "out of host memory"; return EVAC_ERR_INVALID_ARGUMENT; }
    h->cfg = *cfg;
    h->device = device;
    const int o_subwave = option_value("EVAC_SUBWAVE", o.subwave), o_cells = option_value("EVAC_CELLS", o.cells);
    const int o_cu_wide = option_value("EVAC_CU_WIDE", o.cu_wide), o_team = option_value("EVAC_TEAM", o.team);
    const int o_specialize = option_value("EVAC_SPECIALIZE", o.specialize);
    const int o_team_coop = option_value("EVAC_TEAM_COOP", o.team_coop), o_team_fault = option_value("EVAC_TEAM_FAULT", o.team_fault);
    {   // small rooms share a wave: 4 envs per wave for N <= 16, 2 for N <= 32 (subwave = 0 disables, for A/B tests)
        const bool allow = o_subwave != 0;
        const int n = cfg->number_of_pedestrians;
        h->sub_lanes = !allow ? 0 : (n <= 16 ? 16 : (n <= 32 ? 32 : 0));
        // rooms of more than 512 pedestrians use the cell list; cells = 1 / 0 forces it on (for every room of more
        // than one wave) / off, for A/B tests
        h->cells = n > evac::kWave && (o_cells == 1 ? true : (o_cells == 0 ? false : n > 512));
    }
    evac::Params& p = h->p;
    std::memset(&p, 0, sizeof(p));
    p.n_envs = num_envs;
    p.slab_envs = num_envs;
    p.n_ped = cfg->number_of_pedestrians;
    p.width = cfg->width;
    p.height = cfg->height;
    p.step_size = cfg->step_size;
    p.noise_coef = cfg->noise_coef;
    p.eps = cfg->eps;
    p.ens = cfg->enslaving_degree;
    p.one_minus_ens = (float)(1.0 - (double)cfg->enslaving_degree);   // area.py:141 computes (1. - e) in double
    p.init_reward = cfg->init_reward_each_step;
    p.intrinsic_coef = cfg->intrinsic_reward_coef;
    p.flags = (cfg->is_new_exiting_reward ? evac::kFlagNewExitingReward : 0u) |
              (cfg->is_new_followers_reward ? evac::kFlagNewFollowersReward : 0u) |
              (cfg->is_termination_agent_wall_collision ? evac::kFlagTermOnWall : 0u) |
              (cfg->nan_guard ? evac::kFlagNanGuard : 0u) | (cfg->clip_action ? evac::kFlagClipAction : 0u);
    p.max_timesteps = cfg->max_timesteps;
    p.inv_n = (float)(1.0 / (double)cfg->number_of_pedestrians);
    p.inv_200n = (float)(1.0 / (200.0 * (double)cfg->number_of_pedestrians));
    p.obs_pos = cfg->positions;
    p.obs_stat = cfg->statuses;
    p.obs_box = cfg->type == EVAC_TYPE_BOX;
    p.obs_dim = (int32_t)obs_dim_of(cfg);
    p.alpha = cfg->alpha;
    p.neg_alpha = -cfg->alpha;
    p.grav_pow = cfg->alpha + 2.0f;
    const float gp = cfg->alpha + 2.0f;
    p.grav_pow_int = (gp == std::floor(gp) && gp >= 1.0f && gp <= 63.0f) ? (int)gp : 0;
    {
        const float half = std::fabs(cfg->noise_coef) * 0.5f;
        p.small_noise = half <= 0.2f ? 2 : (half <= 0.78539816f ? 1 : 0);
    }
    {   // cell list: 16 x 16 cells over [-max(W,1), max(W,1)] x [-max(H,1), max(H,1)] (reset draws positions in +-1
        // whatever the room, pedestrians.py:17): a cell is >= 0.125 wide, the pedestrian radius is 0.1
        const float wb = std::fmax(cfg->width, 1.0f), hb = std::fmax(cfg->height, 1.0f);
        p.cell_ox = wb;
        p.cell_oy = hb;
        p.cell_inv_hx = (float)evac::kCellsX / (2.0f * wb);
        p.cell_inv_hy = (float)evac::kCellsY / (2.0f * hb);
        // integer heading = rint(heading * head_scale): it must fit v_mad_i32_i24 (< 2^23) and N of them an int32
        // (a unit-heading component can exceed 1 by a few ulp of v_rsq: 16 units of slack cover it)
        const int64_t cap = (int64_t)0x7fffffff / cfg->number_of_pedestrians - 16;
        p.head_scale = (float)(cap < 0x7ffff0 ? cap : (int64_t)0x7ffff0);     // exact in f32 (< 2^24)
        // Rooms of 513..1024 pedestrians (team kernels and Cells<16>, which agree bit for bit): the team kernels sum up to
        // kTeamExactBatch = 8 such headings at a time in packed f32 arithmetic before the partial sum goes to an integer accumulator
        // (evac_team.h) -- exact below 2^24, so the scale is capped at 2^21 - 16 there (N = 1024 has 2^21 - 17 anyway).
        if (cfg->number_of_pedestrians > 512 && p.head_scale > (float)((1 << 24) / evac::kTeamExactBatch - 16))
            p.head_scale = (float)((1 << 24) / evac::kTeamExactBatch - 16);
    }
    {   // CU-wide rollout workgroups pay off once every CU gets its 16 one-wave envs, and as long as the launch is a few
        // rounds deep: a 16-wave workgroup needs a whole CU, so in a long launch every CU idles while the last waves of its
        // workgroup finish (524 288 envs: 1.44e9 against 1.62e9 env-steps/s with 4-wave workgroups; 8 192 envs: 1.75e9
        // against 1.59e9).  EVAC_CU_WIDE=1 / 0 forces, for tests.
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
        h->cus = cus;
        const bool one_wave = h->sub_lanes == 0 && cfg->number_of_pedestrians <= evac::kWave;
        h->cu_wide = one_wave && (o_cu_wide == 1 ? true : (o_cu_wide == 0 ? false : (num_envs >= 16 * cus && num_envs <= 64 * cus)));
        // priority rotation (rollout_body) evens out the waves of a SIMD in launches of one or two rounds; deeper launches
        // even out by themselves and run ~2 % faster without it
        const int wpe = waves_per_env(cfg->number_of_pedestrians);
        const long long waves = h->sub_lanes ? ((long long)num_envs * h->sub_lanes + 63) / 64 : (long long)num_envs * wpe;
        h->p.fair = waves <= 2ll * 16 * cus ? 1 : 0;
        // four-wave envs (N = 129..256, all pairs): 4 envs per CU-wide workgroup with per-env LDS barriers, pace and schedule
        h->cu_wide4 = h->sub_lanes == 0 && wpe == 4 && !h->cells &&
                      (o_cu_wide == 1 ? true : (o_cu_wide == 0 ? false : (num_envs >= 4 * cus && num_envs <= 16 * cus)));
        h->default_cfg = o_specialize != 0;                  // specialize = 0: always the generic kernels (A/B runs)
        const bool obs_default = cfg->positions == EVAC_POS_GRAV
                                     ? p.grav_pow_int == 5
                                     : (cfg->positions == EVAC_POS_REL && cfg->statuses == EVAC_STAT_OHE && cfg->type == EVAC_TYPE_BOX);
        h->default_cfg = h->default_cfg && obs_default && p.small_noise == 2 && p.ens == 1.0f &&
                         p.one_minus_ens == 0.0f &&
                         (p.flags & (evac::kFlagTermOnWall | evac::kFlagNanGuard)) == 0;
        // teams: as many CUs per env as the batch leaves free -- all members must be resident together (one 1024-thread
        // workgroup per CU), teams are laid out in rows of 8 (one per XCD).  EVAC_TEAM=0 disables, 2 / 4 / 8 / 16 forces a size.
        if (cfg->number_of_pedestrians > 512) {
            const int want = o_team;
            const int rows = (num_envs + 7) / 8 * 8;
            for (int k = 16; k >= 2; k >>= 1)
                if ((want < 0 || want == k) && rows * k <= cus) { h->team_k = k; break; }
            if (want == 0 || (want < 0 && o_cells >= 0)) h->team_k = 0;   // an A/B run of the one-workgroup families
        }
        if (h->team_k) {
            DeviceGuard g(device);
            void* host = nullptr;
            void* dev = nullptr;
            if (!take_error_word(device, &host, &dev)) {
                h->team_k = 0;                       // no error word, no teams
            } else {
                h->team_flag_host = (volatile unsigned*)host;
                h->team_flag_dev = (unsigned*)dev;
                int coop = 0;
                if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, device) != hipSuccess) coop = 0;
                h->team_coop = coop != 0 && o_team_coop == 1;        // opt-in: see evac_rollout
                h->team_fault = o_team_fault == 1;
            }
        }
    }
    p.seed_lo = (uint32_t)(seed & 0xffffffffull);
    p.seed_hi = (uint32_t)(seed >> 32);
    p.env_id_offset = (uint32_t)env_id_offset;
    {
        const int wpe = waves_per_env(p.n_ped);
        const bool grav = p.obs_pos == EVAC_POS_GRAV;
        std::string fam = h->sub_lanes == 16 ? evac::Sub<16>::kName : h->sub_lanes == 32 ? evac::Sub<32>::kName :
                          wpe == 1 ? evac::Wave<1>::kName :
                          h->cells ? (wpe == 2 ? evac::Cells<2>::kName : wpe == 4 ? evac::Cells<4>::kName : wpe == 8 ? evac::Cells<8>::kName : evac::Cells<16>::kName)
                                   : (wpe == 2 ? evac::Wave<2>::kName : wpe == 4 ? evac::Wave<4>::kName : wpe == 8 ? evac::Wave<8>::kName : evac::Wave<16>::kName);
        const char* kind = h->default_cfg ? "_default_config<" : "<";     // (the names rocprofv3 shows)
        h->variant[0] = std::string("k_step") + kind + fam + (grav ? ", grav obs>" : ", generic obs>");
        if (h->cu_wide) fam = evac::Wave<1, 1024>::kName;
        if (h->cu_wide4) fam = evac::Wave<4, 1024>::kName;
        h->variant[1] = std::string("k_rollout") + kind + fam + (grav ? ", grav obs>" : ", generic obs>");
        if (h->team_k) fam = h->team_k == 16 ? evac::Team<16>::kName : (h->team_k == 8 ? evac::Team<8>::kName : (h->team_k == 4 ? evac::Team<4>::kName : evac::Team<2>::kName));
        h->variant[2] = std::string("k_rollout") + kind + fam + (grav ? ", grav obs>" : ", generic obs>");
    }
    if (!h->team_k) h->team_fault = o_team_fault == 1;       // (chained launches: fault injection of their own, evac_rollout)
    h->opt = evac_options_t{h->sub_lanes ? 1 : 0, h->cells ? 1 : 0, (h->cu_wide || h->cu_wide4) ? 1 : 0, h->team_k, h->default_cfg ? 1 : 0,
                            1, h->team_coop ? 1 : 0, h->team_fault ? 1 : 0, 0};
    *out = h;
    return EVAC_OK;
}

// ---- evac_options_t.parts = 2: two streams of the handle's own that really run BESIDE each other.  HIP deals its streams onto a
// handful of hardware queues (four by default) in the order of their first use, and two streams that share a queue execute
// strictly one after the other (round 4 found the gather stream on the rollout's queue).  So every candidate is timed
// against the first stream with two one-thread spin kernels of ~100 us: a pair that takes about as long as one of them overlaps.
__global__ void k_spin_100us(unsigned long long ticks, unsigned* sink) {
    unsigned long long t0, t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
    unsigned n = 0;
    do {                                           // (100 MHz constant clock; bounded whatever the clock reads)
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    } while (t - t0 < ticks && ++n < (1u << 22));
    if (sink) *sink = n;
}
float spin_pair_ms(hipStream_t a, hipStream_t b, hipEvent_t e0, hipEvent_t e1, hipEvent_t eb) {
    float ms = -1.0f;
    (void)hipEventRecord(e0, a);
    hipLaunchKernelGGL(k_spin_100us, dim3(1), dim3(1), 0, a, 10000ull, (unsigned*)nullptr);
    if (b) {
        hipLaunchKernelGGL(k_spin_100us, dim3(1), dim3(1), 0, b, 10000ull, (unsigned*)nullptr);
        (void)hipEventRecord(eb, b);
        (void)hipStreamWaitEvent(a, eb, 0);
    }
    (void)hipEventRecord(e1, a);
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { (void)hipGetLastError(); return -1.0f; }
    return ms;
}
bool make_own_streams(evac_handle* h) {
    DeviceGuard g(h->device);
    hipEvent_t e0 = nullptr, e1 = nullptr, eb = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t i = 0; i < g_pool_pairs.size(); ++i)
            if (g_pool_pairs[i].device == h->device) {        // a pair an earlier handle found to overlap, idle since that handle was destroyed
                h->own.s[0] = g_pool_pairs[i].s[0];
                h->own.s[1] = g_pool_pairs[i].s[1];
                g_pool_pairs.erase(g_pool_pairs.begin() + (long)i);
                break;
            }
    }
    bool ok = h->own.s[0] != nullptr;
    if (!ok) {
        ok = hipStreamCreateWithFlags(&h->own.s[0], hipStreamNonBlocking) == hipSuccess && hipEventCreate(&e0) == hipSuccess &&
             hipEventCreate(&e1) == hipSuccess && hipEventCreate(&eb) == hipSuccess;
    }
    if (ok && !h->own.s[1]) {
        (void)spin_pair_ms(h->own.s[0], nullptr, e0, e1, eb);                 // (first launch: the code object is loaded)
        const float one = spin_pair_ms(h->own.s[0], nullptr, e0, e1, eb);
        hipStream_t dropped[8];
        int n_dropped = 0;
        for (int c = 0; ok && c < 8; ++c) {
            hipStream_t cand = nullptr;
            if (hipStreamCreateWithFlags(&cand, hipStreamNonBlocking) != hipSuccess) { ok = false; break; }
            (void)spin_pair_ms(h->own.s[0], cand, e0, e1, eb);                // (first use: the stream gets its queue here)
            const float pair = spin_pair_ms(h->own.s[0], cand, e0, e1, eb);
            if (c == 7 || (one > 0.0f && pair > 0.0f && pair < 1.5f * one)) { h->own.s[1] = cand; break; }
            dropped[n_dropped++] = cand;          // (kept until the search ends: its queue assignment stays used up, which moves the next candidate on)
        }
        for (int k = 0; k < n_dropped; ++k) (void)hipStreamDestroy(dropped[k]);
        ok = ok && h->own.s[1] != nullptr;
    }
    for (int k = 0; ok && k < 2; ++k) ok = hipEventCreateWithFlags(&h->own.done[k], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&h->own.fork, hipEventDisableTiming) == hipSuccess;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (eb) (void)hipEventDestroy(eb);
    if (!ok) (void)hipGetLastError();
    return ok;
}
// a command for the resident kernel: the payload, a store fence, then the sequence number in the same 64-byte segment (through the BAR)
void post_command(evac_handle* h, int n_steps, const void* slab, const void* stats, const void* actions) {
    volatile evac::PersistCmd* c = (volatile evac::PersistCmd*)(h->xchg + (size_t)(h->persist.seq & (evac::kPersistRing - 1)) * 64);
    c->slab = (unsigned long long)(uintptr_t)slab;
    c->stats = (unsigned long long)(uintptr_t)stats;
    c->actions = (unsigned long long)(uintptr_t)actions;
    c->n_steps = n_steps;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    c->seq = (unsigned)h->persist.seq + 1u;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    h->persist.seq += 1;
}
// gives back what the handle took for its form (evac_destroy, or a form that could not be set up): the own streams to the pool, the
// parts, the uncached area; the handle is Plain afterwards.  (evac_destroy has settled first: the own streams are only drained here.)
void release_own(evac_handle* h) {
    DeviceGuard g(h->device);
    for (int k = 0; k < 2; ++k)
        if (h->own.s[k]) (void)hipStreamSynchronize(h->own.s[k]);
    if (h->own.s[0] && h->own.s[1] && pools_on()) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_pool_pairs.push_back(PooledPair{h->device, {h->own.s[0], h->own.s[1]}});
        h->own.s[0] = h->own.s[1] = nullptr;
    }
    for (int k = 0; k < 2; ++k) {
        if (h->own.s[k]) (void)hipStreamDestroy(h->own.s[k]);
        if (h->own.done[k]) (void)hipEventDestroy(h->own.done[k]);
        if (h->part[k]) {
            give_error_word(h->device, (void*)h->part[k]->team_flag_host, (void*)h->part[k]->team_flag_dev);
            delete h->part[k];
        }
        h->part[k] = nullptr;
    }
    if (h->own.fork) (void)hipEventDestroy(h->own.fork);
    if (h->last_ev) (void)hipEventDestroy(h->last_ev);
    give_uncached(h->device, h->xchg, h->xchg_bytes);
    h->own = {};
    h->xchg = nullptr;
    h->xchg_bytes = 0;
    h->last_ev = nullptr;
    h->form = Form::Plain;
}
// the explicit deal (k_schedule) on `s`: evac_reschedule, and the first launch under a fresh schedule
void deal_now(evac_handle_t h, hipStream_t s, bool both);
// What the next launch under the schedule (moving[2][E] | perm[2][E]) gets: launch g reads perm[g & 1] and leaves its loads in
// moving[g & 1]; `deals`: its workgroup 0 also deals perm[(g + 1) & 1] for the next launch from the loads in moving[(g + 1) & 1]
struct Deal { const int32_t* perm; int32_t* moving; const int32_t* loads; int32_t* next; };
Deal deal_of(const evac_handle* h, bool deals) {
    const int E = h->p.n_envs, g = h->sched_gen;
    const bool dealt = h->sched && g >= 0;                  // (never dealt yet, e.g. a first launch under capture: identity)
    deals = deals && dealt;
    return Deal{dealt ? h->sched + (2 + (g & 1)) * E : nullptr, h->sched ? h->sched + (dealt ? (g & 1) : 0) * E : nullptr,
                deals ? h->sched + ((g + 1) & 1) * E : nullptr, deals ? h->sched + (2 + ((g + 1) & 1)) * E : nullptr};
}
// The persistent rollout kernel on the handle's stream.  fresh: the first kernel after a join -- every env starts at command
// h->persist.seq, workgroup 0 deals the next kernel's envs as it starts; resume: every env at the command it had reached when the kernel
// before left; stop_at: the index of a STOP command that is already in the ring (the finisher of a join), else INT_MAX.
int launch_persistent(evac_handle* h, int resume, int stop_at, bool fresh) {
    using FW = evac::Wave<1, 1024>;
    using FW4 = evac::Wave<4, 1024>;
    hipStream_t S = h->own.s[0];
    const int E = h->p.n_envs;
    if (h->sched && h->sched_gen < 0) deal_now(h, S, true);
    const Deal d = deal_of(h, fresh);                       // (workgroup 0 deals the NEXT fresh kernel's envs as it starts)
    if (d.next) h->sched_gen += 1;
    evac::ChainArgs ca{h->xchg, h->persist.seq, nullptr, nullptr, 0, nullptr, resume, stop_at};
    if (h->team_k) {
        // a team grid (evac_team.h): the exchange area starts with the tag of no round, the teams' verdicts at zero; team grids of one
        // device take turns (g_team_chain), whatever handle or stream they come from
        int32_t* decision = (int32_t*)(h->xchg + (size_t)evac::kPersistRing * 64 + 128) + E;
        if (hipMemsetAsync(h->p.team_rec, 0xff, h->team_xchg_bytes, S) != hipSuccess || hipMemsetAsync(decision, 0, 4 * (size_t)E, S) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, EVAC_ERR_HIP, "evac_rollout (persistent team kernel): hipMemsetAsync failed");
        }
        const int* np_ = nullptr;
        int* nq_ = nullptr;
        void* argv[] = {(void*)&h->p, (void*)&np_, (void*)&nq_, (void*)&np_, (void*)&nq_, (void*)&ca};
        const hipError_t le = launch_team_grid(h, team_persist_kernel(h), argv, S, /*in_chain=*/true, /*coop=*/false);
        if (le != hipSuccess) return fail(h, EVAC_ERR_HIP, std::string("evac_rollout (persistent team kernel): ") + hipGetErrorString(le));
    } else {
        const bool four = h->cu_wide4;
        const auto fn = four ? EVAC_PICK(h, k_rollout_persist_default_config, k_rollout_persist, FW4)
                             : EVAC_PICK(h, k_rollout_persist_default_config, k_rollout_persist, FW);
        const dim3 grid((unsigned)(E / (four ? FW4::kEnvsPerBlock : FW::kEnvsPerBlock)));
        hipLaunchKernelGGL(fn, grid, dim3(four ? FW4::kBlock : FW::kBlock), 0, S, h->p, d.perm, d.moving, d.loads, d.next, ca);
    }
    if (const int lc = check_launch(h, "evac_rollout (persistent kernel)"); lc != EVAC_OK) return lc;
    if (hipEventRecord(h->last_ev, S) != hipSuccess) { (void)hipGetLastError(); return fail(h, EVAC_ERR_HIP, "evac_rollout: event record behind the persistent kernel failed"); }
    return EVAC_OK;
}
// STOP, and behind the resident kernel a FINISHER: a kernel that takes up every env that has not yet run everything up to the STOP (the
// resident kernel may have left, or be leaving, for lack of commands) and ends at once where there is nothing to do.
int stop_persistent(evac_handle* h) {
    const int stop_index = h->persist.seq;
    post_command(h, 0, nullptr, nullptr, nullptr);
    h->persist.running = false;
    return launch_persistent(h, /*resume=*/1, stop_index, /*fresh=*/false);
}
// SETTLE the handle: `stream` waits for everything the own streams have been given so far, and the caller's state arrays are the state
// again, whatever the form -- a resident persistent kernel is told to STOP (+ the finisher), the chain's records are exported and the chain
// starts afresh behind whatever follows, since that may write the state.  evac_join is this; every call on the handle that is not a
// rollout in its form does it first (include/evac.h).  host_wait: the host waits for the settled work too -- before a rebind, whose old
// buffers the launches in flight still use.
int settle(evac_handle* h, hipStream_t stream, bool host_wait = false) {
    if (h->form == Form::Chain) h->chain.restart = true;
    if (!h->own.pending) return EVAC_OK;
    DeviceGuard g(h->device);
    if (h->form == Form::Persist && h->persist.running)     // STOP: the waves store their state and the kernel ends (+ the finisher)
        if (const int rc = stop_persistent(h); rc != EVAC_OK) return rc;
    for (int k = 0; k < 2; ++k)
        if (hipEventRecord(h->own.done[k], h->own.s[k]) != hipSuccess || hipStreamWaitEvent(stream, h->own.done[k], 0) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, EVAC_ERR_HIP, "evac_join: event record / wait failed");
        }
    h->own.pending = false;
    h->own.forked = false;
    if (h->form == Form::Chain && h->chain.dirty) {     // the chain's launches kept the state in the exchange records: back to the caller's arrays
        const int wpe = h->cu_wide4 ? 4 : 1;
        hipLaunchKernelGGL(evac::k_chain_export, dim3((unsigned)((h->p.n_envs * wpe + 3) / 4)), dim3(256), 0, stream, h->p, (const char*)h->xchg, wpe);
        h->chain.dirty = false;
        if (hipGetLastError() != hipSuccess) return fail(h, EVAC_ERR_HIP, "evac_join: export of the chain's state failed");
    }
    if (host_wait && hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return fail(h, EVAC_ERR_HIP, "hipDeviceSynchronize failed"); }
    return EVAC_OK;
}
// What the chained and the persistent form allocate themselves, in the device's pools: the own streams, an error word (a handle has one:
// the teams' serves the form too), `bytes` of uncached device memory (zeroed) and last_ev.  false: the handle keeps none of it but the word.
bool take_form_resources(evac_handle* h, size_t bytes) {
    bool ok = make_own_streams(h);
    DeviceGuard g(h->device);
    if (ok && !h->team_flag_host) {
        void* host = nullptr;
        void* dev = nullptr;
        ok = take_error_word(h->device, &host, &dev);
        h->team_flag_host = (volatile unsigned*)host;
        h->team_flag_dev = (unsigned*)dev;
    }
    ok = ok && hipEventCreateWithFlags(&h->last_ev, hipEventDisableTiming) == hipSuccess;
    if (ok) {
        h->xchg = (char*)take_uncached(h->device, bytes, &h->xchg_bytes);
        ok = h->xchg != nullptr;
    }
    if (ok && (hipMemset(h->xchg, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) ok = false;   // (hipMemset does not wait)
    if (!ok) {
        (void)hipGetLastError();
        release_own(h);
    }
    return ok;
}
}  // namespace

extern "C" {

int evac_create(const evac_config_t* cfg, int32_t num_envs, int32_t device, uint64_t seed, uint64_t env_id_offset,
                evac_handle_t* out) {
    return evac_create_ex(cfg, num_envs, device, seed, env_id_offset, nullptr, out);
}

int evac_create_ex(const evac_config_t* cfg, int32_t num_envs, int32_t device, uint64_t seed, uint64_t env_id_offset,
                   const evac_options_t* options, evac_handle_t* out) {
    evac_options_t o = EVAC_OPTIONS_AUTO;
    if (options) o = *options; else o.parts = 1;         // (evac_create: the stream contract existing callers rely on)
    const int32_t* f = &o.subwave;
    for (int k = 0; k < (int)(sizeof(o) / sizeof(int32_t)); ++k)
        if (f[k] < -1 || f[k] > 16) { g_create_error = "evac_options_t: every field must be -1 (automatic) or a small non-negative value"; if (out) *out = nullptr; return EVAC_ERR_INVALID_ARGUMENT; }
    if (!options) o.chain = 0;
    if (o.parts == 0 || o.parts > 2) { g_create_error = "evac_options_t.parts must be -1, 1 or 2"; if (out) *out = nullptr; return EVAC_ERR_INVALID_ARGUMENT; }
    if (o.chain > 2) { g_create_error = "evac_options_t.chain must be -1, 0, 1 or 2"; if (out) *out = nullptr; return EVAC_ERR_INVALID_ARGUMENT; }
    const int rc = create_impl(cfg, num_envs, device, seed, env_id_offset, o, out);
    if (rc != EVAC_OK) return rc;
    evac_handle* h = *out;
    // Chained launches (include/evac.h): the CU-wide kernels of one-wave envs, whole workgroups only (a wave that gives up must not
    // leave others at a barrier: that family has none), and a host-mapped error word like the teams'.  Wins over parts.
    const int chain_opt = option_value("EVAC_CHAIN", o.chain);
    int can_wait_value = 0;
    if (hipDeviceGetAttribute(&can_wait_value, hipDeviceAttributeCanUseStreamWaitValue, device) != hipSuccess) { (void)hipGetLastError(); can_wait_value = 0; }
    const bool chain_one_wave = h->cu_wide && num_envs % 16 == 0 && num_envs >= 32;
    const bool chain_four_waves = h->cu_wide4 && num_envs % 4 == 0 && num_envs >= 8;     // (the CU-wide form of four-wave envs: a barrier per env in LDS)
    // ... and the 256-thread workgroups of one-wave envs (four envs each), on request only (chain = 1 with cu_wide = 0)
    const bool chain_small = chain_opt == 1 && !h->cu_wide && !h->cu_wide4 && h->sub_lanes == 0 && !h->cells && !h->team_k &&
                             waves_per_env(h->p.n_ped) == 1 && num_envs % 4 == 0 && num_envs >= 8;
    // chain = 2: ONE PERSISTENT KERNEL PER JOIN (evac_common.h, PersistCmd).  The CU-wide kernels only (every workgroup resident at once: the grid
    // must fit the device), and only where the host can write device memory directly (large BAR): the command ring lives in uncached device
    // memory, written by the CPU -- no stream operation of ours could run while the resident kernel holds every CU.
    // Where a form cannot be set up, the handle falls back to the next one: persistent, chained, parts, plain.
    int large_bar = 0;
    if (chain_opt == 2 && hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, device) != hipSuccess) { (void)hipGetLastError(); large_bar = 0; }
    const int per_wg = h->cu_wide4 ? 4 : 16;
    // (teams -- one env on K CUs: the grid's fit is checked where it is for plain team launches, at the call, once the exchange areas are bound)
    const bool persist_fits = ((h->cu_wide || h->cu_wide4) && num_envs % per_wg == 0 && num_envs / per_wg <= h->cus) || (h->team_k != 0 && !h->team_fault);
    const size_t ring_bytes = (size_t)evac::kPersistRing * 64 + 128 + 8 * (size_t)num_envs;      // the ring, a line of diagnostics, next_cmd[E], decision[E] (teams)
    if (chain_opt == 2 && large_bar != 0 && persist_fits && take_form_resources(h, ring_bytes)) {
        h->abort_word = (unsigned*)(h->xchg + (size_t)evac::kPersistRing * 64);
        h->form = Form::Persist;
        h->opt.chain = 2;
        h->variant[3] = h->variant[1] + ", one persistent kernel per join";
        return EVAC_OK;
    }
    // The exchange records (evac_common.h) live in UNCACHED device memory, the second thing a chained handle allocates
    // itself.  In ordinary hipMalloc memory -- the caller's workspace -- a record line can sit in the L2 of an XCD that once
    // touched it with a plain access (the workspace's zero fill, the import), and another XCD's write-through store does not
    // refresh that copy: an import written with `sc1` stores over the zero-filled workspace read back as zeros in ~1.5 of a
    // record's 12 lines (tools/chain_debug.py, round 6).  A plain-store import cured that case, but the same can happen to the
    // import's own lines once a batch that fills the chip lets workgroups land on whatever XCD has room.  Memory that no L2
    // ever holds removes the question: 1.5 KB per env and launch at memory speed is nothing next to 20 steps.
    const size_t xchg_bytes = (size_t)num_envs * (size_t)evac::xchg_bytes(h->cu_wide4 ? 256 : 64);
    if (chain_opt != 0 && can_wait_value && (chain_one_wave || chain_four_waves || chain_small) && take_form_resources(h, xchg_bytes)) {
        h->chain.small = chain_small;
        h->form = Form::Chain;
        h->opt.chain = 1;
        h->variant[3] = h->variant[1] + ", chained launches on 2 streams";
        return EVAC_OK;
    }
    // Two parts: where it pays by itself (-1) -- CU-wide rollouts whose halves are whole CU-wide workgroups; the halves keep the
    // CU-wide form although each alone would not fill the device (pace keeping and the in-kernel deal are what they are to keep) --
    // or on request (2) for every handle but the teams' (their grids run one at a time: evac_rollout).
    const int parts_opt = option_value("EVAC_PARTS", o.parts);
    const bool can = h->team_k == 0 && num_envs >= 2 && num_envs % 2 == 0;
    const bool pays = (h->cu_wide || h->cu_wide4) && num_envs % (2 * per_wg) == 0;
    if (!(can && (parts_opt == 2 || (parts_opt < 0 && pays)))) return EVAC_OK;
    evac_options_t po = h->opt;                        // the parts take the parent's resolved choices
    po.parts = 1;
    po.chain = 0;
    const int32_t half = num_envs / 2;
    bool ok = make_own_streams(h);
    for (int k = 0; ok && k < 2; ++k) {
        evac_handle_t c = nullptr;
        ok = create_impl(cfg, half, device, seed, env_id_offset + (uint64_t)k * (uint64_t)half, po, &c) == EVAC_OK;
        h->part[k] = c;
        if (ok) c->p.slab_envs = num_envs;
    }
    if (!ok) { release_own(h); return EVAC_OK; }      // (no second queue, no parts: the handle works as one)
    h->form = Form::Parts;
    h->opt.parts = 2;
    h->variant[3] = h->part[0]->variant[1] + " x 2 streams";
    return EVAC_OK;
}

int evac_get_options(evac_handle_t h, evac_options_t* out) {
    if (!h || !out) return EVAC_ERR_INVALID_ARGUMENT;
    *out = h->opt;
    return EVAC_OK;
}

int evac_join(evac_handle_t h, void* stream) {
    if (!h) return EVAC_ERR_INVALID_ARGUMENT;
    return settle(h, (hipStream_t)stream);
}
int evac_order_next_rollout(evac_handle_t h) {
    if (!h) return EVAC_ERR_INVALID_ARGUMENT;
    h->own.forked = false;
    return EVAC_OK;
}
int32_t evac_num_parts(evac_handle_t h) { return h ? (h->form == Form::Parts ? 2 : 1) : -1; }
int32_t evac_own_streams(evac_handle_t h) { return h ? (h->own.s[0] ? 2 : 0) : -1; }     // (the streams stay when evac_team_clear_error falls back)
void* evac_part_stream(evac_handle_t h, int32_t part) { return (h && h->own.s[0] && part >= 0 && part < 2) ? (void*)h->own.s[part] : nullptr; }

const char* evac_kernel_variant(evac_handle_t h, int32_t rollout) {
    if (!h) return "";
    if (!rollout) return h->variant[0].c_str();
    if (h->form == Form::Persist) {          // (teams: the persistent form of the team kernel, once its exchange areas are bound and its grid fits)
        const bool team = h->team_k && h->team_bound && h->team_fit != 0;
        if (h->team_k && !team) return h->variant[1].c_str();
        h->variant[3] = h->variant[team ? 2 : 1] + ", one persistent kernel per join";
        return h->variant[3].c_str();
    }
    if (h->form == Form::Parts || (h->form == Form::Chain && h->chain.bound)) return h->variant[3].c_str();
    // the path evac_rollout takes right now: teams only with their exchange areas bound and a grid that fits the device
    return h->variant[(h->team_k && h->team_bound && h->team_fit != 0) ? 2 : 1].c_str();
}

int evac_destroy(evac_handle_t h) {
    if (!h) return EVAC_OK;
    DeviceGuard g(h->device);
    (void)settle(h, nullptr);
    // Nothing the handle launched may still run when its streams and its error word go back to the pools -- the plain team launches on the
    // caller's streams included: one that timed out later would raise the word of whatever handle takes it next.
    if (h->own.s[0] || h->team_flag_host) (void)hipDeviceSynchronize();
    release_own(h);
    give_error_word(h->device, (void*)h->team_flag_host, (void*)h->team_flag_dev);
    delete h;
    return EVAC_OK;
}

int64_t evac_obs_dim(evac_handle_t h) { return h ? h->p.obs_dim : -1; }
int32_t evac_num_envs(evac_handle_t h) { return h ? h->p.n_envs : -1; }

int64_t evac_algorithmic_bytes_per_env_step(evac_handle_t h) {
    if (!h) return -1;
    // per agent-update 16 B read + 16 B write of (x,y,dx,dy); per env-step: action 8 +
    // leader pos 8 r / 8 w + now 4 r / 4 w + reward 4 + terminated 1 + truncated 1 = 38; plus the obs write.
    return 32ll * h->p.n_ped + 38ll + 4ll * h->p.obs_dim;
}

int evac_bind_state(evac_handle_t h, float* ped, uint8_t* status, float* agent, int32_t* clock, float* acc) {
    if (!h) return EVAC_ERR_INVALID_ARGUMENT;
    if (!ped || !status || !agent || !clock || !acc) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_bind_state: NULL buffer");
    if (((uintptr_t)ped | (uintptr_t)agent | (uintptr_t)clock | (uintptr_t)acc) & 15u)
        return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_bind_state: ped/agent/clock/acc must be 16-byte aligned");
    if (const int rc = settle(h, nullptr, /*host_wait=*/true); rc != EVAC_OK) return rc;      // (launches in flight use the old buffers)
    h->p.ped = (float4*)ped;
    h->p.status = status;
    h->p.agent = (float4*)agent;
    h->p.clock = (int4*)clock;
    h->p.acc = (float4*)acc;
    h->bound = true;
    for (int k = 0; k < (h->form == Form::Parts ? 2 : 0); ++k) {      // the parts: the same buffers from their first env on
        const size_t first = (size_t)k * (size_t)h->part[k]->p.n_envs, N = (size_t)h->p.n_ped;
        const int rc = evac_bind_state(h->part[k], ped + first * N * 4, status + first * N, agent + first * 4, clock + first * 4, acc + first * 4);
        if (rc != EVAC_OK) return fail(h, rc, std::string("evac_bind_state (part): ") + h->part[k]->err);
    }
    return EVAC_OK;
}

namespace {
struct WorkspaceLayout {
    size_t sched, stats, team_rec, team_tile, team_xchg_end, chain_sched, chain_abort, total;
};
WorkspaceLayout workspace_layout(const evac_handle* h) {
    const size_t E = (size_t)h->p.n_envs;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    WorkspaceLayout w{};
    size_t o = 0;
    w.sched = o; o = up(o + 4 * E * sizeof(int32_t));          // moving[2][E] | perm[2][E]
    w.stats = o; o = up(o + 64);
    if (h->form == Form::Chain) {                              // moving[4][E] | perm[4][E] | the abort word + started-workgroups counter
        w.chain_sched = o; o = up(o + 8 * E * sizeof(int32_t));    // (the exchange records are NOT here: they need memory the L2s do not cache,
        w.chain_abort = o; o = up(o + 128);                        //  which the library allocates itself: evac_create_ex)
    }
    if (h->team_k) {
        w.team_rec = o; o = up(o + evac::kTeamSets * E * 32 * 16);          // (two slot sets: evac_team.h, exchange)
        w.team_tile = o; o = up(o + evac::kTeamSets * E * 1024 * 16);
        w.team_xchg_end = o;
    }
    w.total = o;
    return w;
}
}  // namespace

int64_t evac_workspace_bytes(evac_handle_t h) {
    if (!h) return -1;
    size_t total = workspace_layout(h).total, parts = 0;
    for (int k = 0; k < (h->form == Form::Parts ? 2 : 0); ++k) parts += workspace_layout(h->part[k]).total;   // (the parts carve it up between them)
    return (int64_t)(parts > total ? parts : total);
}

int evac_bind_workspace(evac_handle_t h, void* workspace, int64_t bytes) {
    if (!h) return EVAC_ERR_INVALID_ARGUMENT;
    if (const int rc = settle(h, nullptr, /*host_wait=*/true); rc != EVAC_OK) return rc;    // (launches in flight use the old workspace)
    h->sched = nullptr;
    h->sched_gen = -1;
    h->team_bound = false;
    h->chain.bound = false;
    if (h->form == Form::Parts) {
        // the parts schedule themselves: each gets a slice (moving[2][E/2] | perm[2][E/2] of its own); this handle's own rollouts --
        // the diagnostic face only -- run without a schedule
        if (workspace && (bytes < evac_workspace_bytes(h) || ((uintptr_t)workspace & 255u)))
            return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_bind_workspace: workspace smaller than evac_workspace_bytes() or not 256-byte aligned");
        size_t o = 0;
        for (int k = 0; k < 2; ++k) {
            const size_t t = workspace_layout(h->part[k]).total;
            const int rc = evac_bind_workspace(h->part[k], workspace ? (char*)workspace + o : nullptr, (int64_t)t);
            if (rc != EVAC_OK) return fail(h, rc, std::string("evac_bind_workspace (part): ") + h->part[k]->err);
            o += t;
        }
        return EVAC_OK;
    }
    if (!workspace) return EVAC_OK;
    const WorkspaceLayout w = workspace_layout(h);
    if (bytes < (int64_t)w.total) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_bind_workspace: workspace smaller than evac_workspace_bytes()");
    if ((uintptr_t)workspace & 255u) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_bind_workspace: workspace must be 256-byte aligned");
    char* base = (char*)workspace;
    h->sched = (int32_t*)(base + w.sched);
    if (h->form == Form::Chain) {
        h->chain.sched = (int32_t*)(base + w.chain_sched);
        h->abort_word = (unsigned*)(base + w.chain_abort);
        h->chain.dirty = false;
        h->chain.wgs = 0;                             // (the workspace comes zero-filled: include/evac.h)
        h->chain.bound = true;
    }
    if (h->team_k) {
        h->p.team_err = h->team_flag_dev;           // (host-mapped memory of the handle, not part of the workspace)
        h->p.team_rec = base + w.team_rec;
        h->p.team_tile = base + w.team_tile;
        h->team_xchg_bytes = w.team_xchg_end - w.team_rec;
        h->team_bound = true;
        DeviceGuard g(h->device);
        (void)team_grid_fits(h);                      // (so that evac_kernel_variant names the path the first rollout will take)
    }
    return EVAC_OK;
}

namespace {
// the explicit deal (k_schedule): the permutation launch `gen` will read, from the loads launch gen - 1 left; `both`: the other
// permutation buffer too
void deal_now(evac_handle_t h, hipStream_t s, bool both) {
    const int E = h->p.n_envs;
    if (h->sched_gen < 0) h->sched_gen = 0;
    const int g = h->sched_gen;
    hipLaunchKernelGGL(evac::k_schedule, dim3(1), dim3(1024), 0, s, E, (const int*)(h->sched + ((g + 1) & 1) * E),
                       h->sched + (2 + (g & 1)) * E, both ? h->sched + (2 + ((g + 1) & 1)) * E : (int32_t*)nullptr,
                       h->cu_wide4 ? 4 : 16, h->cu_wide4 ? 4 : 1, 0);
}
}  // namespace

int evac_reschedule(evac_handle_t h, void* stream) {
    if (!h) return EVAC_ERR_INVALID_ARGUMENT;
    // (on the caller's stream, behind everything the own streams have been given: a resident kernel keeps the deal it started with)
    if (const int rc = settle(h, (hipStream_t)stream); rc != EVAC_OK) return rc;
    if (h->form == Form::Chain) return EVAC_OK;       // (the chain deals itself again when it restarts)
    if (h->form == Form::Parts) {
        for (int k = 0; k < 2; ++k)
            if (const int rc = evac_reschedule(h->part[k], stream); rc != EVAC_OK) return fail(h, rc, h->part[k]->err);
        return EVAC_OK;
    }
    if (!h->sched || !(h->cu_wide || h->cu_wide4)) return EVAC_OK;       // nothing to deal
    DeviceGuard g(h->device);
    deal_now(h, (hipStream_t)stream, true);
    return check_launch(h, "evac_reschedule");
}

int32_t evac_schedule_generation(evac_handle_t h) {
    if (h && h->form == Form::Parts) return evac_schedule_generation(h->part[0]);
    return (h && h->sched && (h->cu_wide || h->cu_wide4)) ? h->sched_gen : -1;
}

int evac_peer_gather(const float* src, int64_t rows, int32_t row_words, int32_t take_words, float* const* peer_dst, int32_t world,
                     int32_t my_rank, int32_t wgs_per_peer, void* stream) {
    if (!src || !peer_dst || rows <= 0 || row_words <= 0 || take_words <= 0 || take_words > row_words || world < 1 ||
        world > evac::kMaxPeers || my_rank < 0 || my_rank >= world)
        return EVAC_ERR_INVALID_ARGUMENT;
    if (rows * (int64_t)take_words >= (int64_t)1 << 31) return EVAC_ERR_INVALID_ARGUMENT;      // (32-bit element indices)
    evac::PeerPtrs pp{};
    for (int r = 0; r < world; ++r) {
        if (!peer_dst[r]) return EVAC_ERR_INVALID_ARGUMENT;
        pp.dst[r] = peer_dst[r];
    }
    DeviceGuard g(device_of(src));                    // (no handle: the kernel must run on the device that owns the slab)
    const unsigned n = (unsigned)(rows * take_words);
    int w = wgs_per_peer > 0 ? wgs_per_peer : 8;
    const int need = (int)((n + 1023u) / 1024u);                 // (no more workgroups than 1024-element pieces)
    if (w > need) w = need < 1 ? 1 : need;
    const dim3 grid((unsigned)(w * world)), block(256);
    hipStream_t s_ = (hipStream_t)stream;
    if (take_words == 6)
        hipLaunchKernelGGL((evac::k_peer_gather<6>), grid, block, 0, s_, src, n, (unsigned)row_words, 6u, pp, (int)my_rank, (int)world, n, w);
    else if (take_words == 9)
        hipLaunchKernelGGL((evac::k_peer_gather<9>), grid, block, 0, s_, src, n, (unsigned)row_words, 9u, pp, (int)my_rank, (int)world, n, w);
    else
        hipLaunchKernelGGL((evac::k_peer_gather<0>), grid, block, 0, s_, src, n, (unsigned)row_words, (unsigned)take_words, pp, (int)my_rank,
                           (int)world, n, w);
    return hipGetLastError() == hipSuccess ? EVAC_OK : EVAC_ERR_HIP;
}

int evac_team_error(evac_handle_t h, int32_t* out) {
    if (!h || !out) return EVAC_ERR_INVALID_ARGUMENT;
    *out = 0;
    if (!h->team_flag_host) return EVAC_OK;
    DeviceGuard g(h->device);
    if (hipDeviceSynchronize() != hipSuccess) return fail(h, EVAC_ERR_HIP, "evac_team_error: hipDeviceSynchronize failed");
    *out = (int32_t)*h->team_flag_host;
    return EVAC_OK;
}

int evac_team_error_nosync(evac_handle_t h, int32_t* out) {
    if (!h || !out) return EVAC_ERR_INVALID_ARGUMENT;
    *out = h->team_flag_host ? (int32_t)*h->team_flag_host : 0;
    return EVAC_OK;
}

int evac_team_clear_error(evac_handle_t h) {
    if (!h) return EVAC_ERR_INVALID_ARGUMENT;
    if (!h->team_flag_host) return EVAC_OK;
    if (const int rc = settle(h, nullptr, /*host_wait=*/true); rc != EVAC_OK) return rc;
    if (*h->team_flag_host != 0u) {                  // the handle stays on one workgroup per env and on plain launches
        h->team_k = 0;
        h->form = Form::Plain;
    }
    *h->team_flag_host = 0u;
    return EVAC_OK;
}

#define EVAC_REQUIRE_BOUND(h, name)                                               \
    if (!(h)) return EVAC_ERR_INVALID_ARGUMENT;                                  \
    if (!(h)->bound) return fail((h), EVAC_ERR_NOT_BOUND, name ": call evac_bind_state first"); \
    if (const int ta_ = team_aborted((h), name); ta_ != EVAC_OK) return ta_
// (whatever is not a rollout in the handle's form settles it first: the caller's arrays are the state, `stream` behind the own streams)
#define EVAC_REQUIRE_SETTLED(h, name, stream)                                     \
    EVAC_REQUIRE_BOUND(h, name);                                                  \
    if (const int st_ = settle((h), (hipStream_t)(stream)); st_ != EVAC_OK) return st_

int evac_reset(evac_handle_t h, const uint8_t* mask, const float* draws, float* obs_out, void* stream) {
    EVAC_REQUIRE_SETTLED(h, "evac_reset", stream);
    if (draws && ((uintptr_t)draws & 15u)) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_reset: draws must be 16-byte aligned");
    DeviceGuard g(h->device);
    EVAC_DISPATCH(h, k_reset, stream, h->p, mask, (const float4*)draws, obs_out);
    return check_launch(h, "evac_reset");
}

#define EVAC_STEP_ARGS h->p, (const float2*)actions, noise, obs_out, reward_out, terminated_out, truncated_out, (int)autoreset, final_obs, final_stats, na

static int step_common(evac_handle_t h, const char* name, const float* actions, const float* noise, float* obs_out,
                       float* reward_out, uint8_t* terminated_out, uint8_t* truncated_out, int32_t autoreset, float* final_obs,
                       evac_episode_stats_t* final_stats, const evac::NormArgs& na, void* stream) {
    if (!actions || !obs_out || !reward_out || !terminated_out || !truncated_out)
        return fail(h, EVAC_ERR_INVALID_ARGUMENT, std::string(name) + ": actions/obs/reward/terminated/truncated must be non-NULL");
    if ((uintptr_t)actions & 7u) return fail(h, EVAC_ERR_INVALID_ARGUMENT, std::string(name) + ": actions must be 8-byte aligned");
    DeviceGuard g(h->device);
    if (na.state && h->default_cfg) EVAC_DISPATCH(h, k_step_norm_default_config, stream, EVAC_STEP_ARGS);
    else if (na.state) EVAC_DISPATCH(h, k_step_norm, stream, EVAC_STEP_ARGS);
    else if (h->default_cfg) EVAC_DISPATCH(h, k_step_default_config, stream, EVAC_STEP_ARGS);
    else EVAC_DISPATCH(h, k_step_raw, stream, EVAC_STEP_ARGS);
    return check_launch(h, name);
}

int evac_step(evac_handle_t h, const float* actions, const float* noise, float* obs_out, float* reward_out,
              uint8_t* terminated_out, uint8_t* truncated_out, int32_t autoreset, float* final_obs,
              evac_episode_stats_t* final_stats, void* stream) {
    EVAC_REQUIRE_SETTLED(h, "evac_step", stream);
    return step_common(h, "evac_step", actions, noise, obs_out, reward_out, terminated_out, truncated_out, autoreset, final_obs,
                       final_stats, evac::NormArgs{nullptr, 0.f, 0.f, 0.f, 0.f}, stream);
}

int evac_step_normalized(evac_handle_t h, const float* actions, const float* noise, float* obs_out, float* reward_out,
                         uint8_t* terminated_out, uint8_t* truncated_out, int32_t autoreset, float* final_obs,
                         evac_episode_stats_t* final_stats, double* norm_state, float gamma, float obs_clip,
                         float reward_clip, float epsilon, void* stream) {
    EVAC_REQUIRE_SETTLED(h, "evac_step_normalized", stream);
    if (!norm_state) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_step_normalized: norm_state is NULL");
    return step_common(h, "evac_step_normalized", actions, noise, obs_out, reward_out, terminated_out, truncated_out, autoreset,
                       final_obs, final_stats, evac::NormArgs{norm_state, gamma, obs_clip, reward_clip, epsilon}, stream);
}

// ---- evac_rollout, one function per form ----
static bool capturing(hipStream_t s) {
    hipStreamCaptureStatus c = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &c) != hipSuccess) { (void)hipGetLastError(); return false; }
    return c != hipStreamCaptureStatusNone;
}

// Form::Parts: two half-batch kernels on the handle's own streams, both behind what `stream` holds so far; `stream` is NOT made to
// wait for them (evac_join): consecutive rollout calls must not meet, or the halves would run in lock-step
static int rollout_parts(evac_handle* h, int32_t n_steps, const float* actions, float* slab_out, evac_episode_stats_t* final_stats, hipStream_t s_) {
    // (the fork costs a barrier packet in front of each kernel -- 7-10 us on this platform whether or not the event has fired,
    // DESIGN.md 6 -- which is more than the parts gain.  So the own streams are put behind the caller's stream ONCE per join: at
    // the first rollout call after evac_join / any other call on the handle, and at every call that brings inputs (actions).
    // Asking the stream instead -- hipStreamQuery -- was tried: the query leaves a marker in the stream, the next query finds it
    // busy, and the handle falls into forking at every call: a second, 15-40 % slower mode of the same program.)
    if (!h->own.forked || actions != nullptr) {
        if (hipEventRecord(h->own.fork, s_) != hipSuccess) { (void)hipGetLastError(); return fail(h, EVAC_ERR_HIP, "evac_rollout: hipEventRecord failed"); }
        for (int k = 0; k < 2; ++k)
            if (hipStreamWaitEvent(h->own.s[k], h->own.fork, 0) != hipSuccess) { (void)hipGetLastError(); return fail(h, EVAC_ERR_HIP, "evac_rollout: hipStreamWaitEvent failed"); }
        h->own.forked = true;
    }
    const size_t row = (size_t)h->p.obs_dim + 3;
    for (int k = 0; k < 2; ++k) {
        evac_handle* c = h->part[k];
        const size_t first = (size_t)k * (size_t)c->p.n_envs;
        h->own.pending = true;
        const int rc = evac_rollout(c, n_steps, actions ? actions + first * 2 : nullptr, nullptr, slab_out + first * row,
                                    final_stats ? final_stats + first : nullptr, 0, nullptr, nullptr, h->own.s[k]);
        if (rc != EVAC_OK) return fail(h, rc, std::string("evac_rollout (part): ") + c->err);
    }
    return EVAC_OK;
}

// Form::Persist: ONE PERSISTENT KERNEL PER JOIN: the call becomes a command of the resident kernel's ring.  The kernel is started -- behind
// what the caller's stream holds at this moment, as the parts' fork -- by the first call after a join (or after
// evac_order_next_rollout); the calls that follow cost the host a 64-byte write through the BAR and the device nothing but the
// steps: the state stays in registers.  A kernel that found no command for ~150 us has LEFT by itself (every env's state and place
// in the ring stored): the call then starts one that takes every env up where it stopped.  (Given actions take the plain path:
// their buffer is the caller's stream's business.)
static int rollout_persist(evac_handle* h, int32_t n_steps, float* slab_out, evac_episode_stats_t* final_stats, hipStream_t s_) {
    hipStream_t S = h->own.s[0];
    if (h->persist.running && !h->own.forked)            // the caller touched a buffer (evac_order_next_rollout): a new kernel behind a new fork
        if (const int rc = stop_persistent(h); rc != EVAC_OK) return rc;
    if (h->persist.running && h->persist.seq - h->persist.first >= evac::kPersistRing - 2) {
        // the ring is about to lap the slowest env: the kernel is stopped and WAITED FOR on the host (once per ~1000 calls without a join)
        if (const int rc = stop_persistent(h); rc != EVAC_OK) return rc;
        if (hipStreamSynchronize(S) != hipSuccess) { (void)hipGetLastError(); return fail(h, EVAC_ERR_HIP, "evac_rollout: the persistent kernel did not end"); }
    }
    if (!h->persist.running) {
        if (hipEventRecord(h->own.fork, s_) != hipSuccess || hipStreamWaitEvent(S, h->own.fork, 0) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, EVAC_ERR_HIP, "evac_rollout: fork of the persistent kernel failed");
        }
        h->own.forked = true;
        if (const int rc = launch_persistent(h, /*resume=*/0, /*stop_at=*/0x7fffffff, /*fresh=*/true); rc != EVAC_OK) return rc;
        h->persist.running = true;
        h->persist.first = h->persist.seq;
    } else if (hipEventQuery(h->last_ev) == hipSuccess) {
        // the kernel has left (idle): one that resumes.  (A kernel that is leaving RIGHT NOW is seen at the next call or at the join,
        // whose finisher runs whatever an env has not run yet: no command is lost, it only waits for that kernel.)
        if (const int rc = launch_persistent(h, /*resume=*/1, /*stop_at=*/0x7fffffff, /*fresh=*/false); rc != EVAC_OK) return rc;
    } else {
        (void)hipGetLastError();                         // (hipErrorNotReady: resident)
    }
    post_command(h, (int)n_steps, slab_out, final_stats, nullptr);
    h->own.pending = true;
    return EVAC_OK;
}

// Form::Chain: launch g on stream g & 1, ordered per env on the device (include/evac.h).  Both streams start behind what the
// caller's stream holds -- once per join (below): a barrier packet per launch costs more than the chain gains.
static int rollout_chain(evac_handle* h, int32_t n_steps, const float* actions, float* slab_out, evac_episode_stats_t* final_stats, hipStream_t s_) {
    using FW = evac::Wave<1, 1024>;
    using FW4 = evac::Wave<4, 1024>;
    using FS = evac::Wave<1, 256>;
    evac_handle::ChainState& ch = h->chain;
    const int wpe = h->cu_wide4 ? 4 : 1, per_wg = (h->cu_wide4 || ch.small) ? 4 : 16;
    const int E = h->p.n_envs, c = ch.gen;
    hipStream_t S = h->own.s[c & 1], O = h->own.s[(c + 1) & 1];
    // THE INVARIANT OF THE CHAIN: launch g + 1 must not start being dispatched before every workgroup of launch g has a CU.
    // A workgroup of g + 1 holds its CU while it waits for envs of launch g; were workgroups of g still waiting for CUs then,
    // the dispatcher -- which deals a grid's workgroups to the XCDs in order -- could find an XCD's CUs all held by waiting
    // workgroups of g + 1 and launch g would never be placed (seen: both streams released by ONE event started launches g and
    // g + 1 together and the second launch of a sweep timed out once in ~2000 sweeps; another kernel holding CUs while the
    // chain runs does the same; short of a deadlock the interleaved start left the pipeline in a 15-40 % slower rhythm for
    // the whole sweep).  So every workgroup of a chained launch counts itself in `started` when it gets its CU, and the QUEUE
    // of launch g + 1 waits -- hipStreamWaitValue64: the runtime's one-wave wait kernel (__amd_rocclr_streamOpsWait in a kernel
    // trace), one wave slot held, no workgroup of ours -- until the counter says that all workgroups of
    // launches <= g have started (+0.5 us per launch: tools/microbench/waitvalue.hip).  With it every wait inside a kernel is
    // for a workgroup that is resident or done, by induction down to the oldest launch in flight, which waits for nothing.
    const bool fork = ch.restart || !h->own.forked || actions != nullptr;      // (once per join, and with every new input: see rollout_parts)
    if (fork) {
        if (hipEventRecord(h->own.fork, s_) != hipSuccess || hipStreamWaitEvent(S, h->own.fork, 0) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, EVAC_ERR_HIP, "evac_rollout: fork of the chain failed");
        }
        h->own.forked = true;
    }
    int32_t* moving = ch.sched;
    int32_t* perm = ch.sched + 4 * (size_t)E;
    if (ch.restart) {
        // the state in memory is whatever the caller's stream left: every env at generation c, one deal in all four
        // permutation buffers, the other stream behind both
        hipLaunchKernelGGL(evac::k_chain_import, dim3((unsigned)((E * wpe + 3) / 4)), dim3(256), 0, S, h->p, h->xchg, c, h->abort_word, ch.wgs, wpe);
        if (!ch.small) {
            hipLaunchKernelGGL(evac::k_schedule, dim3(1), dim3(1024), 0, S, E, (const int*)(moving + ((c + 3) & 3) * (size_t)E),
                               perm + (c & 3) * (size_t)E, (int32_t*)nullptr, per_wg, wpe == 4 ? 4 : 1, option_value("EVAC_CHAIN_DEAL", 0));
            hipLaunchKernelGGL(evac::k_copy_perm3, dim3(64), dim3(256), 0, S, E, (const int*)(perm + (c & 3) * (size_t)E),
                               perm + ((c + 1) & 3) * (size_t)E, perm + ((c + 2) & 3) * (size_t)E, perm + ((c + 3) & 3) * (size_t)E);
        }
        // ... and the OTHER queue behind all of this.  Its gate alone does not order it: until the import has set the counter the
        // word holds whatever the workspace's memory held -- the caller's zero fill may not have run yet on this queue's
        // timeline, a recycled allocation carries the count of the handle that used it before -- and a gate that passes on such a
        // value starts launch c + 1 before the deal above exists: it then reads a permutation of ANOTHER batch (seen: a 64-env
        // handle in memory a 512-env handle had used took env indices up to 511 -- tests/test_gpu_parity.py, whole file only).
        if (hipEventRecord(h->last_ev, S) != hipSuccess || hipStreamWaitEvent(O, h->last_ev, 0) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, EVAC_ERR_HIP, "evac_rollout: restart of the chain failed");
        }
        ch.start = c;
        ch.restart = false;
    }
    const bool deals = !ch.small && c - ch.start >= 2;          // (the loads of launch c - 2, the last launch of this stream)
    const int32_t* deal_loads = deals ? moving + ((c + 2) & 3) * (size_t)E : nullptr;
    int32_t* deal_perm = deals ? perm + ((c + 2) & 3) * (size_t)E : nullptr;
    unsigned long long* started = (unsigned long long*)(h->abort_word + 8);      // (the same line as the abort word: bytes 32..39)
    // (the counter is never reset while the workspace is bound: a restart's first launch is gated too -- on the launches before
    // the restart, long done -- and the launch after it on the restart's own workgroups, hence behind its import and deal)
    if (ch.wgs > 0 && hipStreamWaitValue64(S, started, ch.wgs, hipStreamWaitValueGte, ~0ull) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, EVAC_ERR_HIP, "evac_rollout: hipStreamWaitValue64 (the chain's dispatch gate) failed");
    }
    static const int deal_mode = option_value("EVAC_CHAIN_DEAL", 0);                    // (diagnostic: A/B runs of one binary)
    evac::ChainArgs ca{h->xchg, c, h->abort_word, h->team_flag_dev, deal_mode, started};
    evac::Params pp = h->p;
    if (h->team_fault && c == ch.start + 1) pp.n_envs = E - per_wg;    // fault injection: the last workgroup of ONE launch is never run
    // (chain.small: four one-wave envs per 256-thread workgroup, env = slot: the dispatcher places a workgroup of the next launch wherever
    // four waves have retired, so the chain needs no deal and no pace keeping to keep the CUs full)
    const auto fn = ch.small ? EVAC_PICK(h, k_rollout_chain_default_config, k_rollout_chain, FS)
                  : h->cu_wide4 ? EVAC_PICK(h, k_rollout_chain_default_config, k_rollout_chain, FW4)
                                : EVAC_PICK(h, k_rollout_chain_default_config, k_rollout_chain, FW);
    const dim3 grid((unsigned)(E / per_wg)), block(ch.small ? FS::kBlock : (h->cu_wide4 ? FW4::kBlock : FW::kBlock));
    hipLaunchKernelGGL(fn, grid, block, 0, S, pp, (int)n_steps, (const float2*)actions, slab_out, final_stats,
                       (const int*)(ch.small ? nullptr : perm + (c & 3) * (size_t)E), (int*)(ch.small ? nullptr : moving + (c & 3) * (size_t)E),
                       deal_loads, deal_perm, ca);
    if (const int lc = check_launch(h, "evac_rollout (chained)"); lc != EVAC_OK) return lc;      // (a launch that never starts must not be waited for)
    ch.wgs += (unsigned long long)grid.x;
    ch.gen = c + 1;
    h->own.pending = true;
    ch.dirty = true;
    return EVAC_OK;
}

// 513..1024 pedestrians, few envs: K workgroups (CUs) per env (evac_team.h).  Workgroup b = j * 8 + xcd carries team (j / K) * 8 + xcd.  All members of a team spin on its
// counter, so the whole grid must be resident at once: checked by team_grid_fits (occupancy x CUs >= workgroups; a grid
// that does not fit runs the one-workgroup-per-env kernels).  A foreign kernel on another stream (the sharded
// env's all-gather) can delay a member, not starve it -- it ends, the member starts, and the bounded waits (~1 s) outlast
// it: tests/test_gpu_team.py keeps a second stream busy throughout.  EVAC_TEAM_COOP=1 launches cooperatively instead
// (the runtime then guarantees co-residency); it costs 3-4 % of the C5 shard's throughput and is not the default.
static int rollout_team(evac_handle* h, int32_t n_steps, const float* actions, float* slab_out, evac_episode_stats_t* final_stats, hipStream_t s_) {
    // every slot of the exchange area starts a launch with tag 31 in every word -- no round's (the previous launch left tagged data)
    if (hipMemsetAsync(h->p.team_rec, 0xff, h->team_xchg_bytes, s_) != hipSuccess) return fail(h, EVAC_ERR_HIP, "evac_rollout: hipMemsetAsync failed");
    int n_steps_ = (int)n_steps;
    const float2* actions_ = (const float2*)actions;
    const int* perm_ = nullptr;
    int* moving_ = nullptr;
    void* argv[] = {(void*)&h->p, (void*)&n_steps_, (void*)&actions_, (void*)&slab_out, (void*)&final_stats, (void*)&perm_, (void*)&moving_,
                    (void*)&perm_, (void*)&moving_};
    const hipError_t le = launch_team_grid(h, team_kernel(h), argv, s_, /*in_chain=*/!capturing(s_), h->team_coop);
    if (le != hipSuccess) return fail(h, EVAC_ERR_HIP, std::string("evac_rollout (team launch): ") + hipGetErrorString(le));
    return EVAC_OK;
}

// Form::Plain (and every other form's diagnostic faces, given actions on Persist, stream capture on Chain / Persist, after settle): ONE
// kernel on the caller's stream
static int rollout_plain(evac_handle* h, int32_t n_steps, const float* actions, float* actions_out, float* slab_out,
                         evac_episode_stats_t* final_stats, int32_t capture_envs, float* capture, const float* noise, hipStream_t stream) {
    if (capture || actions_out || noise) {
        EVAC_DISPATCH(h, k_rollout_diag, stream, h->p, (int)n_steps, (const float2*)actions, (float2*)actions_out, slab_out,
                      final_stats, (int)capture_envs, capture, noise);
    } else if (h->team_k && h->team_bound && team_grid_fits(h)) {
        return rollout_team(h, n_steps, actions, slab_out, final_stats, stream);
    } else if (h->cu_wide || h->cu_wide4) {
        // one-wave envs, batch >= 16 envs per CU (or four-wave envs, >= 4 per CU): CU-wide workgroups, envs dealt to the SIMDs by
        // load when a schedule scratch is bound.  Launch g reads perm[g & 1], leaves its loads in moving[g & 1] and -- workgroup 0,
        // which carries the lightest envs, before it starts stepping (rollout_body) -- deals perm[(g + 1) & 1] for the next launch
        // from the loads launch g - 1 left in moving[(g - 1) & 1]: no launch is spent on sorting, and no buffer is read and
        // written by the same launch.
        using FW = evac::Wave<1, 1024>;
        using FW4 = evac::Wave<4, 1024>;
        const int E = h->p.n_envs;
        // (while the stream is being captured into a hipGraph the host-side generation must not decide what the graph contains:
        // a captured launch runs under the deal at hand, deals nothing and does not advance the generation -- any permutation
        // gives the same results; call evac_reschedule outside the graph to refresh the deal)
        const bool cap = capturing(stream);
        // Long launches (>= 50 steps): the deal as a launch of its own in front of every rollout launch -- 6.5 us next to >= 100,
        // by the loads the previous launch has just left.  Short launches (the driver's 20 steps): the deal of the NEXT launch is
        // made inside this one (rollout_body: workgroup 0, before it starts stepping), by the loads of the launch before.
        const bool in_kernel = n_steps < 50 && E >= (h->cu_wide4 ? 4 : 16);     // (workgroup 0 sorts: it must be a full one)
        if (h->sched && !cap && (h->sched_gen < 0 || !in_kernel)) deal_now(h, stream, h->sched_gen < 0);
        const Deal d = deal_of(h, !cap && in_kernel);
        if (h->sched && h->sched_gen >= 0 && !cap) h->sched_gen += 1;
        const bool four = h->cu_wide4;
        const auto fn = four ? EVAC_PICK(h, k_rollout_default_config, k_rollout, FW4) : EVAC_PICK(h, k_rollout_default_config, k_rollout, FW);
        const int per_block = four ? FW4::kEnvsPerBlock : FW::kEnvsPerBlock;
        hipLaunchKernelGGL(fn, dim3((unsigned)((E + per_block - 1) / per_block)), dim3(four ? FW4::kBlock : FW::kBlock), 0, stream,
                           h->p, (int)n_steps, (const float2*)actions, slab_out, final_stats, d.perm, d.moving, d.loads, d.next);
    } else if (h->default_cfg) {
        EVAC_DISPATCH(h, k_rollout_default_config, stream, h->p, (int)n_steps, (const float2*)actions, slab_out, final_stats,
                      (const int*)nullptr, (int*)nullptr, (const int*)nullptr, (int*)nullptr);
    } else {
        EVAC_DISPATCH(h, k_rollout, stream, h->p, (int)n_steps, (const float2*)actions, slab_out, final_stats, (const int*)nullptr,
                      (int*)nullptr, (const int*)nullptr, (int*)nullptr);
    }
    return check_launch(h, "evac_rollout");
}

int evac_rollout(evac_handle_t h, int32_t n_steps, const float* actions, float* actions_out, float* slab_out,
                 evac_episode_stats_t* final_stats, int32_t capture_envs, float* capture, const float* noise,
                 void* stream) {
    EVAC_REQUIRE_BOUND(h, "evac_rollout");
    if (n_steps < 1) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_rollout: n_steps must be >= 1");
    if (!slab_out) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_rollout: slab_out must be non-NULL");
    if (((uintptr_t)actions | (uintptr_t)actions_out) & 7u)
        return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_rollout: actions buffers must be 8-byte aligned");
    DeviceGuard g(h->device);
    if (capture && (capture_envs < 1 || capture_envs > h->p.n_envs))
        return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_rollout: capture_envs must be in [1, num_envs] when capture is given");
    hipStream_t s_ = (hipStream_t)stream;
    if (!(capture || actions_out || noise)) {        // (the diagnostic faces: one kernel on `stream` in every form)
        if (h->form == Form::Parts) return rollout_parts(h, n_steps, actions, slab_out, final_stats, s_);
        if (h->form == Form::Persist && !actions && (!h->team_k || (h->team_bound && team_grid_fits(h))) && !capturing(s_))
            return rollout_persist(h, n_steps, slab_out, final_stats, s_);
        if (h->form == Form::Chain && h->chain.bound && !capturing(s_)) return rollout_chain(h, n_steps, actions, slab_out, final_stats, s_);
    }
    if (const int rc = settle(h, s_); rc != EVAC_OK) return rc;
    return rollout_plain(h, n_steps, actions, actions_out, slab_out, final_stats, capture_envs, capture, noise, s_);
}

int evac_observe(evac_handle_t h, float* obs_out, void* stream) {
    EVAC_REQUIRE_SETTLED(h, "evac_observe", stream);
    if (!obs_out) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_observe: obs_out is NULL");
    DeviceGuard g(h->device);
    EVAC_DISPATCH(h, k_observe, stream, h->p, obs_out);
    return check_launch(h, "evac_observe");
}

static unsigned state_grid(const evac::Params& p) {
    const size_t n = (size_t)p.n_envs * p.n_ped;
    const size_t b = (n + 255) / 256;
    return (unsigned)(b < 2048 ? (b ? b : 1) : 2048);
}

int evac_get_state(evac_handle_t h, float* pos, float* dir, uint8_t* status, float* agent_pos, float* agent_dir,
                   int32_t* now, void* stream) {
    EVAC_REQUIRE_SETTLED(h, "evac_get_state", stream);
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(evac::k_get_state, dim3(state_grid(h->p)), dim3(256), 0, (hipStream_t)stream, h->p, (float2*)pos,
                       (float2*)dir, status, (float2*)agent_pos, (float2*)agent_dir, now);
    return check_launch(h, "evac_get_state");
}

int evac_set_state(evac_handle_t h, const float* pos, const float* dir, const uint8_t* status, const float* agent_pos,
                   const float* agent_dir, const int32_t* now, void* stream) {
    EVAC_REQUIRE_SETTLED(h, "evac_set_state", stream);
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(evac::k_set_state, dim3(state_grid(h->p)), dim3(256), 0, (hipStream_t)stream, h->p,
                       (const float2*)pos, (const float2*)dir, status, (const float2*)agent_pos,
                       (const float2*)agent_dir, now);
    return check_launch(h, "evac_set_state");
}

int64_t evac_norm_state_doubles(evac_handle_t h) { return h ? 3ll * h->p.obs_dim + 4 : -1; }

int evac_norm_init(evac_handle_t h, double* norm_state, void* stream) {
    if (!h) return EVAC_ERR_INVALID_ARGUMENT;
    if (!norm_state) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_norm_init: norm_state is NULL");
    if (const int rc = settle(h, (hipStream_t)stream); rc != EVAC_OK) return rc;
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(evac::k_norm_init, dim3(1024), dim3(256), 0, (hipStream_t)stream, h->p.n_envs, h->p.obs_dim, norm_state);
    return check_launch(h, "evac_norm_init");
}

static unsigned norm_grid(const evac::Params& p) {
    const size_t n = (size_t)p.n_envs * (p.obs_dim + 1);
    const size_t b = (n + 255) / 256;
    return (unsigned)(b < 4096 ? (b ? b : 1) : 4096);
}

int evac_norm_reset(evac_handle_t h, const uint8_t* mask, float* obs, double* norm_state, float obs_clip, float epsilon,
                    void* stream) {
    if (!h) return EVAC_ERR_INVALID_ARGUMENT;
    if (!obs || !norm_state) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_norm_reset: obs / norm_state is NULL");
    if (const int rc = settle(h, (hipStream_t)stream); rc != EVAC_OK) return rc;
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(evac::k_norm_step, dim3(norm_grid(h->p)), dim3(256), 0, (hipStream_t)stream, h->p.n_envs, h->p.obs_dim,
                       obs, (float*)nullptr, (float*)nullptr, (const uint8_t*)nullptr, (const uint8_t*)nullptr, mask, norm_state,
                       0.0f, obs_clip, 0.0f, epsilon, 1);
    return check_launch(h, "evac_norm_reset");
}

int evac_norm_step(evac_handle_t h, float* obs, float* final_obs, float* reward, const uint8_t* terminated,
                   const uint8_t* truncated, double* norm_state, float gamma, float obs_clip, float reward_clip,
                   float epsilon, void* stream) {
    if (!h) return EVAC_ERR_INVALID_ARGUMENT;
    if (!obs || !reward || !terminated || !truncated || !norm_state)
        return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_norm_step: obs/reward/terminated/truncated/norm_state must be non-NULL");
    if (const int rc = settle(h, (hipStream_t)stream); rc != EVAC_OK) return rc;
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(evac::k_norm_step, dim3(norm_grid(h->p)), dim3(256), 0, (hipStream_t)stream, h->p.n_envs, h->p.obs_dim,
                       obs, final_obs, reward, terminated, truncated, (const uint8_t*)nullptr, norm_state, gamma, obs_clip,
                       reward_clip, epsilon, 0);
    return check_launch(h, "evac_norm_step");
}

// ---- evac_policy_rollout: the trainer's collection loop with the actor-critic inside the launch (evac_policy.h) ----
// ... and evac_policy_rollout_population (n_learners >= 1, strides set): the same checks, the learners' workgroups in one launch.
static int policy_rollout(evac_handle_t h, const char* what, int32_t n_learners, const evac_mlp_policy_strides_t* strides,
                          int32_t n_steps, const evac_mlp_policy_t* policy, float* next_obs, float* next_done, float* obs_out,
                          float* actions_out, float* logprob_out, float* value_out, float* reward_out, float* done_out,
                          float* next_value_out, evac_episode_stats_t* final_stats, double* norm_state, float gamma, float obs_clip,
                          float reward_clip, float epsilon, void* stream, const evac_learner_hyper_t* hypers = nullptr) {
    const std::string w = what;
    std::string why = one_wave_check(h->p);
    if (!why.empty()) return fail(h, EVAC_ERR_UNSUPPORTED, w + why);
    evac::PolicyArgs a = collect_outputs(next_obs, next_done, obs_out, actions_out, logprob_out, value_out, reward_out, done_out,
                                         next_value_out, final_stats);
    evac::PopulationArgs q{};
    why = collect_check(n_steps, a, true, policy);     // (the first refusal in the entry's order of checks)
    if (why.empty()) why = mlp_policy_check(*policy, h->p.obs_dim, a);
    if (why.empty()) why = collect_aligned(a);
    if (why.empty() && strides) why = learner_shares(h->p.n_envs, n_learners, strides, policy->obs_dim, q);
    if (!why.empty()) return fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    evac::LearnerGammas lg{};
    if (hypers)
        for (int s = 0; s < n_learners; ++s) lg.gamma[s] = (float)hypers[s].gamma;
    // (parts / chained / persistent handles: joined first, then ONE kernel on `stream` over the whole batch)
    if (const int st = settle(h, (hipStream_t)stream); st != EVAC_OK) return st;
    DeviceGuard g(h->device);
    const evac::NormArgs na{norm_state, gamma, obs_clip, reward_clip, epsilon};
    const bool grav = h->p.obs_pos == EVAC_POS_GRAV, norm = norm_state != nullptr, def = h->default_cfg;
    const dim3 block(evac::PolicyFamily::kBlock);
    if (strides && hypers && norm) {                   // (without the chain gamma does not enter collection)
        const auto fn = EVAC_PICK_BOOL2(evac::k_collect_sweep, grav, def);
        hipLaunchKernelGGL(fn, dim3((unsigned)(n_learners * q.wgs)), block, 0, (hipStream_t)stream, h->p, (int)n_steps, a, na, q, lg);
        return check_launch(h, what);
    }
    if (strides) {
        const auto fn = EVAC_PICK_BOOL3(evac::k_collect_population, grav, norm, def);
        hipLaunchKernelGGL(fn, dim3((unsigned)(n_learners * q.wgs)), block, 0, (hipStream_t)stream, h->p, (int)n_steps, a, na, q);
        return check_launch(h, what);
    }
    const auto fn = EVAC_PICK_BOOL3(evac::k_policy_rollout, grav, norm, def);
    hipLaunchKernelGGL(fn, dim3((unsigned)policy_wgs(h->p.n_envs)), block, 0, (hipStream_t)stream, h->p, (int)n_steps, a, na);
    return check_launch(h, what);
}

int evac_policy_rollout(evac_handle_t h, int32_t n_steps, const evac_mlp_policy_t* policy, float* next_obs, float* next_done,
                        float* obs_out, float* actions_out, float* logprob_out, float* value_out, float* reward_out, float* done_out,
                        float* next_value_out, evac_episode_stats_t* final_stats, double* norm_state, float gamma, float obs_clip,
                        float reward_clip, float epsilon, void* stream) {
    EVAC_REQUIRE_BOUND(h, "evac_policy_rollout");
    return policy_rollout(h, "evac_policy_rollout", 0, nullptr, n_steps, policy, next_obs, next_done, obs_out, actions_out, logprob_out,
                          value_out, reward_out, done_out, next_value_out, final_stats, norm_state, gamma, obs_clip, reward_clip, epsilon,
                          stream);
}

int evac_policy_rollout_population(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                   const evac_mlp_policy_strides_t* strides, int32_t n_steps, float* next_obs, float* next_done,
                                   float* obs_out, float* actions_out, float* logprob_out, float* value_out, float* reward_out,
                                   float* done_out, float* next_value_out, evac_episode_stats_t* final_stats, double* norm_state,
                                   float gamma, float obs_clip, float reward_clip, float epsilon, void* stream) {
    EVAC_REQUIRE_BOUND(h, "evac_policy_rollout_population");
    if (!strides) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_policy_rollout_population: strides is NULL");
    return policy_rollout(h, "evac_policy_rollout_population", n_learners, strides, n_steps, policy, next_obs, next_done, obs_out,
                          actions_out, logprob_out, value_out, reward_out, done_out, next_value_out, final_stats, norm_state, gamma,
                          obs_clip, reward_clip, epsilon, stream);
}

static_assert(sizeof(evac::LearnerGammas) == EVAC_MAX_LEARNERS * sizeof(float), "evac::LearnerGammas holds EVAC_MAX_LEARNERS values");
static_assert(evac::kHidden == kMlpHidden, "mlp_policy_check and mlp_sizes: the width the policy kernels take");
static_assert(sizeof(evac::Params) + 8 + sizeof(evac::PolicyArgs) + sizeof(evac::NormArgs) + sizeof(evac::PopulationArgs) +
                      sizeof(evac::LearnerGammas) <= 4096, "k_collect_sweep: arguments beyond the kernel-argument segment");

int evac_policy_rollout_sweep(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                              const evac_mlp_policy_strides_t* strides, int32_t n_steps, float* next_obs, float* next_done,
                              float* obs_out, float* actions_out, float* logprob_out, float* value_out, float* reward_out,
                              float* done_out, float* next_value_out, evac_episode_stats_t* final_stats, double* norm_state,
                              float gamma, float obs_clip, float reward_clip, float epsilon, const evac_learner_hyper_t* hypers,
                              void* stream) {
    EVAC_REQUIRE_BOUND(h, "evac_policy_rollout_sweep");
    if (!strides) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_policy_rollout_sweep: strides is NULL");
    if (n_learners < 1 || n_learners > EVAC_MAX_LEARNERS)
        return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_policy_rollout_sweep: n_learners must be in 1.." + std::to_string(EVAC_MAX_LEARNERS));
    if (!learner_hypers_ok(hypers, n_learners))
        return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_policy_rollout_sweep: hypers is NULL or a learner's values are refused "
                                                  "(see evac_learner_hyper_t)");
    return policy_rollout(h, "evac_policy_rollout_sweep", n_learners, strides, n_steps, policy, next_obs, next_done, obs_out,
                          actions_out, logprob_out, value_out, reward_out, done_out, next_value_out, final_stats, norm_state, gamma,
                          obs_clip, reward_clip, epsilon, stream, hypers);
}

// The double a caller wrote for a setting that evac_config_t holds as float32: the shortest decimal that rounds to the float
// (1.3f -> 1.3, as Python prints a float32).  The reference's scripted agent forms its thresholds from the Python floats of its
// config; from the widened float32 values they can come out one float32 apart (0.7 x 1.3, step 0.03: 1.2299999 for 1.23).
static double as_written(float v) {
    char buf[40];
    for (int digits = 1; digits <= 9; ++digits) {
        snprintf(buf, sizeof buf, "%.*g", digits, (double)v);
        if (strtof(buf, nullptr) == v) return strtod(buf, nullptr);
    }
    return (double)v;
}
// The scripted agent's turning points: extent - SWITCH_DISTANCE_TO_LEADER / 2 + step_size in double, rounded once
// (baseline_wacuum_cleaner.py:18-28, constants.py:35), from the settings as the caller wrote them (as_written)
static void vacuum_turning_points(evac_handle_t h, float& thr_x, float& thr_y) {
    const double step = as_written(h->cfg.step_size);
    thr_x = (float)(as_written(h->cfg.width) - 0.2 / 2 + step);
    thr_y = (float)(as_written(h->cfg.height) - 0.2 / 2 + step);
}

// ---- evac_policy_evaluate: whole episodes under a fixed agent, one record per finished episode (evac_evaluate.h) ----
// ... and evac_policy_evaluate_population (strides set, n_learners >= 1): the same checks, the learners' workgroups in one launch.
static int policy_evaluate(evac_handle_t h, const char* what, int32_t n_learners, const evac_mlp_policy_strides_t* strides,
                           int32_t shared_episodes, int32_t agent, const evac_mlp_policy_t* policy, int32_t n_episodes,
                           int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out, const double* norm_state,
                           float obs_clip, float epsilon, void* stream) {
    const std::string w = what;
    const bool scripted = agent == EVAC_AGENT_VACUUM_CLEANER;
    if (agent != EVAC_AGENT_POLICY_MEAN && agent != EVAC_AGENT_POLICY_SAMPLE && !scripted)
        return fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": unknown agent " + std::to_string(agent));
    if (scripted && strides)
        return fail(h, EVAC_ERR_INVALID_ARGUMENT, w + ": the scripted agent has no learners: evac_policy_evaluate runs it");
    evac::EvalArgs ev{};
    evac::PolicyArgs a{};
    evac::PopulationArgs q{};                          // (below: the first refusal in the entry's order of checks)
    std::string why = evaluate_check(agent, n_episodes, max_steps, progress, episodes_out, norm_state, obs_clip, epsilon, ev);
    if (why.empty() && !scripted) why = policy ? mlp_policy_check(*policy, h->p.obs_dim, a) : ": a policy agent needs a policy";
    if (why.empty() && strides) why = learner_shares(h->p.n_envs, n_learners, strides, policy->obs_dim, q);
    if (!why.empty()) return fail(h, EVAC_ERR_INVALID_ARGUMENT, w + why);
    if (!(why = one_wave_check(h->p)).empty()) return fail(h, EVAC_ERR_UNSUPPORTED, w + why);
    // (parts / chained / persistent handles: joined first, then ONE kernel on `stream` over the whole batch)
    if (const int st = settle(h, (hipStream_t)stream); st != EVAC_OK) return st;
    DeviceGuard g(h->device);
    vacuum_turning_points(h, ev.thr_x, ev.thr_y);
    const dim3 grid((unsigned)policy_wgs(h->p.n_envs)), block(evac::PolicyFamily::kBlock);
    const bool grav = h->p.obs_pos == EVAC_POS_GRAV, norm = norm_state != nullptr, def = h->default_cfg;
    if (strides) {
        const auto fn = EVAC_PICK_BOOL3(evac::k_evaluate_population, grav, norm, def);
        hipLaunchKernelGGL(fn, dim3((unsigned)(n_learners * q.wgs)), block, 0, (hipStream_t)stream, h->p, a, ev, q,
                           (int)(shared_episodes != 0));
    } else if (scripted) {
        using evac::k_policy_evaluate_scripted;
        hipLaunchKernelGGL(def ? k_policy_evaluate_scripted<true> : k_policy_evaluate_scripted<false>, grid, block, 0,
                           (hipStream_t)stream, h->p, ev);
    } else {
        const auto fn = EVAC_PICK_BOOL3(evac::k_policy_evaluate, grav, norm, def);
        hipLaunchKernelGGL(fn, grid, block, 0, (hipStream_t)stream, h->p, a, ev);
    }
    return check_launch(h, what);
}

int evac_policy_evaluate(evac_handle_t h, int32_t agent, const evac_mlp_policy_t* policy, int32_t n_episodes, int32_t max_steps,
                         int32_t* progress, evac_episode_stats_t* episodes_out, const double* norm_state, float obs_clip,
                         float epsilon, void* stream) {
    EVAC_REQUIRE_BOUND(h, "evac_policy_evaluate");
    return policy_evaluate(h, "evac_policy_evaluate", 0, nullptr, 0, agent, policy, n_episodes, max_steps, progress, episodes_out,
                           norm_state, obs_clip, epsilon, stream);
}

int evac_policy_evaluate_population(evac_handle_t h, int32_t n_learners, const evac_mlp_policy_t* policy,
                                    const evac_mlp_policy_strides_t* strides, int32_t agent, int32_t shared_episodes,
                                    int32_t n_episodes, int32_t max_steps, int32_t* progress, evac_episode_stats_t* episodes_out,
                                    const double* norm_state, float obs_clip, float epsilon, void* stream) {
    EVAC_REQUIRE_BOUND(h, "evac_policy_evaluate_population");
    if (!strides) return fail(h, EVAC_ERR_INVALID_ARGUMENT, "evac_policy_evaluate_population: strides is NULL");
    return policy_evaluate(h, "evac_policy_evaluate_population", n_learners, strides, shared_episodes, agent, policy, n_episodes,
                           max_steps, progress, episodes_out, norm_state, obs_clip, epsilon, stream);
}

}  // extern "C"

// ---- evac_handle_host.h: the handle for the entries of other translation units (evac_deepsets_api.hip, ...) ----
namespace evac_host {

int handle_begin(evac_handle_t h, const char* what, HandleView* out) {
    if (!h) return EVAC_ERR_INVALID_ARGUMENT;
    if (!h->bound) return fail(h, EVAC_ERR_NOT_BOUND, std::string(what) + ": call evac_bind_state first");
    if (const int ta = team_aborted(h, what); ta != EVAC_OK) return ta;
    *out = HandleView{h->p, h->device, h->default_cfg};
    return EVAC_OK;
}
int handle_settle(evac_handle_t h, hipStream_t stream) { return settle(h, stream); }
int handle_fail(evac_handle_t h, int code, const std::string& msg) { return fail(h, code, msg); }
int handle_check_launch(evac_handle_t h, const char* what) { return check_launch(h, what); }
void handle_turning_points(evac_handle_t h, float* thr_x, float* thr_y) { vacuum_turning_points(h, *thr_x, *thr_y); }

}  // namespace evac_host
