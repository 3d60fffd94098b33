// csrc/ssd_env.hpp -- the handle behind the C ABI, and the few helpers that ssd_capi.hip (lifecycle, per-call steps, state, render,
// policy rollouts) and ssd_rollout.hip (ssd_rollout_random / ssd_rollout_actions and their dispatch paths) share.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/ssd.h"
#include "ssd_internal.hpp"

struct ChainWorker;               // ssd_rollout.hip: defined there, and deleted there
struct AqlState;
struct __attribute__((visibility("hidden"))) RolloutDelete { void operator()(ChainWorker *w) const; void operator()(AqlState *a) const; };

struct ssd_env {
    int game = 0, H = 0, W = 0, WP = 0, S = 0, E = 0, N = 0, view_len = 7, V = 15, beam_len = 5;
    int device = 0, keep_beams = 0, potential_waste = 0;
    uint64_t seed = 0;
    uint32_t env_base = 0;
    ssd::Params p{};                  // persistent part of the kernel parameters
    std::vector<void *> allocs;
    // staging for SSD_HOST_PTRS
    int32_t *st_actions = nullptr, *st_rew = nullptr, *st_actions_out = nullptr;
    float *st_obs_f32 = nullptr;
    // small handles (the dict API's single env): host-pinned, device-mapped staging -- the kernel reads / writes it
    // directly, so a host-pointer call is one launch + one synchronise instead of five copies
    bool st_mapped = false;
    uint8_t *st_host = nullptr;      // host view of the mapped block; the st_* pointers above are its device view
    std::vector<void *> host_allocs;
    uint8_t *st_order = nullptr, *st_obs = nullptr, *st_done = nullptr, *st_mask = nullptr, *st_rgb = nullptr;
    size_t st_rgb_frames = 0;                          // frames st_rgb holds
    // ssd_rollout_random: extra chains (streams + fork / join events), created on first use
    std::vector<hipStream_t> chain_streams;
    std::vector<hipEvent_t> chain_events;
    hipEvent_t fork_event = nullptr;
    int rollout_chains = 0;           // 0 = automatic
    std::vector<std::unique_ptr<ChainWorker, RolloutDelete>> workers;   // workers[c - 1] enqueues chain c
    std::unique_ptr<AqlState, RolloutDelete> aql;                      // the library's own dispatch path (ssd_aql.hip), set up on first use
    // The stream the last device-pointer call enqueued on.  A host-pointer call (which runs on the stream it is given, usually
    // the NULL stream, and returns finished results) first waits for that stream when it is another one: a caller that
    // mixes the two styles -- tensors on a non-blocking side stream, then a *_host call -- gets program order.
    hipStream_t last_stream = nullptr;
    bool last_stream_set = false;
    int last_path = 0;                                   // SSD_PATH_* of the last rollout call
    std::string err;
};

#define SSD_HIP(env, call)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (env)->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
            return SSD_E_DEVICE;                                                                \
        }                                                                                       \
    } while (0)

static inline size_t obs_bytes(const ssd_env *env, bool f32 = false) { return (size_t)env->E * env->N * env->V * env->V * 3 * (f32 ? 4 : 1); }

// the game's Discrete(n): harvest.py:44, cleanup.py:70
static inline int game_actions(const ssd_env *env) { return env->game == SSD_GAME_HARVEST ? 8 : 9; }

// ssd_rollout.hip, for ssd_destroy and ssd_synchronize
__attribute__((visibility("hidden"))) void stop_workers(ssd_env *env);
__attribute__((visibility("hidden"))) void aql_teardown(ssd_env *env);
__attribute__((visibility("hidden"))) int after_timeout(ssd_env *env);
