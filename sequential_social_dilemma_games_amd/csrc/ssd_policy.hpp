// csrc/ssd_policy.hpp -- the policy kernel's argument block, shared by ssd_policy.hip (kernel, ssd_policy_forward) and
// ssd_capi.hip (ssd_rollout_policy, which interleaves it with the step kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ssd {

struct PolicyArgs {
    const float *w;                // P weight sets of set_floats floats each (include/ssd.h, SSD_POL_*)
    int32_t P, A, B, N, set_floats;
    const uint8_t *obs;            // u8 [B][N][15][15][3]
    float *logits;                 // [B][N][A] or null
    float *value;                  // [B][N] or null
    // action selection (rollouts): null actions = forward pass only
    int32_t *actions;              // [B][N]
    float *logp;                   // [B][N] or null
    const uint4 *hdr;              // [B] the engine's per-env header {key, t, episode, ...}: (episode, t) of the state acted in
    uint32_t seed_lo, seed_hi, env_base;
    int32_t greedy;
};

// hipLaunchKernel of the policy kernel on `stream` (arguments already checked); returns the launch's error code.
hipError_t launch_policy(const PolicyArgs &a, void *stream);

}  // namespace ssd
