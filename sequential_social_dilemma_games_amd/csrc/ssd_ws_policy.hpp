// csrc/ssd_ws_policy.hpp -- what the Watershed policy rollouts (ssd_ws_policy.hip) need of a Watershed handle, whose layout stays
// private to ssd_watershed.hip: the per-env counters the policy kernel reads (never writes) and the handle's constants.
#pragma once
#include <stdint.h>

#include "../../include/ssd.h"

namespace ssd {

struct WsPolicyView {
    const uint8_t *phase;          // [E] current_phase, 0 = never reset
    const int32_t *round;          // [E] internal_step
    const uint32_t *episode;       // [E] PRNG coordinate
    int32_t E, variant, device;
    uint32_t seed_lo, seed_hi, env_base;
};

// Fills *v from the handle (host code only; ssd_watershed.hip).
void ws_policy_view(const ssd_ws_env *env, WsPolicyView *v);
// Sets the handle's ssd_ws_last_error text; returns SSD_E_INVALID.
int ws_fail_invalid(ssd_ws_env *env, const char *msg);
// Sets the handle's error text from a HIP error; returns SSD_E_DEVICE.
int ws_fail_device(ssd_ws_env *env, const char *what, int hip_error);

}  // namespace ssd
