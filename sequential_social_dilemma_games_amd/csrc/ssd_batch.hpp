// csrc/ssd_batch.hpp -- the host scaffold of the stateless calls on the rollout rings (host side, header only): the error slot,
// the ring rules, the device rule and the (bonus, done) choice of a kernel instance.  Used by ssd_gae.hip (ssd_advantages),
// ssd_vtrace.hip (ssd_vtrace) and ssd_moments.hip (ssd_standardize, ssd_explained_variance).  No device code: the kernels of
// those files share nothing (DESIGN.md section 20 has why).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/ssd.h"

namespace ssd {

// A family's last error text.  Each file keeps one thread_local instance, which its own *_last_error export reads.
struct BatchError {
    std::string text;
    int invalid(const char *msg) { text = msg; return SSD_E_INVALID; }
    int device(const char *msg) { text = msg; return SSD_E_DEVICE; }
    // after the launches of call `what`: SSD_OK, or SSD_E_DEVICE with "<what> launch: <HIP's words>"
    int launched(const char *what) {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return SSD_OK;
        text = std::string(what) + " launch: " + hipGetErrorString(e);
        return SSD_E_DEVICE;
    }
    const char *c_str() const { return text.c_str(); }
};

// The rules every call's [ring, lanes] rows follow, in the order callers have always seen them reported: null = fine.
inline const char *check_ring(int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps) {
    if (lanes < 1) return "lanes must be >= 1";
    if (ring < 1) return "ring must be >= 1";
    if (n_steps < 1) return "n_steps must be >= 1";
    if (n_steps > ring) return "n_steps > ring: a call reads each step's slot once";
    if (step0 < 0) return "step0 must be >= 0";
    return nullptr;
}

// Makes device_id the calling thread's device unless it is already: SSD_OK, or the code with err's text set.
inline int use_device(BatchError &err, int32_t device_id) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return err.device("no HIP device available: this call has no CPU path");
    if (device_id < 0 || device_id >= count) return err.invalid("device_id out of range");
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != device_id) {
        if (hipSetDevice(device_id) != hipSuccess) return err.device("hipSetDevice failed");
    }
    return SSD_OK;
}

// f(bonus, done) with the two run-time choices as std::bool_constant types, for a kernel's template arguments
template <class F>
void with_bonus_done(bool bonus, bool done, F &&f) {
    if (bonus && done) f(std::true_type{}, std::true_type{});
    else if (bonus) f(std::true_type{}, std::false_type{});
    else if (done) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}

}  // namespace ssd
