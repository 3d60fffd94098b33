// ssd_policy.hip -- the conv-FC policy network of models/conv_to_fc_net.py:1-51 on the device: its forward pass
// (ssd_policy_forward) and, in ssd_rollout_policy (ssd_capi.hip), its action selection, one launch per step between the step
// launches.  include/ssd.h states the network, the weight layout and the sampling contract; DESIGN.md section 11 the shape.
//
// One workgroup = 16 envs of ONE agent index i, so the weight set (i, or 0 when shared) is uniform across it:
//   1. the 16 observations (u8, 10.8 KB) go to LDS, with the 256-entry normalisation table float32((u8 - 128) / 255);
//   2. conv 3x3x3 -> 6 with ReLU on the VALU: a thread per (env, output position) keeps the 6 filters' sums in registers; the
//      weights are uniform (scalar loads).  The 16 x 1014 outputs stay in LDS in the flatten order (row, col, channel);
//   3. fc1 (16 x 1014) x (1014 x 32) on the matrix cores, v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain per
//      accumulator): wave w takes the 16 output columns w & 1 over half of K (w >> 1), two accumulators each; the two halves
//      are added through LDS.  fc1's weights stream from L2 (130 KB per set, shared by every workgroup of the set);
//   4. fc2, the logits and the value on the VALU (1.3 kMAC per env);
//   5. rollouts: one thread per env picks the action (greedy or the S_POLICY draw) and its log-probability.
// Step 2 is conv_tile and steps 3 and 4 to fc2 are fc_stack, both ssd_policy_device.hpp's (shared with the PPO gradient kernel,
// ssd_policy_grad.hip), as are the heads and the action (heads, pick_actions), shared with the recurrent kernels.  Every sum
// is in a fixed order, so two calls on the same input agree bit for bit.  kModeFeatures stops after fc2 and writes its output
// instead: the trunk of the recurrent policy (ssd_policy_lstm.hip).  kModeMoa runs fc_stack once per FC stack of the MOA
// policy, with tanh for ReLU, on the same conv output and writes both outputs (ssd_policy_moa.hip).  The kernel's text is in
// ssd_policy_trunk.hpp, which ssd_policy_seq.hip instantiates for a fourth mode of its own.  This file also holds the
// argument checks every policy entry point shares (check_policy_net, check_state_out, select_device), those of the six
// loss-and-gradient entry points (check_policy_grad) and the BPTT calls' per-window helpers (declared in ssd_policy.hpp).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string>

#include "../../include/ssd.h"
#include "ssd_policy_device.hpp"
#include "ssd_policy_trunk.hpp"

namespace {

thread_local std::string g_policy_error;

int fail(const char *msg) {
    g_policy_error = msg;
    return SSD_E_INVALID;
}

}  // namespace

namespace ssd {

hipError_t launch_policy(const PolicyArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + kTile - 1) / kTile), (unsigned)a.N), block(kThreads);
    hipLaunchKernelGGL(ssd_policy_kernel<kModeHeads>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

hipError_t launch_policy_features(const PolicyArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + kTile - 1) / kTile), (unsigned)a.N), block(kThreads);
    hipLaunchKernelGGL(ssd_policy_kernel<kModeFeatures>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

hipError_t launch_policy_moa_features(const PolicyArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + kTile - 1) / kTile), (unsigned)a.N), block(kThreads);
    hipLaunchKernelGGL(ssd_policy_kernel<kModeMoa>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

int policy_fail(const char *msg) { return fail(msg); }

const char *check_policy_net(PolicyNet net, const float *weights, int32_t num_sets, int32_t num_agents, int32_t num_actions,
                             int32_t cell_size, const float *moa_scratch) {
    if (reinterpret_cast<uintptr_t>(weights) & 3u) return "weights must be 4-byte aligned";
    if (net == kNetMoa && (reinterpret_cast<uintptr_t>(moa_scratch) & 3u)) return "scratch must be 4-byte aligned";
    if (net != kNetConvFc && cell_size != 64 && cell_size != 128 && cell_size != 256) return "cell_size must be 64, 128 or 256";
    if (net == kNetMoa) {
        if (num_agents < 2 || num_agents > SSD_MOA_MAX_AGENTS) return "the MOA policy needs 2..16 agents";
    } else if (num_agents < 1 || num_agents > 64) {
        return "num_agents must be 1..64";
    }
    if (num_sets != 1 && num_sets != num_agents) return "num_sets must be 1 or num_agents";
    if (num_actions < 1 || num_actions > SSD_POL_MAX_ACTIONS) return "num_actions must be 1..15";
    return nullptr;
}

const char *check_policy_grad(const GradCall &c) {
    const bool bptt = c.net != kNetConvFc;
    if (!c.weights) return "weights are required";
    if (const char *why = check_policy_net(c.net, c.weights, c.num_sets, c.num_agents, c.num_actions, c.cell_size)) return why;
    if (c.n_steps < 1 || c.num_envs < 1) return "n_steps and num_envs must be >= 1";
    if (bptt && c.seq_len < 1) return "seq_len must be >= 1";
    if ((int64_t)c.n_steps * c.num_envs * c.num_agents > INT32_MAX - 16)      // (row + 15 is an int)
        return "n_steps * num_envs * num_agents must be at most 2^31 - 17";
    if (!c.obs && !(c.obs_first && c.n_steps == 1)) return "obs is required (it may be null only with obs_first and n_steps 1)";
    if (bptt && !c.state) return "state is required";
    if (bptt && (reinterpret_cast<uintptr_t>(c.state) & 3u)) return "state must be 4-byte aligned";
    if (c.net == kNetMoa && !c.prev_actions) return "prev_actions is required";
    if (c.net == kNetMoa && (reinterpret_cast<uintptr_t>(c.prev_actions) & 3u)) return "prev_actions must be 4-byte aligned";
    if (c.ac && (!c.actions || !c.advantages || !c.value_targets)) return "actions, advantages and value_targets are required";
    if (!c.ac && (!c.actions || !c.logp_old || !c.advantages || !c.value_targets || !c.vf_preds))
        return "actions, logp_old, advantages, value_targets and vf_preds are required";
    if (!c.scratch || !c.grads || !c.stats) return "scratch, grads and stats are required";
    if ((reinterpret_cast<uintptr_t>(c.scratch) & 7u) || (reinterpret_cast<uintptr_t>(c.stats) & 7u))
        return "scratch and stats must be 8-byte aligned";
    if (reinterpret_cast<uintptr_t>(c.grads) & 3u) return "grads must be 4-byte aligned";
    if (!(isfinite(c.clip_param) && isfinite(c.vf_clip_param) && isfinite(c.vf_loss_coeff) && isfinite(c.entropy_coeff) &&
          isfinite(c.kl_coeff)))
        return "the hyper-parameters must be finite";
    if (c.clip_param < 0.0 || c.vf_clip_param < 0.0) return "clip_param and vf_clip_param must be >= 0";
    if (c.net == kNetMoa && (!isfinite(c.moa_weight) || c.moa_weight < 0.0)) return "moa_weight must be finite and >= 0";
    if ((c.kl_coeff != 0.0) != (c.behaviour_logits != nullptr)) return "behaviour_logits must be given if and only if kl_coeff is not 0";
    if (c.flags) return "flags must be 0";
    return nullptr;
}

GradWindow grad_window(const uint8_t *obs_first, const uint8_t *obs, int k0, size_t step_rows) {
    const size_t obs_step = step_rows * 675;
    if (!obs_first) return {nullptr, obs + (size_t)k0 * obs_step};            // row k reads obs[k]: `rest` from step 0
    if (k0 == 0) return {obs_first, obs};
    return {obs + (size_t)(k0 - 1) * obs_step, obs + (size_t)k0 * obs_step};
}

hipError_t launch_window_features(PolicyArgs f, bool moa, const GradWindow &o, int steps, int num_envs, size_t step_floats, void *stream) {
    const auto launch = moa ? launch_policy_moa_features : launch_policy_features;
    if (!o.first) {
        f.B = steps * num_envs; f.obs = o.rest;
        return launch(f, stream);
    }
    f.B = num_envs; f.obs = o.first;
    if (const hipError_t e = launch(f, stream)) return e;
    if (steps == 1) return hipSuccess;
    f.B = (steps - 1) * num_envs; f.obs = o.rest; f.feat += step_floats;
    return launch(f, stream);
}

PpoGradArgs window_trunk_args(const PolicyArgs &f, const GradWindow &o, int trunk_floats, int groups, int set_rows, int step_rows,
                              float *part_trunk, const float *dx, int accumulate) {
    PpoGradArgs tg{};
    tg.w = f.w; tg.P = f.P; tg.A = f.A; tg.N = f.N; tg.set_floats = trunk_floats; tg.w_pitch = f.set_floats; tg.G = groups;
    tg.set_rows = set_rows; tg.step_rows = step_rows;
    tg.obs_first = o.first; tg.obs = o.rest; tg.scratch = part_trunk; tg.dx = dx; tg.accumulate = accumulate;
    return tg;
}

const char *check_state_out(const float *state_in, const float *state_out, size_t bytes) {
    if (!state_out || state_out == state_in) return nullptr;
    const char *p = reinterpret_cast<const char *>(state_in), *q = reinterpret_cast<const char *>(state_out);
    return q < p + bytes && p < q + bytes ? "state_out must be state_in or not overlap it" : nullptr;
}

hipError_t select_device(int device_id) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device_id) return hipSuccess;
    return hipSetDevice(device_id);
}

int policy_use_device(int device_id) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count) return fail("no such HIP device");
    if (select_device(device_id) != hipSuccess) { g_policy_error = "hipSetDevice failed"; return SSD_E_DEVICE; }
    return SSD_OK;
}

int policy_launched(hipError_t e) {
    if (e == hipSuccess) return SSD_OK;
    g_policy_error = std::string("policy launch: ") + hipGetErrorString(e);
    return SSD_E_DEVICE;
}

}  // namespace ssd

extern "C" {

const char *ssd_policy_last_error(void) { return g_policy_error.c_str(); }

int ssd_policy_forward(const float *weights, int32_t num_sets, int32_t num_actions, const uint8_t *obs, int32_t batch,
                       int32_t num_agents, float *logits, float *value, int32_t device_id, uint32_t flags, void *stream) {
    if (!weights || !obs) return fail("weights and obs are required");
    if (const char *why = ssd::check_policy_net(ssd::kNetConvFc, weights, num_sets, num_agents, num_actions)) return fail(why);
    if (batch < 1) return fail("batch must be >= 1");
    if (flags) return fail("flags must be 0");
    if (const int rc = ssd::policy_use_device(device_id)) return rc;
    ssd::PolicyArgs a{};
    a.w = weights; a.P = num_sets; a.A = num_actions; a.B = batch; a.N = num_agents; a.set_floats = SSD_POL_SET_FLOATS(num_actions);
    a.obs = obs; a.logits = logits; a.value = value;
    return ssd::policy_launched(ssd::launch_policy(a, stream));
}

}  // extern "C"
