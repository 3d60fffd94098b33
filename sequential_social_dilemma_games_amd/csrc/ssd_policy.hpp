// csrc/ssd_policy.hpp -- the policy kernels' argument blocks, their launchers and the argument checks every policy entry point
// shares (host-readable; the device pieces the kernels share are in ssd_policy_device.hpp).  Used by ssd_policy.hip (trunk kernel,
// ssd_policy_forward), ssd_policy_lstm.hip, ssd_policy_moa.hip, ssd_ws_policy.hip, ssd_capi.hip (the rollouts, which interleave
// the launches with the step kernel), ssd_policy_seq.hip (the sequence forwards) and the three gradient files (check_policy_grad and the BPTT calls' window helpers).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"

namespace ssd {

struct PolicyArgs {
    const float *w;                // P weight sets of set_floats floats each (include/ssd.h, SSD_POL_* / SSD_LSTM_*)
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
    float *feat;                   // launch_policy_features only: fc2's output [B][N][32] (the heads are not computed);
                                   // launch_policy_moa_features: both FC stacks' outputs [B][N][2][32]
};

struct LstmArgs {
    const float *w;                // P weight sets of set_floats floats each (SSD_LSTM_SET_FLOATS(C, A))
    int32_t P, A, B, N, C, set_floats;
    const float *feat;             // [B][N][32] the trunk's output
    const float *state_in;         // [B][N][2][C]
    float *state_out;              // [B][N][2][C], null, or state_in itself
    float *state_used;             // [B][N][2][C] the state the step used (after the start rule), or null
    const uint8_t *starts;         // [B][N] start rows (the forward), or null
    const uint4 *hdr;              // [B] start where t == 0 (rollouts), or null; also (episode, t) of the action draw
    float *logits;                 // [B][N][A] or null
    float *value;                  // [B][N] or null
    int32_t *actions;              // [B][N] or null (no action selection)
    float *logp;                   // [B][N] or null
    uint32_t seed_lo, seed_hi, env_base;
    int32_t greedy;
};

// hipLaunchKernel of the policy kernel on `stream` (arguments already checked); returns the launch's error code.
hipError_t launch_policy(const PolicyArgs &a, void *stream);
// The same kernel up to fc2: writes a.feat instead of the heads (logits, value, actions unused).
hipError_t launch_policy_features(const PolicyArgs &a, void *stream);
// The same kernel with the MOA policy's two tanh FC stacks (SSD_MOA_FC1_W(s)): writes a.feat [B][N][2][32].
hipError_t launch_policy_moa_features(const PolicyArgs &a, void *stream);
// The recurrent cell and heads (ssd_policy_lstm.hip); a.C in {64, 128, 256}.
hipError_t launch_policy_lstm(const LstmArgs &a, void *stream);
struct MoaArgs {
    const float *w;                // P weight sets of set_floats floats each (SSD_MOA_SET_FLOATS(C, A, N))
    int32_t P, A, B, N, C, set_floats;
    const float *feat;             // [B][N][2][32] the FC stacks' outputs
    const float *state_in;         // [B][N][4][C] (h1, c1, h2, c2)
    float *state_out;              // [B][N][4][C], null, or state_in itself
    float *state_used;             // [B][N][4][C] the state the step used (after the start rule), or null
    const uint8_t *starts;         // [B][N] start rows (the forward), or null
    const uint4 *hdr;              // [B] start where t == 0 (rollouts), or null; also (episode, t) of the action draw
    // actions cell (launch_policy_moa_actions)
    float *logits;                 // [B][N][A] or null
    float *logits_scratch;         // [B][N][16] this step's logits for the MOA cell, or null
    float *value;                  // [B][N] or null
    int32_t *actions;              // [B][N] or null (no action selection)
    int32_t *actions_copy;         // [B][N] a second copy of the actions (the next step's previous joint action), or null
    float *logp;                   // [B][N] or null
    uint32_t seed_lo, seed_hi, env_base;
    int32_t greedy;
    // MOA cell (launch_policy_moa_cell)
    const int32_t *prev;           // [B][N] the previous joint action by agent index (read where the row does not start)
    int32_t *prev_used;            // [B][N] what the MOA read (zero at a start), or null
    const float *pi_logits;        // [B][N][pi_stride] this step's action logits (for the influence), or null
    int32_t pi_stride;
    const int32_t *taken;          // [B][N] this step's actions (for the influence), or null: no influence
    float *moa_logits;             // [B][N][N-1][A] or null
    float *cf_logits;              // [B][N][A][N-1][A] or null
    float *influence;              // [B][N] or null
    float clip;
};

// The MOA policy's actions cell: the Keras LSTM on stack 0, the heads and the action (ssd_policy_moa.hip).
hipError_t launch_policy_moa_actions(const MoaArgs &a, void *stream);
// The MOA cell: gates, the A counterfactual updates and predictions, moa_logits and the influence (ssd_policy_moa.hip).
hipError_t launch_policy_moa_cell(const MoaArgs &a, void *stream);
// The PPO gradient kernel's arguments (ssd_policy_grad.hip).
struct PpoGradArgs {
    const float *w;                // P weight sets
    int32_t P, A, N, set_floats;
    int32_t G;                     // workgroups per set
    int32_t set_rows;              // rows of one set
    int32_t step_rows;             // E * N: rows of one step
    const uint8_t *obs_first;      // u8 [E][N][675] or null
    const uint8_t *obs;            // u8 [K][E][N][675]
    const int32_t *actions;        // [K][E][N]
    const float *logp_old, *adv, *vt, *vf_pred;   // [K][E][N]
    const float *beh;              // [K][E][N][A] or null
    float clip, vf_clip, vf_coeff, ent_coeff, kl_coeff;
    float *scratch;                // [P][G][set_floats + SSD_PPO_STAT_FLOATS]
    float *grads;                  // [P][set_floats]
    double *stats;                 // [P][5]
    // launch_ppo_trunk_grad only
    const float *dx;               // [K][E][N][32] d loss / d fc2's output (after its ReLU), not yet divided by the rows
    int32_t accumulate;            // add the partial sets to what scratch holds
    int32_t w_pitch;               // floats between the weight sets of w (set_floats is the partial sets' pitch alone)
    // launch_ppo_moa_stack_grad only
    int32_t stack;                 // 0: the actions stack, 1: the MOA stack; dx is [K][E][N][2][32], the stack's half is read
};
// The same kernel as the trunk's backward alone (the recurrent policy's, ssd_policy_lstm_grad.hip): set_floats floats of a
// partial set are the trunk's (SSD_POL_CONV_W .. SSD_POL_FC2_B); a (G, P) grid whatever set_rows is.
hipError_t launch_ppo_trunk_grad(const PpoGradArgs &a, void *stream);
// That backward for one tanh FC stack of the MOA policy (ssd_policy_moa_grad.hip): a partial set is the MOA layout's floats
// below SSD_MOA_LSTM_W (set_floats); stack 1's launch adds its conv sums to those stack 0's launch left in the same scratch.
hipError_t launch_ppo_moa_stack_grad(const PpoGradArgs &a, void *stream);
// The calling thread's ssd_policy_last_error text; returns SSD_E_INVALID.
int policy_fail(const char *msg);

// The rules every policy net's arguments follow, in the order callers have always seen them reported: null = fine, else the
// error text.  kNetConvFc has no cell (cell_size is not looked at); kNetMoa also has a float scratch and 2..16 agents.  The
// rollouts pass the engine's own agent and action counts, which always pass.
enum PolicyNet { kNetConvFc, kNetLstm, kNetMoa };
const char *check_policy_net(PolicyNet net, const float *weights, int32_t num_sets, int32_t num_agents, int32_t num_actions,
                             int32_t cell_size = 0, const float *moa_scratch = nullptr);
// What the six loss-and-gradient entry points (ssd_policy_{,lstm_,moa_}{ppo,ac}_grad) check alike, in the order callers have
// always seen it reported: null = fine, else the error text.  kNetConvFc has no seq_len and no state, only kNetMoa has
// prev_actions and moa_weight; the A3C calls (ac) pass no logp_old, vf_preds or behaviour_logits and zeros for the
// hyper-parameters they do not have, which pass.
struct GradCall {
    PolicyNet net;
    bool ac;
    const float *weights;
    int32_t num_sets, num_actions, cell_size, seq_len;
    const uint8_t *obs_first, *obs;
    const float *state;
    const int32_t *prev_actions, *actions;
    const float *logp_old, *advantages, *value_targets, *vf_preds, *behaviour_logits;
    int32_t n_steps, num_envs, num_agents;
    double clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff, moa_weight;
    const float *scratch, *grads;
    const double *stats;
    uint32_t flags;
};
const char *check_policy_grad(const GradCall &c);

// The BPTT calls' window of `steps` steps from step k0 of the fragment.  The observations its rows acted on (the shift of
// include/ssd.h): `first` [E][N][675] for its step 0 and `rest` from step 1, or first null and `rest` from step 0.
struct GradWindow {
    const uint8_t *first, *rest;
};
GradWindow grad_window(const uint8_t *obs_first, const uint8_t *obs, int k0, size_t step_rows);
// The features of the window's rows to f.feat, step_floats floats a step (f: w, P, A, N, set_floats, feat given): one launch of
// launch_policy_features (moa: launch_policy_moa_features), two where `first` splits the rows.
hipError_t launch_window_features(PolicyArgs f, bool moa, const GradWindow &o, int steps, int num_envs, size_t step_floats, void *stream);
// The trunk's backward of the window from dx (launch_ppo_trunk_grad, launch_ppo_moa_stack_grad): its arguments, with f as above
// and trunk_floats the floats of a partial set.
PpoGradArgs window_trunk_args(const PolicyArgs &f, const GradWindow &o, int trunk_floats, int groups, int set_rows, int step_rows,
                              float *part_trunk, const float *dx, int accumulate);

// p is not a multiple of n bytes, n a power of two (a null pointer is aligned)
inline bool misaligned(const void *p, unsigned n = 4) { return (reinterpret_cast<uintptr_t>(p) & (n - 1u)) != 0; }
// state_out may be state_in itself (in place) or a buffer that does not overlap its `bytes` bytes: null = fine
const char *check_state_out(const float *state_in, const float *state_out, size_t bytes);
// Makes device_id the calling thread's device unless it is already: hipSuccess, or hipSetDevice's error.
hipError_t select_device(int device_id);
// The forward calls' device rule (device_id must exist) and their launch result: SSD_OK, or the code with the error text set.
int policy_use_device(int device_id);
int policy_launched(hipError_t e);

}  // namespace ssd
