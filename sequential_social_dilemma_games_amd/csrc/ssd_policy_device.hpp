// csrc/ssd_policy_device.hpp -- the device pieces the policy kernels are built from, each defined once: the LSTM gate GEMM, the
// two cell rules and the cell update, the start rule and the loader of the h rows, the heads, and the action draw.  Used by
// ssd_policy.hip (conv-FC), ssd_policy_lstm.hip, ssd_policy_moa.hip and ssd_ws_policy.hip; the argument blocks stay in
// ssd_policy.hpp, which host code reads too.  Every sum below is one chain in a fixed order, so a change here changes the
// bits of every kernel that uses the piece, and the tests that compare kernels and paths bit for bit see it.
//
// v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain per accumulator): lane l holds A[l & 15][k = l >> 4] and
// B[k = l >> 4][l & 15]; D: col l & 15, row 4 (l >> 4) + r.
#pragma once
#include <stddef.h>

#include "ssd_policy.hpp"

namespace ssd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ---------------------------------------------------------------------------------------------------------------- the cell
// The gates of the 16 MT rows of s_in (pitch Pitch: the input columns, then the C columns of h; K of them in all) for a
// workgroup of 4 C threads: acc[g][s] = z[16 s .., g C + 16 wave + l15] without the bias, A[m][k] = s_in row m,
// B[k][n] = w[k][g C + 16 wave + n].  Wave w takes cells 16w .. 16w + 15 of all four gates, so lane (l15, l4) ends up with the
// four gates of cell 16 wave + l15 for rows 16 s + 4 l4 + r, and each weight load feeds MT MFMAs.
template <int C, int K, int Pitch, int MT>
__device__ __forceinline__ void lstm_gates(const float *s_in, const float *__restrict__ w, int tid, f32x4 (&acc)[4][MT]) {
    static_assert(K % 4 == 0 && Pitch % 64 == 4, "tile");    // pitch = 4 (mod 64): lane (l15, l4) of an A load hits bank 4 l15 + l4
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const float *a_row = s_in + l15 * Pitch + l4;
    const float *wg = w + (size_t)l4 * 4 * C + 16 * wave + l15;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int s = 0; s < MT; ++s) acc[g][s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int kk = 0; kk < K / 4; ++kk) {
        const float *wk = wg + (size_t)kk * 16 * C;
        float bv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) bv[g] = wk[g * C];
        float av[MT];
#pragma unroll
        for (int s = 0; s < MT; ++s) av[s] = a_row[s * 16 * Pitch + 4 * kk];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int s = 0; s < MT; ++s) acc[g][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[g], acc[g][s], 0, 0, 0);
    }
}

// The two cell rules: the order of the four gate columns z0..z3 (bias added), and where c and h sit in a state's two rows.
struct RllibCell {                  // RLlib 0.7.6: gates i, j, f, o with forget bias 1; a state is (c, h)
    static constexpr int kRowC = 0, kRowH = 1;
    static __device__ __forceinline__ void update(float zi, float zj, float zf, float zo, float c, float *c2, float *h2) {
        *c2 = sigmoidf_(zf + 1.f) * c + sigmoidf_(zi) * tanhf(zj);
        *h2 = sigmoidf_(zo) * tanhf(*c2);
    }
};
struct KerasCell {                  // Keras: gates i, f, c~, o, no forget bias; a state is (h, c)
    static constexpr int kRowH = 0, kRowC = 1;
    static __device__ __forceinline__ void update(float zi, float zf, float zc, float zo, float c, float *c2, float *h2) {
        *c2 = sigmoidf_(zf) * c + sigmoidf_(zi) * tanhf(zc);
        *h2 = sigmoidf_(zo) * tanhf(*c2);
    }
};

// start flag of row `row` of env b: starts[row] in the forward, t == 0 in rollouts; envs past B count as starting (nothing read)
__device__ __forceinline__ int row_start(const uint8_t *starts, const uint4 *hdr, int b, size_t row, int B) {
    if (b >= B) return 1;
    return starts ? starts[row] != 0 : (hdr ? hdr[b].y == 0u : 0);
}

// Where tile row m keeps its state (two rows of C floats, Cell's order): the float offset, and whether the row is the caller's
// to touch at all (a row past the batch, or of another agent id, is not).
struct StateRow {
    bool mine;
    size_t at;
};

// h of the kM tile rows to s_h (pitch floats apart; zero where s_start[m], whose state is never read), and the state each row
// used to state_used where that is given.  in(m), used(m): row m's StateRow in state_in and state_used; in(m).mine is not
// looked at (a row that is not the caller's starts).
template <class Cell, int C, int kM, class In, class Used>
__device__ __forceinline__ void load_h(float *s_h, int pitch, const int *s_start, const float *state_in, float *state_used, int tid,
                                       In in, Used used) {
    for (int q = tid; q < kM * C; q += 4 * C) {
        const int m = q / C, u = q - m * C;
        const size_t r = in(m).at;
        const StateRow ru = used(m);
        const float h = s_start[m] ? 0.f : state_in[r + Cell::kRowH * C + u];
        s_h[m * pitch + u] = h;
        if (state_used && ru.mine) {
            state_used[ru.at + Cell::kRowH * C + u] = h;
            state_used[ru.at + Cell::kRowC * C + u] = s_start[m] ? 0.f : state_in[r + Cell::kRowC * C + u];
        }
    }
}

// The cell update of the rows lstm_gates left in acc: lane (l15, l4) holds the four gates of cell u = 16 wave + l15 for rows
// m = 16 s + 4 l4 + r.  bias: [4][C].  h' goes to s_h (as load_h), c' and h' to state_out where that is given (state_in itself:
// in place).  row(m): row m's StateRow; nothing of a row that is not `mine` is touched.
template <class Cell, int C, int MT, class Row>
__device__ __forceinline__ void cell_update(const f32x4 (&acc)[4][MT], const float *__restrict__ bias, const int *s_start,
                                            const float *state_in, float *state_out, float *s_h, int pitch, int tid, Row row) {
    const int lane = tid & 63, u = 16 * (tid >> 6) + (lane & 15), l4 = lane >> 4;
    const float b0 = bias[u], b1 = bias[C + u], b2 = bias[2 * C + u], b3 = bias[3 * C + u];
#pragma unroll
    for (int s = 0; s < MT; ++s) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 16 * s + 4 * l4 + r;
            const StateRow st = row(m);
            if (!st.mine) continue;
            const float c = s_start[m] ? 0.f : state_in[st.at + Cell::kRowC * C + u];
            float c2, h2;
            Cell::update(acc[0][s][r] + b0, acc[1][s][r] + b1, acc[2][s][r] + b2, acc[3][s][r] + b3, c, &c2, &h2);
            s_h[m * pitch + u] = h2;
            if (state_out) {
                state_out[st.at + Cell::kRowC * C + u] = c2;
                state_out[st.at + Cell::kRowH * C + u] = h2;
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- the heads
// Output j of one row from its K hidden values hr: column j of w_out [K][n_out] plus b_out[j] for j < n_out, the value
// (w_value [K], b_value) for j == n_out.  One fmaf chain in k order.
template <int K>
__device__ __forceinline__ float head(const float *hr, const float *__restrict__ w_out, const float *__restrict__ w_value,
                                      const float *__restrict__ b_out, const float *__restrict__ b_value, int n_out, int j) {
    const float *hw = j < n_out ? w_out + j : w_value;
    const int stride = j < n_out ? n_out : 1;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < K; ++k) s = fmaf(hr[k], hw[k * stride], s);
    return s + (j < n_out ? b_out[j] : *b_value);
}

// The heads of the kM tile rows (envs b0 .., agent i) of a [B][N] batch: logits 0..A-1 and the value at A to s_out [kM][16], and
// to a.logits, a.value (and logits_scratch [B][N][16]) where given.  Args: PolicyArgs, LstmArgs or MoaArgs.
template <int K, int kM, int kThreads, class Args>
__device__ __forceinline__ void heads(const Args &a, const float *s_h, int pitch, const float *__restrict__ w_out,
                                      const float *__restrict__ w_value, const float *__restrict__ b_out,
                                      const float *__restrict__ b_value, float *s_out, float *logits_scratch, int tid, int b0, int i) {
    const int A = a.A;
    for (int q = tid; q < kM * 16; q += kThreads) {
        const int m = q >> 4, j = q & 15, b = b0 + m;
        if (j > A) continue;                                 // j < A: logit j; j == A: the value
        const float s = head<K>(s_h + m * pitch, w_out, w_value, b_out, b_value, A, j);
        s_out[m * 16 + j] = s;
        if (b < a.B) {
            const size_t row = (size_t)b * a.N + i;
            if (j < A) {
                if (a.logits) a.logits[row * A + j] = s;
                if (logits_scratch) logits_scratch[row * 16 + j] = s;
            } else if (a.value) {
                a.value[row] = s;
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- the action
// shared PRNG (prng.py): the triple32 chain of ssd_kernels.hip
__device__ __forceinline__ uint32_t pol_mix32(uint32_t x) {
    x ^= x >> 17; x *= 0xED5AD4BBu;
    x ^= x >> 11; x *= 0xAC4C1B51u;
    x ^= x >> 15; x *= 0x31848BABu;
    x ^= x >> 14;
    return x;
}

// The key of the S_POLICY draws of env `env` at (episode, t) (include/ssd.h): draw d of it is pol_mix32(key ^ d).
__device__ __forceinline__ uint32_t policy_key(uint32_t seed_lo, uint32_t seed_hi, uint32_t env, uint32_t episode, uint32_t t) {
    uint32_t key = 0x243F6A88u;
    key = pol_mix32(key ^ seed_lo);
    key = pol_mix32(key ^ seed_hi);
    key = pol_mix32(key ^ env);
    key = pol_mix32(key ^ episode);
    return pol_mix32(pol_mix32(key ^ t) ^ (uint32_t)SSD_S_POLICY);
}

// The action of agent i of env b from its logits l[0..A-1]: argmax (greedy), or the first a with u < cumulative softmax, u from
// the S_POLICY draw of the env's (episode, t) in h = hdr[b] (include/ssd.h); *logp its log-probability.
__device__ __forceinline__ int policy_pick(const float *l, int A, int greedy, uint4 h, uint32_t seed_lo, uint32_t seed_hi,
                                           uint32_t env, uint32_t i, float *logp) {
    float mx = l[0];
    int arg = 0;
    for (int k = 1; k < A; ++k)
        if (l[k] > mx) { mx = l[k]; arg = k; }
    float s = 0.f;
    for (int k = 0; k < A; ++k) s += expf(l[k] - mx);
    int act = arg;
    if (!greedy) {
        const float u = (float)(pol_mix32(policy_key(seed_lo, seed_hi, env, h.z, h.y) ^ i) >> 8) * 0x1p-24f;
        act = A - 1;
        float c = 0.f;
        for (int k = 0; k < A; ++k) {
            c += expf(l[k] - mx) / s;
            if (u < c) { act = k; break; }
        }
    }
    *logp = l[act] - (mx + logf(s));
    return act;
}

// Rollouts, one thread per tile row: the action of agent i of env b0 + tid from the logits heads() left in s_out, to a.actions
// (and actions_copy) and its log-probability to a.logp where given.  Args as heads().
template <int kM, class Args>
__device__ __forceinline__ void pick_actions(const Args &a, const float *s_out, int32_t *actions_copy, int tid, int b0, int i) {
    if (tid < kM && b0 + tid < a.B) {
        const int b = b0 + tid;
        float lp;
        const int act = policy_pick(s_out + tid * 16, a.A, a.greedy, a.greedy ? uint4{} : a.hdr[b], a.seed_lo, a.seed_hi,
                                    a.env_base + (uint32_t)b, (uint32_t)i, &lp);
        const size_t row = (size_t)b * a.N + i;
        a.actions[row] = act;
        if (actions_copy) actions_copy[row] = act;
        if (a.logp) a.logp[row] = lp;
    }
}

}  // namespace ssd
