// tests/native/stats_plan_driver.cpp -- walks csrc/ssd_stats_plan.hpp (the launch arithmetic of ssd_stats_fold and the index
// functions its two kernels compile) over a grid of folds that reaches the ends of int32: every accepted plan is checked
// against the contract of the kernels it launches, every refusal must give a reason.  Compiled with g++ under the address and
// undefined-behaviour sanitizers by tests/test_stats_plan_cpu.py (a wrapped product stops the program); prints one line per
// group of checks, "ok" last.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ssd_stats_plan.hpp"

using namespace ssd::stats_plan;

#define REQUIRE(cond)                                                                                                  \
    do {                                                                                                               \
        if (!(cond)) { std::printf("FAILED line %d: %s\n   in %s\n", __LINE__, #cond, g_case); return false; }         \
    } while (0)
static char g_case[256] = "(no case)";

namespace {

constexpr int64_t kTwo30 = 1LL << 30, kMax = INT32_MAX;
constexpr int64_t kHipMaxGrid = INT32_MAX;                       // blocks in x

// One wave of pass 1 as the kernel sees it: chunk index from the wave number, then the guard, then the chunk's range.
bool check_wave(const Plan &p, int64_t wave, int64_t n_steps, bool *live) {
    const int64_t c = wave / p.rows;
    *live = wave_has_chunk(c, p.C);
    if (!*live) { REQUIRE(c >= p.C); return true; }               // rejected: nothing else is computed for it
    const int64_t k0 = chunk_begin(c, p.L), k1 = chunk_end(k0, p.L, n_steps);
    REQUIRE(c >= 0 && k0 >= 0 && k0 < n_steps && k0 < k1 && k1 <= n_steps && k1 - k0 <= p.L);
    REQUIRE(global_step1(kMax, k1 - 1) == kMax + k1);             // the global step of the chunk's last step at the largest step0
    REQUIRE((c == p.C - 1) == (k1 == n_steps));                  // the chunks tile 0 .. n_steps
    return true;
}

bool check_case(int32_t E, int32_t N, int32_t n_steps, int32_t chunk, bool *accepted) {
    std::snprintf(g_case, sizeof g_case, "E %d N %d n_steps %d chunk %d", E, N, n_steps, chunk);
    Plan p;
    std::memset(&p, 0x5a, sizeof p);
    *accepted = plan_fold(E, N, n_steps, chunk, p);
    if (!*accepted) {
        REQUIRE(p.why && p.why[0] != 0);
        REQUIRE(p.grid1 == 0 && p.grid2 == 0 && p.scratch_bytes == 0);
        // only what cannot be launched is refused: the waves of one pass outnumber a launch's threads
        const int64_t L = chunk == 0 ? (kAutoChunk < n_steps ? kAutoChunk : n_steps) : chunk < n_steps ? chunk : n_steps;
        const int64_t C = ((int64_t)n_steps + L - 1) / L, rows = ((int64_t)E + kWave / N - 1) / (kWave / N);
        REQUIRE(((C * rows + 3) / 4) * kBlock > kMaxGridThreads);
        return true;
    }
    REQUIRE(p.why && p.why[0] == 0);
    const int64_t n = n_steps, L = p.L, C = p.C;
    REQUIRE(1 <= L && L <= n);
    REQUIRE(chunk == 0 ? L == (n < kAutoChunk ? n : kAutoChunk) : L == (chunk < n ? chunk : n));
    REQUIRE(C >= 1 && (C - 1) * L < n && n <= C * L);
    const int64_t per = kWave / N;
    REQUIRE(p.rows >= 1 && (int64_t)p.rows * per >= E && ((int64_t)p.rows - 1) * per < E);
    // the grids: every (chunk, row) has its wave, fewer than one block of spare waves, and within HIP's limits
    const int64_t waves1 = (int64_t)p.grid1 * kWavesPerBlock, waves2 = (int64_t)p.grid2 * kWavesPerBlock;
    REQUIRE(p.grid1 >= 1 && p.grid2 >= 1 && p.grid1 <= kHipMaxGrid && p.grid2 <= kHipMaxGrid);
    REQUIRE((int64_t)p.grid1 * kBlock <= kMaxGridThreads && (int64_t)p.grid2 * kBlock <= kMaxGridThreads);
    REQUIRE(waves1 >= C * p.rows && waves1 - C * p.rows < kWavesPerBlock);
    REQUIRE(waves2 >= p.rows && waves2 - p.rows < kWavesPerBlock);
    // every launched wave of pass 1, the spare ones of the last block included (a long launch: its two ends and every wave
    // around each of 64 chunk boundaries spread over it)
    int64_t live = 0;
    bool is_live;
    if (waves1 <= (1 << 16)) {
        for (int64_t w = 0; w < waves1; ++w) { if (!check_wave(p, w, n, &is_live)) return false; live += is_live; }
        REQUIRE(live == C * p.rows);
    } else {
        for (int j = 0; j <= 64; ++j) {
            const int64_t mid = (C * p.rows / 64) * j;
            for (int64_t w = mid - 8; w < mid + 8; ++w)
                if (w >= 0 && w < waves1) { if (!check_wave(p, w, n, &is_live)) return false; REQUIRE(is_live == (w < C * p.rows)); }
        }
        for (int64_t w = waves1 - 8; w < waves1; ++w) { if (!check_wave(p, w, n, &is_live)) return false; REQUIRE(is_live == (w < C * p.rows)); }
    }
    // the scratch: C chunks of meta, head and tail, carved one after the other; the last element each kernel writes lies inside
    const int64_t lanes = (int64_t)E * N;
    REQUIRE((int64_t)p.part_lanes == C * lanes);
    REQUIRE((int64_t)p.meta_bytes == C * E * 16 && (int64_t)p.part_bytes == C * lanes * (3 * 8 + 2 * 4));
    REQUIRE(p.scratch_bytes == p.meta_bytes + 2 * p.part_bytes && (int64_t)p.scratch_bytes > 0);
    const int64_t last_o = (C - 1) * lanes + ((int64_t)E - 1) * N + (N - 1);       // pass 1: o = c * EN + lane_off
    REQUIRE(last_o == (int64_t)p.part_lanes - 1);
    REQUIRE((C - 1) * E + (E - 1) == (int64_t)p.meta_bytes / 16 - 1);               // meta[c * E + e]
    return true;
}

}  // namespace

int main() {
    const int64_t steps[] = {1, 2, 7, 8, 9, 63, 64, 65, 600, kTwo30, kMax};
    const int32_t shapes[][2] = {{1, 1}, {37, 5}, {3, 64}, {4096, 5}, {1 << 26, 1}, {1 << 26, 64}};
    long cases = 0, accepted = 0, refused = 0;
    for (int64_t n : steps) {
        const int64_t chunks[] = {0, 1, 2, 63, 64, 65, n - 1, n, n < kMax ? n + 1 : kMax, kTwo30, kMax};
        for (int64_t chunk : chunks)
            for (const auto &s : shapes) {
                bool ok;
                if (!check_case(s[0], s[1], (int32_t)n, (int32_t)chunk, &ok)) return 1;
                cases++;
                (ok ? accepted : refused)++;
            }
    }
    std::printf("grid: %ld cases ok, %ld accepted, %ld refused\n", cases, accepted, refused);
    // what the plan must refuse by its arguments alone
    {
        Plan p;
        bool bad = plan_fold(0, 1, 1, 0, p) || plan_fold(1, 0, 1, 0, p) || plan_fold(1, 65, 1, 0, p) || plan_fold(1, 1, 0, 0, p) ||
                   plan_fold(1, 1, 1, -1, p);
        if (bad || !p.why || !p.why[0]) { std::printf("FAILED: a malformed call was planned\n"); return 1; }
        std::printf("malformed calls: refused\n");
    }
    // the defect this header closes, by hand: 10 steps at a chunk of 2^31 - 1 or 2^30 are one chunk of 10, and the three spare
    // waves of its block leave by the guard
    const int32_t above[] = {INT32_MAX, 1 << 30, 11};
    for (int32_t chunk : above) {
        Plan p;
        if (!plan_fold(1, 5, 10, chunk, p) || p.L != 10 || p.C != 1 || p.grid1 != 1 || p.scratch_bytes != 16 + 2 * 5 * 32) {
            std::printf("FAILED: 10 steps at chunk %d\n", chunk);
            return 1;
        }
        for (int w = 1; w < 4; ++w)
            if (wave_has_chunk(w / p.rows, p.C)) { std::printf("FAILED: a spare wave passed the guard\n"); return 1; }
    }
    std::printf("by hand: ok\n");
    std::printf("ok\n");
    return 0;
}
