// csrc/ssd_stats_plan.hpp -- the launch arithmetic of one fold of the episode statistics (ssd_stats.hip): the chunk length, the
// number of chunks, both grids and the scratch carve.  No HIP: ssd_stats_fold plans through it, the two kernels index through
// its constexpr functions, and a CPU test (tests/test_stats_plan_cpu.py) compiles it with g++ under the sanitizers and walks it
// to the ends of int32, where no GPU run is wanted.
//
// A caller may set any chunk length 0 .. INT32_MAX (ssd_stats_set_chunk: "speed only, never a result"), n_steps <= ring may be
// INT32_MAX and so may step0.  Everything here is therefore computed in 64 bits and nothing wraps:
//   L      the effective chunk length: chunk (0: kAutoChunk) clamped to 1 .. n_steps, so a chunk above n_steps acts as n_steps;
//   C      ceil(n_steps / L) chunks, so (C - 1) * L < n_steps <= C * L and every chunk index c < C starts at c * L < n_steps;
//   rows   waves that hold every (env, agent) lane once, floor(64 / N) whole envs to a wave;
//   grid1  blocks of pass 1, one wave per (chunk, row); a block has kWavesPerBlock waves, so up to three waves of the last block
//          have no chunk: they leave by wave_has_chunk(c, C), a comparison, not by a product that could wrap;
//   grid2  blocks of pass 2, one wave per row;
//   scratch  meta int4 [C][E], then head and tail, each five arrays over [C][E*N].
// A plan is refused, with a reason, when a grid has more threads than a launch can number (the kernels form the global thread
// index in 32 bits, and HIP refuses more) or the scratch does not fit the size type; a scratch that fits the type and not the
// device is hipMalloc's to refuse.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ssd {
namespace stats_plan {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kAutoChunk = 64;                                   // steps per chunk when the caller has not set one
constexpr int kMetaBytes = 16;                                   // one int4 per (chunk, env)
constexpr int kPartLaneBytes = 3 * 8 + 2 * 4;                    // R, tsum, hits int64; pos, tagged int32 per (chunk, env, agent)
constexpr int64_t kMaxGridThreads = 0xffffffffLL;                // grid * kBlock: a launch numbers its threads in 32 bits
constexpr int64_t kMaxScratchBytes = INT64_MAX;                  // (PTRDIFF_MAX where the library is built)

// -- shared with the kernels: both sides compile this text
constexpr bool wave_has_chunk(int64_t c, int64_t C) { return c < C; }                 // pass 1's guard for a launched wave
constexpr int64_t chunk_begin(int64_t c, int64_t L) { return c * L; }                 // c < C: below n_steps
constexpr int64_t chunk_end(int64_t k0, int64_t L, int64_t n_steps) { return k0 + L < n_steps ? k0 + L : n_steps; }
constexpr int64_t global_step1(int64_t step0, int64_t k) { return step0 + k + 1; }    // what reset_every divides at an end

struct Plan {
    int32_t L, C, rows;
    uint32_t grid1, grid2;                                       // blocks of kBlock threads
    size_t part_lanes;                                           // C * E * N: the length of each array of head and tail
    size_t meta_bytes, part_bytes, scratch_bytes;                // scratch = meta + 2 * part
    const char *why;                                             // the reason of a refusal, else ""
};

inline bool refuse(Plan &p, const char *why) { p = Plan{0, 0, 0, 0, 0, 0, 0, 0, 0, why}; return false; }

// false: refused, p.why says why and nothing else of p is to be used.
inline bool plan_fold(int32_t E, int32_t N, int32_t n_steps, int32_t chunk, Plan &p) {
    if (E < 1 || N < 1 || N > kWave) return refuse(p, "the fold's shape: num_envs >= 1, num_agents 1..64");
    if (n_steps < 1) return refuse(p, "a fold is planned for n_steps >= 1");
    if (chunk < 0) return refuse(p, "chunk must be >= 0");
    const int64_t n = n_steps;
    int64_t L = chunk > 0 ? chunk : kAutoChunk;
    if (L > n) L = n;                                            // a chunk above n_steps acts as n_steps
    const int64_t C = (n + L - 1) / L;
    const int64_t per = kWave / N;
    const int64_t rows = ((int64_t)E + per - 1) / per;
    const int64_t grid1 = (C * rows + kWavesPerBlock - 1) / kWavesPerBlock;           // C, rows < 2^31: the product fits
    const int64_t grid2 = (rows + kWavesPerBlock - 1) / kWavesPerBlock;
    if (grid1 * kBlock > kMaxGridThreads) return refuse(p, "too many chunks for one launch of pass 1: set a longer chunk");
    if (grid2 * kBlock > kMaxGridThreads) return refuse(p, "too many envs for one launch of pass 2");
    // (with grid1 accepted C * rows < 2^26 and rows * 64 >= E * N, so C * E * N < 2^32 and the sizes below are far inside 64 bits)
    const int64_t lanes = (int64_t)E * N;
    const int64_t meta = C * E * kMetaBytes, part = C * lanes * kPartLaneBytes;
    if (meta > kMaxScratchBytes - 2 * part) return refuse(p, "the fold's scratch does not fit a size");
    p.L = (int32_t)L; p.C = (int32_t)C; p.rows = (int32_t)rows;
    p.grid1 = (uint32_t)grid1; p.grid2 = (uint32_t)grid2;
    p.part_lanes = (size_t)(C * lanes);
    p.meta_bytes = (size_t)meta; p.part_bytes = (size_t)part; p.scratch_bytes = (size_t)(meta + 2 * part);
    p.why = "";
    return true;
}

}  // namespace stats_plan
}  // namespace ssd
