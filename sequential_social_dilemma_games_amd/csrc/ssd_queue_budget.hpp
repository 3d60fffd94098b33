// csrc/ssd_queue_budget.hpp -- how many dispatch queues of its own the library may hold per device.  A pure function of the two
// environment strings (no HIP, no HSA, no getenv): the library's own dispatch path (ssd_aql.hip, pool_limit) reads the variables
// once and acts on the verdict; a CPU test (tests/test_queue_budget_cpu.py) compiles this header with g++ and runs it over every
// case, because the GPU boxes only ever show one of them.
//
// A process gets about FOUR hardware queues before the hardware scheduler time-slices them, and the HIP runtime maps its streams
// onto at most GPU_MAX_HW_QUEUES of them (default 4, created lazily, as streams need them).  The rule, in order:
//   1. SSD_AQL_QUEUES set: its value (read as atoi reads it: garbage is 0), clamped to 1 .. top.
//   2. GPU_MAX_HW_QUEUES of 1, 2 or 3: the process has told the runtime to take fewer than its default -- the pool gets 4 minus
//      that (bench.py sets 2 for the ranks of a process group: a pool of 2).
//   3. Otherwise -- unset, 4 or more (4 is HIP's own default: exporting it says nothing new), 0, negative, unparsable: TWO, the
//      pool a host application with a few torch streams and RCCL's has room for.
// Every result is clamped to 1 .. top.  Whatever the rule says, a queue that fails its probe when it is created is destroyed again
// (ssd_aql.hip, pool_cap): the rule sets a budget, the probe guards against the cliff.
#pragma once
#include <cerrno>
#include <cstdlib>

namespace ssd {
namespace aql {

constexpr int kDefaultPoolQueues = 2;

inline int queue_pool_limit(const char *gpu_max_hw_queues, const char *ssd_aql_queues, int top) {
    if (top < 1) top = 1;
    int v = kDefaultPoolQueues;
    if (gpu_max_hw_queues) {
        char *end = nullptr;
        errno = 0;
        const long hq = std::strtol(gpu_max_hw_queues, &end, 10);
        if (end != gpu_max_hw_queues && errno == 0 && hq >= 1 && hq <= 3) v = 4 - (int)hq;
    }
    if (ssd_aql_queues) {                                   // (as atoi would read it, without its undefined overflow)
        const long q = std::strtol(ssd_aql_queues, nullptr, 10);
        v = q < 1 ? 1 : q > top ? top : (int)q;
    }
    return v < 1 ? 1 : v > top ? top : v;
}

}  // namespace aql
}  // namespace ssd
