// tests/native/queue_budget_driver.cpp -- runs csrc/ssd_queue_budget.hpp (how many dispatch queues the library may hold per device)
// over every case of its rule.  Compiled with g++ by tests/test_queue_budget_cpu.py; prints one line per group, "ok" last.
#include <cstdio>

#include "ssd_queue_budget.hpp"

using ssd::aql::queue_pool_limit;

#define CHECK(hq, q, top, want)                                                                                        \
    do {                                                                                                               \
        const int got = queue_pool_limit(hq, q, top);                                                                  \
        if (got != (want)) {                                                                                           \
            std::printf("FAILED line %d: GPU_MAX_HW_QUEUES=%s SSD_AQL_QUEUES=%s top=%d: %d, want %d\n", __LINE__,      \
                        (hq) ? (hq) : "(unset)", (q) ? (q) : "(unset)", top, got, want);                               \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

int main() {
    const char *const unset = nullptr;
    // GPU_MAX_HW_QUEUES alone: 1..3 leave 4 - n; unset, HIP's default 4 and anything above it leave the default of two
    CHECK(unset, unset, 3, 2);
    CHECK("1", unset, 3, 3);
    CHECK("2", unset, 3, 2);
    CHECK("3", unset, 3, 1);
    CHECK("4", unset, 3, 2);
    CHECK("8", unset, 3, 2);
    CHECK("32", unset, 3, 2);
    CHECK("99999999999999999999999", unset, 3, 2);     // (out of range for long)
    std::printf("GPU_MAX_HW_QUEUES alone: ok\n");
    // zero, negative, unparsable, empty: the default
    CHECK("0", unset, 3, 2);
    CHECK("-1", unset, 3, 2);
    CHECK("-3", unset, 3, 2);
    CHECK("garbage", unset, 3, 2);
    CHECK("", unset, 3, 2);
    CHECK(" ", unset, 3, 2);
    std::printf("GPU_MAX_HW_QUEUES zero, negative, unparsable: ok\n");
    // SSD_AQL_QUEUES wins whenever it is set, clamped to 1 .. top
    const char *hqs[] = {nullptr, "1", "2", "3", "4", "8", "32", "0", "garbage"};
    for (const char *hq : hqs) {
        CHECK(hq, "1", 3, 1);
        CHECK(hq, "2", 3, 2);
        CHECK(hq, "3", 3, 3);
        CHECK(hq, "4", 3, 3);
        CHECK(hq, "0", 3, 1);
        CHECK(hq, "-2", 3, 1);
        CHECK(hq, "garbage", 3, 1);                   // (atoi's reading: 0, clamped to 1)
        CHECK(hq, "99999999999999999999999", 3, 3);
    }
    std::printf("SSD_AQL_QUEUES over every GPU_MAX_HW_QUEUES: ok\n");
    // the upper bound: nothing above it, never below one (a bound below one counts as one)
    CHECK(unset, unset, 1, 1);
    CHECK("1", unset, 2, 2);
    CHECK("1", unset, 8, 3);
    CHECK("4", unset, 1, 1);
    CHECK(unset, "3", 2, 2);
    CHECK(unset, "7", 8, 7);
    CHECK(unset, "9", 8, 8);
    CHECK(unset, unset, 0, 1);
    CHECK("1", "3", -5, 1);
    std::printf("upper bound: ok\n");
    std::printf("ok\n");
    return 0;
}
