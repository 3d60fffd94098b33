// ws::powf2 (csrc/ssd_ws_square.hpp, the square of the Watershed reward) against this libm's powf(x, 2.0f):
// every float32 in [2^-10, 4096) and a sample of negative and far-out inputs.  Prints "mismatches <n> checked <m>".
// Build: c++ -O2 -ffp-contract=off -fno-builtin -I<csrc> ws_square_check.cpp -lm
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include "ssd_ws_square.hpp"

static float (*volatile libm_powf)(float, float) = powf;   // through a pointer: the compiler may not fold powf(x, 2) into x*x

int main() {
    uint64_t bad = 0, n = 0;
    auto check = [&](float x) {
        float want = libm_powf(x, 2.0f), got = ws::powf2(x);
        ++n;
        if (ws::f2u(want) != ws::f2u(got)) {
            if (bad < 10) printf("x=%a powf=%a powf2=%a\n", x, want, got);
            ++bad;
        }
    };
    for (uint32_t u = ws::f2u(0x1p-10f); u < ws::f2u(4096.0f); ++u) check(ws::u2f(u));
    uint32_t s = 12345u;                                      // xorshift sample over every finite negative float and the edges
    for (int i = 0; i < 4000000; ++i) {
        s ^= s << 13; s ^= s >> 17; s ^= s << 5;
        check(-ws::u2f(s % 0x7f800000u));
        check(ws::u2f(s % 0x7f800000u));
    }
    const float edge[] = {0.0f, -0.0f, INFINITY, -INFINITY, 0x1p-149f, 0x1p-126f, 0x1p63f, 0x1p64f, 0x1.fffffep127f, 1.0f, -1.0f};
    for (float x : edge) check(x);
    printf("mismatches %llu checked %llu\n", (unsigned long long)bad, (unsigned long long)n);
    return bad != 0;
}
