// ssd_ws_square.hpp -- x**2 on a float32 the way the Watershed reward evaluates it.
//
// The reference computes its flow rewards as `a * x**2 + b * x + c` on np.float32 scalars
// (watershedOrderedComm.py:215).  NumPy hands a float32 scalar power to libm's powf, so the
// square is glibc's powf(x, 2.0f), not x*x: powf works in double precision through a
// table-driven log2 and exp2 and rounds that double approximation to float, which on about
// 0.07 % of inputs lands on the other side of a rounding midpoint than the correctly rounded
// x*x does.  ws_powf2 restates that method for y = 2 (the x86-64 FMA build of glibc, i.e. the
// multiply-adds written as fma below are fused there too) so that host and device agree with
// the reference bit for bit.  The constants are the published tables of that method (glibc
// sysdeps/ieee754/flt-32, from Arm's optimized-routines, MIT licensed): 2^(i/32) correctly
// rounded, and for log2 sixteen (1/c, log2 c) pairs with their degree-5 polynomial.
//
// Compiles as plain C++ (tests/native) and as HIP device code: WS_HD expands to __host__ __device__ under hipcc.
#ifndef SSD_WS_SQUARE_HPP
#define SSD_WS_SQUARE_HPP

#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__)
#define WS_HD __host__ __device__
#else
#define WS_HD
#endif

namespace ws {

WS_HD inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
WS_HD inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
WS_HD inline uint64_t d2u(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
WS_HD inline double u2d(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }

// The tables are function-local constexpr arrays: in device code they live in constant memory and a lookup is one load (a switch
// over constants makes the compiler keep every constant in registers across a kernel's loops).

// log2 on [0x3f330000 * 2^k ...]: 16 subintervals, (1/c, log2(c)) per subinterval
WS_HD inline double log2_tab(int i, int which) {
    static constexpr double tab[32] = {
        0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2,
        0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2,
        0x1.49539f0f010b0p+0, -0x1.7418b0a1fb77bp-2,
        0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2,
        0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2,
        0x1.25e227b0b8ea0p+0, -0x1.97c1d1b3b7af0p-3,
        0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3,
        0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4,
        0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5,
        0x1.0000000000000p+0, 0.0,
        0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4,
        0x1.ca4b31f026aa0p-1, 0x1.476a9543891bap-3,
        0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3,
        0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2,
        0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2,
        0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2,
    };
    return tab[i * 2 + which];
}

// bits of 2^(i/32) (correctly rounded double) minus i << 47
WS_HD inline uint64_t exp2_tab(int i) {
    static constexpr uint64_t tab[32] = {
        0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
        0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
        0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
        0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
        0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
        0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
        0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
        0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull,
    };
    return tab[i];
}

// powf(x, 2.0f) as glibc computes it (x86-64, FMA variant)
WS_HD inline float powf2(float x) {
    uint32_t ix = f2u(x) & 0x7fffffffu;          // y = 2 is an even integer: the sign of x never matters
    if (ix == 0 || ix >= 0x7f800000u)            // 0, inf, nan: x * x
        return x * x;
    if (ix < 0x00800000u) {                      // subnormal: normalise so that the exponent goes negative
        ix = f2u(u2f(ix) * 0x1p23f) & 0x7fffffffu;
        ix -= 23u << 23;
    }
    // log2(|x|) = k + log2(c) + log1p(z/c - 1)/ln2,  |x| = 2^k z with z in [0x3f330000, 2*0x3f330000)
    uint32_t tmp = ix - 0x3f330000u;
    int i = (int)((tmp >> 19) % 16u);
    uint32_t top = tmp & 0xff800000u;
    uint32_t iz = ix - top;
    int k = (int32_t)top >> 23;
    double invc = log2_tab(i, 0), logc = log2_tab(i, 1);
    double z = (double)u2f(iz);
    double r = fma(z, invc, -1.0);
    double y0 = logc + (double)k;
    double r2 = r * r;
    double y = fma(0x1.27616c9496e0bp-2, r, -0x1.71969a075c67ap-2);
    double p = fma(0x1.ec70a6ca7baddp-2, r, -0x1.7154748bef6c8p-1);
    double r4 = r2 * r2;
    double q = fma(0x1.71547652ab82bp+0, r, y0);
    q = fma(p, r2, q);
    double logx = fma(y, r4, q);
    double ylogx = 2.0 * logx;
    if (((d2u(ylogx) >> 47) & 0xffff) >= (d2u(126.0) >> 47)) {   // |2 log2 x| >= 126
        if (ylogx > 0x1.fffffffd1d571p+6) return INFINITY;
        if (ylogx <= -150.0) return 0.0f;
    }
    // exp2(ylogx) = 2^(k/32) * 2^r,  r in [-1/64, 1/64]
    double kd = ylogx + 0x1.8p+47;
    uint64_t ki = d2u(kd);
    kd -= 0x1.8p+47;
    double rr = ylogx - kd;
    uint64_t t = exp2_tab((int)(ki % 32u));
    t += ki << 47;
    double s = u2d(t);
    double zz = fma(0x1.c6af84b912394p-5, rr, 0x1.ebfce50fac4f3p-3);
    double rr2 = rr * rr;
    double yy = fma(0x1.62e42ff0c52d6p-1, rr, 1.0);
    yy = fma(zz, rr2, yy);
    yy = yy * s;
    return (float)yy;
}

}  // namespace ws

#endif
