// TEST INFRASTRUCTURE ONLY.  expf_glibc (rl_markets_amd/csrc/lob_env.h: std::exp(float) of REWARD_MM_EXP restated for the device),
// compiled from the engine's own device header through tests/host_env/shim, against this libm's expf, bit for bit:
//   (1) the argument MM_EXP hands it, pos_weight * (f32)|position| as a float product, over the bounds the sweeps draw:
//       pos_weight 0 .. 0.2 in steps of 1e-4, |position| 0 .. 10 000 (2 x 50 x order size 100) -- the sum overflows to +inf from
//       88.72 on, which the range crosses;
//   (2) the over- and underflow thresholds of e_expf.c (88, 0x1.62e42ep6, -0x1.9fe368p6, the first subnormal result at
//       -0x1.5d58ap6) and 64 floats on either side of each;
//   (3) +-0, the smallest and largest subnormals and normals, +-inf, quiet and signalling-pattern NaNs of both signs (a NaN
//       result is compared as "both NaN": the payload of x + x is the hardware's);
//   (4) random bit patterns (argv[1], default 10 000 000).
//   g++ -std=c++17 -O1 -mfma -ffp-contract=off -Itests/host_env/shim -o expf_diff tests/host_env/expf_diff.cpp && ./expf_diff [cases]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>

#include "../../rl_markets_amd/csrc/lob_state.h"
#include "../../rl_markets_amd/csrc/lob_stream.h"
struct TickLds {
    int n;
    f64 lb[LOB_MAX_BANDS];
    f64 tick[LOB_MAX_BANDS];
    i64 cum[LOB_MAX_BANDS];
    f64 pp[LOB_MAX_BANDS];
    i32 pt[LOB_MAX_BANDS];
};
void lob_set_error(const std::string&) {}
#include "../../rl_markets_amd/csrc/lob_env.h"

static long n_checked = 0, n_bad = 0, n_inf = 0, n_zero = 0, n_subnormal = 0, n_nan = 0;

static void check(float x) {
    // (volatile: the compiler may not fold libm's result at build time)
    volatile float xv = x;
    const float got = expf_glibc(xv), want = expf(xv);
    n_checked++;
    if (want != want) {
        n_nan++;
        if (got == got) { if (n_bad++ < 10) printf("x=%a (0x%08x): restatement %a, libm NaN\n", x, __float_as_uint(x), got); }
        return;
    }
    const uint32_t w = __float_as_uint(want);
    n_inf += w == 0x7f800000u; n_zero += w == 0u; n_subnormal += w != 0u && w < 0x00800000u;
    if (__float_as_uint(got) != w && n_bad++ < 10) printf("x=%a (0x%08x): restatement %a, libm %a\n", x, __float_as_uint(x), got, want);
}

int main(int argc, char** argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 10000000;
    // (1)
    long n_range = 0, n_range_inf = 0;
    for (int w = 0; w <= 2000; w++) {
        const float pos_weight = (float)(w * 1e-4);
        for (int pos = 0; pos <= 10000; pos++) {
            const long inf0 = n_inf;
            check(pos_weight * (float)pos);
            n_range++; n_range_inf += n_inf - inf0;
        }
    }
    // (2)
    const float edges[] = {88.0f, -88.0f, 0x1.62e42ep6f, -0x1.9fe368p6f, -0x1.5d58ap6f, 0x1.62e43p6f, 1.0f, -1.0f};
    for (float e : edges) {
        float up = e, down = e;
        check(e);
        for (int i = 0; i < 64; i++) {
            up = nextafterf(up, INFINITY); down = nextafterf(down, -INFINITY);
            check(up); check(down);
        }
    }
    // (3)
    const uint32_t specials[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u,
                                 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xff800001u,
                                 0x7fffffffu, 0xffffffffu};
    for (uint32_t u : specials) check(__uint_as_float(u));
    // (4)
    std::mt19937_64 rng(20260);
    for (long i = 0; i < cases; i++) check(__uint_as_float((uint32_t)rng()));
    printf("checked %ld (%ld of the MM_EXP range, %ld of them +inf); results: %ld inf, %ld zero, %ld subnormal, %ld NaN\n", n_checked, n_range,
           n_range_inf, n_inf, n_zero, n_subnormal, n_nan);
    printf("mismatches %ld\n", n_bad);
    if (n_bad == 0) printf("expf_diff OK\n");
    return n_bad != 0;
}
