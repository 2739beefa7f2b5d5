// The one device digamma: k_elbo (k_params.hip), the Wishart bound's psi_multi (k_wishart.hip) and the tape interpreter's
// U_DIGAMMA (k_tape.hip) all call this function.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else       // a host compiler (column_parents.h under tests/c/column_parents_driver.cpp): the same function, host only
#include <cmath>
#define __host__
#define __device__
#endif

// digamma for positive and for negative non-integer arguments: the recurrence up to x >= 10, then the asymptotic series.
// The recurrence takes 10 - x steps: bounded here, so that no argument (a degenerate qv, -inf, a NaN from bad state) can keep a
// workgroup spinning.  Not finite: NaN (+inf: +inf); below -64: the reflection formula, its cotangent taken of pi (x - rint(x)):
// the difference is exact and tan has period pi, whereas the rounding of pi x (half an ulp of |pi x|, 2e-13 at x = -1000) went
// into the result undiminished -- 1.5e-13 relative at -1000.25, 3e-14 at -64.5 (tests/test_envelope_gpu.py:
// test_device_special_functions).
// Poles: a negative integer below -64 gives NaN; 0 and the negative integers down to -64 meet 1 / 0 in the recurrence and give
// +-inf or NaN, as they always did.  The bounds never pass one.
// (__host__ too: column_parents.h forms psi(qa) of the columns' precision parents once, on the host, and pyvb_pca_set_priors that of
// Beta's shape.)
__host__ __device__ static inline double digamma_pos(double x) {
    if (!(x - x == 0.0) || x < -4.5e15) return x > 0 ? x : __builtin_nan("");      // below -2^52 every double is an integer: a pole
    double r = 0.0;
    if (x < -64.0) {
        const double t = x - rint(x);
        if (t == 0.0) return __builtin_nan("");     // a negative integer: a pole, NaN as below -2^52
        r = -M_PI / tan(M_PI * t); x = 1.0 - x;
    }
    while (x < 10.0) { r -= 1.0 / x; x += 1.0; }
    const double f = 1.0 / (x * x);
    const double ser = f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760 - f / 12))))));
    return r + log(x) - 0.5 / x - ser;
}
