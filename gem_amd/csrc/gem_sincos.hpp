// gem_sincos.hpp -- the sine and cosine of the trajectory-generation contract (include/gem_hip_trajgen.h), written once for the host
// compiler and the device: plain double + - * only, every operation rounded on its own (the build has -ffp-contract=off), so the
// kernel, its host twin and the numpy restatement (tests/trajgen_ref.py) agree to the bit and a pose does not depend on whose cos it
// was.  For |t| <= 64 pi (the contract's bound) the result is within 2^-53 of libm's on the angles tried, 2 * 2^-53 up to 2^20.
//   k = (t * INV + 1.5 * 2^52) - 1.5 * 2^52            the nearest integer to t * 2 / pi
//   r = ((t - k * P1) - k * P2) - k * P3               pi / 2 in three pieces: k * P1 and k * P2 are exact for |k| < 2^20
//   z = r * r
//   sin r = r + r * (z * S(z))                          S: Horner over (-1)^i / (2 i + 1)!, i = 8 .. 1
//   cos r = 1.0 + z * C(z)                              C: Horner over (-1)^i / (2 i)!,     i = 8 .. 1
// and the quadrant (long long)k & 3 swaps and negates.  The coefficients are quotients of integers below 2^53: each is a correctly
// rounded double.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GEM_SINCOS_HD __host__ __device__ __forceinline__
#else
#define GEM_SINCOS_HD inline
#endif

namespace gem {

// s = sin t, c = cos t by the contract's form
GEM_SINCOS_HD void gem_sincos(double t, double& s, double& c)
{
    const double INV = 0x1.45F306DC9C883p-1;                             // 2 / pi: the bits 0x3FE45F306DC9C883
    const double P1 = 0x1.921FB544p+0, P2 = 0x1.0B4611A6p-34, P3 = 0x1.3198A2E037073p-69;     // 0x3FF921FB54400000, 0x3DD0B4611A600000, 0x3BA3198A2E037073
    const double BIG = 6755399441055744.0;                               // 1.5 * 2^52
    const double k = (t * INV + BIG) - BIG;
    const double r = ((t - k * P1) - k * P2) - k * P3;
    const double z = r * r;
    double p = 1.0 / 355687428096000.0;                                  // 1 / 17!
    p = p * z + -1.0 / 1307674368000.0;                                  // -1 / 15!
    p = p * z + 1.0 / 6227020800.0;                                      // 1 / 13!
    p = p * z + -1.0 / 39916800.0;                                       // -1 / 11!
    p = p * z + 1.0 / 362880.0;                                          // 1 / 9!
    p = p * z + -1.0 / 5040.0;                                           // -1 / 7!
    p = p * z + 1.0 / 120.0;                                             // 1 / 5!
    p = p * z + -1.0 / 6.0;                                              // -1 / 3!
    const double sr = r + r * (z * p);
    double q = 1.0 / 20922789888000.0;                                   // 1 / 16!
    q = q * z + -1.0 / 87178291200.0;                                    // -1 / 14!
    q = q * z + 1.0 / 479001600.0;                                       // 1 / 12!
    q = q * z + -1.0 / 3628800.0;                                        // -1 / 10!
    q = q * z + 1.0 / 40320.0;                                           // 1 / 8!
    q = q * z + -1.0 / 720.0;                                            // -1 / 6!
    q = q * z + 1.0 / 24.0;                                              // 1 / 4!
    q = q * z + -1.0 / 2.0;                                              // -1 / 2!
    const double cr = 1.0 + z * q;
    const int quad = (int)((long long)k & 3ll);
    s = quad == 0 ? sr : (quad == 1 ? cr : (quad == 2 ? -sr : -cr));
    c = quad == 0 ? cr : (quad == 1 ? -sr : (quad == 2 ? -cr : sr));
}

} // namespace gem
