/* freddy_similarity.h -- the similarity the plpgsql callers of pq_search derive from an ADC distance, written once as code that a host
 * compiler and the device compiler both take (csrc/assign.h: the key of freddy_gpu_pq_assign):
 *
 *     (1.0 - (distance / 2.0))::float4                                  freddy--0.0.1.sql:527,617
 *
 * where `distance` has been through the SRF's text round trip (freddy.c:164): snprintf("%f") into the tuple, float4in (strtof) on
 * the way out.  The host mirror's similarity_of() does exactly that with snprintf / strtof and stays the yardstick
 * (tests/test_assign_cpu.py compares the two bit for bit); this header computes the same value in integer and IEEE arithmetic
 * that is exact on both sides of the bus.
 *
 * Domain: 0 <= distance < 2^24 (a NaN, a negative or a larger distance is the caller's to exclude: freddy_gpu_pq_assign only
 * evaluates distances below its sentinel, refuses sentinels above 2^24, and an ADC distance is a sum of squares, never negative).
 *
 *   1. "%f" prints round-half-even(distance * 10^6) / 10^6 (glibc converts the exact binary value).  distance has a 24-bit
 *      significand and 10^6 = 2^6 * 15625 with 15625 < 2^14, so the double product distance * 1e6 is EXACT (<= 38 significant bits)
 *      and rint() of it -- half to even on an exact value -- is the printed number of millionths, n < 2^24 * 10^6 < 2^44.
 *   2. strtof of those digits is the correctly rounded binary32 of the rational n / 10^6.  From 2^23 on every binary32 is an
 *      integer and prints as itself; below, n < 2^23 * 10^6 and the significand is M = round-half-even((n << s) / 10^6) with
 *      s >= 0 the shift that puts the quotient into [2^23, 2^24): n << s < 2^44 fits 64 bits, the remainder decides the
 *      rounding exactly (no second rounding, as (float)((double)n / 1e6) would have), and M * 2^-s is exact in binary32 (M <= 2^24,
 *      the value >= 10^-6 is far from the subnormals).
 *   3. 1.0 - y / 2.0 in double is exact (the halving always, the difference because y is 0 or has its last bit at or above
 *      2^-44), so the final conversion is the one rounding of the expression.
 * The function is monotone: a smaller distance never has a smaller similarity (every step is a monotone rounding). */
#ifndef FREDDY_SIMILARITY_H
#define FREDDY_SIMILARITY_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FREDDY_SIM_FN __host__ __device__ static inline
#else
#define FREDDY_SIM_FN static inline
#endif

/* the distance after snprintf("%f") / strtof, for 0 <= distance < 2^24 */
FREDDY_SIM_FN float freddy_emitted_distance(float distance) {
  if (distance >= 8388608.0f) return distance;                    /* an integer: "<digits>.000000" */
  const uint64_t n = (uint64_t)__builtin_rint((double)distance * 1e6);
  if (n == 0) return 0.0f;
  const uint64_t lo = 8388608ull * 1000000ull;                    /* 2^23 * 10^6 (43 bits); n < lo */
  int s = __builtin_clzll(n) - 21;                                /* n << s has 43 bits */
  if ((n << s) < lo) ++s;                                         /* lo <= n << s < 2 lo */
  const uint64_t num = n << s;
  uint64_t m = num / 1000000ull;                                  /* 2^23 <= m < 2^24 */
  const uint64_t r = num - m * 1000000ull;
  if (2 * r > 1000000ull || (2 * r == 1000000ull && (m & 1ull))) ++m;
  const uint32_t scale_bits = (uint32_t)(127 - s) << 23;          /* 2^-s, s in [0, 43] */
  float scale;
  __builtin_memcpy(&scale, &scale_bits, 4);
  return (float)m * scale;                                        /* both factors and the product exact */
}

/* host/freddy_udf.cpp similarity_of(): (float)(1.0 - (double)emitted(distance) / 2.0) */
FREDDY_SIM_FN float freddy_similarity_of(float distance) { return (float)(1.0 - (double)freddy_emitted_distance(distance) / 2.0); }

#endif
