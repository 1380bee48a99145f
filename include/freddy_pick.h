/* freddy_pick.h -- the random rank generic_cluster draws (freddy--0.0.1.sql:1107-1146), written once as code that a host compiler
 * and the device compiler both take (csrc/cluster.h: the initial centroids and the ten samples of a cluster):
 *
 *     round(random() * upper + 0.5)            a float8 expression; float8 round() is rint()
 *
 * as an index 1 .. upper:  pick(u, r) = min(max(rint(r * u + 0.5), 1), u).  Everything is binary64; the product is rounded before
 * the sum (no fused multiply-add: every unit that includes this header is compiled with -ffp-contract=off); rint rounds half to even in the default rounding mode, as nearbyint does.  The clamp is done in
 * binary64, before the conversion, so that no draw -- negative, 1.0 or far outside [0, 1) -- converts a value an int cannot hold.
 * A NaN draw is the caller's to refuse (freddy_gpu_cluster does); here it gives 1. */
#ifndef FREDDY_PICK_H
#define FREDDY_PICK_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FREDDY_PICK_FN __host__ __device__ static inline
#else
#define FREDDY_PICK_FN static inline
#endif

/* 1 <= upper <= 2^31 - 1 */
FREDDY_PICK_FN int32_t freddy_pick(int32_t upper, double r) {
  const double product = r * (double)upper;         /* rounded on its own */
  const double v = __builtin_rint(product + 0.5);
  if (!(v >= 1.0)) return 1;
  if (v > (double)upper) return upper;
  return (int32_t)v;
}

#endif
