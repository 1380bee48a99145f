// scan_tail5.h -- what the integer filter scans (fused5.h, fused8.h, sparse5.h) share around their selection tail, as functions:
// the order-preserving key of a column minimum, the query's running bound, widening a threshold by E, one item's S1 step
// (filter_threshold5: fused8.h), the survivor key, and the switch that picks the gatherers' main loop.  The tail of the cell-grouped scans'
// gatherer waves itself -- column minima and the survivor pass -- is scan_tail5.inc, a fragment both kernels include in their
// bodies (why it is text: there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "refine.h"

namespace freddy {

// order-preserving 32-bit key of a float (NaNs sort above +inf or below -inf: only met with non-finite inputs)
__device__ __forceinline__ uint32_t float_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
// selection threshold of the integer scan from the KEY of tau': tau' + E rounded up, as a float; +inf = keep every row
__device__ __forceinline__ uint32_t widen_threshold5(uint32_t tau_key, float E) {
  const uint32_t b = (tau_key & 0x80000000u) ? (tau_key ^ 0x80000000u) : ~tau_key;
  const float tau = __uint_as_float(b);
  if (!(tau < 3e38f) || !(tau > -3e38f) || !(E < 1e30f)) return 0x7f800000u;
  const float t = tau + E;
  return __float_as_uint(t + __builtin_fabsf(t) * 2.4e-7f + 1e-37f);
}

// The query's running bound (FilterArgs::tau_run), one (item, chunk)'s part: t = key of its own tau', [a_lo, a_up] its coarse
// distance, inv = the bound as read earlier (0: none).  Reports tau' + a_up if that improves on what was read (one atomic at
// most), returns the key the item cuts at: min(tau', bound - a_lo).  (Derivation: ivf_filter5_kernel, S1.)
__device__ __forceinline__ uint32_t running_bound5(uint32_t* __restrict__ tau_run, uint32_t q, uint32_t t, float a_up, float a_lo, uint32_t inv) {
  const uint32_t tb = (t & 0x80000000u) ? (t ^ 0x80000000u) : ~t;   // key -> bits
  const float tau = __uint_as_float(tb);
  if (tau < 3e38f && tau > -3e38f && a_up < 3e38f) {
    const uint32_t mine = ~float_key(tau + a_up);
    if (mine > inv) atomicMax(tau_run + q, mine);
    if (inv != 0u) {
      const uint32_t bk = ~inv;
      const float alt = __uint_as_float((bk & 0x80000000u) ? (bk ^ 0x80000000u) : ~bk) - a_lo;
      if (alt < tau) return float_key(alt);
    }
  }
  return t;
}

// S1, lane 0's part for item i of a cell-grouped entry (rec: its record, entry_record5_kernel): t = the key of tau', the Lt-th
// smallest of the item's sorted column minima; returns the bits of the float the item cuts at, tau' + E (+inf: keep_all).
// inv = the query's running bound as read earlier.  (ivf_filter5_kernel's builder waves call it once per item segment, item w
// and then item w + 8, each after a sort of its own.)
__device__ __forceinline__ uint32_t filter_threshold5(const FilterArgs& a, const int32_t* rec, int i, uint32_t t, uint32_t inv) {
  if (a.tau_run) t = running_bound5(a.tau_run, (uint32_t)rec[24 + i], t, __int_as_float(rec[144 + i]), __int_as_float(rec[160 + i]), inv);
  return a.keep_all ? 0x7f800000u : widen_threshold5(t, __int_as_float(rec[56 + i]));
}

// main_loop(I<NQ>, I<RL>) for nq = 16-byte halves of a slab row in use (1, 2) and rl_wave = row blocks of this wave (RL = the next
// even number, at least 2)
template <class F>
__device__ __forceinline__ void dispatch_nq_rl(int nq, int rl_wave, F&& main_loop) {
  int rl = rl_wave;
  rl = rl < 1 ? 1 : rl;
  const int rc = (rl + 1) >> 1;
  using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
  using I4 = std::integral_constant<int, 4>;
  using I6 = std::integral_constant<int, 6>; using I8 = std::integral_constant<int, 8>;
  switch ((nq < 1 ? 1 : nq) * 4 + rc) {
    case 1 * 4 + 1: main_loop(I1{}, I2{}); break;
    case 1 * 4 + 2: main_loop(I1{}, I4{}); break;
    case 1 * 4 + 3: main_loop(I1{}, I6{}); break;
    case 1 * 4 + 4: main_loop(I1{}, I8{}); break;
    case 2 * 4 + 1: main_loop(I2{}, I2{}); break;
    case 2 * 4 + 2: main_loop(I2{}, I4{}); break;
    case 2 * 4 + 3: main_loop(I2{}, I6{}); break;
    default: main_loop(I2{}, I8{}); break;
  }
}

// A survivor's key, as merge_refine_kernel reads it: the bits of d_lo above the row's location (bit 31 of it: the `amb` flag).
__device__ __forceinline__ u64 surv_key5(float dlo, uint32_t loc) { return ((u64)__float_as_uint(dlo) << 32) | (u64)loc; }

}  // namespace freddy
