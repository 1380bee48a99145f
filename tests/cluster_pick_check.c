/* Compares include/freddy_pick.h with the form the host mirror had (host/cluster.h: (int)nearbyint(r * upper + 0.5), clamped to
 * 1 .. upper) for u in {1, 2, 3, 10, 4096, 2^31 - 1}: the draws 0 and the largest double below 1, the exact halves (r * u + 0.5
 * ending in .5, for even and for odd integer parts) and 10^6 random draws.  A program of its own, so that it can be built with
 * -fsanitize=address,undefined and run as it is; tests/test_cluster_pick_cpu.py compiles it twice (plain and sanitized) and runs it.
 * One line per u ("<mismatches> <bits of the first draw that differs> u=<u> (<values> values)"); exits 0 iff nothing differs, every
 * section had the size it must have and the values below were seen. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "freddy_pick.h"

static int32_t pick_nearbyint(int32_t upper, double r) {
  const double v = nearbyint(r * upper + 0.5);        /* clamped before the conversion: r = 1 - 2^-53 at u = 2^31 - 1 gives 2^31 */
  return v < 1.0 ? 1 : (v > (double)upper ? upper : (int32_t)v);
}

static uint64_t bits_of(double f) { uint64_t u; memcpy(&u, &f, 8); return u; }

typedef struct { int64_t checked, bad, low, high, ties_even, ties_odd; uint64_t first_bad; } tally;

static void note(tally* t, int32_t u, double r) {
  const int32_t got = freddy_pick(u, r), want = pick_nearbyint(u, r);
  ++t->checked;
  if (got == 1) ++t->low;
  if (got == u) ++t->high;
  if ((got != want || got < 1 || got > u) && !t->bad++) t->first_bad = bits_of(r);
}

int main(void) {
  static const int32_t uppers[] = {1, 2, 3, 10, 4096, 2147483647};
  const double below_one = 1.0 - 1.0 / 9007199254740992.0;   /* 1 - 2^-53 */
  int status = 0;
  for (unsigned ui = 0; ui < sizeof uppers / sizeof uppers[0]; ++ui) {
    const int32_t u = uppers[ui];
    tally t = {0, 0, 0, 0, 0, 0, 0};
    note(&t, u, 0.0);
    note(&t, u, below_one);
    /* exact halves: r = j / u gives r * u + 0.5 = j + 0.5 exactly wherever j / u is a binary64 and the product returns j; the loop
     * keeps those (all of them for u a power of two; for the others the j that are multiples of u's odd part times a power of two) */
    for (int64_t j = 0; j <= 64 && j < u; ++j) {
      const double r = (double)j / (double)u;
      if (r * (double)u + 0.5 != (double)j + 0.5) continue;
      const int32_t want = (int32_t)((j & 1) ? j + 1 : j);            /* half to even */
      const int32_t clamped = want < 1 ? 1 : want;
      if (freddy_pick(u, r) != clamped && !t.bad++) t.first_bad = bits_of(r);
      if (j & 1) ++t.ties_odd; else ++t.ties_even;
      note(&t, u, r);
    }
    uint64_t state = 20260101u + (uint64_t)u;                         /* Knuth's 64-bit LCG, its upper 53 bits as a draw in [0, 1) */
    for (int i = 0; i < 1000000; ++i) {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      note(&t, u, (double)(state >> 11) * (1.0 / 9007199254740992.0));
    }
    /* draws outside [0, 1): the clamp, no conversion of a value an int cannot hold */
    note(&t, u, -3.0); note(&t, u, 1.0); note(&t, u, 7.5); note(&t, u, 1e300); note(&t, u, -1e300);
    const int64_t expected = 2 + t.ties_even + t.ties_odd + 1000000 + 5;
    printf("%lld 0x%016llx u=%d (%lld values, %lld even and %lld odd halves)\n", (long long)t.bad, (unsigned long long)t.first_bad, (int)u,
           (long long)t.checked, (long long)t.ties_even, (long long)t.ties_odd);
    if (t.bad || t.checked != expected || !t.low || !t.high || !t.ties_even || (u > 1 && !t.ties_odd)) status = 1;
  }
  return status;
}
