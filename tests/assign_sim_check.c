/* Compares include/freddy_similarity.h with the text round trip it restates (host/freddy_udf.cpp emitted() / similarity_of():
 * snprintf("%f") then strtof, then (float)(1.0 - (double)y / 2.0)), bit for bit.  A program of its own, so that it can be built
 * with -fsanitize=address,undefined and run as it is; tests/test_assign_cpu.py compiles it twice (plain and sanitized) and runs it.
 * It prints one line per section ("<mismatches> <bits of the first one> <section>") and exits 0 iff no value differs and the
 * sections had the sizes they must have. */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "freddy_similarity.h"

static float emitted_text(float distance) {
  char buf[16];
  snprintf(buf, sizeof buf, "%f", distance);
  return strtof(buf, NULL);
}
static float similarity_text(float distance) { return (float)(1.0 - (double)emitted_text(distance) / 2.0); }

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static int differs(float x) {
  return bits_of(freddy_emitted_distance(x)) != bits_of(emitted_text(x)) || bits_of(freddy_similarity_of(x)) != bits_of(similarity_text(x));
}

typedef struct {
  const char* name;
  void (*run)(void* self);
  uint32_t first_bits, count;      /* a band: every binary32 whose bits are first_bits .. first_bits + count - 1 */
  int64_t checked, expected;       /* values looked at; how many there must be (-1: whatever the section finds) */
  int64_t bad;                     /* mismatches */
  uint32_t first_bad;              /* the first one's bits */
} section;

static void note(section* s, float x) {
  ++s->checked;
  if (differs(x) && !s->bad++) s->first_bad = bits_of(x);
}

static void run_band(void* self) {
  section* s = self;
  for (uint32_t i = 0; i < s->count; ++i) note(s, float_of(s->first_bits + i));
}

/* Every binary32 below 16 whose distance * 10^6 ends in exactly .5: x * 10^6 = x * 2^6 * 15625 has the fractional part .5 iff
 * x * 2^7 * 15625 is an odd integer, i.e. x is an odd multiple of 2^-7.  The loop walks the multiples of 2^-7 (all binary32 below
 * 2^17) and keeps the ties: 1024 of them. */
static void run_ties(void* self) {
  section* s = self;
  for (uint32_t j = 1; (float)j / 128.0f < 16.0f; ++j) {
    const float x = (float)j / 128.0f;               /* exact */
    const double y = (double)x * 1e6;                /* exact */
    if (y - (double)(uint64_t)y == 0.5) note(s, x);
  }
}

/* 10^6 values in [0, 1000): Knuth's 64-bit LCG, its upper 53 bits as a double in [0, 1), times 1000, rounded to binary32 (a value
 * that rounds up to 1000 itself is drawn again) */
static void run_random(void* self) {
  section* s = self;
  uint64_t state = 20260101u;
  while (s->checked < 1000000) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    const float x = (float)((double)(state >> 11) * (1.0 / 9007199254740992.0) * 1000.0);
    if (x < 1000.0f) note(s, x);
  }
}

static void* run_section(void* self) {
  section* s = self;
  s->run(s);
  return NULL;
}

#define BAND(name, center_or_first, before, count) {name, run_band, (center_or_first) - (before), count, 0, count, 0, 0}

int main(void) {
  const uint32_t half = bits_of(0.5f), one = bits_of(1.0f), two = bits_of(2.0f), four = bits_of(4.0f);
  section sections[] = {
      BAND("2^22 values around 0.5", half, 1u << 21, 1u << 22),
      BAND("2^22 values around 1", one, 1u << 21, 1u << 22),
      BAND("2^22 values around 2", two, 1u << 21, 1u << 22),
      BAND("2^22 values around 4", four, 1u << 21, 1u << 22),
      BAND("the 65536 values below 1000, and 1000", bits_of(1000.0f), 65536u, 65537u),
      BAND("the smallest 65536 values, 0 included", 0u, 0u, 65536u),
      BAND("the 65536 values below 2^24", bits_of(16777216.0f), 65536u, 65536u),
      {"the exact .5 ties of distance * 10^6 below 16", run_ties, 0, 0, 0, 1024, 0, 0},
      {"10^6 random values in [0, 1000)", run_random, 0, 0, 0, 1000000, 0, 0},
  };
  enum { N_SECTIONS = sizeof sections / sizeof sections[0] };
  pthread_t threads[N_SECTIONS];
  for (int i = 0; i < N_SECTIONS; ++i)
    if (pthread_create(&threads[i], NULL, run_section, &sections[i]) != 0) { fprintf(stderr, "pthread_create failed\n"); return 2; }
  int status = 0;
  for (int i = 0; i < N_SECTIONS; ++i) {
    pthread_join(threads[i], NULL);
    const section* s = &sections[i];
    printf("%lld 0x%08x %s (%lld values)\n", (long long)s->bad, (unsigned)s->first_bad, s->name, (long long)s->checked);
    if (s->bad || s->checked != s->expected) status = 1;
  }
  return status;
}
