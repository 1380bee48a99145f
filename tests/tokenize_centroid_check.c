/* The centroid loop of the reference (core_functions.c:371-379) restated in C, for tests/test_tokenize_inputs_cpu.py to compare
 * tests/tokenize_model.py with: built with cc -O2 -ffp-contract=off, and once with -fsanitize=address,undefined, and run as it is.
 * Input file (argv[1]): int32 n_texts, int32 d, then per text int32 n and n * d floats, the rows in list order.
 * Output file (argv[2]): per text d floats. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static void centroid(const float* rows, int n, int d, float* out) {
  for (int j = 0; j < d; ++j) out[j] = 0.0f;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < d; ++j) out[j] += rows[(size_t)i * d + j] / (float)n;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  int32_t n_texts, d;
  if (!in || !out || fread(&n_texts, 4, 1, in) != 1 || fread(&d, 4, 1, in) != 1 || n_texts < 0 || d <= 0) return 2;
  float* res = malloc(sizeof(float) * (size_t)d);
  for (int32_t t = 0; t < n_texts; ++t) {
    int32_t n;
    if (fread(&n, 4, 1, in) != 1 || n < 0) return 2;
    const size_t count = (size_t)n * (size_t)d;
    float* rows = malloc(sizeof(float) * (count ? count : 1));
    if (!rows || !res || fread(rows, sizeof(float), count, in) != count) return 2;
    centroid(rows, n, d, res);
    if (fwrite(res, sizeof(float), (size_t)d, out) != (size_t)d) return 2;
    free(rows);
  }
  free(res);
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
