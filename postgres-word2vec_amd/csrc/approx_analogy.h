// approx_analogy.h -- batched approximate analogies (freddy--0.0.1.sql:1317-1346 analogy_3cosadd_pq, :1428-1460 analogy_3cosadd_ivfadc,
// :1348-1384 analogy_3cosadd_in_pq): 3CosAdd with the candidates of an approximate search instead of the whole table.  Per triple
// (w1, w2, w3) whose three ids have a row (v1, v2, v3) in the vector handle:
//   raw  = vec_plus_bytea(vec_minus_bytea(v3, v1), v2)         raw[i] = (v3[i] - v1[i]) + v2[i], both rounded binary32
//   unit = vec_normalize_bytea(raw)                            analogy.h's arithmetic: sq += raw[i] * raw[i] (i ascending, multiply and add
//                                                              each rounded), length = (float)sqrt((double)sq), unit[i] = raw[i] / length
//                                                              (a correctly rounded binary32 division, never a reciprocal multiply)
//   L    = the public search for unit at n_cand                stage one IS freddy_gpu_ivfadc_search / freddy_gpu_pq_search: every path of it
//   row  = exact kNN of RAW over S = {id in L : id >= 0, id has a row, id not in (w1, w2, w3)}
//                                                              pv.h's re-rank with the triple's raw row as the query and PvArgs::exclude
// so a result row is bit for bit freddy_gpu_exact_search(vecs, raw, 1, k, S), and (-1, -inf) throughout when S is empty.
//
// aa_query_kernel is the stage in front: one workgroup (one wave) per triple.  Subtraction, addition and division are elementwise
// across the lanes; the sum of squares is the reference's one sequential chain (d dependent adds), walked by lane 0 over the raw
// row in LDS -- a wave per triple keeps it off every other triple's critical path.  raw goes to device memory (the re-rank's query
// column), unit straight into the pinned host block that stage one takes its queries from: a pinned query buffer skips the search's
// staging copy (include/freddy_gpu.h), so the search's copy kernels read it over PCIe as they read any caller's pinned batch.  Input
// vectors and candidate vectors never travel to the host.
//
// Nothing is special-cased: raw == 0 gives length 0 and a unit row of NaN (0 / 0), which the search treats as any NaN query; equal
// ids inside a triple are just equal rows.  A triple with an id that has no row is the SQL's empty join: the entry point resolves
// the ids against the handle's host copy of its ascending ids (as freddy_gpu_exact_analogy does; a subtraction when the ids are
// serial), compacts the triples that are left and scatters their rows back, so such a triple costs nothing, disturbs no neighbour,
// and a batch of them launches nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace freddy {

struct AaQueryArgs {
  const float* rows;        // [N][d] the vector handle's row-major copy
  const int32_t* in_rows;   // [Q'][3] rows of (w1, w2, w3)
  float* raw;               // [Q'][d] device memory
  float* unit;              // [Q'][d] pinned host memory, where stage one reads its queries
  int d;
};
static inline size_t aa_query_lds(int d) { return (size_t)d * sizeof(float); }

__global__ __launch_bounds__(64) void aa_query_kernel(AaQueryArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char aa_smem[];
  float* rs = reinterpret_cast<float*>(aa_smem);   // [d] the raw row
  __shared__ float len_s;
  const int t = blockIdx.x, lane = threadIdx.x, d = a.d;
  const int32_t* r = a.in_rows + (size_t)t * 3;
  const float *v1 = a.rows + (size_t)r[0] * d, *v2 = a.rows + (size_t)r[1] * d, *v3 = a.rows + (size_t)r[2] * d;
  float* raw = a.raw + (size_t)t * d;
  float* unit = a.unit + (size_t)t * d;
  for (int i = lane; i < d; i += 64) {
    const float m = v3[i] - v1[i];   // vec_minus_bytea(v3, v1)
    const float s = m + v2[i];       // vec_plus_bytea(.., v2)
    rs[i] = s;
    raw[i] = s;
  }
  __syncthreads();
  if (lane == 0) {
    float sq = 0.0f;
    for (int i = 0; i < d; ++i) { const float p = rs[i] * rs[i]; sq = sq + p; }   // core_functions.c:255-257
    len_s = (float)sqrt((double)sq);
  }
  __syncthreads();
  const float len = len_s;
  for (int i = lane; i < d; i += 64) unit[i] = rs[i] / len;
}

}  // namespace freddy
