// exact_rank.hip -- option exact_filter_k: the two launches exact kNN's filter + refine chain (exact_host.h: exf_chain) takes for
// result lists of 33 .. 1024 rows -- the threshold by rank selection and the refine stage with a tree merge (exact_rank.h).  A unit
// of its own so that the units that include the chain (exact.hip, analogy.hip, exact_wide.hip) compile the kernels they compiled
// before, and these are built without packed fp32 instructions (the build entry's UNIT_FLAGS).
#include "internal.h"

#include "exact2.h"
#include "exact_rank.h"

void exf_rank_threshold_launch(const freddy_gpu_index* ix, hipStream_t s, unsigned grid_q, const ExfThrArgs& ta) {
  if (ix->tune.exact_rank_hist == 1) hipLaunchKernelGGL((exf_rank_threshold_kernel<4>), dim3(grid_q), dim3(64 * EXF_TW), 0, s, ta);
  else hipLaunchKernelGGL((exf_rank_threshold_kernel<1>), dim3(grid_q), dim3(64 * EXF_TW), 0, s, ta);
}

// exf_refine_tree_kernel<V>, V = 2 .. 16 (V = 1 is exf_refine_kernel<1>: the caller's); false: no such width
bool exf_refine_tree_launch(hipStream_t s, int V, unsigned n_queries, const ExfRefineArgs& ra) {
  if (V < 2) return false;
  const size_t lds = exf_refine_lds(ra.d, V);
  return with_V(V, [&](auto v) {
    constexpr int VV = decltype(v)::value;
    if constexpr (VV >= 2) hipLaunchKernelGGL((exf_refine_tree_kernel<VV>), dim3(n_queries), dim3(64 * EXF_TW), lds, s, ra);
  });
}

// exf_refine_lds(d, V) = 4 d + 8 KiB + V * 8 KiB with d <= 2048 (EXW_MAX_D): V = 2 and 4 stay below 64 KiB (48 KiB at most), V = 8
// takes 72 .. 80 KiB, V = 16 takes 136 .. 144 KiB
std::vector<LdsLimit> lds_limits_exact_rank() {
  return {&exf_refine_tree_kernel<8>, &exf_refine_tree_kernel<16>};
}
