// exact_wide.hip -- option exact_wide: exact kNN as filter + refine (exact2.h) for tables of 512 < d <= 2048.  The option's state
// on the handle (the statistics and the fragment-order copy, taken when the option is set: exf_table_stats takes them at pin time
// only for d <= 512) and the launches of exf_wide_filter_kernel (exact_wide.h).  The chain around the launch -- prep, threshold,
// refine, the redo paths -- is exact.hip's and exact_host.h's, unchanged; the mutation paths keep the copy current through
// exf_table_stats, whose shape rule reads the option.
#include "internal.h"

#include "exact2.h"
#include "exact_wide.h"
#include "exact_host.h"

// Option exact_wide = value on `ix`.  Narrow tables (d <= 512): accepted, no effect.  Wide ones: 1 takes the statistics and builds the
// copy (index_bytes grows by it), 0 releases it.  A table the filter cannot serve (a non-finite element, a row norm^2 >= 1e30, option
// exact_filter = 0) accepts the option and keeps the all-exact kernels, as exf_ok = false means for narrow tables.
int exf_wide_set(freddy_gpu_index* ix, int64_t value) {
  if (ix->kind != KIND_VEC) return fail(FREDDY_E_KIND, "option exact_wide belongs to a vector handle");
  if (int rc = refuse_poisoned(ix)) return rc;
  const int on = value != 0 ? 1 : 0;
  if (ix->d <= EXF_NARROW_D) { ix->tune.exact_wide = on; return FREDDY_OK; }
  if (on == ix->tune.exact_wide) return FREDDY_OK;
  HIP_TRY(hipSetDevice(ix->device));
  if (!on) {
    HIP_TRY(hipStreamSynchronize(ix->stream));   // (no search of this handle reads the copy any more)
    ix->bytes -= (int64_t)ix->exf_xf.cap;
    ix->exf_xf.release();
    ix->exf_xf_strips = 0;
    ix->exf_ok = false; ix->exf_never = false;   // (the next exact_wide = 1 takes the statistics again from row 0)
    ix->tune.exact_wide = 0;
    return FREDDY_OK;
  }
  if (ix->d > EXW_MAX_D || ix->d % 4 != 0)
    return fail(FREDDY_E_LIMIT, "option exact_wide: d=%d is not served (d <= %d and d %% 4 == 0: the bracket of the filter is proven up to there)", ix->d, EXW_MAX_D);
  ix->tune.exact_wide = 1;
  if (int rc = exf_table_stats(ix, 0, ix->N)) {   // (the copy could not be allocated: nothing was, the handle is the one it was)
    ix->tune.exact_wide = 0;
    ix->exf_ok = false;
    return rc;
  }
  return FREDDY_OK;
}

namespace {
template <int TS, int R>
void launch_shape(const freddy_gpu_index* ix, hipStream_t s, const ExfArgs& fa, int nq, bool sample) {
  const dim3 grid(exf_wide_grid(ix->n_cus, fa.n_rows, R, exf_wide_per_cu(TS, R)));
  const int NT = nq <= 32 ? 1 : 2;
  const size_t lds = exf_wide_lds(NT, TS);
  if (NT == 1) {
    if (sample) hipLaunchKernelGGL((exf_wide_filter_kernel<1, true, TS, R>), grid, dim3(EXF_WG), lds, s, fa);
    else hipLaunchKernelGGL((exf_wide_filter_kernel<1, false, TS, R>), grid, dim3(EXF_WG), lds, s, fa);
  } else {
    if (sample) hipLaunchKernelGGL((exf_wide_filter_kernel<2, true, TS, R>), grid, dim3(EXF_WG), lds, s, fa);
    else hipLaunchKernelGGL((exf_wide_filter_kernel<2, false, TS, R>), grid, dim3(EXF_WG), lds, s, fa);
  }
}
template <int TS, int R>
void limits_of_shape(std::vector<LdsLimit>& out) {
  const int b = (int)EX_MAX_LDS;
  out.push_back({&exf_wide_filter_kernel<1, false, TS, R>, b}); out.push_back({&exf_wide_filter_kernel<2, false, TS, R>, b});
  out.push_back({&exf_wide_filter_kernel<1, true, TS, R>, b});  out.push_back({&exf_wide_filter_kernel<2, true, TS, R>, b});
}
}  // namespace

void exf_wide_launch(const freddy_gpu_index* ix, hipStream_t s, const ExfArgs& fa, int nq, bool sample) {
  switch (ix->tune.exact_wide_shape) {   // (the measured alternatives: profiles/exact_wide_timing.txt)
    case 1: launch_shape<16, 1>(ix, s, fa, nq, sample); break;
    case 2: launch_shape<8, 2>(ix, s, fa, nq, sample); break;
    default: launch_shape<8, 1>(ix, s, fa, nq, sample); break;
  }
}

// (segments of 16 k-steps for 64 queries: two buffers of 64 KiB)
std::vector<LdsLimit> lds_limits_exact_wide() {
  std::vector<LdsLimit> out;
  limits_of_shape<8, 1>(out); limits_of_shape<16, 1>(out); limits_of_shape<8, 2>(out);
  return out;
}
