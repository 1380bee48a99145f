// scan_prof.h -- the lab builds' aids of a cell-grouped scan (ivf_scan.hip alone includes it, behind fused5.h): the counters' buffer
// and the printers of what the profiling instantiations leave there.
#pragma once

// the lab builds' aids of a scan: the counters' buffer (option fused_prof) and the filter scan's fence (option scan_fence)
static int scan_prof_buffer(freddy_gpu_index* ix, Workspace* ws, long long** prof, uint32_t* fence = nullptr) {
  *prof = nullptr;
#ifdef FREDDY_LAB
  if (fence) *fence = (uint32_t)ix->tune.scan_fence;
  if (!ix->tune.scan_prof) return 0;
  if (ws->w_prof.ensure(sizeof(long long) * 16 * SCAN5_PROF_WGS))   // (two tables of 8 counters per workgroup: ivf_filter5_kernel)
    return fail(FREDDY_E_NOMEM, "profile buffer");
  *prof = ws->w_prof.as<long long>();
#endif
  (void)ix; (void)ws; (void)fence;
  return 0;
}

#ifdef FREDDY_LAB
// debugging aid (option fused_prof): per-phase shader-clock sums of every persistent workgroup's builder wave 0
// tail_waits (ivf_filter5_kernel): a second table behind the first -- gatherer wave 0's waits at the tail's barriers T1, T2, T3 and at the
// entry's last barrier, and the number of entries of more than 8 items (the ones with a second item segment and T3)
static int scan_prof_print(freddy_gpu_index* ix, hipStream_t s, const long long* prof, unsigned n_persist, bool tail_waits = false) {
  std::vector<long long> h(tail_waits ? 8 * ((size_t)SCAN5_PROF_WGS + n_persist) : 8 * (size_t)n_persist);
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(h.data(), prof, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
  double sum[8] = {0}; long long mx_end = 0, mn_end = -1; double ent = 0;
  for (unsigned b = 0; b < n_persist; ++b) {
    for (int i = 0; i < 6; ++i) sum[i] += (double)h[b * 8 + i];
    ent += (double)h[b * 8 + 7];
    mx_end = std::max(mx_end, h[b * 8 + 6]);
    mn_end = mn_end < 0 ? h[b * 8 + 6] : std::min(mn_end, h[b * 8 + 6]);
  }
  fprintf(stderr, "[scan prof] wgs=%u entries=%.0f  builder cycles/entry: builds=%.0f barrier-wait=%.0f tail=%.0f | gatherer wave 0 (fused5.h): main=%.0f colmin=%.0f S2=%.0f | workgroups ran dry over %.1f us\n",
          n_persist, ent, sum[0] / ent, sum[1] / ent, sum[3] / ent, sum[2] / ent, sum[4] / ent, sum[5] / ent, (mx_end - mn_end) / 100.0);
  if (tail_waits) {
    double w[5] = {0};
    for (unsigned b = 0; b < n_persist; ++b)
      for (int i = 0; i < 5; ++i) w[i] += (double)h[((size_t)SCAN5_PROF_WGS + b) * 8 + i];
    fprintf(stderr, "[scan prof] gatherer wave 0 waits, cycles/entry: T1=%.0f T2=%.0f T3=%.0f last=%.0f | entry total=%.0f | entries of more than 8 items: %.0f\n",
            w[0] / ent, w[1] / ent, w[2] / ent, w[3] / ent, (sum[2] + sum[4] + sum[5] + w[0] + w[1] + w[2] + w[3]) / ent, w[4]);
  }
  (void)ix;
  return 0;
}
// The counters of the filter scan's profiling instantiations (filter_kernel), once the scan of a round is enqueued: ivf_filter5_kernel's
// as above, ivf_filter8_kernel's (fused8.h) are gatherer wave 0's stages
static int filter_prof_print(freddy_gpu_index* ix, hipStream_t s, const FilterArgs& fl, bool whole, unsigned n_persist) {
  if (!fl.prof || fl.cand_count || !(whole || fl.K == 1024)) return 0;
  if (!whole) return scan_prof_print(ix, s, fl.prof, n_persist, true);
  std::vector<long long> h(8 * (size_t)n_persist);
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(h.data(), fl.prof, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
  double sum[8] = {0}, life_max = 0, life_min = 1e30;
  for (unsigned b = 0; b < n_persist; ++b) {
    for (int i = 0; i < 8; ++i) sum[i] += (double)h[b * 8 + i];
    life_max = std::max(life_max, (double)h[b * 8 + 7]); life_min = std::min(life_min, (double)h[b * 8 + 7]);
  }
  int32_t ng = 0;
  HIP_TRY(hipMemcpy(&ng, fl.n_groups, 4, hipMemcpyDeviceToHost));
  const double e = std::max(1, ng);
  fprintf(stderr, "[scan8 prof] wgs=%u entries=%d  gatherer wave 0 cycles/entry (slots 0-5): gather=%.0f B1=%.0f colmin=%.0f B2=%.0f S1=%.0f B3+S2+B4=%.0f | per workgroup: prologue (slot 6) %.0f, stages (0-5) %.0f, life (slot 7) mean %.0f min %.0f max %.0f\n",
          n_persist, ng, sum[0] / e, sum[1] / e, sum[2] / e, sum[3] / e, sum[4] / e, sum[5] / e, sum[6] / n_persist,
          (sum[0] + sum[1] + sum[2] + sum[3] + sum[4] + sum[5]) / n_persist, sum[7] / n_persist, life_min, life_max);
  return 0;
}
#endif
