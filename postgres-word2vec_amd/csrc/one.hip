// one.hip -- ONE query through the host-buffer calls as one launch (one.h): the hand-off buffer and its epochs and the end of such a
// call, for both kernels; and ivf_one, the launch of ivf_one_kernel for ivfadc_search (pipeline.hip calls it).  pq_one stays in
// pq.hip: pq_one_kernel<25> compiled into one module with ivf_one_kernel<25> comes out with its instructions in another order
// (profiles/ivfadc_units_refactor.txt 3.), and this cut changes no kernel's code.
#include "internal.h"

#include "kernels.h"
#include "one.h"
#include "ivf_run.h"
#include "stage_plan.h"   // HioOut

// The one-launch kernels' hand-off buffer: every published word carries the call's epoch in its top bit (one.h).  Calls of
// one shape write exactly the same words, so the epoch just flips; a different shape (or a new allocation) clears the
// buffer to epoch 0 and starts with epoch 1.
int one_buffer(Workspace* ws, hipStream_t s, uint64_t shape, size_t bytes, uint32_t* epoch) {
  void* before = ws->w_oneb.p;
  if (ws->w_oneb.ensure(bytes)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  // (one_pending: the previous call flipped the epoch and then did not launch -- an allocation or launch error in between --
  // so the words still carry the epoch of the call before it, which is this call's: cleared like a change of shape)
  if (ws->w_oneb.p != before || ws->one_shape != shape || ws->one_pending) {
    HIP_TRY(hipMemsetAsync(ws->w_oneb.p, 0, ws->w_oneb.cap, s));
    ws->one_shape = shape;
    ws->one_epoch = 1;
  } else {
    ws->one_epoch ^= 1u;
  }
  *epoch = ws->one_epoch;
  ws->one_pending = true;   // until the caller has seen its kernel launched (one_buffer_launched)
  return 0;
}

bool one_prof() {
  static const bool on = getenv("FREDDY_GPU_ONE_PROF") != nullptr;
  return on;
}

// The end of a one-launch call (one.h): the kernel's last store is the verdict word `err` in mapped host memory (2 = list
// written; ivf_one_kernel: 3 = list written, the reference would probe a second time; 1 = a bounded poll ran out), polled for
// up to a millisecond, then the stream is waited for the usual way.  A poll that ran out (the grid was not co-resident): the
// counters are re-armed and this handle keeps to the multi-launch paths.
int one_finish(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, volatile const int32_t* err,
               void (*print_stamps)(const unsigned long long* st), int* verdict) {
  if (wait_word(err, 1000) != 2) HIP_TRY(hipStreamSynchronize(s));
  if (one_prof()) {
    HIP_TRY(hipStreamSynchronize(s));
    unsigned long long st[16];
    (void)hipMemcpy(st, ws->w_one.as<unsigned long long>() + 8, sizeof(st), hipMemcpyDeviceToHost);
    print_stamps(st);
  }
  *verdict = *err;
  if (*verdict != 2 && *verdict != 3) {
    ix->one_launch_failed = true;
    ws->one_shape = 0;
  }
  return 0;
}

// ONE ivfadc_search query as one launch (one.h ivf_one_kernel).  Returns through *verdict: 2 = the list is in out_ids /
// out_dist; anything else = not answered here (shape not covered, the reference would probe a second time, or the grid
// never met at a barrier): the caller takes the multi-round path.
bool ivf_one_shape(const freddy_gpu_index* ix, int Q, int k, int W, int found_rule) {
  return ix->tune.one_launch && !ix->one_launch_failed && Q == 1 && ix->kind == KIND_IVF && fused_dims(ix) && ix->d == 300 && (ix->K & 3) == 0 && W <= 32 && 2 * k <= 64 && ix->C <= 4096 && ix->coarse && ix->cbT &&
         found_rule != FREDDY_FOUND_BATCH_UDF && ix->replicas.empty();
}
int ivf_one(freddy_gpu_index* ix, const float* queries, int k, int W, float sentinel, int found_rule, int32_t* out_ids,
                   float* out_dist, int* verdict) {
  *verdict = 0;
  hipStream_t s = ix->stream;
  Workspace* ws = workspace_for(ix, s);
  const int K = ix->K, C = ix->C, L = 2 * k;
  const size_t n_out = (size_t)k;
  const int G = ivf_one_groups(ix->n_cus, L);
  if (G < W) return 0;   // (an item per workgroup at least)
  if (ix->hio_out.ensure(HioOut::bytes(n_out))) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
  // the hand-off buffer (coarse distances | the W tables | the workgroups' lists | their accepted-row counts) and the kernel's LDS
  const OneLayout lay{K, C, W, L, G};
  uint32_t epoch = 0;
  if (int rc = one_buffer(ws, s, (2ull << 60) | ((uint64_t)C << 44) | ((uint64_t)K << 32) | ((uint64_t)W << 24) | ((uint64_t)G << 12) | (uint64_t)L,
                          lay.handoff_bytes(), &epoch)) return rc;
  if (one_prof() && ws->w_one.ensure(256)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  const HioOut out(ix->hio_out.p, n_out);
  int32_t* const h_ids = out.ids;
  float* const h_dist = out.dist;
  int32_t* const err = out.verdict;
  *err = 0;
  IvfOneArgs a;
  memcpy(a.qv, queries, sizeof(a.qv));
  a.coarse = ix->coarse; a.cbT = ix->cbT; a.list_off = ix->list_off; a.blk_off = ix->blk_off; a.packed = ix->packed; a.pos = ix->pos;
  char* ob = ws->w_oneb.as<char>();
  a.dist_g = reinterpret_cast<float*>(ob); a.lut_g = reinterpret_cast<float*>(ob + lay.lut_off()); a.part = reinterpret_cast<u64*>(ob + lay.part_off());
  a.cnt_g = reinterpret_cast<uint32_t*>(ob + lay.cnt_off());
  a.out_ids = h_ids; a.out_dist = h_dist; a.epoch = epoch; a.err = err;
  a.C = C; a.K = K; a.W = W; a.L = L; a.k = k; a.found_rule = found_rule == FREDDY_FOUND_ROWS ? 0 : 1;
  a.cell_limit = 100.0f; a.sentinel = sentinel;
  a.prof = one_prof() ? ws->w_one.as<unsigned long long>() + 8 : nullptr;
  memcpy(&a.sentinel_bits, &sentinel, 4);
  const size_t lds = lay.lds_bytes();
  if (lds > 60 * 1024) return 0;
  timed_launch(ix, s, "ivf_one", [&] { hipLaunchKernelGGL((ivf_one_kernel<25>), dim3((unsigned)G), dim3(ONE_WG), lds, s, a); });
  HIP_TRY(hipGetLastError());
  ws->one_pending = false;
  if (int rc = one_finish(ix, ws, s, err, [](const unsigned long long* st) {
        fprintf(stderr, "[ivf_one] wg0: coarse %.2f barrier %.2f plan %.2f tables %.2f barrier %.2f stage %.2f scan %.2f publish %.2f | last: since wg0 start %.2f load %.2f merge+list %.2f us\n",
                (st[1] - st[0]) * 0.01, (st[2] - st[1]) * 0.01, (st[3] - st[2]) * 0.01, (st[4] - st[3]) * 0.01, (st[5] - st[4]) * 0.01, (st[6] - st[5]) * 0.01,
                (st[7] - st[6]) * 0.01, (st[8] - st[7]) * 0.01, (st[10] - st[0]) * 0.01, (st[11] - st[10]) * 0.01, (st[12] - st[11]) * 0.01);
      }, verdict))
    return rc;
  if (*verdict == 2) {
    memcpy(out_ids, h_ids, n_out * 4);
    memcpy(out_dist, h_dist, n_out * 4);
  }
  return 0;
}
