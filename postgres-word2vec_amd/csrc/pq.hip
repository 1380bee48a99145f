// pq.hip -- pq_search / pq_search_in(_batch) (freddy.c:28-152, :1028-1157, :414-653), grouping_pq (freddy.c:1176-1401) and the
// assignment step of cluster_pq (assign.h).
#include "internal.h"

#include "kernels.h"
#include "scan_common.h"
#include "fused5.h"   // query_codebook5_body: the table units of pq_front_kernel
#include "one.h"
#include "io_kernels.h"
#include "assign.h"
#include "ivf_host.h"
#include "query_ids.h"
#include "stage_plan.h"

// kernel choosers (generic.hip says what one is).  M2: dwords of codes per row with an instantiation of its own, else 0 = any m
static decltype(&grouping_kernel<0>) grouping_kernel_for(int M2) {
  return M2 == 6 ? &grouping_kernel<6> : M2 == 15 ? &grouping_kernel<15> : &grouping_kernel<0>;
}
static void (*assign_pq_kernel_for(int M2, int RPT))(AssignPqArgs) {   // RPT: targets per thread, 4 or 1
  if (M2 == 6) return RPT == 4 ? &assign_pq_kernel<6, 4> : &assign_pq_kernel<6, 1>;
  return RPT == 4 ? &assign_pq_kernel<0, 4> : &assign_pq_kernel<0, 1>;
}

// ---------------------------------------------------------------------------------------
// exhaustive / subset PQ
// ---------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------
// Batches over the flat PQ table through the cell-grouped filter + refine scan (fused5.h).
//
// adc_scan_kernel runs one workgroup per (query, chunk): every query re-reads the code table from the caches and gathers
// 4-byte LUT entries one (query, row, position) at a time.  The IVFADC scan shares a chunk's rows among 16 queries and
// gathers eight 16-bit table values per LDS access -- and pq_search's distance is ivfadc_search's with a residual
// r = q - 0: the flat table is pinned a second time only as METADATA -- pseudo-lists of 4096 consecutive rows
// (FUSED_UNIT_BLOCKS blocks; the packed codes are shared), a zero centroid per list, the row terms sum_p |c|^2, the rows'
// ids -- in a shadow index of kind IVF, and a batch "probes" every list: items (query, list) for all pairs, no coarse
// distances, no plan.  The exact stage then evaluates (q_i - 0) - c_i: x - 0 = x exactly, so its squares, their
// order of summation (index_utils.c:500-508, 1126-1133) and the guarded insertion in ascending id order are pq_search's
// (freddy.c:28-152).  The item's bound on |r|^2 is squareDistance(q, 0) evaluated the reference's way.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pq_shadow_meta_kernel(const int32_t* __restrict__ pos, const int32_t* __restrict__ ids,
                                                            int64_t n_blocks, int64_t n_rows, int lists, int32_t* __restrict__ list_off,
                                                            int32_t* __restrict__ blk_off, int32_t* __restrict__ blk_cell,
                                                            int32_t* __restrict__ pos_ids) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i <= lists) {
    const int64_t r = i * (FUSED_UNIT_BLOCKS * 64), b = i * FUSED_UNIT_BLOCKS;
    list_off[i] = (int32_t)(r < n_rows ? r : n_rows);
    blk_off[i] = (int32_t)(b < n_blocks ? b : n_blocks);
  }
  if (i < n_blocks) blk_cell[i] = (int32_t)(i / FUSED_UNIT_BLOCKS);
  if (i < n_blocks * 64) { const int32_t r = pos[i]; pos_ids[i] = r >= 0 ? ids[r] : -1; }
}

// (not fused_shape(): a PQ handle has no paired codebook; the exact stage's cbR and the kernels' own K limit are what this path needs)
static bool pq_fused_shape(const freddy_gpu_index* ix) {
  return ix->kind == KIND_PQ && ix->cbR && ix->m == 12 && ix->S == 25 && ix->K <= FUSED_T * FUSED_E && ix->n_blocks > 0 && ix->N > 0;
}

static bool pq_use_fused(const freddy_gpu_index* ix, int Q, int k) {
  if (ix->tune.pq_fused == 0 || !pq_fused_shape(ix) || 2 * k > 64) return false;
  return ix->tune.pq_fused > 0 || Q >= 16;
}
// A batch over the flat PQ table needs no probe plan and no work table: every query "probes" every pseudo-list, so the
// work entries are (group of 16 queries, pseudo-list) and their records follow from the query's table scale alone.  One
// workgroup per query: |q|^2 in the reference's order (squareDistance(q, 0): the coarse distance of the zero centroid, the
// bound item_bounds builds on), then the query's lane of every record of its group; the first query of a group also writes
// the records' headers.  Replaces pq_items + work_table + entry_record kernels (27 us of three dependent launches).
// item index = q * W + list (W >= lists: padded to a multiple of the merge's slices; the padding items have no entry, their
// survivor regions stay zero).
struct PqFrontArgs {
  const float* queries; int Q, d, lists, W; int64_t n_rows;
  const int32_t* blk_off; const int32_t* list_off;
  const float* cbT; const float* cmax; const float* pmax;
  float* qn; float* qscale; uint32_t* qc; int m, K;
  uint32_t* qc8;   // K <= 256: the compact copy of the table (fused8.h); NULL: not wanted
  float sentinel;
  int32_t* item_cell; int32_t* item_query; float* item_dist; int32_t* round_rows; int32_t* records; int32_t* n_groups;
  ZeroArgs z;   // the call's scratch that must start at zero (counters, running bounds, survivor counts): no memset launches in front
};
__device__ __forceinline__ void pq_records_body(const PqFrontArgs& a, int q, unsigned char* smem) {
  const float* __restrict__ queries = a.queries;
  const int Q = a.Q, d = a.d, lists = a.lists, W = a.W;
  const int64_t n_rows = a.n_rows;
  const int32_t* __restrict__ blk_off = a.blk_off; const int32_t* __restrict__ list_off = a.list_off;
  const float* __restrict__ pmax = a.pmax;
  const float sentinel = a.sentinel;
  int32_t* __restrict__ item_cell = a.item_cell; int32_t* __restrict__ item_query = a.item_query; float* __restrict__ item_dist = a.item_dist;
  int32_t* __restrict__ round_rows = a.round_rows; int32_t* __restrict__ records = a.records; int32_t* __restrict__ n_groups = a.n_groups;
  float* sqs = reinterpret_cast<float*>(smem);          // [1024]
  float* qn_s = sqs + 1024;                              // [16] |q_p| rounded up, as query_codebook5_body forms it
  float* fs = qn_s + 16;                                 // [0] A, [1] scale
  const int tid = threadIdx.x;
  for (int i = tid; i < d; i += 256) { const float t = queries[(size_t)q * d + i] - 0.0f; sqs[i] = t * t; }
  // the query's per-position norms and its table scale: the very operations of query_codebook5_body (same order, same roundings),
  // so that this workgroup needs nothing from the table units of the same launch
  if (tid < 16) {
    const int pp = tid, S = d / a.m;
    float best = 0.0f;
    if (pp < a.m) {
      float n2 = 0.0f;
      for (int j = 0; j < S; ++j) { const float v = queries[(size_t)q * d + pp * S + j]; n2 = __builtin_fmaf(v, v, n2); }
      const float nrm = __builtin_sqrtf(n2) * (1.0f + 1e-5f);
      qn_s[pp] = nrm;
      best = 2.0f * nrm * a.cmax[pp];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    if (pp == 0) fs[1] = best * (1.0f / (float)FILT5_VMAX) * (1.0f + 1e-6f);
  }
  __syncthreads();
  if (tid == 0) {
    float acc = 0.0f;
    for (int i = 0; i < d; ++i) acc = acc + sqs[i];     // index_utils.c:500-508, i ascending
    fs[0] = acc;
    round_rows[q] = (int32_t)n_rows;
    if (q == 0) n_groups[0] = ((Q + SCAN5_G - 1) / SCAN5_G) * lists;
  }
  __syncthreads();
  const float A = fs[0];
  const float sc = fs[1];
  const ItemBounds ib = item_bounds(A, filter_width5<12>(qn_s, pmax, sc), sentinel);
  const int g = q / SCAN5_G, slot = q % SCAN5_G;
  const int cnt = (Q - g * SCAN5_G < SCAN5_G) ? Q - g * SCAN5_G : SCAN5_G;
  for (int c = tid; c < lists; c += 256) {
    const int it = q * W + c;
    item_cell[it] = c; item_query[it] = q; item_dist[it] = A;
    int32_t* rec = records + ((size_t)g * lists + c) * REC_DW;
    rec[8 + slot] = it;
    rec[24 + slot] = q;
    rec[40 + slot] = (int32_t)__float_as_uint(ib.off);
    rec[56 + slot] = (int32_t)__float_as_uint(ib.e);
    rec[72 + slot] = (int32_t)__float_as_uint(ib.shift);
    rec[88 + slot] = (int32_t)ib.lo_bits;
    rec[104 + slot] = (int32_t)ib.hi_bits;
    rec[128 + slot] = (int32_t)__float_as_uint(sc < 1e30f ? sc : 0.0f);
    {   // (entry_record5_kernel: the item's coarse distance -- here |q|^2, the zero centroid's -- as an interval)
      const bool fin = ib.e < 1e30f && A >= 0.0f && A < 1e30f;
      rec[144 + slot] = (int32_t)__float_as_uint(fin ? A * (1.0f + 2e-5f) : __uint_as_float(0x7f800000u));
      rec[160 + slot] = (int32_t)__float_as_uint(fin ? A * (1.0f - 2e-5f) : 0.0f);
    }
    if (slot == 0) {
      const int b0 = blk_off[c];
      rec[0] = c; rec[1] = cnt; rec[2] = 0; rec[3] = b0; rec[4] = blk_off[c + 1] - b0; rec[5] = list_off[c + 1] - list_off[c];
      // the slots beyond the group's queries: no item, the first query's number (a valid table), no bounds (entry_record5_kernel)
      const ItemBounds none = item_bounds(0.0f, 0.0f, sentinel);
      for (int u = cnt; u < SCAN5_G; ++u) {
        rec[8 + u] = -1; rec[24 + u] = q;
        rec[40 + u] = (int32_t)__float_as_uint(none.off); rec[56 + u] = (int32_t)__float_as_uint(none.e); rec[72 + u] = (int32_t)__float_as_uint(none.shift);
        rec[88 + u] = (int32_t)none.lo_bits; rec[104 + u] = (int32_t)none.hi_bits; rec[128 + u] = 0;
        rec[144 + u] = (int32_t)0x7f800000; rec[160 + u] = 0;
      }
    }
  }
}

// The table units of query_codebook5_kernel and the record workgroups above as ONE launch (neither needs the other: the record
// workgroups form the query's scale themselves): a dependent launch less in a PQ batch's chain.
__global__ __launch_bounds__(256) void pq_front_kernel(PqFrontArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n_table = a.m * ((a.Q + 15) / 16);
  const int b = blockIdx.x;
  {
    const int gtid = b * 256 + (int)threadIdx.x, gsz = (int)gridDim.x * 256;
#pragma unroll
    for (int r = 0; r < 5; ++r)
      for (int i = gtid; i < a.z.n[r]; i += gsz) a.z.p[r][i] = 0u;
  }
  if (b < n_table) query_codebook5_body<25, 16>(a.queries, a.cbT, a.cmax, a.qn, a.qscale, a.qc, a.Q, a.d, a.m, a.K, b % a.m, b / a.m, smem, a.qc8);
  else pq_records_body(a, b - n_table, smem);
}

// survivor regions: 32 KiB per (query, pseudo-list) within the workspace budget; the buckets [lists][queries] within 256 MiB
static int pq_fused_queries_per_chunk(const freddy_gpu_index* ix, int64_t n_blocks) {
  const size_t lists = (size_t)((n_blocks + FUSED_UNIT_BLOCKS - 1) / FUSED_UNIT_BLOCKS);
  size_t n = ((size_t)ix->tune.lut_budget_mb << 20) / (sizeof(u64) * lists * FUSED_NW * FUSED_RMAX * 64);
  n = std::min<size_t>(n, ((size_t)256 << 20) / (sizeof(int32_t) * lists));
  return (int)std::max<size_t>(16, std::min<size_t>(n, 1u << 16));
}

// An IVF-shaped view (*view; created on first use) of `n_rows` rows in `n_blocks` packed blocks: pseudo-lists, zero centroids,
// row terms, ids.  Everything is enqueued on s; nothing is synchronised.
static int pq_view_refresh(freddy_gpu_index* ix, freddy_gpu_index** view, hipStream_t s, const uint32_t* packed, const int32_t* pos,
                           int64_t n_blocks, int64_t n_rows) {
  freddy_gpu_index* fx = *view;
  if (!fx) {
    fx = new freddy_gpu_index();
    fx->shadow_of = ix;
    fx->kind = KIND_IVF; fx->device = ix->device; fx->stream = ix->stream; fx->n_cus = ix->n_cus;
    fx->d = ix->d; fx->m = ix->m; fx->K = ix->K; fx->S = ix->S; fx->M2 = ix->M2;
    if (dev_malloc((void**)&fx->viol, 4 * sizeof(int32_t)) != hipSuccess || hipMemset(fx->viol, 0, 4 * sizeof(int32_t)) != hipSuccess) {
      free_index(fx);
      return fail(FREDDY_E_NOMEM, "device allocation failed (PQ table as pseudo-lists)");
    }
    *view = fx;
  }
  fx->tune = ix->tune;
  fx->cbT = ix->cbT; fx->cbR = ix->cbR; fx->pmax = ix->pmax; fx->cmaxp = ix->cmaxp; fx->cbF = ix->cbF;   // shared with the owner
  fx->packed = const_cast<uint32_t*>(packed);
  fx->packed8 = (packed == ix->packed) ? ix->packed8 : nullptr; fx->packed8_own = false;   // (a subset's gathered rows: the int16 layout)
  fx->N = n_rows; fx->n_blocks = n_blocks; fx->max_list_blocks = FUSED_UNIT_BLOCKS;
  const int lists = (int)((n_blocks + FUSED_UNIT_BLOCKS - 1) / FUSED_UNIT_BLOCKS);
  fx->C = lists;
  const size_t slots = (size_t)n_blocks * 64;
  if (fx->v_coarse.ensure(sizeof(float) * (size_t)lists * ix->d) || fx->v_list_off.ensure(sizeof(int32_t) * ((size_t)lists + 1)) ||
      fx->v_blk_off.ensure(sizeof(int32_t) * ((size_t)lists + 1)) || fx->v_blk_cell.ensure(sizeof(int32_t) * (size_t)n_blocks) ||
      fx->v_pos.ensure(sizeof(int32_t) * slots) || fx->v_rterm.ensure(sizeof(float) * slots))
    return fail(FREDDY_E_NOMEM, "device allocation failed (PQ table as pseudo-lists)");
  fx->coarse = fx->v_coarse.as<float>(); fx->list_off = fx->v_list_off.as<int32_t>(); fx->blk_off = fx->v_blk_off.as<int32_t>();
  fx->blk_cell = fx->v_blk_cell.as<int32_t>(); fx->pos = fx->v_pos.as<int32_t>(); fx->rterm = fx->v_rterm.as<float>();
  HIP_TRY(hipMemsetAsync(fx->coarse, 0, sizeof(float) * (size_t)lists * ix->d, s));
  hipLaunchKernelGGL(pq_shadow_meta_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, pos, ix->ids, n_blocks, n_rows, lists,
                     fx->list_off, fx->blk_off, fx->blk_cell, fx->pos);
  hipLaunchKernelGGL(row_term_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, fx->packed, fx->blk_cell, fx->coarse, fx->cbR,
                     fx->rterm, (int64_t)slots, fx->M2, fx->d, fx->m, fx->K, fx->S);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the whole table's view: built once (and again after rows were appended or the codebook was replaced)
int pq_shadow_build(freddy_gpu_index* ix) {
  if (ix->pq_shadow) return 0;
  if (int rc = pq_view_refresh(ix, &ix->pq_shadow, ix->stream, ix->packed, ix->pos, ix->n_blocks, ix->N)) {
    if (ix->pq_shadow) { free_index(ix->pq_shadow); ix->pq_shadow = nullptr; }
    return rc;
  }
  HIP_TRY(hipStreamSynchronize(ix->stream));   // (searches may come in on other streams)
  return 0;
}


static int pq_fused_chunk(freddy_gpu_index* ix, freddy_gpu_index* fx, hipStream_t s, const float* d_q, int Q, int k, float sentinel,
                          int32_t* d_out_ids, float* d_out_dist) {
  fx->tune = ix->tune;
  Workspace* ws = workspace_for(fx, s);
  const int lists = fx->C, m = fx->m;
  // the merge of a small batch over many pseudo-lists: four workgroups per query, each over a quarter of the lists (64 queries
  // x 1 960 survivor regions on 64 workgroups took 62 us on a quarter of the chip); the item space of a query is padded to
  // a multiple of the slices
  const int SL = (lists >= 32 && Q <= 256 && (size_t)lists * FUSED_NW > 256) ? 4 : 0;
  const int W = SL ? ((lists + SL - 1) / SL) * SL : lists;
  // filter + refine over the items (query, pseudo-list): records from pq_front_kernel, no found rule, no running bounds (a few dozen queries x
  // a thousand entries would update the same two cache lines: 96 -> 128 us).  share: the caller's contract, its batches in flight on this handle
  IvfRun r = ivf_run(fx, ws, s, scan_share_now(ix->tune.scan_share, false, ix->device), d_q, Q, k, W, sentinel, d_out_ids, d_out_dist, nullptr);
  r.fused = true; r.records_ready = true; r.merge_slices = SL;
  const size_t n_entries = (size_t)((Q + SCAN5_G - 1) / SCAN5_G) * lists;
  if (ivf_run_ensure(r) || ws->w_records.ensure(sizeof(int32_t) * REC_DW * n_entries))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed (Q=%d over %d pseudo-lists)", Q, lists);
  const PlanArgs pa = plan_items(r, lists);
  const WorkTable wt = work_counters(ws, n_entries);   // (no tables: the entries are the records, and no cell is scanned item by item)
  const QueryTable qt = query_table(ws, fx, Q);
  // ONE launch: the table units (query x codebook, int16) and the record workgroups -- the entry records straight from the
  // queries' table scales: no item / work-table / record kernels (pq_front_kernel)
  PqFrontArgs fa;
  fa.queries = d_q; fa.Q = Q; fa.d = fx->d; fa.lists = lists; fa.W = W; fa.n_rows = fx->N; fa.blk_off = fx->blk_off; fa.list_off = fx->list_off;
  fa.cbT = fx->cbF; fa.cmax = fx->cmaxp; fa.pmax = fx->pmax; fa.qn = qt.qn; fa.qscale = qt.qscale; fa.qc = qt.qc; fa.qc8 = qt.qc8;
  fa.m = m; fa.K = fx->K; fa.sentinel = sentinel; fa.item_cell = pa.item_cell; fa.item_query = pa.item_query;
  fa.item_dist = pa.item_dist; fa.round_rows = pa.round_rows; fa.records = ws->w_records.as<int32_t>(); fa.n_groups = wt.n_groups;
  // (w_cnt[1] = n_groups is WRITTEN by this launch's record workgroups: not among the words it clears)
  fa.z.p[0] = ws->w_cnt.as<uint32_t>(); fa.z.n[0] = 1;
  fa.z.p[1] = ws->w_cnt.as<uint32_t>() + 2; fa.z.n[1] = 6;
  fa.z.p[2] = ws->w_cand.as<uint32_t>() + Q; fa.z.n[2] = Q;   // the queries' running bounds (FilterArgs::tau_run)
  fa.z.p[3] = ws->w_surv_cnt.as<uint32_t>(); fa.z.n[3] = (int)surv_regions(r, (size_t)Q * W);
  fa.z.p[4] = nullptr; fa.z.n[4] = 0;
  const size_t front_lds = std::max<size_t>((size_t)query_codebook5_lds<25, 16>(), (size_t)(1024 + 16 + 2) * sizeof(float));
  timed_launch(fx, s, "pq_front", [&] {
    hipLaunchKernelGGL(pq_front_kernel, dim3((unsigned)(m * ((Q + 15) / 16) + Q)), dim3(256), front_lds, s, fa);
  });
  HIP_TRY(hipGetLastError());
  return ivf_scan_filter(r, pa, wt);
}


// ONE query over the flat table as one launch (one.h): table slices, grid barrier, scan, last-arriver merge.  `err` is a
// word of mapped host memory the kernel sets when one of its bounded polls ran out (the grid was not co-resident): the
// caller then re-arms the counters and takes the three-launch path.
static bool pq_one_shape(const freddy_gpu_index* ix, int Q, int k, int64_t n_blocks) {
  return ix->tune.one_launch && !ix->one_launch_failed && Q == 1 && fused_dims(ix) && (ix->K & 3) == 0 && ix->d == 300 &&
         2 * k <= 64 && n_blocks >= 64 && (int64_t)ix->h_ids.size() == ix->N;
}
static int pq_one(freddy_gpu_index* ix, hipStream_t s, const float* h_q, int k, float sentinel, const int32_t* blk_off,
                  const uint32_t* packed, const int32_t* pos, int64_t n_blocks, int32_t* d_out_ids, float* d_out_dist, int32_t* err) {
  Workspace* ws = workspace_for(ix, s);
  const int K = ix->K, L = 2 * k;
  // (one workgroup per CU at most: all co-resident; the last arriver stages every list in LDS: G * L keys within 56 KB)
  const int G = pq_one_groups(ix->n_cus, L, n_blocks, ONE_WAVES);
  const int chunk_blocks = (int)((n_blocks + G - 1) / G);
  const OneLayout lay{K, 0, 1, L, G};   // (the table | the workgroups' lists; the kernel's LDS: one_layout.h)
  uint32_t epoch = 0;
  if (int rc = one_buffer(ws, s, (1ull << 60) | ((uint64_t)K << 32) | ((uint64_t)G << 16) | (uint64_t)L, lay.handoff_bytes(), &epoch)) return rc;
  if (one_prof() && ws->w_one.ensure(256)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  OneArgs a;
  memcpy(a.qv, h_q, sizeof(a.qv)); a.cbT = ix->cbT; a.lut_g = ws->w_oneb.as<float>(); a.blk_off = blk_off; a.packed = packed; a.pos = pos;
  a.pos_to_id = nullptr;   // (positions out: the caller maps them through its host copy of the ids -- no dependent gather at the kernel's end)
  a.part = reinterpret_cast<u64*>(ws->w_oneb.as<char>() + lay.part_off()); a.out_ids = d_out_ids; a.out_dist = d_out_dist;
  a.epoch = epoch; a.err = err;
  a.prof = one_prof() ? ws->w_one.as<unsigned long long>() + 8 : nullptr;
  a.K = K; a.L = L; a.k = k; a.chunk_blocks = chunk_blocks; a.sentinel = sentinel;
  memcpy(&a.sentinel_bits, &sentinel, 4);
  timed_launch(ix, s, "pq_one", [&] { hipLaunchKernelGGL((pq_one_kernel<25>), dim3((unsigned)G), dim3(ONE_WG), lay.lds_bytes(), s, a); });
  HIP_TRY(hipGetLastError());
  ws->one_pending = false;
  return 0;
}

// Queries per chunk of the generic scan over `n_blocks` row blocks: a LUT per query, one list of L keys per (query, 4096-row
// chunk) -- the finest chunks pq_chunk may choose -- and, from k = 513 on, the keys the selection passes keep (bigk.h).
static int pq_queries_per_chunk(const freddy_gpu_index* ix, int64_t n_blocks, int k) {
  const size_t L = (size_t)std::min(2 * k, 1024), nchunk = (size_t)std::max<int64_t>(1, (n_blocks + 63) / 64);
  size_t per_query = sizeof(float) * (size_t)ix->m * ix->K + sizeof(u64) * nchunk * L;
  if (2 * k > 1024) per_query += sizeof(u64) * (size_t)((2 * k + 1024 - 1) / 1024) * 1024;
  const size_t n = ((size_t)ix->tune.lut_budget_mb << 20) / per_query;
  return (int)std::min<size_t>(std::max<size_t>(n, 1), (size_t)1 << 20);
}

static int pq_chunk(freddy_gpu_index* ix, hipStream_t s, const float* d_q, int Q, int k, float sentinel,
                    const int32_t* blk_off, const uint32_t* packed, const int32_t* pos, int64_t n_blocks,
                    int32_t* d_out_ids, float* d_out_dist) {
  Workspace* ws = workspace_for(ix, s);
  const int m = ix->m, K = ix->K;
  const int L = std::min(2 * k, 64 * 16);
  const size_t lutN = (size_t)m * K;
  // enough (query, chunk) workgroups to fill the chip, but chunks long enough to amortise
  // the 48 KiB LUT staging
  int chunk_blocks = 64;   // 4096 rows; longer chunks once there are enough (query, chunk) workgroups
  while ((n_blocks + chunk_blocks - 1) / chunk_blocks * (int64_t)Q > 4096 && chunk_blocks < 8192) chunk_blocks *= 2;
  const int nchunk = (int)std::max<int64_t>(1, (n_blocks + chunk_blocks - 1) / chunk_blocks);
  if (ws->w_lut.ensure(sizeof(float) * (size_t)Q * lutN) ||
      ws->w_part.ensure(sizeof(u64) * (size_t)Q * nchunk * L))   // (one list of L keys per (query, chunk): kernels.h adc_scan_kernel)
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  if (int rc = launch_lut(ix, s, d_q, nullptr, ws->w_lut.as<float>(), Q)) return rc;
  ScanArgs sa;
  sa.lut = ws->w_lut.as<float>(); sa.item_list = nullptr; sa.item_query = nullptr;
  sa.blk_off = blk_off; sa.packed = packed; sa.pos = pos; sa.part = ws->w_part.as<u64>();
  sa.cand_count = nullptr;
  sa.m = m; sa.K = K; sa.chunk_blocks = chunk_blocks; sa.nchunk = nchunk; sa.L = L;
  memcpy(&sa.sentinel_bits, &sentinel, 4);
  const MergeArgs ma = merge_args_flat(sa.part, Q, nchunk, L, k, sentinel, ix->ids, d_out_ids, d_out_dist);
  if (2 * k > 1024) return bigk_select_replay(ix, s, ws, sa, Q, ma, Q);   // (k > 512: bigk.h)
  if (int rc = launch_scan(ix, s, sa, Q)) return rc;
  return launch_merge(ix, s, ma);
}

// The chunks of a batch: through the cell-grouped scan of `view` (an IVF-shaped view of the rows), or view == NULL: the generic scan.
static int pq_batch(freddy_gpu_index* ix, freddy_gpu_index* view, hipStream_t s, const float* d_q, int Q, int k, float sentinel, const int32_t* blk_off,
                    const uint32_t* packed, const int32_t* pos, int64_t n_blocks, int32_t* d_oi, float* d_od) {
  return for_chunks(Q, view ? pq_fused_queries_per_chunk(ix, n_blocks) : pq_queries_per_chunk(ix, n_blocks, k), [&](int q0, int n) {
    const float* q = d_q + (size_t)q0 * ix->d;
    if (view) return pq_fused_chunk(ix, view, s, q, n, k, sentinel, d_oi + (size_t)q0 * k, d_od + (size_t)q0 * k);
    return pq_chunk(ix, s, q, n, k, sentinel, blk_off, packed, pos, n_blocks, d_oi + (size_t)q0 * k, d_od + (size_t)q0 * k);
  });
}

extern "C" int freddy_gpu_pq_search_dev(freddy_gpu_index_t* ix, const float* d_queries, int32_t Q, int32_t k,
                                        float sentinel, int32_t* d_out_ids, float* d_out_dist, void* hip_stream) {
  if (int rc = check_search_args(ix, KIND_PQ, d_queries, Q, k, d_out_ids, d_out_dist)) return rc;
  if (Q == 0) return FREDDY_OK;
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ix->stream;
  const bool fused_path = pq_use_fused(ix, Q, k);
  if (fused_path) if (int rc = pq_shadow_build(ix)) return rc;
  return pq_batch(ix, fused_path ? ix->pq_shadow : nullptr, s, d_queries, Q, k, sentinel, ix->blk_off, ix->packed, ix->pos, ix->n_blocks, d_out_ids, d_out_dist);
}

// "WHERE id IN (...)" over the flat PQ table: unknown ids vanish, duplicates collapse, order = table
// order; the rows' packed codes are gathered into a temporary one-list table (synchronises the stream).
static int pq_subset(freddy_gpu_index* ix, hipStream_t s, const int32_t* subset_ids, int64_t n_subset, const int32_t** blk_off,
                     const uint32_t** packed, const int32_t** pos, int64_t* n_blocks, int64_t* n_rows_out = nullptr) {
  Workspace* ws = workspace_for(ix, s);
  const std::vector<int32_t> rows = rows_of_ids(ix->h_ids, subset_ids, n_subset);
  const int n_rows = (int)rows.size();
  const int nb = (n_rows + 63) / 64;
  const int n_pad = nb * 64;
  const int32_t h_blk[2] = {0, nb};
  if (ws->w_sub_rows.ensure(sizeof(int32_t) * std::max(n_rows, 1)) ||
      ws->w_sub_packed.ensure(sizeof(uint32_t) * (size_t)std::max(nb, 1) * ix->M2 * 64) ||
      ws->w_sub_pos.ensure(sizeof(int32_t) * (size_t)std::max(n_pad, 1)) || ws->w_sub_blk.ensure(sizeof(int32_t) * 2))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  if (n_rows) HIP_TRY(hipMemcpyAsync(ws->w_sub_rows.p, rows.data(), sizeof(int32_t) * n_rows, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws->w_sub_blk.p, h_blk, sizeof(h_blk), hipMemcpyHostToDevice, s));
  if (n_pad) {
    timed_launch(ix, s, "gather_rows", [&] {
      hipLaunchKernelGGL(gather_rows_kernel, dim3((n_pad + WG - 1) / WG), dim3(WG), 0, s, ws->w_sub_rows.as<int32_t>(),
                         n_rows, ix->packed, ws->w_sub_packed.as<uint32_t>(), ws->w_sub_pos.as<int32_t>(), ix->M2, n_pad);
    });
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(s));  // rows / h_blk are stack/heap temporaries
  *blk_off = ws->w_sub_blk.as<int32_t>();
  *packed = ws->w_sub_packed.as<uint32_t>();
  *pos = ws->w_sub_pos.as<int32_t>();
  *n_blocks = nb;
  if (n_rows_out) *n_rows_out = n_rows;
  return 0;
}

// ---- the host-buffer call, stage by stage: pq_stage_in -> pq_call_rows -> pq_one_try, or pq_batch -> pq_stage_out ------------------
// Queries in, lists out through pinned staging that the kernels read and write themselves (mapped host memory): a handful of
// queries (in_place, stage_plan.h) are read where they are staged and their lists written straight back; larger batches cross PCIe
// once, by a copy kernel each way.  No hipMemcpyAsync in the stream (each one is an SDMA hop with its own latency).
struct PqCall {
  bool in_place;
  size_t n_out;
  const float* d_q;   // where the search reads the queries, and where it writes the lists
  int32_t* d_oi;
  float* d_od;
};
// the rows the call scans: the table's, or the gathered rows of an "id IN (...)" subset; view: their IVF-shaped view if the batch takes the cell-grouped scan
struct PqRows {
  const int32_t* blk_off;
  const uint32_t* packed;
  const int32_t* pos;
  int64_t n_blocks, n_rows;
  freddy_gpu_index* view;
};

// queries == NULL (a source of table rows): their row numbers are staged where the floats would be and a gather fills the query block;
// ONE such query is read where its row lies, with room for its floats behind the number, for the one-launch kernel
static int pq_stage_in(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, const QuerySrc& qs, int Q, int k, PqCall& c) {
  const float* const queries = qs.host;
  const size_t q_bytes = sizeof(float) * (size_t)Q * ix->d;
  c.n_out = (size_t)Q * k;
  if (ix->hio_in.ensure(queries ? q_bytes + 16 : Q == 1 ? 16 + q_bytes : sizeof(int32_t) * (size_t)Q) || ix->hio_out.ensure(HioOut::bytes(c.n_out))) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
  if (queries) memcpy(ix->hio_in.p, queries, q_bytes);
  else memcpy(ix->hio_in.p, qs.rows, sizeof(int32_t) * (size_t)Q);
  c.in_place = Q <= IN_PLACE_QUERIES;
  if (!c.in_place && (ws->w_q.ensure(q_bytes + 16) || ws->w_out_ids.ensure(sizeof(int32_t) * c.n_out) || ws->w_out_dist.ensure(sizeof(float) * c.n_out)))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  const HioOut out(ix->hio_out.p, c.n_out);
  c.d_q = ix->hio_in.as<const float>(); c.d_oi = out.ids; c.d_od = out.dist;
  if (!queries) {
    if (Q == 1) {
      c.d_q = qs.row_ptr(0, ix->d);
    } else {
      if (c.in_place && ws->w_q.ensure(q_bytes + 16)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
      if (int rc = launch_query_gather(ix, s, qs, ix->hio_in.as<const int32_t>(), ws->w_q.as<float>(), Q, ix->d)) return rc;
      c.d_q = ws->w_q.as<float>();
    }
  }
  if (!c.in_place) {
    if (queries) {
      launch_copy_in(s, ix->hio_in.p, ws->w_q.p, 0, (q_bytes + 15) / 16);
      HIP_TRY(hipGetLastError());
    }
    c.d_q = ws->w_q.as<float>(); c.d_oi = ws->w_out_ids.as<int32_t>(); c.d_od = ws->w_out_dist.as<float>();
  }
  return 0;
}

static int pq_call_rows(freddy_gpu_index* ix, hipStream_t s, int Q, int k, const int32_t* subset_ids, int64_t n_subset, PqRows& t) {
  t = PqRows{ix->blk_off, ix->packed, ix->pos, ix->n_blocks, ix->N, nullptr};
  if (subset_ids)
    if (int rc = pq_subset(ix, s, subset_ids, n_subset, &t.blk_off, &t.packed, &t.pos, &t.n_blocks, &t.n_rows)) return rc;
  // (a subset of at least one full pseudo-list: its gathered rows get a view of their own, refreshed on this stream)
  const bool fused_path = pq_use_fused(ix, Q, k) && (!subset_ids || t.n_blocks >= FUSED_UNIT_BLOCKS);
  if (fused_path && !subset_ids) if (int rc = pq_shadow_build(ix)) return rc;
  if (fused_path && subset_ids) if (int rc = pq_view_refresh(ix, &ix->pq_sub_view, s, t.packed, t.pos, t.n_blocks, t.n_rows)) return rc;
  t.view = !fused_path ? nullptr : subset_ids ? ix->pq_sub_view : ix->pq_shadow;
  return 0;
}

// ONE query as one launch (pq_one; the caller has asked pq_one_shape): the kernel takes the query by value, so a device source's
// row is read back first, behind its staged number.  *answered: the lists are in the caller's buffers.
static int pq_one_try(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, const QuerySrc& qs, int k, float sentinel, const PqRows& t, const PqCall& c,
                      int32_t* out_ids, float* out_dist, bool* answered) {
  const HioOut out(ix->hio_out.p, c.n_out);
  *out.verdict = 0;
  const float* queries = qs.host;
  if (!queries) {
    float* const row_q = ix->hio_in.as<float>() + 4;
    if (int rc = fetch_query_row(s, qs, ix->d, row_q)) return rc;
    queries = row_q;
  }
  if (int rc = pq_one(ix, s, queries, k, sentinel, t.blk_off, t.packed, t.pos, t.n_blocks, c.d_oi, c.d_od, out.verdict)) return rc;
  int verdict = 0;
  if (int rc = one_finish(ix, ws, s, out.verdict, [](const unsigned long long* st) {
        fprintf(stderr, "[pq_one] wg0: slice %.2f barrier %.2f stage %.2f scan %.2f publish %.2f | last: since wg0 start %.2f merge %.2f replay %.2f us\n",
                (st[1] - st[0]) * 0.01, (st[2] - st[1]) * 0.01, (st[3] - st[2]) * 0.01, (st[4] - st[3]) * 0.01, (st[5] - st[4]) * 0.01,
                (st[8] - st[0]) * 0.01, (st[9] - st[8]) * 0.01, (st[10] - st[9]) * 0.01);
      }, &verdict))
    return rc;
  *answered = verdict == 2;
  if (*answered) {   // (positions out: mapped through the host copy of the ids)
    for (size_t i = 0; i < c.n_out; ++i) out_ids[i] = out.ids[i] >= 0 ? ix->h_ids[(size_t)out.ids[i]] : -1;
    memcpy(out_dist, out.dist, c.n_out * 4);
  }
  return 0;
}

static int pq_stage_out(freddy_gpu_index* ix, hipStream_t s, const PqCall& c, int32_t* out_ids, float* out_dist) {
  const HioOut out(ix->hio_out.p, c.n_out);
  if (!c.in_place) {
    hipLaunchKernelGGL(host_io_out_kernel, dim3((unsigned)((c.n_out + 255) / 256)), dim3(256), 0, s, c.d_oi, c.d_od, out.ids, (int)c.n_out);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(s));
  memcpy(out_ids, out.ids, c.n_out * 4);
  memcpy(out_dist, out.dist, c.n_out * 4);
  return 0;
}

// The host-buffer search for either query source (query_ids.h; the arguments are checked).
int pq_search_src(freddy_gpu_index* ix, const QuerySrc& qs, int Q, int k, float sentinel, const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids,
                  float* out_dist) {
  if (Q == 0) return FREDDY_OK;
  HIP_TRY(hipSetDevice(ix->device));
  Workspace* ws = workspace_for(ix, ix->stream);
  hipStream_t s = ix->stream;
  PqCall c;
  PqRows t;
  if (int rc = pq_stage_in(ix, ws, s, qs, Q, k, c)) return rc;
  if (int rc = pq_call_rows(ix, s, Q, k, subset_ids, n_subset, t)) return rc;
  if (!t.view && c.in_place && pq_one_shape(ix, Q, k, t.n_blocks)) {
    bool answered = false;
    if (int rc = pq_one_try(ix, ws, s, qs, k, sentinel, t, c, out_ids, out_dist, &answered)) return rc;
    if (answered) return FREDDY_OK;
  }
  if (int rc = pq_batch(ix, t.view, s, c.d_q, Q, k, sentinel, t.blk_off, t.packed, t.pos, t.n_blocks, c.d_oi, c.d_od)) return rc;
  return pq_stage_out(ix, s, c, out_ids, out_dist);
}

static int check_subset(const int32_t* subset_ids, int64_t n_subset) { return (n_subset < 0 || (n_subset > 0 && !subset_ids)) ? fail(FREDDY_E_ARG, "bad subset") : 0; }

extern "C" int freddy_gpu_pq_search(freddy_gpu_index_t* ix, const float* queries, int32_t Q, int32_t k, float sentinel,
                                    const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, float* out_dist) {
  if (int rc = check_search_args(ix, KIND_PQ, queries, Q, k, out_ids, out_dist)) return rc;
  if (int rc = check_subset(subset_ids, n_subset)) return rc;
  return pq_search_src(ix, QuerySrc::of_host(queries), Q, k, sentinel, subset_ids, n_subset, out_ids, out_dist);
}

extern "C" int freddy_gpu_pq_search_ids(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule, int32_t k,
                                        float sentinel, const int32_t* subset_ids, int64_t n_subset, int32_t* out_query_ids, int32_t* n_queries,
                                        int32_t* out_ids, float* out_dist) {
  if (int rc = check_query_ids_front(pq, vecs, query_ids, n_ids, id_rule, out_query_ids, n_queries, out_ids, out_dist)) return rc;
  if (int rc = check_list_count(n_ids, k)) return rc;
  if (int rc = check_list_limit(k)) return rc;
  if (int rc = check_subset(subset_ids, n_subset)) return rc;
  if (int rc = check_ann_vecs(pq, KIND_PQ, vecs, "a search by row id")) return rc;
  return search_selected_ids(vecs, query_ids, n_ids, id_rule, k, sentinel, out_query_ids, n_queries, out_ids, out_dist,
                             [&](const QuerySrc& qs, int n, int32_t* oi, float* od) { return pq_search_src(pq, qs, n, k, sentinel, subset_ids, n_subset, oi, od); });
}

// ---------------------------------------------------------------------------------------
// grouping_pq
// ---------------------------------------------------------------------------------------
extern "C" int freddy_gpu_grouping_pq(freddy_gpu_index_t* ix, const float* group_vectors, int32_t G, const int32_t* subset_ids,
                                      int64_t n_subset, int32_t* out_ids, int32_t* out_group, int64_t* n_out) {
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_PQ) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(ix)) return rc;
  if (G <= 0 || !group_vectors || !out_ids || !out_group || !n_out) return fail(FREDDY_E_ARG, "bad argument");
  if (int rc = check_subset(subset_ids, n_subset)) return rc;
  *n_out = 0;
  HIP_TRY(hipSetDevice(ix->device));
  Workspace* ws = workspace_for(ix, ix->stream);
  hipStream_t s = ix->stream;
  const int m = ix->m, K = ix->K, d = ix->d;
  const size_t lutN = (size_t)m * K;
  if (lutN * sizeof(float) > 160 * 1024) return fail(FREDDY_E_LIMIT, "m*K=%zu LUT entries exceed the 160 KiB of LDS", lutN);
  const int32_t* blk_off = ix->blk_off;
  const uint32_t* packed = ix->packed;
  const int32_t* pos = ix->pos;
  int64_t n_blocks = ix->n_blocks;
  if (subset_ids)
    if (int rc = pq_subset(ix, s, subset_ids, n_subset, &blk_off, &packed, &pos, &n_blocks)) return rc;
  (void)blk_off;
  if (n_blocks == 0) return FREDDY_OK;
  if (ws->w_q.ensure(sizeof(float) * (size_t)G * d) || ws->w_lut.ensure(sizeof(float) * (size_t)G * lutN) ||
      ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)n_blocks * 64))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  HIP_TRY(hipMemcpyAsync(ws->w_q.p, group_vectors, sizeof(float) * (size_t)G * d, hipMemcpyHostToDevice, s));
  if (int rc = launch_lut(ix, s, ws->w_q.as<float>(), nullptr, ws->w_lut.as<float>(), G)) return rc;   // freddy.c:1288-1299
  const dim3 grid((unsigned)((n_blocks + GROUP_BLOCKS - 1) / GROUP_BLOCKS));
  timed_launch(ix, s, "grouping", [&] {
    hipLaunchKernelGGL(grouping_kernel_for(ix->M2), grid, dim3(WG), lutN * sizeof(float), s, ws->w_lut.as<float>(), G, m, K, packed, (int)n_blocks, ws->w_out_ids.as<int32_t>());
  });
  HIP_TRY(hipGetLastError());
  std::vector<int32_t> h_grp((size_t)n_blocks * 64), h_pos((size_t)n_blocks * 64);
  HIP_TRY(hipMemcpyAsync(h_grp.data(), ws->w_out_ids.p, sizeof(int32_t) * h_grp.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h_pos.data(), pos, sizeof(int32_t) * h_pos.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  int64_t n = 0;
  for (size_t i = 0; i < h_pos.size(); ++i)
    if (h_pos[i] >= 0) { out_ids[n] = ix->h_ids[(size_t)h_pos[i]]; out_group[n] = h_grp[i]; ++n; }
  *n_out = n;
  return FREDDY_OK;
}

// ---------------------------------------------------------------------------------------
// the assignment step of cluster_pq (assign.h)
// ---------------------------------------------------------------------------------------
// Targets per pass (ids up, three state arrays) and the bytes of LUTs built at once: more queries than fit are walked in chunks,
// the kernel carrying every target's best between the launches.  The LUT buffer stays on the handle's workspace, so it is kept
// small: 64 MiB hold 5461 LUTs of the 300-d shape (m = 12, K = 256), 1365 at K = 1024.
static constexpr int64_t AS_PQ_PASS = (int64_t)1 << 22;
static constexpr size_t AS_PQ_LUT_BYTES = (size_t)64 << 20;

// LUTs built at a time for a call of Q queries (the size of the buffer pq_assign_pass is given)
int pq_assign_lut_queries(const freddy_gpu_index* ix, int Q) {
  const size_t lut_bytes = (size_t)ix->m * ix->K * sizeof(float);
  return (int)std::min<size_t>((size_t)Q, std::max<size_t>(1, AS_PQ_LUT_BYTES / lut_bytes));
}

// One pass of n targets with everything on the device: the queries, the target ids, the three state arrays and the LUT buffer of Qc
// LUTs (*lut_q0: the first query of the chunk whose LUTs it holds, -1 = none; kept between the passes of a call).  Enqueued on s;
// best / sim hold the result behind the last launch.  freddy_gpu_pq_assign and freddy_gpu_cluster (cluster.hip) both assign through it.
int pq_assign_pass(freddy_gpu_index* ix, hipStream_t s, float* d_lut, int Qc, int* lut_q0, const float* d_queries, int Q, float sentinel,
                   const int32_t* d_targets, int n, int32_t* d_best, float* d_sim, float* d_best_dist) {
  const int m = ix->m, K = ix->K, d = ix->d;
  const size_t lut_bytes = (size_t)m * K * sizeof(float);
  const int LT = (int)std::min<size_t>(8, std::max<size_t>(1, ((size_t)64 << 10) / lut_bytes));   // LUTs staged in LDS at a time
  // four targets per thread once that still gives every CU two workgroups: a staged LUT then serves 1024 targets
  const int RPT = assign_pq_rpt(ix->n_cus, n, AS_PQ_WG);
  const dim3 grid((unsigned)((n + RPT * AS_PQ_WG - 1) / (RPT * AS_PQ_WG)));
  for (int q0 = 0; q0 < Q; q0 += Qc) {
    const int nq = std::min(Qc, Q - q0);
    if (*lut_q0 != q0) {
      if (int rc = launch_lut(ix, s, d_queries + (size_t)q0 * d, nullptr, d_lut, nq)) return rc;   // freddy.c:1288-1299
      *lut_q0 = q0;
    }
    AssignPqArgs aa;
    aa.lut = d_lut; aa.targets = d_targets; aa.ids = ix->ids; aa.packed = ix->packed;
    aa.out_query = d_best; aa.out_sim = d_sim; aa.best_dist = d_best_dist;
    aa.N = ix->N; aa.n_targets = n; aa.q_base = q0; aa.nq = nq; aa.m = m; aa.K = K; aa.LT = LT; aa.first = q0 == 0 ? 1 : 0; aa.sentinel = sentinel;
    const size_t lds = (size_t)LT * lut_bytes;
    timed_launch(ix, s, "assign_pq_kernel", [&] { hipLaunchKernelGGL(assign_pq_kernel_for(ix->M2, RPT), grid, dim3(AS_PQ_WG), lds, s, aa); });
    HIP_TRY(hipGetLastError());
  }
  return FREDDY_OK;
}

extern "C" int freddy_gpu_pq_assign(freddy_gpu_index_t* ix, const float* queries, int32_t Q, float sentinel, const int32_t* target_ids,
                                    int64_t n_targets, int32_t* out_query, float* out_sim) {
  // (the scalar arguments first: they are checked before the handle is looked at, so no device is needed to see these errors)
  if (Q < 0 || n_targets < 0) return fail(FREDDY_E_ARG, "bad sizes (Q=%d, n_targets=%lld)", Q, (long long)n_targets);
  if (Q > 0 && n_targets > 0 && (!queries || !target_ids || !out_query || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  // (freddy_similarity.h is proven for distances below 2^24, and only distances below the sentinel reach it)
  if (!(sentinel <= 16777216.0f)) return fail(FREDDY_E_ARG, "sentinel=%g is not a number or above 2^24, the range the similarity of a distance is defined for", (double)sentinel);
  if (Q > AS_MAX_Q) return fail(FREDDY_E_LIMIT, "Q=%d exceeds this build's limit of %d queries per assign call", Q, AS_MAX_Q);
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_PQ) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(ix)) return rc;
  if (Q == 0 || n_targets == 0) return FREDDY_OK;
  HIP_TRY(hipSetDevice(ix->device));
  Workspace* ws = workspace_for(ix, ix->stream);
  hipStream_t s = ix->stream;
  const int d = ix->d;
  const size_t lut_bytes = (size_t)ix->m * ix->K * sizeof(float);
  const int Qc = pq_assign_lut_queries(ix, Q);
  const int64_t pass = std::min(AS_PQ_PASS, n_targets);
  if (ws->w_q.ensure(sizeof(float) * (size_t)Q * d) || ws->w_lut.ensure(lut_bytes * (size_t)Qc) || ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)pass) ||
      ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)pass) || ws->w_out_dist.ensure(sizeof(float) * (size_t)pass) ||
      ws->w_found.ensure(sizeof(float) * (size_t)pass))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  HIP_TRY(hipMemcpyAsync(ws->w_q.p, queries, sizeof(float) * (size_t)Q * d, hipMemcpyHostToDevice, s));
  int lut_q0 = -1;   // the chunk of queries whose LUTs are in w_lut
  for (int64_t t0 = 0; t0 < n_targets; t0 += pass) {
    const int n = (int)std::min(pass, n_targets - t0);
    HIP_TRY(hipMemcpyAsync(ws->w_sub_rows.p, target_ids + t0, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    if (int rc = pq_assign_pass(ix, s, ws->w_lut.as<float>(), Qc, &lut_q0, ws->w_q.as<float>(), Q, sentinel, ws->w_sub_rows.as<int32_t>(), n,
                                ws->w_out_ids.as<int32_t>(), ws->w_out_dist.as<float>(), ws->w_found.as<float>()))
      return rc;
    HIP_TRY(hipMemcpyAsync(out_query + t0, ws->w_out_ids.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_sim + t0, ws->w_out_dist.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));   // (the next pass overwrites the buffers)
  }
  return FREDDY_OK;
}

// The kernels of this unit that want more than the default 64 KiB of dynamic LDS.
std::vector<LdsLimit> lds_limits_pq() {
  std::vector<LdsLimit> l;
  for (int M2 : {6, 15, 0}) l.emplace_back(grouping_kernel_for(M2));
  // (LUTs staged up to 64 KiB, but at least one: up to 156 KiB for a table at the LUT limit)
  for (int M2 : {6, 0}) { l.emplace_back(assign_pq_kernel_for(M2, 4)); l.emplace_back(assign_pq_kernel_for(M2, 1)); }
  return l;
}
