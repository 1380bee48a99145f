// internal.h -- what the translation units of libfreddy_gpu.so share on the HOST side: the handle, its workspaces and
// options, error reporting, and the functions one unit calls in another.  The C ABI is include/freddy_gpu.h; the units:
//   core.hip    errors, options, workspaces, profiling records, unpin, counters
//   pin.hip     pin_pq / pin_ivf(_multi): table layouts, the codebook's tables, update_codebook; append_rows / remove_rows / update_rows (HBM index mutation:
//               mutate.h the entry points and one function per handle kind, mutate_host.h the staging owner and what else they share, block_plan.h lists ->
//               blocks in plain C++, mutate_kernels.h / remove_kernels.h / update_kernels.h the kernels)
//   ivfadc.hip  the IVFADC search chunk by chunk: the path a chunk takes, its probing rounds, the *_dev entry (launches nothing itself)
//   ivf_select.hip  cell selection: coarse distances (+ the query x codebook table), the probe plan
//   ivf_scan.hip    the cell-grouped scans and their merges: work table, filter + refine, the exact scan, the scan of other shapes
//   generic.hip     LUTs -> adc_scan -> merge_replay and the selection passes of k > 512: every shape's path, and what pq.hip launches of it
//   one.hip     ONE query of a host-buffer call as one launch (one.h): the hand-off buffer and the end of such a call, ivf_one (pq_one: pq.hip)
//   pipeline.hip    the host-buffer IVFADC calls: sub-batches on lanes over ivfadc.hip's chunk driver (stage_plan.h: the staging decisions in plain C++)
//   pq.hip      pq_search (+ subsets, pseudo-list batches, one-query launch), grouping_pq, the assignment step of cluster_pq
//               ivf_run.h what these share on the host: shape predicates and sizes, the query table's layout, the run state of a chain (no kernel
//               header: ivf_sizes.h has the constants); ivf_host.h adds the merge arguments for the units that launch
//               host_io.h the copy-in launch and the layout of the pinned result block, for pipeline.hip, one.hip and pq.hip
//   join.hip    pin_ivpq, knn_join (join.h: overview; join_kernels.h and join_traverse.h the kernels, join_host.h the host heap, join_run.h the run
//               record of a call and its stages)
//   exact.hip   pin_vectors, exact kNN and the exact join (also by row id: query_ids.h, resolve.h), the rows of an id set
//   analogy.hip the exact analogies (analogy.h), the INNER JOIN of analogy triples
//               exact_host.h what these two share on the host: the filter + refine chain and when a call takes it, scan chunking
//   rerank.hip  post verification of pq / ivf lists (pv.h), the approximate analogies over pq / ivf / ivpq (approx_analogy.h), the re-rank stage they share
//   cluster.hip exact_assign (assign.h), the whole k-means of cluster_exact / cluster_pq (cluster.h)
//   similarity.hip  similarities by row id: pairs, matrices, joins (similarity.h)
//   tokenize.hip    text vectors from token ids and the searches over them (tokenize.h)
//   build.hip   encode, insert_quantize, k-means
// Kernel headers are included by the unit that launches them (kernels shared by two units are static or templates).  A kernel with
// an LDS limit is compiled into ONE unit, whose lds_limits_*() names it: the limit belongs to that unit's copy of the function.
#pragma once
#include "../../include/freddy_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "hip_alloc.h"    // dev_malloc / dev_free / host_malloc / host_free: the only callers of the runtime's allocation functions
#include "join_index.h"
#include "pinned.h"
#include "grid_plan.h"   // the grids and path choices made from n_cus

using namespace freddy;

// ---- errors (core.hip) ----
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(e_ == hipErrorOutOfMemory ? FREDDY_E_NOMEM : FREDDY_E_HIP, "%s failed: %s (%s:%d)", #expr,   \
                  hipGetErrorString(e_), __FILE__, __LINE__);                               \
  } while (0)

enum { KIND_PQ = 1, KIND_IVF = 2, KIND_IVPQ = 3, KIND_VEC = 4 };

// Options.  Read from the environment ONCE, when an index is pinned (never on the search path); freddy_gpu_set_option
// changes them on a pinned index.  None of them changes a result: every setting gives the same lists.  The first group
// is for deployments, the second selects the alternative paths the tests compare with each other (every one of them has a
// GPU test), the third the self-checks.  (INTEGRATION.md lists them; timing experiments of earlier rounds are gone --
// profiles/HISTORY.md has their numbers.)
struct Tuning {
  // -- deployment
  int scan_share = 0;          // FREDDY_GPU_SCAN_SHARE (0 = auto: 1, or 2 for a host-buffer search that starts while another BACKEND is searching -- core.hip registry): the batches that share the chip with one of this handle's -- the batches the CALLER keeps
                               // in flight through the *_dev entry points (one stream each), or the other BACKENDS (processes) searching at
                               // the same time: a persistent scan takes n_cus / share CUs so that the scans run side by side.
                               // An explicit contract -- the library does not guess it; the host-buffer calls multiply it by their lane count
  int reserve_cus = 0;         // FREDDY_GPU_RESERVE_CUS: CUs the persistent scan leaves to the kernels of other streams (RCCL beside the scans)
  int scan_elastic = 0;        // FREDDY_GPU_SCAN_ELASTIC: a scan with scan_share > 1 brings EXTRA workgroups beyond its n_cus / share, which take work only while
                               // no other batch's scan is announced and fewer than the cap of scan workgroups are alive (ivf_scan.hip ivf_scan_filter, fused5.h):
                               // 0 off, 1 on, 2 = every extra leaves after its first entry (tests)
  int scan_elastic_reserve = 64;   // FREDDY_GPU_SCAN_ELASTIC_RESERVE: CUs the elastic scans together leave to the small kernels of the batches in flight
  int pipeline_batch = 2048;   // FREDDY_GPU_PIPELINE_BATCH: queries per sub-batch of the host-buffer pipeline (freddy_gpu_ivfadc_search)
  int pipeline_lanes = 4;      // FREDDY_GPU_PIPELINE_LANES: sub-batches in flight inside one host-buffer call (1..4)
  int lane0_own = 0;           // FREDDY_GPU_LANE0_OWN: 1 = the first pipeline lane on a stream of its own (until round 6) instead of the handle's stream
  int coarse_pieces = 1;       // FREDDY_GPU_COARSE_PIECES: a host-buffer call of ONE sub-batch launches its cell selection / table kernel per staged piece of the queries (0 = once, behind the last piece)
  int64_t lut_budget_mb = 8192;      // FREDDY_GPU_LUT_BUDGET_MB: per-call workspace cap (queries are chunked to fit); 288 GB of HBM: 8 GiB = 12 800 queries at nprobe 10
  // -- path selection (tests)
  int fused = -1;              // FREDDY_GPU_FUSED: -1 auto (cell-grouped scans for >= 256 items), 0 generic kernels, 1 always
  int scan_kernel = 5;         // FREDDY_GPU_FUSED_KERNEL: 5 filter + refine on int16 slabs (fused5.h), 3 the reference's arithmetic for every row (fused3.h)
  int coarse_approx = 1;       // FREDDY_GPU_COARSE_APPROX: cell selection as filter + refine (coarse.h); 0 = every distance exact
  int one_launch = 1;          // FREDDY_GPU_ONE_LAUNCH: a single query through the host-buffer calls as ONE launch (one.h) instead of a chain
  int pq_fused = -1;           // FREDDY_GPU_PQ_FUSED: batches over the flat PQ table through the cell-grouped filter + refine scan: -1 = from 16 queries on, 0 never, 1 always
  int sparse_items = 2;        // FREDDY_GPU_SPARSE_ITEMS: cells that at most this many queries of a batch probe are scanned item by item (sparse5.h) instead of as cell-grouped work entries (0 = never, < 0 = always for cells of up to that many items)
  int running_bound = 1;       // FREDDY_GPU_RUNNING_BOUND: the scan's entries share a per-query running bound of the k-th smallest cheap distance
                               // (FilterArgs::tau_run): fewer survivors for the merge; 0 = every (item, chunk) cuts at its own threshold
  int codes_u8 = 1;            // FREDDY_GPU_CODES_U8: K <= 256: the integer-slab scans read one byte per code (packed8, 16 instead of 28 B per row) -- 1: the scan with the whole entry's slab in LDS (fused8.h), 2: the six-phase scan (fused5.h); 0 = the int16 layout
  int exact_filter = -1;       // FREDDY_GPU_EXACT_FILTER: exact kNN as MFMA filter + exact refine (exact2.h): -1 auto (tables of >= 8192 rows, k <= 32), 0 never, 1 always
  int exact_join_tile = 0;     // option exact_join_tile: queries per workgroup of the exact join's filter (exact_join.h): 0 auto (128 when Q > 64 and d <= 320), 64
  int analogy_pass = 0;        // option analogy_pass: triples per pass of the approximate analogies (approx_analogy.h): 0 = pv_search's bound (lists of at most 8 M entries)
  int cluster_pass = 0;        // option cluster_pass: targets per assignment pass of freddy_gpu_cluster (cluster.h): 0 = 2^22; 64 at least
  int cluster_walk = 0;        // option cluster_walk: how cluster_sample_kernel finds a cluster's ranked members: 1 = it walks them from position 0 (what it does for kc > 1024), 2 = over the apply kernel's per-block counts (kc <= 1024), 0 = auto: 2 from n > 32768 on
  int exact_resolve = 0;       // option exact_resolve: how freddy_gpu_exact_search / _exact_join / _exact_analogy turn their id set into table rows: 0 = on the host (rows_of_ids), 1 = on the device (resolve.h); the *_ids forms always take the device
  int resolve_block = 0;       // option resolve_block: bitmap words per block of the device resolve (resolve.h): 0 = 256; tests make small tables span many blocks
  int tokenize_pass = 0;       // option tokenize_pass (set on the vector handle): texts per pass of the *_search_texts calls (tokenize.h): 0 = as many as a pinned block of 256 MiB holds
  int tokenize_unit = 0;       // option tokenize_unit: the sum of squares of freddy_gpu_tokenize's normalisation: 1 = a wave per text with lane 0 walking the chain (tok_unit_wave_kernel), 2 = a chain per lane over 64 texts (tok_unit_kernel), 0 = auto: 1 below 16384 texts, 2 from there on (tokenize.h)
  int64_t similarity_pass_bytes = 0;   // option similarity_pass_bytes: the device result block of one pass of freddy_gpu_similarity_matrix / _join (similarity.h): 0 = 256 MiB, at most 4 GiB; 16 rows of A at least
  // -- self-checks (tests): bit 0 = the scan keeps every row and the merge refines every row (every probed row's bracket is checked),
  //    bit 1 = the cell selection refines every cell, bit 2 = exact kNN refines every row
  int check_brackets = 0;
#ifdef FREDDY_LAB
  int scan_prof = 0;           // FREDDY_GPU_FUSED_PROF (lab builds only): per-phase cycle sums of the scan kernel on stderr
  int scan_fence = 0;          // option scan_fence (lab builds only; tools/lab/ablate.py): FilterArgs::fence -- parts of the scan kernel switched OFF (results wrong, time only)
#endif
};
int64_t env_int(const char* name, int64_t dflt);
int backends_other(bool searching, int device);   // core.hip: live backends (processes) besides this one with handles on the same PHYSICAL GPU as HIP device `device` (-1: on any) -- registered / inside a host-buffer search
void backend_handles(int delta, int device);   // +1 per pinned index of this process (on HIP device `device`), -1 when it is freed: registered while > 0
void backend_busy(int delta);         // this process enters (+1) / leaves (-1) a host-buffer search
void choose_hw_queues(int device);    // GPU_MAX_HW_QUEUES before the first HIP call (never overrides the environment)
struct BackendBusy { BackendBusy() { backend_busy(1); } ~BackendBusy() { backend_busy(-1); } };
// option scan_share as a number: the explicit value, or (0 = auto) 2 while another backend is searching, else 1
static inline int scan_share_now(int option, bool host_call, int device) { return option > 0 ? option : (host_call && backends_other(true, device) > 0 ? 2 : 1); }
Tuning read_tuning();

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) (void)dev_free(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    if (dev_malloc(&p, want) != hipSuccess) { p = nullptr; return -1; }
    cap = want;
    return 0;
  }
  void release() { if (p) (void)dev_free(p); p = nullptr; cap = 0; }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Everything a search writes besides its outputs.  Keyed by the stream the search is enqueued on, so that two
// batches in flight on two streams (the front end of batch i+1 beside the merge of batch i) never share scratch.
struct Workspace {
  bool used = false;
  hipStream_t owner = nullptr;
  uint64_t last_use = 0;           // claim order (the slot a new stream takes over is the least recently used one)
  DevBuf w_q, w_distT, w_used, w_item_cell, w_item_query, w_rows, w_resid, w_lut,
      w_part, w_cand, w_found, w_act0, w_act1, w_cnt, w_out_ids, w_out_dist, w_sub_rows,
      w_sub_packed, w_sub_pos, w_sub_blk, w_cellcnt, w_sorted, w_groups, w_surv, w_surv_cnt, w_prof, w_qc, w_qn, w_records, w_qn2, w_item_dist, w_tmin, w_one, w_oneb, w_bigsel, w_floor;
  uint64_t one_shape = 0;          // the one-launch kernels' buffer (w_oneb): shape of the call that wrote it last, and that call's epoch (one.h)
  uint32_t one_epoch = 0;
  bool one_pending = false;        // one_buffer() flipped the epoch and the kernel was not (yet) launched
  void release() {
    DevBuf* bufs[] = {&w_q, &w_distT, &w_used, &w_item_cell, &w_item_query, &w_rows, &w_resid, &w_lut, &w_part,
                      &w_cand, &w_found, &w_act0, &w_act1, &w_cnt, &w_out_ids, &w_out_dist, &w_sub_rows, &w_sub_packed,
                      &w_sub_pos, &w_sub_blk, &w_cellcnt, &w_sorted, &w_groups, &w_surv, &w_surv_cnt, &w_prof, &w_qc,
                      &w_qn, &w_records, &w_qn2, &w_item_dist, &w_tmin, &w_one, &w_oneb, &w_bigsel, &w_floor};
    for (DevBuf* b : bufs) b->release();
    used = false;
    owner = nullptr;
  }
};
static constexpr int FREDDY_MAX_WS = 12;

// One lane of the host-buffer pipeline (freddy_gpu_ivfadc_search): a library-owned stream, pinned staging for the
// queries going in and the lists coming out, device buffers, and the state of the sub-batch it has in flight.
// State of one chunk of queries while its probing rounds are enqueued.
struct IvfRun {
  freddy_gpu_index* ix;
  Workspace* ws;
  hipStream_t s;       // the stream the search is enqueued on
  int share;           // batches in flight on this handle (the scan takes n_cus / share CUs)
  const float* d_q;
  int Q, k, W, L, found_rule, upi;   // L = 2k: the KEEP count (exact keys that selection-then-replay keeps, every workspace size)
  int Lt;              // the threshold RANK: the order statistic of a cheap bound that becomes a cut (k)
  float sentinel, cell_limit;
  int32_t *d_out_ids, *d_status;
  float* d_out_dist;
  bool fused;          // cell-grouped scans (fused3.h / fused5.h / fused8.h) instead of lut_build + adc_scan
  int scan_kernel;     // 5: filter + refine, 3: exact fused scan
  bool tiled;          // batch coarse kernels (tiles of queries)
  bool zeroed;         // the coarse kernel has cleared the round-one scratch (ZeroArgs): no memsets in round one
  bool approx;         // cell selection as filter + refine: MFMA distances with a proven bracket, exact ones for the candidates
  bool records_ready;  // a batch over the flat PQ table: the entry records were written by pq_front_kernel (no work-table / record kernels)
  int merge_slices;    // > 0: the merge of such a batch as `merge_slices` partial merges per query + merge_replay_kernel
  bool running_bound;  // a query's entries share its running bound (FilterArgs::tau_run; option running_bound, IVFADC batches only)
  // per round
  int n_active, round;
  const int32_t* active;
  int32_t* next;
  bool first() const { return round == 0; }
};

struct LaneSlot {
  hipEvent_t done = nullptr;
  PinnedBuf h_in;          // queries of the sub-batch
  PinnedBuf h_out;         // [ids n*k][dist n*k][n_next][unfinished queries n][completion word]
  DevBuf d_q, d_ids, d_dist;
  bool busy = false;
  int q0 = 0, n = 0;
};
struct Lane {
  hipStream_t stream = nullptr;
  LaneSlot slot[2];        // two sub-batches queued per lane: the stream never runs dry while the host stages the next one
};
static constexpr int FREDDY_LANES = 4;

struct ProfRec {
  int64_t launches = 0;
  double ms = 0.0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> open;
};

struct freddy_gpu_index {
  int kind = 0;
  int device = 0;
  Tuning tune;
  hipStream_t stream = nullptr;
  int d = 0, m = 0, K = 0, C = 0, S = 0, M2 = 0;
  int64_t N = 0;
  int64_t n_blocks = 0;
  int max_list_blocks = 0;
  int64_t bytes = 0;
  int last_Q = 0;
  int n_cus = 256;              // what every CU-sized grid is planned with (grid_plan.h): device_cus, or less under option grid_cus
  int device_cus = 256;         // the device's count (open_device)
  // pinned tables
  float* coarse = nullptr;      // [C][d]
  float* coarseT = nullptr;     // [d][Cpad] for the coarse-distance kernel
  float* coarseP = nullptr;     // centroids in MFMA fragment order [Cpad/32][dp/8][64][4], zero padded (coarse.h)
  void* coarseH = nullptr;      // the centroids split into f16 hi / lo, [Cpad/32][T][2][64][8] (coarse_approx16_body)
  int coarse_ec = 0;            // their power-of-two scale
  float* cn2 = nullptr;         // [Cpad] |c_j|^2
  float cmax = 0.0f;            // max_j |c_j|, rounded up
  int dp = 0;
  int Cpad = 0;
  float* cbT = nullptr;         // [m][S][K]
  float* cbP = nullptr;         // fused kernel layout [m][SP/4][512 slots][4 dims][2 codes] (NULL unless K <= 1024)
  // filter + refine path (refine.h); NULL unless the shape is the fused one and the table fits the budget
  float* cbR = nullptr;         // [m][K][S] row-major codebook for the exact stage
  float* rterm = nullptr;       // [blocks*64] sum_p (|c|^2 + 2 co_p . c) of every row
  int64_t rterm_bytes = 0;      // its share of `bytes` (refresh_row_terms)
  float* pmax = nullptr;        // [m]        max |co_p| + max |c_p|, rounded up
  float* cmaxp = nullptr;       // [m]        max |c_p|, rounded up
  float* cbF = nullptr;         // [m][8 groups][8 tiles][hi / lo][64 lanes][8 halves] the codebook scaled by 2^ecb[p] and split into f16 hi / lo, in the B-fragment
                                // order of the table kernel's matrix instructions, then int32 ecb[m] (cbf_floats; fused5.h query_codebook5_body)
  int32_t* viol = nullptr;      // [4] self-check counters: scan bracket violations / rows checked, coarse bracket violations / cells checked
  int32_t* elastic = nullptr;   // [4] the elastic scan's advisory words (IVF handles; a 64-byte line of viol's allocation): scan workgroups alive over all
                                // streams, guaranteed workgroups announced and not yet started, extras that took work, extras that left for another scan
  int32_t* blk_cell = nullptr;  // [blocks]   list of every row block
  int32_t* list_off = nullptr;  // [lists+1] rows
  int32_t* blk_off = nullptr;   // [lists+1] row blocks
  uint32_t* packed = nullptr;   // [blocks][M2][64]
  uint32_t* packed8 = nullptr;  // K <= 256, m = 12: [blocks][3][64], one BYTE per code -- what the integer-slab scans read (16 B per row with its row term)
  int64_t packed8_bytes = 0;    // its share of `bytes`
  bool packed8_own = false;     // (a PQ handle's view shares its owner's array)
  int32_t* pos = nullptr;       // [blocks*64]
  int32_t* ids = nullptr;       // PQ: [N] position -> id
  std::vector<int32_t> h_ids;   // PQ: ascending ids for "id IN (...)" resolution
  std::vector<int32_t> h_list_off;
  std::vector<float> h_coarse;  // IVF: [C][d], kept for the norm bounds of a replaced codebook
  int32_t max_id = -1;          // largest row id pinned (appended rows must be larger)
  // raw vectors (exact kNN): 64-row blocks [block][d][64]
  float* xb = nullptr;
  // exact kNN as filter + refine (exact2.h): the table's statistics (pin time / append) and the per-call buffers
  bool exf_ok = false;          // every element finite, d % 4 == 0, d <= 512
  bool exf_never = false;       // the statistics were once taken with option exact_filter = 0: rows are missing from them, the filter stays off for good
  bool exf_dirty = true;        // no filter + refine call has completed yet, or the last one failed part-way: its device-side words are cleared before the next
  float exf_xnorm = 0.0f;       // largest row norm, rounded up
  int exf_ex = 0;               // power-of-two scale of the rows for the f16 split
  DevBuf exf_qfrag, exf_small, exf_sample, exf_cand;
  DevBuf exf_xf;                // the rows in MFMA A-fragment order, scaled and split into f16 hi / lo (exf_layout_kernel)
  int64_t exf_xf_strips = 0;    // 32-row strips laid out (capacity is exf_xf.cap)
  // ivpq extras
  JoinIndex join;
  // flat PQ table through the cell-grouped scan (pq_shadow_build): an IVF-shaped view of this table -- pseudo-lists of
  // 4096 consecutive rows, zero centroids -- that shares packed / codebook tables with its owner
  freddy_gpu_index* pq_shadow = nullptr;
  freddy_gpu_index* pq_sub_view = nullptr; // the same for the rows of an "id IN (...)" subset, refreshed by every such call
  freddy_gpu_index* shadow_of = nullptr;   // set in the shadow: profile records and shared arrays belong to this index
  DevBuf v_coarse, v_list_off, v_blk_off, v_blk_cell, v_pos, v_rterm;   // a shadow's own arrays (grown on demand)
  // workspaces: one per stream the caller searches on (searches on different streams may overlap)
  Workspace ws[FREDDY_MAX_WS];
  Workspace* last_ws = nullptr;   // of the most recent search (freddy_gpu_last_* read its counters)
  uint64_t ws_clock = 0;
  std::mutex mu;                  // guards the workspace slots and the profile map (host threads on different streams)
  // host-buffer pipeline (created by the first host-buffer IVFADC call)
  Lane lanes[FREDDY_LANES];
  // pinned staging of the other synchronous host-buffer calls (pq_search): queries in, lists out -- read / written by
  // kernels, no SDMA copies in the stream
  PinnedBuf hio_in, hio_out;
  // replicas of this index on further devices (freddy_gpu_pin_ivf_multi): a host batch is split contiguously over
  // this handle and its replicas; every replica is a complete pinned index of its own
  std::vector<freddy_gpu_index*> replicas;
  // set when a mutation (append_rows / remove_rows / update_rows / update_codebook / set_option) failed after it had already changed some of the devices
  // behind this handle: the replicas no longer hold the same tables, so every search fails loudly until the handle is unpinned
  bool registered = false;        // counted in the registry of backends (core.hip backend_handles)
  bool poisoned = false;
  bool one_launch_failed = false;   // pq_one_kernel once ran out of its bounded polls on this handle: three launches from then on
  // profiling
  bool profiling = false;
  std::map<std::string, ProfRec> prof;
  // the last exact analogy call (freddy_gpu_last_analogy_stats): filter passes, candidates they refined, passes redone all-exact
  int64_t an_stats[3] = {0, 0, 0};
  // the last exact join call (freddy_gpu_last_exact_join_stats): queries the filter answered for, candidates refined, queries redone all-exact
  int64_t exj_stats[3] = {0, 0, 0};
  // post verification on a pq / ivf handle (pv.h): pinned block [stage one's lists][the re-ranked lists][per-query counts] of one pass of
  // queries, the device copy of the queries, and the last call's counts (freddy_gpu_last_pv_stats): candidates, candidates with a row
  PinnedBuf pv_io;
  DevBuf pv_q;
  int64_t pv_stats[2] = {0, 0};
  // the last approximate-analogy call on a pq / ivf handle (freddy_gpu_last_approx_analogy_stats; it shares pv_io / pv_q): triples
  // searched, their candidates, candidates scored
  int64_t aa_stats[3] = {0, 0, 0};
  // text vectors on a vector handle (tokenize.h): the texts of a call on the device ([offsets][ids][rows][counts]), the centroids in
  // front of the normalisation, the vectors of freddy_gpu_tokenize, and the pinned block of one pass of the *_search_texts calls
  // ([the pass's vectors][their texts]) -- buffers of their own, because the searches of a pass run on this handle's workspace
  DevBuf tok_dev, tok_raw, tok_vec;
  PinnedBuf tok_io;
};

template <class F>
static inline void timed_launch(freddy_gpu_index* ix, hipStream_t s, const char* name, F&& f) {
  if (ix->shadow_of) ix = ix->shadow_of;
  if (!ix->profiling) { f(); return; }
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  (void)hipEventRecord(a, s);
  f();
  (void)hipEventRecord(b, s);
  std::lock_guard<std::mutex> lock(ix->mu);
  ProfRec& r = ix->prof[name];
  r.launches++;
  r.open.emplace_back(a, b);
}

// The workspace of the stream a search is enqueued on (core.hip).
Workspace* workspace_for(freddy_gpu_index* ix, hipStream_t s);

// The footprint rule: a device array of n elements occupies, and counts in index_bytes as, one element at least.
template <class T>
static inline int64_t counted_bytes(size_t n) { return (int64_t)(sizeof(T) * std::max<size_t>(n, 1)); }
template <class T>
static int upload(T** dst, const T* src, size_t n, int64_t* bytes) {
  *dst = nullptr;
  const size_t sz = (size_t)counted_bytes<T>(n);
  if (dev_malloc((void**)dst, sz) != hipSuccess) return -1;
  if (n && hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice) != hipSuccess) return -2;
  if (bytes) *bytes += (int64_t)sz;
  return 0;
}

void free_index(freddy_gpu_index* ix);
int refuse_poisoned(const freddy_gpu_index* ix);   // != 0 (FREDDY_E_HIP, "unpin it and pin again"): a mutation failed part-way on this handle; every entry point that reads its tables asks first
int check_search_args(const freddy_gpu_index* ix, int kind, const void* q, int Q, int k, const void* oi, const void* od);
// The scalar refusals the search entry points share, each with its one message: check_search_args and check_ivfadc_args are made of
// them, and so are the entry points that check their scalars before they look at a handle (post verification, the approximate
// analogies, the searches by row id).
static inline int check_list_count(int Q, int k) { return (Q < 0 || k <= 0) ? fail(FREDDY_E_ARG, "Q must be >= 0 and k > 0") : 0; }
static inline int check_list_limit(int k) { return k > 4096 ? fail(FREDDY_E_LIMIT, "k=%d exceeds this build's limit of 4096", k) : 0; }
// a raw-vector handle that a call reads: there, of that kind, not poisoned
static inline int check_vec_handle(const freddy_gpu_index* ix) {
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  return refuse_poisoned(ix);
}
// the id set of the calls that pass one on to a search of their own (post verification, the approximate analogies, the searches by texts)
static inline int pv_check_subset(const int32_t* subset_ids, int64_t n_subset) {
  return (n_subset < 0 || (n_subset > 0 && !subset_ids)) ? fail(FREDDY_E_ARG, "bad subset (n_subset=%lld)", (long long)n_subset) : 0;
}
static inline int check_probe_args(int W, int found_rule) {
  if (W <= 0) return fail(FREDDY_E_ARG, "W must be positive");
  if (found_rule < 0 || found_rule > 2 || (found_rule == FREDDY_FOUND_BATCH_UDF && W != 1))
    return fail(FREDDY_E_ARG, "bad found_rule (FREDDY_FOUND_BATCH_UDF needs W == 1)");
  return 0;
}

// ids -> rows of a table with ascending ids (h_ids): the row of one id (-1: absent), and the rows of "id IN (...)" -- unknown
// ids vanish, duplicates collapse, order = table order
static inline int32_t row_of(const std::vector<int32_t>& h_ids, int32_t id) {
  auto it = std::lower_bound(h_ids.begin(), h_ids.end(), id);
  return it != h_ids.end() && *it == id ? (int32_t)(it - h_ids.begin()) : -1;
}
// (row: the lookup, row_of or row_of_near)
template <class F>
static inline std::vector<int32_t> rows_of_ids_by(F&& row, const std::vector<int32_t>& h_ids, const int32_t* ids, int64_t n) {
  std::vector<int32_t> rows;
  rows.reserve((size_t)n);
  for (int64_t i = 0; i < n; ++i)
    if (const int32_t r = row(h_ids, ids[i]); r >= 0) rows.push_back(r);
  std::sort(rows.begin(), rows.end());
  rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
  return rows;
}
static inline std::vector<int32_t> rows_of_ids(const std::vector<int32_t>& h_ids, const int32_t* ids, int64_t n) { return rows_of_ids_by(row_of, h_ids, ids, n); }
// row_of for a table whose ids are serial or nearly so (google_vecs_norm: 1 .. N, less the rows a DELETE took).  Strictly ascending
// integers give h_ids[r] >= h_ids[0] + r, so the row of `id` is at most id - h_ids[0]: the search gallops DOWN from there (1, 2, 4 ...
// rows) and bisects the last step.  Serial ids: the first probe hits.  g rows missing below the id: about 2 log2(g) probes, all within
// g rows of each other -- against log2(N) probes spread over the whole array, most of them cache misses at N = 3 M.  Ids far apart
// (3 r + 1): at most twice the probes of row_of.  The same result as row_of for every table.
static inline int32_t row_of_near(const std::vector<int32_t>& h_ids, int32_t id) {
  if (h_ids.empty() || id < h_ids.front() || id > h_ids.back()) return -1;
  const int64_t N = (int64_t)h_ids.size();
  int64_t hi = std::min<int64_t>(N - 1, (int64_t)id - h_ids.front());   // h_ids[hi] >= id
  if (h_ids[(size_t)hi] == id) return (int32_t)hi;
  int64_t lo = hi, step = 1;
  while (lo > 0 && h_ids[(size_t)lo] > id) { hi = lo; lo = std::max<int64_t>(0, lo - step); step *= 2; }   // h_ids[lo] <= id < h_ids[hi]
  auto it = std::lower_bound(h_ids.begin() + lo, h_ids.begin() + hi + 1, id);
  return *it == id ? (int32_t)(it - h_ids.begin()) : -1;
}

// ---- pin.hip ----
int open_device(freddy_gpu_index* ix, int device);
// Every unit lists its kernels that want more than the default 64 KiB of dynamic LDS; open_device raises the limits (a
// per-device function attribute) once per device.
struct LdsLimit {
  const void* kernel;
  int bytes;
  template <class K> LdsLimit(K* k, int b = 160 * 1024) : kernel(reinterpret_cast<const void*>(k)), bytes(b) {}
};
std::vector<LdsLimit> lds_limits_ivf_select();
std::vector<LdsLimit> lds_limits_ivf_scan();
std::vector<LdsLimit> lds_limits_generic();
std::vector<LdsLimit> lds_limits_pq();
std::vector<LdsLimit> lds_limits_join();
std::vector<LdsLimit> lds_limits_exact();
std::vector<LdsLimit> lds_limits_analogy();
std::vector<LdsLimit> lds_limits_rerank();

namespace freddy { struct PlanArgs; struct ScanArgs; struct MergeArgs; }

// ---- ivf_scan.hip ----
// The work table shared by both cell-grouped scans: per-cell item counts -> (<= 12 items of a cell, 4096-row
// chunk) entries, largest first.
struct WorkTable {
  size_t max_groups;
  int32_t *group_cell, *group_first, *group_cnt, *n_groups, *work_counter;
  // (item, chunk) units of the cells that few queries probe (sparse5.h); sp_cap = 0: none
  size_t sp_cap;
  int32_t *sp_cell, *sp_first, *sp_chunk, *n_sparse, *sp_counter;
  bool sp_pairs = false;   // units of up to two items (sparse5.h NI = 2)
};
// f(std::integral_constant<int, V>()) for a selection width of pick_V (1, 2, 4, 8, 16); false for any other V
template <class F>
static inline bool with_V(int V, F&& f) {
  switch (V) {
    case 1: f(std::integral_constant<int, 1>()); return true;
    case 2: f(std::integral_constant<int, 2>()); return true;
    case 4: f(std::integral_constant<int, 4>()); return true;
    case 8: f(std::integral_constant<int, 8>()); return true;
    case 16: f(std::integral_constant<int, 16>()); return true;
  }
  return false;
}

// ---- generic.hip ----
int pick_V(int L);
int launch_scan(freddy_gpu_index* ix, hipStream_t s, const ScanArgs& a, int n_items);
int launch_merge(freddy_gpu_index* ix, hipStream_t s, const MergeArgs& a);
int bigk_select_replay(freddy_gpu_index* ix, hipStream_t s, Workspace* ws, ScanArgs sa, int n_items, const MergeArgs& ma, int Q);
int launch_lut(freddy_gpu_index* ix, hipStream_t s, const float* vecs, const int32_t* item_cell, float* lut, int n_items,
               const float* coarse = nullptr, const int32_t* item_query = nullptr);
int ivf_scan_generic(IvfRun& r, const PlanArgs& pa);

// ---- ivf_scan.hip (the work table's record: above) ----
int ivf_work_table(IvfRun& r, WorkTable& wt);
int ivf_scan_filter(IvfRun& r, const PlanArgs& pa, const WorkTable& wt);
int ivf_scan_exact(IvfRun& r, const PlanArgs& pa, const WorkTable& wt);
int ivf_scan_multi(IvfRun& r, const PlanArgs& pa, const WorkTable& wt);

// ---- ivf_select.hip ----
bool ivf_coarse_by_pieces(const IvfRun& r);
int ivf_coarse(IvfRun& r, int q_lo = 0, int q_n = -1);
int ivf_plan(IvfRun& r, PlanArgs& pa);

// ---- ivfadc.hip ----
int ivfadc_begin(freddy_gpu_index* ix, hipStream_t s, int share, const float* d_q, int Q, int k, int W, float sentinel, int found_rule,
                 int32_t* d_out_ids, float* d_out_dist, int32_t* d_status, IvfRun& r, const std::function<int(int, int)>* stage = nullptr,
                 bool by_pieces = false);
int ivfadc_finish(IvfRun& r, int n_next);
int max_queries_per_chunk(const freddy_gpu_index* ix, int W, int k);

// ---- one.hip ----
int one_buffer(Workspace* ws, hipStream_t s, uint64_t shape, size_t bytes, uint32_t* epoch);
bool one_prof();   // FREDDY_GPU_ONE_PROF (read once per process): the one-launch kernels' stamps on stderr
int one_finish(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, volatile const int32_t* err,
               void (*print_stamps)(const unsigned long long* st), int* verdict);
bool ivf_one_shape(const freddy_gpu_index* ix, int Q, int k, int W, int found_rule);
int ivf_one(freddy_gpu_index* ix, const float* queries, int k, int W, float sentinel, int found_rule, int32_t* out_ids, float* out_dist, int* verdict);

// ---- pq.hip ----
int pq_shadow_build(freddy_gpu_index* ix);
// the assignment step of cluster_pq on device pointers (freddy_gpu_pq_assign and freddy_gpu_cluster share it)
int pq_assign_lut_queries(const freddy_gpu_index* ix, int Q);
int pq_assign_pass(freddy_gpu_index* ix, hipStream_t s, float* d_lut, int Qc, int* lut_q0, const float* d_queries, int Q, float sentinel,
                   const int32_t* d_targets, int n, int32_t* d_best, float* d_sim, float* d_best_dist);

// ---- exact.hip ----
int exf_table_stats(freddy_gpu_index* ix, int64_t r0, int64_t n, const std::vector<int32_t>* changed_strips = nullptr);
// Where the table rows of "id = ANY(set)" are: the host vector rows_of_ids made (every function then does exactly what it did
// before), or already in ws->w_sub_rows, `resident` of them, put there by resolve_ids_device -- the copy to the device is skipped.
// The buffer was sized for min(n_ids, N) >= resident rows before the resolve was launched, and DevBuf::ensure leaves a buffer
// that is large enough where it is: the consumers' own ensure() calls for `resident` rows do not move it.
struct RowSet {
  const std::vector<int32_t>* host = nullptr;
  int64_t resident = 0;
  static RowSet of_host(const std::vector<int32_t>& rows) { RowSet r; r.host = &rows; return r; }
  static RowSet on_device(int64_t n) { RowSet r; r.resident = n; return r; }
  int64_t size() const { return host ? (int64_t)host->size() : resident; }
};
// what exact kNN, the exact join and the exact analogies (analogy.hip) do with an id set
int resolve_row_set(freddy_gpu_index* ix, bool on_device, const int32_t* ids, int64_t n, std::vector<int32_t>* h_rows, RowSet* out);
int vec_subset(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, const RowSet& rows, const float** xb, const int32_t** pos, int64_t* n_rows,
               int64_t* n_blocks);

// ---- analogy.hip ----
// the triples of an analogy call that have rows (the exact analogies, and the approximate ones of rerank.hip)
void resolve_triples(const std::vector<int32_t>& h_ids, const int32_t* triples, int32_t Q, std::vector<int32_t>& live, std::vector<int32_t>& rows3,
                     std::vector<int32_t>* ids3 = nullptr);

template <class F>
static int over_replicas(freddy_gpu_index* ix, int Q, F&& fn) {
  const int G = 1 + (int)ix->replicas.size();
  if (G == 1 || Q < 2 * G) return fn(ix, 0, Q);
  std::vector<int> rcs((size_t)G, 0);
  std::vector<std::string> msgs((size_t)G);
  std::vector<std::thread> th;
  const int base = Q / G, rem = Q % G;
  auto bounds = [&](int g, int* lo, int* hi) { *lo = g * base + std::min(g, rem); *hi = *lo + base + (g < rem ? 1 : 0); };
  for (int g = 1; g < G; ++g)
    th.emplace_back([&, g] {
      int lo, hi;
      bounds(g, &lo, &hi);
      rcs[(size_t)g] = fn(ix->replicas[(size_t)g - 1], lo, hi);
      if (rcs[(size_t)g]) msgs[(size_t)g] = freddy_gpu_last_error();
    });
  int lo, hi;
  bounds(0, &lo, &hi);
  rcs[0] = fn(ix, lo, hi);
  if (rcs[0]) msgs[0] = freddy_gpu_last_error();
  for (std::thread& t : th) t.join();
  for (int g = 0; g < G; ++g)
    if (rcs[(size_t)g]) return fail(rcs[(size_t)g], "device %d: %s", g == 0 ? ix->device : ix->replicas[(size_t)g - 1]->device, msgs[(size_t)g].c_str());
  return 0;
}

