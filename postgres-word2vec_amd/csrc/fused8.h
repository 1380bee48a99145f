// fused8.h -- the filter + refine scan for K <= 256 (one byte per code: the reference's shipped default index shape,
// index_creation/config/ivfadc_config.json) with the WHOLE work entry's slab resident in LDS.
//
// ivf_filter5_kernel (fused5.h) walks an entry in six phases of two positions because a K = 1024 slab of twelve positions would be
// 384 KB: every phase is a barrier, the builders' stores share the LDS with the gatherers' reads, and the phase lasts as long as the
// slower of the two roles.  With K <= 256 twelve positions x two halves x 256 codes x 16 B are 96 KB -- the whole entry fits:
//
//   * the builders interleave the table words of ALL twelve positions for the entry's 16 items once, and they do it while the
//     gatherers are in the PREVIOUS entry's tail (column minima, thresholds, survivor pass: VALU work that needs no slab);
//   * the gatherers read a row's twelve positions back to back -- no barrier inside the main loop, nobody stores meanwhile
//     (tools/lab/ubench7.hip: 18.2 k instead of 20.0 k cycles per entry with random codes, 7.9 k instead of 10.4 k conflict-free);
//   * the thresholds (the k-th smallest column minimum per item: FilterArgs::Lt) are taken by the GATHERER waves, so the builders are free
//     for the whole tail; four barriers per entry instead of eight;
//   * the table kernel writes a COMPACT copy of the table beside the general one (qc8: 512 B per (query, position), dword s =
//     code s | code s + 128 << 16): a builder wave's load is 256 consecutive bytes, an entry's table words are 96 KB -- the
//     general layout's 2 KB rows, of which K = 256 uses a quarter, cost the builders as much as K = 1024 (measured: no gain).
//
// The gatherers' tail is the SAME text as ivf_filter5_kernel's (scan_tail5.inc, without that kernel's fence conditions), the
// thresholds scan_tail5.h's filter_threshold5.  Everything else is fused5.h's too: entry queue and records, row terms, the
// (row, item) sums as unsigned 16-bit fields with the
// biased table, s' = fma(scale, V, rterm) in the tail, thresholds tau' + E with the query's running bound, survivor regions,
// merge_refine_kernel.  The sums are the same integers, so the survivors and the lists are the same (tests: every K <= 256 index
// of the GPU suite takes this kernel by default; option codes_u8 = 2 selects fused5.h's one-byte instantiation, 0 the int16 layout).
#pragma once
#include "fused5.h"

namespace freddy {

static constexpr uint32_t SCAN8_HALFB = 256u * 16u;         // one plane: the values of 8 items for every code of a position
static constexpr uint32_t SCAN8_POSB = 2u * SCAN8_HALFB;    // one position: two planes (items 0-7, 8-15)
static constexpr uint32_t scan8_slab_bytes(int m) { return (uint32_t)m * SCAN8_POSB; }

// S1 for ONE item (every wave of the workgroup takes one: builders items 0-7, gatherers 8-15): tau' = the Lt-th smallest of the
// item's 64 column minima, lowered by the query's running bound, widened by E -> thr_s[i]; the column is re-armed.  (The same split
// in ivf_filter5_kernel, where the builders take two items each and the gatherers wait: measured, no gain -- 82.3 against 82.0 us.)
__device__ __forceinline__ void scan8_threshold(const FilterArgs& a, const int32_t* rec, uint32_t* colmin, uint32_t* thr_s, int i, int lane, uint32_t run) {
  uint32_t c = colmin[i * 64 + lane];
  c = wave_sort32(c);   // (order-preserving keys of the float column minima)
  uint32_t t = __shfl(c, a.Lt - 1, 64);
  if (lane == 0) thr_s[i] = filter_threshold5(a, rec, i, t, run);
  colmin[i * 64 + lane] = 0xffffffffu;
}

template <int M, bool CAND, bool PROF = false>   // PROF (lab builds): cycle sums of gatherer wave 0 per stage
__global__ __launch_bounds__(SPEC2_T) void ivf_filter8_kernel(FilterArgs a) {
  constexpr int G = SCAN5_G, RMAX = FUSED_RMAX, NG = SPEC2_NG;
  constexpr int NP = M / 2;             // position pairs
  constexpr uint32_t HROWB = 16, HALFB = SCAN8_HALFB, POSB = SCAN8_POSB;
  static_assert(M == 12 && G == 16 && SPEC2_NB == 8 && SPEC2_NG == 8, "layout");
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* slab = smem;                                                      // [M][2 halves][256][16 B]
  uint32_t* colmin = reinterpret_cast<uint32_t*>(smem + a.desc_offset);           // [16][64]
  uint32_t* thr_s = colmin + 16 * 64;                                             // [16]
  int32_t* dsc = reinterpret_cast<int32_t*>(smem + a.desc_offset + 4096 + 64);    // [2][REC_DW] entry records
  int32_t* gidq = dsc + 2 * REC_DW;
  float* rt_s = reinterpret_cast<float*>(gidq + 4);                                // [4096] row terms of the current entry (from B2 on: of the next)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool builder = wave < SPEC2_NB;
  const long long t_kernel = PROF ? clock64() : 0;
  const int K = a.K;
  const int n_work = a.n_groups[0];

  int cur = 0, ei = 0;
  // The first entry of a workgroup is its own number (the entries are ordered largest first: the grid takes the first gridDim.x of
  // them, one each); the work counter deals out the entries BEYOND those.  A workgroup so starts with ONE round trip -- its record
  // and the claim of its second entry together -- instead of two dependent atomics and then the record.
  if (tid == 0) { gidq[0] = (int)blockIdx.x; gidq[1] = (int)gridDim.x + atomicAdd(a.work_counter, 1); }
  if (tid < REC_DW) dsc[tid] = a.records[(size_t)blockIdx.x * REC_DW + tid];   // (before n_work is known: the grid never exceeds the records' capacity)
  for (int i = tid; i < 16 * 64; i += SPEC2_T) colmin[i] = 0xffffffffu;
  __syncthreads();
  if ((int)blockIdx.x >= n_work) return;

  if (builder) {
    // =====================================================================================
    // BUILDERS: a pair of waves per (position of the pair, half = 8 items), lane li of the pair <-> codes li and li + 128; six
    // passes (position pairs) build the whole entry's slab.  Two register sets of one pass each.
    // =====================================================================================
    const int hpos = (wave >> 1) & 1;
    const int half = wave >> 2;
    const int li = (wave & 1) * 64 + lane;
    const uint32_t qoff = (uint32_t)hpos * POSB + (uint32_t)half * HALFB + (uint32_t)li * HROWB;
    const uint32_t vq = (uint32_t)li * 4u + (uint32_t)hpos * 512u;
    typedef const char __attribute__((address_space(1))) * gptrc;
    typedef const uint32_t __attribute__((address_space(1))) * gptr1u;
    // ALL six passes' table words of an entry are requested at once (48 registers) -- for the next entry that is while the
    // gatherers read this one's slab, so that between the barriers only the LDS stores remain.  The words come from the COMPACT
    // copy of the table (query_codebook5_body, qc8): dword li of row (query, position) = code li | code li + 128 << 16 -- a
    // wave's load is 256 consecutive bytes
    uint32_t qw[NP][8];
#pragma unroll
    for (int s = 0; s < NP; ++s)
#pragma unroll
      for (int g = 0; g < 8; ++g) qw[s][g] = 0u;
    int qid[8];
    auto issue_all = [&](int nh) {   // position 2 pass + hpos of the half's 8 items, pass = 0 .. 5
      if (half >= nh) return;
#pragma unroll
      for (int pass = 0; pass < NP; ++pass) {
        uint32_t voff = vq + (uint32_t)pass * 1024u;
        asm volatile("" : "+v"(voff));
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const gptrc qb = (gptrc)(uintptr_t)a.qc8 + (size_t)(uint32_t)qid[u] * (size_t)(M * 512);
          qw[pass][u] = *(gptr1u)(qb + voff);
        }
      }
    };
    auto emit_all = [&](int nh) {
      if (half >= nh) return;
#pragma unroll
      for (int pass = 0; pass < NP; ++pass) {
        unsigned char* dp = slab + (uint32_t)pass * (2u * POSB) + qoff;
        const uint32_t (&w)[8] = qw[pass];
        // v_perm_b32: bytes 0-3 come from the second operand, 4-7 from the first
        const u4 lo = u4{__builtin_amdgcn_perm(w[1], w[0], 0x05040100u), __builtin_amdgcn_perm(w[3], w[2], 0x05040100u),
                         __builtin_amdgcn_perm(w[5], w[4], 0x05040100u), __builtin_amdgcn_perm(w[7], w[6], 0x05040100u)};
        const u4 hi = u4{__builtin_amdgcn_perm(w[1], w[0], 0x07060302u), __builtin_amdgcn_perm(w[3], w[2], 0x07060302u),
                         __builtin_amdgcn_perm(w[5], w[4], 0x07060302u), __builtin_amdgcn_perm(w[7], w[6], 0x07060302u)};
        if (li < K) *reinterpret_cast<u4*>(dp) = lo;
        if (li + 128 < K) *reinterpret_cast<u4*>(dp + 128u * HROWB) = hi;
      }
    };
    // (rc: the record in LDS, or in global memory -- the next entry's, which the other builder waves cannot see in LDS before B1)
    auto entry_queries = [&](const int32_t* rc) -> int {
#pragma unroll
      for (int u = 0; u < 8; ++u) qid[u] = __builtin_amdgcn_readfirstlane(rc[24 + half * 8 + u]);
      return (__builtin_amdgcn_readfirstlane(rc[1]) + 7) >> 3;
    };
    float rtv[RMAX];
    auto fetch_row_terms = [&](const int32_t* rc) {
      const int b0 = __builtin_amdgcn_readfirstlane(rc[3]), nbk = __builtin_amdgcn_readfirstlane(rc[4]);
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        const int bl = r * NG + wave;
        rtv[r] = a.rterm[(size_t)(uint32_t)(b0 + (bl < nbk - 1 ? bl : nbk - 1)) * 64u + (uint32_t)lane];
      }
    };
    auto stash_row_terms = [&]() {
#pragma unroll
      for (int r = 0; r < RMAX; ++r) rt_s[(r * NG + wave) * 64 + lane] = rtv[r];
    };
    {
      fetch_row_terms(dsc);
      const int nh0 = entry_queries(dsc);
      issue_all(nh0);
      emit_all(nh0);
      stash_row_terms();
    }
    lds_barrier();   // B0: slab and row terms of the first entry
    for (;;) {
      const int nb = cur ^ 1;
      const int ngid = __builtin_amdgcn_readfirstlane(gidq[(ei + 1) & 1]);
      const bool have_next = ngid < n_work;
      // while the gatherers read this entry's slab: the next entry's record into LDS, the entry after next claimed, and the next
      // entry's table words and row terms into registers
      int next_nh = 0;
      {
        int32_t rr0 = 0;
        int gid2 = 0;
        if (tid < REC_DW && have_next) rr0 = a.records[(size_t)ngid * REC_DW + tid];
        if (tid == 0) gid2 = (int)gridDim.x + atomicAdd(a.work_counter, 1);
        if (have_next) {
          const int32_t* grec = a.records + (size_t)ngid * REC_DW;
          next_nh = entry_queries(grec);
          issue_all(next_nh);
          fetch_row_terms(grec);
        }
        if (tid < REC_DW) {
          if (tid == 0) gidq[ei & 1] = gid2;
          dsc[nb * REC_DW + tid] = (tid == 6) ? (have_next ? 1 : -1) : rr0;
        }
      }
      lds_barrier();   // B1: this entry's slab is consumed; the next record is visible
      if (have_next) emit_all(next_nh);     // (LDS stores only: the words arrived during the gather)
      // the running bound of this wave's item (S1 below): requested before the barrier
      uint32_t run_b = 0u;
      const int cnt_b = __builtin_amdgcn_readfirstlane(dsc[cur * REC_DW + 1]);
      if (a.tau_run && wave < cnt_b) run_b = a.tau_run[(uint32_t)dsc[cur * REC_DW + 24 + wave]];
      lds_barrier();   // B2: the gatherers have this entry's row terms in registers, every column minimum is in
      if (wave < cnt_b) scan8_threshold(a, dsc + cur * REC_DW, colmin, thr_s, wave, lane, run_b);   // S1, item `wave`
      if (have_next) stash_row_terms();
      lds_barrier();   // B3
      lds_barrier();   // B4: the next entry's slab and row terms are complete
      if (!have_next) break;
      cur = nb;
      ++ei;
    }
  } else {
    // =====================================================================================
    // GATHERERS: lane <-> 8 rows x 16 items; a row's twelve positions back to back
    // =====================================================================================
    const int gw = wave - SPEC2_NB;
    uint32_t acc[G / 2][RMAX];
    uint32_t cwn[2][3];     // the code dwords of the coming entry's first two rows of this wave: requested an entry ahead
    auto prefetch_codes = [&](const int32_t* rc) {
      const int b0 = __builtin_amdgcn_readfirstlane(rc[3]), nbk = __builtin_amdgcn_readfirstlane(rc[4]);
      const uint32_t l4 = lane_byte4();
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int bl = r * NG + gw;
        const char* rowp = reinterpret_cast<const char*>(a.packed8) + (size_t)((uint32_t)(b0 + (bl < nbk - 1 ? bl : nbk - 1)) * (uint32_t)(M / 4)) * 256u;
#pragma unroll
        for (int t = 0; t < 3; ++t) cwn[r][t] = *reinterpret_cast<const uint32_t*>(rowp + t * 256 + l4);
      }
    };
    prefetch_codes(dsc);
    long long gt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gc = 0;
    auto gtick = [&](int slot) { if constexpr (PROF) { const long long t = clock64(); if (slot >= 0) gt[slot] += t - gc; gc = t; } };
    lds_barrier();   // B0
    if constexpr (PROF) { gt[7] = clock64() - t_kernel; }   // (the prologue: kernel start .. first slab ready)
    for (;;) {
      gtick(-1);
      const int32_t* rec = dsc + cur * REC_DW;
      const int cnt = __builtin_amdgcn_readfirstlane(rec[1]);
      const int chunk = __builtin_amdgcn_readfirstlane(rec[2]);
      const int blk0 = __builtin_amdgcn_readfirstlane(rec[3]);
      const int nblk = __builtin_amdgcn_readfirstlane(rec[4]);
      const int nrows = __builtin_amdgcn_readfirstlane(rec[5]);
      const int nq = (cnt + 7) >> 3;
      const int nb = cur ^ 1;
      const int rl_wave = (nblk - gw + NG - 1) / NG < 0 ? 0 : (nblk - gw + NG - 1) / NG;
      auto row_block = [&](int r) {
        const int bl = r * NG + gw;
        return (uint32_t)(blk0 + (bl < nblk - 1 ? bl : nblk - 1));
      };
      auto main_loop = [&](auto nqc, auto rlc) {
        constexpr int NQ = decltype(nqc)::value, RL = decltype(rlc)::value;
        constexpr int DEPTH = NQ == 1 ? 4 : 2;    // steps of one position pair in flight: 8 reads, 32 registers
        constexpr int NS = RL * NP;               // steps of the entry: (row, position pair)
        u4 va[DEPTH][2][NQ];
        uint32_t cw[3][3];                        // the code dwords of three rows in turn (a row's are requested two rows ahead)
        auto load_codes = [&](int r) {
          const uint32_t l4 = lane_byte4();
          const char* rowp = reinterpret_cast<const char*>(a.packed8) + (size_t)(row_block(r) * (uint32_t)(M / 4)) * 256u;
#pragma unroll
          for (int t = 0; t < 3; ++t) cw[r % 3][t] = *reinterpret_cast<const uint32_t*>(rowp + t * 256 + l4);
        };
        auto issue_step = [&](int i) {
          const int r = i / NP, pp = i % NP;
          const uint32_t w = cw[r % 3][pp >> 1];
          const uint32_t a0 = ((pp & 1) ? ((w >> 12) & 0xff0u) : ((w << 4) & 0xff0u)) + (uint32_t)(2 * pp) * POSB;
          const uint32_t a1 = ((pp & 1) ? ((w >> 20) & 0xff0u) : ((w >> 4) & 0xff0u)) + (uint32_t)(2 * pp + 1) * POSB;
#pragma unroll
          for (int q = 0; q < NQ; ++q) va[i % DEPTH][0][q] = *reinterpret_cast<const u4*>(slab + a0 + (uint32_t)q * HALFB);
#pragma unroll
          for (int q = 0; q < NQ; ++q) va[i % DEPTH][1][q] = *reinterpret_cast<const u4*>(slab + a1 + (uint32_t)q * HALFB);
        };
#pragma unroll
        for (int h = 0; h < G / 2; ++h)
#pragma unroll
          for (int r = 0; r < RMAX; ++r) acc[h][r] = 0u;
#pragma unroll
        for (int t = 0; t < 3; ++t) { cw[0][t] = cwn[0][t]; cw[1][t] = cwn[1][t]; }
#pragma unroll
        for (int i = 0; i < DEPTH - 1; ++i) if (i < NS) issue_step(i);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const int r = i / NP;
          if (i % NP == 0 && r + 2 < RL) load_codes(r + 2);
          if (i + DEPTH - 1 < NS) issue_step(i + DEPTH - 1);
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            const u4 x = va[i % DEPTH][0][q], y = va[i % DEPTH][1][q];
            acc[q * 4 + 0][r] = acc[q * 4 + 0][r] + x.x + y.x;   // (v_add3_u32: unsigned fields, fused5.h filt5_bias)
            acc[q * 4 + 1][r] = acc[q * 4 + 1][r] + x.y + y.y;
            acc[q * 4 + 2][r] = acc[q * 4 + 2][r] + x.z + y.z;
            acc[q * 4 + 3][r] = acc[q * 4 + 3][r] + x.w + y.w;
          }
          if (i + 1 < NS) __builtin_amdgcn_sched_barrier(0);
        }
      };
      dispatch_nq_rl(nq, rl_wave, main_loop);
      // the running bound of this wave's item (S1 below: gatherer wave gw takes item gw + 8): on its way during the column minima
      uint32_t run1 = 0u;
      if (a.tau_run) run1 = gw + NG < cnt ? a.tau_run[(uint32_t)rec[24 + gw + NG]] : 0u;
      gtick(0);
      lds_barrier();   // B1: the slab is free for the next entry
      gtick(1);
      // ---- tail (scan_tail5.inc): s' = fma(scale[item], V, rterm[row]) compared as floats; OFF is added for the survivors only
#define SCAN_TAIL5_FENCE 0u
#define SCAN_TAIL5_PART 1
#include "scan_tail5.inc"
#define SCAN_TAIL5_PART 2
#include "scan_tail5.inc"
      gtick(2);
      lds_barrier();   // B2: every wave's column minima are in
      gtick(3);
      // S1: the threshold tau' + E of item gw + 8 (the builder waves take items 0-7 at the same time)
      if (gw + NG < cnt) scan8_threshold(a, rec, colmin, thr_s, gw + NG, lane, run1);
      gtick(4);
      lds_barrier();   // B3: thresholds
      gtick(5);
#define SCAN_TAIL5_PART 3
#include "scan_tail5.inc"
#undef SCAN_TAIL5_FENCE
      const int next_ok = __builtin_amdgcn_readfirstlane(dsc[nb * REC_DW + 6]);
      if (next_ok > 0) prefetch_codes(dsc + nb * REC_DW);
      gtick(5);
      lds_barrier();   // B4
      gtick(5);
      if (next_ok < 0) break;
      cur = nb;
    }
    if (PROF && a.prof && gw == 0 && lane == 0) {
      // slots 0-5, per entry summed: gather, B1, column minima, B2, S1, B3 + S2 + B4; 6: the prologue; 7: the workgroup's whole life
      for (int i = 0; i < 6; ++i) a.prof[(size_t)blockIdx.x * 8 + i] = gt[i];
      a.prof[(size_t)blockIdx.x * 8 + 6] = gt[7];
      a.prof[(size_t)blockIdx.x * 8 + 7] = clock64() - t_kernel;
    }
  }
}

}  // namespace freddy
