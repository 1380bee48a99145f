// fused5.h -- the filter + refine scan (refine.h) with INTEGER slabs: one LDS access serves eight items, six
// phases instead of twelve.  (DESIGN.md 5.3c has the measurements.)
//
// What bounded the fp32-slab filter scan this one replaced in its main loop was the LDS pipe: per position 48 KB of fp32 slab are
// written (48 wave-level ds_write_b128) and gathered (8 waves x 8 rows x <= 3 ds_read_b128, a third of the read
// cycles being bank conflicts), 87 % of the phase (rocprofv3 SQ_LDS_IDX_ACTIVE / SQ_LDS_BANK_CONFLICT) -- and the
// cost of a gather is per ACCESS, not per byte (tools/lab/ubench6.hip).  Here a slab entry is the table's own 16-bit
// integer:
//
//   * the query x codebook table is quantised with ONE scale per query (not per (query, position)) to
//     |v| <= 2730, so that the sum over the 12 positions fits 16 bits and is EXACT: the gatherers add rows
//     with v_pk_add_u16 and a (row, item) sum is one 16-bit half of a register -- 64 sum registers for
//     16 items x 8 rows;
//   * a slab row is 16 items x 2 B = 32 B = two 16-byte halves of 8 items: ONE ds_read_b128 per (row, position)
//     for an entry of <= 8 items, two for 9..16 (fp32: one per 4 items).  Half h of row c sits at byte
//     32 c + 16 (h ^ bit 3 of c), so that first halves do not all share 8 of the 16 bank groups; the builders only
//     interleave the items' table words (v_perm_b32) -- no conversion, no multiplication;
//   * two positions fit one buffer (2 x 32 KB): SIX phases -- barriers -- per entry instead of twelve, and the
//     rows' code dword of a phase is exactly the two codes it needs;
//   * work entries hold up to 16 items (scan_common.h work_table_kernel, cost_mode 2);
//   * the floating-point value s' = fma(scale[item], V, rterm[row]) is formed in the tail, where the selection
//     needs it -- WITHOUT the item's constant OFF: the selection compares floats (a constant shift changes neither
//     the order nor tau' + E); OFF is added for the survivors only (s = s' + OFF > 0, the bits the merge expects).
//
// The bound (u = 2^-24, B and the reference's error as for the fp32 slabs; D exact, d the reference's binary32 value):
//   reference                                   |d - D|        <= 39 u B
//   rterm (fp64, rounded once)                                  <=  1 u B
//   per position: the dot product on f16-split operands (query_codebook5_body: three v_mfma_f32_16x16x32_f16 per tile), against
//                 T = |q_p| max|c_p| (Cauchy-Schwarz: sum_j |q_j c_j| <= |q_p||c| <= T).  In scaled units (x 2^eq, x 2^ecb: exact)
//                 every element is v = hi + lo + r, |lo| <= 2^-11 |v|, |r| <= 2^-22 |v| + 2^-25 (the 2^-25: f16 subnormals);
//                 the slice's and the position's largest elements are >= 2^9, so |q_p| >= 2^9 and max|c_p| >= 2^9.
//                   representation  sum |r_q c| + |q r_c|  <= (4 + 4) u T + 2 . 2^-25 . 5 . 2^-9 T   (sum_j |v_j| <= 5 |v|)
//                   dropped lo . lo                         <= 2^-22 T = 4 u T                              together <= 12.1 u T
//                   accumulation: binary32, the order inside an instruction unknown and round-to-nearest not assumed -- every
//                     nonzero addend (a product, exact: 22 bits; or the accumulator that comes in) costs one rounding of at most
//                     2 u times the sum of the magnitudes, and so does the result: lo . hi and hi . lo (magnitudes <= 2^-11 T
//                     each, 26 + 27 roundings) < 0.1 u T; hi . hi LAST, 25 products + the accumulator + the result = 27 roundings
//                     of <= (1 + 2^-9) T                  <= 54.2 u T
//                   the zero dimensions 25..31 add nothing; the rescaling by 2^-(eq + ecb) is exact
//                 dot product <= 66.4 u T, and quotient (two roundings) <= 68.4 u 2 T: <= 69 u 2|q_p| max|c_p| ; rint: <= 0.5 scale
//                 (the seven v_mfma_f32_16x16x4_f32 steps of rounds 4-6 were given 58 u; tests/test_table_split_cpu.py has the model)
//                 no clamping: 2 |q_p| max|c_p| <= 2730 scale by construction
//       summed over 12 positions                                <= 69 u B + 6 scale
//   the sum V itself: exact (integers below 2^15)
//   s' = fma(scale, V, rterm), s = s' + OFF: two roundings of values <= 3 B + E      <=  7 u B
//   residual's own rounding (as for the fp32 slabs)                         <=  2 u B
//   =>  |(s - OFF + |r|^2) - d| <= e = 118 u B + 6 scale;  the construction needs e <= E / 4.2 = 121.9 u B + 6.67 scale:
//   E = 512 u B + 28 scale stands   (typical: 2.0e-3 against 1.2e-3 of the fp32 slabs -- 13.7 instead of 11.8 survivors per item).
// Everything downstream (survivor regions, merge_refine_kernel with the same E, the self-check of the bracket on
// every refined row) is refine.h's.
// The gatherer waves' selection tail (column minima, survivor pass) is scan_tail5.inc, ONE text that this kernel and fused8.h's
// include in their bodies; the keys, the running bound, the thresholds and the main loop's dispatch are functions in scan_tail5.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "refine.h"
#include "coarse.h"
#include "scan_tail5.h"

namespace freddy {

// (FILT5_VMAX, filter_width5: refine.h, next to the merge that shares them)
static constexpr int SCAN5_G = 16;   // items per work entry
static constexpr int SCAN5_PROF_WGS = 1024;   // lab builds: workgroups the counters' buffer holds (two tables of 8 counters each)

// The table stores v + bias(p) >= 0 with sum_p bias(p) = 2^15 (m = 12: 2731 for the first eight positions, 2730 for the
// others): a (row, item) sum is then an UNSIGNED 16-bit field in [8, 65528] at every step, so two fields per register are
// added with plain 32-bit adds (v_add3_u32: two positions at once, no carry ever crosses the halves), and field ^ 0x8000 is
// the signed sum V in two's complement.
__host__ __device__ __forceinline__ constexpr int filt5_bias(int p, int m) { return FILT5_VMAX + (p < 32768 - FILT5_VMAX * m ? 1 : 0); }
// 4 x lane id, never hoisted or spilled (two instructions where it is used)
__device__ __forceinline__ uint32_t lane_byte4() {
  uint32_t x;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_lshlrev_b32 %0, 2, %0" : "=v"(x));
  return x;
}
typedef short s2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_add_i16(uint32_t x, uint32_t y) {   // v_pk_add_u16 (wrap-around: never reached)
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(s2v, x) + __builtin_bit_cast(s2v, y));
}

// The table: values rint(-2 q_p . c / scale[q]) clamped to +-2730, scale[q] = max_p 2 |q_p| max|c_p| / 2730 -- ONE per query;
// row (query, position) = 128 uint4, word j of uint4 s = codes 128 j + s (low half) and 128 j + s + 512 (high half).  Every workgroup (position p, 16
// queries) derives the scales of its queries itself (16 lanes per query, lane <-> position: the same fmaf chain and
// the same maximum in every workgroup); the workgroups of position 0 also write qn[q][p] = |q_p| (rounded up) and
// scale[q] for the record and merge kernels.
template <int S, int QT>
__device__ __forceinline__ void query_codebook5_body(const float* __restrict__ queries, const float* __restrict__ cbT,
                                                     const float* __restrict__ cmax, float* __restrict__ qn,
                                                     float* __restrict__ qscale, uint32_t* __restrict__ qc,
                                                     int Q, int d, int m, int K, int bx, int by, unsigned char* smem,
                                                     uint32_t* __restrict__ qc8 = nullptr) {
  // qc8 (K <= 256, fused8.h): a COMPACT copy of the table beside the general one -- row (query, position) = 128 dwords, dword s =
  // code s (low half) | code s + 128 (high half): 512 B instead of the 2 KB row of which K = 256 uses a quarter
  static_assert(QT == 16, "one 16-lane group per query");
  constexpr int SP = (S + 3) & ~3;
  // LDS from the caller: qs [QT][SP] floats, inv_s [QT]
  float (*qs)[SP] = reinterpret_cast<float (*)[SP]>(smem);
  float* inv_s = reinterpret_cast<float*>(smem + QT * SP * 4);
  const int tid = threadIdx.x, p = bx, q0 = by * QT;
  // MFMA path: the B operands of the wave's FIRST group of code slots are requested before anything else -- the codebook
  // round trip runs under the prologue (the workgroup is a chain of latencies: all 768 are resident at once); the second
  // group's are requested into the same registers right after the first group's matrix instructions, under its conversion
  static_assert(S <= 32 && SP % 4 == 0, "one k-step of v_mfma_f32_16x16x32_f16 covers a position");
  ch8v bh[8], bl[8];           // [tile 2 i + e]: codes 128 i + 16 g + col + 512 e, dimensions 8 kq .. 8 kq + 7 of lane (col, kq)
  auto load_b = [&](int g) {   // (cbT here = the f16 hi / lo fragment copy, pin.hip build_fragment_codebook)
    const ch8v* src = reinterpret_cast<const ch8v*>(cbT) + ((size_t)p * 8 + g) * (CBF_GROUP_HALVES / 8) + (tid & 63);
#pragma unroll
    for (int t = 0; t < 8; ++t) { bh[t] = src[(size_t)t * 128]; bl[t] = src[(size_t)t * 128 + 64]; }
  };
  load_b((tid >> 6) * 2);
  const int ecb = reinterpret_cast<const int*>(cbT)[cbf_exp_offset(m) + p];   // the position's power-of-two scale (uniform)
  for (int i = tid; i < QT * SP; i += 256) {
    const int qi = i / SP, j = i - qi * SP;
    qs[qi][j] = (j < S && q0 + qi < Q) ? queries[(size_t)(q0 + qi) * d + p * S + j] : 0.0f;
  }
  {
    const int qi = tid >> 4, pp = tid & 15, q = q0 + qi;
    float best = 0.0f;
    if (pp < m && q < Q) {
      float n2 = 0.0f;
      for (int j = 0; j < S; ++j) { const float v = queries[(size_t)q * d + pp * S + j]; n2 = __builtin_fmaf(v, v, n2); }
      const float nrm = __builtin_sqrtf(n2) * (1.0f + 1e-5f);
      if (p == 0) qn[(size_t)q * m + pp] = nrm;
      best = 2.0f * nrm * cmax[pp];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    if (pp == 0) {
      const float sc = q < Q ? best * (1.0f / (float)FILT5_VMAX) * (1.0f + 1e-6f) : 0.0f;
      inv_s[qi] = (sc > 0.0f && sc < 1e30f) ? 1.0f / sc : 0.0f;
      if (p == 0 && q < Q) qscale[q] = sc;
    }
  }
  {
    // The dot products on the matrix cores, ONE k-step per position (v_mfma_f32_16x16x32_f16: A = 16 queries x 32 dimensions,
    // B = 32 dimensions x 16 codes, S = 25 <= 32) on f16-split operands: the queries' slice times 2^eq (eq per (query, position):
    // the slice's largest finite element in [2^9, 2^10)) = hi + lo + rest, the codebook likewise at pin time (ecb per position), and
    // q . c ~ 2^-(eq + ecb) (lo . hi + hi . lo + hi . hi) -- three instructions per tile into one binary32 accumulator, the small
    // products first, instead of seven v_mfma_f32_16x16x4_f32 at a sixteenth of the rate (error: top of this file).  A wave takes
    // two groups of 16 code slots and, per group, the eight tiles whose codes share a slot's uint4 (code 128 i + slot, i = 0..3,
    // and its partner + 512) -- so a lane ends up with exactly the four words of one 16-byte store per query.
    // A[row = lane & 15][k = 8 (lane >> 4) + j], D[row = 4 (lane >> 4) + reg][col = lane & 15].
    typedef float f4v __attribute__((ext_vector_type(4)));
    __syncthreads();   // (qs, inv_s)
    const int wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int nq = (Q - q0 < QT) ? Q - q0 : QT;
    ch8v ah, al;
    int eq = 0;
    {
      // this lane's eight dimensions of query `col` (rows of qs are zero from S on; a row ends at SP)
      f4v x0 = f4v{0.0f, 0.0f, 0.0f, 0.0f}, x1 = x0;
      if (8 * kq < SP) x0 = *reinterpret_cast<const f4v*>(&qs[col][8 * kq]);
      if (8 * kq + 4 < SP) x1 = *reinterpret_cast<const f4v*>(&qs[col][8 * kq + 4]);
      const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
      // the slice's largest finite magnitude (fmaxf drops a NaN; with an infinity the scale stays 1 and the row is non-finite
      // whatever the other elements become); the four lanes of a query agree on it
      float am = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) am = fmaxf(am, __builtin_fabsf(x[j]));
      am = fmaxf(am, __shfl_xor(am, 16, 64));
      am = fmaxf(am, __shfl_xor(am, 32, 64));
      if (am > 0.0f && am < 3e38f) { (void)__builtin_frexpf(am, &eq); eq = CBF_EXP - eq; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = __builtin_ldexpf(x[j], eq);   // (exact: a power of two)
        const _Float16 hh = (_Float16)v;
        ah[j] = hh;
        al[j] = (_Float16)(v - (float)hh);
      }
    }
    // the exact power of two that undoes both scales, for the four queries (rows of D) this lane stores
    int unscale[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) unscale[reg] = -(__shfl(eq, 4 * kq + reg, 64) + ecb);
    const float vmax = (float)FILT5_VMAX;
    const int bias = filt5_bias(p, m);
#pragma unroll
    for (int gg = 0; gg < 2; ++gg) {
      const int g = wave * 2 + gg;
      f4v acc[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 2; ++e) acc[i][e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[2 * i + e], f4v{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 2; ++e) acc[i][e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[2 * i + e], acc[i][e], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 2; ++e) acc[i][e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[2 * i + e], acc[i][e], 0, 0, 0);
      if (gg == 0) load_b(g + 1);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int qi = 4 * kq + reg;
        if (qi < nq) {
          const float inv = inv_s[qi];
          uint32_t wd[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int i0 = (int)fminf(fmaxf(__builtin_rintf(-2.0f * __builtin_ldexpf(acc[i][0][reg], unscale[reg]) * inv), -vmax), vmax) + bias;
            const int i1 = (int)fminf(fmaxf(__builtin_rintf(-2.0f * __builtin_ldexpf(acc[i][1][reg], unscale[reg]) * inv), -vmax), vmax) + bias;
            wd[i] = (uint32_t)i0 | ((uint32_t)i1 << 16);
          }
          *reinterpret_cast<uint4*>(qc + ((size_t)(q0 + qi) * m + p) * 512 + 4 * (16 * g + col)) = uint4{wd[0], wd[1], wd[2], wd[3]};
          if (qc8) qc8[((size_t)(q0 + qi) * m + p) * 128 + (16 * g + col)] = (wd[0] & 0xffffu) | (wd[1] << 16);
        }
      }
    }
  }
}
// The kernels made of table units are held to four waves per SIMD (128 registers): left to itself the compiler spends 160 on the
// same code (the second group's B operands in registers of their own) -- three waves, and with four batches in flight the launch
// was 3-4 us longer for it (profiles/table_f16_ab.txt).  No spills, no scratch at 128.
#define FREDDY_TABLE_UNIT_KERNEL __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
template <int S, int QT>
static constexpr int query_codebook5_lds() { return QT * ((S + 3) & ~3) * 4 + QT * 4; }
template <int S, int QT>
FREDDY_TABLE_UNIT_KERNEL void query_codebook5_kernel(const float* __restrict__ queries, const float* __restrict__ cbT,
                                                             const float* __restrict__ cmax, float* __restrict__ qn,
                                                             float* __restrict__ qscale, uint32_t* __restrict__ qc,
                                                             int Q, int d, int m, int K, uint32_t* __restrict__ qc8) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[query_codebook5_lds<S, QT>()];
  query_codebook5_body<S, QT>(queries, cbT, cmax, qn, qscale, qc, Q, d, m, K, blockIdx.x, blockIdx.y, smem, qc8);
}

// The MFMA cell-selection distances (coarse.h) and the query x codebook table in ONE launch: the first `n_coarse`
// workgroups are coarse tiles, the others table units (position, 16 queries).  Neither depends on the other and both are a
// few tens of microseconds of small workgroups; as two kernels of a batch's chain they cost two launches, two
// dependencies (with batches in flight the table kernel runs in line: a side stream per batch collides with the other
// batches' streams in the hardware queues).  The workgroups keep their own shape and lifetime -- a version in which every
// workgroup did both jobs was 40 % slower with batches in flight (big workgroups that live long keep the scans of the
// other batches from finding CUs).
struct CoarseTableArgs {
  const float* queries;
  const float* coarseF; const float* cn2; float* dist; float* qn2; int Q, Cpad, d, dp; ZeroArgs z; int coarse_gx, coarse_gy;
  const float* cbT; const float* cmax; float* qn; float* qscale; uint32_t* qc; int m, K;
  float* tmin; int C;   // many cells: the (query, 128-cell tile) minima for the plan's two-level selection (NULL: not wanted)
  const ch8v* coarseH; int ec;   // many cells: the centroids split into f16 hi / lo (coarse_approx16_body); NULL: the fp32 tile
  uint32_t* qc8;                 // K <= 256: the compact copy of the table (query_codebook5_body); NULL: not wanted
};
template <int S, int QT, bool H16 = false>   // H16: the coarse tiles on f16-split operands (many cells); an instantiation of its own, so
FREDDY_TABLE_UNIT_KERNEL void coarse_table5_kernel(CoarseTableArgs a) {   // that the <= 1024-cell kernel compiles as before
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n_coarse = a.coarse_gx * a.coarse_gy;
  const int b = blockIdx.x;
  if (b < n_coarse) {
    if constexpr (H16)
      coarse_approx16_body(a.queries, a.coarseH, a.ec, a.cn2, a.dist, a.qn2, a.Q, a.Cpad, a.d, a.z, b % a.coarse_gx, b / a.coarse_gx,
                           a.coarse_gx, a.coarse_gy, smem, a.tmin, a.C);
    else
    coarse_approx_body(a.queries, a.coarseF, a.cn2, a.dist, a.qn2, a.Q, a.Cpad, a.d, a.dp, a.z, b % a.coarse_gx, b / a.coarse_gx,
                       a.coarse_gx, a.coarse_gy, smem, a.tmin, a.C);
  } else {
    const int t = b - n_coarse;
    query_codebook5_body<S, QT>(a.queries, a.cbT, a.cmax, a.qn, a.qscale, a.qc, a.Q, a.d, a.m, a.K, t % a.m, t / a.m, smem, a.qc8);
  }
}

// Entry records as entry_record_kernel; [128 + g] = the table scale of item g's query.
template <int M>
__global__ __launch_bounds__(256) void entry_record5_kernel(RecordArgs a) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  // the scan behind this launch, announced: the other scans' extra workgroups stop claiming entries (FilterArgs::elastic)
  if (a.elastic && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_fetch_add(a.elastic + EL_PENDING, a.n_announce, FREDDY_RLX_AGENT);
  if (e >= a.n_groups[0]) return;
  const int cell = a.group_cell[e], first = a.group_first[e], gc = a.group_cnt[e];
  const int cnt = gc & 0xff, chunk = gc >> 8;
  int32_t* rec = a.records + (size_t)e * REC_DW;
  if (lane == 0) {
    const int b0 = a.blk_off[cell] + chunk * FUSED_UNIT_BLOCKS;
    int nb = a.blk_off[cell + 1] - b0;
    if (nb > FUSED_UNIT_BLOCKS) nb = FUSED_UNIT_BLOCKS;
    int rows = a.list_off[cell + 1] - a.list_off[cell] - chunk * (FUSED_UNIT_BLOCKS * 64);
    if (rows > FUSED_UNIT_BLOCKS * 64) rows = FUSED_UNIT_BLOCKS * 64;
    rec[0] = cell; rec[1] = cnt; rec[2] = chunk; rec[3] = b0; rec[4] = nb; rec[5] = rows;
  }
  if (lane < 16) {
    const int it = lane < cnt ? a.sorted_item[first + lane] : -1;
    const int q = a.item_query[it >= 0 ? it : a.sorted_item[first]];
    const float sc = a.qscale[q];
    ItemBounds ib = item_bounds(0.0f, 0.0f, a.sentinel);
    if (it >= 0) ib = item_bounds(a.item_dist[it], filter_width5<M>(a.qn + (size_t)q * M, a.pmax, sc), a.sentinel);
    rec[8 + lane] = it;
    rec[24 + lane] = q;
    rec[40 + lane] = (int32_t)__float_as_uint(ib.off);
    rec[56 + lane] = (int32_t)__float_as_uint(ib.e);
    rec[72 + lane] = (int32_t)__float_as_uint(ib.shift);
    rec[88 + lane] = (int32_t)ib.lo_bits;
    rec[104 + lane] = (int32_t)ib.hi_bits;
    rec[128 + lane] = (int32_t)__float_as_uint((it >= 0 && sc < 1e30f) ? sc : 0.0f);
    // the item's coarse distance as an interval (item_bounds: relative error < 2e-5): what makes the cheap distances of
    // different cells comparable (running bound of the query, ivf_filter5_kernel S1); +inf / 0: no part in it
    const float A = it >= 0 ? a.item_dist[it] : -1.0f;
    const bool fin = it >= 0 && ib.e < 1e30f && A >= 0.0f && A < 1e30f;
    rec[144 + lane] = (int32_t)__float_as_uint(fin ? A * (1.0f + 2e-5f) : __uint_as_float(0x7f800000u));
    rec[160 + lane] = (int32_t)__float_as_uint(fin ? A * (1.0f - 2e-5f) : 0.0f);
  }
}

// ---------------------------------------------------------------------------------------
// The scan.  Roles, entry queue, records, row terms, thresholds and survivor regions as ivf_filter_kernel;
// phases j = 0 .. M/2 - 1 cover positions 2j and 2j + 1.
//   LDS: slab[2 buffers][2 positions][K][12] int16 = 96 KB, then colmin / thresholds / records / row terms.
// ---------------------------------------------------------------------------------------
// PROF: the per-phase cycle counters of option fused_prof (18 registers of a builder wave, 8 of a gatherer wave: an
// instantiation of its own, the production kernel does not carry them)
// U8: the rows' codes as one byte each (K <= 256: what the reference's shipped default indexes use) -- packed8[block][3][64],
// dword t of a row = its codes 4 t .. 4 t + 3: 12 instead of 24 bytes of codes per row, three code loads per row and entry
// instead of six (the dword of phases 2 t and 2 t + 1 is the same)
// ELASTIC: the scan with extra workgroups (FilterArgs::elastic) -- a kernel of its own, ivf_filter5_elastic_kernel: the extras'
// prologue alone, whatever form it took, moved the register allocation of the whole kernel (scalar spills 28 -> 35 in the builders'
// preamble), so ivf_filter5_kernel keeps the text and the code it had and a launch without extras runs exactly that
template <int M, bool FULLK, bool CAND, bool PROF, bool U8, bool ELASTIC>
__device__ __forceinline__ void ivf_filter5_body(const FilterArgs& a) {
  static_assert(!(U8 && FULLK), "one byte per code: K <= 256");
  constexpr int G = SCAN5_G, RMAX = FUSED_RMAX, NG = SPEC2_NG;
  constexpr int NP = M / 2;             // phases per entry
  constexpr int ROWB = G * 2;           // bytes of a slab row: two 16-byte halves of 8 items
  constexpr int HROWB = 16;             // a half row; the halves of a position live in two planes of K half rows each
  static_assert(M == 12 && G == 16 && SPEC2_NB == 8, "layout");
  typedef uint32_t u2 __attribute__((ext_vector_type(2)));
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* slab = smem;                                                      // [2][2][K][ROWB]
  uint32_t* colmin = reinterpret_cast<uint32_t*>(smem + a.desc_offset);           // [16][64]
  uint32_t* thr_s = colmin + 16 * 64;                                             // [16]
  int32_t* dsc = reinterpret_cast<int32_t*>(smem + a.desc_offset + 4096 + 64);    // [2][REC_DW] entry records
  int32_t* gidq = dsc + 2 * REC_DW;
  float* rt_s = reinterpret_cast<float*>(gidq + 4);                                // [4096] row terms of the entry about to start

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool builder = wave < SPEC2_NB;
  const int K = FULLK ? 1024 : a.K;
  const uint32_t HALFB = (uint32_t)K * HROWB;        // bytes of one plane: the values of 8 items for every code of a position
  const uint32_t POSB = 2u * HALFB;                  // bytes of one position's slab
  const uint32_t BUFB = 2u * POSB;                   // bytes of one buffer
  const int n_work = a.n_groups[0];

  int cur = 0, ei = 0;
  // The first entry of a workgroup is its own number (the entries are ordered largest first: the grid -- its guaranteed workgroups,
  // n_own, when it brings extras -- takes the first of them, one each); the work counter deals out the entries BEYOND those.  A workgroup so starts with ONE round trip -- its record
  // and the claim of its second entry together -- instead of two dependent atomics and then the record.
  // ELASTIC: the first n_own workgroups are the scan's guaranteed ones and start as above; a workgroup beyond them is an EXTRA -- it looks
  // at the handle's words first and takes an entry from the work counter (one more round trip) only if no other scan is announced and
  // fewer than `cap` scan workgroups are alive; a declined extra touches no entry.  No workgroup waits for another one, and whatever the
  // words hold every entry is claimed exactly once.
  const int n_own = ELASTIC ? a.n_own : (int)gridDim.x;
  const bool extra = ELASTIC && (int)blockIdx.x >= n_own;
  if (!extra) {
    if (tid == 0) {
      gidq[0] = (int)blockIdx.x; gidq[1] = n_own + atomicAdd(a.work_counter, 1);
      if constexpr (ELASTIC) {   // a guaranteed workgroup has started: no longer announced, alive if it has an entry
        __hip_atomic_fetch_sub(a.elastic + EL_PENDING, 1, FREDDY_RLX_AGENT);
        if ((int)blockIdx.x < n_work) __hip_atomic_fetch_add(a.elastic + EL_ACTIVE, 1, FREDDY_RLX_AGENT);
      }
    }
    if (tid < REC_DW) dsc[tid] = a.records[(size_t)blockIdx.x * REC_DW + tid];   // (before n_work is known: the grid never exceeds the records' capacity)
  } else if (tid == 0) {
    // (`pending` still holds this scan's OWN guaranteed workgroups whose decrement has not landed -- on an idle chip the whole grid
    // starts within a microsecond and every extra found itself announced, none took work.  Every guaranteed workgroup adds one to the
    // work counter as it starts, so n_own - counter bounds those from above; it is 0 once any n_own claims were made.)
    const int pend = __hip_atomic_load(a.elastic + EL_PENDING, FREDDY_RLX_AGENT);
    const int claims = __hip_atomic_load(a.work_counter, FREDDY_RLX_AGENT);
    const int alive = __hip_atomic_fetch_add(a.elastic + EL_ACTIVE, 1, FREDDY_RLX_AGENT);
    int g = -1;
    if (pend - (claims < n_own ? n_own - claims : 0) <= 0 && alive < a.cap) g = n_own + atomicAdd(a.work_counter, 1);
    if (g < 0 || g >= n_work) {
      g = -1;
      __hip_atomic_fetch_sub(a.elastic + EL_ACTIVE, 1, FREDDY_RLX_AGENT);
    } else {
      __hip_atomic_fetch_add(a.elastic + EL_STARTED, 1, FREDDY_RLX_AGENT);
    }
    // (the tests' elastic_yield = 2: every extra ends after its first entry; otherwise its next look at `pending` is its next claim)
    const bool leave = g >= 0 && a.elastic_yield == 2;
    if (leave) __hip_atomic_fetch_add(a.elastic + EL_YIELDED, 1, FREDDY_RLX_AGENT);
    gidq[0] = g; gidq[1] = (leave || g < 0) ? 0x7fffffff : n_own + atomicAdd(a.work_counter, 1); gidq[2] = leave ? 1 : 0;
  }
  for (int i = tid; i < 16 * 64; i += SPEC2_T) colmin[i] = 0xffffffffu;
  __syncthreads();
  if (extra) {   // the entry thread 0 has claimed, if any -- and only now its record
    const int first = __builtin_amdgcn_readfirstlane(gidq[0]);
    if (first < 0) return;
    if (tid < REC_DW) dsc[tid] = a.records[(size_t)first * REC_DW + tid];
    __syncthreads();
  } else if ((int)blockIdx.x >= n_work) return;

  if (builder) {
    // =====================================================================================
    // BUILDERS: a pair of waves per (position of the phase, half = 8 items); lane li of the pair <-> code pairs
    // li + 128 k (k < 4), one 16-byte load per item.  A lane holds the values of ALL eight items of its half for its
    // eight codes, so a half row leaves as ONE 16-byte store and consecutive lanes store consecutive half rows: no bank
    // conflicts (8-byte stores per item quad were 4-way conflicts: half of the kernel's conflict cycles).
    // Two register sets of one PHASE each: the set that phase j + 1 is written from at the start of phase j is
    // refilled at once with phase j + 3.
    // =====================================================================================
    const int hpos = (wave >> 1) & 1;    // position 2 j + hpos of phase j
    const int half = wave >> 2;          // items 8 half .. 8 half + 7
    const int li = (wave & 1) * 64 + lane;
    const uint32_t qoff = (uint32_t)hpos * POSB + (uint32_t)half * HALFB + (uint32_t)li * HROWB;
    const uint32_t vq = (uint32_t)li * 16u + (uint32_t)hpos * 2048u;
    u4 qw[2][8];   // [set][item of the half]
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int g = 0; g < 8; ++g) qw[s][g] = u4{0u, 0u, 0u, 0u};
    typedef const char __attribute__((address_space(1))) * gptrc;
    typedef const u4 __attribute__((address_space(1))) * gptr4u;
    auto issue = [&](int set, int phase, const int (&qids)[8], int nh) {   // position 2 phase + hpos of the half's 8 items
      if (half >= nh || (a.fence & 32)) return;
      uint32_t voff = vq + (uint32_t)phase * 4096u;
      asm volatile("" : "+v"(voff));
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const gptrc qb = (gptrc)(uintptr_t)a.qc + (size_t)(uint32_t)qids[u] * (size_t)(M * 2048);
        qw[set][u] = *(gptr4u)(qb + voff);
      }
    };
    // the eight table words of code pair b = li + 128 k interleaved: low halves -> half row b, high halves -> b + 512
    auto emit = [&](int set, unsigned char* dst, int nh) {
      if (half >= nh || (a.fence & 16)) return;
      unsigned char* dp = dst + qoff;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          w[u] = k == 0 ? qw[set][u].x : k == 1 ? qw[set][u].y : k == 2 ? qw[set][u].z : qw[set][u].w;
        // v_perm_b32: bytes 0-3 come from the second operand, 4-7 from the first
        const u4 lo = u4{__builtin_amdgcn_perm(w[1], w[0], 0x05040100u), __builtin_amdgcn_perm(w[3], w[2], 0x05040100u),
                         __builtin_amdgcn_perm(w[5], w[4], 0x05040100u), __builtin_amdgcn_perm(w[7], w[6], 0x05040100u)};
        const u4 hi = u4{__builtin_amdgcn_perm(w[1], w[0], 0x07060302u), __builtin_amdgcn_perm(w[3], w[2], 0x07060302u),
                         __builtin_amdgcn_perm(w[5], w[4], 0x07060302u), __builtin_amdgcn_perm(w[7], w[6], 0x07060302u)};
        const int b = li + 128 * k;
        if (FULLK || b < K) *reinterpret_cast<u4*>(dp + (uint32_t)(128 * k) * HROWB) = lo;
        if (FULLK || b + 512 < K) *reinterpret_cast<u4*>(dp + (uint32_t)(128 * k + 512) * HROWB) = hi;
      }
    };

    long long pt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pc = 0;
    auto tick = [&](int slot) { if constexpr (PROF) { const long long t = clock64(); pt[slot] += t - pc; pc = t; } };
    if constexpr (PROF) pc = clock64();
    int nq = (__builtin_amdgcn_readfirstlane(dsc[1]) + 7) >> 3;   // halves in use
    const int g0 = half * 8;
    int qid[8], nqid[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      qid[u] = __builtin_amdgcn_readfirstlane(dsc[24 + g0 + u]);
      nqid[u] = qid[u];
    }
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
    fetch_row_terms(dsc);
    stash_row_terms();
    issue(0, 0, qid, nq);
    issue(1, 1, qid, nq);
    emit(0, slab, nq);          // phase 0 -> buffer 0 (waits for set 0)
    issue(0, 2, qid, nq);
    lds_barrier();
    for (;;) {
      const int nb = cur ^ 1;
      const int ngid = __builtin_amdgcn_readfirstlane(gidq[(ei + 1) & 1]);
      const bool have_next = ngid < n_work;
      int gid2 = 0;
      int next_nq = 0;
      int32_t rr0 = 0;
      uint32_t run0 = 0u, run1 = 0u;
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        // the next entry's record: requested in phase 0, stored in phase 1, first read in phase 2
        if (j == 1 && tid < REC_DW) {
          if (tid == 0) gidq[ei & 1] = gid2;
          dsc[nb * REC_DW + tid] = rr0;
          if (wave == 0 && lane == 6) dsc[nb * REC_DW + 6] = have_next ? 1 : -1;
        }
        if (j == NP - 3) {   // (the next entry's record is in LDS since the barrier of phase 1)
          const int ncnt = have_next ? __builtin_amdgcn_readfirstlane(dsc[nb * REC_DW + 1]) : 0;
          next_nq = (ncnt + 7) >> 3;
#pragma unroll
          for (int u = 0; u < 8; ++u)
            nqid[u] = !have_next ? qid[u] : __builtin_amdgcn_readfirstlane(dsc[nb * REC_DW + 24 + g0 + u]);
        }
        // slab of phase j + 1 of this entry -- or phase 0 of the next one -- from the set requested two phases ago,
        // then the same set again for phase j + 3
        const int set = (j + 1) & 1;
        if (j + 1 < NP) emit(set, slab + (uint32_t)((j + 1) & 1) * BUFB, nq);
        else emit(set, slab, next_nq);
        if (j + 3 < NP) issue(set, j + 3, qid, nq);
        else issue(set, j + 3 - NP, nqid, next_nq);   // (nqid is the next entry's from phase NP - 3 on: j + 3 >= NP <=> j >= NP - 3)
        if (j == 2) fetch_row_terms(dsc + (have_next ? nb : cur) * REC_DW);
        if (j == NP - 1 && a.tau_run) {   // the running bounds of this wave's two items (S1): on their way while the gatherers finish
          const int32_t* rc = dsc + cur * REC_DW;
          const int cn = __builtin_amdgcn_readfirstlane(rc[1]);
          run0 = wave < cn ? a.tau_run[(uint32_t)rc[24 + wave]] : 0u;
          run1 = wave + NG < cn ? a.tau_run[(uint32_t)rc[24 + wave + NG]] : 0u;
        }
        if (j == 0 && tid < REC_DW && have_next) rr0 = a.records[(size_t)ngid * REC_DW + tid];
        if (j == 0 && tid == 0) {
          // (an extra workgroup that finds another scan announced takes no further entry: it ends after the entry it has claimed)
          // -- and from then on claims nothing: a claim made after the decision to leave would be an entry nobody scans (gidq[2]: the
          // decision; an extra whose next entry is beyond the table is out of work and claims nothing either)
          if (extra && (gidq[2] != 0 || !have_next)) {
            gid2 = 0x7fffffff;
          } else if (extra && __hip_atomic_load(a.elastic + EL_PENDING, FREDDY_RLX_AGENT) > 0) {
            gid2 = 0x7fffffff;
            gidq[2] = 1;
            __hip_atomic_fetch_add(a.elastic + EL_YIELDED, 1, FREDDY_RLX_AGENT);
          } else {
            gid2 = n_own + atomicAdd(a.work_counter, 1);
          }
        }
        tick(0);
        lds_barrier();
        tick(1);
      }
      // S1: thresholds tau + E, one item segment at a time while the gatherers are in their tail on the OTHER segment (builder wave w:
      // item w between the gatherers' barriers T1 and T2, item w + 8 -- entries of more than 8 items -- between T2 and T3).
      // The query's running bound (FilterArgs::tau_run; running_bound5, filter_threshold5).  tau' + A_up of this (item, chunk) is
      // reported (no answer is waited for); the bound read at the start of the last phase -- whatever other workgroups had
      // reported by then -- lowers this item's cut to bound - A_lo.  Why any such value is valid: tau' is at least the k-th smallest
      // s' of the chunk (k = a.Lt, the threshold rank), s' + A is the cheap distance up to the item-independent part of its error,
      // and the k-th smallest over MORE rows is never larger -- so every reported value is an upper bound of the query's k-th
      // smallest cheap distance D_k, and the rows that can matter have s' + A <= D_k + 2 e.  (The three float roundings here are
      // below 10 u B of the 2.2 e = 230 u B + 13 T that E leaves over 2 e.)  Item w reports before item w + 8, as it always did.
      const int32_t* rec_t = dsc + cur * REC_DW;
      const int cnt_t = __builtin_amdgcn_readfirstlane(rec_t[1]);
      auto threshold = [&](int i, uint32_t run) {
        if (i < cnt_t && !(a.fence & 4)) {
          const uint32_t c = wave_sort32(colmin[i * 64 + lane]);   // (order-preserving keys of the float column minima)
          const uint32_t t = __shfl(c, a.Lt - 1, 64);
          if (lane == 0) thr_s[i] = filter_threshold5(a, rec_t, i, t, run);
          colmin[i * 64 + lane] = 0xffffffffu;
        }
      };
      threshold(wave, run0);
      lds_barrier();   // T2
      if (cnt_t > 8) {
        threshold(wave + NG, run1);
        lds_barrier();   // T3
      }
      stash_row_terms();   // (the gatherers took the current entry's into registers before T1)
      lds_barrier();   // S2
      tick(3);
      if constexpr (PROF) pt[7] += 1;
      if (!have_next) break;
      cur = nb;
      ++ei;
      nq = next_nq;
#pragma unroll
      for (int u = 0; u < 8; ++u) qid[u] = nqid[u];
    }
    if (ELASTIC && tid == 0) __hip_atomic_fetch_sub(a.elastic + EL_ACTIVE, 1, FREDDY_RLX_AGENT);   // (every workgroup that reaches the entry loop counted itself alive)
    if (PROF && a.prof && tid == 0) {
      for (int i = 0; i < 8; ++i) if (i != 2 && i != 4 && i != 5) a.prof[(size_t)blockIdx.x * 8 + i] = pt[i];   // (2, 4, 5: gatherer wave 0)
      a.prof[(size_t)blockIdx.x * 8 + 6] = wall_clock64();
    }
  } else {
    // =====================================================================================
    // GATHERERS: lane <-> 8 rows x 12 items, a (row, item) sum = one 16-bit half of a register
    // =====================================================================================
    const int gw = wave - SPEC2_NB;
    uint32_t acc[G / 2][RMAX];     // [item pair][row]: low half = item 2i, high half = item 2i + 1
    uint32_t cwa[RMAX], cwb[RMAX]; // code dwords of the even / odd phases (double buffered: requested a phase ahead)
    // the first two rows' code dwords of phase 0 of the COMING entry, requested an entry ahead (at the end of the survivor pass): a
    // gatherer otherwise starts every entry with an exposed round trip for row 0's codes (the other rows' arrive behind it)
    constexpr int NPRE = 2;
    uint32_t cpre[NPRE] = {};
    auto prefetch_first_codes = [&](const int32_t* rc) {
      const int b0 = __builtin_amdgcn_readfirstlane(rc[3]), nbk = __builtin_amdgcn_readfirstlane(rc[4]);
      const uint32_t l4 = lane_byte4();
#pragma unroll
      for (int r = 0; r < NPRE; ++r) {
        const int bl = r * NG + gw;
        const uint32_t blk = (uint32_t)(b0 + (bl < nbk - 1 ? bl : nbk - 1));
        const char* rowp = U8 ? reinterpret_cast<const char*>(a.packed8) + (size_t)(blk * (uint32_t)(M / 4)) * 256u
                              : reinterpret_cast<const char*>(a.packed) + (size_t)(blk * (uint32_t)(M / 2)) * 256u;
        cpre[r] = *reinterpret_cast<const uint32_t*>(rowp + l4);
      }
    };
    prefetch_first_codes(dsc);
    lds_barrier();   // (pairs with the builders' barrier after the first slab)
    // (PROF slots: 0 main loop, 1 column minima, 2 survivor pass; 3, 4, 5 the waits at the tail's barriers T1, T2, T3; 6 the wait at
    // the entry's last barrier; 7 entries of more than 8 items)
    long long gt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gc = 0;
    auto gtick = [&](int slot) { if constexpr (PROF) { const long long t = clock64(); if (slot >= 0) gt[slot] += t - gc; gc = t; } };
    for (;;) {
      gtick(-1);
      const int32_t* rec = dsc + cur * REC_DW;
      const int cnt = __builtin_amdgcn_readfirstlane(rec[1]);
      const int chunk = __builtin_amdgcn_readfirstlane(rec[2]);
      const int blk0 = __builtin_amdgcn_readfirstlane(rec[3]);
      const int nblk = __builtin_amdgcn_readfirstlane(rec[4]);
      const int nrows = __builtin_amdgcn_readfirstlane(rec[5]);
      const int nq = (cnt + 7) >> 3;     // 16-byte halves of a slab row in use
      const int nb = cur ^ 1;
      const int rl_wave = (nblk - gw + NG - 1) / NG < 0 ? 0 : (nblk - gw + NG - 1) / NG;
      auto row_block = [&](int r) {
        const int bl = r * NG + gw;
        return (uint32_t)(blk0 + (bl < nblk - 1 ? bl : nblk - 1));
      };
      auto main_loop = [&](auto nqc, auto rlc) {
        constexpr int NQ = decltype(nqc)::value, RL = decltype(rlc)::value;
        // (uniform 64-bit row address + this lane's byte offset, recomputed where it is needed: hoisted out of the entry
        // loop it was spilled, and every phase waited for the reload)
        auto load_codes = [&](uint32_t (&cw)[RMAX], int pair) {
          const uint32_t l4 = lane_byte4();
#pragma unroll
          for (int r = 0; r < RL; ++r) {
            const char* rowp = U8 ? reinterpret_cast<const char*>(a.packed8) + (size_t)((row_block(r) * (uint32_t)(M / 4) + (uint32_t)(pair >> 1)) * 256u)
                                  : reinterpret_cast<const char*>(a.packed) + (size_t)((row_block(r) * (uint32_t)(M / 2) + (uint32_t)pair) * 256u);
            cw[r] = *reinterpret_cast<const uint32_t*>(rowp + l4);
          }
        };
        // both positions of a phase, one row at a time: NQ ds_read_b128 per position fetch the values of 8 items each.
        // Half h of row c sits at byte 32 c + 16 (h ^ bit 3 of c): with the plain layout the first halves of all rows
        // would share 8 of the 16 bank groups.
        // Software pipelined: the reads of row r + 1 are issued before the sums of row r -- with one row's 2 NQ reads in
        // flight per wave the LDS pipe idled while the waves added (a closed loop: 8 waves x 4 reads, ~15 cycles of
        // service each, then ~100 cycles of adds before the next batch).
        auto gather = [&](const uint32_t (&cw)[RMAX], int j) {
          constexpr int DEPTH = NQ == 1 ? 4 : 2;   // rows in flight (32 registers either way; 3 rows of two halves spill)
          u4 va[DEPTH][2][NQ];   // [row slot][position of the phase][half]
          // byte offsets of the two codes' half rows: 16 c (| the buffer); halves and positions are constant offsets
          uint32_t bb = (uint32_t)(j & 1) * BUFB;
          asm volatile("" : "+s"(bb));   // (kept out of the constant folder: the halves / positions stay immediate offsets)
          auto issue_row = [&](int r) {
            // (U8: phase j's two codes are bytes 2 (j & 1) and 2 (j & 1) + 1 of the dword)
            const uint32_t a0 = (U8 ? ((j & 1) ? ((cw[r] >> 12) & 0xff0u) : ((cw[r] << 4) & 0xff0u)) : ((cw[r] << 4) & 0x3ff0u)) + bb;
            const uint32_t a1 = (U8 ? ((j & 1) ? ((cw[r] >> 20) & 0xff0u) : ((cw[r] >> 4) & 0xff0u)) : ((cw[r] >> 12) & 0x3ff0u)) + bb;
#pragma unroll
            for (int q = 0; q < NQ; ++q) va[r % DEPTH][0][q] = *reinterpret_cast<const u4*>(slab + a0 + (uint32_t)q * HALFB);
#pragma unroll
            for (int q = 0; q < NQ; ++q) va[r % DEPTH][1][q] = *reinterpret_cast<const u4*>(slab + a1 + POSB + (uint32_t)q * HALFB);
          };
#pragma unroll
          for (int r = 0; r < DEPTH - 1; ++r) if (r < RL) issue_row(r);
#pragma unroll
          for (int r = 0; r < RL; ++r) {
            if (r + DEPTH - 1 < RL) issue_row(r + DEPTH - 1);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
              const u4 x = va[r % DEPTH][0][q], y = va[r % DEPTH][1][q];
              acc[q * 4 + 0][r] = acc[q * 4 + 0][r] + x.x + y.x;   // (v_add3_u32: unsigned fields, see filt5_bias)
              acc[q * 4 + 1][r] = acc[q * 4 + 1][r] + x.y + y.y;
              acc[q * 4 + 2][r] = acc[q * 4 + 2][r] + x.z + y.z;
              acc[q * 4 + 3][r] = acc[q * 4 + 3][r] + x.w + y.w;
            }
            if (r + 1 < RL) __builtin_amdgcn_sched_barrier(0);
          }
        };
#pragma unroll
        for (int h = 0; h < G / 2; ++h)
#pragma unroll
          for (int r = 0; r < RMAX; ++r) acc[h][r] = 0u;
        load_codes(cwa, 0);
#pragma unroll
        for (int r = 0; r < NPRE; ++r) if (r < RL) cwa[r] = cpre[r];   // (requested an entry ahead; the loads above for these rows are dropped by the compiler)
        load_codes(cwb, 1);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          if (!(a.fence & 2)) {
            if (j & 1) gather(cwb, j); else gather(cwa, j);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (j + 2 < NP && !(a.fence & 64)) {   // the codes of phase j + 2 into the set phase j has just used
            if (j & 1) load_codes(cwb, j + 2); else load_codes(cwa, j + 2);
          }
          if (j + 1 < NP) lds_barrier();
        }
      };
      dispatch_nq_rl(nq, rl_wave, main_loop);
      // ---- tail (scan_tail5.inc)
#define SCAN_TAIL5_FENCE a.fence
#define SCAN_TAIL5_PART 1
#include "scan_tail5.inc"
      gtick(0);
      // The tail in two item segments, 0-7 and 8-15: the builders sort a segment's thresholds (S1) while the gatherers work on
      // the other one -- column minima of 8.. under S1 of 0-7, survivors of 0-7 under S1 of 8.. -- instead of waiting for all sixteen.
      // cnt is uniform and both roles read it from the same record: an entry of more than 8 items takes one barrier more, on both
      // sides; one of up to 8 items has no second segment and keeps the sequence it had.
#define SCAN_TAIL5_PART 2
#define SCAN_TAIL5_G0 0
#define SCAN_TAIL5_G1 8
#include "scan_tail5.inc"
      gtick(1);
      lds_barrier();   // T1: the column minima of items 0-7 are in
      gtick(3);
      if (cnt > 8) {
#define SCAN_TAIL5_PART 2
#define SCAN_TAIL5_G0 8
#define SCAN_TAIL5_G1 16
#include "scan_tail5.inc"
      }
      gtick(1);
      lds_barrier();   // T2: thr_s[0..7]; the column minima of items 8.. are in
      gtick(4);
#define SCAN_TAIL5_PART 3
#define SCAN_TAIL5_G0 0
#define SCAN_TAIL5_G1 8
#include "scan_tail5.inc"
      gtick(2);
      if (cnt > 8) {
        lds_barrier();   // T3: thr_s[8..15]
        gtick(5);
#define SCAN_TAIL5_PART 3
#define SCAN_TAIL5_G0 8
#define SCAN_TAIL5_G1 16
#include "scan_tail5.inc"
      }
#define SCAN_TAIL5_PART 4
#include "scan_tail5.inc"
#undef SCAN_TAIL5_FENCE
      gtick(2);
      const int next_ok = __builtin_amdgcn_readfirstlane(dsc[nb * REC_DW + 6]);
      if (next_ok > 0) prefetch_first_codes(dsc + nb * REC_DW);
      lds_barrier();
      gtick(6);
      if constexpr (PROF) gt[7] += cnt > 8 ? 1 : 0;
      if (next_ok < 0) break;
      cur = nb;
    }
    if (PROF && a.prof && gw == 0 && lane == 0) {
      a.prof[(size_t)blockIdx.x * 8 + 2] = gt[0];
      a.prof[(size_t)blockIdx.x * 8 + 4] = gt[1];
      a.prof[(size_t)blockIdx.x * 8 + 5] = gt[2];
      // (a second table behind the first, at a fixed offset: the tail's barrier waits; the host hands out no buffer to a grid
      // of more than SCAN5_PROF_WGS workgroups, scan_prof_buffer)
      long long* p2 = a.prof + ((size_t)SCAN5_PROF_WGS + blockIdx.x) * 8;
      for (int i = 0; i < 5; ++i) p2[i] = gt[3 + i];
    }
  }
}

template <int M, bool FULLK, bool CAND, bool PROF = false, bool U8 = false>
__global__ __launch_bounds__(SPEC2_T) void ivf_filter5_kernel(FilterArgs a) {
  ivf_filter5_body<M, FULLK, CAND, PROF, U8, false>(a);
}
// (a.elastic != NULL, grid >= a.n_own)
template <int M, bool FULLK, bool CAND, bool U8 = false>
__global__ __launch_bounds__(SPEC2_T) void ivf_filter5_elastic_kernel(FilterArgs a) {
  ivf_filter5_body<M, FULLK, CAND, false, U8, true>(a);
}

}  // namespace freddy
