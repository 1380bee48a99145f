// scan_tail5.inc -- the selection tail of the integer filter scans' gatherer waves, ONE copy: what turns a wave's (row, item) sums
// into survivor keys.  A FRAGMENT, not a header: ivf_filter5_kernel (fused5.h) and ivf_filter8_kernel (fused8.h) include it
// inside their bodies, once per part, with their own barriers, profiling ticks and prefetches between the parts:
//
//   #define SCAN_TAIL5_PART 1   row terms -> base[], the biased unsigned fields of acc[][] -> signed sums
//   #define SCAN_TAIL5_PART 2   sval(), live8; per item the lane's smallest / second smallest s' and the row of the smallest
//                               (best[], sec16[], apack[]); column minima -> colmin[item][lane]
//   #define SCAN_TAIL5_PART 3   S2: rows with s' <= tau' + E (thr_s[item], from the kernel's S1 step) -> this wave's
//                               region of each item's survivor buffer
//
// Parts 2 and 3 handle the items one after the other, so an including kernel may cut them into item SEGMENTS and put a barrier of
// its own between two of them (ivf_filter5_kernel: the thresholds of one segment are sorted while the gatherers work on the other):
//
//   #define SCAN_TAIL5_G0 / SCAN_TAIL5_G1   items [G0, G1) of part 2 or 3, integer literals, in ascending segments from 0.  The
//                               segment that starts at 0 declares what the later ones and the later parts use; part 3 of a
//                               segment reads ITS items' thresholds when it starts.
//   #define SCAN_TAIL5_PART 4   after the last segment of part 3: the one store of the entry's survivor counts
//
// Without the two names a part covers all G items and part 3 ends with the store itself (fused8.h).
//
// Why text and not functions: both kernels sit at 128 VGPRs, and the same statements moved into __forceinline__ functions (arrays
// by reference, sval as a free function) came back from the compiler with other code -- the optimiser simplifies a callee before
// it is inlined, later passes then hoist and order the same instructions differently, and the register allocator spills
// (profiles/scan_tail_isa.txt has the figures).  Included text is the same translation unit the kernels had before.
//
// Names the including kernel provides: G, RMAX, NG, CAND (constants); a (FilterArgs), rec (the entry's record in LDS), rt_s, colmin,
// thr_s (LDS); acc[G / 2][RMAX]; cnt, chunk, blk0, nrows, rl_wave, gw, lane; and the macro SCAN_TAIL5_FENCE: FilterArgs::fence in
// ivf_filter5_kernel (always 0 at run time, opaque to the compiler: its conditions keep that kernel's register allocation where
// it is, profiles/HISTORY.md), the literal 0u in ivf_filter8_kernel, where the conditions fold away.
// Names it leaves behind for the later parts: base[] (part 1); sval, gi, p_sc, live8, best[], sec16[], apack[] (part 2, its segment
// from 0); with segments also part 3's per-lane record words and counts -- p_shift, p_off, p_lo, p_hi, p_q, p_reg, cntv -- which its
// later segments and part 4 use.
//
// The contract with merge_refine_kernel (refine.h) -- written down here and in sparse5.h's two survivor passes, nowhere else:
//   key     surv_key5(d_lo, location): d_lo = max(0, (s' + OFF) - shift); location = the row's global slot, bit 31 = `amb` (CAND
//           only: the row is inside the sentinel's bracket, the merge decides whether it counts)
//   region  ((item * upi + chunk) * 8 + wave) * 512 keys; surv_count[(item * upi + chunk) * 8 + wave] of them are valid
//   a NaN passes every threshold test (!(s' > thr)): the exact stage sees it
#if SCAN_TAIL5_PART == 1
// ---- tail.  The selection works on s' = fma(scale[item], V, rterm[row]) -- the stored sum WITHOUT the item's
// constant OFF -- compared as floats: a constant shift changes neither the order nor tau' + E.  OFF (which keeps
// the stored bits positive for the merge) is added for the survivors only: s = s' + OFF.
// base[r] = the row's own term (staged by the builders in the previous entry's tail, replaced in this one's once the last threshold barrier is behind the builders: every gatherer passed this point before the first); +inf for the slots of this wave beyond its last block and for the lanes
// past the end of the list (s = +inf: above every finite threshold; S2 skips the former and masks the latter)
float base[RMAX];
const int last_blk = nrows > 0 ? (nrows - 1) >> 6 : -1;     // chunk-relative block holding the last row
const int rs2 = (last_blk >= 0 && (last_blk % NG) == gw && (nrows & 63)) ? last_blk / NG : -1;
const bool live_lane = lane < (nrows & 63);
{
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    base[r] = rt_s[(r * NG + gw) * 64 + lane];
    if (r >= rl_wave || (r == rs2 && !live_lane)) base[r] = __uint_as_float(0x7f800000u);
  }
}
#pragma unroll
for (int h = 0; h < G / 2; ++h)
#pragma unroll
  for (int r = 0; r < RMAX; ++r) acc[h][r] ^= 0x80008000u;   // biased unsigned fields -> signed sums
#elif SCAN_TAIL5_PART == 2
#ifndef SCAN_TAIL5_G0
#define SCAN_TAIL5_G0 0
#define SCAN_TAIL5_G1 G
#endif
#if SCAN_TAIL5_G0 == 0
auto sval = [&](int g, int r, float sc) -> float {
  const uint32_t w = acc[g >> 1][r];
  const int v = (g & 1) ? ((int32_t)w >> 16) : ((int32_t)(w << 16) >> 16);
  return __builtin_fmaf(sc, (float)v, base[r]);
};
// Per-item parameters: lane g holds item g's (one LDS read each, fetched with v_readlane below -- a chain of
// dependent LDS round trips per item was a quarter of the entry's time).
const int gi = lane & 15;
const float p_sc = __int_as_float(rec[128 + gi]);
// rows this lane really holds: bit r of live8
uint32_t live8 = 0u;
#pragma unroll
for (int r = 0; r < RMAX; ++r)
  if (r < rl_wave && !(r == rs2 && !live_lane)) live8 |= 1u << r;
float best[G];
uint32_t sec16[G / 2];           // second smallest, rounded DOWN to 16 bits (sign, exponent, 7 bits): two items per register
uint32_t apack[2] = {0u, 0u};
#pragma unroll
for (int g = 0; g < G; ++g) best[g] = __uint_as_float(0x7f800000u);
#pragma unroll
for (int i = 0; i < G / 2; ++i) sec16[i] = 0x7f807f80u;
#endif
if (!(SCAN_TAIL5_FENCE & 4)) {
#pragma unroll
  for (int g = SCAN_TAIL5_G0; g < SCAN_TAIL5_G1; ++g) {
    if (g < cnt) {
      // the lane's smallest and second smallest s' of this item and the row of the smallest: a lane hardly ever
      // holds two survivors, so S2 can emit (best, its row) without looking at the sums again
      const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p_sc), g));
      float b1 = __uint_as_float(0x7f800000u), b2 = __uint_as_float(0x7f800000u);
      uint32_t ar = 0u;
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        const float sv = sval(g, r, sc);
        b2 = __builtin_amdgcn_fmed3f(b1, b2, sv);   // (b1 <= b2: the median is the new second smallest)
        ar = sv < b1 ? (uint32_t)r : ar;
        b1 = fminf(b1, sv);
      }
      best[g] = b1;
      {
        const uint32_t bb = __float_as_uint(b2);
        const uint32_t dn = ((bb >> 31) ? bb + 0xffffu : bb) >> 16;   // toward -inf: the test below errs to the slow path
        sec16[g >> 1] = (g & 1) ? ((sec16[g >> 1] & 0x0000ffffu) | (dn << 16)) : ((sec16[g >> 1] & 0xffff0000u) | dn);
      }
      // (opaque: the compiler otherwise folds the shift into the eight selects above, whose constants 128, 192, ... are no inline
      // operands -- a v_mov per row and item)
      asm volatile("" : "+v"(ar));
      apack[g >> 3] |= ar << (3 * (g & 7));
      if (rl_wave > 0) atomicMin(colmin + g * 64 + lane, float_key(b1));
    }
  }
}
#undef SCAN_TAIL5_G0
#undef SCAN_TAIL5_G1
#elif SCAN_TAIL5_PART == 3
#ifndef SCAN_TAIL5_G0
#define SCAN_TAIL5_G0 0
#define SCAN_TAIL5_G1 G
#define SCAN_TAIL5_WHOLE
#endif
// S2: survivors -> this wave's region of each item's buffer.  Normally every lane has at most one (its smallest
// sum, kept from the pass above); otherwise the pass bits of the lane's 8 rows, branch free, then per-row ballots.
#ifdef SCAN_TAIL5_WHOLE
if (!(SCAN_TAIL5_FENCE & 4)) {
  const float p_thr = __uint_as_float(thr_s[gi]);
  const int p_it = rec[8 + gi];
  const float p_shift = __int_as_float(rec[72 + gi]);
  const float p_off = __int_as_float(rec[40 + gi]);
  const uint32_t p_lo = (uint32_t)rec[88 + gi], p_hi = (uint32_t)rec[104 + gi];
  const int p_q = rec[24 + gi];
  // lane g: item g's survivor region of this wave, and (collected below) its count -- ONE store of the counts per entry
  const int p_reg = (p_it * a.upi + chunk) * NG + gw;
  int cntv = 0;
#else
// (segments: the record words outlive this segment's block; the thresholds are read per segment -- a later segment's are
// published after an earlier segment's pass has begun)
#if SCAN_TAIL5_G0 == 0
// (initialised: left undefined on the fence's path they were live -- as undefined values -- around the whole entry loop, three
// registers the main loop does not have)
float p_shift = 0.0f, p_off = 0.0f;
uint32_t p_lo = 0u, p_hi = 0u;
int p_q = 0, p_reg = 0;
int cntv = 0;
#endif
if (!(SCAN_TAIL5_FENCE & 4)) {
  // (the address recomputed per segment from an opaque lane id: as one value of the entry loop it was hoisted over the main loop
  // and spilled there.  Every lane reads the word of item lane & 15, this segment's or not: the builders may be writing a LATER
  // segment's thresholds at this moment, and what such a lane gets is never used -- the readlanes below take lanes G0 .. G1 - 1,
  // whose words were published before the barrier in front of this segment, and the later segment reads again behind its own)
  const float p_thr = __uint_as_float(*reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(thr_s) + (lane_byte4() & 60u)));
#if SCAN_TAIL5_G0 == 0
  p_shift = __int_as_float(rec[72 + gi]);
  p_off = __int_as_float(rec[40 + gi]);
  p_lo = (uint32_t)rec[88 + gi]; p_hi = (uint32_t)rec[104 + gi];
  p_q = rec[24 + gi];
  p_reg = (rec[8 + gi] * a.upi + chunk) * NG + gw;
#endif
#endif
#pragma unroll
  for (int g = SCAN_TAIL5_G0; g < SCAN_TAIL5_G1; ++g) {
    if (g < cnt) {
      const float thr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p_thr), g));
      const float off = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p_off), g));
      const float shift = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p_shift), g));
      const uint32_t region = (uint32_t)__builtin_amdgcn_readlane(p_reg, g);
      u64* dst = a.surv + (size_t)region * (size_t)(RMAX * 64);
      int run = 0;
      if constexpr (!CAND) {   // the common case (freddy.c:366 counts retrieved rows): nothing but the threshold test
       const float second = __uint_as_float((g & 1) ? (sec16[g >> 1] & 0xffff0000u) : (sec16[g >> 1] << 16));
       const u64 multi = __ballot(!(second > thr));   // lanes with two survivors (or: keep every row, NaNs)
       if (__builtin_expect(multi == 0ull, 1)) {
        // (no uniform branch around the emission: nearly every (item, wave) has a survivor, the exec mask does the rest)
        const bool pass = !(best[g] > thr);
        const u64 mask = __ballot(pass);
        if (pass) {
          const uint32_t r = (apack[g >> 3] >> (3 * (g & 7))) & 7u;
          const float dlo = fmaxf(0.0f, (best[g] + off) - shift);
          const uint32_t loc = ((uint32_t)(blk0 + gw) + r * (uint32_t)NG) * 64u + (uint32_t)lane;
          dst[lanes_below(mask)] = surv_key5(dlo, loc);
        }
        run = __popcll(mask);
       } else {
        const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p_sc), g));   // (this path only)
        uint32_t m8 = 0u;
#pragma unroll
        for (int r = RMAX - 1; r >= 0; --r) m8 = m8 + m8 + (!(sval(g, r, sc) > thr) ? 1u : 0u);   // (a NaN passes: exact stage)
        m8 &= live8;
        if ((SCAN_TAIL5_FENCE & 128) == 0 && __ballot(m8 != 0u) != 0ull) {
#pragma unroll
          for (int r = 0; r < RMAX; ++r) {
            const bool pass = (m8 >> r) & 1u;
            const u64 mask = __ballot(pass);
            if (mask != 0ull) {
              if (pass) {
                const float dlo = fmaxf(0.0f, (sval(g, r, sc) + off) - shift);
                const uint32_t loc = (uint32_t)(blk0 + r * NG + gw) * 64u + (uint32_t)lane;
                dst[run + lanes_below(mask)] = surv_key5(dlo, loc);
              }
              run += __popcll(mask);
            }
          }
        }
       }
      } else {   // rows below the sentinel are counted (freddy.c:971): bounds on the bits of s = s' + OFF > 0
        const uint32_t lo_b = (uint32_t)__builtin_amdgcn_readlane((int)p_lo, g);
        const uint32_t hi_b = (uint32_t)__builtin_amdgcn_readlane((int)p_hi, g);
        const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p_sc), g));
        int accepted = 0;
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
          if (r >= rl_wave) break;
          const float sv = sval(g, r, sc);
          const uint32_t sb = __float_as_uint(sv + off);
          const bool live = (live8 >> r) & 1u;
          accepted += __popcll(__ballot(live && sb < lo_b));
          const bool amb = sb >= lo_b && sb < hi_b;
          const bool pass = live && (!(sv > thr) || amb);
          const u64 mask = __ballot(pass);
          if (mask != 0ull) {
            if (pass) {
              const float dlo = fmaxf(0.0f, __uint_as_float(sb) - shift);
              const uint32_t loc = ((uint32_t)(blk0 + r * NG + gw) * 64u + (uint32_t)lane) | (amb ? 0x80000000u : 0u);
              dst[run + lanes_below(mask)] = surv_key5(dlo, loc);
            }
            run += __popcll(mask);
          }
        }
        if (lane == 0 && accepted) atomicAdd(a.cand_count + __builtin_amdgcn_readlane(p_q, g), accepted);
      }
      // (v_writelane: the compiler's own select read its sixteen lane masks back from spilled scalar registers, five instructions per item)
      asm("v_writelane_b32 %0, %1, %2" : "+v"(cntv) : "s"(run), "i"(g));
    }
  }
#ifdef SCAN_TAIL5_WHOLE
  if (lane < cnt) a.surv_count[(uint32_t)p_reg] = cntv;
#endif
}
#undef SCAN_TAIL5_G0
#undef SCAN_TAIL5_G1
#undef SCAN_TAIL5_WHOLE
#elif SCAN_TAIL5_PART == 4
if (!(SCAN_TAIL5_FENCE & 4)) {
  if (lane < cnt) a.surv_count[(uint32_t)p_reg] = cntv;
}
#else
#error "SCAN_TAIL5_PART: 1 .. 4"
#endif
#undef SCAN_TAIL5_PART
