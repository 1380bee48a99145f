// one.h -- ONE query as a single launch (gfx950): pq_one_kernel, ivf_one_kernel.
//
// The generic path answers a single pq_search query with three dependent launches -- lut_build_kernel, adc_scan_kernel,
// merge_replay_kernel: 14 + 22 + 14 us under HIP events for 28 MB of codes that sit in the caches -- i.e. mostly launch
// gaps.  pq_one_kernel is the same three stages in one grid of at most one workgroup per CU (all co-resident):
//   1. every workgroup computes its slice of the query's table lut[pos*K + code] = squareDistance(q_pos, cb[pos][code])
//      (index_utils.c:445-455; the sequential binary32 chain of lut_build_kernel) and publishes it;
//   2. every workgroup waits for the table, stages it in LDS and scans its chunk of row blocks exactly as adc_scan_kernel
//      does (position-order sums, index_utils.c:1126-1133; WaveSelect of the L = 2k smallest (distance, position) keys),
//      then publishes its L keys;
//   3. workgroup 0 collects the lists, merges them and forms the reference's list (merge_replay_kernel's tail: updateTopK +
//      "dist < maxDist", index_utils.c:19-33, freddy.c:128-131), writes it to mapped host memory and then the completion
//      word the host polls.
// Hand-offs carry no counters: every published word carries the call's epoch in its top bit (below, "hand-offs without
// counters").  All waits are bounded: a grid that cannot become co-resident reports through `err` instead of hanging (the
// host then takes the three-launch path).  ivf_one_kernel: further down.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "one_layout.h"
#include "wave_topk.h"

namespace freddy {

struct OneArgs {
  float qv[300];             // the query, by value: it travels with the dispatch (no PCIe read at kernel start)
  const float* cbT;          // [m][S][K]
  float* lut_g;              // [m*K] workspace
  const int32_t* blk_off;    // [2] row blocks of the (one) list
  const uint32_t* packed;    // [blocks][M/2][64]
  const int32_t* pos;        // [blocks*64] scan position, -1 = padding
  const int32_t* pos_to_id;  // NULL: the position is the id
  u64* part;                 // [grid][L] workspace
  int32_t* out_ids;          // [k]
  float* out_dist;           // [k]
  uint32_t epoch;            // 0 / 1: the tag of this call's published words
  int32_t* err;              // [1] mapped host memory: 1 = a poll ran out; 2 = result written (the host may poll this word)
  unsigned long long* prof;  // debugging: phase stamps (100 MHz) of workgroup 0 [0..7] and of the last arriver [8..15]
  int K, L, k, chunk_blocks;
  float sentinel;
  uint32_t sentinel_bits;
};

// (ONE_WG, ONE_WAVES, where the LDS and the hand-off buffer hold what: one_layout.h, which the host reads too)
// ---- hand-offs without counters: every published word carries the call's epoch ----
// Distances are sums of squares: >= +0, so the sign bit of a published float -- and bit 63 of a published (distance,
// position) key -- is free.  A producer stores (value | epoch << 31) with a write-through store and moves on: no drain, no
// arrival counter.  A consumer loads with sc1 loads and accepts a word when its top bit equals the epoch, else loads again
// (bounded).  Every word validates itself, so nothing needs ordering.  The host flips the epoch from call to call as long
// as the calls' shapes are equal (then this call writes exactly the words the previous one wrote, all of which still carry
// the other epoch) and clears the buffer to epoch 0 when the shape changes (freddy_gpu.hip one_buffer()).
__device__ __forceinline__ uint32_t one_tag(float v, uint32_t ep) { return (__float_as_uint(v) & 0x7fffffffu) | (ep << 31); }
__device__ __forceinline__ u64 one_tag_key(u64 key, uint32_t ep) {   // KEY_INF travels as 0x7fff...f
  return ((key == KEY_INF ? 0x7fffffffffffffffull : key) & 0x7fffffffffffffffull) | ((u64)ep << 63);
}
__device__ __forceinline__ u64 one_untag_key(u64 w) {
  const u64 k = w & 0x7fffffffffffffffull;
  return k == 0x7fffffffffffffffull ? KEY_INF : k;
}
static constexpr int ONE_RETRY_LIMIT = 20000;   // rounds of >= 1 us each

// A table of tagged floats -> LDS (tags stripped) by six 16-byte sc1 loads per lane in ONE asm statement that ends with the
// wait (the compiler cannot see that an asm load's result arrives later); words [0, n_valid) are checked, the rest (padding up to a multiple of 4)
// is not.  Returns false when the table did not become valid within the bounded number of rounds.  All threads call.
__device__ __forceinline__ bool one_stage_tagged(const float* g, float* lds, int n_floats, int n_valid, uint32_t ep, int tid, int* retry_sh) {
  typedef uint32_t w4 __attribute__((ext_vector_type(4)));
  const w4* s16 = reinterpret_cast<const w4*>(g);
  w4* d16 = reinterpret_cast<w4*>(lds);
  const int n16 = n_floats >> 2;
  for (int round = 0; round < ONE_RETRY_LIMIT; ++round) {
    if (tid == 0) *retry_sh = 0;
    __syncthreads();
    bool bad = false;
    for (int i0 = 0; i0 < n16; i0 += ONE_WG * 6) {
      w4 t[6];
      const int i = i0 + tid;
      const w4* p0 = s16 + (i < n16 ? i : n16 - 1);
      const w4* p1 = s16 + (i + ONE_WG < n16 ? i + ONE_WG : n16 - 1);
      const w4* p2 = s16 + (i + 2 * ONE_WG < n16 ? i + 2 * ONE_WG : n16 - 1);
      const w4* p3 = s16 + (i + 3 * ONE_WG < n16 ? i + 3 * ONE_WG : n16 - 1);
      const w4* p4 = s16 + (i + 4 * ONE_WG < n16 ? i + 4 * ONE_WG : n16 - 1);
      const w4* p5 = s16 + (i + 5 * ONE_WG < n16 ? i + 5 * ONE_WG : n16 - 1);
      asm volatile(
          "global_load_dwordx4 %0, %6, off sc1\n\t"
          "global_load_dwordx4 %1, %7, off sc1\n\t"
          "global_load_dwordx4 %2, %8, off sc1\n\t"
          "global_load_dwordx4 %3, %9, off sc1\n\t"
          "global_load_dwordx4 %4, %10, off sc1\n\t"
          "global_load_dwordx4 %5, %11, off sc1\n\t"
          "s_waitcnt vmcnt(0)"
          : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5])
          : "v"(p0), "v"(p1), "v"(p2), "v"(p3), "v"(p4), "v"(p5)
          : "memory");
#pragma unroll
      for (int u = 0; u < 6; ++u) {
        const int iu = i + u * ONE_WG;
        if (iu < n16) {
          const int f = iu * 4;
          bad |= (f < n_valid && (t[u].x >> 31) != ep) || (f + 1 < n_valid && (t[u].y >> 31) != ep) ||
                 (f + 2 < n_valid && (t[u].z >> 31) != ep) || (f + 3 < n_valid && (t[u].w >> 31) != ep);
          w4 v = t[u];
          v.x &= 0x7fffffffu; v.y &= 0x7fffffffu; v.z &= 0x7fffffffu; v.w &= 0x7fffffffu;
          d16[iu] = v;
        }
      }
    }
    if (bad) *retry_sh = 1;
    __syncthreads();
    const int again = *retry_sh;
    __syncthreads();   // (everyone has read the flag before the next round clears it)
    if (!again) return true;
    __builtin_amdgcn_s_sleep(16);
  }
  return false;
}

// Smallest key over the wave's lanes [0, 1 << STEPS) (the other lanes are ignored), in every lane.  The minimum of the
// distance words decides almost every time (32-bit exchanges); only lanes that tie on it compare their position words.
template <int STEPS>
__device__ __forceinline__ u64 one_wave_min(u64 key) {
  const uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
  uint32_t m = hi;
#pragma unroll
  for (int st = 0; st < STEPS; ++st) m = min(m, (uint32_t)lane_xor((int)m, 1 << st));
  m = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
  const u64 in_range = STEPS == 6 ? ~0ull : ((1ull << (1 << (STEPS < 6 ? STEPS : 0))) - 1ull);
  const u64 tied = __ballot(hi == m) & in_range;
  uint32_t ml;
  if (__popcll(tied) == 1) {
    ml = (uint32_t)__builtin_amdgcn_readlane((int)lo, __builtin_ctzll(tied));
  } else {
    ml = hi == m ? lo : 0xffffffffu;
#pragma unroll
    for (int st = 0; st < STEPS; ++st) ml = min(ml, (uint32_t)lane_xor((int)ml, 1 << st));
    ml = (uint32_t)__builtin_amdgcn_readfirstlane((int)ml);
  }
  return ((u64)m << 32) | (u64)ml;
}

// The L smallest keys of n <= 8 ascending lists held in LDS (list x: rows[r * stride + x], r = 0.., KEY_INF where a list
// ends), ascending, lane r <- rank r (KEY_INF beyond L): lane x walks list x, each round the smallest head is taken and
// its lane advances.  Keys are unique (the position is part of the key).
__device__ __forceinline__ u64 one_multiway(const u64* rows, int stride, int n, int L, int lane) {
  int h = 0;
  u64 head = lane < n ? rows[lane] : KEY_INF;
  u64 out = KEY_INF;
  for (int r = 0; r < L; ++r) {
    const u64 mn = one_wave_min<3>(head);
    if (mn == KEY_INF) break;   // (uniform)
    if (lane == r) out = mn;
    if (head == mn) {
      ++h;
      head = h < L ? rows[(size_t)h * stride + lane] : KEY_INF;
    }
  }
  return out;
}

// The same over up to 256 lists with ONE wave: lane x walks the lists x, x + 64, x + 128, x + 192 (rows[r * n + list]).
__device__ __forceinline__ u64 one_multiway4(const u64* rows, int n, int L, int lane) {
  int h[4] = {0, 0, 0, 0};
  u64 head[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) head[t] = lane + 64 * t < n ? rows[lane + 64 * t] : KEY_INF;
  u64 out = KEY_INF;
  for (int r = 0; r < L; ++r) {
    const u64 m01 = umin64(head[0], head[1]), m23 = umin64(head[2], head[3]);
    const u64 mine = umin64(m01, m23);
    const u64 mn = one_wave_min<6>(mine);
    if (mn == KEY_INF) break;   // (uniform)
    if (lane == r) out = mn;
    if (mine == mn) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (head[t] == mn) {
          ++h[t];
          head[t] = h[t] < L ? rows[(size_t)h[t] * n + lane + 64 * t] : KEY_INF;
        }
      }
    }
  }
  return out;
}

// ---------------------------------------------------------------------------------------
// The stages both kernels run, each once.  (`a`, `tid`, `w` and STAMP_LAST are the kernel's.)
// ---------------------------------------------------------------------------------------
#define ONE_STAMP(i) do { if (a.prof && tid == 0 && w == 0) a.prof[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define ONE_STAMP_LAST(i) do { if (a.prof && tid == 0) a.prof[STAMP_LAST + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define ONE_GIVE_UP() do { if (tid == 0) a.err[0] = 1; return; } while (0)   // a bounded poll ran out

template <typename T>
__device__ __forceinline__ T* one_at(unsigned char* smem, OneRegion r) { return reinterpret_cast<T*>(smem + r.off); }

// Slice poll.  A table of ONE_M * K words was written in slices of cw codes, n_slot per position: wave 0 polls the first word
// of every slice (a few hundred bytes) until all carry this call's epoch; the full table is then staged and verified word by
// word (and staged again in the rare case that a slice was still in flight).  All threads call; false: the poll ran out.
// (a: the kernel's arguments -- the epoch is read from them where it is compared: handed in as a value it stays in a register
// over the loop, which costs pq_one_kernel two more spilled SGPRs than tests/golden/codegen_ceilings.json allows)
template <typename A>
__device__ __forceinline__ bool one_poll_slices(const A& a, float* lut_g, int n_slot, int cw, int K, int wave, int lane, int* flag_sh) {
  if (wave == 0) {
    bool ok = false;
    for (int round = 0; round < ONE_RETRY_LIMIT && !ok; ++round) {
      bool bad = false;
      for (int unit = lane; unit < ONE_M * n_slot; unit += 64) {
        const int p = unit / n_slot, c0 = (unit - p * n_slot) * cw;
        if (c0 < K) bad |= (__hip_atomic_load(reinterpret_cast<uint32_t*>(lut_g) + p * K + c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 31) != a.epoch;
      }
      ok = __ballot(bad) == 0ull;
      if (!ok) __builtin_amdgcn_s_sleep(8);
    }
    if (lane == 0) *flag_sh = ok ? 1 : 0;
  }
  __syncthreads();
  return *flag_sh != 0;
}

// Scan of the row blocks [b0, b1) by the workgroup's waves (wave x: b0 + x, b0 + x + ONE_WAVES, ...), adc_scan_kernel's loop:
// a ring of PF row blocks per wave in flight, the ADC sum in position order (index_utils.c:1126-1133), WaveSelect of the L
// smallest (distance, position) keys.  prime() requests the first PF blocks -- the kernels issue it BEFORE they poll for the
// table, so that the rows fly across the hand-off; run() needs the table in LDS.
template <int PF>
struct OneScan {
  static constexpr int M2T = ONE_M / 2;
  RowBlock<M2T> ring[PF];
  const uint32_t* packed;
  const int32_t* pos;
  int b, b1, lane;

  __device__ __forceinline__ void init(const uint32_t* packed_, const int32_t* pos_, int b0, int b1_, int wave, int lane_) {
    packed = packed_; pos = pos_; b = b0 + wave; b1 = b1_; lane = lane_;
  }
  __device__ __forceinline__ void fetch(RowBlock<M2T>& rb, int blk) const {
    const int bc = blk < b1 ? blk : b1 - 1;           // (past the end: a repeat of the last block, never used)
    const uint32_t* pk = packed + (size_t)bc * M2T * 64 + lane;
#pragma unroll
    for (int j = 0; j < M2T; ++j) rb.w[j] = pk[j * 64];
    rb.p = pos[(size_t)bc * 64 + lane];
  }
  __device__ __forceinline__ void prime() {
#pragma unroll
    for (int u = 0; u < PF; ++u) fetch(ring[u], b + u * ONE_WAVES);
  }
  // COUNT: returns this wave's rows below the sentinel (the accepted-row count, freddy.c:971), in every lane; else 0.
  template <bool COUNT>
  __device__ __forceinline__ int run(const float* lut, int K, WaveSelect<1>& sel, u64 sentinel_key) {
    int accepted = 0;
    for (; b < b1; b += PF * ONE_WAVES) {
      u64 keys[PF];
      uint32_t mn = 0xffffffffu;   // this lane's smallest distance (bits) among the group's valid rows
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const RowBlock<M2T> cur = ring[u];
        const int bu = b + u * ONE_WAVES;
        if (bu + PF * ONE_WAVES < b1) fetch(ring[u], bu + PF * ONE_WAVES);   // (wave-uniform)
        keys[u] = KEY_INF;
        if (bu < b1) {   // wave-uniform
          float dist = 0.0f;
#pragma unroll
          for (int l = 0; l < ONE_M; ++l) {
            const uint32_t code = (l & 1) ? (cur.w[l >> 1] >> 16) : (cur.w[l >> 1] & 0xffffu);
            dist = dist + lut[l * K + code];
          }
          if (cur.p >= 0) {
            keys[u] = make_key(dist, (uint32_t)cur.p);
            mn = min(mn, __float_as_uint(dist));
          }
          if (COUNT) accepted += __popcll(__ballot(cur.p >= 0 && keys[u] < sentinel_key));
        }
      }
      // L rows of the group are at most as far as the L-th smallest lane minimum: nothing farther can be among the L
      // smallest keys (one 32-bit sort instead of a 64-bit sort + merge per 64 passing keys while the threshold is loose)
      const uint32_t dL = (uint32_t)__builtin_amdgcn_readlane((int)wave_sort32(mn), sel.L - 1);
      const u64 bound = ((u64)dL << 32) | 0xffffffffull;
      if (bound < sel.tau) sel.tau = bound;
#pragma unroll
      for (int u = 0; u < PF; ++u)
        if (b + u * ONE_WAVES < b1) sel.push(keys[u], keys[u] != KEY_INF);
    }
    sel.finish();
    return accepted;
  }
};

// Publish.  The eight waves' lists meet in LDS (the table is dead by now), wave 0 merges them and publishes the workgroup's
// list rank-major: part[r * G + w].  cnt_g != NULL: the workgroup's accepted-row count *acc_sh rides along, tagged.
__device__ __forceinline__ void one_publish(u64* lists, u64 wave_list, int L, u64* part, uint32_t* cnt_g, const int* acc_sh, int G, int w,
                                            uint32_t ep, int wave, int lane) {
  __syncthreads();
  lists[lane * ONE_WAVES + wave] = wave_list;   // [64 ranks][ONE_WAVES]
  __syncthreads();
  if (wave == 0) {
    const u64 mine = one_multiway(lists, ONE_WAVES, ONE_WAVES, L, lane);
    if (lane < L) __hip_atomic_store(part + (size_t)lane * G + w, one_tag_key(mine, ep), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cnt_g && lane == 0) __hip_atomic_store(cnt_g + w, (uint32_t)*acc_sh | (ep << 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Collect, workgroup 0: the G published lists -> all[L][G] (as published), re-read until every word carries this call's
// epoch.  cnt_g != NULL: the workgroups' counts are checked too and summed into *acc_sh.  False: the poll ran out.
__device__ __forceinline__ bool one_collect(u64* part, u64* all, int total, uint32_t* cnt_g, int G, uint32_t ep, int tid, int* retry_sh, int* acc_sh) {
  bool ok = false;
  for (int round = 0; round < ONE_RETRY_LIMIT && !ok; ++round) {
    if (tid == 0) { *retry_sh = 0; if (cnt_g) *acc_sh = 0; }
    __syncthreads();
    bool bad = false;
    for (int i = tid; i < total; i += ONE_WG) {
      const u64 word = __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      bad |= (uint32_t)(word >> 63) != ep;
      all[i] = one_untag_key(word);
    }
    if (cnt_g) {
      int cnt = 0;
      for (int i = tid; i < G; i += ONE_WG) {
        const uint32_t word = __hip_atomic_load(cnt_g + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bad |= (word >> 31) != ep;
        cnt += (int)(word & 0x7fffffffu);
      }
      if (cnt) atomicAdd(acc_sh, cnt);
    }
    if (bad) *retry_sh = 1;
    __syncthreads();
    ok = *retry_sh == 0;
    __syncthreads();   // (everyone has read the flag before the next round clears it)
    if (!ok) __builtin_amdgcn_s_sleep(8);
  }
  return ok;
}

// Finish, one wave: the list goes to (mapped host) memory, and only when it is there the word the host polls.
__device__ __forceinline__ void one_finish(int32_t* out_ids, float* out_dist, int k, int32_t id_slot, float d_slot, int32_t* err, int verdict,
                                           int lane, unsigned long long* stamp) {
  if (lane < k) {
    out_ids[lane] = id_slot;
    out_dist[lane] = d_slot;
  }
  if (stamp && lane == 0) *stamp = __builtin_amdgcn_s_memrealtime();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  if (lane == 0) __hip_atomic_store(err, verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int S>
__global__ __launch_bounds__(ONE_WG) void pq_one_kernel(OneArgs a) {
  constexpr int M = ONE_M, STAMP_LAST = 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int flag_sh, retry_sh;
  const int K = a.K;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int w = blockIdx.x, G = gridDim.x;
  const OneLayout lay{K, 0, 1, a.L, G};
  ONE_STAMP(0);

  // (the first row blocks of every wave are requested between the drain of the table slice and the barrier's poll)
  const int b0 = a.blk_off[0] + w * a.chunk_blocks;
  int b1 = a.blk_off[1];
  if (b0 + a.chunk_blocks < b1) b1 = b0 + a.chunk_blocks;
  OneScan<8> scan;
  scan.init(a.packed, a.pos, b0, b1, wave, lane);
  // ---- 1. this workgroup's slice of the table: unit = (position, range of codes) ----
  {
    static_assert(M * S == ONE_D, "the query travels as 300 floats");
    const int n_slot = G >= M ? G / M : 1, cw = (K + n_slot - 1) / n_slot;
    for (int unit = w; unit < M * n_slot; unit += G) {
      const int p = unit / n_slot, c0 = (unit - p * n_slot) * cw;   // (p: workgroup-uniform)
      const int c1 = c0 + cw < K ? c0 + cw : K;
      for (int c = c0 + tid; c < c1; c += ONE_WG) {
        float cb[S];
#pragma unroll
        for (int j = 0; j < S; ++j) cb[j] = a.cbT[((size_t)p * S + j) * K + c];
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < S; ++j) {
          const float t = a.qv[p * S + j] - cb[j];
          const float pr = t * t;
          acc = acc + pr;
        }
        __hip_atomic_store(reinterpret_cast<uint32_t*>(a.lut_g) + p * K + c, one_tag(acc, a.epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    ONE_STAMP(1);
    if (b0 < b1) scan.prime();   // (the first row blocks of every wave: in flight while the table arrives)
    if (!one_poll_slices(a, a.lut_g, n_slot, cw, K, wave, lane, &flag_sh)) ONE_GIVE_UP();
    ONE_STAMP(2);
  }

  // ---- 2. the table -> LDS, this workgroup's chunk of row blocks ----
  WaveSelect<1> sel;
  const u64 sentinel_key = (u64)a.sentinel_bits << 32;   // key < this  <=>  dist < sentinel
  sel.init(one_at<u64>(smem, lay.wave_rows()) + wave * 64, sentinel_key, a.L);
  if (b0 < b1) {   // workgroup-uniform
    float* lut = one_at<float>(smem, lay.table());
    if (!one_stage_tagged(a.lut_g, lut, M * K, M * K, a.epoch, tid, &retry_sh)) ONE_GIVE_UP();
    ONE_STAMP(3);
    scan.run<false>(lut, K, sel, sentinel_key);
  }
  ONE_STAMP(4);
  one_publish(one_at<u64>(smem, lay.lists()), sel.acc[0], a.L, a.part, nullptr, nullptr, G, w, a.epoch, wave, lane);
  ONE_STAMP(5);
  if (w != 0) return;   // (workgroup 0 collects the lists)
  ONE_STAMP_LAST(0);

  // ---- 3. the last workgroup: multiway merge of the G lists (lane <-> list, 64 lists per wave), replay ----
  u64* all = one_at<u64>(smem, lay.all_lists());   // behind the waves' result rows
  if (!one_collect(a.part, all, G * a.L, nullptr, G, a.epoch, tid, &retry_sh, nullptr)) ONE_GIVE_UP();
  // one wave, lane <-> the lists x = lane, lane + 64, ... (<= 4 for 256 CUs): each round takes the smallest head
  if (wave != 0) return;
  ONE_STAMP_LAST(1);
  const u64 top = one_multiway4(all, G, a.L, lane);
  // The reference's pass inserts in scan order behind a guard "dist < maxDist" (freddy.c:128-131): wave_list_from_sorted
  float d_slot = a.sentinel;
  int32_t id_slot = -1;
  wave_list_from_sorted(d_slot, id_slot, a.k, top, a.L, [&](u64 key) { return key_dist(key) < a.sentinel; },
                        [&](uint32_t p) { return a.pos_to_id ? a.pos_to_id[p] : (int32_t)p; });
  one_finish(a.out_ids, a.out_dist, a.k, id_slot, d_slot, a.err, 2, lane, a.prof ? a.prof + STAMP_LAST + 2 : nullptr);
}

// ---------------------------------------------------------------------------------------
// ivfadc_search for ONE query as a single launch: the reference's own call shape (freddy.c:174-393).  The generic path is
// five dependent launches (coarse_small -> probe_plan -> lut_build -> adc_scan -> merge_replay).  Here:
//   A. every workgroup: the coarse distances of its <= ceil(C / G) cells (the centroid rows staged in LDS, one lane per
//      cell walks the 300 dimensions in order: squareDistance, index_utils.c:500-508) -> published -> grid barrier;
//   B. every workgroup, redundantly: the W nearest cells below the cell limit by the reference's guarded insertion in
//      cell order (probe_plan_kernel's selection: freddy.c:266-283) -- every workgroup arrives at the same list;
//   C. the W tables lut[i][pos*K + code] = squareDistance((q - coarse[cell_i])_pos, cb[pos][code]) (freddy.c:296-303,
//      index_utils.c:445-455) in slices -> published -> grid barrier;
//   D. workgroup (item, part): the item's table -> LDS, its share of the cell's row blocks (adc_scan_kernel's loop),
//      its L smallest keys -> published; the accepted-row count (freddy.c:971) by atomics;
//   E. the last arriver: merge, guarded insertion in scan (= id) order, the list; the query's "found" decides whether the
//      reference would probe again (freddy.c:377): then the host runs the multi-round path instead (flag 3).
// ---------------------------------------------------------------------------------------
struct IvfOneArgs {
  float qv[300];
  const float* coarse;       // [C][d]
  const float* cbT;          // [m][S][K]
  const int32_t* list_off;   // [C+1]
  const int32_t* blk_off;    // [C+1]
  const uint32_t* packed;
  const int32_t* pos;        // row ids (the scan position of an IVF table), -1 = padding
  float* dist_g;             // [C] workspace
  float* lut_g;              // [W][m*K] workspace
  u64* part;                 // [L][grid] workspace
  int32_t* out_ids;          // [k] mapped host memory
  float* out_dist;           // [k]
  uint32_t* cnt_g;           // [grid] workspace: every workgroup's accepted-row count (tagged)
  uint32_t epoch;            // 0 / 1: the tag of this call's published words (pq_one_kernel)
  int32_t* err;              // mapped host word: 1 = a poll ran out, 2 = list written, 3 = list written, the reference would probe again
  unsigned long long* prof;  // debugging: phase stamps (100 MHz) of workgroup 0 [0..9] and of the last arriver [10..12]
  int C, K, W, L, k, found_rule;
  float cell_limit, sentinel;
  uint32_t sentinel_bits;
};

template <int S>
__global__ __launch_bounds__(ONE_WG) void ivf_one_kernel(IvfOneArgs a) {
  constexpr int M = ONE_M, D = M * S, STAMP_LAST = 10;
  static_assert(D == ONE_D, "the query travels as 300 floats");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int flag_sh, retry_sh, acc_sh;
  __shared__ int32_t cells_sh[32];
  const int K = a.K, lutN = M * K, C = a.C, W = a.W;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int w = blockIdx.x, G = gridDim.x;
  const OneLayout lay{K, C, W, a.L, G};
  ONE_STAMP(0);

  // ---- A. coarse distances of the cells w, w + G, ... ----
  {
    const int n_mine = w < C ? (C - w + G - 1) / G : 0;
    float* crow = one_at<float>(smem, lay.coarse_rows(n_mine));   // [cells of this workgroup][D], then the query
    float* qs = one_at<float>(smem, lay.query(n_mine));
    for (int i = tid; i < n_mine * D; i += ONE_WG) {
      const int ci = i / D, j = i - ci * D;
      crow[i] = a.coarse[(size_t)(w + ci * G) * D + j];
    }
    if (tid < D) qs[tid] = a.qv[tid];
    __syncthreads();
    // one lane per cell, the cells of a workgroup on different waves; 16-byte LDS reads, the chain in dimension order
    for (int ci = wave; ci < n_mine; ci += ONE_WAVES) {
      if (lane == 0) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4* c4 = reinterpret_cast<const f4*>(crow + ci * D);
        const f4* q4 = reinterpret_cast<const f4*>(qs);
        float acc = 0.0f;
#pragma unroll 5
        for (int i = 0; i < D / 4; ++i) {
          const f4 cv = c4[i], qv = q4[i];
          { const float t = qv.x - cv.x; const float pr = t * t; acc = acc + pr; }
          { const float t = qv.y - cv.y; const float pr = t * t; acc = acc + pr; }
          { const float t = qv.z - cv.z; const float pr = t * t; acc = acc + pr; }
          { const float t = qv.w - cv.w; const float pr = t * t; acc = acc + pr; }
        }
        __hip_atomic_store(reinterpret_cast<uint32_t*>(a.dist_g) + (w + ci * G), one_tag(acc, a.epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (tid == 0) acc_sh = 0;
    __syncthreads();   // (the centroid rows in LDS are dead)
    ONE_STAMP(1);
  }

  // ---- B. the W nearest cells (every workgroup for itself) ----
  int my_rows = 0;      // wave 0: the rows of this lane's cell (summed by the last arriver)
  bool my_have = false;
  {
    float* dl = one_at<float>(smem, lay.cell_dist());   // [C rounded up to 4]
    if (!one_stage_tagged(a.dist_g, dl, (C + 3) & ~3, C, a.epoch, tid, &retry_sh)) ONE_GIVE_UP();
    ONE_STAMP(2);
    if (wave == 0) {
      const int L2 = 2 * W;
      const u64 limit = (u64)__float_as_uint(a.cell_limit) << 32;
      // the L2-th smallest lane minimum bounds the L2-th smallest distance: the selection starts with a tight threshold
      uint32_t mn = 0xffffffffu;
      for (int j = lane; j < C; j += 64) mn = min(mn, __float_as_uint(dl[j]));
      const uint32_t dL = (uint32_t)__builtin_amdgcn_readlane((int)wave_sort32(mn), L2 - 1);
      const u64 bound = ((u64)dL << 32) | 0xffffffffull;
      WaveSelect<1> sel;
      sel.init(one_at<u64>(smem, lay.cell_row()), bound < limit ? bound : limit, L2);
      for (int base = 0; base < C; base += 64) {
        const int j = base + lane;
        sel.push(make_key(dl[j < C ? j : C - 1], (uint32_t)j), j < C);
      }
      sel.finish();
      // the reference keeps its W nearest cells by guarded insertion in cell order (freddy.c:266-283)
      float d_slot = a.cell_limit;
      int32_t c_slot = -1;
      wave_list_from_sorted(d_slot, c_slot, W, lane < L2 ? sel.acc[0] : KEY_INF, L2, [&](u64 key) { return key < limit; },
                            [](uint32_t cell) { return (int32_t)cell; });
      my_have = lane < W && c_slot >= 0;
      my_rows = my_have ? (a.list_off[c_slot + 1] - a.list_off[c_slot]) : 0;
      if (lane < 32) cells_sh[lane] = lane < W ? c_slot : -1;
    }
    __syncthreads();
  }

  ONE_STAMP(3);
  // this workgroup's share of the scan: item = w / P, part = w % P of the item's row blocks
  const int P = G >= W ? G / W : 1;
  const int my_item = w / P;
  const int my_cell = my_item < W ? cells_sh[my_item] : -1;
  int b0 = 0, b1 = 0;
  if (my_cell >= 0) {
    const int c0 = a.blk_off[my_cell], c1 = a.blk_off[my_cell + 1];
    const int chunk = (c1 - c0 + P - 1) / P;
    b0 = c0 + (w - my_item * P) * chunk;
    b1 = b0 + chunk < c1 ? b0 + chunk : c1;
  }
  OneScan<4> scan;
  scan.init(a.packed, a.pos, b0, b1, wave, lane);

  // ---- C. the items' tables in slices: unit = (item, position, range of codes) ----
  {
    const int n_slot = G >= W * M ? G / (W * M) : 1, cw = (K + n_slot - 1) / n_slot;
    for (int unit = w; unit < W * M * n_slot; unit += G) {
      const int i = unit / (M * n_slot), rem = unit - i * (M * n_slot);
      const int p = rem / n_slot, c0 = (rem - p * n_slot) * cw;   // (i, p: workgroup-uniform)
      const int cell = __builtin_amdgcn_readfirstlane(cells_sh[i]);
      const int c1 = c0 + cw < K ? c0 + cw : K;
      if (cell < 0) {   // no such item this time: its words still get this call's epoch (the next call may read them)
        for (int c = c0 + tid; c < c1; c += ONE_WG)
          __hip_atomic_store(reinterpret_cast<uint32_t*>(a.lut_g) + (size_t)i * lutN + p * K + c, a.epoch << 31, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        continue;
      }
      const float* co = a.coarse + (size_t)cell * D + (size_t)p * S;
      for (int c = c0 + tid; c < c1; c += ONE_WG) {
        float cb[S];
#pragma unroll
        for (int j = 0; j < S; ++j) cb[j] = a.cbT[((size_t)p * S + j) * K + c];
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < S; ++j) {
          const float rj = a.qv[p * S + j] - co[j];   // (the residual: one binary32 subtraction, freddy.c:296-303)
          const float t = rj - cb[j];
          const float pr = t * t;
          acc = acc + pr;
        }
        __hip_atomic_store(reinterpret_cast<uint32_t*>(a.lut_g) + (size_t)i * lutN + p * K + c, one_tag(acc, a.epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    ONE_STAMP(4);
    if (b0 < b1) {   // (the first row blocks in flight while the item's table arrives: the slices of this workgroup's item are polled)
      scan.prime();
      if (!one_poll_slices(a, a.lut_g + (size_t)my_item * lutN, n_slot, cw, K, wave, lane, &flag_sh)) ONE_GIVE_UP();
    }
    ONE_STAMP(5);
  }

  // ---- D. the item's table -> LDS, this workgroup's row blocks ----
  WaveSelect<1> sel;
  const u64 sentinel_key = (u64)a.sentinel_bits << 32;
  sel.init(one_at<u64>(smem, lay.wave_rows()) + wave * 64, sentinel_key, a.L);
  int accepted = 0;
  if (b0 < b1) {   // workgroup-uniform
    float* lut = one_at<float>(smem, lay.table());
    if (!one_stage_tagged(a.lut_g + (size_t)my_item * lutN, lut, lutN, lutN, a.epoch, tid, &retry_sh)) ONE_GIVE_UP();
    ONE_STAMP(6);
    accepted = scan.run<true>(lut, K, sel, sentinel_key);
  }
  ONE_STAMP(7);
  if (lane == 0 && accepted) atomicAdd(&acc_sh, accepted);
  one_publish(one_at<u64>(smem, lay.lists()), sel.acc[0], a.L, a.part, a.cnt_g, &acc_sh, G, w, a.epoch, wave, lane);
  ONE_STAMP(8);
  if (w != 0) return;   // (workgroup 0 collects the lists)
  ONE_STAMP_LAST(0);

  // ---- E. the last workgroup: merge, replay, the list ----
  u64* all = one_at<u64>(smem, lay.all_lists());
  if (!one_collect(a.part, all, G * a.L, a.cnt_g, G, a.epoch, tid, &retry_sh, &acc_sh)) ONE_GIVE_UP();
  if (wave != 0) return;
  ONE_STAMP_LAST(1);
  const u64 top = one_multiway4(all, G, a.L, lane);
  float d_slot = a.sentinel;
  int32_t id_slot = -1;
  wave_list_from_sorted(d_slot, id_slot, a.k, top, a.L, [&](u64 key) { return key_dist(key) < a.sentinel; },
                        [](uint32_t id) { return (int32_t)id; });
  // "found" of the first round: fewer than k and a cell was probed -> the reference probes the next W cells; the host runs
  // that path (round_end's rule)
  const int rows = wave_round_rows(my_have, my_rows);
  const int verdict = round_again(round_found(a.found_rule == 1, acc_sh, rows), a.k, rows) ? 3 : 2;
  one_finish(a.out_ids, a.out_dist, a.k, id_slot, d_slot, a.err, verdict, lane, a.prof ? a.prof + STAMP_LAST + 2 : nullptr);
}
#undef ONE_STAMP
#undef ONE_STAMP_LAST
#undef ONE_GIVE_UP

}  // namespace freddy
