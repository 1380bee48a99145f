// assign_exact_walk.inc -- the all-exact walk of one wave over all queries, ONE copy: the 16-accumulator loop of the binary32 chain
// (dot_chain.h's gather tile with its query tile beside it).  A FRAGMENT, not a header: assign_exact_kernel (assign.h) and
// assign_redo_kernel (assign_filter.h) include it inside their bodies.  (As a device function the same text costs assign_exact_kernel
// 24 more VGPRs -- 176 against the 152 of tests/golden/assign_codegen_ceilings.json: the inliner reorders what the scheduler sees.)
// In scope at the include: a.rows [N][d], a.queries [Q][d], a.Q; int d, lane; int32_t row (the lane's table row, < 0: none); the LDS
// tiles float tile[TILE_FLOATS], qs[TILE_QFLOATS].  It defines best_ord, best_q, best_sim: the first query under assign_ord DESC.
  uint32_t best_ord = 0;   // (no similarity's image)
  int32_t best_q = -1;
  float best_sim = -__builtin_huge_valf();
  if (__ballot(row >= 0) != 0ull) {
    const bool vec4 = (d & 3) == 0;
    for (int q0 = 0; q0 < a.Q; q0 += TILE_QT) {
      float acc[TILE_QT];
#pragma unroll
      for (int t = 0; t < TILE_QT; ++t) acc[t] = 0.0f;
      for (int c0 = 0; c0 < d; c0 += TILE_DCH) {
        const int nd = (d - c0 < TILE_DCH) ? d - c0 : TILE_DCH;
        float4 v[8], qv[2];
#pragma unroll
        for (int it = 0; it < 8; ++it) v[it] = tile_row_piece(a.rows, row, it, lane, d, c0, nd, vec4);
#pragma unroll
        for (int it = 0; it < 2; ++it) qv[it] = tile_query_piece(a.queries, a.Q, q0, it, lane, d, c0, nd, vec4);
#pragma unroll
        for (int it = 0; it < 8; ++it) tile_store_row_piece(tile, v[it], it, lane);
#pragma unroll
        for (int it = 0; it < 2; ++it) tile_store_query_piece(qs, qv[it], it, lane);
        wave_lds_sync();
        const float* col = tile + lane;   // (the 16-accumulator walk, kept in place for registers: dot_chain.h)
        if (nd == TILE_DCH) {
#pragma unroll
          for (int j = 0; j < TILE_DCH; ++j) {
            const float x = col[j * TILE_STRIDE];
#pragma unroll
            for (int t4 = 0; t4 < TILE_QT / 4; ++t4) {
              const float4 qq = *reinterpret_cast<const float4*>(qs + tile_qrow(j) * TILE_QT + t4 * 4);
              float p;
              p = qq.x * x; acc[t4 * 4 + 0] = acc[t4 * 4 + 0] + p;   // core_functions.c:77: scalar += v1[i] * v2[i]
              p = qq.y * x; acc[t4 * 4 + 1] = acc[t4 * 4 + 1] + p;
              p = qq.z * x; acc[t4 * 4 + 2] = acc[t4 * 4 + 2] + p;
              p = qq.w * x; acc[t4 * 4 + 3] = acc[t4 * 4 + 3] + p;
            }
          }
        } else {
          for (int j = 0; j < nd; ++j) {
            const float x = col[j * TILE_STRIDE];
#pragma unroll
            for (int t4 = 0; t4 < TILE_QT / 4; ++t4) {
              const float4 qq = *reinterpret_cast<const float4*>(qs + tile_qrow(j) * TILE_QT + t4 * 4);
              float p;
              p = qq.x * x; acc[t4 * 4 + 0] = acc[t4 * 4 + 0] + p;
              p = qq.y * x; acc[t4 * 4 + 1] = acc[t4 * 4 + 1] + p;
              p = qq.z * x; acc[t4 * 4 + 2] = acc[t4 * 4 + 2] + p;
              p = qq.w * x; acc[t4 * 4 + 3] = acc[t4 * 4 + 3] + p;
            }
          }
        }
        wave_lds_sync();
      }
#pragma unroll
      for (int t = 0; t < TILE_QT; ++t) {   // ascending query index: only a strictly larger similarity replaces the best
        const uint32_t o = assign_ord(acc[t]);
        if (q0 + t < a.Q && o > best_ord) { best_ord = o; best_q = q0 + t; best_sim = acc[t]; }
      }
    }
  }
