// ivf_host.h -- ivf_run.h for the units that launch kernels of the chain (ivf_select.hip, ivf_scan.hip, generic.hip, pq.hip), and
// the arguments of the merge they share.
// (The kernel choosers stay in the unit that launches the family: a unit that sees a chooser emits the device code of all it names.)
#pragma once

#include "ivf_run.h"
#include "kernels.h"

// ---- merge_replay_kernel's arguments -----------------------------------------------------------------------------------------
// one round over everything, no state: `parts` lists of L keys per query -> the queries' final lists
static MergeArgs merge_args_flat(const u64* part, int Q, int parts, int L, int k, float sentinel, const int32_t* pos_to_id,
                                 int32_t* out_ids, float* out_dist) {
  MergeArgs ma{};
  ma.part = part; ma.pos_to_id = pos_to_id; ma.out_ids = out_ids; ma.out_dist = out_dist;
  ma.n_active = Q; ma.parts_per_query = parts; ma.L = L; ma.k = k; ma.first_round = 1; ma.sentinel = sentinel;
  return ma;
}
// a probing round of r: the carried lists, the found counts and the queries that need another round
static MergeArgs merge_args_round(const IvfRun& r, const PlanArgs& pa, const u64* part, int parts, const int32_t* cand_count) {
  MergeArgs ma = merge_args_flat(part, r.n_active, parts, r.L, r.k, r.sentinel, nullptr, r.d_out_ids, r.d_out_dist);
  ma.active = r.active; ma.round_rows = pa.round_rows; ma.cand_count = cand_count;
  ma.found = r.ws->w_found.as<int32_t>(); ma.next_active = r.next; ma.n_next = r.ws->w_cnt.as<int32_t>(); ma.status = r.d_status;
  ma.found_rule = r.found_rule; ma.first_round = r.first() ? 1 : 0;
  return ma;
}
