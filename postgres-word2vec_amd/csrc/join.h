// join.h -- kNN-join: the body of ivpq_search_in (ivpq_search_in.c:61-699) on gfx950.
//
// Files
//   join_index.h    what the handle holds: the pinned tables, the named workspaces, the error buffer
//   join_kernels.h  GPU: the kernels below with their argument records, but for ...
//   join_traverse.h GPU: ... join_traverse_kernel, and the confidence expression both sides evaluate
//   join_host.h     host: the reference's heap for the queries the device does not decide, the worker pool
//   join_run.h      host: the run record of a call (JoinRun) and its stages; join_run() is the loop (needs internal.h: join.hip
//                   includes it, this header does not)
//
// Split of work
//   GPU  sub_dist_kernel : the 2 x coarse_codes sub-distances of every query to the
//                          multi-index centroids (index_utils.c:297-305), fp32 sequential.
//        sub_dist_rows_kernel : the same for queries that are rows of a device table (freddy_gpu_knn_join_ids): it gathers
//                          the row while it computes (join_run.h JoinQueries has the three sources of a call's queries).
//   GPU  join_traverse_kernel : multi-index cell selection with statistics (index_utils.c:252-443)
//        for up to 1024 cells, one wave per query.  The reference's heap pops the cells in ascending
//        d0[c0] + d1[c1]; with no two equal keys among the cells a query takes (and the first it leaves)
//        that sequence IS the sorted order, so the wave sorts the 1024 keys, forms the running sum of the
//        cells' statistics in that order (sequential binary32 adds, as :424) and finds the first count n
//        whose getConfidenceHyp (:673-682) reaches the confidence.  The HOST's libm keeps the last word:
//        it evaluates the reference's expression at the stop the device proposes and one step before it
//        (the confidence is non-decreasing in the running sum); a query whose check fails, or whose
//        prefix holds two equal keys (the heap's order among equals is history-dependent), is traversed
//        on the host exactly as before (join_select_cells).  More than 1024 cells: the host path.
//   host "WHERE coarse_id IN (...) AND id IN (...)" (ivpq_search_in.c:352-401): targets are
//        bucketed by cell once per call; a query's candidates are the buckets of its cells.
//   GPU  join_query_kernel : one workgroup per query: LUT (index_utils.c:445-455, pair LUT
//        :457-475) in LDS, ADC / exact distances of the query's candidates, selection by
//        (distance, row) key, post verification (index_utils.c:477-498) and the final
//        insertion replay -- everything that touches a distance.
//   host alpha-doubling retry loop (ivpq_search_in.c:299-684), target-count skip rule
//        (:553-557), re-queue of queries whose list is still at MAX_DIST (:639-669).
//
// Closed forms used on the device (proved in DESIGN.md, checked against the oracle's
// literal restatement in tests/):
//   method 0/1: final list = insertion replay, in ascending id, over the 2k smallest
//               (distance, id) keys of the query's candidates.
//   method 2:   the reference's append-buffer-and-qsort (updateTopKPVFast/reorderTopKPV,
//               ivpq_search_in.c:40-57) keeps exactly the k*pvf smallest (ADC distance,
//               arrival) keys, ascending -- given a stable qsort (glibc <= 2.36) -- and
//               postverify walks them in that order.
#pragma once

#include "join_kernels.h"
#include "join_traverse.h"
#include "join_host.h"
