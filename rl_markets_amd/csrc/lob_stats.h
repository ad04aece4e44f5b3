// Episode statistics (include/lob_engine.h lob_episode_stats): the record arithmetic shared by the reduction kernels
// (lob_kernels.h episode_stats_partial_kernel / episode_stats_final_kernel) and the host's lob_episode_stats_merge, so that a
// merge on the host and a merge on the device are the same operations.
#ifndef LOB_STATS_H
#define LOB_STATS_H

#include <math.h>
#include <stdint.h>

#include "lob_stream.h"

// The empty group: the neutral element of stats_merge
LOB_HD void stats_identity(lob_episode_record& r, int32_t group) {
    r.group = group;
    r.n_books = r.n_live = r.n_terminal = r.n_out_of_data = r.n_rho = 0;
    for (int k = 0; k < 4; k++) {
        r.f[k].sum = 0.0; r.f[k].sumsq = 0.0; r.f[k].min = (double)INFINITY; r.f[k].max = -(double)INFINITY;
        r.f[k].argmin = -1; r.f[k].argmax = -1;
        r.i[k].sum = 0; r.i[k].sumsq = 0; r.i[k].min = INT64_MAX; r.i[k].max = INT64_MIN;
        r.i[k].argmin = -1; r.i[k].argmax = -1;
    }
}

// An extreme and the book that holds it: the lower id on a tie.  Ids compare as unsigned, so that the identity's -1 ("no
// book") loses to every book; a NaN never wins (both comparisons are false).  Associative and commutative: the extremes do
// not depend on the order in which books and partial records are put together.
template <class T> LOB_HD void stats_take_min(T& m, int64_t& am, T v, int64_t id) {
    if (v < m || (v == m && (uint64_t)id < (uint64_t)am)) { m = v; am = id; }
}
template <class T> LOB_HD void stats_take_max(T& m, int64_t& am, T v, int64_t id) {
    if (v > m || (v == m && (uint64_t)id < (uint64_t)am)) { m = v; am = id; }
}

// One book's value into a statistic (the integer sums wrap like any int64 arithmetic; a square is rounded once)
LOB_HD void stats_add(lob_stat_f64& s, double v, int64_t id) {
    s.sum = s.sum + v; s.sumsq = s.sumsq + v * v;
    stats_take_min(s.min, s.argmin, v, id); stats_take_max(s.max, s.argmax, v, id);
}
LOB_HD void stats_add(lob_stat_i64& s, int64_t v, int64_t id) {
    s.sum = (int64_t)((uint64_t)s.sum + (uint64_t)v); s.sumsq = (int64_t)((uint64_t)s.sumsq + (uint64_t)v * (uint64_t)v);
    stats_take_min(s.min, s.argmin, v, id); stats_take_max(s.max, s.argmax, v, id);
}

// into (+)= from.  The f64 sums are `into + from` in that order: the caller fixes the order of the records.
LOB_HD void stats_merge(lob_stat_f64& a, const lob_stat_f64& b) {
    a.sum = a.sum + b.sum; a.sumsq = a.sumsq + b.sumsq;
    stats_take_min(a.min, a.argmin, b.min, b.argmin); stats_take_max(a.max, a.argmax, b.max, b.argmax);
}
LOB_HD void stats_merge(lob_stat_i64& a, const lob_stat_i64& b) {
    a.sum = (int64_t)((uint64_t)a.sum + (uint64_t)b.sum); a.sumsq = (int64_t)((uint64_t)a.sumsq + (uint64_t)b.sumsq);
    stats_take_min(a.min, a.argmin, b.min, b.argmin); stats_take_max(a.max, a.argmax, b.max, b.argmax);
}
LOB_HD void stats_merge(lob_episode_record& a, const lob_episode_record& b) {
    if (a.group != b.group) a.group = -1;
    a.n_books += b.n_books; a.n_live += b.n_live; a.n_terminal += b.n_terminal; a.n_out_of_data += b.n_out_of_data; a.n_rho += b.n_rho;
    for (int k = 0; k < 4; k++) { stats_merge(a.f[k], b.f[k]); stats_merge(a.i[k], b.i[k]); }
}

#endif
