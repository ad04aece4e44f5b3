// Host side of the C ABI, what reads the engine (include/lob_engine.h; lob_engine_impl.h): the state, reward, terminal and book
// read-backs, lob_clear_inventory, the episode statistics, the model log and the step log, and the diagnostics that are host
// counters.  No kernel is compiled here: every launch goes through lob_launch.h.  gfx950 only; no CPU execution path.
#define LOB_TU_SPLIT 1
#include <algorithm>

#include "lob_engine_impl.h"

namespace lob {

void step_log_free(lob_engine* e) {
    if (e->slog_rows) hipFree(e->slog_rows);
    if (e->slog_cnt) hipFree(e->slog_cnt);
    if (e->slog_sel) hipFree(e->slog_sel);
    e->slog_rows = nullptr; e->slog_cnt = nullptr; e->slog_sel = nullptr;
    e->slog_n = e->slog_cap = 0;
    e->slog_armed = false;
}

}  // namespace lob

extern "C" {

int lob_get_state(lob_engine* e, float* host_out) {
    LOB_GUARD(e, lob_get_state);
    HIPCHK(hipSetDevice(e->device));
    DevTemp<f32> d;
    if (d.alloc((size_t)e->B * e->P.V)) { lob_set_error("lob_get_state: no room for the device buffer"); return LOB_ENOMEM; }
    lobk_get_state(e->stream, (const DevParams*)e->P_dev, e->S, d.p, (f64*)nullptr);
    hipError_t err = hipMemcpyAsync(host_out, d.p, (size_t)e->B * e->P.V * 4, hipMemcpyDeviceToHost, e->stream);
    hipStreamSynchronize(e->stream);
    HIPCHK(err);
    return LOB_OK;
}

int lob_get_reward(lob_engine* e, double* host_out) {
    LOB_GUARD(e, lob_get_reward);
    HIPCHK(hipSetDevice(e->device));
    DevTemp<f64> d;
    if (d.alloc((size_t)e->B)) { lob_set_error("lob_get_reward: no room for the device buffer"); return LOB_ENOMEM; }
    lobk_get_state(e->stream, (const DevParams*)e->P_dev, e->S, (f32*)nullptr, d.p);
    hipError_t err = hipMemcpyAsync(host_out, d.p, (size_t)e->B * 8, hipMemcpyDeviceToHost, e->stream);
    hipStreamSynchronize(e->stream);
    HIPCHK(err);
    return LOB_OK;
}

int lob_get_terminal(lob_engine* e, uint8_t* host_out) {
    LOB_GUARD(e, lob_get_terminal);
    HIPCHK(hipSetDevice(e->device));
    std::vector<i32> done(e->B), tm(e->B);
    HIPCHK(hipMemcpyAsync(done.data(), e->S.done, (size_t)e->B * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(tm.data(), e->S.time_ms, (size_t)e->B * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int b = 0; b < e->B; b++) {
        bool open = ((i64)tm[b] > e->P.open_ms + 30 * 60000LL) && ((i64)tm[b] < e->P.close_ms - 30 * 60000LL);
        host_out[b] = done[b] == 2 ? 2 : (open ? 0 : 1);
    }
    return LOB_OK;
}

int lob_clear_inventory(lob_engine* e) {
    LOB_GUARD(e, lob_clear_inventory);
    HIPCHK(hipSetDevice(e->device));
    lobk_clear_inventory(e->stream, (const DevParams*)e->P_dev, e->S);
    e->hits_ok = false;
    HIPCHK(hipGetLastError());
    return check_device_errors(e);
}

int lob_get_books(lob_engine* e, int32_t first, int32_t n, lob_book_dump* out) {
    if (!e || !out || first < 0 || n < 1 || first + n > e->B) { lob_set_error("lob_get_books: bad range"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    if (e->dump.reserve((size_t)n)) { lob_set_error("lob_get_books: no room for the books' device buffer (read fewer books per call)"); return LOB_ENOMEM; }
    lobk_dump(e->stream, (const DevParams*)e->P_dev, e->S, first, n, e->dump.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, e->dump.p, (size_t)n * sizeof(lob_book_dump), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}
int lob_get_book(lob_engine* e, int32_t book, lob_book_dump* out) { return lob_get_books(e, book, 1, out); }

// The batch's episode statistics, reduced on the device (lob_kernels.h episode_stats_partial_kernel): the kernels get the few field
// arrays they read as arguments; n_out records come back.  Reads only.
int lob_episode_stats(lob_engine* e, int32_t by_day, lob_episode_record* out, int32_t cap, int32_t* n_out) {
    if (!e || !out || !n_out) { lob_set_error("lob_episode_stats: NULL argument"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_episode_stats);
    if (by_day && (!e->lib || e->lib_cur < 0)) { lob_set_error("lob_episode_stats: by_day without an episode on a day library (lob_load_days, a selection, lob_reset)"); return LOB_ESTATE; }
    const int n = by_day ? 1 + e->lib_days : 1;
    *n_out = n;
    if (cap < n) { lob_set_error("lob_episode_stats: " + std::to_string(n) + " records, room for " + std::to_string(cap)); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    const size_t need = (size_t)n * (1 + (size_t)lobk_stats_chunks(e->B));
    if (e->stats.reserve(need)) { lob_set_error("lob_episode_stats: no room for the records' device buffer"); return LOB_ENOMEM; }
    StatsSrc s;
    s.ep_reward = e->S.ep_reward; s.ep_pnl = e->S.ep_pnl; s.ep_bandh = e->S.ep_bandh;
    s.total_ticks = e->S.total_ticks; s.market_buys = e->S.market_buys; s.market_sells = e->S.market_sells;
    s.done = e->S.done; s.time_ms = e->S.time_ms; s.ntr_snap = e->S.ntr_snap; s.tick_pos = e->S.tick_pos;
    s.day = by_day ? e->lib_day[e->lib_cur] : nullptr;
    s.open_ms = e->P.open_ms; s.close_ms = e->P.close_ms; s.book_id_offset = e->P.book_id_offset; s.B = e->B;
    lobk_episode_stats(e->stream, s, n, e->stats.p + n, e->stats.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, e->stats.p, (size_t)n * sizeof(lob_episode_record), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}

int lob_model_log_enable(lob_engine* e, int32_t on) {
    if (!e) return LOB_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    if (on && !e->S.ml_part) {
        int rc = dev_alloc(e, &e->S.ml_part, (size_t)LOB_ML_BLOCKS);
        if (rc == LOB_OK) rc = dev_alloc(e, &e->S.ml_npart, (size_t)LOB_ML_BLOCKS);
        if (rc == LOB_OK) rc = dev_alloc(e, &e->S.ml_agg, 1);
        if (rc == LOB_OK) rc = dev_alloc(e, &e->S.ml_cnt, 2);
        if (rc == LOB_OK) rc = dev_alloc(e, &e->S.ml_rows, (size_t)LOB_ML_ROWS);
        if (rc != LOB_OK) return rc;
    }
    e->model_log = on != 0;
    return LOB_OK;
}
int lob_model_log_read(lob_engine* e, double* rows, int32_t cap, int32_t* n_rows, int64_t* n_lost) {
    if (!e || !rows || cap < 0 || !n_rows) return LOB_EINVAL;
    *n_rows = 0;
    if (n_lost) *n_lost = 0;
    if (!e->S.ml_part) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    i64 cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(cnt, e->S.ml_cnt, sizeof cnt, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const i64 kept = std::min<i64>(cnt[1], LOB_ML_ROWS), n = std::min<i64>(kept, cap);
    if (n > 0) HIPCHK(hipMemcpyAsync(rows, e->S.ml_rows, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
    // the rows are handed over once: the counter starts again (the running aggregate stays)
    HIPCHK(hipMemsetAsync(e->S.ml_cnt + 1, 0, sizeof(i64), e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    *n_rows = (int32_t)n;
    if (n_lost) *n_lost = cnt[1] - n;   // rows beyond the ring (LOB_ML_ROWS between two reads) or beyond `cap`
    return LOB_OK;
}

// The step log (include/lob_engine.h): the log's memory belongs to the engine, not to DevState -- the step kernels never see it.
int lob_step_log_enable(lob_engine* e, const int32_t* host_books, int32_t n_sel, int32_t cap_steps) {
    if (!e) { lob_set_error("lob_step_log_enable: NULL engine"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_step_log_enable);
    HIPCHK(hipSetDevice(e->device));
    if (n_sel == 0) {
        HIPCHK(hipStreamSynchronize(e->stream));   // (steps still in flight write the log)
        step_log_free(e);
        return LOB_OK;
    }
    if (n_sel < 0 || n_sel > e->B || cap_steps < 1) { lob_set_error("lob_step_log_enable: n_sel outside [0, n_books] or cap_steps < 1"); return LOB_EINVAL; }
    if (!host_books && n_sel != e->B) { lob_set_error("lob_step_log_enable: host_books == NULL selects every book: n_sel must be n_books"); return LOB_EINVAL; }
    if (host_books)
        for (int j = 0; j < n_sel; j++)
            if (host_books[j] < 0 || host_books[j] >= e->B || (j > 0 && host_books[j] <= host_books[j - 1])) {
                lob_set_error("lob_step_log_enable: the books must be strictly ascending and within [0, n_books)");
                return LOB_EINVAL;
            }
    HIPCHK(hipStreamSynchronize(e->stream));
    step_log_free(e);
    hipError_t err = hipMalloc((void**)&e->slog_rows, (size_t)n_sel * (size_t)cap_steps * sizeof(lob_step_row));
    if (err == hipSuccess) err = hipMalloc((void**)&e->slog_cnt, 2 * (size_t)n_sel * sizeof(i32));
    if (err == hipSuccess && host_books) err = hipMalloc((void**)&e->slog_sel, (size_t)n_sel * sizeof(i32));
    if (err != hipSuccess) {
        (void)hipGetLastError();
        step_log_free(e);
        lob_set_error(std::string("lob_step_log_enable: hipMalloc failed: ") + hipGetErrorString(err));
        return LOB_ENOMEM;
    }
    e->slog_n = n_sel; e->slog_cap = cap_steps;
    HIPCHK(hipMemsetAsync(e->slog_cnt, 0, 2 * (size_t)n_sel * sizeof(i32), e->stream));
    if (host_books) HIPCHK(hipMemcpyAsync(e->slog_sel, host_books, (size_t)n_sel * sizeof(i32), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));   // (host_books is the caller's again)
    return LOB_OK;
}
static int step_log_on(lob_engine* e, const char* who) {
    if (!e) { lob_set_error(std::string(who) + ": NULL engine"); return LOB_EINVAL; }
    if (!e->slog_n) { lob_set_error(std::string(who) + ": the step log is off (lob_step_log_enable)"); return LOB_ESTATE; }
    return LOB_OK;
}
int lob_step_log_counts(lob_engine* e, int32_t* n_rows, int32_t* n_lost) {
    int rc = step_log_on(e, "lob_step_log_counts");
    if (rc) return rc;
    LOB_GUARD(e, lob_step_log_counts);
    if (!n_rows) { lob_set_error("lob_step_log_counts: n_rows == NULL"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(n_rows, e->slog_cnt, (size_t)e->slog_n * sizeof(i32), hipMemcpyDeviceToHost, e->stream));
    if (n_lost) HIPCHK(hipMemcpyAsync(n_lost, e->slog_cnt + e->slog_n, (size_t)e->slog_n * sizeof(i32), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}
int lob_step_log_read(lob_engine* e, int32_t first_sel, int32_t n_sel, int32_t first_row, int32_t n_rows, lob_step_row* host_out) {
    int rc = step_log_on(e, "lob_step_log_read");
    if (rc) return rc;
    LOB_GUARD(e, lob_step_log_read);
    if (!host_out || first_sel < 0 || n_sel < 1 || n_sel > e->slog_n - first_sel || first_row < 0 || n_rows < 1 || n_rows > e->slog_cap - first_row) {
        lob_set_error("lob_step_log_read: NULL, or a range outside the selection or cap_steps");
        return LOB_EINVAL;
    }
    HIPCHK(hipSetDevice(e->device));
    const size_t need = (size_t)n_sel * (size_t)n_rows;
    if (e->slog_stage.reserve(need)) {
        lob_set_error("lob_step_log_read: no room for the staging buffer (read fewer books or rows per call)");
        return LOB_ENOMEM;
    }
    lobk_step_log_gather(e->stream, e->slog_rows, e->slog_cnt, e->slog_n, first_sel, n_sel, first_row, n_rows, e->slog_stage.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host_out, e->slog_stage.p, need * sizeof(lob_step_row), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}

}  // extern "C"

// Diagnostics (not part of include/lob_engine.h): learner steps (combined update) since lob_create by the shape of their update
// -- [0] updates added to their slots by the learn / trace kernels, accumulate_kernel over the list they left (Q(lambda)),
// [1] steps whose learn_q_rest_kernel ran beside the trace kernels on the second stream, [2] accumulate_block_kernel,
// [3] accumulate_kernel over every book; steps with the action selection inside the env kernel (launch_env_fused): [4] books without a
// usable hit list served in-kernel (act_book), [5] through the work list to the wave-per-book act kernel because the learn
// kernels' hand-back count said most books have none (a dense theta), [6] through the work list for another reason (the first
// step on lists, LOB_INLINE_GENERAL=0); [7] of the steps counted under [2], those whose sums went through the dense ids
// (accumulate_dense_kernel).  The tests use it to know which path they have compared with the oracle.
extern "C" int lob_debug_flow(lob_engine* e, int64_t out[8]) {
    if (!e || !out) return LOB_EINVAL;
    for (int i = 0; i < 8; i++) out[i] = e->flow[i];
    return LOB_OK;
}

// Diagnostics (not part of include/lob_engine.h): launches since lob_create of kernels that share a timer name ("env_kernel",
// "learn_kernel") -- [0] env_step_kernel, [1] env_step16_kernel (which of the two: lobk_env_step says), [2] the fused
// env_kernel<., ., 1>, [3] learn_q_pair_kernel, [4] learn_q_lane_kernel, [5] learn_q_fast_kernel.  Host counters; the tests use
// them to show which kernel a case has compared with the oracle.
extern "C" int lob_debug_launches(lob_engine* e, int64_t out[6]) {
    if (!e || !out) return LOB_EINVAL;
    for (int i = 0; i < 6; i++) out[i] = e->launched[i];
    return LOB_OK;
}

// Diagnostics (not part of include/lob_engine.h): learner steps since lob_create that [0] read the learn kernels' hand-back count
// (the hint of LOB_HINT_LAG steps ago), [1] of those, steps whose hint word had not arrived within the spin limit and that went by
// a count of 0 instead -- the path such a step took was chosen by the host's timing, not by the run.
extern "C" int lob_debug_hint(lob_engine* e, int64_t out[2]) {
    if (!e || !out) return LOB_EINVAL;
    out[0] = e->hint_reads;
    out[1] = e->hint_misses;
    return LOB_OK;
}

// Diagnostics (not part of include/lob_engine.h): sparse exchanges without / with a host synchronisation, exchanges whose union outgrew
// the fixed count (their surplus travelled one exchange later), the fixed count, the last union size known to the host.
extern "C" int lob_debug_exchange(lob_engine* e, int64_t out[5]) {
    if (!e || !out) return LOB_EINVAL;
    out[0] = e->spx_nosync; out[1] = e->spx_synced; out[2] = e->spx_overflows; out[3] = e->spx_fixed; out[4] = e->spx_last_total;
    return LOB_OK;
}
