// Translation unit of the step log (include/lob_engine.h lob_step_log_*; lob_launch.h StepLogSrc): step_log_kernel /
// step_log_gather_kernel.  A unit of its own, so that the units of the step and of lob_reset are compiled from what they were.
// gfx950 only; no CPU execution path.
//   The log is step-major, rows[k * n_sel + j]: logging all 65 536 books of the headline batch writes 65 536 x 96 B = 6.3 MB per
// step, and a 1 400-step episode of all of them takes 8.8 GB of HBM -- the caller chooses the selection and cap_steps.
#define LOB_TU_SPLIT 1
#define LOB_TU_STEPLOG 1
#include <hip/hip_runtime.h>

#include "lob_internal.h"
#include "lob_kernels.h"

static_assert(sizeof(lob_step_row) == 96 && sizeof(lob_step_row) % 16 == 0, "lob_step_row: six 16-byte stores");
#define LOB_STEPLOG_BLOCK 256

// One lane per selected book, behind the step's last kernel.  The lane's book has a row when its total_ticks has advanced past the
// rows it has been given so far (stored + lost) and it is not out of data: a completed performAction counts one tick and gets one
// row, so the two stay equal; the step that runs out of data counts its tick too (base.cpp:278) but returns before LogProfit
// (base.cpp:289-290) -- done == 2 from then on, and the book never steps again.  No help from the step kernels is needed, so the
// rule is the same behind lob_td_step, lob_eval_step, the second half of a split step and lob_step.
//   The fields are gathered as dump_kernel derives them (lob_kernels.h), from the field arrays alone: a dozen coalesced loads and
// the two touch prices out of the book's current record.  The row leaves in six 16-byte stores; lanes that share k (all of them,
// until the first books finish) fill 64 x 96 B without a gap.  No atomics: a lane owns its book's counters.
__global__ __launch_bounds__(LOB_STEPLOG_BLOCK) void step_log_kernel(StepLogSrc s) {
    const int j = blockIdx.x * LOB_STEPLOG_BLOCK + threadIdx.x;
    if (j >= s.n_sel) return;
    const int b = s.sel ? s.sel[j] : j;
    const i32 stored = s.n_rows[j], lost = s.n_lost[j];
    const i32 ticks = s.total_ticks[b], done = s.done[b];
    if (ticks <= stored + lost || done == 2) return;
    if (stored >= s.cap) { s.n_lost[j] = lost + 1; return; }
    const i32 rec = s.rec_cur[b];
    f64 ap0 = 0.0, bp0 = 0.0;   // rec_price (lob_env.h): no snapshot reads as 0
    if (rec >= 0) {
        const size_t first = s.rec_phase ? (size_t)s.rec_phase[b] : (size_t)b * (size_t)s.n_events;
        const uint32_t* r = s.records + (first + (size_t)rec) * (size_t)s.Wd;
        ap0 = (f64)__uint_as_float(r[s.w_ask0]);
        bp0 = (f64)__uint_as_float(r[s.w_bid0]);
    }
    lob_step_row row;
    row.time_ms = (i64)s.time_ms[b];
    row.position = s.position[b];
    row.midprice = (ap0 + bp0) / 2.0;
    row.spread = ap0 - bp0;
    row.ask_quote = s.ask_quote[b]; row.bid_quote = s.bid_quote[b];
    row.pnl_step = s.pnl_step[b];
    row.episode_pnl = s.ep_pnl[b]; row.episode_bandh = s.ep_bandh[b]; row.episode_reward = s.ep_reward[b];
    row.step = ticks;
    row.action = s.last_action[b];
    row.ask_level = s.ask_level[b]; row.bid_level = s.bid_level[b];
    uint4* dst = reinterpret_cast<uint4*>(s.rows + ((size_t)stored * (size_t)s.n_sel + (size_t)j));
    const uint4* src = reinterpret_cast<const uint4*>(&row);
#pragma unroll
    for (int q = 0; q < 6; q++) dst[q] = src[q];
    s.n_rows[j] = stored + 1;
}

// lob_step_log_read: the step-major log into a book-major staging buffer, one thread per 16 bytes of it (the stores coalesce, a
// row is read by six neighbouring lanes); slots beyond a book's stored count become zero.
__global__ __launch_bounds__(LOB_STEPLOG_BLOCK) void step_log_gather_kernel(const lob_step_row* __restrict__ rows, const i32* __restrict__ n_stored,
                                                                           int n_sel_all, int first_sel, int first_row, int n_rows, size_t total16,
                                                                           lob_step_row* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * LOB_STEPLOG_BLOCK + threadIdx.x;
    if (i >= total16) return;
    const size_t slot = i / 6;
    const int q = (int)(i - slot * 6);
    const int jj = (int)(slot / (size_t)n_rows), kk = (int)(slot - (size_t)jj * (size_t)n_rows);
    const int j = first_sel + jj, k = first_row + kk;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (k < n_stored[j]) v = reinterpret_cast<const uint4*>(rows + ((size_t)k * (size_t)n_sel_all + (size_t)j))[q];
    reinterpret_cast<uint4*>(out)[i] = v;
}

void lobk_step_log(hipStream_t st, const StepLogSrc& s) {
    hipLaunchKernelGGL(step_log_kernel, dim3((s.n_sel + LOB_STEPLOG_BLOCK - 1) / LOB_STEPLOG_BLOCK), dim3(LOB_STEPLOG_BLOCK), 0, st, s);
}

void lobk_step_log_gather(hipStream_t st, const lob_step_row* rows, const i32* n_stored, int n_sel_all, int first_sel, int n_sel, int first_row,
                          int n_rows, lob_step_row* out) {
    const size_t total16 = (size_t)n_sel * (size_t)n_rows * 6;
    hipLaunchKernelGGL(step_log_gather_kernel, dim3((unsigned)((total16 + LOB_STEPLOG_BLOCK - 1) / LOB_STEPLOG_BLOCK)), dim3(LOB_STEPLOG_BLOCK), 0, st,
                       rows, n_stored, n_sel_all, first_sel, first_row, n_rows, total16, out);
}
