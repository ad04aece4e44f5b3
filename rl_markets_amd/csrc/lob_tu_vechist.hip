// Translation unit of the event-record window of the vector-env interface (include/lob_engine.h lob_vec_history; lob_launch.h
// VecHistSrc): vec_hist_kernel.  A unit of its own, so that the units of the step and of lob_reset are compiled from
// what they were.  gfx950 only; no CPU execution path.
//   Pure data movement: per book the n_valid x Wd words of the records that end with its current one in, K x (4 x D + 2 x T + 1)
// words out -- the records' own words, the volumes converted to f32.
#define LOB_TU_SPLIT 1
#define LOB_TU_VECHIST 1
#include <hip/hip_runtime.h>

#include "lob_launch.h"

#define LOB_VECHIST_LOADS 5                                           // 16-byte loads per lane, all in flight together
#define LOB_VECHIST_MAX_QUADS (1 + 4 * ((LOB_MAX_DEPTH + 3) / 4) + (2 * LOB_MAX_TRADES + 3) / 4)   // quads of the widest record
static_assert(LOB_VECHIST_ROWS * LOB_VECHIST_MAX_QUADS <= LOB_VECHIST_LOADS * LOB_VECHIST_BLOCK, "a block's quads in one batch of loads");
static_assert(LOB_VECHIST_ROWS <= 64 && LOB_VECHIST_ROWS % 4 == 0, "one wave owns the rows' source words; a block's first byte is 16-byte aligned in every tensor");

// A block's rows are contiguous in the caller's buffer: they leave LDS as consecutive words of consecutive lanes, 16 bytes per lane
// where the destination is 16-byte aligned (`v16`: the caller's pointer is; a block's first row is a multiple of LOB_VECHIST_ROWS),
// the up to three words behind the last whole quad and everything for an unaligned pointer a word per lane.
__device__ __forceinline__ void vec_hist_rows_out(const uint32_t* stage, uint32_t* dst, int n, int v16) {
    const int n4 = v16 ? n >> 2 : 0;
    const uint4* s4 = reinterpret_cast<const uint4*>(stage);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (int i = threadIdx.x; i < n4; i += LOB_VECHIST_BLOCK) d4[i] = s4[i];
    for (int i = (n4 << 2) + threadIdx.x; i < n; i += LOB_VECHIST_BLOCK) dst[i] = stage[i];
}

// One block = LOB_VECHIST_ROWS consecutive rows of the flat [B x K] row space (row = b * K + k): in every output tensor a row is a
// fixed number of words and consecutive rows are adjacent, whichever book they belong to, so K only sets how many blocks there are.
//   Row (b, k) is record r - (K - 1 - k) of book b's stream, r = rec_cur[b] (never past the stream's last record), or nothing
// where that index is negative.  The first wave works the rows' source records out, a lane per row, and leaves them in LDS.
//   Loads.  A row's record is Wd / 4 16-byte quads and the rows of one book are adjacent records, so lane i of the block takes quad
// i of the block's rows x quads: consecutive lanes read consecutive 16 bytes of one run per book.  At most LOB_VECHIST_LOADS quads
// per lane, issued together.  No load is under a branch: a lane past the block's quads, a row past the batch and a row without a
// record fetch a valid address (the last quad, the last row, the first record of the book's stream) and the result is masked to 0.
//   A quad's role is its index within the record (lob_env.h drec_*): 0 the header (word 0 the time), then quad j of level array a,
// then the trade quads -- two interleaved (price, volume) pairs each, parted into the two planes of the contract on their way
// into LDS.  Prices keep their bits; volumes: i32 -> f32 in registers (round to nearest even).
//   Stores: see vec_hist_rows_out; zero slots take the same way.  n_valid / rec: the lane of the row (b, K - 1) writes its book's
// two words.  Nothing is written but the caller's buffers.
__global__ __launch_bounds__(LOB_VECHIST_BLOCK) void vec_hist_kernel(VecHistSrc s, lob_vec_hist_out out, int K, int lv16, int tr16, int tm16) {
    __shared__ __attribute__((aligned(16))) uint32_t lv[LOB_VECHIST_ROWS * 4 * LOB_MAX_DEPTH];
    __shared__ __attribute__((aligned(16))) uint32_t tr[LOB_VECHIST_ROWS * 2 * LOB_MAX_TRADES];
    __shared__ __attribute__((aligned(16))) uint32_t tm[LOB_VECHIST_ROWS];
    __shared__ i64 src[LOB_VECHIST_ROWS];    // the row's record within `records` (a valid one also where the row has none)
    __shared__ i32 live[LOB_VECHIST_ROWS];   // 1: the row has a record
    const i64 n_rows = (i64)s.B * (i64)K;
    const i64 first = (i64)blockIdx.x * LOB_VECHIST_ROWS;
    const int rows = n_rows - first < LOB_VECHIST_ROWS ? (int)(n_rows - first) : LOB_VECHIST_ROWS;
    const int D = s.D, T = s.T;
    if (threadIdx.x < LOB_VECHIST_ROWS) {   // (threads of the first wave)
        const int rl = threadIdx.x;
        const i64 row = first + (rl < rows ? rl : rows - 1);
        const int b = (int)(row / K), k = (int)(row - (i64)b * K);
        const i32 cur = s.rec_cur[b];
        const i32 len = s.rec_len ? s.rec_len[b] : s.n_events;
        const i64 start = s.rec_phase ? s.rec_phase[b] : (i64)b * (i64)s.n_events;   // EnvCtx (lob_env.h)
        const i32 r = cur < 0 ? -1 : (cur < len ? cur : len - 1);
        const i32 ri = r - (K - 1 - k);
        src[rl] = start + (ri >= 0 ? ri : 0);
        live[rl] = ri >= 0 ? 1 : 0;
        if (rl < rows && k == K - 1) {
            if (out.n_valid) out.n_valid[b] = r + 1 < K ? r + 1 : K;
            if (out.rec) out.rec[b] = r;
        }
    }
    __syncthreads();
    if (out.levels || out.trades || out.time_ms) {   // (uniform)
        const int Q = s.Wd >> 2;   // quads per record
        const int q_lv = s.w_ask_px >> 2, q_av = s.w_ask_vol >> 2, q_bp = s.w_bid_px >> 2, q_bv = s.w_bid_vol >> 2, q_tr = s.w_trades >> 2;
        const int n = rows * Q;
        int rl[LOB_VECHIST_LOADS], q[LOB_VECHIST_LOADS];
        uint4 v[LOB_VECHIST_LOADS];
#pragma unroll
        for (int u = 0; u < LOB_VECHIST_LOADS; u++) {
            const int i = u * LOB_VECHIST_BLOCK + threadIdx.x;
            const int ic = i < n ? i : n - 1;
            rl[u] = ic / Q;
            q[u] = ic - rl[u] * Q;
            v[u] = *reinterpret_cast<const uint4*>(s.records + (size_t)src[rl[u]] * (size_t)s.Wd + 4 * q[u]);
        }
#pragma unroll
        for (int u = 0; u < LOB_VECHIST_LOADS; u++) {
            if (u * LOB_VECHIST_BLOCK + (int)threadIdx.x >= n) continue;   // (nothing but LDS writes behind this)
            const bool on = live[rl[u]] != 0;
            const uint32_t w[4] = {on ? v[u].x : 0u, on ? v[u].y : 0u, on ? v[u].z : 0u, on ? v[u].w : 0u};
            if (q[u] < q_lv) {
                if (q[u] == 0) tm[rl[u]] = w[0];
            } else if (q[u] < q_tr) {
                const int a = (q[u] >= q_av) + (q[u] >= q_bp) + (q[u] >= q_bv);   // ask_px, ask_vol, bid_px, bid_vol
                const int j = q[u] - (a == 0 ? q_lv : a == 1 ? q_av : a == 2 ? q_bp : q_bv);
                uint32_t* dst = lv + rl[u] * 4 * D + a * D + 4 * j;
#pragma unroll
                for (int x = 0; x < 4; x++)
                    if (4 * j + x < D) dst[x] = (a & 1) ? __float_as_uint((f32)(i32)w[x]) : w[x];
            } else {
                const int t = 2 * (q[u] - q_tr);   // the quad's first (price, volume) pair
                uint32_t* dst = tr + rl[u] * 2 * T;
                if (t < T) { dst[t] = w[0]; dst[T + t] = __float_as_uint((f32)(i32)w[1]); }
                if (t + 1 < T) { dst[t + 1] = w[2]; dst[T + t + 1] = __float_as_uint((f32)(i32)w[3]); }
            }
        }
    }
    __syncthreads();
    if (out.levels) vec_hist_rows_out(lv, reinterpret_cast<uint32_t*>(out.levels) + (size_t)first * 4 * (size_t)D, rows * 4 * D, lv16);
    if (out.trades) vec_hist_rows_out(tr, reinterpret_cast<uint32_t*>(out.trades) + (size_t)first * 2 * (size_t)T, rows * 2 * T, tr16);
    if (out.time_ms) vec_hist_rows_out(tm, reinterpret_cast<uint32_t*>(out.time_ms) + (size_t)first, rows, tm16);
}

void lobk_vec_history(hipStream_t st, const VecHistSrc& s, int K, const lob_vec_hist_out& out) {
    const int lv16 = ((uintptr_t)out.levels & 15) == 0 ? 1 : 0, tr16 = ((uintptr_t)out.trades & 15) == 0 ? 1 : 0, tm16 = ((uintptr_t)out.time_ms & 15) == 0 ? 1 : 0;
    const i64 n_rows = (i64)s.B * (i64)K;
    hipLaunchKernelGGL(vec_hist_kernel, dim3((unsigned)((n_rows + LOB_VECHIST_ROWS - 1) / LOB_VECHIST_ROWS)), dim3(LOB_VECHIST_BLOCK), 0, st, s, out, K, lv16, tr16, tm16);
}
