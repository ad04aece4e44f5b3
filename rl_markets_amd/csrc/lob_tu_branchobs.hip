// Translation unit of the order-book observation and the event-record window of the branch sets (include/lob_engine.h
// lob_branch_book / lob_branch_history; lob_launch.h BranchObsSrc; lob_branch.h the layout): branch_book_kernel,
// branch_hist_kernel.  A unit of its own, so that every other unit is compiled from what it was.  gfx950 only; no CPU execution path.
//   Pure data movement, as vec_book_kernel (lob_tu_vecbook.hip) and vec_hist_kernel (lob_tu_vechist.hip), whose structure is restated
// here: what differs is where the field words come from -- the live buffer of the set at lane n * Bpad + b instead of the engine's
// field arrays at b -- and where a row goes: n * B + b of branch-major tensors.  The records, rec_phase and rec_len are the engine's and
// belong to the BOOK b, whichever branch reads them.  Nothing is written but the caller's buffers.
#define LOB_TU_SPLIT 1
#define LOB_TU_BRANCHOBS 1
#include <hip/hip_runtime.h>

#include "lob_launch.h"

static constexpr BranchOff BR_OFF = branch_off();

// array of the set whose elements lie `per_lane` bytes per lane behind the base (lob_tu_branch.hip br_arr, read-only here)
template <class T> __device__ __forceinline__ const T* br_arr(const BranchSet& s, uint32_t per_lane) { return (const T*)(s.base + s.lanes * (u64)per_lane); }

#define LOB_BRBOOK_BLOCK LOB_VECBOOK_BLOCK
#define LOB_BRBOOK_BOOKS LOB_VECBOOK_BOOKS                          // books per block: a block never crosses a branch's plane
#define LOB_BRBOOK_LANES 8                                          // lanes per book in the level pass
#define LOB_BRBOOK_PASS (LOB_BRBOOK_BLOCK / LOB_BRBOOK_LANES)       // books per pass
#define LOB_BRBOOK_PASSES (LOB_BRBOOK_BOOKS / LOB_BRBOOK_PASS)
static_assert(LOB_BRBOOK_BOOKS == 64, "a block is one wave of the set's lanes: Bpad is a multiple of the books per block");
static_assert(LOB_BRBOOK_BOOKS % LOB_BRBOOK_PASS == 0, "whole passes");
static_assert(2 * ((LOB_MAX_DEPTH + 3) / 4) <= LOB_BRBOOK_LANES, "a lane per 16-byte quad of a side's prices");
static_assert(LOB_VEC_OWN_WORDS == 16, "four 16-byte stores per book");

#define LOB_BRHIST_BLOCK LOB_VECHIST_BLOCK
#define LOB_BRHIST_ROWS LOB_VECHIST_ROWS
#define LOB_BRHIST_LOADS 5                                          // 16-byte loads per lane, all in flight together
#define LOB_BRHIST_MAX_QUADS (1 + 4 * ((LOB_MAX_DEPTH + 3) / 4) + (2 * LOB_MAX_TRADES + 3) / 4)   // quads of the widest record
static_assert(LOB_BRHIST_ROWS * LOB_BRHIST_MAX_QUADS <= LOB_BRHIST_LOADS * LOB_BRHIST_BLOCK, "a block's quads in one batch of loads");
static_assert(LOB_BRHIST_ROWS <= 64 && LOB_BRHIST_ROWS % 4 == 0, "one wave owns the rows' source words; a block's first byte is 16-byte aligned in every tensor");

// A block's rows are contiguous in the caller's buffer: they leave LDS as consecutive words of consecutive lanes, 16 bytes per lane
// where the destination is 16-byte aligned (`v16`: the caller's pointer is; a block's first byte is a multiple of 16 bytes behind it
// in every tensor, whichever plane the block lies in), the up to three words behind the last whole quad and everything for an
// unaligned pointer a word per lane.
template <int BLOCK>
__device__ __forceinline__ void br_rows_out(const uint32_t* stage, uint32_t* dst, int n, int v16) {
    const int n4 = v16 ? n >> 2 : 0;
    const uint4* s4 = reinterpret_cast<const uint4*>(stage);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (int i = threadIdx.x; i < n4; i += BLOCK) d4[i] = s4[i];
    for (int i = (n4 << 2) + threadIdx.x; i < n; i += BLOCK) dst[i] = stage[i];
}

// One block = LOB_BRBOOK_BOOKS consecutive books of ONE branch: block i is branch i / (Bpad / 64) over the books 64 * (i % (Bpad / 64))
// ..., the grid of branch_step_kernel.  `rows` is what the branch's plane has left, so the last block of a plane stops at the
// plane's end: the next plane's rows are another block's.
//   Levels: vec_book_kernel's pass.  Eight lanes share a book: lane (side, j) fetches quad j of the side's prices and quad j of its
// volumes from the branch's current record, two 16-byte loads, issued for both passes before the first is waited for.  No load is
// under a branch: a lane without a quad, a lane past the plane's books -- it takes the block's last real book, so no address is ever
// formed from a pad lane of the set, whose words nobody wrote -- and a branch without a snapshot (rec_cur < 0: record 0 is read)
// fetch a valid address and the result is masked.  The record is rec_cur of the BRANCH in the stream of the BOOK.
//   Own words and time.  Lane per book of the first wave: coalesced loads of the set's arrays (consecutive books of one branch are
// consecutive lanes of the set), the values as dump_kernel derives them, four 16-byte writes into the staging row.
__global__ __launch_bounds__(LOB_BRBOOK_BLOCK) void branch_book_kernel(BranchObsSrc s, lob_vec_book_out out, int lv16, int own16) {
    __shared__ __attribute__((aligned(16))) f32 lv[LOB_BRBOOK_BOOKS * 4 * LOB_MAX_DEPTH];
    __shared__ __attribute__((aligned(16))) f32 ow[LOB_BRBOOK_BOOKS * LOB_VEC_OWN_WORDS];
    const int bpp = s.Bpad / LOB_BRBOOK_BOOKS;   // blocks per plane
    const int n = blockIdx.x / bpp;
    const int first = (blockIdx.x - n * bpp) * LOB_BRBOOK_BOOKS;
    const int rows = s.B - first < LOB_BRBOOK_BOOKS ? s.B - first : LOB_BRBOOK_BOOKS;   // (>= 1: first < B)
    const size_t lane0 = (size_t)n * (size_t)s.Bpad + (size_t)first;   // the set's lane of the block's first book
    const size_t row0 = (size_t)n * (size_t)s.B + (size_t)first;       // ... and its row in the caller's tensors
    const int D = s.D;
    if (out.levels) {   // (uniform)
        const i32* rec_cur = br_arr<i32>(s.set, BR_OFF.rec_cur);
        const int qpa = (D + 3) >> 2;   // 16-byte quads per level array
        const int sub = threadIdx.x & (LOB_BRBOOK_LANES - 1);
        const bool lane_on = sub < 2 * qpa;
        const int side = lane_on && sub >= qpa ? 1 : 0;
        const int j = lane_on ? sub - side * qpa : 0;
        const int w_px = (side ? s.w_bid_px : s.w_ask_px) + 4 * j, w_vol = (side ? s.w_bid_vol : s.w_ask_vol) + 4 * j;
        i32 rec[LOB_BRBOOK_PASSES];
        uint4 px[LOB_BRBOOK_PASSES], vol[LOB_BRBOOK_PASSES];
#pragma unroll
        for (int p = 0; p < LOB_BRBOOK_PASSES; p++) {
            const int bl = p * LOB_BRBOOK_PASS + (threadIdx.x >> 3);
            rec[p] = rec_cur[lane0 + (size_t)(bl < rows ? bl : rows - 1)];
        }
#pragma unroll
        for (int p = 0; p < LOB_BRBOOK_PASSES; p++) {
            const int bl = p * LOB_BRBOOK_PASS + (threadIdx.x >> 3);
            const int b = first + (bl < rows ? bl : rows - 1);
            const size_t start = s.rec_phase ? (size_t)s.rec_phase[b] : (size_t)b * (size_t)s.n_events;   // EnvCtx (lob_env.h)
            const uint32_t* r = s.records + (start + (size_t)(rec[p] < 0 ? 0 : rec[p])) * (size_t)s.Wd;
            px[p] = *reinterpret_cast<const uint4*>(r + w_px);
            vol[p] = *reinterpret_cast<const uint4*>(r + w_vol);
        }
#pragma unroll
        for (int p = 0; p < LOB_BRBOOK_PASSES; p++) {
            const int bl = p * LOB_BRBOOK_PASS + (threadIdx.x >> 3);
            const bool have = rec[p] >= 0;   // rec_price / book_volume: no snapshot reads as 0
            const uint32_t pw[4] = {px[p].x, px[p].y, px[p].z, px[p].w}, vw[4] = {vol[p].x, vol[p].y, vol[p].z, vol[p].w};
            f32* dst = lv + bl * 4 * D + side * 2 * D + 4 * j;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                if (lane_on && 4 * j + w < D) {
                    const f32 price = have ? __uint_as_float(pw[w]) : 0.0f;
                    dst[w] = price;
                    dst[D + w] = (price > 0.0f || price < 0.0f) ? (f32)(i32)vw[w] : 0.0f;
                }
            }
        }
    }
    if ((out.own || out.time_ms) && (int)threadIdx.x < rows) {   // (threads of the first wave)
        const size_t l = lane0 + threadIdx.x;
        if (out.time_ms) out.time_ms[row0 + threadIdx.x] = (i64)br_arr<i32>(s.set, BR_OFF.time_ms)[l];
        if (out.own) {
            const i32 a_on = br_arr<i32>(s.set, BR_OFF.a_on)[l], b_on = br_arr<i32>(s.set, BR_OFF.b_on)[l];
            const f64 a_opx = br_arr<f64>(s.set, BR_OFF.a_opx)[l], b_opx = br_arr<f64>(s.set, BR_OFF.b_opx)[l];
            const i64 a_rem = br_arr<i64>(s.set, BR_OFF.a_osz)[l] - br_arr<i64>(s.set, BR_OFF.a_oex)[l];
            const i64 b_rem = br_arr<i64>(s.set, BR_OFF.b_osz)[l] - br_arr<i64>(s.set, BR_OFF.b_oex)[l];
            const i64 a_oqh = br_arr<i64>(s.set, BR_OFF.a_oqh)[l], b_oqh = br_arr<i64>(s.set, BR_OFF.b_oqh)[l];
            float4 q0, q1, q2, q3;   // LOB_OWN_* order
            q0.x = (f32)br_arr<i64>(s.set, BR_OFF.position)[l];
            q0.y = (f32)a_on;
            q0.z = a_on ? (f32)a_opx : 0.0f;
            q0.w = a_on ? (f32)(a_rem > 0 ? a_rem : 0) : 0.0f;
            q1.x = a_on ? (f32)a_oqh : 0.0f;
            q1.y = (f32)b_on;
            q1.z = b_on ? (f32)b_opx : 0.0f;
            q1.w = b_on ? (f32)(b_rem > 0 ? b_rem : 0) : 0.0f;
            q2.x = b_on ? (f32)b_oqh : 0.0f;
            q2.y = (f32)br_arr<f64>(s.set, BR_OFF.ask_quote)[l];
            q2.z = (f32)br_arr<f64>(s.set, BR_OFF.bid_quote)[l];
            q2.w = (f32)br_arr<i32>(s.set, BR_OFF.last_action)[l];
            q3.x = (f32)br_arr<f64>(s.set, BR_OFF.pnl_step)[l];
            q3.y = (f32)br_arr<f64>(s.set, BR_OFF.ep_pnl)[l];
            q3.z = (f32)br_arr<f64>(s.set, BR_OFF.ep_reward)[l];
            q3.w = (f32)br_arr<i32>(s.set, BR_OFF.total_ticks)[l];
            float4* o = reinterpret_cast<float4*>(ow + threadIdx.x * LOB_VEC_OWN_WORDS);
            o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3;
        }
    }
    __syncthreads();
    if (out.levels)
        br_rows_out<LOB_BRBOOK_BLOCK>(reinterpret_cast<const uint32_t*>(lv), reinterpret_cast<uint32_t*>(out.levels) + row0 * 4 * (size_t)D, rows * 4 * D, lv16);
    if (out.own)
        br_rows_out<LOB_BRBOOK_BLOCK>(reinterpret_cast<const uint32_t*>(ow), reinterpret_cast<uint32_t*>(out.own) + row0 * LOB_VEC_OWN_WORDS, rows * LOB_VEC_OWN_WORDS, own16);
}

// One block = LOB_BRHIST_ROWS consecutive rows of the flat [N x B x K] row space (row = (n * B + b) * K + k): in every output tensor
// a row is a fixed number of words and consecutive rows are adjacent, whichever branch and book they belong to, so N and K only set
// how many blocks there are.  Row and byte offsets are 64-bit throughout: N * B * K rows of 4 * D words pass 2^31 bytes at the
// workload's sizes.
//   Row (n, b, k) is record r - (K - 1 - k) of book b's stream, r = rec_cur of BRANCH (n, b) (never past the last record of that
// book's stream), or nothing where that index is negative.  The first wave works the rows' source records out, a lane per row, and
// leaves them in LDS; a row past the space takes the last real row, so (n, b) is always a real branch and book.
//   Loads, the quads' roles and the stores: vec_hist_kernel's.  n_valid / rec: the lane of the row (n, b, K - 1) writes the two words
// of [n][b].
__global__ __launch_bounds__(LOB_BRHIST_BLOCK) void branch_hist_kernel(BranchObsSrc s, lob_vec_hist_out out, int K, int lv16, int tr16, int tm16) {
    __shared__ __attribute__((aligned(16))) uint32_t lv[LOB_BRHIST_ROWS * 4 * LOB_MAX_DEPTH];
    __shared__ __attribute__((aligned(16))) uint32_t tr[LOB_BRHIST_ROWS * 2 * LOB_MAX_TRADES];
    __shared__ __attribute__((aligned(16))) uint32_t tm[LOB_BRHIST_ROWS];
    __shared__ i64 src[LOB_BRHIST_ROWS];    // the row's record within `records` (a valid one also where the row has none)
    __shared__ i32 live[LOB_BRHIST_ROWS];   // 1: the row has a record
    const i64 n_rows = (i64)s.n_branches * (i64)s.B * (i64)K;
    const i64 first = (i64)blockIdx.x * LOB_BRHIST_ROWS;
    const int rows = n_rows - first < LOB_BRHIST_ROWS ? (int)(n_rows - first) : LOB_BRHIST_ROWS;
    const int D = s.D, T = s.T;
    if (threadIdx.x < LOB_BRHIST_ROWS) {   // (threads of the first wave)
        const int rl = threadIdx.x;
        const i64 row = first + (rl < rows ? rl : rows - 1);
        const i64 nb = row / K;                    // n * B + b: the row of the [N][B] tensors
        const int k = (int)(row - nb * K);
        const int n = (int)(nb / s.B), b = (int)(nb - (i64)n * s.B);
        const i32 cur = br_arr<i32>(s.set, BR_OFF.rec_cur)[(size_t)n * (size_t)s.Bpad + (size_t)b];
        const i32 len = s.rec_len ? s.rec_len[b] : s.n_events;
        const i64 start = s.rec_phase ? s.rec_phase[b] : (i64)b * (i64)s.n_events;   // EnvCtx (lob_env.h)
        const i32 r = cur < 0 ? -1 : (cur < len ? cur : len - 1);
        const i32 ri = r - (K - 1 - k);
        src[rl] = start + (ri >= 0 ? ri : 0);
        live[rl] = ri >= 0 ? 1 : 0;
        if (rl < rows && k == K - 1) {
            if (out.n_valid) out.n_valid[nb] = r + 1 < K ? r + 1 : K;
            if (out.rec) out.rec[nb] = r;
        }
    }
    __syncthreads();
    if (out.levels || out.trades || out.time_ms) {   // (uniform)
        const int Q = s.Wd >> 2;   // quads per record
        const int q_lv = s.w_ask_px >> 2, q_av = s.w_ask_vol >> 2, q_bp = s.w_bid_px >> 2, q_bv = s.w_bid_vol >> 2, q_tr = s.w_trades >> 2;
        const int n = rows * Q;
        int rl[LOB_BRHIST_LOADS], q[LOB_BRHIST_LOADS];
        uint4 v[LOB_BRHIST_LOADS];
#pragma unroll
        for (int u = 0; u < LOB_BRHIST_LOADS; u++) {
            const int i = u * LOB_BRHIST_BLOCK + threadIdx.x;
            const int ic = i < n ? i : n - 1;
            rl[u] = ic / Q;
            q[u] = ic - rl[u] * Q;
            v[u] = *reinterpret_cast<const uint4*>(s.records + (size_t)src[rl[u]] * (size_t)s.Wd + 4 * q[u]);
        }
#pragma unroll
        for (int u = 0; u < LOB_BRHIST_LOADS; u++) {
            if (u * LOB_BRHIST_BLOCK + (int)threadIdx.x >= n) continue;   // (nothing but LDS writes behind this)
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
    if (out.levels) br_rows_out<LOB_BRHIST_BLOCK>(lv, reinterpret_cast<uint32_t*>(out.levels) + (size_t)first * 4 * (size_t)D, rows * 4 * D, lv16);
    if (out.trades) br_rows_out<LOB_BRHIST_BLOCK>(tr, reinterpret_cast<uint32_t*>(out.trades) + (size_t)first * 2 * (size_t)T, rows * 2 * T, tr16);
    if (out.time_ms) br_rows_out<LOB_BRHIST_BLOCK>(tm, reinterpret_cast<uint32_t*>(out.time_ms) + (size_t)first, rows, tm16);
}

void lobk_branch_book(hipStream_t st, const BranchObsSrc& s, const lob_vec_book_out& out) {
    const int lv16 = ((uintptr_t)out.levels & 15) == 0 ? 1 : 0, own16 = ((uintptr_t)out.own & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(branch_book_kernel, dim3((unsigned)(s.n_branches * (s.Bpad / LOB_BRBOOK_BOOKS))), dim3(LOB_BRBOOK_BLOCK), 0, st, s, out, lv16, own16);
}

void lobk_branch_history(hipStream_t st, const BranchObsSrc& s, int K, const lob_vec_hist_out& out) {
    const int lv16 = ((uintptr_t)out.levels & 15) == 0 ? 1 : 0, tr16 = ((uintptr_t)out.trades & 15) == 0 ? 1 : 0, tm16 = ((uintptr_t)out.time_ms & 15) == 0 ? 1 : 0;
    const i64 n_rows = (i64)s.n_branches * (i64)s.B * (i64)K;
    hipLaunchKernelGGL(branch_hist_kernel, dim3((unsigned)((n_rows + LOB_BRHIST_ROWS - 1) / LOB_BRHIST_ROWS)), dim3(LOB_BRHIST_BLOCK), 0, st, s, out, K, lv16, tr16, tm16);
}
