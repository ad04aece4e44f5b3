// Translation unit of the order-book observation of the vector-env interface (include/lob_engine.h lob_vec_book; lob_launch.h
// VecBookSrc): vec_book_kernel.  A unit of its own, so that the units of the step and of lob_reset are compiled from
// what they were.  gfx950 only; no CPU execution path.
//   Pure data movement: per book 4 x D words of its current record and 18 words of the environment field arrays in, 4 x D + 16
// f32 and one i64 out -- every value the one dump_kernel (lob_kernels.h) derives for lob_get_books, converted to f32.
#define LOB_TU_SPLIT 1
#define LOB_TU_VECBOOK 1
#include <hip/hip_runtime.h>

#include "lob_launch.h"

#define LOB_VECBOOK_LANES 8                                           // lanes per book in the level pass
#define LOB_VECBOOK_PASS (LOB_VECBOOK_BLOCK / LOB_VECBOOK_LANES)      // books per pass
#define LOB_VECBOOK_PASSES (LOB_VECBOOK_BOOKS / LOB_VECBOOK_PASS)
static_assert(LOB_VECBOOK_BOOKS % LOB_VECBOOK_PASS == 0 && LOB_VECBOOK_BOOKS <= 64, "whole passes; one wave owns the books' field words");
static_assert(2 * ((LOB_MAX_DEPTH + 3) / 4) <= LOB_VECBOOK_LANES, "a lane per 16-byte quad of a side's prices");
static_assert(LOB_VEC_OWN_WORDS == 16, "four 16-byte stores per book");

// A block's rows are contiguous in the caller's buffer: they leave LDS as consecutive words of consecutive lanes, 16 bytes per lane
// where the destination is 16-byte aligned (`v16`; a block's first byte is a multiple of 16 bytes behind the buffer's, and `n` is a
// multiple of four words, for every depth), a word per lane where the caller's pointer is not.
__device__ __forceinline__ void vec_book_rows_out(const f32* stage, f32* dst, int n, int v16) {
    if (v16) {
        const float4* s4 = reinterpret_cast<const float4*>(stage);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int i = threadIdx.x; i < (n >> 2); i += LOB_VECBOOK_BLOCK) d4[i] = s4[i];
    } else {
        for (int i = threadIdx.x; i < n; i += LOB_VECBOOK_BLOCK) dst[i] = stage[i];
    }
}

// One block = LOB_VECBOOK_BOOKS consecutive books.
//   Levels.  A book's four planes are four 16-byte aligned runs of D words in its current record (lob_env.h: the device layout),
// and every book's record is elsewhere in HBM.  Eight lanes share a book: lane (side, j) fetches quad j of the side's prices and
// quad j of its volumes, two 16-byte loads, issued for both passes before the first is waited for -- dump_kernel's 4 x D
// dependent 4-byte look-ups per lane become one round trip for the record word and one for the quads.  No load is under a branch:
// a lane without a quad (D <= 8), a book past the batch and a book without a snapshot (rec_cur < 0: record 0 is read) fetch a valid
// address and the result is masked.
//   dump_kernel reports volume(price of level l), a look-up by price key among the side's levels.  The streams are validated to
// have strictly monotone price keys per side (lob_validate_stream), so that look-up hits level l itself and the value is the
// record's vol[l]; it is 0 where the price is 0 (no snapshot) or compares with nothing (a NaN).  The price is the record's f32
// itself: the dump widens it to f64, the contract rounds it back.  Volumes: i32 -> f32 in registers (round to nearest even).
//   Own words and time.  Lane per book of the first wave: coalesced loads of the field arrays, the values as dump_kernel derives
// them, four 16-byte writes into the staging row.
//   Stores: see vec_book_rows_out.  Nothing is written but the caller's buffers.
__global__ __launch_bounds__(LOB_VECBOOK_BLOCK) void vec_book_kernel(VecBookSrc s, lob_vec_book_out out, int lv16, int own16) {
    __shared__ __attribute__((aligned(16))) f32 lv[LOB_VECBOOK_BOOKS * 4 * LOB_MAX_DEPTH];
    __shared__ __attribute__((aligned(16))) f32 ow[LOB_VECBOOK_BOOKS * LOB_VEC_OWN_WORDS];
    const int first = blockIdx.x * LOB_VECBOOK_BOOKS;
    const int rows = s.B - first < LOB_VECBOOK_BOOKS ? s.B - first : LOB_VECBOOK_BOOKS;
    const int D = s.D;
    if (out.levels) {   // (uniform)
        const int qpa = (D + 3) >> 2;   // 16-byte quads per level array
        const int sub = threadIdx.x & (LOB_VECBOOK_LANES - 1);
        const bool lane_on = sub < 2 * qpa;
        const int side = lane_on && sub >= qpa ? 1 : 0;
        const int j = lane_on ? sub - side * qpa : 0;
        const int w_px = (side ? s.w_bid_px : s.w_ask_px) + 4 * j, w_vol = (side ? s.w_bid_vol : s.w_ask_vol) + 4 * j;
        i32 rec[LOB_VECBOOK_PASSES];
        uint4 px[LOB_VECBOOK_PASSES], vol[LOB_VECBOOK_PASSES];
#pragma unroll
        for (int p = 0; p < LOB_VECBOOK_PASSES; p++) {
            const int bl = p * LOB_VECBOOK_PASS + (threadIdx.x >> 3);
            rec[p] = s.rec_cur[first + (bl < rows ? bl : rows - 1)];
        }
#pragma unroll
        for (int p = 0; p < LOB_VECBOOK_PASSES; p++) {
            const int bl = p * LOB_VECBOOK_PASS + (threadIdx.x >> 3);
            const int b = first + (bl < rows ? bl : rows - 1);
            const size_t start = s.rec_phase ? (size_t)s.rec_phase[b] : (size_t)b * (size_t)s.n_events;   // EnvCtx (lob_env.h)
            const uint32_t* r = s.records + (start + (size_t)(rec[p] < 0 ? 0 : rec[p])) * (size_t)s.Wd;
            px[p] = *reinterpret_cast<const uint4*>(r + w_px);
            vol[p] = *reinterpret_cast<const uint4*>(r + w_vol);
        }
#pragma unroll
        for (int p = 0; p < LOB_VECBOOK_PASSES; p++) {
            const int bl = p * LOB_VECBOOK_PASS + (threadIdx.x >> 3);
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
        const int b = first + threadIdx.x;
        if (out.time_ms) out.time_ms[b] = (i64)s.time_ms[b];
        if (out.own) {
            const i32 a_on = s.a_on[b], b_on = s.b_on[b];
            const f64 a_opx = s.a_opx[b], b_opx = s.b_opx[b];
            const i64 a_rem = s.a_osz[b] - s.a_oex[b], b_rem = s.b_osz[b] - s.b_oex[b];
            const i64 a_oqh = s.a_oqh[b], b_oqh = s.b_oqh[b];
            float4 q0, q1, q2, q3;   // LOB_OWN_* order
            q0.x = (f32)s.position[b];
            q0.y = (f32)a_on;
            q0.z = a_on ? (f32)a_opx : 0.0f;
            q0.w = a_on ? (f32)(a_rem > 0 ? a_rem : 0) : 0.0f;
            q1.x = a_on ? (f32)a_oqh : 0.0f;
            q1.y = (f32)b_on;
            q1.z = b_on ? (f32)b_opx : 0.0f;
            q1.w = b_on ? (f32)(b_rem > 0 ? b_rem : 0) : 0.0f;
            q2.x = b_on ? (f32)b_oqh : 0.0f;
            q2.y = (f32)s.ask_quote[b];
            q2.z = (f32)s.bid_quote[b];
            q2.w = (f32)s.last_action[b];
            q3.x = (f32)s.pnl_step[b];
            q3.y = (f32)s.ep_pnl[b];
            q3.z = (f32)s.ep_reward[b];
            q3.w = (f32)s.total_ticks[b];
            float4* o = reinterpret_cast<float4*>(ow + threadIdx.x * LOB_VEC_OWN_WORDS);
            o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3;
        }
    }
    __syncthreads();
    if (out.levels) vec_book_rows_out(lv, out.levels + (size_t)first * 4 * (size_t)D, rows * 4 * D, lv16);
    if (out.own) vec_book_rows_out(ow, out.own + (size_t)first * LOB_VEC_OWN_WORDS, rows * LOB_VEC_OWN_WORDS, own16);
}

void lobk_vec_book(hipStream_t st, const VecBookSrc& s, const lob_vec_book_out& out) {
    const int lv16 = ((uintptr_t)out.levels & 15) == 0 ? 1 : 0, own16 = ((uintptr_t)out.own & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(vec_book_kernel, dim3((s.B + LOB_VECBOOK_BOOKS - 1) / LOB_VECBOOK_BOOKS), dim3(LOB_VECBOOK_BLOCK), 0, st, s, out, lv16, own16);
}
