// Translation unit of the vector-env interface (include/lob_engine.h lob_vec_*; lob_launch.h VecSrc):
// vec_actions_kernel / vec_observe_kernel.  A unit of its own, so that the units of the step and of lob_reset are compiled from
// what they were.  gfx950 only; no CPU execution path.
//   One agent step of an external policy = vec_actions_kernel -> env_kernel (unchanged, lob_tu_env.hip) -> vec_observe_kernel, all
// on the engine's stream: the actions are read from device memory, the observations written to device memory.
#define LOB_TU_SPLIT 1
#define LOB_TU_VEC 1
#include <hip/hip_runtime.h>

#include "lob_internal.h"
#include "lob_kernels.h"

static_assert(LOB_VEC_BLOCK == 256 && LOB_VEC_BLOCK % 64 == 0, "four waves per block");
#define LOB_VEC_WAVES (LOB_VEC_BLOCK / 64)

// lob_get_terminal's value from the two field arrays it reads (is_open, lob_env.h)
__device__ __forceinline__ int vec_terminal(const VecSrc& s, i32 done, i32 time_ms) {
    const bool open = ((i64)time_ms > s.open_ms + 30 * 60000LL) && ((i64)time_ms < s.close_ms - 30 * 60000LL);
    return done == 2 ? 2 : (open ? 0 : 1);
}

// `pred` counted over the block, one lane gets the total: a ballot + popcount per wave, the waves' counts through LDS.  Every thread
// of the block calls this (block barrier).
__device__ __forceinline__ int vec_block_count(bool pred, int* wave_n) {
    const int n = __popcll(__ballot(pred));
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
    __syncthreads();
    int tot = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < LOB_VEC_WAVES; w++) tot += wave_n[w];
    }
    return tot;
}

// Action intake: lane per book.  The book steps in this call when it is live (lob_get_terminal == 0: the runner's
// `while (!env.isTerminal())`, serial.cpp:18-34) and its action is one of the nine; the env kernel launched behind this one with no
// action array takes `go = h.stepped != 0` and `action = h.action` -- the rule the act kernels arm it by, so env_kernel is the
// kernel lob_step runs, untouched.  An action out of range is compared, never used: the header of such a book keeps its action
// word, stepped = 0 keeps the env kernel off the book.  The count of such entries goes to the engine's word with at most one
// atomic per block (same-address atomics at the end of every wave: DESIGN.md 4), and none at all when the block has none.
__global__ __launch_bounds__(LOB_VEC_BLOCK) void vec_actions_kernel(VecSrc s, const i32* __restrict__ actions) {
    __shared__ int wave_n[LOB_VEC_WAVES];
    const int b = blockIdx.x * LOB_VEC_BLOCK + threadIdx.x;
    const bool in = b < s.B;
    bool bad = false;
    if (in) {
        const i32 a = actions[b];
        const i32 done = s.done[b], tm = s.time_ms[b];
        bad = a < 0 || a >= LOB_N_ACTIONS;
        const bool go = !bad && vec_terminal(s, done, tm) == 0;
        LHdr& h = s.hdr[b];
        if (go) h.action = a;
        h.stepped = go ? 1 : 0;
    }
    const int n_bad = vec_block_count(bad, wave_n);
    if (threadIdx.x == 0 && n_bad) atomicAdd(s.n_bad, (u64)n_bad);
}

// The rows a block has staged in LDS ([LOB_VEC_BLOCK][V]) leave as consecutive words of consecutive lanes: the block's rows are
// contiguous in `obs`, so no lane issues V stores strided by V.  Every thread of the block calls this (block barrier).
__device__ __forceinline__ void vec_rows_out(const VecSrc& s, const f32* stage, f32* obs) {
    __syncthreads();
    const int first = blockIdx.x * LOB_VEC_BLOCK;
    const int rows = s.B - first < LOB_VEC_BLOCK ? s.B - first : LOB_VEC_BLOCK;
    f32* dst = obs + (size_t)first * (size_t)s.V;
    for (int i = threadIdx.x; i < rows * s.V; i += LOB_VEC_BLOCK) dst[i] = stage[i];
}

// Observation: lane per book, one launch for obs / reward / terminal / stepped / n_live.  Nothing is evaluated again: the env kernel
// has left the new state in the book's slot-2 copy of S.vars and the reward in LHdr::reward, and for a book that did not step
// slot 2 still holds the state of its last completed step (reset_kernel: the first state) -- what rl::State keeps, and what the
// oracle's record keeps.  `after_step` 0: stepped is written 0 whatever the headers say.
//   The rows of a block are contiguous in `obs`, LOB_VEC_BLOCK x V x 4 bytes.  `vec16` (V x 4 a multiple of 16 and obs 16-byte
// aligned): a lane moves its row as V / 4 16-byte loads and stores (V = 8: two global_store_dwordx4 per lane, a wave fills
// 64 x 32 B without a gap).  Otherwise the rows go through LDS (vec_rows_out).
__global__ __launch_bounds__(LOB_VEC_BLOCK) void vec_observe_kernel(VecSrc s, lob_vec_out out, int after_step, int vec16) {
    __shared__ int wave_n[LOB_VEC_WAVES];
    __shared__ f32 stage[LOB_VEC_BLOCK * LOB_MAX_VARS];
    const int b = blockIdx.x * LOB_VEC_BLOCK + threadIdx.x;
    const bool in = b < s.B;
    const int V = s.V;
    int term = 1;
    if (in) {
        term = vec_terminal(s, s.done[b], s.time_ms[b]);
        const LHdr& h = s.hdr[b];
        const i32 st = after_step && h.stepped != 0 ? 1 : 0;
        if (out.reward) out.reward[b] = st ? h.reward : 0.0;
        if (out.stepped) out.stepped[b] = st;
        if (out.terminal) out.terminal[b] = (uint8_t)term;
        if (out.obs) {
            const f32* vf = s.vars + ((size_t)b * 3 + 2) * 16;
            if (vec16) {
                const float4* src = reinterpret_cast<const float4*>(vf);
                float4* dst = reinterpret_cast<float4*>(out.obs + (size_t)b * (size_t)V);
                for (int q = 0; q < (V >> 2); q++) dst[q] = src[q];
            } else {
                for (int i = 0; i < V; i++) stage[threadIdx.x * V + i] = vf[i];
            }
        }
    }
    if (out.obs && !vec16) vec_rows_out(s, stage, out.obs);   // (uniform)
    const int live = vec_block_count(in && term == 0, wave_n);
    if (threadIdx.x == 0 && live && out.n_live) atomicAdd(out.n_live, live);
}

// lob_vec_observe: the same outputs with no step behind them.  State and reward are evaluated from the environment as
// get_state_kernel evaluates them (the position may have changed since the last step: lob_clear_inventory) -- except the state of
// a book that is out of data, whose slot 2 is kept: the step that ran dry consumed events without completing, and the state of
// the last completed step is the one the contract names.  The rows leave through LDS.
__global__ __launch_bounds__(LOB_VEC_BLOCK) void vec_observe_derive_kernel(VecSrc s, const DevParams* __restrict__ Pp, DevState S, lob_vec_out out) {
    const DevParams& P = *Pp;  // parameters read through the scalar cache, never copied to scratch
    __shared__ int wave_n[LOB_VEC_WAVES];
    __shared__ f32 stage[LOB_VEC_BLOCK * LOB_MAX_VARS];
    __shared__ TickLds tick_lds;
    stage_ticks(P, tick_lds);
    const int b = blockIdx.x * LOB_VEC_BLOCK + threadIdx.x;
    const bool in = b < s.B;
    const int V = s.V;
    int term = 1;
    if (in) {
        term = vec_terminal(s, s.done[b], s.time_ms[b]);
        EnvCtx c(P, S, b, &tick_lds);
        EnvR e;
        env_load(S, b, e);
        if (out.obs) {
            if (term != 2) {
                const Track tk = state_track(c, e);
                for (int i = 0; i < V; i++) stage[threadIdx.x * V + i] = (f32)get_variable(c, e, P.vars[i], tk);
            } else {
                const f32* vf = s.vars + ((size_t)b * 3 + 2) * 16;
                for (int i = 0; i < V; i++) stage[threadIdx.x * V + i] = vf[i];
            }
        }
        if (out.reward) out.reward[b] = get_reward(c, e);
        if (out.stepped) out.stepped[b] = 0;
        if (out.terminal) out.terminal[b] = (uint8_t)term;
    }
    if (out.obs) vec_rows_out(s, stage, out.obs);   // (uniform)
    const int live = vec_block_count(in && term == 0, wave_n);
    if (threadIdx.x == 0 && live && out.n_live) atomicAdd(out.n_live, live);
}

void lobk_vec_actions(hipStream_t st, const VecSrc& s, const i32* dev_actions) {
    hipLaunchKernelGGL(vec_actions_kernel, dim3((s.B + LOB_VEC_BLOCK - 1) / LOB_VEC_BLOCK), dim3(LOB_VEC_BLOCK), 0, st, s, dev_actions);
}

void lobk_vec_observe(hipStream_t st, bool derive, bool after_step, const VecSrc& s, const DevParams* Pd, const DevState& S, const lob_vec_out& out) {
    const dim3 grid((s.B + LOB_VEC_BLOCK - 1) / LOB_VEC_BLOCK), block(LOB_VEC_BLOCK);
    const int vec16 = (s.V % 4 == 0 && ((uintptr_t)out.obs & 15) == 0) ? 1 : 0;
    if (derive) hipLaunchKernelGGL(vec_observe_derive_kernel, grid, block, 0, st, s, Pd, S, out);
    else hipLaunchKernelGGL(vec_observe_kernel, grid, block, 0, st, s, out, after_step ? 1 : 0, vec16);
}
