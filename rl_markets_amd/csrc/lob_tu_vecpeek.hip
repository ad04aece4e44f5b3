// Translation unit of the one-step look-ahead of the vector-env interface (include/lob_engine.h lob_vec_peek; lob_launch.h PeekSrc;
// DESIGN.md 7j): vec_peek_kernel.  A unit of its own, so that the units of the step and of lob_reset are compiled from what they
// were.  gfx950 only; no CPU execution path.
//   What lob_vec_step would write for every book had every book been given action a, for each a of a mask, from device memory to
// device memory -- and nothing of the engine's state moves: the agent half of a step runs on a private copy of the book's scalars
// (EnvR in an LDS slot, env_load) that is never stored, the market half is the track the pre-pass has written.  The step itself is
// env_kernel's, call for call: step_prologue, event_loop_fast (two trade slots) or the step_event loop, then the epilogue -- restated
// in lob_peek.h without its stores, because step_epilogue's rm_apply writes the two PnL windows.  Of everything those functions reach, the
// windows were the only memory written besides EnvCtx::err's flag (a condition the step itself would have raised for that action)
// and, in -DLOB_PROF builds, the pass clocks.
#define LOB_TU_SPLIT 1
#define LOB_TU_VECPEEK 1
#include <hip/hip_runtime.h>

#include "lob_internal.h"
#include "lob_kernels.h"
#include "lob_peek.h"   // the epilogue without its stores: peek_epilogue, peek_reward

#define LOB_PEEK_BLOCK 64   // one wave per block: 64 consecutive books under one action (env_kernel<64, TM>'s shape)

// One lane per (action, book), action-major: block i is the (i / blocks_per_plane)-th action of the mask over the books
// 64 * (i % blocks_per_plane) ..., so a wave holds 64 consecutive books under ONE action -- env_load's [B] field arrays are read
// coalesced, do_action is uniform over the wave, the wave's part of every output plane is contiguous.  The waves of the same books
// under the other actions read the same track entries and rows; nothing shares them explicitly.
//   A book that is over (lob_get_terminal != 0) does not step, as under vec_actions_kernel: stepped 0, reward +0.0, obs = slot 2 of
// S.vars.  A step that runs dry: stepped 0, reward +0.0, terminal 2, obs = slot 2 (vec_observe_kernel behind env_kernel's `ok` false).
//   The rows leave through LDS as in vec_rows_out (lob_tu_vec.hip): the block's rows are contiguous in the action's plane.
template <bool T2>
__global__ void __launch_bounds__(LOB_PEEK_BLOCK) vec_peek_kernel(const DevParams* __restrict__ Pp, DevState S, PeekSrc a) {
    const DevParams& P = *Pp;  // parameters read through the scalar cache, never copied to scratch
    constexpr int TM = T2 ? 2 : LOB_MAX_TRADES;
    __shared__ TickLds tick_lds;
    stage_ticks(P, tick_lds);
    __shared__ EnvSlot lds_env[LOB_PEEK_BLOCK];
    __shared__ f32 stage[LOB_PEEK_BLOCK * LOB_MAX_VARS];
    const int per_plane = a.Bpad / LOB_PEEK_BLOCK;
    const int ai = blockIdx.x / per_plane;
    const int first_b = (blockIdx.x - ai * per_plane) * LOB_PEEK_BLOCK;
    const int action = a.act[ai];
    const int b = first_b + threadIdx.x;
    const int B = a.B, V = P.V;
    const lob_vec_peek_out& out = a.out;
    if (b < B) {
        const int k0 = S.k[b], rc0 = S.rec_cur[b];  // in flight together
        const i32 done0 = S.done[b], tm0 = S.time_ms[b];
        int term = done0 == 2 ? 2 : (is_open(P, tm0) ? 0 : 1);   // lob_get_terminal (lob_tu_vec.hip vec_terminal)
        bool ok = false;
        f64 reward = 0.0;
        if (term == 0) {
            EnvCtx c(P, S, b, &tick_lds);
            const TrackHead64 t0 = c.track_head64(k0);
            RowFull cur;
            row_full_load(c, rc0, cur);
            RowFull first;
            if (LOB_FAST_PASS && TM == 2) { const int last_row = c.n_ev() - 1; row_full_load(c, rc0 + 1 < last_row ? rc0 + 1 : last_row, first); }
            EnvR& e = lds_env[threadIdx.x].e;
            env_load(S, b, e);
            StepAgg g;
            step_prologue(c, e, action, g, cur);
            int st;
            if (LOB_FAST_PASS && TM == 2) {
                TrackHead64 t = t0;
                st = event_loop_fast(c, e, g, t, first);
            } else {
                TrackHead t;
                t.rec_first = t0.rec_first; t.rec_last = t0.rec_last; t.time_ms = t0.time_ms; t.tick_ap0 = t0.tick_ap0;
                t.tick_bp0 = t0.tick_bp0; t.info = t0.info; t.mid = t0.mid;
                do {
                    const TrackHead tn = c.track_head(e.k + 1);
                    st = step_event<TM>(c, e, g, t);
                    t = tn;
                } while (st == 0);
            }
            ok = st != 2;
            if (ok) {
                RMReg wu, wd;
                peek_epilogue(c, e, g, wu, wd);
                if (out.obs) {
                    const Track tk = state_track(c, e);
                    for (int i = 0; i < V; i++) stage[threadIdx.x * V + i] = (f32)get_variable(c, e, P.vars[i], tk);
                }
                reward = peek_reward(c, e, wu, wd);
            }
            term = e.done == 2 ? 2 : (is_open(P, e.time_ms) ? 0 : 1);
        }
        if (!ok && out.obs) {
            const f32* vf = S.vars + ((size_t)b * 3 + 2) * 16;
            for (int i = 0; i < V; i++) stage[threadIdx.x * V + i] = vf[i];
        }
        const size_t o = (size_t)action * (size_t)B + (size_t)b;
        if (out.reward) out.reward[o] = ok ? reward : 0.0;
        if (out.terminal) out.terminal[o] = (uint8_t)term;
        if (out.stepped) out.stepped[o] = ok ? 1 : 0;
    }
    if (out.obs) {   // (uniform)
        __syncthreads();
        const int rows = B - first_b < LOB_PEEK_BLOCK ? B - first_b : LOB_PEEK_BLOCK;
        f32* dst = out.obs + ((size_t)action * (size_t)B + (size_t)first_b) * (size_t)V;
        for (int i = threadIdx.x; i < rows * V; i += LOB_PEEK_BLOCK) dst[i] = stage[i];
    }
}

void lobk_vec_peek(hipStream_t st, bool t2, const DevParams* Pd, const DevState& S, const PeekSrc& a) {
    const dim3 grid((unsigned)(a.n_act * (a.Bpad / LOB_PEEK_BLOCK))), block(LOB_PEEK_BLOCK);
    if (t2) hipLaunchKernelGGL(vec_peek_kernel<true>, grid, block, 0, st, Pd, S, a);
    else hipLaunchKernelGGL(vec_peek_kernel<false>, grid, block, 0, st, Pd, S, a);
}
