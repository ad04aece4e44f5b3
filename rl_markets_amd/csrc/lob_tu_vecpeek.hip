// Translation unit of the one-step look-ahead of the vector-env interface (include/lob_engine.h lob_vec_peek; lob_launch.h PeekSrc;
// DESIGN.md 7j): vec_peek_kernel.  A unit of its own, so that the units of the step and of lob_reset are compiled from what they
// were.  gfx950 only; no CPU execution path.
//   What lob_vec_step would write for every book had every book been given action a, for each a of a mask, from device memory to
// device memory -- and nothing of the engine's state moves: the agent half of a step runs on a private copy of the book's scalars
// (EnvR in an LDS slot, env_load) that is never stored, the market half is the track the pre-pass has written.  The step itself is
// env_kernel's, held once for the look-ahead family in lob_peek.h: look_step_loads / look_step_run, then peek_push and
// look_step_finish -- the epilogue without its stores, because step_epilogue's rm_apply writes the two PnL windows.  Of everything those functions reach, the
// windows were the only memory written besides EnvCtx::err's flag (a condition the step itself would have raised for that action)
// and, in -DLOB_PROF builds, the pass clocks.
#define LOB_TU_SPLIT 1
#define LOB_TU_VECPEEK 1
#include <hip/hip_runtime.h>

#include "lob_internal.h"
#include "lob_kernels.h"
#include "lob_peek.h"   // the family's shape and its private step

// One lane per (action, book), action-major: block i is the (i / blocks_per_plane)-th action of the mask over the books
// 64 * (i % blocks_per_plane) ..., so a wave holds 64 consecutive books under ONE action -- env_load's [B] field arrays are read
// coalesced, do_action is uniform over the wave, the wave's part of every output plane is contiguous.  The waves of the same books
// under the other actions read the same track entries and rows; nothing shares them explicitly.
//   A book that is over (lob_get_terminal != 0) does not step, as under vec_actions_kernel: stepped 0, reward +0.0, obs = slot 2 of
// S.vars.  A step that runs dry: stepped 0, reward +0.0, terminal 2, obs = slot 2 (vec_observe_kernel behind env_kernel's `ok` false).
//   The rows leave through LDS as in vec_rows_out (lob_tu_vec.hip): the block's rows are contiguous in the action's plane.
//   RING (lob_look_ring on a ring track; lob_peek.h): a step that would run past the ring's last entry while the
// pre-pass is not complete is an AHEAD cell -- stepped 0, reward +0.0, obs = slot 2, terminal LOB_LOOK_AHEAD, counted in a.look_cnt[0]
// -- and raises nothing in the engine's error word.  A peek starts at the real cursor: it is never behind.
template <bool T2, bool RING>
__global__ void __launch_bounds__(LOB_LOOK_BLOCK) vec_peek_kernel(const DevParams* __restrict__ Pp, DevState S, PeekSrc a) {
    const DevParams& P = *Pp;  // parameters read through the scalar cache, never copied to scratch
    constexpr int TM = T2 ? 2 : LOB_MAX_TRADES;
    __shared__ TickLds tick_lds;
    stage_ticks(P, tick_lds);
    __shared__ EnvSlot lds_env[LOB_LOOK_BLOCK];
    __shared__ f32 stage[LOB_LOOK_BLOCK * LOB_MAX_VARS];
    const LookPlane pl = look_plane(a.Bpad);
    const int action = a.act[pl.plane];
    const int b = pl.b, B = a.B, V = P.V;
    const lob_vec_peek_out& out = a.out;
    bool ahead = false;
    if (b < B) {
        const int k0 = S.k[b], rc0 = S.rec_cur[b];  // in flight together
        const i32 done0 = S.done[b], tm0 = S.time_ms[b];
        int term = lob_terminal(P, done0, tm0);
        bool ok = false;
        f64 reward = 0.0;
        if (term == 0) {
            EnvCtx c(P, S, b, &tick_lds);
            LookWin w = {0, 0, 1};
            if constexpr (RING) { w = look_window(S, b); look_ring_ctx(c, w); }
            LookLoads L;   // requested before the bulk of the state, so that the round trips overlap
            look_step_loads<TM>(c, k0, rc0, L);
            EnvR& e = lds_env[threadIdx.x].e;
            env_load(S, b, e);
            StepAgg g;
            ok = look_step_run<TM>(c, e, action, g, L) != 2;
            if (ok) {
                e.pnl_step = g.pnl;
                RMReg wu, wd;
                rm_load(S.pnl_ups, b, wu); rm_load(S.pnl_downs, b, wd);
                rm_prep(S.pnl_ups, S.B, b, wu); rm_prep(S.pnl_downs, S.B, b, wd);
                peek_push(c, e, wu, wd);
                reward = look_step_finish(c, e, g, wu, wd, out.obs != nullptr, stage, V);
            }
            term = lob_terminal(P, e.done, e.time_ms);
            if constexpr (RING) {
                if (!ok && !w.complete) { ahead = true; term = LOB_LOOK_AHEAD; }
            }
        }
        if (!ok && out.obs) look_obs_slot2(S, b, &stage[threadIdx.x * V], V);
        const size_t o = (size_t)action * (size_t)B + (size_t)b;
        if (out.reward) out.reward[o] = ok ? reward : 0.0;
        if (out.terminal) out.terminal[o] = (uint8_t)term;
        if (out.stepped) out.stepped[o] = ok ? 1 : 0;
    }
    if (out.obs) look_rows_out(stage, out.obs, action, 1, B, pl.first_b, V);   // (uniform)
    if constexpr (RING) look_count(a.look_cnt, ahead);
}

void lobk_vec_peek(hipStream_t st, bool t2, bool ring, const DevParams* Pd, const DevState& S, const PeekSrc& a) {
    const dim3 grid((unsigned)(a.n_act * (a.Bpad / LOB_LOOK_BLOCK))), block(LOB_LOOK_BLOCK);
    if (ring) {
        if (t2) hipLaunchKernelGGL((vec_peek_kernel<true, true>), grid, block, 0, st, Pd, S, a);
        else hipLaunchKernelGGL((vec_peek_kernel<false, true>), grid, block, 0, st, Pd, S, a);
    } else if (t2) hipLaunchKernelGGL((vec_peek_kernel<true, false>), grid, block, 0, st, Pd, S, a);
    else hipLaunchKernelGGL((vec_peek_kernel<false, false>), grid, block, 0, st, Pd, S, a);
}
