// Translation unit of the multi-step look-ahead of the vector-env interface (include/lob_engine.h lob_vec_rollout; lob_launch.h
// RolloutSrc): vec_rollout_kernel.  A unit of its own, so that every other unit is compiled from what it was.
// gfx950 only; no CPU execution path.
//   What `horizon` consecutive lob_vec_step calls would write for every book under each of `n_plans` action plans, from device memory
// to device memory -- and nothing of the engine's state moves.  It is vec_peek_kernel (lob_tu_vecpeek.hip) with a loop around the step:
// the agent half runs on a private copy of the book's scalars (EnvR in an LDS slot, env_load once) that carries from step to step
// exactly what env_store would have written and the next launch's env_load read back; the market half is the track the pre-pass has
// written, followed through the private cursor e.k / e.rec_cur.  The step is the family's one private step (lob_peek.h).  What one
// step did not need: the entry a full PnL window replaces may be one the plan itself has pushed (roll_rm_prep below).
#define LOB_TU_SPLIT 1
#define LOB_TU_VECROLL 1
#include <hip/hip_runtime.h>

#include "lob_internal.h"
#include "lob_kernels.h"
#include "lob_peek.h"   // the family's shape and its private step

// rm_prep (lob_env.h) `n` pushes into a look-ahead that stores nothing.  A window of w entries that is full replaces the entry w pushes
// back: the n-th push of the look-ahead (n = 0, 1, ...) meets one of its own if and only if n >= w, whatever the fill at entry --
// below that the engine's ring still holds the entry.  w == 1: its own previous push, `prev`.  Otherwise push n - w, which the lane has
// left in `shadow` (its last w pushes, push j at [j % w][lane]; lob_launch.h RolloutSrc -- null when w >= horizon, where n < w holds).
__device__ inline void roll_rm_prep(const RMPtrs& r, int B, int b, RMReg& g, int n, f64 prev, const f64* shadow, size_t lanes, size_t lane) {
    if (g.cnt < r.w) {
        g.slot = (g.cnt == 0) ? 0 : (g.head + 1 == r.w ? 0 : g.head + 1);
        g.old = 0.0;
    } else {
        g.slot = g.head + 1 == r.w ? 0 : g.head + 1;  // the oldest entry is replaced
        if (n < r.w) g.old = r.ring[(size_t)g.slot * B + b];
        else if (r.w == 1) g.old = prev;
        else g.old = shadow[(size_t)(n % r.w) * lanes + lane];
    }
}

// One lane per (plan, book), plan-major: block i is plan i / blocks_per_plane over the books 64 * (i % blocks_per_plane) ..., so a wave
// holds 64 consecutive books under ONE plan -- env_load's [B] field arrays and actions[(p * H + h) * B + b] are read coalesced, the
// wave's part of every output plane is contiguous.  The actions differ per lane, so do_action may diverge inside the wave; a plan that
// is the same for every book runs uniform.
//   Per step, lob_vec_step's rules on the private state: a book steps when lob_get_terminal is 0 and its action is one of the nine
// (vec_actions_kernel); otherwise, and when the step runs dry (env_kernel's `ok` false: the mutated state is kept, done == 2), the
// reward is +0.0 and the lane's LDS row keeps the obs of the last completed step -- slot 2 of S.vars when none has completed.  Actions
// out of range are compared, never used, and not counted.
//   The rows leave through LDS as in vec_rows_out (lob_tu_vec.hip): the block's rows are contiguous in the plan's plane.
//   RING (lob_look_ring on a ring track; lob_peek.h): a step that would run past the ring's last entry while the
// pre-pass is not complete ends the plan for that book -- that step and all later ones reward +0.0, `stepped`, obs and ret as they
// stand behind the last completed step, terminal LOB_LOOK_AHEAD, the cell counted in a.look_cnt[0] -- and raises nothing in the engine's
// error word.  A roll-out starts at the real cursor: it is never behind.
template <bool T2, bool RING>
__global__ void __launch_bounds__(LOB_LOOK_BLOCK) vec_rollout_kernel(const DevParams* __restrict__ Pp, DevState S, RolloutSrc a) {
    const DevParams& P = *Pp;  // parameters read through the scalar cache, never copied to scratch
    constexpr int TM = T2 ? 2 : LOB_MAX_TRADES;
    __shared__ TickLds tick_lds;
    stage_ticks(P, tick_lds);
    __shared__ EnvSlot lds_env[LOB_LOOK_BLOCK];
    __shared__ f32 stage[LOB_LOOK_BLOCK * LOB_MAX_VARS];
    const LookPlane pl = look_plane(a.Bpad);
    const int p = pl.plane, b = pl.b;
    const int B = a.B, V = P.V, H = a.horizon;
    const lob_vec_rollout_out& out = a.out;
    bool ahead = false;
    if (b < B) {
        EnvCtx c(P, S, b, &tick_lds);
        LookWin w = {0, 0, 1};
        if constexpr (RING) { w = look_window(S, b); look_ring_ctx(c, w); }
        EnvR& e = lds_env[threadIdx.x].e;
        env_load(S, b, e);
        // the two PnL windows: read by the LOB_REWARD_NORMED reward only, so only kept then
        const bool win = P.reward_measure == LOB_REWARD_NORMED;
        RMReg wu = rm_zero(), wd = wu;
        if (win) { rm_load(S.pnl_ups, b, wu); rm_load(S.pnl_downs, b, wd); }
        const size_t lanes = (size_t)a.n_plans * (size_t)a.Bpad, lane = (size_t)p * (size_t)a.Bpad + (size_t)b;
        f64* const sh_u = a.shadow;
        f64* const sh_d = a.shadow ? a.shadow + (size_t)S.pnl_ups.w * lanes : nullptr;
        f64 prev_u = 0.0, prev_d = 0.0;
        if (out.obs) look_obs_slot2(S, b, &stage[threadIdx.x * V], V);
        int n_done = 0;
        f64 acc = 0.0, disc = 1.0;
        const i32* act = a.actions + (size_t)p * (size_t)H * (size_t)B + (size_t)b;
        for (int h = 0; h < H; h++) {
            const int action = act[(size_t)h * (size_t)B];
            f64 reward = 0.0;
            if (lob_terminal(P, e.done, e.time_ms) == 0 && action >= 0 && action < LOB_N_ACTIONS) {
                // the private cursor stands where the previous step's env_store would have left the engine's
                LookLoads L;
                look_step_loads<TM>(c, e.k, e.rec_cur, L);
                StepAgg g;
                if (look_step_run<TM>(c, e, action, g, L) != 2) {
                    e.pnl_step = g.pnl;
                    if (win) {
                        roll_rm_prep(S.pnl_ups, S.B, b, wu, n_done, prev_u, sh_u, lanes, lane);
                        roll_rm_prep(S.pnl_downs, S.B, b, wd, n_done, prev_d, sh_d, lanes, lane);
                        prev_u = peek_push_up(e); prev_d = peek_push_down(e);
                        if (sh_u) {
                            sh_u[(size_t)(n_done % S.pnl_ups.w) * lanes + lane] = prev_u;
                            sh_d[(size_t)(n_done % S.pnl_downs.w) * lanes + lane] = prev_d;
                        }
                    }
                    peek_push(c, e, wu, wd);
                    reward = look_step_finish(c, e, g, wu, wd, out.obs != nullptr, stage, V);
                    n_done++;
                } else {
                    if constexpr (RING) ahead = !w.complete;
                }
            }
            if (out.reward) out.reward[((size_t)p * (size_t)H + (size_t)h) * (size_t)B + (size_t)b] = reward;
            if constexpr (RING) {
                // the plan ends here: the rewards behind it are +0.0, and acc + d * (+0.0) leaves acc (never -0.0) as it is
                if (ahead) {
                    if (out.reward) for (int h2 = h + 1; h2 < H; h2++) out.reward[((size_t)p * (size_t)H + (size_t)h2) * (size_t)B + (size_t)b] = 0.0;
                    break;
                }
            }
            acc = __dadd_rn(acc, __dmul_rn(disc, reward));
            disc = __dmul_rn(disc, a.gamma);
        }
        const size_t o = (size_t)p * (size_t)B + (size_t)b;
        if (out.terminal) out.terminal[o] = (uint8_t)((RING && ahead) ? LOB_LOOK_AHEAD : lob_terminal(P, e.done, e.time_ms));
        if (out.stepped) out.stepped[o] = n_done;
        if (out.ret) out.ret[o] = acc;
    }
    if (out.obs) look_rows_out(stage, out.obs, p, 1, B, pl.first_b, V);   // (uniform)
    if constexpr (RING) look_count(a.look_cnt, ahead);
}

void lobk_vec_rollout(hipStream_t st, bool t2, bool ring, const DevParams* Pd, const DevState& S, const RolloutSrc& a) {
    const dim3 grid((unsigned)(a.n_plans * (a.Bpad / LOB_LOOK_BLOCK))), block(LOB_LOOK_BLOCK);
    if (ring) {
        if (t2) hipLaunchKernelGGL((vec_rollout_kernel<true, true>), grid, block, 0, st, Pd, S, a);
        else hipLaunchKernelGGL((vec_rollout_kernel<false, true>), grid, block, 0, st, Pd, S, a);
    } else if (t2) hipLaunchKernelGGL((vec_rollout_kernel<true, false>), grid, block, 0, st, Pd, S, a);
    else hipLaunchKernelGGL((vec_rollout_kernel<false, false>), grid, block, 0, st, Pd, S, a);
}
