// Translation unit of the engine's own policy on the vector-env interface (include/lob_engine.h lob_vec_act / lob_vec_q;
// lob_launch.h VecActSrc): vec_act_kernel.  A unit of its own, so that the units of the step and of lob_reset are
// compiled from what they were.  gfx950 only; no CPU execution path.
//   Q(s, .) under the engine's weights for every book's latest getState() -- or for the caller's free-standing rows -- from device
// memory to device memory, and the action Agent::action would take there: q_values(), policy_sample() and greedy_sample()
// (lob_learn.h) as act_book (lob_kernels.h) calls them, with none of act_book's bookkeeping.
#define LOB_TU_SPLIT 1
#define LOB_TU_VECACT 1
#include <hip/hip_runtime.h>

#include "lob_internal.h"
#include "lob_kernels.h"

// One WAVE per state, LOB_WAVES_PER_BLOCK states in flight per block, a persistent grid: wave t takes states t, t + waves, ... --
// the 8 KB hash table is staged once per block, not once per four states as in features_kernel and the whole-batch act_kernel
// (65 536 states: 2 048 x 8 KB instead of 16 384 x 8 KB through L2).
//   BOOKS: state s is book s.  The row is slot 2 of S.vars (the latest getState(): env_kernel / reset_kernel / a restore write
// it), the weights are the book's agent's (theta of book s under private theta; DQ: theta_b as well, combined as
// DoubleAgent::action does), terminal comes from the two field arrays lob_get_terminal reads, the policy stream from LHdr::rng_ctr.
// All of these are wave-uniform addresses: scalar loads.  Else: row s of the caller's buffer under a.theta / a.nz, no action.
//   The action.  LOB_ACT_ARGMAX: the lowest index among the maxima, nothing drawn.  LOB_ACT_GREEDY / LOB_ACT_BEHAVIOUR:
// policy_sample(greedy / not) on Rng{seed, book id, rng_ctr}, exactly act_book's call; the new counter is the only word written to
// the engine's state, by lane 0, and only when something was drawn for a live book.  A book that is over: action 0, nothing drawn.
// Every lane computes the sample (the nine values are in every lane's registers), as in act_book: no broadcast, no divergence.
//   Stores: lanes 0..8 the row of nine doubles (72 contiguous bytes), lane 0 the action.  No atomics.
//   Registers: six waves per SIMD is what the block's 26 KB of LDS allows, and the single-vector forms are held to it (72 / 80
// vector registers, no scratch); the double agents' form needs 112 and is left at four -- at five it spills.
template <bool BOOKS, bool DQ>
__global__ void __launch_bounds__(LOB_BLOCK, DQ ? 4 : 6) vec_act_kernel(LOB_PS_ARGS, const uint32_t* __restrict__ rnd_g, VecActSrc a) {
    const DevParams& P = *Pp;   // parameters read through the scalar cache, never copied to scratch
    const DevState& S = *Sp;    // (BOOKS only: the free-standing form never reads through it)
    __shared__ LearnLds L;
    const int w = threadIdx.x >> 6, lane0 = threadIdx.x & 63;
    learn_stage_table(rnd_g, L);   // (every thread of the block: ends in the block barrier)
    const int t0 = __builtin_amdgcn_readfirstlane(blockIdx.x * LOB_WAVES_PER_BLOCK + w);
    const int stride = gridDim.x * LOB_WAVES_PER_BLOCK;
    const int V = P.V;
    f32* row = &L.vars[w][0][0];
#pragma unroll 1
    for (int s = t0; s < a.n; s += stride) {
        // (the lane index behind an opaque copy: left loop-invariant, everything q_values derives from it is hoisted out of the
        // loop and held in ~30 vector registers across it -- 106 instead of 78, four waves per SIMD instead of six)
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        // the state's words into the wave's LDS row, as learn_stage_vars hands a book's over (slots >= V hold 0: q_values)
        const f32* src = BOOKS ? S.vars + ((size_t)s * 3 + 2) * 16 : a.rows + (size_t)s * (size_t)V;
        const f32 vv = lane < V ? src[lane] : 0.0f;
        wave_lds_fence();   // the previous state's readers are done with the row
        if (lane < 16) row[lane] = vv;
        wave_lds_fence();
        const size_t off = BOOKS && P.theta_private ? (size_t)s : 0;
        const f64* theta = BOOKS ? S.theta + off * (size_t)P.M : a.theta;
        const uint32_t* nz = BOOKS ? S.theta_nz + off * LOB_NZ_NWORDS(P.M) : a.nz;
        f64 qs[LOB_N_ACTIONS];
        q_values(P, theta, nz, row, false, L.rnd, L.act_terms, L.vals[w], lane, qs);
        if (DQ) {
            // DoubleAgent::action (agent.cpp:196-204): qs[a] = (getQ + getQb) / 2.0f
            f64 qb[LOB_N_ACTIONS];
            q_values(P, S.theta_b + off * (size_t)P.M, S.theta_b_nz + off * LOB_NZ_NWORDS(P.M), row, false, L.rnd, L.act_terms, L.vals[w], lane, qb);
#pragma unroll
            for (int k = 0; k < LOB_N_ACTIONS; k++) qs[k] = (qs[k] + qb[k]) / 2.0;
        }
        if (a.q && lane < LOB_N_ACTIONS) a.q[(size_t)s * LOB_N_ACTIONS + lane] = sel9(qs, lane);
        if (BOOKS && a.action) {   // (uniform)
            const i32 done = S.done[s], tm = S.time_ms[s];
            const bool live = done != 2 && is_open(P, tm);   // lob_get_terminal == 0 (lob_tu_vec.hip vec_terminal)
            int action = 0;
            if (live) {   // (uniform)
                if (a.mode == LOB_ACT_ARGMAX) {
                    f64 best = qs[0];
#pragma unroll
                    for (int k = 1; k < LOB_N_ACTIONS; k++)
                        if (qs[k] > best) { action = k; best = qs[k]; }
                } else {
                    const u64 ctr = S.hdr[s].rng_ctr;   // (one scalar load)
                    Rng g{P.seed, P.book_id_offset + (u64)s, ctr};
                    action = policy_sample(P, qs, a.mode == LOB_ACT_GREEDY, g);
                    if (lane == 0 && g.ctr != ctr) S.hdr[s].rng_ctr = g.ctr;
                }
            }
            if (lane == 0) a.action[s] = action;
        }
    }
}

void lobk_vec_act(hipStream_t st, bool dq, int n_cus, const DevParams* Pd, const DevState* Sd, const uint32_t* rnd, const VecActSrc& a) {
    const int need = (a.n + LOB_WAVES_PER_BLOCK - 1) / LOB_WAVES_PER_BLOCK;
    // the blocks a compute unit holds at once (four waves each: the kernel's waves per SIMD), so that no block waits for another's end
    int grid = n_cus * (!a.rows && dq ? 4 : 6);
    if (grid > LOB_VECACT_MAX_BLOCKS) grid = LOB_VECACT_MAX_BLOCKS;
    if (grid > need) grid = need;
    if (a.rows) hipLaunchKernelGGL((vec_act_kernel<false, false>), dim3(grid), dim3(LOB_BLOCK), 0, st, Pd, Sd, rnd, a);
    else if (dq) hipLaunchKernelGGL((vec_act_kernel<true, true>), dim3(grid), dim3(LOB_BLOCK), 0, st, Pd, Sd, rnd, a);
    else hipLaunchKernelGGL((vec_act_kernel<true, false>), dim3(grid), dim3(LOB_BLOCK), 0, st, Pd, Sd, rnd, a);
}
