// Translation unit of the branch sets of the vector-env interface (include/lob_engine.h lob_branch_*; lob_launch.h BranchSrc;
// lob_branch.h the layout): branch_fork_kernel, branch_step_kernel, branch_select_kernel.  A unit of its own, so that
// every other unit is compiled from what it was.  gfx950 only; no CPU execution path.
//   A branch set is N private copies of every book's agent-side environment state that stay in device memory between launches: what
// vec_rollout_kernel (lob_tu_vecroll.hip) carries from step to step in an LDS slot and registers -- the EnvR, the two PnL windows --
// and the observation of the last completed step, stored behind every step and loaded in front of the next.  The market half is the
// track the pre-pass has written and the records, shared by all copies and constant within an episode.  Nothing of the engine's own
// state is written by any kernel here.
#define LOB_TU_SPLIT 1
#define LOB_TU_BRANCH 1
#include <hip/hip_runtime.h>

#include "lob_internal.h"
#include "lob_kernels.h"
#include "lob_peek.h"   // the family's shape and its private step

static constexpr BranchOff BR_OFF = branch_off();

// array of the set whose elements lie `per_lane` bytes per lane behind the base (a kernel argument: global_ loads and stores)
template <class T> __device__ __forceinline__ T* br_arr(const BranchSet& s, uint32_t per_lane) { return (T*)(s.base + s.lanes * (u64)per_lane); }

// env_load / env_store (lob_env.h) over the set: the same identity on LOB_ENV_FIELDS, with the lane in place of the book
__device__ inline void br_env_load(const BranchSet& s, size_t lane, EnvR& e) {
#define X(t, n) e.n = br_arr<t>(s, BR_OFF.n)[lane];
    LOB_ENV_FIELDS(X)
#undef X
}
__device__ inline void br_env_store(const BranchSet& s, size_t lane, const EnvR& e) {
#define X(t, n) br_arr<t>(s, BR_OFF.n)[lane] = e.n;
    LOB_ENV_FIELDS(X)
#undef X
}
// The set's window `which` (0 pnl_ups, 1 pnl_downs) as the RMPtrs that rm_load / rm_prep / rm_store (lob_env.h) take, with the lane
// for the book and the lanes for the row length of the ring; `w`: the window's length (the engine's RMPtrs::w)
__device__ inline RMPtrs br_window(const BranchSet& s, int which, i32 w) {
    RMPtrs r;
    const uint32_t o = BR_OFF.win[which];
    r.cnt = br_arr<i32>(s, o + LOB_BR_WIN_CNT); r.head = br_arr<i32>(s, o + LOB_BR_WIN_HEAD);
    r.sum = br_arr<f64>(s, o + LOB_BR_WIN_SUM); r.mean = br_arr<f64>(s, o + LOB_BR_WIN_MEAN); r.s = br_arr<f64>(s, o + LOB_BR_WIN_S);
    r.ring = br_arr<f64>(s, BR_OFF.fixed) + (which ? (size_t)s.w_up * s.lanes : 0);   // (not followed when the set holds no rings)
    r.w = w;
    return r;
}
__device__ __forceinline__ float4* br_obs(const BranchSet& s, size_t lane) { return reinterpret_cast<float4*>(br_arr<f32>(s, BR_OFF.obs) + lane * 16); }

// lob_branch_fork: one lane per book reads the book's present state once -- the LOB_ENV_FIELDS, the running state of the two windows,
// slot 2 of S.vars -- and writes it to the N lanes of the book, consecutive books to consecutive words on both sides; then the rings,
// entry by entry, when the set holds them.  Every load of a group is issued before its first store.  out (members may be null):
// plane n = the observation, lob_get_terminal's value, reward +0.0, stepped 0.
__global__ void __launch_bounds__(LOB_LOOK_BLOCK) branch_fork_kernel(const DevParams* __restrict__ Pp, DevState S, BranchSrc a) {
    const DevParams& P = *Pp;
    __shared__ f32 stage[LOB_LOOK_BLOCK * LOB_MAX_VARS];
    const int first_b = blockIdx.x * LOB_LOOK_BLOCK;
    const int b = first_b + threadIdx.x;
    const int B = a.B, V = P.V, N = a.n_branches;
    const BranchSet& set = a.set;
    const lob_branch_out& out = a.out;
    if (b < B) {
        EnvR e;
        env_load(S, b, e);
        RMReg wu, wd;
        rm_load(S.pnl_ups, b, wu); rm_load(S.pnl_downs, b, wd);
        const float4* vf = reinterpret_cast<const float4*>(S.vars + ((size_t)b * 3 + 2) * 16);
        const float4 v0 = vf[0], v1 = vf[1], v2 = vf[2], v3 = vf[3];
        const RMPtrs ru = br_window(set, 0, S.pnl_ups.w), rd = br_window(set, 1, S.pnl_downs.w);
        for (int n = 0; n < N; n++) {
            const size_t lane = (size_t)n * (size_t)a.Bpad + (size_t)b;
            br_env_store(set, lane, e);
            rm_store(ru, (int)lane, wu); rm_store(rd, (int)lane, wd);
            float4* o = br_obs(set, lane);
            o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3;
        }
        for (int k = 0; k < set.w_up; k++) {
            const f64 x = S.pnl_ups.ring[(size_t)k * B + b];
            for (int n = 0; n < N; n++) ru.ring[(size_t)k * set.lanes + (size_t)n * (size_t)a.Bpad + (size_t)b] = x;
        }
        for (int k = 0; k < set.w_dn; k++) {
            const f64 x = S.pnl_downs.ring[(size_t)k * B + b];
            for (int n = 0; n < N; n++) rd.ring[(size_t)k * set.lanes + (size_t)n * (size_t)a.Bpad + (size_t)b] = x;
        }
        const uint8_t term = (uint8_t)lob_terminal(P, e.done, e.time_ms);
        for (int n = 0; n < N; n++) {
            const size_t o = (size_t)n * (size_t)B + (size_t)b;
            if (out.reward) out.reward[o] = 0.0;
            if (out.terminal) out.terminal[o] = term;
            if (out.stepped) out.stepped[o] = 0;
        }
        if (out.obs) {
            const f32 v[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
#pragma unroll
            for (int i = 0; i < LOB_MAX_VARS; i++)
                if (i < V) stage[threadIdx.x * V + i] = v[i];
        }
    }
    if (out.obs) look_rows_out(stage, out.obs, 0, N, B, first_b, V);   // (uniform)
}

// lob_branch_select: one lane per (child, book), branch-major.  Child (n, b) becomes a copy of branch (parent[n][b], b) of the OTHER
// buffer `a.from` -- the set as it stood before the call --, a parent outside [0, N) meaning itself; the host swaps the buffers' roles.
// A gather between lanes of the same book: the loads of a wave are coalesced when its books share a parent, its stores always.  All
// loads of a group before its first store.  out (members may be null): obs and terminal of the new arrangement.
__global__ void __launch_bounds__(LOB_LOOK_BLOCK) branch_select_kernel(const DevParams* __restrict__ Pp, BranchSrc a) {
    const DevParams& P = *Pp;
    __shared__ f32 stage[LOB_LOOK_BLOCK * LOB_MAX_VARS];
    const LookPlane pl = look_plane(a.Bpad);
    const int n = pl.plane, b = pl.b;
    const int B = a.B, V = P.V;
    const BranchSet &dst = a.set, &src = a.from;
    const lob_branch_out& out = a.out;
    if (b < B) {
        i32 p = a.index[(size_t)n * (size_t)B + (size_t)b];
        if (p < 0 || p >= a.n_branches) p = n;
        const size_t from = (size_t)p * (size_t)a.Bpad + (size_t)b, to = (size_t)n * (size_t)a.Bpad + (size_t)b;
        const RMPtrs su = br_window(src, 0, src.w_up), sd = br_window(src, 1, src.w_dn);
        const RMPtrs du = br_window(dst, 0, dst.w_up), dd = br_window(dst, 1, dst.w_dn);
        EnvR e;
        br_env_load(src, from, e);
        RMReg wu, wd;
        rm_load(su, (int)from, wu); rm_load(sd, (int)from, wd);
        const float4* vf = br_obs(src, from);
        const float4 v0 = vf[0], v1 = vf[1], v2 = vf[2], v3 = vf[3];
        br_env_store(dst, to, e);
        rm_store(du, (int)to, wu); rm_store(dd, (int)to, wd);
        float4* o = br_obs(dst, to);
        o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3;
        const int w_min = src.w_up < src.w_dn ? src.w_up : src.w_dn;
        for (int k = 0; k < w_min; k++) {
            const f64 x = su.ring[(size_t)k * src.lanes + from], y = sd.ring[(size_t)k * src.lanes + from];
            du.ring[(size_t)k * dst.lanes + to] = x; dd.ring[(size_t)k * dst.lanes + to] = y;
        }
        for (int k = w_min; k < src.w_up; k++) du.ring[(size_t)k * dst.lanes + to] = su.ring[(size_t)k * src.lanes + from];
        for (int k = w_min; k < src.w_dn; k++) dd.ring[(size_t)k * dst.lanes + to] = sd.ring[(size_t)k * src.lanes + from];
        if (out.terminal) out.terminal[(size_t)n * (size_t)B + (size_t)b] = (uint8_t)lob_terminal(P, e.done, e.time_ms);
        if (out.obs) {
            const f32 v[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
#pragma unroll
            for (int i = 0; i < LOB_MAX_VARS; i++)
                if (i < V) stage[threadIdx.x * V + i] = v[i];
        }
    }
    if (out.obs) look_rows_out(stage, out.obs, n, 1, B, pl.first_b, V);   // (uniform)
}

// lob_branch_step: one lane per (branch, book), branch-major: block i is branch i / blocks_per_plane over the books
// 64 * (i % blocks_per_plane) ..., so every load and store of the set and actions[n * B + b] are consecutive words across the wave.
// The step up to the event loop's status is the family's (lob_peek.h look_step_loads / look_step_run), as in vec_rollout_kernel's
// loop, between a load and a store of the lane's state; what follows a completed step is written out below.  lob_vec_step's rules on the private state -- a branch steps when its lob_get_terminal is 0 and its action is one of the nine;
// otherwise, and when the step runs dry (the mutated state is kept, done == 2), the reward is +0.0 and the observation stays that of
// the last completed step.  The lane owns a full ring of each window when the reward reads them, so the plain rm_prep (lob_env.h)
// finds the entry a full window replaces, the lane's own pushes included.  Under every other reward nothing reads the windows: they
// stay as forked.  The state goes back only on lanes that stepped or ran dry; the epilogue runs over registers, so no store reaches
// the engine's windows.  EnvCtx keeps the real S and b: the track, the records, the meta.
//   RING (lob_look_ring on a ring track; lob_peek.h): a live branch whose cursor is below the window is BEHIND -- nothing
// is attempted, whatever its action, terminal LOB_LOOK_BEHIND --, a step that would run past the ring's last entry while the pre-pass is
// not complete is AHEAD -- terminal LOB_LOOK_AHEAD.  Either way the stored state is not written, so stepped 0, reward +0.0, obs as it
// was; the cells are counted in a.look_cnt[0] / [1], and nothing is raised in the engine's error word.
template <bool T2, bool RING>
__global__ void __launch_bounds__(LOB_LOOK_BLOCK) branch_step_kernel(const DevParams* __restrict__ Pp, DevState S, BranchSrc a) {
    const DevParams& P = *Pp;  // parameters read through the scalar cache, never copied to scratch
    constexpr int TM = T2 ? 2 : LOB_MAX_TRADES;
    __shared__ TickLds tick_lds;
    stage_ticks(P, tick_lds);
    __shared__ EnvSlot lds_env[LOB_LOOK_BLOCK];
    __shared__ f32 stage[LOB_LOOK_BLOCK * LOB_MAX_VARS];
    const LookPlane pl = look_plane(a.Bpad);
    const int n = pl.plane, b = pl.b;
    const int B = a.B, V = P.V;
    const BranchSet& set = a.set;
    const lob_branch_out& out = a.out;
    bool ahead = false, behind = false;
    if (b < B) {
        const size_t lane = (size_t)n * (size_t)a.Bpad + (size_t)b;
        const size_t o = (size_t)n * (size_t)B + (size_t)b;
        const int action = a.index[o];
        EnvCtx c(P, S, b, &tick_lds);
        LookWin w = {0, 0, 1};
        if constexpr (RING) { w = look_window(S, b); look_ring_ctx(c, w); }
        EnvR& e = lds_env[threadIdx.x].e;
        br_env_load(set, lane, e);
        f64 reward = 0.0;
        int stepped = 0;
        bool have_obs = false;
        const int term = lob_terminal(P, e.done, e.time_ms);
        if constexpr (RING) behind = term == 0 && e.k < w.lo;
        if (term == 0 && action >= 0 && action < LOB_N_ACTIONS && !(RING && behind)) {
            const bool win = P.reward_measure == LOB_REWARD_NORMED;   // (the set holds the rings exactly then: lob_branch_fork)
            const RMPtrs ru = br_window(set, 0, S.pnl_ups.w), rd = br_window(set, 1, S.pnl_downs.w);
            RMReg wu = rm_zero(), wd = wu;
            if (win) { rm_load(ru, (int)lane, wu); rm_load(rd, (int)lane, wd); }
            LookLoads L;
            look_step_loads<TM>(c, e.k, e.rec_cur, L);
            StepAgg g;
            const int st = look_step_run<TM>(c, e, action, g, L);
            if (st != 2) {
                // What follows is written out here and not through look_step_finish: with it this kernel measured 0.4 % slower than
                // before the step was shared.  The push and the episode totals stand in BOTH arms on purpose: written once behind the
                // `if`, the compiler spills 33 SGPRs for two trade slots against 31 (without the rings nothing reads the windows).
                e.pnl_step = g.pnl;
                if (win) {
                    rm_prep(ru, (int)set.lanes, (int)lane, wu); rm_prep(rd, (int)set.lanes, (int)lane, wd);
                    const int slot_u = wu.slot, slot_d = wd.slot;
                    peek_push(c, e, wu, wd); e.ep_reward += g.r; e.ep_bandh += g.mpm;
                    ru.ring[(size_t)slot_u * set.lanes + lane] = peek_push_up(e);    // rm_apply's two stores: the ring slot ...
                    rd.ring[(size_t)slot_d * set.lanes + lane] = peek_push_down(e);
                    rm_store(ru, (int)lane, wu); rm_store(rd, (int)lane, wd);        // ... and the running state
                } else {
                    peek_push(c, e, wu, wd); e.ep_reward += g.r; e.ep_bandh += g.mpm;
                }
                const Track tk = state_track(c, e);
                for (int i = 0; i < V; i++) stage[threadIdx.x * V + i] = (f32)get_variable(c, e, P.vars[i], tk);
                // ... and into the lane's row of the set as four 16-byte stores, read back from the lane's own LDS row
                f32 v[16];
#pragma unroll
                for (int i = 0; i < 16; i++) v[i] = i < V ? stage[threadIdx.x * V + i] : 0.0f;
                float4* ob = br_obs(set, lane);
                ob[0] = make_float4(v[0], v[1], v[2], v[3]); ob[1] = make_float4(v[4], v[5], v[6], v[7]);
                ob[2] = make_float4(v[8], v[9], v[10], v[11]); ob[3] = make_float4(v[12], v[13], v[14], v[15]);
                have_obs = true;
                reward = peek_reward(c, e, wu, wd);
                stepped = 1;
            }
            if (RING && st == 2 && !w.complete) ahead = true;   // (the branch stays where it was)
            else br_env_store(set, lane, e);   // stepped, or ran dry: the mutated state
        }
        if (!have_obs && out.obs) {
            const f32* vf = br_arr<f32>(set, BR_OFF.obs) + lane * 16;
            for (int i = 0; i < V; i++) stage[threadIdx.x * V + i] = vf[i];
        }
        if (out.reward) out.reward[o] = reward;
        if (out.terminal) out.terminal[o] = (uint8_t)((RING && ahead) ? LOB_LOOK_AHEAD : (RING && behind) ? LOB_LOOK_BEHIND : lob_terminal(P, e.done, e.time_ms));
        if (out.stepped) out.stepped[o] = stepped;
    }
    if (out.obs) look_rows_out(stage, out.obs, n, 1, B, pl.first_b, V);   // (uniform)
    if constexpr (RING) { look_count(a.look_cnt, ahead); look_count(a.look_cnt + 1, behind); }
}

void lobk_branch_fork(hipStream_t st, const DevParams* Pd, const DevState& S, const BranchSrc& a) {
    hipLaunchKernelGGL(branch_fork_kernel, dim3((unsigned)(a.Bpad / LOB_LOOK_BLOCK)), dim3(LOB_LOOK_BLOCK), 0, st, Pd, S, a);
}
void lobk_branch_select(hipStream_t st, const DevParams* Pd, const BranchSrc& a) {
    hipLaunchKernelGGL(branch_select_kernel, dim3((unsigned)(a.n_branches * (a.Bpad / LOB_LOOK_BLOCK))), dim3(LOB_LOOK_BLOCK), 0, st, Pd, a);
}
void lobk_branch_step(hipStream_t st, bool t2, bool ring, const DevParams* Pd, const DevState& S, const BranchSrc& a) {
    const dim3 grid((unsigned)(a.n_branches * (a.Bpad / LOB_LOOK_BLOCK))), block(LOB_LOOK_BLOCK);
    if (ring) {
        if (t2) hipLaunchKernelGGL((branch_step_kernel<true, true>), grid, block, 0, st, Pd, S, a);
        else hipLaunchKernelGGL((branch_step_kernel<false, true>), grid, block, 0, st, Pd, S, a);
    } else if (t2) hipLaunchKernelGGL((branch_step_kernel<true, false>), grid, block, 0, st, Pd, S, a);
    else hipLaunchKernelGGL((branch_step_kernel<false, false>), grid, block, 0, st, Pd, S, a);
}
