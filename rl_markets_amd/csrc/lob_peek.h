// What the look-ahead family shares (lob_tu_vecpeek.hip vec_peek_kernel; lob_tu_vecroll.hip vec_rollout_kernel, 7k;
// lob_tu_branch.hip branch_*_kernel, 7l): the agent half of a step on a private copy of a book's state, once -- look_step_loads /
// look_step_run are env_kernel's step up to the event loop's status, peek_push and look_step_finish what follows a completed step,
// with step_epilogue's rm_apply (lob_env.h: it writes the two PnL windows, the only memory a step writes before env_store besides
// EnvCtx::err's flag) restated over registers -- and the kernels' common shape: one wave per block, 64 consecutive books of one plane,
// the rows out through LDS.  The kernels keep where the state lives and how the two windows are prepared.  Behind lob_kernels.h.
#ifndef LOB_PEEK_H
#define LOB_PEEK_H

#define LOB_LOOK_BLOCK 64   // one wave per block: 64 consecutive books of one plane (env_kernel<64, TM>'s shape)

// lob_get_terminal (lob_tu_vec.hip vec_terminal): 2 out of data, 1 outside the trading window, 0 live
__device__ __forceinline__ int lob_terminal(const DevParams& P, i32 done, i32 time_ms) { return done == 2 ? 2 : (is_open(P, time_ms) ? 0 : 1); }

// Plane-major geometry: block i is plane i / (Bpad / 64) -- an action, a plan, a branch -- over the books first_b ... first_b + 63
struct LookPlane { int plane, first_b, b; };
__device__ __forceinline__ LookPlane look_plane(int Bpad) {
    const int per_plane = Bpad / LOB_LOOK_BLOCK, plane = blockIdx.x / per_plane;
    const int first_b = (blockIdx.x - plane * per_plane) * LOB_LOOK_BLOCK;
    return {plane, first_b, first_b + (int)threadIdx.x};
}
// The block's staged rows ([64][V] in LDS) leave as consecutive words to each of the planes plane0 ... plane0 + n_planes - 1 of `obs`:
// they are contiguous in a plane (vec_rows_out, lob_tu_vec.hip).  Every thread of the block calls this (block barrier).
__device__ __forceinline__ void look_rows_out(const f32* stage, f32* obs, int plane0, int n_planes, int B, int first_b, int V) {
    __syncthreads();
    const int rows = B - first_b < LOB_LOOK_BLOCK ? B - first_b : LOB_LOOK_BLOCK;
    for (int n = plane0; n < plane0 + n_planes; n++) {
        f32* dst = obs + ((size_t)n * (size_t)B + (size_t)first_b) * (size_t)V;
        for (int i = threadIdx.x; i < rows * V; i += LOB_LOOK_BLOCK) dst[i] = stage[i];
    }
}
// slot 2 of S.vars, the observation of the book's last completed step, into the lane's stage row
__device__ __forceinline__ void look_obs_slot2(const DevState& S, int b, f32* row, int V) {
    const f32* vf = S.vars + ((size_t)b * 3 + 2) * 16;
    for (int i = 0; i < V; i++) row[i] = vf[i];
}
__device__ __forceinline__ RMReg rm_zero() { RMReg g; g.cnt = g.head = g.slot = 0; g.sum = g.mean = g.s = g.old = 0.0; return g; }

// rm_apply (lob_env.h) without its stores: the window's running state after the push of `val`, in registers only
__device__ inline void peek_rm_apply(const RMPtrs& r, RMReg& g, f64 val) {
    g.sum += val;
    if (g.cnt < r.w) {
        g.cnt++;
        f64 n = (f64)g.cnt;
        f64 old_mean = g.mean;
        g.mean += (val - g.mean) / n;
        g.s += (val - g.mean) * (val - old_mean);
    } else {
        f64 n = (f64)(g.cnt + 1);
        f64 old_mean = g.mean;
        g.mean += (val - g.mean) / n;
        g.s += (val - g.mean) * (val - old_mean);
        g.sum -= g.old;
        f64 n2 = (f64)g.cnt;
        f64 old_mean2 = g.mean;
        g.mean -= (g.old - g.mean) / n2;
        g.s -= (g.old - g.mean) * (g.old - old_mean2);
    }
    g.head = g.slot;
}
// rm_std over the registers
__device__ inline f64 peek_rm_std(const RMReg& g) {
    f64 v = g.s / (f64)(g.cnt - 1);
    return v > 0 ? sqrt(v) : 0.0;
}
// the two values a step pushes: the step's PnL split into its gain and its loss
__device__ inline f64 peek_push_up(const EnvR& e) { return 0.0 > e.pnl_step ? 0.0 : e.pnl_step; }
__device__ inline f64 peek_push_down(const EnvR& e) { return fabs(0.0 < e.pnl_step ? 0.0 : e.pnl_step); }
// step_epilogue's two rm_apply (lob_env.h) over `wu` / `wd`, which the caller has loaded and prepared (several steps deep: by its
// own account of the entry that is replaced)
__device__ inline void peek_push(const EnvCtx& c, const EnvR& e, RMReg& wu, RMReg& wd) {
    peek_rm_apply(c.S.pnl_ups, wu, peek_push_up(e));
    peek_rm_apply(c.S.pnl_downs, wd, peek_push_down(e));
}
// get_reward (lob_env.h) of the state behind the push and the episode totals: LOB_REWARD_NORMED reads the two windows, which here
// are `wu` / `wd` and not the engine's memory; every other measure reads the book's scalars only
__device__ inline f64 peek_reward(const EnvCtx& c, const EnvR& e, const RMReg& wu, const RMReg& wd) {
    if (c.P.reward_measure != LOB_REWARD_NORMED) return get_reward(c, e);
    const RMPtrs &u_ = c.S.pnl_ups, &d_ = c.S.pnl_downs;
    f64 r = 0.0;
    if (!(wu.cnt == u_.w && wd.cnt == d_.w)) r = 0.0;
    else {
        f64 u = wu.mean, d = wd.mean, su = peek_rm_std(wu), sd = peek_rm_std(wd);
        f64 numer = (u * sd - d * su), denom = (su + sd);
        if (isnan(numer) || isinf(numer)) numer = 0.0;
        if (isnan(denom) || isinf(denom)) denom = 0.0;
        r = (fabs(denom) < 1e-5) ? numer : (numer / denom);
    }
    return r * 100;
}

// The private step: env_kernel's (lob_kernels.h), from the loads at the cursor to the event loop's status.  What a step's launch reads
// of the previous one's env_store -- the track entry at cursor `k`, the row `rc` and, for the fast pass, the clamped next row -- is
// requested by look_step_loads, which needs only the two scalars: a caller may issue it before the rest of the state (vec_peek_kernel).
// (Plain `inline` throughout: forced inlining of these made the compiler leave EnvCtx's constructor out of line in the kernels of
// three trade slots -- a call, and the lane's state in scratch; profiles/lookahead_shared_resources.csv holds what to expect.)
struct LookLoads { TrackHead64 t0; RowFull cur, first; };
template <int TM>
__device__ inline void look_step_loads(const EnvCtx& c, int k, int rc, LookLoads& L) {
    L.t0 = c.track_head64(k);
    row_full_load(c, rc, L.cur);
    if (LOB_FAST_PASS && TM == 2) { const int last_row = c.n_ev() - 1; row_full_load(c, rc + 1 < last_row ? rc + 1 : last_row, L.first); }
}
// step_prologue, then event_loop_fast (two trade slots) or the step_event loop.  Returns the last pass's status: 1 the step is complete,
// 2 out of data (the mutated state is kept, done == 2).
template <int TM>
__device__ inline int look_step_run(const EnvCtx& c, EnvR& e, int action, StepAgg& g, const LookLoads& L) {
    step_prologue(c, e, action, g, L.cur);
    int st;
    if (LOB_FAST_PASS && TM == 2) {
        TrackHead64 t = L.t0;
        st = event_loop_fast(c, e, g, t, L.first);
    } else {
        TrackHead t;
        t.rec_first = L.t0.rec_first; t.rec_last = L.t0.rec_last; t.time_ms = L.t0.time_ms; t.tick_ap0 = L.t0.tick_ap0;
        t.tick_bp0 = L.t0.tick_bp0; t.info = L.t0.info; t.mid = L.t0.mid;
        do {
            const TrackHead tn = c.track_head(e.k + 1);
            st = step_event<TM>(c, e, g, t);
            t = tn;
        } while (st == 0);
    }
    return st;
}
// Behind a completed step (status != 2) the kernel sets `e.pnl_step = g.pnl` and does the two windows its own way, where
// step_epilogue has rm_load, rm_prep and rm_apply: it prepares them, pushes (peek_push) and stores what it keeps.  Then this: the rest
// of step_epilogue, the observation (V values) into the lane's row of the block's `stage` when `want_obs`, the step's reward.
// (A callable for the windows in the middle of one function measured 0.3 % slower in the roll-out than this form; peek and roll-out
// call this, branch_step_kernel writes the same lines out, where it measured faster: NOTES.md.)
__device__ inline f64 look_step_finish(const EnvCtx& c, EnvR& e, const StepAgg& g, const RMReg& wu, const RMReg& wd, bool want_obs, f32* stage, int V) {
    e.ep_reward += g.r;
    e.ep_bandh += g.mpm;
    if (want_obs) {
        const Track tk = state_track(c, e);
        for (int i = 0; i < V; i++) stage[threadIdx.x * V + i] = (f32)get_variable(c, e, c.P.vars[i], tk);
    }
    return peek_reward(c, e, wu, wd);
}

// ---- the private step over a RING track (include/lob_engine.h lob_look_ring / lob_track_window) ----
// The kernels' `RING` instantiations only; nothing above reads any of this.  A book's ring holds the entries [n_track - track_len,
// n_track).  The window the look-ahead serves is [lo, hi): hi = n_track, lo = n_track - track_len + LOB_TRACK_MARGIN floored at 0 -- the
// margin prepass_extend_kernel (lob_kernels.h) grants the real cursor, for the same reason: a step at cursor k reads the entries k - 1
// (the quotes, state_track) and k .. .  BEHIND: a private cursor < lo; the step is not attempted.  AHEAD: the event loop ended with
// status 2 while the pre-pass is not complete -- next_state's (lob_env.h) LOB_ERR_TRACK_UNDERRUN condition; the mutated state is dropped.
#define LOB_LOOK_AHEAD LOB_TERMINAL_AHEAD     // (include/lob_engine.h)
#define LOB_LOOK_BEHIND LOB_TERMINAL_BEHIND
struct LookWin { int lo, hi, complete; };
__device__ __forceinline__ LookWin look_window(const DevState& S, int b) {
    const BookMeta& M = S.meta[b];
    const int hi = M.n_track, lo = hi - S.track_len + LOB_TRACK_MARGIN;
    return {lo > 0 ? lo : 0, hi, M.complete};
}
// step_prologue takes BookMeta's two words from the context when it holds them: the look-ahead hands it the true n_track and
// complete = 1, so that next_state's out-of-data arm runs without raising LOB_ERR_TRACK_UNDERRUN in the ENGINE's error word -- that
// bit voids the real run.  Every other condition the step reports stays reported.  The kernel tells the two ends of a status 2 apart
// by LookWin::complete.  (An incomplete pre-pass has ex_first = ex_cur = ex_last = -1: that arm then reads no record.)
__device__ __forceinline__ void look_ring_ctx(EnvCtx& c, const LookWin& w) { c.pre_n_track = w.hi; c.pre_complete = 1; }
// The launch's cells of one kind, counted in the engine's word (lob_vec_status): every lane of the one-wave block calls this, outside
// any divergent region; one atomic per block that has such a cell, none otherwise (vec_actions_kernel, lob_tu_vec.hip).
__device__ __forceinline__ void look_count(u64* word, bool mine) {
    const unsigned long long m = __ballot(mine);
    if (m != 0 && threadIdx.x == 0) atomicAdd(word, (u64)__popcll(m));
}

#endif
