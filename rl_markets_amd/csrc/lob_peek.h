// The end of a step without its stores, shared by the two look-ahead units (lob_tu_vecpeek.hip vec_peek_kernel, DESIGN.md 7j;
// lob_tu_vecroll.hip vec_rollout_kernel): step_epilogue's rm_apply (lob_env.h) writes the two PnL windows, the only
// memory a step writes before env_store besides EnvCtx::err's flag -- restated here over registers.  Included behind lob_kernels.h.
#ifndef LOB_PEEK_H
#define LOB_PEEK_H

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
// what step_epilogue (lob_env.h) does behind `e.pnl_step = g.pnl` and the windows' rm_load + rm_prep, with the two windows kept in
// `wu` / `wd`: the caller has loaded and prepared them (several steps deep: by its own account of the entry that is replaced)
__device__ inline void peek_epilogue_apply(const EnvCtx& c, EnvR& e, const StepAgg& g, RMReg& wu, RMReg& wd) {
    peek_rm_apply(c.S.pnl_ups, wu, peek_push_up(e));
    peek_rm_apply(c.S.pnl_downs, wd, peek_push_down(e));
    e.ep_reward += g.r;
    e.ep_bandh += g.mpm;
}
// step_epilogue (lob_env.h) with the two windows kept in `wu` / `wd`
__device__ inline void peek_epilogue(const EnvCtx& c, EnvR& e, const StepAgg& g, RMReg& wu, RMReg& wd) {
    e.pnl_step = g.pnl;
    rm_load(c.S.pnl_ups, c.b, wu); rm_load(c.S.pnl_downs, c.b, wd);
    rm_prep(c.S.pnl_ups, c.S.B, c.b, wu); rm_prep(c.S.pnl_downs, c.S.B, c.b, wd);
    peek_epilogue_apply(c, e, g, wu, wd);
}
// get_reward (lob_env.h) of the state behind peek_epilogue: LOB_REWARD_NORMED reads the two windows, which here are `wu` / `wd` and
// not the engine's memory; every other measure reads the book's scalars only
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

#endif
