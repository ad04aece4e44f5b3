// Host side of the C ABI, the environment's half (include/lob_engine.h; lob_engine_impl.h): lob_step, the vector-env interface
// lob_vec_*, the branch sets lob_branch_* and the book snapshots lob_snapshot_*.  No kernel is compiled here: every launch goes through lob_launch.h (lob_vec_update's
// memo refresh through lob_engine.hip's launch_memo).  gfx950 only; no CPU execution path.
#define LOB_TU_SPLIT 1
#include "lob_engine_impl.h"

extern "C" {

int lob_step(lob_engine* e, const int32_t* host_actions) {
    LOB_GUARD(e, lob_step);
    if (!host_actions) { lob_set_error("lob_step: actions == NULL"); return LOB_EINVAL; }
    for (int b = 0; b < e->B; b++)
        if (host_actions[b] < 0 || host_actions[b] >= LOB_N_ACTIONS) { lob_set_error("lob_step: action out of range"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->actions_dev, host_actions, (size_t)e->B * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(e->S.mk_count, 0, 2 * sizeof(i32), e->stream));  // claims of this step go on a fresh list (nobody evaluates it)
    e->step_id++;
    e->hits_ok = false;
    {
        TimedLaunch t(e, "env_kernel");
        launch_env(e, e->stream, (const i32*)e->actions_dev, 0, 0, e->B, 0);
    }
    launch_step_log(e);
    maybe_refill_track(e);
    HIPCHK(hipGetLastError());
    return check_device_errors(e);
}

// ---- vector-env interface (include/lob_engine.h lob_vec_*; lob_tu_vec.hip) ----
static VecSrc vec_src(lob_engine* e) {
    VecSrc s;
    s.hdr = e->S.hdr; s.done = e->S.done; s.time_ms = e->S.time_ms; s.vars = e->S.vars;
    s.open_ms = e->P.open_ms; s.close_ms = e->P.close_ms; s.B = e->B; s.V = e->P.V;
    s.n_bad = e->vec_bad;
    return s;
}

// lob_step with the actions read, checked and armed on the device and the observation written there: four launches (five with the
// step log on) and two small memsets on the engine's stream, and the call returns.
int lob_vec_step(lob_engine* e, const int32_t* dev_actions, const lob_vec_out* out) {
    if (!e || !out || !dev_actions) { lob_set_error("lob_vec_step: NULL argument"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_vec_step);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemsetAsync(e->S.mk_count, 0, 2 * sizeof(i32), e->stream));  // claims of this step go on a fresh list (nobody evaluates it)
    if (out->n_live) HIPCHK(hipMemsetAsync(out->n_live, 0, sizeof(i32), e->stream));
    e->step_id++;
    e->hits_ok = false;
    const VecSrc s = vec_src(e);
    {
        TimedLaunch t(e, "vec_actions_kernel");
        lobk_vec_actions(e->stream, s, dev_actions);
    }
    {
        TimedLaunch t(e, "env_kernel");
        launch_env(e, e->stream, (const i32*)nullptr, 0, 0, e->B, 0);   // (no action array: go = h.stepped != 0, as armed above)
    }
    launch_step_log(e);
    {
        TimedLaunch t(e, "vec_observe_kernel");
        lobk_vec_observe(e->stream, false, true, s, (const DevParams*)e->P_dev, e->S, *out);
    }
    maybe_refill_track(e);
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

int lob_vec_observe(lob_engine* e, const lob_vec_out* out) {
    if (!e || !out) { lob_set_error("lob_vec_observe: NULL argument"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_vec_observe);
    HIPCHK(hipSetDevice(e->device));
    if (out->n_live) HIPCHK(hipMemsetAsync(out->n_live, 0, sizeof(i32), e->stream));
    {
        TimedLaunch t(e, "vec_observe_derive_kernel", nullptr, true);
        lobk_vec_observe(e->stream, true, false, vec_src(e), (const DevParams*)e->P_dev, e->S, *out);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

int lob_vec_status(lob_engine* e, int64_t* n_bad_actions) {
    if (!e) { lob_set_error("lob_vec_status: NULL engine"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    i32 flag = 0;
    u64 words[3] = {0, 0, 0};   // actions out of range; the look-aheads' ahead and behind cells (lob_look_counts)
    HIPCHK(hipMemcpyAsync(&flag, e->S.error_flag, sizeof flag, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(words, e->vec_bad, sizeof words, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemsetAsync(e->vec_bad, 0, sizeof words, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const u64 bad = words[0];
    e->look_ahead_seen = (int64_t)words[1];
    e->look_behind_seen = (int64_t)words[2];
    if (n_bad_actions) *n_bad_actions = (int64_t)bad;
    if (flag) return device_error_rc(flag);
    if (bad) { lob_set_error("lob_vec_step: " + std::to_string(bad) + " action(s) out of range since the last lob_vec_status; those books were not stepped"); return LOB_EINVAL; }
    return LOB_OK;
}

// ---- look-aheads on a ring track (include/lob_engine.h lob_look_ring) ----
static_assert(LOB_TRACK_WINDOW_MARGIN == LOB_TRACK_MARGIN, "the header states the margin of prepass_extend_kernel");

// A host flag: guard() lets the NO_RING calls through on a chunked engine while it is set.  Survives lob_reset.
int lob_look_ring(lob_engine* e, int on) {
    if (!e) { lob_set_error("lob_look_ring: NULL engine"); return LOB_EINVAL; }
    if (e->half_open) { lob_set_error("lob_look_ring: a learner step is half done (lob_td_step_begin without lob_td_step_end)"); return LOB_ESTATE; }
    e->look_ring = on != 0;
    return LOB_OK;
}

// The window of every book's track, from BookMeta as it stands behind everything enqueued so far: waits for the stream.
int lob_track_window(lob_engine* e, int32_t* lo, int32_t* hi, int32_t* complete) {
    if (!e || !lo || !hi || !complete) { lob_set_error("lob_track_window: NULL argument"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_track_window);
    HIPCHK(hipSetDevice(e->device));
    std::vector<BookMeta> meta((size_t)e->B);
    HIPCHK(hipMemcpyAsync(meta.data(), e->S.meta, (size_t)e->B * sizeof(BookMeta), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int b = 0; b < e->B; b++) {
        const int n = meta[(size_t)b].n_track, first = e->chunked ? n - e->S.track_len + LOB_TRACK_MARGIN : 0;
        lo[b] = first > 0 ? first : 0;
        hi[b] = n;
        complete[b] = meta[(size_t)b].complete;
    }
    return LOB_OK;
}

// (a diagnostic export, beside lob_debug_launches: the real books' cursors in the units of the window -- events, where lob_get_books
// reports records -- into a host array [B]; waits for the stream)
int lob_debug_track_cursor(lob_engine* e, int32_t* k) {
    if (!e || !k) { lob_set_error("lob_debug_track_cursor: NULL argument"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_track_window);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(k, e->S.k, (size_t)e->B * sizeof(i32), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}

// What the last lob_vec_status read of the two cell counts (host words: nothing is waited for here)
int lob_look_counts(lob_engine* e, int64_t* n_ahead, int64_t* n_behind) {
    if (!e) { lob_set_error("lob_look_counts: NULL engine"); return LOB_EINVAL; }
    if (n_ahead) *n_ahead = e->look_ahead_seen;
    if (n_behind) *n_behind = e->look_behind_seen;
    return LOB_OK;
}

// `ring` of the look-ahead launches: the instantiation with the two window checks runs exactly where they can say anything
static bool look_on_ring(const lob_engine* e) { return e->chunked && e->look_ring; }

// The order book and the agent's own words of every book into the caller's device buffers (lob_tu_vecbook.hip vec_book_kernel): one
// launch on the engine's stream, nothing read back, nothing changed.
int lob_vec_book(lob_engine* e, const lob_vec_book_out* out) {
    if (!e || !out) { lob_set_error("lob_vec_book: NULL argument"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_vec_book);
    if (!out->levels && !out->own && !out->time_ms) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    VecBookSrc s;
    s.records = e->S.records; s.rec_phase = e->S.rec_phase; s.rec_cur = e->S.rec_cur;
    s.n_events = e->S.n_events; s.Wd = e->P.Wd; s.D = e->P.D;
    s.w_ask_px = drec_ask_px(e->P.D, e->P.T); s.w_ask_vol = drec_ask_vol(e->P.D, e->P.T);
    s.w_bid_px = drec_bid_px(e->P.D, e->P.T); s.w_bid_vol = drec_bid_vol(e->P.D, e->P.T);
    s.position = e->S.position;
    s.a_osz = e->S.a_osz; s.a_oex = e->S.a_oex; s.a_oqh = e->S.a_oqh; s.b_osz = e->S.b_osz; s.b_oex = e->S.b_oex; s.b_oqh = e->S.b_oqh;
    s.a_on = e->S.a_on; s.b_on = e->S.b_on; s.last_action = e->S.last_action; s.total_ticks = e->S.total_ticks; s.time_ms = e->S.time_ms;
    s.a_opx = e->S.a_opx; s.b_opx = e->S.b_opx; s.ask_quote = e->S.ask_quote; s.bid_quote = e->S.bid_quote;
    s.pnl_step = e->S.pnl_step; s.ep_pnl = e->S.ep_pnl; s.ep_reward = e->S.ep_reward;
    s.B = e->B;
    {
        TimedLaunch t(e, "vec_book_kernel", nullptr, true);
        lobk_vec_book(e->stream, s, *out);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

// The last K event records of every book into the caller's device buffers (lob_tu_vechist.hip vec_hist_kernel): one launch on the
// engine's stream, nothing read back, nothing changed.  e->S.records as it is now: a stream handed over by lob_stage_events is followed.
int lob_vec_history(lob_engine* e, int32_t K, const lob_vec_hist_out* out) {
    if (!e || !out) { lob_set_error("lob_vec_history: NULL argument"); return LOB_EINVAL; }
    if (K < 1 || K > LOB_MAX_HISTORY) { lob_set_error("lob_vec_history: K = " + std::to_string(K) + " is outside [1, " + std::to_string(LOB_MAX_HISTORY) + "]"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_vec_history);
    if (!out->levels && !out->trades && !out->time_ms && !out->n_valid && !out->rec) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    VecHistSrc s;
    s.records = e->S.records; s.rec_phase = e->S.rec_phase; s.rec_cur = e->S.rec_cur; s.rec_len = e->S.rec_len;
    s.n_events = e->S.n_events; s.Wd = e->P.Wd; s.D = e->P.D; s.T = e->P.T; s.B = e->B;
    s.w_ask_px = drec_ask_px(e->P.D, e->P.T); s.w_ask_vol = drec_ask_vol(e->P.D, e->P.T);
    s.w_bid_px = drec_bid_px(e->P.D, e->P.T); s.w_bid_vol = drec_bid_vol(e->P.D, e->P.T); s.w_trades = drec_trades(e->P.D, e->P.T);
    {
        TimedLaunch t(e, "vec_hist_kernel", nullptr, true);
        lobk_vec_history(e->stream, s, K, *out);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

// The engine's own Q values and policy actions for every book, into the caller's device buffers (lob_tu_vecact.hip vec_act_kernel;
// DESIGN.md 7h): one launch on the engine's stream, nothing read back.  The kernel reads the state through its device-resident copy,
// which the first lob_reset has uploaded (sync_state); every array it follows from there is allocated by lob_create and stays.
// Not refused after lob_snapshot_restore: it reads the books' latest getState(), which the restore put back, and nothing of the
// learner's memory of the last transition.
int lob_vec_act(lob_engine* e, int32_t mode, const lob_vec_act_out* out) {
    if (!e || !out) { lob_set_error("lob_vec_act: NULL argument"); return LOB_EINVAL; }
    if (mode < LOB_ACT_GREEDY || mode > LOB_ACT_ARGMAX) { lob_set_error("lob_vec_act: mode " + std::to_string(mode) + " is none of LOB_ACT_GREEDY, LOB_ACT_BEHAVIOUR, LOB_ACT_ARGMAX"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_vec_act);
    if (!out->action && !out->q) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    VecActSrc a;
    a.rows = nullptr; a.theta = nullptr; a.nz = nullptr;
    a.n = e->B; a.mode = mode;
    a.action = out->action; a.q = out->q;
    {
        TimedLaunch t(e, "vec_act_kernel", nullptr, true);
        lobk_vec_act(e->stream, e->P.algo == LOB_ALGO_DOUBLE_Q, e->n_cus, LOB_PS(e), (const uint32_t*)e->rnd_dev, a);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

// What lob_vec_step would write under each action of the mask, into the caller's device buffers (lob_tu_vecpeek.hip vec_peek_kernel;
// DESIGN.md 7j): one launch on the engine's stream, nothing read back, nothing of the engine's state changed -- no step number, no
// memo list, no step-log row, no refill of the track.  Not refused after lob_snapshot_restore: it reads the environment only.
// Refused on a ring track unless lob_look_ring is on; then the refill that would fall due within the look-ahead's one step is made
// first (look_refill_track) and the kernel's ring instantiation runs.
int lob_vec_peek(lob_engine* e, uint32_t action_mask, const lob_vec_peek_out* out) {
    if (!e || !out) { lob_set_error("lob_vec_peek: NULL argument"); return LOB_EINVAL; }
    if (action_mask == 0 || (action_mask & ~(uint32_t)LOB_PEEK_ALL)) {
        lob_set_error("lob_vec_peek: action_mask " + std::to_string(action_mask) + " is empty or has a bit at or above LOB_N_ACTIONS"); return LOB_EINVAL;
    }
    LOB_GUARD(e, lob_vec_peek);
    if (!out->obs && !out->reward && !out->terminal && !out->stepped) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    PeekSrc a;
    a.B = e->B; a.Bpad = (e->B + 63) / 64 * 64;
    a.n_act = 0;
    for (int k = 0; k < 12; k++) a.act[k] = 0;
    for (int k = 0; k < LOB_N_ACTIONS; k++)
        if (action_mask >> k & 1u) a.act[a.n_act++] = (uint8_t)k;
    a.out = *out;
    a.look_cnt = e->vec_bad + 1;
    look_refill_track(e, 1);
    {
        TimedLaunch t(e, "vec_peek_kernel", nullptr, true);
        lobk_vec_peek(e->stream, e->P.T <= 2, look_on_ring(e), (const DevParams*)e->P_dev, e->S, a);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

// What `horizon` consecutive lob_vec_step calls would write under each of `n_plans` plans, into the caller's device buffers
// (lob_tu_vecroll.hip vec_rollout_kernel): one launch on the engine's stream, nothing read back, nothing of the engine's
// state changed.  Allowed and refused where lob_vec_peek is.  The one allocation: the workspace of the PnL windows' entries the plans
// themselves push, needed when the reward reads the windows (LOB_REWARD_NORMED) and 1 < lb_pnl < horizon -- 2 * lb_pnl * n_plans *
// Bpad doubles, made by the first call that needs it and grown (hipFree + hipMalloc: both synchronise the device) only by a call
// that needs more than any before it.
int lob_vec_rollout(lob_engine* e, const int32_t* dev_actions, int n_plans, int horizon, double gamma, const lob_vec_rollout_out* out) {
    if (!e || !out || !dev_actions) { lob_set_error("lob_vec_rollout: NULL argument"); return LOB_EINVAL; }
    if (n_plans < 1 || n_plans > LOB_MAX_ROLLOUT_PLANS) {
        lob_set_error("lob_vec_rollout: n_plans = " + std::to_string(n_plans) + " is outside [1, " + std::to_string(LOB_MAX_ROLLOUT_PLANS) + "]"); return LOB_EINVAL;
    }
    if (horizon < 1 || horizon > LOB_MAX_ROLLOUT_STEPS) {
        lob_set_error("lob_vec_rollout: horizon = " + std::to_string(horizon) + " is outside [1, " + std::to_string(LOB_MAX_ROLLOUT_STEPS) + "]"); return LOB_EINVAL;
    }
    if (!(gamma >= 0.0 && gamma <= 1.0)) { lob_set_error("lob_vec_rollout: gamma = " + std::to_string(gamma) + " is outside [0, 1]"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_vec_rollout);
    if (!out->obs && !out->reward && !out->terminal && !out->stepped && !out->ret) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    RolloutSrc a;
    a.actions = dev_actions;
    a.B = e->B; a.Bpad = (e->B + 63) / 64 * 64;
    a.n_plans = n_plans; a.horizon = horizon;
    a.gamma = gamma;
    a.shadow = nullptr;
    a.out = *out;
    const int w = e->S.pnl_ups.w;
    if (e->P.reward_measure == LOB_REWARD_NORMED && w > 1 && w < horizon) {
        const size_t need = 2 * (size_t)w * (size_t)n_plans * (size_t)a.Bpad;
        if (e->roll_ws.reserve(need)) {
            lob_set_error("lob_vec_rollout: no room for the PnL windows' workspace (" + std::to_string(need * sizeof(f64)) + " bytes; fewer plans or a shorter horizon per call)");
            return LOB_ENOMEM;
        }
        a.shadow = e->roll_ws.p;
    }
    a.look_cnt = e->vec_bad + 1;
    look_refill_track(e, horizon);
    {
        TimedLaunch t(e, "vec_rollout_kernel", nullptr, true);
        lobk_vec_rollout(e->stream, e->P.T <= 2, look_on_ring(e), (const DevParams*)e->P_dev, e->S, a);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

// ---- branch sets (include/lob_engine.h lob_branch_*; lob_tu_branch.hip; lob_branch.h) ----
// The set's shape follows from the engine alone: the books, the branches, and the rings of the two PnL windows when the reward reads
// them (LOB_REWARD_NORMED) -- nothing else ever looks at a branch's ring.
static BranchSrc branch_src(lob_engine* e, int n_branches, int buf) {
    const bool win = e->P.reward_measure == LOB_REWARD_NORMED;
    BranchSrc a;
    memset(&a, 0, sizeof a);
    a.set.base = e->branch_buf[buf].p; a.set.lanes = (u64)branch_lanes(e->B, n_branches);
    a.set.w_up = win ? e->S.pnl_ups.w : 0; a.set.w_dn = win ? e->S.pnl_downs.w : 0;
    a.from = a.set; a.from.base = e->branch_buf[buf ^ 1].p;
    a.B = e->B; a.Bpad = (e->B + 63) / 64 * 64;
    a.n_branches = n_branches;
    return a;
}
// room for a set of n_branches in buffer `buf` (a buffer that must grow is released and allocated: both synchronise the device)
static int branch_reserve(lob_engine* e, const char* who, int n_branches, int buf) {
    const BranchSrc a = branch_src(e, n_branches, buf);
    if (a.set.lanes > (u64)INT32_MAX || e->branch_buf[buf].reserve(branch_bytes(e->B, n_branches, a.set.w_up, a.set.w_dn))) {
        lob_set_error(branch_enomem_message(who, e->B, n_branches, a.set.w_up, a.set.w_dn));
        return LOB_ENOMEM;
    }
    return LOB_OK;
}
static int branch_live_ok(lob_engine* e, const char* who) {
    if (e->branch_live && e->branch_buf[e->branch_cur].p) return LOB_OK;
    lob_set_error(std::string(who) + ": no live branch set (lob_branch_fork makes one; lob_reset and lob_branch_close void it)");
    return LOB_ESTATE;
}

// Every branch becomes a copy of its book's present state (branch_fork_kernel): one launch on the engine's stream, nothing read back,
// nothing of the engine's state changed.  Allowed and refused where lob_vec_rollout is.
int lob_branch_fork(lob_engine* e, int n_branches, const lob_branch_out* out) {
    if (!e) { lob_set_error("lob_branch_fork: NULL engine"); return LOB_EINVAL; }
    if (n_branches < 1 || n_branches > LOB_MAX_BRANCHES) {
        lob_set_error("lob_branch_fork: n_branches = " + std::to_string(n_branches) + " is outside [1, " + std::to_string(LOB_MAX_BRANCHES) + "]"); return LOB_EINVAL;
    }
    LOB_GUARD(e, lob_branch_fork);
    HIPCHK(hipSetDevice(e->device));
    e->branch_live = false;   // (a growth that fails leaves no set behind)
    const int rc = branch_reserve(e, "lob_branch_fork", n_branches, e->branch_cur);
    if (rc) return rc;
    BranchSrc a = branch_src(e, n_branches, e->branch_cur);
    if (out) a.out = *out;
    look_refill_track(e, 1);
    {
        TimedLaunch t(e, "branch_fork_kernel", nullptr, true);
        lobk_branch_fork(e->stream, (const DevParams*)e->P_dev, e->S, a);
    }
    HIPCHK(hipGetLastError());
    e->branch_n = n_branches;
    e->branch_live = true;
    e->branch_fork_real = e->real_steps;   // the set's lead over the real books starts at 0
    e->branch_steps = 0;
    return LOB_OK;
}

// One lob_vec_step of every branch on its private state (branch_step_kernel): one launch on the engine's stream.
int lob_branch_step(lob_engine* e, const int32_t* dev_actions, const lob_branch_out* out) {
    if (!e || !out || !dev_actions) { lob_set_error("lob_branch_step: NULL argument"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_branch_step);
    int rc = branch_live_ok(e, "lob_branch_step");
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    BranchSrc a = branch_src(e, e->branch_n, e->branch_cur);
    a.index = dev_actions;
    a.out = *out;
    a.look_cnt = e->vec_bad + 1;
    {
        // the set's lead: its steps since the fork less the real books' since then; the step reaches one further
        const long long lead = e->branch_steps - (e->real_steps - e->branch_fork_real);
        look_refill_track(e, 1 + (lead > 0 ? lead : 0));
    }
    e->branch_steps++;
    {
        TimedLaunch t(e, "branch_step_kernel", nullptr, true);
        lobk_branch_step(e->stream, e->P.T <= 2, look_on_ring(e), (const DevParams*)e->P_dev, e->S, a);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

// The set rearranged within every book (branch_select_kernel): a gather from the live buffer into the other one, which then is the
// live one.  One launch on the engine's stream.
int lob_branch_select(lob_engine* e, const int32_t* dev_parent, const lob_branch_out* out) {
    if (!e || !dev_parent) { lob_set_error("lob_branch_select: NULL argument"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_branch_select);
    int rc = branch_live_ok(e, "lob_branch_select");
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    const int to = e->branch_cur ^ 1;
    if ((rc = branch_reserve(e, "lob_branch_select", e->branch_n, to))) return rc;   // (the live set stays as it is)
    BranchSrc a = branch_src(e, e->branch_n, to);
    a.index = dev_parent;
    if (out) { a.out.obs = out->obs; a.out.terminal = out->terminal; }
    {
        TimedLaunch t(e, "branch_select_kernel", nullptr, true);
        lobk_branch_select(e->stream, (const DevParams*)e->P_dev, a);
    }
    HIPCHK(hipGetLastError());
    e->branch_cur = to;
    return LOB_OK;
}

// ---- the book and the event window of every branch (include/lob_engine.h lob_branch_book / lob_branch_history; lob_tu_branchobs.hip;
// DESIGN.md 7m) ----
// What the two kernels read: the buffer e->branch_cur designates -- lob_branch_select flips it -- and of the engine what lob_vec_book /
// lob_vec_history read, e->S.records as it is now.
static BranchObsSrc branch_obs_src(lob_engine* e) {
    const BranchSrc a = branch_src(e, e->branch_n, e->branch_cur);
    BranchObsSrc s;
    memset(&s, 0, sizeof s);
    s.set = a.set;
    s.records = e->S.records; s.rec_phase = e->S.rec_phase; s.rec_len = e->S.rec_len;
    s.n_events = e->S.n_events; s.Wd = e->P.Wd; s.D = e->P.D; s.T = e->P.T;
    s.w_ask_px = drec_ask_px(e->P.D, e->P.T); s.w_ask_vol = drec_ask_vol(e->P.D, e->P.T);
    s.w_bid_px = drec_bid_px(e->P.D, e->P.T); s.w_bid_vol = drec_bid_vol(e->P.D, e->P.T); s.w_trades = drec_trades(e->P.D, e->P.T);
    s.B = a.B; s.Bpad = a.Bpad; s.n_branches = a.n_branches;
    return s;
}

// lob_vec_book of every branch (branch_book_kernel): one launch on the engine's stream, nothing read back, nothing of the engine or of
// the set changed.
int lob_branch_book(lob_engine* e, const lob_vec_book_out* out) {
    if (!e || !out) { lob_set_error("lob_branch_book: NULL argument"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_branch_book);
    const int rc = branch_live_ok(e, "lob_branch_book");
    if (rc) return rc;
    if (!out->levels && !out->own && !out->time_ms) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    {
        TimedLaunch t(e, "branch_book_kernel", nullptr, true);
        lobk_branch_book(e->stream, branch_obs_src(e), *out);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

// lob_vec_history(K) of every branch (branch_hist_kernel): one launch on the engine's stream, nothing read back, nothing of the engine
// or of the set changed.
int lob_branch_history(lob_engine* e, int32_t K, const lob_vec_hist_out* out) {
    if (!e || !out) { lob_set_error("lob_branch_history: NULL argument"); return LOB_EINVAL; }
    if (K < 1 || K > LOB_MAX_HISTORY) { lob_set_error("lob_branch_history: K = " + std::to_string(K) + " is outside [1, " + std::to_string(LOB_MAX_HISTORY) + "]"); return LOB_EINVAL; }
    LOB_GUARD(e, lob_branch_history);
    const int rc = branch_live_ok(e, "lob_branch_history");
    if (rc) return rc;
    if (!out->levels && !out->trades && !out->time_ms && !out->n_valid && !out->rec) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    {
        TimedLaunch t(e, "branch_hist_kernel", nullptr, true);
        lobk_branch_history(e->stream, branch_obs_src(e), K, *out);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

int lob_branch_close(lob_engine* e) {
    if (!e) { lob_set_error("lob_branch_close: NULL engine"); return LOB_EINVAL; }
    e->branch_live = false;
    if (!e->branch_buf[0].p && !e->branch_buf[1].p) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));   // (a launch still queued uses the buffers)
    for (auto& b : e->branch_buf) b.release();
    return LOB_OK;
}

// lob_q_values with both ends in device memory: the same kernel over the caller's rows, under theta (book 0's under private theta).
int lob_vec_q(lob_engine* e, const float* dev_vars, int32_t n, double* dev_q) {
    if (!e || !dev_vars || !dev_q || n < 1) { lob_set_error("lob_vec_q: bad argument"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    VecActSrc a;
    a.rows = dev_vars; a.theta = (const f64*)e->S.theta; a.nz = (const uint32_t*)e->S.theta_nz;
    a.n = n; a.mode = LOB_ACT_ARGMAX;
    a.action = nullptr; a.q = dev_q;
    {
        TimedLaunch t(e, "vec_q_kernel", nullptr, true);
        lobk_vec_act(e->stream, false, e->n_cus, LOB_PS(e), (const uint32_t*)e->rnd_dev, a);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

// ---- tile features and external weight updates (include/lob_engine.h lob_vec_features / lob_vec_update; lob_tu_vecfeat.hip) ----
int lob_vec_terms(lob_engine* e, int32_t host_out[27]) {
    if (!e || !host_out) { lob_set_error("lob_vec_terms: NULL argument"); return LOB_EINVAL; }
    for (int i = 0; i < 27; i++) host_out[i] = (int32_t)e->vec_terms[i];   // (< M <= 2^31 - 1)
    return LOB_OK;
}
// The argument checks the two device calls share -- the rows' rule of lob_vec_act / lob_vec_q -- and their guard: the books' own rows
// exist after a lob_reset only
static int vec_feat_entry(lob_engine* e, const float* dev_vars, int32_t n, const char* who, unsigned needs) {
    if (!e) { lob_set_error(std::string(who) + ": NULL engine"); return LOB_EINVAL; }
    if (n < 1) { lob_set_error(std::string(who) + ": n = " + std::to_string(n) + " (at least one row)"); return LOB_EINVAL; }
    if (!dev_vars && n != e->B) { lob_set_error(std::string(who) + ": n = " + std::to_string(n) + " but dev_vars == NULL means the engine's " + std::to_string(e->B) + " books"); return LOB_EINVAL; }
    const int rc = guard(e, who, needs);
    if (rc) return rc;
    return dev_vars ? LOB_OK : guard(e, who, RESET);
}
// The hash sums / tile indices of n states into the caller's device buffers: one launch on the engine's stream, nothing changed.
int lob_vec_features(lob_engine* e, const float* dev_vars, int32_t n, const int32_t* dev_actions, const lob_vec_feat_out* out) {
    if (e && !out) { lob_set_error("lob_vec_features: NULL out"); return LOB_EINVAL; }
    if (e && out->idx && !dev_actions) { lob_set_error("lob_vec_features: idx wanted without dev_actions"); return LOB_EINVAL; }
    int rc = vec_feat_entry(e, dev_vars, n, "lob_vec_features", needs::lob_vec_features);
    if (rc) return rc;
    if (!out->sums && !out->idx) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    VecFeatSrc a;
    memset(&a, 0, sizeof a);
    a.rows = dev_vars; a.actions = out->idx ? dev_actions : nullptr; a.n = n;
    a.sums = out->sums; a.idx = out->idx;
    {
        TimedLaunch t(e, "vec_features_kernel", nullptr, true);
        lobk_vec_feat(e->stream, e->n_cus, LOB_PS(e), (const uint32_t*)e->rnd_dev, a);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}
// theta[tile] += step over the tiles of (row, action), from outside a step.  On the device the kernel keeps the maps as
// delta_apply_kernel does; here the host does what lob_theta_set does around its kernels -- except for the multi-GPU base, which
// stays: the update is a local change and the next exchange carries it.
int lob_vec_update(lob_engine* e, const float* dev_vars, int32_t n, const int32_t* dev_actions, const double* dev_step, int32_t second) {
    if (e && (!dev_actions || !dev_step)) { lob_set_error("lob_vec_update: NULL argument"); return LOB_EINVAL; }
    if (e && second != 0 && second != 1) { lob_set_error("lob_vec_update: second = " + std::to_string(second) + " is neither 0 nor 1"); return LOB_EINVAL; }
    if (e && second && e->P.algo != LOB_ALGO_DOUBLE_Q) { lob_set_error("lob_vec_update: second = 1 needs LOB_ALGO_DOUBLE_Q (there is no theta_b)"); return LOB_EINVAL; }
    int rc = vec_feat_entry(e, dev_vars, n, "lob_vec_update", needs::lob_vec_update);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    VecFeatSrc a;
    memset(&a, 0, sizeof a);
    a.rows = dev_vars; a.actions = dev_actions; a.n = n; a.step = dev_step;
    a.theta = second ? e->S.theta_b : e->S.theta;
    a.nz = second ? e->S.theta_b_nz : e->S.theta_nz;
    if (e->P.memo) {   // (double Q: one set of maps for both vectors)
        a.nzx = e->S.theta_nzx; a.nzc = e->S.theta_nzc; a.nzd = e->S.theta_nzd; a.nzm = e->S.theta_nzm; a.nzd_terms = e->S.nzd_terms;
        a.cshift = e->P.cshift;
    }
    a.nz_epoch = e->S.nz_epoch;
    a.tag = e->vec_upd_tag;
    a.launch = e->vec_upd_launch = e->vec_upd_launch == INT32_MAX ? 1 : e->vec_upd_launch + 1;
    a.n_bad = e->vec_bad;
    e->theta_ver++;  // memo records computed under the old weights are void
    e->hits_ok = false;
    e->hint_step = 0;  // (... and so is what the learn kernels handed back under them)
    e->rest_recent = 0;
    {
        TimedLaunch t(e, "vec_update_kernel", nullptr, true);
        lobk_vec_feat(e->stream, e->n_cus, LOB_PS(e), (const uint32_t*)e->rnd_dev, a);
    }
    if (e->P.memo && e->was_reset) launch_memo(e, e->last_par, 1);  // the current triples under the new weights: the next act stays on the fast path
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

// ---- book snapshots (include/lob_engine.h lob_snapshot_*; lob_tu_snapshot.hip) ----
// The descriptor table of the arrays a snapshot holds and their places in a slot buffer, built once per engine with the first save:
// every array of LOB_ENV_FIELDS, the rolling means pnl_ups / pnl_downs, then the per-book records (LHdr's five environment words,
// slot 2 of vars).  Arrays at multiples of 16 bytes, in the live layout.
static int snap_prepare(lob_engine* e) {
    if (e->snap_tab) return LOB_OK;
    const size_t B = (size_t)e->B;
    std::vector<SnapRow> r4, r8;
    std::vector<SnapArr> arrs;
    size_t off = 0, max_bytes = 0;
    auto add = [&](void* live, size_t width, size_t rows) {
        const size_t bytes = rows * B * width;
        arrs.push_back(SnapArr{live, (u64)off, (u64)bytes, 0});
        for (size_t r = 0; r < rows; r++) (width == 4 ? r4 : r8).push_back(SnapRow{(char*)live + r * B * width, (u64)(off + r * B * width)});
        max_bytes = std::max(max_bytes, bytes);
        off = (off + bytes + 15) & ~(size_t)15;
    };
#define X(t, n) static_assert(sizeof(t) == 4 || sizeof(t) == 8, "two element widths"); add(e->S.n.p, sizeof(t), 1);
    LOB_ENV_FIELDS(X)
#undef X
    for (const RMPtrs* m : {&e->S.pnl_ups, &e->S.pnl_downs}) {
        add(m->ring.p, 8, (size_t)m->w); add(m->cnt.p, 4, 1); add(m->head.p, 4, 1); add(m->sum.p, 8, 1); add(m->mean.p, 8, 1); add(m->s.p, 8, 1);
    }
    SnapArgs& a = e->snap_args;
    a.off_hdr = off; off = (off + 4 * B * 4 + 15) & ~(size_t)15;
    a.off_reward = off; off = (off + B * 8 + 15) & ~(size_t)15;
    a.off_vars = off; off += B * 64;
    a.n4 = (i32)r4.size(); a.n8 = (i32)r8.size(); a.n_arr = (i32)arrs.size(); a.B = e->B;
    a.max_bytes = max_bytes;
    a.hdr = e->S.hdr.p; a.vars = e->S.vars.p;
    r4.insert(r4.end(), r8.begin(), r8.end());
    const size_t rows_bytes = r4.size() * sizeof(SnapRow), arrs_bytes = arrs.size() * sizeof(SnapArr);
    void* tab = nullptr;
    if (hipMalloc(&tab, rows_bytes + arrs_bytes) != hipSuccess) { (void)hipGetLastError(); lob_set_error("lob_snapshot_save: no room for the descriptor table"); return LOB_ENOMEM; }
    if (hipMemcpy(tab, r4.data(), rows_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((char*)tab + rows_bytes, arrs.data(), arrs_bytes, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(tab);
        lob_set_error("lob_snapshot_save: descriptor table upload failed");
        return LOB_EHIP;
    }
    a.rows = (const SnapRow*)tab;
    a.arrs = (const SnapArr*)((char*)tab + rows_bytes);
    e->snap_tab = tab;
    e->snap_bytes = off;
    return LOB_OK;
}
static int snap_slot_ok(lob_engine* e, int32_t slot, const char* who) {
    if (!e) { lob_set_error(std::string(who) + ": NULL engine"); return LOB_EINVAL; }
    if (slot < 0 || slot >= LOB_MAX_SNAPSHOTS) { lob_set_error(std::string(who) + ": slot " + std::to_string(slot) + " is outside [0, " + std::to_string(LOB_MAX_SNAPSHOTS) + ")"); return LOB_EINVAL; }
    return LOB_OK;
}
int lob_snapshot_save(lob_engine* e, int32_t slot, const uint8_t* dev_mask) {
    int rc = snap_slot_ok(e, slot, "lob_snapshot_save");
    if (rc) return rc;
    LOB_GUARD(e, lob_snapshot_save);
    if (dev_mask && !e->snap_valid[slot]) { lob_set_error("lob_snapshot_save: a masked save needs a slot that holds a full save (NULL mask) of this episode"); return LOB_ESTATE; }
    HIPCHK(hipSetDevice(e->device));
    if ((rc = snap_prepare(e))) return rc;
    if (e->snap_buf[slot].reserve(e->snap_bytes)) {   // (the slot's one allocation: hipMalloc synchronises the device)
        lob_set_error("lob_snapshot_save: no room for the slot's buffer (" + std::to_string(e->snap_bytes) + " bytes)");
        return LOB_ENOMEM;
    }
    {
        TimedLaunch t(e, dev_mask ? "snapshot_masked_kernel" : "snapshot_all_kernel", nullptr, true);
        lobk_snapshot(e->stream, false, e->snap_args, e->snap_buf[slot].p, dev_mask);
    }
    HIPCHK(hipGetLastError());
    e->snap_valid[slot] = true;
    return LOB_OK;
}
int lob_snapshot_restore(lob_engine* e, int32_t slot, const uint8_t* dev_mask) {
    int rc = snap_slot_ok(e, slot, "lob_snapshot_restore");
    if (rc) return rc;
    LOB_GUARD(e, lob_snapshot_restore);
    if (e->slog_n) { lob_set_error("lob_snapshot_restore: the step log is enabled (a row is due where total_ticks > n_rows + n_lost: total_ticks cannot go back under it)"); return LOB_ESTATE; }
    if (!e->snap_valid[slot] || !e->snap_buf[slot].p) { lob_set_error("lob_snapshot_restore: slot " + std::to_string(slot) + " holds no save of this episode"); return LOB_ESTATE; }
    HIPCHK(hipSetDevice(e->device));
    {
        TimedLaunch t(e, dev_mask ? "snapshot_masked_kernel" : "snapshot_all_kernel", nullptr, true);
        lobk_snapshot(e->stream, true, e->snap_args, e->snap_buf[slot].p, dev_mask);
    }
    HIPCHK(hipGetLastError());
    e->restored = true;
    e->hits_ok = false;
    return LOB_OK;
}
int lob_snapshot_free(lob_engine* e, int32_t slot) {
    const int rc = snap_slot_ok(e, slot, "lob_snapshot_free");
    if (rc) return rc;
    if (!e->snap_buf[slot].p) return LOB_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));   // (a save or restore still queued uses the buffer)
    e->snap_buf[slot].release();
    e->snap_valid[slot] = false;
    return LOB_OK;
}

}  // extern "C"
