// Host side of the C ABI (include/lob_engine.h), the part that launches kernels of this unit by name: the engine object's life
// (lob_create / lob_destroy / lob_reset), the step pipeline, the weights and both weight exchanges, kernel timing, the
// diagnostics that launch.  gfx950 only; there is no CPU execution path in this file.  (One of the library's fifteen units with
// kernels, lob_launch.h -- the update, memo and trace kernels are compiled here --; the streams, the vector env with the
// snapshots, and the read-backs and logs are host-only units of their own, lob_tu_host_*.hip, over lob_engine_impl.h.)
#define LOB_TU_SPLIT 1
#define LOB_TU_MAIN 1
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <initializer_list>
#include <string>
#include <vector>

#include "lob_internal.h"
#include "lob_fast.h"
#include "lob_kernels.h"
#include "lob_launch.h"

#include "lob_engine_impl.h"

namespace {

// The 2048-entry table of the UNH CMAC hash (reference src/rl/tiles.cpp:133)
// is the low-byte stream of an unseeded glibc rand() (generator left commented
// out at tiles.cpp:141-149).  Regenerated from the glibc TYPE_3 additive
// feedback recurrence r[i] = r[i-3] + r[i-31]; tests compare it with the
// reference's own table.
void make_rndseq(uint32_t* t) {
    const int total = 344 + 4 * 2048;
    std::vector<int32_t> r(total);
    r[0] = 1;
    for (int i = 1; i < 31; i++) {
        int64_t v = (16807LL * r[i - 1]) % 2147483647LL;
        if (v < 0) v += 2147483647LL;
        r[i] = (int32_t)v;
    }
    for (int i = 31; i < 34; i++) r[i] = r[i - 31];
    for (int i = 34; i < total; i++) r[i] = (int32_t)((uint32_t)r[i - 31] + (uint32_t)r[i - 3]);
    for (int k = 0; k < 2048; k++) {
        uint32_t v = 0;
        for (int i = 0; i < 4; i++) v = (v << 8) | ((((uint32_t)r[344 + 4 * k + i]) >> 1) & 0xff);
        t[k] = v;
    }
}

int grid_lanes(int B) { return (B + 255) / 256; }
int grid_waves(int B) { return (B + LOB_WAVES_PER_BLOCK - 1) / LOB_WAVES_PER_BLOCK; }

// The shapes of the switches' values: set at all, to anything; "=0" / "=1" (the first character); a number in [lo, hi]; one of
// {...}; a power of two in [lo, hi].  Anything else leaves the default.
bool env_set(const char* n) { return getenv(n) != nullptr; }
bool env_is(const char* n, char c) { const char* g = getenv(n); return g && g[0] == c; }
long long env_in(const char* n, long long lo, long long hi, long long dflt) { const char* g = getenv(n); const long long v = g ? atoll(g) : dflt; return v >= lo && v <= hi ? v : dflt; }
int env_one_of(const char* n, std::initializer_list<int> allowed, int dflt) {
    const char* g = getenv(n);
    for (int a : allowed) if (g && atoi(g) == a) return a;
    return dflt;
}
int env_pow2(const char* n, int lo, int hi, int dflt) { const int v = (int)env_in(n, lo, hi, dflt); return (v & (v - 1)) == 0 ? v : dflt; }

Switches read_switches() {
    Switches s;
    s.no_memo = env_is("LOB_NO_MEMO", '1'); s.no_carry = env_is("LOB_NO_CARRY", '1'); s.no_combine = env_is("LOB_NO_COMBINE", '1');
    s.light = !env_is("LOB_NO_LIGHT", '1'); s.force_fuse_act = env_is("LOB_FUSE_ACT", '1');
    s.t_light = !env_is("LOB_NO_TLIGHT", '1'); s.no_fuse = env_is("LOB_NO_FUSE", '1');
    s.q_pair = !env_is("LOB_Q_PAIR", '0'); s.dq_pair = !env_is("LOB_DQ_PAIR", '0'); s.trace_lanes_off = env_is("LOB_TRACE_LANES", '0');
    s.acc_fuse = !env_is("LOB_ACC_FUSE", '0'); s.rest_merge = !env_is("LOB_REST_MERGE", '0'); s.acc_dense = !env_is("LOB_ACC_DENSE", '0');
    s.q_lanes = env_set("LOB_Q_LANES") ? (env_is("LOB_Q_LANES", '1') ? 1 : 0) : -1;
    s.force_general = env_is("LOB_MOSTLY_GENERAL", '1') ? 1 : env_is("LOB_MOSTLY_GENERAL", '0') ? 0 : -1;
    const bool exps = lobk_experiments() != 0;
    s.env_lanes = exps ? env_one_of("LOB_ENV_LANES", {16, 32, 64, 256}, 0) : env_one_of("LOB_ENV_LANES", {16, 64}, 0);
    s.env16_max = (int)env_in("LOB_ENV16_MAX", 0, INT_MAX, s.env16_max);
    s.acc_batches = env_one_of("LOB_ACC_BATCHES", {1, 2, 4, 8}, 0);
    const int acc_lanes = env_one_of("LOB_ACC_LANES", {8, 16, 32, 64}, 0);
    s.acc_shift = acc_lanes ? __builtin_ctz(acc_lanes) : -1;
    s.cb_slots = env_pow2("LOB_CB_SLOTS", 64, 1 << 24, 0); s.ow_slots = env_pow2("LOB_OW_SLOTS", 64, 1 << 26, 0);
    s.amb_cap = (int)env_in("LOB_AMB_CAP", 1, 1 << 18, 0); s.cbd_ids = (int)env_in("LOB_CBD_IDS", 8, LOB_CBD_CAP, 0);
    s.track_ring = env_pow2("LOB_TRACK_RING", 256, 1 << 20, s.track_ring); s.track_refill = (int)env_in("LOB_TRACK_REFILL", 1, INT_MAX, s.track_refill);
    s.upload_piece_recs = env_in("LOB_UPLOAD_PIECE_RECS", 1, LLONG_MAX, 0); s.upload_pinned = !env_is("LOB_UPLOAD_PINNED", '0');
    s.spx_count = env_in("LOB_SPX_COUNT", 64, LLONG_MAX, 0);
    if (!exps) return s;
    s.fuse_act = !env_is("LOB_NO_FUSE_ACT", '1'); s.inline_general = !env_is("LOB_INLINE_GENERAL", '0'); s.env_step = !env_is("LOB_ENV_STEP", '0');
    s.prepass_roles = env_is("LOB_PREPASS_ROLES", '1'); s.sarsa_lanes_off = env_is("LOB_SARSA_LANES", '0'); s.dq_fast_off = env_is("LOB_DQ_FAST", '0');
    s.rest_side = !env_is("LOB_REST_SIDE", '0'); s.acc_block = !env_is("LOB_ACC_BLOCK", '0');
    s.exp_learn_first = env_set("LOB_SARSA_LEARN_FIRST"); s.no_hint = env_set("LOB_NO_HINT");
    s.env_step_lanes = env_one_of("LOB_ENV_STEP_LANES", {32}, s.env_step_lanes); s.reset_lanes = env_one_of("LOB_RESET_LANES", {16, 32, 64}, s.reset_lanes);
    s.n_groups = (int)env_in("LOB_GROUPS", 1, 2, s.n_groups); s.acc_reps = env_pow2("LOB_ACC_REPS", 1, 64, 0);
    s.ts_lds = (int)env_in("LOB_TS_LDS", INT_MIN, INT_MAX, 0); s.ts_grid = (int)env_in("LOB_TS_GRID", INT_MIN, INT_MAX, 0);
    return s;
}

// The kernel paths fixed for the engine's life.  `P`: the engine's reading of lob_params (algorithm, theta mode, record shape, trace ring).
EnginePlan plan_paths(const DevParams& P, int B, int n_cus, const Switches& sw) {
    EnginePlan pl;
    const bool sarsa = P.algo == LOB_ALGO_SARSA, ql = P.algo == LOB_ALGO_QLAMBDA, dq = P.algo == LOB_ALGO_DOUBLE_Q;
    pl.groups = B >= 1024 ? sw.n_groups : 1;   // (small batches: one group -- an empty group would be an empty launch)
    pl.combine = !P.theta_private && !sw.no_combine;
    pl.env_lanes = sw.env_lanes ? sw.env_lanes : (B <= 16384 ? 16 : 64);  // (16: the batch is too small to give every SIMD a wave of 64)
    // (batches of 1 024 books and more, env_kernel<64>: the action selection rides in the env kernel -- 4 096 books: 25.0 -> 27.2 M
    // env-steps/s, 16 384: 65.5 -> 75.8 M); up to env16_max books, a book's levels across 16 lanes (layout: lob_envstep.h)
    pl.fused_act_ok = sw.light && sw.fuse_act && sw.env_lanes == 0 && (B >= 1024 || sw.force_fuse_act);
    pl.env_step = P.T <= 2 && sw.env_step;
    pl.half_waves = sw.env_step_lanes == 32 && pl.env_step && !dq;
    pl.inline_ok = pl.env_step && sw.inline_general && !pl.half_waves;
    pl.env16 = !dq && B <= sw.env16_max && P.D <= 16 && P.Wd <= 64;
    // Q(s', .) + TD error: a lane per book once the batch gives every CU a full block of them, else a wave per book; the lane
    // kernel then also takes the light trace step of the books it can (those left go on a list for the trace kernel behind it)
    pl.q_lanes = sw.q_lanes >= 0 ? sw.q_lanes == 1 : (long long)B >= (long long)LOB_QL_BLOCK * n_cus / 2;
    pl.q_pair = sw.q_pair && P.M < (1ll << 27) && (!dq || sw.dq_pair);  // (its LDS rows hold tile indices in 27 bits)
    pl.t_light = (ql || dq) && sw.t_light;
    pl.fuse = pl.t_light && pl.q_lanes && !sw.no_fuse;
    // group-0 memo: shared theta, one book group.  Double Q only through the kernels that know two weight vectors: the fused
    // env_step_kernel, the lane learn kernel with the fused Watkins trace step, the lane trace kernel behind it
    pl.memo = !P.theta_private && !P.r_learn && sw.n_groups == 1 && !sw.no_memo;
    if (dq) pl.memo = pl.memo && pl.fuse && pl.fused_act_ok && pl.env_step && pl.combine && P.trace_gens == 32 && !sw.dq_fast_off;
    pl.carry_verdicts = !P.theta_private && !sw.no_carry && !pl.memo;  // (the memo path never reads the carry-over filter)
    // the trace step with a lane per generation + the tile registry it needs: every book of SARSA(lambda); the books of Q(lambda)
    // / double Q whose traces survive, listed by the lane learn kernel
    pl.sarsa_lanes = pl.memo && pl.combine && P.trace_gens == 32 && !sw.sarsa_lanes_off && !sw.trace_lanes_off && (sarsa || pl.fuse);
    pl.acc_block_ok = sw.acc_block && pl.memo && B >= 4 * LOB_ACB_BLOCK;
    // (SARSA(lambda) sums per block always, Q(lambda) once most actions are greedy)
    pl.dense_ids = pl.acc_block_ok && pl.combine && sw.acc_dense && (sarsa || ql) && P.trace_gens <= LOB_TRACE_GENS;
    pl.acc_fuse_ok = pl.fuse && sw.acc_fuse && pl.combine && pl.sarsa_lanes && (ql || dq) && pl.groups == 1;
    pl.rest_side_ok = pl.fuse && sw.rest_side;
    pl.learn_first = sw.exp_learn_first && sarsa;
    return pl;
}

}  // namespace

namespace lob {

// The device copy of DevState follows the host's (rare: a stream loaded, the exchange's buffers allocated, model_log switched on).
// (Copied byte for byte, so that memcmp compares exactly the bytes that were uploaded, padding included.)
int sync_state(lob_engine* e) {
    DevState now;
    memcpy(&now, &e->S, sizeof(DevState));
    now.cb_par = 0;
    now.cb_dense_on = 0;
    now.self = e->S_dev;
    if (memcmp(&now, &e->S_pushed, sizeof(DevState)) == 0) return LOB_OK;
    if (hipMemcpyAsync(e->S_dev, &now, sizeof(DevState), hipMemcpyHostToDevice, e->stream) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) {
        lob_set_error("state upload failed");
        return LOB_EHIP;
    }
    memcpy(&e->S_pushed, &now, sizeof(DevState));
    return LOB_OK;
}
int push_params(lob_engine* e) {
    if (hipMemcpyAsync(e->P_dev, &e->P, sizeof(DevParams), hipMemcpyHostToDevice, e->stream) != hipSuccess) { lob_set_error("param upload failed"); return LOB_EHIP; }
    return LOB_OK;
}

void drain_timers(lob_engine* e) {
    for (auto& kv : e->timers) {
        for (auto& pr : kv.second.pending) {
            hipEventSynchronize(pr.second);
            float ms = 0;
            hipEventElapsedTime(&ms, pr.first, pr.second);
            kv.second.total_ms += ms;
            kv.second.launches++;
            e->event_pool.push_back(pr.first);
            e->event_pool.push_back(pr.second);
        }
        kv.second.pending.clear();
    }
}

// LOB_EDATA and its message for a non-zero device error word
int device_error_rc(i32 flag) {
    if (flag) {
        std::string m = "device reported a condition on which the reference throws:";
        if (flag & LOB_ERR_BAD_ORDER_PRICE) m += " [order price <= 0]";
        if (flag & LOB_ERR_BAD_LEVEL) m += " [level price/volume <= 0]";
        if (flag & LOB_ERR_UNDEF_PRICE) m += " [undefined book price]";
        if (flag & LOB_ERR_TRADE_OVERFLOW) m += " [more trade price levels in one event than max_trades]";
        if (flag & LOB_ERR_TRACK_UNDERRUN) m += " [market-track ring underrun: raise LOB_TRACK_RING or lower LOB_TRACK_REFILL]";
        lob_set_error(m);
        return LOB_EDATA;
    }
    return LOB_OK;
}
int check_device_errors(lob_engine* e) {
    i32 flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, e->S.error_flag, sizeof flag, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return device_error_rc(flag);
}

int finalize_episode(lob_engine* e) {
    if (!e->episode_open) return LOB_OK;
    lobk_finalize(e->stream, e->P.T <= 2, (const DevParams*)e->P_dev, e->S);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    e->episode_open = false;
    return LOB_OK;
}

// env_kernel with EnginePlan::env_lanes books per wave
void launch_env(lob_engine* e, hipStream_t st, const i32* actions, int count_updates, int b0, int nb, int par) {
    lobk_env(st, e->plan.env_lanes, e->P.T <= 2, (const DevParams*)e->P_dev, e->S, actions, count_updates, b0, nb, e->step_id, par);
}
// Long streams: let the pre-pass run on every `track_refill` steps (lob_kernels.h prepass_extend_kernel)
void maybe_refill_track(lob_engine* e) {
    e->real_steps++;
    if (!e->chunked || ++e->steps_since_fill < e->sw.track_refill) return;
    e->steps_since_fill = 0;
    TimedLaunch t(e, "prepass_extend_kernel", nullptr, true);
    lobk_prepass_extend(e->stream, e->P.T <= 2, e->sw.prepass_roles, (const DevParams*)e->P_dev, e->S);
}
// In front of a look-ahead `depth` steps deep on a ring (lob_look_ring): the real step is safe because the ring is refilled every
// `track_refill` steps; the look-ahead gets the same guarantee when the refill that would fall inside its depth is made now.  A refill
// moves no observable bit of the real books -- the track is a function of the stream alone, and what it overwrites lies behind the real
// cursor by the margin.  Decided on the host's counters: no read, no synchronisation.
void look_refill_track(lob_engine* e, long long depth) {
    if (!e->chunked || !e->look_ring || (long long)e->steps_since_fill + depth <= (long long)e->sw.track_refill) return;
    e->steps_since_fill = 0;
    TimedLaunch t(e, "prepass_extend_kernel", nullptr, true);
    lobk_prepass_extend(e->stream, e->P.T <= 2, e->sw.prepass_roles, (const DevParams*)e->P_dev, e->S);
}
// S0 of every group-0 triple on this step's list (lob_kernels.h memo_kernel): `which` 0 = for learn_kernel
// (theta_t), 1 = for the next act_kernel (after the update)
void launch_memo(lob_engine* e, int par, int which, int reset_lpar) {
    TimedLaunch t(e, "memo_kernel");
    hipLaunchKernelGGL(memo_kernel, dim3(256), dim3(256), 0, e->stream, e->P, e->S, (const uint32_t*)e->rnd_dev, par, which, (u64)e->theta_ver, reset_lpar);
}

// The step log's row of every selected book that has just completed a step (lob_tu_steplog.hip step_log_kernel): on the main stream
// behind the step's last kernel; not launched while the log is off or waits for its first lob_reset.
void launch_step_log(lob_engine* e) {
    if (!e->slog_armed) return;
    TimedLaunch t(e, "step_log_kernel");
    StepLogSrc s;
    s.done = e->S.done; s.time_ms = e->S.time_ms; s.rec_cur = e->S.rec_cur; s.last_action = e->S.last_action;
    s.ask_level = e->S.ask_level; s.bid_level = e->S.bid_level; s.total_ticks = e->S.total_ticks;
    s.position = e->S.position;
    s.ask_quote = e->S.ask_quote; s.bid_quote = e->S.bid_quote; s.pnl_step = e->S.pnl_step;
    s.ep_pnl = e->S.ep_pnl; s.ep_bandh = e->S.ep_bandh; s.ep_reward = e->S.ep_reward;
    s.records = e->S.records; s.rec_phase = e->S.rec_phase;
    s.n_events = e->S.n_events; s.Wd = e->P.Wd; s.w_ask0 = drec_ask_px(e->P.D, e->P.T); s.w_bid0 = drec_bid_px(e->P.D, e->P.T);
    s.sel = e->slog_sel; s.n_sel = e->slog_n; s.cap = e->slog_cap;
    s.rows = e->slog_rows; s.n_rows = e->slog_cnt; s.n_lost = e->slog_cnt + e->slog_n;
    lobk_step_log(e->stream, s);
}

// The one check of the engine's state in front of an entry point (lob_engine_impl.h: the bits, and which call asks for which)
int guard(lob_engine* e, const char* who, unsigned needs) {
    if (!e) return LOB_EINVAL;
    const char* why = nullptr;
    if ((needs & RESET) && !e->was_reset) why = ": call lob_reset first";
    else if ((needs & WHOLE_STEP) && e->half_open) why = ": a learner step is half done (lob_td_step_begin without lob_td_step_end)";
    else if ((needs & NOT_RESTORED) && e->restored) why = ": books were put back by lob_snapshot_restore in this episode; the learner runs again after the next lob_reset";
    else if ((needs & NO_RING) && e->chunked && !e->look_ring) why = ": the market track of this stream is a ring (longer than LOB_TRACK_RING events)";
    else if ((needs & NO_RING_BACK) && e->chunked) why = ": the market track of this stream is a ring (longer than LOB_TRACK_RING events): entries before the cursor are gone, no earlier state can be served";
    if (!why) return LOB_OK;
    lob_set_error(std::string(who) + why);
    return LOB_ESTATE;
}

}  // namespace lob

extern "C" {

static int theta_random_init(lob_engine* e);

int lob_create(const lob_params* p, int32_t n_books, int32_t device, lob_engine** out) {
    if (!p || !out || n_books < 1) { lob_set_error("lob_create: bad argument"); return LOB_EINVAL; }
    if (p->abi_version != LOB_ABI_VERSION) { lob_set_error("lob_create: ABI version mismatch"); return LOB_EINVAL; }
    if (p->depth < 1 || p->depth > LOB_MAX_DEPTH || p->max_trades < 1 || p->max_trades > LOB_MAX_TRADES) {
        lob_set_error("lob_create: depth/max_trades out of range"); return LOB_EINVAL;
    }
    if (p->n_tilings != LOB_N_TILINGS || p->n_actions != LOB_N_ACTIONS) {
        lob_set_error("lob_create: kernels are built for n_tilings=32, n_actions=9"); return LOB_EINVAL;
    }
    if (p->n_vars < 4 || p->n_vars > LOB_MAX_VARS) { lob_set_error("lob_create: n_vars must be in [4,13]"); return LOB_EINVAL; }
    if (p->memory_size < 1 || p->memory_size >= (1LL << 31)) { lob_set_error("lob_create: memory_size out of range"); return LOB_EINVAL; }
    if (p->market.n_bands < 1 || p->market.n_bands > LOB_MAX_BANDS) { lob_set_error("lob_create: bad tick table"); return LOB_EINVAL; }
    if (p->algo < LOB_ALGO_SARSA || p->algo > LOB_ALGO_DOUBLE_R_LEARN) { lob_set_error("lob_create: unknown algorithm"); return LOB_EINVAL; }
    if (p->policy != LOB_POLICY_EPS_GREEDY && p->policy != LOB_POLICY_BOLTZMANN) { lob_set_error("lob_create: unknown policy"); return LOB_EINVAL; }
    if (p->policy == LOB_POLICY_BOLTZMANN && !(p->tau > 0.0)) { lob_set_error("lob_create: Boltzmann temperature must be positive"); return LOB_EINVAL; }
    const int lbs[] = {p->lb_mpm, p->lb_vlt, p->lb_svl, p->lb_vwap, p->lb_rsi, p->lb_spread, p->lb_pnl, p->lb_target};
    for (int w : lbs)
        if (w < 1 || w > LOB_MAX_WINDOW) { lob_set_error("lob_create: lookbacks must be in [1,256]"); return LOB_EINVAL; }
    if (p->order_size < 1) { lob_set_error("lob_create: order_size"); return LOB_EINVAL; }

    // Traces::decay(float rate), quirk Q15: eligibility by age as iterated float products; checked before
    // any HIP resource exists
    float trace_pow[LOB_TRACE_GENS + 1];
    int trace_kmax = -1;
    const float trace_rate = (float)(p->gamma * p->lambda);
    trace_pow[0] = 1.0f;
    for (int k = 1; k <= LOB_TRACE_GENS; k++) {
        trace_pow[k] = trace_pow[k - 1] * trace_rate;
        if (trace_kmax < 0 && trace_pow[k] < 0.01f) trace_kmax = k;
    }
    if (trace_kmax < 0 || trace_kmax > LOB_TRACE_GENS) {
        lob_set_error("lob_create: gamma*lambda too close to 1 for the trace ring (LOB_TRACE_GENS = 64 generations, gamma*lambda <= ~0.93)");
        return LOB_EINVAL;
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev) {
        lob_set_error("lob_create: no usable HIP device (the engine has no CPU fallback)");
        return LOB_ENODEV;
    }
    HIPCHK(hipSetDevice(device));
    lob_engine* e = new lob_engine();
    e->device = device;
    e->B = n_books;
    e->params = *p;
    e->sw = read_switches();
    {   // (the persistent learner kernels run one block on each CU)
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) e->n_cus = prop.multiProcessorCount;
    }
    // from here on every failure path releases what exists so far (lob_destroy copes with null members)
#define HIPCHK_E(expr)                                                                       \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            lob_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                \
            lob_destroy(e);                                                                  \
            return LOB_EHIP;                                                                 \
        }                                                                                    \
    } while (0)
    HIPCHK_E(hipStreamCreate(&e->stream));
    HIPCHK_E(hipStreamCreate(&e->stream2));
    HIPCHK_E(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK_E(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK_E(hipEventCreateWithFlags(&e->ev_stagger, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK_E(hipEventCreateWithFlags(&e->ev_rest_go, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK_E(hipEventCreateWithFlags(&e->ev_rest_done, hipEventDisableTiming | hipEventDisableSystemFence));
    if (hipHostMalloc((void**)&e->rest_hint, LOB_HINT_RING * sizeof(u64), hipHostMallocMapped) == hipSuccess) {
        memset(e->rest_hint, 0, LOB_HINT_RING * sizeof(u64));
        if (hipHostGetDevicePointer((void**)&e->rest_hint_dev, e->rest_hint, 0) != hipSuccess) e->rest_hint_dev = nullptr;
    } else e->rest_hint = nullptr;   // (no hint: the launch stays on the main stream)
    if (!e->rest_hint_dev && e->rest_hint) { hipHostFree(e->rest_hint); e->rest_hint = nullptr; }
    // (these events DO fence to system scope: the host reads the word the kernel in front of them stored to host memory)
    for (int i = 0; i < LOB_HINT_RING && e->rest_hint; i++) HIPCHK_E(hipEventCreateWithFlags(&e->hint_ev[i], hipEventDisableTiming));

    // ---- DevParams ----
    DevParams& P = e->P;
    memset(&P, 0, sizeof P);
    P.D = p->depth; P.T = p->max_trades; P.W = lob_rec_words(p->depth, p->max_trades); P.Wd = drec_words(p->depth, p->max_trades); P.V = p->n_vars;
    for (int i = 0; i < LOB_MAX_VARS; i++) P.vars[i] = p->vars[i];
    lobh::TickTable tt;
    lobh::build_tick_table(p->market, tt);
    P.n_bands = tt.n;
    for (int i = 0; i < LOB_MAX_BANDS; i++) { P.band_lb[i] = tt.lb[i]; P.band_tick[i] = tt.tick[i]; P.band_cum[i] = tt.cum[i]; P.band_pt[i] = tt.pt[i]; P.band_pp[i] = tt.pp[i]; }
    P.open_ms = p->market.open_ms; P.close_ms = p->market.close_ms;
    P.order_size = p->order_size; P.reward_measure = p->reward_measure;
    P.pos_lb = p->pos_lb; P.pos_ub = p->pos_ub;
    P.damping_factor = p->damping_factor; P.pos_weight = p->pos_weight; P.trd_weight = p->trd_weight; P.pnl_weight = p->pnl_weight;
    P.target_price = p->target_price; P.quote_mode = p->quote_mode;
    P.ewma_alpha = 2.0 / ((double)(size_t)p->lb_rsi + 1.0);
    P.M = p->memory_size;
    P.w0 = p->group_weights[0]; P.w1 = p->group_weights[1]; P.w2 = p->group_weights[2];
    P.gamma = p->gamma; P.alpha = p->alpha; P.epsilon = p->epsilon;
    P.policy = p->policy; P.tau = p->tau; P.beta = p->beta;
    P.trace_rate = trace_rate;
    for (int k = 0; k <= LOB_TRACE_GENS; k++) P.trace_pow[k] = trace_pow[k];
    P.trace_kmax = trace_kmax;
    P.trace_gens = P.trace_kmax <= 32 ? 32 : LOB_TRACE_GENS;
    // the average-reward agents are their base algorithm + r_learn (RLearn: Q(lambda), OnlineRLearn: SARSA, DoubleRLearn: double Q)
    P.r_learn = p->algo >= LOB_ALGO_R_LEARN;
    P.algo = p->algo == LOB_ALGO_R_LEARN ? LOB_ALGO_QLAMBDA : p->algo == LOB_ALGO_ONLINE_R_LEARN ? LOB_ALGO_SARSA
             : p->algo == LOB_ALGO_DOUBLE_R_LEARN ? LOB_ALGO_DOUBLE_Q : p->algo;
    P.theta_private = p->theta_mode == LOB_THETA_PRIVATE;
    e->plan = plan_paths(P, n_books, e->n_cus, e->sw);
    P.combine = e->plan.combine;
    P.memo = e->plan.memo;
    P.carry_verdicts = e->plan.carry_verdicts;
    P.sarsa_lanes = e->plan.sarsa_lanes;
    P.epi_epoch = 0;
    P.seed = p->seed; P.book_id_offset = p->book_id_offset;
    P.exp_learn_first = e->sw.exp_learn_first ? 1 : 0;

    // ---- DevState ----
    DevState& S = e->S;
    memset(&S, 0, sizeof S);
    const size_t B = (size_t)n_books;
    S.B = n_books; S.D = P.D; S.T = P.T; S.W = P.W;
    int rc = LOB_OK;
    auto alloc = [&](auto* ptr, size_t count) { if (rc == LOB_OK) rc = dev_alloc(e, ptr, count); };   // (the first failure sticks)
#define X(t, n) alloc(&S.n, B);
    LOB_ENV_FIELDS(X)
#undef X
    alloc(&S.hdr, B);
    auto alloc_rm = [&](RMPtrs& r, int w) {
        r.w = w;
        alloc(&r.ring, B * w); alloc(&r.cnt, B); alloc(&r.head, B); alloc(&r.sum, B); alloc(&r.mean, B); alloc(&r.s, B);
    };
    auto alloc_acc = [&](AccPtrs& r, int w) {
        r.w = w;
        alloc(&r.ring, B * w); alloc(&r.cnt, B); alloc(&r.head, B); alloc(&r.sum, B);
    };
    alloc_rm(S.f_midprice, p->lb_mpm);
    alloc_rm(S.f_volatility, p->lb_vlt);
    alloc_rm(S.f_ask_tx, p->lb_svl);
    alloc_rm(S.f_bid_tx, p->lb_svl);
    alloc_rm(S.spread_window, p->lb_spread);
    alloc_rm(S.pnl_ups, p->lb_pnl);
    alloc_rm(S.pnl_downs, p->lb_pnl);
    alloc_rm(S.tp_mp, p->lb_target);
    alloc_acc(S.f_vwap_numer, p->lb_vwap);
    alloc_acc(S.f_vwap_denom, p->lb_vwap);
    alloc(&S.meta, B); alloc(&S.prep, B); alloc(&S.ewma_up, B); alloc(&S.ewma_down, B); alloc(&S.tp_val, B); alloc(&S.persist, B * LOB_PERSIST_N);
    alloc(&S.k_stop, B); alloc(&S.vars, B * 3 * 16); alloc(&S.qs_last, B * LOB_N_ACTIONS); alloc(&S.tr_idx, B * (size_t)P.trace_gens * 32);
    alloc(&S.tr_alive, B * (size_t)P.trace_gens); alloc(&S.theta, (size_t)P.M * (P.theta_private ? B : 1));
    alloc(&S.theta_nz, LOB_NZ_NWORDS(P.M) * (P.theta_private ? B : 1));
    if (P.algo == LOB_ALGO_DOUBLE_Q) {
        alloc(&S.theta_b, (size_t)P.M * (P.theta_private ? B : 1)); alloc(&S.theta_b_nz, LOB_NZ_NWORDS(P.M) * (P.theta_private ? B : 1));
        alloc(&S.qs_last_b, B * LOB_N_ACTIONS); alloc(&S.mt_state, B * LOB_MT_N); alloc(&S.mt_idx, B);
    }
    {
        const bool rl = P.r_learn != 0;
        const size_t nr = rl ? (P.theta_private ? B : 1) : 1;
        alloc(&S.rho, nr); alloc(&S.rho_inc, nr); alloc(&S.rho_cnt, nr); alloc(&S.rl_t, rl ? B : 1);
    }
    alloc(&S.tr_sig, B * (size_t)P.trace_gens * 4); alloc(&S.tr_cbslot, B * (size_t)P.trace_gens);
    {
        // (slots persist while in use: room for the generations of a few steps; LOB_CB_SLOTS overrides, for the tests)
        int slots = 2048;
        while ((size_t)slots < 8 * B && slots < (1 << 22)) slots <<= 1;
        if (e->sw.cb_slots) slots = e->sw.cb_slots;
        S.cb_slots = slots;
        alloc(&S.cb_key, (size_t)slots); alloc(&S.cb_ident, (size_t)slots * 8);
        // SARSA(lambda) adds 1.6 M terms per step to the slots' sums: a copy of the sums per XCD (0.147 -> 0.100 ms; apply_kernel
        // 0.023 -> 0.03); Q(lambda)'s few additions are a latency chain that the copies do not shorten
        // ... and so do Watkins's Q(lambda) / double Q once the policy is mostly greedy (epsilon decays over the episodes: no cut,
        // 25 generations per book, and the greedy books crowd onto a few (triple, action) pairs: 0.44 ms per step with one copy at
        // epsilon = 0.01).  One copy per XCD for every algorithm on the fast path; apply_kernel adds them up.
        S.cb_reps = e->sw.acc_reps ? e->sw.acc_reps : P.memo ? 8 : 1;
        alloc(&S.cb_acc, (size_t)S.cb_reps * slots * 2); alloc(&S.cb_touch, (size_t)slots); alloc(&S.cb_list, 2 * (size_t)slots);
        S.cb_segs = std::min(2048, slots / 4);
        alloc(&S.cb_count, 2 * (size_t)S.cb_segs);
        if (rc == LOB_OK && hipMemsetAsync(S.cb_key, 0xff, (size_t)slots * 8, e->stream) != hipSuccess) rc = LOB_EHIP;
        // dense ids of the slots (EnginePlan::dense_ids)
        if (e->plan.dense_ids) {
            alloc(&S.cb_dense, (size_t)slots); alloc(&S.cb_free, (size_t)LOB_CBD_CAP); alloc(&S.cb_free_n, 16);
            alloc(&S.tr_cbd, B * (size_t)P.trace_gens); alloc(&S.cb_part, (size_t)LOB_ACD_MAX_BLOCKS * LOB_CBD_CAP);
            alloc(&S.cb_red, (size_t)LOB_ACD_GROUPS * LOB_CBD_CAP);
            if (rc == LOB_OK && hipMemsetAsync(S.cb_dense, 0xff, (size_t)slots * 4, e->stream) != hipSuccess) rc = LOB_EHIP;
            if (rc == LOB_OK && hipMemsetAsync(S.tr_cbd, 0xff, B * (size_t)P.trace_gens * 8, e->stream) != hipSuccess) rc = LOB_EHIP;
            if (rc == LOB_OK) {
                // list x: the ids = x mod 8, the lowest on top; nothing handed out yet
                // (LOB_CBD_IDS=n: only n ids in all, for the tests -- most slots then go without one)
                std::vector<i32> fl(LOB_CBD_CAP), fn(16);
                const int per = LOB_CBD_CAP / 8;
                int have = per;
                if (e->sw.cbd_ids) have = e->sw.cbd_ids / 8;
                S.cb_ids = have * 8;
                for (int x = 0; x < 8; x++) {
                    for (int i = 0; i < have; i++) fl[(size_t)x * per + i] = (have - 1 - i) * 8 + x;
                    fn[2 * x] = have;
                    fn[2 * x + 1] = have;
                }
                if (hipMemcpyAsync(S.cb_free, fl.data(), fl.size() * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
                    hipMemcpyAsync(S.cb_free_n, fn.data(), fn.size() * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
                    hipStreamSynchronize(e->stream) != hipSuccess) rc = LOB_EHIP;
            }
            if (rc == LOB_OK && hipFuncSetAttribute((const void*)accumulate_dense_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)acd_lds_bytes()) != hipSuccess) {
                lob_set_error("hipFuncSetAttribute(accumulate_dense_kernel: dynamic LDS)");
                rc = LOB_EHIP;
            }
        }
    }
    {
        S.mk_slots = 1 << 16;
        const size_t ms = (size_t)S.mk_slots;
        alloc(&S.mk_hash, ms); alloc(&S.mk_ident, ms * 4); alloc(&S.mk_stamp, ms); alloc(&S.mk_list, 2 * ms); alloc(&S.mk_count, 2);
        alloc(&S.mk_rec, 2 * ms * LOB_MK_REC);
        if (P.memo && P.algo == LOB_ALGO_DOUBLE_Q) alloc(&S.mk_rec_b, 2 * ms * LOB_MK_REC);
        alloc(&S.mk_tiles, P.memo ? ms * LOB_N_ACTIONS * 32 : 1); alloc(&S.mk_tiles_ok, ms); alloc(&S.mk_marked, ms); alloc(&S.mk_marklist, ms);
        alloc(&S.mk_markcount, 1); alloc(&S.tr_list, B); alloc(&S.tr_list_n, 2); alloc(&S.tr_list2, B); alloc(&S.tr_list2_n, 2);
        alloc(&S.acc_list, B); alloc(&S.acc_list_n, 2); alloc(&S.acc_pend, B); alloc(&S.dir_list, P.combine ? B * (size_t)P.trace_gens : 1);
        alloc(&S.dir_list_n, 2); alloc(&S.mk_slot, B); alloc(&S.mk_slot_last, B);
        if (rc == LOB_OK && hipMemsetAsync(S.mk_hash, 0xff, ms * 8, e->stream) != hipSuccess) rc = LOB_EHIP;
        if (rc == LOB_OK && hipMemsetAsync(S.mk_slot, 0xff, B * 4, e->stream) != hipSuccess) rc = LOB_EHIP;
        if (rc == LOB_OK && hipMemsetAsync(S.mk_slot_last, 0xff, B * 4, e->stream) != hipSuccess) rc = LOB_EHIP;
        // tile registry of the SARSA lane path (lob_state.h)
        const bool sl = P.sarsa_lanes != 0;
        S.ow_slots = sl ? 1 << 25 : 1;  // 65 536 memo slots x 288 tiles at most: load <= 0.56
        S.amb_cap = sl ? (int)std::min<long long>((long long)P.M, 1 << 18) : 1;
        // (LOB_OW_SLOTS / LOB_AMB_CAP: tiny values for the tests -- a registry without room leaves slots unregistered, a full list
        // of new ambiguous indices switches the lane kernel off until the next reset: every book then goes to the wave-per-book kernel)
        if (sl && e->sw.ow_slots) S.ow_slots = e->sw.ow_slots;
        if (sl && e->sw.amb_cap) S.amb_cap = e->sw.amb_cap;
        alloc(&S.tr_mslot, sl ? B * (size_t)P.trace_gens : 1); alloc(&S.ow_tab, (size_t)S.ow_slots);
        alloc(&S.amb_bits, sl ? (size_t)P.M / 32 + 1 : 1); alloc(&S.amb_new, 2 * (size_t)S.amb_cap); alloc(&S.amb_new_n, 2); alloc(&S.amb_flag, 1);
        alloc(&S.mk_amb, sl ? ms * LOB_N_ACTIONS : 1); alloc(&S.mk_all, sl ? ms : 1); alloc(&S.mk_all_n, 1);
        if (rc == LOB_OK && hipMemsetAsync(S.tr_mslot, 0xff, (sl ? B * (size_t)P.trace_gens : 1) * 4, e->stream) != hipSuccess) rc = LOB_EHIP;
        if (rc == LOB_OK && hipMemsetAsync(S.ow_tab, 0xff, (size_t)S.ow_slots * 8, e->stream) != hipSuccess) rc = LOB_EHIP;
    }
    {
        // coarse written-weights map of the fast path: the finest granularity whose image fits 80 KB of LDS
        int cs = 5;
        while ((((size_t)P.M >> cs) + 31) / 32 > 20480) cs++;
        P.cshift = cs;
        const size_t cwords = (((size_t)P.M >> cs) + 32) / 32;
        P.cwords4 = (int)((cwords + 3) / 4);
        alloc(&S.theta_nzx, P.memo ? (size_t)P.M / 32 + 1 : 1); alloc(&S.theta_nzc, (size_t)P.cwords4 * 4);
        if (P.memo) alloc(&S.theta_nzd, 2 * ((size_t)P.M / 32 + 1));
        // (the per-sum action masks behind it: for the pair kernel only -- 80 MB at M = 20 M)
        if (P.memo && e->plan.q_lanes && e->plan.q_pair) alloc(&S.theta_nzm, 2 * fold_mask_words((uint32_t)P.M));
        alloc(&S.slow_list, 2 * B); alloc(&S.slow_n, 4); alloc(&S.hl_rec, P.memo ? (size_t)LOB_HL_REC * B : 1); alloc(&S.hl_dirty, 1);
        if (rc == LOB_OK && hipMemsetAsync(S.hl_rec, 0xff, (P.memo ? (size_t)LOB_HL_REC * B : 1) * 8, e->stream) != hipSuccess) rc = LOB_EHIP;
        if (rc == LOB_OK && hipMemsetAsync(S.hl_dirty, 0xff, 4, e->stream) != hipSuccess) rc = LOB_EHIP;
        if (P.memo) {
            const int q_lds = (int)fast_lds_bytes(P.cwords4, LOB_FAST_NB, false), tr_lds = (int)trace_lds_bytes();
            hipError_t er = hipFuncSetAttribute((const void*)act_fast_kernel<LOB_FAST_NB>, hipFuncAttributeMaxDynamicSharedMemorySize, q_lds);
            if (er == hipSuccess) er = lobk_learn_set_lds(q_lds, (int)qlane_lds_bytes(P.cwords4), (int)qpair_lds_bytes(P.cwords4));
            if (er == hipSuccess) er = hipFuncSetAttribute((const void*)trace_fast_kernel<LOB_ALGO_SARSA, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, tr_lds);
            if (er == hipSuccess) er = hipFuncSetAttribute((const void*)trace_fast_kernel<LOB_ALGO_SARSA, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, tr_lds);
            if (er == hipSuccess) er = hipFuncSetAttribute((const void*)trace_fast_kernel<LOB_ALGO_QLAMBDA, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, tr_lds);
            if (er == hipSuccess) er = hipFuncSetAttribute((const void*)trace_fast_kernel<LOB_ALGO_QLAMBDA, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, tr_lds);
            if (er == hipSuccess) er = hipFuncSetAttribute((const void*)trace_fast_kernel<LOB_ALGO_QLAMBDA, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, tr_lds);
            if (er == hipSuccess) er = hipFuncSetAttribute((const void*)trace_rest_kernel<LOB_ALGO_QLAMBDA>, hipFuncAttributeMaxDynamicSharedMemorySize, tr_lds);
            if (er == hipSuccess) er = hipFuncSetAttribute((const void*)trace_rest_kernel<LOB_ALGO_DOUBLE_Q>, hipFuncAttributeMaxDynamicSharedMemorySize, tr_lds);
            if (er != hipSuccess && rc == LOB_OK) { lob_set_error(std::string("hipFuncSetAttribute(dynamic LDS): ") + hipGetErrorString(er)); rc = LOB_EHIP; }
        }
    }
    alloc(&S.verdict, B * LOB_VD_STRIDE); alloc(&S.nz_new, 4 * LOB_NZ_WORDS); alloc(&S.verdict_b, P.algo == LOB_ALGO_DOUBLE_Q ? B * 64 : 1);
    alloc(&S.nz_epoch, 1);
    // (striped: lob_state.h cnt_add; [8]: generations apply_kernel applied from trace_rest_kernel's list, lob_debug_deferred)
    alloc(&S.counters, (size_t)LOB_CNT_STRIPES * LOB_CNT_STRIDE); alloc(&e->cnt_sum, 16); alloc(&S.error_flag, 1);
#ifdef LOB_PROF
    alloc(&S.prof, B * LOB_PROF_N);
#endif
    alloc(&e->rnd_dev, 2048 + 64);
    S.nzd_terms = e->rnd_dev ? e->rnd_dev + 2048 + LOB_N_ACTIONS : nullptr;  // term[1][.], term[2][.] (filled below)
    alloc(&e->actions_dev, B); alloc(&e->P_dev, 1); alloc(&e->S_dev, 1);
    alloc(&e->vec_bad, 3);   // (+ the two look-ahead cell counts)
    alloc(&e->vec_upd_tag, 1);
    if (rc == LOB_OK && hipMemsetAsync(e->vec_bad, 0, 3 * sizeof(u64), e->stream) != hipSuccess) rc = LOB_EHIP;
    if (rc == LOB_OK) { S.self = e->S_dev; memset(&e->S_pushed, 0xff, sizeof(DevState)); }
    if (rc == LOB_OK) rc = push_params(e);
    if (rc != LOB_OK) { lob_destroy(e); return rc; }
    // the two rl::State objects start with constructor zeros (src/rl/state.cpp:10-19)
    {
        std::vector<f64> neg1(B, -1.0);
        HIPCHK_E(hipMemcpyAsync(S.tp_val, neg1.data(), B * sizeof(f64), hipMemcpyHostToDevice, e->stream));
        HIPCHK_E(hipStreamSynchronize(e->stream));
        std::vector<LHdr> hdr(B);
        memset(hdr.data(), 0, B * sizeof(LHdr));
        for (size_t b = 0; b < B; b++) hdr[b].zero_mask = 3;
        HIPCHK_E(hipMemcpyAsync(S.hdr, hdr.data(), B * sizeof(LHdr), hipMemcpyHostToDevice, e->stream));
        // hash table followed by the 27 trailing-coordinate (action code) terms
        // rndseq[(code + 449*(nf+1)) & 2047], code = group*9 + action (state.cpp:56-63, tiles.cpp:46,152-163)
        uint32_t rnd[2048 + 64];
        memset(rnd, 0, sizeof rnd);
        make_rndseq(rnd);
        // (reduced mod M: hash_UNH's single final reduction distributes over the sum)
        uint32_t* terms = rnd + 2048;
        std::vector<uint32_t> raw(rnd, rnd + 2048);  // the action terms below index the unreduced table
        for (int g = 0; g < 3; g++) {
            const int nf = g == 0 ? 3 : (g == 1 ? P.V - 3 : P.V);
            for (int a = 0; a < LOB_N_ACTIONS; a++)
                terms[g * LOB_N_ACTIONS + a] = (uint32_t)((uint64_t)raw[((g * LOB_N_ACTIONS + a) + 449 * (nf + 1)) & 2047] % (uint64_t)P.M);
        }
        memcpy(e->vec_terms, terms, sizeof e->vec_terms);
        for (int k = 0; k < 2048; k++) rnd[k] = (uint32_t)((uint64_t)rnd[k] % (uint64_t)P.M);  // the device only ever sums the table mod M
        HIPCHK_E(hipMemcpyAsync(e->rnd_dev, rnd, sizeof rnd, hipMemcpyHostToDevice, e->stream));
        HIPCHK_E(hipStreamSynchronize(e->stream));
    }
    if (P.algo == LOB_ALGO_DOUBLE_Q) {
        hipLaunchKernelGGL(mt_init_kernel, dim3(grid_lanes(e->B)), dim3(256), 0, e->stream, e->P, e->S);
        HIPCHK_E(hipGetLastError());
        HIPCHK_E(hipStreamSynchronize(e->stream));
    }
#undef HIPCHK_E
    if (p->random_init) {
        const int rc_init = theta_random_init(e);
        if (rc_init != LOB_OK) { lob_destroy(e); return rc_init; }
    }
    *out = e;
    return LOB_OK;
}

void lob_destroy(lob_engine* e) {
    if (!e) return;
    hipSetDevice(e->device);
    if (e->stage_thread.joinable()) e->stage_thread.join();
    if (e->stream_up) { hipStreamSynchronize(e->stream_up); hipStreamDestroy(e->stream_up); }
    if (e->records_next) hipFree(e->records_next);
    if (e->stream2) hipStreamSynchronize(e->stream2);
    if (e->stream) hipStreamSynchronize(e->stream);
    drain_timers(e);
    if (e->ev_fork) hipEventDestroy(e->ev_fork);
    if (e->ev_join) hipEventDestroy(e->ev_join);
    if (e->ev_stagger) hipEventDestroy(e->ev_stagger);
    if (e->rest_hint) hipHostFree(e->rest_hint);
    for (int i = 0; i < LOB_HINT_RING; i++) if (e->hint_ev[i]) hipEventDestroy(e->hint_ev[i]);
    if (e->ev_rest_go) hipEventDestroy(e->ev_rest_go);
    if (e->ev_rest_done) hipEventDestroy(e->ev_rest_done);
    if (e->stream2) hipStreamDestroy(e->stream2);
    for (auto ev : e->event_pool) hipEventDestroy(ev);
    for (void* p : e->allocs) hipFree(p);
    if (e->records_dev) hipFree(e->records_dev);
    if (e->phase_dev) hipFree(e->phase_dev);
    free_days(e);
    if (e->track_dev) hipFree(e->track_dev);
    e->dump.release();
    e->stats.release();
    step_log_free(e);
    e->slog_stage.release();
    for (auto& b : e->snap_buf) b.release();
    if (e->snap_tab) hipFree(e->snap_tab);
    e->roll_ws.release();
    for (auto& b : e->branch_buf) b.release();
    e->spx_gather.release();
    if (e->spx_ev) hipEventDestroy(e->spx_ev);
    if (e->spx_total_host) hipHostFree(e->spx_total_host);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
}

// learning.random_init (src/rl/agent.cpp:37-39, DoubleAgent: 190-192): generate(&theta[0], &theta[M], 2.0 * unif_dist(gen) - 1.0)
// with the agent's own std::mt19937_64 -- theta first, then theta_b, and the generator goes on to toss DoubleQLearn's coin from
// where the initialisation left it.  Done on the host (a sequential generator: 20 M draws take a tenth of a second, once per
// engine) with the same restatement of the generator the device uses for the coin (lob_learn.h), loaded through lob_theta_set
// (maps, memo records).  Private theta: every book's agent draws its own vectors.  Shared theta: global book 0's agent draws the
// one vector, on every shard the same; its generator's new state is installed where that book lives (book_id_offset == 0).
struct HostMt64 {
    u64 x[LOB_MT_N];
    int idx;
    explicit HostMt64(u64 seed) { mt64_seed(x, seed); idx = LOB_MT_N; }
    u64 draw() {
        if (idx >= LOB_MT_N) {  // the sequential in-place twist (the device does the same block in three phases, mt64_twist_wave)
            for (int i = 0; i < LOB_MT_N; i++) x[i] = mt64_mix(x[i], x[(i + 1) % LOB_MT_N], x[(i + LOB_MT_M) % LOB_MT_N]);
            idx = 0;
        }
        return mt64_temper(x[idx++]);
    }
};
static int theta_random_init(lob_engine* e) {
    const bool priv = e->P.theta_private != 0, dq = e->P.algo == LOB_ALGO_DOUBLE_Q;
    const int nt = priv ? e->B : 1;
    std::vector<f64> v((size_t)e->P.M);
    for (int t = 0; t < nt; t++) {
        HostMt64 g((u64)(uint32_t)(e->P.seed + (priv ? e->P.book_id_offset + (u64)t : 0ull)));
        for (int vec = 0; vec < (dq ? 2 : 1); vec++) {
            for (size_t i = 0; i < v.size(); i++) v[i] = 2.0 * mt64_canonical(g.draw()) - 1.0;
            int rc = lob_theta_set(e, vec * nt + t, v.data(), (int64_t)e->P.M);
            if (rc) return rc;
        }
        if (dq && (priv || e->P.book_id_offset == 0)) {  // Agent::gen of the book whose agent has just drawn: where the coin continues
            const i32 idx = g.idx;
            HIPCHK(hipMemcpyAsync(e->S.mt_state + (size_t)t * LOB_MT_N, g.x, sizeof g.x, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(e->S.mt_idx + t, &idx, sizeof idx, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
        }
    }
    return LOB_OK;
}

int lob_reset(lob_engine* e) {
    if (!e) return LOB_EINVAL;
    if (!e->have_events) { lob_set_error("lob_reset: no event stream loaded"); return LOB_ESTATE; }
    if (e->lib && e->lib_cur < 0 && !e->lib_pending) { lob_set_error("lob_reset: no days selected from the library (lob_days_select / lob_days_set)"); return LOB_ESTATE; }
    HIPCHK(hipSetDevice(e->device));
    { int rc = finalize_episode(e); if (rc) return rc; }   // (the window sums of the episode that ends: on the stream it ran on)
    { int rc = stage_adopt(e); if (rc) return rc; }        // a stream handed over meanwhile (lob_stage_events) is this episode's
    if (e->lib_pending) {   // ... and so are the days selected meanwhile (lob_days_select / lob_days_set)
        e->lib_cur = e->lib_cur < 0 ? 0 : e->lib_cur ^ 1;
        e->lib_pending = false;
        e->S.rec_phase = e->lib_phase[e->lib_cur];
        e->S.rec_len = e->lib_len[e->lib_cur];
    }
    { int rc = sync_state(e); if (rc) return rc; }
    // the memo table starts empty every episode (reset_kernel voids every book's slot)
    HIPCHK(hipMemsetAsync(e->S.mk_hash, 0xff, (size_t)e->S.mk_slots * 8, e->stream));
    HIPCHK(hipMemsetAsync(e->S.mk_tiles_ok, 0, (size_t)e->S.mk_slots * 4, e->stream));
    HIPCHK(hipMemsetAsync(e->S.mk_marked, 0, (size_t)e->S.mk_slots * 4, e->stream));
    // ... and so do its lists: a lob_theta_set / lob_delta_apply between this reset and the first step runs
    // memo_kernel over the `last_par` list, which must not hold the slots of the episode before (their hashes
    // are gone: re-stamping mk_tiles_ok for a stale triple would hand a later claimant of the slot the wrong tiles)
    HIPCHK(hipMemsetAsync(e->S.mk_count, 0, 2 * sizeof(i32), e->stream));
    HIPCHK(hipMemsetAsync(e->S.mk_markcount, 0, sizeof(i32), e->stream));
    // ... and the step's work lists (nothing is pending across a reset; a step abandoned after its first half -- below -- has
    // left its act list's count behind)
    HIPCHK(hipMemsetAsync(e->S.slow_n, 0, 4 * sizeof(i32), e->stream));
    HIPCHK(hipMemsetAsync(e->S.tr_list_n, 0, 2 * sizeof(i32), e->stream));
    HIPCHK(hipMemsetAsync(e->S.tr_list2_n, 0, 2 * sizeof(i32), e->stream));
    HIPCHK(hipMemsetAsync(e->S.acc_list_n, 0, 2 * sizeof(i32), e->stream));
    HIPCHK(hipMemsetAsync(e->S.acc_pend, 0, (size_t)e->B, e->stream));
    if (e->S.dir_list_n) HIPCHK(hipMemsetAsync(e->S.dir_list_n, 0, 2 * sizeof(i32), e->stream));
    HIPCHK(hipMemsetAsync(e->vec_bad, 0, 3 * sizeof(u64), e->stream));   // (lob_vec_step's count of bad actions starts again, and the look-aheads' two)
    if (e->slog_n) {   // the step log holds the episode that starts here (its rows need no clearing: the counts say which exist)
        HIPCHK(hipMemsetAsync(e->slog_cnt, 0, 2 * (size_t)e->slog_n * sizeof(i32), e->stream));
        e->slog_armed = true;
    }
    if (e->half_open) {
        // a step abandoned between lob_td_step_begin and lob_td_step_end (a weight exchange that failed): its learner half never
        // ran, so the double-buffered lists are where the step found them -- the survivors of the combine table wait in the
        // abandoned step's parity, not the next one's.  The next step takes that parity again.
        e->td_parity ^= 1;
        e->list_par ^= 1;
    }
    if (e->P.sarsa_lanes) {
        // ... and the tile registry with it; the generations that still name a slot of the old table carry the old epoch
        HIPCHK(hipMemsetAsync(e->S.ow_tab, 0xff, (size_t)e->S.ow_slots * 8, e->stream));
        HIPCHK(hipMemsetAsync(e->S.amb_bits, 0, ((size_t)e->P.M / 32 + 1) * 4, e->stream));
        HIPCHK(hipMemsetAsync(e->S.amb_new_n, 0, 2 * sizeof(i32), e->stream));
        e->reg_apar = 0;
        HIPCHK(hipMemsetAsync(e->S.amb_flag, 0, sizeof(i32), e->stream));
        HIPCHK(hipMemsetAsync(e->S.mk_all_n, 0, sizeof(i32), e->stream));
        HIPCHK(hipMemsetAsync(e->S.tr_cbslot, 0xff, (size_t)e->B * e->P.trace_gens * 4, e->stream));  // (slots of books that stopped stepping may be gone)
        if (e->S.tr_cbd) HIPCHK(hipMemsetAsync(e->S.tr_cbd, 0xff, (size_t)e->B * e->P.trace_gens * 8, e->stream));
        hipLaunchKernelGGL(counters_zero_kernel, dim3(1), dim3(LOB_CNT_STRIPES), 0, e->stream, +e->S.counters, 7);
        e->P.epi_epoch++;
        { int rc = push_params(e); if (rc) return rc; }
    }
    {
        TimedLaunch t(e, "reset_kernel", nullptr, true);
        // (a ring: never the two-wave form, which cannot follow a warm-up beyond the ring's first fill -- lob_kernels.h reset2_kernel)
        lobk_reset(e->stream, e->sw.reset_lanes, e->P.T <= 2, e->sw.prepass_roles && !e->chunked, (const DevParams*)e->P_dev, e->S);
    }
    HIPCHK(hipGetLastError());
    e->was_reset = true;
    e->episode_open = true;
    e->steps_since_fill = 0;
    e->hits_ok = false;
    e->hint_step = 0;   // (the hand-back counts of the episode before say nothing about this one's first steps)
    e->rest_recent = 0;
    e->half_open = false;  // (a step begun before the reset -- e.g. an exchange that failed between the halves -- is abandoned with the episode)
    for (bool& v : e->snap_valid) v = false;   // a snapshot belongs to the episode it was taken in (the buffers stay)
    e->branch_live = false;                    // ... and so does a branch set
    e->restored = false;
    return check_device_errors(e);
}


// One env-step of every book (run_steps).  The books are split into EnginePlan::groups contiguous groups, each running its action
// half (act -> env) and its learn half (memo, traces, TD errors) on its own stream; both groups only READ theta, so the
// synchronous-batch semantic is unchanged.  The update of all books runs on the main stream after both groups have joined.
// The choices of one step, made at the top of each call (plan_step): when a step is split in two calls, the second makes them
// again (lob_set_epsilon may come between the halves), and what the first half read for the second stays engine state (hint_now).
struct StepPlan {
    bool first, second;     // the call runs the action half / the learn half and the update
    int mode;               // 0 learner, 1 backtester (lob_eval_step)
    bool learner, fast;     // mode 0; the memo + fast kernels (P.memo: one book group)
    int par, lpar;          // parity of the verdict carry-over lists (lob_state.h) / of the fast path's work lists
    u64 ver;                // theta version the step's memo records are computed under
    bool acc_blocked, dense_on;  // the update sums per block (the books keep many generations), by the slots' dense ids
    int acc_shift;          // accumulate_kernel's lanes per book (log2)
    bool fused_act, mostly_general, inline_general;  // the action selection inside the env kernel; the books without a usable hit
                                                     // list through the work list to the act kernel / served in-kernel
    bool acc_fused;         // updates added to their slots by the learn / trace kernels, accumulate_kernel over the list they leave
    bool rest_merged;       // ... and trace_rest_kernel instead of learn_q_rest_kernel + trace_fast_kernel<., 2> + accumulate_kernel over it
    bool rest_side;         // learn_q_rest_kernel on the second stream beside the trace kernels
    bool registered;        // trace_lane_kernel carries the tile registry's blocks (apply_kernel then carries the scan's)
};

// One book group's share of a step: books [b0, b0 + nb) on `st`
struct StepGroup {
    int g, b0, nb;
    hipStream_t st;
    int gw, gf, gl;   // grids: a wave per book; the persistent kernels (one 16-wave block per CU); the general kernels over a work list
};
static StepGroup step_group(const lob_engine* e, int g, int G) {
    const int b0 = (int)((long long)e->B * g / G), nb = (int)((long long)e->B * (g + 1) / G) - b0;
    return {g, b0, nb, g == 0 ? e->stream : e->stream2, grid_waves(nb),
            std::min(e->n_cus, (nb + LOB_FAST_WAVES * LOB_FAST_NB - 1) / (LOB_FAST_WAVES * LOB_FAST_NB)), 2 * e->n_cus};
}

// The learn kernels' hand-back count of LOB_HINT_LAG learner steps ago (0 until that many have run since the hints were void)
static int read_hint(lob_engine* e, const StepPlan& sp) {
    e->hint_now = 0;
    if (!(sp.fast && sp.learner && e->rest_hint && e->hint_step >= LOB_HINT_LAG)) return LOB_OK;
    // (the latest reporting step that is at least LOB_HINT_LAG steps old)
    const int hs = (int)(((e->hint_step - LOB_HINT_LAG) / LOB_HINT_EVERY * LOB_HINT_EVERY) % LOB_HINT_RING);
    HIPCHK(hipEventSynchronize(e->hint_ev[hs]));
    // (the kernel is done; its store to host memory is a system-scope atomic and carries the launch's tag: wait for that very word)
    u64 w = *(volatile u64*)(e->rest_hint + hs);
    for (int spin = 0; (uint32_t)(w >> 32) != e->hint_tags[hs] && spin < (1 << 16); spin++) w = *(volatile u64*)(e->rest_hint + hs);
    // The count only chooses between two correct paths: a word that has still not arrived (a loaded host, a slow link)
    // is no reason to abort training -- this step goes by "no book handed back" (ADVICE r5), and is counted
    // (lob_debug_hint: a test that asserts which path ran must know that the hint decided it)
    const bool arrived = (uint32_t)(w >> 32) == e->hint_tags[hs];
    e->hint_now = arrived ? (int)(uint32_t)w : 0;
    e->hint_reads++;
    if (!arrived) e->hint_misses++;
    return LOB_OK;
}

// A launch of the kernel that reports the hand-back count to the host (learn_q_rest_kernel, or trace_rest_kernel in the merged
// flow): `launch(hint_dev, hint_tag)`.  Every LOB_HINT_EVERY-th stores it to its ring word, with an event recorded behind it.
extern "C++" template <class Launch> static int report_hint(lob_engine* e, hipStream_t st, Launch launch) {
    const bool on = e->rest_hint && !e->sw.no_hint;  // (LOB_NO_HINT, experiment: the store to host memory costs the kernel 3.5 us and the step nothing)
    const int hs = (int)(e->hint_step % LOB_HINT_RING);
    const bool reports = on && e->hint_step % LOB_HINT_EVERY == 0;
    const uint32_t hint_tag = (uint32_t)(++e->hint_serial);
    launch(reports ? e->rest_hint_dev + hs : (u64*)nullptr, hint_tag);
    if (reports) { HIPCHK(hipEventRecord(e->hint_ev[hs], st)); e->hint_tags[hs] = hint_tag; }
    if (on) e->hint_step++;
    return LOB_OK;
}

static int plan_step(lob_engine* e, int mode, int half, StepPlan& sp) {
    const EnginePlan& pl = e->plan;
    sp = StepPlan{};
    sp.first = half != 2; sp.second = half != 1;
    sp.mode = mode; sp.learner = mode == 0;
    sp.fast = e->P.memo != 0;
    sp.par = sp.learner ? (sp.first ? (e->td_parity ^= 1) : e->td_parity) : 0;
    if (sp.first) e->step_id++;
    if (!e->hits_ok) e->steps_on_lists = 0;
    sp.ver = (u64)e->theta_ver;
    if (sp.first) { const int rc = read_hint(e, sp); if (rc) return rc; }
    sp.lpar = sp.first ? (e->list_par ^= 1) : e->list_par;
    e->last_par = sp.par;
    // SARSA(lambda): every book keeps all its generations -- sums per slot inside 1 024-book blocks first (accumulate_block_kernel).
    // The same for Q(lambda) once most actions are greedy (P(greedy) = 1 - eps + eps / 9 > 0.7: more than three live generations per book)
    const bool greedy = e->P.policy == LOB_POLICY_EPS_GREEDY && e->P.epsilon < 0.34;
    sp.acc_blocked = pl.acc_block_ok && (e->P.algo == LOB_ALGO_SARSA || (e->P.algo == LOB_ALGO_QLAMBDA && greedy));
    sp.dense_on = e->S.cb_dense && sp.acc_blocked;
    // accumulate_kernel's lanes per book (log2): one lane per trace generation.  Two books per wave measured best for both SARSA(lambda)
    // (all trace_kmax generations alive) and Watkins's Q(lambda) at eps = 0.8 (1-2 alive; 8 lanes per book: 0.035 ms, 16: 0.030, 32: 0.029,
    // 64: 0.036); 64 lanes for SARSA(lambda) with a copy of the sums per XCD (0.096 ms, 32 lanes 0.101) and while mostly greedy
    sp.acc_shift = e->sw.acc_shift >= 0 ? e->sw.acc_shift : (e->P.algo == LOB_ALGO_SARSA && e->S.cb_reps > 1) || greedy ? 6 : 5;
    if (sp.first) {
        sp.fused_act = sp.fast && sp.learner && e->hits_ok && pl.fused_act_ok;
        // env_step_kernel serves the books without a usable hit list itself (act_book in-kernel) -- except in the first step on
        // lists after they were void, when a late map bit of the step before has voided them again and EVERY book takes the
        // general path: that step goes through the work list to the general act kernel and env_kernel<64, 2, 2> (either version
        // is correct for any step).  ... and while MOST books have no usable list (a dense weight vector -- learning.random_init,
        // a loaded checkpoint: every tile lies on a written weight and no list fits a record): one wave per book in the general
        // act kernel is far better than a 64-lane wave going through its books one at a time.  The learn kernels hand the same
        // books back: their list's length of LOB_HINT_LAG steps ago (lob_engine::rest_hint) tells.
        sp.mostly_general = e->sw.force_general >= 0 ? e->sw.force_general == 1 : e->hint_now > e->B / 16;
        sp.inline_general = pl.inline_ok && e->steps_on_lists >= 1 && !sp.mostly_general;
        if (sp.fused_act) e->steps_on_lists++;
    }
    if (sp.second && sp.learner && sp.fast) {
        // (not while the learn kernel hands most books back -- a dense theta: every one of them would go on the list through one counter)
        sp.acc_fused = pl.acc_fuse_ok && !sp.acc_blocked && e->hint_now <= std::max(1024, e->B / 16);
        sp.rest_merged = sp.acc_fused && e->sw.rest_merge;
        if (!sp.rest_merged) {
            // learn_q_rest_kernel beside the trace kernels: worth it only while books ARE handed back -- an empty launch is
            // cheaper than the two cross-stream waits
            if (e->hint_now > 0) e->rest_recent = 64;
            else if (e->rest_recent > 0) e->rest_recent--;
            sp.rest_side = pl.rest_side_ok && e->rest_recent > 0;
        }
    }
    sp.registered = sp.second && sp.learner && e->P.sarsa_lanes;
    return LOB_OK;
}

// lob_debug_flow, from the step's plan.  Each half counts what it launches: a step abandoned after its first half has counted
// one of [4]-[6] and nothing else.
static void count_flow(lob_engine* e, const StepPlan& sp, int half) {
    if (half == 1) { e->flow[sp.inline_general ? 4 : sp.mostly_general ? 5 : 6]++; return; }
    e->flow[sp.acc_blocked ? 2 : sp.acc_fused ? 0 : 3]++;
    if (sp.dense_on) e->flow[7]++;
    if (sp.rest_side) e->flow[1]++;
}

// The step words in the host's DevState (cb_par, cb_dense_on; in both halves of a split step).  Slots claimed from here on take
// a dense id while the update sums per block.  The generations' records of their slots' ids (tr_cbd) are only kept up by
// accumulate_dense_kernel: whenever the mode comes on (epsilon has fallen below 0.34, lob_set_epsilon), every record is void --
// the kernels that verified slots meanwhile did not look ids up.  The backtester leaves cb_par as it is.
static int set_step_words(lob_engine* e, const StepPlan& sp) {
    if (sp.learner) e->S.cb_par = sp.par;
    if (sp.dense_on) e->dense_ever = true;
    if (sp.dense_on && !e->S.cb_dense_on) HIPCHK(hipMemsetAsync(e->S.tr_cbd, 0xff, (size_t)e->B * e->P.trace_gens * 8, e->stream));
    e->S.cb_dense_on = sp.dense_on;
    return LOB_OK;
}
// ... and the rule that gets them to the claims.  The claims read both words through the device-resident state (cb_claim_finish,
// lob_learn.h: S.self), which sync_state uploads with both at 0.  So in every learner step that claims combine slots, memo_kernel
// (`which` 0) or step_words_kernel publishes them before any claim: this launch, the first of the learn half.
static void publish_step_words(lob_engine* e, const StepPlan& sp, hipStream_t st) {
    if (sp.fast) launch_memo(e, sp.par, sp.learner ? 0 : 1);  // (learner: S0 under theta_t for the learn kernels; backtester: for the next act)
    else if (sp.learner && e->P.combine) hipLaunchKernelGGL(step_words_kernel, dim3(1), dim3(1), 0, st, e->S_dev, e->S.cb_par, e->S.cb_dense_on);
}

// The action half of one group: action selection + performAction
static int act_half(lob_engine* e, const StepPlan& sp, const StepGroup& gr, int G) {
    const hipStream_t st = gr.st;
    const uint32_t* rnd = (const uint32_t*)e->rnd_dev;
    const bool dq = e->P.algo == LOB_ALGO_DOUBLE_Q;  // (fast && dq: every step without usable hit lists takes the general act kernel over the whole batch)
    const i32* act_list = e->S.slow_list, *act_n = e->S.slow_n + sp.lpar * 2;
    // stagger: group 1 starts acting when group 0 has finished acting, so that the
    // latency-bound env kernel of one group runs beside a gather kernel of the other
    if (G > 1 && gr.g == 1) HIPCHK(hipStreamWaitEvent(st, e->ev_stagger, 0));
    if (sp.fused_act) {
        // The action selection inside the env kernel: env_step_kernel (two trade slots; LOB_ENV_STEP=0: env_kernel<64, 2, 1>),
        // then, unless it served them itself, the general act kernel for the books it left on the work list and their steps
        // (env_kernel<64, TM, 2>)
        count_flow(e, sp, 1);
        const DevParams* Pd = (const DevParams*)e->P_dev;
        const bool t2 = e->P.T <= 2;
        const int nb = e->B, sid = e->step_id;
        const EnvFuse F1{nullptr, nullptr, sp.lpar, sid - 1, sp.ver}, F2{act_list, act_n, sp.lpar, sid - 1, sp.ver};
        {
            TimedLaunch t(e, "env_kernel", st);
            if (e->plan.env_step) e->launched[lobk_env_step(st, sp.inline_general, dq, e->plan.half_waves, e->plan.env16, Pd, e->S, nb, sid, sp.par, F1, rnd)]++;
            else { e->launched[2]++; lobk_env_mode(st, t2, 1, Pd, e->S, nb, sid, sp.par, F1); }
        }
        if (!sp.inline_general) {
            {
                TimedLaunch t(e, "act_rest_kernel", st);
                if (dq) hipLaunchKernelGGL((act_kernel<LOB_ALGO_DOUBLE_Q, true>), dim3(gr.gl), dim3(LOB_BLOCK), 0, st, LOB_PS(e), rnd, 0, 0, e->B, sp.par, act_list, act_n);
                else hipLaunchKernelGGL((act_kernel<LOB_ALGO_SARSA, true>), dim3(gr.gl), dim3(LOB_BLOCK), 0, st, LOB_PS(e), rnd, 0, 0, e->B, sp.par, act_list, act_n);
            }
            TimedLaunch t(e, "env_rest_kernel", st);
            lobk_env_mode(st, t2, 2, Pd, e->S, nb, sid, sp.par, F2);
        }
    } else if (sp.fast && !dq) {
        {
            TimedLaunch t(e, "act_kernel", st);
            if (sp.learner && e->hits_ok && e->sw.light)
                hipLaunchKernelGGL(act_light_kernel, dim3((gr.nb + LOB_LIGHT_BLOCK - 1) / LOB_LIGHT_BLOCK), dim3(LOB_LIGHT_BLOCK), 0, st, LOB_PS(e), sp.par, sp.lpar, sp.ver, e->step_id - 1);
            else
                hipLaunchKernelGGL(act_fast_kernel<LOB_FAST_NB>, dim3(gr.gf), dim3(LOB_FAST_BLOCK), fast_lds_bytes(e->P.cwords4, LOB_FAST_NB, false), st, LOB_PS(e), rnd, sp.mode, sp.par, sp.lpar, sp.ver);
        }
        TimedLaunch t(e, "act_rest_kernel", st);
        hipLaunchKernelGGL((act_kernel<LOB_ALGO_SARSA, true>), dim3(gr.gl), dim3(LOB_BLOCK), 0, st, LOB_PS(e), rnd, sp.mode, 0, e->B, sp.par, act_list, act_n);
    } else {
        TimedLaunch t(e, "act_kernel", st);
        if (dq) hipLaunchKernelGGL((act_kernel<LOB_ALGO_DOUBLE_Q, false>), dim3(gr.gw), dim3(LOB_BLOCK), 0, st, LOB_PS(e), rnd, sp.mode, gr.b0, gr.nb, sp.par, (const i32*)nullptr, (const i32*)nullptr);
        else hipLaunchKernelGGL((act_kernel<LOB_ALGO_SARSA, false>), dim3(gr.gw), dim3(LOB_BLOCK), 0, st, LOB_PS(e), rnd, sp.mode, gr.b0, gr.nb, sp.par, (const i32*)nullptr, (const i32*)nullptr);
    }
    if (G > 1 && gr.g == 0) HIPCHK(hipEventRecord(e->ev_stagger, st));
    if (!sp.fused_act) {
        TimedLaunch t(e, "env_kernel", st);
        launch_env(e, st, (const i32*)nullptr, sp.learner ? 1 : 0, gr.b0, gr.nb, sp.par);
    }
    return LOB_OK;
}

// The learn half of one group: the step words and memo, traces, TD errors
static int learn_half(lob_engine* e, const StepPlan& sp, const StepGroup& gr) {
    const hipStream_t st = gr.st;
    publish_step_words(e, sp, st);
    if (!sp.learner) return LOB_OK;
    const uint32_t* rnd = (const uint32_t*)e->rnd_dev;
    const int algo = e->P.algo, par = sp.par, lpar = sp.lpar, sid = e->step_id;
    const bool dq = algo == LOB_ALGO_DOUBLE_Q;
    if (!sp.fast) {
        TimedLaunch t(e, "learn_kernel", st);
        if (dq) hipLaunchKernelGGL((learn_kernel<LOB_ALGO_DOUBLE_Q, false>), dim3(gr.gw), dim3(LOB_BLOCK), 0, st, LOB_PS(e), rnd, gr.b0, gr.nb, par, (const i32*)nullptr, (const i32*)nullptr);
        else if (algo == LOB_ALGO_QLAMBDA) hipLaunchKernelGGL((learn_kernel<LOB_ALGO_QLAMBDA, false>), dim3(gr.gw), dim3(LOB_BLOCK), 0, st, LOB_PS(e), rnd, gr.b0, gr.nb, par, (const i32*)nullptr, (const i32*)nullptr);
        else hipLaunchKernelGGL((learn_kernel<LOB_ALGO_SARSA, false>), dim3(gr.gw), dim3(LOB_BLOCK), 0, st, LOB_PS(e), rnd, gr.b0, gr.nb, par, (const i32*)nullptr, (const i32*)nullptr);
        return LOB_OK;
    }
    // (the tile registry's entries for the slots that were new in the step before -- the extra blocks of its trace_lane_kernel
    // and apply_kernel launches -- are read from here on: the dup flags by the light trace step, the rest by trace_lane_kernel)
    const EnginePlan& pl = e->plan;
    const int nb = gr.nb;
    const i32* learn_list = e->S.slow_list + e->B, *learn_n = e->S.slow_n + lpar * 2 + 1;
    const int acc_fuse = sp.acc_fused ? (sp.rest_merged ? 2 : 1) : 0;
    const int gt = std::min((4 * LOB_TRACE_OCC / LOB_TRACE_WAVES) * e->n_cus, (nb + LOB_TRACE_WAVES - 1) / LOB_TRACE_WAVES);
    if (pl.t_light && !pl.fuse) {
        // a lane per book where the step leaves no older generation behind, the wave-per-book kernel for the rest
        TimedLaunch t(e, "trace_light_kernel", st);
        hipLaunchKernelGGL(trace_light_kernel, dim3((nb + LOB_LIGHT_BLOCK - 1) / LOB_LIGHT_BLOCK), dim3(LOB_LIGHT_BLOCK), 0, st, LOB_PS(e), lpar);
    }
    auto launch_traces = [&]() {
        if (pl.fuse) return;
        TimedLaunch t(e, "trace_kernel", st);
        if (pl.t_light) hipLaunchKernelGGL((trace_fast_kernel<LOB_ALGO_QLAMBDA, 1>), dim3(gt), dim3(LOB_TRACE_BLOCK), trace_lds_bytes(), st, LOB_PS(e), rnd, par, lpar, sid);
        else if (algo == LOB_ALGO_QLAMBDA) hipLaunchKernelGGL((trace_fast_kernel<LOB_ALGO_QLAMBDA, 0>), dim3(gt), dim3(LOB_TRACE_BLOCK), trace_lds_bytes(), st, LOB_PS(e), rnd, par, lpar, sid);
        else if (e->P.sarsa_lanes) {
            // a lane per generation; the wave-per-book kernel for the books it leaves on the list
            // (LOB_TS_GRID / LOB_TS_LDS, experiments: fewer, persistent blocks / dynamic LDS to throttle the occupancy -- halving
            // it costs 28 %, a persistent grid changes nothing: NOTES.md "Round 5")
            const int ts_full = (nb + LOB_TS_BLOCK / 32 - 1) / (LOB_TS_BLOCK / 32);
            // (its first LOB_REG_BLOCKS blocks: the tile registry for the memo slots that are new on this step's list)
            hipLaunchKernelGGL(trace_lane_kernel<LOB_ALGO_SARSA>, dim3((e->sw.ts_grid > 0 ? std::min(e->sw.ts_grid, ts_full) : ts_full) + LOB_REG_BLOCKS), dim3(LOB_TS_BLOCK), e->sw.ts_lds, st,
                               LOB_PS(e), lpar, sid, 0, rnd, par, e->reg_apar, LOB_REG_BLOCKS);
            hipLaunchKernelGGL((trace_fast_kernel<LOB_ALGO_SARSA, 1>), dim3(gt), dim3(LOB_TRACE_BLOCK), trace_lds_bytes(), st, LOB_PS(e), rnd, par, lpar, sid);
        }
        else hipLaunchKernelGGL((trace_fast_kernel<LOB_ALGO_SARSA, 0>), dim3(gt), dim3(LOB_TRACE_BLOCK), trace_lds_bytes(), st, LOB_PS(e), rnd, par, lpar, sid);
    };
    // (SARSA(lambda)'s trace kernels run IN FRONT OF its learn kernels: they mark the new generation's tiles in the
    // written-weights maps the learn kernels build the hit lists by -- lob_state.h above hl_rec.  The other order exists in
    // -DLOB_EXPERIMENTS builds only (LOB_SARSA_LEARN_FIRST=1), for the test that shows it to fail.)
    if (!pl.learn_first) launch_traces();
    {
        TimedLaunch t(e, "learn_kernel", st);
        if (pl.q_lanes) {
            const bool pair = pl.q_pair;
            if (pair && !e->S.theta_nzm) { lob_set_error("learn_q_pair_kernel: no action-mask table (theta_nzm)"); return LOB_ESTATE; }
            e->launched[pair ? 3 : 4]++;
            const int gq = pair ? std::min(LOB_QP_OCC * e->n_cus, (nb + LOB_QP_BOOKS - 1) / LOB_QP_BOOKS) : std::min(e->n_cus, (nb + LOB_QL_BLOCK - 1) / LOB_QL_BLOCK);
            const size_t lds = pair ? qpair_lds_bytes(e->P.cwords4) : qlane_lds_bytes(e->P.cwords4);
            lobk_learn_q(st, pair, algo, e->P.V == 8, pl.fuse, gq, lds, (const DevParams*)e->P_dev, e->S, rnd, lpar, sp.ver, sid, acc_fuse);
        } else {
            e->launched[5]++;
            lobk_learn_q_fast(st, algo, gr.gf, fast_lds_bytes(e->P.cwords4, LOB_FAST_NB, false), (const DevParams*)e->P_dev, e->S, rnd, lpar, sp.ver);
        }
    }
    if (!sp.rest_merged) {   // (rest_merged: trace_rest_kernel serves the books handed back too, behind the lane trace kernel)
        // The books the lane kernels hand back (a list that is empty in most steps, a handful of books in the others).
        // When trace kernels follow on the main stream (the fused Q(lambda) / double Q flow), this launch may run beside
        // them on the second stream (StepPlan::rest_side): nothing they do depends on it -- the update kernels wait for both.
        const hipStream_t rs = sp.rest_side ? e->stream2 : st;
        if (sp.rest_side) {
            HIPCHK(hipEventRecord(e->ev_rest_go, st));
            HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_rest_go, 0));
        }
        {
            TimedLaunch t(e, "learn_rest_kernel", rs);
            const int rc = report_hint(e, rs, [&](u64* hint_dev, uint32_t hint_tag) {
                if (dq) hipLaunchKernelGGL(learn_q_rest_kernel<LOB_ALGO_DOUBLE_Q>, dim3(gr.gl), dim3(LOB_BLOCK), 0, rs, LOB_PS(e), rnd, learn_list, learn_n, hint_dev, hint_tag);
                else if (algo == LOB_ALGO_QLAMBDA) hipLaunchKernelGGL(learn_q_rest_kernel<LOB_ALGO_QLAMBDA>, dim3(gr.gl), dim3(LOB_BLOCK), 0, rs, LOB_PS(e), rnd, learn_list, learn_n, hint_dev, hint_tag);
                else hipLaunchKernelGGL(learn_q_rest_kernel<LOB_ALGO_SARSA>, dim3(gr.gl), dim3(LOB_BLOCK), 0, rs, LOB_PS(e), rnd, learn_list, learn_n, hint_dev, hint_tag);
            });
            if (rc) return rc;
        }
        if (sp.rest_side) HIPCHK(hipEventRecord(e->ev_rest_done, e->stream2));
    }
    if (pl.learn_first) launch_traces();
    if (pl.fuse) {
        TimedLaunch t(e, "trace_kernel", st);
        // the listed books (their traces survive the step): a lane per generation, then the wave-per-book kernel for
        // those the lane kernel hands on
        if (e->P.sarsa_lanes) {
            // (its first LOB_REG_BLOCKS blocks: the tile registry for the memo slots that are new on this step's list)
            hipLaunchKernelGGL(trace_lane_kernel<LOB_ALGO_QLAMBDA>, dim3(std::min(4 * e->n_cus, (nb + LOB_TS_BLOCK / 32 - 1) / (LOB_TS_BLOCK / 32)) + LOB_REG_BLOCKS), dim3(LOB_TS_BLOCK), 0, st,
                               LOB_PS(e), lpar, sid, acc_fuse, rnd, par, e->reg_apar, LOB_REG_BLOCKS);
        }
        // (rest_merged: what the lane kernel hands on is served by trace_rest_kernel, in the place of accumulate_kernel)
        if (!sp.rest_merged) hipLaunchKernelGGL((trace_fast_kernel<LOB_ALGO_QLAMBDA, 2>), dim3(gt), dim3(LOB_TRACE_BLOCK), trace_lds_bytes(), st, LOB_PS(e), rnd, par, lpar, sid);
    }
    return LOB_OK;
}

// The update of every book, on the main stream behind both groups (and the second stream)
static int update_all(lob_engine* e, const StepPlan& sp) {
    const uint32_t* rnd = (const uint32_t*)e->rnd_dev;
    const int par = sp.par, lpar = sp.lpar;
    if (sp.rest_side) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_rest_done, 0));
    // model_log: the step's |delta| sums, launched where every stepped book's TD error is final -- behind trace_rest_kernel in
    // the merged flow (a book the learn kernel handed back still carries Q(s, a) in LHdr::td until that kernel's learn_q_book
    // has run: ADVICE r5), in front of the update kernels everywhere else
    auto td_stats = [&]() {
        if (!(sp.learner && e->model_log)) return;
        TimedLaunch t(e, "td_stats_kernel");
        const int nblk = std::min(LOB_ML_BLOCKS, (e->B + 255) / 256), per = (e->B + nblk - 1) / nblk;
        hipLaunchKernelGGL(td_stats_kernel, dim3(nblk), dim3(256), 0, e->stream, e->S, per);
        hipLaunchKernelGGL(td_stats_fold_kernel, dim3(1), dim3(64), 0, e->stream, e->S, nblk);
    };
    if (!sp.rest_merged) td_stats();
    if (sp.learner && e->P.combine) {
        int dense_blocks = 0;
        {
            TimedLaunch t(e, "accumulate_kernel");
            count_flow(e, sp, 2);
            if (sp.dense_on) {
                // sums by the slots' dense ids in a direct-indexed LDS array, one block per CU (accumulate_dense_kernel)
                dense_blocks = std::min(std::min(e->n_cus, LOB_ACD_MAX_BLOCKS), (e->B + 127) / 128);   // (a block takes 128 books per pass)
                const int bpb = ((e->B + dense_blocks - 1) / dense_blocks + 31) / 32 * 32;
                dense_blocks = (e->B + bpb - 1) / bpb;
                hipLaunchKernelGGL(accumulate_dense_kernel, dim3(dense_blocks), dim3(LOB_ACD_BLOCK), acd_lds_bytes(), e->stream, LOB_PS(e), par, e->step_id, bpb);
                hipLaunchKernelGGL(reduce_dense_kernel, dim3((e->S.cb_ids + 255) / 256, LOB_ACD_GROUPS), dim3(256), 0, e->stream, e->S, dense_blocks);
            } else if (sp.acc_blocked) {
                // (batches per block: SARSA(lambda) 80 us with one, 89 with two or four -- its blocks are bound by their LDS insertions, not by what
                // they send to memory; mostly-greedy Q(lambda) 58 -> 50 us with four)
                const int nbat = e->sw.acc_batches ? e->sw.acc_batches : (e->P.algo == LOB_ALGO_SARSA ? 1 : std::max(1, std::min(LOB_ACB_K, e->B / (16 * LOB_ACB_BLOCK))));
                hipLaunchKernelGGL(accumulate_block_kernel, dim3((e->B + LOB_ACB_BLOCK * nbat - 1) / (LOB_ACB_BLOCK * nbat), e->P.trace_kmax), dim3(LOB_ACB_BLOCK), 0, e->stream, LOB_PS(e), par, e->step_id, nbat);
            } else if (sp.rest_merged) {
                // the books the learn kernel handed back (TD error + their sums), the books the lane trace kernel handed on (trace
                // step + their sums) and what the fused accumulation left, in one launch; it reports the hand-back count to the
                // host as learn_q_rest_kernel does in the other flows
                const dim3 rg(std::min(e->n_cus, (std::min(e->B, 4096) + LOB_TRACE_WAVES - 1) / LOB_TRACE_WAVES));
                const int rc = report_hint(e, e->stream, [&](u64* hint_dev, uint32_t hint_tag) {
                    if (e->P.algo == LOB_ALGO_DOUBLE_Q)
                        hipLaunchKernelGGL(trace_rest_kernel<LOB_ALGO_DOUBLE_Q>, rg, dim3(LOB_TRACE_BLOCK), trace_lds_bytes(), e->stream, LOB_PS(e), rnd, par, lpar, e->step_id, sp.acc_shift, hint_dev, hint_tag);
                    else
                        hipLaunchKernelGGL(trace_rest_kernel<LOB_ALGO_QLAMBDA>, rg, dim3(LOB_TRACE_BLOCK), trace_lds_bytes(), e->stream, LOB_PS(e), rnd, par, lpar, e->step_id, sp.acc_shift, hint_dev, hint_tag);
                });
                if (rc) return rc;
            } else if (sp.acc_fused) {
                // what the fused accumulation left: a few hundred books (the grid's waves stride over the list)
                const int waves = (std::min(e->B, 4096) + (64 >> sp.acc_shift) - 1) / (64 >> sp.acc_shift);
                hipLaunchKernelGGL(accumulate_kernel, dim3((waves + LOB_WAVES_PER_BLOCK - 1) / LOB_WAVES_PER_BLOCK), dim3(LOB_BLOCK), 0, e->stream, LOB_PS(e), par, sp.acc_shift, e->step_id,
                                   (const i32*)e->S.acc_list, (const i32*)&e->S.acc_list_n[lpar]);
            } else {
                const int waves = (e->B + (64 >> sp.acc_shift) - 1) / (64 >> sp.acc_shift);
                hipLaunchKernelGGL(accumulate_kernel, dim3((waves + LOB_WAVES_PER_BLOCK - 1) / LOB_WAVES_PER_BLOCK), dim3(LOB_BLOCK), 0, e->stream, LOB_PS(e), par, sp.acc_shift, e->step_id,
                                   (const i32*)nullptr, (const i32*)nullptr);
            }
        }
        if (sp.rest_merged) td_stats();
        {
            TimedLaunch t(e, "apply_kernel");
            const int blocks = e->S.cb_segs;
            // (dense_blocks -1: no slot has ever been given a dense id -- apply_kernel does not look any up)
            // (+ the indices the step's registry blocks -- trace_lane_kernel's launch -- found ambiguous, marked in every registered slot)
            hipLaunchKernelGGL(apply_kernel, dim3(blocks + (sp.registered ? LOB_SCAN_BLOCKS : 0)), dim3(256), 0, e->stream, LOB_PS(e), rnd, par, e->step_id,
                               e->dense_ever ? dense_blocks : -1, e->reg_apar);
            if (sp.registered) e->reg_apar ^= 1;
        }
    } else if (sp.learner) {
        TimedLaunch t(e, "update_kernel");
        hipLaunchKernelGGL(update_kernel, dim3(grid_waves(e->B)), dim3(LOB_BLOCK), 0, e->stream, LOB_PS(e), par, e->step_id);
    }
    if (sp.learner && e->P.r_learn) {
        // R-learning: the average reward rho, after updateQ (rho_kernel, lob_kernels.h)
        TimedLaunch t(e, "rho_kernel");
        const int nr = e->P.theta_private ? e->B : 1;
        hipLaunchKernelGGL(rho_kernel, dim3(grid_waves(e->B)), dim3(LOB_BLOCK), 0, e->stream, e->P, e->S, rnd);
        hipLaunchKernelGGL(rho_fold_kernel, dim3((nr + 255) / 256), dim3(256), 0, e->stream, e->S, nr);
    }
    if (sp.learner) {
        e->theta_ver++;                          // theta_{t+1}
        if (e->P.memo) launch_memo(e, par, 1, lpar);   // the same triples again, for the next action selection (+ its list resets)
    }
    e->hits_ok = sp.learner && sp.fast;          // learn_q_fast_kernel has left the hit lists of the States the next step acts on
    maybe_refill_track(e);
    return LOB_OK;
}

// `half`: 0 = whole steps; 1 = the first half of ONE learner step (action selection + performAction), 2 = its second half
// (memo, traces, TD errors, update) -- lob_td_step_begin / lob_td_step_end: a weight exchange fits between the two, where
// no hit list is live (the step's action has consumed the previous step's, the learn kernel builds the next under
// whatever maps it then finds).
static int run_steps(lob_engine* e, int32_t n_steps, int mode, int half = 0) {
    HIPCHK(hipSetDevice(e->device));
    { int rc = sync_state(e); if (rc) return rc; }
    const int G = e->plan.groups;
    for (int s = 0; s < n_steps; s++) {
        StepPlan sp;
        { int rc = plan_step(e, mode, half, sp); if (rc) return rc; }
        if (G > 1) {
            HIPCHK(hipEventRecord(e->ev_fork, e->stream));
            HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
        }
        { int rc = set_step_words(e, sp); if (rc) return rc; }
        for (int g = 0; g < G; g++) {
            const StepGroup gr = step_group(e, g, G);
            if (sp.first) { int rc = act_half(e, sp, gr, G); if (rc) return rc; }
            if (sp.second) { int rc = learn_half(e, sp, gr); if (rc) return rc; }
        }
        if (G > 1) {
            HIPCHK(hipEventRecord(e->ev_join, e->stream2));
            HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join, 0));
        }
        if (!sp.second) { e->half_open = true; continue; }
        e->half_open = false;
        { int rc = update_all(e, sp); if (rc) return rc; }
        launch_step_log(e);
    }
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

int lob_td_step(lob_engine* e, int32_t n_steps) {
    int rc = guard(e, "lob_td_step", RESET);
    if (rc) return rc;
    if (n_steps < 0) return LOB_EINVAL;
    if (e->half_open) { lob_set_error("lob_td_step: a step is half done (lob_td_step_begin without lob_td_step_end)"); return LOB_ESTATE; }
    LOB_GUARD(e, lob_td_step);
    return run_steps(e, n_steps, 0);
}
int lob_td_step_begin(lob_engine* e) {
    int rc = guard(e, "lob_td_step_begin", RESET);
    if (rc) return rc;
    if (e->half_open) { lob_set_error("lob_td_step_begin: the previous step has not been ended"); return LOB_ESTATE; }
    LOB_GUARD(e, lob_td_step_begin);
    if (e->plan.groups > 1) { lob_set_error("lob_td_step_begin: not with two book groups (LOB_GROUPS=2)"); return LOB_ESTATE; }
    return run_steps(e, 1, 0, 1);
}
int lob_td_split_supported(lob_engine* e) { return e && e->plan.groups == 1 ? 1 : 0; }
int lob_td_step_end(lob_engine* e) {
    int rc = guard(e, "lob_td_step_end", RESET);
    if (rc) return rc;
    if (!e->half_open) { lob_set_error("lob_td_step_end: no step begun"); return LOB_ESTATE; }
    return run_steps(e, 1, 0, 2);
}
int lob_eval_step(lob_engine* e, int32_t n_steps) {
    int rc = guard(e, "lob_eval_step", RESET);
    if (rc) return rc;
    if (n_steps < 0) return LOB_EINVAL;
    if (e->half_open) { lob_set_error("lob_eval_step: a learner step is half done"); return LOB_ESTATE; }
    LOB_GUARD(e, lob_eval_step);
    return run_steps(e, n_steps, 1);
}


int lob_handle_terminal(lob_engine* e) {
    if (!e) return LOB_EINVAL;
    LOB_GUARD(e, lob_handle_terminal);
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(clear_traces_kernel, dim3(grid_lanes(e->B)), dim3(256), 0, e->stream, e->S);
    HIPCHK(hipGetLastError());
    return LOB_OK;
}
int lob_set_alpha(lob_engine* e, double alpha) { if (!e) return LOB_EINVAL; e->P.alpha = alpha; e->params.alpha = alpha; hipSetDevice(e->device); return push_params(e); }
int lob_set_tau(lob_engine* e, double tau) { if (!e || !(tau > 0.0)) return LOB_EINVAL; e->P.tau = tau; e->params.tau = tau; hipSetDevice(e->device); return push_params(e); }
int lob_set_epsilon(lob_engine* e, double eps) { if (!e) return LOB_EINVAL; e->P.epsilon = eps; e->params.epsilon = eps; hipSetDevice(e->device); return push_params(e); }

static int features_impl(lob_engine* e, const float* host_vars, int32_t n, int32_t* out_idx, double* out_q) {
    if (!e || !host_vars || n < 1) { lob_set_error("lob_features: bad argument"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    DevTemp<f32> dv;
    DevTemp<i32> di;
    DevTemp<f64> dq;
    if (dv.alloc((size_t)n * e->P.V) || (out_idx && di.alloc((size_t)n * LOB_N_ACTIONS * 96)) || (out_q && dq.alloc((size_t)n * LOB_N_ACTIONS))) {
        lob_set_error("lob_features: no room for the rows' device buffers");
        return LOB_ENOMEM;
    }
    HIPCHK(hipMemcpyAsync(dv.p, host_vars, (size_t)n * e->P.V * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(features_kernel, dim3(grid_waves(n)), dim3(LOB_BLOCK), 0, e->stream, e->P, (const f64*)e->S.theta,
                       (const uint32_t*)e->S.theta_nz, (const uint32_t*)e->rnd_dev, (const f32*)dv.p, n, di.p, dq.p);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess && out_idx) err = hipMemcpyAsync(out_idx, di.p, (size_t)n * LOB_N_ACTIONS * 96 * 4, hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess && out_q) err = hipMemcpyAsync(out_q, dq.p, (size_t)n * LOB_N_ACTIONS * 8, hipMemcpyDeviceToHost, e->stream);
    hipStreamSynchronize(e->stream);   // (the buffers are freed behind it, on every way out)
    HIPCHK(err);
    return LOB_OK;
}
int lob_features(lob_engine* e, const float* host_vars, int32_t n, int32_t* host_out) { return features_impl(e, host_vars, n, host_out, nullptr); }
int lob_q_values(lob_engine* e, const float* host_vars, int32_t n, double* host_out) { return features_impl(e, host_vars, n, nullptr, host_out); }

// `which`: shared theta: 0 = theta, 1 = theta_b (double Q); private theta: book, or n_books + book for theta_b
static int theta_slot(lob_engine* e, int32_t which, f64** th, uint32_t** nz) {
    const int n = e->P.theta_private ? e->B : 1;
    const bool dq = e->P.algo == LOB_ALGO_DOUBLE_Q;
    if (which < 0 || which >= (dq ? 2 * n : n)) { lob_set_error("lob_theta_*: `which` out of range"); return LOB_EINVAL; }
    const bool second = which >= n;
    const int idx = second ? which - n : which;
    *th = (second ? e->S.theta_b : e->S.theta) + (size_t)idx * e->P.M;
    *nz = (second ? e->S.theta_b_nz : e->S.theta_nz) + (size_t)idx * LOB_NZ_NWORDS(e->P.M);
    return LOB_OK;
}
int lob_theta_get(lob_engine* e, int32_t which, double* host_out, int64_t count) {
    if (!e || !host_out || count < 0 || count > e->P.M) return LOB_EINVAL;
    f64* th; uint32_t* nz;
    int rc = theta_slot(e, which, &th, &nz);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(host_out, th, (size_t)count * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}
int lob_theta_set(lob_engine* e, int32_t which, const double* host_in, int64_t count) {
    if (!e || !host_in || count < 0 || count > e->P.M) return LOB_EINVAL;
    f64* th; uint32_t* nz;
    int rc = theta_slot(e, which, &th, &nz);
    if (rc) return rc;
    LOB_GUARD(e, lob_theta_set);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(th, host_in, (size_t)count * 8, hipMemcpyHostToDevice, e->stream));
    if (e->S.theta_sync) {
        // multi-GPU exchange already initialised: the loaded weights are the new common base, not a local
        // delta (every rank loads the same checkpoint); otherwise the next all-reduce would add
        // world_size x (loaded - sync)
        f64* sync = e->S.theta_sync + (th == e->S.theta_b ? (size_t)e->P.M : 0);
        HIPCHK(hipMemcpyAsync(sync, th, (size_t)count * 8, hipMemcpyDeviceToDevice, e->stream));
    }
    e->theta_ver++;  // memo records computed under the old weights are void
    e->hits_ok = false;
    e->hint_step = 0;  // (... and so is what the learn kernels handed back under them)
    e->rest_recent = 0;
    hipLaunchKernelGGL(rebuild_nz_kernel, dim3(1024), dim3(256), 0, e->stream, (const f64*)th, nz, e->S.nz_epoch, e->P.M);
    if (e->P.memo && (th == e->S.theta || th == e->S.theta_b)) {  // (double Q: one pair of maps for both vectors)
        // the maps keep the bits they have (monotone: the tiles of live trace generations stay marked, whatever the
        // loaded value of their weights -- a set bit only means "fetch the weight") and gain those of the loaded non-zeros
        hipLaunchKernelGGL(rebuild_nzx_kernel, dim3(2048), dim3(256), 0, e->stream, (const f64*)th, e->S.theta_nzx, e->S.theta_nzc, e->P.cshift, e->P.M);
        hipLaunchKernelGGL(rebuild_nzd_kernel, dim3(2048), dim3(256), 0, e->stream, (const uint32_t*)e->S.theta_nzx, e->S.theta_nzd, e->S.theta_nzm, e->S.nzd_terms, e->P.M);
        launch_memo(e, e->last_par, 1);  // the current triples under the loaded weights: the next act stays on the fast path
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}

static int fetch_hdr(lob_engine* e, std::vector<LHdr>& h) {
    h.resize(e->B);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(h.data(), e->S.hdr, (size_t)e->B * sizeof(LHdr), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}
#define HDR_GETTER(name, T, field)                                   \
    int name(lob_engine* e, T* host_out) {                           \
        if (!e || !host_out) return LOB_EINVAL;                      \
        std::vector<LHdr> h;                                         \
        int rc = fetch_hdr(e, h);                                    \
        if (rc) return rc;                                           \
        for (int b = 0; b < e->B; b++) host_out[b] = (T)h[b].field;  \
        return LOB_OK;                                               \
    }
HDR_GETTER(lob_get_last_actions, int32_t, action)
HDR_GETTER(lob_get_last_td, double, td)
HDR_GETTER(lob_get_last_rewards, double, reward)
HDR_GETTER(lob_get_stepped, int32_t, stepped)
HDR_GETTER(lob_get_rng_counters, uint64_t, rng_ctr)

/* current `state` variables of the learner (the rl::State the last step produced): float[B][n_vars] */
int lob_get_learner_state(lob_engine* e, float* host_out) {
    if (!e || !host_out) return LOB_EINVAL;
    std::vector<LHdr> h;
    int rc = fetch_hdr(e, h);
    if (rc) return rc;
    std::vector<f32> v((size_t)e->B * 48);
    HIPCHK(hipMemcpyAsync(v.data(), e->S.vars, v.size() * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int b = 0; b < e->B; b++)
        for (int i = 0; i < e->P.V; i++) host_out[(size_t)b * e->P.V + i] = v[((size_t)b * 3 + h[b].slot_cur) * 16 + i];
    return LOB_OK;
}

int lob_get_traces(lob_engine* e, int32_t book, int32_t* idx, float* elig, int32_t cap, int32_t* n) {
    if (!e || book < 0 || book >= e->B || !n) return LOB_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    const int G = e->P.trace_gens;
    std::vector<i32> ti((size_t)G * 32);
    std::vector<uint32_t> al(G);
    i32 head = 0, ng = 0;
    HIPCHK(hipMemcpyAsync(ti.data(), e->S.tr_idx + (size_t)book * G * 32, ti.size() * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(al.data(), e->S.tr_alive + (size_t)book * G, al.size() * 4, hipMemcpyDeviceToHost, e->stream));
    LHdr hb;
    HIPCHK(hipMemcpyAsync(&hb, e->S.hdr + book, sizeof hb, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    head = hb.tr_head;
    ng = hb.tr_n;
    int k = 0;
    for (int age = 0; age < ng; age++) {
        int slot = (head - age + G) & (G - 1);
        for (int j = 0; j < 32; j++)
            if ((al[slot] >> j) & 1u) {
                if (k < cap) {
                    if (idx) idx[k] = ti[slot * 32 + j];
                    if (elig) elig[k] = e->P.trace_pow[age];
                }
                k++;
            }
    }
    *n = k;
    return LOB_OK;
}

// the striped device counters, summed on the device, into c[16] (asynchronous: the caller synchronises the stream)
static int read_counters(lob_engine* e, i64* c) {
    hipLaunchKernelGGL(counters_fold_kernel, dim3(1), dim3(LOB_CNT_STRIPES), 0, e->stream, (const i64*)e->S.counters, e->cnt_sum, (const i32*)e->S.done, e->B);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c, e->cnt_sum, 16 * sizeof(i64), hipMemcpyDeviceToHost, e->stream));
    return LOB_OK;
}

int lob_get_counters(lob_engine* e, int64_t out[4]) {
    if (!e || !out) return LOB_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    i64 c[16];
    { int rc = read_counters(e, c); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(e->stream));
    out[0] = c[0]; out[1] = c[1]; out[2] = c[15]; out[3] = c[3];   // ([15]: the live books, counted by the fold kernel)
    return LOB_OK;
}

int lob_get_path_stats(lob_engine* e, int64_t out[8]) {
    if (!e || !out) return LOB_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    i64 c[16];
    i32 n_all = 0, flag = 0, mk_n[2] = {0, 0};
    { int rc = read_counters(e, c); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(mk_n, e->S.mk_count, sizeof mk_n, hipMemcpyDeviceToHost, e->stream));
    if (e->P.sarsa_lanes) {
        HIPCHK(hipMemcpyAsync(&n_all, e->S.mk_all_n, 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(&flag, e->S.amb_flag, 4, hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 8; i++) out[i] = 0;
    out[0] = c[6]; out[1] = c[5]; out[2] = n_all; out[3] = c[7]; out[4] = flag; out[5] = mk_n[e->last_par & 1];
    out[6] = c[2]; out[7] = c[4];
    return LOB_OK;
}

// Double Q carries two weight vectors: sync / delta buffers hold [theta | theta_b] back to back and
// one all-reduce of 2M doubles exchanges both.
static int delta_vectors(const lob_engine* e) { return e->P.algo == LOB_ALGO_DOUBLE_Q ? 2 : 1; }
// R-learning: the shared average reward rho travels behind the weights as [rho - rho_sync, 1.0] (rho_delta_*_kernel)
static int delta_extra(const lob_engine* e) { return e->P.r_learn ? 2 : 0; }

int lob_delta_init(lob_engine* e) {
    if (!e) return LOB_EINVAL;
    if (e->P.theta_private) { lob_set_error("lob_delta_*: shared theta only"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    const size_t M = (size_t)e->P.M;
    const int nv = delta_vectors(e);
    if (!e->S.theta_sync) {
        int rc = dev_alloc(e, &e->S.theta_sync, M * nv + delta_extra(e));
        if (rc == LOB_OK) rc = dev_alloc(e, &e->S.delta, M * nv + delta_extra(e));
        if (rc != LOB_OK) return rc;
    }
    HIPCHK(hipMemcpyAsync(e->S.theta_sync, e->S.theta, M * 8, hipMemcpyDeviceToDevice, e->stream));
    if (nv == 2) HIPCHK(hipMemcpyAsync(e->S.theta_sync + M, e->S.theta_b, M * 8, hipMemcpyDeviceToDevice, e->stream));
    if (delta_extra(e)) HIPCHK(hipMemcpyAsync(e->S.theta_sync + M * nv, e->S.rho, 8, hipMemcpyDeviceToDevice, e->stream));
    return LOB_OK;
}
int lob_delta_begin_async(lob_engine* e, double** dev_delta, int64_t* count) {
    if (!e || !dev_delta || !count) return LOB_EINVAL;
    if (!e->S.theta_sync) { lob_set_error("lob_delta_begin: call lob_delta_init first"); return LOB_ESTATE; }
    HIPCHK(hipSetDevice(e->device));
    const size_t M = (size_t)e->P.M;
    const int nv = delta_vectors(e);
    for (int v = 0; v < nv; v++) {
        TimedLaunch t(e, "delta_begin_kernel", nullptr, true);
        hipLaunchKernelGGL(delta_begin_kernel, dim3(2048), dim3(256), 0, e->stream, (const f64*)(v ? e->S.theta_b : e->S.theta),
                           (const f64*)(e->S.theta_sync + v * M), e->S.delta + v * M, e->P.M);
    }
    if (delta_extra(e))
        hipLaunchKernelGGL(rho_delta_begin_kernel, dim3(1), dim3(1), 0, e->stream, (const f64*)e->S.rho, (const f64*)(e->S.theta_sync + M * nv), e->S.delta + M * nv);
    HIPCHK(hipGetLastError());
    *dev_delta = e->S.delta;
    *count = (int64_t)(M * nv + delta_extra(e));
    return LOB_OK;
}
int lob_delta_begin(lob_engine* e, double** dev_delta, int64_t* count) {
    int rc = lob_delta_begin_async(e, dev_delta, count);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}
int lob_delta_apply(lob_engine* e) {
    if (!e) return LOB_EINVAL;
    if (!e->S.theta_sync) { lob_set_error("lob_delta_apply: call lob_delta_init first"); return LOB_ESTATE; }
    HIPCHK(hipSetDevice(e->device));
    const size_t M = (size_t)e->P.M;
    const int nv = delta_vectors(e);
    e->theta_ver++;  // memo records computed under the pre-exchange weights are void
    // between lob_td_step_begin and lob_td_step_end no hit list is live and the step's own memo launches follow: nothing to void
    const bool mid_step = e->half_open;
    if (!mid_step) e->hits_ok = false;
    for (int v = 0; v < nv; v++) {
        TimedLaunch t(e, "delta_apply_kernel", nullptr, true);
        hipLaunchKernelGGL(delta_apply_kernel, dim3(2048), dim3(256), 0, e->stream, v ? e->S.theta_b : e->S.theta, e->S.theta_sync + v * M,
                           (const f64*)(e->S.delta + v * M), v ? e->S.theta_b_nz : e->S.theta_nz, e->S.nz_epoch, e->P.M,
                           e->P.memo ? e->S.theta_nzx : (uint32_t*)nullptr, e->S.theta_nzc, e->P.cshift, e->S.theta_nzd, e->S.theta_nzm, e->S.nzd_terms);
    }
    if (delta_extra(e))
        hipLaunchKernelGGL(rho_delta_apply_kernel, dim3(1), dim3(1), 0, e->stream, e->S.rho, e->S.theta_sync + M * nv, (const f64*)(e->S.delta + M * nv));
    if (e->P.memo && !mid_step) launch_memo(e, e->last_par, 1);  // the current triples under the exchanged weights
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

// ---- sparse exchange (include/lob_engine.h) ------------------------------------------------------------------------------
static int64_t spx_words(const lob_engine* e) { return (int64_t)((size_t)e->P.M / 32 + 1); }
int lob_delta_sparse_supported(lob_engine* e) { return e && e->P.memo && e->P.algo != LOB_ALGO_DOUBLE_Q && e->S.theta_sync && e->S.theta_nzx ? 1 : 0; }
int lob_delta_sparse_maps(lob_engine* e, int32_t world, uint32_t** dev_own, uint32_t** dev_gather, int64_t* words) {
    if (!e || world < 1 || !dev_own || !dev_gather || !words) return LOB_EINVAL;
    if (!lob_delta_sparse_supported(e)) { lob_set_error("lob_delta_sparse_*: needs the shared-theta fast path and lob_delta_init"); return LOB_ESTATE; }
    HIPCHK(hipSetDevice(e->device));
    const int64_t W = spx_words(e);
    if (e->spx_gather.reserve((size_t)world * W)) {
        e->spx_world = 0;
        lob_set_error("lob_delta_sparse_maps: no room for the ranks' gathered maps");
        return LOB_ENOMEM;
    }
    e->spx_world = std::max(e->spx_world, world);
    if (!e->spx_union) {
        // the pinned word the union's size is handed over in, and its event.  A rank without them would ask for the exact count at
        // every exchange while the others use the fixed one -- collectives of different lengths: it fails HERE instead, where a
        // failing rank makes all of them fail together (see below)
        if (!e->spx_total_host && hipHostMalloc((void**)&e->spx_total_host, sizeof(i64), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); e->spx_total_host = nullptr;
            lob_set_error("lob_delta_sparse_maps: no pinned memory for the exchange's size hand-over");
            return LOB_ENOMEM;
        }
        if (!e->spx_ev && hipEventCreateWithFlags(&e->spx_ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError(); hipHostFree(e->spx_total_host); e->spx_total_host = nullptr;
            lob_set_error("lob_delta_sparse_maps: no event for the exchange's size hand-over");
            return LOB_ENOMEM;
        }
        const int nb = (int)((W + LOB_SPX_BLOCK - 1) / LOB_SPX_BLOCK);
        int rc = dev_alloc(e, &e->spx_union, (size_t)W);
        if (rc == LOB_OK) rc = dev_alloc(e, &e->spx_block_cnt, (size_t)nb);
        if (rc == LOB_OK) rc = dev_alloc(e, &e->spx_block_off, (size_t)nb);
        if (rc == LOB_OK) rc = dev_alloc(e, &e->spx_total, 1);
        if (rc != LOB_OK) return rc;
        // (the first fixed count: a 64th of the table, 4 096 .. 262 144 entries; LOB_SPX_COUNT: the tests' small one)
        e->spx_fixed = std::max<int64_t>(4096, std::min<int64_t>(1 << 18, e->P.M / 64));
        if (e->sw.spx_count) e->spx_fixed = e->sw.spx_count;
        e->spx_fixed = std::min<int64_t>(e->spx_fixed, e->P.M);
    }
    // every buffer of the exchange exists before its first collective starts (lob_theta_allreduce calls this once BEFORE the ranks
    // agree on the exchange's form, and a rank that failed here makes all of them fail together): a rank that failed to allocate
    // between two collectives would leave the others waiting in the second.  The packed deltas go into the dense exchange's
    // scratch vector (lob_delta_init: M doubles, idle while the exchange is sparse): the union has at most M entries, and
    // nothing of that size is allocated for it.
    e->spx_buf = e->S.delta;
    e->spx_cap = e->P.M;
    *dev_own = e->S.theta_nzx;
    *dev_gather = e->spx_gather.p;
    *words = W;
    return LOB_OK;
}
int lob_delta_sparse_pack(lob_engine* e, int32_t world, double** dev_buf, int64_t* count) {
    if (!e || !dev_buf || !count || world < 1 || world > e->spx_world || !e->spx_buf) {
        lob_set_error("lob_delta_sparse_pack: bad argument (call lob_delta_sparse_maps with this world size first)");
        return LOB_EINVAL;
    }
    HIPCHK(hipSetDevice(e->device));
    const int64_t W = spx_words(e);
    const int nb = (int)((W + LOB_SPX_BLOCK - 1) / LOB_SPX_BLOCK);
    {
        TimedLaunch t(e, "delta_begin_kernel", nullptr, true);
        hipLaunchKernelGGL(sparse_union_kernel, dim3(nb), dim3(LOB_SPX_BLOCK), 0, e->stream, (const uint32_t*)e->spx_gather.p, (int)world, (i64)W, e->spx_union, e->spx_block_cnt);
        hipLaunchKernelGGL(sparse_scan_kernel, dim3(1), dim3(1024), 0, e->stream, (const i32*)e->spx_block_cnt, nb, e->spx_block_off, e->spx_total);
    }
    // the union's size of the exchange BEFORE this one (its copy to pinned memory has had a whole exchange interval to land)
    if (e->spx_ev_pending) {
        HIPCHK(hipEventSynchronize(e->spx_ev));
        if (e->spx_total_host[0] != e->spx_last_total) { e->spx_prev_total = e->spx_last_total; e->spx_last_total = e->spx_total_host[0]; }
        e->spx_ev_pending = false;
        if (e->spx_last_total > e->spx_count) e->spx_overflows++;   // (that exchange left entries for this one)
    }
    const bool no_sync = e->spx_total_host && e->spx_last_total >= 0 && e->spx_prev_total >= 0 &&
                         e->spx_last_total + 2 * std::max<int64_t>(e->spx_last_total - e->spx_prev_total, 0) <= e->spx_fixed;
    i64 count_now;
    if (no_sync) {
        count_now = e->spx_fixed;
        e->spx_nosync++;
    } else {
        // the exact count, with the one synchronisation the exchange used to need every time
        i64 total = 0;
        HIPCHK(hipMemcpyAsync(&total, e->spx_total, sizeof total, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (total > e->spx_cap) { lob_set_error("lob_delta_sparse_pack: more union entries than weights"); return LOB_ESTATE; }  // (cannot happen: cap = M)
        while (e->spx_fixed < 2 * total && e->spx_fixed < e->spx_cap) e->spx_fixed = std::min<int64_t>(e->spx_fixed * 2, e->spx_cap);
        if (total != e->spx_last_total) { e->spx_prev_total = e->spx_last_total; e->spx_last_total = total; }
        count_now = total;
        e->spx_synced++;
    }
    e->spx_count = count_now;
    {
        TimedLaunch t(e, "delta_begin_kernel", nullptr, true);
        hipLaunchKernelGGL(sparse_pack_kernel, dim3(nb), dim3(LOB_SPX_BLOCK), 0, e->stream, (const uint32_t*)e->spx_union, (i64)W, (const i64*)e->spx_block_off,
                           (const f64*)e->S.theta, (const f64*)e->S.theta_sync, e->spx_buf, (i64)count_now);
        if (no_sync) hipLaunchKernelGGL(sparse_tail_kernel, dim3(64), dim3(256), 0, e->stream, e->spx_buf, (const i64*)e->spx_total, (i64)count_now);
    }
    if (e->spx_total_host) {   // this exchange's union size, for the next one
        HIPCHK(hipMemcpyAsync(e->spx_total_host, e->spx_total, sizeof(i64), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipEventRecord(e->spx_ev, e->stream));
        e->spx_ev_pending = true;
    }
    HIPCHK(hipGetLastError());
    *dev_buf = e->spx_buf;
    *count = count_now;
    return LOB_OK;
}
int lob_delta_sparse_apply(lob_engine* e) {
    if (!e || !e->spx_union) { lob_set_error("lob_delta_sparse_apply: no packed exchange to apply"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    const int64_t W = spx_words(e);
    const int nb = (int)((W + LOB_SPX_BLOCK - 1) / LOB_SPX_BLOCK);
    e->theta_ver++;  // memo records computed under the pre-exchange weights are void
    const bool mid_step = e->half_open;  // (see lob_delta_apply)
    if (!mid_step) e->hits_ok = false;
    if (e->spx_count > 0) {
        TimedLaunch t(e, "delta_apply_kernel", nullptr, true);
        hipLaunchKernelGGL(sparse_apply_kernel, dim3(nb), dim3(LOB_SPX_BLOCK), 0, e->stream, (const uint32_t*)e->spx_union, (i64)W, (const i64*)e->spx_block_off,
                           e->S.theta, e->S.theta_sync, (const f64*)e->spx_buf, e->S.theta_nz, e->S.nz_epoch, e->S.theta_nzx, e->S.theta_nzc, e->P.cshift,
                           e->S.theta_nzd, e->S.theta_nzm, e->S.nzd_terms, (i64)e->P.M, (i64)e->spx_count);
    }
    if (e->P.memo && !mid_step) launch_memo(e, e->last_par, 1);  // the current triples under the exchanged weights
    HIPCHK(hipGetLastError());
    return LOB_OK;
}

int lob_sync(lob_engine* e) {
    if (!e) return LOB_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    return check_device_errors(e);
}
void* lob_stream(lob_engine* e) { return e ? (void*)e->stream : nullptr; }

int lob_kernel_timing(lob_engine* e, int32_t enable) {
    if (!e) return LOB_EINVAL;
    hipSetDevice(e->device);
    hipStreamSynchronize(e->stream);
    drain_timers(e);
    e->timers.clear();
    e->timing = enable != 0;
    e->timing_period = enable > 1 ? enable : 1;
    return LOB_OK;
}
int lob_kernel_time_ms(lob_engine* e, const char* kernel, double* avg_ms, int64_t* launches) {
    if (!e || !kernel || !avg_ms || !launches) return LOB_EINVAL;
    hipSetDevice(e->device);
    drain_timers(e);
    auto it = e->timers.find(kernel);
    if (it == e->timers.end() || it->second.launches == 0) { *avg_ms = 0.0; *launches = 0; return LOB_OK; }
    *avg_ms = it->second.total_ms / (double)it->second.launches;
    *launches = it->second.launches;
    return LOB_OK;
}

}  // extern "C"

// Diagnostics (not part of include/lob_engine.h): 1 in a -DLOB_EXPERIMENTS build -- the kernel variants measured and lost
// (env_compact_kernel, the two-wave pre-pass, 32-lane env_step_kernel, two book groups, ...) exist and their switches work.
extern "C" int lob_experiments_enabled(void) { return lobk_experiments(); }

// Diagnostics (not part of include/lob_engine.h): phase clocks of a -DLOB_PROF build, summed over books
// (tools/exp_prof.py); LOB_ESTATE on a regular build.
extern "C" int lob_debug_prof(lob_engine* e, int64_t out[LOB_PROF_N]) {
    if (!e || !out) return LOB_EINVAL;
    if (!e->S.prof) { lob_set_error("lob_debug_prof: not a -DLOB_PROF build"); return LOB_ESTATE; }
    HIPCHK(hipSetDevice(e->device));
    std::vector<i64> h((size_t)e->B * LOB_PROF_N);
    HIPCHK(hipMemcpyAsync(h.data(), e->S.prof, h.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < LOB_PROF_N; i++) out[i] = 0;
    for (size_t b = 0; b < (size_t)e->B; b++)
        for (int i = 0; i < LOB_PROF_N; i++) out[i] += h[b * LOB_PROF_N + i];
    return LOB_OK;
}

// Diagnostics (not part of include/lob_engine.h): the state the fast path's shortcuts depend on -- [0] weights the exact
// written-weights map shows, [1] live books, [2] live books without a hit list, [3] sum of the live books' list lengths,
// [4 + n] live books whose list has n entries (the last bin, n = 256: that many or more).  bench.py's sustained leg prints it.
extern "C" int lob_debug_fastpath(lob_engine* e, int64_t* out, int32_t n_out) {
    if (!e || !out || n_out < 4 + LOB_FP_BINS) return LOB_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    DevTemp<i64> d;
    if (d.alloc(4 + LOB_FP_BINS)) { lob_set_error("lob_debug_fastpath: no room for the counts"); return LOB_ENOMEM; }
    hipError_t err = hipMemsetAsync(d.p, 0, (size_t)(4 + LOB_FP_BINS) * 8, e->stream);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(fastpath_stats_kernel, dim3(512), dim3(256), 0, e->stream, e->S, (i64)e->P.M, e->P.memo ? 1 : 0, d.p);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(out, d.p, (size_t)(4 + LOB_FP_BINS) * 8, hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    HIPCHK(err);
    return LOB_OK;
}


// Diagnostics (not part of include/lob_engine.h): books whose action came from act_light_kernel so far, and the step id of
// the last update that voided the hit lists (-1: never).
extern "C" int lob_debug_light(lob_engine* e, int64_t out[2]) {
    if (!e || !out) return LOB_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    i64 c[16];
    i32 d = 0;
    { int rc = read_counters(e, c); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(&d, e->S.hl_dirty, sizeof d, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    out[0] = c[5];
    out[1] = d;
    return LOB_OK;
}


// Diagnostics (not part of include/lob_engine.h): generations without a combine slot that trace_rest_kernel left to apply_kernel so far.
extern "C" int lob_debug_deferred(lob_engine* e, int64_t out[1]) {
    if (!e || !out) return LOB_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    i64 c[16];
    { int rc = read_counters(e, c); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(e->stream));
    out[0] = c[8];
    return LOB_OK;
}

// Diagnostics (not part of include/lob_engine.h): rho of the R-learning agents (`n` = 1 shared, n_books private).
extern "C" int lob_debug_rho(lob_engine* e, double* out, int32_t n) {
    if (!e || !out || n < 1 || !e->S.rho) return LOB_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(out, e->S.rho, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}

// Diagnostics (not part of include/lob_engine.h): how many weights the last two updates wrote for
// the first time -- the quantity that decides whether act_kernel can reuse learn_kernel's verdicts.
extern "C" int lob_debug_new_weights(lob_engine* e, int32_t out[2]) {
    if (!e || !out) return LOB_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    i32 h[2 * LOB_NZ_WORDS];
    HIPCHK(hipMemcpyAsync(h, e->S.nz_new, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    out[0] = h[0]; out[1] = h[LOB_NZ_WORDS];
    return LOB_OK;
}

// Diagnostics (not part of include/lob_engine.h): the written-weights maps of the pair learn kernel as they stand once the stream
// has drained -- the exact map [M / 32 + 1], the two maps folded over the actions [2][M / 32 + 1], the two tables of per-sum action
// masks [2][2 * fold_mask_words(M)] (16 bits each; LOB_ESTATE when the plan keeps none) and the 18 action terms of groups 1 and 2.
// The tests check the invariant between them: mask bit a of (g, s) = exact bit (s + term[g][a]) mod M, folded bit = mask != 0.
extern "C" int lob_debug_fold_maps(lob_engine* e, uint32_t* nzx, uint32_t* nzd, uint16_t* nzm, uint32_t* terms18) {
    if (!e || !nzx || !nzd || !nzm || !terms18) return LOB_EINVAL;
    if (!e->S.theta_nzd || !e->S.theta_nzm) { lob_set_error("lob_debug_fold_maps: this engine keeps no action-mask table"); return LOB_ESTATE; }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->stream2) HIPCHK(hipStreamSynchronize(e->stream2));
    const size_t words = (size_t)e->P.M / 32 + 1, mwords = fold_mask_words((uint32_t)e->P.M);
    HIPCHK(hipMemcpyAsync(nzx, e->S.theta_nzx, words * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(nzd, e->S.theta_nzd, 2 * words * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(nzm, e->S.theta_nzm, 2 * mwords * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(terms18, e->S.nzd_terms, 18 * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}
