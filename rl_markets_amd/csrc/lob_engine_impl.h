// The engine object and what the host-side translation units share (private: include/lob_engine.h is the interface).  The host side
// of the C ABI is four units: lob_engine.hip -- create / destroy / reset, the step pipeline, the weights and everything else that
// launches a kernel of its own by name --, lob_tu_host_streams.hip (event streams and the day library), lob_tu_host_vec.hip
// (lob_step, lob_vec_*, lob_branch_*, lob_snapshot_*) and lob_tu_host_reads.hip (read-backs, episode statistics, the logs, host counters).  The
// last three hold no kernel: they launch through lob_launch.h.
#ifndef LOB_ENGINE_IMPL_H
#define LOB_ENGINE_IMPL_H

#include <hip/hip_runtime.h>
#include <string.h>

#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "lob_internal.h"
#include "lob_kernels.h"
#include "lob_launch.h"
#include "lob_devbuf.h"

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            lob_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                \
            return LOB_EHIP;                                                                 \
        }                                                                                    \
    } while (0)

// parameters and state of the kernels that take them by pointer (lob_state.h LOB_PS_ARGS): their device-resident copies
#define LOB_PS(e) (const DevParams*)(e)->P_dev, (e)->S.self

// lob_devbuf.h over the device's memory
namespace lob {
struct HipAlloc {
    static int alloc(void** p, size_t bytes) {
        if (hipMalloc(p, bytes) == hipSuccess) return 0;
        (void)hipGetLastError();   // (or the next launch's HIPCHK(hipGetLastError()) reports the failed allocation as its own)
        return 1;
    }
    static void free(void* p) { hipFree(p); }
};
template <class T> using DevBuf = GrowBuf<T, HipAlloc>;    // grow-only, the engine's for its life (lob_destroy releases it)
template <class T> using DevTemp = ScopedBuf<T, HipAlloc>;  // one call's
}  // namespace lob

#define LOB_HINT_RING 64
#define LOB_HINT_LAG 16
#define LOB_HINT_EVERY 8   /* the count goes to host memory in every 8th learner step only: the store costs the kernel that makes it 3.5 us */

struct KTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0.0;
    int64_t launches = 0;
};

// Runtime switches (INTEGRATION.md §6 says what each does), read once by read_switches at lob_create.  Honoured by every build:
// the A/B switches of first-class paths that the parity tests force on or off at sizes that would not select them, the table sizes
// the tests squeeze, the track ring, the upload's pieces and the exchange's first count.  The switches of variants measured and
// lost, and of timing experiments, only by a -DLOB_EXPERIMENTS build (tools/exp_variants.sh; NOTES.md): read_switches leaves
// them at their defaults otherwise.  (LOB_DENSE_EXCHANGE is lob_comm.cpp's.)
struct Switches {
    bool no_memo = false, no_carry = false, no_combine = false, light = true, force_fuse_act = false, t_light = true, no_fuse = false;
    bool q_pair = true, dq_pair = true, trace_lanes_off = false, acc_fuse = true, rest_merge = true, acc_dense = true;
    int q_lanes = -1, force_general = -1;  // -1: by batch size / by the learn kernels' hand-back count
    int env_lanes = 0, env16_max = 4096;   // env_lanes 0: by batch size
    int acc_batches = 0, acc_shift = -1;   // 0 / -1: by algorithm, batch size and epsilon
    int cb_slots = 0, ow_slots = 0, amb_cap = 0, cbd_ids = 0;  // 0: by size
    int track_ring = 4096, track_refill = 64;
    long long upload_piece_recs = 0, spx_count = 0;  // 0: 64 MB pieces / by table size
    bool upload_pinned = true;
    // (-DLOB_EXPERIMENTS builds only)
    bool fuse_act = true, inline_general = true, env_step = true, prepass_roles = false, sarsa_lanes_off = false, dq_fast_off = false;
    bool rest_side = true, acc_block = true, exp_learn_first = false, no_hint = false;
    int env_step_lanes = 64, reset_lanes = 64, n_groups = 1, acc_reps = 0, ts_lds = 0, ts_grid = 0;  // acc_reps 0: by path
};

// The kernel paths fixed for the engine's life, by plan_paths from the parameters, the batch, the CU count and the switches.
// DevParams carries memo / combine / carry_verdicts / sarsa_lanes from here; run_steps takes every other fixed choice from here.
struct EnginePlan {
    int groups = 1;             // book groups of the step pipeline
    bool combine = false, memo = false, carry_verdicts = false, sarsa_lanes = false;  // (DevParams)
    bool q_lanes = false;       // Q(s', .) + TD error with lanes per book, else a wave per book (learn_q_fast_kernel)
    bool q_pair = false;        // ... two per book (learn_q_pair_kernel), else one (learn_q_lane_kernel)
    bool t_light = false;       // Q(lambda) / double Q: the light trace step for the books that keep no older generation
    bool fuse = false;          // ... inside the lane learn kernel, else trace_light_kernel
    bool fused_act_ok = false;  // the action selection may ride in the env kernel (fast-path learner steps on live hit lists)
    bool env_step = false, half_waves = false, env16 = false;  // ... in env_step_kernel (else env_kernel<64, TM, 1>): 32 lanes / 16 lanes per book
    bool inline_ok = false;     // ... which may serve the books without a hit list itself
    int env_lanes = 64;         // books per env_kernel wave
    bool acc_block_ok = false;  // the update may sum per block (StepPlan::acc_blocked), ...
    bool dense_ids = false;     // ... by the slots' dense ids
    bool acc_fuse_ok = false;   // updates may be added to their slots by the learn / trace kernels (StepPlan::acc_fused)
    bool rest_side_ok = false;  // learn_q_rest_kernel may run on the second stream
    bool learn_first = false;   // (experiment) SARSA(lambda)'s learn kernels in front of its trace kernels
};

struct lob_engine {
    int device = 0;
    int B = 0;
    lob_params params;
    Switches sw;
    EnginePlan plan;
    DevParams P;
    DevParams* P_dev = nullptr;  // device copy for the lane-per-book kernels
    DevState S;
    // The device-resident copy of S, at one address for the engine's lifetime (S.self): kernels that take the state by POINTER read
    // the fields they need where they need them, through the scalar cache -- 1 728 bytes of by-value kernel arguments are loaded at
    // the kernel's entry, live across all of it and cost env_step_kernel 104 spilled scalar registers + 160 vector registers parked
    // in AGPRs (round 6).  Kept up by sync_state() before every launch sequence, which uploads the two words a learner step
    // changes (cb_par, cb_dense_on) as 0; the claims read them through the pointer (cb_claim_finish), so every learner step
    // publishes them before its first claim (publish_step_words).
    DevState* S_dev = nullptr;
    DevState S_pushed;
    hipStream_t stream = nullptr;   // main stream (all API calls)
    hipStream_t stream2 = nullptr;  // second book group of the step pipeline
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_stagger = nullptr;
    hipEvent_t ev_rest_go = nullptr, ev_rest_done = nullptr;  // learn_q_rest_kernel on stream2 beside the trace kernels
    long long flow[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // lob_debug_flow: learner steps by the shape of their update / action selection (see there)
    long long hint_reads = 0, hint_misses = 0;  // lob_debug_hint: learner steps that read a hint word / found it still unwritten after the spin limit
    bool dense_ever = false;    // the dense sums have been on at some step: slots may hold dense ids (apply_kernel frees them with their slots)
    // learn_q_rest_kernel reports its list's length (the books the lane learn kernels handed back) through host-mapped memory:
    // a ring of LOB_HINT_RING words, one per learner step, each with an event recorded behind the kernel that writes it.  The
    // step launched now reads the word of LOB_HINT_LAG steps ago after waiting for THAT event (long past, unless the host is
    // more than LOB_HINT_LAG steps ahead of the device -- then it waits: the device still has that many steps queued), so which
    // path a step takes is a function of the run, not of the host's timing.  The first LOB_HINT_LAG steps after
    // lob_reset / lob_theta_set read 0.  A weight exchange (lob_delta_apply / lob_delta_sparse_apply) does NOT void the counts:
    // it runs every 64 steps, the written set only grows by the union of the ranks', and which books have no usable hit list
    // hardly changes -- voiding them would send a quarter of a dense-theta run's steps down the slower path.
    u64* rest_hint = nullptr;   // word = (step tag) << 32 | count: the host checks the tag, so it never reads a word the device has not written yet
    u64* rest_hint_dev = nullptr;
    hipEvent_t hint_ev[LOB_HINT_RING] = {};
    long long hint_step = 0;    // learner steps (fast path) since the hints were last void
    unsigned long long hint_serial = 0;  // launches of learn_q_rest_kernel since lob_create (the tag of a ring word)
    uint32_t hint_tags[LOB_HINT_RING] = {};
    int hint_now = 0;           // the hint this step goes by (run_steps)
    int rest_recent = 0;        // steps left to keep the launch on the second stream after the last non-empty list seen
    int reg_apar = 0;   // which of the two lists of newly ambiguous indices this step's registry blocks fill (trace_lane_kernel's launch) and its scan blocks read (apply_kernel's)
    int td_parity = 0;
    int step_id = 0;            // stamps the memo claims of one step
    int list_par = 0;           // parity of the fast path's work lists
    int last_par = 0;           // `par` of the most recent step (its memo list is the current one)
    int n_cus = 256;            // compute units: the persistent learner kernels run one block on each
    bool chunked = false;       // the loaded stream is longer than the ring
    int steps_since_fill = 0;
    uint64_t theta_ver = 1;     // bumped whenever theta changes: memo records carry the version they were computed under
    bool half_open = false;     // between lob_td_step_begin and lob_td_step_end
    bool hits_ok = false;       // the previous call was a fast-path learner step and nothing has touched weights, maps or states since:
                                // the hit lists its learn kernel left are those of the States the next step acts on (act_light_kernel)
    int steps_on_lists = 0;     // fused steps since the hit lists were last void
    std::vector<void*> allocs;
    // sparse weight exchange (lob_delta_sparse_*): the ranks' gathered maps, their union, per-block counts / offsets, the packed deltas
    lob::DevBuf<uint32_t> spx_gather;   // [spx_world][M / 32 + 1]
    int spx_world = 0;
    uint32_t* spx_union = nullptr;
    i32* spx_block_cnt = nullptr;
    i64* spx_block_off = nullptr;
    i64* spx_total = nullptr;
    f64* spx_buf = nullptr;
    int64_t spx_cap = 0, spx_count = 0;
    // The exchange without a host synchronisation: the packed vector's length is a host argument of the
    // collective, and the union's true size is only known on the device.  So the ranks exchange a FIXED count -- spx_fixed, the
    // same on every rank because it is a function of the union sizes of the exchanges before, which are the same on every rank --
    // with the tail behind the union zero-filled, and every exchange leaves its union's size in pinned host memory behind an event
    // that the NEXT exchange (64 steps later: long past) reads.  The union only grows, ever more slowly (the written set saturates):
    // an exchange goes without a synchronisation when the last size + twice the last increase still fits spx_fixed; the first two
    // exchanges, and any whose prediction does not fit, take the exact count with a synchronisation and set spx_fixed to at least
    // twice it.  A union that outgrows the count anyway (its growth more than doubled from one interval to the next) loses nothing:
    // the entries beyond it keep theta - theta_sync and travel with the next exchange (counted: lob_debug_exchange; the parity
    // tests of the exchange assert that it never happens in them).
    i64* spx_total_host = nullptr;   // pinned
    hipEvent_t spx_ev = nullptr;
    int64_t spx_fixed = 1 << 18, spx_last_total = -1, spx_prev_total = -1;
    bool spx_ev_pending = false;
    long long spx_nosync = 0, spx_synced = 0, spx_overflows = 0;
    uint32_t* rnd_dev = nullptr;
    uint32_t* records_dev = nullptr;
    // The NEXT episode's streams, handed over while the current episode runs (lob_stage_events): a second record buffer filled by
    // a host thread through a stream of its own -- validation, pinned staging, DMA, repack, none of it on the engine's stream --
    // and adopted by the lob_reset that follows.  The reference loads a fresh day before every episode (src/main.cpp:53-55).
    size_t records_bytes = 0, track_bytes = 0;   // sizes of records_dev / track_dev (set_records re-uses buffers of the right size)
    uint32_t* records_next = nullptr;
    hipStream_t stream_up = nullptr;
    std::thread stage_thread;
    bool stage_active = false;      // a hand-over has been started and not adopted / waited for yet
    int stage_rc = LOB_OK;
    std::string stage_err;
    i64* phase_dev = nullptr;  // replayed stream: first record of every book's window
    // Day library (lob_load_days): the days back to back in records_dev, their tables, and two sets of every book's
    // (first record, length, day) -- the set the current episode plays and the one a selection writes for the next
    bool lib = false;
    int lib_days = 0;
    i64* day_first_dev = nullptr;   // [lib_days] first record of each day
    i32* day_len_dev = nullptr;     // [lib_days] its events
    uint32_t* day_rng = nullptr;    // [B] each book's minstd_rand0 state (persists across draws)
    i32* day_explicit = nullptr;    // [B] lob_days_set's days on the device
    i32* day_explicit_host = nullptr;  // [B] pinned: the host side of that copy
    hipEvent_t day_copied = nullptr;   // the copy out of day_explicit_host has been done
    i64* lib_phase[2] = {nullptr, nullptr};
    i32* lib_len[2] = {nullptr, nullptr};
    i32* lib_day[2] = {nullptr, nullptr};
    int lib_cur = -1;           // the set the current episode plays (-1: no episode on the library yet)
    bool lib_pending = false;   // a selection waits for the next lob_reset (in set lib_cur ^ 1, or 0)
    Track* track_dev = nullptr;
    i32* actions_dev = nullptr;
    lob::DevBuf<f64> roll_ws;   // lob_vec_rollout: the PnL windows' entries the plans push (lob_launch.h RolloutSrc::shadow), made by the first
                                // call that needs it, grown when a later call needs more, never per call
    // lob_branch_*: the branch set (lob_branch.h) and the buffer lob_branch_select gathers into -- the two swap roles with every
    // select --, each made by the first call that needs it and grown only by a fork that needs more; the shape of the live set, and
    // whether it belongs to the current episode (lob_reset clears it)
    lob::DevBuf<char> branch_buf[2];
    int branch_cur = 0;         // which of the two holds the set
    int branch_n = 0;           // branches of the live set
    bool branch_live = false;
    u64* vec_bad = nullptr;     // lob_vec_step: actions out of range since the last lob_vec_status / lob_reset (one device word); behind it
                                // [1], [2]: the look-aheads' ahead / behind cells on a ring track (lob_launch.h PeekSrc::look_cnt)
    // lob_look_ring: the look-aheads run on a ring track.  Host words only: the real steps of the engine's life
    // (maybe_refill_track counts them), their count at the set's last fork and the lob_branch_step calls since -- the set's lead over
    // the real books --, and what the last lob_vec_status read of the two cell counts (lob_look_counts)
    bool look_ring = false;
    long long real_steps = 0, branch_fork_real = 0, branch_steps = 0;
    int64_t look_ahead_seen = 0, look_behind_seen = 0;
    i32* vec_upd_tag = nullptr; // lob_vec_update: the number of the last launch that wrote a weight (one device word; lob_launch.h VecFeatSrc)
    i32 vec_upd_launch = 0;     // ... and the number of the last launch (never 0 once used)
    uint32_t vec_terms[27] = {0};   // lob_vec_terms: the 27 action terms mod M, as uploaded behind the hash table
    i64* cnt_sum = nullptr;     // the striped device counters added up (read_counters)
    lob::DevBuf<lob_book_dump> dump;          // lob_get_books
    lob::DevBuf<lob_episode_record> stats;    // lob_episode_stats: the result records, then the blocks' partial records
    // lob_step_log_*: the device log of the selected books' profit-log rows (lob_tu_steplog.hip), all of it the engine's own
    lob_step_row* slog_rows = nullptr;    // [slog_cap][slog_n], step-major
    i32* slog_cnt = nullptr;              // [2][slog_n]: stored rows, lost rows
    i32* slog_sel = nullptr;              // [slog_n] local book indices (null: every book)
    int slog_n = 0, slog_cap = 0;         // slog_n == 0: the log is off
    bool slog_armed = false;              // a lob_reset has come since lob_step_log_enable: the steps record
    lob::DevBuf<lob_step_row> slog_stage; // lob_step_log_read's book-major staging buffer
    // lob_snapshot_*: the slot buffers (one allocation each, made by the slot's first save), whether each holds a full save of the
    // current episode, the descriptor table of the saved arrays (lob_launch.h SnapArgs; built with the first save) and the flag
    // that keeps the learner calls off a restored batch until the next lob_reset
    lob::DevBuf<char> snap_buf[LOB_MAX_SNAPSHOTS];   // (snap_bytes each)
    bool snap_valid[LOB_MAX_SNAPSHOTS] = {false, false, false, false};
    void* snap_tab = nullptr;
    SnapArgs snap_args;
    size_t snap_bytes = 0;
    bool restored = false;
    bool have_events = false, was_reset = false;
    bool episode_open = false;  // a pre-pass ran and its window sums have not been rolled back to the stop point yet
    bool model_log = false;     // lob_model_log_enable: the step sums |delta| (td_stats_kernel)
    bool timing = false;
    int timing_period = 1;  // kernels of every n-th step are timed (two event records per launch are not free: 9 % at n = 1)
    std::map<std::string, KTimer> timers;
    std::vector<hipEvent_t> event_pool;
    // lob_debug_launches (below, beside lob_debug_flow): launches of kernels that share a timer name
    int64_t launched[6] = {0, 0, 0, 0, 0, 0};
};

// What more than one unit uses (defined in lob_engine.hip unless said otherwise), in a namespace: the library exports no new C name
namespace lob {

// What an entry point needs of the engine's state before it may run, as bits for guard().  The rules are part of the interface
// (include/lob_engine.h says what each call may follow); guard() refuses with LOB_ESTATE and the caller's name in front of the
// reason, checking in the order of the bits.
//   RESET        a lob_reset has come since the stream was loaded
//   WHOLE_STEP   not between lob_td_step_begin and lob_td_step_end: only the weight exchange may run there -- anything that moves
//                the books, the traces or the weights would change what the second half consumes
//   NOT_RESTORED no lob_snapshot_restore in this episode: the learner's memory of the books' last transition (the rl::State objects,
//                the traces, the hit lists) then belongs to another trajectory, and the learner calls wait for the next lob_reset
//   NO_RING      the market track is resident, not a ring (a stream of more than LOB_TRACK_RING events): the look-aheads read the
//                entries ahead of the cursor, and a ring has outcomes a resident track cannot produce ("beyond the window", "fell
//                behind the window": DESIGN.md 7n) -- refused unless the caller has asked for them with lob_look_ring
//   NO_RING_BACK ... the same for the snapshots, which need the entries before the cursor: those are gone (a longer message)
enum : unsigned { RESET = 1, WHOLE_STEP = 2, NOT_RESTORED = 4, NO_RING = 8, NO_RING_BACK = 16 };
int guard(lob_engine* e, const char* who, unsigned needs);   // (e == NULL: LOB_EINVAL, no message)

// Which call needs what.  Argument checks (LOB_EINVAL) come in front of the guard, "nothing wanted" returns behind it.
namespace needs {
constexpr unsigned lob_step = RESET | WHOLE_STEP;
constexpr unsigned lob_vec_step = RESET | WHOLE_STEP, lob_vec_observe = RESET | WHOLE_STEP;
constexpr unsigned lob_vec_book = RESET | WHOLE_STEP, lob_vec_history = RESET | WHOLE_STEP, lob_vec_act = RESET | WHOLE_STEP;
constexpr unsigned lob_vec_peek = RESET | WHOLE_STEP | NO_RING, lob_vec_rollout = RESET | WHOLE_STEP | NO_RING;
constexpr unsigned lob_branch_fork = RESET | WHOLE_STEP | NO_RING, lob_branch_step = RESET | WHOLE_STEP | NO_RING, lob_branch_select = RESET | WHOLE_STEP | NO_RING;
constexpr unsigned lob_branch_book = lob_branch_step, lob_branch_history = lob_branch_step;
constexpr unsigned lob_vec_features = WHOLE_STEP, lob_vec_update = WHOLE_STEP;   // (+ RESET behind it when the rows are the books')
constexpr unsigned lob_snapshot_save = RESET | WHOLE_STEP | NO_RING_BACK, lob_snapshot_restore = RESET | WHOLE_STEP | NO_RING_BACK;
constexpr unsigned lob_track_window = RESET;
constexpr unsigned lob_get_state = RESET, lob_get_reward = RESET, lob_get_terminal = RESET;
constexpr unsigned lob_clear_inventory = RESET | WHOLE_STEP, lob_episode_stats = RESET | WHOLE_STEP;
constexpr unsigned lob_step_log_enable = WHOLE_STEP, lob_step_log_counts = WHOLE_STEP, lob_step_log_read = WHOLE_STEP;
constexpr unsigned lob_days_select = WHOLE_STEP, lob_days_set = WHOLE_STEP;
constexpr unsigned lob_theta_set = WHOLE_STEP, lob_handle_terminal = WHOLE_STEP | NOT_RESTORED;
// The step calls word their own refusal of a half-done step (and lob_td_step_end wants one): RESET in front of it, behind it
constexpr unsigned lob_td_step = NOT_RESTORED, lob_td_step_begin = NOT_RESTORED, lob_eval_step = NOT_RESTORED, lob_td_step_end = 0;
}  // namespace needs
#define LOB_GUARD(e, fn)                                        \
    do {                                                        \
        const int _rc = lob::guard((e), #fn, lob::needs::fn);   \
        if (_rc) return _rc;                                    \
    } while (0)

int sync_state(lob_engine* e);
int push_params(lob_engine* e);
int check_device_errors(lob_engine* e);
int device_error_rc(i32 flag);
int finalize_episode(lob_engine* e);
void launch_env(lob_engine* e, hipStream_t st, const i32* actions, int count_updates, int b0, int nb, int par);
void launch_step_log(lob_engine* e);
void maybe_refill_track(lob_engine* e);
void look_refill_track(lob_engine* e, long long depth);   // the same in front of a look-ahead `depth` steps deep (lob_look_ring)
void launch_memo(lob_engine* e, int par, int which, int reset_lpar = -1);
void drain_timers(lob_engine* e);
void free_days(lob_engine* e);       // lob_tu_host_streams.hip
int stage_adopt(lob_engine* e);      // lob_tu_host_streams.hip
void step_log_free(lob_engine* e);   // lob_tu_host_reads.hip

template <class T> int dev_alloc(lob_engine* e, T** p, size_t count) {
    void* q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    hipError_t err = hipMalloc(&q, bytes);
    if (err != hipSuccess) {
        lob_set_error(std::string("hipMalloc failed: ") + hipGetErrorString(err));
        return LOB_ENOMEM;
    }
    err = hipMemsetAsync(q, 0, bytes, e->stream);
    if (err != hipSuccess) { lob_set_error("hipMemset failed"); return LOB_EHIP; }
    e->allocs.push_back(q);
    *p = (T*)q;
    return LOB_OK;
}

template <class T> int dev_alloc(lob_engine* e, GP<T>* p, size_t count) { return dev_alloc(e, &p->p, count); }

struct TimedLaunch {
    lob_engine* e;
    KTimer* t = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    // `always`: kernels that do not run every step (reset, weight exchange, ring refill) are timed whenever timing is on
    TimedLaunch(lob_engine* e_, const char* name, hipStream_t s = nullptr, bool always = false) : e(e_), st(s ? s : e_->stream) {
        if (!e->timing || (!always && e->timing_period > 1 && e->step_id % e->timing_period != 0)) return;
        t = &e->timers[name];
        auto get = [&]() {
            hipEvent_t ev;
            if (!e->event_pool.empty()) { ev = e->event_pool.back(); e->event_pool.pop_back(); }
            else hipEventCreateWithFlags(&ev, hipEventDisableSystemFence);
            return ev;
        };
        a = get();
        b = get();
        hipEventRecord(a, st);
    }
    ~TimedLaunch() {
        if (!t) return;
        hipEventRecord(b, st);
        t->pending.push_back({a, b});
    }
};

}  // namespace lob
using namespace lob;

#endif
