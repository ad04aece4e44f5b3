// Launch entry points of the kernel families that are compiled in translation units of their own (the engine library is sixteen
// .hip files with kernels, built in parallel with three that hold host code only -- lob_tu_host_streams.hip, lob_tu_host_vec.hip,
// lob_tu_host_reads.hip: the C ABI's families that launch through this header alone, lob_engine_impl.h --: lob_engine.hip -- the
// engine object, the step pipeline, the weights and the update / memo / trace kernels --, lob_tu_env.hip,
// lob_tu_prepass.hip, lob_tu_learn.hip, lob_tu_stats.hip, lob_tu_steplog.hip, lob_tu_vec.hip, lob_tu_vecbook.hip, lob_tu_vechist.hip, lob_tu_snapshot.hip,
// lob_tu_vecact.hip, lob_tu_vecfeat.hip, lob_tu_vecpeek.hip, lob_tu_vecroll.hip, lob_tu_branch.hip, lob_tu_branchobs.hip).  Plain host functions: which instantiation runs is decided here, by the same rules
// lob_engine.hip used when it held the launches itself.  Kernels measured and lost (NOTES.md "Round 4") are only compiled with
// -DLOB_EXPERIMENTS (tools/exp_variants.sh); a product build answers LOB_EXPERIMENTS-only requests with the product kernel.
#ifndef LOB_LAUNCH_H
#define LOB_LAUNCH_H

#include <hip/hip_runtime.h>

#include "lob_state.h"
#include "lob_branch.h"

struct EnvFuse {  // env_kernel MODE 1 / 2, env_step_kernel (lob_kernels.h)
    const i32* list;
    const i32* list_n;
    int lpar, sid_prev;
    u64 ver;
};

// 1 in a -DLOB_EXPERIMENTS build (lob_experiments_enabled(), a diagnostic export: the tests of the opt-in variants skip without it)
int lobk_experiments();

// ---- lob_tu_env.hip ----
// env_kernel<lanes, TM, 0>: `lanes` 16 | 64 (32, and 256 = env_compact_kernel: experiments)
void lobk_env(hipStream_t st, int lanes, bool t2, const DevParams* Pd, const DevState& S, const i32* actions, int count_updates, int b0, int nb, int sid, int par);
// env_kernel<64, TM, mode>: 1 = action selection fused (books without a list go on the work list), 2 = the work list's books
void lobk_env_mode(hipStream_t st, bool t2, int mode, const DevParams* Pd, const DevState& S, int nb, int sid, int par, const EnvFuse& F);
// env_step_kernel<inline_general, dq> (two trade slots); half_waves: <false, false, 32> (experiments)
// `lanes16`: env_step16_kernel<inline_general> -- a book's levels across 16 lanes, four books per wave (small batches; one weight vector)
int lobk_env_step(hipStream_t st, bool inline_general, bool dq, bool half_waves, bool lanes16, const DevParams* Pd, const DevState& S, int nb, int sid, int par,
                   const EnvFuse& F, const uint32_t* rnd);
void lobk_clear_inventory(hipStream_t st, const DevParams* Pd, const DevState& S);
void lobk_get_state(hipStream_t st, const DevParams* Pd, const DevState& S, f32* out, f64* reward);
void lobk_dump(hipStream_t st, const DevParams* Pd, const DevState& S, int first, int n, lob_book_dump* out);

// ---- lob_tu_prepass.hip ----
void lobk_gen_events(hipStream_t st, const lob_gen_params& g, int D, int T, u64 first_book, int B, uint32_t* out);
void lobk_repack(hipStream_t st, const uint32_t* src, int D, int T, size_t n_records, uint32_t* dst);
void lobk_days_draw(hipStream_t st, int B, u64 first_book, int mode, int first, int n, const i32* explicit_day, uint32_t* rng, const i64* day_first,
                    const i32* day_len, i64* rec_phase, i32* rec_len, i32* day);
// reset_kernel<lanes, TM> (`roles`: reset2_kernel, `lanes` 16 | 32: experiments)
void lobk_reset(hipStream_t st, int lanes, bool t2, bool roles, const DevParams* Pd, const DevState& S);
void lobk_prepass_extend(hipStream_t st, bool t2, bool roles, const DevParams* Pd, const DevState& S);
void lobk_finalize(hipStream_t st, bool t2, const DevParams* Pd, const DevState& S);

// ---- lob_tu_stats.hip ----
// What the episode-statistics reduction reads, as kernel arguments (the DevState does not grow and does not travel): the environment
// field arrays of LOB_ENV_FIELDS it needs, the books' day words (null: no day groups) and the two session times of is_open
#define LOB_STATS_BLOCK 256
#define LOB_STATS_CHUNK 2048   // books per block: the unit that fixes the summation order (lob_kernels.h), so a constant
struct StatsSrc {
    const f64 *ep_reward, *ep_pnl, *ep_bandh;
    const i32 *total_ticks, *market_buys, *market_sells, *done, *time_ms;
    const i64 *ntr_snap, *tick_pos;
    const i32* day;
    i64 open_ms, close_ms;
    u64 book_id_offset;
    i32 B;
};
// out[0 .. n_groups): group 0 = every book, 1 + d = the books of day d; partial: n_groups * lobk_stats_chunks(B) records of scratch
int lobk_stats_chunks(int B);
void lobk_episode_stats(hipStream_t st, const StatsSrc& s, int n_groups, lob_episode_record* partial, lob_episode_record* out);

// ---- lob_tu_steplog.hip ----
// What the step log reads and writes, as kernel arguments (the DevState does not grow and does not travel): the environment field
// arrays of LOB_ENV_FIELDS behind a row of lob_step_row, the event records with the two words of a record that hold the touch
// prices, the selection and the log itself.  rows[k * n_sel + j] = row k of selected book j (step-major: in the live phase the
// lanes of a wave share k and write 64 x 96 B contiguous); n_rows / n_lost: [n_sel], one lane owns one book's two counters.
struct StepLogSrc {
    const i32 *done, *time_ms, *rec_cur, *last_action, *ask_level, *bid_level, *total_ticks;
    const i64* position;
    const f64 *ask_quote, *bid_quote, *pnl_step, *ep_pnl, *ep_bandh, *ep_reward;
    const uint32_t* records;   // DevState::records / rec_phase (null: book b's stream starts at record b * n_events)
    const i64* rec_phase;
    i32 n_events, Wd, w_ask0, w_bid0;   // record stride in words; the words of a record holding ask_px[0] / bid_px[0]
    const i32* sel;            // [n_sel] local book of selected j, ascending (null: j itself, every book)
    i32 n_sel, cap;
    lob_step_row* rows;
    i32 *n_rows, *n_lost;
};
void lobk_step_log(hipStream_t st, const StepLogSrc& s);
// out[(j - first_sel) * n_rows + (k - first_row)] = row k of selected book j, 96 zero bytes beyond the book's stored count
void lobk_step_log_gather(hipStream_t st, const lob_step_row* rows, const i32* n_stored, int n_sel_all, int first_sel, int n_sel, int first_row,
                          int n_rows, lob_step_row* out);

// ---- lob_tu_vec.hip ----
// What the vector-env interface (include/lob_engine.h lob_vec_*) reads and arms, as kernel arguments (the DevState does not grow):
// the books' step headers, the two field arrays of lob_get_terminal, the state vectors with their slot-2 copy of the latest
// getState(), the two session times of is_open and the engine's word that counts actions out of range.
#define LOB_VEC_BLOCK 256
struct VecSrc {
    LHdr* hdr;
    const i32 *done, *time_ms;
    const f32* vars;           // [B][3][16]
    i64 open_ms, close_ms;
    i32 B, V;
    u64* n_bad;
};
// vec_actions_kernel: LHdr::action / stepped of every book from the caller's device actions, for env_kernel's `go = h.stepped != 0`
void lobk_vec_actions(hipStream_t st, const VecSrc& s, const i32* dev_actions);
// vec_observe_kernel (`after_step`: behind lobk_env, stepped / reward from the headers; obs from slot 2 either way) or, `derive`,
// vec_observe_derive_kernel: obs and reward evaluated as get_state_kernel does (lob_vec_observe).  out.n_live must have been cleared
// on the stream.
void lobk_vec_observe(hipStream_t st, bool derive, bool after_step, const VecSrc& s, const DevParams* Pd, const DevState& S, const lob_vec_out& out);

// ---- lob_tu_vecbook.hip ----
// What lob_vec_book (include/lob_engine.h) reads, as kernel arguments (the DevState does not grow): the event records with the
// words of a record at which the four level arrays start (the device layout, lob_env.h drec_*: each array 16-byte aligned, `D`
// words used), the books' current-record word -- dump_kernel takes e.rec_cur from this field array and follows it through
// EnvCtx::row, i.e. records + (rec_phase[b] or b * n_events, + rec_cur[b]) * Wd; neither the per-book meta nor the track is on that
// way -- and the environment field arrays of LOB_ENV_FIELDS behind the sixteen words of `own` and time_ms.
#define LOB_VECBOOK_BLOCK 256
#define LOB_VECBOOK_BOOKS 64   // books per block (8 lanes per book and pass, two passes): 14 KB of staging, so LDS never bounds the waves per CU
struct VecBookSrc {
    const uint32_t* records;   // DevState::records / rec_phase (null: book b's stream starts at record b * n_events)
    const i64* rec_phase;
    const i32* rec_cur;
    i32 n_events, Wd, D;
    i32 w_ask_px, w_ask_vol, w_bid_px, w_bid_vol;
    const i64 *position, *a_osz, *a_oex, *a_oqh, *b_osz, *b_oex, *b_oqh;
    const i32 *a_on, *b_on, *last_action, *total_ticks, *time_ms;
    const f64 *a_opx, *b_opx, *ask_quote, *bid_quote, *pnl_step, *ep_pnl, *ep_reward;
    i32 B;
};
void lobk_vec_book(hipStream_t st, const VecBookSrc& s, const lob_vec_book_out& out);

// ---- lob_tu_vechist.hip ----
// What lob_vec_history (include/lob_engine.h) reads, as kernel arguments (the DevState does not grow): the event records, the first
// record of every book's stream (rec_phase, or b * n_events), the books' current-record word, the length of every book's stream
// (rec_len, or n_events: the bound of the window's last record) and the words of a record at which its arrays start (the device
// layout, lob_env.h drec_*: header quad, four level arrays of D words padded to quads, T interleaved (price, volume) pairs).
#define LOB_VECHIST_BLOCK 256
#define LOB_VECHIST_ROWS 64   // (book, slot) rows per block: 15 KB of staging for D = 10, T = 8, so LDS never bounds the waves per CU
struct VecHistSrc {
    const uint32_t* records;   // DevState::records / rec_phase (null: book b's stream starts at record b * n_events)
    const i64* rec_phase;
    const i32* rec_cur;
    const i32* rec_len;        // DevState::rec_len (null: every stream has n_events records)
    i32 n_events, Wd, D, T, B;
    i32 w_ask_px, w_ask_vol, w_bid_px, w_bid_vol, w_trades;
};
void lobk_vec_history(hipStream_t st, const VecHistSrc& s, int K, const lob_vec_hist_out& out);

// ---- lob_tu_snapshot.hip ----
// What lob_snapshot_save / lob_snapshot_restore (include/lob_engine.h) move, as a descriptor table in device memory (the DevState does
// not grow, and sixty pointers do not travel by value): one SnapRow per [B] row of every saved array -- the arrays of LOB_ENV_FIELDS,
// the rolling means pnl_ups / pnl_downs (a ring of w rows: w entries) --, the `n4` rows of 4-byte elements first, the `n8` rows of
// 8-byte elements behind them (the masked path: a lane per book walks the rows); one SnapArr per whole array (the all-books path:
// contiguous bytes on both sides).  `off`: the array's (row's) place in a slot buffer, arrays at multiples of 16 bytes in the live
// layout.  The two per-book records -- the environment's words of LHdr, slot 2 of `vars` -- come as kernel arguments.
#define LOB_SNAP_BLOCK 256
struct SnapRow {
    void* live;   // the row's first element in the engine's state
    u64 off;      // ... and its byte offset in a slot buffer
};
struct SnapArr {
    void* live;
    u64 off, bytes, _pad;
};
struct SnapArgs {
    const SnapRow* rows;   // [n4 + n8], device memory
    const SnapArr* arrs;   // [n_arr], device memory
    i32 n4, n8, n_arr, B;
    u64 max_bytes;         // the largest array
    LHdr* hdr;             // [B]: done, time_ms, action, stepped, reward are the environment's
    f32* vars;             // [B][3][16]: slot 2
    u64 off_hdr, off_reward, off_vars;   // slot buffer: i32 [4][B] (done, time_ms, action, stepped), f64 [B], f32 [B][16]
};
// snapshot_masked_kernel (dev_mask: uint8 [B] in device memory, nonzero selects) or, dev_mask == NULL, snapshot_all_kernel
void lobk_snapshot(hipStream_t st, bool restore, const SnapArgs& a, void* slot, const uint8_t* dev_mask);

// ---- lob_tu_vecact.hip ----
// What lob_vec_act / lob_vec_q (include/lob_engine.h) read and write beyond the parameters and the state, which vec_act_kernel takes by
// pointer (lob_state.h LOB_PS_ARGS): the caller's device buffers, the mode and -- for free-standing states -- the rows and the one
// weight vector with its "ever written" map, so that this form reads nothing of the state (valid before the first lob_reset, when the
// state's device-resident copy has not been uploaded yet).
#define LOB_VECACT_MAX_BLOCKS 2048
struct VecActSrc {
    const f32* rows;       // free-standing states [n][V] (null: the books' latest getState(), slot 2 of DevState::vars)
    const f64* theta;      // free-standing states: the weights lob_q_values uses ...
    const uint32_t* nz;    // ... and their map
    i32 n;                 // states: the books, or the caller's rows
    i32 mode;              // LOB_ACT_*
    i32* action;           // [n] (null: nothing is sampled)
    f64* q;                // [n][LOB_N_ACTIONS] (null: not wanted)
};
// vec_act_kernel<books, dq>: a persistent grid of at most LOB_VECACT_MAX_BLOCKS blocks, sized from the compute units (`n_cus`); `dq`: the
// double agents' second weight vector (the books' form only: a.rows null)
void lobk_vec_act(hipStream_t st, bool dq, int n_cus, const DevParams* Pd, const DevState* Sd, const uint32_t* rnd, const VecActSrc& a);

// ---- lob_tu_vecfeat.hip ----
// What lob_vec_features / lob_vec_update (include/lob_engine.h) read and write beyond the parameters and the state, which
// vec_feat_kernel takes by pointer (lob_state.h LOB_PS_ARGS): the caller's device buffers and, for an update, the target weight vector
// with every map delta_apply_kernel keeps for it -- filled in by the host in both forms, so that the free-standing form reads nothing
// of the state (valid before the first lob_reset, when the state's device-resident copy has not been uploaded yet) and the books'
// form only the rows.
#define LOB_VECFEAT_MAX_BLOCKS 2048
struct VecFeatSrc {
    const f32* rows;       // free-standing states [n][V] (null: the books' latest getState(), slot 2 of DevState::vars)
    const i32* actions;    // [n] (null: no action; features without idx only)
    i32 n;                 // states: the books, or the caller's rows
    i32* sums;             // features: [n][LOB_N_TILES] (null: not wanted)
    i32* idx;              // features: [n][LOB_N_TILES] (null: not wanted)
    const f64* step;       // update: [n] per-tile increments (null: a features launch)
    f64* theta;            // update: the target vector -- theta or theta_b; book 0's under private theta (the books' form adds s * M)
    uint32_t* nz;          // ... its "ever written" map (the books' form adds s * LOB_NZ_NWORDS(M) under private theta)
    uint32_t* nzx;         // ... the memo path's exact map (null: not on the memo path), its coarse image, the maps folded over the
    uint32_t* nzc;         //     actions and their terms: delta_apply_kernel's arguments
    uint32_t* nzd;
    uint32_t* nzm;
    const uint32_t* nzd_terms;
    i32 cshift;
    i32* nz_epoch;         // bumped once by a launch that writes anything
    i32* tag;              // ... [1] the number of the last launch that did (`launch`: this one's, never 0)
    i32 launch;
    u64* n_bad;            // rows skipped for an action out of range (the word lob_vec_status reports and clears)
};
// vec_feat_kernel<books, update>: a persistent grid of at most LOB_VECFEAT_MAX_BLOCKS blocks, sized from the compute units (`n_cus`)
void lobk_vec_feat(hipStream_t st, int n_cus, const DevParams* Pd, const DevState* Sd, const uint32_t* rnd, const VecFeatSrc& a);

// ---- lob_tu_vecpeek.hip ----
// What lob_vec_peek (include/lob_engine.h) takes beyond the parameters and the state, which vec_peek_kernel receives as env_kernel
// does: the actions of the mask in ascending order, the batch and its size rounded up to whole waves -- block i of the grid is action
// act[i / (Bpad / 64)] over the books 64 * (i % (Bpad / 64)) ... -- and the caller's device buffers, action-major planes.
struct PeekSrc {
    i32 B, Bpad;           // books; B rounded up to a multiple of 64
    i32 n_act;             // actions in the mask
    uint8_t act[12];       // [n_act] the set bits of the mask, ascending
    lob_vec_peek_out out;  // obs [9][B][V], reward [9][B], terminal [9][B], stepped [9][B]; NULL: not wanted
    u64* look_cnt;         // `ring` launches: the engine's words [0] ahead, [1] behind cells (lob_vec_status); last, so nothing above moves
};
// vec_peek_kernel<t2, ring>: n_act * Bpad / 64 one-wave blocks; `t2` as lobk_env's; `ring`: the look-ahead over a ring track (lob_peek.h)
void lobk_vec_peek(hipStream_t st, bool t2, bool ring, const DevParams* Pd, const DevState& S, const PeekSrc& a);

// ---- lob_tu_vecroll.hip ----
// What lob_vec_rollout (include/lob_engine.h) takes beyond the parameters and the state, which vec_rollout_kernel receives as
// env_kernel does: the plans' actions [P][H][B], the batch and its size rounded up to whole waves -- block i of the grid is plan
// i / (Bpad / 64) over the books 64 * (i % (Bpad / 64)) ... --, the discount, the caller's device buffers (plan-major planes) and the
// engine's workspace for the PnL windows' entries a plan itself has pushed: `shadow` [2][w][n_plans * Bpad] f64, lane
// p * Bpad + b innermost, null unless the reward reads the windows and 1 < lb_pnl < horizon.
struct RolloutSrc {
    const i32* actions;    // [n_plans][horizon][B]
    i32 B, Bpad;           // books; B rounded up to a multiple of 64
    i32 n_plans, horizon;
    f64 gamma;
    f64* shadow;
    lob_vec_rollout_out out;
    u64* look_cnt;         // `ring` launches: as PeekSrc's
};
// vec_rollout_kernel<t2, ring>: n_plans * Bpad / 64 one-wave blocks; `t2`, `ring` as lobk_vec_peek's
void lobk_vec_rollout(hipStream_t st, bool t2, bool ring, const DevParams* Pd, const DevState& S, const RolloutSrc& a);

// ---- lob_tu_branch.hip ----
// What lob_branch_fork / lob_branch_step / lob_branch_select (include/lob_engine.h) take beyond the parameters and the state, which
// branch_fork_kernel and branch_step_kernel receive as env_kernel does (branch_select_kernel: the parameters only): the set the launch
// writes (lob_branch.h: base, lanes, ring lengths), for a select the buffer it gathers from, the caller's [N][B] words -- actions for
// a step, parents for a select --, the batch and its size rounded up to whole waves -- block i of the step and select grids is branch
// i / (Bpad / 64) over the books 64 * (i % (Bpad / 64)) ... -- and the caller's device buffers, branch-major planes.
struct BranchSrc {
    BranchSet set;         // fork, step: the live buffer; select: the buffer that becomes the live one
    BranchSet from;        // select: the live buffer as it stands (fork, step: unused)
    const i32* index;      // step: actions [N][B]; select: parents [N][B]; fork: unused
    i32 B, Bpad;           // books; B rounded up to a multiple of 64
    i32 n_branches;
    lob_branch_out out;    // obs [N][B][V], reward [N][B], terminal [N][B], stepped [N][B]; NULL: not wanted
    u64* look_cnt;         // step, `ring` launches: as PeekSrc's
};
// branch_fork_kernel: Bpad / 64 one-wave blocks, a lane per book writing its N copies
void lobk_branch_fork(hipStream_t st, const DevParams* Pd, const DevState& S, const BranchSrc& a);
// branch_step_kernel<t2, ring>: n_branches * Bpad / 64 one-wave blocks; `t2`, `ring` as lobk_vec_peek's
void lobk_branch_step(hipStream_t st, bool t2, bool ring, const DevParams* Pd, const DevState& S, const BranchSrc& a);
// branch_select_kernel: n_branches * Bpad / 64 one-wave blocks
void lobk_branch_select(hipStream_t st, const DevParams* Pd, const BranchSrc& a);

// ---- lob_tu_branchobs.hip ----
// What lob_branch_book / lob_branch_history (include/lob_engine.h) read, as kernel arguments: the LIVE buffer of the set (lob_branch.h:
// the field words of branch n of book b at lane n * Bpad + b), and what VecBookSrc / VecHistSrc name of the engine -- the event records,
// the first record and the length of every BOOK's stream (indexed by b, never by the lane) and the words of a record at which its
// arrays start.  Outputs are branch-major: row n * B + b, no padding to Bpad.
struct BranchObsSrc {
    BranchSet set;             // the live buffer
    const uint32_t* records;   // DevState::records / rec_phase (null: book b's stream starts at record b * n_events)
    const i64* rec_phase;
    const i32* rec_len;        // DevState::rec_len (null: every stream has n_events records)
    i32 n_events, Wd, D, T;
    i32 w_ask_px, w_ask_vol, w_bid_px, w_bid_vol, w_trades;
    i32 B, Bpad;               // books; B rounded up to a multiple of 64
    i32 n_branches;
};
// branch_book_kernel: n_branches * Bpad / 64 blocks of LOB_VECBOOK_BLOCK threads, block i branch i / (Bpad / 64)
void lobk_branch_book(hipStream_t st, const BranchObsSrc& s, const lob_vec_book_out& out);
// branch_hist_kernel: a block per LOB_VECHIST_ROWS rows of the flat [n_branches x B x K] row space
void lobk_branch_history(hipStream_t st, const BranchObsSrc& s, int K, const lob_vec_hist_out& out);

// ---- lob_tu_learn.hip ----
// learn_q_pair_kernel / learn_q_lane_kernel<algo, vt, tr>: vt = 8 when the state has eight variables (else 0)
void lobk_learn_q(hipStream_t st, bool pair, int algo, bool v8, bool tr, int grid, size_t lds, const DevParams* Pd, const DevState& S, const uint32_t* rnd,
                  int lpar, u64 ver, int sid, int acc_fuse);
void lobk_learn_q_fast(hipStream_t st, int algo, int grid, size_t lds, const DevParams* Pd, const DevState& S, const uint32_t* rnd, int lpar, u64 ver);
// hipFuncAttributeMaxDynamicSharedMemorySize of every instantiation above
hipError_t lobk_learn_set_lds(int fast_lds, int lane_lds, int pair_lds);

#endif
