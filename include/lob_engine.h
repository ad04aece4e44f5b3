/*
 * lob_engine.h — C ABI of the MI355X-native batched limit-order-book
 * environment + tile-coded TD(lambda) learner.
 *
 * This is the drop-in boundary for the ONE hot path of tspooner/rl_markets
 * (SURVEY.md §8): `market::Book` / `environment::Intraday` step, state/reward
 * extraction, CMAC tile coding and the linear-Q SARSA(lambda)/Q(lambda)
 * update, batched struct-of-arrays over thousands of independent books and
 * executed by hand-written HIP kernels for gfx950.  Plain pointers and sizes
 * only: no C++/torch types cross this boundary.  The reference has no FFI
 * layer of its own; each entry point below names the reference C++ interface
 * it stands in for (paths relative to the reference checkout).
 *
 * Conventions
 *   - every function returning `int` returns LOB_OK (0) or a negative
 *     LOB_E* code; `lob_last_error()` gives a human-readable message
 *     (the reference throws std::runtime_error / returns bool — see
 *     INTEGRATION.md for the mapping);
 *   - "host" pointers are caller-owned host memory, "dev" pointers are device
 *     (HBM) addresses valid on the engine's GPU;
 *   - one engine handle per GPU, not thread-safe per handle (same rule as the
 *     reference: one Environment + Runner per thread, src/main.cpp:45-58).
 *   - the library needs a gfx950 GPU: there is NO CPU fallback.  Without a
 *     device `lob_create` fails with LOB_ENODEV.
 */
#ifndef LOB_ENGINE_H
#define LOB_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOB_ABI_VERSION 6

#define LOB_N_ACTIONS 9   /* reference Intraday::DoAction table, src/environment/intraday.cpp:181-219 */
#define LOB_N_TILINGS 32  /* config/example.yaml:18 (compile-time in the kernels) */
#define LOB_MAX_DEPTH 10
#define LOB_MAX_TRADES 8
#define LOB_MAX_BANDS 20
#define LOB_MAX_VARS 13
#define LOB_MAX_WINDOW 256
#define LOB_TRACE_GENS 64 /* largest trace ring, in generations of 32 tiles: gamma*lambda up to ~0.93;
                             the engine allocates 32 when the decay allows (example.yaml: 25 generations) */

enum {
    LOB_OK = 0,
    LOB_EINVAL = -1,   /* bad argument / unsupported parameter */
    LOB_ENODEV = -2,   /* no usable gfx950 device */
    LOB_ENOMEM = -3,   /* hipMalloc failed */
    LOB_ESTATE = -4,   /* call sequence error (e.g. step before reset) */
    LOB_EDATA = -5,    /* malformed event stream (the reference throws, src/market/book.cpp:74-77) */
    LOB_EHIP = -6      /* HIP runtime error */
};

/* Variable ids: reference enum class Variable, include/environment/intraday.h:17-24 */
enum {
    LOB_VAR_POS = 0, LOB_VAR_SPD, LOB_VAR_MPM, LOB_VAR_IMB, LOB_VAR_SVL, LOB_VAR_VOL,
    LOB_VAR_RSI, LOB_VAR_VWAP, LOB_VAR_A_DIST, LOB_VAR_A_QUEUE, LOB_VAR_B_DIST,
    LOB_VAR_B_QUEUE, LOB_VAR_LAST_ACTION
};

/* Reward measures: reference enum class RewardMeasure, include/environment/base.h:24-35 */
enum {
    LOB_REWARD_NONE = 0, LOB_REWARD_PNL, LOB_REWARD_PNL_DAMPED, LOB_REWARD_SPREAD,
    LOB_REWARD_NORMED, LOB_REWARD_LOVOL, LOB_REWARD_MM_LINEAR, LOB_REWARD_MM_EXP,
    LOB_REWARD_MM_DIV
};

/* Target-price object actually instantiated by the reference factory
 * (src/environment/base.cpp:101-112, quirk Q5: "midprice" -> MicroPrice,
 * anything else -> MidPrice) and the quoting mode of the Intraday ctor
 * (src/environment/intraday.cpp:64-82). */
enum { LOB_TP_MIDPRICE = 0, LOB_TP_MICROPRICE = 1 };
enum { LOB_QUOTE_TARGET = 0, LOB_QUOTE_BOOK = 1 };

/* Learning algorithms: rl::SARSA (src/rl/agent.cpp:296-311),
 * rl::QLearn = Watkins Q(lambda) (src/rl/agent.cpp:268-292),
 * rl::DoubleQLearn (src/rl/agent.cpp:185-264,315-353; config/example.yaml's default): a second
 * weight vector theta_b (`which` = 1 in lob_theta_get/set for shared theta, book + n_books for
 * private), actions from (Qa+Qb)/2, a coin flip per step from the agent's own
 * std::mt19937_64 (seeded with seed + global book id) choosing which vector is updated. */
/* SARSA / QLearn / DoubleQLearn (src/rl/agent.cpp:268-353); RLearn / OnlineRLearn / DoubleRLearn (average-reward:
 * src/rl/agent.cpp:357-467, selected by learning.algorithm r_learn / online_r_learn / double_r_learn, src/main.cpp:179-186;
 * they run the general kernels). */
enum { LOB_ALGO_SARSA = 0, LOB_ALGO_QLAMBDA = 1, LOB_ALGO_DOUBLE_Q = 2, LOB_ALGO_R_LEARN = 3, LOB_ALGO_ONLINE_R_LEARN = 4,
       LOB_ALGO_DOUBLE_R_LEARN = 5 };

/* Weight sharing: one theta shared by all books of the engine (the batched
 * analogue of the reference's Hogwild threads, src/main.cpp:196-206), or one
 * private theta per book (B independent learners = B copies of the
 * single-book reference; used for exact parity tests). */
enum { LOB_THETA_SHARED = 0, LOB_THETA_PRIVATE = 1 };

/* Behaviour policy: rl::EpsilonGreedy (src/rl/policy.cpp:58-82; epsilon 0 = rl::Greedy, 1 = rl::Random's
 * uniform action) or rl::Boltzmann (policy.cpp:85-122): P(a) ~ exp(Q(a) / tau), one uniform draw.
 * The exponential is glibc 2.35's exp(double) restated on the device from the library's own table and constants
 * (rl_markets_amd/csrc/lob_exp_table.h; tools/check_exp.c: 0 differences from libm over 4e8 inputs), so the sampled
 * action -- an index -- is bit-exact like every other. */
enum { LOB_POLICY_EPS_GREEDY = 0, LOB_POLICY_BOLTZMANN = 1 };

/* Venue description: reference market::Market (include/market/market.h:13-52).
 * Bands ascending by lower bound, as std::map<double,double> pts_ iterates. */
typedef struct lob_market {
    int64_t open_ms;                   /* mo_ */
    int64_t close_ms;                  /* mc_ */
    int32_t n_bands;
    int32_t _pad;
    double band_lb[LOB_MAX_BANDS];     /* price lower bound of band i   */
    double band_tick[LOB_MAX_BANDS];   /* tick size inside band i       */
} lob_market;

/* Engine parameters = the subset of the reference YAML config the hot path
 * reads (config/example.yaml; consumers src/environment/base.cpp:14-115,
 * src/rl/agent.cpp:13-60, src/rl/policy.cpp:58-82). */
typedef struct lob_params {
    int32_t abi_version;        /* LOB_ABI_VERSION */
    int32_t depth;              /* book levels per side, 1..LOB_MAX_DEPTH (reference: 5, quirk Q18) */
    int32_t max_trades;         /* trade price levels per event, 1..LOB_MAX_TRADES */
    int32_t n_vars;             /* state variables V (example.yaml: 8) */
    int32_t vars[LOB_MAX_VARS]; /* LOB_VAR_* in config order */

    lob_market market;

    int32_t order_size;         /* market.order_size */
    int32_t reward_measure;     /* LOB_REWARD_* */
    int64_t pos_lb, pos_ub;     /* market.pos_lb / pos_ub */
    float damping_factor;       /* reward.damping_factor (float in the reference) */
    float pos_weight, trd_weight, pnl_weight;

    int32_t lb_mpm, lb_vlt, lb_svl, lb_vwap, lb_rsi; /* state.lookback.* (>=1 after max(.,1)) */
    int32_t lb_spread;          /* policy.spread_lookback */
    int32_t lb_pnl;             /* reward.pnl_lookback */
    int32_t lb_target;          /* market.target_price.lookback */
    int32_t target_price;       /* LOB_TP_* */
    int32_t quote_mode;         /* LOB_QUOTE_* */

    int64_t memory_size;        /* learning.memory_size M (theta length, < 2^31) */
    int32_t n_tilings;          /* must be LOB_N_TILINGS */
    int32_t n_actions;          /* must be LOB_N_ACTIONS */
    double group_weights[3];    /* learning.group_weights */
    double gamma, lambda;
    double alpha;               /* current step size (alpha schedule is host-side, lob_set_alpha) */
    double epsilon;             /* current epsilon (schedule host-side, lob_set_epsilon) */
    int32_t algo;               /* LOB_ALGO_* */
    int32_t theta_mode;         /* LOB_THETA_* */
    uint64_t seed;              /* counter-based policy RNG seed (DESIGN.md "RNG") */
    uint64_t book_id_offset;    /* global id of local book 0 (multi-GPU shards) */
    int32_t policy;             /* LOB_POLICY_* */
    int32_t random_init;        /* learning.random_init (src/rl/agent.cpp:37-39,190-192): 0 = every weight +0.0; 1 = every weight 2u - 1, u
                                 * drawn in index order from the agent's own std::mt19937_64 (debug.random_seed; theta, then theta_b
                                 * of the double agents) -- private theta: every book's agent draws its own vectors (seed + global
                                 * book id, as for the coin); shared theta: the one vector is global book 0's agent's, whatever
                                 * shard this engine holds, and that agent's generator moves on as in the reference */
    double tau;                 /* Boltzmann temperature (schedule host-side, lob_set_tau) */
    double beta;                /* learning.beta: step size of the average reward rho (R-learning agents) */
} lob_params;

/* Synthetic event-stream generator. */
typedef struct lob_gen_params {
    uint64_t seed;
    int32_t n_events;
    int32_t t0_ms;              /* timestamp of event 0 */
    int32_t dt_ms;              /* cadence */
    int32_t start_ticks;        /* best bid = start_ticks * tick (0.1-tick grid of LSE HSBA band [500,1000)) */
    int32_t min_ticks, max_ticks;
    int32_t move_prob_q16;      /* P(best bid moves +-1 tick) * 65536 */
    int32_t spread2_prob_q16;   /* P(spread == 2 ticks) * 65536 */
    int32_t trade_prob_q16;     /* P(a trade in the interval) * 65536 */
    int32_t trade2_prob_q16;    /* P(a second trade on the other side | first) * 65536 */
    int32_t touch_prob_q16;     /* P(trade at touch rather than 2nd level) * 65536 */
    int32_t vol_min, vol_max;   /* level volumes U{min..max} */
    int32_t trade_min, trade_max;
} lob_gen_params;

/* Parity dump of one book's full environment state (test / debugging aid;
 * mirrors the protected members of environment::Base, include/environment/base.h:39-95,
 * and market::Book, include/market/book.h:34-48). */
typedef struct lob_book_dump {
    double ask_px[LOB_MAX_DEPTH], bid_px[LOB_MAX_DEPTH];
    double ask_last_px[LOB_MAX_DEPTH], bid_last_px[LOB_MAX_DEPTH];
    int64_t ask_vol[LOB_MAX_DEPTH], bid_vol[LOB_MAX_DEPTH];
    int64_t ask_last_vol[LOB_MAX_DEPTH], bid_last_vol[LOB_MAX_DEPTH];
    int64_t ask_total_volume, bid_total_volume;
    int64_t ask_last_total_volume, bid_last_total_volume;
    int32_t ask_n_transacted, bid_n_transacted;
    /* the (at most one, quirk Q13) live order per side */
    int32_t ask_has_order, bid_has_order;
    double ask_order_px, bid_order_px;
    int64_t ask_order_rem, bid_order_rem;
    int64_t ask_q_head, bid_q_head, ask_q_tail, bid_q_tail;
    int64_t position;
    double ask_quote, bid_quote;
    int32_t ask_level, bid_level;
    double pnl_step, momentum_pnl_step;
    int32_t lo_vol_step;
    int32_t last_action;
    double episode_reward, episode_pnl, episode_bandh;
    double spread_mean, target_price;
    int64_t time_ms;
    int32_t cursor;            /* next unread event index */
    int32_t terminal;          /* 1 = isTerminal(), 2 = stream exhausted */
    int32_t total_ticks;       /* TickStatistics::total_ticks */
    int32_t n_traces;          /* live eligibility traces */
    /* TradeStatistics / TickStatistics of the episode (include/environment/statistics.h:19-50): what Base::ClearInventory
     * (base.cpp:339-349) and Base::UpdateStats (base.cpp:412-442) count; the reference never touches the placed / cancelled /
     * "no ..." counters */
    int32_t market_buys, market_sells;
    int32_t ticks_with_ask, ticks_with_bid, ticks_with_both;
    int32_t ticks_with_position, ticks_long, ticks_short;
    /* TradeStatistics::ask_transactions / bid_transactions: ask/bid_n_transacted AS OF THE LAST DECISION -- Base::UpdateStats
     * (base.cpp:415-416) copies them when performAction has placed its orders (base.cpp:278), before the step's events run;
     * what the step's own events fill shows here one decision later (after an episode's last step: never).  getTotalTransactions /
     * getOrderRatio / writeStats (base.cpp:451-473) read these. */
    int32_t ask_transactions, bid_transactions;
} lob_book_dump;

typedef struct lob_engine lob_engine;

/* ---- library / parameter helpers (host only, no GPU needed) -------------- */

int lob_abi_version(void);
const char* lob_last_error(void);

/* config/example.yaml defaults (D=5, T=2, 8 vars, SARSA, LSE HSBA venue). */
void lob_default_params(lob_params* p);

/* Venue tables: reference Market::make_market, src/market/market.cpp:39-59
 * (tables :142-314).  `ticker` = "SYMBOL.VENUE", e.g. "HSBA.L". */
int lob_market_preset(const char* ticker, lob_market* out);

/* Tick maths on the host (reference Market::ToTicks / ToPrice / tick_size,
 * src/market/market.cpp:78-138).  Exposed for the host adaptors and tests. */
int lob_to_ticks(const lob_market* m, double price, int32_t* ticks);
int lob_to_price(const lob_market* m, int32_t ticks, double* price);
int lob_tick_size(const lob_market* m, double price, double* tick);

/* ---- event streams -------------------------------------------------------
 * One record per (book, event), little-endian 32-bit words:
 *   [0] time_ms  [1] flags
 *   ask_px[D] f32, ask_vol[D] i32, bid_px[D] f32, bid_vol[D] i32,
 *   trade_px[T] f32 (ascending), trade_vol[T] i32 (0 = empty slot),
 *   zero padding to a multiple of 4 words.
 * An event = what one Intraday::NextState consumes (src/environment/intraday.cpp:225-272):
 * the trades aggregated per price since the previous depth snapshot
 * (data::TimeAndSalesRecord, include/data/records.h:30-37) followed by the
 * new depth snapshot (data::MarketDepthRecord, include/data/records.h:20-28).
 * Layout in memory: records[book][event] (each book's events contiguous).
 */
#define LOB_EVT_FLAG_SAME_TIME 1u /* more depth rows with this timestamp follow (quirk Q14) */
#define LOB_EVT_FLAG_TAS_DRY 2u   /* no event may START at this row: the time-and-sales stream has run dry (Streamer::LoadUntil
                                   * fails, src/data/streamer.cpp:61-85, so Intraday::NextState returns false before it
                                   * touches the books); set by lob_convert_csv from the last trade rows of the file */

int32_t lob_record_words(int32_t depth, int32_t max_trades);
void lob_default_gen_params(lob_gen_params* g);
/* Fill `out` (n_books * n_events * record_words * 4 bytes) on the host. */
int lob_gen_stream_host(const lob_gen_params* g, int32_t depth, int32_t max_trades,
                        uint64_t first_book_id, int32_t n_books, uint32_t* out);
/* Check a host stream against the engine preconditions (positive prices and
 * volumes, strictly monotone price keys per side, ascending trade prices, and no more than max_trades distinct trade price
 * keys in the rows whose trades one event merges: those after the previous event's first row up to its own first row, where
 * a row ends an event when the next row's time differs and the book it leaves is a valid state -- otherwise a step would end in
 * "more trade price levels in one event than max_trades"). */
int lob_validate_stream(const uint32_t* records, int32_t depth, int32_t max_trades,
                        int32_t n_books, int32_t n_events);

/* ---- ingestion of recorded data -------------------------
 * lob_convert_csv: the reference's two CSV formats (include/data/basic.h:17-24,49-52:
 * 22-column 5-level market depth, 4-column time-and-sales; header row skipped,
 * `stof` prices, rows with a non-positive price dropped, src/data/basic.cpp:45-70,
 * 148-162) -> one record per depth row carrying the trades of its own interval
 * (time-and-sales rows with prev_depth_time < time <= depth_time, aggregated per
 * 1e-4 price key like TimeAndSalesRecord::transactions).  Depth is 5.
 * lob_convert_lobster: LOBSTER message + orderbook files (prices x 10000): one
 * record per distinct millisecond = last snapshot of that millisecond + the
 * executions (types 4, 5) of that millisecond aggregated per price; the first
 * `depth` of `levels_in_file` levels are kept, records with a missing level are
 * dropped.  Both allocate *out_records (n_events * lob_record_words * 4 bytes);
 * release with lob_free. */
int lob_convert_csv(const char* md_path, const char* tas_path, int32_t max_trades, uint32_t** out_records,
                    int32_t* n_events);
int lob_convert_lobster(const char* orderbook_path, const char* message_path, int32_t levels_in_file, int32_t depth,
                        int32_t max_trades, uint32_t** out_records, int32_t* n_events);
void lob_free(void* p);

/* ---- engine lifetime ----------------------------------------------------- */

/* Replaces constructing environment::Intraday<> + rl::Agent + serial::Learner
 * (src/main.cpp:45-58,140-189) for `n_books` books on GPU `device`. */
int lob_create(const lob_params* p, int32_t n_books, int32_t device, lob_engine** out);
void lob_destroy(lob_engine* e);

/* Replaces Intraday::LoadData (src/environment/intraday.cpp:141-150):
 * upload host records / synthesise the same records directly in HBM.
 * 2 <= n_events (an int32: the per-book TickStatistics counters are 32-bit like the reference's ints, one count per agent
 * step, and an agent step consumes at least one event). */
int lob_load_events(lob_engine* e, const uint32_t* host_records, int32_t n_events);
int lob_gen_events_device(lob_engine* e, const lob_gen_params* g);
/* The NEXT episode's per-book streams, handed over WHILE the current episode runs -- the reference loads a fresh day before every
 * episode (src/main.cpp:53-55: rs.sample() + env.LoadData per episode and thread): validation and the host-to-HBM copy run on a
 * host thread and a HIP stream of their own into a second record buffer (another n_books x n_events records of HBM) and the call
 * returns at once; the lob_reset that follows waits for the hand-over if it has to and makes the staged stream the current one.
 * `host_records` must stay valid until that lob_reset (or lob_stage_wait) returns; n_events must equal the loaded stream's.
 * lob_stage_wait: block until the hand-over is complete and return its status (LOB_EDATA etc. as lob_load_events would). */
int lob_stage_events(lob_engine* e, const uint32_t* host_records, int32_t n_events);
int lob_stage_wait(lob_engine* e);
/* One recorded stream replayed by every book (BASELINE config 5: a converted LOBSTER day):
 * `host_records` holds n_total records of ONE book; book b plays the n_events records
 * starting at record phase[b] (0 <= phase[b], phase[b] + n_events <= n_total), i.e. it
 * behaves exactly like a book loaded with that window through lob_load_events.  The
 * reference replays one file pair per episode and thread (Intraday::LoadData,
 * src/environment/intraday.cpp:141-150; file cycling in src/experiment/serial.cpp:38-50);
 * the phases stand in for its per-thread choice of episode file. */
int lob_load_events_shared(lob_engine* e, const uint32_t* host_records, int64_t n_total, const int64_t* phase,
                           int32_t n_events);
/* A library of recorded days resident in HBM, a day drawn per book and episode on the device (the reference's training loop:
 * rs.sample() + env.LoadData before every episode, src/main.cpp:51-55, include/utilities/sampler.h:29-46; its test loop,
 * src/main.cpp:215-239).  lob_load_days: `host_records` holds the n_days days back to back, day d is records
 * day_first[d] .. day_first[d + 1] - 1 (day_first: int64[n_days + 1], day_first[0] = 0, at least 2 events per day); every
 * day is validated and the library uploaded once.  It replaces any stream loaded before; lob_reset returns LOB_ESTATE
 * until a selection has been made, and lob_stage_events returns LOB_ESTATE while the library is loaded (lob_load_events,
 * lob_load_events_shared and lob_gen_events_device return the engine to their modes).  The track is sized by the longest
 * day: a ring when that day is longer than the resident track.
 * lob_days_select: every book draws its next day from days first_day .. first_day + n_days - 1.  LOB_DAYS_RANDOM:
 * std::uniform_int_distribution<size_t>{0, n_days - 1} over each book's std::default_random_engine, seeded with
 * (unsigned)(seed + global book id) at lob_load_days and persisting across draws.  LOB_DAYS_IN_ORDER: global book g plays
 * first_day + g mod n_days.  lob_days_set: the day of every book from the host (int32[n_books]).  Both are enqueued on the
 * engine's stream without waiting for it and take effect at the next lob_reset; a lob_reset without a new selection
 * replays the same days.  LOB_EINVAL: a day out of range; LOB_ESTATE: no library, or between lob_td_step_begin and
 * lob_td_step_end.  lob_get_days: the day each book is playing (int32[n_books]; LOB_ESTATE before the first lob_reset on
 * the library). */
#define LOB_DAYS_RANDOM 0
#define LOB_DAYS_IN_ORDER 1
int lob_load_days(lob_engine* e, const uint32_t* host_records, const int64_t* day_first, int32_t n_days);
int lob_days_select(lob_engine* e, int32_t mode, int32_t first_day, int32_t n_days);
int lob_days_set(lob_engine* e, const int32_t* host_day);
int lob_get_days(lob_engine* e, int32_t* host_out);

/* ---- environment interface (environment::Base, include/environment/base.h:117-151) */

/* Initialise() for every book: clear books/stats/windows, fast-forward to
 * market open, warm the windows, place the (1,1) quotes, extract the first
 * state and its tile features (Runner::RunEpisode prologue,
 * src/experiment/serial.cpp:18-26). */
int lob_reset(lob_engine* e);
/* performAction(action) for every live book; `actions` host int32[n_books]. */
int lob_step(lob_engine* e, const int32_t* host_actions);
/* getState(): host float[n_books][n_vars]. */
int lob_get_state(lob_engine* e, float* host_out);
/* getReward(): host double[n_books]. */
int lob_get_reward(lob_engine* e, double* host_out);
/* isTerminal() (1) / out of data (2) / live (0): host uint8[n_books]. */
int lob_get_terminal(lob_engine* e, uint8_t* host_out);
/* ClearInventory() for every book (Runner::RunEpisode epilogue, serial.cpp:31). */
int lob_clear_inventory(lob_engine* e);
int lob_get_book(lob_engine* e, int32_t book, lob_book_dump* out);
int lob_get_books(lob_engine* e, int32_t first, int32_t n, lob_book_dump* out);

/* ---- vector-env interface: step and observe without the host ---------------
 * The environment face above (lob_step + lob_get_state / lob_get_reward / lob_get_terminal) for a policy that lives on the
 * GPU: actions are read from device memory, the observations are written to device memory, and everything is enqueued on
 * the engine's stream (lob_stream) -- no host read of the actions, no allocation, no copy to or from the host and no
 * synchronisation per step.  It stands in for the same members of environment::Base (include/environment/base.h:117-151:
 * performAction, getState, getReward, isTerminal) inside the loop of Runner::RunEpisode (src/experiment/serial.cpp:18-34:
 * `while (!env.isTerminal()) _step()`).
 *   lob_vec_out: where the results go, all DEVICE pointers on the engine's GPU, written in stream order; a NULL member is
 * skipped.  After either call
 *     terminal[b] = what lob_get_terminal reports at that moment; n_live = the number of zeros among them;
 *     a book with stepped == 1: obs and reward are bit for bit what lob_get_state / lob_get_reward return right after;
 *     every other book: reward 0.0 (lob_vec_step), obs = the state of its last completed step, or of the reset -- the
 *     vector its rl::State last took from getState().  Wherever terminal != 2 that is lob_get_state's row as well.
 *   lob_vec_step: performAction(dev_actions[b]) for every book that is live at entry (terminal == 0) -- the runner's
 * `while (!env.isTerminal())`.  A book that is over keeps its state, stepped 0.  A step that runs out of data leaves
 * terminal == 2 and stepped == 0, as with lob_step.  WHERE lob_step DIFFERS: lob_step steps every book with done != 2,
 * also one whose session is over (terminal == 1), and refuses the whole call for one action out of range.  Here an action
 * outside [0, LOB_N_ACTIONS) is never used as an index: that book is not stepped in this call (state untouched, stepped 0)
 * and the entry is counted in a device word of the engine's until lob_vec_status reads it (every out-of-range entry of
 * dev_actions counts, whether or not its book is live).  The step log gets the row of a book stepped here exactly as from
 * lob_step, and a ring-mode track is refilled on its schedule.  LOB_ESTATE before the first lob_reset and between
 * lob_td_step_begin and lob_td_step_end; LOB_EINVAL for a NULL engine, dev_actions or out.
 *   lob_vec_observe: the same outputs without a step (after lob_reset, after lob_clear_inventory): stepped is written 0,
 * reward is what lob_get_reward returns, obs is lob_get_state's row wherever terminal != 2.
 *   lob_vec_status: the one call of this interface that waits.  It synchronises the stream once and returns what the other
 * entry points report after their steps (LOB_EDATA and its message); otherwise LOB_EINVAL if any action was out of range
 * since the last call.  *n_bad_actions (may be NULL) gets that count, and the word is cleared; lob_reset clears it too. */
typedef struct lob_vec_out {      /* all DEVICE pointers on the engine's GPU; any may be NULL = not wanted */
    float*   obs;                 /* [n_books][n_vars] row-major: getState()                        */
    double*  reward;              /* [n_books]: getReward() of a stepped book, 0.0 otherwise        */
    uint8_t* terminal;            /* [n_books]: 0 / 1 / 2 as lob_get_terminal                       */
    int32_t* stepped;             /* [n_books]: 1 where this call ran a performAction to its end    */
    int32_t* n_live;              /* one word: books with terminal == 0 after the call              */
} lob_vec_out;
int lob_vec_step(lob_engine* e, const int32_t* dev_actions, const lob_vec_out* out);
int lob_vec_observe(lob_engine* e, const lob_vec_out* out);
int lob_vec_status(lob_engine* e, int64_t* n_bad_actions);

/* ---- vector-env interface: the order book itself, written to device memory ---
 * What a network behind lob_vec_step wants to see beyond the `n_vars` hand-made variables of lob_vec_out::obs: the `depth`
 * levels of both sides of every book (market::Book's current snapshot, include/market/book.h:34-48) and the agent's own
 * standing orders, queue positions, inventory and episode sums (the protected members of environment::Base,
 * include/environment/base.h:39-95) -- until now only reachable through the parity dump lob_get_books (912 bytes per book, to
 * the host).
 *   lob_vec_book_out: where the values go, all DEVICE pointers on the engine's GPU, written in stream order; a NULL member is
 * skipped.  ONE rule: for EVERY book b, whatever its `terminal` value, every written element is the lob_book_dump field that
 * lob_get_books would report for b at that point of the stream, converted f64 -> f32 and int64 / int32 -> f32 by IEEE
 * round-to-nearest-even (a NaN stays a NaN); time_ms is copied as int64.
 *     levels[b][0][l] = (float)ask_px[l]   levels[b][1][l] = (float)ask_vol[l]
 *     levels[b][2][l] = (float)bid_px[l]   levels[b][3][l] = (float)bid_vol[l]      l < depth (lob_params::depth, not
 *     LOB_MAX_DEPTH); level 0 is the touch.  Where the dump has price 0.0 (no snapshot yet) price and volume are 0.
 *     own[b][LOB_OWN_*]: the sixteen dump fields named below, in that order; the order fields of a side without a live order
 *     are 0, *_order_rem is the order's remaining volume, as in the dump.
 *   lob_vec_book: enqueued on the engine's stream (lob_stream), returns at once -- no host read, no allocation, no copy and no
 * synchronisation -- and changes no engine state.  Valid whenever lob_get_books is meaningful: after the first lob_reset, after
 * lob_vec_step, lob_step, lob_td_step, lob_eval_step and lob_clear_inventory.  LOB_EINVAL for a NULL engine or a NULL out; a
 * struct whose three members are all NULL is LOB_OK and launches nothing.  LOB_ESTATE before the first lob_reset and between
 * lob_td_step_begin and lob_td_step_end. */
#define LOB_VEC_OWN_WORDS 16
#define LOB_OWN_POSITION 0
#define LOB_OWN_ASK_HAS_ORDER 1
#define LOB_OWN_ASK_ORDER_PX 2
#define LOB_OWN_ASK_ORDER_REM 3
#define LOB_OWN_ASK_Q_HEAD 4
#define LOB_OWN_BID_HAS_ORDER 5
#define LOB_OWN_BID_ORDER_PX 6
#define LOB_OWN_BID_ORDER_REM 7
#define LOB_OWN_BID_Q_HEAD 8
#define LOB_OWN_ASK_QUOTE 9
#define LOB_OWN_BID_QUOTE 10
#define LOB_OWN_LAST_ACTION 11
#define LOB_OWN_PNL_STEP 12
#define LOB_OWN_EPISODE_PNL 13
#define LOB_OWN_EPISODE_REWARD 14
#define LOB_OWN_TOTAL_TICKS 15
typedef struct lob_vec_book_out {   /* all DEVICE pointers on the engine's GPU; any may be NULL = not wanted */
    float*   levels;    /* [n_books][4][depth] row-major: plane 0 ask_px, 1 ask_vol, 2 bid_px, 3 bid_vol; level 0 = touch */
    float*   own;       /* [n_books][LOB_VEC_OWN_WORDS] */
    int64_t* time_ms;   /* [n_books] */
} lob_vec_book_out;
int lob_vec_book(lob_engine* e, const lob_vec_book_out* out);

/* ---- vector-env interface: the last K event records of every book, written to device memory ---
 * What a network over a WINDOW of book updates wants (a DeepLOB-style input: the last K events x 4 * depth level values, and the
 * trades that came with them): for every book the K most recent records of its own event stream, ending with the record its
 * current snapshot comes from -- the data::MarketDepthRecord (time, ask / bid prices and volumes per level) and the
 * data::TimeAndSalesRecord (trade prices and volumes) of each of the last K events, as one Intraday::NextState consumes them.
 * Between two agent steps a book consumes a variable number of events, so stacking successive lob_vec_book outputs does not give
 * this window; the records themselves are resident in device memory and are read there.
 *   lob_vec_hist_out: where the values go, all DEVICE pointers on the engine's GPU, written in stream order; a NULL member is
 * skipped.  ONE rule, for EVERY book b, whatever its `terminal` value.  Let r = rec[b], the record the book's current snapshot
 * comes from -- the one lob_get_books reads ask_px / ask_vol / bid_px / bid_vol from (cursor - 1 wherever terminal != 2); -1 when
 * the book has no snapshot.
 *     slot k (0 <= k < K) holds record r - (K - 1 - k) OF THAT BOOK'S STREAM: the n_events records loaded for it, the n_events
 *     records from phase[b] of a replayed stream (lob_load_events_shared), the records of the day it is playing (lob_load_days);
 *     a slot whose record index is negative is all zeros -- levels, trades and time --, never a record of the previous book, of the
 *     previous day or of the replayed stream before phase[b];
 *     levels[b][k][0][l] = ask_px[l]   levels[b][k][1][l] = ask_vol[l]   levels[b][k][2][l] = bid_px[l]   levels[b][k][3][l] =
 *     bid_vol[l], l < depth, level 0 the touch;  trades[b][k][0][i] = trade_px[i]   trades[b][k][1][i] = trade_vol[i], i <
 *     max_trades;  time_ms[b][k] = word 0 of the record.  Prices are the record's f32 bit for bit; volumes go int32 -> f32 by IEEE
 *     round-to-nearest-even; an empty trade slot is whatever the record holds (volume 0);
 *     n_valid[b] = min(K, r + 1), the slots k >= K - n_valid[b] that hold a record; 0 when the book has no snapshot.
 *   Every element of every non-NULL tensor is written on every call.  Slot K - 1 of `levels` is lob_vec_book's levels[b] for every
 * book with r >= 0.  K is the caller's, per call: any 1 <= K <= LOB_MAX_HISTORY is valid on any stream, also K > n_events.
 *   lob_vec_history: enqueued on the engine's stream (lob_stream), returns at once -- no host read, no allocation, no copy and no
 * synchronisation -- and changes no engine state.  Valid whenever lob_get_books is meaningful (see lob_vec_book).  LOB_EINVAL for a
 * NULL engine, a NULL out or K outside [1, LOB_MAX_HISTORY]; a struct whose five members are all NULL is LOB_OK and launches
 * nothing.  LOB_ESTATE before the first lob_reset and between lob_td_step_begin and lob_td_step_end. */
#define LOB_MAX_HISTORY 128
typedef struct lob_vec_hist_out {   /* all DEVICE pointers on the engine's GPU; any may be NULL = not wanted */
    float*   levels;    /* [n_books][K][4][depth]: planes ask_px, ask_vol, bid_px, bid_vol; level 0 = touch */
    float*   trades;    /* [n_books][K][2][max_trades]: plane 0 trade_px, plane 1 trade_vol                 */
    int32_t* time_ms;   /* [n_books][K]: word 0 of the record                                             */
    int32_t* n_valid;   /* [n_books]: min(K, rec + 1); 0 when the book has no snapshot                      */
    int32_t* rec;       /* [n_books]: index, within the book's own stream, of the record in slot K-1; -1 = none */
} lob_vec_hist_out;
int lob_vec_history(lob_engine* e, int32_t K, const lob_vec_hist_out* out);

/* ---- vector-env interface: save and restore the books on the device, by mask ---
 * What a policy on the GPU needs to go BACK: branch rollouts from one state, rewind the books that broke a limit, compare two
 * action sequences on common random numbers, restart the books that have finished while the others carry on.  Everything that
 * depends on the event stream alone is in the market track, written once per episode and indexed by the book's event count; the
 * agent-dependent state of a book is a few hundred bytes of struct-of-arrays words, and putting those back puts the book back --
 * no pre-pass, no stream, no host.
 *   A snapshot slot (0 <= slot < LOB_MAX_SNAPSHOTS) holds the environment state of all n_books books.  dev_mask: uint8 [n_books]
 * in DEVICE memory on the engine's GPU, read in stream order; a nonzero byte selects the book, NULL selects every book.
 *   ONE rule for restore.  A restored book continues exactly as it would have continued from the moment of the save: every later
 * lob_vec_step, lob_step, lob_vec_observe, lob_get_books, lob_get_state, lob_get_reward, lob_get_terminal, lob_vec_book,
 * lob_vec_history, lob_clear_inventory and lob_episode_stats gives, for that book, the bits it would have given then.  A book
 * restored from terminal 1 or 2 to a saved state with terminal == 0 is live again.  A book outside the mask is not touched, not
 * one byte of it.
 *   What is saved: the book's environment state only -- its order, inventory, PnL, cursor and statistics words, the two rolling
 * means of its own PnL (reward_measure LOB_REWARD_NORMED), the latest getState() and the environment's words of the step header
 * (done, time, action, stepped, reward).  The market's windows belong to the episode's pre-pass and are not saved.  The learner is
 * not touched: weights, traces, the two rl::State objects, the policy's random stream, TD errors and the memo tables stay as they
 * are, and the cumulative counters of lob_get_counters are not wound back.
 *   Learner calls after a restore: the learner's memory of the books' last transition then belongs to another trajectory, so
 * lob_td_step, lob_td_step_begin, lob_eval_step and lob_handle_terminal return LOB_ESTATE (the message names the restore) from any
 * successful lob_snapshot_restore until the next lob_reset.  The environment and vector-env calls go on working.
 *   A snapshot belongs to the episode it was taken in: lob_reset invalidates every slot (track, days and stream may change there;
 * the buffers stay allocated).  lob_snapshot_save with a NULL mask (re)starts the slot; with a mask it overwrites the selected
 * books of a slot that already holds a full save of this episode, and is LOB_ESTATE if the slot holds none.
 * lob_snapshot_restore of an empty or invalidated slot is LOB_ESTATE.
 *   lob_snapshot_save / lob_snapshot_restore: one kernel enqueued on the engine's stream (lob_stream); the call returns at once --
 * no host read, no copy, no synchronisation.  The only allocation is one hipMalloc the first time a slot is saved, kept until
 * lob_snapshot_free / lob_destroy: THE FIRST SAVE OF A SLOT SYNCHRONISES THE DEVICE (hipMalloc does), every later call does not.
 *   LOB_ESTATE also: before the first lob_reset; between lob_td_step_begin and lob_td_step_end; on an engine whose market track is
 * a ring (a stream longer than LOB_TRACK_RING events: entries before the cursor have been overwritten, so an earlier event count
 * cannot be served), for save and restore alike; on restore while the step log is enabled (its row rule total_ticks > n_rows +
 * n_lost cannot survive total_ticks going back).  LOB_EINVAL: a NULL engine, or a slot outside [0, LOB_MAX_SNAPSHOTS).
 * LOB_ENOMEM: the slot's buffer does not fit.  lob_snapshot_free releases the slot's buffer (after the work queued on the stream);
 * of an empty slot it is LOB_OK.  A refused call changes nothing. */
#define LOB_MAX_SNAPSHOTS 4
int lob_snapshot_save(lob_engine* e, int32_t slot, const uint8_t* dev_mask);
int lob_snapshot_restore(lob_engine* e, int32_t slot, const uint8_t* dev_mask);
int lob_snapshot_free(lob_engine* e, int32_t slot);

/* ---- vector-env interface: the engine's own Q values and policy actions, on the device ---
 * The one agent the interface above could not use: the engine's own tile-coded linear-Q agent.  lob_vec_act stands in for
 * Agent::getQ, Agent::action and Greedy::Sample / EpsilonGreedy::Sample / Boltzmann::Sample (src/rl/agent.cpp:117-169, 196-204;
 * src/rl/policy.cpp:37-117) over the whole batch, from device memory to device memory: lob_vec_act then lob_vec_step(action) is one
 * agent step of the engine's policy -- as a teacher, a baseline, an opponent or an epsilon-mix partner of a network on the same GPU,
 * and on books that lob_snapshot_restore has put back, where lob_eval_step and lob_td_step are refused.
 *   lob_vec_act_out: where the results go, DEVICE pointers on the engine's GPU, written in stream order; a NULL member is skipped.
 * ONE rule for EVERY book b, whatever its `terminal` value:
 *     q[b][a] = Agent::getQ(a) on the book's latest getState() vector -- the row lob_vec_step wrote to obs -- under the weights that
 *     book's agent uses (theta of book b under LOB_THETA_PRIVATE); for the double agents (LOB_ALGO_DOUBLE_Q, LOB_ALGO_DOUBLE_R_LEARN)
 *     (Qa + Qb) / 2.0, as DoubleAgent::action forms it.  Bit for bit the sum the reference computes; every element is written on
 *     every call.
 *     action[b], a live book (lob_get_terminal == 0): the mode's choice among q[b][.].  A sample is drawn from the book's own policy
 *     stream at its counter (lob_get_rng_counters) and the new counter is written back -- the draws lob_eval_step / lob_td_step make
 *     for the same values; that counter is the only word of engine state the call writes.
 *     action[b], a book with terminal != 0: 0, and nothing is drawn (lob_vec_step never counts it as out of range).
 *     action == NULL: nothing is sampled and no counter moves, in any mode.
 *   Modes:
 *     LOB_ACT_GREEDY     Agent::GoGreedy() then Agent::action -- what lob_eval_step plays: Greedy::Sample, ties among the maxima
 *                        broken by draws from the book's stream (none without a tie);
 *     LOB_ACT_BEHAVIOUR  the learner's behaviour policy at the current epsilon / tau (lob_set_epsilon, lob_set_tau): epsilon-greedy
 *                        or Boltzmann;
 *     LOB_ACT_ARGMAX     the lowest index among the maxima.  It draws nothing and changes not one byte of engine state.
 *   Nothing else changes: the learner's record of the last step, its verdicts, traces, written-weights maps and memo tables, the
 * step headers' action / stepped words and the counters of lob_get_counters stay as they are.
 *   lob_vec_act: enqueued on the engine's stream (lob_stream), returns at once -- no host read, no allocation, no copy and no
 * synchronisation.  Valid whenever lob_vec_book is, also after lob_snapshot_restore.  LOB_EINVAL for a NULL engine, a NULL out or a
 * mode outside 0..2; a struct whose two members are both NULL is LOB_OK and launches nothing.  LOB_ESTATE before the first lob_reset
 * and between lob_td_step_begin and lob_td_step_end.
 *   lob_vec_q: the device form of lob_q_values, for n free-standing states.  dev_vars: f32 [n][n_vars], dev_q: f64 [n][LOB_N_ACTIONS],
 * both in device memory on the engine's GPU.  The weights are the ones lob_q_values uses (theta; book 0's under private theta; Qa
 * only) and the output is bit for bit what it returns for the same rows.  Needs no lob_reset; enqueued like lob_vec_act, with no
 * allocation and no synchronisation.  LOB_EINVAL for a NULL engine or pointer, or n < 1. */
#define LOB_ACT_GREEDY    0
#define LOB_ACT_BEHAVIOUR 1
#define LOB_ACT_ARGMAX    2
typedef struct lob_vec_act_out {   /* DEVICE pointers on the engine's GPU; any may be NULL = not wanted */
    int32_t* action;   /* [n_books] */
    double*  q;        /* [n_books][LOB_N_ACTIONS]: the values the policy looked at */
} lob_vec_act_out;
int lob_vec_act(lob_engine* e, int32_t mode, const lob_vec_act_out* out);
int lob_vec_q(lob_engine* e, const float* dev_vars, int32_t n, double* dev_q);

/* ---- vector-env interface: the tile features of a state and external weight updates, on the device ---
 * The other direction of lob_vec_act / lob_vec_q: a learner on the same GPU sees the representation the engine's agent is built on
 * -- the CMAC tiles of State::populateFeatures (src/rl/state.cpp:56-63, src/rl/tiles.cpp:31-75) -- and lands any target it has
 * computed in the engine's weights as a semi-gradient step on the tiles of (state, action).  theta keeps its format: lob_theta_get,
 * lob_run and the reference's own agent read it, and lob_vec_act, lob_eval_step and lob_td_step use the new weights in the next call.
 *   Rows, in both calls (lob_vec_act / lob_vec_q's rule): dev_vars == NULL: the books' latest getState() -- the row lob_vec_step
 * wrote to obs --, n must be n_books and a lob_reset must have happened; else n >= 1 free-standing states, f32 [n][n_vars] in device
 * memory on the engine's GPU, and no lob_reset is needed.
 *   Tile positions: p = 32 g + j is tiling j of tile group g (0: the first three variables, 1: the others, 2: all) -- the order of
 * lob_features' last axis; LOB_N_TILES = 96 of them.
 *   lob_vec_terms: host_out[g * LOB_N_ACTIONS + a] = the action term of group g, reduced mod memory_size.  Host-only: it touches no
 * device and never fails for a valid engine and pointer.
 *   lob_vec_features: out->sums[s][p] = the action-independent hash sum of position p, reduced mod M = memory_size.  ONE contract
 * for all nine actions:
 *         (sums[s][p] + terms[g][a]) mod M   ==   lob_features' [s][a][p], bit for bit
 * -- 384 bytes per state where the cube takes 3 456.  0 <= sums < M <= 2^31 - 1 and 0 <= terms < M: DO THE ADDITION IN 64 BITS (or
 * unsigned 32), a signed 32-bit sum can overflow.  out->idx[s][p] = that index for a = dev_actions[s]; a row whose action is outside
 * [0, LOB_N_ACTIONS) gets -1 in all 96 places.  A NULL member is skipped (the buffer is not touched); both NULL: LOB_OK, nothing is
 * launched.  Nothing of the engine's state changes.
 *   lob_vec_update: for every row s whose action is in range and whose dev_step[s] != 0.0, dev_step[s] is added to each of the 96
 * weights of (row s, dev_actions[s]).  The increment is the caller's whole per-tile amount: the engine applies no alpha and does not
 * divide by the number of tilings (the learner's own step adds alpha * delta / 32 per tile).  Target: shared theta: the one vector;
 * private theta: book s's vector in the books' form, book 0's for free-standing rows (the vector lob_vec_q reads); second = 1: theta_b
 * -- LOB_EINVAL unless the algorithm is LOB_ALGO_DOUBLE_Q.  The action is looked at first: a row whose action is out of range is
 * skipped and counted in the word lob_vec_status reports and clears (no error flag is raised); then a row whose step is exactly 0.0
 * writes and marks nothing.  A non-finite step is the caller's business and is added as it is.  The additions are f64 atomics in no
 * fixed order, as the learner's own: a weight that several rows share receives its increments in an order that can differ from run
 * to run (exact whenever every partial sum is).  The written-weights maps, the verdicts and the memo records are kept as
 * lob_delta_apply keeps them; the multi-GPU base is NOT moved -- an external update is a local change and the next exchange carries
 * it.  Traces, rho, the random counters and the learner's record of the last step are not touched.
 *   Both device calls are enqueued on the engine's stream (lob_stream) and return at once: no host read, no allocation, no copy and
 * no synchronisation.  LOB_EINVAL, with a message naming the call: a NULL engine, a NULL out / dev_actions / dev_step where required
 * (idx wanted without dev_actions), n < 1, n != n_books in the books' form, second outside 0 / 1.  LOB_ESTATE: between
 * lob_td_step_begin and lob_td_step_end, and the books' form before the first lob_reset.  Allowed after lob_snapshot_restore: neither
 * call reads the learner's memory of the last transition. */
#define LOB_N_TILES 96            /* 3 groups x 32 tilings, the order of lob_features' last axis */
typedef struct lob_vec_feat_out { /* DEVICE pointers on the engine's GPU; NULL = not wanted */
    int32_t* sums;                /* [n][LOB_N_TILES] */
    int32_t* idx;                 /* [n][LOB_N_TILES]; needs dev_actions */
} lob_vec_feat_out;
int lob_vec_terms(lob_engine* e, int32_t host_out[27]);   /* [group][action], reduced mod memory_size */
int lob_vec_features(lob_engine* e, const float* dev_vars, int32_t n, const int32_t* dev_actions, const lob_vec_feat_out* out);
int lob_vec_update(lob_engine* e, const float* dev_vars, int32_t n, const int32_t* dev_actions, const double* dev_step, int32_t second);

/* ---- vector-env interface: one-step look-ahead over the nine actions, on the device ---
 * The environment as a model: "what would each action give me from here?" -- for one-step expectimax targets
 * r(s, a) + gamma * max Q(s'_a, .) (lob_vec_q on the result), exact advantage baselines, hindsight labels, a teacher that looks one
 * step ahead.  One launch instead of lob_snapshot_save + nine times (lob_vec_step, a copy, lob_snapshot_restore), and no snapshot
 * slot is taken.
 *   lob_vec_peek_out: where the results go, DEVICE pointers on the engine's GPU, written in stream order; a NULL member is skipped.
 * Every tensor is action-major: plane a = elements [a * n_books, (a + 1) * n_books).
 *   lob_vec_peek: for every action a whose bit is set in action_mask (LOB_PEEK_ALL: all nine), plane a holds bit for bit what
 * lob_vec_step would have written to obs / reward / terminal / stepped had every book been given action a at this point -- a book
 * that is over: stepped 0, reward +0.0, obs = the state of its last completed step, terminal as it stands; a step that runs out of
 * data (necessarily under all nine actions alike): stepped 0, reward +0.0, terminal 2, obs kept.  The planes of actions that are not
 * in the mask are not written.
 *   Nothing of the engine changes: no book, no PnL window, no state vector, no step header, no memo / verdict / hit-list word, no
 * counter of lob_get_counters, no step number, no step-log row and no random stream; the next lob_vec_step, lob_step or learner call
 * gives what it would have given without the call.  (The one exception is the engine's sticky error word: a condition on the event
 * data that the step with action a would have reported -- LOB_EDATA from lob_vec_status -- is reported by the look-ahead as well.)
 *   Enqueued on the engine's stream (lob_stream) as one launch, returns at once: no host read, no allocation, no copy and no
 * synchronisation.  Allowed after lob_snapshot_restore (it reads the environment only).  LOB_EINVAL, with a message naming the call:
 * a NULL engine or out, action_mask 0 or with a bit at or above LOB_N_ACTIONS.  LOB_ESTATE: before the first lob_reset, between
 * lob_td_step_begin and lob_td_step_end, and on a stream whose market track is a ring (longer than LOB_TRACK_RING events: the
 * snapshot calls are refused there too) unless lob_look_ring is on.  All four members NULL: LOB_OK, nothing is launched. */
#define LOB_PEEK_ALL 0x1FFu
typedef struct lob_vec_peek_out {   /* DEVICE pointers on the engine's GPU; any may be NULL = not wanted; action-major planes */
    float*   obs;                   /* [9][n_books][n_vars] */
    double*  reward;                /* [9][n_books] */
    uint8_t* terminal;              /* [9][n_books] */
    int32_t* stepped;               /* [9][n_books] */
} lob_vec_peek_out;
int lob_vec_peek(lob_engine* e, uint32_t action_mask, const lob_vec_peek_out* out);

/* ---- vector-env interface: multi-step look-ahead under action plans, on the device ---
 * The environment as a model several steps deep: the books rolled forward `horizon` steps under each of `n_plans` candidate plans PER
 * BOOK -- n-step targets, random-shooting or CEM model-predictive control, "which of these K quote schedules is best from here" -- in
 * one launch instead of lob_snapshot_save + n_plans times (horizon lob_vec_step, copies, lob_snapshot_restore), and no snapshot slot
 * is taken.
 *   dev_actions: DEVICE memory on the engine's GPU, int32 [n_plans][horizon][n_books]: the action of plan p at step h for book b.
 *   lob_vec_rollout_out: where the results go, DEVICE pointers on the engine's GPU, written in stream order; a NULL member is skipped.
 * Every tensor is plan-major.
 *   lob_vec_rollout: take plan p and imagine `horizon` consecutive lob_vec_step calls from the engine's present state, the h-th with
 * dev_actions[p][h][:].  Bit for bit, reward[p][h][b] is what the h-th call would write to reward[b]; obs[p][b] and terminal[p][b]
 * are what the last call would write; stepped[p][b] is the sum of the calls' stepped[b].  The rules of every step are
 * lob_vec_step's: a book steps only if its terminal is 0 at the entry of that step; a book that is over, or a step that runs out of
 * data, gives reward +0.0 and keeps the obs of the last completed step (if no step of the plan completed: the state the engine holds
 * now); an action outside [0, LOB_N_ACTIONS) means the book is not stepped at that step and the plan goes on with the next.  Such an
 * action is NOT counted in the word lob_vec_status reports: padding a plan with -1 is the way to make plans of unequal length.
 *   ret[p][b] is the discounted sum of the plan's rewards in exactly this order, every operation rounded on its own (no fused
 * multiply-add): acc = +0.0, d = 1.0; for h = 0 .. horizon - 1: acc = acc + d * r_h, d = d * gamma -- the discount follows h whether
 * or not the step completed.
 *   Nothing of the engine changes, as under lob_vec_peek: no book, no PnL window, no state vector, no step header, no memo / verdict /
 * hit-list word, no counter of lob_get_counters, no step number, no step-log row, no random stream, no snapshot slot; with the same
 * exception, the engine's sticky error word.
 *   Enqueued on the engine's stream (lob_stream) as one launch, returns at once: no host read, no copy and no synchronisation -- with
 * one exception, as for lob_snapshot_save's slot buffers: when the reward is LOB_REWARD_NORMED and 1 < lb_pnl < horizon, the engine
 * keeps the PnL windows' entries the plans themselves push in a workspace of 2 * lb_pnl * n_plans * (n_books rounded up to 64)
 * doubles.  The first call that needs it allocates it, a later call that needs a larger one replaces it (allocation and release
 * synchronise the device); every other call allocates nothing.  lob_destroy releases it.
 *   Allowed after lob_snapshot_restore and while the step log records.  Refusals carry a message naming the call, and a refused call
 * writes nothing.  LOB_EINVAL: a NULL engine, out or dev_actions; n_plans outside 1 .. LOB_MAX_ROLLOUT_PLANS; horizon outside
 * 1 .. LOB_MAX_ROLLOUT_STEPS; gamma NaN or outside [0, 1].  LOB_ESTATE: before the first lob_reset, between lob_td_step_begin and
 * lob_td_step_end, and on a stream whose market track is a ring (longer than LOB_TRACK_RING events) unless lob_look_ring is on.  LOB_ENOMEM: the workspace does
 * not fit.  All five members NULL: LOB_OK, nothing is launched. */
#define LOB_MAX_ROLLOUT_PLANS 64
#define LOB_MAX_ROLLOUT_STEPS 64
typedef struct lob_vec_rollout_out {   /* device pointers; NULL = not wanted, not written */
    float*   obs;       /* [P][B][V]  the observation behind the plan's last step             */
    double*  reward;    /* [P][H][B]  the reward of every step of the plan                    */
    uint8_t* terminal;  /* [P][B]     lob_get_terminal's value behind the last step           */
    int32_t* stepped;   /* [P][B]     how many of the H steps completed, 0 .. H               */
    double*  ret;       /* [P][B]     the discounted sum of the plan's rewards                */
} lob_vec_rollout_out;
int lob_vec_rollout(lob_engine* e, const int32_t* dev_actions /* [P][H][B] */, int n_plans, int horizon,
                    double gamma, const lob_vec_rollout_out* out);

/* ---- vector-env interface: branches, private copies of the books stepped in a loop ---
 * The two look-aheads above are open loop: every action must be known before the launch.  A BRANCH SET lets the imagined worlds persist
 * between launches: n_branches private copies of every book's agent-side environment state (the per-book scalars, the two PnL
 * windows, the observation of the last completed step), all reading the same market track, stepped one step at a time with actions
 * from device memory and rearranged on the device -- closed-loop returns under any policy (lob_vec_q on the branches' obs continues
 * a plan under the engine's own weights), beam search, particle resampling, tree expansion that keeps only what it selects.  One
 * set per engine; no snapshot slot is taken.
 *   lob_branch_out: where results go, DEVICE pointers on the engine's GPU, written in stream order; a NULL member is skipped.  Every
 * tensor is branch-major: plane n = elements [n * n_books, (n + 1) * n_books).
 *   lob_branch_fork (re)makes the set: every branch (n, b), n < n_branches, becomes a copy of book b's present environment state.
 * out, when given: the observation of the book's last completed step, lob_get_terminal's value, reward +0.0, stepped 0, in every
 * plane.  The first fork allocates the set (416 bytes per branch and book rounded up to 64 books, plus 16 * lb_pnl when the reward is
 * LOB_REWARD_NORMED), and so does a fork that needs a larger one than any before it: allocation and release synchronise the device.
 * Every other fork only enqueues one launch.
 *   lob_branch_step: imagine the engine's books were in branch n's state and lob_vec_step were called with dev_actions[n][:].  Bit
 * for bit, obs / reward / terminal / stepped at [n][b] are what that call would write, and the branch's state becomes what that call
 * would leave behind.  The rules of the step are lob_vec_rollout's: a branch steps only if its terminal is 0 at entry; a branch that
 * is over, or a step that runs out of data, gives reward +0.0, stepped 0 and keeps the obs of the last completed step (a step that
 * ran dry keeps its consumed events: terminal 2); an action outside [0, LOB_N_ACTIONS) leaves the branch as it is and is NOT counted
 * in the word lob_vec_status reports: -1 steps a subset.  h calls with a_0 .. a_{h-1} give, per step, the rewards of lob_vec_rollout
 * under that plan and, behind the last, its obs and terminal.
 *   lob_branch_select: branch (n, b) becomes a copy of branch (dev_parent[n][b], b) as it stood before the call; a parent outside
 * [0, n_branches) means "keep yourself"; many children of one parent are the point.  It goes through a second buffer of the set's
 * size, allocated by the first select (and by the first select after the set has grown): that one synchronises the device, every
 * other select only enqueues one launch.  out, when given: obs and terminal of the new arrangement; reward and stepped are not written.
 *   lob_branch_close releases both buffers and synchronises the device; lob_destroy does the same.
 *   Nothing of the engine changes, as under lob_vec_peek: no book, no PnL window, no state vector, no step header, no memo / verdict /
 * hit-list word, no counter, no step number, no step-log row, no random stream, no snapshot slot; with the same exception, the engine's
 * sticky error word.  The branches read only the track and the records, which do not change within an episode: they stay valid while
 * the real books step on and across lob_snapshot_save / lob_snapshot_restore.  lob_reset voids the set (the buffers stay): step and
 * select then return LOB_ESTATE until the next fork.
 *   All work is enqueued on the engine's stream (lob_stream) and nothing is read back.  Allowed after lob_snapshot_restore and while
 * the step log records.  Refusals carry a message naming the call, and a refused call writes nothing.  LOB_EINVAL: a NULL engine; NULL
 * dev_actions or dev_parent; NULL out for lob_branch_step; n_branches outside 1 .. LOB_MAX_BRANCHES.  LOB_ESTATE: before the first
 * lob_reset, between lob_td_step_begin and lob_td_step_end, on a stream whose market track is a ring unless lob_look_ring is on, and -- step and select -- with
 * no live set.  LOB_ENOMEM: a buffer does not fit (the message gives its bytes).  All members NULL: fork and select still act on the
 * set and step still steps; nothing is written to the caller. */
#define LOB_MAX_BRANCHES 64
typedef struct lob_branch_out {      /* device pointers on the engine's GPU; NULL = not wanted, not written */
    float*   obs;        /* [N][B][V] */
    double*  reward;     /* [N][B]    */
    uint8_t* terminal;   /* [N][B]    */
    int32_t* stepped;    /* [N][B]    */
} lob_branch_out;
int lob_branch_fork  (lob_engine* e, int n_branches, const lob_branch_out* out /* may be NULL */);
int lob_branch_step  (lob_engine* e, const int32_t* dev_actions /* [N][B] */, const lob_branch_out* out);
int lob_branch_select(lob_engine* e, const int32_t* dev_parent  /* [N][B] */, const lob_branch_out* out /* may be NULL */);
int lob_branch_close (lob_engine* e);

/* ---- branch sets: the order book and the event window of every branch ---
 * lob_branch_out carries what the engine's own tile-coded agent reads.  A network that reads the book's levels, its own orders and
 * inventory (lob_vec_book) and a window of the last K event records (lob_vec_history) gets the same two observations at every
 * branch's state here, so that it can choose the actions of a closed loop over a branch set.  The two out-structs of the real books
 * are reused; every tensor is branch-major as in lob_branch_out, N = the live set's n_branches, plane n = elements [n * n_books,
 * (n + 1) * n_books), no padding:
 *     lob_branch_book:    levels [N][B][4][depth], own [N][B][LOB_VEC_OWN_WORDS], time_ms [N][B]
 *     lob_branch_history: levels [N][B][K][4][depth], trades [N][B][K][2][max_trades], time_ms [N][B][K], n_valid [N][B], rec [N][B]
 *   ONE rule: element [n][b] is, bit for bit, what lob_vec_book / lob_vec_history(K) would write at [b] had the engine's books been in
 * branch n's state -- for every branch, whatever its terminal word; behind lob_branch_fork, behind any lob_branch_step (an action
 * out of range, a "stay", included) and behind lob_branch_select, in the new arrangement.  Every rule of the two calls carries over:
 * `depth` levels, zeros where there is no snapshot, own in LOB_OWN_* order, time_ms copied as int64; history slots with a negative
 * record index all zero, n_valid = min(K, rec + 1), rec never past the last record of THAT BOOK's stream (a replayed stream's phase,
 * the day the book is playing) -- branches of one book differ in rec, not in the stream; every element of every non-NULL tensor is
 * written on every call; any 1 <= K <= LOB_MAX_HISTORY is valid.
 *   Each call is one launch enqueued on the engine's stream (lob_stream): no host read, no allocation, no copy and no
 * synchronisation.  Nothing of the engine and nothing of the set changes.  Allowed after lob_snapshot_restore, while the step log
 * records and while the real books step on.  LOB_EINVAL: a NULL engine, a NULL out, K outside [1, LOB_MAX_HISTORY]; a struct whose
 * members are all NULL is LOB_OK and launches nothing.  LOB_ESTATE, with a message naming the call: before the first lob_reset,
 * between lob_td_step_begin and lob_td_step_end, on a stream whose market track is a ring unless lob_look_ring is on, and with no
 * live set -- never forked, voided by lob_reset, closed.  A refused call writes nothing.
 *   Not offered: the book and the window at the leaves of lob_vec_peek / lob_vec_rollout -- those launches keep no end state; a
 * leaf's book is a branch set stepped under the plan. */
int lob_branch_book   (lob_engine* e, const lob_vec_book_out* out);
int lob_branch_history(lob_engine* e, int32_t K, const lob_vec_hist_out* out);

/* ---- look-aheads on a ring-mode stream: the switch and the window ---
 * A stream of more than LOB_TRACK_RING events keeps only the latest entries of its market track, as a ring that the step calls
 * refill every LOB_TRACK_REFILL steps.  lob_vec_peek, lob_vec_rollout, lob_branch_* and lob_branch_book / lob_branch_history are
 * refused there (LOB_ESTATE) UNLESS the caller has switched them on, per engine, because on a ring they have two outcomes that a
 * resident track cannot produce and a caller must know of.
 *   lob_look_ring(e, on): a host flag, off after lob_create, kept across lob_reset; LOB_ESTATE between lob_td_step_begin and
 * lob_td_step_end, LOB_EINVAL for a NULL engine.  While it is on, the calls named above run on a ring track.  The snapshot calls stay
 * refused there: they need entries BEHIND the cursor, which are gone.  On a resident track the flag changes nothing at all.
 *   THE WINDOW.  Per book, the pre-pass has written n_track entries so far (all of the stream once `complete`), and the ring holds
 * the latest of them.  With hi = n_track and lo = max(0, n_track - ring length + LOB_TRACK_WINDOW_MARGIN) the one rule is:
 *     a private state at cursor k can be served while lo <= k; a private step is served when it never needs an entry >= hi while
 *     complete == 0.
 * lo carries the margin of LOB_TRACK_WINDOW_MARGIN (4) entries that every refill grants the real cursor, which therefore is always
 * inside the window.  On a resident track lo = 0 and hi = n_track.
 *   lob_track_window(e, lo, hi, complete): the three words of every book into HOST arrays [n_books], as they stand behind everything
 * enqueued so far.  It waits for the stream (the second call of this interface that does, after lob_vec_status): for diagnostics and
 * tests.  LOB_EINVAL for a NULL argument, LOB_ESTATE before the first lob_reset.
 *   THE REFILL.  In front of its launch a look-ahead d steps deep makes the refill that would fall due within its depth (one launch
 * on the engine's stream, decided on the host without a read; the schedule of the step calls starts again from there): d = 1 for
 * lob_vec_peek and lob_branch_fork, d = horizon for lob_vec_rollout, d = 1 + lead for lob_branch_step, lead = the lob_branch_step
 * calls since the set's last fork less the real steps since then, floored at 0.  A refill changes no bit that any call reports of the
 * real books.  It can push a branch that LAGS behind the real books out of the window.
 *   THE TWO OUTCOMES, per cell, in the `terminal` planes of the look-ahead calls only (never in lob_vec_step / lob_get_terminal):
 *     LOB_TERMINAL_AHEAD   the step would have read an entry >= hi while complete == 0.  It is dropped: stepped 0, reward +0.0.
 *                          lob_vec_peek: obs = the book's present state.  lob_vec_rollout: the plan ends at that step for that book --
 *                          that step and all later ones reward +0.0, stepped / obs / ret as behind the last completed step.
 *                          lob_branch_step: the branch's stored state is NOT written; the same call succeeds once the real books
 *                          have moved the window on.
 *     LOB_TERMINAL_BEHIND  lob_branch_step only: a live branch (its own terminal 0) whose cursor is < lo.  Nothing is attempted,
 *                          whatever its action: state not written, stepped 0, reward +0.0, obs unchanged.  lob_branch_select copies
 *                          whatever a branch holds; lob_branch_fork makes every branch live again; lob_branch_book /
 *                          lob_branch_history read the records, which are resident, and report the state the branch holds.
 * Neither outcome touches the engine's sticky error word.  lob_vec_status reads and clears, with its own word, the number of AHEAD
 * and of BEHIND cells since the last lob_vec_status / lob_reset; lob_look_counts returns the two numbers that call read (host words,
 * nothing is waited for; either pointer may be NULL). */
#define LOB_TERMINAL_AHEAD  3
#define LOB_TERMINAL_BEHIND 4
#define LOB_TRACK_WINDOW_MARGIN 4
int lob_look_ring   (lob_engine* e, int on);
int lob_track_window(lob_engine* e, int32_t* lo, int32_t* hi, int32_t* complete);
int lob_look_counts (lob_engine* e, int64_t* n_ahead, int64_t* n_behind);

/* ---- episode statistics of the whole batch ---------------------------------
 * What the reference logs about ONE environment after an episode -- the `training_log` row of Runner::RunEpisode
 * (src/experiment/serial.cpp:81-88: getEpisodeReward, getEpisodePnL, total_ticks), Base::writeStats and getTotalTransactions
 * (src/environment/base.cpp:458-473), the test loop's console line `Rwd, Rho, Pnl, nTr, Ppt` per day
 * (src/main.cpp:215-239) -- reduced over the books of the engine ON THE DEVICE: count, sum, sum of squares, extremes and
 * the books that hold them, for the whole engine and, with a day library, for the books playing each day.  One record of
 * 408 bytes per group comes back instead of one lob_book_dump per book.
 *   Every per-book value is exactly what lob_get_books reports for that book at that moment (episode_reward, episode_pnl,
 * episode_bandh, total_ticks, ask_transactions + bid_transactions + market_buys + market_sells, market_buys + market_sells,
 * ticks_with_position; n_live / n_terminal / n_out_of_data count the dump's `terminal` 0 / 1 / 2).  LOB_STATF_RHO is the
 * IEEE f64 quotient episode_reward / total_ticks of each book (Base::getMeanEpisodeReward); a book with total_ticks == 0
 * (the reference would print 0/0) is left out of RHO and of n_rho.  A NaN value goes into sum and sumsq as IEEE addition
 * takes it and is passed over by min / max (every comparison with it is false).
 *   lob_episode_stats: out[0] is the whole engine (group -1).  by_day != 0 on a day library: out[1 + d] is library day d
 * for EVERY day of the library, *n_out = 1 + n_days; a day nobody plays comes back as the identity record (n_books 0,
 * sums 0, min +inf / INT64_MAX, max -inf / INT64_MIN, argmin = argmax = -1).  argmin / argmax are GLOBAL book ids
 * (book_id_offset + b); ties go to the lowest id.  Two calls on the same state, and two engines that ran the same run,
 * return bit-identical records (the order of the f64 additions is fixed: DESIGN.md 7b).  Valid whenever lob_get_books is
 * meaningful: after the first lob_reset, mid-episode (n_live > 0), after lob_clear_inventory.  It is enqueued on the
 * engine's stream, waits once for its own result and changes no engine state.  LOB_ESTATE: before the first lob_reset,
 * between lob_td_step_begin and lob_td_step_end, by_day without an episode on a day library; LOB_EINVAL: a NULL argument,
 * or cap < *n_out (with *n_out set, so that the caller can size its buffer).
 *   lob_episode_stats_merge (host only): adds `from` into `into` -- counts, sums and sums of squares add, min / max keep
 * the lower id on a tie, `group` is kept where both agree and becomes -1 otherwise.  The identity record is its neutral
 * element; it is how a multi-GPU caller puts the ranks' records together. */
#define LOB_STATF_REWARD 0   /* episode_reward                       (Base::getEpisodeReward)     */
#define LOB_STATF_RHO    1   /* episode_reward / total_ticks         (Base::getMeanEpisodeReward) */
#define LOB_STATF_PNL    2   /* episode_pnl                                                       */
#define LOB_STATF_BANDH  3   /* episode_bandh                                                     */
#define LOB_STATI_STEPS          0   /* total_ticks                                               */
#define LOB_STATI_TRANSACTIONS   1   /* Base::getTotalTransactions (base.cpp:469-473)             */
#define LOB_STATI_MARKET_ORDERS  2   /* market_buys + market_sells                                */
#define LOB_STATI_TICKS_POSITION 3   /* ticks_with_position                                       */
typedef struct lob_stat_f64 { double sum, sumsq, min, max; int64_t argmin, argmax; } lob_stat_f64;
typedef struct lob_stat_i64 { int64_t sum, sumsq, min, max; int64_t argmin, argmax; } lob_stat_i64;
typedef struct lob_episode_record {
    int32_t group;                  /* -1: every book of the engine; d >= 0: the books playing library day d */
    int32_t n_books;                /* books in the group */
    int32_t n_live, n_terminal, n_out_of_data;   /* by lob_get_terminal's 0 / 1 / 2; they add up to n_books */
    int32_t n_rho;                  /* books with total_ticks > 0: the only ones LOB_STATF_RHO counts */
    lob_stat_f64 f[4];              /* LOB_STATF_* */
    lob_stat_i64 i[4];              /* LOB_STATI_* */
} lob_episode_record;   /* (not lob_episode_stats: in C a typedef and a function cannot share a name) */
int lob_episode_stats(lob_engine* e, int32_t by_day, lob_episode_record* out, int32_t cap, int32_t* n_out);
void lob_episode_stats_merge(lob_episode_record* into, const lob_episode_record* from);

/* ---- learner interface (rl::Agent, include/rl/agent.h:48-77) ------------- */

/* `n_steps` x Learner::_step (src/experiment/serial.cpp:53-70) for every live
 * book: action(s) -> performAction -> newState -> HandleTransition. */
int lob_td_step(lob_engine* e, int32_t n_steps);
/* One such step in two halves: lob_td_step_begin = swap, isTerminal, action, performAction, newState of every book;
 * lob_td_step_end = HandleTransition (traces, TD errors, update).  Between them no cached action-selection data is live, so
 * that is where a multi-GPU weight exchange goes (include/lob_comm.h lob_theta_allreduce): Q(from_state, .) of the step is
 * what it was when the action was chosen, Q(to_state, .) sees the exchanged weights.  Nothing else may come in between:
 * lob_td_step, lob_td_step_begin, lob_eval_step, lob_step, lob_clear_inventory, lob_handle_terminal and lob_theta_set return
 * LOB_ESTATE there; lob_reset abandons the half-done step with its episode.  begin + end without an exchange =
 * lob_td_step(e, 1), bit for bit. */
int lob_td_step_begin(lob_engine* e);
int lob_td_step_end(lob_engine* e);
/* 1 if this engine can split a step (always, except an experiments build run with two book groups, LOB_GROUPS=2): the
 * caller that cannot split runs the whole step and exchanges after it -- asked for explicitly instead of being inferred
 * from a LOB_ESTATE of lob_td_step_begin, which has other causes (no reset, a half step left open). */
int lob_td_split_supported(lob_engine* e);
/* Backtester::_step (serial.cpp:124-137): greedy action, no learning.  The reference's Backtester is a runner of its own; here a
 * greedy step may stand among learner steps, and like lob_step and lob_vec_step it leaves the state BEHIND the step in the learner's
 * `state` object: the lob_td_step that follows chooses its action in the books' present state. */
int lob_eval_step(lob_engine* e, int32_t n_steps);
/* Agent::HandleTerminal (src/rl/agent.cpp:103-109): traces.decay(0). The
 * alpha / epsilon schedules are evaluated by the host adaptor. */
int lob_handle_terminal(lob_engine* e);

/* Replaces the `model_log` logger of Agent::HandleTransition (src/rl/agent.cpp:53-59,93-100: `_agg_delta += abs(delta)`, and
 * every 1000 updates one row `_agg_delta / 1000`).  After lob_model_log_enable(e, 1) every learner step adds the stepped books'
 * |delta| to a running aggregate on the device; once it holds 1000 updates or more, a row aggregate / count is written and
 * both start again.  One book: the reference's rows exactly (the count reaches 1000 one update at a time).  A batch: a row
 * per step once the batch has 1000 books, the mean |delta| of the step.  lob_model_log_read hands over the rows written since
 * the last read (at most `cap`; `n_lost`, if not NULL: rows that did not fit the device ring of 8192 or `cap`). */
int lob_model_log_enable(lob_engine* e, int32_t on);
int lob_model_log_read(lob_engine* e, double* rows, int32_t cap, int32_t* n_rows, int64_t* n_lost);

/* ---- step log: the profit-log row of every step, recorded on the device -----
 * Replaces Intraday::LogProfit (src/environment/intraday.cpp:438-451; schema src/experiment/serial.cpp:101-107), which the
 * reference's Backtester calls after every step (src/environment/base.cpp:333) -- for any chosen set of books, inside the
 * stream of steps: no dump, no copy and no synchronisation per step, and any number of steps per call.
 *   Every field of a row is, bit for bit, what lob_get_books would report for that book had it been called right after that
 * step.  The row carries the running totals: the step's own bandh / reward is the difference of two consecutive rows (row 0:
 * from 0.0), taken by the caller in f64 -- the engine keeps the totals and nothing else.  sizeof == 96, a multiple of 16: the
 * rows of the device log are 16-byte aligned (on the host the type has its natural alignment, 8).
 *   What gets a row: every performAction that ran to its end (base.cpp:333), by lob_td_step, lob_eval_step, lob_td_step_begin +
 * lob_td_step_end (written by the end half) and lob_step.  A step that runs out of data writes NONE (it returns at
 * base.cpp:289-290 although it has counted its tick, base.cpp:278): such a book (terminal == 2) ends with total_ticks = its
 * rows + 1, every other book with total_ticks = its rows, stored plus lost.  A book that is already over gets none, and
 * lob_clear_inventory writes none.  The k-th logged step of a book (k from 0) is its row k; rows with k >= cap_steps are
 * not stored but counted in n_lost -- the log never overwrites.
 *   lob_step_log_enable: host_books = LOCAL book indices (as lob_get_books takes them), strictly ascending, within
 * [0, n_books); NULL with n_sel == n_books selects every book.  n_sel == 0 switches the log off and frees its memory.  The log
 * is sized n_sel x cap_steps x 96 B at this call (all 65 536 books of the headline batch: 6.3 MB per step, 8.8 GB for a
 * 1 400-step episode): LOB_ENOMEM if that does not fit, LOB_EINVAL for a bad list or cap_steps < 1, LOB_ESTATE between
 * lob_td_step_begin and lob_td_step_end.  Recording starts with the NEXT lob_reset and every lob_reset empties the log: it
 * holds the current episode, never half of one.  While the log is on, a step issues one more kernel launch; off, none.
 *   lob_step_log_counts: int32[n_sel] stored rows and (n_lost may be NULL) lost rows.  lob_step_log_read: book-major,
 * host_out[(j - first_sel) * n_rows + (k - first_row)] = row k of selected book j; slots beyond a book's stored count are 96
 * zero bytes (step == 0 marks "no row").  Both wait once for their own result and change no engine state.  LOB_ESTATE when
 * the log is off or inside a half step, LOB_EINVAL for NULL or a range outside the selection or cap_steps. */
typedef struct lob_step_row {
    int64_t time_ms;                   /* dump.time_ms                     (market->time())            */
    int64_t position;                  /* dump.position                    (risk_manager_.exposure())  */
    double  midprice;                  /* (dump.ask_px[0] + dump.bid_px[0]) / 2.0, in f64              */
    double  spread;                    /* dump.ask_px[0] - dump.bid_px[0], in f64                      */
    double  ask_quote, bid_quote;      /* dump.ask_quote / bid_quote                                   */
    double  pnl_step;                  /* dump.pnl_step                                                */
    double  episode_pnl;               /* dump.episode_pnl     running totals: the step's own          */
    double  episode_bandh;             /* dump.episode_bandh   bandh / reward is the difference of two */
    double  episode_reward;            /* dump.episode_reward  consecutive rows (row 0: from 0.0)      */
    int32_t step;                      /* dump.total_ticks after the step: >= 1 in every written row   */
    int32_t action;                    /* dump.last_action                                             */
    int32_t ask_level, bid_level;      /* dump.ask_level / bid_level                                   */
} lob_step_row;
int lob_step_log_enable(lob_engine* e, const int32_t* host_books, int32_t n_sel, int32_t cap_steps);
int lob_step_log_counts(lob_engine* e, int32_t* n_rows, int32_t* n_lost);
int lob_step_log_read(lob_engine* e, int32_t first_sel, int32_t n_sel, int32_t first_row, int32_t n_rows,
                      lob_step_row* host_out);

int lob_set_alpha(lob_engine* e, double alpha);
int lob_set_epsilon(lob_engine* e, double epsilon);
int lob_set_tau(lob_engine* e, double tau);

/* State::newState(vector<float>&) + getFeatures (src/rl/state.cpp:45-70):
 * n states of n_vars floats -> int32[n][9][96] tile indices. */
int lob_features(lob_engine* e, const float* host_vars, int32_t n, int32_t* host_out);
/* Agent::getQ for all actions (src/rl/agent.cpp:117-135): double[n][9]. */
int lob_q_values(lob_engine* e, const float* host_vars, int32_t n, double* host_out);

/* theta access: Agent::write_theta (src/rl/agent.cpp:176-181) + the missing
 * load path.  `which` = book for LOB_THETA_PRIVATE, 0 for shared. */
int lob_theta_get(lob_engine* e, int32_t which, double* host_out, int64_t count);
int lob_theta_set(lob_engine* e, int32_t which, const double* host_in, int64_t count);
/* Last actions / rewards / TD errors of the most recent lob_td_step. */
int lob_get_last_actions(lob_engine* e, int32_t* host_out);
int lob_get_last_td(lob_engine* e, double* host_out);
int lob_get_last_rewards(lob_engine* e, double* host_out);
/* 1 where the most recent step performed an env-step + TD update */
int lob_get_stepped(lob_engine* e, int32_t* host_out);
/* draws consumed so far from each book's policy RNG stream */
int lob_get_rng_counters(lob_engine* e, uint64_t* host_out);
/* state_vars of the rl::State produced by the last step: float[n_books][n_vars] */
int lob_get_learner_state(lob_engine* e, float* host_out);
/* Live traces of one book: indices and eligibilities (rl::Traces). */
int lob_get_traces(lob_engine* e, int32_t book, int32_t* idx, float* elig, int32_t cap, int32_t* n);

/* Counters: [0] env-steps performed, [1] market events consumed,
 * [2] live books, [3] td updates applied. */
int lob_get_counters(lob_engine* e, int64_t out[4]);
/* Which kernels served the books (diagnostics of the fast paths, cumulative since lob_create unless noted):
 * [0] books the SARSA lane trace kernel (trace_sarsa_kernel) handed back to the wave-per-book kernel,
 * [1] books whose action came from the hit-list replay (the light action selection), [2] memo slots registered this episode,
 * [3] weight indices found ambiguous this episode (tile registry), [4] 1 if the registry overflowed this episode,
 * [5] memo slots in use in the latest step, [6] books whose action the fused env kernel had to evaluate in full (no usable hit
 * list: act_book in-kernel), [7] books the lane learn kernels handed back to the wave-per-book evaluation (trace_rest_kernel /
 * learn_q_rest_kernel). */
int lob_get_path_stats(lob_engine* e, int64_t out[8]);

/* ---- multi-GPU weight exchange ---------------------------
 * The engine library never calls a collective itself: it exposes the dense
 * delta buffer, and include/lob_comm.h (liblob_comm.so, RCCL) all-reduces it
 * in place over xGMI on the engine's stream (lob_theta_allreduce) -- the batched
 * stand-in for the reference's shared Agent* of src/main.cpp:196-206.
 *   lob_delta_init  : theta_sync = theta (call once, after create; lob_theta_set keeps it in step)
 *   lob_delta_begin : dev_delta[i] = theta[i] - theta_sync[i]   (then waits for the stream;
 *                     lob_delta_begin_async only enqueues it)
 *   (caller: all-reduce SUM dev_delta over ranks)
 *   lob_delta_apply : theta = theta_sync + dev_delta ; theta_sync = theta
 * `count` = memory_size, or 2 x memory_size for LOB_ALGO_DOUBLE_Q (theta then theta_b); the average-reward agents
 * append two slots [rho - rho_sync, 1.0] (the sum's second slot = the number of ranks: rho moves by the mean change).
 */
int lob_delta_init(lob_engine* e);
int lob_delta_begin(lob_engine* e, double** dev_delta, int64_t* count);
int lob_delta_begin_async(lob_engine* e, double** dev_delta, int64_t* count);
int lob_delta_apply(lob_engine* e);
/* The same exchange without the dense vector (shared theta on the fast path, i.e. SARSA / Q(lambda); dense otherwise).  The
 * engine's exact written-weights map (one bit per weight) enumerates every weight a step of this rank has touched:
 *   lob_delta_sparse_maps  : the rank's map and a [world][words] buffer to ALL-GATHER the ranks' maps into (uint32 words)
 *   lob_delta_sparse_pack  : union of the gathered maps -> one compact vector layout common to all ranks;
 *                            dev_buf[p] = theta[f] - theta_sync[f] for the p-th weight f of the union.  Returns the element
 *                            count (identical on all ranks) after ONE stream synchronisation: the collective needs it.
 *   (caller: all-reduce SUM dev_buf[0 .. count) over ranks)
 *   lob_delta_sparse_apply : theta[f] = theta_sync[f] + dev_buf[p] ; theta_sync[f] = theta[f]
 * A few hundred thousand doubles instead of memory_size = 20 M of them. */
int lob_delta_sparse_supported(lob_engine* e);
int lob_delta_sparse_maps(lob_engine* e, int32_t world, uint32_t** dev_own, uint32_t** dev_gather, int64_t* words);
int lob_delta_sparse_pack(lob_engine* e, int32_t world, double** dev_buf, int64_t* count);
int lob_delta_sparse_apply(lob_engine* e);

/* Synchronise the engine's stream / expose it (hipStream_t as void*). */
int lob_sync(lob_engine* e);
void* lob_stream(lob_engine* e);
/* Average duration (ms) of the named kernel over the TIMED launches since the last
 * reset of the timers, measured with HIP events on the engine stream.
 * lob_kernel_timing(e, n): 0 = off, 1 = every launch, n > 1 = the launches of every n-th
 * step (two event records per launch cost ~9 % of a step when every launch is timed). */
int lob_kernel_time_ms(lob_engine* e, const char* kernel, double* avg_ms, int64_t* launches);
int lob_kernel_timing(lob_engine* e, int32_t enable);

#ifdef __cplusplus
}
#endif
#endif /* LOB_ENGINE_H */
