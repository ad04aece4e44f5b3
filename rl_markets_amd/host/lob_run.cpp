// Thin driver with the reference's factory choices (src/main.cpp:82-245) for the
// hot path: read a YAML config, build the batched environment + learner, train
// n episodes on synthetic streams, evaluate greedily, print the per-episode
// rows of the reference's training_log (serial.cpp:81-88) for book 0.
//
//   lob_run -c config/engine.yaml [-n books] [-e episodes (default: training.n_episodes)] [-a sarsa|q_learn|double_q_learn|r_learn|online_r_learn|double_r_learn] [--events N] [--depth D]
//           [--theta out.bin] [--profit-log profit_log.csv [--profit-log-books first:count]]   (the greedy backtest's profit log of book 0;
//            with --profit-log-books one file profit_log.csv.<book> per book of the range; recorded on the device, lob_step_log_*)
//           [--batch-log FILE]   (or logging.batch_log: after every training episode and every greedy test round one CSV row for the
//            WHOLE batch -- mean / std / min / max over the books of what the training_log row shows of book 0 -- and, with a
//            directory of days, one more row per day that had books; reduced on the device, lob_episode_stats.  --gpus N: every
//            rank writes FILE.rank<r>, its own shard)
//           [--gpus N [--sync-every K]]   one process per GPU (forked here), -n books EACH, book ids rank * n ..,
//            delta-theta all-reduced over RCCL/xGMI every K steps (include/lob_comm.h): the stand-in for the
//            reference's N training threads on one shared Agent (src/main.cpp:196-206)
//           [--md depth.csv --tas trades.csv | --lobster orderbook.csv message.csv LEVELS]   (a recorded day, replayed
//            by every book from evenly spread starting records; default: synthetic streams)
//           [--md-dir D --tas-dir D]   (or data.md_dir / data.tas_dir: the reference's directory of recorded days, src/main.cpp:89-239 --
//            get_file_sample, the train / test split, a training day drawn per book before every episode, then one greedy
//            evaluation over the held-out days with a row per day)
#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <random>

#include "lob_host.hpp"

static int run(int argc, char** argv, int rank, int world, const std::string& rdzv);

int main(int argc, char** argv) {
    int gpus = 1;
    for (int i = 1; i + 1 < argc; i++)
        if (!strcmp(argv[i], "--gpus")) gpus = atoi(argv[i + 1]);
    // rendezvous token of the RCCL communicator: a file in a private (0700) directory of this run
    char rdir[] = "/tmp/lob_run_XXXXXX";
    if (!mkdtemp(rdir)) { perror("mkdtemp"); return 2; }
    char rdzv[128];
    snprintf(rdzv, sizeof rdzv, "%s/rdzv", rdir);
    // LOB_FORCE_DIST=1: the whole exchange path with a one-rank communicator (a 1-GPU box can run it)
    const char* fd = getenv("LOB_FORCE_DIST");
    if (gpus <= 1) {
        const int rc1 = run(argc, argv, 0, 1, (fd && fd[0] == '1') ? rdzv : "");
        unlink(rdzv);
        rmdir(rdir);
        return rc1;
    }
    // one process per GPU, forked before anything touches the HIP runtime
    std::vector<pid_t> kids;
    for (int r = 0; r < gpus; r++) {
        pid_t pid = fork();
        if (pid < 0) { perror("fork"); return 2; }
        if (pid == 0) _exit(run(argc, argv, r, gpus, rdzv));
        kids.push_back(pid);
    }
    // wait for whichever rank ends first: when one fails (no device, no data, an exception) the others would sit in
    // ncclCommInitRank or the next all-reduce for ever -- stop exactly the processes forked above
    int rc = 0;
    size_t left = kids.size();
    while (left > 0) {
        int st = 0;
        const pid_t k = waitpid(-1, &st, 0);
        if (k < 0) break;
        bool ours = false;
        for (pid_t& q : kids) if (q == k) { q = -1; ours = true; }
        if (!ours) continue;
        left--;
        const int code = WIFEXITED(st) ? WEXITSTATUS(st) : 2;
        if (code && !rc) {
            rc = code;
            fprintf(stderr, "[lob_run] a rank exited with %d: stopping the other ranks\n", code);
            for (pid_t q : kids) if (q > 0) kill(q, SIGTERM);
        }
    }
    unlink(rdzv);
    rmdir(rdir);
    return rc;
}

// The reference's directory of recorded days (src/main.cpp:89-126): the (symbol, md, tas) pairs of get_file_sample, split into
// a training and a test set, converted and uploaded once as the engine's day library -- the training days first, then the
// held-out ones (none of their own when evaluation.use_train_sample replays the training days).
struct DaySplit {
    std::vector<std::array<std::string, 3>> files;   // in library order
    int n_train = 0, test_first = 0, n_test = 0;
    std::vector<uint32_t> records;                  // the converted days back to back, day i = records first[i] .. first[i + 1] - 1
    std::vector<int64_t> first{0};
};
static DaySplit load_day_library(const lob::Config& c, const lob_params& p, const std::string& md_dir, const std::string& tas_dir,
                                 lob::BatchedIntraday& env) {
    if (md_dir.empty() || tas_dir.empty()) throw std::runtime_error("data.md_dir and data.tas_dir (--md-dir, --tas-dir) go together");
    if (p.depth != 5) throw std::invalid_argument("the reference's CSV days have 5 levels (--depth 5)");
    const std::vector<std::string> symbols = c.has("data.symbols") ? c.list("data.symbols") : std::vector<std::string>{"HSBA.L"};
    // one venue per engine: the tick table is a parameter of the whole batch
    lob_market m0, m;
    for (size_t i = 0; i < symbols.size(); i++) {
        lob::check(lob_market_preset(symbols[i].c_str(), i ? &m : &m0), "Market::make_market");
        if (i && memcmp(&m, &m0, sizeof m) != 0)
            throw std::invalid_argument("symbols " + symbols[0] + " and " + symbols[i] + " trade on different venues: one venue per engine");
    }
    auto files = lob::get_file_sample(md_dir, tas_dir, symbols);
    const unsigned seed = (unsigned)p.seed;
    const bool eval_from_train = c.boolean("evaluation.use_train_sample", false);
    long n_eval = c.integer("evaluation.n_samples", -1);
    long n_train_samples = c.integer("training.n_samples", -1);
    std::vector<std::array<std::string, 3>> train, test;
    if (eval_from_train) {
        std::shuffle(files.begin(), files.end(), std::default_random_engine(seed));
        train = files;
    } else {
        if (n_eval == -1) n_eval = (long)files.size();
        if (n_eval < 0 || n_eval > (long)files.size()) throw std::runtime_error("evaluation.n_samples exceeds the days found");
        const long pivot = (long)files.size() - n_eval;
        train.assign(files.begin(), files.begin() + pivot);
        test.assign(files.begin() + pivot, files.end());
    }
    if (n_train_samples < 0) n_train_samples = (long)train.size();
    else if ((size_t)n_train_samples > train.size()) throw std::runtime_error("Insufficient training samples.");
    train.erase(train.begin(), train.begin() + (train.size() - n_train_samples));
    if (train.empty()) throw std::runtime_error("no training days in " + md_dir);
    DaySplit d;
    d.files = train;
    d.n_train = (int)train.size();
    if (eval_from_train) {
        d.test_first = 0;
        d.n_test = n_eval < 0 ? 0 : (int)std::min<long>(n_eval, d.n_train);
    } else {
        d.test_first = d.n_train;
        d.n_test = (int)test.size();
        d.files.insert(d.files.end(), test.begin(), test.end());
    }
    const size_t W = (size_t)lob_record_words(p.depth, p.max_trades);
    for (const auto& f : d.files) {
        uint32_t* rec = nullptr;
        int32_t n = 0;
        lob::check(lob_convert_csv(f[1].c_str(), f[2].c_str(), p.max_trades, &rec, &n), "LoadData");
        d.records.insert(d.records.end(), rec, rec + (size_t)n * W);
        lob_free(rec);
        d.first.push_back(d.first.back() + n);
    }
    env.LoadDays(d.records.data(), d.first);
    fprintf(stderr, "[-] %zu days: training on %d, testing on %d\n", d.files.size(), d.n_train, d.n_test);
    return d;
}

// --batch-log: the episode statistics of the whole batch (lob_episode_stats), one row per group that has books.  `episode`: the
// training episode's number, or "test<round>" for a greedy round over the held-out days; `epsilon`: the training row's column (the
// policy's descr() after HandleTerminal).  std is the population figure from
// sum and sum of squares, clamped at 0; rho's figures are over the books that made a step (n_rho); ppt = sum of pnl / sum of
// transactions of the group (src/main.cpp:236 for one book).
struct BatchLog {
    FILE* f = nullptr;
    ~BatchLog() { if (f) fclose(f); }
    void open(const std::string& path) {
        f = fopen(path.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + path);
        fprintf(f, "episode,group,day_file,n_books,n_terminal,n_out_of_data,epsilon,reward_mean,reward_std,reward_min,reward_max,"
                   "rho_mean,rho_std,rho_min,rho_max,pnl_mean,pnl_std,pnl_min,pnl_max,steps_mean,steps_min,steps_max,"
                   "transactions_mean,transactions_min,transactions_max,ppt\n");
    }
    void write(const std::string& episode, lob::BatchedIntraday& env, const std::vector<std::array<std::string, 3>>* files, double epsilon) {
        if (!f) return;
        for (const lob_episode_record& r : env.EpisodeStats(files != nullptr)) {
            if (r.group >= 0 && r.n_books == 0) continue;
            fprintf(f, "%s,%d,%s,%d,%d,%d,%.6g", episode.c_str(), r.group, r.group >= 0 ? (*files)[r.group][1].c_str() : "", r.n_books, r.n_terminal,
                    r.n_out_of_data, epsilon);
            const int fq[3] = {LOB_STATF_REWARD, LOB_STATF_RHO, LOB_STATF_PNL};
            for (int q : fq) {
                const lob_stat_f64& s = r.f[q];
                const double n = q == LOB_STATF_RHO ? r.n_rho : r.n_books, mean = s.sum / n, var = s.sumsq / n - mean * mean;
                fprintf(f, ",%.10g,%.10g,%.10g,%.10g", mean, var > 0 ? std::sqrt(var) : 0.0, s.min, s.max);
            }
            const int iq[2] = {LOB_STATI_STEPS, LOB_STATI_TRANSACTIONS};
            for (int q : iq) fprintf(f, ",%.10g,%lld,%lld", (double)r.i[q].sum / r.n_books, (long long)r.i[q].min, (long long)r.i[q].max);
            fprintf(f, ",%.10g\n", r.f[LOB_STATF_PNL].sum / (double)r.i[LOB_STATI_TRANSACTIONS].sum);
        }
        fflush(f);
    }
};

// The final testing phase (src/main.cpp:211-239): GoGreedy(), then every test day in a FRESH environment (main.cpp:214) with the
// trained weights -- here one lock-step Backtester episode per n_books test days, book i of a round playing test day i
// (LOB_DAYS_IN_ORDER) -- and the reference's five figures per day.  Private theta: every test book gets book 0's weights.
static void evaluate_days(const lob::Config& c, const lob_params& p, const DaySplit& d, lob::BatchedIntraday& trained, BatchLog& batch_log) {
    const int B = std::min(d.n_test, trained.n_books());
    lob_params q = p;
    q.book_id_offset = 0;
    lob::BatchedIntraday env(q, B, 0);
    env.LoadDays(d.records.data(), d.first);
    lob::Agent agent(env, c);
    {   // the trained agent's weights (theta, then theta_b of the double agents)
        const bool priv = p.theta_mode == LOB_THETA_PRIVATE, dq = p.algo == LOB_ALGO_DOUBLE_Q;
        const int nt_src = priv ? trained.n_books() : 1, nt = priv ? B : 1;
        std::vector<double> th((size_t)p.memory_size);
        for (int vec = 0; vec < (dq ? 2 : 1); vec++) {
            lob::check(lob_theta_get(trained.handle(), vec * nt_src, th.data(), (int64_t)th.size()), "GoGreedy");
            for (int t = 0; t < nt; t++) lob::check(lob_theta_set(env.handle(), vec * nt + t, th.data(), (int64_t)th.size()), "GoGreedy");
        }
    }
    agent.GoGreedy();
    printf("test,episode,symbol,file,reward,rho,pnl,n_tr,ppt\n");
    for (int r0 = 0; r0 < d.n_test; r0 += B) {
        const int n = std::min(B, d.n_test - r0);
        env.SelectDays(LOB_DAYS_IN_ORDER, d.test_first + r0, n);
        lob::Backtester bt(env);
        if (!bt.RunEpisode(&agent)) { fprintf(stderr, "[!] no data in test days %d..%d\n", r0 + 1, r0 + n); continue; }
        batch_log.write("test" + std::to_string(r0 / B + 1), env, &d.files, agent.epsilon_);
        for (int i = 0; i < n; i++) {
            const auto& f = d.files[d.test_first + r0 + i];
            const double pnl = env.getEpisodePnL(i);
            const int ntr = env.getTotalTransactions(i);
            printf("test,%d,%s,%s,%.10g,%.10g,%.10g,%d,%.10g\n", r0 + i + 1, f[0].c_str(), f[1].c_str(), env.getEpisodeReward(i),
                   env.getMeanEpisodeReward(i), pnl, ntr, pnl / ntr);
        }
    }
}

static int run(int argc, char** argv, int rank, int world, const std::string& rdzv) {
    std::string cfg_path, algo, theta_out, profit_log, stats_out, batch_log_path, md, tas, lob_ob, lob_msg, md_dir, tas_dir;
    int lob_levels = 0, plog_first = 0, plog_count = 0;
    int books = 1, episodes = -1, events = 2112, depth = 5, sync_every = 64;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(1); } return std::string(argv[++i]); };
        if (a == "-c" || a == "--config") cfg_path = next();
        else if (a == "-n") books = atoi(next().c_str());
        else if (a == "-e") episodes = atoi(next().c_str());
        else if (a == "-a" || a == "--algorithm") algo = next();
        else if (a == "--events") events = atoi(next().c_str());
        else if (a == "--depth") depth = atoi(next().c_str());
        else if (a == "--theta") theta_out = next();
        else if (a == "--profit-log") profit_log = next();
        else if (a == "--profit-log-books") {
            const std::string v = next();
            if (sscanf(v.c_str(), "%d:%d", &plog_first, &plog_count) != 2 || plog_first < 0 || plog_count < 1) { fprintf(stderr, "--profit-log-books first:count\n"); return 1; }
        }
        else if (a == "--stats-out") stats_out = next();   // env.writeStats(output_dir + "test_stats.csv"), src/main.cpp:242
        else if (a == "--batch-log") batch_log_path = next();
        else if (a == "--md") md = next();
        else if (a == "--tas") tas = next();
        else if (a == "--md-dir") md_dir = next();
        else if (a == "--tas-dir") tas_dir = next();
        else if (a == "--lobster") { lob_ob = next(); lob_msg = next(); lob_levels = atoi(next().c_str()); }
        else if (a == "--gpus") next();
        else if (a == "--sync-every") sync_every = atoi(next().c_str());
        else { fprintf(stderr, "unknown flag %s\n", a.c_str()); return 1; }
    }
    try {
        if (cfg_path.empty()) throw std::runtime_error("A configuration file must be provided (-c)");  // main.cpp:300-304
        lob::Config c(cfg_path);
        if (!algo.empty()) c.set("learning.algorithm", algo);  // CLI override, main.cpp:342-347
        std::string ticker = c.has("data.symbols") ? c.list("data.symbols").at(0) : "HSBA.L";
        lob_params p = c.to_params(ticker, depth, 2);
        // training.n_episodes (src/main.cpp:91 reads it into n_train_episodes -- a required key there too --, train() runs until that
        // many episodes are done, main.cpp:53-77); -e overrides it (the reference has no such flag: its tests edit the yaml)
        if (episodes < 0) episodes = (int)c.integer("training.n_episodes");
        p.book_id_offset = (uint64_t)rank * (uint64_t)books;  // global book ids: streams and RNG draws do not depend on the sharding
        lob::BatchedIntraday env(p, books, rank);
        lob_comm* comm = nullptr;
        if (!rdzv.empty()) lob::check(lob_comm_create_file(rdzv.c_str(), rank, world, rank, 300, &comm), "lob_comm_create_file");
        if (md_dir.empty() && c.has("data.md_dir")) md_dir = c.str("data.md_dir");
        if (tas_dir.empty() && c.has("data.tas_dir")) tas_dir = c.str("data.tas_dir");
        DaySplit days;
        if (!md_dir.empty() || !tas_dir.empty()) {
            days = load_day_library(c, p, md_dir, tas_dir, env);
        } else if (!md.empty() || !lob_ob.empty()) {
            // the reference's data files (Intraday::LoadData reads the CSV pair, intraday.cpp:141-150)
            uint32_t* rec = nullptr;
            int32_t n = 0;
            if (!md.empty()) lob::check(lob_convert_csv(md.c_str(), tas.c_str(), p.max_trades, &rec, &n), "LoadData");
            else lob::check(lob_convert_lobster(lob_ob.c_str(), lob_msg.c_str(), lob_levels, depth, p.max_trades, &rec, &n), "LoadData");
            const int window = events < n ? events : n;
            std::vector<int64_t> phase(books);
            for (int b = 0; b < books; b++) phase[b] = books > 1 ? (int64_t)(n - window) * b / (books - 1) : 0;
            env.LoadReplay(rec, n, phase, window);
            lob_free(rec);
        } else {
            lob_gen_params g;
            lob_default_gen_params(&g);
            g.n_events = events;
            g.seed = p.seed;
            env.LoadSynthetic(g);
        }
        lob::Agent agent(env, c);
        lob::Learner learner(env, 8);
        if (comm) learner.set_comm(comm, sync_every);
        BatchLog batch_log;
        if (batch_log_path.empty()) batch_log_path = c.str("logging.batch_log", "");
        if (!batch_log_path.empty()) batch_log.open(world > 1 ? batch_log_path + ".rank" + std::to_string(rank) : batch_log_path);
        if (rank == 0) printf("episode,episode_id,reward,pnl,n_steps,epsilon\n");
        for (int ep = 0; ep < episodes; ep++) {
            auto t0 = std::chrono::steady_clock::now();
            if (days.n_train > 0) env.SelectDays(LOB_DAYS_RANDOM, 0, days.n_train);   // rs.sample() + env.LoadData, src/main.cpp:53-55
            if (!learner.RunEpisode(&agent)) { fprintf(stderr, "[!] no data\n"); return 2; }
            double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            int64_t cnt[4];
            lob::check(lob_get_counters(env.handle(), cnt), "counters");
            const std::string ep_id = days.n_train > 0 ? days.files[env.Days()[0]][1] : env.getEpisodeId();
            if (rank == 0) printf("%d,%s,%.10g,%.10g,%d,%.6g\n", ep + 1, ep_id.c_str(), env.getEpisodeReward(0), env.getEpisodePnL(0),
                   env.book(0).total_ticks, agent.epsilon_);
            batch_log.write(std::to_string(ep + 1), env, days.n_train > 0 ? &days.files : nullptr, agent.epsilon_);
            fprintf(stderr, "[rank %d/%d] episode %d: %lld env-steps over %d books in %.3f s\n", rank, world, ep + 1, (long long)cnt[0], books, sec);
        }
        if (!theta_out.empty() && rank == 0) agent.write_theta(theta_out);  // replicas agree after the last exchange
        if (comm) { lob_comm_barrier(comm); lob_comm_destroy(comm); comm = nullptr; }
        if (days.n_test > 0 && rank == 0) evaluate_days(c, p, days, env, batch_log);
        if (!profit_log.empty() && rank == 0) {
            // src/main.cpp:217-239: GoGreedy() then one Backtester episode with profit logging (book 0)
            agent.GoGreedy();
            lob::Backtester bt(env, 8);
            if (plog_count > 0) bt.start_logging_books(profit_log, plog_first, plog_count, 20200102);
            else bt.start_logging(profit_log, 20200102);
            if (!bt.RunEpisode(&agent)) { fprintf(stderr, "[!] no data\n"); return 2; }
            bt.stop_logging();
            printf("backtest,%.10g,%.10g,%d\n", env.getEpisodeReward(0), env.getEpisodePnL(0), env.book(0).total_ticks);
        }
        if (!stats_out.empty() && rank == 0) {
            // src/main.cpp:234-242: nTr / Ppt on the console, then writeStats (book 0; quirk Q17: the trade statistics survive)
            printf("stats,%d,%.10g\n", env.getTotalTransactions(0), env.getEpisodePnL(0) / env.getTotalTransactions(0));
            env.writeStats(stats_out, 0);
        }
    } catch (std::exception& e) {
        fprintf(stderr, "Unhandled Exception: %s\n", e.what());  // main.cpp:364-368
        return 2;
    }
    return 0;
}
