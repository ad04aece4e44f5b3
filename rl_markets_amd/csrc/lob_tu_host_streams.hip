// Host side of the C ABI, what feeds the engine (include/lob_engine.h; lob_engine_impl.h): the event streams -- loaded, staged for the
// next episode, replayed from one shared stream, generated on the device -- and the day library with its selections.  No kernel
// is compiled here: every launch goes through lob_launch.h.  gfx950 only; no CPU execution path.
#define LOB_TU_SPLIT 1
#include <limits.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <system_error>

#include "lob_engine_impl.h"

static int stage_join(lob_engine* e) {
    if (e->stage_thread.joinable()) e->stage_thread.join();
    if (e->stage_rc != LOB_OK) lob_set_error(e->stage_err);
    return e->stage_rc;
}

namespace lob {

// the day library's tables and per-book sets (set_records, lob_destroy)
void free_days(lob_engine* e) {
    if (e->day_copied) hipEventSynchronize(e->day_copied);   // (the pinned buffer may still be read by a copy in flight)
    for (void* p : {(void*)e->day_first_dev, (void*)e->day_len_dev, (void*)e->day_rng, (void*)e->day_explicit, (void*)e->lib_phase[0],
                    (void*)e->lib_phase[1], (void*)e->lib_len[0], (void*)e->lib_len[1], (void*)e->lib_day[0], (void*)e->lib_day[1]})
        if (p) hipFree(p);
    if (e->day_explicit_host) hipHostFree(e->day_explicit_host);
    if (e->day_copied) hipEventDestroy(e->day_copied);
    e->day_first_dev = nullptr; e->day_len_dev = nullptr; e->day_rng = nullptr; e->day_explicit = nullptr; e->day_explicit_host = nullptr;
    e->day_copied = nullptr;
    for (int i = 0; i < 2; i++) { e->lib_phase[i] = nullptr; e->lib_len[i] = nullptr; e->lib_day[i] = nullptr; }
    e->lib = false;
    e->lib_days = 0;
    e->lib_cur = -1;
    e->lib_pending = false;
}

// (lob_reset) the staged stream becomes the current one: the buffers change places
int stage_adopt(lob_engine* e) {
    if (!e->stage_active) return LOB_OK;
    const int rc = stage_join(e);
    e->stage_active = false;
    if (rc != LOB_OK) return rc;
    std::swap(e->records_dev, e->records_next);
    e->S.records = e->records_dev;
    return LOB_OK;
}

}  // namespace lob

extern "C" {

// n_rows: records to allocate (B * n_events for per-book streams, the stream length for a replayed one)
static int set_records(lob_engine* e, int32_t n_events, size_t n_rows) {
    // (the TickStatistics counters of a book are 32-bit like the reference's ints, lob_state.h tick_ab / tick_pos / tick_both: one count
    // per agent step, at most one agent step per event, n_events < 2^31 -- a recorded day of millions of rows is fine)
    { int rc = finalize_episode(e); if (rc) return rc; }  // needs the old stream
    if (e->stage_active) { (void)stage_join(e); e->stage_active = false; }   // (a staged stream is void once another one is loaded)
    if (e->records_next) { hipFree(e->records_next); e->records_next = nullptr; }
    // the old stream is gone from here on, whatever happens below: no kernel may see a freed pointer
    e->have_events = false;
    e->was_reset = false;
    e->S.records = nullptr;
    e->S.track = nullptr;
    e->S.rec_phase = nullptr;
    e->S.rec_len = nullptr;
    e->S.n_events = 0;
    if (e->phase_dev) { hipFree(e->phase_dev); e->phase_dev = nullptr; }
    free_days(e);
    const size_t bytes = n_rows * e->P.Wd * 4 + 256;  // (tail pad: drec_levels reads whole 16-byte quads past a short level array)
    // market track: resident (one entry per event) up to track_ring events per book, a ring of that many beyond
    e->chunked = n_events > e->sw.track_ring;
    e->S.track_len = e->chunked ? e->sw.track_ring : n_events;
    e->S.track_mask = e->chunked ? e->sw.track_ring - 1 : 0x7fffffff;
    const size_t track_bytes = (size_t)e->B * e->S.track_len * sizeof(Track);
    // (a stream of the size of the one before it -- a fresh day per episode -- moves into the buffers that are there: freeing and
    // allocating 31 + 18 GB cost more than the copy of a whole stream, round 6)
    hipError_t err = hipSuccess;
    if (!e->records_dev || e->records_bytes != bytes) {
        if (e->records_dev) { hipFree(e->records_dev); e->records_dev = nullptr; }
        err = hipMalloc((void**)&e->records_dev, bytes);
        if (err != hipSuccess) { e->records_dev = nullptr; e->records_bytes = 0; lob_set_error("hipMalloc(records) failed"); return LOB_ENOMEM; }
        e->records_bytes = bytes;
    }
    if (!e->track_dev || e->track_bytes != track_bytes) {
        if (e->track_dev) { hipFree(e->track_dev); e->track_dev = nullptr; }
        err = hipMalloc((void**)&e->track_dev, track_bytes);
        if (err != hipSuccess) {
            e->track_dev = nullptr; e->track_bytes = 0;
            hipFree(e->records_dev);
            e->records_dev = nullptr; e->records_bytes = 0;
            lob_set_error("hipMalloc(track) failed");
            return LOB_ENOMEM;
        }
        e->track_bytes = track_bytes;
    }
    e->S.track = e->track_dev;
    e->S.records = e->records_dev;
    e->S.n_events = n_events;
    e->have_events = true;
    e->was_reset = false;
    return LOB_OK;
}

// A few host threads that copy one piece into a pinned staging buffer together, started once per upload (round 5 started and joined
// up to seven per 64 MB piece: ~2 900 thread creations for 26.6 GB).  std::thread's constructor throws when the process may not
// start another thread; the pool then runs with the workers it got -- none at all is fine, the caller's thread copies alone.
struct CopyPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    char* dst = nullptr;
    const char* src = nullptr;
    size_t nb = 0;
    unsigned long long gen = 0;
    unsigned pending = 0;
    bool quit = false;
    unsigned parts() const { return (unsigned)th.size() + 1; }
    explicit CopyPool(unsigned want) {
        try {
            for (unsigned t = 1; t < want; t++) th.emplace_back([this, t] { worker(t); });
        } catch (const std::system_error&) {
        }
    }
    void worker(unsigned t) {
        unsigned long long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(mu);
            cv_go.wait(lk, [&] { return quit || gen != seen; });
            if (quit) return;
            seen = gen;
            char* d = dst; const char* s = src; const size_t n = nb; const unsigned np = parts();
            lk.unlock();
            if (t < np) { const size_t a = n * t / np, b = n * (t + 1) / np; memcpy(d + a, s + a, b - a); }
            lk.lock();
            if (--pending == 0) cv_done.notify_one();
        }
    }
    void copy(char* d, const char* s, size_t n) {
        {
            std::lock_guard<std::mutex> lk(mu);
            dst = d; src = s; nb = n; pending = (unsigned)th.size(); gen++;
        }
        cv_go.notify_all();
        memcpy(d, s, n / parts());
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
    }
    ~CopyPool() {
        { std::lock_guard<std::mutex> lk(mu); quit = true; }
        cv_go.notify_all();
        for (auto& t : th) t.join();
    }
};

// host ABI records -> HBM in the device layout.  Small uploads: one pageable copy into a temporary device buffer, one repack.
// Big ones (the 26.6 GB of 65 536 private streams): 64 MB pieces through two pinned staging buffers -- a few host threads copy
// piece k + 1 into its buffer while the DMA engine and the repack kernel are on piece k -- so the hand-over runs at what the
// slower of the host's memcpy and the link gives instead of the runtime's pageable path, and the temporary device copy is two
// pieces, not another whole stream.  Without pinned memory (a locked-memory limit; LOB_UPLOAD_PINNED=0 forces it, for the tests)
// the same pieces go from the caller's pageable memory directly: slower, and still two pieces of device memory, never a second
// whole stream.
static int upload_records(lob_engine* e, const uint32_t* host_records, size_t n_records, hipStream_t st = nullptr, uint32_t* dst = nullptr) {
    if (!st) st = e->stream;
    if (!dst) dst = e->records_dev;
    const size_t rec_bytes = (size_t)e->P.W * 4;
    const size_t bytes = n_records * rec_bytes;
    size_t piece_recs = std::max<size_t>(1, ((size_t)64 << 20) / rec_bytes);
    if (e->sw.upload_piece_recs) piece_recs = (size_t)e->sw.upload_piece_recs;  // (tests: many small pieces)
    if (n_records <= 2 * piece_recs) {
        uint32_t* tmp = nullptr;
        if (hipMalloc((void**)&tmp, bytes) != hipSuccess) { lob_set_error("hipMalloc(upload buffer) failed"); return LOB_ENOMEM; }
        hipError_t err = hipMemcpyAsync(tmp, host_records, bytes, hipMemcpyHostToDevice, st);
        if (err == hipSuccess) {
            lobk_repack(st, (const uint32_t*)tmp, e->P.D, e->P.T, n_records, dst);
            err = hipGetLastError();
        }
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        hipFree(tmp);
        if (err != hipSuccess) { lob_set_error(std::string("record upload: ") + hipGetErrorString(err)); return LOB_EHIP; }
        return LOB_OK;
    }
    const size_t piece_bytes = piece_recs * rec_bytes;
    void* pinned[2] = {nullptr, nullptr};
    uint32_t* tmp[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    auto release = [&]() {
        for (int i = 0; i < 2; i++) {
            if (done[i]) hipEventDestroy(done[i]);
            if (tmp[i]) hipFree(tmp[i]);
            if (pinned[i]) hipHostFree(pinned[i]);
        }
    };
    hipError_t err = hipSuccess;
    for (int i = 0; i < 2 && err == hipSuccess; i++) {
        err = hipMalloc((void**)&tmp[i], piece_bytes);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&done[i], hipEventDisableTiming);
    }
    if (err != hipSuccess) { release(); lob_set_error("hipMalloc(upload pieces) failed"); return LOB_ENOMEM; }
    bool use_pinned = e->sw.upload_pinned;
    for (int i = 0; i < 2 && use_pinned; i++)
        if (hipHostMalloc(&pinned[i], piece_bytes, hipHostMallocDefault) != hipSuccess) {   // (no pinned memory to be had: the pageable pieces below)
            (void)hipGetLastError();
            pinned[i] = nullptr;
            use_pinned = false;
        }
    if (!use_pinned) for (int i = 0; i < 2; i++) if (pinned[i]) { hipHostFree(pinned[i]); pinned[i] = nullptr; }
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 8 ? 8 : nt;
    int rc = LOB_OK;
    try {
        CopyPool pool(use_pinned ? nt : 1);
        const size_t n_pieces = (n_records + piece_recs - 1) / piece_recs;
        for (size_t k = 0; k < n_pieces && err == hipSuccess; k++) {
            const int i = (int)(k & 1);
            const size_t r0 = k * piece_recs, nr = std::min(piece_recs, n_records - r0), nb = nr * rec_bytes;
            if (k >= 2) err = hipEventSynchronize(done[i]);  // (piece k - 2 has left this staging buffer and its device copy)
            if (err != hipSuccess) break;
            const char* src = reinterpret_cast<const char*>(host_records) + r0 * rec_bytes;
            if (use_pinned) {
                pool.copy(reinterpret_cast<char*>(pinned[i]), src, nb);
                err = hipMemcpyAsync(tmp[i], pinned[i], nb, hipMemcpyHostToDevice, st);
            } else {
                err = hipMemcpyAsync(tmp[i], src, nb, hipMemcpyHostToDevice, st);   // (pageable: the runtime stages it, synchronously)
            }
            if (err == hipSuccess) {
                lobk_repack(st, (const uint32_t*)tmp[i], e->P.D, e->P.T, nr, dst + r0 * (size_t)e->P.Wd);
                err = hipGetLastError();
            }
            if (err == hipSuccess) err = hipEventRecord(done[i], st);
        }
    } catch (const std::exception& ex) {   // (nothing may cross the C ABI)
        lob_set_error(std::string("record upload: ") + ex.what());
        rc = LOB_ENOMEM;
    }
    const hipError_t err2 = hipStreamSynchronize(st);
    if (err == hipSuccess) err = err2;
    release();
    if (rc != LOB_OK) return rc;
    if (err != hipSuccess) { lob_set_error(std::string("record upload: ") + hipGetErrorString(err)); return LOB_EHIP; }
    return LOB_OK;
}

int lob_load_events(lob_engine* e, const uint32_t* host_records, int32_t n_events) {
    if (!e || !host_records || n_events < 2) { lob_set_error("lob_load_events: bad argument"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    int rc = lob_validate_stream(host_records, e->P.D, e->P.T, e->B, n_events);
    if (rc != LOB_OK) return rc;
    rc = set_records(e, n_events, (size_t)e->B * n_events);
    if (rc != LOB_OK) return rc;
    e->have_events = false;  // (a failed upload leaves no stream behind)
    rc = upload_records(e, host_records, (size_t)e->B * n_events);
    e->have_events = rc == LOB_OK;
    return rc;
}

int lob_stage_events(lob_engine* e, const uint32_t* host_records, int32_t n_events) {
    if (!e || !host_records) { lob_set_error("lob_stage_events: bad argument"); return LOB_EINVAL; }
    if (!e->have_events || e->lib || e->S.rec_phase || n_events != e->S.n_events) {
        lob_set_error("lob_stage_events: needs a loaded per-book stream of the same length (lob_load_events first)");
        return LOB_ESTATE;
    }
    if (e->stage_active) { lob_set_error("lob_stage_events: the stream staged before has not been adopted (lob_reset) or waited for"); return LOB_ESTATE; }
    HIPCHK(hipSetDevice(e->device));
    const size_t n_rows = (size_t)e->B * n_events;
    if (!e->records_next) {
        if (hipMalloc((void**)&e->records_next, n_rows * e->P.Wd * 4 + 256) != hipSuccess) { e->records_next = nullptr; lob_set_error("hipMalloc(second record buffer) failed"); return LOB_ENOMEM; }
    }
    if (!e->stream_up) HIPCHK(hipStreamCreateWithFlags(&e->stream_up, hipStreamNonBlocking));
    e->stage_rc = LOB_OK;
    e->stage_err.clear();
    e->stage_active = true;
    try {
        e->stage_thread = std::thread([e, host_records, n_events, n_rows] {
            int rc = hipSetDevice(e->device) == hipSuccess ? LOB_OK : LOB_EHIP;
            if (rc == LOB_OK) rc = lob_validate_stream(host_records, e->P.D, e->P.T, e->B, n_events);
            if (rc == LOB_OK) rc = upload_records(e, host_records, n_rows, e->stream_up, e->records_next);
            e->stage_rc = rc;
            if (rc != LOB_OK) e->stage_err = lob_last_error();   // (the error text is the failing thread's: handed to whoever waits)
        });
    } catch (const std::system_error&) {   // no thread to be had: the hand-over happens here and now
        int rc = lob_validate_stream(host_records, e->P.D, e->P.T, e->B, n_events);
        if (rc == LOB_OK) rc = upload_records(e, host_records, n_rows, e->stream_up, e->records_next);
        e->stage_rc = rc;
        if (rc != LOB_OK) e->stage_err = lob_last_error();
    }
    return LOB_OK;
}
int lob_stage_wait(lob_engine* e) {
    if (!e) return LOB_EINVAL;
    if (!e->stage_active) { lob_set_error("lob_stage_wait: nothing staged"); return LOB_ESTATE; }
    return stage_join(e);
}

int lob_load_events_shared(lob_engine* e, const uint32_t* host_records, int64_t n_total, const int64_t* phase, int32_t n_events) {
    if (!e || !host_records || !phase || n_events < 2 || n_total < n_events || n_total > INT32_MAX) {
        lob_set_error("lob_load_events_shared: bad argument");
        return LOB_EINVAL;
    }
    for (int b = 0; b < e->B; b++)
        if (phase[b] < 0 || phase[b] + n_events > n_total) {
            lob_set_error("lob_load_events_shared: phase[" + std::to_string(b) + "] + n_events runs past the stream");
            return LOB_EINVAL;
        }
    HIPCHK(hipSetDevice(e->device));
    int rc = lob_validate_stream(host_records, e->P.D, e->P.T, 1, (int32_t)n_total);
    if (rc != LOB_OK) return rc;
    rc = set_records(e, n_events, (size_t)n_total);
    if (rc != LOB_OK) return rc;
    // until the phases are in place the buffer (n_total rows) must not pass for a per-book stream (B * n_events rows)
    e->have_events = false;
    hipError_t err = hipMalloc((void**)&e->phase_dev, (size_t)e->B * sizeof(i64));
    if (err != hipSuccess) { e->phase_dev = nullptr; lob_set_error("hipMalloc(phase) failed"); return LOB_ENOMEM; }
    rc = upload_records(e, host_records, (size_t)n_total);
    if (rc != LOB_OK) return rc;
    HIPCHK(hipMemcpyAsync(e->phase_dev, phase, (size_t)e->B * sizeof(i64), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->have_events = true;
    e->S.rec_phase = e->phase_dev;
    return LOB_OK;
}

int lob_load_days(lob_engine* e, const uint32_t* host_records, const int64_t* day_first, int32_t n_days) {
    if (!e || !host_records || !day_first || n_days < 1) { lob_set_error("lob_load_days: bad argument"); return LOB_EINVAL; }
    if (day_first[0] != 0) { lob_set_error("lob_load_days: day_first[0] must be 0"); return LOB_EINVAL; }
    int32_t longest = 0;
    std::vector<i32> len((size_t)n_days);
    for (int d = 0; d < n_days; d++) {
        const int64_t n = day_first[d + 1] - day_first[d];
        if (n < 2 || day_first[d + 1] > INT32_MAX) {
            lob_set_error("lob_load_days: day " + std::to_string(d) + " has fewer than 2 events, or day_first is not monotone / runs past 2^31 records");
            return LOB_EINVAL;
        }
        len[d] = (i32)n;
        longest = std::max(longest, (int32_t)n);
    }
    const int64_t n_total = day_first[n_days];
    HIPCHK(hipSetDevice(e->device));
    for (int d = 0; d < n_days; d++) {
        const int rc = lob_validate_stream(host_records + (size_t)day_first[d] * e->P.W, e->P.D, e->P.T, 1, len[d]);
        if (rc != LOB_OK) return rc;
    }
    // the track is sized by the longest day: a ring when that one is longer than the resident track
    int rc = set_records(e, longest, (size_t)n_total);
    if (rc != LOB_OK) return rc;
    e->have_events = false;   // (until the library and its tables are in place)
    rc = upload_records(e, host_records, (size_t)n_total);
    if (rc != LOB_OK) return rc;
    const size_t B = (size_t)e->B;
    bool ok = hipMalloc((void**)&e->day_first_dev, (size_t)n_days * sizeof(i64)) == hipSuccess &&
              hipMalloc((void**)&e->day_len_dev, (size_t)n_days * sizeof(i32)) == hipSuccess &&
              hipMalloc((void**)&e->day_rng, B * sizeof(uint32_t)) == hipSuccess && hipMalloc((void**)&e->day_explicit, B * sizeof(i32)) == hipSuccess &&
              hipHostMalloc((void**)&e->day_explicit_host, B * sizeof(i32), hipHostMallocDefault) == hipSuccess &&
              hipEventCreateWithFlags(&e->day_copied, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && ok; i++)
        ok = hipMalloc((void**)&e->lib_phase[i], B * sizeof(i64)) == hipSuccess && hipMalloc((void**)&e->lib_len[i], B * sizeof(i32)) == hipSuccess &&
             hipMalloc((void**)&e->lib_day[i], B * sizeof(i32)) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); free_days(e); lob_set_error("hipMalloc(day library tables) failed"); return LOB_ENOMEM; }
    // RandomSampler's std::default_random_engine rng(seed) (sampler.h:34-39): minstd_rand0 seeded with (unsigned)(seed + global book id)
    std::vector<uint32_t> rng(B);
    for (size_t b = 0; b < B; b++) {
        const uint32_t s = (uint32_t)(e->P.seed + e->P.book_id_offset + (u64)b);
        rng[b] = s % 2147483647u == 0 ? 1u : s % 2147483647u;
    }
    HIPCHK(hipMemcpyAsync(e->day_first_dev, day_first, (size_t)n_days * sizeof(i64), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->day_len_dev, len.data(), (size_t)n_days * sizeof(i32), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->day_rng, rng.data(), B * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->lib = true;
    e->lib_days = n_days;
    e->have_events = true;
    return LOB_OK;
}

// a selection needs a library (and a whole step: the guard behind it)
static int days_ready(lob_engine* e, const char* who) {
    if (!e->lib) { lob_set_error(std::string(who) + ": no day library loaded (lob_load_days)"); return LOB_ESTATE; }
    return LOB_OK;
}
// a selection for the next episode: days_draw_kernel writes the set the current episode does not play
static int days_draw(lob_engine* e, int mode, int first, int n) {
    HIPCHK(hipSetDevice(e->device));
    const int nx = e->lib_cur < 0 ? 0 : e->lib_cur ^ 1;
    TimedLaunch t(e, "days_draw_kernel", nullptr, true);
    lobk_days_draw(e->stream, e->B, e->P.book_id_offset, mode, first, n, e->day_explicit, e->day_rng, e->day_first_dev, e->day_len_dev, e->lib_phase[nx],
                   e->lib_len[nx], e->lib_day[nx]);
    HIPCHK(hipGetLastError());
    e->lib_pending = true;
    return LOB_OK;
}
int lob_days_select(lob_engine* e, int32_t mode, int32_t first_day, int32_t n_days) {
    if (!e) return LOB_EINVAL;
    { int rc = days_ready(e, "lob_days_select"); if (rc) return rc; }
    LOB_GUARD(e, lob_days_select);
    if ((mode != LOB_DAYS_RANDOM && mode != LOB_DAYS_IN_ORDER) || first_day < 0 || n_days < 1 || (int64_t)first_day + n_days > e->lib_days) {
        lob_set_error("lob_days_select: bad mode, or days " + std::to_string(first_day) + " + " + std::to_string(n_days) + " outside the library");
        return LOB_EINVAL;
    }
    return days_draw(e, mode, first_day, n_days);
}
int lob_days_set(lob_engine* e, const int32_t* host_day) {
    if (!e || !host_day) { lob_set_error("lob_days_set: bad argument"); return LOB_EINVAL; }
    { int rc = days_ready(e, "lob_days_set"); if (rc) return rc; }
    LOB_GUARD(e, lob_days_set);
    for (int b = 0; b < e->B; b++)
        if (host_day[b] < 0 || host_day[b] >= e->lib_days) { lob_set_error("lob_days_set: day of book " + std::to_string(b) + " outside the library"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipEventSynchronize(e->day_copied));   // (the copy of the selection before has left the pinned buffer)
    memcpy(e->day_explicit_host, host_day, (size_t)e->B * sizeof(i32));
    HIPCHK(hipMemcpyAsync(e->day_explicit, e->day_explicit_host, (size_t)e->B * sizeof(i32), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipEventRecord(e->day_copied, e->stream));
    return days_draw(e, LOB_DAYS_EXPLICIT, 0, 1);
}
int lob_get_days(lob_engine* e, int32_t* host_out) {
    if (!e || !host_out) { lob_set_error("lob_get_days: bad argument"); return LOB_EINVAL; }
    if (!e->lib || e->lib_cur < 0) { lob_set_error("lob_get_days: no episode on a day library yet (lob_load_days, a selection, lob_reset)"); return LOB_ESTATE; }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(host_out, e->lib_day[e->lib_cur], (size_t)e->B * sizeof(i32), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}

int lob_gen_events_device(lob_engine* e, const lob_gen_params* g) {
    if (!e || !g || g->n_events < 2) { lob_set_error("lob_gen_events_device: bad argument"); return LOB_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    int rc = set_records(e, g->n_events, (size_t)e->B * g->n_events);
    if (rc != LOB_OK) return rc;
    lobk_gen_events(e->stream, *g, e->P.D, e->P.T, e->P.book_id_offset, e->B, e->records_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return LOB_OK;
}

}  // extern "C"
