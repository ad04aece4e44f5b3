// Translation unit of the book snapshots of the vector-env interface (include/lob_engine.h lob_snapshot_*; lob_launch.h SnapArgs;
// DESIGN.md 7g): snapshot_masked_kernel / snapshot_all_kernel.  A unit of its own, so that the units of the step and of lob_reset are
// compiled from what they were.  gfx950 only; no CPU execution path.
//   Pure data movement between the live arrays of a book's environment state and one slot buffer that holds them in the live layout
// ([B], or [w][B] for the rings), each at a 16-byte aligned offset: RESTORE = false copies live -> slot, true slot -> live.  The
// arrays are named by a descriptor table in device memory (SnapRow per [B] row, the 4-byte rows first; SnapArr per whole array), so
// the kernels carry two pointers instead of sixty.
#define LOB_TU_SPLIT 1
#define LOB_TU_SNAPSHOT 1
#include <hip/hip_runtime.h>

#include "lob_launch.h"

#define LOB_SNAP_BATCH 8   // rows whose loads are in flight before the first store (masked path)
#define LOB_SNAP_QUADS 4   // 16-byte loads per lane in flight before the first store (all-books path)

static_assert(LOB_SNAP_QUADS == 4 && sizeof(LHdr) == 64 && sizeof(SnapRow) == 16 && sizeof(SnapArr) == 32, "the records the kernels index");

// A pointer read from the table is generic to the compiler: lob_g (lob_state.h) makes its loads and stores global_, not flat_.
template <class T> __device__ __forceinline__ T* snap_global(T* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return lob_g(p);
#else
    return p;   // (the host pass only parses the kernels)
#endif
}

// Book b's element of LOB_SNAP_BATCH rows (`n` of them where the table ends), all loads first, then the stores.  The table entries
// are uniform: scalar loads.
template <class T, bool RESTORE, bool FULL>
__device__ __forceinline__ void snap_batch(const SnapRow* __restrict__ tab, int n, char* slot, int b) {
    const T* src[LOB_SNAP_BATCH];
    T* dst[LOB_SNAP_BATCH];
    T v[LOB_SNAP_BATCH];
#pragma unroll
    for (int u = 0; u < LOB_SNAP_BATCH; u++) {
        const SnapRow r = tab[FULL || u < n ? u : 0];
        T* live = snap_global(reinterpret_cast<T*>(r.live));
        T* held = reinterpret_cast<T*>(slot + r.off);
        src[u] = RESTORE ? held : live;
        dst[u] = RESTORE ? live : held;
    }
#pragma unroll
    for (int u = 0; u < LOB_SNAP_BATCH; u++)
        if (FULL || u < n) v[u] = src[u][b];
#pragma unroll
    for (int u = 0; u < LOB_SNAP_BATCH; u++)
        if (FULL || u < n) dst[u][b] = v[u];
}
template <class T, bool RESTORE>
__device__ __forceinline__ void snap_rows(const SnapRow* __restrict__ tab, int n, char* slot, int b) {
    int i = 0;
    for (; i + LOB_SNAP_BATCH <= n; i += LOB_SNAP_BATCH) snap_batch<T, RESTORE, true>(tab + i, LOB_SNAP_BATCH, slot, b);
    if (i < n) snap_batch<T, RESTORE, false>(tab + i, n - i, slot, b);
}

// The two per-book records: the environment's five words of the step header -- done, time_ms, action, stepped, reward; the learner's
// words of the same 64 bytes are neither read nor written -- held as four i32 rows and one f64 row, and slot 2 of the state vectors
// (the latest getState(), 64 bytes: four quads), held book-major as it lives.
template <bool RESTORE>
__device__ __forceinline__ void snap_book_records(const SnapArgs& a, char* slot, int b) {
    const size_t B = (size_t)a.B;
    i32* hw = reinterpret_cast<i32*>(slot + a.off_hdr);
    f64* hr = reinterpret_cast<f64*>(slot + a.off_reward);
    uint4* hv = reinterpret_cast<uint4*>(slot + a.off_vars) + (size_t)b * 4;
    LHdr* h = a.hdr + b;
    uint4* lv = reinterpret_cast<uint4*>(a.vars + ((size_t)b * 3 + 2) * 16);
    if (RESTORE) {
        const i32 done = hw[b], time_ms = hw[B + b], action = hw[2 * B + b], stepped = hw[3 * B + b];
        const f64 reward = hr[b];
        const uint4 v0 = hv[0], v1 = hv[1], v2 = hv[2], v3 = hv[3];
        h->done = done; h->time_ms = time_ms; h->action = action; h->stepped = stepped;
        h->reward = reward;
        lv[0] = v0; lv[1] = v1; lv[2] = v2; lv[3] = v3;
    } else {
        const i32 done = h->done, time_ms = h->time_ms, action = h->action, stepped = h->stepped;
        const f64 reward = h->reward;
        const uint4 v0 = lv[0], v1 = lv[1], v2 = lv[2], v3 = lv[3];
        hw[b] = done; hw[B + b] = time_ms; hw[2 * B + b] = action; hw[3 * B + b] = stepped;
        hr[b] = reward;
        hv[0] = v0; hv[1] = v1; hv[2] = v2; hv[3] = v3;
    }
}

// Masked path: a lane per book.  The lane reads its mask byte once; a lane whose book is not selected, or lies past B, issues
// nothing.  Consecutive lanes touch consecutive elements of every row: every access is coalesced.  No atomics, no LDS.
// (The table comes as a `const __restrict__` kernel argument of its own: its entries then stay scalar loads behind the first store.)
template <bool RESTORE>
__global__ __launch_bounds__(LOB_SNAP_BLOCK) void snapshot_masked_kernel(SnapArgs a, const SnapRow* __restrict__ rows, char* slot, const uint8_t* __restrict__ mask) {
    const int b = blockIdx.x * LOB_SNAP_BLOCK + threadIdx.x;
    if (b >= a.B) return;
    if (mask[b] == 0) return;
    snap_rows<uint32_t, RESTORE>(rows, a.n4, slot, b);
    snap_rows<u64, RESTORE>(rows + a.n4, a.n8, slot, b);
    snap_book_records<RESTORE>(a, slot, b);
}

// All-books path: every array is `bytes` contiguous bytes on both sides, both 16-byte aligned.  blockIdx.y names the array (y ==
// n_arr: the per-book records, a lane per book), the blocks of a row of the grid stride over the array's quads with LOB_SNAP_QUADS
// 16-byte loads in flight per lane; the words behind the last whole quad (B x 4 need not be a multiple of 16) go a word per lane.
template <bool RESTORE>
__global__ __launch_bounds__(LOB_SNAP_BLOCK) void snapshot_all_kernel(SnapArgs a, const SnapArr* __restrict__ arrs, char* slot) {
    if ((int)blockIdx.y == a.n_arr) {
        for (int b = blockIdx.x * LOB_SNAP_BLOCK + threadIdx.x; b < a.B; b += gridDim.x * LOB_SNAP_BLOCK) snap_book_records<RESTORE>(a, slot, b);
        return;
    }
    const SnapArr r = arrs[blockIdx.y];
    char* live = snap_global(reinterpret_cast<char*>(r.live));
    char* held = slot + r.off;
    const char* src = RESTORE ? held : live;
    char* dst = RESTORE ? live : held;
    const size_t nq = r.bytes >> 4;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    const size_t step = (size_t)gridDim.x * LOB_SNAP_BLOCK * LOB_SNAP_QUADS;
    for (size_t q0 = (size_t)blockIdx.x * LOB_SNAP_BLOCK * LOB_SNAP_QUADS + threadIdx.x; q0 < nq; q0 += step) {
        // (four named registers, not an array: an array written under the guards is placed in LDS.  No load under a branch: a quad
        // past the array's end is fetched from q0 instead, a valid address, and not stored)
        const size_t q1 = q0 + LOB_SNAP_BLOCK, q2 = q0 + 2 * LOB_SNAP_BLOCK, q3 = q0 + 3 * LOB_SNAP_BLOCK;
        const bool h1 = q1 < nq, h2 = q2 < nq, h3 = q3 < nq;
        const uint4 v0 = s4[q0];
        const uint4 v1 = s4[h1 ? q1 : q0];
        const uint4 v2 = s4[h2 ? q2 : q0];
        const uint4 v3 = s4[h3 ? q3 : q0];
        d4[q0] = v0;
        if (h1) d4[q1] = v1;
        if (h2) d4[q2] = v2;
        if (h3) d4[q3] = v3;
    }
    if (blockIdx.x == 0) {
        const size_t w = (nq << 2) + threadIdx.x;   // (at most three words)
        if (w < (r.bytes >> 2)) reinterpret_cast<uint32_t*>(dst)[w] = reinterpret_cast<const uint32_t*>(src)[w];
    }
}

void lobk_snapshot(hipStream_t st, bool restore, const SnapArgs& a, void* slot, const uint8_t* dev_mask) {
    const dim3 block(LOB_SNAP_BLOCK);
    if (dev_mask) {
        const dim3 grid((a.B + LOB_SNAP_BLOCK - 1) / LOB_SNAP_BLOCK);
        if (restore) hipLaunchKernelGGL(snapshot_masked_kernel<true>, grid, block, 0, st, a, a.rows, (char*)slot, dev_mask);
        else hipLaunchKernelGGL(snapshot_masked_kernel<false>, grid, block, 0, st, a, a.rows, (char*)slot, dev_mask);
        return;
    }
    // a row of the grid covers the largest array in one pass where 64 blocks do (a ring of w rows: w x B x 8 bytes), else strides
    const size_t per_block = (size_t)LOB_SNAP_BLOCK * LOB_SNAP_QUADS * 16;
    size_t gx = (a.max_bytes + per_block - 1) / per_block;
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    const dim3 grid((unsigned)gx, (unsigned)a.n_arr + 1);
    if (restore) hipLaunchKernelGGL(snapshot_all_kernel<true>, grid, block, 0, st, a, a.arrs, (char*)slot);
    else hipLaunchKernelGGL(snapshot_all_kernel<false>, grid, block, 0, st, a, a.arrs, (char*)slot);
}
