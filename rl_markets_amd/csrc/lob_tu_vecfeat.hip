// Translation unit of the tile features and the external weight updates on the vector-env interface (include/lob_engine.h
// lob_vec_features / lob_vec_update; lob_launch.h VecFeatSrc): vec_feat_kernel.  A unit of its own, so that the units
// of the step and of lob_reset are compiled from what they were.  gfx950 only; no CPU execution path.
//   The 96 action-independent hash sums of a state's tiles (lob_tiles.h tile_base_m) from device memory to device memory, the
// tile indices of one action per state, and theta[tile] += step over those indices with the written-weights maps kept as
// delta_apply_kernel (lob_kernels.h) keeps them.
#define LOB_TU_SPLIT 1
#define LOB_TU_VECFEAT 1
#include <hip/hip_runtime.h>

#include "lob_internal.h"
#include "lob_kernels.h"

// One weight of the target vector is about to be written from outside a step: what delta_apply_kernel (lob_kernels.h, compiled in
// the main unit only) does where d != 0, restated -- the vector's "ever written" bit and, on the memo path (nzx non-null), the exact
// map's bit with the folded maps on first set (nzd_mark) and the coarse image's bit; every bit tested before its atomic.
__device__ __forceinline__ void vec_feat_mark(const VecFeatSrc& a, uint32_t* nz, uint32_t M, uint32_t f) {
    const uint32_t bit = LOB_NZ_BIT(f);
    if (!(nz[LOB_NZ_WORD(f)] & bit)) atomicOr(&nz[LOB_NZ_WORD(f)], bit);
    if (a.nzx) {  // the fast path's maps (shared theta; the double agents' two vectors share them)
        const uint32_t xb = 1u << (f & 31);
        if (!(a.nzx[f >> 5] & xb)) {
            const uint32_t old = atomicOr(&a.nzx[f >> 5], xb);
            if (!(old & xb) && a.nzd) nzd_mark(a.nzd, a.nzm, a.nzd_terms, M, f);
        }
        const uint32_t c = f >> a.cshift;
        if (!(a.nzc[c >> 5] & (1u << (c & 31)))) atomicOr(&a.nzc[c >> 5], 1u << (c & 31));
    }
}

// One WAVE per state in a persistent grid, as vec_act_kernel (lob_tu_vecact.hip): wave t takes states t, t + waves, ..., the 8 KB
// hash table and the 27 action terms are staged once per block, the state's sixteen words go through the wave's LDS row between two
// wave-level fences.
//   BOOKS: state s is book s, the row is slot 2 of S.vars (the latest getState()) -- the only thing read through the state pointer,
// whose device-resident copy the first lob_reset uploads; else row s of the caller's buffer, and nothing is read through it.
//   Lane l owns tile positions l and, below 32, l + 64: position p = 32 g + j is tiling j of group g (lanes 0..31: groups 0 and 2,
// lanes 32..63: group 1), each through tile_base_m with features_kernel's group rule.  Stores are contiguous per state: 256 + 128
// bytes of `sums`, the same of `idx`.
//   UPDATE: the lanes that own a position add step[s] to the weight of (state s, action[s]) there -- f64 atomics in no fixed order,
// as apply_kernel's -- after marking it (vec_feat_mark).  A row whose action is out of range is counted (one atomic per wave, at
// the end) and skipped; a row whose step is exactly 0.0 writes and marks nothing.  The first wave of the launch that writes bumps
// nz_epoch: `tag` holds the number of the last launch that did.
//   No LDS beyond LearnLds, no scratch.
template <bool BOOKS, bool UPDATE>
__global__ void __launch_bounds__(LOB_BLOCK, 6) vec_feat_kernel(LOB_PS_ARGS, const uint32_t* __restrict__ rnd_g, VecFeatSrc a) {
    const DevParams& P = *Pp;   // parameters read through the scalar cache, never copied to scratch
    __shared__ LearnLds L;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    learn_stage_table(rnd_g, L);   // (every thread of the block: ends in the block barrier)
    const int t0 = __builtin_amdgcn_readfirstlane(blockIdx.x * LOB_WAVES_PER_BLOCK + w);
    const int stride = gridDim.x * LOB_WAVES_PER_BLOCK;
    const int V = P.V;
    const uint32_t M = (uint32_t)P.M;
    f32* row = &L.vars[w][0][0];
    // the lane's positions: p0 = lane (group lane >> 5), p1 = lane + 64 (group 2; lanes 0..31)
    const int g0 = lane >> 5, j = lane & 31;
    const int nf0 = g0 == 0 ? 3 : V - 3;
    const f32* v0 = g0 == 0 ? row : row + 3;
    const bool two = lane < 32;
    int n_bad = 0;
    bool wrote = false;
#pragma unroll 1
    for (int s = t0; s < a.n; s += stride) {
        int act = 0;
        bool valid = true;
        f64 st = 0.0;
        if (a.actions) {   // (uniform; a wave-uniform address: scalar loads)
            act = a.actions[s];
            valid = (uint32_t)act < (uint32_t)LOB_N_ACTIONS;
        }
        if (UPDATE) {
            if (!valid) { n_bad++; continue; }
            st = a.step[s];
            if (st == 0.0) continue;   // (a NaN compares unequal: it is added as it is)
        }
        // the state's words into the wave's LDS row, as learn_stage_vars hands a book's over (slots >= V hold 0)
        const f32* src = BOOKS ? Sp->vars + ((size_t)s * 3 + 2) * 16 : a.rows + (size_t)s * (size_t)V;
        const f32 vv = lane < V ? src[lane] : 0.0f;
        wave_lds_fence();   // the previous state's readers are done with the row
        if (lane < 16) row[lane] = vv;
        wave_lds_fence();
        const uint32_t b0 = tile_base_m(M, v0, nf0, j, L.rnd);
        const uint32_t b1 = two ? tile_base_m(M, row, V, j, L.rnd) : 0u;
        const size_t o = (size_t)s * LOB_N_TILES;
        if (!UPDATE && a.sums) {
            a.sums[o + lane] = (i32)b0;
            if (two) a.sums[o + 64 + lane] = (i32)b1;
        }
        if (!UPDATE && !a.idx) continue;
        const i32 i0 = valid ? tile_index(b0, L.act_terms[g0 * LOB_N_ACTIONS + act], M) : -1;
        const i32 i1 = valid ? tile_index(b1, L.act_terms[2 * LOB_N_ACTIONS + act], M) : -1;
        if (!UPDATE) {
            a.idx[o + lane] = i0;
            if (two) a.idx[o + 64 + lane] = i1;
        } else {
            const size_t off = BOOKS && P.theta_private ? (size_t)s : 0;
            f64* theta = a.theta + off * (size_t)M;
            uint32_t* nz = a.nz + off * LOB_NZ_NWORDS(M);
            vec_feat_mark(a, nz, M, (uint32_t)i0);
            __hip_atomic_fetch_add(&theta[(uint32_t)i0], st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (two) {
                vec_feat_mark(a, nz, M, (uint32_t)i1);
                __hip_atomic_fetch_add(&theta[(uint32_t)i1], st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            wrote = true;
        }
    }
    if (UPDATE && lane == 0) {
        if (n_bad) atomicAdd(a.n_bad, (u64)n_bad);
        // verdicts saved before this update are stale: once per launch that writes anything
        if (wrote && __hip_atomic_load(a.tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != a.launch) {
            if (atomicExch(a.tag, a.launch) != a.launch) atomicAdd(a.nz_epoch, 1);
        }
    }
}

void lobk_vec_feat(hipStream_t st, int n_cus, const DevParams* Pd, const DevState* Sd, const uint32_t* rnd, const VecFeatSrc& a) {
    const int need = (a.n + LOB_WAVES_PER_BLOCK - 1) / LOB_WAVES_PER_BLOCK;
    // the blocks a compute unit holds at once (four waves each: the kernel's waves per SIMD), so that no block waits for another's end
    int grid = n_cus * 6;
    if (grid > LOB_VECFEAT_MAX_BLOCKS) grid = LOB_VECFEAT_MAX_BLOCKS;
    if (grid > need) grid = need;
    const bool upd = a.step != nullptr;
    if (a.rows) {
        if (upd) hipLaunchKernelGGL((vec_feat_kernel<false, true>), dim3(grid), dim3(LOB_BLOCK), 0, st, Pd, Sd, rnd, a);
        else hipLaunchKernelGGL((vec_feat_kernel<false, false>), dim3(grid), dim3(LOB_BLOCK), 0, st, Pd, Sd, rnd, a);
    } else {
        if (upd) hipLaunchKernelGGL((vec_feat_kernel<true, true>), dim3(grid), dim3(LOB_BLOCK), 0, st, Pd, Sd, rnd, a);
        else hipLaunchKernelGGL((vec_feat_kernel<true, false>), dim3(grid), dim3(LOB_BLOCK), 0, st, Pd, Sd, rnd, a);
    }
}
