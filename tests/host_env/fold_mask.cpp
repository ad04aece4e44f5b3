// TEST INFRASTRUCTURE ONLY.  The index arithmetic of the per-sum action masks (rl_markets_amd/csrc/lob_tiles.h: fold_sum,
// fold_mask_words / _word / _shift), on the CPU, compiled from the engine's own device header through tests/host_env/shim:
//   (1) fold_sum(f, t, M) is the ONE hash sum s < M with (s + t) mod M == f -- against the 64-bit remainder and against tile_index,
//       the function the walk goes the other way with -- for every weight f of the small tables and a seeded sample of the large
//       ones, the wrap-around case f < t and the edges f = 0, t - 1, t, M - 1 always included;
//   (2) a mask marked through (word, shift) in a table of 32-bit words is read back at [s] of the same memory seen as 16-bit
//       masks (what the learn kernel loads), touches no neighbour and stays inside fold_mask_words(M) words -- even and odd s,
//       and the last s of a table of odd length.
//   g++ -std=c++17 -O1 -Itests/host_env/shim -o fold_mask tests/host_env/fold_mask.cpp && ./fold_mask
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../../rl_markets_amd/csrc/lob_tiles.h"

static std::mt19937_64 rng(20260819);
static long bad = 0;

static void check_sum(uint32_t M, uint32_t f, uint32_t t) {
    const uint32_t s = fold_sum(f, t, M);
    const bool ok = s < M && (uint32_t)(((uint64_t)s + t) % M) == f && (uint32_t)tile_index(s, t, M) == f;
    if (!ok && bad++ < 10) printf("fold_sum: M %u f %u t %u -> s %u\n", M, f, t, s);
}

static void check_mask(uint32_t M, uint32_t s, int a) {
    const size_t words = fold_mask_words(M);
    std::vector<uint32_t> tab(words + 2, 0u);   // (two guard words behind the table)
    const size_t w = fold_mask_word(s);
    const uint32_t sh = fold_mask_shift(s);
    bool ok = w < words && (sh == 0 || sh == 16);
    if (ok) {
        tab[w] |= (1u << a) << sh;
        uint16_t m16[2];
        memcpy(m16, &tab[w], 4);                // the two masks of the word, as the kernel's 16-bit load sees them
        ok = m16[s & 1] == (uint16_t)(1u << a) && m16[(s & 1) ^ 1] == 0 && 2 * w + (s & 1) == s;
        for (size_t i = 0; i < tab.size(); i++) ok = ok && (i == w || tab[i] == 0);
    }
    if (!ok && bad++ < 10) printf("mask: M %u s %u a %d -> word %zu shift %u of %zu\n", M, s, a, w, sh, words);
}

int main() {
    const uint32_t Ms[] = {61u, 4099u, 65536u, 20000000u};
    long n_wrap = 0, n = 0;
    for (uint32_t M : Ms) {
        uint32_t terms[18];
        for (int i = 0; i < 18; i++) terms[i] = (uint32_t)(rng() % M);
        terms[0] = 0; terms[1] = M - 1; terms[2] = 1;   // (the extreme terms too)
        for (int i = 0; i < 18; i++) {
            const uint32_t t = terms[i];
            const uint32_t edges[] = {0u, t ? t - 1 : 0u, t, t + 1 < M ? t + 1 : M - 1, M - 1, M / 2};
            for (uint32_t f : edges) { check_sum(M, f, t); n++; n_wrap += f < t; }
            if (M <= 65536u) {
                for (uint32_t f = 0; f < M; f++) { check_sum(M, f, t); n++; n_wrap += f < t; }
            } else {
                for (int k = 0; k < 200000; k++) { const uint32_t f = (uint32_t)(rng() % M); check_sum(M, f, t); n++; n_wrap += f < t; }
            }
        }
        // even and odd sums, the table's first and last ones, every action bit
        const uint32_t sums[] = {0u, 1u, 2u, 3u, M / 2, M / 2 + 1, M - 3, M - 2, M - 1};
        for (uint32_t s : sums)
            for (int a = 0; a < 9; a++) check_mask(M, s, a);
        for (int k = 0; k < 2000; k++) check_mask(M, (uint32_t)(rng() % M), (int)(rng() % 9));
        if (fold_mask_words(M) != ((size_t)M + 1) / 2 && bad++ < 10) printf("fold_mask_words(%u)\n", M);
    }
    if (n_wrap == 0) { printf("no wrap-around case was tried\n"); bad++; }
    printf("%ld sums (%ld with f < t), bad %ld\n", n, n_wrap, bad);
    if (bad) return 1;
    printf("fold_mask OK\n");
    return 0;
}
