// The layout of a branch set (rl_markets_amd/csrc/lob_branch.h): branch_layout spells out every array the kernels address through
// BranchOff, branch_bytes is what the host allocates, branch_enomem_message what it says when that fails.  Built with
// -fsanitize=address,undefined and run on its own (tests/test_vec_branch_abi.py): every array is written, with a byte of its own, into a
// heap block of exactly the total size, so an array that reaches past the set is the sanitizer's to report, and one that overlaps
// another shows when the block is read back.
#include <hip/hip_runtime.h>   // (tests/host_env/shim: lob_state.h's __host__ __device__ as plain host code)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../rl_markets_amd/csrc/lob_branch.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { printf("FAIL %s:%d: %s (B %d N %d w %d %d)\n", __FILE__, __LINE__, #c, B, N, wu, wd); return 1; } \
    } while (0)

static int one(int B, int N, int wu, int wd) {
    lob::BranchLayout L;
    lob::branch_layout(B, N, wu, wd, L);
    const size_t Bpad = ((size_t)B + 63) / 64 * 64;
    CHECK(L.lanes == (size_t)N * Bpad && L.lanes % 64 == 0);
    CHECK(L.total == lob::branch_bytes(B, N, wu, wd));
    // the fixed part: the LOB_ENV_FIELDS, two windows' running state, the observation row; then 8 bytes per ring entry
    size_t env = 0;
    int n_env = 0;
#define X(t, n) env += sizeof(t); n_env++;
    LOB_ENV_FIELDS(X)
#undef X
    CHECK(branch_off().fixed == env + 2 * LOB_BR_WIN_BYTES + LOB_BR_OBS_BYTES);
    CHECK(L.total == L.lanes * (env + 2 * LOB_BR_WIN_BYTES + LOB_BR_OBS_BYTES + 8 * ((size_t)wu + (size_t)wd)));
    CHECK(L.n == n_env + 10 + 1 + (wu ? 1 : 0) + (wd ? 1 : 0) && L.n <= LOB_BR_MAX_ARR);
    unsigned char* blk = (unsigned char*)malloc(L.total);
    CHECK(blk != nullptr);
    memset(blk, 0, L.total);
    size_t sum = 0;
    for (int i = 0; i < L.n; i++) {
        const lob::BranchArr& a = L.arr[i];
        CHECK(a.off % 16 == 0 && a.bytes > 0 && a.off + a.bytes <= L.total);
        CHECK(i == 0 || a.off == L.arr[i - 1].off + L.arr[i - 1].bytes);   // address order, back to back
        for (size_t k = 0; k < a.bytes; k++) {
            if (blk[a.off + k] != 0) { printf("FAIL: array %s overlaps another (B %d N %d w %d %d)\n", a.name, B, N, wu, wd); free(blk); return 1; }
            blk[a.off + k] = (unsigned char)(i + 1);
        }
        sum += a.bytes;
    }
    for (size_t k = 0; k < L.total; k++)
        if (blk[k] == 0) { printf("FAIL: byte %zu belongs to no array (B %d N %d w %d %d)\n", k, B, N, wu, wd); free(blk); return 1; }
    free(blk);
    CHECK(sum == L.total && L.arr[0].off == 0);
    // the kernels' addresses: array `n` of LOB_ENV_FIELDS at lanes * BranchOff::n, the rings behind BranchOff::fixed
    constexpr BranchOff o = branch_off();
    int i = 0;
#define X(t, n) CHECK(L.arr[i].off == L.lanes * o.n && L.arr[i].bytes == L.lanes * sizeof(t) && strcmp(L.arr[i].name, #n) == 0); i++;
    LOB_ENV_FIELDS(X)
#undef X
    CHECK(L.arr[i].off == L.lanes * (o.win[0] + LOB_BR_WIN_CNT) && L.arr[i + 5].off == L.lanes * (o.win[1] + LOB_BR_WIN_CNT));
    CHECK(L.arr[i + 10].off == L.lanes * o.obs && L.arr[i + 10].bytes == L.lanes * 64);
    if (wu) CHECK(L.arr[i + 11].off == L.lanes * o.fixed && L.arr[i + 11].bytes == L.lanes * 8 * (size_t)wu);
    if (wd) CHECK(L.arr[L.n - 1].off == L.lanes * (o.fixed + 8 * (size_t)wu) && L.arr[L.n - 1].bytes == L.lanes * 8 * (size_t)wd);
    // the bytes the refusal quotes
    const std::string msg = lob::branch_enomem_message("lob_branch_fork", B, N, wu, wd);
    CHECK(msg.find("lob_branch_fork: ") == 0);
    const size_t at = msg.find('(');
    CHECK(at != std::string::npos && strtoull(msg.c_str() + at + 1, nullptr, 10) == (unsigned long long)L.total);
    CHECK(msg.find(" bytes", at) != std::string::npos);
    return 0;
}

int main() {
    const int Bs[3] = {1, 63, 65}, Ns[2] = {1, 64}, ws[3] = {0, 1, 8};
    for (int B : Bs)
        for (int N : Ns)
            for (int w : ws)
                if (one(B, N, w, w)) return 1;
    if (one(65, 9, 3, 8) || one(65, 9, 8, 3)) return 1;   // (the two windows need not be equally long)
    printf("branch_layout_test OK\n");
    return 0;
}
