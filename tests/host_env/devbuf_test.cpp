// The engine's two device-buffer owners (rl_markets_amd/csrc/lob_devbuf.h) over an allocator that counts its live blocks and can be
// told to fail its k-th allocation.  Built with -fsanitize=address,undefined and run on its own (tests/test_host_env_diff.py): the
// blocks are real heap blocks, so a double free or a use of a released buffer is the sanitizer's to report, beside the counts.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>

#include "../../rl_markets_amd/csrc/lob_devbuf.h"

struct FakeAlloc {
    static std::set<void*> live;
    static int allocs, frees, fail_at;   // fail_at: the allocation (counted from 1 since arm()) that fails; 0: none
    static void arm(int k) { allocs = frees = 0; fail_at = k; }
    static int alloc(void** p, size_t bytes) {
        if (++allocs == fail_at) return 1;
        *p = malloc(bytes ? bytes : 1);
        live.insert(*p);
        return 0;
    }
    static void free(void* p) {
        frees++;
        if (!live.erase(p)) { printf("FAIL: free of a block that is not live\n"); exit(1); }
        ::free(p);
    }
};
std::set<void*> FakeAlloc::live;
int FakeAlloc::allocs = 0, FakeAlloc::frees = 0, FakeAlloc::fail_at = 0;

typedef lob::GrowBuf<double, FakeAlloc> Buf;
typedef lob::ScopedBuf<double, FakeAlloc> Tmp;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

// the shape of features_impl: up to three temporaries, the first failure returns at once
static int three(int want) {
    Tmp a, b, c;
    if (a.alloc(8) || (want > 1 && b.alloc(16)) || (want > 2 && c.alloc(4))) return LOB_ENOMEM;
    memset(a.p, 0, 8 * sizeof(double));
    if (want > 1) memset(b.p, 0, 16 * sizeof(double));
    if (want > 2) memset(c.p, 0, 4 * sizeof(double));
    return LOB_OK;
}
static int early_exit(bool leave) {
    Tmp t;
    if (t.alloc(32)) return LOB_ENOMEM;
    if (leave) return LOB_EHIP;   // (a failed copy behind the allocation)
    t.p[31] = 1.0;
    return LOB_OK;
}

int main() {
    {
        Buf b;
        FakeAlloc::arm(0);
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.reserve(0) == LOB_OK && FakeAlloc::allocs == 0);          // nothing needed: nothing done
        CHECK(b.reserve(10) == LOB_OK && b.p && b.cap == 10 && FakeAlloc::allocs == 1 && FakeAlloc::live.size() == 1);
        b.p[9] = 1.0;
        double* const first = b.p;
        // need <= cap: no allocator call, the buffer untouched
        CHECK(b.reserve(10) == LOB_OK && b.reserve(3) == LOB_OK && b.reserve(0) == LOB_OK);
        CHECK(b.p == first && b.cap == 10 && FakeAlloc::allocs == 1 && FakeAlloc::frees == 0 && b.p[9] == 1.0);
        // a growth that succeeds: the old block freed once, the new one of the new size
        CHECK(b.reserve(11) == LOB_OK && b.cap == 11 && FakeAlloc::allocs == 2 && FakeAlloc::frees == 1 && FakeAlloc::live.size() == 1);
        b.p[10] = 2.0;
        // a growth that fails: the old block is gone, pointer and capacity are null and 0
        FakeAlloc::arm(1);
        CHECK(b.reserve(100) == LOB_ENOMEM);
        CHECK(b.p == nullptr && b.cap == 0 && FakeAlloc::frees == 1 && FakeAlloc::live.empty());
        // ... so even a need the old buffer would have served allocates, and the same need again succeeds
        FakeAlloc::arm(0);
        CHECK(b.reserve(100) == LOB_OK && b.p && b.cap == 100 && FakeAlloc::allocs == 1 && FakeAlloc::live.size() == 1);
        b.p[99] = 3.0;
        // release after a failed growth frees nothing twice (the allocator exits on a block that is not live)
        FakeAlloc::arm(1);
        CHECK(b.reserve(200) == LOB_ENOMEM && FakeAlloc::frees == 1);
        b.release();
        b.release();
        CHECK(FakeAlloc::frees == 1 && b.p == nullptr && b.cap == 0 && FakeAlloc::live.empty());
        // a first allocation that fails, then a retry
        Buf c;
        FakeAlloc::arm(1);
        CHECK(c.reserve(5) == LOB_ENOMEM && c.p == nullptr && c.cap == 0 && FakeAlloc::frees == 0);
        CHECK(c.reserve(5) == LOB_OK && c.cap == 5 && FakeAlloc::live.size() == 1);
        c.release();
        CHECK(FakeAlloc::live.empty());
    }
    // the scoped temporary: zero live blocks behind every way out
    for (int want = 1; want <= 3; want++)
        for (int fail = 0; fail <= want; fail++) {   // fail 0: none; 2 of 3: "the second of three allocations fails"
            FakeAlloc::arm(fail);
            const int rc = three(want);
            CHECK(rc == (fail ? LOB_ENOMEM : LOB_OK));
            CHECK(FakeAlloc::allocs == (fail ? fail : want));   // nothing is tried behind the first failure
            CHECK(FakeAlloc::frees == (fail ? fail - 1 : want));
            CHECK(FakeAlloc::live.empty());
        }
    FakeAlloc::arm(0);
    CHECK(early_exit(true) == LOB_EHIP && FakeAlloc::live.empty() && FakeAlloc::frees == 1);
    CHECK(early_exit(false) == LOB_OK && FakeAlloc::live.empty() && FakeAlloc::frees == 2);
    FakeAlloc::arm(1);
    CHECK(early_exit(false) == LOB_ENOMEM && FakeAlloc::live.empty() && FakeAlloc::frees == 0);
    CHECK(FakeAlloc::live.empty());
    printf("devbuf_test OK\n");
    return 0;
}
