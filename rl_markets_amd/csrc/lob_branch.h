// The branch set of the vector-env interface (include/lob_engine.h lob_branch_*): where N private copies of every book's
// agent-side environment state lie in one device buffer.  Shared by the host side (lob_tu_host_vec.hip: size, allocation, the
// LOB_ENOMEM message), the kernels (lob_tu_branch.hip) and tests/host_env/branch_layout_test.cpp, which drives branch_layout on the CPU.
//   The set is field-major like the live state: every array has one element per LANE, lane = n * Bpad + b for branch n of book b,
// Bpad = the books rounded up to whole waves, so the 64 lanes of a wave (64 consecutive books of one branch) touch consecutive words
// of every array.  The arrays lie back to back in a fixed order, each `lanes` elements long: the place of an array is
// lanes * (the bytes per lane in front of it), a compile-time constant per array (BranchOff).  lanes is a multiple of 64, so every
// array starts at a multiple of 256 bytes and nothing but {base, lanes, ring lengths} travels to a kernel.
//   Order: the arrays of LOB_ENV_FIELDS; the running state of pnl_ups, then pnl_downs (cnt, head, sum, mean, s); the observation of the
// last completed step, [lanes][16] f32 (a lane's row is 64 contiguous bytes, as slot 2 of DevState::vars); then -- only when the reward
// reads the windows (LOB_REWARD_NORMED) -- the two rings, [w_up][lanes] and [w_dn][lanes] f64, the live ring layout over lanes.
#ifndef LOB_BRANCH_H
#define LOB_BRANCH_H

#include <stddef.h>

#include <string>

#include "lob_state.h"

struct BranchSet {
    char* base;
    u64 lanes;        // n_branches * Bpad
    i32 w_up, w_dn;   // entries of the two rings held behind the fixed part (0, 0: no rings)
};

// bytes per lane in front of each array
struct BranchOff {
#define X(t, n) uint32_t n;
    LOB_ENV_FIELDS(X)
#undef X
    uint32_t win[2];   // pnl_ups, pnl_downs: cnt + 0, head + 4, sum + 8, mean + 16, s + 24 (times lanes)
    uint32_t obs;
    uint32_t fixed;    // ... in front of the rings: the bytes per lane of a set without them
};
#define LOB_BR_WIN_CNT 0
#define LOB_BR_WIN_HEAD 4
#define LOB_BR_WIN_SUM 8
#define LOB_BR_WIN_MEAN 16
#define LOB_BR_WIN_S 24
#define LOB_BR_WIN_BYTES 32
#define LOB_BR_OBS_BYTES 64
constexpr BranchOff branch_off() {
    BranchOff o{};
    uint32_t at = 0;
#define X(t, n) o.n = at; at += (uint32_t)sizeof(t);
    LOB_ENV_FIELDS(X)
#undef X
    o.win[0] = at; at += LOB_BR_WIN_BYTES;
    o.win[1] = at; at += LOB_BR_WIN_BYTES;
    o.obs = at; at += LOB_BR_OBS_BYTES;
    o.fixed = at;
    return o;
}

namespace lob {

// One array of the set as the host sees it: its place and size in bytes
struct BranchArr {
    const char* name;
    size_t off, bytes;
};
#define LOB_BR_MAX_ARR 96
struct BranchLayout {
    size_t lanes, total;
    int n;
    BranchArr arr[LOB_BR_MAX_ARR];
};
inline size_t branch_lanes(int B, int n_branches) { return (size_t)n_branches * (((size_t)B + 63) / 64 * 64); }
// the whole set in bytes; w_up / w_dn: the ring lengths, 0 without rings
inline size_t branch_bytes(int B, int n_branches, int w_up, int w_dn) {
    return branch_lanes(B, n_branches) * ((size_t)branch_off().fixed + 8 * ((size_t)w_up + (size_t)w_dn));
}
// every array of the set, in address order -- what the kernels compute from BranchOff, spelled out
inline void branch_layout(int B, int n_branches, int w_up, int w_dn, BranchLayout& L) {
    constexpr BranchOff o = branch_off();
    L.lanes = branch_lanes(B, n_branches);
    L.n = 0;
    auto add = [&](const char* name, size_t per_lane_before, size_t width) {
        L.arr[L.n++] = BranchArr{name, L.lanes * per_lane_before, L.lanes * width};
    };
#define X(t, n) add(#n, o.n, sizeof(t));
    LOB_ENV_FIELDS(X)
#undef X
    static const char* const wn[2][5] = {{"pnl_ups.cnt", "pnl_ups.head", "pnl_ups.sum", "pnl_ups.mean", "pnl_ups.s"},
                                         {"pnl_downs.cnt", "pnl_downs.head", "pnl_downs.sum", "pnl_downs.mean", "pnl_downs.s"}};
    for (int k = 0; k < 2; k++) {
        add(wn[k][0], o.win[k] + LOB_BR_WIN_CNT, 4); add(wn[k][1], o.win[k] + LOB_BR_WIN_HEAD, 4); add(wn[k][2], o.win[k] + LOB_BR_WIN_SUM, 8);
        add(wn[k][3], o.win[k] + LOB_BR_WIN_MEAN, 8); add(wn[k][4], o.win[k] + LOB_BR_WIN_S, 8);
    }
    add("obs", o.obs, LOB_BR_OBS_BYTES);
    if (w_up) add("pnl_ups.ring", o.fixed, 8 * (size_t)w_up);
    if (w_dn) add("pnl_downs.ring", o.fixed + 8 * (size_t)w_up, 8 * (size_t)w_dn);
    L.total = branch_bytes(B, n_branches, w_up, w_dn);
}
// the refusal of a set that does not fit
inline std::string branch_enomem_message(const char* who, int B, int n_branches, int w_up, int w_dn) {
    return std::string(who) + ": no room for the branch set (" + std::to_string(branch_bytes(B, n_branches, w_up, w_dn)) + " bytes for " +
           std::to_string(n_branches) + " branches of " + std::to_string(B) + " books; fewer branches per set)";
}

}  // namespace lob

#endif
