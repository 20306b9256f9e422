// The per-slot rules of the stitch, shared by the kernels that walk a
// contig's vote tables against its draft (edits.hip: edit compaction;
// stitch.hip: the polished sequence). One thread takes one draft position,
// one 256-thread workgroup EDIT_TILE positions.

#pragma once

#include <cstdint>

#include "common.h"
#include "votes.h"

namespace rk {

constexpr int EDIT_TILE = 256;        // positions (threads) per workgroup
constexpr int EDIT_WAVES = EDIT_TILE / 64;
constexpr int EDIT_SCAN_THREADS = 1024;
constexpr uint32_t EDIT_GAP_CLASS = 4;
constexpr uint32_t EDIT_GAP_CHAR = '*';
constexpr uint32_t EDIT_BASE_CHARS = 0x54474341u;  // "ACGT", class c in byte c

RK_DEV uint32_t edit_base_char(uint32_t cls) {
    return (EDIT_BASE_CHARS >> (8 * cls)) & 0xFFu;
}

RK_DEV uint32_t edit_upper(uint32_t d) {
    return (d >= 'a' && d <= 'z') ? d - 32u : d;
}

// The 4 slots of one position -> bit k set when slot k is an edit; maj4 gets
// the four majorities, one per byte. `d` is the draft byte, uppercased.
RK_DEV uint32_t edit_mask(const uint4 v, uint32_t d, bool in_window,
                          uint32_t* maj4) {
    const uint32_t m0 = vote_majority(v.x), m1 = vote_majority(v.y),
                   m2 = vote_majority(v.z), m3 = vote_majority(v.w);
    *maj4 = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
    if (!in_window) return 0u;
    // ins == 0: not voted (0xFF), GAP, or a base other than the draft's
    const uint32_t e0 =
        (m0 >= EDIT_GAP_CLASS || edit_base_char(m0) != d) ? 1u : 0u;
    return e0 | (m1 < EDIT_GAP_CLASS ? 2u : 0u) |
           (m2 < EDIT_GAP_CLASS ? 4u : 0u) | (m3 < EDIT_GAP_CLASS ? 8u : 0u);
}

// Is position p inside the stitch window of `state`? first = s0 / 4 and
// last = (last voted slot) / 4; with no voted ins == 0 slot s0 is INT64_MAX
// and nothing is inside.
RK_DEV bool edit_in_window(int64_t p, int64_t n_pos, const long long* state) {
    const int64_t first = state[0] / VOTE_INS_SLOTS;
    const int64_t last = state[1] / VOTE_INS_SLOTS;
    return p < n_pos && p >= first && p <= last;
}

}  // namespace rk
