// Vote table formats and the per-slot readers shared by the kernels that
// read the tables (votes.hip: consensus; edits.hip: edit compaction).
//
// Count table: one uint32 per column slot, slot = pos * (MAX_INS + 1) + ins,
// holding five 4-bit class counters (class c in bits [4c, 4c+4)).
// Quality table `qsum`: one uint64 per slot, class k in the 12-bit field at
// bits [12k, 12k+12) holding the sum of that class's quarter-Phred units
// (head.hip) over the slot's votes.

#pragma once

#include <cstdint>

#include "common.h"

namespace rk {

constexpr int VOTE_CLASSES = 5;
constexpr int VOTE_INS_SLOTS = 4;  // MAX_INS + 1
constexpr uint32_t VOTE_ERR_RANGE = 1u;     // pos / ins / class out of range
constexpr uint32_t VOTE_ERR_OVERFLOW = 2u;  // a 4-bit counter was already 15

constexpr int QSUM_BITS = 12;
constexpr uint64_t QSUM_MASK = (1ull << QSUM_BITS) - 1;
constexpr uint32_t QUAL_UNITS_PER_Q = 4;
constexpr uint32_t QUAL_MAX = 60;
constexpr uint32_t NO_QUAL = 0xFFu;

// majority class of one packed slot; ties -> smallest class id (the strict
// '>' keeps the first maximum, as numpy's argmax does); no votes -> 0xFF
RK_DEV uint32_t vote_majority(uint32_t v) {
    if (v == 0u) return 0xFFu;
    uint32_t best = 0, bc = v & 15u;
#pragma unroll
    for (uint32_t c = 1; c < VOTE_CLASSES; ++c) {
        const uint32_t n = (v >> (4 * c)) & 15u;
        if (n > bc) { bc = n; best = c; }
    }
    return best;
}

// quality of one slot: the called class's mean Phred over ALL votes of the
// slot, Q = min(60, S_c / (4 n)); no votes -> NO_QUAL
RK_DEV uint32_t vote_quality(uint32_t v, unsigned long long q, uint32_t maj) {
    if (v == 0u) return NO_QUAL;
    uint32_t n = 0;
#pragma unroll
    for (uint32_t c = 0; c < VOTE_CLASSES; ++c) n += (v >> (4 * c)) & 15u;
    const uint32_t s = (uint32_t)((q >> (QSUM_BITS * maj)) & QSUM_MASK);
    const uint32_t ql = s / (QUAL_UNITS_PER_Q * n);
    return ql < QUAL_MAX ? ql : QUAL_MAX;
}

}  // namespace rk
