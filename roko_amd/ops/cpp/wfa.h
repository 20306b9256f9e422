#pragma once
#include <cstdint>
#include <string>

#include "align.h"

namespace rk {

// Exact unit-cost global alignment by diagonal transition; the contract
// (candidate order, tie rule, traceback) is roko_amd/wfa.py. Returns the op
// string: one byte of {X, D, I} per edit, in forward order. max_score < 0
// means no bound; a distance above it throws std::runtime_error.
std::string wfa_ops(const std::string& query, const std::string& target,
                    int64_t max_score = -1);

// Replays an op string from (0, 0) with greedy extension. Throws
// std::invalid_argument when an op is not legal where it stands or the walk
// does not end on (n, m). `cigar` receives the M/I/D run-length path in the
// align_stats convention.
AlignStats replay_ops(const std::string& query, const std::string& target,
                      const std::string& ops, std::string* cigar = nullptr);

}  // namespace rk
