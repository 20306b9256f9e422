// Exact unit-cost global alignment by diagonal transition (wavefront): the
// C++ route of roko_amd/wfa.py, which holds the contract. O(n + s^2) time for
// edit distance s, no band. Offsets are int32; the direction table is one
// byte per (score, diagonal) and is kept for the traceback, so memory is
// about s^2 bytes.

#include "wfa.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

namespace rk {

namespace {

constexpr int32_t NEG = -(1 << 30);

// length of the common prefix of q[i..n) and t[j..m), 8 bytes at a time
inline int64_t match_run(const uint8_t* q, const uint8_t* t, int64_t i,
                         int64_t j, int64_t n, int64_t m) {
    const int64_t lim = std::min(n - i, m - j);
    int64_t r = 0;
    while (r + 8 <= lim) {
        uint64_t a, b;
        std::memcpy(&a, q + i + r, 8);
        std::memcpy(&b, t + j + r, 8);
        const uint64_t x = a ^ b;
        if (x) return r + (__builtin_ctzll(x) >> 3);  // little endian
        r += 8;
    }
    while (r < lim && q[i + r] == t[j + r]) ++r;
    return r;
}

}  // namespace

std::string wfa_ops(const std::string& query, const std::string& target,
                    int64_t max_score) {
    const int64_t n = int64_t(query.size()), m = int64_t(target.size());
    if (n + m + 3 >= (int64_t(1) << 31))
        throw std::runtime_error("wfa_ops: sequences too long for int32 offsets");
    const uint8_t* q = reinterpret_cast<const uint8_t*>(query.data());
    const uint8_t* t = reinterpret_cast<const uint8_t*>(target.data());

    // offsets indexed by k + n + 1 over [-n-1, m+1]; a step writes every
    // diagonal of its range, so what lies outside the previous range is
    // still NEG
    std::vector<int32_t> prev(size_t(n + m + 3), NEG), cur(size_t(n + m + 3), NEG);
    std::vector<std::unique_ptr<uint8_t[]>> dirs;  // dirs[s][k - lo(s)]
    dirs.emplace_back();                           // score 0 has no direction

    prev[size_t(n + 1)] = int32_t(match_run(q, t, 0, 0, n, m));
    int64_t s = 0;
    while (prev[size_t(m + 1)] != m) {  // diagonal m - n
        ++s;
        if (max_score >= 0 && s > max_score)
            throw std::runtime_error("wfa_ops: edit distance exceeds max_score");
        const int64_t lo = std::max(-s, -n), hi = std::min(s, m);
        std::unique_ptr<uint8_t[]> dir(new uint8_t[size_t(hi - lo + 1)]);
        for (int64_t k = lo; k <= hi; ++k) {
            const size_t b = size_t(k + n + 1);
            const int32_t fx = prev[b], fd = prev[b - 1], fi = prev[b + 1];
            int64_t j = NEG;
            uint8_t d = 0;
            if (fx >= 0 && fx + 1 <= m && fx + 1 - k <= n) { j = fx + 1; d = 'X'; }
            if (fd >= 0 && fd + 1 <= m && fd + 1 > j) { j = fd + 1; d = 'D'; }
            if (fi >= 0 && fi - k <= n && fi > j) { j = fi; d = 'I'; }
            if (d) j += match_run(q, t, j - k, j, n, m);
            cur[b] = int32_t(j);
            dir[size_t(k - lo)] = d;
        }
        dirs.push_back(std::move(dir));
        std::swap(prev, cur);
    }

    std::string ops(size_t(s), '?');
    int64_t k = m - n;
    for (int64_t r = s; r >= 1; --r) {
        const int64_t lo = std::max(-r, -n), hi = std::min(r, m);
        if (k < lo || k > hi)
            throw std::runtime_error("wfa_ops: traceback left the wavefront");
        const uint8_t d = dirs[size_t(r)][size_t(k - lo)];
        ops[size_t(r - 1)] = char(d);
        if (d == 'D') --k;
        else if (d == 'I') ++k;
        else if (d != 'X')
            throw std::runtime_error("wfa_ops: traceback hit an empty cell");
    }
    return ops;
}

AlignStats replay_ops(const std::string& query, const std::string& target,
                      const std::string& ops, std::string* cigar) {
    const int64_t n = int64_t(query.size()), m = int64_t(target.size());
    const uint8_t* q = reinterpret_cast<const uint8_t*>(query.data());
    const uint8_t* t = reinterpret_cast<const uint8_t*>(target.data());
    std::vector<std::pair<int64_t, char>> runs;
    auto push = [&](int64_t cnt, char op) {
        if (!cigar || cnt <= 0) return;
        if (!runs.empty() && runs.back().second == op) runs.back().first += cnt;
        else runs.emplace_back(cnt, op);
    };
    auto fail = [&](size_t pos, const char* why) {
        throw std::invalid_argument("replay_ops: op " + std::to_string(pos) +
                                    " " + why);
    };

    AlignStats st{};
    int64_t i = match_run(q, t, 0, 0, n, m), j = i;
    push(i, 'M');
    for (size_t p = 0; p < ops.size(); ++p) {
        switch (ops[p]) {
            case 'X':
                if (!(i < n && j < m && q[i] != t[j])) fail(p, "(X) is not legal");
                ++i; ++j; ++st.mismatches;
                push(1, 'M');
                break;
            case 'D':
                if (!(j < m)) fail(p, "(D) is not legal");
                ++j; ++st.deletions;
                push(1, 'D');
                break;
            case 'I':
                if (!(i < n)) fail(p, "(I) is not legal");
                ++i; ++st.insertions;
                push(1, 'I');
                break;
            default:
                fail(p, "is not one of X, D, I");
        }
        const int64_t r = match_run(q, t, i, j, n, m);
        push(r, 'M');
        i += r;
        j += r;
    }
    if (i != n || j != m)
        throw std::invalid_argument(
            "replay_ops: op string ends at (" + std::to_string(i) + ", " +
            std::to_string(j) + "), not (" + std::to_string(n) + ", " +
            std::to_string(m) + ")");
    st.edit_distance = st.mismatches + st.insertions + st.deletions;
    st.matches = n - st.mismatches - st.insertions;
    if (cigar) {
        cigar->clear();
        for (const auto& r : runs) {
            *cigar += std::to_string(r.first);
            *cigar += r.second;
        }
    }
    return st;
}

}  // namespace rk
