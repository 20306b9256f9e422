// Exact edit-distance alignment by diagonal transition (wavefront) on the
// device; the contract (candidates, tie rule, traceback) is roko_amd/wfa.py
// and the C++ route is ops/cpp/wfa.cpp. The op string must equal theirs byte
// for byte.
//
// Sequences: uint8, each followed by WFA_PAD bytes of a pad value that occurs
// in neither input (the Python entry admits printable ASCII only) and differs
// between query and target. A match run therefore ends at a sequence end by
// the byte comparison alone; every load is guarded against the allocation
// (len + WFA_PAD) all the same, and the run is clamped to n and m.
//
// Offsets: two int32 rows of n + m + 3 words, indexed by k + n + 1 over
// [-n-1, m+1], filled with WFA_NEG once by the caller. Score s reads row
// (s-1)&1 and writes every diagonal of its range into row s&1 (WFA_NEG where
// no candidate is valid), so stale words are always overwritten and a
// neighbour outside the previous range still reads WFA_NEG.
//
// wfa_step_kernel: one launch per score, one diagonal per thread.
//   a. candidate selection as in the contract
//   b. per-lane probe: WFA_PROBE bytes, alone, in one batch of loads
//   c. wave-cooperative extension of the runs still open: for each such lane
//      in turn its (i, j) is broadcast and all 64 lanes compare WFA_COOP
//      consecutive bytes a round (four byte stripes, loads independent of each
//      other), ballot the first difference and go on until the run ends.
//      Without this the lane on the optimal diagonal walks ~n/s bases alone
//      while 63 lanes idle.
//   d. offset and direction stores; the owner of diagonal m - n stores s into
//      `done` when it reaches m. Every later launch returns at once.
//
// wfa_trace_kernel: one lane walks a chunk's direction table from its last
// score to its first, carrying the diagonal in device memory between chunks.

#include <cstdint>

#include "api.h"
#include "common.h"

namespace rk {

constexpr int WFA_THREADS = 256;
constexpr int WFA_PROBE = 8;
constexpr int WFA_STRIPES = 4;
constexpr int WFA_COOP = 64 * WFA_STRIPES;
constexpr int WFA_PAD = WFA_COOP;
constexpr int WFA_NEG = -(1 << 30);

int wfa_probe() { return WFA_PROBE; }
int wfa_coop() { return WFA_COOP; }
int wfa_pad() { return WFA_PAD; }

static int64_t wfa_sum_min(int64_t s, int64_t a) {  // sum of min(r, a), r < s
    if (s <= 0) return 0;
    if (s - 1 <= a) return s * (s - 1) / 2;
    return a * (a + 1) / 2 + (s - 1 - a) * a;
}

int64_t wfa_dir_cells(int64_t n, int64_t m, int64_t s0, int64_t s1) {
    if (s1 <= s0) return 0;
    return wfa_sum_min(s1, m) - wfa_sum_min(s0, m) + wfa_sum_min(s1, n) -
           wfa_sum_min(s0, n) + (s1 - s0);
}

__global__ __launch_bounds__(WFA_THREADS) void wfa_step_kernel(
    const uint8_t* __restrict__ q, const uint8_t* __restrict__ t, int n, int m,
    int s, const int* __restrict__ prev, int* __restrict__ cur,
    uint8_t* __restrict__ dir, int* done) {
    if (__builtin_amdgcn_readfirstlane(*done) >= 0) return;  // wave-uniform

    const int lo = s < n ? -s : -n, hi = s < m ? s : m;
    const int64_t gid = (int64_t)blockIdx.x * WFA_THREADS + threadIdx.x;
    const bool active = gid <= (int64_t)hi - lo;
    const int k = active ? lo + (int)gid : 0;
    const int lane = threadIdx.x & 63;

    // a. candidates: X, D, I; a later kind wins only with a greater offset
    int j = WFA_NEG;
    uint32_t d = 0;
    if (active) {
        if (s == 0) {
            j = 0;
        } else {
            const int64_t b = (int64_t)k + n + 1;
            const int fx = prev[b], fd = prev[b - 1], fi = prev[b + 1];
            if (fx >= 0 && fx + 1 <= m && fx + 1 - k <= n) { j = fx + 1; d = 'X'; }
            if (fd >= 0 && fd + 1 <= m && fd + 1 > j) { j = fd + 1; d = 'D'; }
            if (fi >= 0 && fi - k <= n && fi > j) { j = fi; d = 'I'; }
        }
    }
    int i = j >= 0 ? j - k : 0;
    const int64_t q_end = (int64_t)n + WFA_PAD, t_end = (int64_t)m + WFA_PAD;

    // b. probe: WFA_PROBE byte pairs loaded at once (i + r <= n + WFA_PROBE
    // lies inside the pad), the pads end the run at a sequence end
    bool open = false;
    if (j >= 0) {
        uint32_t neq = 0;
#pragma unroll
        for (int r = 0; r < WFA_PROBE; ++r) {
            const uint32_t a = (int64_t)i + r < q_end ? q[i + r] : 0u;
            const uint32_t b = (int64_t)j + r < t_end ? t[j + r] : 1u;
            neq |= (a != b ? 1u : 0u) << r;
        }
        int r = neq ? __ffs((int)neq) - 1 : WFA_PROBE;
        r = min(r, min(n - i, m - j));
        i += r;
        j += r;
        open = r == WFA_PROBE;
    }

    // c. the wave extends its open runs together, one after the other
    unsigned long long todo = __ballot(open);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int ci = __shfl(i, src), cj = __shfl(j, src);
        int run = 0;
        for (;;) {
            unsigned long long diff[WFA_STRIPES];
#pragma unroll
            for (int u = 0; u < WFA_STRIPES; ++u) {
                const int64_t qi = (int64_t)ci + run + u * 64 + lane;
                const int64_t tj = (int64_t)cj + run + u * 64 + lane;
                const uint32_t a = qi < q_end ? q[qi] : 0u;
                const uint32_t b = tj < t_end ? t[tj] : 1u;
                diff[u] = __ballot(a != b);
            }
            int first = WFA_COOP;
#pragma unroll
            for (int u = WFA_STRIPES - 1; u >= 0; --u)
                if (diff[u]) first = u * 64 + __ffsll((long long)diff[u]) - 1;
            run += first;
            // a full round means both sequences still had WFA_COOP bytes
            if (first < WFA_COOP || run >= n - ci || run >= m - cj) break;
        }
        run = min(run, min(n - ci, m - cj));
        if (lane == src) {
            i += run;
            j += run;
        }
    }

    // d. stores
    if (active) {
        cur[(int64_t)k + n + 1] = j;
        dir[gid] = (uint8_t)d;
        if (k == m - n && j == m) *done = s;
    }
}

// walk[0]: the diagonal at score s_hi on entry, at score max(s0, 1) - 1 on
// exit; walk[1]: set when the walk meets an empty cell or leaves the range.
// dir holds scores [s0, ...); `off_hi` is the offset of score s_hi in it.
__global__ void wfa_trace_kernel(const uint8_t* __restrict__ dir, int n, int m,
                                 int s0, int s_hi, int64_t off_hi, int* walk,
                                 uint8_t* __restrict__ ops) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (walk[1]) return;
    int k = walk[0];
    int64_t off = off_hi;
    const int s_lo = s0 > 1 ? s0 : 1;
    for (int s = s_hi; s >= s_lo; --s) {
        const int lo = s < n ? -s : -n, hi = s < m ? s : m;
        if (k < lo || k > hi) { walk[1] = 1; return; }
        const uint32_t d = dir[off + (k - lo)];
        ops[s - 1] = (uint8_t)d;
        if (d == 'D') --k;
        else if (d == 'I') ++k;
        else if (d != 'X') { walk[1] = 1; return; }
        // width of score s - 1
        const int p = s - 1;
        off -= (int64_t)(p < m ? p : m) + (p < n ? p : n) + 1;
    }
    walk[0] = k;
}

// Scores [s0, s1) of one chunk, one launch each. `offs` is the two offset
// rows back to back, `dir` the chunk's table (wfa_dir_cells entries).
void wfa_steps(const uint8_t* q, const uint8_t* t, int n, int m, int s0,
               int s1, int* offs, uint8_t* dir, int* done,
               hipStream_t stream) {
    const int64_t row = (int64_t)n + m + 3;
    int64_t off = 0;
    for (int s = s0; s < s1; ++s) {
        const int64_t width = (int64_t)(s < m ? s : m) + (s < n ? s : n) + 1;
        const unsigned blocks =
            (unsigned)((width + WFA_THREADS - 1) / WFA_THREADS);
        hipLaunchKernelGGL(wfa_step_kernel, dim3(blocks), dim3(WFA_THREADS),
                           0, stream, q, t, n, m, s,
                           offs + ((s - 1) & 1) * row, offs + (s & 1) * row,
                           dir + off, done);
        off += width;
    }
}

void wfa_trace(const uint8_t* dir, int n, int m, int s0, int s_hi, int* walk,
               uint8_t* ops, hipStream_t stream) {
    hipLaunchKernelGGL(wfa_trace_kernel, dim3(1), dim3(64), 0, stream, dir, n,
                       m, s0, s_hi, wfa_dir_cells(n, m, s0, s_hi), walk, ops);
}

}  // namespace rk
