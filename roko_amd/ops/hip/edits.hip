// Polishing edits compacted on the device (contract: roko_amd/edits.py).
// From a contig's vote tables and its draft bytes the kernels return only the
// slots at which the polished sequence differs from the draft, in slot order;
// the dense majority and quality arrays are never written to memory.
//
// One thread takes one draft position: its 4 slots are one 16-byte load of
// the count table (as in vote_consensus_q_kernel) and yield 0..4 edits. One
// 256-thread workgroup covers EDIT_TILE = 256 positions. Four kernels, ordered
// by kernel boundaries on one stream, no workgroup ever waits on another:
//
//   edit_bounds_kernel  first voted ins == 0 slot and last voted slot, one
//                       64-bit min and one max atomic per workgroup of a
//                       capped grid that strides over the tiles
//   edit_count_kernel   edits per workgroup (needs the bounds: an unvoted
//                       position is an edit only inside the stitch window)
//   edit_scan_kernel    exclusive scan of the workgroup counts in place, one
//                       workgroup looping over them; total into state[2]
//   edit_write_kernel   every workgroup writes its records at its offset; the
//                       placement inside it is an ordered prefix over the
//                       per-thread counts (wave64 shuffle scan + wave totals
//                       in LDS), no atomics, so the order is slot order
//
// state: int64[3] = {s0, last voted slot, total}; the host sets it to
// {INT64_MAX, -1, 0} before the first kernel and reads it back in one copy
// before it sizes the record buffer.
//
// Record: 16 bytes, {int64 pos; uint8 ins, ref, alt, qual; 4 bytes zero}.

#include <cstdint>

#include "api.h"
#include "common.h"
#include "edits.h"
#include "votes.h"

namespace rk {

// the bounds kernel ends in two same-address atomics per workgroup, which
// the L2 serialises (measured ~12 ns each): a capped grid keeps that constant
constexpr unsigned EDIT_BOUNDS_BLOCKS = 512;

__global__ __launch_bounds__(EDIT_TILE) void edit_bounds_kernel(
    const uint32_t* __restrict__ table, int64_t n_pos,
    long long* __restrict__ state) {
    __shared__ long long lo_s[EDIT_WAVES], hi_s[EDIT_WAVES];
    long long lo = INT64_MAX, hi = -1;
    // the grid is capped (EDIT_BOUNDS_BLOCKS), a workgroup strides over the
    // tiles: positions ascend, so the first hit is lo and the last is hi
    for (int64_t p = (int64_t)blockIdx.x * EDIT_TILE + threadIdx.x; p < n_pos;
         p += (int64_t)gridDim.x * EDIT_TILE) {
        const int64_t s = p * VOTE_INS_SLOTS;
        const uint4 v = *reinterpret_cast<const uint4*>(table + s);
        if (v.x && lo == INT64_MAX) lo = s;
        if (v.x) hi = s;
        if (v.y) hi = s + 1;
        if (v.z) hi = s + 2;
        if (v.w) hi = s + 3;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { lo_s[wave] = lo; hi_s[wave] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < EDIT_WAVES; ++w) {
            lo = lo_s[w] < lo ? lo_s[w] : lo;
            hi = hi_s[w] > hi ? hi_s[w] : hi;
        }
        // relaxed agent scope: read by the next kernel only
        if (lo != INT64_MAX)
            __hip_atomic_fetch_min(&state[0], lo, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        if (hi >= 0)
            __hip_atomic_fetch_max(&state[1], hi, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(EDIT_TILE) void edit_count_kernel(
    const uint32_t* __restrict__ table, const uint8_t* __restrict__ draft,
    int64_t n_pos, const long long* __restrict__ state,
    long long* __restrict__ counts) {
    __shared__ uint32_t tot_s[EDIT_WAVES];
    const int64_t p = (int64_t)blockIdx.x * EDIT_TILE + threadIdx.x;
    uint32_t n = 0;
    if (edit_in_window(p, n_pos, state)) {
        const uint4 v =
            *reinterpret_cast<const uint4*>(table + p * VOTE_INS_SLOTS);
        uint32_t maj4;
        n = __popc(edit_mask(v, edit_upper(draft[p]), true, &maj4));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) tot_s[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < EDIT_WAVES; ++w) n += tot_s[w];
        counts[blockIdx.x] = n;
    }
}

// One workgroup: counts[0..n) -> exclusive prefix in place, EDIT_SCAN_THREADS
// at a pass with the running total carried in a register; state[2] = total.
__global__ __launch_bounds__(EDIT_SCAN_THREADS) void edit_scan_kernel(
    long long* __restrict__ counts, int64_t n, long long* __restrict__ state) {
    constexpr int WAVES = EDIT_SCAN_THREADS / 64;
    __shared__ long long tot_s[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (int64_t base = 0; base < n; base += EDIT_SCAN_THREADS) {
        const int64_t i = base + threadIdx.x;
        const long long own = i < n ? counts[i] : 0;
        long long x = own;  // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) tot_s[wave] = x;
        __syncthreads();
        long long before = 0, pass = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const long long t = tot_s[w];
            if (w < wave) before += t;
            pass += t;
        }
        if (i < n) counts[i] = carry + before + x - own;
        carry += pass;
        __syncthreads();  // tot_s is rewritten by the next pass
    }
    if (threadIdx.x == 0) state[2] = carry;
}

__global__ __launch_bounds__(EDIT_TILE) void edit_write_kernel(
    const uint32_t* __restrict__ table,
    const unsigned long long* __restrict__ qsum,
    const uint8_t* __restrict__ draft, int64_t n_pos,
    const long long* __restrict__ state,
    const long long* __restrict__ offsets, ulonglong2* __restrict__ records,
    int64_t total) {
    __shared__ uint32_t tot_s[EDIT_WAVES];
    const int64_t p = (int64_t)blockIdx.x * EDIT_TILE + threadIdx.x;
    const bool in_window = edit_in_window(p, n_pos, state);
    uint4 v = make_uint4(0, 0, 0, 0);
    uint32_t d = 0, maj4 = 0, mask = 0;
    if (in_window) {
        v = *reinterpret_cast<const uint4*>(table + p * VOTE_INS_SLOTS);
        d = edit_upper(draft[p]);
        mask = edit_mask(v, d, true, &maj4);
    }
    const uint32_t own = __popc(mask);
    uint32_t x = own;  // inclusive scan inside the wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t y = __shfl_up(x, s);
        if (lane >= s) x += y;
    }
    if (lane == 63) tot_s[wave] = x;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < EDIT_WAVES; ++w)
        if (w < wave) before += tot_s[w];
    if (!mask) return;

    int64_t o = offsets[blockIdx.x] + before + x - own;
    const uint32_t vk[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!((mask >> k) & 1u)) continue;
        const uint32_t m = (maj4 >> (8 * k)) & 0xFFu;
        const uint32_t ref = k == 0 ? d : EDIT_GAP_CHAR;
        const uint32_t alt =
            m < EDIT_GAP_CLASS ? edit_base_char(m) : EDIT_GAP_CHAR;
        // an unvoted slot never reads qsum: vote_quality returns NO_QUAL
        const uint32_t q = vote_quality(
            vk[k], vk[k] ? qsum[p * VOTE_INS_SLOTS + k] : 0ull,
            m < VOTE_CLASSES ? m : 0u);
        if (o < total)  // holds by construction; a record never lands outside
            records[o] = make_ulonglong2(
                (unsigned long long)p,
                (unsigned long long)((uint32_t)k | (ref << 8) | (alt << 16) |
                                     (q << 24)));
        ++o;
    }
}

static unsigned edit_blocks(int64_t n_pos) {
    return (unsigned)((n_pos + EDIT_TILE - 1) / EDIT_TILE);
}

int64_t edit_num_blocks(int64_t n_pos) { return edit_blocks(n_pos); }

// state[0], state[1] = first voted ins == 0 slot, last voted slot
void edit_bounds(const uint32_t* table, int64_t n_pos, int64_t* state,
                 hipStream_t stream) {
    if (n_pos <= 0) return;
    const unsigned blocks = edit_blocks(n_pos);
    hipLaunchKernelGGL(
        edit_bounds_kernel,
        dim3(blocks < EDIT_BOUNDS_BLOCKS ? blocks : EDIT_BOUNDS_BLOCKS),
        dim3(EDIT_TILE), 0, stream, table, n_pos,
        reinterpret_cast<long long*>(state));
}

// counts[0..n) -> exclusive prefix in place; state[2] = their sum
void edit_scan(int64_t* counts, int64_t n, int64_t* state,
               hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(edit_scan_kernel, dim3(1), dim3(EDIT_SCAN_THREADS), 0,
                       stream, reinterpret_cast<long long*>(counts), n,
                       reinterpret_cast<long long*>(state));
}

// bounds, count and scan: fills state and turns counts (edit_num_blocks
// words) into the workgroups' record offsets
void edit_count(const uint32_t* table, const uint8_t* draft, int64_t n_pos,
                int64_t* state, int64_t* counts, hipStream_t stream) {
    if (n_pos <= 0) return;
    const unsigned blocks = edit_blocks(n_pos);
    edit_bounds(table, n_pos, state, stream);
    hipLaunchKernelGGL(edit_count_kernel, dim3(blocks), dim3(EDIT_TILE), 0,
                       stream, table, draft, n_pos,
                       reinterpret_cast<const long long*>(state),
                       reinterpret_cast<long long*>(counts));
    edit_scan(counts, (int64_t)blocks, state, stream);
}

void edit_write(const uint32_t* table, const uint64_t* qsum,
                const uint8_t* draft, int64_t n_pos, const int64_t* state,
                const int64_t* offsets, void* records, int64_t total,
                hipStream_t stream) {
    if (n_pos <= 0 || total <= 0) return;
    hipLaunchKernelGGL(edit_write_kernel, dim3(edit_blocks(n_pos)),
                       dim3(EDIT_TILE), 0, stream, table,
                       reinterpret_cast<const unsigned long long*>(qsum),
                       draft, n_pos,
                       reinterpret_cast<const long long*>(state),
                       reinterpret_cast<const long long*>(offsets),
                       reinterpret_cast<ulonglong2*>(records), total);
}

}  // namespace rk
