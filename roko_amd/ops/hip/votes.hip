// On-device majority vote (reference: inference.py:119-147 — the per-base
// Counter loop + most_common). Predictions never leave the GPU: every
// (window, column) adds one vote into a dense per-contig table, and the
// consensus is a per-slot argmax of which only one byte per slot is copied
// back (docs/KERNELS.md "Device votes").
//
// Table: one uint32 per column slot, slot = pos * (MAX_INS + 1) + ins, holding
// five 4-bit class counters (class c in bits [4c, 4c+4)). A column receives at
// most 6 votes from the extractor's window geometry, so 4 bits (max 15) hold
// it; a 16th vote for one class is detected through the atomic's return value
// and reported in err_flag, never silent.

#include <cstdint>

#include "api.h"
#include "common.h"
#include "votes.h"  // table formats, vote_majority, vote_quality

namespace rk {

// One thread per (window, column). Rows with pos < 0 are padding and do not
// vote. Integer adds commute, so the table is exact and reproducible whatever
// the order the slots' streams arrive in; relaxed agent-scope atomics are
// enough because the table is only read by a later kernel.
__global__ __launch_bounds__(256) void vote_scatter_kernel(
    const uint8_t* __restrict__ preds,  // (n_cols)
    const int2* __restrict__ positions, // (n_cols) {pos, ins}
    uint32_t* __restrict__ table,       // (n_slots)
    int64_t n_slots, uint32_t* __restrict__ err_flag, int n_cols) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cols) return;
    const int2 p = positions[i];
    if (p.x < 0) return;
    const uint32_t cls = preds[i];
    const int64_t slot = (int64_t)p.x * VOTE_INS_SLOTS + p.y;
    if (p.y < 0 || p.y >= VOTE_INS_SLOTS || slot >= n_slots ||
        cls >= VOTE_CLASSES) {
        __hip_atomic_fetch_or(err_flag, VOTE_ERR_RANGE, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const uint32_t old = __hip_atomic_fetch_add(
        &table[slot], 1u << (4 * cls), __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT);
    if (((old >> (4 * cls)) & 15u) == 15u)
        __hip_atomic_fetch_or(err_flag, VOTE_ERR_OVERFLOW, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
}

// One thread per 4 slots: one 16-byte load, one packed 4-byte store (a wave
// reads 1 KiB and writes 256 B, both contiguous). The last, partial group
// goes slot by slot.
__global__ __launch_bounds__(256) void vote_consensus_kernel(
    const uint32_t* __restrict__ table, int64_t n_slots,
    uint8_t* __restrict__ maj) {
    const int64_t s0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (s0 >= n_slots) return;
    if (s0 + 4 <= n_slots) {
        const uint4 v = *reinterpret_cast<const uint4*>(table + s0);
        const uint32_t out = vote_majority(v.x) | (vote_majority(v.y) << 8) |
                             (vote_majority(v.z) << 16) |
                             (vote_majority(v.w) << 24);
        *reinterpret_cast<uint32_t*>(maj + s0) = out;
    } else {
        for (int64_t s = s0; s < n_slots; ++s)
            maj[s] = (uint8_t)vote_majority(table[s]);
    }
}

// ---------------------------------------------------------------------------
// Quality: a second table `qsum`, one uint64 per slot, class k in the 12-bit
// field at bits [12k, 12k+12) holding the sum of that class's quarter-Phred
// units (head.hip) over the slot's votes. 16 votes x 255 = 4080 < 4096, so
// both the extractor's bound (6 votes) and the count table's (15 per class)
// fit; a field that would pass 4095 is seen in the atomic's return value and
// sets VOTE_ERR_OVERFLOW.
// (constants and the per-slot readers: votes.h)

// vote_scatter_kernel plus one 64-bit add of the five packed units: same
// guard, same padding rule, same relaxed agent-scope atomics.
__global__ __launch_bounds__(256) void vote_scatter_q_kernel(
    const uint8_t* __restrict__ preds,  // (n_cols)
    const uint8_t* __restrict__ units,  // (n_cols, 5)
    const int2* __restrict__ positions, // (n_cols) {pos, ins}
    uint32_t* __restrict__ table,       // (n_slots)
    unsigned long long* __restrict__ qsum,  // (n_slots)
    int64_t n_slots, uint32_t* __restrict__ err_flag, int n_cols) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cols) return;
    const int2 p = positions[i];
    if (p.x < 0) return;
    const uint32_t cls = preds[i];
    const int64_t slot = (int64_t)p.x * VOTE_INS_SLOTS + p.y;
    if (p.y < 0 || p.y >= VOTE_INS_SLOTS || slot >= n_slots ||
        cls >= VOTE_CLASSES) {
        __hip_atomic_fetch_or(err_flag, VOTE_ERR_RANGE, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const uint8_t* u = units + (size_t)i * VOTE_CLASSES;
    uint32_t uk[VOTE_CLASSES];
    unsigned long long packed = 0;
#pragma unroll
    for (int k = 0; k < VOTE_CLASSES; ++k) {
        uk[k] = u[k];
        packed |= (unsigned long long)uk[k] << (QSUM_BITS * k);
    }
    const uint32_t old = __hip_atomic_fetch_add(
        &table[slot], 1u << (4 * cls), __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long oldq = __hip_atomic_fetch_add(
        &qsum[slot], packed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool over = ((old >> (4 * cls)) & 15u) == 15u;
#pragma unroll
    for (int k = 0; k < VOTE_CLASSES; ++k)
        over |= ((oldq >> (QSUM_BITS * k)) & QSUM_MASK) + uk[k] > QSUM_MASK;
    if (over)
        __hip_atomic_fetch_or(err_flag, VOTE_ERR_OVERFLOW, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
}

// One thread per 4 slots: one 16-byte load of counts, two of qsum, packed
// 4-byte stores of maj and qual. The last, partial group goes slot by slot.
__global__ __launch_bounds__(256) void vote_consensus_q_kernel(
    const uint32_t* __restrict__ table,
    const unsigned long long* __restrict__ qsum, int64_t n_slots,
    uint8_t* __restrict__ maj, uint8_t* __restrict__ qual) {
    const int64_t s0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (s0 >= n_slots) return;
    if (s0 + 4 <= n_slots) {
        const uint4 v = *reinterpret_cast<const uint4*>(table + s0);
        const ulonglong2 qa = *reinterpret_cast<const ulonglong2*>(qsum + s0);
        const ulonglong2 qb =
            *reinterpret_cast<const ulonglong2*>(qsum + s0 + 2);
        const uint32_t m0 = vote_majority(v.x), m1 = vote_majority(v.y),
                       m2 = vote_majority(v.z), m3 = vote_majority(v.w);
        *reinterpret_cast<uint32_t*>(maj + s0) =
            m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
        *reinterpret_cast<uint32_t*>(qual + s0) =
            vote_quality(v.x, qa.x, m0) | (vote_quality(v.y, qa.y, m1) << 8) |
            (vote_quality(v.z, qb.x, m2) << 16) |
            (vote_quality(v.w, qb.y, m3) << 24);
    } else {
        for (int64_t s = s0; s < n_slots; ++s) {
            const uint32_t v = table[s], m = vote_majority(v);
            maj[s] = (uint8_t)m;
            qual[s] = (uint8_t)vote_quality(v, qsum[s], m);
        }
    }
}

void vote_scatter_q(const uint8_t* preds, const uint8_t* units,
                    const int32_t* positions, uint32_t* table, uint64_t* qsum,
                    int64_t n_slots, uint32_t* err_flag, int n_cols,
                    hipStream_t stream) {
    if (n_cols <= 0) return;
    hipLaunchKernelGGL(vote_scatter_q_kernel, dim3((n_cols + 255) / 256),
                       dim3(256), 0, stream, preds, units,
                       reinterpret_cast<const int2*>(positions), table,
                       reinterpret_cast<unsigned long long*>(qsum), n_slots,
                       err_flag, n_cols);
}

void vote_consensus_q(const uint32_t* table, const uint64_t* qsum,
                      int64_t n_slots, uint8_t* maj, uint8_t* qual,
                      hipStream_t stream) {
    if (n_slots <= 0) return;
    const int64_t groups = (n_slots + 3) / 4;
    hipLaunchKernelGGL(vote_consensus_q_kernel,
                       dim3((unsigned)((groups + 255) / 256)), dim3(256), 0,
                       stream, table,
                       reinterpret_cast<const unsigned long long*>(qsum),
                       n_slots, maj, qual);
}

void vote_scatter(const uint8_t* preds, const int32_t* positions,
                  uint32_t* table, int64_t n_slots, uint32_t* err_flag,
                  int n_cols, hipStream_t stream) {
    if (n_cols <= 0) return;
    hipLaunchKernelGGL(vote_scatter_kernel, dim3((n_cols + 255) / 256),
                       dim3(256), 0, stream, preds,
                       reinterpret_cast<const int2*>(positions), table,
                       n_slots, err_flag, n_cols);
}

void vote_consensus(const uint32_t* table, int64_t n_slots, uint8_t* maj,
                    hipStream_t stream) {
    if (n_slots <= 0) return;
    const int64_t groups = (n_slots + 3) / 4;
    hipLaunchKernelGGL(vote_consensus_kernel,
                       dim3((unsigned)((groups + 255) / 256)), dim3(256), 0,
                       stream, table, n_slots, maj);
}

}  // namespace rk
