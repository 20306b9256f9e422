// The polished sequence and its quality string emitted on the device, under
// the quality filter (contract: roko_amd/stitch.py, stitch_filtered). From a
// contig's vote tables and its draft bytes the kernels write two compact byte
// arrays of exactly the polished length; the dense majority and quality
// arrays are never written to memory and only polished bytes go back to the
// host.
//
// The structure is that of edits.hip, whose bounds and scan kernels and
// per-slot helpers (edits.h) are used as they are. One thread takes one draft
// position: its 4 slots are one 16-byte load of the count table and emit 0..4
// bytes; outside the stitch window it emits exactly the draft byte. One
// 256-thread workgroup covers EDIT_TILE positions, so it writes at most 1024
// contiguous bytes, at an offset of any alignment. Kernels are ordered by
// kernel boundaries on one stream, no workgroup ever waits on another:
//
//   edit_bounds_kernel   (edits.hip) first voted ins == 0 slot, last voted slot
//   stitch_count_kernel  bytes per workgroup
//   edit_scan_kernel     (edits.hip) exclusive scan in place, total -> state[2]
//   stitch_write_kernel  every workgroup places its bytes in LDS by an ordered
//                        prefix over the per-thread counts (no atomics, so
//                        the order is slot order), then stores them at its
//                        offset: single bytes up to the first 4-byte boundary
//                        of the output, whole words from there, single bytes
//                        for what is left
//
// state: int64[3] = {s0, last voted slot, total} as in edits.hip.
//
// qsum is read only for a voted slot whose quality is needed: to judge an
// edit against min_qual > 0, or for the quality string of an emitted base.
// With qsum null min_qual is 0 and no quality is written.

#include <cstdint>

#include "api.h"
#include "common.h"
#include "edits.h"
#include "votes.h"

namespace rk {

constexpr uint32_t STITCH_PHRED_OFFSET = 33;  // FASTQ encoding
constexpr int STITCH_MAX_BYTES = EDIT_TILE * VOTE_INS_SLOTS;

// What position p emits: the return value is the number of bytes (0..4),
// byte i of *seq4 the i-th sequence byte and byte i of *q4 its quality.
// `judge_only` leaves the qualities of accepted bases unread (count kernel,
// or no quality string wanted).
RK_DEV uint32_t stitch_position(const uint32_t* __restrict__ table,
                                const unsigned long long* __restrict__ qsum,
                                const uint8_t* __restrict__ draft, int64_t p,
                                int64_t n_pos, const long long* state,
                                uint32_t min_qual, bool keep_uncovered,
                                bool judge_only, uint32_t* seq4,
                                uint32_t* q4) {
    *seq4 = 0u;
    *q4 = 0u;
    if (p >= n_pos) return 0u;
    const uint32_t raw = draft[p];
    if (!edit_in_window(p, n_pos, state)) {
        *seq4 = raw;  // prefix and suffix: the draft byte as it is, Q0
        return 1u;
    }
    const uint4 v = *reinterpret_cast<const uint4*>(table + p * VOTE_INS_SLOTS);
    uint32_t maj4;
    const uint32_t mask = edit_mask(v, edit_upper(raw), true, &maj4);
    const uint32_t vk[4] = {v.x, v.y, v.z, v.w};
    uint32_t n = 0, seq = 0, qs = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t m = (maj4 >> (8 * k)) & 0xFFu;
        const bool edit = (mask >> k) & 1u;
        if (k == 0 && vk[0] == 0u) {  // uncovered: min_qual does not apply
            if (keep_uncovered) seq |= raw << (8 * n++);
            continue;
        }
        if (k > 0 && !edit) continue;  // GAP or not voted
        // a voted slot: any class at ins == 0, a base at ins > 0
        const bool gap = m >= EDIT_GAP_CLASS;
        const bool judge = edit && min_qual > 0u;
        uint32_t q = 0;
        if (judge || (!judge_only && !gap))
            q = vote_quality(vk[k], qsum[p * VOTE_INS_SLOTS + k],
                             m < VOTE_CLASSES ? m : 0u);
        if (judge && q < min_qual) {
            // rejected: the draft base stays at Q0, an insertion vanishes
            if (k == 0) seq |= raw << (8 * n++);
            continue;
        }
        if (gap) continue;  // accepted deletion
        seq |= edit_base_char(m) << (8 * n);
        qs |= q << (8 * n);
        ++n;
    }
    *seq4 = seq;
    *q4 = qs;
    return n;
}

__global__ __launch_bounds__(EDIT_TILE) void stitch_count_kernel(
    const uint32_t* __restrict__ table,
    const unsigned long long* __restrict__ qsum,
    const uint8_t* __restrict__ draft, int64_t n_pos,
    const long long* __restrict__ state, uint32_t min_qual,
    uint32_t keep_uncovered, long long* __restrict__ counts) {
    __shared__ uint32_t tot_s[EDIT_WAVES];
    const int64_t p = (int64_t)blockIdx.x * EDIT_TILE + threadIdx.x;
    uint32_t seq4, q4;
    uint32_t n = stitch_position(table, qsum, draft, p, n_pos, state, min_qual,
                                 keep_uncovered != 0u, true, &seq4, &q4);
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

// n <= STITCH_MAX_BYTES staged bytes -> out[0..n): thread t stores word t of
// the 4-byte-aligned middle (at most EDIT_TILE words), the up to 3 bytes
// before it go out from wave 0 and the up to 3 after it from wave 1.
RK_DEV void stitch_flush(const uint8_t* lds, uint8_t* __restrict__ out,
                         uint32_t n) {
    const uint32_t t = threadIdx.x;
    uint32_t head = (uint32_t)(-reinterpret_cast<uintptr_t>(out) & 3u);
    head = head < n ? head : n;
    const uint32_t words = (n - head) >> 2;
    const uint32_t tail = head + 4u * words;
    if (t < words) {
        const uint8_t* s = lds + head + 4u * t;
        *reinterpret_cast<uint32_t*>(out + head + 4u * t) =
            (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) |
            ((uint32_t)s[3] << 24);
    }
    if (t < head) out[t] = lds[t];
    if (t >= 64u && tail + (t - 64u) < n)
        out[tail + (t - 64u)] = lds[tail + (t - 64u)];
}

__global__ __launch_bounds__(EDIT_TILE) void stitch_write_kernel(
    const uint32_t* __restrict__ table,
    const unsigned long long* __restrict__ qsum,
    const uint8_t* __restrict__ draft, int64_t n_pos,
    const long long* __restrict__ state,
    const long long* __restrict__ offsets, uint32_t min_qual,
    uint32_t keep_uncovered, uint8_t* __restrict__ seq,
    uint8_t* __restrict__ qual, int64_t total) {
    __shared__ uint32_t tot_s[EDIT_WAVES];
    __shared__ uint8_t seq_s[STITCH_MAX_BYTES], qual_s[STITCH_MAX_BYTES];
    const int64_t p = (int64_t)blockIdx.x * EDIT_TILE + threadIdx.x;
    uint32_t seq4, q4;
    const uint32_t own =
        stitch_position(table, qsum, draft, p, n_pos, state, min_qual,
                        keep_uncovered != 0u, qual == nullptr, &seq4, &q4);
    uint32_t x = own;  // inclusive scan inside the wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t y = __shfl_up(x, s);
        if (lane >= s) x += y;
    }
    if (lane == 63) tot_s[wave] = x;
    __syncthreads();
    uint32_t before = 0, n = 0;
#pragma unroll
    for (int w = 0; w < EDIT_WAVES; ++w) {
        if (w < wave) before += tot_s[w];
        n += tot_s[w];
    }
    const uint32_t lo = before + x - own;  // lo + own <= n <= STITCH_MAX_BYTES
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        if (i < own) {
            seq_s[lo + i] = (uint8_t)(seq4 >> (8 * i));
            qual_s[lo + i] =
                (uint8_t)(((q4 >> (8 * i)) & 0xFFu) + STITCH_PHRED_OFFSET);
        }
    }
    __syncthreads();
    // base + n <= total holds by construction; a byte never lands outside
    const int64_t base = offsets[blockIdx.x];
    if (base < 0 || base >= total) return;
    if (base + (int64_t)n > total) n = (uint32_t)(total - base);
    stitch_flush(seq_s, seq + base, n);
    if (qual != nullptr) stitch_flush(qual_s, qual + base, n);
}

// bounds, bytes per workgroup and their scan: fills state and turns counts
// (edit_num_blocks words) into the workgroups' byte offsets
void stitch_count(const uint32_t* table, const uint64_t* qsum,
                  const uint8_t* draft, int64_t n_pos, int64_t* state,
                  int64_t* counts, int min_qual, bool keep_uncovered,
                  hipStream_t stream) {
    if (n_pos <= 0) return;
    const int64_t blocks = edit_num_blocks(n_pos);
    edit_bounds(table, n_pos, state, stream);
    hipLaunchKernelGGL(stitch_count_kernel, dim3((unsigned)blocks),
                       dim3(EDIT_TILE), 0, stream, table,
                       reinterpret_cast<const unsigned long long*>(qsum),
                       draft, n_pos,
                       reinterpret_cast<const long long*>(state),
                       (uint32_t)min_qual, keep_uncovered ? 1u : 0u,
                       reinterpret_cast<long long*>(counts));
    edit_scan(counts, blocks, state, stream);
}

// `total` (state[2] as read back by the caller) bytes into seq and, unless it
// is null, into qual (Phred+33)
void stitch_write(const uint32_t* table, const uint64_t* qsum,
                  const uint8_t* draft, int64_t n_pos, const int64_t* state,
                  const int64_t* offsets, int min_qual, bool keep_uncovered,
                  uint8_t* seq, uint8_t* qual, int64_t total,
                  hipStream_t stream) {
    if (n_pos <= 0 || total <= 0) return;
    hipLaunchKernelGGL(stitch_write_kernel,
                       dim3((unsigned)edit_num_blocks(n_pos)), dim3(EDIT_TILE),
                       0, stream, table,
                       reinterpret_cast<const unsigned long long*>(qsum),
                       draft, n_pos,
                       reinterpret_cast<const long long*>(state),
                       reinterpret_cast<const long long*>(offsets),
                       (uint32_t)min_qual, keep_uncovered ? 1u : 0u, seq, qual,
                       total);
}

}  // namespace rk
