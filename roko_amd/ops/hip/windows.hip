// Device window builder: a region's packed reads -> the (n, 200, 90) window
// tensor and its (n, 90, 2) positions, in device memory. The GPU twin of
// extract_features (ops/cpp/pileup.cpp) in counter-sampler mode; that
// function is the byte-exact oracle (tests/test_gpu_windows.py).
//
// Input is what BAM stores: per read the reference bounds, the strand, the
// CIGAR words (len << 4 | op) and the 4-bit packed bases. Nothing is walked
// on the host. Six small kernels, all on one stream:
//
//   1 read_scan_mark   one wave per read: wave scan of the ops to (rpos, qpos)
//                      per op; every M/=/X/D op adds +1/-1 to a difference
//                      array over the region's positions (coverage), every
//                      attached I raises the insertion depth of its position
//                      (atomicMax). O(1) per op, whatever its length.
//   2 scan_columns     one workgroup: prefix sum of the difference array ->
//                      covered?, columns per position = 1 + insertion depth,
//                      exclusive scan -> first column of every position; the
//                      column and window counts go to `meta`.
//   3 column_table     the inverse: column -> position.
//   4 valid_mask       one lane per (window, read): does the read have an
//                      event with a known base in the window's 90 columns? A
//                      wave ballot is one 64-bit word of the window's read
//                      bitmask, so the valid list keeps ascending read order
//                      by construction (no compaction to get wrong).
//   5 word_prefix,     per window the exclusive popcount prefix of its mask
//     window_scan      words (V = total), then output slots of the non-empty
//                      windows.
//   6 fill_windows     one workgroup per non-empty window: 200 lanes draw
//                      their read (counter sampler: k-th set bit of the mask),
//                      then 256 lanes write the 18000 cells four at a time
//                      (one 32-bit store per lane, consecutive lanes on
//                      consecutive words).
//
// A cell is evaluated on its own: binary search of the read's op that covers
// the position (between the ops at the window's first and last position,
// found once per row), then the base. Rows of one window mostly share a few
// reads and neighbouring lanes share a row, so the searches hit the same
// cache lines.
//
// Zero-length CIGAR ops are not representable here the way the host builder
// treats them (an `0M` before an I re-attaches the insertion): they set
// WIN_ERR_ZERO_OP and the caller refuses the region.
//
// The end of the file holds the two kernels of the training route, which
// share the per-cell lookup: truth_scan and label_windows (7, 8) give every
// column of the built windows its truth label.

#include <cstdint>

#include "api.h"
#include "common.h"

namespace rk {

constexpr int WIN_ROWS = 200;
constexpr int WIN_COLS = 90;
constexpr int WIN_STRIDE = 30;
constexpr int WIN_MAX_INS = 3;
constexpr int WIN_CELLS = WIN_ROWS * WIN_COLS;  // 18000, a multiple of 4

constexpr uint32_t WB_GAP = 4, WB_UNKNOWN = 5, WB_STRAND = 6, WB_NONE = 255;
constexpr uint32_t OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_EQ = 7,
                   OP_X = 8;

// meta words
constexpr int WIN_META_NCOLS = 0, WIN_META_NALL = 1, WIN_META_NOUT = 2,
              WIN_META_ERR = 3;
constexpr int WIN_ERR_ZERO_OP = 1;   // a zero-length CIGAR op
constexpr int WIN_ERR_CAPACITY = 2;  // more columns than the caller's bound

struct WinPack {
    const int32_t* ref_start;   // (n)
    const int32_t* ref_end;     // (n) exclusive
    const uint8_t* reverse;     // (n)
    const uint32_t* cigar_off;  // (n + 1) words
    const uint32_t* seq_off;    // (n + 1) bytes
    const uint32_t* cigar;
    const uint8_t* seq4;
    int32_t* op_rpos;  // per op: reference position where it starts
    int32_t* op_qpos;  // per op: query index where it starts
    int n;
    int start, end;  // clamped region
};

RK_DEV bool op_is_match(uint32_t op) {
    return op == OP_M || op == OP_EQ || op == OP_X;
}

RK_DEV uint64_t mix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

RK_DEV int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// Exclusive scan of one int per thread over the workgroup (<= 1024 threads);
// `total` is the workgroup sum. `lds` holds 17 ints.
RK_DEV int block_excl_scan(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (blockDim.x + 63) >> 6;
    const int incl = wave_incl_scan(v);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        const int s = lane < nw ? lds[lane] : 0;
        const int si = wave_incl_scan(s);
        if (lane < nw) lds[lane] = si - s;
        if (lane == nw - 1) lds[16] = si;
    }
    __syncthreads();
    const int r = lds[wave] + incl - v;
    total = lds[16];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------------------
// 1. per-read op scan + coverage / insertion-depth marks
__global__ __launch_bounds__(256) void read_scan_mark_kernel(
    WinPack P, int32_t* __restrict__ diff,  // (L + 1), zeroed
    int32_t* __restrict__ insd,             // (L), zeroed
    int32_t* __restrict__ meta) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= P.n) return;
    const uint32_t c0 = P.cigar_off[r], c1 = P.cigar_off[r + 1];
    int rbase = P.ref_start[r], qbase = 0;
    for (uint32_t base = c0; base < c1; base += 64) {
        const uint32_t i = base + lane;
        const bool live = i < c1;
        const uint32_t w = live ? P.cigar[i] : 0u;
        const uint32_t op = w & 15u;
        const int len = (int)(w >> 4);
        const int rl = (live && (op_is_match(op) || op == OP_D || op == OP_N))
                           ? len : 0;
        const int ql = (live && (op_is_match(op) || op == OP_I || op == OP_S))
                           ? len : 0;
        const int ri = wave_incl_scan(rl), qi = wave_incl_scan(ql);
        const int rpos = rbase + ri - rl, qpos = qbase + qi - ql;
        rbase += __shfl(ri, 63);
        qbase += __shfl(qi, 63);
        if (!live) continue;
        P.op_rpos[i] = rpos;
        P.op_qpos[i] = qpos;
        if (len == 0)
            __hip_atomic_fetch_or(&meta[WIN_META_ERR], WIN_ERR_ZERO_OP,
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (op_is_match(op) || op == OP_D) {
            // slot-0 events at [rpos, rpos + len) ∩ [start, end)
            const int k0 = max(rpos, P.start), k1 = min(rpos + len, P.end);
            if (k0 < k1) {
                __hip_atomic_fetch_add(&diff[k0 - P.start], 1,
                                       __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&diff[k1 - P.start], -1,
                                       __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
        } else if (op == OP_I && i > c0 && op_is_match(P.cigar[i - 1] & 15u)) {
            // attaches to the last base of the M/=/X op right before it
            const int p = rpos - 1;
            if (p >= P.start && p < P.end)
                __hip_atomic_fetch_max(&insd[p - P.start],
                                       min(len, WIN_MAX_INS),
                                       __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---------------------------------------------------------------------------
// 2. positions -> first column (one workgroup of 1024, 4 positions a lane)
__global__ __launch_bounds__(1024) void scan_columns_kernel(
    const int32_t* __restrict__ diff, const int32_t* __restrict__ insd,
    int32_t* __restrict__ col0,  // (L + 1)
    int L, int ncols_max, int32_t* __restrict__ meta) {
    __shared__ int lds[17];
    int carry_cov = 0, carry_col = 0;
    for (int base = 0; base < L; base += 4096) {
        const int i0 = base + (int)threadIdx.x * 4;
        int c[4];
        int run = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            run += (i0 + j < L) ? diff[i0 + j] : 0;
            c[j] = run;
        }
        int tot;
        const int ex = block_excl_scan(run, lds, tot);
        int cnt[4];
        int sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool covered = (i0 + j < L) && (carry_cov + ex + c[j] > 0);
            cnt[j] = covered ? 1 + min(insd[i0 + j], WIN_MAX_INS) : 0;
            sum += cnt[j];
        }
        int tot2;
        int at = carry_col + block_excl_scan(sum, lds, tot2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < L) col0[i0 + j] = at;
            at += cnt[j];
        }
        carry_cov += tot;
        carry_col += tot2;
    }
    if (threadIdx.x == 0) {
        col0[L] = carry_col;
        int n_all = carry_col >= WIN_COLS
                        ? (carry_col - WIN_COLS) / WIN_STRIDE + 1 : 0;
        if (carry_col > ncols_max) {  // the caller's scratch would not hold it
            n_all = 0;
            __hip_atomic_fetch_or(&meta[WIN_META_ERR], WIN_ERR_CAPACITY,
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        meta[WIN_META_NCOLS] = carry_col;
        meta[WIN_META_NALL] = n_all;
    }
}

// ---------------------------------------------------------------------------
// 3. column -> position (relative to start)
__global__ __launch_bounds__(256) void column_table_kernel(
    const int32_t* __restrict__ col0, int32_t* __restrict__ colpos, int L,
    int ncols_max) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    const int a = col0[p], b = min(col0[p + 1], ncols_max);
    for (int c = a; c < b; ++c) colpos[c] = p;
}

// ---------------------------------------------------------------------------
// events of one read

// largest op j in [lo, hi] with op_rpos[j] <= pos (op_rpos[lo] <= pos given)
RK_DEV uint32_t find_op(const WinPack& P, uint32_t lo, uint32_t hi, int pos) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (P.op_rpos[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

RK_DEV uint32_t read_base(const WinPack& P, int r, int q) {
    const uint32_t s0 = P.seq_off[r], s1 = P.seq_off[r + 1];
    if (q < 0 || (uint32_t)(q >> 1) >= s1 - s0) return WB_UNKNOWN;
    const uint32_t b = P.seq4[s0 + (uint32_t)(q >> 1)];
    switch ((q & 1) ? (b & 15u) : (b >> 4)) {
        case 1: return 0;
        case 2: return 1;
        case 4: return 2;
        case 8: return 3;
        default: return WB_UNKNOWN;  // N and IUPAC codes
    }
}

// Base of read r's event at column (pos, slot), WB_NONE if it has none.
// ref_start <= pos < ref_end; [lo, hi] brackets the op that covers pos; c1 is
// the end of the read's ops.
RK_DEV uint32_t event_base(const WinPack& P, int r, int pos, int slot,
                           uint32_t lo, uint32_t hi, uint32_t c1) {
    const uint32_t j = find_op(P, lo, hi, pos);
    const uint32_t w = P.cigar[j];
    const uint32_t op = w & 15u;
    const int len = (int)(w >> 4);
    const int rp = P.op_rpos[j];
    if (slot == 0) {
        if (op_is_match(op)) return read_base(P, r, P.op_qpos[j] + pos - rp);
        return op == OP_D ? WB_GAP : WB_NONE;  // N-skip: no event
    }
    if (!op_is_match(op) || pos != rp + len - 1 || j + 1 >= c1) return WB_NONE;
    const uint32_t nx = P.cigar[j + 1];
    if ((nx & 15u) != OP_I || slot > min((int)(nx >> 4), WIN_MAX_INS))
        return WB_NONE;
    return read_base(P, r, P.op_qpos[j] + len - 1 + slot);
}

// ---------------------------------------------------------------------------
// 4. valid reads of every window, as a bitmask. Block b = (window, group of
// 256 reads); wave v of the block owns mask word group * 4 + v.
__global__ __launch_bounds__(256) void valid_mask_kernel(
    WinPack P, const int32_t* __restrict__ col0,
    const int32_t* __restrict__ colpos, const int32_t* __restrict__ meta,
    unsigned long long* __restrict__ mask, int nwords, int ngroups) {
    __shared__ int s_pos[WIN_COLS], s_slot[WIN_COLS];
    const int w = blockIdx.x / ngroups;
    const int group = blockIdx.x - w * ngroups;
    if (w >= meta[WIN_META_NALL]) return;
    if (threadIdx.x < WIN_COLS) {
        const int c = w * WIN_STRIDE + threadIdx.x;
        const int p = colpos[c];
        s_pos[threadIdx.x] = P.start + p;
        s_slot[threadIdx.x] = c - col0[p];
    }
    __syncthreads();
    const int r = group * 256 + threadIdx.x;
    bool valid = false;
    if (r < P.n) {
        const int rs = P.ref_start[r], re = P.ref_end[r];
        if (rs <= s_pos[WIN_COLS - 1] && re > s_pos[0]) {
            const uint32_t c0 = P.cigar_off[r], c1 = P.cigar_off[r + 1];
            for (int c = 0; c < WIN_COLS && !valid; ++c) {
                const int pos = s_pos[c];
                if (pos < rs) continue;
                if (pos >= re) break;
                valid = event_base(P, r, pos, s_slot[c], c0, c1 - 1, c1) <=
                        WB_GAP;
            }
        }
    }
    const unsigned long long word = __ballot(valid);
    const int wi = group * 4 + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && wi < nwords)
        mask[(size_t)w * nwords + wi] = word;
}

// 5a. one wave per window: exclusive popcount prefix of its mask words
__global__ __launch_bounds__(256) void word_prefix_kernel(
    const unsigned long long* __restrict__ mask,
    const int32_t* __restrict__ meta, int32_t* __restrict__ wpre,
    int32_t* __restrict__ nvalid, int nwords) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= meta[WIN_META_NALL]) return;
    int carry = 0;
    for (int base = 0; base < nwords; base += 64) {
        const int i = base + lane;
        const int pc = i < nwords ? __popcll(mask[(size_t)w * nwords + i]) : 0;
        const int incl = wave_incl_scan(pc);
        if (i < nwords) wpre[(size_t)w * nwords + i] = carry + incl - pc;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) nvalid[w] = carry;
}

// 5b. output slot of every non-empty window (one workgroup)
__global__ __launch_bounds__(1024) void window_scan_kernel(
    const int32_t* __restrict__ nvalid, int32_t* __restrict__ out_idx,
    int32_t* __restrict__ meta) {
    __shared__ int lds[17];
    const int n_all = meta[WIN_META_NALL];
    int carry = 0;
    for (int base = 0; base < n_all; base += 1024) {
        const int w = base + (int)threadIdx.x;
        const int f = (w < n_all && nvalid[w] > 0) ? 1 : 0;
        int tot;
        const int ex = block_excl_scan(f, lds, tot);
        if (w < n_all) out_idx[w] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) meta[WIN_META_NOUT] = carry;
}

// ---------------------------------------------------------------------------
// 6. one workgroup per window
__global__ __launch_bounds__(256) void fill_windows_kernel(
    WinPack P, const int32_t* __restrict__ col0,
    const int32_t* __restrict__ colpos,
    const unsigned long long* __restrict__ mask,
    const int32_t* __restrict__ wpre, const int32_t* __restrict__ nvalid,
    const int32_t* __restrict__ out_idx, int nwords, uint64_t region_key,
    uint32_t* __restrict__ x32,  // (n_out, 18000 / 4)
    int32_t* __restrict__ pos_out,  // (n_out, 90, 2)
    int n_out) {
    __shared__ int s_pos[WIN_COLS], s_slot[WIN_COLS];
    __shared__ int s_rid[WIN_ROWS];
    __shared__ uint32_t s_lo[WIN_ROWS], s_hi[WIN_ROWS];
    const int w = blockIdx.x;
    const int V = nvalid[w];
    const int out = out_idx[w];
    if (V <= 0 || out >= n_out) return;
    const int tid = threadIdx.x;
    if (tid < WIN_COLS) {
        const int c = w * WIN_STRIDE + tid;
        const int p = colpos[c];
        const int slot = c - col0[p];
        s_pos[tid] = P.start + p;
        s_slot[tid] = slot;
        pos_out[((size_t)out * WIN_COLS + tid) * 2] = P.start + p;
        pos_out[((size_t)out * WIN_COLS + tid) * 2 + 1] = slot;
    }
    __syncthreads();
    if (tid < WIN_ROWS) {
        const uint64_t draw = mix64(
            region_key ^ mix64(((uint64_t)(uint32_t)w << 32) | (uint64_t)tid));
        const int k = (int)(draw % (uint64_t)V);
        // the mask word that holds the k-th valid read, then the bit
        const int32_t* pre = wpre + (size_t)w * nwords;
        int lo = 0, hi = nwords - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pre[mid] <= k) lo = mid; else hi = mid - 1;
        }
        unsigned long long m = mask[(size_t)w * nwords + lo];
        for (int i = k - pre[lo]; i > 0; --i) m &= m - 1;
        const int rid = min(lo * 64 + (m ? __ffsll(m) - 1 : 0), P.n - 1);
        s_rid[tid] = rid;
        // ops at the window's first and last position bracket every search
        const int rs = P.ref_start[rid], re = P.ref_end[rid];
        const uint32_t c0 = P.cigar_off[rid], c1 = P.cigar_off[rid + 1];
        const int p_lo = s_pos[0], p_hi = s_pos[WIN_COLS - 1];
        uint32_t olo = c0, ohi = c1 - 1;
        if (p_lo >= rs && p_lo < re) olo = find_op(P, c0, c1 - 1, p_lo);
        if (p_hi >= rs && p_hi < re) ohi = find_op(P, olo, c1 - 1, p_hi);
        s_lo[tid] = olo;
        s_hi[tid] = ohi;
    }
    __syncthreads();
    for (int g = tid; g < WIN_CELLS / 4; g += 256) {
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = g * 4 + j;
            const int row = i / WIN_COLS, c = i - row * WIN_COLS;
            const int rid = s_rid[row];
            const int pos = s_pos[c];
            const int rs = P.ref_start[rid], re = P.ref_end[rid];
            uint32_t b = WB_NONE;
            if (pos >= rs && pos < re)
                b = event_base(P, rid, pos, s_slot[c], s_lo[row], s_hi[row],
                               P.cigar_off[rid + 1]);
            if (b == WB_NONE)  // exclusive end counted inside (pileup.cpp)
                b = (pos >= rs && pos <= re) ? WB_GAP : WB_UNKNOWN;
            if (P.reverse[rid]) b += WB_STRAND;
            word |= b << (8 * j);
        }
        x32[(size_t)out * (WIN_CELLS / 4) + g] = word;
    }
}

// ---------------------------------------------------------------------------
// host side

static WinPack make_pack(const int32_t* ref_start, const int32_t* ref_end,
                         const uint8_t* reverse, const uint32_t* cigar_off,
                         const uint32_t* seq_off, const uint32_t* cigar,
                         const uint8_t* seq4, int32_t* op_rpos,
                         int32_t* op_qpos, int n, int start, int end) {
    WinPack P;
    P.ref_start = ref_start;
    P.ref_end = ref_end;
    P.reverse = reverse;
    P.cigar_off = cigar_off;
    P.seq_off = seq_off;
    P.cigar = cigar;
    P.seq4 = seq4;
    P.op_rpos = op_rpos;
    P.op_qpos = op_qpos;
    P.n = n;
    P.start = start;
    P.end = end;
    return P;
}

bool windows_geometry_ok(int rows, int cols, int stride, int max_ins) {
    return rows == WIN_ROWS && cols == WIN_COLS && stride == WIN_STRIDE &&
           max_ins == WIN_MAX_INS;
}

// Kernels 1-5. diff (L + 1), insd (L) and meta (4) come in zeroed. n >= 1,
// L >= 1. After it meta holds {ncols, n_all, n_out, err}.
void windows_index(const int32_t* ref_start, const int32_t* ref_end,
                   const uint8_t* reverse, const uint32_t* cigar_off,
                   const uint32_t* seq_off, const uint32_t* cigar,
                   const uint8_t* seq4, int32_t* op_rpos, int32_t* op_qpos,
                   int n, int start, int end, int32_t* diff, int32_t* insd,
                   int32_t* col0, int32_t* colpos, int ncols_max,
                   int n_all_max, unsigned long long* mask, int32_t* wpre,
                   int32_t* nvalid, int32_t* out_idx, int32_t* meta,
                   hipStream_t stream) {
    const WinPack P = make_pack(ref_start, ref_end, reverse, cigar_off,
                                seq_off, cigar, seq4, op_rpos, op_qpos, n,
                                start, end);
    const int L = end - start;
    const int nwords = (n + 63) / 64, ngroups = (n + 255) / 256;
    hipLaunchKernelGGL(read_scan_mark_kernel, dim3((n + 3) / 4), dim3(256), 0,
                       stream, P, diff, insd, meta);
    hipLaunchKernelGGL(scan_columns_kernel, dim3(1), dim3(1024), 0, stream,
                       diff, insd, col0, L, ncols_max, meta);
    hipLaunchKernelGGL(column_table_kernel, dim3((L + 255) / 256), dim3(256),
                       0, stream, col0, colpos, L, ncols_max);
    if (n_all_max <= 0) return;  // meta says n_all = 0 too
    hipLaunchKernelGGL(valid_mask_kernel,
                       dim3((unsigned)n_all_max * (unsigned)ngroups),
                       dim3(256), 0, stream, P, col0, colpos, meta, mask,
                       nwords, ngroups);
    hipLaunchKernelGGL(word_prefix_kernel, dim3((n_all_max + 3) / 4),
                       dim3(256), 0, stream, mask, meta, wpre, nvalid, nwords);
    hipLaunchKernelGGL(window_scan_kernel, dim3(1), dim3(1024), 0, stream,
                       nvalid, out_idx, meta);
}

// Kernel 6, with n_all and n_out read back from meta by the caller.
void windows_fill(const int32_t* ref_start, const int32_t* ref_end,
                  const uint8_t* reverse, const uint32_t* cigar_off,
                  const uint32_t* seq_off, const uint32_t* cigar,
                  const uint8_t* seq4, int32_t* op_rpos, int32_t* op_qpos,
                  int n, int start, int end, const int32_t* col0,
                  const int32_t* colpos, const unsigned long long* mask,
                  const int32_t* wpre, const int32_t* nvalid,
                  const int32_t* out_idx, uint64_t region_key, int n_all,
                  int n_out, uint8_t* x, int32_t* pos, hipStream_t stream) {
    if (n_all <= 0 || n_out <= 0) return;
    const WinPack P = make_pack(ref_start, ref_end, reverse, cigar_off,
                                seq_off, cigar, seq4, op_rpos, op_qpos, n,
                                start, end);
    hipLaunchKernelGGL(fill_windows_kernel, dim3(n_all), dim3(256), 0, stream,
                       P, col0, colpos, mask, wpre, nvalid, out_idx,
                       (n + 63) / 64, region_key,
                       reinterpret_cast<uint32_t*>(x), pos, n_out);
}

// ---------------------------------------------------------------------------
// Truth labels of built windows (training features). The label of a column
// (pos, slot) is the truth alignment's base there: the per-cell CIGAR lookup
// of the read windows, applied to one alignment. labels.get_pos_and_labels
// plus the lookup of features._generate_train is the oracle; the numpy twin
// is ops/labels_device.py::label_windows_reference.
//
// A truth pack is a contig's truth alignments in the layout of the read pack
// (no strand). truth_scan runs once per contig; label_windows once per kept
// alignment of a region.

constexpr uint32_t OP_H = 5, OP_P = 6;
constexpr uint32_t LABEL_GAP = WB_GAP, LABEL_UNKNOWN = WB_UNKNOWN;
constexpr int LBL_ERR_ZERO_OP = 1;  // a zero-length CIGAR op
constexpr int LBL_ERR_CLIP = 2;     // S/H/P between aligned ops, or op > 8
constexpr int LBL_ERR_RANGE = 4;    // a column outside the label span

RK_DEV bool op_is_clip(uint32_t op) {
    return op == OP_S || op == OP_H || op == OP_P;
}

// 7. one wave per truth alignment: the op scan of read_scan_mark, without
// marks. err[r] collects the alignment's refusal bits.
__global__ __launch_bounds__(256) void truth_scan_kernel(
    WinPack P, int32_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= P.n) return;
    const uint32_t c0 = P.cigar_off[r], c1 = P.cigar_off[r + 1];
    // first and last op that is not a clip: clips outside them are the ends
    uint32_t first = c1, last = c0;
    for (uint32_t base = c0; base < c1; base += 64) {
        const uint32_t i = base + lane;
        const bool body = i < c1 && !op_is_clip(P.cigar[i] & 15u);
        const unsigned long long m = __ballot(body);
        if (m) {
            if (first == c1) first = base + (uint32_t)(__ffsll(m) - 1);
            last = base + 63u - (uint32_t)__clzll(m);
        }
    }
    int rbase = P.ref_start[r], qbase = 0;
    unsigned long long zero = 0, clip = 0;
    for (uint32_t base = c0; base < c1; base += 64) {
        const uint32_t i = base + lane;
        const bool live = i < c1;
        const uint32_t w = live ? P.cigar[i] : 0u;
        const uint32_t op = w & 15u;
        const int len = (int)(w >> 4);
        const int rl = (live && (op_is_match(op) || op == OP_D || op == OP_N))
                           ? len : 0;
        const int ql = (live && (op_is_match(op) || op == OP_I || op == OP_S))
                           ? len : 0;
        const int ri = wave_incl_scan(rl), qi = wave_incl_scan(ql);
        const int rpos = rbase + ri - rl, qpos = qbase + qi - ql;
        rbase += __shfl(ri, 63);
        qbase += __shfl(qi, 63);
        zero |= __ballot(live && len == 0);
        clip |= __ballot(live && (op > OP_X ||
                                  (op_is_clip(op) && i > first && i < last)));
        if (!live) continue;
        P.op_rpos[i] = rpos;
        P.op_qpos[i] = qpos;
    }
    if (lane == 0)
        err[r] = (zero ? LBL_ERR_ZERO_OP : 0) | (clip ? LBL_ERR_CLIP : 0);
}

// 8. one workgroup of two waves per window, one lane per column. Alignment r
// labels the columns; [lo, hi) is its label span (clamped to the alignment
// here, so no search leaves its ops).
__global__ __launch_bounds__(128) void label_windows_kernel(
    WinPack P, const int32_t* __restrict__ pos,  // (n, 90, 2)
    int r, int lo, int hi, uint8_t* __restrict__ labels,  // (n, 90)
    uint8_t* __restrict__ keep,                           // (n)
    int32_t* __restrict__ err) {
    __shared__ uint32_t s_op[2];
    __shared__ int s_p[2];
    const int w = blockIdx.x, tid = threadIdx.x;
    const uint32_t c0 = P.cigar_off[r], c1 = P.cigar_off[r + 1];
    lo = max(lo, P.ref_start[r]);
    hi = min(hi, P.ref_end[r]);
    const bool live = tid < WIN_COLS;
    int p = 0, slot = 0;
    if (live) {
        p = pos[((size_t)w * WIN_COLS + tid) * 2];
        slot = pos[((size_t)w * WIN_COLS + tid) * 2 + 1];
    }
    const bool inside = live && p >= lo && p < hi && slot >= 0;
    // the ops at the window's first and last position bracket every search
    if (tid == 0 || tid == WIN_COLS - 1) {
        const int e = tid == 0 ? 0 : 1;
        s_p[e] = p;
        s_op[e] = inside ? find_op(P, c0, c1 - 1, p) : (e ? c1 - 1 : c0);
        if (!inside) s_p[e] = e ? hi : lo - 1;  // brackets nothing
    }
    __syncthreads();
    uint32_t label = LABEL_GAP;
    if (live && !inside)
        __hip_atomic_fetch_or(err, LBL_ERR_RANGE, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
    if (inside) {
        // positions ascend inside a window; one that does not gets the
        // whole alignment
        const uint32_t olo = p >= s_p[0] && s_p[0] >= lo ? s_op[0] : c0;
        const uint32_t ohi = p <= s_p[1] && s_p[1] < hi ? s_op[1] : c1 - 1;
        const uint32_t j = find_op(P, olo, max(olo, ohi), p);
        const uint32_t cw = P.cigar[j];
        const uint32_t op = cw & 15u;
        const int len = (int)(cw >> 4);
        const int rp = P.op_rpos[j];
        if (slot == 0) {
            if (op_is_match(op))
                label = read_base(P, r, P.op_qpos[j] + p - rp);
            else if (op != OP_D && op != OP_N)  // no aligned op covers p
                __hip_atomic_fetch_or(err, LBL_ERR_RANGE, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
        } else if (p == rp + len - 1) {
            // the slot-th base of the run of I ops behind the op's last
            // position, whatever the op (M/=/X, D or N)
            int need = slot;
            for (uint32_t k = j + 1; k < c1; ++k) {
                const uint32_t nx = P.cigar[k];
                if ((nx & 15u) != OP_I) break;
                const int l = (int)(nx >> 4);
                if (need <= l) {
                    label = read_base(P, r, P.op_qpos[k] + need - 1);
                    break;
                }
                need -= l;
            }
        }
    }
    if (live) labels[(size_t)w * WIN_COLS + tid] = (uint8_t)label;
    const int unknown = __syncthreads_or(live && label == LABEL_UNKNOWN);
    if (tid == 0) keep[w] = unknown ? 0 : 1;
}

void truth_scan(const int32_t* ref_start, const int32_t* ref_end,
                const uint32_t* cigar_off, const uint32_t* seq_off,
                const uint32_t* cigar, const uint8_t* seq4, int32_t* op_rpos,
                int32_t* op_qpos, int n, int32_t* err, hipStream_t stream) {
    if (n <= 0) return;
    const WinPack P = make_pack(ref_start, ref_end, nullptr, cigar_off,
                                seq_off, cigar, seq4, op_rpos, op_qpos, n, 0,
                                0);
    hipLaunchKernelGGL(truth_scan_kernel, dim3((n + 3) / 4), dim3(256), 0,
                       stream, P, err);
}

// `err` (one word) comes in zeroed; 0 <= index < n.
void label_windows(const int32_t* ref_start, const int32_t* ref_end,
                   const uint32_t* cigar_off, const uint32_t* seq_off,
                   const uint32_t* cigar, const uint8_t* seq4,
                   int32_t* op_rpos, int32_t* op_qpos, int n, int index,
                   int lo, int hi, const int32_t* pos, int n_windows,
                   uint8_t* labels, uint8_t* keep, int32_t* err,
                   hipStream_t stream) {
    if (n_windows <= 0) return;
    const WinPack P = make_pack(ref_start, ref_end, nullptr, cigar_off,
                                seq_off, cigar, seq4, op_rpos, op_qpos, n, 0,
                                0);
    hipLaunchKernelGGL(label_windows_kernel, dim3(n_windows), dim3(128), 0,
                       stream, P, pos, index, lo, hi, labels, keep, err);
}

}  // namespace rk
