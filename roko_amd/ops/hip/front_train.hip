// Fused TRAINING front: embedding gather + dropout + fc1 + relu + dropout +
// fc2 + relu + dropout, forward AND backward, for gfx950.
//
// Replaces the reference's rnn_model.py:47-56 training graph (embedding ->
// permute -> fc1 -> fc2 -> reshape) which, executed op-by-op on torch/aten,
// cost ~3 ms/step at b=128 in dropout/reduce/scatter/GEMM glue
// (profiles/train_r01_kernel_stats.txt). Design:
//
//   * a workgroup (8 waves) owns a SLICE of one window's 90 columns
//     (CSPLIT workgroups per window — grid B x CSPLIT fills the 256 CUs);
//     all weights are staged in LDS once; each column is a chain of small
//     MFMA GEMMs over LDS tiles;
//   * dropout masks are COUNTER-BASED HASHES (common.h hash32) of
//     (seed, element index) — nothing is materialised. One 32-bit hash
//     yields TWO 16-bit keep decisions for an element pair, halving the
//     hash VALU. The backward regenerates the embedding mask from the same
//     seed and recovers the relu/dropout derivatives of t1/t2 from the
//     recomputed activations' signs (post > 0 <=> kept AND pre > 0);
//   * the backward RECOMPUTES m and t1 per column (MFMA is ~100x cheaper
//     than round-tripping the 173 MB of activations through HBM), carries
//     dW1/dW2 in REGISTER fragment accumulators across its columns, reduces
//     db1/db2 with lane shuffles into small LDS tables, accumulates the
//     embedding gradient in a (12,50) LDS table, and commits everything
//     with one atomic pass per workgroup at the end;
//   * EVERY MFMA operand is a 16-byte ds_read_b128 fragment read — tiles
//     are written in the layouts their consumers need. The LDS array is
//     per-CU, and scalar u16 fragment reads cost 16x more array cycles per
//     byte: the first version of this kernel was LDS-array-bound at 39.5%
//     SQ_LDS_IDX_ACTIVE (profiles/pmc_front_r01.txt). The one exception
//     (dm's W1 operand) reuses the resident row-major w1t via 8-scalar
//     reads, where a second 50 KB transposed copy would not fit; phase-dead
//     tiles share storage (unions) to stay under 160 KB, with the aliased
//     pad regions re-zeroed each column;
//   * dx is never needed: the input is integer base ids.

#include <cstdint>

#include "api.h"
#include "common.h"

namespace rk {
namespace front {

constexpr int R = 200;    // reads per window
constexpr int W = 90;     // columns per window
constexpr int E = 50;     // embedding dim
constexpr int F1 = 100;   // fc1 out
constexpr int F2 = 10;    // fc2 out
constexpr int OUT = 500;  // E * F2

constexpr int KP = 224;        // R padded to 7 k-steps of 32
constexpr int KP_LD = KP + 8;  // +8 bf16 padding against bank conflicts
constexpr int MP = 112;        // F1 padded to 7 m-tiles
constexpr int EP = 64;         // E padded to 4 n-tiles
constexpr int CSPLIT = 2;      // workgroups per window (column slices)

// dropout-mask hashes: one 32-bit hash covers an index PAIR; bit-halves give
// the two 16-bit keep decisions. thresh16 = keep * 65536.
RK_DEV uint32_t mask_hash(uint32_t seed, uint32_t pair_key) {
    return hash32(pair_key ^ (seed * 0x9E3779B9U));
}
RK_DEV bool keep_half(uint32_t h, int which, uint32_t thresh16) {
    return ((h >> (16 * which)) & 0xFFFFu) < thresh16;
}
// embedding-mask pair key: pairs over consecutive reads (r0 = 2q, r0+1)
RK_DEV uint32_t ekey(int b, int w, int q, int e) {
    return ((uint32_t)(b * W + w) * (R / 2) + q) * E + e;
}
// t1-mask pair key: pairs over consecutive fc1 rows (f0 = 2p, f0+1)
RK_DEV uint32_t t1key(int b, int w, int p, int e) {
    return ((uint32_t)(b * W + w) * (MP / 2) + p) * E + e;
}
// t2 mask: single elements (tiny count), half 0 of its hash
RK_DEV uint32_t t2key(int b, int w, int j, int e) {
    return ((uint32_t)(b * W + w) * F2 + j) * E + e;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(512, 2) void front_fwd_kernel(
    const uint8_t* __restrict__ ids,  // (B, R, W)
    const bf16* __restrict__ w1,      // (F1, R)
    const float* __restrict__ b1,     // (F1)
    const bf16* __restrict__ w2,      // (F2, F1)
    const float* __restrict__ b2,     // (F2)
    const bf16* __restrict__ emb,     // (12, E)
    bf16* __restrict__ out,           // (W, B, OUT)
    int B, uint32_t seed, float keep,
    const uint32_t* __restrict__ seed_ptr) {  // overrides `seed` if non-null
    __shared__ struct {
        bf16 w1t[MP][KP_LD];     // zero-padded W1 [f][r] (G1 A-operand)
        bf16 m_t[EP][KP_LD];     // masked embedding tile [e][r] (G1 B)
        bf16 t1_t[EP][136];      // t1 post-activation [e][f] (G3 B)
        bf16 w2_lds[16][136];    // zero-padded W2 [j][f] (G3 A)
        bf16 emb_s[12][E];
        bf16 t2st[OUT + 12];
        bf16 b1s[MP];
        bf16 b2s[16];
        uint8_t col_ids[R];
    } lds;

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;
    if (seed_ptr) seed = *seed_ptr;
    const uint32_t thresh16 = (uint32_t)(keep * 65536.0f);
    const float inv_keep = 1.0f / keep;
    const bool no_drop = keep >= 1.0f;  // eval/inference: skip every hash
    const int w_begin = blockIdx.y * (W / CSPLIT);
    const int w_end = (blockIdx.y + 1 == CSPLIT) ? W : w_begin + W / CSPLIT;

    // ---- one-time staging -------------------------------------------------
    for (int e = tid; e < MP * KP_LD; e += 512) (&lds.w1t[0][0])[e] = f2bf(0.f);
    for (int e = tid; e < EP * KP_LD; e += 512) (&lds.m_t[0][0])[e] = f2bf(0.f);
    for (int e = tid; e < EP * 136; e += 512) (&lds.t1_t[0][0])[e] = f2bf(0.f);
    for (int e = tid; e < 16 * 136; e += 512) (&lds.w2_lds[0][0])[e] = f2bf(0.f);
    for (int e = tid; e < MP; e += 512) lds.b1s[e] = f2bf(0.f);
    for (int e = tid; e < 16; e += 512) lds.b2s[e] = f2bf(0.f);
    __syncthreads();
    for (int e = tid; e < F1 * R; e += 512) lds.w1t[e / R][e % R] = w1[e];
    for (int e = tid; e < 12 * E; e += 512) lds.emb_s[e / E][e % E] = emb[e];
    for (int e = tid; e < F2 * F1; e += 512) lds.w2_lds[e / F1][e % F1] = w2[e];
    for (int e = tid; e < F1; e += 512) lds.b1s[e] = f2bf(b1[e]);
    for (int e = tid; e < F2; e += 512) lds.b2s[e] = f2bf(b2[e]);
    __syncthreads();

    for (int w = w_begin; w < w_end; ++w) {
        // ---- stage this column's read ids --------------------------------
        if (tid < R) lds.col_ids[tid] = ids[((size_t)b * R + tid) * W + w];
        __syncthreads();
        // ---- masked embedding tile, one hash per read PAIR ----------------
        if (no_drop) {
            uint8_t bid0[10], bid1[10];
            bf16 bev0[10], bev1[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const int p = tid + k * 512;
                if (p < E * (R / 2)) {
                    const int q = p % (R / 2);
                    bid0[k] = lds.col_ids[2 * q];
                    bid1[k] = lds.col_ids[2 * q + 1];
                }
            }
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const int p = tid + k * 512;
                if (p < E * (R / 2)) {
                    const int e = p / (R / 2);
                    bev0[k] = lds.emb_s[bid0[k]][e];
                    bev1[k] = lds.emb_s[bid1[k]][e];
                }
            }
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const int p = tid + k * 512;
                if (p < E * (R / 2)) {
                    const int e = p / (R / 2), q = p % (R / 2);
                    bf16 pk[2] = {bev0[k], bev1[k]};
                    *reinterpret_cast<uint32_t*>(&lds.m_t[e][2 * q]) =
                        *reinterpret_cast<const uint32_t*>(pk);
                }
            }
        } else {
            // three passes so the id reads, the embedding reads and the
            // stores each issue as one batch — the naive fused loop was a
            // col_ids -> emb -> store dependent LDS chain per pair
            uint8_t bid0[10], bid1[10];
            bf16 bev0[10], bev1[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const int p = tid + k * 512;
                if (p < E * (R / 2)) {
                    const int q = p % (R / 2);
                    bid0[k] = lds.col_ids[2 * q];
                    bid1[k] = lds.col_ids[2 * q + 1];
                }
            }
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const int p = tid + k * 512;
                if (p < E * (R / 2)) {
                    const int e = p / (R / 2);
                    bev0[k] = lds.emb_s[bid0[k]][e];
                    bev1[k] = lds.emb_s[bid1[k]][e];
                }
            }
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const int p = tid + k * 512;
                if (p < E * (R / 2)) {
                    const int e = p / (R / 2), q = p % (R / 2);
                    const uint32_t h = mask_hash(seed, ekey(b, w, q, e));
                    float v0 = keep_half(h, 0, thresh16)
                                   ? bf2f(bev0[k]) * inv_keep : 0.f;
                    float v1 = keep_half(h, 1, thresh16)
                                   ? bf2f(bev1[k]) * inv_keep : 0.f;
                    bf16 pk[2] = {f2bf(v0), f2bf(v1)};
                    *reinterpret_cast<uint32_t*>(&lds.m_t[e][2 * q]) =
                        *reinterpret_cast<const uint32_t*>(pk);
                }
            }
        }
        __syncthreads();

        // ---- G1: t1 = drop(relu(W1 · m + b1)) — 28 tiles over 8 waves ----
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int tile = wid + s * 8;
            if (tile < 28) {
                const int mt = tile >> 2, nt = tile & 3;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kb = 0; kb < 7; ++kb) {
                    bf16x8 a = lds_load_a_frag(&lds.w1t[0][0], mt * 16, kb * 32, KP_LD);
                    bf16x8 bb = lds_load_b_frag_t(&lds.m_t[0][0], nt * 16, kb * 32, KP_LD);
                    acc = mfma16x16x32(a, bb, acc);
                }
                const int e = nt * 16 + lcol;
#pragma unroll
                for (int i = 0; i < 4; i += 2) {
                    const int f = mt * 16 + lrow * 4 + i;
                    const uint32_t h = no_drop ? 0u
                        : mask_hash(seed ^ 0x51u, t1key(b, w, f >> 1, e));
                    bf16 pk[2];
#pragma unroll
                    for (int uu = 0; uu < 2; ++uu) {
                        float v = fmaxf(acc[i + uu] + bf2f(lds.b1s[f + uu]), 0.f);
                        const bool live = (f + uu < F1) && (e < E) &&
                                          (no_drop || keep_half(h, uu, thresh16));
                        pk[uu] = f2bf(live ? (no_drop ? v : v * inv_keep) : 0.f);
                    }
                    *reinterpret_cast<uint32_t*>(&lds.t1_t[e][f]) =
                        *reinterpret_cast<const uint32_t*>(pk);
                }
            }
        }
        __syncthreads();

        // ---- G3: t2 = drop(relu(W2 · t1 + b2)) — 4 tiles, waves 0..3 -----
        if (wid < 4) {
            const int nt = wid;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                bf16x8 a = lds_load_a_frag(&lds.w2_lds[0][0], 0, kb * 32, 136);
                bf16x8 bb = lds_load_b_frag_t(&lds.t1_t[0][0], nt * 16, kb * 32, 136);
                acc = mfma16x16x32(a, bb, acc);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = lrow * 4 + i;
                const int e = nt * 16 + lcol;
                if (j < F2 && e < E) {
                    float v = fmaxf(acc[i] + bf2f(lds.b2s[j]), 0.f);
                    const bool live = no_drop ||
                        keep_half(mask_hash(seed ^ 0x52u, t2key(b, w, j, e)),
                                  0, thresh16);
                    lds.t2st[e * F2 + j] =
                        f2bf(live ? (no_drop ? v : v * inv_keep) : 0.f);
                }
            }
        }
        __syncthreads();

        // ---- coalesced store: out[(w, b), :] ------------------------------
        {
            bf16* dst = out + ((size_t)w * B + b) * OUT;
            if (tid < 62)
                *reinterpret_cast<bf16x8*>(dst + tid * 8) =
                    *reinterpret_cast<const bf16x8*>(&lds.t2st[tid * 8]);
            else if (tid == 62)
#pragma unroll
                for (int q = 0; q < 4; ++q) dst[496 + q] = lds.t2st[496 + q];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// backward (recompute)
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(512, 2) void front_bwd_kernel(
    const uint8_t* __restrict__ ids,   // (B, R, W)
    const bf16* __restrict__ dseq,     // (W, B, OUT) grad wrt forward output
    const bf16* __restrict__ w1, const float* __restrict__ b1,
    const bf16* __restrict__ w2, const float* __restrict__ b2,
    const bf16* __restrict__ emb,
    float* __restrict__ dw1,  // (F1, R)  pre-zeroed, atomic-accumulated
    float* __restrict__ db1,  // (F1)
    float* __restrict__ dw2,  // (F2, F1)
    float* __restrict__ db2,  // (F2)
    const bf16* __restrict__ w1t_g,  // (208, 128) zero-padded W1^T image:
                              // source of the LDS w1t_t stage
    float* __restrict__ de,   // (12, E) pre-zeroed, atomic-accumulated
    int B, uint32_t seed, float keep, uint32_t phase_mask,
    const uint32_t* __restrict__ seed_ptr,
    const bf16* __restrict__ w1g) {  // (112, 232) zero-padded W1 in L2:
                              // the G1 recompute's A-fragments (frees the
                              // 52 KB [f][r] LDS copy for w1t_t)
    // phase_mask: timing-experiment switch (default 0x1F = all phases).
    // bit0 G1 recompute, bit1 G3+dt2, bit2 dt1, bit3 dW1/dW2, bit4 dm/de.
    __shared__ struct {
        // W1^T staged [r][f] ONCE at kernel start: the dm GEMM's B-operand
        // as conflict-free b128 reads. The former [f][r] W1 copy is gone —
        // the G1 recompute reads its A-fragments straight from the L2-
        // resident padded W1 image (w1g), the v2/v3 eval-front pattern.
        // Round-1's dm phase read W1^T from L2 per tile with no pipelining
        // cover: the dm/de phases were 332 us of the 736 us kernel.
        bf16 w1t_t[R + 8][136];
        union {
            bf16 m_t[EP][KP_LD];  // [e][r]: G1 B-operand (dead after G1)
            struct {              // live from the G3 phase on
                bf16 je[16][72];  // [j][e]: dW2 A-operand
                bf16 ej[EP][40];  // [e][j]: dt1 A-operand
            } g;
            bf16 dmm[EP][KP_LD];  // [e][r]: masked dm — the de GEMM's
                                  // B-operand (dead dt2 region, same size)
        } u1;
        bf16 m_rt[R + 8][72];     // [r][e]: dW1 B-operand (b128 fragments;
                                  // the k-major scalar read from m_t
                                  // measured 4-way bank-conflicted: +82 us)
        union {
            bf16 t1_t[EP][136];   // [e][f]: G3 B-operand (dead after G3)
            // 128 rows: the dm A-fragment reads k = f up to 127; rows
            // 112..119 alias t1_t's tail (finite values x zero W1^T pad),
            // rows 120..127 are zeroed once at staging (NaN hazard:
            // 0 x uninitialized-LDS-NaN = NaN — docs/KERNELS.md lesson 9)
            bf16 dt1_fe[128][72]; // [f][e]: dW1 + dm A-operand
        } u2;
        union {
            bf16 t1_fe[MP][72];     // [f][e]: dW2 B-operand + relu/drop mask
            // hot aliases t1_fe's first 3712 elements: t1_fe is dead after
            // the dt1/dW2 reads of the SAME column and fully rewritten by
            // the next column's G1 epilogue; its e-pad columns 64..71 are
            // never fragment-read (k stops at 63)
            bf16 hot_t[16][KP_LD];  // [c][r]: de GEMM A-operand
        } u4;
        bf16 w2_lds[32][136];    // [j][f]: G3 A-operand + dt1 B-operand
                                 // (k-major fragments read j up to 31:
                                 // rows 10..31 stay zero)
        bf16 dseq_st[OUT];
        bf16 emb_s[12][E];
        bf16 b1s[MP];
        bf16 b2s[16];
        uint8_t col_ids[R];
    } lds;

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;
    if (seed_ptr) seed = *seed_ptr;
    const uint32_t thresh16 = (uint32_t)(keep * 65536.0f);
    const float inv_keep = 1.0f / keep;
    const int w_begin = blockIdx.y * (W / CSPLIT);
    const int w_end = (blockIdx.y + 1 == CSPLIT) ? W : w_begin + W / CSPLIT;

    // ---- one-time staging + zero ------------------------------------------
    for (int e = tid; e < EP * KP_LD; e += 512) (&lds.u1.m_t[0][0])[e] = f2bf(0.f);
    for (int e = tid; e < EP * 136; e += 512) (&lds.u2.t1_t[0][0])[e] = f2bf(0.f);
    for (int e = tid; e < 16 * 72; e += 512)
        lds.u2.dt1_fe[112 + e / 72][e % 72] = f2bf(0.f);
    for (int e = tid; e < (R + 8) * 72; e += 512) (&lds.m_rt[0][0])[e] = f2bf(0.f);
    for (int e = tid; e < MP * 72; e += 512) (&lds.u4.t1_fe[0][0])[e] = f2bf(0.f);
    for (int e = tid; e < 32 * 136; e += 512) (&lds.w2_lds[0][0])[e] = f2bf(0.f);
    for (int e = tid; e < MP; e += 512) lds.b1s[e] = f2bf(0.f);
    for (int e = tid; e < 16; e += 512) lds.b2s[e] = f2bf(0.f);
    __syncthreads();
    // W1^T [r][f] from the padded L2 image (rows 200..207 / cols 100..127
    // are zero in the source; stride pad cols 128..135 are never read)
    for (int p = tid; p < (R + 8) * 128 / 8; p += 512) {
        const int r = p / 16, f = (p % 16) * 8;
        *reinterpret_cast<bf16x8*>(&lds.w1t_t[r][f]) =
            *reinterpret_cast<const bf16x8*>(w1t_g + (size_t)r * 128 + f);
    }
    for (int e = tid; e < 12 * E; e += 512) lds.emb_s[e / E][e % E] = emb[e];
    for (int e = tid; e < F2 * F1; e += 512) lds.w2_lds[e / F1][e % F1] = w2[e];
    for (int e = tid; e < F1; e += 512) lds.b1s[e] = f2bf(b1[e]);
    for (int e = tid; e < F2; e += 512) lds.b2s[e] = f2bf(b2[e]);

    // register accumulators carried across this slice's columns
    f32x4 dw1acc[12];
#pragma unroll
    for (int s = 0; s < 12; ++s) dw1acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 dw2acc = {0.f, 0.f, 0.f, 0.f};
    float db1acc[4] = {0.f, 0.f, 0.f, 0.f};
    float db2acc[4] = {0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    f32x4 de_acc = {0.f, 0.f, 0.f, 0.f};  // embedding-grad tile fragments
    for (int w = w_begin; w < w_end; ++w) {
        // ---- stage ids + dseq; rebuild m in BOTH layouts; re-zero the pad
        // regions of the aliased tiles (trashed by last column's grads) ----
        if (tid < R) lds.col_ids[tid] = ids[((size_t)b * R + tid) * W + w];
        if (tid < OUT)
            lds.dseq_st[tid] = dseq[((size_t)w * B + b) * OUT + tid];
        for (int z = tid; z < EP * 3; z += 512) {   // m_t K-pad r in [200,224)
            const int e = z / 3, c = 200 + (z % 3) * 8;
            *reinterpret_cast<bf16x8*>(&lds.u1.m_t[e][c]) = bf16x8{};
        }
        for (int z = tid; z < 14 * 25; z += 512) {  // m_t rows e in [50,64)
            const int e = 50 + z / 25, c = (z % 25) * 8;
            *reinterpret_cast<bf16x8*>(&lds.u1.m_t[e][c]) = bf16x8{};
        }
        for (int z = tid; z < EP * 3; z += 512) {   // t1_t K-pad f in [112,136)
            const int e = z / 3, c = 112 + (z % 3) * 8;
            *reinterpret_cast<bf16x8*>(&lds.u2.t1_t[e][c]) = bf16x8{};
        }
        __syncthreads();
        {
            // batched 3-pass build (see the forward kernel's comment)
            uint8_t bid0[10], bid1[10];
            bf16 bev0[10], bev1[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const int p = tid + k * 512;
                if (p < E * (R / 2)) {
                    const int q = p % (R / 2);
                    bid0[k] = lds.col_ids[2 * q];
                    bid1[k] = lds.col_ids[2 * q + 1];
                }
            }
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const int p = tid + k * 512;
                if (p < E * (R / 2)) {
                    const int e = p / (R / 2);
                    bev0[k] = lds.emb_s[bid0[k]][e];
                    bev1[k] = lds.emb_s[bid1[k]][e];
                }
            }
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const int p = tid + k * 512;
                if (p < E * (R / 2)) {
                    const int e = p / (R / 2), q = p % (R / 2);
                    const uint32_t h = mask_hash(seed, ekey(b, w, q, e));
                    float v0 = keep_half(h, 0, thresh16)
                                   ? bf2f(bev0[k]) * inv_keep : 0.f;
                    float v1 = keep_half(h, 1, thresh16)
                                   ? bf2f(bev1[k]) * inv_keep : 0.f;
                    bf16 pk[2] = {f2bf(v0), f2bf(v1)};
                    *reinterpret_cast<uint32_t*>(&lds.u1.m_t[e][2 * q]) =
                        *reinterpret_cast<const uint32_t*>(pk);
                    lds.m_rt[2 * q][e] = pk[0];
                    lds.m_rt[2 * q + 1][e] = pk[1];
                }
            }
        }
        __syncthreads();

        // ---- G1 recompute: t1 (same code path as forward => same bits) ----
#pragma clang loop unroll(disable)
        for (int s = 0; s < ((phase_mask & 1u) ? 4 : 0); ++s) {
            const int tile = wid + s * 8;
            if (tile < 28) {
                const int mt = tile >> 2, nt = tile & 3;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                // A-fragments from L2: batch-issue 4, then 3 more under the
                // first MFMAs (un-pipelined per-kb loads exposed ~200 cyc
                // of L2 latency per k-step: +74 us on this phase)
                bf16x8 ag0[4], ag1[3];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    ag0[q] = global_load_a_frag(w1g, mt * 16, q * 32, KP_LD);
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
                    if (kb < 3)
                        ag1[kb] = global_load_a_frag(w1g, mt * 16,
                                                     (kb + 4) * 32, KP_LD);
                    bf16x8 bb = lds_load_b_frag_t(&lds.u1.m_t[0][0], nt * 16,
                                                  kb * 32, KP_LD);
                    acc = mfma16x16x32(ag0[kb], bb, acc);
                }
#pragma unroll
                for (int kb = 0; kb < 3; ++kb) {
                    bf16x8 bb = lds_load_b_frag_t(&lds.u1.m_t[0][0], nt * 16,
                                                  (kb + 4) * 32, KP_LD);
                    acc = mfma16x16x32(ag1[kb], bb, acc);
                }
                const int e = nt * 16 + lcol;
#pragma unroll
                for (int i = 0; i < 4; i += 2) {
                    const int f = mt * 16 + lrow * 4 + i;
                    const uint32_t h =
                        mask_hash(seed ^ 0x51u, t1key(b, w, f >> 1, e));
                    bf16 pk[2];
#pragma unroll
                    for (int uu = 0; uu < 2; ++uu) {
                        float v = fmaxf(acc[i + uu] + bf2f(lds.b1s[f + uu]), 0.f);
                        const bool live = (f + uu < F1) && (e < E) &&
                                          keep_half(h, uu, thresh16);
                        pk[uu] = f2bf(live ? v * inv_keep : 0.f);
                    }
                    *reinterpret_cast<uint32_t*>(&lds.u2.t1_t[e][f]) =
                        *reinterpret_cast<const uint32_t*>(pk);
                    lds.u4.t1_fe[f][e] = pk[0];
                    lds.u4.t1_fe[f + 1][e] = pk[1];
                }
            }
        }
        __syncthreads();

        // ---- G3 recompute -> dt2 in both layouts (m_t region dies here) ---
        if (wid < 4 && (phase_mask & 2u)) {
            const int nt = wid;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                bf16x8 a = lds_load_a_frag(&lds.w2_lds[0][0], 0, kb * 32, 136);
                bf16x8 bb = lds_load_b_frag_t(&lds.u2.t1_t[0][0], nt * 16, kb * 32, 136);
                acc = mfma16x16x32(a, bb, acc);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = lrow * 4 + i;
                const int e = nt * 16 + lcol;
                float g = 0.f;
                if (j < F2 && e < E) {
                    const float t2pre = acc[i] + bf2f(lds.b2s[j]);
                    const uint32_t h =
                        mask_hash(seed ^ 0x52u, t2key(b, w, j, e));
                    if (t2pre > 0.f && keep_half(h, 0, thresh16))
                        g = bf2f(lds.dseq_st[e * F2 + j]) * inv_keep;
                }
                lds.u1.g.je[j][e] = f2bf(g);
                lds.u1.g.ej[e][j] = f2bf(g);
                db2acc[i] += g;  // per-lane partial; reduced once at the end
            }
        } else if (wid >= 4 && (phase_mask & 2u)) {
            // waves 4..7: zero the j in [16,32) pad of dt2_ej (read by the
            // dt1 GEMM's K loop; aliased memory holds stale m values)
            for (int z = tid - 256; z < EP * 2; z += 256) {
                const int e = z >> 1, c = 16 + (z & 1) * 8;
                *reinterpret_cast<bf16x8*>(&lds.u1.g.ej[e][c]) = bf16x8{};
            }
        }
        __syncthreads();

        // ---- dt1^T = dt2^T · W2, through relu1'/drop1' --------------------
        // (rows = e so each lane holds 4 CONSECUTIVE e values: the global
        // dt1g store packs them into one 8-byte write)
#pragma clang loop unroll(disable)
        for (int s = 0; s < ((phase_mask & 4u) ? 4 : 0); ++s) {
            const int tile = wid + s * 8;
            if (tile < 28) {
                const int emt = tile & 3, fnt = tile >> 2;
                bf16x8 a = lds_load_a_frag(&lds.u1.g.ej[0][0], emt * 16, 0, 40);
                // W2 read k-major from w2_lds (8-scalar; rows 10..31 zero)
                bf16x8 bb = lds_load_b_frag_km(&lds.w2_lds[0][0], 0,
                                               fnt * 16, 136);
                f32x4 acc = mfma16x16x32(a, bb, f32x4{0.f, 0.f, 0.f, 0.f});
                const int f = fnt * 16 + lcol;
                const int e0 = emt * 16 + lrow * 4;
                // one 8-byte read for the lane's 4 consecutive t1post values
                const bf16x4 t1p4 = *reinterpret_cast<const bf16x4*>(
                    &lds.u4.t1_fe[f][e0]);
                bf16x4 pk;
                float fsum = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // post > 0 <=> kept AND pre > 0 (chain rule collapses)
                    const float g =
                        (bf2f(t1p4[i]) > 0.f) ? acc[i] * inv_keep : 0.f;
                    pk[i] = f2bf(g);
                    fsum += g;
                }
                *reinterpret_cast<bf16x4*>(&lds.u2.dt1_fe[f][e0]) = pk;
                db1acc[s] += fsum;  // per-lane partial; reduced at the end
            }
        }
        __syncthreads();

        // ---- read-only phase: dW2 and dW1 fragment accumulation -----------
        if (wid < 7 && (phase_mask & 8u)) {  // dW2 += dt2 · t1^T
            const int nt = wid;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                bf16x8 a = lds_load_a_frag(&lds.u1.g.je[0][0], 0, kb * 32, 72);
                bf16x8 bb = lds_load_b_frag_t(&lds.u4.t1_fe[0][0], nt * 16, kb * 32, 72);
                dw2acc = mfma16x16x32(a, bb, dw2acc);
            }
        }
#pragma unroll
        for (int s = 0; s < 12; ++s) {  // dW1 += dt1 · m^T (A (f,e), B (e,r))
            const int tile = wid + s * 8;
            if (tile < 91 && (phase_mask & 8u)) {
                const int mt = tile / 13, nt = tile % 13;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    bf16x8 a = lds_load_a_frag(&lds.u2.dt1_fe[0][0], mt * 16, kb * 32, 72);
                    bf16x8 bb = lds_load_b_frag_t(&lds.m_rt[0][0], nt * 16, kb * 32, 72);
                    dw1acc[s] = mfma16x16x32(a, bb, dw1acc[s]);
                }
            }
        }
        __syncthreads();  // dW phases done: u1 (dt2) and u4 (t1_fe) are dead

        // ---- dm/de (merged from the former front_de kernel: the dt1 tile
        // is already in LDS here, so the (B,W,112,64) dt1g workspace round-
        // trip through HBM and the second kernel's launch/staging/barriers
        // all disappear) --------------------------------------------------
        if (phase_mask & 16u) {
            for (int z = tid; z < 16 * KP_LD / 8; z += 512)
                *reinterpret_cast<bf16x8*>(&lds.u4.hot_t[0][0] + z * 8) =
                    bf16x8{};
            __syncthreads();
            if (tid < R) lds.u4.hot_t[lds.col_ids[tid]][tid] = f2bf(1.0f);

            // dm^T[e][r] = dt1^T · W1: A from dt1_fe ([f][e], transposed
            // fragment reads), B = W1^T from the LDS stage (b128 reads —
            // round 1 read it per-tile from L2 with no latency cover and
            // the dm/de phases were 45% of this kernel)
#pragma clang loop unroll(disable)
            for (int s = 0; s < 7; ++s) {
                const int tile = wid + s * 8;
                if (tile < 52) {
                    const int emt = tile & 3, rnt = tile >> 2;
                    const int r = rnt * 16 + lcol;
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kb = 0; kb < 4; ++kb) {
                        bf16x8 a = lds_load_a_frag_t(&lds.u2.dt1_fe[0][0],
                                                     emt * 16, kb * 32, 72);
                        bf16x8 bb = lds_load_b_frag_t(&lds.w1t_t[0][0],
                                                      rnt * 16, kb * 32, 136);
                        acc = mfma16x16x32(a, bb, acc);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = emt * 16 + lrow * 4 + i;
                        float v = 0.f;
                        if (r < R && e < E) {
                            const uint32_t h =
                                mask_hash(seed, ekey(b, w, r >> 1, e));
                            if (keep_half(h, r & 1, thresh16))
                                v = acc[i] * inv_keep;
                        }
                        lds.u1.dmm[e][r] = f2bf(v);
                    }
                }
            }
            __syncthreads();
            // de += Hot^T · dmm — k-range split over both wave halves so
            // no half idles at the phase barrier
            {
                const int nt = wid & 3;
                const int kb0 = (wid < 4) ? 0 : 4;
                const int kb1 = (wid < 4) ? 4 : 7;
                for (int kb = kb0; kb < kb1; ++kb) {
                    bf16x8 a = lds_load_a_frag(&lds.u4.hot_t[0][0], 0,
                                               kb * 32, KP_LD);
                    bf16x8 bb = lds_load_b_frag_t(&lds.u1.dmm[0][0], nt * 16,
                                                  kb * 32, KP_LD);
                    de_acc = mfma16x16x32(a, bb, de_acc);
                }
            }
        }
        __syncthreads();
    }

    // ---- commit the per-workgroup accumulators ----------------------------
    if (phase_mask & 16u) {
        const int nt = wid & 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lrow * 4 + i;
            const int e = nt * 16 + lcol;
            if (c < 12 && e < E && de_acc[i] != 0.f)
                agent_atomic_add(&de[c * E + e], de_acc[i]);
        }
    }
#pragma unroll
    for (int s = 0; s < 12; ++s) {
        const int tile = wid + s * 8;
        if (tile < 91) {
            const int mt = tile / 13, nt = tile % 13;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = mt * 16 + lrow * 4 + i;
                const int r = nt * 16 + lcol;
                if (f < F1 && r < R) agent_atomic_add(&dw1[f * R + r], dw1acc[s][i]);
            }
        }
    }
    if (wid < 7) {
        const int nt = wid;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lrow * 4 + i;
            const int f = nt * 16 + lcol;
            if (j < F2 && f < F1) agent_atomic_add(&dw2[j * F1 + f], dw2acc[i]);
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {  // db1: fold lrow groups, lane per f commits
        const int tile = wid + s * 8;
        if (tile < 28) {
            const int f = (tile >> 2) * 16 + lcol;
            float red = db1acc[s];
            red += __shfl_xor(red, 16);
            red += __shfl_xor(red, 32);
            if (lrow == 0 && f < F1) agent_atomic_add(&db1[f], red);
        }
    }
    if (wid < 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // db2: fold the 16 lcol lanes
            const int j = lrow * 4 + i;
            float red = db2acc[i];
#pragma unroll
            for (int moff = 1; moff < 16; moff <<= 1)
                red += __shfl_xor(red, moff, 16);
            if (lcol == 0 && j < F2) agent_atomic_add(&db2[j], red);
        }
    }
}

// ---------------------------------------------------------------------------
// embedding gradient (dm -> de), standalone
// ---------------------------------------------------------------------------
// de[c,e] = sum over (b,w,r) of [ids==c] * maskE(r,e) * dm[b,w,r,e], with
// dm = W1^T · dt1 recomputed per column from the dt1g workspace. Kept out of
// front_bwd_kernel because the dm GEMM needs W1 in [r][f] layout — both W1
// layouts plus the backward's tiles exceed 160 KB LDS, and reading the
// resident [f][r] copy with scalar fragment loads measured as HALF the
// backward kernel (profiles/front_bwd_phases_r01). Here the transposed W1
// tile has LDS to itself and every operand is a b128 fragment read.

__global__ __launch_bounds__(512, 2) void front_de_kernel(
    const uint8_t* __restrict__ ids,   // (B, R, W)
    const bf16* __restrict__ dt1g,     // (B, W, MP, EP)
    const bf16* __restrict__ w1t_g,    // (R+8, 128) = W1^T zero-padded —
                                       // A-fragments read straight from L2
                                       // (53 KB shared by every CU) so LDS
                                       // stays under 80 KB and TWO
                                       // workgroups share each CU
    float* __restrict__ de,            // (12, E) pre-zeroed
    int B, uint32_t seed, float keep,
    unsigned long long* __restrict__ timing,  // optional (4) cycle counters
    uint32_t dbg,  // timing-bisection: 1 skip atomics, 2 skip hash, 4 skip epi
    const uint32_t* __restrict__ seed_ptr) {
    __shared__ struct {
        bf16 dt1_ef[EP][136];     // [e][f] staged column of dt1g
        bf16 dmm_er[EP][KP_LD];   // [e][r] masked dm (de-GEMM B-operand)
        bf16 hot_t[16][KP_LD];    // [c][r] one-hot of col_ids (de-GEMM A)
        uint8_t col_ids[R];
    } lds;

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;
    if (seed_ptr) seed = *seed_ptr;
    const uint32_t thresh16 = (uint32_t)(keep * 65536.0f);
    const float inv_keep = 1.0f / keep;
    const int w_begin = blockIdx.y * (W / CSPLIT);
    const int w_end = (blockIdx.y + 1 == CSPLIT) ? W : w_begin + W / CSPLIT;

    for (int e = tid; e < EP * 136; e += 512)
        (&lds.dt1_ef[0][0])[e] = f2bf(0.f);
    for (int e = tid; e < EP * KP_LD; e += 512)
        (&lds.dmm_er[0][0])[e] = f2bf(0.f);
    __syncthreads();

    unsigned long long tacc[3] = {0, 0, 0};
    unsigned long long tw0 = (timing && tid == 0) ? __builtin_amdgcn_s_memtime() : 0;
    float sink = 0.f;
    f32x4 de_acc = {0.f, 0.f, 0.f, 0.f};  // waves 0..3: de tile fragments
    for (int w = w_begin; w < w_end; ++w) {
        unsigned long long tp0 = (timing && tid == 0) ? __builtin_amdgcn_s_memtime() : 0;
        if (tid < R) lds.col_ids[tid] = ids[((size_t)b * R + tid) * W + w];
        for (int z = tid; z < 16 * KP_LD / 8; z += 512)
            *reinterpret_cast<bf16x8*>(&lds.hot_t[0][0] + z * 8) = bf16x8{};
        // stage dt1[b, w] (MP, EP) -> [e][f]: vector global reads, scalar
        // transposed LDS writes
        {
            const bf16* src = dt1g + ((size_t)b * W + w) * MP * EP;
            for (int p = tid; p < MP * EP / 8; p += 512) {
                const int f = p / (EP / 8), e0 = (p % (EP / 8)) * 8;
                bf16 v[8];
                *reinterpret_cast<bf16x8*>(v) = *reinterpret_cast<const bf16x8*>(
                    src + (size_t)f * EP + e0);
#pragma unroll
                for (int q = 0; q < 8; ++q) lds.dt1_ef[e0 + q][f] = v[q];
            }
        }
        __syncthreads();
        if (tid < R) lds.hot_t[lds.col_ids[tid]][tid] = f2bf(1.0f);
        if (timing && tid == 0) {
            unsigned long long t1 = __builtin_amdgcn_s_memtime();
            tacc[0] += t1 - tp0;
            tp0 = t1;
        }

        // dm^T[e, r] = dt1^T · W1 — 13x4 tiles over 8 waves, all b128.
        // The lane's read id is loaded ONCE per tile, FIRST, so its LDS
        // latency hides under the fragment loads: a per-element
        // col_ids read fed the atomic's ADDRESS and serialized the whole
        // epilogue into read -> lgkmcnt(0) -> ds_add chains (~150 cycles
        // per element, the dominant cost of v1 of this kernel).
#pragma clang loop unroll(disable)
        for (int s = 0; s < 7; ++s) {
            const int tile = wid + s * 8;
            if (tile < 52) {
                const int emt = tile & 3, rnt = tile >> 2;
                const int r = rnt * 16 + lcol;
                const int myid = lds.col_ids[r < R ? r : 0];
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
                    bf16x8 a = lds_load_a_frag(&lds.dt1_ef[0][0], emt * 16, kb * 32, 136);
                    bf16x8 bb = global_load_a_frag(w1t_g, rnt * 16, kb * 32, 128);
                    acc = mfma16x16x32(a, bb, acc);
                }
                (void)myid;
                if (dbg & 4u) {  // timing: epilogue stripped, sink the acc
                    sink += acc[0] + acc[1] + acc[2] + acc[3];
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = emt * 16 + lrow * 4 + i;
                        float v = 0.f;
                        if (r < R && e < E) {
                            const uint32_t h = (dbg & 2u) ? (uint32_t)e
                                : mask_hash(seed, ekey(b, w, r >> 1, e));
                            if (keep_half(h, r & 1, thresh16))
                                v = acc[i] * inv_keep;
                        }
                        lds.dmm_er[e][r] = f2bf(v);
                    }
                }
            }
        }
        __syncthreads();
        // de += Hot^T · dmm — ONE 16x64xK GEMM per column instead of ~13k
        // LDS atomics (the atomics measured ~20k cycles/column); the de
        // fragments live in registers across all columns
        if (wid < 4 && !(dbg & 4u)) {
            const int nt = wid;
#pragma unroll
            for (int kb = 0; kb < 7; ++kb) {
                bf16x8 a = lds_load_a_frag(&lds.hot_t[0][0], 0, kb * 32, KP_LD);
                bf16x8 bb = lds_load_b_frag_t(&lds.dmm_er[0][0], nt * 16, kb * 32, KP_LD);
                de_acc = mfma16x16x32(a, bb, de_acc);
            }
        }
        __syncthreads();
        if (timing && tid == 0) tacc[1] += __builtin_amdgcn_s_memtime() - tp0;
    }
    if (wid < 4) {
        const int nt = wid;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lrow * 4 + i;
            const int e = nt * 16 + lcol;
            if (c < 12 && e < E && de_acc[i] != 0.f)
                agent_atomic_add(&de[c * E + e], de_acc[i]);
        }
    }
    if (timing && tid == 0) {
        atomicAdd(&timing[0], tacc[0]);
        atomicAdd(&timing[1], tacc[1]);
        atomicAdd(&timing[3], __builtin_amdgcn_s_memtime() - tw0);
    }
    if (dbg && sink == 12345.678f) de[0] = sink;  // keep the sink alive
}

}  // namespace front

void front_fwd(const uint8_t* ids, const void* w1, const float* b1,
               const void* w2, const float* b2, const void* emb, void* out,
               int B, uint32_t seed, float keep, hipStream_t stream,
               const uint32_t* seed_ptr) {
    hipLaunchKernelGGL(front::front_fwd_kernel,
                       dim3(B, front::CSPLIT), dim3(512), 0, stream,
                       ids, static_cast<const bf16*>(w1), b1,
                       static_cast<const bf16*>(w2), b2,
                       static_cast<const bf16*>(emb), static_cast<bf16*>(out),
                       B, seed, keep, seed_ptr);
}

void front_de(const uint8_t* ids, const void* dt1g, const void* w1t_g,
              float* de, int B, uint32_t seed, float keep, hipStream_t stream,
              unsigned long long* timing, uint32_t dbg,
              const uint32_t* seed_ptr) {
    hipLaunchKernelGGL(front::front_de_kernel,
                       dim3(B, front::CSPLIT), dim3(512), 0, stream,
                       ids, static_cast<const bf16*>(dt1g),
                       static_cast<const bf16*>(w1t_g), de, B, seed, keep,
                       timing, dbg, seed_ptr);
}

void front_bwd(const uint8_t* ids, const void* dseq, const void* w1,
               const float* b1, const void* w2, const float* b2,
               const void* emb, float* dw1, float* db1, float* dw2, float* db2,
               const void* w1t_g, float* de, int B, uint32_t seed, float keep,
               hipStream_t stream, uint32_t phase_mask,
               const uint32_t* seed_ptr, const void* w1g) {
    hipLaunchKernelGGL(front::front_bwd_kernel,
                       dim3(B, front::CSPLIT), dim3(512), 0, stream,
                       ids, static_cast<const bf16*>(dseq),
                       static_cast<const bf16*>(w1), b1,
                       static_cast<const bf16*>(w2), b2,
                       static_cast<const bf16*>(emb), dw1, db1, dw2, db2,
                       static_cast<const bf16*>(w1t_g), de, B, seed, keep,
                       phase_mask, seed_ptr, static_cast<const bf16*>(w1g));
}

}  // namespace rk
