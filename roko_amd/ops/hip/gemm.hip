// bf16 GEMM + bias for the GRU input-projection shape family
// (M ~ 11520 = T*B, N <= 768, K <= 768) on gfx950.
//
// hipBLASLt's heuristic picks ~110 TF/s tiles for these shapes (xg GEMM
// measured 81 us — profiles/train_r01_kernel_stats.txt); the MFMA floor is
// ~10x lower. Canonical CDNA GEMM structure (cdna_hip_programming.md §5):
// 256x64 C-tiles, K staged in 32-wide slices through double-buffered LDS,
// A-fragments ds_read_b128 from row-major [row][k] images, B transposed at
// staging time into [col][k] images, bias fused into the epilogue, output
// staged through LDS for 16-byte coalesced stores.
//
//   C (M, N) bf16 = A (M, K) bf16 · B (K, N) bf16 + bias (N) f32
//
// M/N/K need not be multiples of the tile sizes (tails are masked).

#include <cstdint>

#include "api.h"
#include "common.h"

namespace rk {
namespace gemm {

constexpr int BM = 256;  // C-tile rows per workgroup
constexpr int BN = 64;   // C-tile cols per workgroup
constexpr int BK = 32;   // K slice per stage
constexpr int LDA = BK + 8;   // LDS row strides (bank-conflict pad)
constexpr int WAVES = 8;

__global__ __launch_bounds__(WAVES * 64, 2) void gemm_bias_kernel(
    const bf16* __restrict__ A,   // (M, K) row-major
    const bf16* __restrict__ B,   // (K, N) row-major
    const float* __restrict__ bias,  // (N) or nullptr
    bf16* __restrict__ C,         // (M, N) row-major
    int M, int N, int K) {
    __shared__ struct {
        bf16 a[2][BM][LDA];   // [row][k]
        bf16 bt[2][BN][LDA];  // [col][k] (transposed at staging)
    } lds;

    const int m0 = blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;

    // wave tiling: 8 waves x (2 m-subtiles x 4 n-subtiles)? -> each wave owns
    // two 16-row strips across two 16-col strips: tiles (mt, nt) with
    // mt = wid * 2 + {0,1} over 16 m-subtiles, nt = {0..3}
    // accumulators: 2 mt x 4 nt = 8 fragments
    f32x4 acc[2][4];
#pragma unroll
    for (int a_ = 0; a_ < 2; ++a_)
#pragma unroll
        for (int b_ = 0; b_ < 4; ++b_) acc[a_][b_] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int kq = (K + BK - 1) / BK;

    // cooperative staging: A tile BM x BK (8192 elems = 16/thread = 2 x b128),
    // B tile BK x BN (2048 elems = 4/thread, transposed scalar writes)
    // b128 loads/stores need 16-byte alignment: row starts are only aligned
    // when the row stride is a multiple of 8 bf16 elements (live shapes like
    // K=500 are not) — take the scalar tail path otherwise
    const bool a_aligned = (K % 8) == 0;
    auto stage = [&](int buf, int k0) {
        const bool full_k = (k0 + BK <= K);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int e = (p * 512 + tid) * 8;
            const int r = e / BK, kk = e % BK;
            const int row = m0 + r;
            bf16 v[8];
            if (full_k && a_aligned && row < M) {
                *reinterpret_cast<bf16x8*>(v) =
                    *reinterpret_cast<const bf16x8*>(A + (size_t)row * K + k0 + kk);
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    v[q] = (row < M && k0 + kk + q < K)
                               ? A[(size_t)row * K + k0 + kk + q] : f2bf(0.f);
            }
            *reinterpret_cast<bf16x8*>(&lds.a[buf][r][kk]) =
                *reinterpret_cast<const bf16x8*>(v);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int e = p * 512 + tid;
            const int kk = e / BN, c = e % BN;
            bf16 v = f2bf(0.f);
            if (k0 + kk < K && n0 + c < N) v = B[(size_t)(k0 + kk) * N + n0 + c];
            lds.bt[buf][c][kk] = v;
        }
    };

    stage(0, 0);
    __syncthreads();

    for (int q = 0; q < kq; ++q) {
        if (q + 1 < kq) stage((q + 1) & 1, (q + 1) * BK);
        bf16x8 bfr[4];
#pragma unroll
        for (int b_ = 0; b_ < 4; ++b_)
            bfr[b_] = lds_load_b_frag_t(&lds.bt[q & 1][0][0], b_ * 16, 0, LDA);
#pragma unroll
        for (int a_ = 0; a_ < 2; ++a_) {
            const int mt = wid * 2 + a_;
            bf16x8 af = lds_load_a_frag(&lds.a[q & 1][0][0], mt * 16, 0, LDA);
#pragma unroll
            for (int b_ = 0; b_ < 4; ++b_)
                acc[a_][b_] = mfma16x16x32(af, bfr[b_], acc[a_][b_]);
        }
        __syncthreads();
    }

    // epilogue: bias + staged coalesced store (reuse the A buffers)
    bf16* cst = &lds.a[0][0][0];  // BM x BN staging, stride BN
#pragma unroll
    for (int a_ = 0; a_ < 2; ++a_) {
        const int mt = wid * 2 + a_;
#pragma unroll
        for (int b_ = 0; b_ < 4; ++b_) {
            const int c = b_ * 16 + lcol;
            const float bv = bias ? bias[min(n0 + c, N - 1)] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = mt * 16 + lrow * 4 + i;
                cst[r * BN + c] = f2bf(acc[a_][b_][i] + bv);
            }
        }
    }
    __syncthreads();
    {
        const int n_full = (n0 + BN <= N) && ((N % 8) == 0);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int e = (p * 512 + tid) * 8;
            const int r = e / BN, c = e % BN;
            const int row = m0 + r;
            if (row < M) {
                if (n_full) {
                    *reinterpret_cast<bf16x8*>(C + (size_t)row * N + n0 + c) =
                        *reinterpret_cast<const bf16x8*>(&cst[r * BN + c]);
                } else {
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (n0 + c + u < N)
                            C[(size_t)row * N + n0 + c + u] = cst[r * BN + c + u];
                }
            }
        }
    }
}

}  // namespace gemm

void gemm_bias(const void* A, const void* B, const float* bias, void* C,
               int M, int N, int K, hipStream_t stream) {
    dim3 grid((M + gemm::BM - 1) / gemm::BM, (N + gemm::BN - 1) / gemm::BN);
    hipLaunchKernelGGL(gemm::gemm_bias_kernel, grid, dim3(gemm::WAVES * 64), 0,
                       stream, static_cast<const bf16*>(A),
                       static_cast<const bf16*>(B), bias, static_cast<bf16*>(C),
                       M, N, K);
}

// ---------------------------------------------------------------------------
// split-K  C (M, N) f32  +=  A (K, M)^T · B (K, N),  bf16 inputs
// ---------------------------------------------------------------------------
// The GRU weight-gradient reductions (dU = dhg^T·h_prev at (384,128) and
// dW_ih = dxg^T·x at (768,500), both K = T*B ~ 11520) map to transpose-A
// GEMMs that hipBLASLt runs WITHOUT split-K — 6 workgroups on a 256-CU chip,
// 81 us each (profiles/train_r01_latest). Here K is sliced across the grid
// (one 64-row stage per iteration, both operands transposed into LDS at
// staging time) and every workgroup commits its partial tile with relaxed
// agent-scope f32 atomics.

namespace gemmatb {

constexpr int BM = 128;  // C rows (= A cols) per workgroup
constexpr int BN = 128;  // C cols per workgroup
constexpr int BK = 64;   // K slice per stage
constexpr int KSLICE = 256;  // K rows per workgroup (KSLICE/BK stages)
constexpr int LDM = BM + 8;  // [k][m] row stride (staged UNtransposed)
constexpr int WAVES = 8;

__global__ __launch_bounds__(WAVES * 64, 2) void atb_splitk_kernel(
    const bf16* __restrict__ A,  // (K, M) rows strided by lda
    const bf16* __restrict__ B,  // (K, N) rows strided by ldb
    float* __restrict__ ws,      // (n_slices, M, N) partials (plain stores —
                                 // the atomic-commit version spent ~50 us in
                                 // 45-way same-address contention on dW_ih)
    int M, int N, int K, int lda, int ldb) {
    // staged in the GLOBAL orientation [k][m] / [k][n]: the transposed
    // staging this replaced wrote 8 scalar u16 per thread at an 8-row lane
    // stride whose dword period gcd'd with the 64 banks to 32 — 8-way bank
    // conflicts on every write, 88% LDS-conflict rate and 7.6% ACTIVE in
    // PMC (profiles/pmc_train_r01.txt). Un-transposed staging is straight
    // b128 stores; the fragment reads below pay scalar u16 loads instead
    // (2-cyc issues that hide under the MFMAs — docs/KERNELS.md lesson 3).
    __shared__ struct {
        bf16 at[2][BK][LDM];  // [k][m]
        bf16 bt[2][BK][LDM];  // [k][n]
    } lds;

    const int k_begin = blockIdx.x * KSLICE;
    const int m0 = blockIdx.y * BM;
    const int n0 = blockIdx.z * BN;
    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;

    // 8x8 = 64 sub-tiles over 8 waves: wave owns one 16-row strip (mt = wid)
    // across all 8 col strips
    f32x4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // stage one BK-slice: A rows [k0, k0+BK) cols [m0, m0+BM) transposed to
    // [m][k]; same for B. 128*64 elems each = 16/thread.
    // same alignment rule as gemm_bias_kernel: vector loads only when the
    // row stride keeps every row 16-byte aligned
    const bool m_aligned = (lda % 8) == 0;
    const bool n_aligned = (ldb % 8) == 0;
    auto stage = [&](int buf, int k0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int e = (p * 512 + tid) * 8;   // element in (BK, BM) slab
            const int kk = e / BM, m = e % BM;   // 8 consecutive m per thread
            bf16 v[8];
            const int krow = k0 + kk;
            if (krow < K && m_aligned && m0 + m + 7 < M) {
                *reinterpret_cast<bf16x8*>(v) = *reinterpret_cast<const bf16x8*>(
                    A + (size_t)krow * lda + m0 + m);
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    v[q] = (krow < K && m0 + m + q < M)
                               ? A[(size_t)krow * lda + m0 + m + q] : f2bf(0.f);
            }
            *reinterpret_cast<bf16x8*>(&lds.at[buf][kk][m]) =
                *reinterpret_cast<const bf16x8*>(v);
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int e = (p * 512 + tid) * 8;
            const int kk = e / BN, n = e % BN;
            bf16 v[8];
            const int krow = k0 + kk;
            if (krow < K && n_aligned && n0 + n + 7 < N) {
                *reinterpret_cast<bf16x8*>(v) = *reinterpret_cast<const bf16x8*>(
                    B + (size_t)krow * ldb + n0 + n);
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    v[q] = (krow < K && n0 + n + q < N)
                               ? B[(size_t)krow * ldb + n0 + n + q] : f2bf(0.f);
            }
            *reinterpret_cast<bf16x8*>(&lds.bt[buf][kk][n]) =
                *reinterpret_cast<const bf16x8*>(v);
        }
    };

    stage(0, k_begin);
    __syncthreads();
    const int stages = KSLICE / BK;
    for (int s = 0; s < stages; ++s) {
        if (s + 1 < stages) stage((s + 1) & 1, k_begin + (s + 1) * BK);
#pragma unroll
        for (int kb = 0; kb < BK / 32; ++kb) {
            bf16x8 af = lds_load_a_frag_t(&lds.at[s & 1][0][0], wid * 16,
                                          kb * 32, LDM);
#pragma unroll
            for (int b_ = 0; b_ < 8; ++b_) {
                bf16x8 bf_ = lds_load_b_frag_km(&lds.bt[s & 1][0][0], kb * 32,
                                                b_ * 16, LDM);
                acc[b_] = mfma16x16x32(af, bf_, acc[b_]);
            }
        }
        __syncthreads();
    }

    // plain-store the partial tile into this slice's workspace slab
    float* slab = ws + (size_t)blockIdx.x * M * N;
#pragma unroll
    for (int b_ = 0; b_ < 8; ++b_) {
        const int n = n0 + b_ * 16 + lcol;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + wid * 16 + lrow * 4 + i;
            if (m < M && n < N) slab[(size_t)m * N + n] = acc[b_][i];
        }
    }
}

// ws (S, MN) -> out (MN): one coalesced sweep
__global__ __launch_bounds__(256) void slice_sum_kernel(
    const float* __restrict__ ws, float* __restrict__ out, int S,
    int64_t MN) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 + 3 >= MN) {
        for (int64_t i = i0; i < MN; ++i) {
            float a = 0.f;
            for (int s = 0; s < S; ++s) a += ws[(size_t)s * MN + i];
            out[i] = a;
        }
        return;
    }
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
        const float* p = ws + (size_t)s * MN + i0;
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] += p[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) out[i0 + q] = a[q];
}

}  // namespace gemmatb

// ---------------------------------------------------------------------------
// Serving xg projection GEMM:  C (M, 768) = A (M, KP) · B (KP, 768) + bias
// (M = T*B, K <= 512). An LDS-free first attempt lost to hipBLASLt and is
// gone (docs/KERNELS.md lessons 13-15).
// xg_gemm2: the LDS-staged, shape-specialized kernel. gemm_bias (the generic
// kernel) compiles its runtime-K loop into per-chunk exec-mask branches and
// a vmcnt(0) drain after every staging load (ISA audit in the r2 notes) —
// 119 us for this shape. Here K is a template constant (fully unrolled,
// register-set double-buffering), staging is branchless b64/b128 with no
// bounds masks (M % 256 == 0, N = 768 exactly), and B stages straight from
// the (768, KP) padded W image whose [n][k] rows already ARE the
// b-fragment layout (no transpose, no conflicts).
namespace xg2 {

constexpr int XN = 768;
constexpr int BM = 256;   // C rows per workgroup (2 m-subtiles per wave)
constexpr int BN = 128;   // C cols per workgroup (8 n-subtiles)
constexpr int LD = 40;    // LDS k-slice stride (32 + 8 pad)
constexpr int WAVES = 8;

// phase timing (wave 0, workgroup 0 only): cycles in [commit+issue, mfma,
// barrier, epilogue] accumulated into timing[0..3] when non-null
#define XG2_T0 unsigned long long tp0 = (timing && tid == 0) \
        ? __builtin_amdgcn_s_memtime() : 0
#define XG2_T1(i) if (timing && tid == 0) { \
        unsigned long long tn = __builtin_amdgcn_s_memtime(); \
        tacc[i] += tn - tp0; tp0 = tn; }

template <int KP, int KREAL>
__global__ __launch_bounds__(WAVES * 64, 1) void xg_gemm2_kernel(
    const bf16* __restrict__ A,     // (M, KREAL) row-major (8-B aligned rows)
    const bf16* __restrict__ Bt,    // (768, KP) row-major = B^T, zero-padded
    const bf16* __restrict__ bias,  // (768)
    bf16* __restrict__ C,           // (M, 768)
    int M, unsigned long long* timing = nullptr) {
    unsigned long long tacc[4] = {0, 0, 0, 0};
    // 64-wide k-slices: half the barrier count of the 32-wide version
    // (phase timing showed ~480 cyc/iter of barrier wave-skew), two
    // 16-MFMA bursts per slice.
    constexpr int BK = 64;
    constexpr int KB = KP / BK;
    constexpr int LDK = BK + 8;
    __shared__ struct {
        bf16 a[2][BM][LDK];   // [row][k]
        bf16 b[2][BN][LDK];   // [n][k]
    } lds;

    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;
    const int m0 = blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;

    f32x4 acc[2][8];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging, branchless: A 256x64 = 32 el/thread as 8 b64 (8-B row
    // alignment holds for KREAL % 4 == 0), B 128x64 = 16 el/thread as
    // 2 b128 (KP % 8 == 0). Two register sets; the loop runs the MFMA
    // burst FIRST and commits after it, so the commit's vmcnt wait sits
    // a full ~1100-cycle MFMA burst after the loads were issued — the
    // 3-set variant bought the same cover with 24 more registers.
    uint64_t ra[2][8];
    bf16x8 rb[2][2];
    const int a_row = tid >> 1, a_c0 = (tid & 1) * 32;     // 2 threads/row
    const int b_row = tid >> 2, b_c0 = (tid & 3) * 16;     // 4 threads/row
    auto issue = [&](int kq, uint64_t(&va)[8], bf16x8(&vb)[2]) {
        const int k0 = kq * BK;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int col = k0 + a_c0 + q * 4;
            va[q] = (KREAL == KP || col + 4 <= KREAL)
                        ? *reinterpret_cast<const uint64_t*>(
                              A + (size_t)(m0 + a_row) * KREAL + col)
                        : 0u;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
            vb[j] = *reinterpret_cast<const bf16x8*>(
                Bt + (size_t)(n0 + b_row) * KP + k0 + b_c0 + j * 8);
    };
    auto commit = [&](int buf, uint64_t(&va)[8], bf16x8(&vb)[2]) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            *reinterpret_cast<uint64_t*>(&lds.a[buf][a_row][a_c0 + q * 4]) =
                va[q];
#pragma unroll
        for (int j = 0; j < 2; ++j)
            *reinterpret_cast<bf16x8*>(&lds.b[buf][b_row][b_c0 + j * 8]) =
                vb[j];
    };
    auto mfma_step = [&](int buf) {
        // two k-halves; within each, batch the fragment reads before the
        // MFMA burst so the lgkmcnt waits overlap
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            bf16x8 af[2], bfr[8];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                af[mt] = lds_load_a_frag(&lds.a[buf][0][0],
                                         (wid * 2 + mt) * 16, kh * 32, LDK);
#pragma unroll
            for (int nt = 0; nt < 8; ++nt)
                bfr[nt] = lds_load_b_frag_t(&lds.b[buf][0][0], nt * 16,
                                            kh * 32, LDK);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 8; ++nt)
                    acc[mt][nt] = mfma16x16x32(af[mt], bfr[nt], acc[mt][nt]);
        }
    };

    issue(0, ra[0], rb[0]);
    commit(0, ra[0], rb[0]);
    if (KB > 1) issue(1, ra[1], rb[1]);
    __syncthreads();
    XG2_T0;
#pragma unroll
    for (int kq = 0; kq < KB; ++kq) {
        mfma_step(kq & 1);
        XG2_T1(1);
        if (kq + 1 < KB) commit((kq + 1) & 1, ra[(kq + 1) & 1],
                                rb[(kq + 1) & 1]);
        if (kq + 2 < KB) issue(kq + 2, ra[kq & 1], rb[kq & 1]);
        XG2_T1(0);
        __syncthreads();
        XG2_T1(2);
    }

    // epilogue: bias + direct stores from the accumulators. A quarter-wave
    // writes 16 consecutive bf16 (one 32-B chunk) per fragment row; no LDS
    // round-trip (the staged version cost ~4k cycles of exposed latency).
    float br[8];
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
        br[nt] = bf2f(bias[n0 + nt * 16 + lcol]);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const size_t rbase = (size_t)(m0 + (wid * 2 + mt) * 16 + lrow * 4);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                C[(rbase + i) * XN + n0 + nt * 16 + lcol] =
                    f2bf(acc[mt][nt][i] + br[nt]);
    }
    XG2_T1(3);
    if (timing && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = 0; i < 4; ++i) timing[i] = tacc[i];
}

}  // namespace xg2

void xg_gemm2(const void* A, const void* Bt, const void* bias, void* C,
              int M, int KREAL, int KP, hipStream_t stream,
              unsigned long long* timing) {
    dim3 grid(M / xg2::BM, xg2::XN / xg2::BN);
    dim3 block(xg2::WAVES * 64);
    if (KP == 512 && KREAL == 500)
        hipLaunchKernelGGL((xg2::xg_gemm2_kernel<512, 500>), grid, block, 0,
                           stream, static_cast<const bf16*>(A),
                           static_cast<const bf16*>(Bt),
                           static_cast<const bf16*>(bias),
                           static_cast<bf16*>(C), M, timing);
    else if (KP == 512 && KREAL == 512)
        hipLaunchKernelGGL((xg2::xg_gemm2_kernel<512, 512>), grid, block, 0,
                           stream, static_cast<const bf16*>(A),
                           static_cast<const bf16*>(Bt),
                           static_cast<const bf16*>(bias),
                           static_cast<bf16*>(C), M, timing);
    else if (KP == 256 && KREAL == 256)
        hipLaunchKernelGGL((xg2::xg_gemm2_kernel<256, 256>), grid, block, 0,
                           stream, static_cast<const bf16*>(A),
                           static_cast<const bf16*>(Bt),
                           static_cast<const bf16*>(bias),
                           static_cast<bf16*>(C), M, timing);
}

// ---------------------------------------------------------------------------
// xg_gemm3: xg_gemm2 re-shaped for the coalesced serving width (M = 92160,
// 4320 tiles instead of 270 — docs/KERNELS.md lesson 21). Same arithmetic
// (one 16x16x32 accumulator chain per output, k ascending, fp32 bias add,
// one bf16 round), so the output equals xg_gemm2's byte for byte. What
// changed around the MFMAs:
//   * 128x128 tile, 4 waves of 64x64 (8 fragment reads per 16 MFMAs, not
//     10), 64 KB of LDS -> TWO workgroups per CU: one block's barrier skew
//     and epilogue run under the other block's MFMA bursts;
//   * 1-D grid with the bijective XCD remap: the six n-tiles of one m-tile
//     run back to back on one XCD, so an A tile leaves HBM once and the
//     other five reads hit that XCD's L2;
//   * A rows are 16-B aligned with a leading dimension (the layer-0 input
//     is a 512-stride zero-padded buffer): every staging access is b128 and
//     one 8-lane group reads one full 128-B line. No K=500 select;
//   * unpadded 128-B LDS rows with the 16-B chunk index XORed by
//     (row >> 1) & 7: conflict-free for ds_read_b128's four 16-lane groups
//     (the 144-B pitch of xg_gemm2 is 2-way conflicted on 7 of 8 rows) and
//     for the b128 staging writes;
//   * the MFMA takes the W fragment as its A operand, so a lane holds four
//     CONSECUTIVE output columns of one row; the tile goes through a
//     wave-private swizzled LDS image (the dead staging buffers) and leaves
//     as b128 stores, eight lanes covering one 128-B line per row.
namespace xg3 {

constexpr int XN = 768;
constexpr int BM = 128;   // C rows per workgroup
constexpr int BN = 128;   // C cols per workgroup
constexpr int BK = 64;    // k-slice per stage (128-B LDS rows)
constexpr int WAVES = 4;  // 2 (m) x 2 (n), 64x64 per wave
constexpr int NT = XN / BN;
constexpr int TILE_BYTES = BM * BK * 2;  // one operand, one buffer: 16 KB

// byte offset of 16-B chunk q (0..7) of row `row` in a [rows][64] image
RK_DEV int swz(int row, int q) {
    return row * 128 + ((q ^ ((row >> 1) & 7)) << 4);
}

// Phase stamps, STAMP instantiations only (scripts/xg4_phases.py): the
// shader clock as one statement with its own lgkmcnt(0), fenced so nothing
// moves across it. A stamped build forbids overlaps the real kernel has:
// read its shares, never its length.
constexpr int STAMP_WORDS = 16;  // u64 per workgroup, layout in xg4_phases.py
RK_DEV unsigned long long stamp_clock() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
RK_DEV unsigned long long stamp_realtime() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
// (XCC id << 32) | HW_ID: which CU of which XCD this workgroup ran on
RK_DEV unsigned long long stamp_place() {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\t"
                 "s_getreg_b32 %1, hwreg(HW_REG_XCC_ID)"
                 : "=s"(hw), "=s"(xcc));
    return ((unsigned long long)xcc << 32) | hw;
}

template <int KP, bool STAMP = false>
__global__ __launch_bounds__(WAVES * 64, 2) void xg_gemm3_kernel(
    const bf16* __restrict__ A,     // (M, KP) rows strided by lda (16-B rows)
    const bf16* __restrict__ Bt,    // (768, KP) row-major = B^T, zero-padded
    const bf16* __restrict__ bias,  // (768)
    bf16* __restrict__ C,           // (M, 768)
    int lda, int nwg, unsigned long long* __restrict__ stamps = nullptr) {
    constexpr int KB = KP / BK;
    // [buf][A | B][16 KB]; the epilogue reuses it as 4 x 8 KB wave images
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * 2 * TILE_BYTES];
    unsigned long long ts[KB + 3] = {}, rt0 = 0;
    if constexpr (STAMP) {
        rt0 = stamp_realtime();
        ts[0] = stamp_clock();
    }

    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;
    const int wm = wid >> 1, wn = wid & 1;

    // bijective XCD remap: workgroups that share blockIdx % 8 share an XCD
    // and are dispatched in blockIdx order, so give each such group one
    // contiguous run of tile ids (n fastest)
    const int orig = blockIdx.x;
    const int xcd = orig & 7;
    const int q8 = nwg >> 3, r8 = nwg & 7;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8)
                     + (orig >> 3);
    const int m0 = (wgid / NT) * BM;
    const int n0 = (wgid % NT) * BN;

    f32x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging: each operand slice is 128 rows x 128 B = 4 b128 per thread,
    // 8 threads per row. Two register sets, committed after the MFMA burst
    // that follows their issue (the xg_gemm2 schedule).
    bf16x8 ra[2][4], rb[2][4];
    const int s_row = tid >> 3, s_q = tid & 7;
    const bf16* a_src = A + (size_t)(m0 + s_row) * lda + s_q * 8;
    const bf16* b_src = Bt + (size_t)(n0 + s_row) * KP + s_q * 8;
    const int s_off = swz(s_row, s_q);  // + p * 32 rows: swizzle unchanged
    auto issue = [&](int kq, bf16x8(&va)[4], bf16x8(&vb)[4]) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            va[p] = *reinterpret_cast<const bf16x8*>(
                a_src + (size_t)p * 32 * lda + kq * BK);
            vb[p] = *reinterpret_cast<const bf16x8*>(
                b_src + (size_t)p * 32 * KP + kq * BK);
        }
    };
    auto commit = [&](int buf, bf16x8(&va)[4], bf16x8(&vb)[4]) {
        unsigned char* ab = lds + buf * 2 * TILE_BYTES;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<bf16x8*>(ab + p * 32 * 128 + s_off) = va[p];
            *reinterpret_cast<bf16x8*>(ab + TILE_BYTES + p * 32 * 128 + s_off) =
                vb[p];
        }
    };
    // fragment reads: row = 16-row subtile + lcol, chunk = kh * 4 + lrow
    const int fsw = (lcol >> 1) & 7;
    const int fa_off = (wm * 64 + lcol) * 128;
    const int fb_off = TILE_BYTES + (wn * 64 + lcol) * 128;
    auto mfma_step = [&](int buf) {
        const unsigned char* ab = lds + buf * 2 * TILE_BYTES;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            const int ch = ((kh * 4 + lrow) ^ fsw) << 4;
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = *reinterpret_cast<const bf16x8*>(
                    ab + fa_off + t * 16 * 128 + ch);
                wf[t] = *reinterpret_cast<const bf16x8*>(
                    ab + fb_off + t * 16 * 128 + ch);
            }
            // W fragment as the A operand: D[n][m], lane (lrow, lcol) holds
            // C[m = lcol][n = lrow * 4 + i]
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[mt][nt] = mfma16x16x32(wf[nt], af[mt], acc[mt][nt]);
        }
    };

    // slice kq + 2 is issued into the set slice kq was committed from, BEFORE
    // slice kq's MFMA burst: its loads stay in flight across two bursts and
    // the barrier between them (the commit waits a counted vmcnt(8))
    issue(0, ra[0], rb[0]);
    if (KB > 1) issue(1, ra[1], rb[1]);
    commit(0, ra[0], rb[0]);
    __syncthreads();
    if constexpr (STAMP) ts[1] = stamp_clock();
#pragma unroll
    for (int kq = 0; kq < KB; ++kq) {
        if (kq + 2 < KB) issue(kq + 2, ra[kq & 1], rb[kq & 1]);
        mfma_step(kq & 1);
        if (kq + 1 < KB) commit((kq + 1) & 1, ra[(kq + 1) & 1],
                                rb[(kq + 1) & 1]);
        __syncthreads();
        if constexpr (STAMP) ts[2 + kq] = stamp_clock();
    }

    // epilogue: fp32 bias add, one bf16 round, 8-B packed writes into this
    // wave's 64 x 128-B image (chunk ^ (row & 7)), then b128 row reads and
    // b128 global stores — 8 lanes per 128-B line of C
    unsigned char* img = lds + wid * (64 * 128);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int nl = nt * 16 + lrow * 4;
        bf16x4 bv = *reinterpret_cast<const bf16x4*>(
            reinterpret_cast<const __bf16*>(bias) + n0 + wn * 64 + nl);
        float br[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) br[i] = (float)bv[i];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int row = mt * 16 + lcol;
            alignas(8) bf16 o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = f2bf(acc[mt][nt][i] + br[i]);
            *reinterpret_cast<uint64_t*>(
                img + row * 128 + (((nl >> 3) ^ (row & 7)) << 4) +
                (nl & 4) * 2) = *reinterpret_cast<const uint64_t*>(o);
        }
    }
    __syncthreads();
    {
        const int r8l = lane >> 3, j = lane & 7;
        bf16* cdst = C + (size_t)(m0 + wm * 64 + r8l) * XN + n0 + wn * 64 + j * 8;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int row = p * 8 + r8l;
            *reinterpret_cast<bf16x8*>(cdst + (size_t)p * 8 * XN) =
                *reinterpret_cast<const bf16x8*>(
                    img + row * 128 + ((j ^ (row & 7)) << 4));
        }
    }
    if constexpr (STAMP) {
        // [0] entry, [1] first barrier, [2 .. 2+KB) end of each slice (the
        // last one is the epilogue's start), [10] last store issued, [11]/[12]
        // wall clock at entry / exit, [13] placement. Lane 0 of wave 0
        // writes them, to a buffer nothing else in the kernel touches.
        ts[KB + 2] = stamp_clock();
        const unsigned long long rt1 = stamp_realtime();
        const unsigned long long place = stamp_place();
        if (tid == 0) {
            unsigned long long* o = stamps + (size_t)orig * STAMP_WORDS;
#pragma unroll
            for (int i = 0; i < KB + 2; ++i) o[i] = ts[i];
            o[10] = ts[KB + 2];
            o[11] = rt0;
            o[12] = rt1;
            o[13] = place;
        }
    }
}

}  // namespace xg3

// A (M, KP) with leading dimension lda (elements, % 8 == 0, 16-B aligned
// base), M % 128 == 0, KP in {256, 512}
void xg_gemm3(const void* A, int lda, const void* Bt, const void* bias,
              void* C, int M, int KP, hipStream_t stream) {
    const int nwg = (M / xg3::BM) * xg3::NT;
    dim3 grid(nwg), block(xg3::WAVES * 64);
    if (KP == 512)
        hipLaunchKernelGGL((xg3::xg_gemm3_kernel<512>), grid, block, 0, stream,
                           static_cast<const bf16*>(A),
                           static_cast<const bf16*>(Bt),
                           static_cast<const bf16*>(bias),
                           static_cast<bf16*>(C), lda, nwg, nullptr);
    else if (KP == 256)
        hipLaunchKernelGGL((xg3::xg_gemm3_kernel<256>), grid, block, 0, stream,
                           static_cast<const bf16*>(A),
                           static_cast<const bf16*>(Bt),
                           static_cast<const bf16*>(bias),
                           static_cast<bf16*>(C), lda, nwg, nullptr);
}

int xg_gemm3_tile_m() { return xg3::BM; }

// The timing-only instantiation of xg_gemm3 (scripts/xg4_phases.py): same
// grid, same output, plus STAMP_WORDS u64 per workgroup in `stamps`.
void xg_gemm3_stamped(const void* A, int lda, const void* Bt,
                      const void* bias, void* C, int M, int KP,
                      unsigned long long* stamps, hipStream_t stream) {
    const int nwg = (M / xg3::BM) * xg3::NT;
    dim3 grid(nwg), block(xg3::WAVES * 64);
    if (KP == 512)
        hipLaunchKernelGGL((xg3::xg_gemm3_kernel<512, true>), grid, block, 0,
                           stream, static_cast<const bf16*>(A),
                           static_cast<const bf16*>(Bt),
                           static_cast<const bf16*>(bias),
                           static_cast<bf16*>(C), lda, nwg, stamps);
    else if (KP == 256)
        hipLaunchKernelGGL((xg3::xg_gemm3_kernel<256, true>), grid, block, 0,
                           stream, static_cast<const bf16*>(A),
                           static_cast<const bf16*>(Bt),
                           static_cast<const bf16*>(bias),
                           static_cast<bf16*>(C), lda, nwg, stamps);
}

int xg_gemm3_stamp_words() { return xg3::STAMP_WORDS; }

// ---------------------------------------------------------------------------
// xg_gemm4: xg_gemm3 as a persistent tile stream (docs/KERNELS.md lesson 24).
// Tile, waves, swizzled LDS image, fragment reads, MFMA order, bias add and
// rounding are xg_gemm3's, so the output equals it byte for byte. What
// changed is everything BETWEEN tiles: min(tiles, 2 x CUs) workgroups each
// walk their share of the tiles (n fastest; an XCD's workgroups hold one
// contiguous range and stride through it together, so an m-tile's six
// n-tiles still meet in one L2), and the k-slices of a workgroup's whole
// walk form ONE stream: slice s + 2 is issued
// before burst s and slice s + 1 committed after it whether or not a tile
// ends in between. The next tile's first two slices are in flight under
// this tile's last two bursts and its epilogue; the prologue's exposed load
// latency is paid once per workgroup instead of once per tile.
//
// Tile boundary. KB is even: a tile's last slice is read from buffer 1 and
// the next tile's slice 0 is committed to buffer 0 in the usual place. The
// epilogue's four 8 KB wave images therefore live in buffer 1 only:
//   barrier (end of the last slice: every wave is done reading buffer 1)
//   -> each wave writes and reads back ITS OWN image (LDS operations of one
//      wave execute in order; no other wave touches that image)
//   -> barrier (every image read has landed)
//   -> next tile: burst 0 from buffer 0, then commit of slice 1 INTO buffer 1.
// The bias values are loaded at the head of the tile, not in the epilogue,
// where the load would queue behind two slices of staged loads.
namespace xg4 {

using xg3::BK;
using xg3::BM;
using xg3::BN;
using xg3::NT;
using xg3::TILE_BYTES;
using xg3::WAVES;
using xg3::XN;
using xg3::swz;

template <int KP>
__global__ __launch_bounds__(WAVES * 64, 2) void xg_gemm4_kernel(
    const bf16* __restrict__ A,     // (M, KP) rows strided by lda (16-B rows)
    const bf16* __restrict__ Bt,    // (768, KP) row-major = B^T, zero-padded
    const bf16* __restrict__ bias,  // (768)
    bf16* __restrict__ C,           // (M, 768)
    int lda, int tq, int tr) {      // tiles / grid, tiles % grid
    constexpr int KB = KP / BK;
    static_assert(KB >= 2 && KB % 2 == 0, "a tile must end in buffer 1");
    // [buf][A | B][16 KB]; buffer 1 doubles as the 4 x 8 KB wave images
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * 2 * TILE_BYTES];

    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;
    const int wm = wid >> 1, wn = wid & 1;

    // xg_gemm3's bijective XCD remap over the persistent grid: workgroups
    // that share blockIdx % 8 share an XCD and are numbered w0 .. w0 + gx - 1.
    // Balanced runs (the first tr workgroups tq + 1 tiles, the rest tq) give
    // that XCD the contiguous tile range [ta, tb); inside it workgroup j
    // takes every gx-th tile from ta + j. At any moment the XCD's workgroups
    // are therefore on ~gx CONSECUTIVE tiles, as under xg_gemm3's dispatch
    // order: an m-tile's six n-tiles run side by side in one L2. (One
    // contiguous run per workgroup puts gx different m-tiles in flight per
    // XCD, 64 x 64 KB against 4 MB of L2, and measured 1.28x SLOWER than
    // xg_gemm3 at M = 92,160.)
    const int nwg = gridDim.x;
    const int orig = blockIdx.x;
    const int xcd = orig & 7;
    const int q8 = nwg >> 3, r8 = nwg & 7;
    const int w0 = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
    const int gx = q8 + (xcd < r8 ? 1 : 0);
    const int ta = w0 * tq + (w0 < tr ? w0 : tr);
    const int tb = (w0 + gx) * tq + (w0 + gx < tr ? w0 + gx : tr);
    const int t0 = ta + (orig >> 3);
    if (t0 >= tb) return;  // a spare workgroup touches nothing

    f32x4 acc[4][4];
    bf16x8 ra[2][4], rb[2][4];
    const int s_row = tid >> 3, s_q = tid & 7;
    const int s_off = swz(s_row, s_q);
    auto a_of = [&](int t) {
        return A + (size_t)((t / NT) * BM + s_row) * lda + s_q * 8;
    };
    auto b_of = [&](int t) {
        return Bt + (size_t)((t % NT) * BN + s_row) * KP + s_q * 8;
    };
    auto issue = [&](const bf16* a_src, const bf16* b_src, int kq,
                     bf16x8(&va)[4], bf16x8(&vb)[4]) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            va[p] = *reinterpret_cast<const bf16x8*>(
                a_src + (size_t)p * 32 * lda + kq * BK);
            vb[p] = *reinterpret_cast<const bf16x8*>(
                b_src + (size_t)p * 32 * KP + kq * BK);
        }
    };
    auto commit = [&](int buf, bf16x8(&va)[4], bf16x8(&vb)[4]) {
        unsigned char* ab = lds + buf * 2 * TILE_BYTES;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<bf16x8*>(ab + p * 32 * 128 + s_off) = va[p];
            *reinterpret_cast<bf16x8*>(ab + TILE_BYTES + p * 32 * 128 + s_off) =
                vb[p];
        }
    };
    const int fsw = (lcol >> 1) & 7;
    const int fa_off = (wm * 64 + lcol) * 128;
    const int fb_off = TILE_BYTES + (wn * 64 + lcol) * 128;
    auto mfma_step = [&](int buf) {
        const unsigned char* ab = lds + buf * 2 * TILE_BYTES;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            const int ch = ((kh * 4 + lrow) ^ fsw) << 4;
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = *reinterpret_cast<const bf16x8*>(
                    ab + fa_off + t * 16 * 128 + ch);
                wf[t] = *reinterpret_cast<const bf16x8*>(
                    ab + fb_off + t * 16 * 128 + ch);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[mt][nt] = mfma16x16x32(wf[nt], af[mt], acc[mt][nt]);
        }
    };

    // One tile of the walk. On entry slice 0 is in buffer 0 (committed and
    // barriered) and slice 1 is in flight in set 1; on exit the same holds
    // for tile `nxt`. The last tile of a run names itself as `nxt`: its
    // look-ahead loads re-read valid lines of its own tile and are never
    // used, which keeps every load of the stream out of a branch.
    unsigned char* img = lds + 2 * TILE_BYTES + wid * (64 * 128);
    const int r8l = lane >> 3, j8 = lane & 7;
    auto tile = [&](int t, int nxt) {
        const int m0 = (t / NT) * BM, n0 = (t % NT) * BN;
        const bf16* a_cur = a_of(t);
        const bf16* b_cur = b_of(t);
        const bf16* a_nxt = a_of(nxt);
        const bf16* b_nxt = b_of(nxt);
        bf16x4 bv[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            bv[nt] = *reinterpret_cast<const bf16x4*>(
                reinterpret_cast<const __bf16*>(bias) + n0 + wn * 64 + nt * 16 +
                lrow * 4);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kq = 0; kq < KB; ++kq) {
            if (kq + 2 < KB)
                issue(a_cur, b_cur, kq + 2, ra[kq & 1], rb[kq & 1]);
            else
                issue(a_nxt, b_nxt, kq + 2 - KB, ra[kq & 1], rb[kq & 1]);
            // pin the loads ahead of the burst: left alone, the scheduler
            // sinks a tile's last look-ahead below the epilogue and the
            // next tile opens on vmcnt(0) (lesson 23 again)
            __builtin_amdgcn_sched_barrier(0);
            mfma_step(kq & 1);
            commit((kq + 1) & 1, ra[(kq + 1) & 1], rb[(kq + 1) & 1]);
            __syncthreads();
        }
        // epilogue: xg_gemm3's, through this wave's image in buffer 1
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int nl = nt * 16 + lrow * 4;
            float br[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) br[i] = (float)bv[nt][i];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int row = mt * 16 + lcol;
                alignas(8) bf16 o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = f2bf(acc[mt][nt][i] + br[i]);
                *reinterpret_cast<uint64_t*>(
                    img + row * 128 + (((nl >> 3) ^ (row & 7)) << 4) +
                    (nl & 4) * 2) = *reinterpret_cast<const uint64_t*>(o);
            }
        }
        bf16* cdst = C + (size_t)(m0 + wm * 64 + r8l) * XN + n0 + wn * 64 + j8 * 8;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int row = p * 8 + r8l;
            *reinterpret_cast<bf16x8*>(cdst + (size_t)p * 8 * XN) =
                *reinterpret_cast<const bf16x8*>(
                    img + row * 128 + ((j8 ^ (row & 7)) << 4));
        }
        __syncthreads();  // image reads landed before slice 1 enters buffer 1
    };

    // the walk's only full drain: slice 0 of the first tile
    issue(a_of(t0), b_of(t0), 0, ra[0], rb[0]);
    issue(a_of(t0), b_of(t0), 1, ra[1], rb[1]);
    commit(0, ra[0], rb[0]);
    __syncthreads();
    // One loop, first tile included. (Peeling the first tile lets the loop
    // count the previous epilogue's stores, vmcnt(27..20) instead of
    // (19..12) at a tile's first commit; it measured 1-3% SLOWER.)
    for (int t = t0; t < tb; t += gx) tile(t, t + gx < tb ? t + gx : t);
}

}  // namespace xg4

// ---------------------------------------------------------------------------
// xg_gemm4w: the K = 256 projections with W STATIONARY (lesson 24). The stamps
// of xg_gemm3 and the stream form above agree that these kernels are bound by
// what a CU can pull out of L2, not by what is serial in a tile: so fetch
// less. One 512-thread workgroup per CU (8 waves, 4 (m) x 2 (n), 64 x 64
// each) is bound to ONE 128-column n-tile, loads that tile's W (128 x 256
// bf16, 64 KB) into LDS once, and then streams 256-row A slices through two
// 32 KB buffers with the cross-tile slice stream of xg_gemm4: no B staging
// at all, global fetch per output halved, LDS array work per MFMA cycle
// 0.75 of xg_gemm3's. Arithmetic, fragment layout and rounding are
// xg_gemm3's: the output equals it byte for byte.
//
// Placement. The grid is 6 x G workgroups, G "walkers" of m-tiles per
// n-tile. With G a multiple of 8, workgroup b runs on XCD b % 8; that XCD
// gets a contiguous eighth of the m-tiles and G / 8 walkers per n-tile, and
// its six workgroups of one walker are on the SAME m-tile at the same time:
// the A tile leaves HBM once and is read six times from that XCD's L2.
// Default G = 8 x (CUs per XCD / 6) = 40: 240 of 256 CUs, 9 exact rounds at
// M = 92,160 (16 CUs idle buys zero tail). Any other G (tests) walks
// m = g, g + G, ... with no XCD structure.
//
// Epilogue. A tile ends in A buffer 1 (KB = 4); buffer 0 is already being
// filled with the next tile's slice 0. Eight 8 KB images do not fit in one
// 32 KB buffer, so each wave goes through a 4 KB image twice (32 rows each).
// The image is wave-private and one wave's LDS operations execute in order,
// so neither the write -> read nor the read -> rewrite needs a barrier; one
// barrier after the last read precedes the commit of slice 1 into buffer 1.
namespace xg4w {

using xg3::BK;
using xg3::BN;
using xg3::NT;
using xg3::TILE_BYTES;
using xg3::XN;
using xg3::swz;

constexpr int KP = 256;
constexpr int KB = KP / BK;             // 4: even, a tile ends in buffer 1
constexpr int BMW = 256;                // C rows per tile
constexpr int WAVES = 8;                // 4 (m) x 2 (n)
constexpr int A_BYTES = BMW * BK * 2;   // one A slice: 32 KB
constexpr int W_BYTES = KB * TILE_BYTES;  // the W tile, [kq][128 rows][128 B]

__global__ __launch_bounds__(WAVES * 64, 2) void xg_gemm4w_kernel(
    const bf16* __restrict__ A,     // (M, 256) rows strided by lda (16-B rows)
    const bf16* __restrict__ Bt,    // (768, 256) row-major = B^T
    const bf16* __restrict__ bias,  // (768)
    bf16* __restrict__ C,           // (M, 768)
    int lda, int mtiles, int groups) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[W_BYTES + 2 * A_BYTES];
    unsigned char* abuf = lds + W_BYTES;

    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;
    const int wm = wid >> 1, wn = wid & 1;

    const int b = blockIdx.x;
    int n_t, m_first, m_step, m_end;
    if ((groups & 7) == 0) {
        const int xcd = b & 7, j = b >> 3;
        const int q = mtiles >> 3, r = mtiles & 7;
        const int ta = xcd * q + (xcd < r ? xcd : r);
        n_t = j % NT;
        m_step = groups >> 3;
        m_first = ta + j / NT;
        m_end = ta + q + (xcd < r ? 1 : 0);
    } else {
        n_t = b % NT;
        m_step = groups;
        m_first = b / NT;
        m_end = mtiles;
    }
    if (m_first >= m_end) return;  // a spare workgroup touches nothing
    const int n0 = n_t * BN;

    // W tile -> LDS, once: 32 lanes read one full 512-B row of Bt
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = (tid >> 5) + 16 * i, cc = tid & 31;
        *reinterpret_cast<bf16x8*>(lds + (cc >> 3) * TILE_BYTES + swz(row, cc & 7)) =
            *reinterpret_cast<const bf16x8*>(Bt + (size_t)(n0 + row) * KP + cc * 8);
    }
    bf16x4 bv[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
        bv[nt] = *reinterpret_cast<const bf16x4*>(
            reinterpret_cast<const __bf16*>(bias) + n0 + wn * 64 + nt * 16 +
            lrow * 4);

    f32x4 acc[4][4];
    bf16x8 ra[2][4];
    const int s_row = tid >> 3, s_q = tid & 7;  // + p * 64 rows: same swizzle
    const int s_off = swz(s_row, s_q);
    auto a_of = [&](int m) {
        return A + (size_t)(m * BMW + s_row) * lda + s_q * 8;
    };
    auto issue = [&](const bf16* a_src, int kq, bf16x8(&va)[4]) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            va[p] = *reinterpret_cast<const bf16x8*>(
                a_src + (size_t)p * 64 * lda + kq * BK);
    };
    auto commit = [&](int buf, bf16x8(&va)[4]) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            *reinterpret_cast<bf16x8*>(abuf + buf * A_BYTES + p * 64 * 128 +
                                       s_off) = va[p];
    };
    const int fsw = (lcol >> 1) & 7;
    const int fa_off = (wm * 64 + lcol) * 128;
    const int fb_off = (wn * 64 + lcol) * 128;
    auto mfma_step = [&](int buf, int kq) {
        const unsigned char* ab = abuf + buf * A_BYTES;
        const unsigned char* wb = lds + kq * TILE_BYTES;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            const int ch = ((kh * 4 + lrow) ^ fsw) << 4;
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = *reinterpret_cast<const bf16x8*>(
                    ab + fa_off + t * 16 * 128 + ch);
                wf[t] = *reinterpret_cast<const bf16x8*>(
                    wb + fb_off + t * 16 * 128 + ch);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[mt][nt] = mfma16x16x32(wf[nt], af[mt], acc[mt][nt]);
        }
    };

    unsigned char* img = abuf + A_BYTES + wid * (32 * 128);
    const int r8l = lane >> 3, j8 = lane & 7;
    // as xg_gemm4's tile: slice 0 committed and slice 1 in flight on entry,
    // the same for m-tile `nxt` on exit; the last tile names itself
    auto tile = [&](int m, int nxt) {
        const bf16* a_cur = a_of(m);
        const bf16* a_nxt = a_of(nxt);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kq = 0; kq < KB; ++kq) {
            if (kq + 2 < KB)
                issue(a_cur, kq + 2, ra[kq & 1]);
            else
                issue(a_nxt, kq + 2 - KB, ra[kq & 1]);
            __builtin_amdgcn_sched_barrier(0);  // loads stay ahead of the burst
            mfma_step(kq & 1, kq);
            commit((kq + 1) & 1, ra[(kq + 1) & 1]);
            __syncthreads();
        }
        bf16* cdst = C + (size_t)(m * BMW + wm * 64 + r8l) * XN + n0 +
                     wn * 64 + j8 * 8;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int nl = nt * 16 + lrow * 4;
                float br[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) br[i] = (float)bv[nt][i];
#pragma unroll
                for (int mh = 0; mh < 2; ++mh) {
                    const int row = mh * 16 + lcol;
                    alignas(8) bf16 o[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        o[i] = f2bf(acc[h * 2 + mh][nt][i] + br[i]);
                    *reinterpret_cast<uint64_t*>(
                        img + row * 128 + (((nl >> 3) ^ (row & 7)) << 4) +
                        (nl & 4) * 2) = *reinterpret_cast<const uint64_t*>(o);
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int row = p * 8 + r8l;
                *reinterpret_cast<bf16x8*>(cdst + (size_t)(h * 32 + p * 8) * XN) =
                    *reinterpret_cast<const bf16x8*>(
                        img + row * 128 + ((j8 ^ (row & 7)) << 4));
            }
        }
        __syncthreads();  // image reads landed before slice 1 enters buffer 1
    };

    issue(a_of(m_first), 0, ra[0]);
    issue(a_of(m_first), 1, ra[1]);
    commit(0, ra[0]);
    __syncthreads();  // also publishes the W tile
    for (int m = m_first; m < m_end; m += m_step)
        tile(m, m + m_step < m_end ? m + m_step : m);
}

}  // namespace xg4w

static int xg4_cus_cached = 0;

// CU count of the current device, queried once (never under stream capture:
// ServeSlot asks for it when a slot is built)
int xg_gemm4_cus() {
    if (xg4_cus_cached == 0) {
        int dev = 0, cus = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                    dev);
        xg4_cus_cached = cus > 0 ? cus : 256;
    }
    return xg4_cus_cached;
}

// Same contract as xg_gemm3. max_wgs > 0 caps the grid (tests force long
// walks at small M with it); 0 is the default, 2 x CU count: the two
// workgroups per CU that 64 KB of LDS and 2 waves per SIMD allow.
void xg_gemm4(const void* A, int lda, const void* Bt, const void* bias,
              void* C, int M, int KP, int max_wgs, hipStream_t stream) {
    const int tiles = (M / xg4::BM) * xg4::NT;
    const int cap = max_wgs > 0 ? max_wgs : 2 * xg_gemm4_cus();
    const int nwg = tiles < cap ? tiles : cap;
    dim3 grid(nwg), block(xg4::WAVES * 64);
    if (KP == 512)
        hipLaunchKernelGGL((xg4::xg_gemm4_kernel<512>), grid, block, 0, stream,
                           static_cast<const bf16*>(A),
                           static_cast<const bf16*>(Bt),
                           static_cast<const bf16*>(bias),
                           static_cast<bf16*>(C), lda, tiles / nwg, tiles % nwg);
    else if (KP == 256)
        hipLaunchKernelGGL((xg4::xg_gemm4_kernel<256>), grid, block, 0, stream,
                           static_cast<const bf16*>(A),
                           static_cast<const bf16*>(Bt),
                           static_cast<const bf16*>(bias),
                           static_cast<bf16*>(C), lda, tiles / nwg, tiles % nwg);
}

// The W-stationary form: KP = 256 and M % 256 == 0 only (the callers fall
// back to xg_gemm3 otherwise). max_wgs > 0 caps the grid at 6 x
// max(1, max_wgs / 6) workgroups; 0 is 6 x 8 x (CUs per XCD / 6).
int xg_gemm4w_tile_m() { return xg4w::BMW; }

static int xg4w_default_groups() {
    const int g = 8 * (xg_gemm4_cus() / 8 / xg4w::NT);
    return g > 0 ? g : 1;
}

// where the serving slots take this form: whole tiles and at least eight
// rounds per walker (measured at nine; it loses at two)
bool xg_gemm4w_pays(int M) {
    return M % xg4w::BMW == 0 && M / xg4w::BMW >= 8 * xg4w_default_groups();
}

void xg_gemm4w(const void* A, int lda, const void* Bt, const void* bias,
               void* C, int M, int max_wgs, hipStream_t stream) {
    const int mtiles = M / xg4w::BMW;
    int groups = max_wgs > 0 ? max_wgs / xg4w::NT : xg4w_default_groups();
    if (groups < 1) groups = 1;
    if (groups > mtiles) groups = mtiles;
    hipLaunchKernelGGL(xg4w::xg_gemm4w_kernel, dim3(groups * xg4w::NT),
                       dim3(xg4w::WAVES * 64), 0, stream,
                       static_cast<const bf16*>(A), static_cast<const bf16*>(Bt),
                       static_cast<const bf16*>(bias), static_cast<bf16*>(C),
                       lda, mtiles, groups);
}

int atb_splitk_nslices(int K) {
    return (K + gemmatb::KSLICE - 1) / gemmatb::KSLICE;
}

void atb_splitk_ld(const void* A, int lda, const void* B, int ldb,
                   float* ws, float* C, int M, int N, int K,
                   hipStream_t stream) {
    const int S = atb_splitk_nslices(K);
    dim3 grid(S, (M + gemmatb::BM - 1) / gemmatb::BM,
              (N + gemmatb::BN - 1) / gemmatb::BN);
    hipLaunchKernelGGL(gemmatb::atb_splitk_kernel, grid,
                       dim3(gemmatb::WAVES * 64), 0, stream,
                       static_cast<const bf16*>(A), static_cast<const bf16*>(B),
                       ws, M, N, K, lda, ldb);
    const int64_t MN = (int64_t)M * N;
    // ceil over the 4-element stride: floor(MN/4) left the last MN%4
    // outputs unwritten for odd shapes
    hipLaunchKernelGGL(gemmatb::slice_sum_kernel,
                       dim3(((MN + 3) / 4 + 255) / 256), dim3(256), 0, stream,
                       ws, C, S, MN);
}

void atb_splitk(const void* A, const void* B, float* ws, float* C, int M,
                int N, int K, hipStream_t stream) {
    atb_splitk_ld(A, M, B, N, ws, C, M, N, K, stream);
}

// column sums: out[n] = sum_k X[k*ldx + n], bf16 in / fp32 out. Replaces
// the ones-vector hipBLASLt GEMVs in the weight-grad path (each a separate
// aten launch; the whole weight-grad section is now raw kernel calls —
// the aten form cost ~1.3 ms of HOST enqueue per train step, tr5 trace).
namespace colsum {

__global__ __launch_bounds__(256, 4) void colsum_kernel(
    const bf16* __restrict__ X, float* __restrict__ out, int ldx, int K,
    int N, int ksplit) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int k0 = blockIdx.y * ksplit;
    const int k1 = min(K, k0 + ksplit);
    // 8 independent accumulators with the loads batched per iteration:
    // a single-accumulator runtime loop compiled to load->wait->add per
    // element (~340 us measured); this form keeps 8 loads in flight
    float acc[8] = {0.f};
    int k = k0;
    for (; k + 8 <= k1; k += 8) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            v[q] = bf2f(X[(size_t)(k + q) * ldx + n]);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] += v[q];
    }
    for (; k < k1; ++k) acc[0] += bf2f(X[(size_t)k * ldx + n]);
    // plain store of this k-split's partial (no memset, no atomics: a
    // hipMemsetAsync enqueued just before front_bwd stretched to 659 us
    // of CU starvation — tr6 trace)
    out[(size_t)blockIdx.y * N + n] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) +
                                      ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

__global__ __launch_bounds__(256, 4) void colsum_reduce_kernel(
    const float* __restrict__ part, float* __restrict__ out, int N,
    int ksp) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float acc = 0.f;
    for (int q = 0; q < ksp; ++q) acc += part[(size_t)q * N + n];
    out[n] = acc;
}

}  // namespace colsum

void colsum_f32(const void* X, int ldx, int K, int N, float* out,
                float* part, hipStream_t stream) {
    const int KSP = 32;
    const int ksplit = (K + KSP - 1) / KSP;
    hipLaunchKernelGGL(colsum::colsum_kernel,
                       dim3((N + 255) / 256, KSP), dim3(256), 0, stream,
                       static_cast<const bf16*>(X), part, ldx, K, N, ksplit);
    hipLaunchKernelGGL(colsum::colsum_reduce_kernel, dim3((N + 255) / 256),
                       dim3(256), 0, stream, part, out, N, KSP);
}

}  // namespace rk
