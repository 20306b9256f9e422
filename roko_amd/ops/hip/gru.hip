// Persistent bidirectional GRU layer forward + BPTT backward for gfx950.
//
// Replaces the reference's cuDNN GRU (rnn_model.py:57).
// Design (SURVEY.md §7 hard part (a), re-thought for CDNA4):
//   * the input projections W_ih·x + b_ih for ALL T steps are one plain GEMM
//     done on the host side (hipBLASLt via torch.matmul) — this kernel gets
//     the precomputed per-step gate inputs `xg`;
//   * ONE kernel launch runs the full T-step recurrence of a layer: grid =
//     (B/MBT batch tiles) x (2 directions); each workgroup owns MBT batch
//     rows (default 16 — the gate phase is VALU-issue-floor bound, so the
//     smallest MFMA-viable tile halves the per-step wall AND doubles the
//     workgroup supply for serving packing; docs/KERNELS.md lesson 18)
//     whose hidden state lives in fp32 registers with a bf16 mirror in LDS
//     as the MFMA A-operand — no per-step launches, no grid-wide sync;
//   * 8 waves per workgroup = two per SIMD: the matrix and VALU pipes are
//     separate and arbitrate between co-resident waves, so one wave's
//     dependent gate math overlaps its partner's MFMAs;
//   * U = weight_hh^T fragments are loaded ONCE into registers (12 bf16x8
//     per wave) and reused for all T steps; per-step work is 12 (MBT=16)
//     or 24 (MBT=32) v_mfma_f32_16x16x32_bf16 per wave + fused
//     sigmoid/tanh gate math;
//   * the hidden-state mirror is double-buffered in LDS, so each step needs
//     exactly ONE __syncthreads(): MFMAs read h[cur] while gate math writes
//     h[cur^1]; the barrier publishes h[cur^1] for the next step;
//   * per-step xg tiles (32x384 or 16x384 bf16) are double-buffered through
//     LDS; the source issues the loads for step t+2 at the top of step t and
//     writes them to LDS a step later (issue-early / write-late, T14). That
//     is the intent, not what runs: the loads sit behind runtime branches
//     (`ti + 2 < T`, the dbg probes), so the compiler must drain them where
//     it stands — the emitted step loop waits vmcnt(0), or vmcnt(2/1/0),
//     a few instructions after issuing them, and one xg load latency is
//     exposed in every step (docs/KERNELS.md lesson 23);
//   * eval (cache == nullptr, B % 16 == 0) runs gru_eval2_kernel below
//     instead: operands swapped so a lane's gate inputs are contiguous in
//     xg and go straight to registers, with a prefetch whose counted waits
//     were read from the ISA. gru_layer_fwd_kernel<false, 0, 16> stays as
//     its byte-exact reference (ROKO_GRU_EVAL=v1, or impl=1).
//
// PyTorch GRU semantics (gate order r,z,n in weight rows; n-gate bias split):
//   r = sigmoid(xr + U_r h + bhh_r)
//   z = sigmoid(xz + U_z h + bhh_z)
//   n = tanh(xn + r * (U_n h + bhh_n))        (xg already contains b_ih)
//   h' = (1 - z) * n + z * h

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "api.h"
#include "common.h"

namespace rk {

constexpr int H = 128;       // hidden size (config.HIDDEN_SIZE)
constexpr int G3 = 3 * H;    // gate rows
constexpr int MB = 32;       // batch rows per workgroup
constexpr int WAVES = 8;     // 512 threads, two waves per SIMD: a wave's
                             // dependent gate VALU hides under its partner's
                             // MFMAs (MI355X_MICROARCH.md "Two waves per
                             // SIMD" — the pipes are separate and arbitrate)
constexpr int HPAD = H + 8;  // LDS row padding (bank-conflict fix)
constexpr int XCH = MB * G3 / (WAVES * 64 * 8);  // xg chunks per thread (3)

constexpr int XKP = 512;        // max padded input width for the fused xg GEMM
constexpr int XLD = XKP + 8;    // x-stage LDS row stride (bank pad)

// FUSEXG (serving variant): the input-projection GEMM xg = x·W_ihᵀ + b_ih
// runs as PHASE 1 of this kernel instead of a separate hipBLASLt launch.
// Rationale (profiles/infer_r02_v3_kernel_stats.csv): hipBLASLt runs the
// (11520, 768, K<=500) GEMM at ~543 TF/s on ~225 workgroups — ~105 CU·us
// per window of aggregate chip time, tied with the front as the top serving
// cost. Here each of the 8 workgroups computes its OWN (90x32, 384) slice
// with the W slice L2-resident and reused across all 90 steps, at a small
// fraction of the aggregate CU time; the per-chain latency rises (~+60 us),
// which deep pipelining absorbs. Not used by training: there the step's
// LATENCY is the metric and 225 workgroups beat 8.
template <bool TRAIN, int FUSEKP = 0, int MBT = MB>
// FUSEKP: 0 = xg precomputed; 256/512 = in-kernel xg GEMM width.
// MBT: batch rows per workgroup. 32 is the default; 16 (eval only) doubles
// the workgroup count and HALVES each thread's gate-chain count — the gate
// phase sits at the 2-wave VALU-issue floor, so per-step time drops with
// per-thread instruction count, and b=128 serving gets 16 WGs of supply.
__global__ __launch_bounds__(WAVES * 64, 2) void gru_layer_fwd_kernel(
    const bf16* __restrict__ xg,   // (T, B, 2, 3H)  W_ih·x + b_ih
                                   // (FUSEXG: workspace this kernel fills)
    const bf16* __restrict__ u,    // (2, 3H, H)     weight_hh
    const float* __restrict__ bhh, // (2, 3H)        bias_hh
    bf16* __restrict__ hseq,       // (T, B, 2, H)   output
    bf16* __restrict__ cache,      // (T, B, 2, H, 4) [r z n hgn] or nullptr
    int T, int B,
    uint32_t dbg,   // timing bisection: 1 no hseq store, 2 no cache store,
                    // 4 no gate VALU, 8 no xg staging, 16 no MFMA
    const bf16* __restrict__ x = nullptr,     // (T, B, IN) layer input
    const bf16* __restrict__ w_ih_p = nullptr,  // (768, KP) row-padded W_ih
    const bf16* __restrict__ b_ih = nullptr,   // (768)
    int IN = 0) {
    constexpr bool FUSEXG = FUSEKP > 0;
    static_assert(!FUSEXG || MBT == 32, "fused xg path is MB=32 only");
    constexpr int MT = MBT / 16;         // 16-row m-subtiles per thread
    constexpr int CW = (MBT == 32) ? 8 : 4;  // staging chunk width (bf16)
    constexpr int XCHT = MBT * G3 / (WAVES * 64 * CW);  // xg chunks/thread
    using xvec = std::conditional_t<CW == 8, bf16x8, bf16x4>;
    constexpr int XLDK = FUSEXG ? FUSEKP + 8 : 1;
    __shared__ struct {
        bf16 h[2][MBT][HPAD];        // double-buffered hidden-state mirror
        bf16 xgb[2][MBT][G3];        // double-buffered step gate inputs
        bf16 x_st[FUSEXG ? 2 : 1][FUSEXG ? MBT : 1][XLDK];
    } lds;

    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * MBT;
    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int j0 = wid * 16;         // this wave's 16 hidden columns
    const int lrow = lane >> 4;      // fragment row group (0..3)
    const int lcol = lane & 15;      // fragment column
    // static priority for the second-dispatched wave half: the younger
    // wave on each SIMD loses VALU arbitration at every barrier-paced
    // segment (MI355X_MICROARCH.md "Two waves per SIMD" item 4)
    if (wid >= WAVES / 2) __builtin_amdgcn_s_setprio(1);

    // ---- PHASE 1 (FUSEXG): xg[t, b0:b0+MB, dir, :] = x·Wᵀ + b_ih ----------
    if constexpr (FUSEXG) {
        // x[t] tile (MB, KP) double-buffered through LDS; W B-fragments read
        // straight from L2 ((768, KP) row-major = [col][k], so the B-frag
        // load is the A-frag address pattern). Wave owns 3 n-tiles
        // (nt = wid + 8s) x 2 m-tiles; one barrier per t. KP is a template
        // constant: the k-loop fully unrolls and the W/A fragment loads for
        // kb+1 issue under kb's MFMAs (a runtime trip count compiled to a
        // serial load->mfma->load chain — 1.47 ms/layer vs ~210 split).
        constexpr int KB = FUSEKP / 32;
        auto stage_x = [&](int t, int buf) {
            const bf16* src = x + ((size_t)t * B + b0) * IN;
#pragma unroll
            for (int p = 0; p < MBT * FUSEKP / 4 / (WAVES * 64); ++p) {
                const int c = p * WAVES * 64 + tid;
                const int row = (c * 4) / FUSEKP, col = (c * 4) % FUSEKP;
                uint64_t v = 0;  // 4 bf16 (zero pads cols IN..KP)
                if (col + 4 <= IN)
                    v = *reinterpret_cast<const uint64_t*>(
                        src + (size_t)row * IN + col);
                *reinterpret_cast<uint64_t*>(&lds.x_st[buf][row][col]) = v;
            }
        };
        float bih_reg[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int col = (wid + 8 * s) * 16 + lcol;
            bih_reg[s] = b_ih ? bf2f(b_ih[dir * G3 + col]) : 0.f;
        }
        const int col0w = dir * G3 + wid * 16;
        stage_x(0, 0);
        __syncthreads();
        for (int t = 0; t < T; ++t) {
            if (t + 1 < T) stage_x(t + 1, (t + 1) & 1);
            f32x4 acc[3][2];
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[s][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            bf16x8 wfA[3], wfB[3], a0A, a1A, a0B, a1B;
#pragma unroll
            for (int s = 0; s < 3; ++s)
                wfA[s] = global_load_a_frag(w_ih_p, col0w + s * 128, 0,
                                            FUSEKP);
            a0A = lds_load_a_frag(&lds.x_st[t & 1][0][0], 0, 0, XLDK);
            a1A = lds_load_a_frag(&lds.x_st[t & 1][0][0], 16, 0, XLDK);
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                bf16x8(&wc)[3] = (kb & 1) ? wfB : wfA;
                bf16x8(&wn)[3] = (kb & 1) ? wfA : wfB;
                const bf16x8 a0 = (kb & 1) ? a0B : a0A;
                const bf16x8 a1 = (kb & 1) ? a1B : a1A;
                if (kb + 1 < KB) {
#pragma unroll
                    for (int s = 0; s < 3; ++s)
                        wn[s] = global_load_a_frag(w_ih_p, col0w + s * 128,
                                                   (kb + 1) * 32, FUSEKP);
                    ((kb & 1) ? a0A : a0B) = lds_load_a_frag(
                        &lds.x_st[t & 1][0][0], 0, (kb + 1) * 32, XLDK);
                    ((kb & 1) ? a1A : a1B) = lds_load_a_frag(
                        &lds.x_st[t & 1][0][0], 16, (kb + 1) * 32, XLDK);
                }
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    acc[s][0] = mfma16x16x32(a0, wc[s], acc[s][0]);
                    acc[s][1] = mfma16x16x32(a1, wc[s], acc[s][1]);
                }
            }
            // epilogue: + b_ih, scalar bf16 stores into the xg workspace
            // (xg is a mutable workspace in the FUSEXG instantiation)
            bf16* dst = const_cast<bf16*>(xg) +
                        (((size_t)t * B + b0) * 2 + dir) * G3;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int col = (wid + 8 * s) * 16 + lcol;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = mt * 16 + lrow * 4 + i;
                        dst[(size_t)row * 2 * G3 + col] =
                            f2bf(acc[s][mt][i] + bih_reg[s]);
                    }
            }
            __syncthreads();
        }
        // all xg stores must land before phase 2 reads them back
        __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) & lgkmcnt(0)
        __syncthreads();
    }

    // ---- load U fragments (kept in registers for all T steps) -------------
    // B-fragment for gates = h·U^T: B[k][col] = U[gate*H + j0 + 16ct + col][k]
    bf16x8 ufrag[3][4];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int jrow = g * H + j0 + lcol;
            const int k = kb * 32 + 8 * lrow;
            ufrag[g][kb] = *reinterpret_cast<const bf16x8*>(
                u + (size_t)dir * G3 * H + (size_t)jrow * H + k);
        }
    float bhh_reg[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) bhh_reg[g] = bhh[dir * G3 + g * H + j0 + lcol];

    // ---- zero hidden state -------------------------------------------------
    float hreg[MT][4];  // [mt][i] fp32 master copy, fragment-shaped
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) hreg[mt][i] = 0.0f;
    for (int e = tid; e < MBT * HPAD; e += WAVES * 64) lds.h[0][0][e] = f2bf(0.0f);

    const int stp = (dir == 0) ? 1 : -1;
    const int tfirst = (dir == 0) ? 0 : T - 1;
    auto xg_src = [&](int t) {
        return xg + (((size_t)t * B + b0) * 2 + dir) * G3;
    };

    // ---- prologue: xg[t0] -> LDS buffer 0; xg[t1] -> stage registers ------
    {
        const bf16* src = xg_src(tfirst);
#pragma unroll
        for (int p = 0; p < XCHT; ++p) {
            int e = (p * WAVES * 64 + tid) * CW;
            int row = e / G3, col = e % G3;
            *reinterpret_cast<xvec*>(&lds.xgb[0][row][col]) =
                *reinterpret_cast<const xvec*>(src + (size_t)row * 2 * G3 + col);
        }
    }
    xvec stageA[XCHT], stageB[XCHT];
    if (T > 1) {
        const bf16* src = xg_src(tfirst + stp);
#pragma unroll
        for (int p = 0; p < XCHT; ++p) {
            int e = (p * WAVES * 64 + tid) * CW;
            int row = e / G3, col = e % G3;
            stageA[p] =
                *reinterpret_cast<const xvec*>(src + (size_t)row * 2 * G3 + col);
        }
    }
    __syncthreads();

    // ---- T-step recurrence, ONE barrier per step --------------------------
    // The loop is unrolled by TWO with alternating stage register sets so no
    // register copy ever waits on the loads issued in the SAME step: the xg
    // write into LDS only touches registers loaded a FULL step earlier (the
    // v3 kernel's stage rotation copy forced an end-of-step vmcnt(0) on
    // loads ~200 cycles old — profiles/pmc_gru_r01.txt's 36% SQ_WAIT_ANY).
    auto body = [&](int ti, int curp, xvec (&st_wr)[XCHT],
                    xvec (&st_ld)[XCHT]) {
        const int t = tfirst + stp * ti;
        // issue xg[t+2] loads FIRST (they retire next step), then write the
        // staged xg[t+1] (loaded last step) into the back LDS buffer
        if (ti + 2 < T && !(dbg & 8u)) {
            const bf16* src = xg_src(t + 2 * stp);
#pragma unroll
            for (int p = 0; p < XCHT; ++p) {
                int e = (p * WAVES * 64 + tid) * CW;
                int row = e / G3, col = e % G3;
                st_ld[p] =
                    *reinterpret_cast<const xvec*>(src + (size_t)row * 2 * G3 + col);
            }
        }
        if (ti + 1 < T && !(dbg & 8u)) {
#pragma unroll
            for (int p = 0; p < XCHT; ++p) {
                int e = (p * WAVES * 64 + tid) * CW;
                int row = e / G3, col = e % G3;
                *reinterpret_cast<xvec*>(&lds.xgb[curp ^ 1][row][col]) = st_wr[p];
            }
        }

        // gates_h = h · U^T  (24 MFMA per wave, A-frags shared 3-ways)
        f32x4 acc[MT][3];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[mt][g] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!(dbg & 16u)) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    bf16x8 a = lds_load_a_frag(&lds.h[curp][0][0], mt * 16, kb * 32, HPAD);
#pragma unroll
                    for (int g = 0; g < 3; ++g)
                        acc[mt][g] = mfma16x16x32(a, ufrag[g][kb], acc[mt][g]);
                }
            }
        }

        // fused gate math; updates the fp32 register hidden state and writes
        // the bf16 mirror into the BACK h buffer (no reader until barrier).
        // Structured as: batch ALL 24 xg reads first, then run the 8
        // elements' serial exp/rcp chains as INDEPENDENT interleavable
        // streams — the original per-element form (reads + chain + a dbg
        // branch per element) compiled to 16 fenced basic blocks whose
        // ~200-cycle dependency chains executed back to back: the gate
        // phase alone was 55% of the kernel (scripts/gru_timing.py).
        if (dbg & 4u) {  // timing: gate math stripped (separate cold loop)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = mt * 16 + lrow * 4 + i;
                    const int j = j0 + lcol;
                    const float hnew =
                        acc[mt][0][i] + acc[mt][1][i] + acc[mt][2][i];
                    hreg[mt][i] = hnew;
                    lds.h[curp ^ 1][row][j] = f2bf(hnew);
                    if constexpr (TRAIN) {
                        if (!(dbg & 2u)) {
                            bf16x4 pk = {f2bf(hnew), f2bf(hnew), f2bf(hnew),
                                         f2bf(hnew)};
                            *reinterpret_cast<bf16x4*>(
                                cache +
                                (((size_t)t * B + b0 + row) * 2 + dir) * 4 * H +
                                4 * j) = pk;
                        }
                    }
                }
        } else {
            const int j = j0 + lcol;
            float xr[MT][4], xz[MT][4], xn[MT][4];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = mt * 16 + lrow * 4 + i;
                    xr[mt][i] = bf2f(lds.xgb[curp][row][0 * H + j]);
                    xz[mt][i] = bf2f(lds.xgb[curp][row][1 * H + j]);
                    xn[mt][i] = bf2f(lds.xgb[curp][row][2 * H + j]);
                }
            float r8[MT][4], z8[MT][4], n8[MT][4], hg8[MT][4];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    hg8[mt][i] = acc[mt][2][i] + bhh_reg[2];
                    r8[mt][i] =
                        sigmoidf_dev(xr[mt][i] + acc[mt][0][i] + bhh_reg[0]);
                    z8[mt][i] =
                        sigmoidf_dev(xz[mt][i] + acc[mt][1][i] + bhh_reg[1]);
                }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    n8[mt][i] = tanhf_dev(xn[mt][i] + r8[mt][i] * hg8[mt][i]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = mt * 16 + lrow * 4 + i;
                    const float hnew = (1.0f - z8[mt][i]) * n8[mt][i] +
                                       z8[mt][i] * hreg[mt][i];
                    hreg[mt][i] = hnew;
                    lds.h[curp ^ 1][row][j] = f2bf(hnew);
                    if constexpr (TRAIN) {
                        // cache stores straight from registers (8-byte,
                        // 128 B per 16-lane group): no LDS staging tile,
                        // no post-barrier round-trip
                        if (!(dbg & 2u)) {
                            bf16x4 pk = {f2bf(r8[mt][i]), f2bf(z8[mt][i]),
                                         f2bf(n8[mt][i]), f2bf(hg8[mt][i])};
                            *reinterpret_cast<bf16x4*>(
                                cache +
                                (((size_t)t * B + b0 + row) * 2 + dir) * 4 * H +
                                4 * j) = pk;
                        }
                    }
                }
        }
        __syncthreads();  // h[curp^1] (+ cache staging) published

        // cooperative wide store of h to hseq (coalesced 16B per lane),
        // overlaps the next step's MFMAs as plain VMEM traffic
        if (!(dbg & 1u)) {
            bf16* dst = hseq + (((size_t)t * B + b0) * 2 + dir) * H;
            const int e = tid * CW;
            const int row = e / H, col = e % H;
            *reinterpret_cast<xvec*>(dst + (size_t)row * 2 * H + col) =
                *reinterpret_cast<const xvec*>(&lds.h[curp ^ 1][row][col]);
        }
    };

    int ti = 0;
    for (; ti + 2 <= T; ti += 2) {
        body(ti, 0, stageA, stageB);
        body(ti + 1, 1, stageB, stageA);
    }
    if (ti < T) body(ti, 0, stageA, stageB);
}

// ---------------------------------------------------------------------------
// Eval GRU, transposed step (docs/KERNELS.md lesson 23). Same grid, tile,
// waves, U-in-registers, double-buffered h mirror and one barrier per step as
// gru_layer_fwd_kernel<false, 0, 16>, and the same arithmetic per output (kb
// ascending over the same four MFMAs, (x + acc) + bhh, the same sigmoid /
// tanh / blend expressions, one bf16 round): hseq is byte-identical.
//
// The MFMA operands are swapped: the U fragment is A, the h fragment read
// from the mirror is B (the two fragment layouts are the same, so neither
// address changes). A lane's accumulator is then
//     gate[j = j0 + 4*lrow + i][row = lcol],  i = 0..3
// — four consecutive hidden columns of ONE batch row. So
//   * a lane's gate inputs are 8 contiguous bytes of the row-major xg per
//     gate: three global_load_dwordx2 per step straight into registers. No
//     xg tile in LDS, no staging writes, no 16-bit reads;
//   * the new h goes to the mirror as one 8-byte write of four packed bf16;
//   * bhh is four values per gate per lane.
//
// Prefetch: the loads for step t + NSET - 1 issue at the top of step t,
// before the MFMAs, into one of NSET register sets (the loop is unrolled by
// NSET, so the set is a compile-time choice); the gate phase of the step
// that consumes them is the first instruction to touch them. No branch
// surrounds a load — the step index is clamped to T - 1 instead (a re-read of
// a valid step of this workgroup's rows; no address outside steps [0, T) is
// formed). sched_barrier(0) after the issue and before the gate phase keeps
// the scheduler from sinking the loads or hoisting the conversions, so the
// compiler's own wait is a counted vmcnt(N) that only covers loads a full
// step old.
//
// h mirror pitch audit (HPAD = 136 bf16 = 272 B = 68 dwords, unchanged):
//   * fragment reads, ds_read_b128, four 16-lane groups, bank = dword mod
//     64: lane (lrow, lcol) reads 16-B slot (17*lcol + lrow + 4*kb) mod 16 =
//     (lcol + lrow) mod 16. Group {0-3, 12-15, 20-27} holds lrow 0 with lcol
//     0-3, 12-15 (slots 0-3, 12-15) and lrow 1 with lcol 4-11 (slots 5-12):
//     slot 12 twice, every other slot at most once — one 2-way conflict, 5
//     LDS cycles where 4 is the floor; the other three groups are the same
//     picture shifted. These are the reads the old kernel does too.
//   * mirror writes, ds_write_b64, four contiguous 16-lane groups (one lrow,
//     lcol 0-15), bank = dword mod 32: dword = 68*lcol + 8*wid + 2*lrow, so
//     lcol and lcol + 8 share a bank pair: 2-way, 8 array cycles against the
//     instruction's own 6. Any 16-B-aligned pitch is a multiple of 4 dwords
//     and gives >= 2-way here; 2-way is the best a row-per-lane 8-byte write
//     can do without a swizzle.
//   * a 288-B pitch would make the reads conflict-free (slot 2*lcol + lrow)
//     and the writes 4-way: -16 and +8 LDS cycles per wave per step, a net
//     ~64 cycles per workgroup per ~1,900-cycle step on a pipe that is idle
//     most of the step. HPAD stays.
//
// DBG (compile time, timing probes only; production is DBG = 0):
//   1 no hseq store, 4 no gate VALU, 8 no xg loads, 16 no MFMA.
// HSREG: hseq is stored from the packed registers before the barrier (true)
// or from the mirror after it, coalesced (false).
// STAGED: the fallback form, kept for the timing script — coalesced 8-byte
// loads of the whole 16 x 384 step tile, parked in LDS a step later behind
// the same counted waits, read back with three ds_read_b64 per lane.
// Resources of the shipped <0, 2, false, false>: 108 VGPRs, 0 AGPRs, 0
// scratch, 8,704 B LDS (old kernel: 118 / 0 / 0 / 33,280 B).
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

constexpr int E2_MBT = 16;
constexpr int E2_NSET = 2;        // shipped: prefetch distance one step
constexpr bool E2_HSREG = false;  // shipped hseq store
// STAGED tile pitch: 392 bf16 = 196 dwords. The three ds_read_b64 per lane
// (two 32-lane groups, bank = dword mod 64) touch dwords 196*lcol + 8*wid +
// 2*lrow + {0, 1} = 4*lcol + 2*lrow + c (mod 64): 64 distinct banks per
// group. The unpadded 384 puts all 16 rows of a group on the same banks.
constexpr int E2_XPAD = G3 + 8;

RK_DEV float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
RK_DEV float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
RK_DEV uint32_t pack_bf16x2(float a, float b) {
    union {
        bf16x2 v;
        uint32_t w;
    } p;
    p.v = __builtin_convertvector(f32x2{a, b}, bf16x2);
    return p.w;
}

template <int DBG, int NSET, bool HSREG, bool STAGED = false>
__global__ __launch_bounds__(WAVES * 64, 2) void gru_eval2_kernel(
    const bf16* __restrict__ xg,   // (T, B, 2, 3H)  W_ih·x + b_ih
    const bf16* __restrict__ u,    // (2, 3H, H)     weight_hh
    const float* __restrict__ bhh, // (2, 3H)        bias_hh
    bf16* __restrict__ hseq,       // (T, B, 2, H)   output
    int T, int B) {
    static_assert(!STAGED || NSET == 2, "the staged form has two sets");
    constexpr int DIST = NSET - 1;  // register sets loaded ahead of the loop
    // step distance of the load a step issues: the staged form parks a set
    // in LDS one step before its use, so it looks one step further
    constexpr int LOOK = STAGED ? NSET : NSET - 1;
    constexpr int HBUF = E2_MBT * HPAD;
    constexpr int XBUF = E2_MBT * E2_XPAD;
    __shared__ bf16 hm[2 * HBUF];   // double-buffered hidden-state mirror
    __shared__ bf16 xst[STAGED ? 2 * XBUF : 1];  // STAGED: xg step tiles

    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * E2_MBT;
    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;
    const int j0 = wid * 16;          // this wave's 16 hidden columns
    const int jl = j0 + 4 * lrow;     // this lane's four hidden columns
    if (wid >= WAVES / 2) __builtin_amdgcn_s_setprio(1);

    // A-fragment: A[m = lcol][k] = U[g*H + j0 + lcol][kb*32 + 8*lrow + ..]
    bf16x8 ufrag[3][4];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
            ufrag[g][kb] = *reinterpret_cast<const bf16x8*>(
                u + (size_t)dir * G3 * H + (size_t)(g * H + j0 + lcol) * H +
                kb * 32 + 8 * lrow);
    float bhh_reg[3][4];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            bhh_reg[g][i] = bhh[dir * G3 + g * H + jl + i];

    float hreg[4] = {0.f, 0.f, 0.f, 0.f};  // fp32 master copy of h
    for (int e = tid; e < HBUF; e += WAVES * 64) hm[e] = f2bf(0.0f);

    const int stp = (dir == 0) ? 1 : -1;
    const int tfirst = (dir == 0) ? 0 : T - 1;
    const size_t xstep = (size_t)B * 2 * G3;
    const bf16* xlane = xg + ((size_t)(b0 + lcol) * 2 + dir) * G3 + jl;
    // STAGED: chunk c = 512*p + tid of the 16 x 384 step tile, 4 bf16 each
    // (96 chunks per row: a 16-lane group never straddles a row)
    int srow[3], scol[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const int e = (p * WAVES * 64 + tid) * 4;
        srow[p] = e / G3;
        scol[p] = e % G3;
    }
    // xg of step index s (clamped into [0, T)) -> one register set
    auto load_x = [&](int s, u32x2 (&set)[3]) {
        const int sc = s < T - 1 ? s : T - 1;
        const size_t toff = (size_t)(tfirst + stp * sc) * xstep;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            if constexpr (STAGED)
                set[g] = *reinterpret_cast<const u32x2*>(
                    xg + toff + ((size_t)(b0 + srow[g]) * 2 + dir) * G3 +
                    scol[g]);
            else
                set[g] =
                    *reinterpret_cast<const u32x2*>(xlane + toff + g * H);
        }
    };
    auto stage_x = [&](int buf_off, const u32x2 (&set)[3]) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
            *reinterpret_cast<u32x2*>(xst + buf_off + srow[g] * E2_XPAD +
                                      scol[g]) = set[g];
    };

    u32x2 xs[NSET][3];
#pragma unroll
    for (int s = 0; s < NSET; ++s)
#pragma unroll
        for (int g = 0; g < 3; ++g) xs[s][g] = u32x2{0u, 0u};
    if constexpr (STAGED && !(DBG & 8)) {
        load_x(0, xs[1]);
        stage_x(0, xs[1]);  // step 0 straight into tile buffer 0
        load_x(1, xs[0]);
    } else if constexpr (!(DBG & 8)) {
#pragma unroll
        for (int s = 0; s < DIST; ++s) load_x(s, xs[s]);
    }
    // Drain the prologue (U, bhh and the first xg sets, all needed by step
    // 0 anyway) so the loop is entered with nothing in flight. Entered with
    // loads pending, the compiler's counted waits inside the loop must also
    // be right for the entry path, and come out as vmcnt(5/4/3) where the
    // steady state allows 7/6/5: each step would wait for the hseq store
    // issued just before it.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only
    __syncthreads();

    int rd = 0;   // element offset of the mirror buffer this step reads
    int xrd = 0;  // STAGED: element offset of the xg tile this step reads
    auto body = [&](int ti, u32x2 (&x_ld)[3], u32x2 (&x)[3]) {
        const int t = tfirst + stp * ti;
        const int wr = rd ^ HBUF;
        if constexpr (!(DBG & 8)) load_x(ti + LOOK, x_ld);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (STAGED && !(DBG & 8)) {
            // park the set loaded a step ago (step ti + 1) in the back tile
#pragma unroll
            for (int g = 0; g < 3; ++g) asm volatile("" : "+v"(x[g]));
            stage_x(xrd ^ XBUF, x);
            __builtin_amdgcn_sched_barrier(0);
        }

        // gates_h^T = U · h^T  (12 MFMA per wave, h fragment shared 3-ways)
        f32x4 acc[3];
        if constexpr (DBG & 16) {
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const bf16x8 hf = lds_load_a_frag(hm + rd, 0, kb * 32, HPAD);
#pragma unroll
                for (int g = 0; g < 3; ++g)
                    acc[g] = mfma16x16x32(
                        ufrag[g][kb], hf,
                        kb == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[g]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // the set is opaque up to here: without this the bf16 -> f32 shifts
        // of x are placed above the MFMAs and take the vmcnt wait with them
        u32x2 xv[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            if constexpr (STAGED) {
                xv[g] = *reinterpret_cast<const u32x2*>(
                    xst + xrd + lcol * E2_XPAD + g * H + jl);
            } else {
                asm volatile("" : "+v"(x[g]));
                xv[g] = x[g];
            }
        }

        float hnew[4];
        if constexpr (DBG & 4) {  // timing: gate math stripped, loads kept
#pragma unroll
            for (int i = 0; i < 4; ++i)
                hnew[i] = acc[0][i] + acc[1][i] + acc[2][i];
        } else {
            float xr[4], xz[4], xn[4];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                xr[2 * p] = bf_lo(xv[0][p]);
                xr[2 * p + 1] = bf_hi(xv[0][p]);
                xz[2 * p] = bf_lo(xv[1][p]);
                xz[2 * p + 1] = bf_hi(xv[1][p]);
                xn[2 * p] = bf_lo(xv[2][p]);
                xn[2 * p + 1] = bf_hi(xv[2][p]);
            }
            float r4[4], z4[4], n4[4], hg4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                hg4[i] = acc[2][i] + bhh_reg[2][i];
                r4[i] = sigmoidf_dev(xr[i] + acc[0][i] + bhh_reg[0][i]);
                z4[i] = sigmoidf_dev(xz[i] + acc[1][i] + bhh_reg[1][i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                n4[i] = tanhf_dev(xn[i] + r4[i] * hg4[i]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                hnew[i] = (1.0f - z4[i]) * n4[i] + z4[i] * hreg[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) hreg[i] = hnew[i];
        const u32x2 pk = {pack_bf16x2(hnew[0], hnew[1]),
                          pack_bf16x2(hnew[2], hnew[3])};
        *reinterpret_cast<u32x2*>(hm + wr + lcol * HPAD + jl) = pk;
        bf16* dst = hseq + (((size_t)t * B + b0) * 2 + dir) * H;
        if constexpr (HSREG && !(DBG & 1))
            *reinterpret_cast<u32x2*>(dst + (size_t)lcol * 2 * H + jl) = pk;
        __syncthreads();  // h[wr] published
        if constexpr (!HSREG && !(DBG & 1)) {
            // cooperative store from the mirror: 8 B per lane, a wave
            // covers two whole 256-B rows
            const int row = tid >> 5, col = (tid & 31) * 4;
            *reinterpret_cast<u32x2*>(dst + (size_t)row * 2 * H + col) =
                *reinterpret_cast<const u32x2*>(hm + wr + row * HPAD + col);
        }
        rd = wr;
        if constexpr (STAGED) xrd ^= XBUF;
    };

    int ti = 0;
    for (; ti + NSET <= T; ti += NSET) {
#pragma unroll
        for (int s = 0; s < NSET; ++s)
            body(ti + s, xs[(s + DIST) % NSET], xs[s]);
    }
#pragma unroll
    for (int s = 0; s < NSET - 1; ++s)
        if (ti + s < T) body(ti + s, xs[(s + DIST) % NSET], xs[s]);
}

static void launch_eval2(const bf16* xg, const bf16* u, const float* bhh,
                         bf16* hseq, int T, int B, hipStream_t stream,
                         uint32_t dbg) {
    const dim3 grid(B / E2_MBT, 2), block(WAVES * 64);
#define RK_E2(D)                                                             \
    hipLaunchKernelGGL((gru_eval2_kernel<D, E2_NSET, E2_HSREG>), grid,       \
                       block, 0, stream, xg, u, bhh, hseq, T, B)
    switch (dbg) {
        case 0: RK_E2(0); break;
        case 1: RK_E2(1); break;
        case 4: RK_E2(4); break;
        case 8: RK_E2(8); break;
        case 16: RK_E2(16); break;
        default:
            throw std::invalid_argument(
                "gru eval2 probe mask must be one of 0, 1, 4, 8, 16");
    }
#undef RK_E2
}

// ROKO_GRU_EVAL=v1: the old eval kernels, process-wide
static bool env_gru_eval_v1() {
    static const bool v = [] {
        const char* f = getenv("ROKO_GRU_EVAL");
        return f && std::string(f) == "v1";
    }();
    return v;
}

// ROKO_GRU_MB=32: the 32-row tile in the training forward, the old eval
// kernels and the backward, process-wide
static bool env_gru_mb32() {
    static const bool v = [] {
        const char* f = getenv("ROKO_GRU_MB");
        return f && std::string(f) == "32";
    }();
    return v;
}

// Which eval kernel a gru_layer_fwd(cache == nullptr) call launches:
// 1 the old kernels, 2 the transposed kernel; for the timing script only, 3
// the transposed kernel with the hseq store variant that is not shipped and
// 4 the transposed kernel with xg staged through LDS (the fallback form).
// impl: 0 default (the transposed kernel; ROKO_GRU_EVAL=v1 or ROKO_GRU_MB=32
// make that the old kernels, process-wide), 1/2/3 as above.
int gru_eval_select(int impl, int B) {
    const bool eval_v1 = env_gru_eval_v1(), mb32 = env_gru_mb32();
    if (impl < 0 || impl > 4)
        throw std::invalid_argument("gru_layer_fwd: impl must be 0..4");
    if (impl >= 2 && (B % 16) != 0)
        throw std::invalid_argument(
            "the transposed eval GRU needs a batch that is a multiple of 16");
    if (impl >= 2) return impl;
    return (impl == 0 && !eval_v1 && !mb32 && (B % 16) == 0) ? 2 : 1;
}

void gru_layer_fwd(const void* xg, const void* u, const float* bhh, void* hseq,
                   void* cache, int T, int B, hipStream_t stream,
                   uint32_t dbg, int impl) {
    dim3 grid(B / MB, 2);
    dim3 block(WAVES * 64);
    if (cache && impl >= 2)
        throw std::invalid_argument("impl 2..4 are eval kernels");
    const int sel = cache ? 1 : gru_eval_select(impl, B);
    if (sel >= 2) {
        if (sel >= 3) {
            if (dbg)
                throw std::invalid_argument(
                    "probe masks exist for the shipped eval kernel only");
            if (sel == 3)
                hipLaunchKernelGGL(
                    (gru_eval2_kernel<0, E2_NSET, !E2_HSREG>),
                    dim3(B / E2_MBT, 2), block, 0, stream,
                    static_cast<const bf16*>(xg),
                    static_cast<const bf16*>(u), bhh,
                    static_cast<bf16*>(hseq), T, B);
            else
                hipLaunchKernelGGL(
                    (gru_eval2_kernel<0, 2, E2_HSREG, true>),
                    dim3(B / E2_MBT, 2), block, 0, stream,
                    static_cast<const bf16*>(xg),
                    static_cast<const bf16*>(u), bhh,
                    static_cast<bf16*>(hseq), T, B);
        } else {
            launch_eval2(static_cast<const bf16*>(xg),
                         static_cast<const bf16*>(u), bhh,
                         static_cast<bf16*>(hseq), T, B, stream, dbg);
        }
        return;
    }
    // MBT=16 halves each thread's gate-chain count — the gate phase sits
    // at the 2-wave VALU-issue floor, so the wall nearly halves (eval
    // 175.6 -> 97.7 us measured) and the WG count doubles (serving
    // packing). ROKO_GRU_MB=32 reverts both paths.
    const int mb_sel = env_gru_mb32() ? 32 : 16;
    if (cache) {
        if (mb_sel == 16 && (B % 16) == 0)
            hipLaunchKernelGGL((gru_layer_fwd_kernel<true, 0, 16>),
                               dim3(B / 16, 2), block, 0, stream,
                               static_cast<const bf16*>(xg),
                               static_cast<const bf16*>(u), bhh,
                               static_cast<bf16*>(hseq),
                               static_cast<bf16*>(cache), T, B, dbg, nullptr,
                               nullptr, nullptr, 0);
        else
            hipLaunchKernelGGL((gru_layer_fwd_kernel<true, 0>), grid, block,
                               0, stream, static_cast<const bf16*>(xg),
                               static_cast<const bf16*>(u), bhh,
                               static_cast<bf16*>(hseq),
                               static_cast<bf16*>(cache), T, B, dbg, nullptr,
                               nullptr, nullptr, 0);
    }
    else {
        // eval tile choice: MBT=16 doubles the WG count and halves each
        // thread's gate-chain count (ROKO_GRU_MB=32 reverts)
        // (a batch that is a multiple of 16 only has no 32-row form)
        if ((mb_sel == 16 || (B % 32) != 0) && (B % 16) == 0)
            hipLaunchKernelGGL((gru_layer_fwd_kernel<false, 0, 16>),
                               dim3(B / 16, 2), block, 0, stream,
                               static_cast<const bf16*>(xg),
                               static_cast<const bf16*>(u), bhh,
                               static_cast<bf16*>(hseq), nullptr, T, B, dbg,
                               nullptr, nullptr, nullptr, 0);
        else
            hipLaunchKernelGGL((gru_layer_fwd_kernel<false, 0>), grid, block,
                               0, stream, static_cast<const bf16*>(xg),
                               static_cast<const bf16*>(u), bhh,
                               static_cast<bf16*>(hseq), nullptr, T, B, dbg,
                               nullptr, nullptr, nullptr, 0);
    }
}

// serving variant: xg computed in-kernel from (x, W_ih, b_ih); `xg` is a
// (T, B, 2, 3H) workspace
void gru_layer_fwd_fused(const void* x, const void* w_ih_p, const void* b_ih,
                         const void* u, const float* bhh, void* xg_ws,
                         void* hseq, int T, int B, int IN, int KP,
                         hipStream_t stream) {
    dim3 grid(B / MB, 2);
    dim3 block(WAVES * 64);
    if (KP == 512)
        hipLaunchKernelGGL((gru_layer_fwd_kernel<false, 512>), grid, block, 0,
                           stream, static_cast<bf16*>(xg_ws),
                           static_cast<const bf16*>(u),
                           static_cast<const float*>(bhh),
                           static_cast<bf16*>(hseq), nullptr, T, B, 0u,
                           static_cast<const bf16*>(x),
                           static_cast<const bf16*>(w_ih_p),
                           static_cast<const bf16*>(b_ih), IN);
    else if (KP == 256)
        hipLaunchKernelGGL((gru_layer_fwd_kernel<false, 256>), grid, block, 0,
                           stream, static_cast<bf16*>(xg_ws),
                           static_cast<const bf16*>(u),
                           static_cast<const float*>(bhh),
                           static_cast<bf16*>(hseq), nullptr, T, B, 0u,
                           static_cast<const bf16*>(x),
                           static_cast<const bf16*>(w_ih_p),
                           static_cast<const bf16*>(b_ih), IN);
    else
        (void)0;  // unsupported KP: caller validates (bindings.cpp)
}

// ---------------------------------------------------------------------------
// Backward (BPTT) — the sequential part only. The kernel walks the T steps
// in reverse, carrying dL/dh in registers and emitting per-step gate
// gradients dg = [dxr, dxz, dxn, dhgn]; the batched weight/input gradient
// reductions (dU = dhg^T·h_prev, dW_ih = dxg^T·x, dx = dxg·W_ih) are plain
// GEMMs done host-side with hipBLASLt.
//
// Math per step (forward: r,z = sig, n = tanh(xn + r*hgn), h' = (1-z)n + zh):
//   dn   = dh * (1-z)            dz  = dh * (h_prev - n)
//   dan  = dn * (1 - n^2)        dxn = dan         dhgn = dan * r
//   dr   = dan * hgn             dxr = dhgr = dr * r * (1-r)
//   dxz  = dhgz = dz * z * (1-z)
//   dh_prev = dh * z + dhg · U
// ---------------------------------------------------------------------------

constexpr int BW_WAVES = 8;  // dhg GEMM has K=384: 24 MFMA/wave at 8 waves
constexpr int BWCH_C = 4;    // cache chunks per thread (32x512 / 512 / 8)

template <int MBT = MB>
__global__ __launch_bounds__(BW_WAVES * 64, 2) void gru_layer_bwd_kernel(
    const bf16* __restrict__ cache,  // (T, B, 2, H, 4) [r z n hgn] packed
    const bf16* __restrict__ hseq,   // (T, B, 2, H)
    const bf16* __restrict__ dhin,   // (T, B, 2, H) grad wrt layer output
    const bf16* __restrict__ ut,     // (2, H, 3H) = weight_hh^T
    bf16* __restrict__ dxg,          // (T, B, 2, 3H) out: [dxr dxz dxn] —
                                     // (T*B, 768) view feeds dW_ih/dx GEMMs
    bf16* __restrict__ dhg,          // (2, T, B, 3H) out: [dxr dxz dhgn]
                                     // dir-major so each dir slice is a
                                     // contiguous (T*B, 384) GEMM operand
    int T, int B,
    uint32_t dbg) {  // timing bisection: 1 no global stores, 2 no gate
                     // VALU, 4 no MFMA, 8 no staging
    // ONE barrier per step (was two): dhg is double-buffered so the next
    // step's gate writes never touch the tile the current step's dh GEMM
    // and output stores still read, and the dg_st staging tile is gone —
    // dxg/dhg stores read straight from lds.dhg (dxr/dxz/dhgn blocks) plus
    // per-lane register stores for the dxn column block.
    constexpr int MT = MBT / 16;               // 16-row m-subtiles
    constexpr int BWCH = MBT * 4 * H / (BW_WAVES * 64 * 8);  // cache chunks
    __shared__ struct {
        bf16 cache_st[2][MBT][4 * H];  // double-buffered staged cache[t]
        bf16 dhin_st[2][MBT][H];       // double-buffered staged dhin[t]
        bf16 hprev_st[2][MBT][H];      // double-buffered staged h_{t-1}
        bf16 dhg[2][MBT][G3 + 8];      // A-operand of the dh GEMM (2 bufs)
    } lds;

    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * MBT;
    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int j0 = wid * 16;
    const int lrow = lane >> 4;
    const int lcol = lane & 15;
    if (wid >= BW_WAVES / 2) __builtin_amdgcn_s_setprio(1);

    // B-fragments of U for dh_prev = dhg·U: B[k=j][col=khid] = Ut[khid][j]
    bf16x8 ufrag[12];
#pragma unroll
    for (int kb = 0; kb < 12; ++kb) {
        const int col = j0 + lcol;          // this wave's hidden column
        const int j = kb * 32 + 8 * lrow;   // gate-row index
        ufrag[kb] = *reinterpret_cast<const bf16x8*>(
            ut + ((size_t)dir * H + col) * G3 + j);
    }

    float dhc[MT][4];  // dh carry, fragment-shaped
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) dhc[mt][i] = 0.0f;

    const int stp = (dir == 0) ? -1 : 1;     // BPTT walks t backwards
    const int t0 = (dir == 0) ? T - 1 : 0;
    auto t_of = [&](int sidx) { return t0 + stp * sidx; };

    // register-staged loads for one step: cache (4 chunks) + dhin + hprev
    auto issue_loads = [&](int sidx, bf16x8 (&rc)[BWCH], bf16x8& rdh,
                           bf16x8& rhp) {
        if (dbg & 8u) return;
        const int t = t_of(sidx);
        const int tp = (dir == 0) ? t - 1 : t + 1;
        const bf16* src = cache + (((size_t)t * B + b0) * 2 + dir) * 4 * H;
        const int row4 = tid / 64, col4 = (tid % 64) * 8;
#pragma unroll
        for (int q = 0; q < BWCH; ++q)
            rc[q] = *reinterpret_cast<const bf16x8*>(
                src + (size_t)(row4 + q * 8) * 2 * 4 * H + col4);
        const int row = tid / 16, col = (tid % 16) * 8;
        rhp = bf16x8{};
        if (row < MBT) {
            rdh = *reinterpret_cast<const bf16x8*>(
                dhin + (((size_t)t * B + b0) * 2 + dir) * H + (size_t)row * 2 * H + col);
            if (tp >= 0 && tp < T)
                rhp = *reinterpret_cast<const bf16x8*>(
                    hseq + (((size_t)tp * B + b0) * 2 + dir) * H + (size_t)row * 2 * H + col);
        } else
            rdh = bf16x8{};
    };
    auto write_stage = [&](int buf, bf16x8 (&rc)[BWCH], bf16x8& rdh,
                           bf16x8& rhp) {
        const int row4 = tid / 64, col4 = (tid % 64) * 8;
#pragma unroll
        for (int q = 0; q < BWCH; ++q)
            *reinterpret_cast<bf16x8*>(&lds.cache_st[buf][row4 + q * 8][col4]) = rc[q];
        const int row = tid / 16, col = (tid % 16) * 8;
        if (row < MBT) {
            *reinterpret_cast<bf16x8*>(&lds.dhin_st[buf][row][col]) = rdh;
            *reinterpret_cast<bf16x8*>(&lds.hprev_st[buf][row][col]) = rhp;
        }
    };

    bf16x8 rcA[BWCH], rcB[BWCH];
    bf16x8 rdhA, rhpA, rdhB, rhpB;
    // prologue: step 0 straight to LDS buffer 0; step 1 to registers A
    issue_loads(0, rcA, rdhA, rhpA);
    write_stage(0, rcA, rdhA, rhpA);
    if (T > 1) issue_loads(1, rcA, rdhA, rhpA);
    __syncthreads();

    auto body = [&](int sidx, int curp, bf16x8 (&rc_wr)[BWCH], bf16x8& rdh_wr,
                    bf16x8& rhp_wr, bf16x8 (&rc_ld)[BWCH], bf16x8& rdh_ld,
                    bf16x8& rhp_ld) {
        const int t = t_of(sidx);
        // issue step s+2 loads FIRST, then write step s+1's staged registers
        if (sidx + 2 < T) issue_loads(sidx + 2, rc_ld, rdh_ld, rhp_ld);
        if (sidx + 1 < T) write_stage(curp ^ 1, rc_wr, rdh_wr, rhp_wr);

        // ---- gate gradients from stage[curp] ------------------------------
        // reads batched first, then 8 independent arithmetic chains, then
        // the stores — same restructure as the forward's gate phase (the
        // interleaved per-element form serialized the read latencies)
        float dhp_part[MT][4];
        float dxn8[MT][4];  // kept in registers for the direct dxg store
        {
            const int j = j0 + lcol;
            float dh8[MT][4], hp8[MT][4];
            bf16x4 pk8[MT][4];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = mt * 16 + lrow * 4 + i;
                    dh8[mt][i] =
                        dhc[mt][i] + bf2f(lds.dhin_st[curp][row][j]);
                    pk8[mt][i] = *reinterpret_cast<const bf16x4*>(
                        &lds.cache_st[curp][row][4 * j]);
                    hp8[mt][i] = bf2f(lds.hprev_st[curp][row][j]);
                }
            if (dbg & 2u) {  // timing: gate math stripped
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = mt * 16 + lrow * 4 + i;
                        const float v = dh8[mt][i] + hp8[mt][i];
                        dhp_part[mt][i] = v;
                        dxn8[mt][i] = v;
                        lds.dhg[curp][row][0 * H + j] = f2bf(v);
                        lds.dhg[curp][row][1 * H + j] = f2bf(v);
                        lds.dhg[curp][row][2 * H + j] = f2bf(v);
                    }
            } else
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = mt * 16 + lrow * 4 + i;
                    const float dh = dh8[mt][i];
                    const float r = bf2f(pk8[mt][i][0]);
                    const float z = bf2f(pk8[mt][i][1]);
                    const float n = bf2f(pk8[mt][i][2]);
                    const float hgn = bf2f(pk8[mt][i][3]);
                    const float dn = dh * (1.0f - z);
                    const float dz = dh * (hp8[mt][i] - n);
                    const float dan = dn * (1.0f - n * n);
                    const float dhgn = dan * r;
                    const float dxr = dan * hgn * r * (1.0f - r);
                    const float dxz = dz * z * (1.0f - z);
                    dhp_part[mt][i] = dh * z;
                    dxn8[mt][i] = dan;
                    lds.dhg[curp][row][0 * H + j] = f2bf(dxr);
                    lds.dhg[curp][row][1 * H + j] = f2bf(dxz);
                    lds.dhg[curp][row][2 * H + j] = f2bf(dhgn);
                }
        }
        __syncthreads();  // dhg[curp] and stage[curp^1] published (the ONLY
                          // barrier per step; next step writes dhg[curp^1])

        // ---- dh_prev = dh*z + dhg · U  (24 MFMA per wave) -----------------
        f32x4 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!(dbg & 4u)) {
#pragma unroll
            for (int kb = 0; kb < 12; ++kb) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    bf16x8 a = lds_load_a_frag(&lds.dhg[curp][0][0], mt * 16,
                                               kb * 32, G3 + 8);
                    acc[mt] = mfma16x16x32(a, ufrag[kb], acc[mt]);
                }
            }
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) dhc[mt][i] = dhp_part[mt][i] + acc[mt][i];

        // ---- store dxg + dhg tiles (GEMM-ready layouts, no host cats) -----
        // dxg = [dxr dxz dxn]: the dxr/dxz blocks copy wide from lds.dhg,
        // dxn comes from this lane's registers (scalar stores)
        if (!(dbg & 1u)) {
            bf16* dst = dxg + (((size_t)t * B + b0) * 2 + dir) * G3;
            const int row = tid / 32, col = (tid % 32) * 8;  // 2H block
#pragma unroll
            for (int q = 0; q < MT; ++q)
                *reinterpret_cast<bf16x8*>(
                    dst + (size_t)(row + q * 16) * 2 * G3 + col) =
                    *reinterpret_cast<const bf16x8*>(
                        &lds.dhg[curp][row + q * 16][col]);
            const int j = j0 + lcol;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row2 = mt * 16 + lrow * 4 + i;
                    dst[(size_t)row2 * 2 * G3 + 2 * H + j] =
                        f2bf(dxn8[mt][i]);
                }
        }
        if (!(dbg & 1u)) {
            // dhg tensor = [dxr dxz dhgn] — exactly lds.dhg's live columns
            bf16* dst = dhg + (((size_t)dir * T + t) * B + b0) * G3;
            const int row = tid / 64, col = (tid % 64) * 8;
            if (col < G3) {
#pragma unroll
                for (int q = 0; q < MBT / 8; ++q)
                    *reinterpret_cast<bf16x8*>(
                        dst + (size_t)(row + q * 8) * G3 + col) =
                        *reinterpret_cast<const bf16x8*>(
                            &lds.dhg[curp][row + q * 8][col]);
            }
        }
    };

    int sidx = 0;
    for (; sidx + 2 <= T; sidx += 2) {
        body(sidx, 0, rcA, rdhA, rhpA, rcB, rdhB, rhpB);
        body(sidx + 1, 1, rcB, rdhB, rhpB, rcA, rdhA, rhpA);
    }
    if (sidx < T) body(sidx, 0, rcA, rdhA, rhpA, rcB, rdhB, rhpB);
}

void gru_layer_bwd(const void* cache, const void* hseq, const void* dhin,
                   const void* ut, void* dxg, void* dhg, int T, int B,
                   hipStream_t stream, uint32_t dbg) {
    dim3 block(BW_WAVES * 64);
    const int mb_sel = env_gru_mb32() ? 32 : 16;
    if (mb_sel == 16 && (B % 16) == 0)
        hipLaunchKernelGGL((gru_layer_bwd_kernel<16>), dim3(B / 16, 2), block,
                           0, stream, static_cast<const bf16*>(cache),
                           static_cast<const bf16*>(hseq),
                           static_cast<const bf16*>(dhin),
                           static_cast<const bf16*>(ut),
                           static_cast<bf16*>(dxg), static_cast<bf16*>(dhg),
                           T, B, dbg);
    else
        hipLaunchKernelGGL((gru_layer_bwd_kernel<32>), dim3(B / MB, 2), block,
                           0, stream, static_cast<const bf16*>(cache),
                           static_cast<const bf16*>(hseq),
                           static_cast<const bf16*>(dhin),
                           static_cast<const bf16*>(ut),
                           static_cast<bf16*>(dxg), static_cast<bf16*>(dhg),
                           T, B, dbg);
}

}  // namespace rk
