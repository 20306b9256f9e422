// Per-position 5-class head: logits = h·W4^T + b4, optionally fused argmax
// (reference: rnn_model.py:59 fc4 + inference.py:116 argmax — SURVEY.md §2.4
// K5/K8). Skinny N=5 GEMV: one lane per (t, b) row, W4 staged in LDS,
// 16B-vectorised K loop on the VALU (MFMA has nothing to win at N=5).

#include <cstdint>

#include "api.h"
#include "common.h"

namespace rk {

constexpr int HH = 256;  // 2 * HIDDEN_SIZE
constexpr int NC = 5;    // classes

// Per-vote quality units (docs/KERNELS.md "Device votes"): for every class k
// the probability that the column is NOT k, e_k = sum_{j != k} t_j / sum_j t_j
// with t_j = exp(z_j - max z), as quarter-Phred units
// u_k = min(255, floor(4 * -10 log10(e_k) + 0.5)); e_k = 0 gives 255. The sum
// over the others is taken directly, never as 1 - p_k, so a dominant class
// keeps its small e_k. QUAL = false compiles the block out: that
// instantiation is the kernel as it was before the quality output existed,
// and it is the one launched whenever qv is null.
template <bool QUAL>
__global__ __launch_bounds__(256) void head_fwd_kernel(
    const bf16* __restrict__ hseq,  // (T, B, HH)
    const bf16* __restrict__ w4,    // (NC, HH)
    const float* __restrict__ b4,   // (NC)
    float* __restrict__ logits,     // (B, T, NC) or nullptr
    uint8_t* __restrict__ amax,     // (B, T) or nullptr
    uint8_t* __restrict__ qv,       // (B, T, NC) quality units, QUAL only
    int T, int B) {
    __shared__ bf16 w[NC][HH];
    __shared__ float bias[NC];
    const int tid = threadIdx.x;
    for (int e = tid; e < NC * HH; e += 256) (&w[0][0])[e] = w4[e];
    if (tid < NC) bias[tid] = b4[tid];
    __syncthreads();

    const int row = blockIdx.x * 256 + tid;  // row over T*B, layout (T, B)
    if (row >= T * B) return;
    const int t = row / B, b = row % B;
    const bf16* x = hseq + (size_t)row * HH;

    float acc[NC] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < HH; k += 8) {
        bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + k);
#pragma unroll
        for (int o = 0; o < NC; ++o) {
            bf16x8 wv = *reinterpret_cast<const bf16x8*>(&w[o][k]);
#pragma unroll
            for (int q = 0; q < 8; ++q)
                acc[o] += float(xv[q]) * float(wv[q]);
        }
    }
#pragma unroll
    for (int o = 0; o < NC; ++o) acc[o] += bias[o];

    if (logits) {
        float* dst = logits + ((size_t)b * T + t) * NC;
#pragma unroll
        for (int o = 0; o < NC; ++o) dst[o] = acc[o];
    }
    if (amax) {
        int best = 0;
        float bv = acc[0];
#pragma unroll
        for (int o = 1; o < NC; ++o)
            if (acc[o] > bv) { bv = acc[o]; best = o; }
        amax[(size_t)b * T + t] = uint8_t(best);
    }
    if constexpr (QUAL) {
        float m = acc[0];
#pragma unroll
        for (int o = 1; o < NC; ++o) m = fmaxf(m, acc[o]);
        float tj[NC], total = 0.f;
#pragma unroll
        for (int o = 0; o < NC; ++o) {
            tj[o] = expf(acc[o] - m);
            total += tj[o];
        }
        uint8_t* dst = qv + ((size_t)b * T + t) * NC;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            float others = 0.f;
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (j != k) others += tj[j];
            const float e = others / total;
            // -40 log10(e) >= 0 up to rounding; fmaxf also maps NaN to 0
            const float u = fminf(fmaxf(-40.f * log10f(e), 0.f), 255.f);
            dst[k] = e > 0.f ? uint8_t(floorf(u + 0.5f)) : uint8_t(255);
        }
    }
}

// qv: optional (B, T, NC) u8 quality units; null launches the kernel without
// the quality block
void head_fwd(const void* hseq, const void* w4, const float* b4, float* logits,
              uint8_t* amax, int T, int B, hipStream_t stream, uint8_t* qv) {
    const int rows = T * B;
    const dim3 grid((rows + 255) / 256), block(256);
    const bf16* h = static_cast<const bf16*>(hseq);
    const bf16* w = static_cast<const bf16*>(w4);
    if (qv)
        hipLaunchKernelGGL(head_fwd_kernel<true>, grid, block, 0, stream, h, w,
                           b4, logits, amax, qv, T, B);
    else
        hipLaunchKernelGGL(head_fwd_kernel<false>, grid, block, 0, stream, h,
                           w, b4, logits, amax, qv, T, B);
}

}  // namespace rk
