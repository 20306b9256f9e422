// Training batches and validation metrics for a window set that lives in
// device memory (ops/device_data.py; the reference feeds train.py:18-129
// through a host DataLoader). Both kernels are memory-bound and tiny next to
// the 2.4 ms step: the gather moves 2.3 MB at b=128, the metrics read 20 B
// and one label per column (docs/KERNELS.md "Device training data").

#include <cstdint>

#include "api.h"
#include "common.h"

namespace rk {

constexpr int GB_ROW_BYTES = 200 * 90;          // one window, 18,000 B
constexpr int GB_ROW_VECS = GB_ROW_BYTES / 16;  // 1,125 16-byte vectors
constexpr int GB_COLS = 90;
constexpr int GB_CHUNKS = (GB_ROW_VECS + 255) / 256;  // 5 blocks per row
// the last chunk holds 1125 - 1024 = 101 vectors; its upper half is idle, so
// lanes [128, 218) of that block carry the row's 90 labels
constexpr int GB_LABEL_LANE0 = 128;
static_assert(GB_ROW_BYTES % 16 == 0, "rows are whole 16-byte vectors");
static_assert(GB_ROW_VECS - (GB_CHUNKS - 1) * 256 <= GB_LABEL_LANE0 &&
                  GB_LABEL_LANE0 + GB_COLS <= 256,
              "label lanes must be free lanes of the last chunk");

// out_x[b] = X[idx[b]], out_y[b] = int64(Y[idx[b]]). Block (b, chunk): one
// 16-byte load and store per lane, contiguous across the wave. The row offset
// is 64-bit: idx * 18000 passes 2^32 from row 238,610 on. idx is trusted: the
// host validated 0 <= idx < N before it uploaded the epoch's permutation.
__global__ __launch_bounds__(256) void gather_batch_kernel(
    const uint4* __restrict__ X,      // (N, 1125) vectors
    const uint8_t* __restrict__ Y,    // (N, 90)
    const int32_t* __restrict__ idx,  // (B)
    uint4* __restrict__ out_x,        // (B, 1125) vectors
    int64_t* __restrict__ out_y) {    // (B, 90)
    const int64_t b = blockIdx.x;
    const int chunk = blockIdx.y;
    const int64_t row = idx[b];
    const int v = chunk * 256 + (int)threadIdx.x;
    if (v < GB_ROW_VECS) {
        out_x[b * GB_ROW_VECS + v] = X[row * GB_ROW_VECS + v];
    } else if (chunk == GB_CHUNKS - 1) {
        const int c = (int)threadIdx.x - GB_LABEL_LANE0;
        if (c >= 0 && c < GB_COLS)
            out_y[b * GB_COLS + c] = (int64_t)Y[row * GB_COLS + c];
    }
}

void gather_batch(const uint8_t* X, const uint8_t* Y, const int32_t* idx,
                  uint8_t* out_x, int64_t* out_y, int64_t B,
                  hipStream_t stream) {
    if (B <= 0) return;
    hipLaunchKernelGGL(gather_batch_kernel, dim3((uint32_t)B, GB_CHUNKS),
                       dim3(256), 0, stream,
                       reinterpret_cast<const uint4*>(X), Y, idx,
                       reinterpret_cast<uint4*>(out_x), out_y);
}

// ---------------------------------------------------------------------------
// Validation metrics of one batch, no host sync: acc[0] (uint64) += columns
// whose argmax equals the label, acc[1] (double) += mean CE of the batch.
// A lane owns one column (5 logits). argmax ties go to the smallest class id
// (strict '>', as head.hip); the CE is ce.hip's: max-subtracted,
// logf(s) - (x[t] - m). Lanes reduce through the wave, waves through LDS, and
// one lane per block issues the two atomics. The loss is summed in fp64 from
// the lane on, so the result does not depend on how many batches were added.

constexpr int EM_CLS = 5;

__global__ __launch_bounds__(256) void eval_metrics_kernel(
    const float* __restrict__ logits,   // (n, 5)
    const uint8_t* __restrict__ labels, // (n)
    int64_t n, double inv_n, unsigned long long* __restrict__ correct,
    double* __restrict__ loss_sum) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double loss = 0.0;
    uint32_t hit = 0;
    if (row < n) {
        const float* p = logits + row * EM_CLS;
        float x[EM_CLS];
#pragma unroll
        for (int c = 0; c < EM_CLS; ++c) x[c] = p[c];
        const int t = labels[row];
        int best = 0;
        float m = x[0];
#pragma unroll
        for (int c = 1; c < EM_CLS; ++c)
            if (x[c] > m) { m = x[c]; best = c; }
        float s = 0.0f, xt = 0.0f;
#pragma unroll
        for (int c = 0; c < EM_CLS; ++c) {
            s += __expf(x[c] - m);
            xt = (c == t) ? x[c] : xt;  // select, never an indexed read
        }
        loss = (double)(logf(s) - (xt - m));
        hit = (best == t) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        loss += __shfl_down(loss, off, 64);
        hit += __shfl_down(hit, off, 64);
    }
    __shared__ double w_loss[4];
    __shared__ uint32_t w_hit[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        w_loss[wave] = loss;
        w_hit[wave] = hit;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double l = (w_loss[0] + w_loss[1]) + (w_loss[2] + w_loss[3]);
        const uint32_t h = w_hit[0] + w_hit[1] + w_hit[2] + w_hit[3];
        __hip_atomic_fetch_add(loss_sum, l * inv_n, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        if (h)
            __hip_atomic_fetch_add(correct, (unsigned long long)h,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

void eval_metrics(const float* logits, const uint8_t* labels, int64_t n,
                  double inv_n, uint64_t* correct, double* loss_sum,
                  hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(eval_metrics_kernel,
                       dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream,
                       logits, labels, n, inv_n,
                       reinterpret_cast<unsigned long long*>(correct),
                       loss_sum);
}

}  // namespace rk
