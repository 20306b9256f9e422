// Torch bindings for the gfx950 kernels (roko_amd.ops._hip_ops).

#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>
#include <c10/cuda/CUDAStream.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

namespace rk {
void mfma_probe(const float* a, const float* b, float* d, hipStream_t stream);
void embed_mlp_fwd(const uint8_t* ids, const void* w1, const float* b1,
                   const void* w2, const float* b2, const void* emb, void* out,
                   int B, hipStream_t stream, uint32_t dbg,
                   unsigned long long* timing);
void embed_mlp_fwd2(const uint8_t* ids, const void* w1g, const float* b1,
                    const void* w2, const float* b2, const void* emb,
                    void* out, int B, hipStream_t stream);
void embed_mlp_fwd3(const uint8_t* ids, const void* w1g, const float* b1,
                    const void* w2, const float* b2, const void* emb,
                    void* out, int B, hipStream_t stream,
                    unsigned long long* timing, int ldo = 500);
void embed_mlp_fwd4(const uint8_t* ids, const void* w1g, const float* b1,
                    const void* w2, const float* b2, const void* emb,
                    void* out, int B, hipStream_t stream,
                    unsigned long long* timing, int ldo = 500,
                    int max_blocks = 0);
void gru_layer_fwd(const void* xg, const void* u, const float* bhh, void* hseq,
                   void* cache, int T, int B, hipStream_t stream, uint32_t dbg,
                   int impl = 0);
int gru_eval_select(int impl, int B);
void gru_layer_fwd_fused(const void* x, const void* w_ih_p, const void* b_ih,
                         const void* u, const float* bhh, void* xg_ws,
                         void* hseq, int T, int B, int IN, int KP,
                         hipStream_t stream);
void gru_layer_bwd(const void* cache, const void* hseq, const void* dhin,
                   const void* ut, void* dxg, void* dhg, int T, int B,
                   hipStream_t stream, uint32_t dbg);
void ce_fwd_bwd(const float* logits, const int64_t* target, float* dlogits,
                float* loss_sum, int64_t n, hipStream_t stream);
void adam_step(float* p, const float* g, float* m, float* v, int64_t n,
               float lr, float beta1, float beta2, float eps, int step,
               hipStream_t stream, const int* step_ptr);
void adam_mt(const int64_t* table, int n_params, float* p, float* m, float* v,
             float lr, float beta1, float beta2, float eps, int step,
             hipStream_t stream, const int* step_ptr);
void grad_gather(const int64_t* table, int n_params, float* flat_g,
                 hipStream_t stream);
void head_fwd(const void* hseq, const void* w4, const float* b4, float* logits,
              uint8_t* amax, int T, int B, hipStream_t stream,
              uint8_t* qv = nullptr);
void emb_grad(const void* dm, const uint8_t* ids, float* de, int64_t n,
              hipStream_t stream);
void front_fwd(const uint8_t* ids, const void* w1, const float* b1,
               const void* w2, const float* b2, const void* emb, void* out,
               int B, uint32_t seed, float keep, hipStream_t stream,
               const uint32_t* seed_ptr);
void front_bwd(const uint8_t* ids, const void* dseq, const void* w1,
               const float* b1, const void* w2, const float* b2,
               const void* emb, float* dw1, float* db1, float* dw2, float* db2,
               const void* w1t_g, float* de, int B, uint32_t seed, float keep,
               hipStream_t stream, uint32_t phase_mask,
               const uint32_t* seed_ptr, const void* w1g);
void gemm_bias(const void* A, const void* B, const float* bias, void* C,
               int M, int N, int K, hipStream_t stream);
void xg_gemm(const void* A, const void* B, const void* bias, void* C, int M,
             int KP, hipStream_t stream);
void xg_gemm2(const void* A, const void* Bt, const void* bias, void* C,
              int M, int KREAL, int KP, hipStream_t stream,
              unsigned long long* timing = nullptr);
void xg_gemm3(const void* A, int lda, const void* Bt, const void* bias,
              void* C, int M, int KP, hipStream_t stream);
int xg_gemm3_tile_m();
void xg_gemm3_stamped(const void* A, int lda, const void* Bt,
                      const void* bias, void* C, int M, int KP,
                      unsigned long long* stamps, hipStream_t stream);
int xg_gemm3_stamp_words();
void xg_gemm4(const void* A, int lda, const void* Bt, const void* bias,
              void* C, int M, int KP, int max_wgs, hipStream_t stream);
void xg_gemm4w(const void* A, int lda, const void* Bt, const void* bias,
               void* C, int M, int max_wgs, hipStream_t stream);
int xg_gemm4w_tile_m();
bool xg_gemm4w_pays(int M);
int xg_gemm4_cus();
int atb_splitk_nslices(int K);
void atb_splitk(const void* A, const void* B, float* ws, float* C, int M,
                int N, int K, hipStream_t stream);
void atb_splitk_ld(const void* A, int lda, const void* B, int ldb,
                   float* ws, float* C, int M, int N, int K,
                   hipStream_t stream);
void colsum_f32(const void* X, int ldx, int K, int N, float* out,
                float* part, hipStream_t stream);
void front_de(const uint8_t* ids, const void* dt1g, const void* w1t_g,
              float* de, int B, uint32_t seed, float keep, hipStream_t stream,
              unsigned long long* timing, uint32_t dbg,
              const uint32_t* seed_ptr);
void vote_scatter(const uint8_t* preds, const int32_t* positions,
                  uint32_t* table, int64_t n_slots, uint32_t* err_flag,
                  int n_cols, hipStream_t stream);
void vote_consensus(const uint32_t* table, int64_t n_slots, uint8_t* maj,
                    hipStream_t stream);
void vote_scatter_q(const uint8_t* preds, const uint8_t* units,
                    const int32_t* positions, uint32_t* table, uint64_t* qsum,
                    int64_t n_slots, uint32_t* err_flag, int n_cols,
                    hipStream_t stream);
void vote_consensus_q(const uint32_t* table, const uint64_t* qsum,
                      int64_t n_slots, uint8_t* maj, uint8_t* qual,
                      hipStream_t stream);
int64_t edit_num_blocks(int64_t n_pos);
void edit_count(const uint32_t* table, const uint8_t* draft, int64_t n_pos,
                int64_t* state, int64_t* counts, hipStream_t stream);
void edit_write(const uint32_t* table, const uint64_t* qsum,
                const uint8_t* draft, int64_t n_pos, const int64_t* state,
                const int64_t* offsets, void* records, int64_t total,
                hipStream_t stream);
bool windows_geometry_ok(int rows, int cols, int stride, int max_ins);
void windows_index(const int32_t* ref_start, const int32_t* ref_end,
                   const uint8_t* reverse, const uint32_t* cigar_off,
                   const uint32_t* seq_off, const uint32_t* cigar,
                   const uint8_t* seq4, int32_t* op_rpos, int32_t* op_qpos,
                   int n, int start, int end, int32_t* diff, int32_t* insd,
                   int32_t* col0, int32_t* colpos, int ncols_max,
                   int n_all_max, unsigned long long* mask, int32_t* wpre,
                   int32_t* nvalid, int32_t* out_idx, int32_t* meta,
                   hipStream_t stream);
void windows_fill(const int32_t* ref_start, const int32_t* ref_end,
                  const uint8_t* reverse, const uint32_t* cigar_off,
                  const uint32_t* seq_off, const uint32_t* cigar,
                  const uint8_t* seq4, int32_t* op_rpos, int32_t* op_qpos,
                  int n, int start, int end, const int32_t* col0,
                  const int32_t* colpos, const unsigned long long* mask,
                  const int32_t* wpre, const int32_t* nvalid,
                  const int32_t* out_idx, uint64_t region_key, int n_all,
                  int n_out, uint8_t* x, int32_t* pos, hipStream_t stream);
void truth_scan(const int32_t* ref_start, const int32_t* ref_end,
                const uint32_t* cigar_off, const uint32_t* seq_off,
                const uint32_t* cigar, const uint8_t* seq4, int32_t* op_rpos,
                int32_t* op_qpos, int n, int32_t* err, hipStream_t stream);
void label_windows(const int32_t* ref_start, const int32_t* ref_end,
                   const uint32_t* cigar_off, const uint32_t* seq_off,
                   const uint32_t* cigar, const uint8_t* seq4,
                   int32_t* op_rpos, int32_t* op_qpos, int n, int index,
                   int lo, int hi, const int32_t* pos, int n_windows,
                   uint8_t* labels, uint8_t* keep, int32_t* err,
                   hipStream_t stream);
void gather_batch(const uint8_t* X, const uint8_t* Y, const int32_t* idx,
                  uint8_t* out_x, int64_t* out_y, int64_t B,
                  hipStream_t stream);
void eval_metrics(const float* logits, const uint8_t* labels, int64_t n,
                  double inv_n, uint64_t* correct, double* loss_sum,
                  hipStream_t stream);
}  // namespace rk

namespace {

hipStream_t cur_stream() {
    return at::cuda::getCurrentCUDAStream().stream();
}

void check(const torch::Tensor& t, torch::ScalarType dt, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t.scalar_type() == dt, name, " has wrong dtype");
}

torch::Tensor mfma_probe(torch::Tensor a, torch::Tensor b) {
    check(a, torch::kFloat32, "a");
    check(b, torch::kFloat32, "b");
    TORCH_CHECK(a.sizes() == torch::IntArrayRef({16, 32}), "a must be (16,32)");
    TORCH_CHECK(b.sizes() == torch::IntArrayRef({32, 16}), "b must be (32,16)");
    auto d = torch::empty({16, 16}, a.options());
    rk::mfma_probe(a.data_ptr<float>(), b.data_ptr<float>(), d.data_ptr<float>(),
                   cur_stream());
    return d;
}

// ids (B, 200, 90) u8 -> (90, B, 500) bf16
torch::Tensor embed_mlp_fwd(torch::Tensor ids, torch::Tensor w1, torch::Tensor b1,
                            torch::Tensor w2, torch::Tensor b2, torch::Tensor emb,
                            int64_t dbg = 0,
                            c10::optional<torch::Tensor> timing = c10::nullopt) {
    check(ids, torch::kUInt8, "ids");
    check(w1, torch::kBFloat16, "w1");
    check(b1, torch::kFloat32, "b1");
    check(w2, torch::kBFloat16, "w2");
    check(b2, torch::kFloat32, "b2");
    check(emb, torch::kBFloat16, "emb");
    const int B = ids.size(0);
    TORCH_CHECK(ids.size(1) == 200 && ids.size(2) == 90, "ids must be (B,200,90)");
    TORCH_CHECK(w1.size(0) == 100 && w1.size(1) == 200, "w1 must be (100,200)");
    TORCH_CHECK(w2.size(0) == 10 && w2.size(1) == 100, "w2 must be (10,100)");
    TORCH_CHECK(emb.size(0) == 12 && emb.size(1) == 50, "emb must be (12,50)");
    auto out = torch::empty({90, B, 500}, ids.options().dtype(torch::kBFloat16));
    rk::embed_mlp_fwd(ids.data_ptr<uint8_t>(), w1.data_ptr(), b1.data_ptr<float>(),
                      w2.data_ptr(), b2.data_ptr<float>(), emb.data_ptr(),
                      out.data_ptr(), B, cur_stream(), dbg,
                      timing ? reinterpret_cast<unsigned long long*>(
                                   timing->data_ptr<int64_t>())
                             : nullptr);
    return out;
}

// ids (B, 200, 90) u8, w1g (112, 232) zero-padded -> (90, B, 500) bf16
torch::Tensor embed_mlp_fwd2(torch::Tensor ids, torch::Tensor w1g,
                             torch::Tensor b1, torch::Tensor w2,
                             torch::Tensor b2, torch::Tensor emb) {
    check(ids, torch::kUInt8, "ids");
    check(w1g, torch::kBFloat16, "w1g");
    check(b1, torch::kFloat32, "b1");
    check(w2, torch::kBFloat16, "w2");
    check(b2, torch::kFloat32, "b2");
    check(emb, torch::kBFloat16, "emb");
    const int B = ids.size(0);
    TORCH_CHECK(ids.size(1) == 200 && ids.size(2) == 90, "ids must be (B,200,90)");
    TORCH_CHECK(w1g.size(0) == 112 && w1g.size(1) == 232,
                "w1g must be (112,232) zero-padded");
    auto out = torch::empty({90, B, 500}, ids.options().dtype(torch::kBFloat16));
    rk::embed_mlp_fwd2(ids.data_ptr<uint8_t>(), w1g.data_ptr(),
                       b1.data_ptr<float>(), w2.data_ptr(),
                       b2.data_ptr<float>(), emb.data_ptr(), out.data_ptr(),
                       B, cur_stream());
    return out;
}

// same contract as embed_mlp_fwd2, wave-private-column kernels: v3 (one
// wave per SIMD, `version` 3) and v4 (persistent, three waves per SIMD)
torch::Tensor front_wave_private(int version, torch::Tensor ids,
                                 torch::Tensor w1g, torch::Tensor b1,
                                 torch::Tensor w2, torch::Tensor b2,
                                 torch::Tensor emb,
                                 c10::optional<torch::Tensor> timing,
                                 int64_t ldo,
                                 c10::optional<torch::Tensor> out_,
                                 int64_t max_blocks) {
    check(ids, torch::kUInt8, "ids");
    check(w1g, torch::kBFloat16, "w1g");
    check(b1, torch::kFloat32, "b1");
    check(w2, torch::kBFloat16, "w2");
    check(b2, torch::kFloat32, "b2");
    check(emb, torch::kBFloat16, "emb");
    const int B = ids.size(0);
    TORCH_CHECK(ids.size(1) == 200 && ids.size(2) == 90, "ids must be (B,200,90)");
    TORCH_CHECK(w1g.size(0) == 112 && w1g.size(1) == 232,
                "w1g must be (112,232) zero-padded");
    // ldo: output row stride. Columns [500, ldo) are never written, so a
    // padded output is returned zero-filled (or is the caller's `out`)
    TORCH_CHECK(ldo == 500 || (ldo > 500 && ldo % 8 == 0),
                "ldo must be 500 or a multiple of 8 above it");
    torch::Tensor out;
    if (out_.has_value()) {
        out = *out_;
        check(out, torch::kBFloat16, "out");
        TORCH_CHECK(out.dim() == 3 && out.size(0) == 90 && out.size(1) == B &&
                        out.size(2) == ldo, "out must be (90, B, ldo)");
    } else if (ldo == 500) {
        out = torch::empty({90, B, 500}, ids.options().dtype(torch::kBFloat16));
    } else {
        out = torch::zeros({90, B, ldo}, ids.options().dtype(torch::kBFloat16));
    }
    unsigned long long* tim =
        timing ? reinterpret_cast<unsigned long long*>(
                     timing->data_ptr<int64_t>())
               : nullptr;
    if (version == 4)
        rk::embed_mlp_fwd4(ids.data_ptr<uint8_t>(), w1g.data_ptr(),
                           b1.data_ptr<float>(), w2.data_ptr(),
                           b2.data_ptr<float>(), emb.data_ptr(),
                           out.data_ptr(), B, cur_stream(), tim, (int)ldo,
                           (int)max_blocks);
    else
        rk::embed_mlp_fwd3(ids.data_ptr<uint8_t>(), w1g.data_ptr(),
                           b1.data_ptr<float>(), w2.data_ptr(),
                           b2.data_ptr<float>(), emb.data_ptr(),
                           out.data_ptr(), B, cur_stream(), tim, (int)ldo);
    return out;
}

torch::Tensor embed_mlp_fwd3(torch::Tensor ids, torch::Tensor w1g,
                             torch::Tensor b1, torch::Tensor w2,
                             torch::Tensor b2, torch::Tensor emb,
                             c10::optional<torch::Tensor> timing = c10::nullopt,
                             int64_t ldo = 500,
                             c10::optional<torch::Tensor> out_ = c10::nullopt) {
    return front_wave_private(3, ids, w1g, b1, w2, b2, emb, timing, ldo, out_,
                              0);
}

// max_blocks > 0 caps the persistent grid (tests: several windows per
// workgroup at a small batch)
torch::Tensor embed_mlp_fwd4(torch::Tensor ids, torch::Tensor w1g,
                             torch::Tensor b1, torch::Tensor w2,
                             torch::Tensor b2, torch::Tensor emb,
                             c10::optional<torch::Tensor> timing = c10::nullopt,
                             int64_t ldo = 500,
                             c10::optional<torch::Tensor> out_ = c10::nullopt,
                             int64_t max_blocks = 0) {
    TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
    return front_wave_private(4, ids, w1g, b1, w2, b2, emb, timing, ldo, out_,
                              max_blocks);
}

// Serving fused variant: x (T, B, IN) bf16 + row-padded W_ih (768, KP) +
// b_ih (768) bf16 -> hseq; the xg GEMM runs inside the kernel.
torch::Tensor gru_layer_fused(torch::Tensor x, torch::Tensor w_ih_p,
                              torch::Tensor b_ih, torch::Tensor u,
                              torch::Tensor bhh) {
    check(x, torch::kBFloat16, "x");
    check(w_ih_p, torch::kBFloat16, "w_ih_p");
    check(b_ih, torch::kBFloat16, "b_ih");
    check(u, torch::kBFloat16, "u");
    check(bhh, torch::kFloat32, "bhh");
    const int T = x.size(0), B = x.size(1), IN = x.size(2);
    const int KP = w_ih_p.size(1);
    TORCH_CHECK(w_ih_p.size(0) == 768 && (KP == 256 || KP == 512) && KP >= IN,
                "w_ih_p must be (768, 256|512)");
    TORCH_CHECK(IN % 4 == 0, "IN must be a multiple of 4");
    TORCH_CHECK(B % 32 == 0, "batch must be a multiple of 32 (pad on host)");
    auto xg_ws = torch::empty({T, B, 2, 384}, x.options());
    auto hseq = torch::empty({T, B, 2, 128}, x.options());
    rk::gru_layer_fwd_fused(x.data_ptr(), w_ih_p.data_ptr(), b_ih.data_ptr(),
                            u.data_ptr(), bhh.data_ptr<float>(),
                            xg_ws.data_ptr(), hseq.data_ptr(), T, B, IN, KP,
                            cur_stream());
    return hseq;
}

// xg (T, B, 2, 384) bf16, u (2, 384, 128) bf16, bhh (2, 384) f32
//   -> (hseq (T, B, 2, 128) bf16 [, cache (T, B, 2, 512) bf16 when train])
std::vector<torch::Tensor> gru_layer_fwd(torch::Tensor xg, torch::Tensor u,
                                         torch::Tensor bhh, bool train,
                                         int64_t dbg, int64_t impl,
                                         c10::optional<torch::Tensor> out_buf) {
    check(xg, torch::kBFloat16, "xg");
    check(u, torch::kBFloat16, "u");
    check(bhh, torch::kFloat32, "bhh");
    const int T = xg.size(0), B = xg.size(1);
    TORCH_CHECK(xg.size(2) == 2 && xg.size(3) == 384, "xg must be (T,B,2,384)");
    TORCH_CHECK(u.size(0) == 2 && u.size(1) == 384 && u.size(2) == 128,
                "u must be (2,384,128)");
    TORCH_CHECK(bhh.size(0) == 2 && bhh.size(1) == 384, "bhh must be (2,384)");
    // the 16-row eval tile takes any multiple of 16; training keeps 32
    TORCH_CHECK(B % 32 == 0 || (!train && B % 16 == 0),
                "batch must be a multiple of 32 (eval: 16; pad on host)");
    TORCH_CHECK(T >= 1, "xg must hold at least one step");
    TORCH_CHECK(impl >= 0 && impl <= 4, "impl: 0 default, 1 old, 2 new; 3 new "
                "with the other hseq store, 4 new with xg staged through LDS");
    TORCH_CHECK(impl < 2 || !train, "impl 2..4 are eval kernels");
    torch::Tensor hseq;
    if (out_buf.has_value()) {  // caller-owned output (tests prefill it)
        hseq = *out_buf;
        check(hseq, torch::kBFloat16, "out");
        TORCH_CHECK(hseq.dim() == 4 && hseq.size(0) == T && hseq.size(1) == B &&
                        hseq.size(2) == 2 && hseq.size(3) == 128,
                    "out must be (T,B,2,128)");
    } else {
        hseq = torch::empty({T, B, 2, 128}, xg.options());
    }
    torch::Tensor cache;
    void* cp = nullptr;
    if (train) {
        cache = torch::empty({T, B, 2, 512}, xg.options());
        cp = cache.data_ptr();
    }
    rk::gru_layer_fwd(xg.data_ptr(), u.data_ptr(), bhh.data_ptr<float>(),
                      hseq.data_ptr(), cp, T, B, cur_stream(), (uint32_t)dbg,
                      (int)impl);
    std::vector<torch::Tensor> out{hseq};
    if (train) out.push_back(cache);
    return out;
}

// BPTT sequential backward -> dxg (T,B,2,384) [dxr dxz dxn] and
// dhg (2,T,B,384) [dxr dxz dhgn] in GEMM-ready layouts
std::vector<torch::Tensor> gru_layer_bwd(torch::Tensor cache, torch::Tensor hseq,
                                         torch::Tensor dhin, torch::Tensor ut,
                                         int64_t dbg = 0) {
    check(cache, torch::kBFloat16, "cache");
    check(hseq, torch::kBFloat16, "hseq");
    check(dhin, torch::kBFloat16, "dhin");
    check(ut, torch::kBFloat16, "ut");
    const int T = cache.size(0), B = cache.size(1);
    TORCH_CHECK(cache.size(2) == 2 && cache.size(3) == 512, "cache (T,B,2,512)");
    TORCH_CHECK(hseq.size(2) == 2 && hseq.size(3) == 128, "hseq (T,B,2,128)");
    TORCH_CHECK(dhin.sizes() == hseq.sizes(), "dhin must match hseq");
    TORCH_CHECK(ut.size(0) == 2 && ut.size(1) == 128 && ut.size(2) == 384,
                "ut must be (2,128,384)");
    auto dxg = torch::empty({T, B, 2, 384}, cache.options());
    auto dhg = torch::empty({2, T, B, 384}, cache.options());
    rk::gru_layer_bwd(cache.data_ptr(), hseq.data_ptr(), dhin.data_ptr(),
                      ut.data_ptr(), dxg.data_ptr(), dhg.data_ptr(), T, B,
                      cur_stream(), (uint32_t)dbg);
    return {dxg, dhg};
}

// fused CE: returns (loss scalar f32, dlogits (N,5) f32) for mean reduction
std::vector<torch::Tensor> ce_fwd_bwd(torch::Tensor logits, torch::Tensor target) {
    check(logits, torch::kFloat32, "logits");
    TORCH_CHECK(target.is_cuda() && target.is_contiguous(), "target");
    TORCH_CHECK(target.scalar_type() == torch::kInt64, "target must be int64");
    TORCH_CHECK(logits.dim() == 2 && logits.size(1) == 5, "logits must be (N,5)");
    const int64_t n = logits.size(0);
    TORCH_CHECK(target.numel() == n, "target size mismatch");
    auto dlogits = torch::empty_like(logits);
    auto loss = torch::zeros({1}, logits.options());
    rk::ce_fwd_bwd(logits.data_ptr<float>(), target.data_ptr<int64_t>(),
                   dlogits.data_ptr<float>(), loss.data_ptr<float>(), n,
                   cur_stream());
    return {loss.squeeze(0) / double(n), dlogits};
}

// fused Adam on flat fp32 buffers
void adam_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
               torch::Tensor v, double lr, double beta1, double beta2,
               double eps, int64_t step,
               c10::optional<torch::Tensor> step_buf) {
    check(p, torch::kFloat32, "p");
    check(g, torch::kFloat32, "g");
    check(m, torch::kFloat32, "m");
    check(v, torch::kFloat32, "v");
    const int64_t n = p.numel();
    TORCH_CHECK(g.numel() == n && m.numel() == n && v.numel() == n, "size mismatch");
    const int* sp = nullptr;
    if (step_buf.has_value()) {
        TORCH_CHECK(step_buf->is_cuda() &&
                    step_buf->scalar_type() == torch::kInt32);
        sp = step_buf->data_ptr<int>();
    }
    rk::adam_step(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                  v.data_ptr<float>(), n, float(lr), float(beta1), float(beta2),
                  float(eps), int(step), cur_stream(), sp);
}

// multi-tensor Adam: table rows [grad_ptr, flat_offset, numel] (GPU int64)
void adam_mt(torch::Tensor table, int64_t n_params, torch::Tensor p,
             torch::Tensor m, torch::Tensor v, double lr, double beta1,
             double beta2, double eps, int64_t step,
             c10::optional<torch::Tensor> step_buf) {
    TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kInt64);
    const int* sp = nullptr;
    if (step_buf.has_value()) {
        TORCH_CHECK(step_buf->is_cuda() &&
                    step_buf->scalar_type() == torch::kInt32);
        sp = step_buf->data_ptr<int>();
    }
    rk::adam_mt(table.data_ptr<int64_t>(), (int)n_params, p.data_ptr<float>(),
                m.data_ptr<float>(), v.data_ptr<float>(), (float)lr,
                (float)beta1, (float)beta2, (float)eps, (int)step,
                cur_stream(), sp);
}

void grad_gather(torch::Tensor table, int64_t n_params, torch::Tensor flat_g) {
    TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kInt64);
    rk::grad_gather(table.data_ptr<int64_t>(), (int)n_params,
                    flat_g.data_ptr<float>(), cur_stream());
}

// dm (N, 50) bf16 + ids (N) u8 -> dE (12, 50) f32
torch::Tensor emb_grad(torch::Tensor dm, torch::Tensor ids) {
    check(dm, torch::kBFloat16, "dm");
    check(ids, torch::kUInt8, "ids");
    TORCH_CHECK(dm.dim() == 2 && dm.size(1) == 50, "dm must be (N,50)");
    const int64_t n = dm.size(0);
    TORCH_CHECK(ids.numel() == n, "ids size mismatch");
    auto de = torch::zeros({12, 50}, dm.options().dtype(torch::kFloat32));
    rk::emb_grad(dm.data_ptr(), ids.data_ptr<uint8_t>(), de.data_ptr<float>(),
                 n, cur_stream());
    return de;
}

// hseq (T, B, 256) bf16 -> (logits (B,T,5) f32, argmax (B,T) u8, quality
// units (B,T,5) u8) per flags, in that order
std::vector<torch::Tensor> head_fwd(torch::Tensor hseq, torch::Tensor w4,
                                    torch::Tensor b4, bool want_logits,
                                    bool want_argmax,
                                    bool want_quality = false) {
    check(hseq, torch::kBFloat16, "hseq");
    check(w4, torch::kBFloat16, "w4");
    check(b4, torch::kFloat32, "b4");
    const int T = hseq.size(0), B = hseq.size(1);
    TORCH_CHECK(hseq.size(2) == 256, "hseq must be (T,B,256)");
    TORCH_CHECK(w4.size(0) == 5 && w4.size(1) == 256, "w4 must be (5,256)");
    torch::Tensor logits, amax, qv;
    float* lp = nullptr;
    uint8_t* ap = nullptr;
    uint8_t* qp = nullptr;
    if (want_logits) {
        logits = torch::empty({B, T, 5}, hseq.options().dtype(torch::kFloat32));
        lp = logits.data_ptr<float>();
    }
    if (want_argmax) {
        amax = torch::empty({B, T}, hseq.options().dtype(torch::kUInt8));
        ap = amax.data_ptr<uint8_t>();
    }
    if (want_quality) {
        qv = torch::empty({B, T, 5}, hseq.options().dtype(torch::kUInt8));
        qp = qv.data_ptr<uint8_t>();
    }
    rk::head_fwd(hseq.data_ptr(), w4.data_ptr(), b4.data_ptr<float>(), lp, ap,
                 T, B, cur_stream(), qp);
    std::vector<torch::Tensor> out;
    if (want_logits) out.push_back(logits);
    if (want_argmax) out.push_back(amax);
    if (want_quality) out.push_back(qv);
    return out;
}

// fused train front fwd: ids -> (W, B, 500) bf16 GRU input sequence
const uint32_t* seed_ptr_of(const c10::optional<torch::Tensor>& s) {
    if (!s.has_value()) return nullptr;
    TORCH_CHECK(s->is_cuda() && s->scalar_type() == torch::kInt32,
                "seed_buf must be a cuda int32 tensor");
    return reinterpret_cast<const uint32_t*>(s->data_ptr<int>());
}

torch::Tensor front_fwd(torch::Tensor ids, torch::Tensor w1, torch::Tensor b1,
                        torch::Tensor w2, torch::Tensor b2, torch::Tensor emb,
                        int64_t seed, double keep,
                        c10::optional<torch::Tensor> seed_buf) {
    check(ids, torch::kUInt8, "ids");
    check(w1, torch::kBFloat16, "w1");
    check(b1, torch::kFloat32, "b1");
    check(w2, torch::kBFloat16, "w2");
    check(b2, torch::kFloat32, "b2");
    check(emb, torch::kBFloat16, "emb");
    const int B = ids.size(0);
    TORCH_CHECK(ids.size(1) == 200 && ids.size(2) == 90, "ids must be (B,200,90)");
    auto out = torch::empty({90, B, 500}, ids.options().dtype(torch::kBFloat16));
    rk::front_fwd(ids.data_ptr<uint8_t>(), w1.data_ptr(), b1.data_ptr<float>(),
                  w2.data_ptr(), b2.data_ptr<float>(), emb.data_ptr(),
                  out.data_ptr(), B, (uint32_t)seed, (float)keep, cur_stream(),
                  seed_ptr_of(seed_buf));
    return out;
}

// serving xg projection: A (M, 256|512) bf16 x Bt (768, KP) + bias -> (M, 768)
torch::Tensor xg_gemm(torch::Tensor A, torch::Tensor Bt, torch::Tensor bias) {
    check(A, torch::kBFloat16, "A");
    check(Bt, torch::kBFloat16, "Bt");
    check(bias, torch::kBFloat16, "bias");
    const int M = A.size(0), KP = A.size(1);
    TORCH_CHECK(KP == 256 || KP == 512, "A must be (M, 256|512) K-padded");
    TORCH_CHECK(Bt.size(0) == 768 && Bt.size(1) == KP, "Bt must be (768, KP)");
    TORCH_CHECK(M % 256 == 0, "M must be a multiple of 256");
    auto C = torch::empty({M, 768}, A.options());
    rk::xg_gemm(A.data_ptr(), Bt.data_ptr(), bias.data_ptr(), C.data_ptr(),
                M, KP, cur_stream());
    return C;
}

// xg projection, LDS-staged specialized kernel: A (M, 500|512|256) bf16
// UNPADDED x Bt (768, KP) K-padded + bias -> (M, 768)
torch::Tensor xg_gemm2(torch::Tensor A, torch::Tensor Bt, torch::Tensor bias,
                       c10::optional<torch::Tensor> timing) {
    check(A, torch::kBFloat16, "A");
    check(Bt, torch::kBFloat16, "Bt");
    check(bias, torch::kBFloat16, "bias");
    const int M = A.size(0), KREAL = A.size(1), KP = Bt.size(1);
    TORCH_CHECK((KREAL == 500 && KP == 512) || (KREAL == 512 && KP == 512) ||
                    (KREAL == 256 && KP == 256),
                "unsupported (KREAL, KP): ", KREAL, " ", KP);
    TORCH_CHECK(Bt.size(0) == 768, "Bt must be (768, KP)");
    TORCH_CHECK(M % 256 == 0, "M must be a multiple of 256");
    auto C = torch::empty({M, 768}, A.options());
    unsigned long long* tptr = nullptr;
    if (timing.has_value())
        tptr = reinterpret_cast<unsigned long long*>(timing->data_ptr());
    rk::xg_gemm2(A.data_ptr(), Bt.data_ptr(), bias.data_ptr(), C.data_ptr(),
                 M, KREAL, KP, cur_stream(), tptr);
    return C;
}

// xg projection at the coalesced serving width (docs/KERNELS.md lesson 21):
// A (M, 256|512) bf16, rows 16-B aligned with any leading dimension (a
// column slice of a wider buffer is fine) x Bt (768, KP) + bias -> (M, 768).
// Byte-identical to xg_gemm2 on the same values. This is the argument
// contract xg_gemm3 and xg_gemm4 share; it returns the output tensor.
static torch::Tensor xg3_contract(const torch::Tensor& A,
                                  const torch::Tensor& Bt,
                                  const torch::Tensor& bias,
                                  c10::optional<torch::Tensor> out_,
                                  int64_t& lda) {
    check(Bt, torch::kBFloat16, "Bt");
    check(bias, torch::kBFloat16, "bias");
    TORCH_CHECK(A.is_cuda() && A.scalar_type() == torch::kBFloat16 &&
                    A.dim() == 2, "A must be a 2-D bf16 GPU tensor");
    const int64_t M = A.size(0), KP = A.size(1);
    TORCH_CHECK(KP == 256 || KP == 512, "A must be (M, 256|512)");
    lda = M > 1 ? A.stride(0) : KP;
    TORCH_CHECK(A.stride(1) == 1 && lda >= KP && lda % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(A.data_ptr()) % 16 == 0,
                "A rows must be unit-stride and 16-byte aligned");
    TORCH_CHECK(Bt.size(0) == 768 && Bt.size(1) == KP, "Bt must be (768, KP)");
    TORCH_CHECK(bias.numel() == 768, "bias must be (768)");
    TORCH_CHECK(M > 0 && M % rk::xg_gemm3_tile_m() == 0,
                "M must be a positive multiple of ", rk::xg_gemm3_tile_m());
    torch::Tensor C;
    if (out_.has_value()) {
        C = *out_;
        check(C, torch::kBFloat16, "out");
        TORCH_CHECK(C.dim() == 2 && C.size(0) == M && C.size(1) == 768,
                    "out must be (M, 768)");
    } else {
        C = torch::empty({M, 768}, A.options());
    }
    return C;
}

torch::Tensor xg_gemm3(torch::Tensor A, torch::Tensor Bt, torch::Tensor bias,
                       c10::optional<torch::Tensor> out_) {
    int64_t lda = 0;
    torch::Tensor C = xg3_contract(A, Bt, bias, out_, lda);
    rk::xg_gemm3(A.data_ptr(), (int)lda, Bt.data_ptr(), bias.data_ptr(),
                 C.data_ptr(), (int)A.size(0), (int)A.size(1), cur_stream());
    return C;
}

// xg_gemm3's successors (docs/KERNELS.md lesson 24): same contract,
// byte-identical output. form "stream" is the persistent tile stream (both
// K), "wstat" the W-stationary kernel (K = 256 and M % 256 == 0 only);
// "auto" takes wstat where it applies, else stream. max_wgs > 0 caps the
// grid; 0 is each form's default.
static bool xg4w_applies(int64_t M, int64_t KP) {
    return KP == 256 && M % rk::xg_gemm4w_tile_m() == 0;
}

torch::Tensor xg_gemm4(torch::Tensor A, torch::Tensor Bt, torch::Tensor bias,
                       c10::optional<torch::Tensor> out_, int64_t max_wgs,
                       const std::string& form) {
    int64_t lda = 0;
    torch::Tensor C = xg3_contract(A, Bt, bias, out_, lda);
    const int64_t M = A.size(0), KP = A.size(1);
    TORCH_CHECK(max_wgs >= 0 && max_wgs <= (1 << 20), "max_wgs out of range");
    TORCH_CHECK(form == "auto" || form == "stream" || form == "wstat",
                "form must be auto, stream or wstat");
    TORCH_CHECK(form != "wstat" || xg4w_applies(M, KP),
                "form wstat needs K = 256 and M % 256 == 0");
    if (form == "wstat" || (form == "auto" && xg4w_applies(M, KP)))
        rk::xg_gemm4w(A.data_ptr(), (int)lda, Bt.data_ptr(), bias.data_ptr(),
                      C.data_ptr(), (int)M, (int)max_wgs, cur_stream());
    else
        rk::xg_gemm4(A.data_ptr(), (int)lda, Bt.data_ptr(), bias.data_ptr(),
                     C.data_ptr(), (int)M, (int)KP, (int)max_wgs,
                     cur_stream());
    return C;
}

// The timing-only instantiation of xg_gemm3 (scripts/xg4_phases.py):
// returns (out, stamps) with stamps (workgroups, xg_gemm3_stamp_words) i64.
std::tuple<torch::Tensor, torch::Tensor> xg_gemm3_phases(
    torch::Tensor A, torch::Tensor Bt, torch::Tensor bias) {
    int64_t lda = 0;
    torch::Tensor C = xg3_contract(A, Bt, bias, c10::nullopt, lda);
    const int64_t nwg = A.size(0) / rk::xg_gemm3_tile_m() * 6;
    torch::Tensor stamps = torch::zeros(
        {nwg, (int64_t)rk::xg_gemm3_stamp_words()},
        A.options().dtype(torch::kInt64));
    rk::xg_gemm3_stamped(
        A.data_ptr(), (int)lda, Bt.data_ptr(), bias.data_ptr(), C.data_ptr(),
        (int)A.size(0), (int)A.size(1),
        reinterpret_cast<unsigned long long*>(stamps.data_ptr<int64_t>()),
        cur_stream());
    return {C, stamps};
}

// GRU layer weight gradients in ONE binding call: dU (both dirs, via
// strided-slice split-K AtB — the t-shifted h_prev pairing makes both
// operands regular slices, no torch.cat), dW_ih, and the three bias
// column-sums. The aten form of this section (cats, contiguous copies,
// ones-GEMVs, stack/float) cost ~1.3 ms of HOST enqueue per train step
// (kernel trace tr5) — this is 7 raw launches.
void gru_wgrads(torch::Tensor dhg,   // (2, T, B, 384) bf16, dir-major
                torch::Tensor dxg,   // (T*B, 768) bf16 view
                torch::Tensor hseq,  // (T, B, 2, 128) bf16
                torch::Tensor x,     // (T*B, IN) bf16
                torch::Tensor ws_u,  // (S', 384, 128) f32 scratch
                torch::Tensor ws_w,  // (S, 768, IN) f32 scratch
                torch::Tensor du,    // (2, 384, 128) f32 out
                torch::Tensor dw,    // (768, IN) f32 out
                torch::Tensor dbhh,  // (2, 384) f32 out
                torch::Tensor dbih)  // (768,) f32 out
{
    check(dhg, torch::kBFloat16, "dhg");
    check(dxg, torch::kBFloat16, "dxg");
    check(hseq, torch::kBFloat16, "hseq");
    check(x, torch::kBFloat16, "x");
    const int TB = dxg.size(0), IN = x.size(1);
    const int T = hseq.size(0), B = hseq.size(1);
    constexpr int H = 128, G3 = 384;
    TORCH_CHECK(T * B == TB && dhg.size(1) == T && dhg.size(2) == B,
                "shape mismatch");
    const int Kp = TB - B;
    TORCH_CHECK(ws_u.size(0) >= rk::atb_splitk_nslices(Kp) &&
                    ws_w.size(0) >= rk::atb_splitk_nslices(TB) &&
                    ws_w.size(2) >= IN,
                "workspace too small");
    hipStream_t s = cur_stream();
    const auto* dhg_f = static_cast<const uint16_t*>(dhg.data_ptr());
    const auto* dhg_r = dhg_f + (size_t)TB * G3;
    const auto* hs = static_cast<const uint16_t*>(hseq.data_ptr());
    float* du_p = du.data_ptr<float>();
    float* dbhh_p = dbhh.data_ptr<float>();
    // forward dir: dhg[t] x h[t-1] -> drop t=0 (h_prev = 0)
    rk::atb_splitk_ld(dhg_f + (size_t)B * G3, G3, hs, 2 * H,
                      ws_u.data_ptr<float>(), du_p, G3, H, Kp, s);
    // reverse dir: dhg[t] x h[t+1] -> drop t=T-1
    rk::atb_splitk_ld(dhg_r, G3, hs + (size_t)B * 2 * H + H, 2 * H,
                      ws_u.data_ptr<float>(), du_p + (size_t)G3 * H, G3, H,
                      Kp, s);
    rk::atb_splitk_ld(dxg.data_ptr(), 2 * G3, x.data_ptr(), IN,
                      ws_w.data_ptr<float>(), dw.data_ptr<float>(), 2 * G3,
                      IN, TB, s);
    float* part = ws_u.data_ptr<float>();  // scratch; stream-ordered reuse
    rk::colsum_f32(dhg_f, G3, TB, G3, dbhh_p, part, s);
    rk::colsum_f32(dhg_r, G3, TB, G3, dbhh_p + G3, part, s);
    rk::colsum_f32(dxg.data_ptr(), 2 * G3, TB, 2 * G3,
                   dbih.data_ptr<float>(), part, s);
}

// head weight gradients: dw4 = dl^T x seq, db4 = column sums of dl
void head_wgrads(torch::Tensor dl,    // (T*B, 5) bf16
                 torch::Tensor seq,   // (T*B, 256) bf16
                 torch::Tensor ws,    // (S, 5, 256) f32 scratch
                 torch::Tensor dw4,   // (5, 256) f32 out
                 torch::Tensor db4)   // (5,) f32 out
{
    check(dl, torch::kBFloat16, "dl");
    check(seq, torch::kBFloat16, "seq");
    const int TB = dl.size(0), N = seq.size(1), M = dl.size(1);
    hipStream_t s = cur_stream();
    rk::atb_splitk_ld(dl.data_ptr(), M, seq.data_ptr(), N,
                      ws.data_ptr<float>(), dw4.data_ptr<float>(), M, N, TB,
                      s);
    rk::colsum_f32(dl.data_ptr(), M, TB, M, db4.data_ptr<float>(),
                   ws.data_ptr<float>(), s);
}

// fused train front bwd: -> (de, dw1, db1, dw2, db2) fp32
std::vector<torch::Tensor> front_bwd(torch::Tensor ids, torch::Tensor dseq,
                                     torch::Tensor w1, torch::Tensor b1,
                                     torch::Tensor w2, torch::Tensor b2,
                                     torch::Tensor emb, int64_t seed,
                                     double keep, int64_t phase_mask,
                                     c10::optional<torch::Tensor> seed_buf) {
    check(ids, torch::kUInt8, "ids");
    check(dseq, torch::kBFloat16, "dseq");
    check(w1, torch::kBFloat16, "w1");
    check(b1, torch::kFloat32, "b1");
    check(w2, torch::kBFloat16, "w2");
    check(b2, torch::kFloat32, "b2");
    check(emb, torch::kBFloat16, "emb");
    const int B = ids.size(0);
    TORCH_CHECK(dseq.size(0) == 90 && dseq.size(1) == B && dseq.size(2) == 500,
                "dseq must be (90,B,500)");
    auto opt = b1.options();
    auto dw1 = torch::zeros({100, 200}, opt);
    auto db1 = torch::zeros({100}, opt);
    auto dw2 = torch::zeros({10, 100}, opt);
    auto db2 = torch::zeros({10}, opt);
    auto de = torch::zeros({12, 50}, opt);
    // zero-padded W1 images: W1^T (208,128) is LDS-staged for the dm GEMM,
    // W1 (112,232) feeds the G1 recompute's L2 A-fragments
    auto w1t_g = torch::zeros({208, 128}, w1.options());
    w1t_g.slice(0, 0, 200).slice(1, 0, 100).copy_(w1.t());
    auto w1g = torch::zeros({112, 232}, w1.options());
    w1g.slice(0, 0, 100).slice(1, 0, 200).copy_(w1);
    rk::front_bwd(ids.data_ptr<uint8_t>(), dseq.data_ptr(), w1.data_ptr(),
                  b1.data_ptr<float>(), w2.data_ptr(), b2.data_ptr<float>(),
                  emb.data_ptr(), dw1.data_ptr<float>(), db1.data_ptr<float>(),
                  dw2.data_ptr<float>(), db2.data_ptr<float>(),
                  w1t_g.data_ptr(), de.data_ptr<float>(), B, (uint32_t)seed,
                  (float)keep, cur_stream(), (uint32_t)phase_mask,
                  seed_ptr_of(seed_buf), w1g.data_ptr());
    return {de, dw1, db1, dw2, db2};
}

// standalone de kernel with optional cycle-timing output (4 uint64)
std::vector<torch::Tensor> front_de_timed(torch::Tensor ids, torch::Tensor dt1g,
                                          torch::Tensor w1, int64_t seed,
                                          double keep, int64_t dbg) {
    check(ids, torch::kUInt8, "ids");
    check(dt1g, torch::kBFloat16, "dt1g");
    check(w1, torch::kBFloat16, "w1");
    const int B = ids.size(0);
    auto de = torch::zeros({12, 50}, w1.options().dtype(torch::kFloat32));
    auto tim = torch::zeros({4}, w1.options().dtype(torch::kInt64));
    auto w1t_g = torch::zeros({208, 128}, w1.options());
    w1t_g.slice(0, 0, 200).slice(1, 0, 100).copy_(w1.t());
    rk::front_de(ids.data_ptr<uint8_t>(), dt1g.data_ptr(), w1t_g.data_ptr(),
                 de.data_ptr<float>(), B, (uint32_t)seed, (float)keep,
                 cur_stream(),
                 reinterpret_cast<unsigned long long*>(tim.data_ptr<int64_t>()),
                 (uint32_t)dbg, nullptr);
    return {de, tim};
}

// C (M,N) bf16 = A (M,K) bf16 · B (K,N) bf16 [+ bias f32]
torch::Tensor gemm_bias(torch::Tensor A, torch::Tensor B,
                        c10::optional<torch::Tensor> bias) {
    check(A, torch::kBFloat16, "A");
    check(B, torch::kBFloat16, "B");
    const int M = A.size(0), K = A.size(1), N = B.size(1);
    TORCH_CHECK(B.size(0) == K, "inner dims mismatch");
    const float* bp = nullptr;
    if (bias.has_value()) {
        check(*bias, torch::kFloat32, "bias");
        TORCH_CHECK(bias->numel() == N, "bias size");
        bp = bias->data_ptr<float>();
    }
    auto Cout = torch::empty({M, N}, A.options());
    rk::gemm_bias(A.data_ptr(), B.data_ptr(), bp, Cout.data_ptr(), M, N, K,
                  cur_stream());
    return Cout;
}

// C (M,N) f32 = A (K,M)^T · B (K,N), split-K with atomic accumulation
torch::Tensor atb_splitk(torch::Tensor A, torch::Tensor B) {
    check(A, torch::kBFloat16, "A");
    check(B, torch::kBFloat16, "B");
    const int K = A.size(0), M = A.size(1), N = B.size(1);
    TORCH_CHECK(B.size(0) == K, "inner dims mismatch");
    auto Cout = torch::empty({M, N}, A.options().dtype(torch::kFloat32));
    auto ws = torch::empty({rk::atb_splitk_nslices(K), M, N},
                           Cout.options());
    rk::atb_splitk(A.data_ptr(), B.data_ptr(), ws.data_ptr<float>(),
                   Cout.data_ptr<float>(), M, N, K, cur_stream());
    return Cout;
}

// ---------------------------------------------------------------------------
// Device votes (votes.hip). The packed table and the error flag are int32
// tensors on the Python side (torch has no first-class uint32); the kernels
// treat the same bits as uint32.
void check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    TORCH_CHECK(e == hipSuccess, what, " launch: ", hipGetErrorString(e));
}

uint32_t* vote_table_ptr(const torch::Tensor& table, int64_t n_slots) {
    check(table, torch::kInt32, "table");
    TORCH_CHECK(n_slots >= 0 && n_slots <= table.numel(),
                "n_slots exceeds the vote table");
    return reinterpret_cast<uint32_t*>(table.data_ptr<int32_t>());
}

uint32_t* vote_err_ptr(const torch::Tensor& err_flag) {
    check(err_flag, torch::kInt32, "err_flag");
    TORCH_CHECK(err_flag.numel() == 1, "err_flag must hold one int32");
    return reinterpret_cast<uint32_t*>(err_flag.data_ptr<int32_t>());
}

// preds (B, 90) u8 + positions (B, 90, 2) i32 -> one vote per column with
// pos >= 0 added into `table`
void vote_scatter(torch::Tensor preds, torch::Tensor positions,
                  torch::Tensor table, int64_t n_slots,
                  torch::Tensor err_flag) {
    check(preds, torch::kUInt8, "preds");
    check(positions, torch::kInt32, "positions");
    TORCH_CHECK(positions.dim() >= 1 && positions.size(-1) == 2 &&
                    positions.numel() == 2 * preds.numel(),
                "positions must be preds.shape + (2,)");
    TORCH_CHECK(preds.numel() < (int64_t(1) << 31), "batch too large");
    rk::vote_scatter(preds.data_ptr<uint8_t>(), positions.data_ptr<int32_t>(),
                     vote_table_ptr(table, n_slots), n_slots,
                     vote_err_ptr(err_flag), (int)preds.numel(), cur_stream());
    check_launch("vote kernel");
}

// table -> maj (n_slots) u8: majority class per slot, 0xFF where no votes
void vote_consensus(torch::Tensor table, int64_t n_slots, torch::Tensor maj) {
    check(maj, torch::kUInt8, "maj");
    TORCH_CHECK(maj.numel() >= n_slots, "maj shorter than n_slots");
    rk::vote_consensus(vote_table_ptr(table, n_slots), n_slots,
                       maj.data_ptr<uint8_t>(), cur_stream());
    check_launch("vote kernel");
}

// the quality table beside a count table: int64 on the Python side, one
// word per slot; the consensus kernel reads it in 16-byte pairs
uint64_t* vote_qsum_ptr(const torch::Tensor& qsum, int64_t n_slots) {
    check(qsum, torch::kInt64, "qsum");
    TORCH_CHECK(n_slots <= qsum.numel(), "n_slots exceeds the qsum table");
    return reinterpret_cast<uint64_t*>(qsum.data_ptr<int64_t>());
}

// vote_scatter plus the five quality units (preds.shape + (5,)) u8 of every
// column summed into `qsum`
void vote_scatter_q(torch::Tensor preds, torch::Tensor units,
                    torch::Tensor positions, torch::Tensor table,
                    torch::Tensor qsum, int64_t n_slots,
                    torch::Tensor err_flag) {
    check(preds, torch::kUInt8, "preds");
    check(units, torch::kUInt8, "units");
    check(positions, torch::kInt32, "positions");
    TORCH_CHECK(positions.dim() >= 1 && positions.size(-1) == 2 &&
                    positions.numel() == 2 * preds.numel(),
                "positions must be preds.shape + (2,)");
    TORCH_CHECK(units.dim() >= 1 && units.size(-1) == 5 &&
                    units.numel() == 5 * preds.numel(),
                "units must be preds.shape + (5,)");
    TORCH_CHECK(preds.numel() < (int64_t(1) << 31), "batch too large");
    rk::vote_scatter_q(preds.data_ptr<uint8_t>(), units.data_ptr<uint8_t>(),
                       positions.data_ptr<int32_t>(),
                       vote_table_ptr(table, n_slots),
                       vote_qsum_ptr(qsum, n_slots), n_slots,
                       vote_err_ptr(err_flag), (int)preds.numel(),
                       cur_stream());
    check_launch("vote kernel");
}

// (table, qsum) -> maj (n_slots) u8 as vote_consensus, and qual (n_slots) u8:
// Phred of the majority class, 0xFF where no votes
void vote_consensus_q(torch::Tensor table, torch::Tensor qsum,
                      int64_t n_slots, torch::Tensor maj, torch::Tensor qual) {
    check(maj, torch::kUInt8, "maj");
    check(qual, torch::kUInt8, "qual");
    TORCH_CHECK(maj.numel() >= n_slots && qual.numel() >= n_slots,
                "maj or qual shorter than n_slots");
    uint32_t* tab = vote_table_ptr(table, n_slots);
    uint64_t* qs = vote_qsum_ptr(qsum, n_slots);
    auto aligned = [](const void* p, uintptr_t a) {
        return reinterpret_cast<uintptr_t>(p) % a == 0;
    };
    TORCH_CHECK(aligned(tab, 16) && aligned(qs, 16) &&
                    aligned(maj.data_ptr(), 4) && aligned(qual.data_ptr(), 4),
                "vote tables must be 16-byte and outputs 4-byte aligned");
    rk::vote_consensus_q(tab, qs, n_slots, maj.data_ptr<uint8_t>(),
                         qual.data_ptr<uint8_t>(), cur_stream());
    check_launch("vote kernel");
}

// ---------------------------------------------------------------------------
// Polishing edits (edits.hip). `state` is int64[3] {s0, last voted slot,
// total}, set to {INT64_MAX, -1, 0} by the caller; `counts` holds one int64
// per 256-position workgroup and comes back as the workgroups' record
// offsets. The table holds exactly 4 slots per draft byte.
const uint8_t* edit_draft_ptr(const torch::Tensor& draft, int64_t n_slots) {
    check(draft, torch::kUInt8, "draft");
    TORCH_CHECK(draft.numel() * 4 == n_slots,
                "the table must hold 4 slots per draft byte");
    return draft.data_ptr<uint8_t>();
}

int64_t* edit_state_ptr(const torch::Tensor& state) {
    check(state, torch::kInt64, "state");
    TORCH_CHECK(state.numel() == 3, "state must hold three int64");
    return state.data_ptr<int64_t>();
}

int64_t* edit_counts_ptr(const torch::Tensor& counts, int64_t n_pos) {
    check(counts, torch::kInt64, "counts");
    TORCH_CHECK(counts.numel() == rk::edit_num_blocks(n_pos),
                "counts must hold one int64 per workgroup");
    return counts.data_ptr<int64_t>();
}

int64_t edit_num_blocks(int64_t n_pos) {
    TORCH_CHECK(n_pos >= 0, "negative length");
    return rk::edit_num_blocks(n_pos);
}

// bounds + per-workgroup counts + their exclusive scan, three kernels
void edit_count(torch::Tensor table, torch::Tensor draft, int64_t n_slots,
                torch::Tensor state, torch::Tensor counts) {
    uint32_t* tab = vote_table_ptr(table, n_slots);
    const uint8_t* dr = edit_draft_ptr(draft, n_slots);
    TORCH_CHECK(reinterpret_cast<uintptr_t>(tab) % 16 == 0,
                "vote tables must be 16-byte aligned");
    const int64_t n_pos = draft.numel();
    rk::edit_count(tab, dr, n_pos, edit_state_ptr(state),
                   edit_counts_ptr(counts, n_pos), cur_stream());
    check_launch("edit kernel");
}

// the records, `total` of them (state[2] as read back by the caller), 16
// bytes each, into `records` (int64, 2 words per record)
void edit_write(torch::Tensor table, torch::Tensor qsum, torch::Tensor draft,
                int64_t n_slots, torch::Tensor state, torch::Tensor offsets,
                torch::Tensor records, int64_t total) {
    uint32_t* tab = vote_table_ptr(table, n_slots);
    uint64_t* qs = vote_qsum_ptr(qsum, n_slots);
    const uint8_t* dr = edit_draft_ptr(draft, n_slots);
    check(records, torch::kInt64, "records");
    TORCH_CHECK(total >= 0 && records.numel() == 2 * total,
                "records must hold two int64 per edit");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(tab) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(records.data_ptr()) % 16 == 0,
                "vote tables and records must be 16-byte aligned");
    const int64_t n_pos = draft.numel();
    rk::edit_write(tab, qs, dr, n_pos, edit_state_ptr(state),
                   edit_counts_ptr(offsets, n_pos), records.data_ptr(), total,
                   cur_stream());
    check_launch("edit kernel");
}

// ---------------------------------------------------------------------------
// Device window builder (windows.hip): a region's packed reads -> (x (n, 200,
// 90) u8, pos (n, 90, 2) i32) on the current stream. The u32 offset and CIGAR
// arrays arrive as int32 tensors holding the same bits (no first-class uint32
// in torch); ops/windows.py has checked them against the array lengths.
// `ncols_max` bounds the region's column count (the scratch is sized by it).
// One 16-byte D2H read of the counts sits between the index kernels and the
// fill, so the window tensor is allocated at its exact size.
std::vector<torch::Tensor> build_windows(
    torch::Tensor ref_start, torch::Tensor ref_end, torch::Tensor reverse,
    torch::Tensor cigar_off, torch::Tensor seq_off, torch::Tensor cigar,
    torch::Tensor seq4, int64_t start, int64_t end, uint64_t region_key,
    int64_t ncols_max, int64_t rows, int64_t cols, int64_t stride,
    int64_t max_ins) {
    TORCH_CHECK(rk::windows_geometry_ok((int)rows, (int)cols, (int)stride,
                                        (int)max_ins),
                "build_windows is compiled for 200 rows x 90 columns, stride "
                "30, 3 insertion slots");
    check(ref_start, torch::kInt32, "ref_start");
    check(ref_end, torch::kInt32, "ref_end");
    check(reverse, torch::kUInt8, "reverse");
    check(cigar_off, torch::kInt32, "cigar_off");
    check(seq_off, torch::kInt32, "seq_off");
    check(cigar, torch::kInt32, "cigar");
    check(seq4, torch::kUInt8, "seq4");
    const int64_t n = ref_start.numel();
    TORCH_CHECK(ref_end.numel() == n && reverse.numel() == n &&
                    cigar_off.numel() == n + 1 && seq_off.numel() == n + 1,
                "per-read arrays disagree on the number of reads");
    const int64_t L = end - start;
    TORCH_CHECK(start >= 0 && L <= (int64_t(1) << 28) &&
                    end < (int64_t(1) << 31),
                "region out of range");
    TORCH_CHECK(n < (int64_t(1) << 31) && cigar.numel() < (int64_t(1) << 31),
                "too many reads or CIGAR ops in one region");
    auto i32 = ref_start.options();
    auto x = torch::empty({0, rows, cols}, reverse.options());
    auto pos = torch::empty({0, cols, 2}, i32);
    if (n == 0 || L <= 0 || cigar.numel() == 0) return {x, pos};
    TORCH_CHECK(ncols_max >= 0 && ncols_max <= L * (max_ins + 1),
                "ncols_max out of range");
    const int64_t n_all_max =
        ncols_max >= cols ? (ncols_max - cols) / stride + 1 : 0;
    const int64_t nwords = (n + 63) / 64, ngroups = (n + 255) / 256;
    TORCH_CHECK(n_all_max * ngroups < (int64_t(1) << 31),
                "region too large for one window build");

    auto op_rpos = torch::empty({cigar.numel()}, i32);
    auto op_qpos = torch::empty({cigar.numel()}, i32);
    auto zeros = torch::zeros({2 * L + 1 + 4}, i32);  // diff | insd | meta
    auto col0 = torch::empty({L + 1}, i32);
    auto colpos = torch::empty({std::max<int64_t>(ncols_max, 1)}, i32);
    auto mask = torch::empty({std::max<int64_t>(n_all_max * nwords, 1)},
                             i32.dtype(torch::kInt64));
    auto wpre = torch::empty({std::max<int64_t>(n_all_max * nwords, 1)}, i32);
    auto nvalid = torch::empty({std::max<int64_t>(n_all_max, 1)}, i32);
    auto out_idx = torch::empty({std::max<int64_t>(n_all_max, 1)}, i32);
    int32_t* diff = zeros.data_ptr<int32_t>();
    int32_t* insd = diff + L + 1;
    int32_t* meta = insd + L;
    auto u32 = [](const torch::Tensor& t) {
        return reinterpret_cast<const uint32_t*>(t.data_ptr<int32_t>());
    };
    auto mask_p =
        reinterpret_cast<unsigned long long*>(mask.data_ptr<int64_t>());
    hipStream_t s = cur_stream();
    rk::windows_index(ref_start.data_ptr<int32_t>(),
                      ref_end.data_ptr<int32_t>(), reverse.data_ptr<uint8_t>(),
                      u32(cigar_off), u32(seq_off), u32(cigar),
                      seq4.data_ptr<uint8_t>(), op_rpos.data_ptr<int32_t>(),
                      op_qpos.data_ptr<int32_t>(), (int)n, (int)start,
                      (int)end, diff, insd, col0.data_ptr<int32_t>(),
                      colpos.data_ptr<int32_t>(), (int)ncols_max,
                      (int)n_all_max, mask_p, wpre.data_ptr<int32_t>(),
                      nvalid.data_ptr<int32_t>(), out_idx.data_ptr<int32_t>(),
                      meta, s);
    check_launch("window index kernels");
    int32_t h[4];
    hipError_t e = hipMemcpyAsync(h, meta, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    TORCH_CHECK(e == hipSuccess, "window counts read-back: ",
                hipGetErrorString(e));
    TORCH_CHECK(!(h[3] & 2), "build_windows: the region has ", h[0],
                " columns, more than the bound ", ncols_max);
    TORCH_CHECK(!(h[3] & 1), "build_windows: zero-length CIGAR op in the "
                "region; the device builder does not take such reads "
                "(use the host extractor)");
    const int64_t n_all = h[1], n_out = h[2];
    TORCH_CHECK(n_all >= 0 && n_all <= n_all_max && n_out >= 0 &&
                    n_out <= n_all, "window counts out of range");
    if (n_out == 0) return {x, pos};
    x = torch::empty({n_out, rows, cols}, reverse.options());
    pos = torch::empty({n_out, cols, 2}, i32);
    rk::windows_fill(ref_start.data_ptr<int32_t>(),
                     ref_end.data_ptr<int32_t>(), reverse.data_ptr<uint8_t>(),
                     u32(cigar_off), u32(seq_off), u32(cigar),
                     seq4.data_ptr<uint8_t>(), op_rpos.data_ptr<int32_t>(),
                     op_qpos.data_ptr<int32_t>(), (int)n, (int)start, (int)end,
                     col0.data_ptr<int32_t>(), colpos.data_ptr<int32_t>(),
                     mask_p, wpre.data_ptr<int32_t>(),
                     nvalid.data_ptr<int32_t>(), out_idx.data_ptr<int32_t>(),
                     region_key, (int)n_all, (int)n_out,
                     x.data_ptr<uint8_t>(), pos.data_ptr<int32_t>(), s);
    check_launch("window fill kernel");
    return {x, pos};
}

// ---------------------------------------------------------------------------
// Truth labels (windows.hip). A truth pack is a contig's truth alignments in
// the read pack's layout, uploaded once; ops/labels_device.py has checked the
// offsets against the array lengths, as for build_windows.
static int64_t check_truth_pack(const torch::Tensor& ref_start,
                                const torch::Tensor& ref_end,
                                const torch::Tensor& cigar_off,
                                const torch::Tensor& seq_off,
                                const torch::Tensor& cigar,
                                const torch::Tensor& seq4) {
    check(ref_start, torch::kInt32, "ref_start");
    check(ref_end, torch::kInt32, "ref_end");
    check(cigar_off, torch::kInt32, "cigar_off");
    check(seq_off, torch::kInt32, "seq_off");
    check(cigar, torch::kInt32, "cigar");
    check(seq4, torch::kUInt8, "seq4");
    const int64_t n = ref_start.numel();
    TORCH_CHECK(ref_end.numel() == n && cigar_off.numel() == n + 1 &&
                    seq_off.numel() == n + 1,
                "per-alignment arrays disagree on the number of alignments");
    TORCH_CHECK(n < (int64_t(1) << 31) && cigar.numel() < (int64_t(1) << 31) &&
                    seq4.numel() < (int64_t(1) << 31),
                "truth pack too large");
    return n;
}

// -> [op_rpos, op_qpos, err (n)]: the per-op scan of every alignment and its
// refusal bits (1: zero-length op, 2: S/H/P between aligned ops).
std::vector<torch::Tensor> truth_scan(
    torch::Tensor ref_start, torch::Tensor ref_end, torch::Tensor cigar_off,
    torch::Tensor seq_off, torch::Tensor cigar, torch::Tensor seq4) {
    const int64_t n = check_truth_pack(ref_start, ref_end, cigar_off, seq_off,
                                       cigar, seq4);
    auto i32 = ref_start.options();
    auto op_rpos = torch::empty({cigar.numel()}, i32);
    auto op_qpos = torch::empty({cigar.numel()}, i32);
    auto err = torch::zeros({n}, i32);
    auto u32 = [](const torch::Tensor& t) {
        return reinterpret_cast<const uint32_t*>(t.data_ptr<int32_t>());
    };
    rk::truth_scan(ref_start.data_ptr<int32_t>(), ref_end.data_ptr<int32_t>(),
                   u32(cigar_off), u32(seq_off), u32(cigar),
                   seq4.data_ptr<uint8_t>(), op_rpos.data_ptr<int32_t>(),
                   op_qpos.data_ptr<int32_t>(), (int)n,
                   err.data_ptr<int32_t>(), cur_stream());
    check_launch("truth scan kernel");
    return {op_rpos, op_qpos, err};
}

// pos (n, 90, 2) i32 of built windows, one alignment of the scanned pack and
// its label span [lo, hi) -> [labels (n, 90) u8, keep (n) u8, err (1) i32]
// on the current stream. err bit 4: a column outside the span.
std::vector<torch::Tensor> label_windows(
    torch::Tensor pos, torch::Tensor ref_start, torch::Tensor ref_end,
    torch::Tensor cigar_off, torch::Tensor seq_off, torch::Tensor cigar,
    torch::Tensor seq4, torch::Tensor op_rpos, torch::Tensor op_qpos,
    int64_t align_index, int64_t lo, int64_t hi) {
    const int64_t n = check_truth_pack(ref_start, ref_end, cigar_off, seq_off,
                                       cigar, seq4);
    check(pos, torch::kInt32, "pos");
    check(op_rpos, torch::kInt32, "op_rpos");
    check(op_qpos, torch::kInt32, "op_qpos");
    TORCH_CHECK(pos.dim() == 3 && pos.size(1) == 90 && pos.size(2) == 2,
                "pos must be (n, 90, 2)");
    TORCH_CHECK(op_rpos.numel() == cigar.numel() &&
                    op_qpos.numel() == cigar.numel(),
                "the pack is not scanned (truth_scan)");
    TORCH_CHECK(align_index >= 0 && align_index < n,
                "align_index out of range");
    TORCH_CHECK(lo >= 0 && lo <= hi && hi < (int64_t(1) << 31),
                "label span out of range");
    const int64_t nw = pos.size(0);
    TORCH_CHECK(nw < (int64_t(1) << 31) / 90, "too many windows");
    auto u8 = seq4.options();
    auto labels = torch::empty({nw, 90}, u8);
    auto keep = torch::empty({nw}, u8);
    auto err = torch::zeros({1}, pos.options());
    auto u32 = [](const torch::Tensor& t) {
        return reinterpret_cast<const uint32_t*>(t.data_ptr<int32_t>());
    };
    rk::label_windows(ref_start.data_ptr<int32_t>(),
                      ref_end.data_ptr<int32_t>(), u32(cigar_off),
                      u32(seq_off), u32(cigar), seq4.data_ptr<uint8_t>(),
                      op_rpos.data_ptr<int32_t>(), op_qpos.data_ptr<int32_t>(),
                      (int)n, (int)align_index, (int)lo, (int)hi,
                      pos.data_ptr<int32_t>(), (int)nw,
                      labels.data_ptr<uint8_t>(), keep.data_ptr<uint8_t>(),
                      err.data_ptr<int32_t>(), cur_stream());
    check_launch("label windows kernel");
    return {labels, keep, err};
}

// ---------------------------------------------------------------------------
// Serving fast path: ONE C++ call enqueues the whole b-batch inference
// forward on a slot-owned HIP stream.
//
// Why this exists (profiles/PERF_HISTORY.md): the pipelined server is
// HOST-bound, not GPU-bound. A torch hipGraph replay costs ~51 us host time
// plus ~15 us per node (ROCm re-enqueues every node at launch), so the
// 11-node forward graph costs ~200 us of host per batch, and extra Python
// threads do not help (a runtime-global lock serializes enqueue). Replacing
// the per-batch Python/graph work with one pybind call of direct kernel
// enqueues cuts the host cost to the raw HIP launches.
// default of ROKO_FRONT: v4 (true) or v3
constexpr bool FRONT_V4_DEFAULT = true;

struct ServeSlot {
    // weights (kernel-ready layouts from roko_amd.ops.forward._bf16_weights)
    torch::Tensor w1, b1, w2, b2, emb, w4, b4;
    torch::Tensor w1gt;  // (112,232) zero-padded W1 for the chunked front
    std::vector<torch::Tensor> w_ih_t, b_ih, u, bhh;
    std::vector<torch::Tensor> w_ih_p;  // (768, KP) row-padded, xg-fold path
    torch::Tensor hseq2;                // ping-pong buffer for the fold path
    // slot state + workspaces
    torch::Tensor x_buf;     // (B, 200, 90) u8 static input
    torch::Tensor seq;       // (90, B, seq_ld) bf16 front output; seq_ld is
                             // 500, or 512 on the xg3 path (cols 500..511
                             // zeroed once here and never written again)
    torch::Tensor xg;        // (90*B, 768) bf16 per-layer gate inputs
    torch::Tensor hseq;      // (90, B, 2, 128) bf16 per-layer output
    torch::Tensor amax;      // (B, 90) u8 fused-argmax predictions
    torch::Tensor qv;        // (B, 90, 5) u8 quality units; `quality` only
    bool quality = false;    // fixed at construction, so one captured graph
                             // per mode serves the slot's whole life
    torch::Tensor host_out;  // (B, 90) u8 pinned
    torch::Tensor seq2d, hseq2d, xg2d;  // cached views for addmm_out
    int B;
    // coalescing: the slot is filled in `parts` blocks of Bp = B / parts
    // rows (submit_part) and the model body is launched once per fill.
    // part_mask: parts received in this round; unlaunched_parts: parts
    // copied into x_buf that no launch has covered yet.
    int parts = 1, Bp = 0;
    uint64_t part_mask = 0;
    int unlaunched_parts = 0;
    at::cuda::CUDAStream stream;
    hipEvent_t ev_in = nullptr, ev_done = nullptr;
    // front kernel choice (ROKO_FRONT env; v3 measured 22.7M vs 19.8M
    // bases/s serving with v2, bit-exact). use_v3 covers both wave-private
    // kernels (they share the ldo contract); use_v4 picks the persistent
    // three-waves-per-SIMD one, byte-identical to v3 (ROKO_FRONT=v3 for A/B)
    bool use_v3 = [] {
        const char* f = getenv("ROKO_FRONT");
        return !(f && std::string(f) == "v2");
    }();
    bool use_v4 = [] {
        const char* f = getenv("ROKO_FRONT");
        return FRONT_V4_DEFAULT ? !(f && std::string(f) != "v4")
                                : (f && std::string(f) == "v4");
    }();
    // xg-GEMM fold into the GRU kernel (ROKO_XGFOLD=1 to enable for A/B)
    bool use_fold = [] {
        const char* f = getenv("ROKO_XGFOLD");
        return f && std::string(f) == "1";
    }();
    // specialized xg GEMM kernel (ROKO_XG2=0 to fall back to hipBLASLt)
    bool use_xg2 = [] {
        const char* f = getenv("ROKO_XG2");
        return !(f && std::string(f) == "0");
    }();
    // raw hipGraph per slot (ROKO_GSLOT=1 to enable): when the forward is
    // torch-free (xg2 or fold path — no hipBLASLt workspace allocs), the
    // whole kernel sequence is captured once and replayed with ONE
    // hipGraphLaunch per batch instead of ~8 kernel enqueues. MEASURED
    // NEGATIVE, default off: raw hipGraphLaunch costs MORE host time than
    // the 8 direct enqueues on ROCm 7 (26.6 vs 27.7 M bases/s at b=128 —
    // the round-1 "~15 us/node replay" cost is in the runtime, not in
    // torch's wrapper). The effective host-bound lever is batch size
    // (serve_soak sweep: b=128 26.6 -> b=512 38.1 M bases/s).
    // auto default (set in ctor): ON for batch >= 256 where it wins the
    // same-box A/B (b=512: 38.0 vs 36.4 M bases/s), OFF at b=128 where the
    // graph launch costs more than the direct enqueues (26.6 vs 27.7).
    // Re-measured with 4 hardware queues at the coalesced widths: the
    // graph wins at 256 / 512 / 1024 (29.5 / 33.3 / 35.3 vs 27.0 / 31.9 /
    // 34.8) and loses at 128 (19.9 vs 20.0) — the rule stands.
    // xg_gemm3 for the three projections (ROKO_XG3=0 keeps xg_gemm2 and the
    // 500-stride front output — the A/B partner and bit-exact reference)
    bool use_xg3 = [] {
        const char* f = getenv("ROKO_XG3");
        return !(f && std::string(f) == "0");
    }();
    // xg_gemm3's successors (lesson 24) on the xg3 path, selected per K.
    // Shipped: the W-stationary kernel for the K = 256 layers of slots wide
    // enough for it to pay (set in ctor), xg_gemm3 for layer 0 and for
    // narrower slots. ROKO_XG4=0 keeps xg_gemm3 everywhere; ROKO_XG4=wstat
    // takes the W-stationary kernel at every width it can run;
    // ROKO_XG4=stream takes the persistent tile stream for both K (the
    // measured negative, kept as the A/B partner).
    bool use_xg4 = [] {
        const char* f = getenv("ROKO_XG4");
        return !(f && std::string(f) == "0");
    }();
    // per layer family: 0 xg_gemm3, 1 stream, 2 W-stationary
    int xg4_k256 = 2, xg4_k512 = 0;
    bool use_gslot = false;
    bool xg2_path = false;   // set in ctor: raw (capture-legal) layer path
    bool xg3_path = false;   // set in ctor: xg2_path taken with xg_gemm3
    int seq_ld = 500;
    hipGraph_t slot_graph = nullptr;
    hipGraphExec_t slot_gexec = nullptr;
    int n_runs = 0;
    // votes mode (submit_votes): per-slot positions buffer, allocated on
    // first use, and a second captured graph of the model body WITHOUT the
    // prediction D2H — the vote scatter runs after it, outside the graph,
    // because its table pointer changes per contig
    torch::Tensor pos_buf;  // (B, 90, 2) i32
    hipGraph_t votes_graph = nullptr;
    hipGraphExec_t votes_gexec = nullptr;
    bool votes_capture_failed = false;

    ServeSlot(py::dict w, int B_, torch::Tensor host_out_, int parts_ = 1,
              bool quality_ = false)
        : quality(quality_), B(B_), parts(parts_),
          stream(at::cuda::getStreamFromPool(/*high_priority=*/false)) {
        namespace t = torch;
        TORCH_CHECK(parts >= 1 && parts <= 64 && B % parts == 0,
                    "parts must be in 1..64 and divide the slot batch");
        Bp = B / parts;
        auto need = [&](const char* k) {
            torch::Tensor v = w[k].cast<torch::Tensor>();
            TORCH_CHECK(v.is_cuda() && v.is_contiguous(), "weight ", k);
            return v;
        };
        w1 = need("w1"); b1 = need("b1"); w2 = need("w2"); b2 = need("b2");
        emb = need("emb"); w4 = need("w4"); b4 = need("b4");
        if (w.contains("w1g")) w1gt = need("w1g");
        for (int l = 0; l < 3; ++l) {
            auto sfx = std::to_string(l);
            w_ih_t.push_back(need(("w_ih_t" + sfx).c_str()));
            b_ih.push_back(need(("b_ih" + sfx).c_str()));
            u.push_back(need(("u" + sfx).c_str()));
            bhh.push_back(need(("bhh" + sfx).c_str()));
            if (w.contains(("w_ih_p" + sfx).c_str()))
                w_ih_p.push_back(need(("w_ih_p" + sfx).c_str()));
        }
        if (w_ih_p.size() != 3) {
            w_ih_p.clear();
            use_fold = false;
            use_xg2 = false;
        }
        xg2_path = use_xg2 && !w_ih_p.empty() && ((90 * B_) % 256) == 0;
        // xg3 needs the front that takes a leading dimension (v3) and the
        // K-padded layer-0 weight image its A rows are padded to match
        xg3_path = xg2_path && use_xg3 && !use_fold && use_v3 &&
                   w1gt.defined() && ((90 * B_) % rk::xg_gemm3_tile_m()) == 0 &&
                   w_ih_p[0].size(1) == 512 && w_ih_p[1].size(1) == 256 &&
                   w_ih_p[2].size(1) == 256;
        seq_ld = xg3_path ? 512 : 500;
        bool force_wstat = false;
        if (const char* f = getenv("ROKO_XG4")) {
            if (std::string(f) == "stream") xg4_k256 = xg4_k512 = 1;
            force_wstat = std::string(f) == "wstat";
        }
        if (!use_xg4 || !xg3_path) xg4_k256 = xg4_k512 = 0;
        // W-stationary tiles are 256 rows, and with one walker per 1/40 of
        // the m-tiles the kernel wins only where a walker has many rounds:
        // measured 1.09x at M = 92,160 (9 rounds) and 0.87x at 11,520 (45
        // m-tiles on 40 walkers). Narrower slots keep xg_gemm3 unless
        // ROKO_XG4=wstat forces it wherever it applies.
        if (xg4_k256 == 2 && !(force_wstat ? (90 * B_) % rk::xg_gemm4w_tile_m() == 0
                                           : rk::xg_gemm4w_pays(90 * B_)))
            xg4_k256 = 0;
        // the grid size comes from a device query: make it here, not under
        // stream capture
        if (xg4_k256 || xg4_k512) (void)rk::xg_gemm4_cus();
        if (const char* f = getenv("ROKO_GSLOT"))
            use_gslot = std::string(f) == "1";
        else
            use_gslot = B_ >= 256;
        TORCH_CHECK(B % 32 == 0, "serving batch must be a multiple of 32");
        TORCH_CHECK(host_out_.is_pinned() && host_out_.scalar_type() == t::kUInt8
                        && host_out_.size(0) == B && host_out_.size(1) == 90,
                    "host_out must be pinned (B,90) u8");
        host_out = host_out_;
        auto dev = w1.options();
        x_buf = t::zeros({B, 200, 90}, dev.dtype(t::kUInt8));
        // zeros, not empty: on the xg3 path the GEMM multiplies the pad
        // columns by W's zero padding, and 0 x NaN from stale memory is NaN
        seq = xg3_path ? t::zeros({90, B, 512}, dev.dtype(t::kBFloat16))
                       : t::empty({90, B, 500}, dev.dtype(t::kBFloat16));
        xg = t::empty({(int64_t)90 * B, 768}, dev.dtype(t::kBFloat16));
        hseq = t::empty({90, B, 2, 128}, dev.dtype(t::kBFloat16));
        if (use_fold) hseq2 = t::empty({90, B, 2, 128}, dev.dtype(t::kBFloat16));
        amax = t::empty({B, 90}, dev.dtype(t::kUInt8));
        if (quality) qv = t::zeros({B, 90, 5}, dev.dtype(t::kUInt8));
        seq2d = seq.view({(int64_t)90 * B, seq_ld});  // lt path: seq_ld 500
        hseq2d = hseq.view({(int64_t)90 * B, 256});
        xg2d = xg;
        (void)hipEventCreateWithFlags(&ev_in, hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&ev_done, hipEventDisableTiming);
    }
    ~ServeSlot() {
        if (slot_gexec) (void)hipGraphExecDestroy(slot_gexec);
        if (slot_graph) (void)hipGraphDestroy(slot_graph);
        if (votes_gexec) (void)hipGraphExecDestroy(votes_gexec);
        if (votes_graph) (void)hipGraphDestroy(votes_graph);
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_done) (void)hipEventDestroy(ev_done);
    }

    // the torch-free model body (front -> 3x(xg + GRU) -> head): every call
    // is a raw kernel enqueue on `s`, so the sequence is hipGraph
    // capture-legal. Callers guarantee use_fold || xg2_path.
    void enqueue_model(hipStream_t s) {
        if (w1gt.defined() && use_v3 && use_v4)
            rk::embed_mlp_fwd4(x_buf.data_ptr<uint8_t>(), w1gt.data_ptr(),
                               b1.data_ptr<float>(), w2.data_ptr(),
                               b2.data_ptr<float>(), emb.data_ptr(),
                               seq.data_ptr(), B, s, nullptr, seq_ld);
        else if (w1gt.defined() && use_v3)
            rk::embed_mlp_fwd3(x_buf.data_ptr<uint8_t>(), w1gt.data_ptr(),
                               b1.data_ptr<float>(), w2.data_ptr(),
                               b2.data_ptr<float>(), emb.data_ptr(),
                               seq.data_ptr(), B, s, nullptr, seq_ld);
        else if (w1gt.defined())
            rk::embed_mlp_fwd2(x_buf.data_ptr<uint8_t>(), w1gt.data_ptr(),
                               b1.data_ptr<float>(), w2.data_ptr(),
                               b2.data_ptr<float>(), emb.data_ptr(),
                               seq.data_ptr(), B, s);
        else
            rk::embed_mlp_fwd(x_buf.data_ptr<uint8_t>(), w1.data_ptr(),
                              b1.data_ptr<float>(), w2.data_ptr(),
                              b2.data_ptr<float>(), emb.data_ptr(),
                              seq.data_ptr(), B, s, 0, nullptr);
        if (use_fold) {
            const void* xin = seq.data_ptr();
            int in_dim = 500;
            for (int l = 0; l < 3; ++l) {
                torch::Tensor& out_t = (l % 2) ? hseq2 : hseq;
                rk::gru_layer_fwd_fused(
                    xin, w_ih_p[l].data_ptr(), b_ih[l].data_ptr(),
                    u[l].data_ptr(), bhh[l].data_ptr<float>(), xg.data_ptr(),
                    out_t.data_ptr(), 90, B, in_dim,
                    (int)w_ih_p[l].size(1), s);
                xin = out_t.data_ptr();
                in_dim = 256;
            }
        } else {
            for (int l = 0; l < 3; ++l) {
                const int xg4_form = l == 0 ? xg4_k512 : xg4_k256;
                if (xg4_form == 2)
                    rk::xg_gemm4w(hseq.data_ptr(), 256, w_ih_p[l].data_ptr(),
                                  b_ih[l].data_ptr(), xg.data_ptr(), 90 * B,
                                  0, s);
                else if (xg4_form == 1)
                    rk::xg_gemm4((l == 0 ? seq : hseq).data_ptr(),
                                 l == 0 ? 512 : 256, w_ih_p[l].data_ptr(),
                                 b_ih[l].data_ptr(), xg.data_ptr(), 90 * B,
                                 l == 0 ? 512 : 256, 0, s);
                else if (xg3_path)
                    rk::xg_gemm3((l == 0 ? seq : hseq).data_ptr(),
                                 l == 0 ? 512 : 256, w_ih_p[l].data_ptr(),
                                 b_ih[l].data_ptr(), xg.data_ptr(), 90 * B,
                                 l == 0 ? 512 : 256, s);
                else
                    rk::xg_gemm2((l == 0 ? seq : hseq).data_ptr(),
                                 w_ih_p[l].data_ptr(), b_ih[l].data_ptr(),
                                 xg.data_ptr(), 90 * B, l == 0 ? 500 : 256,
                                 (int)w_ih_p[l].size(1), s);
                rk::gru_layer_fwd(xg.data_ptr(), u[l].data_ptr(),
                                  bhh[l].data_ptr<float>(), hseq.data_ptr(),
                                  nullptr, 90, B, s, 0);
            }
        }
        rk::head_fwd(hseq.data_ptr(), w4.data_ptr(), b4.data_ptr<float>(),
                     nullptr, amax.data_ptr<uint8_t>(), 90, B, s,
                     quality ? qv.data_ptr<uint8_t>() : nullptr);
    }

    // capture the model body (plus the prediction D2H when `d2h`) into
    // graph/gexec; false (both left null) if any step fails
    bool capture(hipStream_t s, bool d2h, hipGraph_t& graph,
                 hipGraphExec_t& gexec) {
        hipError_t e =
            hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) return false;
        enqueue_model(s);
        if (d2h)
            (void)hipMemcpyAsync(host_out.data_ptr(), amax.data_ptr(),
                                 (size_t)B * 90, hipMemcpyDeviceToHost, s);
        e = hipStreamEndCapture(s, &graph);
        if (e != hipSuccess || !graph) {
            graph = nullptr;
            return false;
        }
        e = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
        if (e != hipSuccess) {
            (void)hipGraphDestroy(graph);
            graph = nullptr;
            gexec = nullptr;
            return false;
        }
        return true;
    }

    void try_capture(hipStream_t s) {
        if (!capture(s, true, slot_graph, slot_gexec)) use_gslot = false;
    }

    // the hipBLASLt model body (slot batches the specialised xg GEMM does
    // not cover): front -> 3x(addmm + GRU) -> head. The caller holds a
    // CUDAStreamGuard on the slot stream for addmm_out.
    void enqueue_model_lt(hipStream_t s) {
        if (w1gt.defined() && use_v3 && use_v4)
            rk::embed_mlp_fwd4(x_buf.data_ptr<uint8_t>(), w1gt.data_ptr(),
                               b1.data_ptr<float>(), w2.data_ptr(),
                               b2.data_ptr<float>(), emb.data_ptr(),
                               seq.data_ptr(), B, s, nullptr);
        else if (w1gt.defined() && use_v3)
            rk::embed_mlp_fwd3(x_buf.data_ptr<uint8_t>(), w1gt.data_ptr(),
                               b1.data_ptr<float>(), w2.data_ptr(),
                               b2.data_ptr<float>(), emb.data_ptr(),
                               seq.data_ptr(), B, s, nullptr);
        else if (w1gt.defined())
            rk::embed_mlp_fwd2(x_buf.data_ptr<uint8_t>(), w1gt.data_ptr(),
                               b1.data_ptr<float>(), w2.data_ptr(),
                               b2.data_ptr<float>(), emb.data_ptr(),
                               seq.data_ptr(), B, s);
        else
            rk::embed_mlp_fwd(x_buf.data_ptr<uint8_t>(), w1.data_ptr(),
                              b1.data_ptr<float>(), w2.data_ptr(),
                              b2.data_ptr<float>(), emb.data_ptr(),
                              seq.data_ptr(), B, s, 0, nullptr);
        for (int l = 0; l < 3; ++l) {
            at::addmm_out(xg2d, b_ih[l], l == 0 ? seq2d : hseq2d, w_ih_t[l]);
            rk::gru_layer_fwd(xg.data_ptr(), u[l].data_ptr(),
                              bhh[l].data_ptr<float>(), hseq.data_ptr(),
                              nullptr, 90, B, s, 0);
        }
        rk::head_fwd(hseq.data_ptr(), w4.data_ptr(), b4.data_ptr<float>(),
                     nullptr, amax.data_ptr<uint8_t>(), 90, B, s,
                     quality ? qv.data_ptr<uint8_t>() : nullptr);
    }

    // input half of a submit: order the slot stream behind the producer of
    // x and copy rows [0, n) of x into x_buf rows [row0, row0 + n). The read
    // of x is enqueued here, never deferred.
    void copy_in(const torch::Tensor& x, int64_t n, int64_t row0) {
        // x may live on the GPU or on (ideally pinned) host memory — the
        // copy into the static slot buffer below is D2D or H2D accordingly
        TORCH_CHECK(x.scalar_type() == torch::kUInt8 && x.is_contiguous() &&
                        n >= 0 && row0 >= 0 && row0 + n <= B &&
                        x.numel() >= n * 200 * 90,
                    "x must be contiguous u8, n <= slot batch");
        // order the slot stream behind the producer of x
        auto prod = at::cuda::getCurrentCUDAStream();
        (void)hipEventRecord(ev_in, prod.stream());
        (void)hipStreamWaitEvent(stream.stream(), ev_in, 0);
        // x may be a caller-side temporary (dtype/contiguity conversion in
        // Python) that dies when submit() returns while the copy below is
        // still queued on the slot stream; pin its storage to this stream so
        // the caching allocator cannot hand the memory out early.
        if (x.is_cuda())
            c10::cuda::CUDACachingAllocator::recordStream(
                x.storage().data_ptr(), stream);
        if (n == 0) return;
        if (use_fold || xg2_path) {
            (void)hipMemcpyAsync(
                x_buf.data_ptr<uint8_t>() + (size_t)row0 * 200 * 90,
                x.data_ptr(), (size_t)n * 200 * 90, hipMemcpyDefault,
                stream.stream());
        } else {
            at::cuda::CUDAStreamGuard guard(stream);
            x_buf.narrow(0, row0, n).copy_(x.narrow(0, 0, n), true);
        }
    }

    // model half of a submit: the whole forward at full slot width on the
    // slot stream, one D2H of amax into the pinned host_out, ev_done
    void launch_body() {
        if (use_fold || xg2_path) {
            // torch-free path: raw kernels, optionally one hipGraphLaunch
            // replacing the per-batch kernel enqueues
            hipStream_t s = stream.stream();
            // the first run executes eagerly (warms caches); the second
            // captures + launches; later runs just launch
            if (use_gslot && !slot_gexec && n_runs >= 1) try_capture(s);
            if (slot_gexec) {
                (void)hipGraphLaunch(slot_gexec, s);
            } else {
                enqueue_model(s);
                (void)hipMemcpyAsync(host_out.data_ptr(), amax.data_ptr(),
                                     (size_t)B * 90, hipMemcpyDeviceToHost,
                                     s);
            }
            ++n_runs;
        } else {
            at::cuda::CUDAStreamGuard guard(stream);
            enqueue_model_lt(stream.stream());
            host_out.copy_(amax, true);
        }
        unlaunched_parts = 0;
        (void)hipEventRecord(ev_done, stream.stream());
    }

    void run(torch::Tensor x, int64_t n) {
        copy_in(x, n, 0);
        part_mask = 0;
        launch_body();
    }

    // Coalesced submit: rows [0, n) of x become rows [part*Bp, part*Bp + n)
    // of the slot. The input copy is enqueued now (x may be freed or
    // overwritten as soon as this returns); the model body is enqueued once,
    // at full width, by the call that completes the round (every part seen).
    // Returns true when this call launched the body.
    bool submit_part(torch::Tensor x, int64_t n, int64_t part) {
        TORCH_CHECK(part >= 0 && part < parts && n <= Bp,
                    "part out of range or n > part rows");
        copy_in(x, n, part * Bp);
        part_mask |= uint64_t(1) << part;
        ++unlaunched_parts;
        const uint64_t full =
            parts == 64 ? ~uint64_t(0) : (uint64_t(1) << parts) - 1;
        if (part_mask != full) return false;
        part_mask = 0;
        launch_body();
        return true;
    }

    // Launch the body for a partly filled slot (rows of parts not yet
    // received hold stale input, like rows n..B of a short batch; their
    // predictions are ignored). The round is not reset: the parts still to
    // come land in their usual rows and the call that completes the round
    // launches the body again. Returns true if anything was launched.
    bool flush() {
        if (unlaunched_parts == 0) return false;
        launch_body();
        return true;
    }

    // parts copied into the slot that no launch has covered yet
    int64_t unlaunched() const { return unlaunched_parts; }

    void sync() {
        hipError_t e = hipEventSynchronize(ev_done);
        TORCH_CHECK(e == hipSuccess, "serve slot sync failed: ",
                    hipGetErrorString(e));
    }

    // one-call hot path. There is deliberately NO event sync here:
    // hipEventSynchronize costs ~80 us with ~32 live streams (measured —
    // it was the serving throughput bound), and stream ordering already
    // makes slot reuse safe (x_buf/host_out overwrites are enqueued on the
    // same slot stream, and tickets materialize() — which does sync —
    // before the pipeline reuses a slot's host_out). If a caller outruns
    // the GPU the AQL ring eventually blocks the enqueue: bounded, safe.
    void submit(torch::Tensor x, int64_t n) {
        run(std::move(x), n);
    }
    bool done() { return hipEventQuery(ev_done) == hipSuccess; }

    // Votes mode: H2D of x and pos, the model, then one vote per column of
    // rows 0..n added into `table` — all on the slot stream, and no D2H of
    // predictions. Rows n..B of x_buf still hold the previous tenant, so the
    // model does predict for them; they are kept from voting by pos = -1 in
    // the positions buffer (data, not a launch scalar, so the same route
    // serves the captured-graph and the eager body). All slots add into one
    // table from their own streams; the adds are atomic. The caller keeps
    // x/pos (pinned staging) untouched until sync(), and waits for every
    // slot's ev_done before reading the table.
    // With `qsum` (a quality slot only) the fused scatter also sums the
    // head's quality units into it.
    void submit_votes(torch::Tensor x, torch::Tensor pos, int64_t n,
                      torch::Tensor table, int64_t n_slots,
                      torch::Tensor err_flag,
                      c10::optional<torch::Tensor> qsum) {
        TORCH_CHECK(parts == 1, "votes mode needs an uncoalesced slot");
        TORCH_CHECK(!qsum.has_value() || quality,
                    "a qsum table needs a slot built with quality=True");
        uint64_t* qs = qsum.has_value() ? vote_qsum_ptr(*qsum, n_slots)
                                        : nullptr;
        TORCH_CHECK(x.scalar_type() == torch::kUInt8 && x.is_contiguous() &&
                        n >= 0 && n <= B && x.numel() >= n * 200 * 90,
                    "x must be contiguous u8 with n <= slot batch rows");
        TORCH_CHECK(pos.scalar_type() == torch::kInt32 && pos.is_contiguous()
                        && pos.numel() >= n * 180,
                    "pos must be contiguous i32 (>=n, 90, 2)");
        uint32_t* tab = vote_table_ptr(table, n_slots);
        uint32_t* err = vote_err_ptr(err_flag);
        if (!pos_buf.defined())
            pos_buf = torch::empty({B, 90, 2},
                                   x_buf.options().dtype(torch::kInt32));
        // order the slot stream behind the producer of x/pos and of the
        // table's zero fill
        auto prod = at::cuda::getCurrentCUDAStream();
        (void)hipEventRecord(ev_in, prod.stream());
        (void)hipStreamWaitEvent(stream.stream(), ev_in, 0);
        for (const torch::Tensor* t : {&x, &pos, &table, &err_flag})
            if (t->is_cuda())
                c10::cuda::CUDACachingAllocator::recordStream(
                    t->storage().data_ptr(), stream);
        if (qs)
            c10::cuda::CUDACachingAllocator::recordStream(
                qsum->storage().data_ptr(), stream);
        at::cuda::CUDAStreamGuard guard(stream);
        hipStream_t s = stream.stream();
        if (n > 0) {
            (void)hipMemcpyAsync(x_buf.data_ptr(), x.data_ptr(),
                                 (size_t)n * 200 * 90, hipMemcpyDefault, s);
            (void)hipMemcpyAsync(pos_buf.data_ptr(), pos.data_ptr(),
                                 (size_t)n * 180 * sizeof(int32_t),
                                 hipMemcpyDefault, s);
        }
        if (n < B)  // every byte 0xFF -> pos = ins = -1: the row does not vote
            (void)hipMemsetAsync(pos_buf.data_ptr<int32_t>() + n * 180, 0xFF,
                                 (size_t)(B - n) * 180 * sizeof(int32_t), s);
        if (use_fold || xg2_path) {
            if (use_gslot && !votes_gexec && !votes_capture_failed &&
                n_runs >= 1)
                votes_capture_failed =
                    !capture(s, false, votes_graph, votes_gexec);
            if (votes_gexec)
                (void)hipGraphLaunch(votes_gexec, s);
            else
                enqueue_model(s);
        } else {
            enqueue_model_lt(s);
        }
        if (qs)
            rk::vote_scatter_q(amax.data_ptr<uint8_t>(),
                               qv.data_ptr<uint8_t>(),
                               pos_buf.data_ptr<int32_t>(), tab, qs, n_slots,
                               err, B * 90, s);
        else
            rk::vote_scatter(amax.data_ptr<uint8_t>(),
                             pos_buf.data_ptr<int32_t>(), tab, n_slots, err,
                             B * 90, s);
        ++n_runs;
        (void)hipEventRecord(ev_done, stream.stream());
    }
};

// Create a HIP stream restricted to all but the first `reserve_cus` CUs.
// Chip-wide kernels launched on it leave headroom for the latency-bound
// 8-workgroup GRU chain on the default/main stream (the deferred weight-grad
// GEMMs measured as BLOCKING the BPTT kernels when launched unmasked —
// profiles/PERF_HISTORY.md). Returned as an integer handle for
// torch.cuda.ExternalStream; lives for the process lifetime.
uint64_t cu_masked_stream(int64_t reserve_cus) {
    hipDeviceProp_t prop;
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipGetDeviceProperties(&prop, dev);
    const int ncu = prop.multiProcessorCount;
    TORCH_CHECK(reserve_cus >= 0 && reserve_cus < ncu, "bad reserve_cus");
    const int words = (ncu + 31) / 32;
    std::vector<uint32_t> mask(words, 0u);
    for (int cu = (int)reserve_cus; cu < ncu; ++cu)
        mask[cu / 32] |= (1u << (cu % 32));
    hipStream_t s = nullptr;
    hipError_t e = hipExtStreamCreateWithCUMask(&s, words, mask.data());
    TORCH_CHECK(e == hipSuccess, "hipExtStreamCreateWithCUMask: ",
                hipGetErrorString(e));
    return reinterpret_cast<uint64_t>(s);
}

// ---------------------------------------------------------------------------
// Device training data (batch.hip). gather_batch: X (N, 200, 90) u8, Y (N, 90)
// u8, idx (B) i32 -> out_x[b] = X[idx[b]], out_y[b] = int64(Y[idx[b]]), into
// caller-owned buffers on the current stream. idx is on the device and is NOT
// read here: ops/device_data.py checks 0 <= idx < N on the host, once per
// epoch, before it uploads the permutation.
void gather_batch(torch::Tensor X, torch::Tensor Y, torch::Tensor idx,
                  torch::Tensor out_x, torch::Tensor out_y) {
    check(X, torch::kUInt8, "X");
    check(Y, torch::kUInt8, "Y");
    check(idx, torch::kInt32, "idx");
    check(out_x, torch::kUInt8, "out_x");
    check(out_y, torch::kInt64, "out_y");
    TORCH_CHECK(X.dim() == 3 && X.size(1) == 200 && X.size(2) == 90,
                "X must be (N, 200, 90)");
    TORCH_CHECK(Y.dim() == 2 && Y.size(0) == X.size(0) && Y.size(1) == 90,
                "Y must be (N, 90) with X's N");
    TORCH_CHECK(X.size(0) >= 1, "X holds no windows");
    TORCH_CHECK(idx.dim() == 1 && idx.size(0) >= 1, "idx must be (B), B >= 1");
    const int64_t B = idx.size(0);
    TORCH_CHECK(B < (int64_t(1) << 31), "batch too large");
    TORCH_CHECK(out_x.dim() == 3 && out_x.size(0) == B &&
                    out_x.size(1) == 200 && out_x.size(2) == 90,
                "out_x must be (B, 200, 90)");
    TORCH_CHECK(out_y.dim() == 2 && out_y.size(0) == B && out_y.size(1) == 90,
                "out_y must be (B, 90)");
    TORCH_CHECK(Y.device() == X.device() && idx.device() == X.device() &&
                    out_x.device() == X.device() &&
                    out_y.device() == X.device(),
                "gather_batch tensors must share one device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(X.data_ptr()) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(out_x.data_ptr()) % 16 == 0,
                "X and out_x must be 16-byte aligned");
    c10::cuda::CUDAGuard guard(X.device());
    rk::gather_batch(X.data_ptr<uint8_t>(), Y.data_ptr<uint8_t>(),
                     idx.data_ptr<int32_t>(), out_x.data_ptr<uint8_t>(),
                     out_y.data_ptr<int64_t>(), B, cur_stream());
    check_launch("gather_batch kernel");
}

// eval_metrics: logits (B, 90, 5) f32, labels (B, 90) u8; acc (2) int64 on
// the Python side: word 0 is the count of correct columns, word 1 holds the
// bits of a double, the sum of `loss * inv_n` (torch has one dtype per
// tensor). Adds to acc on the current stream; no host sync.
void eval_metrics(torch::Tensor logits, torch::Tensor labels, double inv_n,
                  torch::Tensor acc) {
    check(logits, torch::kFloat32, "logits");
    check(labels, torch::kUInt8, "labels");
    check(acc, torch::kInt64, "acc");
    TORCH_CHECK(logits.dim() >= 1 && logits.size(-1) == 5,
                "logits must be (..., 5)");
    TORCH_CHECK(labels.numel() * 5 == logits.numel(),
                "labels must hold one class per logits row");
    TORCH_CHECK(acc.numel() == 2, "acc must hold two 64-bit words");
    TORCH_CHECK(labels.device() == logits.device() &&
                    acc.device() == logits.device(),
                "eval_metrics tensors must share one device");
    c10::cuda::CUDAGuard guard(logits.device());
    int64_t* a = acc.data_ptr<int64_t>();
    rk::eval_metrics(logits.data_ptr<float>(), labels.data_ptr<uint8_t>(),
                     labels.numel(), inv_n, reinterpret_cast<uint64_t*>(a),
                     reinterpret_cast<double*>(a + 1), cur_stream());
    check_launch("eval_metrics kernel");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "roko-mi355x CDNA4 kernels (gfx950)";
    m.def("mfma_probe", &mfma_probe);
    m.def("embed_mlp_fwd2", &embed_mlp_fwd2);
    m.def("embed_mlp_fwd3", &embed_mlp_fwd3, py::arg("ids"), py::arg("w1g"),
          py::arg("b1"), py::arg("w2"), py::arg("b2"), py::arg("emb"),
          py::arg("timing") = c10::nullopt, py::arg("ldo") = 500,
          py::arg("out") = c10::nullopt);
    m.def("embed_mlp_fwd4", &embed_mlp_fwd4, py::arg("ids"), py::arg("w1g"),
          py::arg("b1"), py::arg("w2"), py::arg("b2"), py::arg("emb"),
          py::arg("timing") = c10::nullopt, py::arg("ldo") = 500,
          py::arg("out") = c10::nullopt, py::arg("max_blocks") = 0);
    m.def("embed_mlp_fwd", &embed_mlp_fwd, py::arg("ids"), py::arg("w1"),
          py::arg("b1"), py::arg("w2"), py::arg("b2"), py::arg("emb"),
          py::arg("dbg") = 0, py::arg("timing") = c10::nullopt);
    m.def("gru_layer_fwd", &gru_layer_fwd, py::arg("xg"), py::arg("u"),
          py::arg("bhh"), py::arg("train") = false, py::arg("dbg") = 0,
          py::arg("impl") = 0, py::arg("out") = c10::nullopt);
    m.def("gru_eval_impl",
          [](int64_t B, int64_t impl) {
              return rk::gru_eval_select((int)impl, (int)B);
          },
          py::arg("B"), py::arg("impl") = 0,
          "which eval GRU kernel gru_layer_fwd(train=False, impl=impl) "
          "launches at batch B: 1 old, 2 transposed, 3 transposed with the "
          "other hseq store, 4 transposed with xg staged through LDS");
    m.def("gru_layer_fused", &gru_layer_fused, py::arg("x"), py::arg("w_ih_p"),
          py::arg("b_ih"), py::arg("u"), py::arg("bhh"));
    m.def("gru_layer_bwd", &gru_layer_bwd, py::arg("cache"), py::arg("hseq"),
          py::arg("dhin"), py::arg("ut"), py::arg("dbg") = 0);
    m.def("ce_fwd_bwd", &ce_fwd_bwd);
    m.def("adam_step", &adam_step, py::arg("p"), py::arg("g"),
          py::arg("m"), py::arg("v"), py::arg("lr"), py::arg("beta1"),
          py::arg("beta2"), py::arg("eps"), py::arg("step"),
          py::arg("step_buf") = c10::nullopt);
    m.def("adam_mt", &adam_mt, py::arg("table"), py::arg("n_params"),
          py::arg("p"), py::arg("m"), py::arg("v"), py::arg("lr"),
          py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
          py::arg("step"), py::arg("step_buf") = c10::nullopt);
    m.def("grad_gather", &grad_gather);
    m.def("emb_grad", &emb_grad);
    m.def("front_fwd", &front_fwd, py::arg("ids"), py::arg("w1"),
          py::arg("b1"), py::arg("w2"), py::arg("b2"), py::arg("emb"),
          py::arg("seed"), py::arg("keep"),
          py::arg("seed_buf") = c10::nullopt);
    m.def("atb_splitk", &atb_splitk);
    m.def("gemm_bias", &gemm_bias, py::arg("A"), py::arg("B"),
          py::arg("bias") = c10::nullopt);
    m.def("xg_gemm", &xg_gemm);
    m.def("gru_wgrads", &gru_wgrads);
    m.def("head_wgrads", &head_wgrads);
    m.def("xg_gemm2", &xg_gemm2, py::arg("A"), py::arg("Bt"), py::arg("bias"),
          py::arg("timing") = py::none());
    m.def("xg_gemm3", &xg_gemm3, py::arg("A"), py::arg("Bt"), py::arg("bias"),
          py::arg("out") = py::none());
    m.def("xg_gemm4", &xg_gemm4, py::arg("A"), py::arg("Bt"), py::arg("bias"),
          py::arg("out") = py::none(), py::arg("max_wgs") = 0,
          py::arg("form") = "auto");
    m.def("xg_gemm4_cus", [] { return rk::xg_gemm4_cus(); });
    m.def("xg_gemm3_phases", &xg_gemm3_phases, py::arg("A"), py::arg("Bt"),
          py::arg("bias"));
    m.def("front_de_timed", &front_de_timed, py::arg("ids"), py::arg("dt1g"),
          py::arg("w1"), py::arg("seed"), py::arg("keep"), py::arg("dbg") = 0);
    m.def("front_bwd", &front_bwd, py::arg("ids"), py::arg("dseq"),
          py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
          py::arg("emb"), py::arg("seed"), py::arg("keep"),
          py::arg("phase_mask") = 0x1F, py::arg("seed_buf") = c10::nullopt);
    m.def("head_fwd", &head_fwd, py::arg("hseq"), py::arg("w4"), py::arg("b4"),
          py::arg("want_logits") = true, py::arg("want_argmax") = false,
          py::arg("want_quality") = false);
    m.def("cu_masked_stream", &cu_masked_stream, py::arg("reserve_cus"));
    m.def("vote_scatter", &vote_scatter, py::arg("preds"),
          py::arg("positions"), py::arg("table"), py::arg("n_slots"),
          py::arg("err_flag"));
    m.def("vote_consensus", &vote_consensus, py::arg("table"),
          py::arg("n_slots"), py::arg("maj"));
    m.def("vote_scatter_q", &vote_scatter_q, py::arg("preds"),
          py::arg("units"), py::arg("positions"), py::arg("table"),
          py::arg("qsum"), py::arg("n_slots"), py::arg("err_flag"));
    m.def("vote_consensus_q", &vote_consensus_q, py::arg("table"),
          py::arg("qsum"), py::arg("n_slots"), py::arg("maj"),
          py::arg("qual"));
    m.def("edit_num_blocks", &edit_num_blocks, py::arg("n_pos"));
    m.def("edit_count", &edit_count, py::arg("table"), py::arg("draft"),
          py::arg("n_slots"), py::arg("state"), py::arg("counts"));
    m.def("edit_write", &edit_write, py::arg("table"), py::arg("qsum"),
          py::arg("draft"), py::arg("n_slots"), py::arg("state"),
          py::arg("offsets"), py::arg("records"), py::arg("total"));
    m.def("build_windows", &build_windows, py::arg("ref_start"),
          py::arg("ref_end"), py::arg("reverse"), py::arg("cigar_off"),
          py::arg("seq_off"), py::arg("cigar"), py::arg("seq4"),
          py::arg("start"), py::arg("end"), py::arg("region_key"),
          py::arg("ncols_max"), py::arg("rows"), py::arg("cols"),
          py::arg("stride"), py::arg("max_ins"));
    m.def("truth_scan", &truth_scan, py::arg("ref_start"), py::arg("ref_end"),
          py::arg("cigar_off"), py::arg("seq_off"), py::arg("cigar"),
          py::arg("seq4"));
    m.def("label_windows", &label_windows, py::arg("pos"),
          py::arg("ref_start"), py::arg("ref_end"), py::arg("cigar_off"),
          py::arg("seq_off"), py::arg("cigar"), py::arg("seq4"),
          py::arg("op_rpos"), py::arg("op_qpos"), py::arg("align_index"),
          py::arg("lo"), py::arg("hi"));
    m.def("gather_batch", &gather_batch, py::arg("X"), py::arg("Y"),
          py::arg("idx"), py::arg("out_x"), py::arg("out_y"));
    m.def("eval_metrics", &eval_metrics, py::arg("logits"), py::arg("labels"),
          py::arg("inv_n"), py::arg("acc"));
    py::class_<ServeSlot>(m, "ServeSlot")
        .def(py::init<py::dict, int, torch::Tensor, int, bool>(),
             py::arg("weights"), py::arg("batch"), py::arg("host_out"),
             py::arg("parts") = 1, py::arg("quality") = false)
        .def("run", &ServeSlot::run, py::arg("x"), py::arg("n"))
        .def("submit", &ServeSlot::submit, py::arg("x"), py::arg("n"),
             py::call_guard<py::gil_scoped_release>())
        .def("submit_part", &ServeSlot::submit_part, py::arg("x"),
             py::arg("n"), py::arg("part"),
             py::call_guard<py::gil_scoped_release>())
        .def("flush", &ServeSlot::flush,
             py::call_guard<py::gil_scoped_release>())
        .def("unlaunched", &ServeSlot::unlaunched)
        .def_readonly("parts", &ServeSlot::parts)
        .def("sync", &ServeSlot::sync,
             py::call_guard<py::gil_scoped_release>())
        .def("done", &ServeSlot::done)
        .def("submit_votes", &ServeSlot::submit_votes, py::arg("x"),
             py::arg("pos"), py::arg("n"), py::arg("table"),
             py::arg("n_slots"), py::arg("err_flag"),
             py::arg("qsum") = c10::nullopt,
             py::call_guard<py::gil_scoped_release>())
        .def_readonly("amax", &ServeSlot::amax)
        .def_readonly("qv", &ServeSlot::qv)
        .def_readonly("quality", &ServeSlot::quality)
        .def_readonly("host_out", &ServeSlot::host_out);
}
