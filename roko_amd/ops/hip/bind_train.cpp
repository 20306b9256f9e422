// Bindings of the training kernels and the CU-masked stream.

#include "api.h"
#include "bind_util.h"

namespace {

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
    const int B = check_front(ids, w1, "w1", b1, w2, b2, emb);
    auto out = torch::empty({90, B, 500}, ids.options().dtype(torch::kBFloat16));
    rk::front_fwd(ids.data_ptr<uint8_t>(), w1.data_ptr(), b1.data_ptr<float>(),
                  w2.data_ptr(), b2.data_ptr<float>(), emb.data_ptr(),
                  out.data_ptr(), B, (uint32_t)seed, (float)keep, cur_stream(),
                  seed_ptr_of(seed_buf));
    return out;
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

}  // namespace

void bind_train(py::module_& m) {
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
    m.def("gru_wgrads", &gru_wgrads);
    m.def("head_wgrads", &head_wgrads);
    m.def("front_de_timed", &front_de_timed, py::arg("ids"), py::arg("dt1g"),
          py::arg("w1"), py::arg("seed"), py::arg("keep"), py::arg("dbg") = 0);
    m.def("front_bwd", &front_bwd, py::arg("ids"), py::arg("dseq"),
          py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
          py::arg("emb"), py::arg("seed"), py::arg("keep"),
          py::arg("phase_mask") = 0x1F, py::arg("seed_buf") = c10::nullopt);
    m.def("cu_masked_stream", &cu_masked_stream, py::arg("reserve_cus"));
}
