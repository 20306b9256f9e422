// Bindings of the model and eval kernels, with the timing and probe entries.

#include "api.h"
#include "bind_util.h"

namespace {

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
    const int B = check_front(ids, w1, "w1", b1, w2, b2, emb);
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
    const int B = check_front(ids, w1g, "w1g", b1, w2, b2, emb);
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
    const int B = check_front(ids, w1g, "w1g", b1, w2, b2, emb);
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

}  // namespace

void bind_model(py::module_& m) {
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
    m.def("head_fwd", &head_fwd, py::arg("hseq"), py::arg("w4"), py::arg("b4"),
          py::arg("want_logits") = true, py::arg("want_argmax") = false,
          py::arg("want_quality") = false);
}
