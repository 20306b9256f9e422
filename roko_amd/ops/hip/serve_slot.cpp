// Serving fast path: ONE C++ call enqueues the whole b-batch inference
// forward on a slot-owned HIP stream.
//
// Why this exists (profiles/PERF_HISTORY.md): the pipelined server is
// HOST-bound, not GPU-bound. A torch hipGraph replay costs ~51 us host time
// plus ~15 us per node (ROCm re-enqueues every node at launch), and extra
// Python threads do not help (a runtime-global lock serializes enqueue).
// Replacing the per-batch Python/graph work with one pybind call of direct
// kernel enqueues cuts the host cost to the raw HIP launches.

#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>
#include <c10/cuda/CUDAStream.h>

#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "api.h"
#include "bind_util.h"

namespace {

// What a slot launches, decided once when it is built (make_plan) and only
// read afterwards. ServeSlot.plan shows it to Python.
enum class Front { v2, v3, v4 };
enum class Xg { lt, fold, xg2, xg3, stream, wstat };

struct ServePlan {
    Front front = Front::v4;
    Xg xg[3] = {Xg::lt, Xg::lt, Xg::lt};  // per GRU layer
    int seq_ld = 500;    // row stride of the front output
    bool raw = false;    // every launch is a raw kernel enqueue, so the body
                         // is hipGraph capture-legal
    bool graph = false;  // the slot captures its body on the second run
};

const char* name_of(Front f) {
    return f == Front::v4 ? "v4" : f == Front::v3 ? "v3" : "v2";
}

const char* name_of(Xg x) {
    switch (x) {
        case Xg::lt: return "lt";
        case Xg::fold: return "fold";
        case Xg::xg2: return "xg2";
        case Xg::xg3: return "xg3";
        case Xg::stream: return "stream";
        case Xg::wstat: return "wstat";
    }
    return "?";
}

// The plan of a slot of B rows with the padded projection weights w_ih_p.
// The environment is read here, per slot, and nowhere else in this file.
//   ROKO_FRONT   v4 (default) | v2 | anything else: v3. v3 is the
//                wave-private front, v4 its persistent three-waves-per-SIMD
//                form, byte-identical; v2 is the chunked front.
//   ROKO_XGFOLD  1: the xg GEMM runs inside the GRU kernel (A/B only).
//   ROKO_XG2     0: hipBLASLt addmm for the projections, the path every
//                slot whose 90*B is no multiple of 256 takes anyway.
//   ROKO_XG3     0: xg_gemm2 and the 500-stride front output, the bit-exact
//                reference of xg_gemm3 and its successors.
//   ROKO_XG4     unset: the W-stationary kernel for the K = 256 layers of
//                slots wide enough for it to pay (xg_gemm4w_pays), xg_gemm3
//                for layer 0 and narrower slots. 0: xg_gemm3 everywhere.
//                wstat: W-stationary wherever its 256-row tiles fit.
//                stream: the persistent tile stream for all three layers
//                (the measured negative, kept as the A/B partner).
//   ROKO_GSLOT   1 | 0: capture the raw body into a hipGraph or not. Unset:
//                from B = 256 up, where one graph launch costs less host
//                time than the direct enqueues (it costs more at 128).
ServePlan make_plan(int B, const std::vector<torch::Tensor>& w_ih_p) {
    auto is = [](const char* f, const char* v) { return f && !strcmp(f, v); };
    const char* front = getenv("ROKO_FRONT");
    const char* xg4 = getenv("ROKO_XG4");
    const char* gslot = getenv("ROKO_GSLOT");
    const bool fold = is(getenv("ROKO_XGFOLD"), "1");
    const bool xg2 = !is(getenv("ROKO_XG2"), "0") && (90 * B) % 256 == 0;
    const int M = 90 * B;

    ServePlan p;
    p.front = (!front || is(front, "v4")) ? Front::v4
              : is(front, "v2")          ? Front::v2
                                         : Front::v3;
    p.raw = fold || xg2;
    if (!p.raw) return p;  // hipBLASLt: not capture-legal, so no graph
    p.graph = gslot ? is(gslot, "1") : B >= 256;
    if (fold) {
        p.xg[0] = p.xg[1] = p.xg[2] = Xg::fold;
        return p;
    }
    // xg3 needs a front that takes a leading dimension (v3, v4) and the
    // K-padded weight images its A rows are padded to match
    const bool xg3 = !is(getenv("ROKO_XG3"), "0") && p.front != Front::v2 &&
                     M % rk::xg_gemm3_tile_m() == 0 &&
                     w_ih_p[0].size(1) == 512 && w_ih_p[1].size(1) == 256 &&
                     w_ih_p[2].size(1) == 256;
    if (!xg3) {
        p.xg[0] = p.xg[1] = p.xg[2] = Xg::xg2;
        return p;
    }
    p.seq_ld = 512;
    p.xg[0] = p.xg[1] = p.xg[2] = Xg::xg3;
    if (is(xg4, "stream")) {
        p.xg[0] = p.xg[1] = p.xg[2] = Xg::stream;
    } else if (!is(xg4, "0")) {
        // W-stationary tiles are 256 rows, and a walker needs many rounds
        // of them to win: 1.09x at M = 92,160, 0.87x at 11,520
        const bool w = is(xg4, "wstat") ? M % rk::xg_gemm4w_tile_m() == 0
                                        : rk::xg_gemm4w_pays(M);
        if (w) p.xg[1] = p.xg[2] = Xg::wstat;
    }
    // the xg4 grids come from a device query: make it here, not under
    // stream capture
    if (p.xg[1] != Xg::xg3) (void)rk::xg_gemm4_cus();
    return p;
}

struct ServeSlot {
    // weights (kernel-ready layouts from roko_amd.ops.forward._bf16_weights)
    torch::Tensor b1, w2, b2, emb, w4, b4;
    torch::Tensor w1g;  // (112,232) zero-padded W1
    std::vector<torch::Tensor> w_ih_t, b_ih, u, bhh;
    std::vector<torch::Tensor> w_ih_p;  // (768, KP) row-padded
    ServePlan plan;
    // slot state + workspaces
    torch::Tensor x_buf;     // (B, 200, 90) u8 static input
    torch::Tensor seq;       // (90, B, seq_ld) bf16 front output; with
                             // seq_ld 512, cols 500..511 are zeroed once
                             // here and never written again
    torch::Tensor xg;        // (90*B, 768) bf16 per-layer gate inputs
    torch::Tensor hseq;      // (90, B, 2, 128) bf16 per-layer output
    torch::Tensor hseq2;     // ping-pong partner of hseq, fold only
    torch::Tensor amax;      // (B, 90) u8 fused-argmax predictions
    torch::Tensor qv;        // (B, 90, 5) u8 quality units; `quality` only
    bool quality = false;    // fixed at construction, so one captured graph
                             // per mode serves the slot's whole life
    torch::Tensor host_out;  // (B, 90) u8 pinned
    torch::Tensor seq2d, hseq2d;  // cached views for addmm_out
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
    // plan.graph until a capture fails; then the slot enqueues directly
    bool graph_ok = false;
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
        auto need = [&](const std::string& k) {
            TORCH_CHECK(w.contains(k.c_str()), "ServeSlot: no weight ", k);
            torch::Tensor v = w[k.c_str()].cast<torch::Tensor>();
            TORCH_CHECK(v.is_cuda() && v.is_contiguous(), "weight ", k);
            return v;
        };
        w1g = need("w1g"); b1 = need("b1"); w2 = need("w2"); b2 = need("b2");
        emb = need("emb"); w4 = need("w4"); b4 = need("b4");
        for (int l = 0; l < 3; ++l) {
            auto sfx = std::to_string(l);
            w_ih_t.push_back(need("w_ih_t" + sfx));
            w_ih_p.push_back(need("w_ih_p" + sfx));
            b_ih.push_back(need("b_ih" + sfx));
            u.push_back(need("u" + sfx));
            bhh.push_back(need("bhh" + sfx));
        }
        TORCH_CHECK(B % 32 == 0, "serving batch must be a multiple of 32");
        TORCH_CHECK(host_out_.is_pinned() && host_out_.scalar_type() == t::kUInt8
                        && host_out_.size(0) == B && host_out_.size(1) == 90,
                    "host_out must be pinned (B,90) u8");
        host_out = host_out_;
        plan = make_plan(B, w_ih_p);
        graph_ok = plan.graph;
        auto dev = b1.options();
        x_buf = t::zeros({B, 200, 90}, dev.dtype(t::kUInt8));
        // zeros, not empty: with pad columns the GEMM multiplies them by
        // W's zero padding, and 0 x NaN from stale memory is NaN
        seq = plan.seq_ld == 512
                  ? t::zeros({90, B, 512}, dev.dtype(t::kBFloat16))
                  : t::empty({90, B, 500}, dev.dtype(t::kBFloat16));
        xg = t::empty({(int64_t)90 * B, 768}, dev.dtype(t::kBFloat16));
        hseq = t::empty({90, B, 2, 128}, dev.dtype(t::kBFloat16));
        if (plan.xg[0] == Xg::fold)
            hseq2 = t::empty({90, B, 2, 128}, dev.dtype(t::kBFloat16));
        amax = t::empty({B, 90}, dev.dtype(t::kUInt8));
        if (quality) qv = t::zeros({B, 90, 5}, dev.dtype(t::kUInt8));
        seq2d = seq.view({(int64_t)90 * B, plan.seq_ld});  // lt: 500
        hseq2d = hseq.view({(int64_t)90 * B, 256});
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

    py::dict plan_dict() const {
        py::dict d;
        py::list layers;
        for (Xg x : plan.xg) layers.append(name_of(x));
        d["front"] = name_of(plan.front);
        d["xg"] = layers;
        d["seq_ld"] = plan.seq_ld;
        d["raw"] = plan.raw;
        d["graph"] = plan.graph;
        return d;
    }

    void launch_front(hipStream_t s) {
        const uint8_t* ids = x_buf.data_ptr<uint8_t>();
        const float* b1p = b1.data_ptr<float>();
        const float* b2p = b2.data_ptr<float>();
        switch (plan.front) {
            case Front::v4:
                rk::embed_mlp_fwd4(ids, w1g.data_ptr(), b1p, w2.data_ptr(),
                                   b2p, emb.data_ptr(), seq.data_ptr(), B, s,
                                   nullptr, plan.seq_ld);
                break;
            case Front::v3:
                rk::embed_mlp_fwd3(ids, w1g.data_ptr(), b1p, w2.data_ptr(),
                                   b2p, emb.data_ptr(), seq.data_ptr(), B, s,
                                   nullptr, plan.seq_ld);
                break;
            case Front::v2:  // no leading dimension: seq_ld is 500
                rk::embed_mlp_fwd2(ids, w1g.data_ptr(), b1p, w2.data_ptr(),
                                   b2p, emb.data_ptr(), seq.data_ptr(), B, s);
                break;
        }
    }

    // the model body on the slot stream `s`: front -> 3x(xg + GRU) -> head.
    // With plan.raw every call is a raw kernel enqueue on `s`, so the
    // sequence is hipGraph capture-legal.
    void enqueue_model(hipStream_t s) {
        launch_front(s);
        const void* fold_in = seq.data_ptr();
        for (int l = 0; l < 3; ++l) {
            const void* a = (l == 0 ? seq : hseq).data_ptr();
            const int kp = l == 0 ? 512 : 256;  // padded K, and lda of xg3 on
            const void* wp = w_ih_p[l].data_ptr();
            const void* bi = b_ih[l].data_ptr();
            switch (plan.xg[l]) {
                case Xg::fold: {  // projection and recurrence in one kernel
                    torch::Tensor& out_t = (l % 2) ? hseq2 : hseq;
                    rk::gru_layer_fwd_fused(
                        fold_in, wp, bi, u[l].data_ptr(),
                        bhh[l].data_ptr<float>(), xg.data_ptr(),
                        out_t.data_ptr(), 90, B, l == 0 ? 500 : 256,
                        (int)w_ih_p[l].size(1), s);
                    fold_in = out_t.data_ptr();
                    continue;
                }
                case Xg::lt: {  // hipBLASLt, on torch's current stream
                    at::cuda::CUDAStreamGuard guard(stream);
                    at::addmm_out(xg, b_ih[l], l == 0 ? seq2d : hseq2d,
                                  w_ih_t[l]);
                    break;
                }
                case Xg::xg2:
                    rk::xg_gemm2(a, wp, bi, xg.data_ptr(), 90 * B,
                                 l == 0 ? 500 : 256, (int)w_ih_p[l].size(1),
                                 s);
                    break;
                case Xg::xg3:
                    rk::xg_gemm3(a, kp, wp, bi, xg.data_ptr(), 90 * B, kp, s);
                    break;
                case Xg::stream:
                    rk::xg_gemm4(a, kp, wp, bi, xg.data_ptr(), 90 * B, kp, 0,
                                 s);
                    break;
                case Xg::wstat:  // K = 256 layers only
                    rk::xg_gemm4w(hseq.data_ptr(), 256, wp, bi, xg.data_ptr(),
                                  90 * B, 0, s);
                    break;
            }
            rk::gru_layer_fwd(xg.data_ptr(), u[l].data_ptr(),
                              bhh[l].data_ptr<float>(), hseq.data_ptr(),
                              nullptr, 90, B, s, 0);
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

    // Order the slot stream behind the current stream, the producer of the
    // tensors a submit reads. They may be caller-side temporaries (a dtype
    // or contiguity conversion in Python) that die when the submit returns
    // while the slot stream's reads are still queued: pin the storage of
    // those on the GPU to the slot stream, so the caching allocator cannot
    // hand the memory out early. Null entries are skipped.
    void follow_producer(std::initializer_list<const torch::Tensor*> reads) {
        auto prod = at::cuda::getCurrentCUDAStream();
        (void)hipEventRecord(ev_in, prod.stream());
        (void)hipStreamWaitEvent(stream.stream(), ev_in, 0);
        for (const torch::Tensor* t : reads)
            if (t && t->is_cuda())
                c10::cuda::CUDACachingAllocator::recordStream(
                    t->storage().data_ptr(), stream);
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
        follow_producer({&x});
        if (n == 0) return;
        if (plan.raw) {
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
        hipStream_t s = stream.stream();
        if (plan.raw) {
            // the first run executes eagerly (warms caches); with a graph
            // the second captures + launches and later runs just launch,
            // one hipGraphLaunch replacing the per-batch kernel enqueues
            if (graph_ok && !slot_gexec && n_runs >= 1)
                graph_ok = capture(s, true, slot_graph, slot_gexec);
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
            enqueue_model(s);
            host_out.copy_(amax, true);
        }
        unlaunched_parts = 0;
        (void)hipEventRecord(ev_done, s);
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
        // behind the producer of x/pos and of the table's zero fill
        follow_producer({&x, &pos, &table, &err_flag, qs ? &*qsum : nullptr});
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
        if (plan.raw && graph_ok && !votes_gexec && !votes_capture_failed &&
            n_runs >= 1)
            votes_capture_failed = !capture(s, false, votes_graph, votes_gexec);
        if (votes_gexec)
            (void)hipGraphLaunch(votes_gexec, s);
        else
            enqueue_model(s);
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
        (void)hipEventRecord(ev_done, s);
    }
};

}  // namespace

void bind_serve(py::module_& m) {
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
        .def_property_readonly("plan", &ServeSlot::plan_dict)
        .def_readonly("amax", &ServeSlot::amax)
        .def_readonly("qv", &ServeSlot::qv)
        .def_readonly("quality", &ServeSlot::quality)
        .def_readonly("host_out", &ServeSlot::host_out);
}
