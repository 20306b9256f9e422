// Bindings of the data kernels: votes, edits, stitch, windows, truth labels, batch
// gather and eval metrics.

#include <c10/cuda/CUDAGuard.h>

#include <algorithm>
#include <vector>

#include "api.h"
#include "bind_util.h"

namespace {

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
// Device stitch (stitch.hip): the polished sequence and its quality string
// under the quality filter. `state` and `counts` are those of the edit
// kernels; `qsum` may be None (tables built without quality), and then
// min_qual is 0 and no quality string can be asked for.
const uint64_t* stitch_qsum_ptr(const c10::optional<torch::Tensor>& qsum,
                                int64_t n_slots, int64_t min_qual) {
    TORCH_CHECK(min_qual >= 0 && min_qual <= 60, "min_qual outside 0..60");
    if (!qsum.has_value()) {
        TORCH_CHECK(min_qual == 0, "min_qual > 0 needs the quality table");
        return nullptr;
    }
    return vote_qsum_ptr(*qsum, n_slots);
}

// bounds + bytes per workgroup + their exclusive scan, three kernels
void stitch_count(torch::Tensor table, c10::optional<torch::Tensor> qsum,
                  torch::Tensor draft, int64_t n_slots, torch::Tensor state,
                  torch::Tensor counts, int64_t min_qual,
                  bool keep_uncovered) {
    uint32_t* tab = vote_table_ptr(table, n_slots);
    const uint64_t* qs = stitch_qsum_ptr(qsum, n_slots, min_qual);
    const uint8_t* dr = edit_draft_ptr(draft, n_slots);
    TORCH_CHECK(reinterpret_cast<uintptr_t>(tab) % 16 == 0,
                "vote tables must be 16-byte aligned");
    const int64_t n_pos = draft.numel();
    rk::stitch_count(tab, qs, dr, n_pos, edit_state_ptr(state),
                     edit_counts_ptr(counts, n_pos), (int)min_qual,
                     keep_uncovered, cur_stream());
    check_launch("stitch kernel");
}

// the polished bytes, `total` of them (state[2] as read back by the caller),
// into `seq` and, if given, their Phred+33 qualities into `qual`
void stitch_write(torch::Tensor table, c10::optional<torch::Tensor> qsum,
                  torch::Tensor draft, int64_t n_slots, torch::Tensor state,
                  torch::Tensor offsets, int64_t min_qual, bool keep_uncovered,
                  torch::Tensor seq, c10::optional<torch::Tensor> qual,
                  int64_t total) {
    uint32_t* tab = vote_table_ptr(table, n_slots);
    const uint64_t* qs = stitch_qsum_ptr(qsum, n_slots, min_qual);
    const uint8_t* dr = edit_draft_ptr(draft, n_slots);
    check(seq, torch::kUInt8, "seq");
    TORCH_CHECK(total >= 0 && seq.numel() == total,
                "seq must hold one byte per polished base");
    uint8_t* ql = nullptr;
    if (qual.has_value()) {
        TORCH_CHECK(qs != nullptr, "a quality string needs the quality table");
        check(*qual, torch::kUInt8, "qual");
        TORCH_CHECK(qual->numel() == total,
                    "qual must hold one byte per polished base");
        ql = qual->data_ptr<uint8_t>();
    }
    TORCH_CHECK(reinterpret_cast<uintptr_t>(tab) % 16 == 0,
                "vote tables must be 16-byte aligned");
    const int64_t n_pos = draft.numel();
    rk::stitch_write(tab, qs, dr, n_pos, edit_state_ptr(state),
                     edit_counts_ptr(offsets, n_pos), (int)min_qual,
                     keep_uncovered, seq.data_ptr<uint8_t>(), ql, total,
                     cur_stream());
    check_launch("stitch kernel");
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

// ---------------------------------------------------------------------------
// Wavefront aligner (wfa.hip; contract and driver: roko_amd/wfa.py). `q` and
// `t` carry wfa_pad() pad bytes after their n and m sequence bytes, `offs` is
// the two offset rows (2, n + m + 3) int32, `done` one int32 (-1 until the
// end cell is reached, then the edit distance).
void wfa_check_seqs(const torch::Tensor& q, const torch::Tensor& t, int64_t n,
                    int64_t m) {
    check(q, torch::kUInt8, "q");
    check(t, torch::kUInt8, "t");
    TORCH_CHECK(n >= 0 && m >= 0 && n + m + 3 + rk::wfa_pad() < (int64_t(1) << 31),
                "sequence lengths out of range");
    TORCH_CHECK(q.numel() == n + rk::wfa_pad() && t.numel() == m + rk::wfa_pad(),
                "q and t must hold the sequence plus wfa_pad() bytes");
}

// scores [s0, s1) of one chunk, one launch each; `dir` is the chunk's
// direction table of exactly wfa_dir_cells(n, m, s0, s1) bytes
void wfa_steps(torch::Tensor q, torch::Tensor t, int64_t n, int64_t m,
               int64_t s0, int64_t s1, torch::Tensor offs, torch::Tensor dir,
               torch::Tensor done) {
    wfa_check_seqs(q, t, n, m);
    check(offs, torch::kInt32, "offs");
    check(dir, torch::kUInt8, "dir");
    check(done, torch::kInt32, "done");
    TORCH_CHECK(0 <= s0 && s0 < s1 && s1 <= std::max(n, m) + 1,
                "score range out of bounds");
    TORCH_CHECK(offs.numel() == 2 * (n + m + 3), "offs must be (2, n + m + 3)");
    TORCH_CHECK(dir.numel() == rk::wfa_dir_cells(n, m, s0, s1),
                "dir must hold wfa_dir_cells(n, m, s0, s1) bytes");
    TORCH_CHECK(done.numel() == 1, "done must hold one int32");
    const c10::cuda::CUDAGuard guard(q.device());
    rk::wfa_steps(q.data_ptr<uint8_t>(), t.data_ptr<uint8_t>(), (int)n, (int)m,
                  (int)s0, (int)s1, offs.data_ptr<int32_t>(),
                  dir.data_ptr<uint8_t>(), done.data_ptr<int32_t>(),
                  cur_stream());
    check_launch("wfa step kernel");
}

// one chunk of the traceback: scores s_hi down to max(s0, 1) of the table
// that starts at score s0; walk = {diagonal, error flag}
void wfa_trace(torch::Tensor dir, int64_t n, int64_t m, int64_t s0,
               int64_t s_hi, torch::Tensor walk, torch::Tensor ops) {
    check(dir, torch::kUInt8, "dir");
    check(walk, torch::kInt32, "walk");
    check(ops, torch::kUInt8, "ops");
    TORCH_CHECK(n >= 0 && m >= 0 && n + m + 3 < (int64_t(1) << 31),
                "sequence lengths out of range");
    TORCH_CHECK(0 <= s0 && s0 <= s_hi && 1 <= s_hi && s_hi <= ops.numel(),
                "score range out of bounds");
    TORCH_CHECK(dir.numel() >= rk::wfa_dir_cells(n, m, s0, s_hi + 1),
                "dir does not reach score s_hi");
    TORCH_CHECK(walk.numel() == 2, "walk must hold two int32");
    const c10::cuda::CUDAGuard guard(dir.device());
    rk::wfa_trace(dir.data_ptr<uint8_t>(), (int)n, (int)m, (int)s0, (int)s_hi,
                  walk.data_ptr<int32_t>(), ops.data_ptr<uint8_t>(),
                  cur_stream());
    check_launch("wfa trace kernel");
}

}  // namespace

void bind_data(py::module_& m) {
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
    m.def("stitch_count", &stitch_count, py::arg("table"), py::arg("qsum"),
          py::arg("draft"), py::arg("n_slots"), py::arg("state"),
          py::arg("counts"), py::arg("min_qual"), py::arg("keep_uncovered"));
    m.def("stitch_write", &stitch_write, py::arg("table"), py::arg("qsum"),
          py::arg("draft"), py::arg("n_slots"), py::arg("state"),
          py::arg("offsets"), py::arg("min_qual"), py::arg("keep_uncovered"),
          py::arg("seq"), py::arg("qual"), py::arg("total"));
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
    m.def("wfa_probe", &rk::wfa_probe);
    m.def("wfa_coop", &rk::wfa_coop);
    m.def("wfa_pad", &rk::wfa_pad);
    m.def("wfa_dir_cells", &rk::wfa_dir_cells, py::arg("n"), py::arg("m"),
          py::arg("s0"), py::arg("s1"));
    m.def("wfa_steps", &wfa_steps, py::arg("q"), py::arg("t"), py::arg("n"),
          py::arg("m"), py::arg("s0"), py::arg("s1"), py::arg("offs"),
          py::arg("dir"), py::arg("done"));
    m.def("wfa_trace", &wfa_trace, py::arg("dir"), py::arg("n"), py::arg("m"),
          py::arg("s0"), py::arg("s_hi"), py::arg("walk"), py::arg("ops"));
}
