// Helpers shared by the binding translation units of roko_amd.ops._hip_ops.
// Nothing here names a torch stream type: the build's source translation
// leaves this header as it is.

#pragma once

#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <cstdint>

// one per translation unit; bindings.cpp calls them from PYBIND11_MODULE
void bind_model(py::module_& m);
void bind_train(py::module_& m);
void bind_data(py::module_& m);
void bind_serve(py::module_& m);

// torch's current stream on the current device (bindings.cpp)
hipStream_t cur_stream();

inline void check(const torch::Tensor& t, torch::ScalarType dt,
                  const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t.scalar_type() == dt, name, " has wrong dtype");
}

inline void check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    TORCH_CHECK(e == hipSuccess, what, " launch: ", hipGetErrorString(e));
}

// The arguments every front kernel takes: ids (B, 200, 90) u8, bf16 W1 (as
// `w1_name`: the plain or the zero-padded image), W2 and embedding, fp32
// biases. Returns B; the weight shapes are the caller's to check.
inline int check_front(const torch::Tensor& ids, const torch::Tensor& w1,
                       const char* w1_name, const torch::Tensor& b1,
                       const torch::Tensor& w2, const torch::Tensor& b2,
                       const torch::Tensor& emb) {
    check(ids, torch::kUInt8, "ids");
    check(w1, torch::kBFloat16, w1_name);
    check(b1, torch::kFloat32, "b1");
    check(w2, torch::kBFloat16, "w2");
    check(b2, torch::kFloat32, "b2");
    check(emb, torch::kBFloat16, "emb");
    TORCH_CHECK(ids.dim() == 3 && ids.size(1) == 200 && ids.size(2) == 90,
                "ids must be (B,200,90)");
    return (int)ids.size(0);
}

// Device votes (votes.hip). The packed table and the error flag are int32
// tensors on the Python side (torch has no first-class uint32); the kernels
// treat the same bits as uint32.
inline uint32_t* vote_table_ptr(const torch::Tensor& table, int64_t n_slots) {
    check(table, torch::kInt32, "table");
    TORCH_CHECK(n_slots >= 0 && n_slots <= table.numel(),
                "n_slots exceeds the vote table");
    return reinterpret_cast<uint32_t*>(table.data_ptr<int32_t>());
}

inline uint32_t* vote_err_ptr(const torch::Tensor& err_flag) {
    check(err_flag, torch::kInt32, "err_flag");
    TORCH_CHECK(err_flag.numel() == 1, "err_flag must hold one int32");
    return reinterpret_cast<uint32_t*>(err_flag.data_ptr<int32_t>());
}

// the quality table beside a count table: int64 on the Python side, one
// word per slot; the consensus kernel reads it in 16-byte pairs
inline uint64_t* vote_qsum_ptr(const torch::Tensor& qsum, int64_t n_slots) {
    check(qsum, torch::kInt64, "qsum");
    TORCH_CHECK(n_slots <= qsum.numel(), "n_slots exceeds the qsum table");
    return reinterpret_cast<uint64_t*>(qsum.data_ptr<int64_t>());
}
