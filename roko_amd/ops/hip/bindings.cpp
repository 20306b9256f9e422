// Torch bindings for the gfx950 kernels (roko_amd.ops._hip_ops): the module,
// filled by one bind_* per translation unit (bind_model.cpp, bind_train.cpp,
// bind_data.cpp, serve_slot.cpp). The kernels' host entry points are declared
// in api.h.

#include <ATen/cuda/CUDAContext.h>

#include "bind_util.h"

hipStream_t cur_stream() {
    return at::cuda::getCurrentCUDAStream().stream();
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "roko-mi355x CDNA4 kernels (gfx950)";
    bind_model(m);
    bind_train(m);
    bind_data(m);
    bind_serve(m);
}
