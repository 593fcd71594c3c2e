// Host-side argument checks shared by the torch bindings. The kernels
// reinterpret raw pointers, so anything they cannot handle (a dtype other
// than bf16/fp32, a mismatched operand dtype, a strided or off-device
// tensor, a wrong length) must be refused here, before any launch.
#pragma once

#include <torch/extension.h>

namespace fleetx {

// the dispatching tensor: on the GPU, contiguous, bf16 or fp32
inline void check_data(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.defined(), name, " is undefined");
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16 ||
                  t.scalar_type() == torch::kFloat,
              name, " must be bfloat16 or float32, got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// a tensor with a fixed dtype (statistics, labels, ...) next to `ref`
inline void check_aux(const torch::Tensor& t, torch::ScalarType st,
                      const torch::Tensor& ref, const char* name) {
  TORCH_CHECK(t.defined(), name, " is undefined");
  TORCH_CHECK(t.scalar_type() == st, name, " must be ", st, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.device() == ref.device(), name, " is on ", t.device(),
              ", expected ", ref.device());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// a tensor the kernel reads with the element type of `ref`
inline void check_same(const torch::Tensor& t, const torch::Tensor& ref,
                       const char* name) {
  check_aux(t, ref.scalar_type(), ref, name);
}

inline void check_numel(const torch::Tensor& t, long n, const char* name) {
  TORCH_CHECK(t.numel() == n, name, " must have ", n, " elements, got ",
              t.numel());
}

}  // namespace fleetx
