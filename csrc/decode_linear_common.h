// Pieces shared by the weight-streaming decode linears (decode_linear.hip:
// bf16 weights, decode_linear_fp8.hip: fp8 codes plus a per-row scale): the
// 16-byte load and the fragment cast, the tanh-GELU, the per-element
// epilogue, the launch arguments and every host-side check the two bindings
// have in common. A fix applied to one copy of these alone would give wrong
// numbers and no crash.
//
// The main loops are NOT here. They are the measured part and they differ on
// purpose: the bf16 kernel has a specialised path for full batches of
// k-steps, the fp8 kernel one path with a measured load order (the two-path
// form spilled). Each loop stays in its file next to the comments that say
// why it looks the way it does; so do the two geometry rules and the
// launches, which name different kernels with different tile counts.
//
// The per-lane setup (predicates, pointers, chunk bounds) and the LDS
// reduction in wave order are NOT here either, although both files hold the
// same text. As inline functions they are simplified on their own before
// they are inlined and reach the kernel in another canonical form (k offset,
// address arithmetic), which changed the schedule and register allocation
// of every instance. The condition for this header is gfx950 ISA identical
// to the unshared kernels (profiles/decode_linear_shared_header.txt); what
// is here meets it.
//
// Masked lanes. Rows of W at index >= N, rows of x at index >= M and k-steps
// past a wave's chunk are never loaded: every such load sits behind a
// predicate (exec-masked, as in decode_attention.hip) and its address keeps
// row 0 as a valid base. The fragments of masked lanes need no zero either:
// row n of C depends on row n of A alone and column m on column m of B
// alone, and neither rows >= N nor columns >= M reach finish_element. They
// start as zero and keep whatever they held.
//
// Everything sits in an unnamed namespace: each translation unit that
// includes this header keeps its own copies.
#pragma once

#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>
#include <initializer_list>
#include <string>

namespace {

constexpr int TILE = 16;     // MFMA rows (n) and columns (m)
constexpr float GELU_K = 0.7978845608028654f;  // sqrt(2/pi)

// the tanh-GELU of elementwise.hip (bias_gelu), written with __expf
DEV_INLINE float gelu_tanh(float x) {
  const float t =
      1.f - 2.f / (__expf(2.f * GELU_K * (x + 0.044715f * x * x * x)) + 1.f);
  return 0.5f * x * (1.f + t);
}

// V: the 16-byte vector the caller keeps its fragments in
template <typename V, bool NT>
DEV_INLINE V load16(const void* p) {
  static_assert(sizeof(V) == 16, "load16 is one 16-byte load");
  if constexpr (NT)
    return __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
  else
    return *reinterpret_cast<const V*>(p);
}

template <typename V>
DEV_INLINE mfma_bf16x8 as_frag(const V& v) {
  union { V v; mfma_bf16x8 f; } u;
  u.v = v;
  return u.f;
}

// What becomes of one summed element (m, n): scale (SCALED only: the fp8
// kernel's per-row scale, before anything else), bias, tanh-GELU, residual
// and the one rounding to bf16.
template <bool SCALED>
DEV_INLINE void finish_element(float v, int m, int n, int N,
                               const float* w_scale, const short* bias,
                               const short* res, short* y, int gelu) {
  if constexpr (SCALED) v *= w_scale[n];
  if (bias) v += bf_raw2f((unsigned short)bias[n]);
  if (gelu) v = gelu_tanh(v);
  const size_t o = (size_t)m * N + n;
  if (res) v += bf_raw2f((unsigned short)res[o]);
  y[o] = (short)f2bf_raw(v);
}

// ---- host side ----

// What a launch takes; w_scale stays null for bf16 weights.
template <typename WT>
struct Args {
  const short* x;
  const WT* w;
  const float* w_scale;
  const short *bias, *res;
  short* y;
  int M, N, K, rows, gelu;
};

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

struct Checked {
  long M, N, K;
  const short *bias, *res;  // null when absent
};

// Everything that stands between raw pointers and a launch and is the same
// for both bindings. op and wname are the binding's and its weight
// argument's names, wdtype / kstep / rows_ok what its kernel takes.
Checked check_decode_linear(const char* op, const char* wname,
                            const torch::Tensor& x, const torch::Tensor& w,
                            torch::ScalarType wdtype, int kstep,
                            const c10::optional<torch::Tensor>& bias,
                            const c10::optional<torch::Tensor>& residual,
                            const std::string& act, long rows,
                            std::initializer_list<long> rows_ok, long waves,
                            long nontemporal) {
  TORCH_CHECK(x.defined() && w.defined(), op, ": x and ", wname,
              " must be defined");
  TORCH_CHECK(x.is_cuda() && w.is_cuda(), op, ": x and ", wname,
              " must be GPU tensors");
  TORCH_CHECK(w.device() == x.device(), op, ": ", wname, " is on ", w.device(),
              ", expected ", x.device());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, op,
              ": x must be BFloat16, got ", x.scalar_type());
  TORCH_CHECK(w.scalar_type() == wdtype, op, ": ", wname, " must be ", wdtype,
              ", got ", w.scalar_type());
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2, op, ": x must be [M, K] and ",
              wname, " [N, K]");
  TORCH_CHECK(x.is_contiguous(), op, ": x must be contiguous");
  TORCH_CHECK(w.is_contiguous(), op, ": ", wname, " must be contiguous");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, op, ": ", wname, " must be [N, ", K, "], got [",
              N, ", ", w.size(1), "]");
  TORCH_CHECK(M >= 1 && M <= TILE, op, ": M must be in [1, 16], got ", M);
  TORCH_CHECK(K >= kstep && K % kstep == 0, op,
              ": K must be a positive multiple of ", kstep, ", got ", K);
  TORCH_CHECK(N >= 8 && N % 8 == 0, op,
              ": N must be a positive multiple of 8, got ", N);
  TORCH_CHECK(N * K < (1L << 40) && N < (1L << 30) && K < (1L << 30), op,
              ": bad weight extent");
  TORCH_CHECK(aligned16(x) && aligned16(w), op, ": x and ", wname,
              " must be 16-byte aligned");
  TORCH_CHECK(act == "none" || act == "gelu", op,
              ": act must be 'none' or 'gelu', got '", act, "'");
  Checked c{M, N, K, nullptr, nullptr};
  if (bias.has_value() && bias->defined()) {
    const torch::Tensor& b = *bias;
    TORCH_CHECK(b.scalar_type() == torch::kBFloat16 &&
                    b.device() == x.device() && b.is_contiguous() &&
                    b.dim() == 1 && b.size(0) == N,
                op, ": bias must be a contiguous bfloat16 [", N, "] on ",
                x.device());
    c.bias = (const short*)b.data_ptr();
  }
  if (residual.has_value() && residual->defined()) {
    const torch::Tensor& rs = *residual;
    TORCH_CHECK(rs.scalar_type() == torch::kBFloat16 &&
                    rs.device() == x.device() && rs.is_contiguous() &&
                    rs.dim() == 2 && rs.size(0) == M && rs.size(1) == N,
                op, ": residual must be a contiguous bfloat16 [", M, ", ", N,
                "] on ", x.device());
    c.res = (const short*)rs.data_ptr();
  }
  bool rows_known = rows == 0;
  std::string set;  // "8, 16 or 32"
  for (const long* p = rows_ok.begin(); p != rows_ok.end(); ++p) {
    rows_known |= rows == *p;
    set += (p == rows_ok.begin() ? "" : p + 1 == rows_ok.end() ? " or " : ", ");
    set += std::to_string(*p);
  }
  TORCH_CHECK(rows_known, op, ": rows must be 0 (auto), ", set);
  TORCH_CHECK(waves == 0 || waves == 4 || waves == 8, op,
              ": waves must be 0 (auto), 4 or 8");
  TORCH_CHECK(nontemporal >= -1 && nontemporal <= 1, op,
              ": nontemporal must be -1 (auto), 0 or 1");
  return c;
}

}  // namespace
