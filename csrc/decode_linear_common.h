// Pieces shared by the weight-streaming decode linears (decode_linear.hip:
// bf16 weights, decode_linear_fp8.hip: fp8 codes plus a per-row scale,
// decode_linear_mxfp4.hip: MXFP4 codes plus a scale per 32 elements of K): the
// 16-byte load and the fragment cast, the tanh-GELU, the per-element
// epilogue, the launch arguments and every host-side check the two bindings
// have in common. A fix applied to one copy of these alone would give wrong
// numbers and no crash. It also holds the LayerNorm prologue of the two
// *_ln_kernel (statistics, variance rule, fragment normalisation), which is
// not tied to the weight type; see "LayerNorm prologue" below.
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
// is here meets it, and the kernels without LN are still ISA identical
// with the LN prologue next to them (profiles/decode_linear_ln.txt).
//
// Masked lanes. Rows of W at index >= N, rows of x at index >= M and k-steps
// past a wave's chunk are never loaded: every such load sits behind a
// predicate (exec-masked, as in decode_attention.hip) and its address keeps
// row 0 as a valid base. The fragments of masked lanes need no zero either:
// row n of C depends on row n of A alone and column m on column m of B
// alone, and neither rows >= N nor columns >= M reach finish_element. They
// start as zero and keep whatever they held. (decode_linear_mxfp4.hip sends
// its masked lanes to a valid row another lane reads instead of predicating
// them, for the sake of its counted waits; the reasoning above holds as is.)
//
// Everything sits in an unnamed namespace: each translation unit that
// includes this header keeps its own copies.
#pragma once

#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>
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

// ---- LayerNorm prologue (the *_ln_kernel of both files) ----
//
// y = act(LN(x) . W^T ...) with LN(x) = bf16((x - mu) * rstd * g + b): the
// statistics of the <= 16 rows are computed by every workgroup (x is in L2,
// and there is no way to hand them over without a flag or a second launch),
// then every x fragment is normalised in registers on its way into the MFMA.
// Same roundings as layernorm + decode_linear: h to bf16 once, y once.
//
// Not tied to the weight type: a k-step is XL 16-byte loads of x per lane
// (1 with bf16 weights, 2 with fp8 codes), the l-th at xp + step*KSTEP + 8*l.

// largest K of the LN kernels: g and b sit in LDS (4*K bytes) next to the
// partial tiles, at most 32 KiB + 1.5 KiB of statistics; 64 KiB in all
constexpr int LN_MAX_K = 7168;
// 16-byte loads in flight per lane in the statistics passes (LN_LOADS / XL
// k-steps): a wave's whole chunk at K = 2048, so a pass is one trip to L2
constexpr int LN_LOADS = 16;

// On the LN kernels: their fp32 arithmetic on pairs of bf16 (statistics,
// normalisation) is compiled to scalar-per-lane VALU ops, never to the
// packed v_pk_*_f32 forms. The kernels without LN hold no such arithmetic.
#define NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))

DEV_INLINE float bf_lo(unsigned int w) { return __uint_as_float(w << 16); }
DEV_INLINE float bf_hi(unsigned int w) {
  return __uint_as_float(w & 0xffff0000u);
}

// sum over the wave's four lane groups: lanes r, r+16, r+32, r+48 hold the
// k slices of one row. Every one of them ends with the same bits.
DEV_INLINE float ln_group_sum(float v) {
  v += __shfl_xor(v, 16, WAVE);
  v += __shfl_xor(v, 32, WAVE);
  return v;
}

// One pass over the wave's k-steps [s_beg, s_end) with the addressing and
// the predicate of its B fragments. DEV false: s += x, q += x*x; DEV true:
// q += (x - mu)^2. Masked lanes load nothing and keep zeros. between() runs
// once, in every lane, after the first batch of loads is issued and before
// it is waited for.
template <typename V, int KSTEP, int XL, bool DEV, typename F>
DEV_INLINE void ln_pass(const short* xp, bool x_ok, int s_beg, int s_end,
                        float mu, float& s, float& q, F between) {
  constexpr int LN_SU = LN_LOADS / XL;
  for (int st = s_beg; st < s_end; st += LN_SU) {
    const int nb = s_end - st;  // wave-uniform
    union { V v; unsigned int w[4]; } f[LN_SU][XL];
    if (x_ok) {
#pragma unroll
      for (int u = 0; u < LN_SU; ++u) {
        if (u < nb) {
#pragma unroll
          for (int l = 0; l < XL; ++l)
            f[u][l].v =
                load16<V, false>(xp + (size_t)(st + u) * KSTEP + 8 * l);
        }
      }
    }
    if (st == s_beg) between();
    if (x_ok) {
#pragma unroll
      for (int u = 0; u < LN_SU; ++u) {
        if (u < nb) {
#pragma unroll
          for (int l = 0; l < XL; ++l) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float lo = bf_lo(f[u][l].w[i]), hi = bf_hi(f[u][l].w[i]);
              if constexpr (DEV) {
                q += (lo - mu) * (lo - mu);
                q += (hi - mu) * (hi - mu);
              } else {
                s += lo;
                q += lo * lo;
                s += hi;
                q += hi * hi;
              }
            }
          }
        }
      }
    }
  }
}

// mu and rstd of the lane's row (lane & 15) from the whole workgroup, and g
// and b staged into s_gb ([0, K): g, [K, 2K): b) under the same barrier.
// Each wave sums the chunk it is about to stream, writes one (sum, sumsq)
// per row, and after the barrier every lane adds the NW partials of its row
// in wave order; a wave with an empty chunk contributes zeros. The variance
// rule is layernorm.hip's: E[x^2] - mu^2 where that is >= E[x^2] / 4, else
// a second pass over (x - mu)^2. All waves read the same partials, so the
// ballot is the same in every wave and the second barrier is reached by all
// or none; a row that passes the test keeps its one-pass variance whatever
// the other rows do.
// first_w() issues the wave's first batch of weight loads. It runs behind
// the x loads of the statistics pass and ahead of their wait: loads return
// in issue order, so the statistics are computed, exchanged and turned into
// mu and rstd while the weights are on their way from HBM.
template <typename V, int NW, int KSTEP, int XL, typename F>
DEV_INLINE void ln_prologue(const short* xp, bool x_ok, int s_beg, int s_end,
                            int K, const short* ln_w, const short* ln_b,
                            float eps, short* s_gb, float (*s_stat)[2 * TILE],
                            float (*s_dev)[TILE], int tid, int wid, int r,
                            float& mu, float& rstd, F first_w) {
  float s = 0.f, q = 0.f;
  ln_pass<V, KSTEP, XL, false>(xp, x_ok, s_beg, s_end, 0.f, s, q, first_w);
  s = ln_group_sum(s);
  q = ln_group_sum(q);
  if ((tid & (WAVE - 1)) < TILE) {
    s_stat[wid][2 * r] = s;
    s_stat[wid][2 * r + 1] = q;
  }
  for (int i = tid * 8; i < K; i += NW * WAVE * 8) {  // K % 8 == 0
    *reinterpret_cast<V*>(s_gb + i) = load16<V, false>(ln_w + i);
    *reinterpret_cast<V*>(s_gb + K + i) = load16<V, false>(ln_b + i);
  }
  __syncthreads();
  s = 0.f;
  q = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    s += s_stat[i][2 * r];
    q += s_stat[i][2 * r + 1];
  }
  mu = s / K;
  const float ex2 = q / K;
  float var = ex2 - mu * mu;
  const bool redo = x_ok && !(var >= 0.25f * ex2);
  if (__builtin_amdgcn_ballot_w64(redo) != 0) {  // workgroup-uniform
    float d = 0.f, unused = 0.f;
    ln_pass<V, KSTEP, XL, true>(xp, x_ok, s_beg, s_end, mu, unused, d,
                                [] {});
    d = ln_group_sum(d);
    if ((tid & (WAVE - 1)) < TILE) s_dev[wid][r] = d;
    __syncthreads();
    d = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) d += s_dev[i][r];
    if (redo) var = d / K;
  }
  rstd = rsqrtf(var + eps);
}

// The B fragment of one 16-byte load of x at k: 8 values normalised in fp32
// in layernorm.hip's expression order and rounded to bf16 (RNE).
template <typename V>
DEV_INLINE mfma_bf16x8 ln_frag(const V& xv, const short* s_gb, int K,
                               size_t k, float mu, float rstd) {
  union { V v; unsigned int w[4]; } x, g, b, o;
  x.v = xv;
  g.v = *reinterpret_cast<const V*>(s_gb + k);
  b.v = *reinterpret_cast<const V*>(s_gb + K + k);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o.w[i] = cvt_pk_bf16(
        (bf_lo(x.w[i]) - mu) * rstd * bf_lo(g.w[i]) + bf_lo(b.w[i]),
        (bf_hi(x.w[i]) - mu) * rstd * bf_hi(g.w[i]) + bf_hi(b.w[i]));
  return as_frag(o.v);
}

// ---- host side ----

// What a launch takes; w_scale stays null for bf16 weights, ln_w and ln_b
// without a LayerNorm prologue.
template <typename WT>
struct Args {
  const short* x;
  const WT* w;
  const float* w_scale;
  const short *bias, *res;
  short* y;
  int M, N, K, rows, gelu;
  const short *ln_w, *ln_b;
  float ln_eps;
};

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

struct Checked {
  long M, N, K;
  const short *bias, *res;    // null when absent
  const short *ln_w, *ln_b;   // both null, or the LayerNorm prologue's
};

// Everything that stands between raw pointers and a launch and is the same
// for both bindings. op and wname are the binding's and its weight
// argument's names, wdtype / kstep / rows_ok what its kernel takes, pack the
// stored elements per entry of w (2 for 4-bit codes: w is [N, K / 2]),
// [m_lo, m_hi] the batch rows it serves (decode_linear_wide.hip: 17 to 64).
Checked check_decode_linear(const char* op, const char* wname,
                            const torch::Tensor& x, const torch::Tensor& w,
                            torch::ScalarType wdtype, int kstep,
                            const c10::optional<torch::Tensor>& bias,
                            const c10::optional<torch::Tensor>& residual,
                            const std::string& act, long rows,
                            std::initializer_list<long> rows_ok, long waves,
                            long nontemporal,
                            const c10::optional<torch::Tensor>& ln_weight,
                            const c10::optional<torch::Tensor>& ln_bias,
                            double ln_eps, int pack = 1, long m_lo = 1,
                            long m_hi = TILE) {
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
  TORCH_CHECK(w.size(1) * pack == K, op, ": ", wname, " must be [N, ",
              K / pack, "], got [", N, ", ", w.size(1), "]");
  TORCH_CHECK(M >= m_lo && M <= m_hi, op, ": M must be in [", m_lo, ", ", m_hi,
              "], got ", M);
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
  Checked c{M, N, K, nullptr, nullptr, nullptr, nullptr};
  const bool has_g = ln_weight.has_value() && ln_weight->defined();
  const bool has_b = ln_bias.has_value() && ln_bias->defined();
  TORCH_CHECK(has_g == has_b, op,
              ": ln_weight and ln_bias go together (LayerNorm without a bias "
              "is not built)");
  if (has_g) {
    for (const torch::Tensor* t : {&*ln_weight, &*ln_bias}) {
      TORCH_CHECK(t->scalar_type() == torch::kBFloat16 &&
                      t->device() == x.device() && t->is_contiguous() &&
                      t->dim() == 1 && t->size(0) == K,
                  op, ": ln_weight and ln_bias must be contiguous bfloat16 [",
                  K, "] on ", x.device());
      TORCH_CHECK(aligned16(*t), op,
                  ": ln_weight and ln_bias must be 16-byte aligned");
    }
    TORCH_CHECK(std::isfinite(ln_eps) && ln_eps > 0, op,
                ": ln_eps must be finite and positive, got ", ln_eps);
    TORCH_CHECK(K <= LN_MAX_K, op, ": K must be <= ", LN_MAX_K,
                " with a LayerNorm prologue, got ", K);
    c.ln_w = (const short*)ln_weight->data_ptr();
    c.ln_b = (const short*)ln_bias->data_ptr();
  }
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
