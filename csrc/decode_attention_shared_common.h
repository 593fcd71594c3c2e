// Pieces shared by the two shared-prompt decode-attention ops
// (decode_attention_shared.hip: bf16 prefix, decode_attention_shared_fp8.hip:
// e4m3 codes plus one fp32 scale per stored row). The fp8 prefix pass was
// written as the bf16 one with another way of moving the data; what the two
// have in common sits here once, so that a fix to the chunk bounds or to the
// merge of the waves cannot be made in one file alone.
//
// Device side: the geometry of a prefix workgroup (PNW, PSTEP, COLS), frag,
// the permuted contraction order of the second product (perm_pos), the chunk
// bounds, the wave's state store and the in-order merge of the four waves
// with its workspace store.
// Host side: every refusal the two bindings have in common
// (check_decode_attn_shared), the automatic chunk count (shared_chunks), the
// three-launch scaffold (launch_shared: workspace, chunk, the suffix and
// merge launches around a prefix launch the caller supplies) and aligned16.
//
// NOT here, on purpose: load_step, the V image build, the two MFMA loops,
// decode8 / transpose4x4, the scale strip, the LDS layouts with their bank
// comments and the kernel signatures. That is where the two passes differ,
// and each stays in its file next to the comments that say why it looks the
// way it does. There is no prefix kernel templated over a storage policy: it
// would be longer and harder to read than the two loops it replaces. The
// rest of the per-workgroup prologue (indices, the Q fragments, the
// accumulator initialisation) stays too: it is tied to each file's fragment
// shapes.
//
// The online-softmax step is NOT here either, although both files hold the
// same text but for the factor on the score (scale, or scale * k_scale) and
// on the probability (none, or v_scale). As an inline function over a
// SCALED flag it cost registers in three of the four prefix instances (104
// -> 107 and 164 -> 166 VGPRs with a bf16 prefix, 138 -> 139 with fp8 at
// D = 128), and unchanged resources were the condition for a move that
// changes the ISA. A fix to it has to be made in both files. Which moves
// kept the gfx950 ISA, which changed it and what was measured for those:
// profiles/decode_attention_shared_header.txt.
//
// Everything sits in an unnamed namespace, as in decode_common.h: each
// translation unit that includes this header keeps its own copies.
#pragma once

#include "decode_attention_kernel.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>
#include <initializer_list>

namespace {

constexpr int PNW = 4;     // waves per prefix workgroup
constexpr int PSTEP = 32;  // positions per wave step (two score tiles)
constexpr int COLS = 16;   // samples per column group (MFMA N)

DEV_INLINE mfma_bf16x8 frag(const short8v& v) {
  return __builtin_bit_cast(mfma_bf16x8, v);
}

// position (inside a 32-position step) of column c of the permuted order:
// slot j of lane group g (c = g*8 + j) is position g*4 + j of the first
// score tile for j < 4 and 16 + g*4 + (j - 4) of the second for j >= 4
DEV_INLINE int perm_pos(int c) {
  const int gg = c >> 3, jj = c & 7;
  return (jj < 4) ? gg * 4 + jj : 16 + gg * 4 + (jj - 4);
}

// positions [start, end) of chunk ck of nck of a prefix of len positions
DEV_INLINE void chunk_bounds(int len, int Lcap, int chunk, int ck, int nck,
                             int& start, int& end) {
  // a bad length gives wrong numbers, never an out-of-bounds address
  const int Lp = min(max(len, 0), Lcap);
  // the last chunk runs to Lp so an under-estimated max_prefix_len cannot
  // drop positions
  start = min(ck * chunk, Lp);
  end = (ck == nck - 1) ? Lp : min((ck + 1) * chunk, Lp);
}

// After the walk: this wave's state -> its own LDS region as
// [sample][acc[D], m, l, pad]. The region held the wave's V image; LDS
// serves one wave's instructions in order, so its reads are done.
template <int D>
DEV_INLINE void store_wave_state(float* region, int r, int g,
                                 const mfma_f32x4* acc, float m, float l) {
  l += __shfl_xor(l, 16, WAVE);
  l += __shfl_xor(l, 32, WAVE);
  __builtin_amdgcn_wave_barrier();
  float* sw = region + r * (D + 4);
#pragma unroll
  for (int db = 0; db < D / 16; ++db)
    *reinterpret_cast<mfma_f32x4*>(sw + db * 16 + g * 4) = acc[db];
  if (g == 0) { sw[D] = m; sw[D + 1] = l; }
}

// Behind the workgroup barrier: thread (sample c, channels d0 .. d0 + D/16)
// merges the waves' states in wave order and writes chunk ck's slot 1 + ck
// of ws (fp32 [B*h, ws_slots, D+4]) with 16-byte stores. region0 is wave 0's
// region, WSTRIDE the floats between two waves' regions.
template <int D, int WSTRIDE>
DEV_INLINE void merge_waves(const float* region0, float* ws, int tid, int cg,
                            int p, int head, int ck, int h, int G,
                            int ws_slots) {
  constexpr int ND = D / 16;
  const int c = tid & 15;
  const int d0 = (tid >> 4) * ND;
  const float* s0 = region0 + c * (D + 4);
  float M = -INFINITY;
#pragma unroll
  for (int w = 0; w < PNW; ++w) M = fmaxf(M, s0[w * WSTRIDE + D]);
  const float Ms = (M == -INFINITY) ? 0.f : M;
  float Lsum = 0.f;
  float o[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) o[i] = 0.f;
#pragma unroll
  for (int w = 0; w < PNW; ++w) {
    const float* sw = s0 + w * WSTRIDE;
    const float m_w = sw[D];
    const float wt = (m_w == -INFINITY) ? 0.f : __expf(m_w - Ms);
    Lsum = fmaf(wt, sw[D + 1], Lsum);
#pragma unroll
    for (int i = 0; i < ND; i += 4) {
      const float4v a = *reinterpret_cast<const float4v*>(sw + d0 + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[i + e] = fmaf(wt, a[e], o[i + e]);
    }
  }
  const int sc = cg * COLS + c;
  if (sc < G) {
    float* w = ws + (((size_t)(p * G + sc) * h + head) * ws_slots + 1 + ck) *
                        (D + 4);
#pragma unroll
    for (int i = 0; i < ND; i += 4) {
      const float4v a = {o[i], o[i + 1], o[i + 2], o[i + 3]};
      *reinterpret_cast<float4v*>(w + d0 + i) = a;
    }
    if (d0 == 0) { w[D] = M; w[D + 1] = Lsum; }
  }
}

// ---- host side ----

bool aligned16(const torch::Tensor& t) {
  return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
}

struct SharedDims {
  long B, h, D, P, Lcap, Scap;
};

// Every refusal the two bindings have in common, under the op's name.
// prefix_dtype is what k_prefix and v_prefix hold; extra lists the tensors a
// binding takes beyond these seven (they must be on the GPU, on qkv's device
// and contiguous like the rest; their dtype and shape are the binding's).
SharedDims check_decode_attn_shared(
    const char* op, const torch::Tensor& qkv, const torch::Tensor& k_prefix,
    const torch::Tensor& v_prefix, const torch::Tensor& prefix_lens,
    const torch::Tensor& k_cache, const torch::Tensor& v_cache,
    const torch::Tensor& seq_lens, long group, long max_prefix_len,
    long num_splits, torch::ScalarType prefix_dtype,
    std::initializer_list<const torch::Tensor*> extra = {}) {
  auto placed = [&](const torch::Tensor& t) {
    TORCH_CHECK(t.is_cuda(), op, ": all tensors must be on the GPU");
    TORCH_CHECK(t.device() == qkv.device(), op,
                ": tensors must share one device");
    TORCH_CHECK(t.is_contiguous(), op, ": tensors must be contiguous");
  };
  for (const torch::Tensor* t : {&qkv, &k_prefix, &v_prefix, &prefix_lens,
                                 &k_cache, &v_cache, &seq_lens})
    placed(*t);
  for (const torch::Tensor* t : extra) placed(*t);
  if (prefix_dtype == torch::kBFloat16) {
    TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 &&
                    k_prefix.scalar_type() == torch::kBFloat16 &&
                    v_prefix.scalar_type() == torch::kBFloat16 &&
                    k_cache.scalar_type() == torch::kBFloat16 &&
                    v_cache.scalar_type() == torch::kBFloat16,
                op, ": qkv, prefix and caches must be bf16");
  } else {  // the binding says what qkv and the caches must be
    TORCH_CHECK(k_prefix.scalar_type() == prefix_dtype &&
                    v_prefix.scalar_type() == prefix_dtype,
                op, ": k_prefix and v_prefix must be float8_e4m3fn");
  }
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(1) == 1 && qkv.size(3) == 3, op,
              ": qkv must be [B, 1, h, 3, D]");
  const long B = qkv.size(0), h = qkv.size(2), D = qkv.size(4);
  TORCH_CHECK(D == 64 || D == 128, op, ": head_dim must be 64 or 128");
  TORCH_CHECK(group >= 1 && B >= 1 && B % group == 0, op,
              ": group must be >= 1 and divide B");
  TORCH_CHECK(k_prefix.dim() == 4 && k_prefix.size(1) == h &&
                  k_prefix.size(3) == D,
              op, ": k_prefix must be [P, h, Lcap, D]");
  TORCH_CHECK(v_prefix.sizes() == k_prefix.sizes(), op,
              ": v_prefix shape must equal k_prefix shape");
  const long P = k_prefix.size(0), Lcap = k_prefix.size(2);
  TORCH_CHECK(P * group == B, op,
              ": P * group must equal B (rows are grouped by prompt)");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(0) == B &&
                  k_cache.size(1) == h && k_cache.size(3) == D,
              op, ": k_cache must be [B, h, Scap, D]");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(), op,
              ": v_cache shape must equal k_cache shape");
  const long Scap = k_cache.size(2);
  TORCH_CHECK(Scap >= 1 && Lcap >= 1 && h >= 1 &&
                  B * h * Scap * D < (1L << 40) &&
                  P * h * Lcap * D < (1L << 40) && B * h < (1L << 30),
              op, ": bad cache extent");
  TORCH_CHECK(seq_lens.scalar_type() == torch::kInt && seq_lens.dim() == 1 &&
                  seq_lens.size(0) == B,
              op, ": seq_lens must be int32 [B]");
  TORCH_CHECK(prefix_lens.scalar_type() == torch::kInt &&
                  prefix_lens.dim() == 1 && prefix_lens.size(0) == P,
              op, ": prefix_lens must be int32 [P]");
  TORCH_CHECK(max_prefix_len >= 1 && max_prefix_len <= Lcap, op,
              ": max_prefix_len must be in [1, Lcap]");
  TORCH_CHECK(num_splits >= 0 && num_splits <= MAX_SPLITS - 1, op,
              ": num_splits must be 0 (auto) or 1..31 prefix chunks");
  return {B, h, D, P, Lcap, Scap};
}

// prefix chunks: num_splits, or with 0 the split rule over the prefix
// workgroups, capped at what the workspace of the merge holds beside slot 0
int shared_chunks(long P, long h, long group, long max_prefix_len,
                  long num_splits) {
  if (num_splits != 0) return (int)num_splits;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const long wgs = P * h * ((group + COLS - 1) / COLS);
  return std::min(choose_splits(wgs, max_prefix_len, cus), MAX_SPLITS - 1);
}

// The three launches over one workspace [B*h, 1 + chunks, D+4]: the caller's
// prefix pass, prefix_launch(grid, stream, wsp, ncg, chunk, slots), which
// fills slots 1.., then the suffix (slot 0, and the append) and the merge.
template <int D, typename F>
torch::Tensor launch_shared(const torch::Tensor& qkv,
                            const torch::Tensor& prefix_lens,
                            torch::Tensor& k_cache, torch::Tensor& v_cache,
                            const torch::Tensor& seq_lens,
                            const SharedDims& s, long group,
                            long max_prefix_len, long num_splits, float scale,
                            F prefix_launch) {
  auto stream = at::hip::getCurrentHIPStream();
  const int chunks = shared_chunks(s.P, s.h, group, max_prefix_len, num_splits);
  const int slots = chunks + 1;
  const int ncg = (int)((group + COLS - 1) / COLS);
  auto out = torch::empty({s.B, 1, s.h * D}, qkv.options());
  auto ws = torch::empty({s.B * s.h, (long)slots, (long)D + 4},
                         qkv.options().dtype(torch::kFloat));
  float* wsp = ws.data_ptr<float>();
  const int chunk = (int)((max_prefix_len + chunks - 1) / chunks);
  prefix_launch(dim3(s.P * s.h * ncg, chunks), stream, wsp, ncg, chunk, slots);
  hipLaunchKernelGGL((decode_attn_kernel<D, true>), dim3(s.B * s.h, 1),
                     dim3(BLOCK), 0, stream, (const short*)qkv.data_ptr(),
                     (short*)k_cache.data_ptr(), (short*)v_cache.data_ptr(),
                     seq_lens.data_ptr<int>(), (short*)out.data_ptr(), wsp,
                     (int)s.h, (int)s.Scap, (int)s.Scap, scale,
                     (const int*)prefix_lens.data_ptr<int>(), (int)group,
                     (int)s.Lcap, slots);
  hipLaunchKernelGGL(decode_merge_kernel<D>, dim3(s.B * s.h), dim3(D), 0,
                     stream, (const float*)wsp, (short*)out.data_ptr(), slots);
  return out;
}

}  // namespace
