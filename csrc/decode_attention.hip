// Single-token (decode) attention over a preallocated KV cache, gfx950.
//
// One query row per head: a memory-bound KV read (2*(L+1)*D*2 bytes per
// head, ~2 flop/byte), so no MFMA and no LDS staging. K/V rows go straight
// to VGPRs with 16-byte loads; a group of D/8 lanes owns one KV row per
// step and reduces the dot product with shuffles inside the group.
//
// The new token's K/V come from the fused-QKV linear output (viewed
// [B,1,h,3,D] like attn_fwd_packed), are appended to the cache in place at
// position seq_lens[b], and enter the softmax from registers (never read
// back from the cache, so there is no intra-launch ordering question).
//
// Split-KV: grid (B*h, splits). With splits > 1 every split writes fp32
// (acc[D], m, l) to a workspace and a second small launch merges them.
// No in-launch counters or flags.
#include "decode_attention_kernel.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

template <int D>
void launch(torch::Tensor& qkv, torch::Tensor& kc, torch::Tensor& vc,
            torch::Tensor& lens, torch::Tensor& out, long B, long h,
            long Smax, long max_seq_len, int splits, float scale) {
  auto stream = at::hip::getCurrentHIPStream();
  torch::Tensor ws;
  float* wsp = nullptr;
  if (splits > 1) {
    ws = torch::empty({B * h, (long)splits, (long)D + 4},
                      qkv.options().dtype(torch::kFloat));
    wsp = ws.data_ptr<float>();
  }
  const int chunk = (int)((max_seq_len + splits - 1) / splits);
  hipLaunchKernelGGL(decode_attn_kernel<D>, dim3(B * h, splits), dim3(BLOCK),
                     0, stream, (const short*)qkv.data_ptr(),
                     (short*)kc.data_ptr(), (short*)vc.data_ptr(),
                     lens.data_ptr<int>(), (short*)out.data_ptr(), wsp, (int)h,
                     (int)Smax, chunk, scale, (const int*)nullptr, 1, 0, 0);
  if (splits > 1)
    hipLaunchKernelGGL(decode_merge_kernel<D>, dim3(B * h), dim3(D), 0, stream,
                       (const float*)wsp, (short*)out.data_ptr(), splits);
}

}  // namespace

torch::Tensor decode_attn(torch::Tensor qkv, torch::Tensor k_cache,
                          torch::Tensor v_cache, torch::Tensor seq_lens,
                          double scale, long max_seq_len, long num_splits) {
  TORCH_CHECK(qkv.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() &&
                  seq_lens.is_cuda(),
              "decode_attn: all tensors must be on the GPU");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 &&
                  k_cache.scalar_type() == torch::kBFloat16 &&
                  v_cache.scalar_type() == torch::kBFloat16,
              "decode_attn: qkv and caches must be bf16");
  TORCH_CHECK(qkv.is_contiguous() && k_cache.is_contiguous() &&
                  v_cache.is_contiguous() && seq_lens.is_contiguous(),
              "decode_attn: tensors must be contiguous");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(1) == 1 && qkv.size(3) == 3,
              "decode_attn: qkv must be [B, 1, h, 3, D]");
  const long B = qkv.size(0), h = qkv.size(2), D = qkv.size(4);
  TORCH_CHECK(D == 64 || D == 128, "decode_attn: head_dim must be 64 or 128");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(0) == B &&
                  k_cache.size(1) == h && k_cache.size(3) == D,
              "decode_attn: k_cache must be [B, h, Smax, D]");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(),
              "decode_attn: v_cache shape must equal k_cache shape");
  const long Smax = k_cache.size(2);
  TORCH_CHECK(Smax >= 1 && B * h >= 1 && B * h * Smax * D < (1L << 40),
              "decode_attn: bad cache extent");
  TORCH_CHECK(seq_lens.scalar_type() == torch::kInt && seq_lens.dim() == 1 &&
                  seq_lens.size(0) == B,
              "decode_attn: seq_lens must be int32 [B]");
  TORCH_CHECK(seq_lens.device() == qkv.device() &&
                  k_cache.device() == qkv.device() &&
                  v_cache.device() == qkv.device(),
              "decode_attn: tensors must share one device");
  TORCH_CHECK(max_seq_len >= 1 && max_seq_len <= Smax,
              "decode_attn: max_seq_len must be in [1, Smax]");
  TORCH_CHECK(num_splits >= 0 && num_splits <= MAX_SPLITS,
              "decode_attn: num_splits must be 0 (auto) or 1..32");

  int splits = (int)num_splits;
  if (splits == 0) {
    const int cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    splits = choose_splits(B * h, max_seq_len, cus);
  }
  auto out = torch::empty({B, 1, h * D}, qkv.options());
  if (D == 64)
    launch<64>(qkv, k_cache, v_cache, seq_lens, out, B, h, Smax, max_seq_len,
               splits, (float)scale);
  else
    launch<128>(qkv, k_cache, v_cache, seq_lens, out, B, h, Smax, max_seq_len,
                splits, (float)scale);
  return out;
}
