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
#include "decode_common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

constexpr int BLOCK = 256;
constexpr int NW = BLOCK / WAVE;
constexpr int UNROLL = 4;   // independent KV rows in flight per lane group

// grid (B*h, splits), 256 threads. Lane group = D/8 lanes, 256/(D/8) groups
// per block; each group keeps its own running (m, l, acc[8 per lane]) and
// the groups are merged once at the end (shuffles inside the wave, then
// NW*(D+2) floats of LDS across waves).
//
// ws: fp32 [B*h, splits, D+4] = acc[D], m, l, pad (rows stay 16-byte
// aligned); only touched when splits > 1
template <int D>
__global__ __launch_bounds__(BLOCK) void decode_attn_kernel(
    const short* __restrict__ qkv,      // [B, 1, h, 3, D] bf16
    short* __restrict__ k_cache,        // [B, h, Smax, D] bf16
    short* __restrict__ v_cache,
    const int* __restrict__ seq_lens,   // [B]
    short* __restrict__ out,            // [B, 1, h*D] bf16
    float* __restrict__ ws, int h, int Smax, int chunk, float scale) {
  constexpr int GL = D / 8;             // lanes per KV row
  constexpr int NG = BLOCK / GL;        // rows per block step
  __shared__ float s_acc[NW][D];
  __shared__ float s_ml[NW][2];

  const int bh = blockIdx.x;
  const int b = bh / h;
  const int split = blockIdx.y;
  const int splits = gridDim.y;
  const int tid = threadIdx.x;
  const int g = tid / GL;
  const int li = tid % GL;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;

  // a bad length gives wrong numbers, never an out-of-bounds address
  const int L = min(max(seq_lens[b], 0), Smax - 1);
  // cached positions [start, end) of this split; the last split runs to L
  // so an under-estimated max_seq_len cannot drop positions
  const int start = min(split * chunk, L);
  const int end = (split == splits - 1) ? L : min((split + 1) * chunk, L);

  const short* qp = qkv + (size_t)bh * 3 * D + li * 8;
  float q[8];
  {
    const short8v qpk = *reinterpret_cast<const short8v*>(qp);
    unpack8(qpk, q);
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] *= scale;
  }
  const short8v knew = *reinterpret_cast<const short8v*>(qp + D);
  const short8v vnew = *reinterpret_cast<const short8v*>(qp + 2 * D);

  const size_t head_off = (size_t)bh * Smax * D + li * 8;
  const short* kbase = k_cache + head_off;
  const short* vbase = v_cache + head_off;

  float m = -INFINITY, l = 0.f;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;

  const short8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  // block-uniform trip count: every lane stays active for the shuffles
  for (int base = start; base < end; base += NG * UNROLL) {
    short8v kk[UNROLL], vv[UNROLL];
    bool ok[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int p = base + g + u * NG;
      ok[u] = p < end;
      // positions >= end are never loaded (they may be uninitialised)
      kk[u] = ok[u] ? *reinterpret_cast<const short8v*>(kbase + (size_t)p * D)
                    : zero8;
      vv[u] = ok[u] ? *reinterpret_cast<const short8v*>(vbase + (size_t)p * D)
                    : zero8;
    }
    float s[UNROLL];
    float mn = m;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      float kf[8];
      unpack8(kk[u], kf);
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) d = fmaf(q[i], kf[i], d);
#pragma unroll
      for (int off = GL / 2; off > 0; off >>= 1)
        d += __shfl_xor(d, off, WAVE);
      s[u] = ok[u] ? d : -INFINITY;
      mn = fmaxf(mn, s[u]);
    }
    // a group past the end of its split has seen nothing yet: mn = -inf
    const float ms = (mn == -INFINITY) ? 0.f : mn;
    const float alpha = __expf(m - ms);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] *= alpha;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const float pw = ok[u] ? __expf(s[u] - ms) : 0.f;
      float vf[8];
      unpack8(vv[u], vf);
      l += pw;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(pw, vf[i], acc[i]);
    }
    m = mn;
  }

  // new token: appended to the cache and folded in by group 0 of split 0
  const bool owns_new = (split == 0) && (g == 0);
  if (owns_new) {
    *reinterpret_cast<short8v*>(k_cache + head_off + (size_t)L * D) = knew;
    *reinterpret_cast<short8v*>(v_cache + head_off + (size_t)L * D) = vnew;
  }
  {
    float kf[8], vf[8];
    unpack8(knew, kf);
    unpack8(vnew, vf);
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) d = fmaf(q[i], kf[i], d);
#pragma unroll
    for (int off = GL / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, WAVE);
    const float m_o = owns_new ? d : -INFINITY;
    const float l_o = owns_new ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) vf[i] = owns_new ? vf[i] : 0.f;
    merge_state(m, l, acc, m_o, l_o, vf);
  }

  // groups inside the wave
#pragma unroll
  for (int off = GL; off < WAVE; off <<= 1) {
    const float m_o = __shfl_xor(m, off, WAVE);
    const float l_o = __shfl_xor(l, off, WAVE);
    float acc_o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc_o[i] = __shfl_xor(acc[i], off, WAVE);
    merge_state(m, l, acc, m_o, l_o, acc_o);
  }
  // waves through LDS
  if (lane < GL) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s_acc[wid][li * 8 + i] = acc[i];
    if (lane == 0) { s_ml[wid][0] = m; s_ml[wid][1] = l; }
  }
  __syncthreads();
  if (tid < GL) {
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      float acc_o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc_o[i] = s_acc[w][li * 8 + i];
      merge_state(m, l, acc, s_ml[w][0], s_ml[w][1], acc_o);
    }
    if (splits == 1) {
      // l >= 1 term of the new token, so the division is safe
      const float inv = 1.f / l;
      short8v o;
#pragma unroll
      for (int i = 0; i < 8; i += 2) {
        const unsigned int u = cvt_pk_bf16(acc[i] * inv, acc[i + 1] * inv);
        ((unsigned short*)&o)[i] = (unsigned short)u;
        ((unsigned short*)&o)[i + 1] = (unsigned short)(u >> 16);
      }
      *reinterpret_cast<short8v*>(out + (size_t)bh * D + li * 8) = o;
    } else {
      float* w = ws + ((size_t)bh * splits + split) * (D + 4);
      float4v lo = {acc[0], acc[1], acc[2], acc[3]};
      float4v hi = {acc[4], acc[5], acc[6], acc[7]};
      *reinterpret_cast<float4v*>(w + li * 8) = lo;
      *reinterpret_cast<float4v*>(w + li * 8 + 4) = hi;
      if (tid == 0) { w[D] = m; w[D + 1] = l; }
    }
  }
}

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
                     (int)Smax, chunk, scale);
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
