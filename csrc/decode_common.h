// Pieces shared by the decode-attention kernels (decode_attention.hip: bf16
// cache, decode_attention_fp8.hip: fp8 cache): bf16 unpack, online-softmax
// state merge, the split-KV merge launch and the split rule.
//
// Everything sits in an unnamed namespace on purpose: each translation unit
// that includes this header gets its own copy of the merge kernel and
// registers it with its own code object.
#pragma once

#include "common.h"

#include <algorithm>

namespace {

constexpr int MAX_SPLITS = 32;

DEV_INLINE void unpack8(const short8v& pk, float* f) {
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = bf_raw2f(((const unsigned short*)&pk)[i]);
}

// Merge the online-softmax state (m_o, l_o, acc_o) into (m, l, acc); N
// channels per lane. Either side may be empty (m = -inf, l = 0): the max is
// replaced by 0 for the exponent so exp(-inf - -inf) never appears.
template <int N = 8>
DEV_INLINE void merge_state(float& m, float& l, float* acc, float m_o,
                            float l_o, const float* acc_o) {
  const float mn = fmaxf(m, m_o);
  const float ms = (mn == -INFINITY) ? 0.f : mn;
  const float a = __expf(m - ms);
  const float b = __expf(m_o - ms);
  l = l * a + l_o * b;
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = acc[i] * a + acc_o[i] * b;
  m = mn;
}

// ws: fp32 [B*h, splits, D+4] = acc[D], m, l, pad (rows stay 16-byte
// aligned), written by the attention launch when splits > 1.
//
// grid B*h, D threads: thread d merges channel d over the splits. Empty
// splits carry m = -inf, l = 0 and get weight exp(-inf) = 0; split 0 always
// holds the new token, so the global max is finite and the sum is > 0.
template <int D>
__global__ __launch_bounds__(D) void decode_merge_kernel(
    const float* __restrict__ ws, short* __restrict__ out, int splits) {
  const int bh = blockIdx.x;
  const int d = threadIdx.x;
  const float* w = ws + (size_t)bh * splits * (D + 4);
  float mx = -INFINITY;
  for (int s = 0; s < splits; ++s) mx = fmaxf(mx, w[s * (D + 4) + D]);
  const float ms = (mx == -INFINITY) ? 0.f : mx;
  float num = 0.f, den = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float* ws_s = w + s * (D + 4);
    const float m_s = ws_s[D];
    const float wt = (m_s == -INFINITY) ? 0.f : __expf(m_s - ms);
    num = fmaf(wt, ws_s[d], num);
    den = fmaf(wt, ws_s[D + 1], den);
  }
  out[(size_t)bh * D + d] = (short)f2bf_raw(num / den);
}

// Split rule: the smallest split count that brings B*h*splits to about the
// CU count (one 256-thread workgroup per CU is enough to saturate HBM when
// every lane keeps 8 16-byte loads in flight), capped so that every
// split keeps at least 256 positions of max_seq_len (below that the merge
// launch costs more than the extra parallelism returns) and at MAX_SPLITS.
inline int choose_splits(long bh, long max_seq_len, int num_cus) {
  long want = (num_cus + bh - 1) / bh;
  long cap = std::max<long>(1, max_seq_len / 256);
  return (int)std::max<long>(1, std::min<long>({want, cap, MAX_SPLITS}));
}

}  // namespace
