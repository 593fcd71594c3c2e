// Single-token (decode) attention over a preallocated fp8 KV cache, gfx950,
// and the prefill store that fills such a cache.
//
// Storage: k_cache/v_cache [B, h, Smax, D] OCP e4m3fn codes, k_scale/v_scale
// [B, h, Smax] fp32, one scale per cached row. A row x[D] is quantised as
//   amax = max|x|;  scale = amax / 448, inv = 448 / amax  (1, 1 if amax == 0)
//   code = e4m3_rne(clamp(x * inv, -448, 448));  dequantised = code * scale
// in IEEE fp32 arithmetic (the clamp makes the conversion's overflow
// behaviour irrelevant). A cached row costs D + 4 bytes instead of 2*D.
//
// The decode kernel keeps the shape of decode_attention.hip: no MFMA, no
// LDS staging, 16-byte loads straight to VGPRs, one running (m, l, acc) per
// lane group, split-KV through an fp32 workspace and the shared merge
// launch. A lane owns 16 codes, so a row takes D/16 lanes. The scales are
// applied outside the dot products: s = (q.codes_k) * k_scale and
// acc += (p * v_scale) * codes_v. The new token's K/V enter the softmax
// unquantised from the registers that hold qkv; group 0 of split 0
// quantises them and appends codes and scales at position seq_lens[b].
#include "decode_common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

namespace {

typedef __attribute__((ext_vector_type(4))) int int4v;

constexpr int BLOCK = 256;
constexpr int NW = BLOCK / WAVE;
constexpr int UNROLL = 4;   // independent KV rows in flight per lane group
constexpr float FP8_MAX = 448.f;

// 16 e4m3 codes -> 8 float pairs (v_cvt_pk_f32_fp8, low/high word)
DEV_INLINE void unpack_fp8x16(const int4v& pk, float2v* f) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    f[2 * w] = __builtin_amdgcn_cvt_pk_f32_fp8(pk[w], false);
    f[2 * w + 1] = __builtin_amdgcn_cvt_pk_f32_fp8(pk[w], true);
  }
}

// 16 bf16 of one row (two 16-byte loads) -> fp32
DEV_INLINE void load_bf16x16(const short* p, float* f) {
  const short8v lo = *reinterpret_cast<const short8v*>(p);
  const short8v hi = *reinterpret_cast<const short8v*>(p + 8);
  unpack8(lo, f);
  unpack8(hi, f + 8);
}

// Row scale of the recipe from this lane's 16 values; the GL lanes of a
// group hold one row, and every lane of the group must call this.
template <int GL>
DEV_INLINE void row_scale(const float* x, float& scale, float& inv) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(x[i]));
#pragma unroll
  for (int off = GL / 2; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, WAVE));
  const bool nz = amax > 0.f;
  scale = nz ? amax / FP8_MAX : 1.f;
  inv = nz ? FP8_MAX / amax : 1.f;
}

// 16 fp32 -> 16 e4m3 codes (v_cvt_pk_fp8_f32, round to nearest even)
DEV_INLINE int4v quantize16(const float* x, float inv) {
  int4v r;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      c[j] = fminf(fmaxf(x[4 * w + j] * inv, -FP8_MAX), FP8_MAX);
    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], 0, false);
    r[w] = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], lo, true);
  }
  return r;
}

// grid (B*h, splits), 256 threads. Lane group = D/16 lanes, 256/(D/16)
// groups per block; each group keeps its own running (m, l, acc[16 per
// lane]) and the groups are merged once at the end (shuffles inside the
// wave, then NW*(D+2) floats of LDS across waves). One block iteration
// covers NG*UNROLL positions: 128 at D=128, 256 at D=64.
//
// ws: fp32 [B*h, splits, D+4], see decode_common.h; only touched when
// splits > 1
template <int D>
__global__ __launch_bounds__(BLOCK) void decode_attn_fp8_kernel(
    const short* __restrict__ qkv,          // [B, 1, h, 3, D] bf16
    unsigned char* __restrict__ k_cache,    // [B, h, Smax, D] e4m3
    unsigned char* __restrict__ v_cache,
    float* __restrict__ k_scale,            // [B, h, Smax]
    float* __restrict__ v_scale,
    const int* __restrict__ seq_lens,       // [B]
    short* __restrict__ out,                // [B, 1, h*D] bf16
    float* __restrict__ ws, int h, int Smax, int chunk, float scale) {
  constexpr int GL = D / 16;            // lanes per KV row
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

  const short* qp = qkv + (size_t)bh * 3 * D + li * 16;
  float q[16], knew[16], vnew[16];
  load_bf16x16(qp, q);
#pragma unroll
  for (int i = 0; i < 16; ++i) q[i] *= scale;
  load_bf16x16(qp + D, knew);
  load_bf16x16(qp + 2 * D, vnew);

  const size_t row0 = (size_t)bh * Smax;
  const unsigned char* kbase = k_cache + row0 * D + li * 16;
  const unsigned char* vbase = v_cache + row0 * D + li * 16;
  const float* ksc = k_scale + row0;
  const float* vsc = v_scale + row0;

  float m = -INFINITY, l = 0.f;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  const int4v zero4 = {0, 0, 0, 0};
  // block-uniform trip count: every lane stays active for the shuffles
  for (int base = start; base < end; base += NG * UNROLL) {
    int4v kk[UNROLL], vv[UNROLL];
    float ks[UNROLL], vs[UNROLL];
    bool ok[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int p = base + g + u * NG;
      ok[u] = p < end;
      // positions >= end are never loaded (they may be uninitialised);
      // the scale is one address per group, broadcast by the load unit
      kk[u] = ok[u] ? *reinterpret_cast<const int4v*>(kbase + (size_t)p * D)
                    : zero4;
      vv[u] = ok[u] ? *reinterpret_cast<const int4v*>(vbase + (size_t)p * D)
                    : zero4;
      ks[u] = ok[u] ? ksc[p] : 0.f;
      vs[u] = ok[u] ? vsc[p] : 0.f;
    }
    float s[UNROLL];
    float mn = m;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      float2v kf[8];
      unpack_fp8x16(kk[u], kf);
      float2v d2 = {0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float2v q2 = {q[2 * i], q[2 * i + 1]};
        d2 = __builtin_elementwise_fma(q2, kf[i], d2);
      }
      float d = d2.x + d2.y;
#pragma unroll
      for (int off = GL / 2; off > 0; off >>= 1)
        d += __shfl_xor(d, off, WAVE);
      s[u] = ok[u] ? d * ks[u] : -INFINITY;
      mn = fmaxf(mn, s[u]);
    }
    // a group past the end of its split has seen nothing yet: mn = -inf
    const float ms = (mn == -INFINITY) ? 0.f : mn;
    const float alpha = __expf(m - ms);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] *= alpha;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const float pw = ok[u] ? __expf(s[u] - ms) : 0.f;
      const float pv = pw * vs[u];
      const float2v pv2 = {pv, pv};
      float2v vf[8];
      unpack_fp8x16(vv[u], vf);
      l += pw;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float2v a2 = {acc[2 * i], acc[2 * i + 1]};
        a2 = __builtin_elementwise_fma(pv2, vf[i], a2);
        acc[2 * i] = a2.x;
        acc[2 * i + 1] = a2.y;
      }
    }
    m = mn;
  }

  // new token: quantised and appended by group 0 of split 0 (every group
  // runs the shuffles of row_scale; only the owner stores), folded into
  // the softmax unquantised
  const bool owns_new = (split == 0) && (g == 0);
  {
    float k_s, k_inv, v_s, v_inv;
    row_scale<GL>(knew, k_s, k_inv);
    row_scale<GL>(vnew, v_s, v_inv);
    if (owns_new) {
      const size_t row = row0 + (size_t)L;
      *reinterpret_cast<int4v*>(k_cache + row * D + li * 16) =
          quantize16(knew, k_inv);
      *reinterpret_cast<int4v*>(v_cache + row * D + li * 16) =
          quantize16(vnew, v_inv);
      if (li == 0) {
        k_scale[row] = k_s;
        v_scale[row] = v_s;
      }
    }
  }
  {
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) d = fmaf(q[i], knew[i], d);
#pragma unroll
    for (int off = GL / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, WAVE);
    const float m_o = owns_new ? d : -INFINITY;
    const float l_o = owns_new ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) vnew[i] = owns_new ? vnew[i] : 0.f;
    merge_state<16>(m, l, acc, m_o, l_o, vnew);
  }

  // groups inside the wave
#pragma unroll
  for (int off = GL; off < WAVE; off <<= 1) {
    const float m_o = __shfl_xor(m, off, WAVE);
    const float l_o = __shfl_xor(l, off, WAVE);
    float acc_o[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc_o[i] = __shfl_xor(acc[i], off, WAVE);
    merge_state<16>(m, l, acc, m_o, l_o, acc_o);
  }
  // waves through LDS
  if (lane < GL) {
#pragma unroll
    for (int i = 0; i < 16; ++i) s_acc[wid][li * 16 + i] = acc[i];
    if (lane == 0) { s_ml[wid][0] = m; s_ml[wid][1] = l; }
  }
  __syncthreads();
  if (tid < GL) {
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      float acc_o[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc_o[i] = s_acc[w][li * 16 + i];
      merge_state<16>(m, l, acc, s_ml[w][0], s_ml[w][1], acc_o);
    }
    if (splits == 1) {
      // l >= 1 term of the new token, so the division is safe
      const float inv = 1.f / l;
      short* op = out + (size_t)bh * D + li * 16;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        short8v o;
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
          const unsigned int u = cvt_pk_bf16(acc[half * 8 + i] * inv,
                                             acc[half * 8 + i + 1] * inv);
          ((unsigned short*)&o)[i] = (unsigned short)u;
          ((unsigned short*)&o)[i + 1] = (unsigned short)(u >> 16);
        }
        *reinterpret_cast<short8v*>(op + half * 8) = o;
      }
    } else {
      float* w = ws + ((size_t)bh * splits + split) * (D + 4) + li * 16;
#pragma unroll
      for (int i = 0; i < 16; i += 4) {
        const float4v t = {acc[i], acc[i + 1], acc[i + 2], acc[i + 3]};
        *reinterpret_cast<float4v*>(w + i) = t;
      }
      if (tid == 0) { w[D] = m; w[D + 1] = l; }
    }
  }
}

// Prefill store: one lane group per (b, s, head, K|V) row of the packed
// qkv [B, S, h, 3, D]; quantises it into position s of the caches. grid
// ceil(rows / NG), 256 threads. Positions >= S are not touched.
template <int D>
__global__ __launch_bounds__(BLOCK) void kv_store_fp8_kernel(
    const short* __restrict__ qkv, unsigned char* __restrict__ k_cache,
    unsigned char* __restrict__ v_cache, float* __restrict__ k_scale,
    float* __restrict__ v_scale, int S, int h, int Smax, long rows) {
  constexpr int GL = D / 16;
  constexpr int NG = BLOCK / GL;
  const int li = threadIdx.x % GL;
  const long r = (long)blockIdx.x * NG + threadIdx.x / GL;
  // a group past the last row computes on row 0 and stores nothing, so
  // every lane stays active for the shuffles
  const bool ok = r < rows;
  const long rr = ok ? r : 0;
  const int which = (int)(rr & 1);      // 0: K, 1: V
  const long tok = rr >> 1;             // (b*S + s)*h + head
  const long head = tok % h;
  const long s = (tok / h) % S;
  const long b = tok / h / S;

  float x[16];
  load_bf16x16(qkv + (size_t)(tok * 3 + 1 + which) * D + li * 16, x);
  float sc, inv;
  row_scale<GL>(x, sc, inv);
  if (ok) {
    const size_t row = (size_t)(b * h + head) * Smax + s;
    unsigned char* cache = which ? v_cache : k_cache;
    float* scales = which ? v_scale : k_scale;
    *reinterpret_cast<int4v*>(cache + row * D + li * 16) = quantize16(x, inv);
    if (li == 0) scales[row] = sc;
  }
}

template <int D>
void launch(torch::Tensor& qkv, torch::Tensor& kc, torch::Tensor& vc,
            torch::Tensor& ks, torch::Tensor& vs, torch::Tensor& lens,
            torch::Tensor& out, long B, long h, long Smax, long max_seq_len,
            int splits, float scale) {
  auto stream = at::hip::getCurrentHIPStream();
  torch::Tensor ws;
  float* wsp = nullptr;
  if (splits > 1) {
    ws = torch::empty({B * h, (long)splits, (long)D + 4},
                      qkv.options().dtype(torch::kFloat));
    wsp = ws.data_ptr<float>();
  }
  const int chunk = (int)((max_seq_len + splits - 1) / splits);
  hipLaunchKernelGGL(decode_attn_fp8_kernel<D>, dim3(B * h, splits),
                     dim3(BLOCK), 0, stream, (const short*)qkv.data_ptr(),
                     (unsigned char*)kc.data_ptr(),
                     (unsigned char*)vc.data_ptr(), ks.data_ptr<float>(),
                     vs.data_ptr<float>(), lens.data_ptr<int>(),
                     (short*)out.data_ptr(), wsp, (int)h, (int)Smax, chunk,
                     scale);
  if (splits > 1)
    hipLaunchKernelGGL(decode_merge_kernel<D>, dim3(B * h), dim3(D), 0, stream,
                       (const float*)wsp, (short*)out.data_ptr(), splits);
}

bool aligned16(const torch::Tensor& t) {
  return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
}

// Checks shared by both entry points: the fp8 caches and their scales
// against B, h, D of qkv. Returns Smax.
long check_fp8_cache(const char* op, const torch::Tensor& qkv,
                     const torch::Tensor& k_cache,
                     const torch::Tensor& v_cache,
                     const torch::Tensor& k_scale,
                     const torch::Tensor& v_scale) {
  TORCH_CHECK(qkv.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() &&
                  k_scale.is_cuda() && v_scale.is_cuda(),
              op, ": all tensors must be on the GPU");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16, op,
              ": qkv must be bf16");
  TORCH_CHECK(k_cache.scalar_type() == torch::kFloat8_e4m3fn &&
                  v_cache.scalar_type() == torch::kFloat8_e4m3fn,
              op, ": caches must be float8_e4m3fn");
  TORCH_CHECK(k_scale.scalar_type() == torch::kFloat &&
                  v_scale.scalar_type() == torch::kFloat,
              op, ": scales must be fp32");
  TORCH_CHECK(qkv.is_contiguous() && k_cache.is_contiguous() &&
                  v_cache.is_contiguous() && k_scale.is_contiguous() &&
                  v_scale.is_contiguous(),
              op, ": tensors must be contiguous");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(3) == 3, op,
              ": qkv must be [B, S, h, 3, D]");
  const long B = qkv.size(0), h = qkv.size(2), D = qkv.size(4);
  TORCH_CHECK(D == 64 || D == 128, op, ": head_dim must be 64 or 128");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(0) == B &&
                  k_cache.size(1) == h && k_cache.size(3) == D,
              op, ": k_cache must be [B, h, Smax, D]");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(), op,
              ": v_cache shape must equal k_cache shape");
  const long Smax = k_cache.size(2);
  TORCH_CHECK(Smax >= 1 && Smax < (1L << 26) && B * h >= 1 &&
                  B * h * Smax * D < (1L << 40),
              op, ": bad cache extent");
  TORCH_CHECK(k_scale.dim() == 3 && k_scale.size(0) == B &&
                  k_scale.size(1) == h && k_scale.size(2) == Smax &&
                  v_scale.sizes() == k_scale.sizes(),
              op, ": k_scale and v_scale must be [B, h, Smax]");
  TORCH_CHECK(k_cache.device() == qkv.device() &&
                  v_cache.device() == qkv.device() &&
                  k_scale.device() == qkv.device() &&
                  v_scale.device() == qkv.device(),
              op, ": tensors must share one device");
  TORCH_CHECK(aligned16(qkv) && aligned16(k_cache) && aligned16(v_cache),
              op, ": qkv and caches must be 16-byte aligned");
  return Smax;
}

}  // namespace

torch::Tensor decode_attn_fp8(torch::Tensor qkv, torch::Tensor k_cache,
                              torch::Tensor v_cache, torch::Tensor k_scale,
                              torch::Tensor v_scale, torch::Tensor seq_lens,
                              double scale, long max_seq_len,
                              long num_splits) {
  const long Smax = check_fp8_cache("decode_attn_fp8", qkv, k_cache, v_cache,
                                    k_scale, v_scale);
  TORCH_CHECK(qkv.size(1) == 1, "decode_attn_fp8: qkv must be [B, 1, h, 3, D]");
  const long B = qkv.size(0), h = qkv.size(2), D = qkv.size(4);
  TORCH_CHECK(seq_lens.is_cuda() && seq_lens.scalar_type() == torch::kInt &&
                  seq_lens.dim() == 1 && seq_lens.size(0) == B &&
                  seq_lens.is_contiguous(),
              "decode_attn_fp8: seq_lens must be a contiguous int32 [B] on "
              "the GPU");
  TORCH_CHECK(seq_lens.device() == qkv.device(),
              "decode_attn_fp8: tensors must share one device");
  TORCH_CHECK(max_seq_len >= 1 && max_seq_len <= Smax,
              "decode_attn_fp8: max_seq_len must be in [1, Smax]");
  TORCH_CHECK(num_splits >= 0 && num_splits <= MAX_SPLITS,
              "decode_attn_fp8: num_splits must be 0 (auto) or 1..32");

  int splits = (int)num_splits;
  if (splits == 0) {
    const int cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    splits = choose_splits(B * h, max_seq_len, cus);
  }
  auto out = torch::empty({B, 1, h * D}, qkv.options());
  if (D == 64)
    launch<64>(qkv, k_cache, v_cache, k_scale, v_scale, seq_lens, out, B, h,
               Smax, max_seq_len, splits, (float)scale);
  else
    launch<128>(qkv, k_cache, v_cache, k_scale, v_scale, seq_lens, out, B, h,
                Smax, max_seq_len, splits, (float)scale);
  return out;
}

void kv_store_fp8(torch::Tensor qkv, torch::Tensor k_cache,
                  torch::Tensor v_cache, torch::Tensor k_scale,
                  torch::Tensor v_scale) {
  const long Smax = check_fp8_cache("kv_store_fp8", qkv, k_cache, v_cache,
                                    k_scale, v_scale);
  const long B = qkv.size(0), S = qkv.size(1), h = qkv.size(2),
             D = qkv.size(4);
  TORCH_CHECK(S <= Smax, "kv_store_fp8: S must be <= Smax");
  const long rows = B * S * h * 2;
  if (rows == 0) return;
  const long ng = BLOCK / (D / 16);  // rows per block
  const long blocks = (rows + ng - 1) / ng;
  TORCH_CHECK(blocks < (1L << 31), "kv_store_fp8: too many rows");
  auto stream = at::hip::getCurrentHIPStream();
  auto run = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(BLOCK), 0, stream,
                       (const short*)qkv.data_ptr(),
                       (unsigned char*)k_cache.data_ptr(),
                       (unsigned char*)v_cache.data_ptr(),
                       k_scale.data_ptr<float>(), v_scale.data_ptr<float>(),
                       (int)S, (int)h, (int)Smax, rows);
  };
  if (D == 64)
    run(kv_store_fp8_kernel<64>);
  else
    run(kv_store_fp8_kernel<128>);
}
