// Weight-streaming linear for the decode step with fp8 weights, gfx950.
//
//   y[M,N] = act((x[M,K] . Wq[N,K]^T) * w_scale[N] + bias[N]) + residual[M,N]
//
// x, bias, residual and y are bf16; Wq holds float8_e4m3fn codes in the
// nn.Linear layout [N][K] and w_scale one fp32 scale per output row
// (ref.quantize_weight_rows). The op is a read of Wq, N*K bytes: half of what
// decode_linear.hip streams for the same layer.
//
// Structure of decode_linear.hip: Wq goes from global memory straight to
// VGPRs in 16-byte loads and is read once, x comes from L2, the k-steps are
// dealt to the waves in contiguous chunks, partial tiles are summed through
// LDS in wave order (bitwise reproducible) and the epilogue runs in the same
// launch. No counters, flags or atomics, no workspace.
//
// Fragments. A 16-byte load is 16 codes, so a k-step is 64 wide: a lane owns
// row lane&15, k (lane>>4)*16 .. +16 of it. Codes 0-7 and 8-15 become the A
// fragments of two v_mfma_f32_16x16x32_bf16; the B fragments are the two
// 16-byte loads of x at the same k. The MFMA sums over (lane group, element)
// pairs, so any k assignment that A and B share is a valid contraction.
//
// Decode. Every finite e4m3fn value is exactly a bf16 value (4 significand
// bits, exponent range inside bf16's), so codes are converted in registers:
// v_cvt_pk_f32_fp8 gives two fp32 whose low 16 bits are zero, v_perm_b32
// packs their high halves. About one VALU op per code, no rounding: the
// kernel computes x . codes^T exactly as the bf16 kernel would from the
// decoded matrix, and the one new rounding is the multiply by the scale.
//
// Rows of Wq and entries of w_scale at index >= N, rows of x at index >= M
// and k-steps past a wave's chunk are never loaded: every such load sits
// behind a predicate (exec-masked, valid base address), and nothing such a
// lane holds reaches a stored element.
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>
#include <string>

namespace {

typedef __attribute__((ext_vector_type(4))) int int4v;

constexpr int TILE = 16;     // MFMA rows (n) and columns (m)
constexpr int KSTEP = 64;    // k per 16-byte load of codes: two MFMAs
constexpr float GELU_K = 0.7978845608028654f;  // sqrt(2/pi)

// the tanh-GELU of elementwise.hip (bias_gelu) and decode_linear.hip
DEV_INLINE float gelu_tanh(float x) {
  const float t =
      1.f - 2.f / (__expf(2.f * GELU_K * (x + 0.044715f * x * x * x)) + 1.f);
  return 0.5f * x * (1.f + t);
}

template <bool NT>
DEV_INLINE int4v load16(const void* p) {
  if constexpr (NT)
    return __builtin_nontemporal_load(reinterpret_cast<const int4v*>(p));
  else
    return *reinterpret_cast<const int4v*>(p);
}

DEV_INLINE mfma_bf16x8 as_frag(const int4v& v) {
  union { int4v i; mfma_bf16x8 f; } u;
  u.i = v;
  return u.f;
}

// 8 e4m3 codes (two words) -> 8 bf16, exact: the high halves of the fp32 pair
DEV_INLINE mfma_bf16x8 decode8(int w0, int w1) {
  int4v o;
  const int w[2] = {w0, w1};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float2v lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);
    const float2v hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
    o[2 * i] = (int)__builtin_amdgcn_perm(__float_as_uint(lo[1]),
                                          __float_as_uint(lo[0]), 0x07060302u);
    o[2 * i + 1] = (int)__builtin_amdgcn_perm(
        __float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
  }
  return as_frag(o);
}

// k-steps in flight per wave. Codes take 4 VGPRs per step and tile, x 8 per
// step: four tiles keep 4 steps (64 + 32 VGPRs), fewer tiles 8.
template <int TILES>
struct Flight { static constexpr int U = TILES == 4 ? 4 : 8; };

// grid ceil(N / rows), NW*64 threads; rows = 16*TILES, or 8 with TILES = 1
// (the upper half of the MFMA tile masked). The TILES tiles of a workgroup
// share every x fragment.
template <int NW, int TILES, bool NT>
__global__ __launch_bounds__(NW * WAVE) void decode_linear_fp8_kernel(
    const short* __restrict__ x,          // [M, K] bf16
    const unsigned char* __restrict__ w,  // [N, K] e4m3fn
    const float* __restrict__ w_scale,    // [N]
    const short* __restrict__ bias,       // [N] or null
    const short* __restrict__ res,        // [M, N] or null
    short* __restrict__ y,                // [M, N]
    int M, int N, int K, int rows, int gelu) {
  constexpr int U = Flight<TILES>::U;
  __shared__ float s_part[NW][TILES * TILE * TILE];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  // wave-uniform: keeps the chunk bounds and their branches scalar
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int r = lane & 15;              // W row in the tile / x row
  const int kg = (lane >> 4) * 16;      // k offset inside a k-step
  const int n0 = blockIdx.x * rows;
  const int tile_rows = min(rows, TILE);

  // masked lanes keep a valid base (row 0) and never dereference it
  bool w_ok[TILES];
  const unsigned char* wp[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const int row = n0 + t * TILE + r;
    w_ok[t] = (r < tile_rows) && (row < N);
    wp[t] = w + (size_t)(w_ok[t] ? row : 0) * K + kg;
  }
  const bool x_ok = r < M;
  const short* xp = x + (size_t)(x_ok ? r : 0) * K + kg;

  // this wave's k-steps [s_beg, s_end): contiguous, sizes differ by <= 1
  const int steps = K / KSTEP;
  const int s_beg = (int)(((long)steps * wid) / NW);
  const int s_end = (int)(((long)steps * (wid + 1)) / NW);

  mfma_f32x4 acc[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc[t] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
  // Fragments of masked lanes are never loaded and need no zero: row n of C
  // depends on row n of A alone and column m on column m of B alone, and
  // the epilogue stores neither rows >= N nor columns >= M. They start as
  // zero and keep whatever they held.
  const int4v zero4 = {0, 0, 0, 0};
  int4v a[TILES][U], b[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    b[u][0] = b[u][1] = zero4;
#pragma unroll
    for (int t = 0; t < TILES; ++t) a[t][u] = zero4;
  }
  // Wave-uniform trip count and batch size. One code path for full and
  // partial batches (u < nb is a scalar branch): a second, specialised path
  // keeps a second set of fragments live, which the fp8 kernel's registers
  // do not have room for. K-steps past the chunk are neither loaded nor
  // multiplied.
  // Order of the loads (measured, KERNELS.md): with one tile, step by step
  // with the x loads between the code loads; with more tiles, tile by tile
  // (the loads of one row's consecutive 64 bytes adjacent), then x. The
  // other order costs 10 % with one tile and up to 40 % with two.
  for (int s = s_beg; s < s_end; s += U) {
    const size_t off = (size_t)s * KSTEP;
    const int nb = s_end - s;
    if constexpr (TILES > 1) {
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        if (w_ok[t]) {
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (u < nb) a[t][u] = load16<NT>(wp[t] + off + u * KSTEP);
        }
      }
      if (x_ok) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u < nb) {
            b[u][0] = load16<false>(xp + off + u * KSTEP);
            b[u][1] = load16<false>(xp + off + u * KSTEP + 8);
          }
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u < nb) {
          if (w_ok[0]) a[0][u] = load16<NT>(wp[0] + off + u * KSTEP);
          if (x_ok) {
            b[u][0] = load16<false>(xp + off + u * KSTEP);
            b[u][1] = load16<false>(xp + off + u * KSTEP + 8);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < nb) {
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              decode8(a[t][u][0], a[t][u][1]), as_frag(b[u][0]), acc[t], 0, 0,
              0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              decode8(a[t][u][2], a[t][u][3]), as_frag(b[u][1]), acc[t], 0, 0,
              0);
        }
      }
    }
  }

  // C[n][m]: m = lane & 15, n = (lane >> 4) * 4 + i -> s_part[w][t][m*16 + n]
#pragma unroll
  for (int t = 0; t < TILES; ++t)
    *reinterpret_cast<float4v*>(
        &s_part[wid][t * TILE * TILE + r * TILE + (lane >> 4) * 4]) = acc[t];
  __syncthreads();

  // element e = (tile t, m, n in tile): summed over the waves in wave order
  for (int e = tid; e < TILES * TILE * TILE; e += NW * WAVE) {
    const int m = (e >> 4) & 15;
    const int nt = e & 15;
    const int n = n0 + (e >> 8) * TILE + nt;
    if (m < M && nt < tile_rows && n < N) {
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < NW; ++i) v += s_part[i][e];
      v *= w_scale[n];
      if (bias) v += bf_raw2f((unsigned short)bias[n]);
      if (gelu) v = gelu_tanh(v);
      const size_t o = (size_t)m * N + n;
      if (res) v += bf_raw2f((unsigned short)res[o]);
      y[o] = (short)f2bf_raw(v);
    }
  }
}

struct Args {
  const short* x;
  const unsigned char* w;
  const float* w_scale;
  const short *bias, *res;
  short* y;
  int M, N, K, rows, gelu;
};

template <int NW, int TILES, bool NT>
void launch(const Args& a) {
  auto stream = at::hip::getCurrentHIPStream();
  const int grid = (a.N + a.rows - 1) / a.rows;
  hipLaunchKernelGGL((decode_linear_fp8_kernel<NW, TILES, NT>), dim3(grid),
                     dim3(NW * WAVE), 0, stream, a.x, a.w, a.w_scale, a.bias,
                     a.res, a.y, a.M, a.N, a.K, a.rows, a.gelu);
}

template <int NW, bool NT>
void launch_tiles(const Args& a) {
  if (a.rows == 64) launch<NW, 4, NT>(a);
  else if (a.rows == 32) launch<NW, 2, NT>(a);
  else launch<NW, 1, NT>(a);
}

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

}  // namespace

// rows / waves / nontemporal: 0 / 0 / -1 choose automatically; other values
// are the benchmark's sweep (rows 8, 16, 32 or 64, waves 4 or 8, nt 0 or 1).
torch::Tensor decode_linear_fp8(torch::Tensor x, torch::Tensor wq,
                                torch::Tensor w_scale,
                                c10::optional<torch::Tensor> bias,
                                c10::optional<torch::Tensor> residual,
                                const std::string& act, long rows, long waves,
                                long nontemporal) {
  TORCH_CHECK(x.defined() && wq.defined() && w_scale.defined(),
              "decode_linear_fp8: x, wq and w_scale must be defined");
  TORCH_CHECK(x.is_cuda() && wq.is_cuda() && w_scale.is_cuda(),
              "decode_linear_fp8: x, wq and w_scale must be GPU tensors");
  TORCH_CHECK(wq.device() == x.device() && w_scale.device() == x.device(),
              "decode_linear_fp8: wq and w_scale must be on ", x.device());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16,
              "decode_linear_fp8: x must be bfloat16, got ", x.scalar_type());
  TORCH_CHECK(wq.scalar_type() == torch::kFloat8_e4m3fn,
              "decode_linear_fp8: wq must be float8_e4m3fn, got ",
              wq.scalar_type());
  TORCH_CHECK(x.dim() == 2 && wq.dim() == 2,
              "decode_linear_fp8: x must be [M, K] and wq [N, K]");
  TORCH_CHECK(x.is_contiguous(), "decode_linear_fp8: x must be contiguous");
  TORCH_CHECK(wq.is_contiguous(), "decode_linear_fp8: wq must be contiguous");
  const long M = x.size(0), K = x.size(1), N = wq.size(0);
  TORCH_CHECK(wq.size(1) == K, "decode_linear_fp8: wq must be [N, ", K,
              "], got [", N, ", ", wq.size(1), "]");
  TORCH_CHECK(M >= 1 && M <= TILE,
              "decode_linear_fp8: M must be in [1, 16], got ", M);
  TORCH_CHECK(K >= KSTEP && K % KSTEP == 0,
              "decode_linear_fp8: K must be a positive multiple of 64, got ",
              K);
  TORCH_CHECK(N >= 8 && N % 8 == 0,
              "decode_linear_fp8: N must be a positive multiple of 8, got ",
              N);
  TORCH_CHECK(N * K < (1L << 40) && N < (1L << 30) && K < (1L << 30),
              "decode_linear_fp8: bad weight extent");
  TORCH_CHECK(aligned16(x) && aligned16(wq),
              "decode_linear_fp8: x and wq must be 16-byte aligned");
  TORCH_CHECK(w_scale.scalar_type() == torch::kFloat32 &&
                  w_scale.is_contiguous() && w_scale.dim() == 1 &&
                  w_scale.size(0) == N,
              "decode_linear_fp8: w_scale must be a contiguous float32 [", N,
              "]");
  TORCH_CHECK(act == "none" || act == "gelu",
              "decode_linear_fp8: act must be 'none' or 'gelu', got '", act,
              "'");
  const short* bp = nullptr;
  const short* rp = nullptr;
  if (bias.has_value() && bias->defined()) {
    const torch::Tensor& b = *bias;
    TORCH_CHECK(b.scalar_type() == torch::kBFloat16 &&
                    b.device() == x.device() && b.is_contiguous() &&
                    b.dim() == 1 && b.size(0) == N,
                "decode_linear_fp8: bias must be a contiguous bfloat16 [", N,
                "] on ", x.device());
    bp = (const short*)b.data_ptr();
  }
  if (residual.has_value() && residual->defined()) {
    const torch::Tensor& rs = *residual;
    TORCH_CHECK(rs.scalar_type() == torch::kBFloat16 &&
                    rs.device() == x.device() && rs.is_contiguous() &&
                    rs.dim() == 2 && rs.size(0) == M && rs.size(1) == N,
                "decode_linear_fp8: residual must be a contiguous bfloat16 [",
                M, ", ", N, "] on ", x.device());
    rp = (const short*)rs.data_ptr();
  }
  TORCH_CHECK(rows == 0 || rows == 8 || rows == 16 || rows == 32 || rows == 64,
              "decode_linear_fp8: rows must be 0 (auto), 8, 16, 32 or 64");
  TORCH_CHECK(waves == 0 || waves == 4 || waves == 8,
              "decode_linear_fp8: waves must be 0 (auto), 4 or 8");
  TORCH_CHECK(nontemporal >= -1 && nontemporal <= 1,
              "decode_linear_fp8: nontemporal must be -1 (auto), 0 or 1");

  // Measured choice (benchmarks/bench_decode_linear.py --weight-dtype fp8
  // --sweep at M = 1 and 16, GPT-1.3B and 6.7B shapes, KERNELS.md). Half
  // tiles while full tiles would leave CUs without a workgroup. More tiles
  // share the x fragments, which at 16 rows are M/8 times the bytes of the
  // codes: from M = 8 on, the most of 64 / 32 rows that still gives 3/4 of
  // the CUs a workgroup. A grid of at most two workgroups per CU runs 8
  // waves and non-temporal code loads, a larger one 4 waves and plain loads.
  const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  if (rows == 0) {
    rows = (N + 15) / 16 < cus ? 8 : 16;
    if (rows == 16 && M >= 8) {
      for (long cand : {64L, 32L})
        if ((N + cand - 1) / cand >= (3 * cus) / 4) { rows = cand; break; }
    }
  }
  const bool small_grid = (N + rows - 1) / rows <= 2 * cus;
  if (waves == 0) waves = small_grid ? 8 : 4;
  const bool nt = nontemporal < 0 ? small_grid : nontemporal != 0;

  auto y = torch::empty({M, N}, x.options());
  const Args a{(const short*)x.data_ptr(),
               (const unsigned char*)wq.data_ptr(),
               (const float*)w_scale.data_ptr(), bp, rp, (short*)y.data_ptr(),
               (int)M, (int)N, (int)K, (int)rows, act == "gelu"};
  if (waves == 4) {
    if (nt) launch_tiles<4, true>(a);
    else launch_tiles<4, false>(a);
  } else {
    if (nt) launch_tiles<8, true>(a);
    else launch_tiles<8, false>(a);
  }
  return y;
}
