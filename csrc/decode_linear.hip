// Weight-streaming linear for the decode step (1 <= M <= 16 rows), gfx950.
//
//   y[M,N] = act(x[M,K] . W[N,K]^T + bias[N]) + residual[M,N]      (bf16)
//
// At M <= 16 the op is a read of W (N*K*2 bytes, ~M flop/byte): memory
// bound. W goes from global memory straight to VGPRs in 16-byte loads and
// is read exactly once; there is no LDS staging of W.
//
// One v_mfma_f32_16x16x32_bf16 per 16 rows x 32 k of W: the W tile is the A
// operand, x^T the B operand, so C[n][m] holds up to 16 batch rows and the
// columns m >= M are zero. With W stored [N][K] (the nn.Linear layout) a
// lane's A fragment (row lane&15, k (lane>>4)*8 .. +8) is one 16-byte load,
// and so is its B fragment from x[M][K]; no repacking.
//
// Workgroup = NW waves on `rows` weight rows (8: half an MFMA tile, 16: one
// tile, 32: two tiles that share the x fragments); the k-steps are dealt to
// the waves in contiguous chunks. Partial
// tiles are summed through LDS in wave order (fixed, so the result is
// bitwise reproducible) and the epilogue (bias, tanh-GELU, residual, one
// rounding to bf16) runs in the same launch. No counters, flags or atomics.
//
// Rows of W at index >= N, rows of x at index >= M and k-steps past a wave's
// chunk are never loaded: the load sits behind a predicate (exec-masked,
// as in decode_attention.hip), and nothing such a lane holds reaches a
// stored element.
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>
#include <string>

namespace {

constexpr int TILE = 16;     // MFMA rows (n) and columns (m)
constexpr int KSTEP = 32;    // k per MFMA
constexpr int U = 8;         // k-steps in flight: 16-byte loads per operand
constexpr float GELU_K = 0.7978845608028654f;  // sqrt(2/pi)

// the tanh-GELU of elementwise.hip (bias_gelu), same formula and exp unit
DEV_INLINE float gelu_tanh(float x) {
  const float t =
      1.f - 2.f / (__expf(2.f * GELU_K * (x + 0.044715f * x * x * x)) + 1.f);
  return 0.5f * x * (1.f + t);
}

template <bool NT>
DEV_INLINE short8v load16(const short* p) {
  if constexpr (NT)
    return __builtin_nontemporal_load(reinterpret_cast<const short8v*>(p));
  else
    return *reinterpret_cast<const short8v*>(p);
}

DEV_INLINE mfma_bf16x8 as_frag(const short8v& v) {
  union { short8v s; mfma_bf16x8 f; } u;
  u.s = v;
  return u.f;
}

// grid ceil(N / rows), NW*64 threads; rows = 16*TILES, or 8 with TILES = 1
// (the upper half of the MFMA tile masked). The TILES tiles of a workgroup
// share every x fragment.
template <int NW, int TILES, bool NT>
__global__ __launch_bounds__(NW * WAVE) void decode_linear_kernel(
    const short* __restrict__ x,        // [M, K] bf16
    const short* __restrict__ w,        // [N, K] bf16
    const short* __restrict__ bias,     // [N] or null
    const short* __restrict__ res,      // [M, N] or null
    short* __restrict__ y,              // [M, N]
    int M, int N, int K, int rows, int gelu) {
  __shared__ float s_part[NW][TILES * TILE * TILE];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  // wave-uniform: keeps the chunk bounds and their branches scalar
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int r = lane & 15;              // W row in the tile / x row
  const int kg = (lane >> 4) * 8;       // k offset inside a k-step
  const int n0 = blockIdx.x * rows;
  const int tile_rows = min(rows, TILE);

  // masked lanes keep a valid base (row 0) and never dereference it
  bool w_ok[TILES];
  const short* wp[TILES];
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
  const short8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  short8v a[TILES][U], b[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    b[u] = zero8;
#pragma unroll
    for (int t = 0; t < TILES; ++t) a[t][u] = zero8;
  }
  // wave-uniform trip count and batch size
  for (int s = s_beg; s < s_end; s += U) {
    const size_t off = (size_t)s * KSTEP;
    const int nb = s_end - s;
    if (nb >= U) {
      // full batch: one exec mask per operand, all loads issued back to back
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        if (w_ok[t]) {
#pragma unroll
          for (int u = 0; u < U; ++u)
            a[t][u] = load16<NT>(wp[t] + off + u * KSTEP);
        }
      }
      if (x_ok) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          b[u] = load16<false>(xp + off + u * KSTEP);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int t = 0; t < TILES; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              as_frag(a[t][u]), as_frag(b[u]), acc[t], 0, 0, 0);
      }
    } else {
      // last batch of the chunk: k-steps past it are neither loaded nor
      // multiplied
#pragma unroll
      for (int u = 0; u < U - 1; ++u) {
        if (u < nb) {
#pragma unroll
          for (int t = 0; t < TILES; ++t)
            if (w_ok[t]) a[t][u] = load16<NT>(wp[t] + off + u * KSTEP);
          if (x_ok) b[u] = load16<false>(xp + off + u * KSTEP);
        }
      }
#pragma unroll
      for (int u = 0; u < U - 1; ++u) {
        if (u < nb) {
#pragma unroll
          for (int t = 0; t < TILES; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                as_frag(a[t][u]), as_frag(b[u]), acc[t], 0, 0, 0);
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
      if (bias) v += bf_raw2f((unsigned short)bias[n]);
      if (gelu) v = gelu_tanh(v);
      const size_t o = (size_t)m * N + n;
      if (res) v += bf_raw2f((unsigned short)res[o]);
      y[o] = (short)f2bf_raw(v);
    }
  }
}

struct Args {
  const short *x, *w, *bias, *res;
  short* y;
  int M, N, K, rows, gelu;
};

template <int NW, int TILES, bool NT>
void launch(const Args& a) {
  auto stream = at::hip::getCurrentHIPStream();
  const int grid = (a.N + a.rows - 1) / a.rows;
  hipLaunchKernelGGL((decode_linear_kernel<NW, TILES, NT>), dim3(grid),
                     dim3(NW * WAVE), 0, stream, a.x, a.w, a.bias, a.res, a.y,
                     a.M, a.N, a.K, a.rows, a.gelu);
}

template <int NW>
void launch_tiles(const Args& a, bool nt) {
  if (a.rows == 32) {
    if (nt) launch<NW, 2, true>(a);
    else launch<NW, 2, false>(a);
  } else {
    if (nt) launch<NW, 1, true>(a);
    else launch<NW, 1, false>(a);
  }
}

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

}  // namespace

// rows / waves / nontemporal: 0 / 0 / -1 choose automatically; other values
// are the benchmark's sweep (rows 8, 16 or 32, waves 4 or 8, nt 0 or 1).
torch::Tensor decode_linear(torch::Tensor x, torch::Tensor weight,
                            c10::optional<torch::Tensor> bias,
                            c10::optional<torch::Tensor> residual,
                            const std::string& act, long rows, long waves,
                            long nontemporal) {
  TORCH_CHECK(x.defined() && weight.defined(),
              "decode_linear: x and weight must be defined");
  TORCH_CHECK(x.is_cuda() && weight.is_cuda(),
              "decode_linear: x and weight must be GPU tensors");
  TORCH_CHECK(weight.device() == x.device(),
              "decode_linear: weight is on ", weight.device(), ", expected ",
              x.device());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
                  weight.scalar_type() == torch::kBFloat16,
              "decode_linear: x and weight must be bfloat16, got ",
              x.scalar_type(), " and ", weight.scalar_type());
  TORCH_CHECK(x.dim() == 2 && weight.dim() == 2,
              "decode_linear: x must be [M, K] and weight [N, K]");
  TORCH_CHECK(x.is_contiguous(), "decode_linear: x must be contiguous");
  TORCH_CHECK(weight.is_contiguous(),
              "decode_linear: weight must be contiguous");
  const long M = x.size(0), K = x.size(1), N = weight.size(0);
  TORCH_CHECK(weight.size(1) == K, "decode_linear: weight must be [N, ", K,
              "], got [", N, ", ", weight.size(1), "]");
  TORCH_CHECK(M >= 1 && M <= TILE, "decode_linear: M must be in [1, 16], got ",
              M);
  TORCH_CHECK(K >= KSTEP && K % KSTEP == 0,
              "decode_linear: K must be a positive multiple of 32, got ", K);
  TORCH_CHECK(N >= 8 && N % 8 == 0,
              "decode_linear: N must be a positive multiple of 8, got ", N);
  TORCH_CHECK(N * K < (1L << 40) && N < (1L << 30) && K < (1L << 30),
              "decode_linear: bad weight extent");
  TORCH_CHECK(aligned16(x) && aligned16(weight),
              "decode_linear: x and weight must be 16-byte aligned");
  TORCH_CHECK(act == "none" || act == "gelu",
              "decode_linear: act must be 'none' or 'gelu', got '", act, "'");
  const short* bp = nullptr;
  const short* rp = nullptr;
  if (bias.has_value() && bias->defined()) {
    const torch::Tensor& b = *bias;
    TORCH_CHECK(b.scalar_type() == torch::kBFloat16 &&
                    b.device() == x.device() && b.is_contiguous() &&
                    b.dim() == 1 && b.size(0) == N,
                "decode_linear: bias must be a contiguous bfloat16 [", N,
                "] on ", x.device());
    bp = (const short*)b.data_ptr();
  }
  if (residual.has_value() && residual->defined()) {
    const torch::Tensor& rs = *residual;
    TORCH_CHECK(rs.scalar_type() == torch::kBFloat16 &&
                    rs.device() == x.device() && rs.is_contiguous() &&
                    rs.dim() == 2 && rs.size(0) == M && rs.size(1) == N,
                "decode_linear: residual must be a contiguous bfloat16 [", M,
                ", ", N, "] on ", x.device());
    rp = (const short*)rs.data_ptr();
  }
  TORCH_CHECK(rows == 0 || rows == 8 || rows == 16 || rows == 32,
              "decode_linear: rows must be 0 (auto), 8, 16 or 32");
  TORCH_CHECK(waves == 0 || waves == 4 || waves == 8,
              "decode_linear: waves must be 0 (auto), 4 or 8");
  TORCH_CHECK(nontemporal >= -1 && nontemporal <= 1,
              "decode_linear: nontemporal must be -1 (auto), 0 or 1");

  // Measured choice (benchmarks/bench_decode_linear.py --sweep, KERNELS.md):
  // the most rows per workgroup that still give 3/4 of the CUs a workgroup,
  // since two tiles share the x fragments and a full tile uses every lane;
  // half tiles (the upper 8 MFMA rows masked) below that. Half tiles carry
  // half the loads per wave and want 8 waves, the others 4.
  if (rows == 0) {
    const long cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    rows = 8;
    for (long cand : {32L, 16L})
      if ((N + cand - 1) / cand >= (3 * cus) / 4) { rows = cand; break; }
  }
  if (waves == 0) waves = rows == 8 ? 8 : 4;
  // non-temporal W loads: faster up to the layer-sized weights, slower on
  // the vocabulary-sized one
  const bool nt = nontemporal < 0 ? N * K * 2 < (128L << 20)
                                  : nontemporal != 0;

  auto y = torch::empty({M, N}, x.options());
  const Args a{(const short*)x.data_ptr(), (const short*)weight.data_ptr(),
               bp, rp, (short*)y.data_ptr(), (int)M, (int)N, (int)K,
               (int)rows, act == "gelu"};
  if (waves == 4)
    launch_tiles<4>(a, nt);
  else
    launch_tiles<8>(a, nt);
  return y;
}
