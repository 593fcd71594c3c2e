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
// chunk are never loaded ("Masked lanes" in decode_linear_common.h, which
// also holds the 16-byte load, the per-element epilogue and the binding's
// checks, shared with decode_linear_fp8.hip).
//
// decode_linear_ln_kernel further down is the same linear over LayerNorm(x): statistics
// per workgroup, x fragments normalised in registers, one launch.
#include "decode_linear_common.h"

namespace {

constexpr int KSTEP = 32;    // k per MFMA
constexpr int U = 8;         // k-steps in flight: 16-byte loads per operand

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

  // setup and reduction: same text in both kernels, see the header for why
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
  // Fragments of masked lanes are never loaded and need no zero ("Masked
  // lanes" in decode_linear_common.h).
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
            a[t][u] = load16<short8v, NT>(wp[t] + off + u * KSTEP);
        }
      }
      if (x_ok) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          b[u] = load16<short8v, false>(xp + off + u * KSTEP);
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
            if (w_ok[t])
              a[t][u] = load16<short8v, NT>(wp[t] + off + u * KSTEP);
          if (x_ok) b[u] = load16<short8v, false>(xp + off + u * KSTEP);
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
      finish_element<false>(v, m, n, N, nullptr, bias, res, y, gelu);
    }
  }
}

// The same linear over LN(x) = bf16((x - mu) * rstd * g + b): "LayerNorm
// prologue" in decode_linear_common.h. A kernel of its own, so that the one
// above keeps its ISA; setup and reduction are its text once more. The main
// loop is the one-path form of decode_linear_fp8.hip (u < nb is a scalar
// branch): every x fragment is normalised between its wait and its MFMAs,
// g and b of its k come from LDS. The first batch of W loads is issued
// under the statistics pass. Dynamic LDS: 4*K bytes.
template <int NW, int TILES, bool NT>
__global__ __launch_bounds__(NW * WAVE) NO_PK_F32 void decode_linear_ln_kernel(
    const short* __restrict__ x,        // [M, K] bf16, not normalised
    const short* __restrict__ w,        // [N, K] bf16
    const short* __restrict__ bias,     // [N] or null
    const short* __restrict__ res,      // [M, N] or null
    const short* __restrict__ ln_w,     // [K]
    const short* __restrict__ ln_b,     // [K]
    short* __restrict__ y,              // [M, N]
    int M, int N, int K, int rows, int gelu, float eps) {
  __shared__ float s_part[NW][TILES * TILE * TILE];
  __shared__ float s_stat[NW][2 * TILE];
  __shared__ float s_dev[NW][TILE];
  extern __shared__ __attribute__((aligned(16))) short s_gb[];  // g, b

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int r = lane & 15;              // W row in the tile / x row
  const int kg = (lane >> 4) * 8;       // k offset inside a k-step
  const int n0 = blockIdx.x * rows;
  const int tile_rows = min(rows, TILE);

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

  const int steps = K / KSTEP;
  const int s_beg = (int)(((long)steps * wid) / NW);
  const int s_end = (int)(((long)steps * (wid + 1)) / NW);

  mfma_f32x4 acc[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc[t] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
  const short8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  short8v a[TILES][U], b[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    b[u] = zero8;
#pragma unroll
    for (int t = 0; t < TILES; ++t) a[t][u] = zero8;
  }
  // the W loads of the batch of k-steps that starts at s
  auto load_w = [&](int s) __attribute__((always_inline)) {
    const size_t off = (size_t)s * KSTEP;
    const int nb = s_end - s;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      if (w_ok[t]) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (u < nb) a[t][u] = load16<short8v, NT>(wp[t] + off + u * KSTEP);
      }
    }
  };

  // the first batch of W is in flight under the statistics
  float mu, rstd;
  ln_prologue<short8v, NW, KSTEP, 1>(xp, x_ok, s_beg, s_end, K, ln_w, ln_b,
                                     eps, s_gb, s_stat, s_dev, tid, wid, r,
                                     mu, rstd, [&]() __attribute__((always_inline)) { load_w(s_beg); });

  for (int s = s_beg; s < s_end; s += U) {
    const size_t off = (size_t)s * KSTEP;
    const int nb = s_end - s;
    if (s != s_beg) load_w(s);
    if (x_ok) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (u < nb) b[u] = load16<short8v, false>(xp + off + u * KSTEP);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < nb) {
        // a masked lane's column (m >= M) is finite garbage, never stored
        const mfma_bf16x8 h =
            ln_frag(b[u], s_gb, K, off + u * KSTEP + kg, mu, rstd);
#pragma unroll
        for (int t = 0; t < TILES; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              as_frag(a[t][u]), h, acc[t], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int t = 0; t < TILES; ++t)
    *reinterpret_cast<float4v*>(
        &s_part[wid][t * TILE * TILE + r * TILE + (lane >> 4) * 4]) = acc[t];
  __syncthreads();

  for (int e = tid; e < TILES * TILE * TILE; e += NW * WAVE) {
    const int m = (e >> 4) & 15;
    const int nt = e & 15;
    const int n = n0 + (e >> 8) * TILE + nt;
    if (m < M && nt < tile_rows && n < N) {
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < NW; ++i) v += s_part[i][e];
      finish_element<false>(v, m, n, N, nullptr, bias, res, y, gelu);
    }
  }
}

template <int NW, int TILES, bool NT>
void launch(const Args<short>& a) {
  auto stream = at::hip::getCurrentHIPStream();
  const int grid = (a.N + a.rows - 1) / a.rows;
  if (a.ln_w) {
    hipLaunchKernelGGL((decode_linear_ln_kernel<NW, TILES, NT>), dim3(grid),
                       dim3(NW * WAVE), 4 * (size_t)a.K, stream, a.x, a.w,
                       a.bias, a.res, a.ln_w, a.ln_b, a.y, a.M, a.N, a.K,
                       a.rows, a.gelu, a.ln_eps);
    return;
  }
  hipLaunchKernelGGL((decode_linear_kernel<NW, TILES, NT>), dim3(grid),
                     dim3(NW * WAVE), 0, stream, a.x, a.w, a.bias, a.res, a.y,
                     a.M, a.N, a.K, a.rows, a.gelu);
}

template <int NW>
void launch_tiles(const Args<short>& a, bool nt) {
  if (a.rows == 32) {
    if (nt) launch<NW, 2, true>(a);
    else launch<NW, 2, false>(a);
  } else {
    if (nt) launch<NW, 1, true>(a);
    else launch<NW, 1, false>(a);
  }
}

}  // namespace

// rows / waves / nontemporal: 0 / 0 / -1 choose automatically; other values
// are the benchmark's sweep (rows 8, 16 or 32, waves 4 or 8, nt 0 or 1).
// ln_weight and ln_bias (both or neither) put LayerNorm(x, eps) in front.
torch::Tensor decode_linear(torch::Tensor x, torch::Tensor weight,
                            c10::optional<torch::Tensor> bias,
                            c10::optional<torch::Tensor> residual,
                            const std::string& act, long rows, long waves,
                            long nontemporal,
                            c10::optional<torch::Tensor> ln_weight,
                            c10::optional<torch::Tensor> ln_bias,
                            double ln_eps) {
  const Checked c = check_decode_linear(
      "decode_linear", "weight", x, weight, torch::kBFloat16, KSTEP, bias,
      residual, act, rows, {8, 16, 32}, waves, nontemporal, ln_weight,
      ln_bias, ln_eps);
  const long M = c.M, N = c.N, K = c.K;

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
  const Args<short> a{(const short*)x.data_ptr(),
                      (const short*)weight.data_ptr(), nullptr, c.bias, c.res,
                      (short*)y.data_ptr(), (int)M, (int)N, (int)K, (int)rows,
                      act == "gelu", c.ln_w, c.ln_b, (float)ln_eps};
  if (waves == 4)
    launch_tiles<4>(a, nt);
  else
    launch_tiles<8>(a, nt);
  return y;
}
