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
// and k-steps past a wave's chunk are never loaded ("Masked lanes" in
// decode_linear_common.h, which also holds the 16-byte load, the per-element
// epilogue and the binding's checks, shared with decode_linear.hip).
//
// decode_linear_fp8_ln_kernel further down is the same linear over LayerNorm(x): statistics
// per workgroup, x fragments normalised in registers, one launch.
#include "decode_linear_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int int4v;

constexpr int KSTEP = 64;    // k per 16-byte load of codes: two MFMAs

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

  // setup and reduction: same text in both kernels, see the header for why
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
  // Fragments of masked lanes are never loaded and need no zero ("Masked
  // lanes" in decode_linear_common.h).
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
            if (u < nb)
              a[t][u] = load16<int4v, NT>(wp[t] + off + u * KSTEP);
        }
      }
      if (x_ok) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u < nb) {
            b[u][0] = load16<int4v, false>(xp + off + u * KSTEP);
            b[u][1] = load16<int4v, false>(xp + off + u * KSTEP + 8);
          }
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u < nb) {
          if (w_ok[0])
            a[0][u] = load16<int4v, NT>(wp[0] + off + u * KSTEP);
          if (x_ok) {
            b[u][0] = load16<int4v, false>(xp + off + u * KSTEP);
            b[u][1] = load16<int4v, false>(xp + off + u * KSTEP + 8);
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
      finish_element<true>(v, m, n, N, w_scale, bias, res, y, gelu);
    }
  }
}

// The same linear over LN(x) = bf16((x - mu) * rstd * g + b): "LayerNorm
// prologue" in decode_linear_common.h. A kernel of its own, so that the one
// above keeps its ISA; setup, load order and reduction are its text once
// more. Both x loads of a k-step are normalised between their wait and
// their MFMAs, g and b of their k come from LDS. Dynamic LDS: 4*K bytes.
template <int NW, int TILES, bool NT>
__global__ __launch_bounds__(NW * WAVE) NO_PK_F32 void decode_linear_fp8_ln_kernel(
    const short* __restrict__ x,          // [M, K] bf16, not normalised
    const unsigned char* __restrict__ w,  // [N, K] e4m3fn
    const float* __restrict__ w_scale,    // [N]
    const short* __restrict__ bias,       // [N] or null
    const short* __restrict__ res,        // [M, N] or null
    const short* __restrict__ ln_w,       // [K]
    const short* __restrict__ ln_b,       // [K]
    short* __restrict__ y,                // [M, N]
    int M, int N, int K, int rows, int gelu, float eps) {
  constexpr int U = Flight<TILES>::U;
  __shared__ float s_part[NW][TILES * TILE * TILE];
  __shared__ float s_stat[NW][2 * TILE];
  __shared__ float s_dev[NW][TILE];
  extern __shared__ __attribute__((aligned(16))) short s_gb[];  // g, b

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int r = lane & 15;              // W row in the tile / x row
  const int kg = (lane >> 4) * 16;      // k offset inside a k-step
  const int n0 = blockIdx.x * rows;
  const int tile_rows = min(rows, TILE);

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

  const int steps = K / KSTEP;
  const int s_beg = (int)(((long)steps * wid) / NW);
  const int s_end = (int)(((long)steps * (wid + 1)) / NW);

  mfma_f32x4 acc[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc[t] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
  const int4v zero4 = {0, 0, 0, 0};
  int4v a[TILES][U], b[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    b[u][0] = b[u][1] = zero4;
#pragma unroll
    for (int t = 0; t < TILES; ++t) a[t][u] = zero4;
  }
  // Statistics first, then the stream: issuing the first batch of codes
  // under the statistics pass (as decode_linear.hip does) was measured
  // slower here, 200 VGPRs in the one-tile instances and the one-tile load
  // order lost for that batch.
  float mu, rstd;
  ln_prologue<int4v, NW, KSTEP, 2>(xp, x_ok, s_beg, s_end, K, ln_w, ln_b, eps,
                                   s_gb, s_stat, s_dev, tid, wid, r, mu,
                                   rstd, [] {});

  // the measured load order of the kernel above
  for (int s = s_beg; s < s_end; s += U) {
    const size_t off = (size_t)s * KSTEP;
    const int nb = s_end - s;
    if constexpr (TILES > 1) {
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        if (w_ok[t]) {
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (u < nb)
              a[t][u] = load16<int4v, NT>(wp[t] + off + u * KSTEP);
        }
      }
      if (x_ok) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u < nb) {
            b[u][0] = load16<int4v, false>(xp + off + u * KSTEP);
            b[u][1] = load16<int4v, false>(xp + off + u * KSTEP + 8);
          }
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u < nb) {
          if (w_ok[0])
            a[0][u] = load16<int4v, NT>(wp[0] + off + u * KSTEP);
          if (x_ok) {
            b[u][0] = load16<int4v, false>(xp + off + u * KSTEP);
            b[u][1] = load16<int4v, false>(xp + off + u * KSTEP + 8);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < nb) {
        // a masked lane's column (m >= M) is finite garbage, never stored
        const size_t k = off + u * KSTEP + kg;
        const mfma_bf16x8 h0 = ln_frag(b[u][0], s_gb, K, k, mu, rstd);
        const mfma_bf16x8 h1 = ln_frag(b[u][1], s_gb, K, k + 8, mu, rstd);
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              decode8(a[t][u][0], a[t][u][1]), h0, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              decode8(a[t][u][2], a[t][u][3]), h1, acc[t], 0, 0, 0);
        }
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
      finish_element<true>(v, m, n, N, w_scale, bias, res, y, gelu);
    }
  }
}

template <int NW, int TILES, bool NT>
void launch(const Args<unsigned char>& a) {
  auto stream = at::hip::getCurrentHIPStream();
  const int grid = (a.N + a.rows - 1) / a.rows;
  if (a.ln_w) {
    hipLaunchKernelGGL((decode_linear_fp8_ln_kernel<NW, TILES, NT>),
                       dim3(grid), dim3(NW * WAVE), 4 * (size_t)a.K, stream,
                       a.x, a.w, a.w_scale, a.bias, a.res, a.ln_w, a.ln_b,
                       a.y, a.M, a.N, a.K, a.rows, a.gelu, a.ln_eps);
    return;
  }
  hipLaunchKernelGGL((decode_linear_fp8_kernel<NW, TILES, NT>), dim3(grid),
                     dim3(NW * WAVE), 0, stream, a.x, a.w, a.w_scale, a.bias,
                     a.res, a.y, a.M, a.N, a.K, a.rows, a.gelu);
}

template <int NW, bool NT>
void launch_tiles(const Args<unsigned char>& a) {
  if (a.rows == 64) launch<NW, 4, NT>(a);
  else if (a.rows == 32) launch<NW, 2, NT>(a);
  else launch<NW, 1, NT>(a);
}

}  // namespace

// rows / waves / nontemporal: 0 / 0 / -1 choose automatically; other values
// are the benchmark's sweep (rows 8, 16, 32 or 64, waves 4 or 8, nt 0 or 1).
// ln_weight and ln_bias (both or neither) put LayerNorm(x, eps) in front.
torch::Tensor decode_linear_fp8(torch::Tensor x, torch::Tensor wq,
                                torch::Tensor w_scale,
                                c10::optional<torch::Tensor> bias,
                                c10::optional<torch::Tensor> residual,
                                const std::string& act, long rows, long waves,
                                long nontemporal,
                                c10::optional<torch::Tensor> ln_weight,
                                c10::optional<torch::Tensor> ln_bias,
                                double ln_eps) {
  const Checked c = check_decode_linear(
      "decode_linear_fp8", "wq", x, wq, torch::kFloat8_e4m3fn, KSTEP, bias,
      residual, act, rows, {8, 16, 32, 64}, waves, nontemporal, ln_weight,
      ln_bias, ln_eps);
  const long M = c.M, N = c.N;
  TORCH_CHECK(w_scale.defined() && w_scale.device() == x.device() &&
                  w_scale.scalar_type() == torch::kFloat32 &&
                  w_scale.is_contiguous() && w_scale.dim() == 1 &&
                  w_scale.size(0) == N,
              "decode_linear_fp8: w_scale must be a contiguous float32 [", N,
              "] on ", x.device());

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
  const Args<unsigned char> a{
      (const short*)x.data_ptr(), (const unsigned char*)wq.data_ptr(),
      (const float*)w_scale.data_ptr(), c.bias, c.res, (short*)y.data_ptr(),
      (int)M, (int)N, (int)c.K, (int)rows, act == "gelu", c.ln_w, c.ln_b,
      (float)ln_eps};
  if (waves == 4) {
    if (nt) launch_tiles<4, true>(a);
    else launch_tiles<4, false>(a);
  } else {
    if (nt) launch_tiles<8, true>(a);
    else launch_tiles<8, false>(a);
  }
  return y;
}
