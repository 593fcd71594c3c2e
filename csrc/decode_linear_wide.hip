// Weight-streaming linear for decode batches of 17 to 64 rows, gfx950.
//
//   y[M,N] = act((x[M,K] . W[N,K]^T) (* w_scale[N]) + bias[N]) + residual[M,N]
//
// x, bias, residual and y are bf16. W is bf16 [N][K], or float8_e4m3fn codes
// [N][K] with one fp32 scale per output row (ref.quantize_weight_rows): one
// kernel template over the weight type. At M <= 64 the op is still a read of
// W (M flop per byte with bf16 weights, 2M with codes), so the structure is
// the one of decode_linear.hip and decode_linear_fp8.hip: W goes from global
// memory straight to VGPRs in 16-byte loads of the stored layout and is read
// once, the waves of a workgroup split K in contiguous chunks, partial tiles
// are summed through LDS in wave order (bitwise reproducible) and the
// epilogue runs in the same launch. No counters, flags or atomics, no
// workspace.
//
// Column tiles. One v_mfma_f32_16x16x32_bf16 holds 16 batch rows, so the
// batch is MT = ceil(M / 16) column tiles (2, 3 or 4, a template parameter)
// and a wave keeps TILES x MT accumulators. One A fragment (16 rows x 32 k of
// W) feeds MT MFMAs: a W load is used MT times as often as in the sibling
// kernels and an fp8 decode is paid once per MT MFMAs. Column tile j holds
// rows 16 j .. 16 j + 15 of x; only the last one can be partial.
//
// Fragments. bf16: a k-step is 32 wide, a lane owns row lane&15 and k
// (lane>>4)*8 .. +8 of it, one 16-byte load per W tile and one per column
// tile of x. fp8: a 16-byte load is 16 codes, so a k-step is 64 wide, a lane
// owns k (lane>>4)*16 .. +16, codes 0-7 and 8-15 are decoded (exactly, see
// decode8) into the A fragments of two MFMAs and a column tile of x is two
// 16-byte loads. The MFMA sums over (lane group, element) pairs, so any k
// assignment that A and B share is a valid contraction.
//
// Registers are the design (KERNELS.md has the table): a k-step is
// L = TILES + XL * MT 16-byte loads per lane (XL = 1 or 2 x loads per column
// tile), the accumulators take 4 * TILES * MT, so the number of k-steps in
// flight shrinks as L grows: Flight<L>::U.
//
// The sum over the waves runs column tile by column tile through ONE buffer
// of NW * TILES KiB: with all MT tiles at once, 8 waves x 4 row tiles x 4
// column tiles would be 128 KiB. The order is fixed: wave 0, 1, ...
//
// Rows of W and entries of w_scale at index >= N, rows of x at index >= M
// and k-steps past a wave's chunk are never loaded, and the fragments of
// masked lanes need no zero ("Masked lanes" in decode_linear_common.h, which
// also holds the 16-byte load, the per-element epilogue and the checks).
#include "decode_linear_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int int4v;

// What the weight type decides: the k-step and the 16-byte loads of x per
// column tile and k-step.
template <typename WT> struct Weight;
template <> struct Weight<short> {
  static constexpr int KSTEP = 32, XL = 1;
  static constexpr bool SCALED = false;
};
template <> struct Weight<unsigned char> {
  static constexpr int KSTEP = 64, XL = 2;
  static constexpr bool SCALED = true;
};

// decode8 of decode_linear_fp8.hip: 8 e4m3 codes (two words) -> 8 bf16,
// exact: the high halves of the fp32 pairs v_cvt_pk_f32_fp8 gives.
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

// k-steps in flight per wave for L 16-byte loads per lane and k-step: the
// most of 8, 4, 2 that keeps the fragments within 128 VGPRs (4 * L * U).
template <int L>
struct Flight { static constexpr int U = L <= 4 ? 8 : L <= 8 ? 4 : 2; };

// grid ceil(N / rows), NW*64 threads; rows = 16*TILES, or 8 with TILES = 1
// (the upper half of the MFMA tile masked). 16*(MT-1) < M <= 16*MT.
template <typename WT, int NW, int TILES, int MT, bool NT>
__global__ __launch_bounds__(NW * WAVE) NO_PK_F32 void decode_linear_wide_kernel(
    const short* __restrict__ x,        // [M, K] bf16
    const WT* __restrict__ w,           // [N, K] bf16 or e4m3fn
    const float* __restrict__ w_scale,  // [N], fp8 only
    const short* __restrict__ bias,     // [N] or null
    const short* __restrict__ res,      // [M, N] or null
    short* __restrict__ y,              // [M, N]
    int M, int N, int K, int rows, int gelu) {
  constexpr int KSTEP = Weight<WT>::KSTEP, XL = Weight<WT>::XL;
  constexpr int U = Flight<TILES + XL * MT>::U;
  __shared__ float s_part[NW][TILES * TILE * TILE];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  // wave-uniform: keeps the chunk bounds and their branches scalar
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int r = lane & 15;                   // W row in the tile / x row
  const int kg = (lane >> 4) * (KSTEP / 4);  // k offset inside a k-step
  const int n0 = blockIdx.x * rows;
  const int tile_rows = min(rows, TILE);

  // masked lanes keep a valid base (row 0) and never dereference it
  bool w_ok[TILES];
  const WT* wp[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const int row = n0 + t * TILE + r;
    w_ok[t] = (r < tile_rows) && (row < N);
    wp[t] = w + (size_t)(w_ok[t] ? row : 0) * K + kg;
  }
  // column tiles before the last are full
  const bool x_last = (MT - 1) * TILE + r < M;
  const short* xp[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const bool ok = j < MT - 1 || x_last;
    xp[j] = x + (size_t)(ok ? j * TILE + r : 0) * K + kg;
  }

  // this wave's k-steps [s_beg, s_end): contiguous, sizes differ by <= 1
  const int steps = K / KSTEP;
  const int s_beg = (int)(((long)steps * wid) / NW);
  const int s_end = (int)(((long)steps * (wid + 1)) / NW);

  mfma_f32x4 acc[TILES][MT];
#pragma unroll
  for (int t = 0; t < TILES; ++t)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[t][j] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
  const int4v zero4 = {0, 0, 0, 0};
  int4v a[TILES][U], b[MT][U][XL];
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) a[t][u] = zero4;
#pragma unroll
    for (int j = 0; j < MT; ++j)
#pragma unroll
      for (int l = 0; l < XL; ++l) b[j][u][l] = zero4;
  }
  // Wave-uniform trip count and batch size, one code path for full and
  // partial batches (u < nb is a scalar branch). W first, tile by tile (the
  // loads of one row's consecutive bytes adjacent), then x column tile by
  // column tile: loads return in issue order, so the HBM stream is requested
  // before the L2 one.
  for (int s = s_beg; s < s_end; s += U) {
    const size_t off = (size_t)s * KSTEP;
    const int nb = s_end - s;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      if (w_ok[t]) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (u < nb) a[t][u] = load16<int4v, NT>(wp[t] + off + u * KSTEP);
      }
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      if (j < MT - 1 || x_last) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u < nb) {
#pragma unroll
            for (int l = 0; l < XL; ++l)
              b[j][u][l] =
                  load16<int4v, false>(xp[j] + off + u * KSTEP + 8 * l);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < nb) {
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
          if constexpr (Weight<WT>::SCALED) {
            const mfma_bf16x8 a0 = decode8(a[t][u][0], a[t][u][1]);
            const mfma_bf16x8 a1 = decode8(a[t][u][2], a[t][u][3]);
#pragma unroll
            for (int j = 0; j < MT; ++j) {
              acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a0, as_frag(b[j][u][0]), acc[t][j], 0, 0, 0);
              acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a1, as_frag(b[j][u][XL - 1]), acc[t][j], 0, 0, 0);
            }
          } else {
#pragma unroll
            for (int j = 0; j < MT; ++j)
              acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  as_frag(a[t][u]), as_frag(b[j][u][0]), acc[t][j], 0, 0, 0);
          }
        }
      }
    }
  }

  // One round per column tile j through the same buffer.
  // C[n][m]: m = lane & 15, n = (lane >> 4) * 4 + i -> s_part[w][t][m*16 + n]
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    if (j) __syncthreads();  // round j - 1 has been read
#pragma unroll
    for (int t = 0; t < TILES; ++t)
      *reinterpret_cast<float4v*>(
          &s_part[wid][t * TILE * TILE + r * TILE + (lane >> 4) * 4]) =
          acc[t][j];
    __syncthreads();
    // element e = (tile t, m, n in tile): summed over the waves in wave order
    for (int e = tid; e < TILES * TILE * TILE; e += NW * WAVE) {
      const int m = j * TILE + ((e >> 4) & 15);
      const int nt = e & 15;
      const int n = n0 + (e >> 8) * TILE + nt;
      if (m < M && nt < tile_rows && n < N) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < NW; ++i) v += s_part[i][e];
        finish_element<Weight<WT>::SCALED>(v, m, n, N, w_scale, bias, res, y,
                                           gelu);
      }
    }
  }
}

template <typename WT, int NW, int TILES, int MT>
void launch(const Args<WT>& a, bool nt) {
  auto stream = at::hip::getCurrentHIPStream();
  const int grid = (a.N + a.rows - 1) / a.rows;
  if (nt)
    hipLaunchKernelGGL((decode_linear_wide_kernel<WT, NW, TILES, MT, true>),
                       dim3(grid), dim3(NW * WAVE), 0, stream, a.x, a.w,
                       a.w_scale, a.bias, a.res, a.y, a.M, a.N, a.K, a.rows,
                       a.gelu);
  else
    hipLaunchKernelGGL((decode_linear_wide_kernel<WT, NW, TILES, MT, false>),
                       dim3(grid), dim3(NW * WAVE), 0, stream, a.x, a.w,
                       a.w_scale, a.bias, a.res, a.y, a.M, a.N, a.K, a.rows,
                       a.gelu);
}

template <typename WT, int NW, int TILES>
void launch_cols(const Args<WT>& a, bool nt) {
  const int mt = (a.M + TILE - 1) / TILE;
  if (mt == 2) launch<WT, NW, TILES, 2>(a, nt);
  else if (mt == 3) launch<WT, NW, TILES, 3>(a, nt);
  else launch<WT, NW, TILES, 4>(a, nt);
}

template <typename WT>
void launch_wide(const Args<WT>& a, long waves, bool nt) {
  if (waves == 4) {
    if (a.rows == 64) launch_cols<WT, 4, 4>(a, nt);
    else if (a.rows == 32) launch_cols<WT, 4, 2>(a, nt);
    else launch_cols<WT, 4, 1>(a, nt);
  } else {
    if (a.rows == 64) launch_cols<WT, 8, 4>(a, nt);
    else if (a.rows == 32) launch_cols<WT, 8, 2>(a, nt);
    else launch_cols<WT, 8, 1>(a, nt);
  }
}

}  // namespace

// weight: bf16 [N, K], or float8_e4m3fn codes [N, K] with w_scale fp32 [N].
// rows / waves / nontemporal: 0 / 0 / -1 choose automatically; other values
// are the benchmark's sweep (rows 8, 16, 32 or 64, waves 4 or 8, nt 0 or 1).
torch::Tensor decode_linear_wide(torch::Tensor x, torch::Tensor weight,
                                 c10::optional<torch::Tensor> w_scale,
                                 c10::optional<torch::Tensor> bias,
                                 c10::optional<torch::Tensor> residual,
                                 const std::string& act, long rows, long waves,
                                 long nontemporal) {
  const char* op = "decode_linear_wide";
  TORCH_CHECK(weight.defined(), op, ": x and weight must be defined");
  const bool fp8 = weight.scalar_type() == torch::kFloat8_e4m3fn;
  const Checked c = check_decode_linear(
      op, "weight", x, weight, fp8 ? torch::kFloat8_e4m3fn : torch::kBFloat16,
      fp8 ? Weight<unsigned char>::KSTEP : Weight<short>::KSTEP, bias,
      residual, act, rows, {8, 16, 32, 64}, waves, nontemporal, c10::nullopt,
      c10::nullopt, 0.0, 1, TILE + 1, 4 * TILE);
  const long M = c.M, N = c.N, K = c.K;
  const bool has_scale = w_scale.has_value() && w_scale->defined();
  TORCH_CHECK(has_scale == fp8, op,
              ": w_scale goes with a float8_e4m3fn weight and only with one");
  if (fp8)
    TORCH_CHECK(w_scale->device() == x.device() &&
                    w_scale->scalar_type() == torch::kFloat32 &&
                    w_scale->is_contiguous() && w_scale->dim() == 1 &&
                    w_scale->size(0) == N,
                op, ": w_scale must be a contiguous float32 [", N, "] on ",
                x.device());

  // Measured choice (benchmarks/bench_decode_linear.py --wide --sweep at
  // M = 32 and 64, GPT-1.3B and 6.7B shapes, KERNELS.md). Every workgroup
  // reads all of x from L2, M / rows (bf16) or 2 M / rows (fp8) times the
  // bytes of its weights, so rows are the most that still give 3/4 of the
  // CUs a workgroup (N = 6144 and 12288 on 256 CUs: 192 workgroups beat 384
  // with half the rows); below that the CUs are worth more than the x
  // stream, down to half tiles (N = 2048). Four row tiles keep enough loads
  // in flight with 4 waves; fewer want 8. Non-temporal weight loads gain a
  // few percent on weights under 64 MiB and lose up to 8 % above.
  if (rows == 0) {
    const long cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    rows = 8;
    for (long cand : {64L, 32L, 16L})
      if ((N + cand - 1) / cand >= (3 * cus) / 4) { rows = cand; break; }
  }
  if (waves == 0) waves = rows == 64 ? 4 : 8;
  const bool nt = nontemporal < 0 ? N * K * (fp8 ? 1 : 2) < (64L << 20)
                                  : nontemporal != 0;

  auto y = torch::empty({M, N}, x.options());
  const int gelu = act == "gelu";
  if (fp8) {
    const Args<unsigned char> a{
        (const short*)x.data_ptr(), (const unsigned char*)weight.data_ptr(),
        (const float*)w_scale->data_ptr(), c.bias, c.res, (short*)y.data_ptr(),
        (int)M, (int)N, (int)K, (int)rows, gelu, nullptr, nullptr, 0.f};
    launch_wide(a, waves, nt);
  } else {
    const Args<short> a{(const short*)x.data_ptr(),
                        (const short*)weight.data_ptr(), nullptr, c.bias,
                        c.res, (short*)y.data_ptr(), (int)M, (int)N, (int)K,
                        (int)rows, gelu, nullptr, nullptr, 0.f};
    launch_wide(a, waves, nt);
  }
  return y;
}
