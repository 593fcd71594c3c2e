// Tiled GEMM over weight codes for M >= 65 rows, gfx950.
//
//   y[M,N] = act((x[M,K] . W[N,K]^T) (* w_scale[N]) + bias[N]) + residual[M,N]
//
// x, bias, residual and y are bf16. W is stored as codes, in the layouts the
// decode linears already read (no repacking):
//   fp8    float8_e4m3fn [N][K] and one fp32 scale per row, applied in the
//          epilogue (ref.quantize_weight_rows);
//   MXFP4  e2m1 pairs uint8 [N][K/2] (even k the low nibble) and e8m0 scales
//          uint8 [N][K/32], applied by the decode (ref.quantize_weight_mxfp4).
//
// Why not the wide kernels with more column tiles: there every wave decodes
// every code it multiplies and every workgroup reads all of x. Here a
// workgroup owns a BM x BN tile of y, and per 64-wide slab of K every code
// byte and every x element of the tile is loaded from global memory ONCE by
// ONE thread (16-byte loads), decoded once and shared through LDS: a decode
// serves BM rows of x, an x element BN rows of W.
//
// Slab. BK = 64 for both formats: 64 fp8 codes are four 16-byte pieces per
// row, 64 e2m1 codes two (a piece is one MX block, loaded with its scale
// byte). Piece c of the W slab is row c / PR, piece c % PR of it; x pieces
// are 8 bf16, 8 to a row. 8 (x), 4 or 2 (codes) consecutive threads read
// consecutive bytes of one row. Both decodes are exact (decode8_fp8,
// decode8_mx: the siblings' decoders, copied), so LDS holds the bf16 the
// float64 reference multiplies.
//
// LDS layout. One buffer is [BN rows of W][BM rows of x], each row 64 bf16 =
// 128 bytes at a stride of 144. A fragment read is ds_read_b128 by lane
// (r = lane & 15, g = lane >> 4) at row r, bytes 64 kk + 16 g: with 144 bytes
// = 36 banks between rows, the 16 rows of a lane group start at banks
// 36 r mod 64 = {0, 36, 8, 44, ...}, sixteen different multiples of 4, so the
// group's sixteen 4-bank reads cover the 64 banks once. A 128-byte stride
// would put rows r and r + 2 on the same banks (8-way conflict). The writes
// (16 bytes per thread, consecutive threads consecutive pieces of a row) are
// conflict-free at any stride that is a multiple of 16. attention.hip keeps
// its K tile the same way ([64][D + 8] shorts).
//
// Waves. 4 waves as WGM x WGN; a wave owns (BM / WGM) x (BN / WGN) of the
// tile as TM x TN MFMA tiles and walks all of K: its accumulators are final,
// the epilogue runs from registers, nothing is summed across waves. Per
// 32-wide k-step a wave reads TN A fragments (W) and TM B fragments (x) and
// issues TM * TN v_mfma_f32_16x16x32_bf16. A = W, so that a lane's four
// accumulator values are four consecutive n of one row m: one 8-byte store.
//
// Pipeline (attention.hip's issue-early / write-late). Two buffers, one
// barrier per slab. Step s: issue the global loads of slab s + 1 into
// registers, multiply slab s from buffer s & 1, then decode the registers and
// write them to the other buffer, barrier. The loop body has no branch: lanes
// whose row lies past N or M load row N - 1 or M - 1 instead (a valid row
// that other lanes read anyway; it lands in rows of C that are never
// stored), and threads without a piece of a small W slab reload another
// thread's piece and skip only the LDS write, which comes after the MFMAs.
//
// Rows of codes and scales at index >= N, rows of x at index >= M and k >= K
// (K % 64 == 0: slabs are whole) are never read. Row n of W reaches row n of
// C alone and row m of x column m alone, so a NaN stays where it was. No
// workspace, counters, flags or atomics; K is not split across workgroups or
// waves: two calls give the same bits.
#include "decode_linear_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int int4v;
typedef __attribute__((ext_vector_type(2))) int int2v;

constexpr int BK = 64;            // k per slab
constexpr int STRIDE = 144;       // bytes between slab rows: 128 + 16, above
constexpr int NTHR = 4 * WAVE;    // threads of a workgroup

// decode8 of decode_linear_fp8.hip: 8 e4m3 codes (two words) -> 8 bf16 in k
// order, exact: the high halves of the fp32 pairs v_cvt_pk_f32_fp8 gives.
DEV_INLINE int4v decode8_fp8(int w0, int w1) {
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
  return o;
}

// decode8 of decode_linear_mxfp4.hip: 8 e2m1 codes (one word) times
// 2^(e-127) -> 8 bf16 in k order, exact
DEV_INLINE int4v decode8_mx(int w, float scale) {
  int4v o;
  o[0] = __builtin_bit_cast(
      int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)w, scale, 0));
  o[1] = __builtin_bit_cast(
      int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)w, scale, 1));
  o[2] = __builtin_bit_cast(
      int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)w, scale, 2));
  o[3] = __builtin_bit_cast(
      int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)w, scale, 3));
  return o;
}

// What the format decides: 16-byte pieces of codes per row and slab, and the
// bytes of bf16 a piece decodes to.
template <bool MX>
struct Fmt {
  static constexpr int PR = MX ? 2 : 4;
  static constexpr int OUT = MX ? 64 : 32;
};

// grid (ceil(M / BM), ceil(N / BN)), 256 threads.
template <bool MX, int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(NTHR) void linear_codes_kernel(
    const short* __restrict__ x,                // [M, K] bf16
    const unsigned char* __restrict__ w,        // [N, K] e4m3 / [N, K/2] e2m1
    const void* __restrict__ w_scale,           // fp32 [N] / e8m0 [N, K/32]
    const short* __restrict__ bias,             // [N] or null
    const short* __restrict__ res,              // [M, N] or null
    short* __restrict__ y,                      // [M, N]
    int M, int N, int K, int gelu) {
  static_assert(WGM * WGN * WAVE == NTHR, "four waves");
  constexpr int PR = Fmt<MX>::PR, OUT = Fmt<MX>::OUT;
  constexpr int TM = BM / WGM / TILE, TN = BN / WGN / TILE;
  constexpr int WPIECES = BN * PR;                    // of one W slab
  constexpr int CW = (WPIECES + NTHR - 1) / NTHR;     // per thread
  constexpr int CX = BM * (BK / 8) / NTHR;            // x pieces per thread
  constexpr int XOFF = BN * STRIDE;                   // x rows follow W rows
  constexpr int BUF = (BN + BM) * STRIDE;             // bytes of one buffer
  static_assert(BM * (BK / 8) % NTHR == 0, "whole x pieces per thread");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int r = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int wm = (wid / WGN) * (BM / WGM);  // the wave's corner in the tile
  const int wn = (wid % WGN) * (BN / WGN);
  const size_t wrow = MX ? (size_t)K / 2 : (size_t)K;  // bytes of a code row

  // This thread's pieces. Rows past the end load the last row; a thread past
  // the slab's pieces reloads piece c % WPIECES and does not write it.
  const unsigned char* wp[CW];
  const unsigned char* sp[CW];
  int ww[CW];
  bool w_on[CW];
#pragma unroll
  for (int i = 0; i < CW; ++i) {
    const int c = tid + i * NTHR;
    w_on[i] = c < WPIECES;
    const int row = (c % WPIECES) / PR, p = c % PR;
    const size_t n = (size_t)min(n0 + row, N - 1);
    wp[i] = w + n * wrow + p * 16;
    sp[i] = (const unsigned char*)w_scale + n * (size_t)(K / 32) + p;
    ww[i] = row * STRIDE + p * OUT;
  }
  const short* xp[CX];
  int xw[CX];
#pragma unroll
  for (int i = 0; i < CX; ++i) {
    const int c = tid + i * NTHR;
    const int row = c / (BK / 8), col = c % (BK / 8);
    xp[i] = x + (size_t)min(m0 + row, M - 1) * K + col * 8;
    xw[i] = XOFF + row * STRIDE + col * 16;
  }
  // fragment (tile t or j, k-step kk): + 16 t STRIDE + 64 kk
  const int rd_w = (wn + r) * STRIDE + g * 16;
  const int rd_x = XOFF + (wm + r) * STRIDE + g * 16;

  mfma_f32x4 acc[TN][TM];
#pragma unroll
  for (int t = 0; t < TN; ++t)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[t][j] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};

  int4v cw[CW], cx[CX];
  unsigned int ce[CW];
  auto load_slab = [&](int s) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < CW; ++i) {
      cw[i] = load16<int4v, false>(wp[i] + (size_t)s * (PR * 16));
      if constexpr (MX) ce[i] = sp[i][(size_t)s * (BK / 32)];
    }
#pragma unroll
    for (int i = 0; i < CX; ++i)
      cx[i] = load16<int4v, false>(xp[i] + (size_t)s * BK);
  };
  auto store_slab = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < CW; ++i) {
      if (CW * NTHR == WPIECES || w_on[i]) {
        int4v* d = reinterpret_cast<int4v*>(&smem[buf + ww[i]]);
        if constexpr (MX) {
          const float sc = __uint_as_float(ce[i] << 23);
#pragma unroll
          for (int q = 0; q < 4; ++q) d[q] = decode8_mx(cw[i][q], sc);
        } else {
          d[0] = decode8_fp8(cw[i][0], cw[i][1]);
          d[1] = decode8_fp8(cw[i][2], cw[i][3]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < CX; ++i)
      *reinterpret_cast<int4v*>(&smem[buf + xw[i]]) = cx[i];
  };
  auto compute = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      int4v a[TN], b[TM];
#pragma unroll
      for (int t = 0; t < TN; ++t)
        a[t] = *reinterpret_cast<const int4v*>(
            &smem[buf + rd_w + t * TILE * STRIDE + kk * 64]);
#pragma unroll
      for (int j = 0; j < TM; ++j)
        b[j] = *reinterpret_cast<const int4v*>(
            &smem[buf + rd_x + j * TILE * STRIDE + kk * 64]);
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int j = 0; j < TM; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              as_frag(a[t]), as_frag(b[j]), acc[t][j], 0, 0, 0);
    }
  };

  const int steps = K / BK;
  load_slab(0);
  store_slab(0);
  __syncthreads();
  int cur = 0;  // byte offset of the buffer being multiplied
  for (int s = 0; s + 1 < steps; ++s) {
    load_slab(s + 1);
    // the loads stay ahead of the MFMAs they are to hide behind
    __builtin_amdgcn_sched_barrier(0);
    compute(cur);
    store_slab(cur ^ BUF);
    __syncthreads();
    cur ^= BUF;
  }
  compute(cur);

  // C[n][m]: m = lane & 15 (+ 16 j), n = 4 (lane >> 4) + i (+ 16 t). N % 8
  // == 0 and n % 4 == 0: the four n of a lane are inside N together.
#pragma unroll
  for (int j = 0; j < TM; ++j) {
    const int m = m0 + wm + j * TILE + r;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const int n = n0 + wn + t * TILE + g * 4;
      if (m < M && n < N) {
        // finish_element on a row of four: its y is this lane's registers
        const size_t o = (size_t)m * N + n;
        union { short s[4]; int2v v; } out;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          finish_element<!MX>(acc[t][j][i], 0, i, N,
                              (const float*)w_scale + n,
                              bias ? bias + n : nullptr,
                              res ? res + o : nullptr, out.s, gelu);
        *reinterpret_cast<int2v*>(y + o) = out.v;
      }
    }
  }
}

struct CodesArgs {
  const short* x;
  const unsigned char* w;
  const void* w_scale;
  const short *bias, *res;
  short* y;
  int M, N, K, gelu;
};

template <bool MX, int BM, int BN, int WGM, int WGN>
void launch(const CodesArgs& a) {
  auto stream = at::hip::getCurrentHIPStream();
  // M tiles on x (up to 2^31 - 1 of them), N tiles on y (checked below)
  const dim3 grid((a.M + BM - 1) / BM, (a.N + BN - 1) / BN);
  hipLaunchKernelGGL((linear_codes_kernel<MX, BM, BN, WGM, WGN>), grid,
                     dim3(NTHR), 0, stream, a.x, a.w, a.w_scale, a.bias,
                     a.res, a.y, a.M, a.N, a.K, a.gelu);
}

template <bool MX>
void launch_tile(const CodesArgs& a, long tile_n) {
  if (tile_n == 128) launch<MX, 128, 128, 2, 2>(a);
  else if (tile_n == 64) launch<MX, 128, 64, 2, 2>(a);
  else launch<MX, 128, 32, 4, 1>(a);
}

}  // namespace

// codes: float8_e4m3fn [N, K] with w_scale fp32 [N], or uint8 [N, K/2] (MXFP4)
// with w_scale uint8 [N, K/32]. tile_n: 0 chooses automatically; 128, 64 or
// 32 name the instance (the benchmark's sweep and the tests).
torch::Tensor linear_codes(torch::Tensor x, torch::Tensor codes,
                           torch::Tensor w_scale,
                           c10::optional<torch::Tensor> bias,
                           c10::optional<torch::Tensor> residual,
                           const std::string& act, long tile_n) {
  const char* op = "linear_codes";
  TORCH_CHECK(codes.defined() && w_scale.defined(), op,
              ": x, codes and w_scale must be defined");
  const bool fp8 = codes.scalar_type() == torch::kFloat8_e4m3fn;
  const Checked c = check_decode_linear(
      op, "codes", x, codes, fp8 ? torch::kFloat8_e4m3fn : torch::kUInt8,
      fp8 ? BK : 2 * BK, bias, residual, act, 0, {}, 0, -1, c10::nullopt,
      c10::nullopt, 0.0, fp8 ? 1 : 2, 4 * TILE + 1, (1L << 31) - 1);
  const long M = c.M, N = c.N, K = c.K;
  if (fp8) {
    TORCH_CHECK(w_scale.device() == x.device() &&
                    w_scale.scalar_type() == torch::kFloat32 &&
                    w_scale.is_contiguous() && w_scale.dim() == 1 &&
                    w_scale.size(0) == N,
                op, ": w_scale must be a contiguous float32 [", N, "] on ",
                x.device());
  } else {
    TORCH_CHECK(w_scale.device() == x.device() &&
                    w_scale.scalar_type() == torch::kUInt8 &&
                    w_scale.is_contiguous() && w_scale.dim() == 2 &&
                    w_scale.size(0) == N && w_scale.size(1) == K / 32,
                op, ": w_scale must be a contiguous uint8 [", N, ", ", K / 32,
                "] on ", x.device());
  }
  TORCH_CHECK(tile_n == 0 || tile_n == 32 || tile_n == 64 || tile_n == 128, op,
              ": tile_n must be 0 (auto), 32, 64 or 128");
  TORCH_CHECK((N + 31) / 32 <= 65535, op, ": N must be at most ", 65535 * 32,
              ", got ", N);

  // Measured choice (benchmarks/bench_decode_linear.py --codes --sweep at
  // M = 128, 256 and 2048, GPT-1.3B and 6.7B shapes, both formats,
  // KERNELS.md). A workgroup walks all of K with one barrier per slab, and
  // two fit a CU: the widest tile wins once its grid is 3/2 of the CUs (the
  // logits at M = 128: 393 workgroups of 128 x 128 beat 786 of 128 x 64 by
  // 15 %), below that the grid is worth more than the reuse (256 workgroups
  // of 128 x 128 lose 10 to 13 % to 512 of 128 x 64), down to 128 x 32.
  if (tile_n == 0) {
    const long cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    const long mt = (M + 127) / 128;
    tile_n = 32;
    for (long cand : {128L, 64L})
      if (2 * mt * ((N + cand - 1) / cand) >= 3 * cus) {
        tile_n = cand;
        break;
      }
  }

  auto y = torch::empty({M, N}, x.options());
  const CodesArgs a{(const short*)x.data_ptr(),
                    (const unsigned char*)codes.data_ptr(),
                    w_scale.data_ptr(), c.bias, c.res, (short*)y.data_ptr(),
                    (int)M, (int)N, (int)K, act == "gelu"};
  if (fp8) launch_tile<false>(a, tile_n);
  else launch_tile<true>(a, tile_n);
  return y;
}
