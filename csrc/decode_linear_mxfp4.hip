// Weight-streaming linear for the decode step with MXFP4 weights, gfx950.
//
//   y[M,N] = act(x[M,K] . D[N,K]^T + bias[N]) + residual[M,N]
//
// x, bias, residual and y are bf16. D is never stored: Wq [N][K/2] holds OCP
// e2m1 codes, two per byte (element k of a row in byte k/2, even k the low
// nibble), and w_scale [N][K/32] one e8m0 byte per 32 elements along K,
// D[n][k] = e2m1(code) * 2^(w_scale[n][k/32] - 127)
// (ref.quantize_weight_mxfp4). The op is a read of N*K/2 + N*K/32 bytes:
// 0.53 of what decode_linear_fp8.hip streams, 0.27 of decode_linear.hip.
//
// Structure of the two siblings: codes go from global memory straight to
// VGPRs in 16-byte loads and are read once, x comes from L2, the k-steps are
// dealt to the waves in contiguous chunks, partial tiles are summed through
// LDS in wave order (bitwise reproducible) and the epilogue runs in the same
// launch. No counters, flags or atomics, no workspace.
//
// Fragments. A 16-byte load is 32 codes, exactly one MX block, so a k-step is
// 128 wide: a lane owns row lane&15, block lane>>4 of the step and that
// block's one scale byte. Word i of the load (codes 8i .. 8i+7 of the block)
// becomes the A fragment of the i-th of four v_mfma_f32_16x16x32_bf16; the B
// fragments are the four 16-byte loads of x at the same k. The MFMA sums over
// (lane group, element) pairs, so any k assignment that A and B share is a
// valid contraction.
//
// Decode. v_cvt_scalef32_pk_bf16_fp4 turns one byte of a word (two codes,
// the low nibble first) and the block's scale into two bf16: four per word,
// half a VALU op per code. An e2m1 value times a power of two is a bf16
// value, so nothing is rounded: the kernel computes x . D^T exactly as the
// bf16 kernel would from the decoded matrix, with no scale in the epilogue.
// The instruction reads the exponent field of an fp32 as the scale, so the
// byte e is handed over as e << 23 (the quantiser emits e in [2, 252]).
//
// Pipeline. A byte of codes in flight needs four bytes of x in registers (4
// VGPRs of codes against 16 of x per k-step), so the fp8 kernel's "a batch of
// everything in flight, wait, compute" does not fit. The two streams are
// pipelined across batches of U k-steps instead, with two sets of fragments:
//
//     codes(0) codes(1) x(0)
//     loop:  x(1)  | compute(0) | codes(2) x(2) | compute(1) | codes(3) ...
//
// While batch j is multiplied, the codes of batch j+1 (issued a whole batch
// earlier: the HBM stream, the deep one) and the x of batch j+1 (L2, issued
// just before) are outstanding, and the codes of batch j+2 follow as soon as
// their registers are free. Loads return in issue order, so each wait is a
// counted vmcnt that leaves the younger batch in flight.
//
// Rows of Wq and w_scale at index >= N, rows of x at index >= M and k-steps
// past a wave's chunk are never loaded ("Masked lanes" in
// decode_linear_common.h, which also holds the 16-byte load, the per-element
// epilogue and the binding's checks).
#include "decode_linear_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int int4v;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

constexpr int KSTEP = 128;          // k per 16-byte load of codes: four MFMAs
constexpr int CODE_STEP = KSTEP / 2;   // bytes of codes per row and k-step
constexpr int SCALE_STEP = KSTEP / 32;  // scale bytes per row and k-step

// 8 e2m1 codes (one word) times 2^(e-127) -> 8 bf16 in k order, exact
DEV_INLINE mfma_bf16x8 decode8(int w, float scale) {
  int4v o;
  o[0] = __builtin_bit_cast(
      int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)w, scale, 0));
  o[1] = __builtin_bit_cast(
      int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)w, scale, 1));
  o[2] = __builtin_bit_cast(
      int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)w, scale, 2));
  o[3] = __builtin_bit_cast(
      int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)w, scale, 3));
  return as_frag(o);
}

// k-steps per batch; two batches of fragments are live. Per step and lane,
// codes take 4 VGPRs per tile, the scale 1 per tile, x 16. One tile: 2 x 4
// steps, 8 code loads (128 bytes per lane) in flight as in the fp8 kernel;
// two and four tiles: 2 x 2 steps, 128 and 256 bytes.
template <int TILES>
struct Flight { static constexpr int U = TILES == 1 ? 4 : 2; };

// One batch of fragments: U k-steps of codes and scale bytes for every tile,
// and the x of the same k.
template <int TILES, int U>
struct Batch {
  int4v a[TILES][U];
  unsigned int e[TILES][U];
  int4v b[U][4];
};

// grid ceil(N / rows), NW*64 threads; rows = 16*TILES, or 8 with TILES = 1
// (the upper half of the MFMA tile masked). The TILES tiles of a workgroup
// share every x fragment.
// At least two waves per SIMD in every instance: the register allocator is
// held to 256 VGPRs + AGPRs also where 4 waves would let it take 512.
template <int NW, int TILES, bool NT>
__global__ __launch_bounds__(NW * WAVE)
    __attribute__((amdgpu_waves_per_eu(2))) NO_PK_F32
    void decode_linear_mxfp4_kernel(
    const short* __restrict__ x,                // [M, K] bf16
    const unsigned char* __restrict__ w,        // [N, K/2] e2m1 pairs
    const unsigned char* __restrict__ w_scale,  // [N, K/32] e8m0
    const short* __restrict__ bias,             // [N] or null
    const short* __restrict__ res,              // [M, N] or null
    short* __restrict__ y,                      // [M, N]
    int M, int N, int K, int rows, int gelu) {
  constexpr int U = Flight<TILES>::U;
  __shared__ float s_part[NW][TILES * TILE * TILE];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  // wave-uniform: keeps the chunk bounds and their branches scalar
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int r = lane & 15;    // W row in the tile / x row
  const int g = lane >> 4;    // MX block inside a k-step
  const int n0 = blockIdx.x * rows;
  const int tile_rows = min(rows, TILE);

  // Masked lanes (W rows past the tile or N, x rows >= M) load the
  // workgroup's first row / x row 0 in place of their own: a valid address
  // that another lane of the wave reads anyway, so no byte is fetched twice
  // and no row >= N or >= M is ever touched. Their fragments feed rows of C
  // that are never stored ("Masked lanes" in decode_linear_common.h). A
  // predicate here would be an exec-mask branch around every load, and the
  // waits below could no longer be counted.
  const unsigned char* wp[TILES];
  const unsigned char* sp[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const int row = n0 + t * TILE + r;
    const size_t rw = (r < tile_rows && row < N) ? row : n0;
    wp[t] = w + rw * (size_t)(K / 2) + g * 16;
    sp[t] = w_scale + rw * (size_t)(K / 32) + g;
  }
  const short* xp = x + (size_t)(r < M ? r : 0) * K + g * 32;

  // this wave's k-steps [s_beg, s_end): contiguous, sizes differ by <= 1
  const int steps = K / KSTEP;
  const int s_beg = (int)(((long)steps * wid) / NW);
  const int s_end = (int)(((long)steps * (wid + 1)) / NW);

  mfma_f32x4 acc[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc[t] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
  // k-steps past the chunk are neither loaded nor multiplied; their
  // fragments start as zero and keep whatever they held.
  const int4v zero4 = {0, 0, 0, 0};
  Batch<TILES, U> f0, f1;
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f0.b[u][i] = f1.b[u][i] = zero4;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      f0.a[t][u] = f1.a[t][u] = zero4;
      f0.e[t][u] = f1.e[t][u] = 0u;
    }
  }

  // tail = true puts every k-step behind s + u < s_end (wave-uniform, a
  // scalar branch); tail = false is for batches known to lie inside the
  // chunk. Codes tile by tile (one row's consecutive 64-byte pieces
  // adjacent, the fp8 kernel's measured order), each followed by its scale.
  auto load_codes = [&](Batch<TILES, U>& f, int s, bool tail)
                        __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!tail || s + u < s_end) {
          f.a[t][u] = load16<int4v, NT>(wp[t] + (size_t)(s + u) * CODE_STEP);
          f.e[t][u] = sp[t][(size_t)(s + u) * SCALE_STEP];
        }
      }
    }
  };
  auto load_x = [&](Batch<TILES, U>& f, int s, bool tail)
                    __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!tail || s + u < s_end) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          f.b[u][i] =
              load16<int4v, false>(xp + (size_t)(s + u) * KSTEP + 8 * i);
      }
    }
  };
  auto compute = [&](const Batch<TILES, U>& f, int s, bool tail)
                     __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!tail || s + u < s_end) {
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
          const float sc = __uint_as_float(f.e[t][u] << 23);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                decode8(f.a[t][u][i], sc), as_frag(f.b[u][i]), acc[t], 0, 0,
                0);
        }
      }
    }
  };
  // One turn: batches s and s + U are multiplied, s + 2U and s + 3U issued.
  auto turn = [&](int s, bool tail) __attribute__((always_inline)) {
    load_x(f1, s + U, tail);
    compute(f0, s, tail);
    load_codes(f0, s + 2 * U, tail);
    load_x(f0, s + 2 * U, tail);
    compute(f1, s + U, tail);
    load_codes(f1, s + 3 * U, tail);
  };

  // Steady state while a turn's four batches lie inside the chunk: no
  // branch between the loads and the MFMAs, so every wait is a counted
  // vmcnt that leaves the younger batch (codes and x) in flight. A
  // predicated load may or may not have been issued, and one s_waitcnt has
  // to be right for both: the tail's waits fall back to vmcnt(0). The tail
  // is at most 4U - 1 k-steps, everything it needs already in flight; a
  // short chunk (K = 2048 with 8 waves is 2 k-steps per wave) is all tail,
  // which is then the siblings' "everything in flight, wait, compute".
  int s = s_beg;
  if (s + 4 * U <= s_end) {
    load_codes(f0, s, false);
    load_codes(f1, s + U, false);
    load_x(f0, s, false);
    for (; s + 4 * U <= s_end; s += 2 * U) turn(s, false);
  } else {
    load_codes(f0, s, true);
    load_codes(f1, s + U, true);
    load_x(f0, s, true);
  }
  for (; s < s_end; s += 2 * U) turn(s, true);

  // C[n][m]: m = lane & 15, n = (lane >> 4) * 4 + i -> s_part[w][t][m*16 + n]
#pragma unroll
  for (int t = 0; t < TILES; ++t)
    *reinterpret_cast<float4v*>(
        &s_part[wid][t * TILE * TILE + r * TILE + g * 4]) = acc[t];
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

struct Mx4Args {
  const short* x;
  const unsigned char *w, *w_scale;
  const short *bias, *res;
  short* y;
  int M, N, K, rows, gelu;
};

template <int NW, int TILES, bool NT>
void launch(const Mx4Args& a) {
  auto stream = at::hip::getCurrentHIPStream();
  const int grid = (a.N + a.rows - 1) / a.rows;
  hipLaunchKernelGGL((decode_linear_mxfp4_kernel<NW, TILES, NT>), dim3(grid),
                     dim3(NW * WAVE), 0, stream, a.x, a.w, a.w_scale, a.bias,
                     a.res, a.y, a.M, a.N, a.K, a.rows, a.gelu);
}

template <int NW, bool NT>
void launch_tiles(const Mx4Args& a) {
  if (a.rows == 64) launch<NW, 4, NT>(a);
  else if (a.rows == 32) launch<NW, 2, NT>(a);
  else launch<NW, 1, NT>(a);
}

}  // namespace

// rows / waves / nontemporal: 0 / 0 / -1 choose automatically; other values
// are the benchmark's sweep (rows 8, 16, 32 or 64, waves 4 or 8, nt 0 or 1).
torch::Tensor decode_linear_mxfp4(torch::Tensor x, torch::Tensor wq,
                                  torch::Tensor w_scale,
                                  c10::optional<torch::Tensor> bias,
                                  c10::optional<torch::Tensor> residual,
                                  const std::string& act, long rows,
                                  long waves, long nontemporal) {
  const Checked c = check_decode_linear(
      "decode_linear_mxfp4", "wq", x, wq, torch::kUInt8, KSTEP, bias, residual,
      act, rows, {8, 16, 32, 64}, waves, nontemporal, c10::nullopt,
      c10::nullopt, 1e-5, /*pack=*/2);
  const long M = c.M, N = c.N, K = c.K;
  TORCH_CHECK(w_scale.defined() && w_scale.device() == x.device() &&
                  w_scale.scalar_type() == torch::kUInt8 &&
                  w_scale.is_contiguous() && w_scale.dim() == 2 &&
                  w_scale.size(0) == N && w_scale.size(1) == K / 32,
              "decode_linear_mxfp4: w_scale must be a contiguous uint8 [", N,
              ", ", K / 32, "] on ", x.device());

  // Measured choice (benchmarks/bench_decode_linear.py --weight-dtype mxfp4
  // --sweep at M = 1 and 16, GPT-1.3B and 6.7B shapes, KERNELS.md); NOT the
  // fp8 kernel's rule. Half tiles while full tiles would leave CUs without a
  // workgroup. A k-step is one code load against four x loads whatever M is,
  // so more tiles (which share the x fragments) pay from M = 1 on: the most
  // of 64 / 32 rows that still gives 3/4 of the CUs a workgroup; 64 rows on
  // a grid of more than two workgroups per CU (the vocabulary matrix) only
  // from M = 8 on. A grid of at most two workgroups per CU runs 8 waves and
  // non-temporal code loads, a larger one 4 waves and plain loads; a
  // one-tile workgroup whose 8 waves would get less than a batch of 4
  // k-steps each (K < 4096) stays at 4 waves.
  const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  if (rows == 0) {
    rows = (N + 15) / 16 < cus ? 8 : 16;
    if (rows == 16) {
      for (long cand : {64L, 32L}) {
        const long grid = (N + cand - 1) / cand;
        if (grid >= (3 * cus) / 4 &&
            (cand == 32 || M >= 8 || grid <= 2 * cus)) {
          rows = cand;
          break;
        }
      }
    }
  }
  const bool small_grid = (N + rows - 1) / rows <= 2 * cus;
  if (waves == 0)
    waves = small_grid && (rows > 16 || K >= 8 * 4 * KSTEP) ? 8 : 4;
  const bool nt = nontemporal < 0 ? small_grid : nontemporal != 0;

  auto y = torch::empty({M, N}, x.options());
  const Mx4Args a{(const short*)x.data_ptr(),
                  (const unsigned char*)wq.data_ptr(),
                  (const unsigned char*)w_scale.data_ptr(), c.bias, c.res,
                  (short*)y.data_ptr(), (int)M, (int)N, (int)K, (int)rows,
                  act == "gelu"};
  if (waves == 4) {
    if (nt) launch_tiles<4, true>(a);
    else launch_tiles<4, false>(a);
  } else {
    if (nt) launch_tiles<8, true>(a);
    else launch_tiles<8, false>(a);
  }
  return y;
}
