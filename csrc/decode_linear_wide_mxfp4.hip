// Weight-streaming linear for decode batches of 17 to 64 rows with MXFP4
// weights, gfx950.
//
//   y[M,N] = act(x[M,K] . D[N,K]^T + bias[N]) + residual[M,N]
//
// x, bias, residual and y are bf16; D is what ref.dequantize_weight_mxfp4
// yields from Wq [N][K/2] (e2m1 codes, two per byte, even k the low nibble)
// and w_scale [N][K/32] (e8m0), the stored layout of decode_linear_mxfp4.hip.
//
// Why not a third weight type of decode_linear_wide.hip: there every wave
// pulls its own x fragments from L2 into registers, and an MXFP4 k-step (128
// wide: one 16-byte code load is one MX block) would need 4 * MT 16-byte x
// loads per lane next to one code load per tile. Here x goes through LDS
// instead, once per workgroup:
//
// Slab. The workgroup copies x[0:M, 128 s : 128 s + 128] (one k-step, all
// column tiles) into LDS with coalesced 16-byte loads, 16 consecutive threads
// per row. Every wave reads its B fragments from it with ds_read_b128: lane
// (r = lane & 15, g = lane >> 4) reads row 16 j + r, k = 32 g + 8 i for
// column tile j and word i of its code load. A row is 256 bytes; the stride
// is 272, so the 16 rows of a fragment read start 4 banks apart and cover
// the 64 banks once (a 256-byte stride would put all 16 on the same four).
// Two buffers, one barrier per slab: step s reads buffer s & 1 and, after its
// MFMAs, writes slab s + 1 into the other one.
//
// Waves split rows, not K. Wave w of NW owns weight rows
// n0 + w * rows .. + rows (rows = 16 * TILES, or 8: the upper half of the
// MFMA tile masked) and walks all of K, so its TILES x MT accumulators are
// final: no sum over the waves, the epilogue runs from registers. A decoded A
// fragment feeds MT v_mfma_f32_16x16x32_bf16 and a B fragment read from LDS
// feeds TILES.
//
// Pipeline. Loads return in issue order, so a wait for slab registers also
// waits for every code load issued before them. Both streams therefore run
// the same distance CD ahead in two register rings: step s issues the codes
// of step s + CD and the x of slab s + 1 + CD, and its one wait (before the
// LDS write of slab s + 1) is a counted vmcnt that leaves CD k-steps of
// codes, CD * TILES >= 8 16-byte loads per lane, and CD - 1 slabs in flight.
// The steady state is unrolled CD times (ring slots and the buffer parity
// are compile-time) and has no branch; the tail repeats the step behind
// workgroup-uniform predicates.
//
// Rows of Wq and w_scale at index >= N, rows of x at index >= M and k past K
// are never read: masked lanes load a row another lane reads anyway (see
// decode_linear_mxfp4.hip), slab rows >= M are copies of row M - 1 and feed
// columns of C that are never stored. No counters, flags, atomics or
// workspace: two calls give the same bits.
#include "decode_linear_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int int4v;

constexpr int KSTEP = 128;              // k per 16-byte load of codes = slab
constexpr int CODE_STEP = KSTEP / 2;    // bytes of codes per row and k-step
constexpr int SCALE_STEP = KSTEP / 32;  // scale bytes per row and k-step
constexpr int ROW_BYTES = KSTEP * 2;    // a slab row of bf16
constexpr int STRIDE = ROW_BYTES + 16;  // padded: rows start 4 banks apart
constexpr int ROW_CHUNKS = ROW_BYTES / 16;

// decode8 of decode_linear_mxfp4.hip: 8 e2m1 codes (one word) times
// 2^(e-127) -> 8 bf16 in k order, exact
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

// k-steps both streams run ahead: 8 code loads per lane in flight, at least
// two steps (even, so the slab buffer of an unrolled step is static).
template <int TILES>
struct Flight { static constexpr int CD = TILES >= 4 ? 2 : 8 / TILES; };

// grid ceil(N / (NW * rows)), NW*64 threads. 16*(MT-1) < M <= 16*MT.
template <int NW, int TILES, int MT, bool NT>
__global__ __launch_bounds__(NW * WAVE) NO_PK_F32
    void decode_linear_wide_mxfp4_kernel(
    const short* __restrict__ x,                // [M, K] bf16
    const unsigned char* __restrict__ w,        // [N, K/2] e2m1 pairs
    const unsigned char* __restrict__ w_scale,  // [N, K/32] e8m0
    const short* __restrict__ bias,             // [N] or null
    const short* __restrict__ res,              // [M, N] or null
    short* __restrict__ y,                      // [M, N]
    int M, int N, int K, int rows, int gelu) {
  constexpr int CD = Flight<TILES>::CD;
  constexpr int NTHR = NW * WAVE;
  constexpr int CHUNKS = MT * TILE * ROW_CHUNKS;     // 16-byte pieces of a slab
  constexpr int XC = (CHUNKS + NTHR - 1) / NTHR;     // per thread
  constexpr int SLAB = MT * TILE * STRIDE;           // bytes of one buffer
  __shared__ __attribute__((aligned(16))) unsigned char s_x[2 * SLAB];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int r = lane & 15;  // W row in the tile / x row in the column tile
  const int g = lane >> 4;  // MX block inside a k-step
  const int n0 = blockIdx.x * (NW * rows);
  const int nw = n0 + wid * rows;  // this wave's first row
  const int tile_rows = min(rows, TILE);

  // Masked lanes (W rows past the half tile or N) load the wave's first row,
  // a wave past N the workgroup's: an address another lane reads anyway.
  const unsigned char* wp[TILES];
  const unsigned char* sp[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const int row = nw + t * TILE + r;
    const size_t rw =
        (r < tile_rows && row < N) ? row : (nw < N ? nw : n0);
    wp[t] = w + rw * (size_t)(K / 2) + g * 16;
    sp[t] = w_scale + rw * (size_t)(K / 32) + g;
  }
  // This thread's pieces of a slab: piece c is row c / 16, bytes 16 (c % 16)
  // of it. Rows >= M copy row M - 1; a thread without an XC-th piece (MT = 3
  // with 8 waves) repeats its previous one.
  const short* xp[XC];
  int xw[XC];
#pragma unroll
  for (int i = 0; i < XC; ++i) {
    int c = tid + i * NTHR;
    if (c >= CHUNKS) c -= NTHR;
    const int row = c / ROW_CHUNKS, col = c % ROW_CHUNKS;
    xp[i] = x + (size_t)min(row, M - 1) * K + col * 8;
    xw[i] = row * STRIDE + col * 16;
  }
  const int rd = r * STRIDE + g * 64;  // fragment (j, i): + 16 j STRIDE + 16 i

  const int steps = K / KSTEP;  // >= 4

  mfma_f32x4 acc[TILES][MT];
#pragma unroll
  for (int t = 0; t < TILES; ++t)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[t][j] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
  // the rings: slot u holds the codes of step s + u and the x of slab
  // s + u + 1 (slot (u + 1) % CD), s a multiple of CD
  const int4v zero4 = {0, 0, 0, 0};
  int4v a[CD][TILES], xs[CD][XC];
  unsigned int e[CD][TILES];
#pragma unroll
  for (int u = 0; u < CD; ++u) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      a[u][t] = zero4;
      e[u][t] = 0u;
    }
#pragma unroll
    for (int i = 0; i < XC; ++i) xs[u][i] = zero4;
  }

  auto load_codes = [&](int u, int s) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      a[u][t] = load16<int4v, NT>(wp[t] + (size_t)s * CODE_STEP);
      e[u][t] = sp[t][(size_t)s * SCALE_STEP];
    }
  };
  auto load_x = [&](int u, int s) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < XC; ++i)
      xs[u][i] = load16<int4v, false>(xp[i] + (size_t)s * KSTEP);
  };
  auto store_x = [&](int u, int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < XC; ++i)
      *reinterpret_cast<int4v*>(&s_x[buf * SLAB + xw[i]]) = xs[u][i];
  };
  auto compute = [&](int u, int buf) __attribute__((always_inline)) {
    float sc[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) sc[t] = __uint_as_float(e[u][t] << 23);
    // the MT fragments of word i + 1 are read while word i is multiplied:
    // read one by one, each ds_read's latency lay open before its MFMAs
    int4v b[2][MT];
    auto read_b = [&](int i) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < MT; ++j)
        b[i & 1][j] = *reinterpret_cast<const int4v*>(
            &s_x[buf * SLAB + rd + j * TILE * STRIDE + i * 16]);
    };
    read_b(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < 3) read_b(i + 1);
      mfma_bf16x8 af[TILES];
#pragma unroll
      for (int t = 0; t < TILES; ++t) af[t] = decode8(a[u][t][i], sc[t]);
#pragma unroll
      for (int j = 0; j < MT; ++j)
#pragma unroll
        for (int t = 0; t < TILES; ++t)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[t], as_frag(b[i & 1][j]), acc[t][j], 0, 0, 0);
    }
  };
  // Step s = base + u: multiply slab s by the codes of step s, refill the
  // code slot, move slab s + 1 from its registers into the spare buffer,
  // refill those registers, barrier. tail puts what lies past K behind
  // predicates that are the same in every wave of the workgroup.
  auto step = [&](int s, int u, bool tail) __attribute__((always_inline)) {
    const int v = (u + 1) % CD;
    compute(u, u & 1);
    if (!tail || s + CD < steps) load_codes(u, s + CD);
    if (!tail || s + 1 < steps) store_x(v, (u + 1) & 1);
    if (!tail || s + 1 + CD < steps) load_x(v, s + 1 + CD);
    __syncthreads();
    // nothing of a later step (its scale shifts, with their waits for the
    // whole ring) is scheduled ahead of this barrier
    __builtin_amdgcn_sched_barrier(0);
  };

  // Prologue: slab 0 first (it is waited for first), then both rings.
  {
    int4v x0[XC];
#pragma unroll
    for (int i = 0; i < XC; ++i) x0[i] = load16<int4v, false>(xp[i]);
#pragma unroll
    for (int u = 0; u < CD; ++u) {
      if (u < steps) load_codes(u, u);
      if (u + 1 < steps) load_x((u + 1) % CD, u + 1);
    }
#pragma unroll
    for (int i = 0; i < XC; ++i)
      *reinterpret_cast<int4v*>(&s_x[xw[i]]) = x0[i];
    __syncthreads();
  }

  int s = 0;
  for (; s + 2 * CD < steps; s += CD) {
#pragma unroll
    for (int u = 0; u < CD; ++u) step(s + u, u, false);
  }
  for (; s < steps; s += CD) {
#pragma unroll
    for (int u = 0; u < CD; ++u)
      if (s + u < steps) step(s + u, u, true);
  }

  // C[n][m]: m = lane & 15 (+ 16 j), n = (lane >> 4) * 4 + i (+ 16 t)
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const int m = j * TILE + r;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int nt = g * 4 + i;
        const int n = nw + t * TILE + nt;
        if (m < M && nt < tile_rows && n < N)
          finish_element<false>(acc[t][j][i], m, n, N, nullptr, bias, res, y,
                                gelu);
      }
    }
  }
}

struct WideMx4Args {
  const short* x;
  const unsigned char *w, *w_scale;
  const short *bias, *res;
  short* y;
  int M, N, K, rows, gelu;
};

template <int NW, int TILES, int MT>
void launch(const WideMx4Args& a, bool nt) {
  auto stream = at::hip::getCurrentHIPStream();
  const int wg_rows = NW * a.rows;
  const int grid = (a.N + wg_rows - 1) / wg_rows;
  if (nt)
    hipLaunchKernelGGL((decode_linear_wide_mxfp4_kernel<NW, TILES, MT, true>),
                       dim3(grid), dim3(NW * WAVE), 0, stream, a.x, a.w,
                       a.w_scale, a.bias, a.res, a.y, a.M, a.N, a.K, a.rows,
                       a.gelu);
  else
    hipLaunchKernelGGL((decode_linear_wide_mxfp4_kernel<NW, TILES, MT, false>),
                       dim3(grid), dim3(NW * WAVE), 0, stream, a.x, a.w,
                       a.w_scale, a.bias, a.res, a.y, a.M, a.N, a.K, a.rows,
                       a.gelu);
}

template <int NW, int TILES>
void launch_cols(const WideMx4Args& a, bool nt) {
  const int mt = (a.M + TILE - 1) / TILE;
  if (mt == 2) launch<NW, TILES, 2>(a, nt);
  else if (mt == 3) launch<NW, TILES, 3>(a, nt);
  else launch<NW, TILES, 4>(a, nt);
}

template <int NW>
void launch_tiles(const WideMx4Args& a, bool nt) {
  if (a.rows == 64) launch_cols<NW, 4>(a, nt);
  else if (a.rows == 32) launch_cols<NW, 2>(a, nt);
  else launch_cols<NW, 1>(a, nt);
}

}  // namespace

// rows: weight rows per WAVE (8, 16, 32 or 64); a workgroup serves
// waves * rows of them. rows / waves / nontemporal: 0 / 0 / -1 choose
// automatically; other values are the benchmark's sweep (waves 4 or 8, nt 0
// or 1, every combination legal).
torch::Tensor decode_linear_wide_mxfp4(torch::Tensor x, torch::Tensor wq,
                                       torch::Tensor w_scale,
                                       c10::optional<torch::Tensor> bias,
                                       c10::optional<torch::Tensor> residual,
                                       const std::string& act, long rows,
                                       long waves, long nontemporal) {
  const char* op = "decode_linear_wide_mxfp4";
  const Checked c = check_decode_linear(
      op, "wq", x, wq, torch::kUInt8, KSTEP, bias, residual, act, rows,
      {8, 16, 32, 64}, waves, nontemporal, c10::nullopt, c10::nullopt, 0.0,
      /*pack=*/2, TILE + 1, 4 * TILE);
  const long M = c.M, N = c.N, K = c.K;
  // fewer than four k-steps leave the rings nothing to run ahead of
  TORCH_CHECK(K >= 4 * KSTEP, op, ": K must be at least ", 4 * KSTEP,
              ", got ", K);
  TORCH_CHECK(w_scale.defined() && w_scale.device() == x.device() &&
                  w_scale.scalar_type() == torch::kUInt8 &&
                  w_scale.is_contiguous() && w_scale.dim() == 2 &&
                  w_scale.size(0) == N && w_scale.size(1) == K / 32,
              op, ": w_scale must be a contiguous uint8 [", N, ", ", K / 32,
              "] on ", x.device());

  // Measured choice (benchmarks/bench_decode_linear.py --wide --weight-dtype
  // mxfp4 --sweep at M = 32 and 64, GPT-1.3B and 6.7B shapes, KERNELS.md).
  // A workgroup walks all of K, one barrier per k-step, so the time is the
  // walk's latency until the grid covers the CUs several times over: the
  // largest workgroup of 8 x 32, 4 x 32, 4 x 16 rows that still gives 3/4 of
  // the CUs one (N = 50304: 256 rows; 12288 and 16384: 64), else 4 half
  // tiles (N <= 8192 on 256 CUs). Non-temporal code loads never won by more
  // than the noise and lose up to 10 % on the vocabulary matrix: off.
  if (rows == 0 && waves == 0) {
    const long cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    rows = 8;
    waves = 4;
    for (long wg : {256L, 128L, 64L}) {
      if ((N + wg - 1) / wg >= (3 * cus) / 4) {
        waves = wg == 256 ? 8 : 4;
        rows = wg / waves;
        break;
      }
    }
  }
  if (waves == 0) waves = 4;  // the sweep: 4 waves won at every rows but 32
  if (rows == 0) rows = 8;
  const bool nt = nontemporal > 0;

  auto y = torch::empty({M, N}, x.options());
  const WideMx4Args a{(const short*)x.data_ptr(),
                      (const unsigned char*)wq.data_ptr(),
                      (const unsigned char*)w_scale.data_ptr(), c.bias, c.res,
                      (short*)y.data_ptr(), (int)M, (int)N, (int)K, (int)rows,
                      act == "gelu"};
  if (waves == 4) launch_tiles<4>(a, nt);
  else launch_tiles<8>(a, nt);
  return y;
}
