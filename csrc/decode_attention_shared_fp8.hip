// Shared-prompt decode attention with an fp8 prompt prefix, gfx950.
//
// decode_attention_shared.hip with the prompt's K/V stored as e4m3fn codes
// ([P, h, Lcap, D] bytes plus one fp32 scale per stored row, [P, h, Lcap]:
// the layout kv_store_fp8 writes, the recipe of ref.quantize_kv_rows): D + 4
// bytes per prefix row instead of 2*D. The rows' own tokens stay bf16. Three
// launches, no counters, flags or atomics:
//   1. prefix  (decode_prefix_fp8_kernel, this file);
//   2. suffix  (decode_attn_kernel<D, true>, decode_attention_kernel.h,
//      unchanged: the bf16 walk over each row's own tokens and the append);
//   3. merge   (decode_merge_kernel, decode_common.h).
// Workspace, grid, wave split, the permuted contraction order of the second
// product and the in-order merge of the four waves are those of the bf16
// prefix pass; what differs is how the data moves.
//
// S^T = K Q^T. K codes go from global memory to VGPRs in 16-byte loads of the
// stored layout: a lane owns position lane & 15 and the 16 channels
// (lane >> 4)*16 .. +16 of a 64-wide k-step (one load per position row at
// D = 64, two at D = 128). Codes 0-7 and 8-15 are the A fragments of two
// v_mfma_f32_16x16x32_bf16 (the scheme of decode_linear_fp8.hip); the Q
// fragments are loaded once with the same k assignment, and any assignment
// the two operands share is a valid contraction. Codes are decoded in
// registers with v_cvt_pk_f32_fp8 + v_perm_b32 (exact: every finite e4m3fn
// value is a bf16 value). The row scale stays outside the product:
// s = st * scale * k_scale[pos].
//
// O^T = V^T P^T. v_scale[pos] is folded into P before its one bf16 rounding,
// pf = bf16(pw * v_scale); l sums the unscaled pw, as decode_attn_fp8_kernel
// does. V^T lives in LDS as CODES: a per-wave byte image whose columns are in
// the permuted order, so a lane's A fragment (8 contraction slots) is ONE
// ds_read_b64, decoded after the read. The image is built with dword writes
// from a 4x4 byte transpose in registers (v_perm_b32): a lane loads the same
// D/8 channels of four positions that are neighbours in the permuted order
// (16-byte loads at D = 128, 8-byte at D = 64: 32 positions x D bytes per
// wave step). Every V element is still decoded once; LDS bytes written and
// read are half of the bf16 image's.
//
// Scales. A lane needs the K and V scales of the 8 positions whose scores it
// holds (g*4 .. +4 of both tiles). They are NOT loaded as four-float vectors:
// that needs Lcap % 4 == 0 and 16-byte aligned chunk starts, and a vector
// that straddles prefix_lens would read past the end. Instead every lane
// loads ONE scale per step (lanes 0-31 the K scales of the step's 32
// positions, lanes 32-63 the V scales; one coalesced dword load, selected to
// 0 past the end), the wave writes them to a 64-float LDS strip next to the V
// image and every lane reads its 2 x 4 + 2 x 4 back as four ds_read_b128. No
// alignment condition, nothing past the end is read, one VMEM instruction
// instead of 4 (vectors) or 16 (dwords).
//
// Masking: positions >= prefix_lens[p] are never loaded; their codes and V
// scales are zero by select and their scores -inf by select, so a NaN code or
// scale past the end never reaches an MFMA. Sample columns >= G carry a zero
// Q and are never stored.
#include "decode_attention_shared_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int int4v;
typedef __attribute__((ext_vector_type(2))) int int2v;

// Byte image Vt8: row d (a channel) holds the step's 32 codes in the permuted
// order and starts at d*VT8_STRIDE + (d >> 4)*VT8_SKEW.
// Reads (ds_read_b64, lane (r, g) reads bytes g*8 .. +8 of row db*16 + r):
// rows are 10 dwords apart, so the 16 rows of a quarter-wave start at dwords
// 10*r = 0, 10, 20, 30, 40, 50, 60, 6, 16, 26, 36, 46, 56, 2, 12, 22 (mod
// 64) and a lane takes dwords 2*g, 2*g + 1 from there: the 32 lanes of a
// b64 pass (g = 0, 1) touch 64 different dwords, and modulo 32 each g alone
// covers all 32 banks once. 40 is a multiple of 8, so reads stay aligned.
// Writes (ds_write_b32, lane (q, cb) writes column dword q of rows
// cb*(D/8) .. +D/8, one row per instruction): at D = 128 the lane's rows are
// one 16-row block, whose 160 dwords are 0 modulo 32, so without the skew all
// eight cb would hit banks q; 8 more dwords per block put cb at 168*cb =
// 0, 40, 16, 56, 32, 8, 48, 24 (mod 64): 64 lanes on 64 different dwords. A
// read instruction has one db, so the skew shifts all its lanes alike. At
// D = 64 (8 rows per lane) two cb share a block and writes stay 2-way.
constexpr int VT8_STRIDE = 40;
constexpr int VT8_SKEW = 32;

// 8 e4m3 codes (two words) -> 8 bf16, exact: the high halves of the fp32
// pairs v_cvt_pk_f32_fp8 gives, packed by v_perm_b32 (4 VALU ops per 4 codes)
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
  return __builtin_bit_cast(mfma_bf16x8, o);
}

// 4x4 byte transpose: w[i] holds bytes b = 0..3 of row i; t[b] gets byte i
// from row i. v_perm_b32 selector bytes 0-3 pick from the second operand,
// 4-7 from the first.
DEV_INLINE void transpose4x4(const unsigned int* w, unsigned int* t) {
  const unsigned int a0 = __builtin_amdgcn_perm(w[1], w[0], 0x05010400u);
  const unsigned int a1 = __builtin_amdgcn_perm(w[1], w[0], 0x07030602u);
  const unsigned int b0 = __builtin_amdgcn_perm(w[3], w[2], 0x05010400u);
  const unsigned int b1 = __builtin_amdgcn_perm(w[3], w[2], 0x07030602u);
  t[0] = __builtin_amdgcn_perm(b0, a0, 0x05040100u);
  t[1] = __builtin_amdgcn_perm(b0, a0, 0x07060302u);
  t[2] = __builtin_amdgcn_perm(b1, a1, 0x05040100u);
  t[3] = __builtin_amdgcn_perm(b1, a1, 0x07060302u);
}

// grid (P*h*ncg, chunks), 256 threads.
// ws: fp32 [B*h, ws_slots, D+4]; chunk ck goes to slot 1 + ck.
template <int D>
__global__ __launch_bounds__(PNW * WAVE) void decode_prefix_fp8_kernel(
    const short* __restrict__ qkv,               // [B, 1, h, 3, D] bf16
    const unsigned char* __restrict__ k_prefix,  // [P, h, Lcap, D] e4m3
    const unsigned char* __restrict__ v_prefix,
    const float* __restrict__ k_scale,           // [P, h, Lcap]
    const float* __restrict__ v_scale,
    const int* __restrict__ prefix_lens,         // [P]
    float* __restrict__ ws, int h, int G, int ncg, int Lcap, int chunk,
    int ws_slots, float scale) {
  constexpr int KS = D / 64;   // 64-wide k-steps of K Q^T
  constexpr int DB = D / 16;   // row blocks of O^T
  constexpr int VW = D / 32;   // words (4 channels each) a lane loads per V row
  constexpr int SROW = D + 4;  // floats per sample of a wave's final state
  constexpr int IMAGE = D * VT8_STRIDE + DB * VT8_SKEW;  // bytes
  constexpr int STATE = COLS * SROW * 4;
  // the bf16 kernel reuses its image for the final state; the byte image is
  // half as large, so the region is sized for the larger of the two
  constexpr int REGION = IMAGE > STATE ? IMAGE : STATE;
  static_assert(STATE <= REGION && IMAGE <= REGION && REGION % 16 == 0,
                "the wave's final state and its V image share one region");
  __shared__ __attribute__((aligned(16))) unsigned char s_vt[PNW][REGION];
  __shared__ __attribute__((aligned(16))) float s_sc[PNW][2 * PSTEP];

  const int cg = blockIdx.x % ncg;
  const int ph = blockIdx.x / ncg;
  const int p = ph / h, head = ph % h;
  const int ck = blockIdx.y, nck = gridDim.y;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int r = lane & 15, g = lane >> 4;

  int start, end;  // positions of this chunk
  chunk_bounds(prefix_lens[p], Lcap, chunk, ck, nck, start, end);

  const short8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  // Q^T: column = sample; columns >= G are zero and never stored. Fragment
  // (ks, half) holds channels ks*64 + g*16 + half*8 .. + 8: the k assignment
  // of the K codes.
  const int smp = cg * COLS + r;
  const bool q_ok = smp < G;
  short8v qf[KS][2];
  {
    const short* qp =
        qkv + ((size_t)(p * G + (q_ok ? smp : 0)) * h + head) * 3 * D + g * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        qf[ks][hf] =
            q_ok ? *reinterpret_cast<const short8v*>(qp + ks * 64 + hf * 8)
                 : zero8;
  }

  const unsigned char* kbase = k_prefix + (size_t)ph * Lcap * D + g * 16;
  // V image items of this lane: columns 4*vq .. + 4 of the permuted order,
  // which are positions va .. va + 4 of the step, channels vcb*(D/8) .. + D/8
  const int vcb = lane & 7, vq = lane >> 3;
  const int va = perm_pos(4 * vq);
  const unsigned char* vbase =
      v_prefix + (size_t)ph * Lcap * D + vcb * (D / 8);
  // lanes 0-31: K scale, lanes 32-63: V scale of position lane & 31
  const float* scbase =
      (lane < PSTEP ? k_scale : v_scale) + (size_t)ph * Lcap + (lane & 31);
  unsigned char* vt = s_vt[wid];
  float* strip = s_sc[wid];

  float m = -INFINITY, l = 0.f;
  mfma_f32x4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};

  int4v kk[2][KS];
  unsigned int vv[VW][4];  // [word][position]
  float sc = 0.f;
  const int4v zero4 = {0, 0, 0, 0};
  // positions >= end are never loaded (they may be uninitialised): codes and
  // scales past the end are zeros, their scores are set to -inf below
  auto load_step = [&](int pos0) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int pos = pos0 + t * 16 + r;
      const bool ok = pos < end;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        kk[t][ks] = ok ? *reinterpret_cast<const int4v*>(
                             kbase + (size_t)pos * D + ks * 64)
                       : zero4;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pos = pos0 + va + i;
      const bool ok = pos < end;
      const unsigned char* vp = vbase + (size_t)pos * D;
      if constexpr (VW == 4) {
        const int4v x = ok ? *reinterpret_cast<const int4v*>(vp) : zero4;
#pragma unroll
        for (int w = 0; w < 4; ++w) vv[w][i] = (unsigned int)x[w];
      } else {
        const int2v z2 = {0, 0};
        const int2v x = ok ? *reinterpret_cast<const int2v*>(vp) : z2;
        vv[0][i] = (unsigned int)x[0];
        vv[1][i] = (unsigned int)x[1];
      }
    }
    sc = (pos0 + (lane & 31) < end) ? scbase[pos0] : 0.f;
  };

  int pos0 = start + wid * PSTEP;
  if (pos0 < end) load_step(pos0);
  // wave-uniform trip count
  for (; pos0 < end; pos0 += PNW * PSTEP) {
    // V registers -> transposed byte image, scales -> strip. LDS serves one
    // wave's instructions in order, so the reads of the previous step are
    // done; the barrier keeps the compiler from moving accesses across it.
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int w = 0; w < VW; ++w) {
      unsigned int t4[4];
      transpose4x4(vv[w], t4);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int d = vcb * (D / 8) + w * 4 + b;
        *reinterpret_cast<unsigned int*>(vt + d * VT8_STRIDE +
                                         (d >> 4) * VT8_SKEW + 4 * vq) = t4[b];
      }
    }
    strip[lane] = sc;
    __builtin_amdgcn_wave_barrier();
    // scales of positions g*4 + e of tile t: K at strip[t*16 ..], V 32 on
    float4v ksc[2], vsc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      ksc[t] = *reinterpret_cast<const float4v*>(strip + t * 16 + g * 4);
      vsc[t] =
          *reinterpret_cast<const float4v*>(strip + PSTEP + t * 16 + g * 4);
    }

    // S^T tiles: rows = positions g*4 + e of tile t, column = sample r
    mfma_f32x4 st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      st[t] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            decode8(kk[t][ks][0], kk[t][ks][1]), frag(qf[ks][0]), st[t], 0, 0,
            0);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            decode8(kk[t][ks][2], kk[t][ks][3]), frag(qf[ks][1]), st[t], 0, 0,
            0);
      }
    }
    // the next step's loads fly under the softmax and the second product
    const int valid_base = pos0 + g * 4;
    const int next = pos0 + PNW * PSTEP;
    if (next < end) load_step(next);

    float s[8];
    bool ok[8];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ok[j] = valid_base + (j >> 2) * 16 + (j & 3) < end;
      // select, never multiply
      s[j] = ok[j] ? st[j >> 2][j & 3] * (scale * ksc[j >> 2][j & 3])
                   : -INFINITY;
      mx = fmaxf(mx, s[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
    const float mn = fmaxf(m, mx);
    const float ms = (mn == -INFINITY) ? 0.f : mn;
    const float alpha = __expf(m - ms);
    float pv[8];
    float ls = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float pw = ok[j] ? __expf(s[j] - ms) : 0.f;
      ls += pw;
      // the V scale rides in P: one bf16 rounding of the product
      pv[j] = ok[j] ? pw * vsc[j >> 2][j & 3] : 0.f;
    }
    // l stays a per-lane partial sum (alpha is the same in the 4 lanes of a
    // sample); it is reduced once after the walk
    l = l * alpha + ls;
    m = mn;
    union { unsigned int u[4]; short8v v; } pf;
#pragma unroll
    for (int j = 0; j < 4; ++j) pf.u[j] = cvt_pk_bf16(pv[2 * j], pv[2 * j + 1]);

    // O^T += V^T P^T
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const int2v a = *reinterpret_cast<const int2v*>(
          vt + (db * 16 + r) * VT8_STRIDE + db * VT8_SKEW + g * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[db][e] *= alpha;
      acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          decode8(a[0], a[1]), frag(pf.v), acc[db], 0, 0, 0);
    }
  }

  // this wave's state -> its own region, over its V image
  store_wave_state<D>(reinterpret_cast<float*>(vt), r, g, acc, m, l);
  __syncthreads();

  merge_waves<D, REGION / 4>(reinterpret_cast<const float*>(s_vt[0]), ws, tid,
                             cg, p, head, ck, h, G, ws_slots);
}

}  // namespace

torch::Tensor decode_attn_shared_fp8(
    torch::Tensor qkv, torch::Tensor k_prefix, torch::Tensor v_prefix,
    torch::Tensor k_prefix_scale, torch::Tensor v_prefix_scale,
    torch::Tensor prefix_lens, torch::Tensor k_cache, torch::Tensor v_cache,
    torch::Tensor seq_lens, long group, double scale, long max_prefix_len,
    long num_splits) {
  const SharedDims s = check_decode_attn_shared(
      "decode_attn_shared_fp8", qkv, k_prefix, v_prefix, prefix_lens, k_cache,
      v_cache, seq_lens, group, max_prefix_len, num_splits,
      torch::kFloat8_e4m3fn, {&k_prefix_scale, &v_prefix_scale});
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 &&
                  k_cache.scalar_type() == torch::kBFloat16 &&
                  v_cache.scalar_type() == torch::kBFloat16,
              "decode_attn_shared_fp8: qkv, k_cache and v_cache must be bf16 "
              "(only the prefix is fp8)");
  TORCH_CHECK(k_prefix_scale.scalar_type() == torch::kFloat &&
                  v_prefix_scale.scalar_type() == torch::kFloat,
              "decode_attn_shared_fp8: prefix scales must be fp32");
  TORCH_CHECK(k_prefix_scale.dim() == 3 && k_prefix_scale.size(0) == s.P &&
                  k_prefix_scale.size(1) == s.h &&
                  k_prefix_scale.size(2) == s.Lcap &&
                  v_prefix_scale.sizes() == k_prefix_scale.sizes(),
              "decode_attn_shared_fp8: prefix scales must be [P, h, Lcap]");
  TORCH_CHECK(aligned16(qkv) && aligned16(k_prefix) && aligned16(v_prefix) &&
                  aligned16(k_cache) && aligned16(v_cache),
              "decode_attn_shared_fp8: qkv, prefix and caches must be 16-byte "
              "aligned");
  auto run = [&](auto d) {
    constexpr int D = decltype(d)::value;
    return launch_shared<D>(
        qkv, prefix_lens, k_cache, v_cache, seq_lens, s, group, max_prefix_len,
        num_splits, (float)scale,
        [&](dim3 grid, hipStream_t stream, float* wsp, int ncg, int chunk,
            int slots) {
          hipLaunchKernelGGL(
              decode_prefix_fp8_kernel<D>, grid, dim3(PNW * WAVE), 0, stream,
              (const short*)qkv.data_ptr(),
              (const unsigned char*)k_prefix.data_ptr(),
              (const unsigned char*)v_prefix.data_ptr(),
              k_prefix_scale.data_ptr<float>(),
              v_prefix_scale.data_ptr<float>(), prefix_lens.data_ptr<int>(),
              wsp, (int)s.h, (int)group, ncg, (int)s.Lcap, chunk, slots,
              (float)scale);
        });
  };
  return s.D == 64 ? run(std::integral_constant<int, 64>{})
                   : run(std::integral_constant<int, 128>{});
}

