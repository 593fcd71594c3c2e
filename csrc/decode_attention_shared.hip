// Decode attention for G samples of one prompt (num_return_sequences = G),
// gfx950. The prompt's K/V are stored ONCE per prompt ([P, h, Lcap, D]) and
// read once per step for all of its samples; only the tokens a sample
// generated itself live in a per-row cache ([B, h, Scap, D], B = P*G).
//
// Three launches, no counters, flags or atomics:
//   1. prefix  (decode_prefix_kernel, this file): MFMA, one workgroup per
//      (prompt, head, column group of <= 16 samples, chunk of the prefix);
//   2. suffix  (decode_attn_kernel<D, true>, decode_attention_kernel.h): the
//      VALU walk over each row's own tokens plus the new token, which it
//      also appends;
//   3. merge   (decode_merge_kernel, decode_common.h).
// Every pass writes fp32 (acc[D], m, l, pad) into its slot of one workspace
// [B*h, 1 + chunks, D + 4]: slot 0 the suffix (it holds the new token, so its
// max is finite), slots 1.. the prefix chunks (an empty one: m = -inf, l = 0).
//
// Prefix pass. With G query rows per K/V tile the work is G flop/byte, so it
// runs on the matrix cores, v_mfma_f32_16x16x32_bf16 twice per tile:
//
//   S^T = K Q^T   A = K rows straight from global memory (16-byte loads of
//                 the stored layout: row = position lane & 15, k = d slice
//                 (lane >> 4)*8), B = Q^T, D/32 fragments held in registers.
//                 A lane then owns scores of ONE sample (column lane & 15):
//                 the softmax state (m, l) is a per-lane scalar.
//   O^T = V^T P^T B = two 16-position score tiles of the step, handed over
//                 in registers as one 32-deep fragment; A = V^T from a
//                 transposed LDS image. Accumulator rows are d, the column
//                 is the sample: the online rescale is per-lane again.
//
// The contraction index of the second product is permuted: slot j of lane
// group g (k = g*8 + j) is position g*4 + j of the first score tile for
// j < 4 and 16 + g*4 + (j - 4) of the second for j >= 4, which is exactly
// what the lane holds after the first product. The V image uses the same
// order for its columns, so a lane's A fragment is ONE 16-byte LDS read.
//
// LDS: per wave a private image Vt[D][32 + 8] bf16 (80-byte rows: 16-byte
// aligned for the b128 reads, and the 8-short pad spreads the 16 rows a
// quarter-wave reads over the banks). It is built with 4-byte writes: a lane
// loads the SAME 8 channels of two positions that are neighbours in the
// permuted order and writes 8 (lo, hi) pairs. The waves of a workgroup split
// the chunk's positions 32 at a time, each with its own (m, l, acc) and its
// own image: no workgroup barrier in the walk. At the end every wave leaves
// its state in its own region and the workgroup merges them in wave order.
#include "decode_attention_shared_common.h"

namespace {

constexpr int VT_STRIDE = 40;  // shorts per row of the transposed V image

// grid (P*h*ncg, chunks), 256 threads.
// ws: fp32 [B*h, ws_slots, D+4]; chunk ck goes to slot 1 + ck.
template <int D>
__global__ __launch_bounds__(PNW * WAVE) void decode_prefix_kernel(
    const short* __restrict__ qkv,          // [B, 1, h, 3, D] bf16
    const short* __restrict__ k_prefix,     // [P, h, Lcap, D] bf16
    const short* __restrict__ v_prefix,
    const int* __restrict__ prefix_lens,    // [P]
    float* __restrict__ ws, int h, int G, int ncg, int Lcap, int chunk,
    int ws_slots, float scale) {
  constexpr int KB = D / 32;   // k blocks of K Q^T
  constexpr int DB = D / 16;   // row blocks of O^T
  constexpr int SROW = D + 4;  // floats per sample of a wave's final state
  static_assert(COLS * SROW * 4 <= D * VT_STRIDE * 2,
                "the final state reuses the wave's V image");
  __shared__ __attribute__((aligned(16))) short s_vt[PNW][D * VT_STRIDE];

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
  // Q^T: column = sample; columns >= G are zero and never stored
  const int smp = cg * COLS + r;
  const bool q_ok = smp < G;
  short8v qf[KB];
  {
    const short* qp =
        qkv + ((size_t)(p * G + (q_ok ? smp : 0)) * h + head) * 3 * D + g * 8;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
      qf[kb] = q_ok ? *reinterpret_cast<const short8v*>(qp + kb * 32) : zero8;
  }

  const short* kbase = k_prefix + (size_t)ph * Lcap * D;
  const short* vbase = v_prefix + (size_t)ph * Lcap * D;
  // V image items of this lane: item = i*64 + lane -> column pair lane & 15
  // (columns 2*pp, 2*pp + 1 = positions va, va + 1), channels
  // (i*4 + g)*8 .. + 8
  const int pp = lane & 15;
  const int va = perm_pos(2 * pp);
  short* vt = s_vt[wid];

  float m = -INFINITY, l = 0.f;
  mfma_f32x4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};

  short8v kk[2][KB], v0[KB], v1[KB];
  // positions >= end are never loaded (they may be uninitialised): K rows
  // and V entries past the end are zeros, their scores are set to -inf below
  auto load_step = [&](int pos0) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int pos = pos0 + t * 16 + r;
      const bool ok = pos < end;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        kk[t][kb] = ok ? *reinterpret_cast<const short8v*>(
                             kbase + (size_t)pos * D + kb * 32 + g * 8)
                       : zero8;
    }
    const bool ok0 = pos0 + va < end, ok1 = pos0 + va + 1 < end;
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      const short* vp = vbase + (size_t)(pos0 + va) * D + (i * 4 + g) * 8;
      v0[i] = ok0 ? *reinterpret_cast<const short8v*>(vp) : zero8;
      v1[i] = ok1 ? *reinterpret_cast<const short8v*>(vp + D) : zero8;
    }
  };

  int pos0 = start + wid * PSTEP;
  if (pos0 < end) load_step(pos0);
  // wave-uniform trip count
  for (; pos0 < end; pos0 += PNW * PSTEP) {
    // V registers -> transposed image. LDS serves one wave's instructions in
    // order, so the reads of the previous step are done; the barrier keeps
    // the compiler from moving accesses across it.
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < KB; ++i) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned int lo = (unsigned short)v0[i][e];
        const unsigned int hi = (unsigned short)v1[i][e];
        *reinterpret_cast<unsigned int*>(
            vt + ((i * 4 + g) * 8 + e) * VT_STRIDE + 2 * pp) = lo | (hi << 16);
      }
    }
    __builtin_amdgcn_wave_barrier();

    // S^T tiles: rows = positions g*4 + e of tile t, column = sample r
    mfma_f32x4 st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      st[t] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            frag(kk[t][kb]), frag(qf[kb]), st[t], 0, 0, 0);
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
      s[j] = ok[j] ? st[j >> 2][j & 3] * scale : -INFINITY;
      mx = fmaxf(mx, s[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
    const float mn = fmaxf(m, mx);
    const float ms = (mn == -INFINITY) ? 0.f : mn;
    const float alpha = __expf(m - ms);
    float pw[8];
    float ls = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pw[j] = ok[j] ? __expf(s[j] - ms) : 0.f;
      ls += pw[j];
    }
    // l stays a per-lane partial sum (alpha is the same in the 4 lanes of a
    // sample); it is reduced once after the walk
    l = l * alpha + ls;
    m = mn;
    union { unsigned int u[4]; short8v v; } pf;
#pragma unroll
    for (int j = 0; j < 4; ++j) pf.u[j] = cvt_pk_bf16(pw[2 * j], pw[2 * j + 1]);

    // O^T += V^T P^T
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const short8v a = *reinterpret_cast<const short8v*>(
          vt + (db * 16 + r) * VT_STRIDE + g * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[db][e] *= alpha;
      acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(a), frag(pf.v),
                                                        acc[db], 0, 0, 0);
    }
  }

  // this wave's state -> its own region, over its V image
  store_wave_state<D>(reinterpret_cast<float*>(vt), r, g, acc, m, l);
  __syncthreads();

  // the regions are the images: D * VT_STRIDE / 2 floats apart
  merge_waves<D, D * VT_STRIDE / 2>(reinterpret_cast<const float*>(s_vt[0]),
                                    ws, tid, cg, p, head, ck, h, G, ws_slots);
}

}  // namespace

torch::Tensor decode_attn_shared(torch::Tensor qkv, torch::Tensor k_prefix,
                                 torch::Tensor v_prefix,
                                 torch::Tensor prefix_lens,
                                 torch::Tensor k_cache, torch::Tensor v_cache,
                                 torch::Tensor seq_lens, long group,
                                 double scale, long max_prefix_len,
                                 long num_splits) {
  const SharedDims s = check_decode_attn_shared(
      "decode_attn_shared", qkv, k_prefix, v_prefix, prefix_lens, k_cache,
      v_cache, seq_lens, group, max_prefix_len, num_splits, torch::kBFloat16);
  auto run = [&](auto d) {
    constexpr int D = decltype(d)::value;
    return launch_shared<D>(
        qkv, prefix_lens, k_cache, v_cache, seq_lens, s, group, max_prefix_len,
        num_splits, (float)scale,
        [&](dim3 grid, hipStream_t stream, float* wsp, int ncg, int chunk,
            int slots) {
          hipLaunchKernelGGL(
              decode_prefix_kernel<D>, grid, dim3(PNW * WAVE), 0, stream,
              (const short*)qkv.data_ptr(), (const short*)k_prefix.data_ptr(),
              (const short*)v_prefix.data_ptr(), prefix_lens.data_ptr<int>(),
              wsp, (int)s.h, (int)group, ncg, (int)s.Lcap, chunk, slots,
              (float)scale);
        });
  };
  return s.D == 64 ? run(std::integral_constant<int, 64>{})
                   : run(std::integral_constant<int, 128>{});
}
