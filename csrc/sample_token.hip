// Fused on-device sampler, gfx950: one launch turns a row of logits into the
// next token and updates the generation state (ids_buf, unfinished,
// next_tokens). Replaces the decode loop's sampling tail (logits processors,
// softmax, topk, a full-vocabulary sort, top-p cut, draw, where/cat/ne/and).
//
// One 1024-thread workgroup per row holds the whole row in registers
// (token v lives in thread v % 1024, slot v / 1024), so every pass below is
// register-only plus ONE block reduction:
//   * top-k threshold: bisect over the ordered bit pattern of the
//     non-negative probabilities for the largest t with count(p >= t) >= k;
//   * top-p threshold: bisect for the smallest t whose strictly-greater mass
//     is <= top_p (tie-inclusive: every token equal to the last kept one is
//     kept, where a sort keeps an arbitrary subset of a tie);
//   * draw: bisect over the token index for the first token in vocabulary
//     order whose inclusive kept mass reaches u * kept_mass.
// No sort, no workspace, no floating-point atomics: every mass is reduced in
// a fixed order (four chains per thread, a DPP tree per wave, then the 16
// wave totals in order), so the
// result is bit-reproducible, and a sum over a superset is never smaller,
// which is what makes the three bisections valid.
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace {

constexpr int BLOCK = 1024;
constexpr int NW = BLOCK / WAVE;
constexpr int MAX_V = 65536;
constexpr int ONE_BITS = 0x3f800000;  // bit pattern of 1.0f

struct SampleArgs {
  const void* logits;
  long logits_stride;  // elements between rows
  long* ids_buf;
  long ids_stride;
  const int* lens;
  unsigned char* unfinished;
  const float* u;
  long u_stride;
  long* next_tokens;
  int* kept_count;
  float* kept_mass;
  int T, V;
  int greedy;
  float temperature;
  int top_k;
  float top_p;
  float penalty;
  int min_length;
  long eos, pad;
};

struct Lds {
  alignas(16) float red[2][NW];
  unsigned int seen[MAX_V / 32];
};

// Block-wide reductions with one barrier each: results alternate between
// two LDS rows, so a wave can only overwrite a row after every wave has
// passed the barrier that follows the row's last read.
//
// The wave step of the sum runs on DPP (no LDS crossbar round trips): xor 1
// and xor 2 inside quads, two rotations inside each row of 16, then the row
// totals are chained into rows 1 and 3 and into the upper half; lane 63
// ends with the wave total. Lanes a step masks out add 0.
template <int CTRL, int ROW_MASK>
DEV_INLINE float dpp_add(float x) {
  return x + __int_as_float(__builtin_amdgcn_update_dpp(
                 0, __float_as_int(x), CTRL, ROW_MASK, 0xf, false));
}

DEV_INLINE float wave_sum_lane63(float x) {
  x = dpp_add<0xb1, 0xf>(x);   // quad_perm:[1,0,3,2]
  x = dpp_add<0x4e, 0xf>(x);   // quad_perm:[2,3,0,1]
  x = dpp_add<0x124, 0xf>(x);  // row_ror:4
  x = dpp_add<0x128, 0xf>(x);  // row_ror:8
  x = dpp_add<0x142, 0xa>(x);  // row_bcast:15 into rows 1 and 3
  x = dpp_add<0x143, 0xc>(x);  // row_bcast:31 into rows 2 and 3
  return x;
}

// LEAN: the 64-slot kernel has no registers to spare; it takes the plain
// butterfly, reads the wave totals one by one and sums on a single chain.
template <bool LEAN>
DEV_INLINE float block_sum(float x, Lds& s, int& par) {
  if constexpr (LEAN) {
    x = wave_reduce_sum(x);
    if ((threadIdx.x & (WAVE - 1)) == 0) s.red[par][threadIdx.x / WAVE] = x;
    __syncthreads();
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) r += s.red[par][w];
    par ^= 1;
    return r;
  }
  x = wave_sum_lane63(x);
  if ((threadIdx.x & (WAVE - 1)) == WAVE - 1)
    s.red[par][threadIdx.x / WAVE] = x;
  __syncthreads();
  const float4v* t = reinterpret_cast<const float4v*>(s.red[par]);
  float r = 0.f;
#pragma unroll
  for (int w = 0; w < NW / 4; ++w) {
    const float4v q = t[w];
    r += (q[0] + q[1]) + (q[2] + q[3]);
  }
  par ^= 1;
  return r;
}

DEV_INLINE float block_max(float x, Lds& s, int& par) {
  x = wave_reduce_max(x);
  if ((threadIdx.x & (WAVE - 1)) == 0) s.red[par][threadIdx.x / WAVE] = x;
  __syncthreads();
  float r = -INFINITY;
#pragma unroll
  for (int w = 0; w < NW; ++w) r = fmaxf(r, s.red[par][w]);
  par ^= 1;
  return r;
}

// Sum of f(i) over the slots of a thread on independent chains (a single
// chain of ITEMS dependent adds is latency-bound), in a fixed order.
template <int ITEMS, typename F>
DEV_INLINE float slot_sum(F f) {
  constexpr int CHAINS = ITEMS > 50 ? 1 : 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) acc[i % CHAINS] += f(i);
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

template <typename T>
DEV_INLINE float load_logit(const T* p) {
  if constexpr (sizeof(T) == 2) return bf_raw2f(*p);
  else return *p;
}

// Is token i * BLOCK + tid below n = q * BLOCK + r? Written per slot so that
// all but one slot decide on scalars (no 64 lane masks to keep alive).
DEV_INLINE bool slot_below(int i, int q, int r) {
  return i < q || (i == q && (int)threadIdx.x < r);
}

template <typename T, int ITEMS>
__global__ void __launch_bounds__(BLOCK)
sample_token_kernel(SampleArgs a) {
  __shared__ Lds s;
  const int tid = threadIdx.x;
  const long row = blockIdx.x;
  const int V = a.V;
  int par = 0;

  int L = a.lens[row];
  L = L < 0 ? 0 : (L > a.T ? a.T : L);
  long* ids_row = a.ids_buf + row * a.ids_stride;

  // history bitmap for the repetition penalty (a set: duplicates are free)
  const bool penalise = a.penalty != 1.0f;
  if (penalise) {
    for (int j = tid; j < MAX_V / 32; j += BLOCK) s.seen[j] = 0u;
    __syncthreads();
    for (int j = tid; j < L; j += BLOCK) {
      const long id = ids_row[j];
      if (id >= 0 && id < V) atomicOr(&s.seen[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
  }

  // 1-3) load, min length, repetition penalty, temperature
  const T* lrow = reinterpret_cast<const T*>(a.logits) + row * a.logits_stride;
  const bool mask_eos = L < a.min_length;
  const int vq = V / BLOCK, vr = V % BLOCK;
  float p[ITEMS];  // logits, then probabilities; slots past V: -inf, then 0
  // branch-free so that all loads of a thread are in flight together; a
  // slot past V re-reads the row's last element and is masked afterwards
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int v = i * BLOCK + tid;
    p[i] = load_logit<T>(lrow + (slot_below(i, vq, vr) ? v : V - 1));
  }
  const int eos_slot = mask_eos && a.eos >= 0 && a.eos < V &&
                               (int)(a.eos % BLOCK) == tid
                           ? (int)(a.eos / BLOCK) : -1;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int v = i * BLOCK + tid;
    const bool valid = slot_below(i, vq, vr);
    float x = (valid && i != eos_slot) ? p[i] : -INFINITY;
    if (penalise) {  // uniform branch
      const int vc = valid ? v : V - 1;
      const bool hit = (s.seen[vc >> 5] >> (vc & 31)) & 1u;
      const float y = x < 0.f ? x * a.penalty : x / a.penalty;
      x = hit ? y : x;
    }
    p[i] = x;
  }

  long pick;
  float mass = 0.f;
  int count = 1;
  if (a.greedy) {
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) m = fmaxf(m, p[i]);
    m = block_max(m, s, par);
    float best = -1e9f;  // max of -index = first index; V <= 65536 is exact
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      const int v = i * BLOCK + tid;
      if (p[i] == m) best = fmaxf(best, -(float)v);
    }
    best = block_max(best, s, par);
    // a NaN row has no arg-max and an all -inf row matches its padding:
    // the token must stay a valid index for the next embedding lookup
    pick = best > -1e9f ? (long)(-best) : 0;
    pick = pick < V ? pick : V - 1;
  } else {
    // 3-4) temperature, softmax
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      if (a.temperature != 1.0f) p[i] = p[i] / a.temperature;
      m = fmaxf(m, p[i]);
    }
    m = block_max(m, s, par);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      p[i] = expf(p[i] - m);  // slots past V: exp(-inf) = 0
      sum += p[i];
    }
    sum = block_sum<(ITEMS > 50)>(sum, s, par);
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) p[i] = p[i] / sum;

    // Probabilities are >= +0, so their bit patterns order as signed ints.
    // A padding slot holds 0: it passes no test with t >= 1 and adds no mass.
    // 5) top-k: largest t with count(p >= t) >= k
    int t_k = 0;
    if (a.top_k > 0 && a.top_k < V) {
      const float k = (float)a.top_k;  // counts <= 65536 are exact in fp32
      int lo = 0, hi = ONE_BITS + 1;
      while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        const float c = block_sum<(ITEMS > 50)>(slot_sum<ITEMS>([&](int i) {
          return (__float_as_int(p[i]) >= mid) ? 1.f : 0.f; }), s, par);
        if (c >= k) lo = mid; else hi = mid;
        // exactly k tokens reach mid: it separates the same set as the k-th
        // largest value itself would
        if (c == k) break;
      }
      t_k = lo;
    }
    // 6) top-p on the unrenormalised top-k survivors: smallest t whose
    // strictly-greater mass M(t + 1) is <= top_p
    int thr = t_k;
    if (a.top_p < 1.0f) {
      const float top_p = fmaxf(a.top_p, 0.f);
      int lo = t_k > 0 ? t_k - 1 : -1, hi = ONE_BITS + 1;  // M(hi) = 0
      // below t_k the mass no longer grows, so the search starts there
      while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        const float mm = block_sum<(ITEMS > 50)>(slot_sum<ITEMS>([&](int i) {
          return (__float_as_int(p[i]) >= mid) ? p[i] : 0.f; }), s, par);
        if (mm <= top_p) hi = mid; else lo = mid;
      }
      const int t_p = hi > 0 ? hi - 1 : 0;
      thr = t_p > t_k ? t_p : t_k;
    }
    // drop everything that is not kept; zero-probability tokens are never
    // kept, so none can be drawn
    float c = 0.f;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      const bool keep = __float_as_int(p[i]) >= thr && p[i] > 0.f;
      p[i] = keep ? p[i] : 0.f;
      c += keep ? 1.f : 0.f;
    }
    count = (int)block_sum<(ITEMS > 50)>(c, s, par);
    // 7) draw: S(v) = kept mass of tokens <= v, always by the same
    // reduction, so S(V-1) is kept_mass itself and S is monotone
    mass = block_sum<(ITEMS > 50)>(slot_sum<ITEMS>([&](int i) { return p[i]; }), s, par);
    const float uu = a.u[row * a.u_stride + (L < a.T ? L : a.T - 1)];
    const float target = fminf(uu * mass, mass);
    int lo = -1, hi = V - 1;
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      const int mq = (mid + 1) / BLOCK, mr = (mid + 1) % BLOCK;
      const float sv = block_sum<(ITEMS > 50)>(slot_sum<ITEMS>([&](int i) {
        return slot_below(i, mq, mr) ? p[i] : 0.f; }), s, par);
      if (sv >= target && sv > 0.f) hi = mid; else lo = mid;
    }
    pick = hi;
  }

  // 8) finish
  if (tid == 0) {
    const bool unf = a.unfinished[row] != 0;
    const long tok = unf ? pick : a.pad;
    if (L < a.T) ids_row[L] = tok;
    a.next_tokens[row] = tok;
    a.unfinished[row] = (unf && tok != a.eos) ? 1 : 0;
    a.kept_count[row] = count;
    a.kept_mass[row] = mass;
  }
}

template <typename T>
void launch(const SampleArgs& a, long B, hipStream_t stream) {
#define SAMPLE_LAUNCH(N)                                                   \
  hipLaunchKernelGGL((sample_token_kernel<T, N>), dim3(B), dim3(BLOCK), 0, \
                     stream, a)
  if (a.V <= 4 * BLOCK) SAMPLE_LAUNCH(4);
  else if (a.V <= 16 * BLOCK) SAMPLE_LAUNCH(16);
  else if (a.V <= 50 * BLOCK) SAMPLE_LAUNCH(50);
  else SAMPLE_LAUNCH(64);
#undef SAMPLE_LAUNCH
}

}  // namespace

std::vector<torch::Tensor> sample_token(
    torch::Tensor logits, torch::Tensor ids_buf, torch::Tensor lens,
    torch::Tensor unfinished, torch::Tensor u, torch::Tensor next_tokens,
    bool greedy, double temperature, long top_k, double top_p,
    double repetition_penalty, long min_length, long eos_token_id,
    long pad_token_id) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1,
              "sample_token: logits must be a CUDA [B, V] tensor with unit "
              "inner stride");
  TORCH_CHECK(logits.scalar_type() == torch::kFloat ||
                  logits.scalar_type() == torch::kBFloat16,
              "sample_token: logits must be fp32 or bf16");
  const long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(B >= 1 && V >= 1 && V <= MAX_V,
              "sample_token: V must be in [1, 65536]");
  TORCH_CHECK(ids_buf.is_cuda() && ids_buf.scalar_type() == torch::kLong &&
                  ids_buf.dim() == 2 && ids_buf.size(0) == B &&
                  ids_buf.size(1) >= 1 && ids_buf.stride(1) == 1,
              "sample_token: ids_buf must be int64 [B, T]");
  const long T = ids_buf.size(1);
  TORCH_CHECK(lens.is_cuda() && lens.scalar_type() == torch::kInt &&
                  lens.dim() == 1 && lens.size(0) == B && lens.is_contiguous(),
              "sample_token: lens must be int32 [B]");
  TORCH_CHECK(unfinished.is_cuda() &&
                  (unfinished.scalar_type() == torch::kBool ||
                   unfinished.scalar_type() == torch::kByte) &&
                  unfinished.dim() == 1 && unfinished.size(0) == B &&
                  unfinished.is_contiguous(),
              "sample_token: unfinished must be bool or uint8 [B]");
  TORCH_CHECK(u.is_cuda() && u.scalar_type() == torch::kFloat &&
                  u.dim() == 2 && u.size(0) == B && u.size(1) == T &&
                  u.stride(1) == 1,
              "sample_token: u must be fp32 [B, T]");
  TORCH_CHECK(next_tokens.is_cuda() &&
                  next_tokens.scalar_type() == torch::kLong &&
                  next_tokens.numel() == B && next_tokens.is_contiguous(),
              "sample_token: next_tokens must be int64 [B, 1]");
  TORCH_CHECK(temperature > 0.0, "sample_token: temperature must be > 0");
  TORCH_CHECK(repetition_penalty > 0.0,
              "sample_token: repetition_penalty must be > 0");

  auto kept_count = torch::empty({B}, logits.options().dtype(torch::kInt));
  auto kept_mass = torch::empty({B}, logits.options().dtype(torch::kFloat));

  SampleArgs a;
  a.logits = logits.data_ptr();
  a.logits_stride = logits.stride(0);
  a.ids_buf = ids_buf.data_ptr<long>();
  a.ids_stride = ids_buf.stride(0);
  a.lens = lens.data_ptr<int>();
  a.unfinished = reinterpret_cast<unsigned char*>(unfinished.data_ptr());
  a.u = u.data_ptr<float>();
  a.u_stride = u.stride(0);
  a.next_tokens = next_tokens.data_ptr<long>();
  a.kept_count = kept_count.data_ptr<int>();
  a.kept_mass = kept_mass.data_ptr<float>();
  a.T = (int)T;
  a.V = (int)V;
  a.greedy = greedy ? 1 : 0;
  a.temperature = (float)temperature;
  a.top_k = (int)std::min<long>(std::max<long>(top_k, 0), V);
  a.top_p = (float)top_p;
  a.penalty = (float)repetition_penalty;
  a.min_length = (int)std::min<long>(std::max<long>(min_length, 0), 1L << 30);
  a.eos = eos_token_id;
  a.pad = pad_token_id;

  auto stream = at::hip::getCurrentHIPStream();
  if (logits.scalar_type() == torch::kFloat)
    launch<float>(a, B, stream);
  else
    launch<unsigned short>(a, B, stream);
  return {kept_count, kept_mass};
}
