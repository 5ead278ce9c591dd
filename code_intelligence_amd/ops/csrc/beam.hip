// K11 beam search: the per-word selection of fastai's
// LanguageLearner.beam_search as two launches. topk_logprobs turns a row of
// logits into its k largest log-probabilities (descending, ties to the lower
// vocabulary index); beam_select forms the B*k candidate scores
// score[b] - lp[b][j], sorts them (ascending, ties to the lower flat index) and
// writes the best beam_sz with their parent row and token. No atomics; every
// reduction runs in an order fixed by the shape alone.
#include "common.h"

#include <hip/hip_fp16.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <type_traits>

namespace ci {

template <> struct Cvt<__half> {
  static __device__ __forceinline__ float load(const __half* p) {
    return __half2float(*p);
  }
  static __device__ __forceinline__ void store(__half* p, float v) {
    *p = __float2half(v);
  }
};

constexpr int kTopkThreads = 256;
constexpr int kTopkWaves = kTopkThreads / kWave;
constexpr int kTopkMaxSegs = 1024;     // segments per row (LDS)
constexpr int kTopkMaxK = 64;
constexpr int kSelThreads = 1024;
constexpr int kSelMaxN = 16384;        // candidates: 128 KB of 64-bit keys

// ---- top-k -----------------------------------------------------------------
// (value, index) pairs; index < 0 is "nothing". A strict total order over
// pairs with distinct indices: larger value first, then the lower index.
static __device__ __forceinline__ bool topk_better(float v1, int i1, float v2,
                                                   int i2) {
  return i1 >= 0 && (i2 < 0 || v1 > v2 || (v1 == v2 && i1 < i2));
}

static __device__ __forceinline__ void topk_wave_best(float& v, int& i) {
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, kWave);
    const int oi = __shfl_xor(i, off, kWave);
    if (topk_better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// (m, s) = (max, sum exp(l - max)) of two disjoint sets. The products and the
// sum are rounded separately, so both partners of a butterfly get the same
// bits.
static __device__ __forceinline__ void lse_merge(float& m, float& s, float om,
                                                 float os) {
  const float nm = fmaxf(m, om);
  const float a = m == -INFINITY ? 0.f : __fmul_rn(s, expf(m - nm));
  const float b = om == -INFINITY ? 0.f : __fmul_rn(os, expf(om - nm));
  s = __fadd_rn(a, b);
  m = nm;
}

// One workgroup per row. The row is cut into nseg <= 1024 segments of
// seg_len = 64*VEC*iters consecutive entries; wave s % 4 owns segment s and
// reads it 64*VEC entries at a time, lane l taking entries l*VEC.. of each
// chunk. Pass 1 is the only read from HBM: every lane keeps a running
// (max, sum exp) over all its entries (unk included: log_softmax comes before
// the exclusion) and each segment leaves its best candidate (entry != unk) in
// LDS. Then k rounds: a block arg-max over the segment bests, thread 0 emits
// the winner, and one wave rescans the winner's segment for its best entry
// that comes after the winner in (value desc, index asc) order. Everything
// emitted from that segment so far comes at or before the winner, so no list
// of emitted entries is kept. Selection compares the raw logits only.
template <typename T, int VEC>
__global__ __launch_bounds__(kTopkThreads) void topk_logprobs_kernel(
    const T* __restrict__ logits, long row_stride,   // (B,V), unit stride in V
    float* __restrict__ out_vals,                    // (B,k)
    int64_t* __restrict__ out_idx,                   // (B,k)
    int V, int k, int iters, int nseg, int unk) {
  __shared__ float s_max[kTopkMaxSegs];
  __shared__ int s_arg[kTopkMaxSegs];
  __shared__ float s_lm[kTopkWaves], s_ls[kTopkWaves];
  __shared__ float s_rv[kTopkWaves];
  __shared__ int s_ri[kTopkWaves];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const long b = blockIdx.x;
  const T* row = logits + b * row_stride;
  constexpr int CH = kWave * VEC;
  const long seg_len = (long)CH * iters;

  auto load = [&](long e0, float* l) {
    if (VEC > 1 && e0 + VEC <= V) { ldv<T, VEC>(row + e0, l); return; }
    #pragma unroll
    for (int i = 0; i < VEC; ++i)
      l[i] = e0 + i < V ? ld(row + e0 + i) : -INFINITY;
  };

  // pass 1
  float m = -INFINITY, s = 0.f;
  for (int seg = wave; seg < nseg; seg += kTopkWaves) {
    float bv = -INFINITY;
    int bi = -1;
    for (int it = 0; it < iters; ++it) {
      const long e0 = (long)seg * seg_len + (long)it * CH + lane * VEC;
      if (e0 < V) {
        float l[VEC];
        load(e0, l);
        float cm = l[0];
        #pragma unroll
        for (int i = 1; i < VEC; ++i) cm = fmaxf(cm, l[i]);
        if (cm > m) { s = __fmul_rn(s, expf(m - cm)); m = cm; }
        #pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const long e = e0 + i;
          if (e < V) {
            if (l[i] > -INFINITY) s += expf(l[i] - m);
            if (e != unk && (bi < 0 || l[i] > bv)) { bv = l[i]; bi = (int)e; }
          }
        }
      }
    }
    topk_wave_best(bv, bi);
    if (lane == 0) { s_max[seg] = bv; s_arg[seg] = bi; }
  }
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
    lse_merge(m, s, __shfl_xor(m, off, kWave), __shfl_xor(s, off, kWave));
  if (lane == 0) { s_lm[wave] = m; s_ls[wave] = s; }
  __syncthreads();
  m = s_lm[0];
  s = s_ls[0];
  for (int w = 1; w < kTopkWaves; ++w) lse_merge(m, s, s_lm[w], s_ls[w]);
  const float lse = m + logf(s);

  for (int r = 0; r < k; ++r) {
    float bv = -INFINITY;
    int bi = -1;
    for (int seg = threadIdx.x; seg < nseg; seg += kTopkThreads) {
      const float v = s_max[seg];
      const int i = s_arg[seg];
      if (topk_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    topk_wave_best(bv, bi);
    if (lane == 0) { s_rv[wave] = bv; s_ri[wave] = bi; }
    __syncthreads();
    bv = s_rv[0];
    bi = s_ri[0];
    for (int w = 1; w < kTopkWaves; ++w)
      if (topk_better(s_rv[w], s_ri[w], bv, bi)) { bv = s_rv[w]; bi = s_ri[w]; }
    // the host guarantees k candidates, so bi >= 0 unless the row holds NaNs;
    // the clamp keeps the id a valid vocabulary index even then
    bi = min(max(bi, 0), V - 1);
    if (threadIdx.x == 0) {
      out_vals[b * k + r] = bv - lse;
      out_idx[b * k + r] = bi;
    }
    const int seg = (int)(bi / seg_len);             // block-uniform, < nseg
    if (wave == seg % kTopkWaves) {
      float nv = -INFINITY;
      int ni = -1;
      for (int it = 0; it < iters; ++it) {
        const long e0 = (long)seg * seg_len + (long)it * CH + lane * VEC;
        if (e0 < V) {
          float l[VEC];
          load(e0, l);
          #pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const long e = e0 + i;
            const bool after = l[i] < bv || (l[i] == bv && e > bi);
            if (e < V && e != unk && after && (ni < 0 || l[i] > nv)) {
              nv = l[i];
              ni = (int)e;
            }
          }
        }
      }
      topk_wave_best(nv, ni);
      if (lane == 0) { s_max[seg] = nv; s_arg[seg] = ni; }
    }
    __syncthreads();
  }
}

void topk_logprobs(at::Tensor logits, long k, long unk, at::Tensor out_vals,
                   at::Tensor out_idx) {
  CI_CHECK_CUDA(logits); CI_CHECK_CUDA(out_vals); CI_CHECK_CUDA(out_idx);
  CI_CHECK_CONTIG(out_vals); CI_CHECK_CONTIG(out_idx);
  TORCH_CHECK(logits.dim() == 2, "logits must be (B,V)");
  const long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(B > 0 && V > 0, "topk_logprobs: empty input");
  TORCH_CHECK(V <= INT_MAX, "topk_logprobs: V exceeds INT_MAX");
  TORCH_CHECK(V == 1 || logits.stride(1) == 1,
              "logits must have unit stride along V");
  TORCH_CHECK(logits.stride(0) >= 0, "logits row stride must be non-negative");
  TORCH_CHECK(unk >= -1 && unk < V, "unk must be in [-1, V)");
  TORCH_CHECK(k >= 1 && k <= kTopkMaxK, "k must be in [1, ", kTopkMaxK, "]");
  TORCH_CHECK(k <= V - (unk >= 0 ? 1 : 0),
              "k exceeds the number of candidates in a row");
  TORCH_CHECK(out_vals.scalar_type() == at::ScalarType::Float &&
              out_vals.numel() == B * k, "out_vals must be fp32 (B,k)");
  TORCH_CHECK(out_idx.scalar_type() == at::ScalarType::Long &&
              out_idx.numel() == B * k, "out_idx must be int64 (B,k)");
  const long rs = logits.stride(0);
  auto run = [&](auto tag) {
    using scalar_t = typename decltype(tag)::type;
    auto launch = [&](auto vec) {
      constexpr int VEC = decltype(vec)::value;
      constexpr long CH = kWave * VEC;
      const long iters = std::max<long>(1, (V + CH * kTopkMaxSegs - 1) /
                                               (CH * kTopkMaxSegs));
      const long seg_len = CH * iters;
      const long nseg = (V + seg_len - 1) / seg_len;
      hipLaunchKernelGGL((topk_logprobs_kernel<scalar_t, VEC>), dim3(B),
          dim3(kTopkThreads), 0, stream(),
          reinterpret_cast<const scalar_t*>(logits.data_ptr()), rs,
          out_vals.data_ptr<float>(), out_idx.data_ptr<int64_t>(), (int)V,
          (int)k, (int)iters, (int)nseg, (int)unk);
    };
    // 16-B packets need every row 16-B aligned
    constexpr int PK = 16 / sizeof(scalar_t);
    if (reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0 &&
        (B == 1 || rs % PK == 0))
      launch(std::integral_constant<int, PK>{});
    else
      launch(std::integral_constant<int, 1>{});
  };
  switch (logits.scalar_type()) {
    case at::ScalarType::Float: run(std::common_type<float>{}); break;
    case at::ScalarType::BFloat16:
      run(std::common_type<__hip_bfloat16>{}); break;
    case at::ScalarType::Half: run(std::common_type<__half>{}); break;
    default:
      TORCH_CHECK(false, "topk_logprobs: unsupported dtype ",
                  logits.scalar_type());
  }
}

// ---- select ----------------------------------------------------------------
// One workgroup. Candidate i = b*k + j gets the 64-bit key
// (order-preserving bits of the fp32 score) << 32 | i, so ascending keys are
// ascending scores with ties to the lower flat index. The keys are sorted by a
// bitonic network in LDS, padded to npad (a power of two) with all-ones keys
// that sort last; the first nout are written out.
static __device__ __forceinline__ float beam_score(const float* scores,
                                                   const float* vals, int i,
                                                   int k) {
  return __fsub_rn(scores[i / k], vals[i]);
}

__global__ __launch_bounds__(kSelThreads) void beam_select_kernel(
    const float* __restrict__ scores,          // (B)
    const float* __restrict__ vals,            // (B,k)
    const int64_t* __restrict__ idx,           // (B,k)
    int N, int k, int npad, int nout,
    float* __restrict__ out_scores, long score_stride,
    int64_t* __restrict__ out_parent, long parent_stride,
    int64_t* __restrict__ out_token, long token_stride) {
  extern __shared__ __align__(16) unsigned long long s_keys[];   // npad
  for (int i = threadIdx.x; i < npad; i += kSelThreads) {
    unsigned long long key = ~0ull;
    if (i < N) {
      // + 0 folds -0 into +0: equal scores must have equal keys
      const unsigned u = __float_as_uint(beam_score(scores, vals, i, k) + 0.f);
      const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      key = ((unsigned long long)ord << 32) | (unsigned)i;
    }
    s_keys[i] = key;
  }
  __syncthreads();
  for (int size = 2; size <= npad; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < npad / 2; t += kSelThreads) {
        const int i = 2 * t - (t & (stride - 1));
        const int j = i + stride;
        const unsigned long long a = s_keys[i], c = s_keys[j];
        const bool up = (i & size) == 0;
        if ((a > c) == up) { s_keys[i] = c; s_keys[j] = a; }
      }
      __syncthreads();
    }
  }
  for (int r = threadIdx.x; r < nout; r += kSelThreads) {
    // nout <= N and the pads sort last, so the low word is a candidate; the
    // clamp keeps the reads in bounds whatever the scores hold
    const int i = (int)min((unsigned)s_keys[r], (unsigned)(N - 1));
    out_scores[r * score_stride] = beam_score(scores, vals, i, k);
    out_parent[r * parent_stride] = i / k;
    out_token[r * token_stride] = idx[i];
  }
}

static bool overlaps(const at::Tensor& a, const at::Tensor& b) {
  auto span = [](const at::Tensor& t) {
    const char* p = static_cast<const char*>(t.data_ptr());
    // inputs are contiguous, outputs 1-D views with a positive stride
    const long last = t.is_contiguous() ? t.numel()
                                        : (t.size(0) - 1) * t.stride(0) + 1;
    return std::make_pair(p, p + last * t.element_size());
  };
  const auto x = span(a), y = span(b);
  return x.first < y.second && y.first < x.second;
}

void beam_select(at::Tensor scores, at::Tensor vals, at::Tensor idx,
                 long beam_sz, at::Tensor out_scores, at::Tensor out_parent,
                 at::Tensor out_token) {
  CI_CHECK_CUDA(scores); CI_CHECK_CUDA(vals); CI_CHECK_CUDA(idx);
  CI_CHECK_CUDA(out_scores); CI_CHECK_CUDA(out_parent);
  CI_CHECK_CUDA(out_token);
  CI_CHECK_CONTIG(scores); CI_CHECK_CONTIG(vals); CI_CHECK_CONTIG(idx);
  TORCH_CHECK(vals.dim() == 2 && vals.scalar_type() == at::ScalarType::Float,
              "vals must be fp32 (B,k)");
  const long B = vals.size(0), k = vals.size(1);
  const long N = B * k;
  TORCH_CHECK(N > 0, "beam_select: empty input");
  TORCH_CHECK(N <= kSelMaxN, "beam_select: B*k = ", N, " exceeds ", kSelMaxN);
  TORCH_CHECK(beam_sz >= 1, "beam_sz must be >= 1");
  TORCH_CHECK(scores.scalar_type() == at::ScalarType::Float &&
              scores.dim() == 1 && scores.size(0) == B,
              "scores must be fp32 (B,)");
  TORCH_CHECK(idx.scalar_type() == at::ScalarType::Long && idx.dim() == 2 &&
              idx.size(0) == B && idx.size(1) == k, "idx must be int64 (B,k)");
  const long nout = std::min(beam_sz, N);
  auto check_out = [&](const at::Tensor& t, at::ScalarType st,
                       const char* name) {
    TORCH_CHECK(t.scalar_type() == st && t.dim() == 1 && t.size(0) == nout &&
                t.stride(0) >= 1,
                name, " must be a (", nout, ",) view of the right dtype with "
                "a positive stride");
  };
  check_out(out_scores, at::ScalarType::Float, "out_scores");
  check_out(out_parent, at::ScalarType::Long, "out_parent");
  check_out(out_token, at::ScalarType::Long, "out_token");
  // the outputs are written while scores, vals and idx are still being read
  TORCH_CHECK(!overlaps(out_scores, scores) && !overlaps(out_scores, vals) &&
              !overlaps(out_parent, idx) && !overlaps(out_token, idx),
              "beam_select: outputs must not overlap the inputs");
  long npad = 2;
  while (npad < N) npad <<= 1;
  const size_t lds = (size_t)npad * sizeof(unsigned long long);
  if (lds > 64 * 1024) {  // above the default dynamic-LDS cap
    static bool attr_set = false;
    if (!attr_set) {
      const hipError_t e = hipFuncSetAttribute(
          reinterpret_cast<const void*>(&beam_select_kernel),
          hipFuncAttributeMaxDynamicSharedMemorySize,
          (int)(kSelMaxN * sizeof(unsigned long long)));
      TORCH_CHECK(e == hipSuccess, "beam_select: cannot reserve ",
                  kSelMaxN * sizeof(unsigned long long), " B of LDS: ",
                  hipGetErrorString(e));
      attr_set = true;
    }
  }
  hipLaunchKernelGGL(beam_select_kernel, dim3(1), dim3(kSelThreads), lds,
      stream(), scores.data_ptr<float>(), vals.data_ptr<float>(),
      idx.data_ptr<int64_t>(), (int)N, (int)k, (int)npad, (int)nout,
      out_scores.data_ptr<float>(), (long)out_scores.stride(0),
      out_parent.data_ptr<int64_t>(), (long)out_parent.stride(0),
      out_token.data_ptr<int64_t>(), (long)out_token.stride(0));
  const hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "beam_select launch failed: ",
              hipGetErrorString(e));
}

}  // namespace ci
