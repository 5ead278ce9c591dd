// K6 epilogues: fused tied-decoder softmax+CE row reductions.
// The (chunked) logits GEMM runs on hipBLASLt; these kernels do the
// per-row max/logsumexp pass and the in-place dlogits transform so full
// logits never round-trip more than once (SURVEY.md par.7 "hard parts").
//
// Three kernels, one block per row, built from one set of row pieces:
//   row_load       x + bias for VEC columns as fp32 lanes (VEC = 1 is the
//                  scalar tail, so vector and tail loops share every body)
//   lse_update / lse_wave_merge / lse_block_merge
//                  the online logsumexp: ce_rowstats_kernel and phase 1 of
//                  ce_onepass_dual_kernel call the same three functions
//   dlogits_store  (exp(v - lse) - onehot) * scale stored in T and, under
//                  DUAL, as e4m3 bytes: ce_dlogits_kernel<DUAL> and phase 2
//                  of ce_onepass_dual_kernel
// so the one-pass kernel's lse, bf16 dlogits and e4m3 bytes equal the
// two-kernel path's by construction.
//
// The decoder bias is folded in HERE (template<HAS_BIAS>, vectorized
// float4 bias loads — a per-element `bias ? bias[v] : 0` conditional made
// hipcc branch around every load and cost 5x, the par.5 trap (c) of the
// CDNA guide) so the (chunk, 60k) bias broadcast-add never materializes.
#include "common.h"

#include <hip/hip_fp8.h>

#include <type_traits>

namespace ci {

constexpr int kCeThreads = 256;

// ---- row pieces -----------------------------------------------------------

template <int VEC, bool HAS_BIAS>
static __device__ __forceinline__ void add_bias(const float* bias, float* v) {
  if constexpr (HAS_BIAS) {
    float b[VEC];
    ldv_f32<VEC>(bias, b);
    #pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] += b[e];
  }
}

// out[0..VEC) = x[0..VEC) + bias[0..VEC)
template <typename T, int VEC, bool HAS_BIAS>
static __device__ __forceinline__ void row_load(const T* x, const float* bias,
                                                float* out) {
  ldv<T, VEC>(x, out);
  add_bias<VEC, HAS_BIAS>(bias, out);
}

// Online logsumexp: per-thread running (m, sum) with sum = sum(exp(v - m)),
// merged wave-wide, then across waves. lse = log(sum(exp(v - max))) + max.
//
// The multiply-add forms below are FROZEN: lse values are saved between
// forward and backward and compared bit for bit by the tests, so the three
// functions run with contraction off (the pragma is lexical, each needs its
// own) and say where a multiply-add is fused:
//   update       sum * exp(m - bm), then plain adds: nothing fused
//   wave merge   fma(sum, exp(m - nm), os * exp(om - nm)) at offsets 32..2,
//                two products and a sum at offset 1
//   block merge  gs += red_s[w] * exp(red_m[w] - gm): nothing fused
template <int VEC>
static __device__ __forceinline__ void lse_update(const float* v, float& m,
                                                  float& sum) {
  #pragma clang fp contract(off)
  float bm = v[0];
  #pragma unroll
  for (int e = 1; e < VEC; ++e) bm = fmaxf(bm, v[e]);
  // rescale the running sum once per VEC-wide block
  if (bm > m) {
    sum *= __expf(m - bm);
    m = bm;
  }
  #pragma unroll
  for (int e = 0; e < VEC; ++e) sum += __expf(v[e] - m);
}

static __device__ __forceinline__ void lse_wave_merge(float& m, float& sum) {
  #pragma clang fp contract(off)
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const float om = __shfl_down(m, off);
    const float os = __shfl_down(sum, off);
    const float nm = fmaxf(m, om);
    const float t = os * __expf(om - nm);
    sum = off > 1 ? __builtin_fmaf(sum, __expf(m - nm), t)
                  : sum * __expf(m - nm) + t;
    m = nm;
  }
}

// the row's lse, valid on thread 0 only; every thread of the block calls it
template <int THREADS>
static __device__ __forceinline__ float lse_block_merge(float m, float sum) {
  #pragma clang fp contract(off)
  constexpr int NW = THREADS / kWave;
  __shared__ float red_m[NW];
  __shared__ float red_s[NW];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red_m[threadIdx.x / kWave] = m;
    red_s[threadIdx.x / kWave] = sum;
  }
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) {
    float gm = red_m[0];
    for (int w = 1; w < NW; ++w) gm = fmaxf(gm, red_m[w]);
    float gs = 0.f;
    for (int w = 0; w < NW; ++w) {
      const float t = red_s[w] * __expf(red_m[w] - gm);
      gs = gs + t;
    }
    r = gm + __logf(gs);
  }
  return r;
}

// (p - onehot) * sc for the in-place store. At the target column p - 1
// rounds at 2^-25, as much as the fp32 result's own half-ulp, so the plain
// form rounds twice; an fp32 store gets the single-rounding fma instead. A
// bf16 store's half-ulp (2^-9) hides the difference, and the bf16 instances
// keep the plain form and their bits.
template <typename T>
static __device__ __forceinline__ float dlogit(float p, bool hot, float sc) {
  #pragma clang fp contract(off)
  if constexpr (sizeof(T) == 4) {
    return hot ? __builtin_fmaf(p, sc, -sc) : p * sc;
  } else {
    return (hot ? p - 1.f : p) * sc;
  }
}

// v[0..VEC) = logits + bias of columns col..col+VEC of the row x, whose
// logsumexp is l: x[col..] <- T((exp(v - l) - onehot) * sc) and, under DUAL,
// s8[col..] <- e4m3((exp(v - l) - onehot) * store_scale), 8, 4 or 1 bytes
template <typename T, int VEC, bool DUAL>
static __device__ __forceinline__ void dlogits_store(
    const float* v, int col, int tgt, float l, float sc, float store_scale,
    T* x, unsigned char* s8) {
  #pragma clang fp contract(off)
  float q[VEC];
  unsigned char q8[VEC];
  #pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const float p = __expf(v[e] - l);
    const bool hot = col + e == tgt;
    q[e] = dlogit<T>(p, hot, sc);
    if constexpr (DUAL)
      q8[e] = __hip_fp8_e4m3((hot ? p - 1.f : p) * store_scale).__x;
  }
  stv<T, VEC>(x + col, q);
  if constexpr (DUAL) {
    if constexpr (VEC == 8) {
      *reinterpret_cast<uint2*>(s8 + col) = *reinterpret_cast<const uint2*>(q8);
    } else if constexpr (VEC == 4) {
      *reinterpret_cast<unsigned int*>(s8 + col) =
          *reinterpret_cast<const unsigned int*>(q8);
    } else {
      static_assert(VEC == 1, "e4m3 store widths: 8, 4 or 1 bytes");
      s8[col] = q8[0];
    }
  }
}

// ---- kernels --------------------------------------------------------------

// lse[row] and the target logit, one read of the row
template <typename T, int THREADS, bool HAS_BIAS>
__global__ void ce_rowstats_kernel(const T* __restrict__ logits, long row_stride,
                                   const long* __restrict__ targets,
                                   const float* __restrict__ bias,
                                   float* __restrict__ lse,
                                   float* __restrict__ tgt, int V) {
  constexpr int VEC = 16 / sizeof(T);
  const int row = blockIdx.x;
  const T* x = logits + (long)row * row_stride;
  const int Vv = V / VEC * VEC;
  float v8[VEC];
  float m = -3.4e38f, sum = 0.f;
  for (int v = threadIdx.x * VEC; v < Vv; v += THREADS * VEC) {
    row_load<T, VEC, HAS_BIAS>(x + v, bias + v, v8);
    lse_update<VEC>(v8, m, sum);
  }
  for (int v = Vv + threadIdx.x; v < V; v += THREADS) {
    row_load<T, 1, HAS_BIAS>(x + v, bias + v, v8);
    lse_update<1>(v8, m, sum);
  }
  lse_wave_merge(m, sum);
  const float r = lse_block_merge<THREADS>(m, sum);
  if (threadIdx.x == 0) {
    lse[row] = r;
    tgt[row] = ld(x + targets[row]) + (HAS_BIAS ? bias[targets[row]] : 0.f);
  }
}

// in-place: logits <- (exp(logits + bias - lse) - onehot) * scale; DUAL also
// emits the e4m3 copy scaled by store_scale in the same read of the row.
//
// Why a dual form (CI_CE_FP8R), measured on MI355X (scripts/fp8r_probe.py,
// profiles/fp8r_probe.log): the fp8->fp8 GEMM epilogue is UNTUNED on this
// stack (1.83 ms vs 1.15 ms for fp8->bf16 at the chunk shape) and
// _scaled_mm ignores scale_result, so a fully fp8-RESIDENT logits buffer
// loses. The winning composition is hybrid: bf16-resident logits produced
// by the fp8-input GEMM, rewritten here to (softmax-onehot)*dloss/N for the
// bf16 dW GEMM, plus an e4m3 copy scaled by STORE=448 for the fp8 dh GEMM
// (0.78 vs 1.44 ms).
template <typename T, int THREADS, bool HAS_BIAS, bool DUAL>
__global__ void ce_dlogits_kernel(T* __restrict__ logits, long row_stride,
                                  const long* __restrict__ targets,
                                  const float* __restrict__ bias,
                                  const float* __restrict__ lse,
                                  const float* __restrict__ scale,
                                  unsigned char* __restrict__ out8, long srs,
                                  float store_scale, int V) {
  constexpr int VEC = 16 / sizeof(T);
  const int row = blockIdx.x;
  T* x = logits + (long)row * row_stride;
  unsigned char* s8 = DUAL ? out8 + (long)row * srs : nullptr;
  const float l = lse[row];
  const float sc = scale[0];
  const int tgt = (int)targets[row];
  const int Vv = V / VEC * VEC;
  float v8[VEC];
  for (int v = threadIdx.x * VEC; v < Vv; v += THREADS * VEC) {
    row_load<T, VEC, HAS_BIAS>(x + v, bias + v, v8);
    dlogits_store<T, VEC, DUAL>(v8, v, tgt, l, sc, store_scale, x, s8);
  }
  for (int v = Vv + threadIdx.x; v < V; v += THREADS) {
    row_load<T, 1, HAS_BIAS>(x + v, bias + v, v8);
    dlogits_store<T, 1, DUAL>(v8, v, tgt, l, sc, store_scale, x, s8);
  }
}

// ---- one-pass CE epilogue -------------------------------------------------
// ce_rowstats + ce_dlogits_dual read the same logits row twice (once in
// forward for lse, once in backward for dlogits). A 60k bf16 row is 7500
// 16-B vectors = 30 per thread of a 256-thread block, so the whole row fits
// in VGPRs: load it once, reduce to lse, then write both dlogits forms from
// the registers, through the same row pieces as the two kernels above.
constexpr int kOnepassMaxVec = 32;  // cached 16-B vectors per thread

// bf16 -> fp32 is a 16-bit shift; done on whole registers (no pointer
// punning) so the cached row stays 4 registers per vector
static __device__ __forceinline__ void unpack_bf16x8(const uint4& c,
                                                     float* out) {
  out[0] = __uint_as_float(c.x << 16); out[1] = __uint_as_float(c.x & 0xffff0000u);
  out[2] = __uint_as_float(c.y << 16); out[3] = __uint_as_float(c.y & 0xffff0000u);
  out[4] = __uint_as_float(c.z << 16); out[5] = __uint_as_float(c.z & 0xffff0000u);
  out[6] = __uint_as_float(c.w << 16); out[7] = __uint_as_float(c.w & 0xffff0000u);
}

template <int THREADS, bool HAS_BIAS>
__global__ __launch_bounds__(THREADS) void ce_onepass_dual_kernel(
    __hip_bfloat16* __restrict__ logits, long row_stride,
    const long* __restrict__ targets, const float* __restrict__ bias,
    float* __restrict__ lse, const float* __restrict__ scale,
    unsigned char* __restrict__ out8, long srs, float store_scale, int V) {
  using T = __hip_bfloat16;
  constexpr int VEC = 8;
  const int row = blockIdx.x;
  T* x = logits + (long)row * row_stride;
  unsigned char* s8 = out8 + (long)row * srs;
  __shared__ float lse_sh;
  const int Vv = V / VEC * VEC;
  // All loads first (compile-time indices keep the cache in registers).
  // No branch here: a slot past the row end re-reads the row's last
  // vector (Vv >= VEC is the wrapper's check; a cache hit that is never
  // used), so the loads stay unpredicated and issue back to back.
  uint4 cache[kOnepassMaxVec];
  #pragma unroll
  for (int k = 0; k < kOnepassMaxVec; ++k) {
    const int v = (threadIdx.x + k * THREADS) * VEC;
    cache[k] = *reinterpret_cast<const uint4*>(x + min(v, Vv - VEC));
  }
  // Opaque barrier for the compiler (emits nothing): without it the bf16
  // unpack of phase 1 is hoisted up to each load, which serializes the
  // loads behind a wait each and doubles the live registers.
  #pragma unroll
  for (int k = 0; k < kOnepassMaxVec; ++k)
    asm volatile("" : "+v"(cache[k].x), "+v"(cache[k].y), "+v"(cache[k].z),
                      "+v"(cache[k].w));
  // phase 1: the online (max, sum) over the cached row
  float v8[VEC];
  float m = -3.4e38f, sum = 0.f;
  #pragma unroll
  for (int k = 0; k < kOnepassMaxVec; ++k) {
    const int v = (threadIdx.x + k * THREADS) * VEC;
    if (v < Vv) {
      unpack_bf16x8(cache[k], v8);
      add_bias<VEC, HAS_BIAS>(bias + v, v8);
      lse_update<VEC>(v8, m, sum);
    }
  }
  for (int v = Vv + threadIdx.x; v < V; v += THREADS) {
    row_load<T, 1, HAS_BIAS>(x + v, bias + v, v8);
    lse_update<1>(v8, m, sum);
  }
  lse_wave_merge(m, sum);
  const float r = lse_block_merge<THREADS>(m, sum);
  if (threadIdx.x == 0) {
    lse[row] = r;
    lse_sh = r;
  }
  __syncthreads();
  // Make the cached row and the bias pointer opaque again (no instruction
  // is emitted), so phase 2 re-derives x + bias from the 128 cached
  // registers and the compiler has no reason to keep phase 1's 256
  // unpacked fp32 values alive across the barrier.
  #pragma unroll
  for (int k = 0; k < kOnepassMaxVec; ++k)
    asm volatile("" : "+v"(cache[k].x), "+v"(cache[k].y), "+v"(cache[k].z),
                      "+v"(cache[k].w));
  const float* bias2 = bias;
  asm volatile("" : "+s"(bias2));
  // phase 2: both dlogits forms from the cached row
  const float l = lse_sh;
  const float sc = scale[0];
  const int tgt = (int)targets[row];
  #pragma unroll
  for (int k = 0; k < kOnepassMaxVec; ++k) {
    const int v = (threadIdx.x + k * THREADS) * VEC;
    if (v < Vv) {
      unpack_bf16x8(cache[k], v8);
      add_bias<VEC, HAS_BIAS>(bias2 + v, v8);
      dlogits_store<T, VEC, true>(v8, v, tgt, l, sc, store_scale, x, s8);
    }
  }
  for (int v = Vv + threadIdx.x; v < V; v += THREADS) {
    row_load<T, 1, HAS_BIAS>(x + v, bias2 + v, v8);
    dlogits_store<T, 1, true>(v8, v, tgt, l, sc, store_scale, x, s8);
  }
}

// ---- host side ------------------------------------------------------------

// One argument check for all four wrappers: every pointer a kernel gets is
// a device pointer to at least the elements the kernel touches. lse is
// required; rowvec2 (ce_rowstats' target-logit output), scale and out8 are
// checked where the caller has one. Returns false when there is no row.
static bool ce_check(const char* name, const at::Tensor& logits,
                     const at::Tensor& targets, const at::Tensor& bias,
                     const at::Tensor& lse, const at::Tensor* rowvec2,
                     const at::Tensor* scale, const at::Tensor* out8) {
  constexpr auto kF32 = at::ScalarType::Float;
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2,
              name, ": logits must be a contiguous 2-D device tensor");
  const long N = logits.size(0), V = logits.size(1);
  TORCH_CHECK(targets.is_cuda() && targets.is_contiguous() &&
              targets.scalar_type() == at::ScalarType::Long &&
              targets.numel() >= N,
              name, ": targets must be N int64 on the device");
  for (const at::Tensor* t : {&lse, rowvec2}) {
    if (t == nullptr) continue;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                t->scalar_type() == kF32 && t->numel() >= N,
                name, ": lse / target logits must be N fp32 on the device");
  }
  TORCH_CHECK(bias.numel() == 0 ||
              (bias.is_cuda() && bias.is_contiguous() &&
               bias.scalar_type() == kF32 && bias.numel() >= V),
              name, ": bias must be empty or V fp32 on the device");
  if (scale != nullptr)
    TORCH_CHECK(scale->is_cuda() && scale->scalar_type() == kF32 &&
                scale->numel() >= 1,
                name, ": scale must be one fp32 on the device");
  if (out8 != nullptr)
    TORCH_CHECK(out8->is_cuda() && out8->is_contiguous() &&
                out8->dim() == 2 && out8->size(0) >= N &&
                out8->size(1) == V &&
                (out8->scalar_type() == at::ScalarType::Byte ||
                 out8->scalar_type() == at::ScalarType::Float8_e4m3fn),
                name, ": fp8 output too small (needs (N, V) bytes on the "
                "device)");
  return N > 0;
}

// f(std::bool_constant<HAS_BIAS>, bias pointer or nullptr)
template <typename F>
static void ce_dispatch_bias(const at::Tensor& bias, F&& f) {
  if (bias.numel() > 0) f(std::true_type{}, bias.data_ptr<float>());
  else f(std::false_type{}, static_cast<const float*>(nullptr));
}

// f(T{}, std::bool_constant<HAS_BIAS>, bias pointer): logits dtype and
// HAS_BIAS resolved once for every launch below
template <typename F>
static void ce_dispatch(const at::Tensor& logits, const at::Tensor& bias,
                        F&& f) {
  CI_DISPATCH_FB(logits.scalar_type(), "CE epilogue", [&] {
    ce_dispatch_bias(bias, [&](auto hb, const float* b) {
      f(scalar_t{}, hb, b);
    });
  });
}

void ce_rowstats(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                 at::Tensor lse, at::Tensor tgt) {
  if (!ce_check("ce_rowstats", logits, targets, bias, lse, &tgt, nullptr,
                nullptr))
    return;
  const int N = logits.size(0), V = logits.size(1);
  ce_dispatch(logits, bias, [&](auto t, auto hb, const float* b) {
    using T = decltype(t);
    hipLaunchKernelGGL(
        (ce_rowstats_kernel<T, kCeThreads, decltype(hb)::value>), dim3(N),
        dim3(kCeThreads), 0, stream(),
        reinterpret_cast<const T*>(logits.data_ptr()), (long)V,
        targets.data_ptr<long>(), b, lse.data_ptr<float>(),
        tgt.data_ptr<float>(), V);
  });
}

template <bool DUAL>
static void launch_dlogits(at::Tensor& logits, at::Tensor& targets,
                           at::Tensor& bias, at::Tensor& lse,
                           at::Tensor& scale, unsigned char* out8,
                           double store_scale) {
  const int N = logits.size(0), V = logits.size(1);
  ce_dispatch(logits, bias, [&](auto t, auto hb, const float* b) {
    using T = decltype(t);
    hipLaunchKernelGGL(
        (ce_dlogits_kernel<T, kCeThreads, decltype(hb)::value, DUAL>),
        dim3(N), dim3(kCeThreads), 0, stream(),
        reinterpret_cast<T*>(logits.data_ptr()), (long)V,
        targets.data_ptr<long>(), b, lse.data_ptr<float>(),
        scale.data_ptr<float>(), out8, (long)V, (float)store_scale, V);
  });
}

void ce_dlogits(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                at::Tensor lse, at::Tensor scale) {
  if (ce_check("ce_dlogits", logits, targets, bias, lse, nullptr, &scale,
               nullptr))
    launch_dlogits<false>(logits, targets, bias, lse, scale, nullptr, 0.0);
}

void ce_dlogits_dual(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                     at::Tensor lse, at::Tensor scale, at::Tensor scratch8,
                     double store_scale) {
  if (ce_check("ce_dlogits_dual", logits, targets, bias, lse, nullptr, &scale,
               &scratch8))
    launch_dlogits<true>(logits, targets, bias, lse, scale,
                         reinterpret_cast<unsigned char*>(scratch8.data_ptr()),
                         store_scale);
}

void ce_onepass_dual(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                     at::Tensor lse, at::Tensor scale, at::Tensor out8,
                     double store_scale) {
  using T = __hip_bfloat16;
  TORCH_CHECK(logits.scalar_type() == at::ScalarType::BFloat16,
              "ce_onepass_dual: bf16 logits only");
  TORCH_CHECK(logits.dim() == 2, "ce_onepass_dual: logits must be 2-D");
  const int N = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 8, "ce_onepass_dual: V must hold one 16-byte vector");
  TORCH_CHECK(V / 8 <= kOnepassMaxVec * kCeThreads,
              "ce_onepass_dual: V=", V, " exceeds the register-cached row (",
              kOnepassMaxVec * kCeThreads * 8, ")");
  if (!ce_check("ce_onepass_dual", logits, targets, bias, lse, nullptr, &scale,
                &out8))
    return;
  ce_dispatch_bias(bias, [&](auto hb, const float* b) {
    hipLaunchKernelGGL(
        (ce_onepass_dual_kernel<kCeThreads, decltype(hb)::value>), dim3(N),
        dim3(kCeThreads), 0, stream(),
        reinterpret_cast<T*>(logits.data_ptr()), (long)V,
        targets.data_ptr<long>(), b, lse.data_ptr<float>(),
        scale.data_ptr<float>(),
        reinterpret_cast<unsigned char*>(out8.data_ptr()), (long)V,
        (float)store_scale, V);
  });
}

}  // namespace ci
