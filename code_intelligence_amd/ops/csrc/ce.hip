// K6 epilogues: fused tied-decoder softmax+CE row reductions.
// The (chunked) logits GEMM runs on hipBLASLt; these kernels do the
// per-row max/logsumexp pass and the in-place dlogits transform so full
// logits never round-trip more than once (SURVEY.md par.7 "hard parts").
// The decoder bias is folded in HERE (template<HAS_BIAS>, vectorized
// float4 bias loads — a per-element `bias ? bias[v] : 0` conditional made
// hipcc branch around every load and cost 5x, the par.5 trap (c) of the
// CDNA guide) so the (chunk, 60k) bias broadcast-add never materializes.
#include "common.h"

#include <hip/hip_fp8.h>

namespace ci {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename T, int VEC>
static __device__ __forceinline__ void load_vec(const T* p, float* out) {
  T buf[VEC];
  *reinterpret_cast<int4*>(buf) = *reinterpret_cast<const int4*>(p);
  #pragma unroll
  for (int e = 0; e < VEC; ++e) out[e] = ld(buf + e);
}

template <int VEC>
static __device__ __forceinline__ void load_bias(const float* b, float* out) {
  #pragma unroll
  for (int e = 0; e < VEC; e += 4)
    *reinterpret_cast<f32x4*>(out + e) = *reinterpret_cast<const f32x4*>(b + e);
}

// one block per row, ONLINE single-pass logsumexp (one read of the row
// instead of two): per-thread running (max, sum) merged wave-wide then
// across waves. lse[i] = log(sum(exp(x + bias - max))) + max.
template <typename T, int THREADS, bool HAS_BIAS>
__global__ void ce_rowstats_kernel(const T* __restrict__ logits, long row_stride,
                                   const long* __restrict__ targets,
                                   const float* __restrict__ bias,
                                   float* __restrict__ lse,
                                   float* __restrict__ tgt, int V) {
  constexpr int NW = THREADS / kWave;
  constexpr int VEC = 16 / sizeof(T);
  const int row = blockIdx.x;
  const T* x = logits + (long)row * row_stride;
  __shared__ float red_m[NW];
  __shared__ float red_s[NW];
  const int Vv = V / VEC * VEC;
  float v8[VEC], b8[VEC];
  float m = -3.4e38f, sum = 0.f;
  for (int v = threadIdx.x * VEC; v < Vv; v += THREADS * VEC) {
    load_vec<T, VEC>(x + v, v8);
    if (HAS_BIAS) {
      load_bias<VEC>(bias + v, b8);
      #pragma unroll
      for (int e = 0; e < VEC; ++e) v8[e] += b8[e];
    }
    float bm = v8[0];
    #pragma unroll
    for (int e = 1; e < VEC; ++e) bm = fmaxf(bm, v8[e]);
    // rescale the running sum once per 8-wide block
    if (bm > m) {
      sum *= __expf(m - bm);
      m = bm;
    }
    #pragma unroll
    for (int e = 0; e < VEC; ++e) sum += __expf(v8[e] - m);
  }
  for (int v = Vv + threadIdx.x; v < V; v += THREADS) {
    const float val = ld(x + v) + (HAS_BIAS ? bias[v] : 0.f);
    if (val > m) {
      sum *= __expf(m - val);
      m = val;
    }
    sum += __expf(val - m);
  }
  // wave merge
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const float om = __shfl_down(m, off);
    const float os = __shfl_down(sum, off);
    const float nm = fmaxf(m, om);
    sum = sum * __expf(m - nm) + os * __expf(om - nm);
    m = nm;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red_m[threadIdx.x / kWave] = m;
    red_s[threadIdx.x / kWave] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float gm = red_m[0];
    for (int w = 1; w < NW; ++w) gm = fmaxf(gm, red_m[w]);
    float gs = 0.f;
    for (int w = 0; w < NW; ++w) gs += red_s[w] * __expf(red_m[w] - gm);
    lse[row] = gm + __logf(gs);
    tgt[row] = ld(x + targets[row]) + (HAS_BIAS ? bias[targets[row]] : 0.f);
  }
}

void ce_rowstats(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                 at::Tensor lse, at::Tensor tgt) {
  CI_CHECK_CUDA(logits); CI_CHECK_CONTIG(logits);
  const int N = logits.size(0), V = logits.size(1);
  constexpr int THREADS = 256;
  const bool hb = bias.numel() > 0;
  CI_DISPATCH_FB(logits.scalar_type(), "ce_rowstats", [&] {
    if (hb) {
      hipLaunchKernelGGL((ce_rowstats_kernel<scalar_t, THREADS, true>), dim3(N),
          dim3(THREADS), 0, stream(),
          reinterpret_cast<const scalar_t*>(logits.data_ptr()), (long)V,
          targets.data_ptr<long>(), bias.data_ptr<float>(),
          lse.data_ptr<float>(), tgt.data_ptr<float>(), V);
    } else {
      hipLaunchKernelGGL((ce_rowstats_kernel<scalar_t, THREADS, false>), dim3(N),
          dim3(THREADS), 0, stream(),
          reinterpret_cast<const scalar_t*>(logits.data_ptr()), (long)V,
          targets.data_ptr<long>(), nullptr,
          lse.data_ptr<float>(), tgt.data_ptr<float>(), V);
    }
  });
}

// (p - onehot) * sc for the in-place store. At the target column p - 1
// rounds at 2^-25, as much as the fp32 result's own half-ulp, so the plain
// form rounds twice; an fp32 store gets the single-rounding fma instead. A
// bf16 store's half-ulp (2^-9) hides the difference, and the bf16 instances
// keep the plain form and their bits.
template <typename T>
static __device__ __forceinline__ float dlogit(float p, bool hot, float sc) {
  if constexpr (sizeof(T) == 4) {
    return hot ? __builtin_fmaf(p, sc, -sc) : p * sc;
  } else {
    return (hot ? p - 1.f : p) * sc;
  }
}

// in-place: logits <- (exp(logits + bias - lse) - onehot) * scale
template <typename T, int THREADS, bool HAS_BIAS>
__global__ void ce_dlogits_kernel(T* __restrict__ logits, long row_stride,
                                  const long* __restrict__ targets,
                                  const float* __restrict__ bias,
                                  const float* __restrict__ lse,
                                  const float* __restrict__ scale, int V) {
  constexpr int VEC = 16 / sizeof(T);
  const int row = blockIdx.x;
  T* x = logits + (long)row * row_stride;
  const float l = lse[row];
  const float sc = scale[0];
  const int tgt = (int)targets[row];
  const int Vv = V / VEC * VEC;
  float v8[VEC], b8[VEC];
  for (int v = threadIdx.x * VEC; v < Vv; v += THREADS * VEC) {
    load_vec<T, VEC>(x + v, v8);
    if (HAS_BIAS) {
      load_bias<VEC>(bias + v, b8);
      #pragma unroll
      for (int e = 0; e < VEC; ++e) v8[e] += b8[e];
    }
    T buf[VEC];
    #pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const float p = __expf(v8[e] - l);
      st(buf + e, dlogit<T>(p, v + e == tgt, sc));
    }
    *reinterpret_cast<int4*>(x + v) = *reinterpret_cast<const int4*>(buf);
  }
  for (int v = Vv + threadIdx.x; v < V; v += THREADS) {
    const float p = __expf(ld(x + v) + (HAS_BIAS ? bias[v] : 0.f) - l);
    st(x + v, dlogit<T>(p, v == tgt, sc));
  }
}

void ce_dlogits(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                at::Tensor lse, at::Tensor scale) {
  CI_CHECK_CUDA(logits); CI_CHECK_CONTIG(logits);
  const int N = logits.size(0), V = logits.size(1);
  constexpr int THREADS = 256;
  const bool hb = bias.numel() > 0;
  CI_DISPATCH_FB(logits.scalar_type(), "ce_dlogits", [&] {
    if (hb) {
      hipLaunchKernelGGL((ce_dlogits_kernel<scalar_t, THREADS, true>),
          dim3(N), dim3(THREADS), 0, stream(),
          reinterpret_cast<scalar_t*>(logits.data_ptr()), (long)V,
          targets.data_ptr<long>(), bias.data_ptr<float>(),
          lse.data_ptr<float>(), scale.data_ptr<float>(), V);
    } else {
      hipLaunchKernelGGL((ce_dlogits_kernel<scalar_t, THREADS, false>),
          dim3(N), dim3(THREADS), 0, stream(),
          reinterpret_cast<scalar_t*>(logits.data_ptr()), (long)V,
          targets.data_ptr<long>(), nullptr,
          lse.data_ptr<float>(), scale.data_ptr<float>(), V);
    }
  });
}

// ---- fp8 CE GEMM support (CI_CE_FP8R) ------------------------------------
// Measured on MI355X (scripts/fp8r_probe.py, profiles/fp8r_probe.log):
// the fp8->fp8 GEMM epilogue is UNTUNED on this stack (1.83 ms vs 1.15 ms
// for fp8->bf16 at the chunk shape) and _scaled_mm ignores scale_result,
// so a fully fp8-RESIDENT logits buffer loses. The winning composition is
// hybrid: bf16-resident logits produced by the fp8-input GEMM, and this
// dual epilogue that (in one read of the row) rewrites the bf16 buffer to
// (softmax-onehot)*dloss/N for the bf16 dW GEMM while emitting an e4m3
// copy scaled by STORE=448 for the fp8 dh GEMM (0.78 vs 1.44 ms).
template <typename T, int THREADS, bool HAS_BIAS>
__global__ void ce_dlogits_dual_kernel(T* __restrict__ logits, long row_stride,
                                       const long* __restrict__ targets,
                                       const float* __restrict__ bias,
                                       const float* __restrict__ lse,
                                       const float* __restrict__ scale,
                                       unsigned char* __restrict__ scratch8,
                                       long srs, float store_scale, int V) {
  constexpr int VEC = 16 / sizeof(T);
  const int row = blockIdx.x;
  T* x = logits + (long)row * row_stride;
  unsigned char* s8 = scratch8 + (long)row * srs;
  const float l = lse[row];
  const float sc = scale[0];
  const int tgt = (int)targets[row];
  const int Vv = V / VEC * VEC;
  float v8[VEC], b8[VEC];
  for (int v = threadIdx.x * VEC; v < Vv; v += THREADS * VEC) {
    load_vec<T, VEC>(x + v, v8);
    if (HAS_BIAS) {
      load_bias<VEC>(bias + v, b8);
      #pragma unroll
      for (int e = 0; e < VEC; ++e) v8[e] += b8[e];
    }
    T buf[VEC];
    unsigned char q8[VEC];
    #pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float p = __expf(v8[e] - l);
      st(buf + e, dlogit<T>(p, v + e == tgt, sc));
      if (v + e == tgt) p -= 1.f;
      q8[e] = __hip_fp8_e4m3(p * store_scale).__x;
    }
    *reinterpret_cast<int4*>(x + v) = *reinterpret_cast<const int4*>(buf);
    if constexpr (VEC == 8) {  // bf16 path: 8 fp8 bytes
      *reinterpret_cast<uint2*>(s8 + v) = *reinterpret_cast<const uint2*>(q8);
    } else {                   // fp32 path: 4 fp8 bytes
      *reinterpret_cast<unsigned int*>(s8 + v) =
          *reinterpret_cast<const unsigned int*>(q8);
    }
  }
  for (int v = Vv + threadIdx.x; v < V; v += THREADS) {
    float p = __expf(ld(x + v) + (HAS_BIAS ? bias[v] : 0.f) - l);
    st(x + v, dlogit<T>(p, v == tgt, sc));
    if (v == tgt) p -= 1.f;
    s8[v] = __hip_fp8_e4m3(p * store_scale).__x;
  }
}

void ce_dlogits_dual(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                     at::Tensor lse, at::Tensor scale, at::Tensor scratch8,
                     double store_scale) {
  CI_CHECK_CUDA(logits); CI_CHECK_CONTIG(logits); CI_CHECK_CONTIG(scratch8);
  const int N = logits.size(0), V = logits.size(1);
  TORCH_CHECK(scratch8.size(0) >= N && scratch8.size(1) == V,
              "ce_dlogits_dual: scratch too small");
  TORCH_CHECK(scratch8.scalar_type() == at::ScalarType::Byte ||
              scratch8.scalar_type() == at::ScalarType::Float8_e4m3fn);
  constexpr int THREADS = 256;
  const bool hb = bias.numel() > 0;
  CI_DISPATCH_FB(logits.scalar_type(), "ce_dlogits_dual", [&] {
    if (hb) {
      hipLaunchKernelGGL((ce_dlogits_dual_kernel<scalar_t, THREADS, true>),
          dim3(N), dim3(THREADS), 0, stream(),
          reinterpret_cast<scalar_t*>(logits.data_ptr()), (long)V,
          targets.data_ptr<long>(), bias.data_ptr<float>(),
          lse.data_ptr<float>(), scale.data_ptr<float>(),
          reinterpret_cast<unsigned char*>(scratch8.data_ptr()),
          (long)V, (float)store_scale, V);
    } else {
      hipLaunchKernelGGL((ce_dlogits_dual_kernel<scalar_t, THREADS, false>),
          dim3(N), dim3(THREADS), 0, stream(),
          reinterpret_cast<scalar_t*>(logits.data_ptr()), (long)V,
          targets.data_ptr<long>(), nullptr,
          lse.data_ptr<float>(), scale.data_ptr<float>(),
          reinterpret_cast<unsigned char*>(scratch8.data_ptr()),
          (long)V, (float)store_scale, V);
    }
  });
}

// ---- one-pass CE epilogue -------------------------------------------------
// ce_rowstats + ce_dlogits_dual read the same logits row twice (once in
// forward for lse, once in backward for dlogits). A 60k bf16 row is 7500
// 16-B vectors = 30 per thread of a 256-thread block, so the whole row fits
// in VGPRs: load it once, reduce to lse, then write both dlogits forms from
// the registers. The arithmetic of both phases is the two kernels' above,
// element for element and in the same order, so lse, the bf16 buffer and
// the e4m3 bytes are bit-identical to the two-kernel path.
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
  // lse must equal ce_rowstats_kernel's to the bit, so nothing here may be
  // left to the compiler's choice of which a*b+c to fuse: contraction is
  // off in this body and the merges below spell out the fused / unfused
  // forms that ce_rowstats_kernel compiles to for gfx950.
  #pragma clang fp contract(off)
  using T = __hip_bfloat16;
  constexpr int NW = THREADS / kWave;
  constexpr int VEC = 8;
  const int row = blockIdx.x;
  T* x = logits + (long)row * row_stride;
  unsigned char* s8 = out8 + (long)row * srs;
  __shared__ float red_m[NW];
  __shared__ float red_s[NW];
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
  // phase 1: ce_rowstats_kernel's online (max, sum) over the cached row
  float v8[VEC], b8[VEC];
  float m = -3.4e38f, sum = 0.f;
  #pragma unroll
  for (int k = 0; k < kOnepassMaxVec; ++k) {
    const int v = (threadIdx.x + k * THREADS) * VEC;
    if (v < Vv) {
      unpack_bf16x8(cache[k], v8);
      if (HAS_BIAS) {
        load_bias<VEC>(bias + v, b8);
        #pragma unroll
        for (int e = 0; e < VEC; ++e) v8[e] += b8[e];
      }
      float bm = v8[0];
      #pragma unroll
      for (int e = 1; e < VEC; ++e) bm = fmaxf(bm, v8[e]);
      if (bm > m) {
        sum *= __expf(m - bm);
        m = bm;
      }
      #pragma unroll
      for (int e = 0; e < VEC; ++e) sum += __expf(v8[e] - m);
    }
  }
  for (int v = Vv + threadIdx.x; v < V; v += THREADS) {
    const float val = ld(x + v) + (HAS_BIAS ? bias[v] : 0.f);
    if (val > m) {
      sum *= __expf(m - val);
      m = val;
    }
    sum += __expf(val - m);
  }
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const float om = __shfl_down(m, off);
    const float os = __shfl_down(sum, off);
    const float nm = fmaxf(m, om);
    const float t = os * __expf(om - nm);
    // one fused multiply-add per step, except the last (two products)
    sum = off > 1 ? __builtin_fmaf(sum, __expf(m - nm), t)
                  : sum * __expf(m - nm) + t;
    m = nm;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red_m[threadIdx.x / kWave] = m;
    red_s[threadIdx.x / kWave] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float gm = red_m[0];
    for (int w = 1; w < NW; ++w) gm = fmaxf(gm, red_m[w]);
    float gs = 0.f;
    for (int w = 0; w < NW; ++w) gs += red_s[w] * __expf(red_m[w] - gm);
    const float r = gm + __logf(gs);
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
  // phase 2: ce_dlogits_dual_kernel's transform from the cached row
  const float l = lse_sh;
  const float sc = scale[0];
  const int tgt = (int)targets[row];
  #pragma unroll
  for (int k = 0; k < kOnepassMaxVec; ++k) {
    const int v = (threadIdx.x + k * THREADS) * VEC;
    if (v < Vv) {
      unpack_bf16x8(cache[k], v8);
      if (HAS_BIAS) {
        load_bias<VEC>(bias2 + v, b8);
        #pragma unroll
        for (int e = 0; e < VEC; ++e) v8[e] += b8[e];
      }
      T buf[VEC];
      unsigned char q8[VEC];
      #pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float p = __expf(v8[e] - l);
        if (v + e == tgt) p -= 1.f;
        st(buf + e, p * sc);
        q8[e] = __hip_fp8_e4m3(p * store_scale).__x;
      }
      *reinterpret_cast<int4*>(x + v) = *reinterpret_cast<const int4*>(buf);
      *reinterpret_cast<uint2*>(s8 + v) = *reinterpret_cast<const uint2*>(q8);
    }
  }
  for (int v = Vv + threadIdx.x; v < V; v += THREADS) {
    float p = __expf(ld(x + v) + (HAS_BIAS ? bias2[v] : 0.f) - l);
    if (v == tgt) p -= 1.f;
    st(x + v, p * sc);
    s8[v] = __hip_fp8_e4m3(p * store_scale).__x;
  }
}

void ce_onepass_dual(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                     at::Tensor lse, at::Tensor scale, at::Tensor out8,
                     double store_scale) {
  CI_CHECK_CUDA(logits); CI_CHECK_CONTIG(logits); CI_CHECK_CONTIG(out8);
  CI_CHECK_CUDA(targets); CI_CHECK_CUDA(lse); CI_CHECK_CUDA(scale);
  CI_CHECK_CUDA(out8);
  TORCH_CHECK(logits.dim() == 2 && out8.dim() == 2);
  TORCH_CHECK(logits.scalar_type() == at::ScalarType::BFloat16,
              "ce_onepass_dual: bf16 logits only");
  constexpr int THREADS = 256;
  const int N = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 8, "ce_onepass_dual: V must hold one 16-byte vector");
  TORCH_CHECK(V / 8 <= kOnepassMaxVec * THREADS,
              "ce_onepass_dual: V=", V, " exceeds the register-cached row (",
              kOnepassMaxVec * THREADS * 8, ")");
  TORCH_CHECK(out8.size(0) >= N && out8.size(1) == V,
              "ce_onepass_dual: fp8 output too small");
  TORCH_CHECK(out8.scalar_type() == at::ScalarType::Byte ||
              out8.scalar_type() == at::ScalarType::Float8_e4m3fn);
  TORCH_CHECK(targets.scalar_type() == at::ScalarType::Long &&
              targets.numel() >= N && lse.numel() >= N &&
              lse.scalar_type() == at::ScalarType::Float &&
              scale.scalar_type() == at::ScalarType::Float &&
              scale.numel() >= 1);
  const bool hb = bias.numel() > 0;
  TORCH_CHECK(!hb || (bias.is_cuda() && bias.numel() >= V &&
                      bias.scalar_type() == at::ScalarType::Float));
  if (N == 0) return;
  using T = __hip_bfloat16;
  if (hb) {
    hipLaunchKernelGGL((ce_onepass_dual_kernel<THREADS, true>),
        dim3(N), dim3(THREADS), 0, stream(),
        reinterpret_cast<T*>(logits.data_ptr()), (long)V,
        targets.data_ptr<long>(), bias.data_ptr<float>(),
        lse.data_ptr<float>(), scale.data_ptr<float>(),
        reinterpret_cast<unsigned char*>(out8.data_ptr()),
        (long)V, (float)store_scale, V);
  } else {
    hipLaunchKernelGGL((ce_onepass_dual_kernel<THREADS, false>),
        dim3(N), dim3(THREADS), 0, stream(),
        reinterpret_cast<T*>(logits.data_ptr()), (long)V,
        targets.data_ptr<long>(), nullptr,
        lse.data_ptr<float>(), scale.data_ptr<float>(),
        reinterpret_cast<unsigned char*>(out8.data_ptr()),
        (long)V, (float)store_scale, V);
  }
}

}  // namespace ci
