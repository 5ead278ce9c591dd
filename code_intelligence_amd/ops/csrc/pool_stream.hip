// K5 serve path for the fine-tuned classifier: a streaming concat-pool that
// folds one encoder chunk at a time into a (B,3H) fp32 state, and a fused
// finalise + two-layer head.
#include "common.h"
#include "pool_tile.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <type_traits>
#include <vector>

namespace ci {

// state (B,3H) fp32 = [sum | max | last], fresh = [0 | -inf | 0]. Row b's
// window is [lo_b, len_b) in absolute document positions (len_b is NOT clamped
// to the chunk: lengths are whole-document lengths); the chunk covers
// [t0, t0+Tc). The block folds the intersection [a, e) into the state and
// returns without a single store when it is empty.
//
// Same thread map as concat_pool_fwd_idx_kernel: slice ty sums t = a+ty,
// a+ty+TS, ... in ascending order, slice 0 adds slices 1..TS-1 in that order
// and then the state, so the result depends on the chunking only, never on
// scheduling. One thread owns each (b, h) column of the state: no atomics.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void concat_pool_accum_kernel(
    float* __restrict__ state,          // (B,3H) contiguous
    const T* __restrict__ hidden,       // (B,Tc,H), strides (sb, st, 1)
    const int* __restrict__ lengths, int Tc, int H, long sb, long st,
    int t0, int max_len) {
  constexpr int HL = PoolTile<VEC>::HL, TS = PoolTile<VEC>::TS;
  // [slice][element][lane]: consecutive lanes hit consecutive banks
  __shared__ float s_sum[TS][VEC][HL];
  __shared__ float s_max[TS][VEC][HL];
  const int lane = threadIdx.x % HL, ty = threadIdx.x / HL;
  const int b = blockIdx.y;
  const long h = ((long)blockIdx.x * HL + lane) * VEC;
  const bool active = h < H;
  int lo, len;
  pool_window(lengths, b, INT_MAX, max_len, lo, len);
  // chunk-relative [a, e); block-uniform, so the early return is barrier-safe
  const int a = max(lo - t0, 0);
  const int e = (int)min((long)len - t0, (long)Tc);
  if (a >= e) return;
  float sum[VEC], mx[VEC];
  #pragma unroll
  for (int i = 0; i < VEC; ++i) { sum[i] = 0.f; mx[i] = -INFINITY; }
  const T* row = hidden + (long)b * sb + h;
  if (active) {
    #pragma unroll 4
    for (int t = a + ty; t < e; t += TS) {
      float v[VEC];
      ldv<T, VEC>(row + (long)t * st, v);
      #pragma unroll
      for (int i = 0; i < VEC; ++i) {
        sum[i] += v[i];
        mx[i] = fmaxf(mx[i], v[i]);
      }
    }
  }
  #pragma unroll
  for (int i = 0; i < VEC; ++i) {
    s_sum[ty][i][lane] = sum[i];
    s_max[ty][i][lane] = mx[i];
  }
  __syncthreads();
  if (ty != 0 || !active) return;
  for (int s = 1; s < TS; ++s) {
    #pragma unroll
    for (int i = 0; i < VEC; ++i) {
      sum[i] += s_sum[s][i][lane];
      mx[i] = fmaxf(mx[i], s_max[s][i][lane]);
    }
  }
  float* srow = state + (long)b * 3 * H + h;
  float psum[VEC], pmax[VEC];
  ldv_f32<VEC>(srow, psum);
  ldv_f32<VEC>(srow + H, pmax);
  #pragma unroll
  for (int i = 0; i < VEC; ++i) {
    psum[i] += sum[i];
    pmax[i] = fmaxf(pmax[i], mx[i]);
  }
  stv_f32<VEC>(srow, psum);
  stv_f32<VEC>(srow + H, pmax);
  const long tl = (long)len - 1 - t0;
  if (tl >= 0 && tl < Tc) {
    float last[VEC];
    ldv<T, VEC>(row + tl * st, last);
    stv_f32<VEC>(srow + 2 * H, last);
  }
}

void concat_pool_accum(at::Tensor state, at::Tensor hidden,
                       at::Tensor lengths, long t0, long max_len) {
  CI_CHECK_CUDA(state); CI_CHECK_CUDA(hidden); CI_CHECK_CUDA(lengths);
  CI_CHECK_CONTIG(state); CI_CHECK_CONTIG(lengths);
  TORCH_CHECK(hidden.dim() == 3, "hidden must be (B,Tc,H)");
  const long B = hidden.size(0), Tc = hidden.size(1), H = hidden.size(2);
  TORCH_CHECK(B > 0 && Tc > 0 && H > 0, "hidden must be non-empty");
  TORCH_CHECK(H == 1 || hidden.stride(2) == 1,
              "hidden must have unit stride along H");
  TORCH_CHECK(B <= 65535, "batch exceeds grid.y");
  TORCH_CHECK(state.scalar_type() == at::ScalarType::Float &&
              state.dim() == 2 && state.size(0) == B && state.size(1) == 3 * H,
              "state must be fp32 (B,3H)");
  TORCH_CHECK(lengths.scalar_type() == at::ScalarType::Int &&
              lengths.numel() == B, "lengths must be int32 (B,)");
  TORCH_CHECK(t0 >= 0 && t0 + Tc <= INT_MAX, "chunk position out of range");
  const long sb = hidden.stride(0), st = hidden.stride(1);
  const int ml = (int)std::min<long>(std::max<long>(max_len, 0), INT_MAX);
  CI_DISPATCH_FB(hidden.scalar_type(), "concat_pool_accum", [&] {
    auto launch = [&](auto vec) {
      constexpr int VEC = decltype(vec)::value;
      const dim3 grid(ceil_div(ceil_div(H, VEC), PoolTile<VEC>::HL), B);
      hipLaunchKernelGGL((concat_pool_accum_kernel<scalar_t, VEC>), grid,
          dim3(256), 0, stream(), state.data_ptr<float>(),
          reinterpret_cast<const scalar_t*>(hidden.data_ptr()),
          lengths.data_ptr<int>(), (int)Tc, (int)H, sb, st, (int)t0, ml);
    };
    // the fp32 state rows start at multiples of H floats: H % VEC == 0 with
    // VEC >= 4 keeps their float4 accesses aligned too
    if (pool_can_vec<scalar_t>(hidden.data_ptr(), H, sb, st) &&
        reinterpret_cast<uintptr_t>(state.data_ptr()) % 16 == 0)
      launch(std::integral_constant<int, 16 / sizeof(scalar_t)>{});
    else
      launch(std::integral_constant<int, 1>{});
  });
}


// ---- finalise + head -------------------------------------------------------
// One 256-thread workgroup per batch row; LDS holds the row's features (3H),
// h1 (N1) and the logits (C). Each wave owns outputs n = wave, wave+4, ...:
// lane l accumulates k = l*VEC + 64*VEC*j in ascending j with fmaf, then a
// fixed xor butterfly sums the 64 lanes, so every output has one summation
// order. M = B is tiny: plain fp32 VALU dot products, no MFMA.
constexpr int kHeadThreads = 256;
constexpr int kHeadWaves = kHeadThreads / kWave;

static __device__ __forceinline__ float wave_sum(float v) {
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

static __device__ __forceinline__ float wave_max(float v) {
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}

// w (global, row of K floats) . x (LDS, K floats); VEC = 4 needs K % 4 == 0
// and 16-B aligned rows
template <int VEC>
static __device__ __forceinline__ float head_dot(const float* __restrict__ w,
                                                 const float* x, int K,
                                                 int lane) {
  float acc = 0.f;
  for (int k = lane * VEC; k < K; k += kWave * VEC) {
    float wv[VEC], xv[VEC];
    ldv_f32<VEC>(w + k, wv);
    ldv_f32<VEC>(x + k, xv);
    #pragma unroll
    for (int i = 0; i < VEC; ++i) acc = fmaf(wv[i], xv[i], acc);
  }
  return wave_sum(acc);
}

template <int VEC>
__global__ __launch_bounds__(kHeadThreads) void pool_head_kernel(
    const float* __restrict__ state,    // (B,3H) [sum | max | last]
    const int* __restrict__ lengths, int max_len,
    const float* __restrict__ w1, const float* __restrict__ b1,  // (N1,3H)
    const float* __restrict__ w2, const float* __restrict__ b2,  // (C,N1)
    float* __restrict__ probs, float* __restrict__ logits,       // (B,C)
    int H, int N1, int C, int multi_label) {
  extern __shared__ __align__(16) float smem[];
  const int K1 = 3 * H;
  float* s_f = smem;                    // K1
  float* s_h = smem + K1;               // N1
  float* s_z = s_h + N1;                // C
  const int b = blockIdx.x;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  int lo, len;
  pool_window(lengths, b, INT_MAX, max_len, lo, len);
  const float n = (float)(len - lo);
  const float* srow = state + (long)b * K1;
  for (int k = threadIdx.x; k < K1; k += kHeadThreads)
    s_f[k] = k < H ? srow[k] / n : srow[k];
  __syncthreads();
  for (int j = wave; j < N1; j += kHeadWaves) {
    const float d = head_dot<VEC>(w1 + (long)j * K1, s_f, K1, lane);
    if (lane == 0) s_h[j] = fmaxf(d + b1[j], 0.f);
  }
  __syncthreads();
  float* zrow = logits + (long)b * C;
  float* prow = probs + (long)b * C;
  for (int c = wave; c < C; c += kHeadWaves) {
    const float d = head_dot<1>(w2 + (long)c * N1, s_h, N1, lane);
    if (lane == 0) { const float z = d + b2[c]; s_z[c] = z; zrow[c] = z; }
  }
  __syncthreads();
  if (multi_label) {
    for (int c = threadIdx.x; c < C; c += kHeadThreads)
      prow[c] = 1.0f / (1.0f + expf(-s_z[c]));
    return;
  }
  // softmax over C by wave 0 alone: lane-strided partials in ascending c,
  // then the butterfly; s_z is reused for the exponentials
  if (wave != 0) return;
  float m = -INFINITY;
  for (int c = lane; c < C; c += kWave) m = fmaxf(m, s_z[c]);
  m = wave_max(m);
  float sum = 0.f;
  for (int c = lane; c < C; c += kWave) {
    const float ex = expf(s_z[c] - m);
    s_z[c] = ex;       // lane c % 64 is the only reader and writer of s_z[c]
    sum += ex;
  }
  sum = wave_sum(sum);
  for (int c = lane; c < C; c += kWave) prow[c] = s_z[c] / sum;
}

std::vector<at::Tensor> pool_head_fwd(at::Tensor state, at::Tensor lengths,
                                      long max_len, at::Tensor w1,
                                      at::Tensor b1, at::Tensor w2,
                                      at::Tensor b2, bool multi_label) {
  CI_CHECK_CUDA(state); CI_CHECK_CUDA(lengths); CI_CHECK_CUDA(w1);
  CI_CHECK_CUDA(b1); CI_CHECK_CUDA(w2); CI_CHECK_CUDA(b2);
  CI_CHECK_CONTIG(state); CI_CHECK_CONTIG(lengths); CI_CHECK_CONTIG(w1);
  CI_CHECK_CONTIG(b1); CI_CHECK_CONTIG(w2); CI_CHECK_CONTIG(b2);
  for (const at::Tensor* t : {&state, &w1, &b1, &w2, &b2})
    TORCH_CHECK(t->scalar_type() == at::ScalarType::Float,
                "pool_head_fwd: state and head parameters must be fp32");
  TORCH_CHECK(state.dim() == 2 && state.size(0) > 0 && state.size(1) > 0 &&
              state.size(1) % 3 == 0, "state must be (B,3H)");
  const long B = state.size(0), K1 = state.size(1), H = K1 / 3;
  TORCH_CHECK(w1.dim() == 2 && w1.size(1) == K1 && w1.size(0) > 0,
              "w1 must be (N1,3H)");
  const long N1 = w1.size(0);
  TORCH_CHECK(b1.numel() == N1, "b1 must be (N1,)");
  TORCH_CHECK(w2.dim() == 2 && w2.size(1) == N1 && w2.size(0) > 0,
              "w2 must be (C,N1)");
  const long C = w2.size(0);
  TORCH_CHECK(b2.numel() == C, "b2 must be (C,)");
  TORCH_CHECK(lengths.scalar_type() == at::ScalarType::Int &&
              lengths.numel() == B, "lengths must be int32 (B,)");
  const long lds = (K1 + N1 + C) * (long)sizeof(float);
  TORCH_CHECK(lds <= 64 * 1024, "pool_head_fwd: LDS footprint ", lds,
              " B exceeds 64 KB");
  auto probs = at::empty({B, C}, state.options());
  auto logits = at::empty({B, C}, state.options());
  const int ml = (int)std::min<long>(std::max<long>(max_len, 0), INT_MAX);
  auto launch = [&](auto vec) {
    constexpr int VEC = decltype(vec)::value;
    hipLaunchKernelGGL((pool_head_kernel<VEC>), dim3(B), dim3(kHeadThreads),
        (size_t)lds, stream(), state.data_ptr<float>(),
        lengths.data_ptr<int>(), ml, w1.data_ptr<float>(),
        b1.data_ptr<float>(), w2.data_ptr<float>(), b2.data_ptr<float>(),
        probs.data_ptr<float>(), logits.data_ptr<float>(), (int)H, (int)N1,
        (int)C, multi_label ? 1 : 0);
  };
  if (K1 % 4 == 0 && reinterpret_cast<uintptr_t>(w1.data_ptr()) % 16 == 0)
    launch(std::integral_constant<int, 4>{});
  else
    launch(std::integral_constant<int, 1>{});
  return {probs, logits};
}

}  // namespace ci
