// K5: masked concat-pool — cat([mean, max, last], -1) over true lengths.
// Single-pass reduction over T; reference semantics inference.py:232-263
// (batch_seq_pool: padding masked per true length; "last" = h[length-1]).
#include "common.h"
#include "pool_tile.h"

#include <algorithm>
#include <cstdint>
#include <type_traits>
#include <vector>

namespace ci {

template <typename T>
__global__ void concat_pool_kernel(const T* __restrict__ hidden,
                                   const int* __restrict__ lengths,
                                   T* __restrict__ out, int B, int Tn, int H) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * H) return;
  const int b = idx / H, h = idx % H;
  const int len = max(1, lengths[b]);
  const T* row = hidden + (long)b * Tn * H + h;
  float sum = 0.f, mx = -3.4e38f;
  for (int t = 0; t < len; ++t) {
    const float v = ld(row + (long)t * H);
    sum += v;
    mx = fmaxf(mx, v);
  }
  const float last = ld(row + (long)(len - 1) * H);
  T* orow = out + (long)b * 3 * H + h;
  st(orow, sum / len);
  st(orow + H, mx);
  st(orow + 2 * H, last);
}

at::Tensor concat_pool(at::Tensor hidden, at::Tensor lengths) {
  CI_CHECK_CUDA(hidden); CI_CHECK_CONTIG(hidden); CI_CHECK_CONTIG(lengths);
  TORCH_CHECK(lengths.scalar_type() == at::ScalarType::Int);
  const int B = hidden.size(0), Tn = hidden.size(1), H = hidden.size(2);
  auto out = at::empty({B, 3 * H}, hidden.options());
  const int threads = 256;
  const int blocks = ceil_div((long)B * H, threads);
  CI_DISPATCH_FB(hidden.scalar_type(), "concat_pool", [&] {
    hipLaunchKernelGGL((concat_pool_kernel<scalar_t>), dim3(blocks), dim3(threads),
        0, stream(),
        reinterpret_cast<const scalar_t*>(hidden.data_ptr()),
        lengths.data_ptr<int>(),
        reinterpret_cast<scalar_t*>(out.data_ptr()), B, Tn, H);
  });
  return out;
}


// ---- differentiable, windowed, stride-aware variant ------------------------
// Classifier fine-tuning backpropagates through the pool, and fastai's
// MultiBatchEncoder keeps only the last max_len positions. Row b is pooled
// over t in [lo_b, len_b): len_b = clamp(lengths[b], 1, T),
// lo_b = max(0, len_b - max_len) (0 when max_len <= 0, i.e. "no window").
//
// Layout: hidden is (B,T,H) with element strides (sb, st, 1), so both the
// contiguous batch-major tensor and the (B,T,H) transpose view of the LSTM's
// native (T,B,H) storage are read in place (artar.hip does the same for raw).
//
// Thread map (both kernels): PoolTile in pool_tile.h. The forward combines
// its t slices through LDS in a fixed order, so results are deterministic;
// the backward additionally splits T over blockIdx.z.

template <typename T, int VEC>
__global__ __launch_bounds__(256) void concat_pool_fwd_idx_kernel(
    const T* __restrict__ hidden, const int* __restrict__ lengths,
    T* __restrict__ out,        // (B,3H) contiguous
    int* __restrict__ argmax,   // (B,H) absolute t of the max
    int Tn, int H, long sb, long st, int max_len) {
  constexpr int HL = PoolTile<VEC>::HL, TS = PoolTile<VEC>::TS;
  __shared__ float s_sum[TS][HL * VEC];
  __shared__ float s_max[TS][HL * VEC];
  __shared__ int s_arg[TS][HL * VEC];
  const int lane = threadIdx.x % HL, ty = threadIdx.x / HL;
  const int b = blockIdx.y;
  const long h = ((long)blockIdx.x * HL + lane) * VEC;
  const bool active = h < H;
  int lo, len;
  pool_window(lengths, b, Tn, max_len, lo, len);
  float sum[VEC], mx[VEC];
  int am[VEC];
  #pragma unroll
  for (int e = 0; e < VEC; ++e) { sum[e] = 0.f; mx[e] = -INFINITY; am[e] = lo; }
  if (active) {
    const T* row = hidden + (long)b * sb + h;
    // ascending t with a strict '>' keeps the first maximum of this slice
    #pragma unroll 4
    for (int t = lo + ty; t < len; t += TS) {
      float v[VEC];
      ldv<T, VEC>(row + (long)t * st, v);
      #pragma unroll
      for (int e = 0; e < VEC; ++e) {
        sum[e] += v[e];
        if (v[e] > mx[e]) { mx[e] = v[e]; am[e] = t; }
      }
    }
  }
  #pragma unroll
  for (int e = 0; e < VEC; ++e) {
    s_sum[ty][lane * VEC + e] = sum[e];
    s_max[ty][lane * VEC + e] = mx[e];
    s_arg[ty][lane * VEC + e] = am[e];
  }
  __syncthreads();
  if (ty != 0 || !active) return;
  for (int s = 1; s < TS; ++s) {
    #pragma unroll
    for (int e = 0; e < VEC; ++e) {
      sum[e] += s_sum[s][lane * VEC + e];
      const float m = s_max[s][lane * VEC + e];
      const int a = s_arg[s][lane * VEC + e];
      // ties go to the smallest t (slices interleave in time)
      if (m > mx[e] || (m == mx[e] && a < am[e])) { mx[e] = m; am[e] = a; }
    }
  }
  float mean[VEC], last[VEC];
  const float n = (float)(len - lo);
  #pragma unroll
  for (int e = 0; e < VEC; ++e) mean[e] = sum[e] / n;
  ldv<T, VEC>(hidden + (long)b * sb + (long)(len - 1) * st + h, last);
  T* orow = out + (long)b * 3 * H + h;
  stv<T, VEC>(orow, mean);
  stv<T, VEC>(orow + H, mx);
  stv<T, VEC>(orow + 2 * H, last);
  #pragma unroll
  for (int e = 0; e < VEC; ++e) argmax[(long)b * H + h + e] = am[e];
}

// dhidden[b,t,h] = dmean/(len-lo) + [t==argmax]*dmax + [t==len-1]*dlast for
// t in [lo,len), exact 0 elsewhere; summed in fp32, rounded once. Every
// element is written exactly once (no atomics, dhidden need not be zeroed).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void concat_pool_bwd_kernel(
    const T* __restrict__ dout,       // (B,3H) contiguous
    const int* __restrict__ argmax,   // (B,H)
    const int* __restrict__ lengths,
    T* __restrict__ dhidden,          // (B,T,H), strides (sb, st, 1)
    int Tn, int H, long sb, long st, int max_len, int t_chunk) {
  constexpr int HL = PoolTile<VEC>::HL, TS = PoolTile<VEC>::TS;
  const int lane = threadIdx.x % HL, ty = threadIdx.x / HL;
  const int b = blockIdx.y;
  const long h = ((long)blockIdx.x * HL + lane) * VEC;
  if (h >= H) return;
  int lo, len;
  pool_window(lengths, b, Tn, max_len, lo, len);
  float gmean[VEC], gmax[VEC], glast[VEC];
  int am[VEC];
  const T* drow = dout + (long)b * 3 * H + h;
  ldv<T, VEC>(drow, gmean);
  ldv<T, VEC>(drow + H, gmax);
  ldv<T, VEC>(drow + 2 * H, glast);
  const float n = (float)(len - lo);
  #pragma unroll
  for (int e = 0; e < VEC; ++e) {
    gmean[e] /= n;
    am[e] = argmax[(long)b * H + h + e];
  }
  T* row = dhidden + (long)b * sb + h;
  const int t0 = blockIdx.z * t_chunk;
  const int t1 = min(Tn, t0 + t_chunk);
  for (int t = t0 + ty; t < t1; t += TS) {
    float g[VEC];
    const bool in = t >= lo && t < len;
    #pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float v = gmean[e];
      if (t == am[e]) v += gmax[e];
      if (t == len - 1) v += glast[e];
      g[e] = in ? v : 0.f;
    }
    stv<T, VEC>(row + (long)t * st, g);
  }
}

static void pool_check_hidden(const at::Tensor& hidden,
                              const at::Tensor& lengths) {
  CI_CHECK_CUDA(hidden); CI_CHECK_CUDA(lengths); CI_CHECK_CONTIG(lengths);
  TORCH_CHECK(hidden.dim() == 3, "hidden must be (B,T,H)");
  TORCH_CHECK(hidden.size(2) == 1 || hidden.stride(2) == 1,
              "hidden must have unit stride along H");
  TORCH_CHECK(hidden.size(0) > 0 && hidden.size(1) > 0 && hidden.size(2) > 0,
              "hidden must be non-empty");
  TORCH_CHECK(hidden.size(0) <= 65535, "batch exceeds grid.y");
  TORCH_CHECK(lengths.scalar_type() == at::ScalarType::Int &&
              lengths.numel() == hidden.size(0), "lengths must be int32 (B,)");
}

std::vector<at::Tensor> concat_pool_fwd_idx(at::Tensor hidden,
                                            at::Tensor lengths, long max_len) {
  pool_check_hidden(hidden, lengths);
  const int B = hidden.size(0), Tn = hidden.size(1), H = hidden.size(2);
  const long sb = hidden.stride(0), st = hidden.stride(1);
  auto out = at::empty({B, 3 * H}, hidden.options());
  auto argmax = at::empty({B, H}, hidden.options().dtype(at::kInt));
  const int ml = (int)std::min<long>(std::max<long>(max_len, 0), Tn);
  CI_DISPATCH_FB(hidden.scalar_type(), "concat_pool_fwd_idx", [&] {
    auto launch = [&](auto vec) {
      constexpr int VEC = decltype(vec)::value;
      const dim3 grid(ceil_div(ceil_div(H, VEC), PoolTile<VEC>::HL), B);
      hipLaunchKernelGGL((concat_pool_fwd_idx_kernel<scalar_t, VEC>), grid,
          dim3(256), 0, stream(),
          reinterpret_cast<const scalar_t*>(hidden.data_ptr()),
          lengths.data_ptr<int>(),
          reinterpret_cast<scalar_t*>(out.data_ptr()),
          argmax.data_ptr<int>(), Tn, H, sb, st, ml);
    };
    if (pool_can_vec<scalar_t>(hidden.data_ptr(), H, sb, st))
      launch(std::integral_constant<int, 16 / sizeof(scalar_t)>{});
    else
      launch(std::integral_constant<int, 1>{});
  });
  return {out, argmax};
}

at::Tensor concat_pool_bwd(at::Tensor dout, at::Tensor argmax,
                           at::Tensor lengths, long max_len,
                           at::Tensor like_hidden) {
  pool_check_hidden(like_hidden, lengths);
  CI_CHECK_CUDA(dout); CI_CHECK_CONTIG(dout); CI_CHECK_CONTIG(argmax);
  const int B = like_hidden.size(0), Tn = like_hidden.size(1),
            H = like_hidden.size(2);
  TORCH_CHECK(dout.dim() == 2 && dout.size(0) == B && dout.size(1) == 3 * H &&
              dout.scalar_type() == like_hidden.scalar_type(),
              "dout must be (B,3H) of hidden's dtype");
  TORCH_CHECK(argmax.scalar_type() == at::ScalarType::Int &&
              argmax.dim() == 2 && argmax.size(0) == B && argmax.size(1) == H,
              "argmax must be int32 (B,H)");
  // same layout as the input: time-major storage stays time-major, so the
  // LSTM backward's transpose(0,1).contiguous() of this grad is a no-op
  at::Tensor dh;
  if (!like_hidden.is_contiguous() &&
      like_hidden.transpose(0, 1).is_contiguous())
    dh = at::empty({Tn, B, H}, like_hidden.options()).transpose(0, 1);
  else
    dh = at::empty({B, Tn, H}, like_hidden.options());
  const long sb = dh.stride(0), st = dh.stride(1);
  const int ml = (int)std::min<long>(std::max<long>(max_len, 0), Tn);
  const int t_chunk = 256;
  CI_DISPATCH_FB(dh.scalar_type(), "concat_pool_bwd", [&] {
    auto launch = [&](auto vec) {
      constexpr int VEC = decltype(vec)::value;
      const dim3 grid(ceil_div(ceil_div(H, VEC), PoolTile<VEC>::HL), B,
                      ceil_div(Tn, t_chunk));
      hipLaunchKernelGGL((concat_pool_bwd_kernel<scalar_t, VEC>), grid,
          dim3(256), 0, stream(),
          reinterpret_cast<const scalar_t*>(dout.data_ptr()),
          argmax.data_ptr<int>(), lengths.data_ptr<int>(),
          reinterpret_cast<scalar_t*>(dh.data_ptr()),
          Tn, H, sb, st, ml, t_chunk);
    };
    if (pool_can_vec<scalar_t>(dh.data_ptr(), H, sb, st) &&
        reinterpret_cast<uintptr_t>(dout.data_ptr()) % 16 == 0)
      launch(std::integral_constant<int, 16 / sizeof(scalar_t)>{});
    else
      launch(std::integral_constant<int, 1>{});
  });
  return dh;
}

}  // namespace ci
