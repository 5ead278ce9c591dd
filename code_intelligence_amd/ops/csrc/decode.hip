// K10 text generation: the per-word decoder step of the language model as
// two launches. decode_logits streams the (V,H) decoder weight once for a
// group of up to 8 rows of h and leaves fp32 logits plus one (max, sum exp)
// partial per vocabulary tile; decode_sample turns a row of logits into one
// sampled id with fastai's filters (no_unk, min_p, temperature) by an
// inverse-CDF draw against a caller-supplied uniform. With top-k / nucleus
// sampling a third launch between them, decode_cutoff, finds the logit at
// which the kept set of each row ends.
#include "common.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <type_traits>
#include <vector>

namespace ci {

constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / kWave;
constexpr int kDecTileV = 64;          // vocabulary rows per workgroup
constexpr int kDecMaxGroup = 8;        // rows of h that share one read of W
constexpr int kDecMaxSegs = 1024;      // CDF segments per row (LDS)

static __device__ __forceinline__ float dec_wave_sum(float v) {
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

static __device__ __forceinline__ float dec_wave_max(float v) {
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}

static __device__ __forceinline__ int dec_wave_max_i(int v) {
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
    v = max(v, __shfl_xor(v, off, kWave));
  return v;
}

// inclusive prefix sum over the 64 lanes, lower lanes first
static __device__ __forceinline__ float dec_wave_scan(float v, int lane) {
  #pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const float o = __shfl_up(v, off, kWave);
    if (lane >= off) v += o;
  }
  return v;
}

// ---- logits ----------------------------------------------------------------
// grid = (vocabulary tiles, row groups). The workgroup stages its group's rows
// of h in LDS as fp32 (G*H floats, rows past nb zero), then each wave owns
// vocabulary rows v = tile*64 + wave, +4, ...: lane l accumulates
// k = l*VEC + 64*VEC*j in ascending j with fmaf for every row of the group
// from one 16-B packet of W, and a fixed xor butterfly sums the lanes. Lane 0
// adds the bias and stores: one thread owns each logit. The tile's logits are
// kept in LDS and wave g % 4 reduces row g's 64 of them to (max, sum exp).
template <typename T, int VEC, int G>
__global__ __launch_bounds__(kDecThreads) void decode_logits_kernel(
    const T* __restrict__ h, long h_stride,    // (B,H), unit stride along H
    const T* __restrict__ w,                   // (V,H) contiguous
    const T* __restrict__ bias,                // (V) or null
    float* __restrict__ logits,                // (B,V)
    float* __restrict__ partials,              // (B,NT,2)
    int B, int V, int H, int NT) {
  extern __shared__ __align__(16) float smem[];
  float* s_h = smem;                           // G*H
  float* s_l = smem + (long)G * H;             // G*kDecTileV
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int tile = blockIdx.x;
  const int b0 = blockIdx.y * kDecMaxGroup;
  const int nb = min(B - b0, G);
  for (int i = threadIdx.x; i < G * H; i += kDecThreads) {
    const int g = i / H, k = i - g * H;
    s_h[i] = g < nb ? ld(h + (long)(b0 + g) * h_stride + k) : 0.f;
  }
  __syncthreads();
  for (int r = wave; r < kDecTileV; r += kDecWaves) {
    const long v = (long)tile * kDecTileV + r;
    float acc[G];
    #pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0.f;
    if (v < V) {                               // wave-uniform
      const T* wrow = w + v * H;
      for (int k = lane * VEC; k < H; k += kWave * VEC) {
        float wv[VEC];
        ldv<T, VEC>(wrow + k, wv);
        #pragma unroll
        for (int g = 0; g < G; ++g) {
          float hv[VEC];
          ldv_f32<VEC>(s_h + g * H + k, hv);
          #pragma unroll
          for (int i = 0; i < VEC; ++i) acc[g] = fmaf(wv[i], hv[i], acc[g]);
        }
      }
    }
    #pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = dec_wave_sum(acc[g]);
    if (lane == 0) {
      const float bv = (v < V && bias != nullptr) ? ld(bias + v) : 0.f;
      #pragma unroll
      for (int g = 0; g < G; ++g) {
        const float l = v < V ? acc[g] + bv : -INFINITY;
        s_l[g * kDecTileV + r] = l;
        if (v < V && g < nb) logits[(long)(b0 + g) * V + v] = l;
      }
    }
  }
  __syncthreads();
  // every tile holds at least one v < V, so the max is finite
  for (int g = wave; g < nb; g += kDecWaves) {
    const float l = s_l[g * kDecTileV + lane];
    const float m = dec_wave_max(l);
    const float s = dec_wave_sum(expf(l - m));
    if (lane == 0) {
      float* p = partials + ((long)(b0 + g) * NT + tile) * 2;
      p[0] = m;
      p[1] = s;
    }
  }
}

void decode_logits(at::Tensor h, at::Tensor weight,
                   c10::optional<at::Tensor> bias, at::Tensor logits,
                   at::Tensor partials) {
  CI_CHECK_CUDA(h); CI_CHECK_CUDA(weight); CI_CHECK_CUDA(logits);
  CI_CHECK_CUDA(partials);
  CI_CHECK_CONTIG(weight); CI_CHECK_CONTIG(logits); CI_CHECK_CONTIG(partials);
  TORCH_CHECK(h.dim() == 2 && weight.dim() == 2, "h must be (B,H), weight (V,H)");
  const long B = h.size(0), H = h.size(1), V = weight.size(0);
  TORCH_CHECK(B > 0 && H > 0 && V > 0, "decode_logits: empty input");
  TORCH_CHECK(weight.size(1) == H, "weight must be (V,H)");
  TORCH_CHECK(H == 1 || h.stride(1) == 1, "h must have unit stride along H");
  TORCH_CHECK(h.scalar_type() == weight.scalar_type(),
              "h and weight must share a dtype");
  TORCH_CHECK(V <= INT_MAX, "decode_logits: V exceeds INT_MAX");
  const bool has_bias = bias.has_value() && bias->defined();
  if (has_bias) {
    CI_CHECK_CUDA(*bias); CI_CHECK_CONTIG(*bias);
    TORCH_CHECK(bias->numel() == V &&
                bias->scalar_type() == weight.scalar_type(),
                "bias must be (V,) in the weight's dtype");
  }
  const long NT = (V + kDecTileV - 1) / kDecTileV;
  TORCH_CHECK(logits.scalar_type() == at::ScalarType::Float &&
              logits.dim() == 2 && logits.size(0) == B && logits.size(1) == V,
              "logits scratch must be fp32 (B,V)");
  TORCH_CHECK(partials.scalar_type() == at::ScalarType::Float &&
              partials.numel() == B * NT * 2,
              "partials must be fp32 (B, ceil(V/64), 2)");
  const long groups = (B + kDecMaxGroup - 1) / kDecMaxGroup;
  TORCH_CHECK(groups <= 65535, "batch exceeds grid.y");
  const long hs = h.stride(0);
  CI_DISPATCH_FB(weight.scalar_type(), "decode_logits", [&] {
    auto launch = [&](auto vec, auto grp) {
      constexpr int VEC = decltype(vec)::value;
      constexpr int G = decltype(grp)::value;
      const long lds = ((long)G * H + G * kDecTileV) * (long)sizeof(float);
      TORCH_CHECK(lds <= 64 * 1024, "decode_logits: LDS footprint ", lds,
                  " B exceeds 64 KB (H too large)");
      hipLaunchKernelGGL((decode_logits_kernel<scalar_t, VEC, G>),
          dim3(NT, groups), dim3(kDecThreads), (size_t)lds, stream(),
          reinterpret_cast<const scalar_t*>(h.data_ptr()), hs,
          reinterpret_cast<const scalar_t*>(weight.data_ptr()),
          has_bias ? reinterpret_cast<const scalar_t*>(bias->data_ptr())
                   : nullptr,
          logits.data_ptr<float>(), partials.data_ptr<float>(), (int)B,
          (int)V, (int)H, (int)NT);
    };
    auto with_group = [&](auto vec) {
      const long g = std::min<long>(B, kDecMaxGroup);
      if (g <= 1) launch(vec, std::integral_constant<int, 1>{});
      else if (g <= 2) launch(vec, std::integral_constant<int, 2>{});
      else if (g <= 4) launch(vec, std::integral_constant<int, 4>{});
      else launch(vec, std::integral_constant<int, 8>{});
    };
    // 16-B packets: rows of W start at multiples of H elements; the fp32
    // rows of h in LDS start at multiples of H floats (H % VEC == 0, VEC >= 4)
    constexpr int PK = 16 / sizeof(scalar_t);
    if (H % PK == 0 && reinterpret_cast<uintptr_t>(weight.data_ptr()) % 16 == 0)
      with_group(std::integral_constant<int, PK>{});
    else
      with_group(std::integral_constant<int, 1>{});
  });
}

// ---- sample ----------------------------------------------------------------
// Block-wide reductions in a fixed order: wave butterflies, then wave 0's
// lane 0 combines the four wave results in ascending wave order.
static __device__ __forceinline__ float dec_block_max(float v, float* s_red) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  v = dec_wave_max(v);
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  float r = s_red[0];
  for (int i = 1; i < kDecWaves; ++i) r = fmaxf(r, s_red[i]);
  return r;
}

static __device__ __forceinline__ float dec_block_sum(float v, float* s_red) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  v = dec_wave_sum(v);
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  float r = s_red[0];
  for (int i = 1; i < kDecWaves; ++i) r += s_red[i];
  return r;
}

// One workgroup per row. The row is cut into nseg <= 1024 segments of
// seg_len = 64*VEC*iters consecutive entries; wave s % 4 owns segment s and
// reads it 64*VEC entries at a time, lane l taking entries l*VEC.. of each
// chunk. An entry is a candidate unless it is unk; it passes when
// exp(l - lse) >= min_p. Pass 1 keeps, per segment, the weight sums of the
// candidates and of the passing entries, and per block the number of passing
// entries and the last candidate / last passing index; the filter applies iff
// something passes. Wave 0 then scans the chosen segment sums (16 per lane in
// ascending order, a lane prefix scan, then the 16 of the crossing lane) and
// walks the one segment that holds u * total. Every sum has one order, fixed
// by V alone. CUT adds the top-k / nucleus cutoff of decode_cutoff: an entry
// is a candidate only if its logit is >= cut[b].
template <int VEC, bool CUT>
__global__ __launch_bounds__(kDecThreads) void decode_sample_kernel(
    const float* __restrict__ logits,          // (B,V)
    const float* __restrict__ partials,        // (B,NT,2)
    const float* __restrict__ u,               // (B)
    const float* __restrict__ cut,             // (B), read iff CUT
    int64_t* __restrict__ out_ids, long id_stride,
    float* __restrict__ out_logp, long logp_stride,
    int V, int NT, int iters, int nseg, float inv_temp, float min_p, int unk) {
  __shared__ float s_all[kDecMaxSegs];
  __shared__ float s_pass[kDecMaxSegs];
  __shared__ float s_red[kDecWaves];
  __shared__ int s_redi[3][kDecWaves];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int b = blockIdx.x;
  const float* row = logits + (long)b * V;
  const float* part = partials + (long)b * NT * 2;
  const float cutv = CUT ? cut[b] : -INFINITY;

  // m and lse from the tile partials
  float m = -INFINITY;
  for (int t = threadIdx.x; t < NT; t += kDecThreads) m = fmaxf(m, part[2 * t]);
  m = dec_block_max(m, s_red);
  float se = 0.f;
  for (int t = threadIdx.x; t < NT; t += kDecThreads)
    se += part[2 * t + 1] * expf(part[2 * t] - m);
  se = dec_block_sum(se, s_red);
  const float lse = m + logf(se);

  constexpr int CH = kWave * VEC;              // entries per wave chunk
  const long seg_len = (long)CH * iters;

  auto weigh = [&](long e, float l, float& w_all, float& w_pass, bool& cand,
                   bool& pass) {
    cand = e < V && e != unk;
    if (CUT) cand = cand && l >= cutv;
    pass = cand && expf(l - lse) >= min_p;
    const float wgt = cand ? expf((l - m) * inv_temp) : 0.f;
    w_all = wgt;
    w_pass = pass ? wgt : 0.f;
  };
  auto load = [&](long e0, float* l) {
    if (VEC > 1 && e0 + VEC <= V) { ldv_f32<VEC>(row + e0, l); return; }
    #pragma unroll
    for (int i = 0; i < VEC; ++i) l[i] = e0 + i < V ? row[e0 + i] : 0.f;
  };

  // pass 1
  int n_pass = 0, last_all = -1, last_pass = -1;
  for (int s = wave; s < nseg; s += kDecWaves) {
    float sum_all = 0.f, sum_pass = 0.f;
    for (int it = 0; it < iters; ++it) {
      const long e0 = (long)s * seg_len + (long)it * CH + lane * VEC;
      if (e0 < V) {
        float l[VEC];
        load(e0, l);
        #pragma unroll
        for (int i = 0; i < VEC; ++i) {
          float wa, wp; bool cand, pass;
          weigh(e0 + i, l[i], wa, wp, cand, pass);
          sum_all += wa;
          sum_pass += wp;
          if (cand) last_all = (int)(e0 + i);
          if (pass) { last_pass = (int)(e0 + i); ++n_pass; }
        }
      }
    }
    sum_all = dec_wave_sum(sum_all);
    sum_pass = dec_wave_sum(sum_pass);
    if (lane == 0) { s_all[s] = sum_all; s_pass[s] = sum_pass; }
  }
  for (int s = nseg + threadIdx.x; s < kDecMaxSegs; s += kDecThreads) {
    s_all[s] = 0.f;
    s_pass[s] = 0.f;
  }
  // any() of n_pass is all that matters: a max cannot overflow
  n_pass = dec_wave_max_i(n_pass);
  last_all = dec_wave_max_i(last_all);
  last_pass = dec_wave_max_i(last_pass);
  if (lane == 0) {
    s_redi[0][wave] = n_pass;
    s_redi[1][wave] = last_all;
    s_redi[2][wave] = last_pass;
  }
  __syncthreads();
  if (wave != 0) return;
  for (int i = 1; i < kDecWaves; ++i) {
    n_pass = max(n_pass, s_redi[0][i]);
    last_all = max(last_all, s_redi[1][i]);
    last_pass = max(last_pass, s_redi[2][i]);
  }
  const bool filtered = n_pass > 0;
  const float* s_seg = filtered ? s_pass : s_all;
  const int last_kept = filtered ? last_pass : last_all;

  // scan of the segment sums
  constexpr int PER = kDecMaxSegs / kWave;     // 16 segments per lane
  float mine = 0.f;
  #pragma unroll
  for (int j = 0; j < PER; ++j) mine += s_seg[lane * PER + j];
  const float incl = dec_wave_scan(mine, lane);
  const float total = __shfl(incl, kWave - 1, kWave);
  const float target = u[b] * total;
  const unsigned long long hit = __ballot(incl > target);
  int chosen = last_kept;
  if (hit != 0ull) {
    const int L = __ffsll((long long)hit) - 1;
    float acc = L > 0 ? __shfl(incl, L - 1, kWave) : 0.f;
    int seg = L * PER + PER - 1;
    for (int j = 0; j < PER; ++j) {
      const float nxt = acc + s_seg[L * PER + j];
      if (nxt > target) { seg = L * PER + j; break; }
      acc = nxt;
    }
    // walk segment seg in ascending order from the running sum acc; if
    // rounding keeps the walk below the target, the segment's last kept
    // entry is taken
    int found = -1, seg_last = -1;
    for (int it = 0; it < iters && found < 0; ++it) {
      const long e0 = (long)seg * seg_len + (long)it * CH + lane * VEC;
      float wk[VEC];
      float lsum = 0.f;
      #pragma unroll
      for (int i = 0; i < VEC; ++i) wk[i] = 0.f;
      if (e0 < V) {
        float l[VEC];
        load(e0, l);
        #pragma unroll
        for (int i = 0; i < VEC; ++i) {
          float wa, wp; bool cand, pass;
          weigh(e0 + i, l[i], wa, wp, cand, pass);
          wk[i] = filtered ? wp : wa;
          if (filtered ? pass : cand) seg_last = (int)(e0 + i);
          lsum += wk[i];
        }
      }
      const float lincl = dec_wave_scan(lsum, lane);
      float run = acc + (lincl - lsum);
      int my = INT_MAX;
      #pragma unroll
      for (int i = 0; i < VEC; ++i) {
        run += wk[i];
        if (my == INT_MAX && wk[i] > 0.f && run > target) my = (int)(e0 + i);
      }
      const unsigned long long got = __ballot(my != INT_MAX);
      if (got != 0ull) found = __shfl(my, __ffsll((long long)got) - 1, kWave);
      acc += __shfl(lincl, kWave - 1, kWave);
    }
    seg_last = dec_wave_max_i(seg_last);
    chosen = found >= 0 ? found : (seg_last >= 0 ? seg_last : last_kept);
  }
  // no candidate at all (V == 1 and it is unk): index 0
  chosen = min(max(chosen, 0), V - 1);
  if (lane == 0) {
    out_ids[(long)b * id_stride] = chosen;
    out_logp[(long)b * logp_stride] = row[chosen] - lse;
  }
}

void decode_sample(at::Tensor logits, at::Tensor partials, at::Tensor u,
                   double temperature, double min_p, long unk,
                   at::Tensor out_ids, at::Tensor out_logp,
                   c10::optional<at::Tensor> cut) {
  CI_CHECK_CUDA(logits); CI_CHECK_CUDA(partials); CI_CHECK_CUDA(u);
  CI_CHECK_CUDA(out_ids); CI_CHECK_CUDA(out_logp);
  CI_CHECK_CONTIG(logits); CI_CHECK_CONTIG(partials); CI_CHECK_CONTIG(u);
  TORCH_CHECK(logits.dim() == 2 &&
              logits.scalar_type() == at::ScalarType::Float,
              "logits must be fp32 (B,V)");
  const long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(B > 0 && V > 0, "decode_sample: empty input");
  TORCH_CHECK(V <= INT_MAX, "decode_sample: V exceeds INT_MAX");
  const long NT = (V + kDecTileV - 1) / kDecTileV;
  TORCH_CHECK(partials.scalar_type() == at::ScalarType::Float &&
              partials.numel() == B * NT * 2,
              "partials must be fp32 (B, ceil(V/64), 2)");
  TORCH_CHECK(u.scalar_type() == at::ScalarType::Float && u.numel() == B,
              "u must be fp32 (B,)");
  TORCH_CHECK(temperature > 0, "temperature must be > 0");
  TORCH_CHECK(min_p >= 0 && min_p <= 1, "min_p must be in [0, 1]");
  TORCH_CHECK(unk >= -1 && unk < V, "unk must be in [-1, V)");
  TORCH_CHECK(out_ids.scalar_type() == at::ScalarType::Long &&
              out_ids.dim() == 1 && out_ids.size(0) == B,
              "out_ids must be an int64 (B,) view");
  TORCH_CHECK(out_logp.scalar_type() == at::ScalarType::Float &&
              out_logp.dim() == 1 && out_logp.size(0) == B,
              "out_logp must be an fp32 (B,) view");
  TORCH_CHECK(out_ids.stride(0) >= 0 && out_logp.stride(0) >= 0,
              "output strides must be non-negative");
  const bool has_cut = cut.has_value() && cut->defined();
  if (has_cut) {
    CI_CHECK_CUDA(*cut); CI_CHECK_CONTIG(*cut);
    TORCH_CHECK(cut->scalar_type() == at::ScalarType::Float &&
                cut->numel() == B, "cut must be fp32 (B,)");
  }
  auto launch = [&](auto vec, auto with_cut) {
    constexpr int VEC = decltype(vec)::value;
    constexpr bool CUT = decltype(with_cut)::value;
    constexpr long CH = kWave * VEC;
    const long iters = std::max<long>(1, (V + CH * kDecMaxSegs - 1) /
                                             (CH * kDecMaxSegs));
    const long seg_len = CH * iters;
    const long nseg = (V + seg_len - 1) / seg_len;
    hipLaunchKernelGGL((decode_sample_kernel<VEC, CUT>), dim3(B),
        dim3(kDecThreads), 0, stream(), logits.data_ptr<float>(),
        partials.data_ptr<float>(), u.data_ptr<float>(),
        CUT ? cut->data_ptr<float>() : nullptr,
        out_ids.data_ptr<int64_t>(), (long)out_ids.stride(0),
        out_logp.data_ptr<float>(), (long)out_logp.stride(0), (int)V, (int)NT,
        (int)iters, (int)nseg, (float)(1.0 / temperature), (float)min_p,
        (int)unk);
  };
  // float4 reads need every row of the logits 16-B aligned
  auto with_vec = [&](auto with_cut) {
    if (V % 4 == 0 && reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0)
      launch(std::integral_constant<int, 4>{}, with_cut);
    else
      launch(std::integral_constant<int, 1>{}, with_cut);
  };
  if (has_cut) with_vec(std::true_type{});
  else with_vec(std::false_type{});
}

// ---- cutoff ----------------------------------------------------------------
// The logit at which the top-k / nucleus set of a row ends. One workgroup of
// 1024 threads per row; thread t keeps entries t, t + 1024, ... as
// order-preserving 32-bit keys in registers (kCutRegs of them: the only read
// of the row from HBM), longer rows re-read the rest through L2. unk and the
// padding get key 0, below every real key.
//
// A search finds the largest key x whose measure S(x) over {key >= x} reaches
// a target: S = count, target k (top-k); S = sum exp(l - max), target
// top_p * S(min key) (nucleus). Two phases:
//   1. histogram passes over the whole row. The bracket [lo, hi) is cut into
//      kCutBins bins (edges linear in the logit, or linear in the key after
//      a pass that did not halve the key span); every thread adds its entries, in ascending
//      entry order, to bins of its own in LDS; a bin is summed over the
//      threads by the wave butterfly and then over the 16 waves in ascending
//      order; the bins are walked from the top one down. The bracket becomes
//      the bin in which the running sum reaches the target, and the sum above
//      it is carried. Repeated until the bracket holds at most kCutCap
//      entries or a single key.
//   2. the bracket's entries are compacted into LDS in entry order (ballot
//      prefix, no atomics) and the key range is bisected there, each probe
//      summing the entries >= x per thread in ascending order, then by the
//      same butterfly and wave order, onto the carried sum.
// Every sum has one order, fixed by V and the bracket, and an entry below the
// probe contributes nothing to it, so each phase's predicate is monotone in x
// (a rounded add is monotone in both operands) and the result is a key of the
// row. Phase 1 sums the same entries in another order than phase 2; if
// rounding makes them disagree, the bracket's lowest key is the answer.
constexpr int kCutThreads = 1024;
constexpr int kCutWaves = kCutThreads / kWave;
constexpr int kCutRegs = 60;           // cached entries per thread
constexpr int kCutBins = 14;
constexpr int kCutCap = kCutBins * kCutThreads / 2;   // (key, weight) pairs

static __device__ __forceinline__ uint32_t dec_key(float l) {
  const uint32_t b = __float_as_uint(l);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

static __device__ __forceinline__ float dec_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <typename T>
static __device__ __forceinline__ T cut_wave_sum(T v) {
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// wave butterfly, then the 16 wave results in ascending wave order
template <typename T>
static __device__ __forceinline__ T cut_block_sum(T v, T* s_red) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  v = cut_wave_sum(v);
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  T r = s_red[0];
  for (int i = 1; i < kCutWaves; ++i) r += s_red[i];
  return r;
}

static __device__ __forceinline__ uint32_t cut_block_max(uint32_t v,
                                                         uint32_t* s_red) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  #pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
    v = max(v, (uint32_t)__shfl_xor((int)v, off, kWave));
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  uint32_t r = s_red[0];
  for (int i = 1; i < kCutWaves; ++i) r = max(r, s_red[i]);
  return r;
}

struct CutShared {
  uint32_t buf[kCutBins * kCutThreads];   // bins[b][thread] / keys | weights
  uint32_t edge[17];                      // bin b = [edge[b], edge[b + 1])
  uint32_t wred[kCutWaves][kCutBins];
  uint32_t tot[kCutBins];
  uint32_t red[kCutWaves];
};

// T = uint32_t: count, T = float: mass. `keys` are the thread's cached
// entries, `row` / `V` / `unk` serve the entries past them. Preconditions:
// lo < hi, S(lo) >= target > S(hi) = 0 (hi is above every key).
template <typename T>
static __device__ __forceinline__ uint32_t cut_search(const uint32_t (&keys)[kCutRegs],
                                      int nreg, const float* __restrict__ row,
                                      int V, int unk, float m, uint32_t lo,
                                      uint32_t hi, T target, float top_p,
                                      CutShared& sh) {
  constexpr bool MASS = std::is_same<T, float>::value;
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  T* bins = reinterpret_cast<T*>(sh.buf);
  T* wred = reinterpret_cast<T*>(&sh.wred[0][0]);
  T* tot = reinterpret_cast<T*>(sh.tot);
  T* red = reinterpret_cast<T*>(sh.red);

  // f(key) for every entry of the thread, ascending entry index
  auto for_each = [&](auto&& f) {
    #pragma unroll
    for (int j = 0; j < kCutRegs; ++j)
      if (j < nreg) f(keys[j]);
    for (long e = (long)kCutRegs * kCutThreads + tid; e < V; e += kCutThreads)
      f(e == unk ? 0u : dec_key(row[e]));
  };
  auto weight = [&](uint32_t key) -> T {
    if constexpr (MASS) return expf(dec_unkey(key) - m);
    else return 1u;
  };

  T above = T(0);
  bool first = MASS, key_edges = false;
  for (;;) {
    if (hi - lo == 1) return lo;
    // how many entries the bracket holds, per wave
    uint32_t n_wave = 0;
    for_each([&](uint32_t key) {
      n_wave += __popcll(__ballot(key >= lo && key < hi));
    });
    __syncthreads();
    if (lane == 0) sh.red[wave] = n_wave;
    __syncthreads();
    uint32_t n_act = 0, wave_off = 0;
    for (int i = 0; i < kCutWaves; ++i) {
      if (i == wave) wave_off = n_act;
      n_act += sh.red[i];
    }
    if (n_act <= kCutCap && !first) {
      // phase 2: compact in entry order, then bisect in LDS
      uint32_t* s_key = sh.buf;
      T* s_w = reinterpret_cast<T*>(sh.buf + kCutCap);
      __syncthreads();
      uint32_t pos = wave_off;
      for_each([&](uint32_t key) {
        const bool act = key >= lo && key < hi;
        const unsigned long long mask = __ballot(act);
        if (act) s_key[pos + __popcll(mask & ((1ull << lane) - 1))] = key;
        pos += __popcll(mask);
      });
      __syncthreads();
      if constexpr (MASS)
        for (uint32_t i = tid; i < n_act; i += kCutThreads)
          s_w[i] = weight(s_key[i]);
      __syncthreads();
      while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        T s = T(0);
        for (uint32_t i = tid; i < n_act; i += kCutThreads)
          if (s_key[i] >= mid) s += MASS ? s_w[i] : T(1);
        s = cut_block_sum(s, red);
        if (above + s >= target) lo = mid; else hi = mid;
      }
      return lo;
    }
    // phase 1: one histogram pass over [lo, hi)
    if (tid == 0) {
      const float flo = dec_unkey(lo), fhi = dec_unkey(hi - 1);
      sh.edge[0] = lo;
      for (int i = 1; i < kCutBins; ++i) {
        const uint32_t c = key_edges
            ? lo + (uint32_t)(((uint64_t)(hi - lo) * i) / kCutBins)
            : dec_key(flo + (fhi - flo) * ((float)i / kCutBins));
        sh.edge[i] = min(max(c, sh.edge[i - 1]), hi);
      }
      for (int i = kCutBins; i < 17; ++i) sh.edge[i] = hi;
    }
    #pragma unroll
    for (int b = 0; b < kCutBins; ++b) bins[b * kCutThreads + tid] = T(0);
    __syncthreads();
    for_each([&](uint32_t key) {
      if (key >= lo && key < hi) {
        int b = key >= sh.edge[8] ? 8 : 0;
        b += key >= sh.edge[b + 4] ? 4 : 0;
        b += key >= sh.edge[b + 2] ? 2 : 0;
        b += key >= sh.edge[b + 1] ? 1 : 0;
        bins[b * kCutThreads + tid] += weight(key);
      }
    });
    #pragma unroll
    for (int b = 0; b < kCutBins; ++b) {
      const T v = cut_wave_sum(bins[b * kCutThreads + tid]);
      if (lane == 0) wred[wave * kCutBins + b] = v;
    }
    __syncthreads();
    if (tid < kCutBins) {
      T r = wred[tid];
      for (int i = 1; i < kCutWaves; ++i) r += wred[i * kCutBins + tid];
      tot[tid] = r;
    }
    __syncthreads();
    if (first) {
      // the nucleus target: top_p of the candidates' mass, summed as below
      T z = above;
      for (int b = kCutBins - 1; b >= 0; --b) z += tot[b];
      target = T(top_p) * z;
      first = false;
    }
    // bin 0 if rounding keeps the walk below the target (see above)
    int pick = 0;
    T acc = above;
    for (int b = kCutBins - 1; b >= 1; --b) {
      const T nxt = acc + tot[b];
      if (nxt >= target) { pick = b; break; }
      acc = nxt;
    }
    const uint32_t nlo = sh.edge[pick], nhi = sh.edge[pick + 1];
    // not halved: cut by key next time, so two passes always halve the span
    key_edges = nhi - nlo > (hi - lo) / 2;
    above = acc;
    lo = nlo;
    hi = nhi;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCutThreads) void decode_cutoff_kernel(
    const float* __restrict__ logits,          // (B,V)
    float* __restrict__ out,                   // (B)
    int V, long k, float top_p, int unk) {
  __shared__ CutShared sh;
  const int tid = threadIdx.x;
  const float* row = logits + (long)blockIdx.x * V;
  const int nreg = (int)min((long)kCutRegs,
                            ((long)V + kCutThreads - 1) / kCutThreads);
  uint32_t keys[kCutRegs];
  uint32_t kmax = 0, kmin = 0xffffffffu, n = 0;
  auto see = [&](uint32_t key) {
    if (key != 0u) {
      kmax = max(kmax, key);
      kmin = min(kmin, key);
      ++n;
    }
  };
  #pragma unroll
  for (int j = 0; j < kCutRegs; ++j) {
    const long e = (long)j * kCutThreads + tid;
    keys[j] = (e < V && e != unk) ? dec_key(row[e]) : 0u;
    see(keys[j]);
  }
  for (long e = (long)kCutRegs * kCutThreads + tid; e < V; e += kCutThreads)
    see(e == unk ? 0u : dec_key(row[e]));
  kmax = cut_block_max(kmax, sh.red);
  kmin = ~cut_block_max(~kmin, sh.red);
  n = cut_block_sum(n, sh.red);
  uint32_t cut = 0;                            // key 0: nothing filters
  if (n > 0 && kmax != 0xffffffffu) {
    if (k >= 1 && k < (long)n)
      cut = cut_search<uint32_t>(keys, nreg, row, V, unk, 0.f, kmin, kmax + 1,
                                 (uint32_t)k, 0.f, sh);
    if (top_p > 0.f) {
      __syncthreads();
      const uint32_t cp = cut_search<float>(keys, nreg, row, V, unk,
                                            dec_unkey(kmax), kmin, kmax + 1,
                                            0.f, top_p, sh);
      cut = max(cut, cp);
    }
  }
  if (tid == 0) out[blockIdx.x] = cut == 0u ? -INFINITY : dec_unkey(cut);
}

void decode_cutoff(at::Tensor logits, long k, double top_p, long unk,
                   at::Tensor out) {
  CI_CHECK_CUDA(logits); CI_CHECK_CUDA(out);
  CI_CHECK_CONTIG(logits); CI_CHECK_CONTIG(out);
  TORCH_CHECK(logits.dim() == 2 &&
              logits.scalar_type() == at::ScalarType::Float,
              "logits must be fp32 (B,V)");
  const long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(B > 0 && V > 0, "decode_cutoff: empty input");
  TORCH_CHECK(V <= INT_MAX, "decode_cutoff: V exceeds INT_MAX");
  TORCH_CHECK(k >= 0, "top_k must be >= 1 (0: no top-k filter)");
  TORCH_CHECK(top_p >= 0 && top_p <= 1,
              "top_p must be in (0, 1] (0: no nucleus filter)");
  TORCH_CHECK(unk >= -1 && unk < V, "unk must be in [-1, V)");
  TORCH_CHECK(out.scalar_type() == at::ScalarType::Float && out.numel() == B,
              "out must be fp32 (B,)");
  hipLaunchKernelGGL(decode_cutoff_kernel, dim3(B), dim3(kCutThreads), 0,
      stream(), logits.data_ptr<float>(), out.data_ptr<float>(), (int)V, k,
      (float)top_p, (int)unk);
}

}  // namespace ci
