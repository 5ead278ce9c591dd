// K2 serve variant: fused GEMV + cell kernel for small batches
// (SURVEY.md §2.4 "persistent-LSTM variant for small B serve path").
//
// At B<=8 (single-request serving) the recurrent step is a GEMV bound by
// streaming the 46 MB weight matrix; tiling for MFMA is pointless. One
// block per hidden unit j: its four waves compute the four gate dot
// products <h_b, W[g*H+j,:]> with lane-split K (coalesced 16-B row reads,
// wave shfl reduction), then lane 0 finishes the cell and stores
// h/c/gates — a single launch per timestep replaces hipBLASLt GEMV +
// pointwise kernel. Grid = H blocks (2400 at the deployed shape) fills
// all 256 CUs; batch rows loop inside the block (B tiny).
#include "lstm_cell.h"

namespace ci {

typedef __bf16 bf16x8g __attribute__((ext_vector_type(8)));

constexpr int BMAX = 8;  // dispatch guarantees B <= 8

// ---- weight-row loaders: one row of W_hh as fp32, W elements per lane-step
struct RowBf16 {
  static constexpr int W = 8;
  const __hip_bfloat16* row;
  __device__ __forceinline__ void load(int k, float* w) const {
    const bf16x8g v = *reinterpret_cast<const bf16x8g*>(row + k);
    #pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = (float)v[e];
  }
  __device__ __forceinline__ float at(int k) const { return ld(row + k); }
  __device__ __forceinline__ float scaled(float a) const { return a; }
};

struct RowFp8 {  // e4m3 row with its per-row scale
  static constexpr int W = 16;
  const unsigned char* row;
  float scale;
  __device__ __forceinline__ void load(int k, float* w) const {
    const uint4 q = *reinterpret_cast<const uint4*>(row + k);  // 16 fp8
    fp8x4_to_f32(q.x, w);
    fp8x4_to_f32(q.y, w + 4);
    fp8x4_to_f32(q.z, w + 8);
    fp8x4_to_f32(q.w, w + 12);
  }
  __device__ __forceinline__ float at(int k) const {
    float w1[4];
    fp8x4_to_f32((unsigned int)row[k], w1);  // low byte -> w1[0]
    return w1[0];
  }
  __device__ __forceinline__ float scaled(float a) const { return a * scale; }
};

// dots[b][wave] = <h_prev[b,:], wrow> for this wave's gate row, all b < B:
// lane-split K, shfl reduction. Callers __syncthreads() before reading dots.
template <typename WRow>
static __device__ __forceinline__ void gemv_dots(
    float (*dots)[4], const WRow& wrow,
    const __hip_bfloat16* __restrict__ h_prev, long h_rs, int B, int H) {
  constexpr int W = WRow::W;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int Hv = H / W * W;
  // read each W element ONCE; accumulate all batch rows simultaneously
  // (h rows are tiny and L2-resident; W is the 46 MB stream)
  float acc[BMAX];
  #pragma unroll
  for (int b = 0; b < BMAX; ++b) acc[b] = 0.f;
  // acc[] must be register-resident: unroll over BMAX with a guard so
  // every index is compile-time (runtime-indexed arrays go to scratch —
  // CDNA guide §5.4 rule 20)
  for (int k = lane * W; k < Hv; k += 64 * W) {
    float wf[W];
    wrow.load(k, wf);
    #pragma unroll
    for (int b = 0; b < BMAX; ++b) {
      if (b >= B) break;
      #pragma unroll
      for (int v = 0; v < W; v += 8) {
        const bf16x8g hv = *reinterpret_cast<const bf16x8g*>(
            h_prev + (long)b * h_rs + k + v);
        #pragma unroll
        for (int e = 0; e < 8; ++e) acc[b] += wf[v + e] * (float)hv[e];
      }
    }
  }
  for (int k = Hv + lane; k < H; k += 64) {
    const float wv = wrow.at(k);
    #pragma unroll
    for (int b = 0; b < BMAX; ++b) {
      if (b >= B) break;
      acc[b] += wv * ld(h_prev + (long)b * h_rs + k);
    }
  }
  #pragma unroll
  for (int b = 0; b < BMAX; ++b) {
    if (b >= B) break;
    float a = wrow.scaled(acc[b]);
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      a += __shfl_down(a, off);
    if (lane == 0) dots[b][wave] = a;
  }
}

// the block's first B threads finish hidden unit j from its four dots
static __device__ __forceinline__ void gemv_finish(
    const float (*dots)[4], int j,
    const __hip_bfloat16* __restrict__ xp, long xp_rs,
    const float* __restrict__ bias,
    const float* __restrict__ c_prev, long cp_rs,
    __hip_bfloat16* __restrict__ h_out, long ho_rs,
    float* __restrict__ c_out, long co_rs,
    __hip_bfloat16* __restrict__ gates_out, long go_rs, int B, int H) {
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const Cell r = lstm_cell_at<CellFma::IG>(
        dots[b][0], dots[b][1], dots[b][2], dots[b][3],
        xp + (long)b * xp_rs + j, bias + j, H, c_prev[(long)b * cp_rs + j]);
    store_cell(r, h_out + (long)b * ho_rs + j, c_out + (long)b * co_rs + j,
               gates_out + (long)b * go_rs + j, H);
  }
}

__global__ __launch_bounds__(256) void lstm_cell_gemv(
    const __hip_bfloat16* __restrict__ h_prev, long h_rs,
    const __hip_bfloat16* __restrict__ w_hh,   // (4H, H) row-major
    const __hip_bfloat16* __restrict__ xp, long xp_rs,
    const float* __restrict__ bias,
    const float* __restrict__ c_prev, long cp_rs,
    __hip_bfloat16* __restrict__ h_out, long ho_rs,
    float* __restrict__ c_out, long co_rs,
    __hip_bfloat16* __restrict__ gates_out, long go_rs,
    int B, int H) {
  const int j = blockIdx.x;          // hidden unit
  const int wave = threadIdx.x >> 6; // gate g in {i,f,g,o}
  __shared__ float dots[BMAX][4];
  gemv_dots(dots, RowBf16{w_hh + (long)(wave * H + j) * H}, h_prev, h_rs, B, H);
  __syncthreads();
  gemv_finish(dots, j, xp, xp_rs, bias, c_prev, cp_rs, h_out, ho_rs,
              c_out, co_rs, gates_out, go_rs, B, H);
}

// ---- persistent whole-sequence variant (CI_SERVE_PERSISTENT) ------------
// One launch per LAYER instead of one per timestep: the grid stays
// resident and a software grid barrier separates timesteps (NOTES r1
// item 2: the cross-timestep persistent grid aiming at the ~3 ms
// weight-stream floor; ~2x T x n_layers launch overheads removed).
// Safety: the spin has a hard cap — on overflow the kernel sets a fail
// flag and EXITS instead of hanging the GPU; the host falls back to the
// per-step path when the flag is set. Grid size = occupancy-derived
// resident capacity (all blocks must be co-resident for the barrier).
//
// MEASURED NEGATIVE (kept as a documented experiment, opt-in only):
// at the deployed shape the barrier itself costs ~50 us/step — the
// generation counter bounces across all 8 XCDs' L2s — so the best
// persistent config (nb=256, 15.4 ms at T=300) is ~4.7x SLOWER than
// per-step launches (3.3 ms). gpurun_out/r2m_pers.log /
// profiles/BENCH_HISTORY.md. Also: hipOccupancyMaxActiveBlocks
// overestimates by 1 block/CU here (claimed 7, 6 resident), hence the
// safety margin below.

__device__ __forceinline__ bool grid_sync_capped(unsigned int* cnt,
                                                 unsigned int* gen,
                                                 unsigned int nb) {
  __syncthreads();
  __shared__ int ok_s;
  if (threadIdx.x == 0) {
    ok_s = 1;
    __threadfence();                       // publish this block's writes
    const unsigned int g = atomicAdd(gen, 0u);   // read generation FIRST
    if (atomicAdd(cnt, 1u) == nb - 1) {
      atomicExch(cnt, 0u);
      __threadfence();
      atomicAdd(gen, 1u);                  // release the cohort
    } else {
      long spins = 0;
      while (atomicAdd(gen, 0u) == g) {
        __builtin_amdgcn_s_sleep(32);
        if (++spins > (1 << 20)) { ok_s = 0; break; }  // bail, don't hang
      }
    }
    __threadfence();                       // acquire: invalidate caches
  }
  __syncthreads();
  return ok_s != 0;
}

__global__ __launch_bounds__(256) void lstm_seq_gemv_persistent(
    const __hip_bfloat16* __restrict__ h0, long h_rs,
    const __hip_bfloat16* __restrict__ w_hh,
    const __hip_bfloat16* __restrict__ xp,
    const float* __restrict__ bias,
    const float* __restrict__ c0, long cp_rs,
    __hip_bfloat16* __restrict__ hs,
    float* __restrict__ cs,
    __hip_bfloat16* __restrict__ gates_out,
    unsigned int* __restrict__ barrier_ws,   // [cnt, gen]
    int* __restrict__ fail_flag,
    int B, int H, int T) {
  const unsigned int NB = gridDim.x;
  const int wave = threadIdx.x >> 6;
  __shared__ float dots[BMAX][4];
  for (int t = 0; t < T; ++t) {
    const __hip_bfloat16* hp = (t == 0) ? h0 : hs + (long)(t - 1) * B * H;
    const float* cp = (t == 0) ? c0 : cs + (long)(t - 1) * B * H;
    const long h_prev_rs = (t == 0) ? h_rs : (long)H;
    const long c_prev_rs = (t == 0) ? cp_rs : (long)H;
    for (int j = blockIdx.x; j < H; j += NB) {
      gemv_dots(dots, RowBf16{w_hh + (long)(wave * H + j) * H}, hp, h_prev_rs,
                B, H);
      __syncthreads();
      gemv_finish(dots, j, xp + (long)t * B * 4 * H, (long)4 * H, bias,
                  cp, c_prev_rs, hs + (long)t * B * H, (long)H,
                  cs + (long)t * B * H, (long)H,
                  gates_out + (long)t * B * 4 * H, (long)4 * H, B, H);
      __syncthreads();  // dots reused by the next j of this block
    }
    if (!grid_sync_capped(barrier_ws, barrier_ws + 1, NB)) {
      if (threadIdx.x == 0) atomicExch(fail_flag, 1);
      return;
    }
  }
}

// whole-sequence driver over time-major (T,B,·) saves, one launch/step.
void lstm_seq_forward_gemv(at::Tensor xp, at::Tensor bias, at::Tensor h0,
                           at::Tensor c0, at::Tensor w_hh, at::Tensor hs,
                           at::Tensor cs, at::Tensor gates) {
  TORCH_CHECK(xp.scalar_type() == at::ScalarType::BFloat16,
              "gemv cell kernel is bf16");
  TORCH_CHECK(w_hh.is_contiguous(), "w_hh must be contiguous");
  const SeqSteps<__hip_bfloat16> s(xp, bias, h0, c0, hs, cs, gates, w_hh.size(1));
  const int B = s.B, H = s.H;
  TORCH_CHECK(B <= 8, "gemv cell kernel is for B <= 8 (got ", B, ")");
  auto* wp = reinterpret_cast<const __hip_bfloat16*>(w_hh.data_ptr());
  for (int t = 0; t < s.T; ++t) {
    hipLaunchKernelGGL(lstm_cell_gemv, dim3(H), dim3(256), 0, stream(),
        s.h_prev(t), (long)H, wp, s.xp_at(t), (long)4 * H, s.bias(),
        s.c_prev(t), (long)H, s.h_out(t), (long)H, s.c_out(t), (long)H,
        s.gates_at(t), (long)4 * H, B, H);
  }
}

// persistent driver: ONE launch for the whole sequence. Returns the grid
// size used, or 0 when a co-resident grid is not available (caller falls
// back to the per-step driver). ws = int32[4] zeroed workspace
// [cnt, gen, fail, pad]; caller checks ws[2] after the stream syncs.
long lstm_seq_forward_gemv_persistent(at::Tensor xp, at::Tensor bias,
                                      at::Tensor h0, at::Tensor c0,
                                      at::Tensor w_hh, at::Tensor hs,
                                      at::Tensor cs, at::Tensor gates,
                                      at::Tensor ws) {
  CI_CHECK_CONTIG(ws);
  TORCH_CHECK(xp.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(w_hh.is_contiguous(), "w_hh must be contiguous");
  TORCH_CHECK(ws.numel() >= 4 && ws.scalar_type() == at::ScalarType::Int);
  const SeqSteps<__hip_bfloat16> s(xp, bias, h0, c0, hs, cs, gates, w_hh.size(1));
  const int B = s.B, H = s.H;
  TORCH_CHECK(B <= 8, "gemv persistent kernel is for B <= 8");
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &per_cu, reinterpret_cast<const void*>(&lstm_seq_gemv_persistent),
          256, 0) != hipSuccess || per_cu < 1) {
    return 0;
  }
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  per_cu = std::max(1, per_cu - 1);  // measured: API claims 7/CU, 6 resident
  long nb = std::min<long>((long)per_cu * cus, H);
  if (const char* env = getenv("CI_PERS_NB")) {   // residency experiments
    nb = std::min<long>(std::max(1L, atol(env)), H);
  }
  hipLaunchKernelGGL(lstm_seq_gemv_persistent, dim3(nb), dim3(256), 0,
      stream(),
      s.h_prev(0), (long)H,
      reinterpret_cast<const __hip_bfloat16*>(w_hh.data_ptr()),
      s.xp_at(0), s.bias(), s.c_prev(0), (long)H,
      s.h_out(0), s.c_out(0), s.gates_at(0),
      reinterpret_cast<unsigned int*>(ws.data_ptr()),
      reinterpret_cast<int*>(ws.data_ptr()) + 2, B, H, s.T);
  return nb;
}

// ---- fp8 (OCP e4m3) weight variant --------------------------------------
// Serving is bound by streaming W_hh (46 MB/layer-step at the deployed
// shape); storing W as e4m3 with per-row scales halves that stream.
// Hardware unpack: __builtin_amdgcn_cvt_pk_f32_fp8 converts packed fp8
// pairs at VALU rate. Opt-in (CI_SERVE_FP8W=1), eval-path only.
// fp8x4_to_f32 unpack helper now lives in common.h (shared with ce.hip)

__global__ __launch_bounds__(256) void lstm_cell_gemv_fp8(
    const __hip_bfloat16* __restrict__ h_prev, long h_rs,
    const unsigned char* __restrict__ w8,      // (4H, H) e4m3
    const float* __restrict__ wscale,          // (4H) per-row scales
    const __hip_bfloat16* __restrict__ xp, long xp_rs,
    const float* __restrict__ bias,
    const float* __restrict__ c_prev, long cp_rs,
    __hip_bfloat16* __restrict__ h_out, long ho_rs,
    float* __restrict__ c_out, long co_rs,
    __hip_bfloat16* __restrict__ gates_out, long go_rs,
    int B, int H) {
  const int j = blockIdx.x;
  const int row = (threadIdx.x >> 6) * H + j;
  __shared__ float dots[BMAX][4];
  gemv_dots(dots, RowFp8{w8 + (long)row * H, wscale[row]}, h_prev, h_rs, B, H);
  __syncthreads();
  gemv_finish(dots, j, xp, xp_rs, bias, c_prev, cp_rs, h_out, ho_rs,
              c_out, co_rs, gates_out, go_rs, B, H);
}

void lstm_seq_forward_gemv_fp8(at::Tensor xp, at::Tensor bias, at::Tensor h0,
                               at::Tensor c0, at::Tensor w8, at::Tensor wscale,
                               at::Tensor hs, at::Tensor cs, at::Tensor gates) {
  CI_CHECK_CONTIG(w8);
  TORCH_CHECK(xp.scalar_type() == at::ScalarType::BFloat16,
              "fp8 gemv kernel is bf16-activation only");
  TORCH_CHECK(w8.scalar_type() == at::ScalarType::Byte,
              "w8 must hold e4m3 bytes (uint8)");
  const SeqSteps<__hip_bfloat16> s(xp, bias, h0, c0, hs, cs, gates, w8.size(1));
  const int B = s.B, H = s.H;
  TORCH_CHECK(B <= 8, "fp8 gemv kernel is for B <= 8");
  for (int t = 0; t < s.T; ++t) {
    hipLaunchKernelGGL(lstm_cell_gemv_fp8, dim3(H), dim3(256), 0, stream(),
        s.h_prev(t), (long)H, w8.data_ptr<unsigned char>(),
        wscale.data_ptr<float>(), s.xp_at(t), (long)4 * H, s.bias(),
        s.c_prev(t), (long)H, s.h_out(t), (long)H, s.c_out(t), (long)H,
        s.gates_at(t), (long)4 * H, B, H);
  }
}

}  // namespace ci
