// K2 (lib mode): LSTM cell pointwise kernels + C++ sequence drivers.
// The recurrent GEMM runs through hipBLASLt (at::mm) per timestep; the gate
// activation + c/h update (and their backward) are fused HIP kernels.
// Reference semantics: fastai AWD_LSTM nn.LSTM cell, gate order i,f,g,o
// (/root/reference/Issue_Embeddings/train.py:88-92).
#include "lstm_cell.h"

#include <hip/hip_fp8.h>

namespace ci {

// |h| < 1 exactly (sigmoid * tanh), so the fp8 copy of the hidden state
// uses a FIXED scale of 1/448: h8 = e4m3(h * 448), dequant h = h8/448.
// Emitted by the cell kernel for free (CI_LSTM_FP8 recurrent GEMM path).
constexpr float kH8Scale = 448.0f;

void quantize_e4m3(at::Tensor src, at::Tensor dst, at::Tensor scale);  // fp8util.hip

// VEC consecutive j per thread with 16-B vector loads/stores (ldv/stv in
// common.h) over columns [j0, j0 + ncol); the H % VEC columns left over run
// the same body with VECTOR = false (VEC = 1).

// one thread per (b, j-block): gates = xp + rec (+bias); c' = f*c + i*g;
// h' = o*tanh(c')
template <typename T, bool VECTOR>
__global__ void lstm_cell_fwd(
    const T* __restrict__ xp, long xp_rs,      // (B,4H) view, row stride xp_rs
    const T* __restrict__ rec, long rec_rs,    // (B,4H) recurrent GEMM out
    const float* __restrict__ bias,            // (4H) b_ih + b_hh
    const float* __restrict__ c_prev, long cp_rs,
    T* __restrict__ h_out, long h_rs,
    float* __restrict__ c_out, long c_rs,
    T* __restrict__ gates_out, long g_rs,      // post-activation i,f,g,o
    unsigned char* __restrict__ h8_out,        // optional e4m3(h*448)
    int B, int H, int j0, int ncol) {
  constexpr int VEC = VECTOR ? 16 / (int)sizeof(T) : 1;
  constexpr CellFma FMA = VECTOR ? CellFma::IG : CellFma::FC;
  const int nv = ncol / VEC;  // column blocks per row
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * nv) return;
  const int b = idx / nv, j = j0 + (idx % nv) * VEC;
  const long xo = (long)b * xp_rs + j;
  const long ro = (long)b * rec_rs + j;
  float gi[VEC], gf[VEC], gg[VEC], go[VEC], tmp[VEC], cprev[VEC];
  ldv<T, VEC>(xp + xo, gi); ldv<T, VEC>(rec + ro, tmp);
  #pragma unroll
  for (int e = 0; e < VEC; ++e) gi[e] = (tmp[e] + gi[e]) + bias[j + e];
  ldv<T, VEC>(xp + xo + H, gf); ldv<T, VEC>(rec + ro + H, tmp);
  #pragma unroll
  for (int e = 0; e < VEC; ++e) gf[e] = (tmp[e] + gf[e]) + bias[j + H + e];
  ldv<T, VEC>(xp + xo + 2 * H, gg); ldv<T, VEC>(rec + ro + 2 * H, tmp);
  #pragma unroll
  for (int e = 0; e < VEC; ++e) gg[e] = (tmp[e] + gg[e]) + bias[j + 2 * H + e];
  ldv<T, VEC>(xp + xo + 3 * H, go); ldv<T, VEC>(rec + ro + 3 * H, tmp);
  #pragma unroll
  for (int e = 0; e < VEC; ++e) go[e] = (tmp[e] + go[e]) + bias[j + 3 * H + e];
  ldv_f32<VEC>(c_prev + (long)b * cp_rs + j, cprev);
  float c[VEC], h[VEC];
  #pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const Cell r = lstm_cell<FMA>(gi[e], gf[e], gg[e], go[e], cprev[e]);
    gi[e] = r.i; gf[e] = r.f; gg[e] = r.g; go[e] = r.o; c[e] = r.c; h[e] = r.h;
  }
  if (h8_out != nullptr) {
    unsigned char q[VEC];
    #pragma unroll
    for (int e = 0; e < VEC; ++e)
      q[e] = __hip_fp8_e4m3(h[e] * kH8Scale).__x;
    unsigned char* h8 = h8_out + (long)b * h_rs + j;
    if constexpr (VEC == 8) {
      *reinterpret_cast<uint2*>(h8) = *reinterpret_cast<const uint2*>(q);
    } else if constexpr (VEC == 4) {
      *reinterpret_cast<unsigned int*>(h8) =
          *reinterpret_cast<const unsigned int*>(q);
    } else {
      *h8 = q[0];
    }
  }
  store_cells<T, VEC>(h, c, gi, gf, gg, go, h_out + (long)b * h_rs + j,
                      c_out + (long)b * c_rs + j,
                      gates_out + (long)b * g_rs + j, H);
}

// backward pointwise: consumes dh_ext (upstream) + dh_rec (t+1 GEMM),
// running dc (fp32, in/out), saved post-act gates, c_{t-1}, c_t.
template <typename T, bool VECTOR>
__global__ void lstm_cell_bwd(
    const T* __restrict__ dh_ext, long dhe_rs,
    const T* __restrict__ dh_rec, long dhr_rs,
    float* __restrict__ dc_buf, long dc_rs,    // in: dc_t ; out: dc_{t-1}
    const T* __restrict__ gates, long g_rs,
    const float* __restrict__ c_prev, long cp_rs,
    const float* __restrict__ c_t, long ct_rs,
    T* __restrict__ dgates, long dg_rs,
    float* __restrict__ dgates32,              // optional unrounded copy, (B,4H)
    int B, int H) {
  constexpr int VEC = VECTOR ? 16 / (int)sizeof(T) : 1;
  const int Hv = H / VEC;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * Hv) return;
  const int b = idx / Hv, j = (idx % Hv) * VEC;
  const long go_ = (long)b * g_rs + j;
  float gi[VEC], gf[VEC], gg[VEC], gout[VEC], dh[VEC], tmp[VEC];
  float ct[VEC], cprev[VEC], dcin[VEC];
  if (VECTOR) {
    ldv<T, VEC>(gates + go_, gi);
    ldv<T, VEC>(gates + go_ + H, gf);
    ldv<T, VEC>(gates + go_ + 2 * H, gg);
    ldv<T, VEC>(gates + go_ + 3 * H, gout);
    ldv<T, VEC>(dh_ext + (long)b * dhe_rs + j, dh);
    ldv<T, VEC>(dh_rec + (long)b * dhr_rs + j, tmp);
    ldv_f32<VEC>(c_t + (long)b * ct_rs + j, ct);
    ldv_f32<VEC>(c_prev + (long)b * cp_rs + j, cprev);
    ldv_f32<VEC>(dc_buf + (long)b * dc_rs + j, dcin);
  } else {
    gi[0] = ld(gates + go_); gf[0] = ld(gates + go_ + H);
    gg[0] = ld(gates + go_ + 2 * H); gout[0] = ld(gates + go_ + 3 * H);
    dh[0] = ld(dh_ext + (long)b * dhe_rs + j);
    tmp[0] = ld(dh_rec + (long)b * dhr_rs + j);
    ct[0] = c_t[(long)b * ct_rs + j];
    cprev[0] = c_prev[(long)b * cp_rs + j];
    dcin[0] = dc_buf[(long)b * dc_rs + j];
  }
  float dgi[VEC], dgf[VEC], dgg[VEC], dgo[VEC], dcout[VEC];
  #pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const float dhe = dh[e] + tmp[e];
    const float tct = tanhf(ct[e]);
    const float do_ = dhe * tct;
    const float dct = dcin[e] + dhe * gout[e] * (1.f - tct * tct);
    dgi[e] = dct * gg[e] * gi[e] * (1.f - gi[e]);
    dgf[e] = dct * cprev[e] * gf[e] * (1.f - gf[e]);
    dgg[e] = dct * gi[e] * (1.f - gg[e] * gg[e]);
    dgo[e] = do_ * gout[e] * (1.f - gout[e]);
    dcout[e] = dct * gf[e];
  }
  const long dgo_ = (long)b * dg_rs + j;
  if (VECTOR) {
    stv_f32<VEC>(dc_buf + (long)b * dc_rs + j, dcout);
    stv<T, VEC>(dgates + dgo_, dgi);
    stv<T, VEC>(dgates + dgo_ + H, dgf);
    stv<T, VEC>(dgates + dgo_ + 2 * H, dgg);
    stv<T, VEC>(dgates + dgo_ + 3 * H, dgo);
  } else {
    dc_buf[(long)b * dc_rs + j] = dcout[0];
    st(dgates + dgo_, dgi[0]);
    st(dgates + dgo_ + H, dgf[0]);
    st(dgates + dgo_ + 2 * H, dgg[0]);
    st(dgates + dgo_ + 3 * H, dgo[0]);
  }
  if (dgates32 != nullptr) {
    float* d32 = dgates32 + (long)b * 4 * H + j;
    #pragma unroll
    for (int e = 0; e < VEC; ++e) {
      d32[e] = dgi[e]; d32[H + e] = dgf[e];
      d32[2 * H + e] = dgg[e]; d32[3 * H + e] = dgo[e];
    }
  }
}

// 64-thread blocks quadruple the workgroup count (the deployed shape
// yields only 600 WGs at 256 threads = 2.3/CU and the kernel is
// latency-bound; measured 432.3 vs 435.2 ms/step e2e at 64 vs 256) —
// CI_CELL_THREADS overrides. Forward and backward cell kernels share it.
static int cell_threads() {
  static const int threads = [] {
    const char* e = getenv("CI_CELL_THREADS");
    return e ? atoi(e) : 64;
  }();
  return threads;
}

// step t of s from rec = h_prev @ w_hh^T: a vector launch over the H / VEC
// column blocks, a scalar launch over the H % VEC columns that remain
template <typename ST>
static void launch_fwd_step(const SeqSteps<ST>& s, int t, const at::Tensor& rec,
                            unsigned char* h8_base = nullptr) {
  const int threads = cell_threads();
  constexpr int VEC = 16 / sizeof(ST);
  const int B = s.B, H = s.H, nvec = H / VEC * VEC;
  unsigned char* h8p = h8_base ? h8_base + (long)t * B * H : nullptr;
  auto launch = [&](auto kern, int j0, int ncol, int per_thread) {
    hipLaunchKernelGGL(kern,
        dim3(ceil_div((long)B * (ncol / per_thread), threads)), dim3(threads),
        0, stream(),
        s.xp_at(t), (long)4 * H, reinterpret_cast<const ST*>(rec.data_ptr()),
        (long)4 * H, s.bias(), s.c_prev(t), (long)H, s.h_out(t), (long)H,
        s.c_out(t), (long)H, s.gates_at(t), (long)4 * H, h8p, B, H, j0, ncol);
  };
  if (nvec > 0) launch(lstm_cell_fwd<ST, true>, 0, nvec, VEC);
  if (H > nvec) launch(lstm_cell_fwd<ST, false>, nvec, H - nvec, 1);
}

// hs,cs,gates are (T,B,·) preallocated; xp (T,B,4H); h0 (B,H); c0 fp32 (B,H).
void lstm_seq_forward_lib(at::Tensor xp, at::Tensor bias, at::Tensor h0,
                          at::Tensor c0, at::Tensor w_hh, at::Tensor hs,
                          at::Tensor cs, at::Tensor gates) {
  auto w_hh_t = w_hh.t();
  CI_DISPATCH_FB(xp.scalar_type(), "lstm_seq_forward_lib", [&] {
    const SeqSteps<scalar_t> s(xp, bias, h0, c0, hs, cs, gates, w_hh.size(1));
    auto rec = at::empty({s.B, 4 * s.H}, xp.options());
    for (int t = 0; t < s.T; ++t) {
      at::mm_out(rec, t == 0 ? h0 : hs.select(0, t - 1), w_hh_t);
      launch_fwd_step(s, t, rec);
    }
  });
}

// fp8 recurrent GEMM variant (CI_LSTM_FP8): the per-timestep GEMM runs
// at::_scaled_mm with an e4m3 weight (quantized once per layer-forward by
// the caller) and the e4m3 hidden state the cell kernel emitted at t-1
// with the fixed 1/448 scale (|h| < 1). Measured 28.2 vs 35.0 us/call at
// the deployed shape (scripts/lstm_fp8_probe.py). Backward is unchanged
// (bf16 saves).
void lstm_seq_forward_lib_fp8(at::Tensor xp, at::Tensor bias, at::Tensor h0,
                              at::Tensor c0, at::Tensor w8, at::Tensor wscale,
                              at::Tensor hs, at::Tensor cs, at::Tensor gates) {
  CI_CHECK_CONTIG(w8);
  TORCH_CHECK(xp.scalar_type() == at::ScalarType::BFloat16,
              "fp8 recurrent path is bf16-activation only");
  TORCH_CHECK(w8.scalar_type() == at::ScalarType::Float8_e4m3fn);
  const SeqSteps<__hip_bfloat16> s(xp, bias, h0, c0, hs, cs, gates, w8.size(1));
  const int T = s.T, B = s.B, H = s.H;
  auto w8_t = w8.t();  // (H, 4H) column-major for _scaled_mm mat2
  auto rec = at::empty({B, 4 * H}, xp.options());
  auto hs8 = at::empty({T, B, H},
                       xp.options().dtype(at::ScalarType::Float8_e4m3fn));
  auto h8_scale = at::full({}, 1.0 / 448.0,
                           xp.options().dtype(at::ScalarType::Float));
  // t=0: quantize the incoming h0 with the same fixed scale
  auto h0_8 = at::empty({B, H},
                        xp.options().dtype(at::ScalarType::Float8_e4m3fn));
  quantize_e4m3(h0.contiguous(), h0_8, h8_scale);
  auto* h8_base = reinterpret_cast<unsigned char*>(hs8.data_ptr());
  for (int t = 0; t < T; ++t) {
    auto h8_prev = (t == 0) ? h0_8 : hs8.select(0, t - 1);
    at::_scaled_mm_out(rec, h8_prev, w8_t, h8_scale, wscale,
                       c10::nullopt, c10::nullopt,
                       at::ScalarType::BFloat16, false);
    launch_fwd_step(s, t, rec, h8_base);
  }
}

// reverse loop over (T,B,·) time-major saves; dh0/dc0 are (B,H) fp32 outs.
void lstm_seq_backward(at::Tensor dhs, at::Tensor dhT, at::Tensor dcT,
                       at::Tensor gates, at::Tensor hs, at::Tensor cs,
                       at::Tensor c0, at::Tensor w_hh, at::Tensor dgates,
                       at::Tensor dh0, at::Tensor dc0, bool need_dh0) {
  CI_CHECK_CUDA(dhs); CI_CHECK_CONTIG(dhs); CI_CHECK_CONTIG(dgates);
  CI_CHECK_CONTIG(c0);
  const int T = dhs.size(0), B = dhs.size(1);
  const int H = w_hh.size(1);
  auto dc_buf = dcT.clone(at::MemoryFormat::Contiguous);  // (B,H) fp32 running dc
  // clone, not contiguous(): mm_out below overwrites dh_rec every step and
  // contiguous() would alias the caller's gradient tensor
  auto dh_rec = dhT.clone(at::MemoryFormat::Contiguous);  // (B,H) running rec grad
  // one 46 MB transpose buys the NT GEMM layout for all T steps:
  // mm(dgates, w_hh) NN measured 304 TF vs 503 TF as mm(dgates, w_t.t())
  // (scripts/gemm_probe.py on MI355X)
  auto w_hh_tc = w_hh.t().contiguous();
  auto w_hh_nt = w_hh_tc.t();
  const int threads = cell_threads();
  CI_DISPATCH_FB(dhs.scalar_type(), "lstm_seq_backward", [&] {
    constexpr int VEC = 16 / sizeof(scalar_t);
    const bool vec_ok = (H % VEC) == 0;
    const int blocks = ceil_div((long)B * (vec_ok ? H / VEC : H), threads);
    // dh0 is an fp32 output, so the last step's GEMM must not start from
    // the bf16-stored dgates (a 2^-9 error per product that shows wherever
    // the 4H-term sum cancels): step 0 also emits its dgates unrounded and
    // dh0 = dgates32 @ w_hh runs in fp32. Callers whose h0 needs no
    // gradient (the trainer detaches carried state) skip that GEMM.
    const bool lowp = dhs.scalar_type() != at::ScalarType::Float;
    at::Tensor dg32;
    if (lowp && need_dh0)
      dg32 = at::empty({B, 4 * H}, dhs.options().dtype(at::ScalarType::Float));
    for (int t = T - 1; t >= 0; --t) {
      const float* cprev = (t == 0) ? c0.data_ptr<float>()
                                    : cs.data_ptr<float>() + (long)(t - 1) * B * H;
      auto kern = vec_ok ? lstm_cell_bwd<scalar_t, true>
                         : lstm_cell_bwd<scalar_t, false>;
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, stream(),
          reinterpret_cast<const scalar_t*>(dhs.data_ptr()) + (long)t * B * H, (long)H,
          reinterpret_cast<const scalar_t*>(dh_rec.data_ptr()), (long)H,
          dc_buf.data_ptr<float>(), (long)H,
          reinterpret_cast<const scalar_t*>(gates.data_ptr()) + (long)t * B * 4 * H, (long)4 * H,
          cprev, (long)H,
          cs.data_ptr<float>() + (long)t * B * H, (long)H,
          reinterpret_cast<scalar_t*>(dgates.data_ptr()) + (long)t * B * 4 * H, (long)4 * H,
          (t == 0 && dg32.defined()) ? dg32.data_ptr<float>() : nullptr,
          B, H);
      // dh_{t-1} recurrent contribution: dgates_t @ w_hh (NT layout,
      // contiguous A thanks to time-major dgates)
      if (t > 0 || (need_dh0 && !lowp))
        at::mm_out(dh_rec, dgates.select(0, t), w_hh_nt);
    }
    if (need_dh0) {
      if (lowp) dh0.copy_(at::mm(dg32, w_hh.to(at::ScalarType::Float)));
      else dh0.copy_(dh_rec);
    }
  });
  dc0.copy_(dc_buf);
}

}  // namespace ci
