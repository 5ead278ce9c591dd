// What the LSTM forward kernels and their per-step drivers share
// (lstm_pointwise.hip, lstm_gemv.hip, lstm_gemm.hip): the cell body and its
// stores on the device, the step pointers and the argument check on the host.
// Gate order i,f,g,o (PyTorch/cuDNN).
#pragma once

#include "common.h"

namespace ci {

// c = f*c_prev + i*g rounds one product on its own and fuses the other into
// the add. Which one was hipcc's choice per kernel before the cell body was
// shared (read from the gfx950 ISA), and a driver's bits depend on it, so
// every kernel names the form it has always had:
//   FC: fma(f, c_prev, i*g)   scalar pointwise kernel, fused MFMA epilogue
//   IG: fma(i, g, f*c_prev)   vector pointwise kernel, the three GEMV kernels
enum class CellFma { FC, IG };

struct Cell { float i, f, g, o, c, h; };  // post-activation gates, new state

// pre-activations p* = (rec + xp) + bias, in that association
template <CellFma FMA>
static __device__ __forceinline__ Cell lstm_cell(float pi, float pf, float pg,
                                                 float po, float c_prev) {
  // contraction off: the fused form is spelled out, not left to the
  // inlining context
  #pragma clang fp contract(off)
  Cell r;
  r.i = sigmoidf_(pi); r.f = sigmoidf_(pf); r.g = tanhf(pg); r.o = sigmoidf_(po);
  r.c = FMA == CellFma::FC ? __builtin_fmaf(r.f, c_prev, r.i * r.g)
                           : __builtin_fmaf(r.i, r.g, r.f * c_prev);
  r.h = r.o * tanhf(r.c);
  return r;
}

// the cell of one (b, j): rec* are the four recurrent dot products, xp and
// bias point at column j of gate i (the other gates follow at stride H)
template <CellFma FMA, typename T>
static __device__ __forceinline__ Cell lstm_cell_at(
    float rec_i, float rec_f, float rec_g, float rec_o, const T* xp,
    const float* bias, int H, float c_prev) {
  return lstm_cell<FMA>((rec_i + ld(xp)) + bias[0],
                        (rec_f + ld(xp + H)) + bias[H],
                        (rec_g + ld(xp + 2 * H)) + bias[2 * H],
                        (rec_o + ld(xp + 3 * H)) + bias[3 * H], c_prev);
}

// store one cell; h, c and gates point at column j of row b
template <typename T>
static __device__ __forceinline__ void store_cell(const Cell& r, T* h, float* c,
                                                  T* gates, int H) {
  st(h, r.h);
  *c = r.c;
  st(gates, r.i);
  st(gates + H, r.f);
  st(gates + 2 * H, r.g);
  st(gates + 3 * H, r.o);
}

// VEC consecutive cells of one row, one vector store per tensor and gate
template <typename T, int VEC>
static __device__ __forceinline__ void store_cells(
    const float* h, const float* c, const float* gi, const float* gf,
    const float* gg, const float* go, T* h_out, float* c_out, T* gates, int H) {
  stv<T, VEC>(h_out, h);
  stv_f32<VEC>(c_out, c);
  stv<T, VEC>(gates, gi);
  stv<T, VEC>(gates + H, gf);
  stv<T, VEC>(gates + 2 * H, gg);
  stv<T, VEC>(gates + 3 * H, go);
}

// ---- host side -----------------------------------------------------------

// What every forward driver requires of (xp, h0, c0, hs, cs, gates): xp, hs,
// cs, gates time-major (T,B,·) and dense, c0 dense fp32 (B,H), shapes agreeing
// with H = w_hh.size(1). h0 may be strided: SeqSteps packs it.
static inline void check_seq_args(const at::Tensor& xp, const at::Tensor& c0,
                                  const at::Tensor& hs, const at::Tensor& cs,
                                  const at::Tensor& gates, long H) {
  CI_CHECK_CUDA(xp); CI_CHECK_CUDA(c0); CI_CHECK_CUDA(hs); CI_CHECK_CUDA(cs);
  CI_CHECK_CUDA(gates);
  CI_CHECK_CONTIG(xp); CI_CHECK_CONTIG(c0); CI_CHECK_CONTIG(hs);
  CI_CHECK_CONTIG(cs); CI_CHECK_CONTIG(gates);
  TORCH_CHECK(c0.scalar_type() == at::ScalarType::Float, "c0 must be fp32");
  TORCH_CHECK(xp.dim() == 3 && xp.size(2) == 4 * H, "xp must be (T,B,4H)");
  const long T = xp.size(0), B = xp.size(1);
  TORCH_CHECK(c0.sizes() == at::IntArrayRef({B, H}), "c0 must be (B,H)");
  TORCH_CHECK(hs.sizes() == at::IntArrayRef({T, B, H}), "hs must be (T,B,H)");
  TORCH_CHECK(cs.sizes() == at::IntArrayRef({T, B, H}), "cs must be (T,B,H)");
  TORCH_CHECK(gates.sizes() == at::IntArrayRef({T, B, 4 * H}),
              "gates must be (T,B,4H)");
}

// Checked, typed step pointers of one driver call. TIME-MAJOR layout: slice t
// of xp/hs/cs/gates is a contiguous (B,·) block, so every kernel gets unit
// row strides H and 4H. Step 0 reads h0/c0, step t > 0 the outputs of t-1.
template <typename ST>
struct SeqSteps {
  int T, B, H;
  SeqSteps(const at::Tensor& xp, const at::Tensor& bias, const at::Tensor& h0,
           const at::Tensor& c0, at::Tensor& hs, at::Tensor& cs,
           at::Tensor& gates, long H_)
      : h0_(h0.contiguous()) {
    check_seq_args(xp, c0, hs, cs, gates, H_);
    T = xp.size(0); B = xp.size(1); H = H_;
    xp_ = reinterpret_cast<const ST*>(xp.data_ptr());
    bias_ = bias.data_ptr<float>();
    c0_ = c0.data_ptr<float>();
    hs_ = reinterpret_cast<ST*>(hs.data_ptr());
    cs_ = cs.data_ptr<float>();
    gates_ = reinterpret_cast<ST*>(gates.data_ptr());
  }
  const float* bias() const { return bias_; }
  const ST* xp_at(int t) const { return xp_ + (long)t * B * 4 * H; }
  ST* h_out(int t) const { return hs_ + (long)t * B * H; }
  float* c_out(int t) const { return cs_ + (long)t * B * H; }
  ST* gates_at(int t) const { return gates_ + (long)t * B * 4 * H; }
  const ST* h_prev(int t) const {
    return t == 0 ? reinterpret_cast<const ST*>(h0_.data_ptr()) : h_out(t - 1);
  }
  const float* c_prev(int t) const { return t == 0 ? c0_ : c_out(t - 1); }

 private:
  at::Tensor h0_;  // packed copy (or h0 itself) kept alive for h_prev(0)
  const ST* xp_;
  const float* bias_;
  const float* c0_;
  ST* hs_;
  float* cs_;
  ST* gates_;
};

}  // namespace ci
