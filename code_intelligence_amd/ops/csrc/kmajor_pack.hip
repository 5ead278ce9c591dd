// K-major operand pack + LSTM weight gradients as ONE library NN GEMM.
//
// torch.mm(dg.t(), x) hands hipBLASLt a GEMM in which neither operand is
// contiguous along the reduction dimension K = T*B. Writing the SMALL operand
// (x / h_prev, In+H columns) K-major once turns
//
//   dW_ih^T (In,4H) = xT     (In, T*B) @ dg2 (T*B, 4H)
//   dW_hh^T (H ,4H) = hprevT (H , T*B) @ dg2 (T*B, 4H)   hprev[t] = t ? hs[t-1] : h0
//
// into one plain row-major GEMM [xT ; hprevT] @ dg2 per layer (three
// launches before: dgates[0] x h0, dgates[1:] x hs[:-1], dg2 x x).
//
// pack_kmajor is a pure data move (bit-equal to src.t()): a tile of
// 16*VEC x 16*VEC elements (256 B per tile row for both dtypes) goes through
// LDS; both global sides move 16 B per lane, 16 lanes per 256-B row segment.
//
// LDS layout: rows are NOT padded. A pad that keeps the 16-B LDS writes
// aligned is a multiple of 4 dwords, and with any such row stride the
// transposed scalar reads (row = rv*VEC + e, 16 rv per wave) land 4- to
// 8-way on the same banks. Instead the 16-B slot of tile row r is XOR-ed
// with (r / VEC) & 15: the 16 rv of one read instruction then hit 16
// different slots (x 4 columns inside the slot = all 64 banks once), and a
// write still fills one whole 256-B bank row per 16 lanes.
#include "common.h"

#include <cstdint>
#include <tuple>

namespace ci {

template <typename U, bool VLD, bool VST>
__global__ __launch_bounds__(256) void pack_kmajor_kernel(
    const U* __restrict__ src, U* __restrict__ dst, long R, long C,
    long ld_dst, long row_off, long col_off) {
  constexpr int VEC = 16 / sizeof(U);
  constexpr int TILE = 16 * VEC;
  __shared__ __attribute__((aligned(16))) U tile[TILE * TILE];
  const long r0 = (long)blockIdx.x * TILE;
  const long c0 = (long)blockIdx.y * TILE;
  const int l16 = threadIdx.x & 15;   // 16-B vector inside a 256-B row
  const int grp = threadIdx.x >> 4;   // 16 rows per pass

  // global (r, c..c+VEC) -> LDS row r, swizzled slot
  #pragma unroll
  for (int i = 0; i < TILE / 16; ++i) {
    const int rl = grp + 16 * i;
    const long r = r0 + rl, c = c0 + l16 * VEC;
    __attribute__((aligned(16))) U v[VEC];
    if (VLD && r < R && c + VEC <= C) {
      *reinterpret_cast<int4*>(v) =
          *reinterpret_cast<const int4*>(src + r * C + c);
    } else {
      #pragma unroll
      for (int e = 0; e < VEC; ++e)
        v[e] = (r < R && c + e < C) ? src[r * C + c + e] : U(0);
    }
    const int slot = l16 ^ ((rl / VEC) & 15);
    *reinterpret_cast<int4*>(&tile[rl * TILE + slot * VEC]) =
        *reinterpret_cast<const int4*>(v);
  }
  __syncthreads();

  // LDS column cl, rows rv*VEC..+VEC -> dst row (row_off + c), 16 B
  #pragma unroll
  for (int i = 0; i < TILE / 16; ++i) {
    const int cl = grp + 16 * i;
    const long c = c0 + cl;
    if (c >= C) continue;
    const int slot = (cl / VEC) ^ l16;   // (rl / VEC) & 15 == l16 below
    __attribute__((aligned(16))) U v[VEC];
    #pragma unroll
    for (int e = 0; e < VEC; ++e)
      v[e] = tile[(l16 * VEC + e) * TILE + slot * VEC + (cl % VEC)];
    const long r = r0 + l16 * VEC;
    U* p = dst + (row_off + c) * ld_dst + col_off + r;
    if (VST && r + VEC <= R) {
      *reinterpret_cast<int4*>(p) = *reinterpret_cast<const int4*>(v);
    } else {
      #pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (r + e < R) p[e] = v[e];
    }
  }
}

template <typename U>
static void launch_pack(const at::Tensor& src, at::Tensor& dst, long R, long C,
                        long row_off, long col_off) {
  constexpr int VEC = 16 / sizeof(U);
  constexpr int TILE = 16 * VEC;
  const long ld = dst.size(1);
  const U* s = reinterpret_cast<const U*>(src.data_ptr());
  U* d = reinterpret_cast<U*>(dst.data_ptr());
  const bool vld = C % VEC == 0 && reinterpret_cast<uintptr_t>(s) % 16 == 0;
  const bool vst = ld % VEC == 0 && col_off % VEC == 0 &&
                   reinterpret_cast<uintptr_t>(d) % 16 == 0;
  const dim3 grid(ceil_div(R, TILE), ceil_div(C, TILE));
  TORCH_CHECK(grid.y <= 65535, "pack_kmajor: too many columns");
#define CI_PACK_LAUNCH(VLD, VST)                                            \
  hipLaunchKernelGGL((pack_kmajor_kernel<U, VLD, VST>), grid, dim3(256), 0, \
                     stream(), s, d, R, C, ld, row_off, col_off)
  if (vld && vst) CI_PACK_LAUNCH(true, true);
  else if (vld) CI_PACK_LAUNCH(true, false);
  else if (vst) CI_PACK_LAUNCH(false, true);
  else CI_PACK_LAUNCH(false, false);
#undef CI_PACK_LAUNCH
}

// dst[row_off + c, col_off + r] = src[r, c]; src dense (R, C), dst dense
// (Ctot, Rtot), same dtype (bf16 or fp32). Every element of the target
// block is written exactly once; nothing outside it is touched.
void pack_kmajor(at::Tensor src, at::Tensor dst, long row_off, long col_off) {
  CI_CHECK_CUDA(src); CI_CHECK_CUDA(dst);
  CI_CHECK_CONTIG(src); CI_CHECK_CONTIG(dst);
  TORCH_CHECK(src.dim() == 2 && dst.dim() == 2, "pack_kmajor: 2-D tensors");
  TORCH_CHECK(src.scalar_type() == dst.scalar_type(),
              "pack_kmajor: src/dst dtype mismatch");
  const long R = src.size(0), C = src.size(1);
  TORCH_CHECK(row_off >= 0 && col_off >= 0 && row_off + C <= dst.size(0) &&
              col_off + R <= dst.size(1),
              "pack_kmajor: target block outside dst");
  if (R == 0 || C == 0) return;
  switch (src.scalar_type()) {
    case at::ScalarType::BFloat16:
    case at::ScalarType::Half:   // bits only: any 2-byte type moves alike
      launch_pack<uint16_t>(src, dst, R, C, row_off, col_off); break;
    case at::ScalarType::Float:
      launch_pack<uint32_t>(src, dst, R, C, row_off, col_off); break;
    default:
      TORCH_CHECK(false, "pack_kmajor: unsupported dtype ", src.scalar_type());
  }
}

// dgates (T,B,4H), x_tm (T,B,In), hs (T,B,H), h0 (B,H), one dtype.
// Returns (dw_ih (4H,In), dw_hh (4H,H)); a gradient that is not needed is
// neither packed nor multiplied and comes back undefined (None).
std::tuple<at::Tensor, at::Tensor> lstm_weight_grads(
    at::Tensor dgates, at::Tensor x_tm, at::Tensor hs, at::Tensor h0,
    bool need_ih, bool need_hh) {
  CI_CHECK_CUDA(dgates); CI_CHECK_CONTIG(dgates); CI_CHECK_CONTIG(x_tm);
  CI_CHECK_CONTIG(hs); CI_CHECK_CONTIG(h0);
  TORCH_CHECK(dgates.dim() == 3 && x_tm.dim() == 3 && hs.dim() == 3 &&
              h0.dim() == 2, "lstm_weight_grads: bad ranks");
  const long T = dgates.size(0), B = dgates.size(1), G = dgates.size(2);
  const long In = x_tm.size(2), H = hs.size(2);
  TORCH_CHECK(G == 4 * H && x_tm.size(0) == T && x_tm.size(1) == B &&
              hs.size(0) == T && hs.size(1) == B && h0.size(0) == B &&
              h0.size(1) == H, "lstm_weight_grads: shape mismatch");
  const auto dt = dgates.scalar_type();
  TORCH_CHECK(x_tm.scalar_type() == dt && hs.scalar_type() == dt &&
              h0.scalar_type() == dt, "lstm_weight_grads: dtype mismatch");
  at::Tensor dw_ih, dw_hh;
  if (!need_ih && !need_hh) return {dw_ih, dw_hh};
  const long rows_ih = need_ih ? In : 0;
  const long rows = rows_ih + (need_hh ? H : 0);
  // transient [xT ; hprevT] (rows, T*B): freed on return
  at::Tensor packed = at::empty({rows, T * B}, dgates.options());
  if (need_ih) pack_kmajor(x_tm.view({T * B, In}), packed, 0, 0);
  if (need_hh) {
    pack_kmajor(h0, packed, rows_ih, 0);
    if (T > 1)
      pack_kmajor(hs.narrow(0, 0, T - 1).view({(T - 1) * B, H}), packed,
                  rows_ih, B);
  }
  at::Tensor dwT = at::mm(packed, dgates.view({T * B, G}));  // (rows, 4H)
  if (need_ih) {
    dw_ih = at::empty({G, In}, dgates.options());
    pack_kmajor(dwT.narrow(0, 0, In), dw_ih, 0, 0);
  }
  if (need_hh) {
    dw_hh = at::empty({G, H}, dgates.options());
    pack_kmajor(dwT.narrow(0, rows_ih, H), dw_hh, 0, 0);
  }
  return {dw_ih, dw_hh};
}

}  // namespace ci
