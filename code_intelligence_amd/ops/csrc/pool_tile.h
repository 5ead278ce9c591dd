// Thread map and window rule shared by the concat-pool kernels (pool.hip,
// pool_stream.hip).
#pragma once

#include "common.h"

#include <cstdint>

namespace ci {

// Thread map: a 256-thread block is HL h-lanes x TS t-slices; consecutive
// lanes own consecutive 16-B packets of h (VEC = 16/sizeof(T), or VEC = 1
// scalars when H or a stride is not packet-aligned), so every access is a run
// of HL*16 contiguous bytes in either layout. B*H/VEC alone is only ~3k lanes
// at the fine-tune shape (32 x 800 bf16), far too few to cover HBM latency,
// so the T loop is split over the TS slices of a block.
template <int VEC> struct PoolTile {
  static constexpr int HL = VEC == 1 ? 64 : 16;  // h lanes per block
  static constexpr int TS = 256 / HL;            // t slices per block
};

// Row b is pooled over t in [lo, len): len = clamp(lengths[b], 1, Tn),
// lo = max(0, len - max_len) (0 when max_len <= 0, i.e. "no window").
static __device__ __forceinline__ void pool_window(const int* lengths, int b,
                                                   int Tn, int max_len,
                                                   int& lo, int& len) {
  len = min(max(lengths[b], 1), Tn);
  lo = max_len > 0 ? max(0, len - max_len) : 0;
}

// 16-B packets need every packet start 16-B aligned in both tensors
template <typename T>
static bool pool_can_vec(const void* p, int H, long sb, long st) {
  constexpr int VEC = 16 / sizeof(T);
  return H % VEC == 0 && sb % VEC == 0 && st % VEC == 0 &&
         reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

}  // namespace ci
