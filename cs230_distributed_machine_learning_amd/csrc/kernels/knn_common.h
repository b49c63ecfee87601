// knn_common.h — what the KNN search kernels share (neighbors.hip: one wave per query
// group, K <= 64; neighbors_wide.hip: one workgroup per query group, K <= 512): the query
// group size, the key format and the per-feature accumulation.  Both kernels run the same
// chain per (query, row) pair in feature order, so their accumulators are bit-equal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dml {
namespace knn {

constexpr int QPW = 8;           // queries per group (they share one split)
constexpr uint64_t kInf = ~0ull;

// metric: 0 squared-L2, 1 L1, 2 Linf, 3 sum |t|^p, 4 cosine (dot product of unit rows)
template <int METRIC>
__device__ __forceinline__ float accum(float acc, float x, float q, float p) {
  if constexpr (METRIC == 4) return __builtin_fmaf(x, q, acc);
  const float t = x - q;
  if constexpr (METRIC == 0) return __builtin_fmaf(t, t, acc);   // squared L2
  if constexpr (METRIC == 1) return acc + __builtin_fabsf(t);     // L1
  if constexpr (METRIC == 2) return __builtin_fmaxf(acc, __builtin_fabsf(t));   // Linf
  return acc + __powf(__builtin_fabsf(t), p);                     // general Minkowski (p-th power sum)
}

// accumulator -> the distance the key ranks by (cosine: sklearn's clip(1 - cos, 0, 2))
template <int METRIC>
__device__ __forceinline__ float key_distance(float acc) {
  if constexpr (METRIC == 4) return __builtin_fminf(__builtin_fmaxf(1.f - acc, 0.f), 2.f);
  return acc;
}

// dist_bits << 32 | row: unique per row, so the order of keys is total
__device__ __forceinline__ uint64_t make_key(float dist, int64_t row) {
  return ((uint64_t)__builtin_bit_cast(uint32_t, dist) << 32) | (uint32_t)row;
}

}  // namespace knn
}  // namespace dml
