// neighbors_wide.hip — exact brute-force k-nearest-neighbour search for 1 <= K <= 512.
//
// neighbors.hip keeps a query's running top list as one sorted key per lane of a wave, so
// it ends at K = 64.  Here the lists live in LDS and a whole workgroup serves one query
// group (docs/KNN_WIDE.md):
//  * a workgroup of 4 waves owns the QPW = 8 queries of one group (they share a split).
//    A ROUND is 256 rows of the feature-major table XT[d, n]: wave w takes rows
//    [base + 64 w, base + 64 w + 64), one row per lane, and accumulates the 8 distances of
//    its row with the chain of ``k_knn`` (wave-uniform query values, feature order, the
//    shared ``accum``) -- the accumulator of a (query, row) pair is bit-equal to k_knn's;
//  * per query, LDS holds REGION = 960 keys (dist_bits << 32 | row): the sorted top list
//    [0, Kp), Kp = K rounded up to a power of two, and behind it an unsorted candidate
//    buffer of CAP = 960 - Kp >= 448 keys;
//  * filter and append: a lane whose key is below the query's K-th key (top[K - 1]; +inf
//    while fewer than K rows were kept) appends it: ballot, popcount prefix, one integer
//    LDS counter bump per wave.  Rows that are not TRAIN in the split never enter;
//  * flush: when some buffer could not take another full round (count + 256 > CAP) --
//    each wave knows the count after its own bump, and the largest of those is the final
//    count, so an OR over the workgroup barrier decides it uniformly -- all 256 threads
//    sort every buffer with a bitonic network, merge its first Kp keys into the top list
//    with one more bitonic merge, and empty the buffers.  The network is the all-ascending
//    form (first step of a merge mirrors, partner = i ^ (k - 1), the rest halve,
//    partner = i ^ j; the smaller key always goes to the lower slot): slots past a
//    query's real length behave as +inf without being stored, because a compare-exchange
//    never moves +inf down -- pairs whose upper slot is past the length are skipped;
//  * the result is the K smallest of a set of unique keys, so the order in which waves
//    append cannot change it.  No floating-point atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knn_common.h"
#include "wave_ops.h"

namespace {

using dml::knn::accum;
using dml::knn::kInf;
using dml::knn::QPW;
using dml::wave::lane_id;

constexpr int WAVES = 4;              // waves per workgroup
constexpr int THREADS = 64 * WAVES;
constexpr int ROUND = THREADS;        // rows per round, one per thread
constexpr int REGION = 960;           // keys per query: top list [0, Kp) + buffer [Kp, REGION)
constexpr int KP_MAX = 512;
static_assert(REGION - KP_MAX >= ROUND, "an empty buffer takes one round");
static_assert(QPW * REGION * 8 + QPW * 4 <= 64 * 1024, "LDS budget");

// One compare-exchange step over every query's array keys[q * REGION + off ...]: ``half``
// (a power of two) pairs per query, merge block ``k``, distance ``j`` (j == k / 2: the
// mirror step).  Slots >= len(q) are virtual +inf.
template <typename Len>
__device__ __forceinline__ void net_step(uint64_t* keys, int off, int half, int k, int j, Len len, int tid) {
  const int lh = __builtin_ctz(half);
  for (int item = tid; item < QPW * half; item += THREADS) {
    const int q = item >> lh, t = item & (half - 1);
    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const int hi = (j == (k >> 1)) ? (lo ^ (k - 1)) : (lo | j);
    if (hi < len(q)) {
      uint64_t* a = keys + q * REGION + off;
      const uint64_t x = a[lo], y = a[hi];
      if (y < x) {
        a[lo] = y;
        a[hi] = x;
      }
    }
  }
  __syncthreads();
}

// Buffers -> top lists.  Called by all threads after a barrier that follows the last
// append; ``cnt`` does not change until the reset at the end.
__device__ void flush(uint64_t* keys, int* cnt, int Kp, int tid) {
  int cmax = 0;
#pragma unroll
  for (int i = 0; i < QPW; ++i) cmax = cnt[i] > cmax ? cnt[i] : cmax;
  if (cmax == 0) return;   // workgroup-uniform
  int P = 2;
  while (P < cmax) P <<= 1;
  // sort each buffer ascending (P virtual slots, cnt[q] real ones)
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1)
      net_step(keys, Kp, P >> 1, k, j, [&](int q) { return cnt[q]; }, tid);
  // merge the block [top list | first Kp keys of the buffer]; its lower half is the new top list
  for (int j = Kp; j >= 1; j >>= 1)
    net_step(keys, 0, Kp, 2 * Kp, j, [&](int q) { return Kp + (cnt[q] < Kp ? cnt[q] : Kp); }, tid);
  if (tid < QPW) cnt[tid] = 0;
  __syncthreads();
}

template <int METRIC>
__global__ __launch_bounds__(THREADS) void k_knn_wide(const float* __restrict__ X, const float* __restrict__ XT,
                                                      int64_t n, int64_t d, const uint8_t* __restrict__ roles,
                                                      const int32_t* __restrict__ qrow,
                                                      const int32_t* __restrict__ qsplit, float p, int32_t K,
                                                      int32_t Kp, float* __restrict__ out_d,
                                                      int32_t* __restrict__ out_i) {
  __shared__ uint64_t keys[QPW * REGION];
  __shared__ int cnt[QPW];
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = tid >> 6;
  const int64_t group = blockIdx.x;
  const int split = __builtin_amdgcn_readfirstlane(qsplit[group * QPW]);
  int q[QPW];
#pragma unroll
  for (int i = 0; i < QPW; ++i) q[i] = __builtin_amdgcn_readfirstlane(qrow[group * QPW + i]);
  const uint8_t* role = roles + (int64_t)split * n;

#pragma unroll
  for (int i = 0; i < QPW; ++i)
    for (int t = tid; t < Kp; t += THREADS) keys[i * REGION + t] = kInf;
  if (tid < QPW) cnt[tid] = 0;
  __syncthreads();

  const int cap = REGION - Kp;
  for (int64_t base = 0; base < n; base += ROUND) {
    const int64_t j = base + 64 * wave + lane;
    const bool valid = j < n && role[j < n ? j : 0] == 1;
    float acc[QPW];
#pragma unroll
    for (int i = 0; i < QPW; ++i) acc[i] = 0.f;
    if (j < n) {
      for (int64_t f = 0; f < d; ++f) {
        const float x = XT[f * n + j];
#pragma unroll
        for (int i = 0; i < QPW; ++i) {
          const float qv = q[i] >= 0 ? X[(int64_t)q[i] * d + f] : 0.f;
          acc[i] = accum<METRIC>(acc[i], x, qv, p);
        }
      }
    }
    bool full = false;   // wave-uniform: some buffer cannot take another round
#pragma unroll
    for (int i = 0; i < QPW; ++i) {
      const uint64_t key = (valid && q[i] >= 0) ? dml::knn::make_key(dml::knn::key_distance<METRIC>(acc[i]), j) : kInf;
      const uint64_t thr = keys[i * REGION + K - 1];
      const bool pass = key < thr;
      const uint64_t m = __builtin_amdgcn_ballot_w64(pass);
      if (m != 0) {
        const int add = __builtin_popcountll(m);
        int at = 0;
        if (lane == 0) at = atomicAdd(&cnt[i], add);
        at = __builtin_amdgcn_readfirstlane(at);
        const int pre = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (pass) keys[i * REGION + Kp + at + pre] = key;   // at + add <= cap: the flush rule below
        full |= at + add + ROUND > cap;
      }
    }
    // the wave that bumped a counter last saw its final value, so the OR is "some final
    // count + ROUND > cap" -- the same for every thread
    if (__syncthreads_or(full ? 1 : 0)) flush(keys, cnt, Kp, tid);
  }
  __syncthreads();
  flush(keys, cnt, Kp, tid);

  for (int t = tid; t < QPW * K; t += THREADS) {
    const int i = t / K, c = t - i * K;
    const int64_t slot = group * QPW + i;
    if (qrow[slot] < 0) continue;
    const uint64_t k = keys[i * REGION + c];
    out_d[slot * K + c] = k == kInf ? __builtin_inff() : __builtin_bit_cast(float, (uint32_t)(k >> 32));
    out_i[slot * K + c] = k == kInf ? -1 : (int32_t)(uint32_t)k;
  }
}

}  // namespace

// The arguments of ``dml_knn`` (neighbors.hip), for 1 <= K <= 512: qrow/qsplit [nq_groups * 8]
// (qrow -1 = padding), out_d/out_i [nq_groups * 8, K] ascending in (distance bits, row id);
// slots past the number of TRAIN rows hold +inf / -1.
extern "C" int dml_knn_wide(const float* X, const float* XT, int64_t n, int64_t d, const uint8_t* roles,
                            const int32_t* qrow, const int32_t* qsplit, int64_t nq_groups, int32_t metric, float p,
                            int32_t K, float* out_d, int32_t* out_i, hipStream_t st) {
  if (K < 1 || K > KP_MAX || nq_groups <= 0) return nq_groups == 0 ? 0 : 2;
  int32_t Kp = 1;
  while (Kp < K) Kp <<= 1;
  const unsigned blocks = (unsigned)nq_groups;
  switch (metric) {
    case 0: k_knn_wide<0><<<blocks, THREADS, 0, st>>>(X, XT, n, d, roles, qrow, qsplit, p, K, Kp, out_d, out_i); break;
    case 1: k_knn_wide<1><<<blocks, THREADS, 0, st>>>(X, XT, n, d, roles, qrow, qsplit, p, K, Kp, out_d, out_i); break;
    case 2: k_knn_wide<2><<<blocks, THREADS, 0, st>>>(X, XT, n, d, roles, qrow, qsplit, p, K, Kp, out_d, out_i); break;
    case 4: k_knn_wide<4><<<blocks, THREADS, 0, st>>>(X, XT, n, d, roles, qrow, qsplit, p, K, Kp, out_d, out_i); break;
    default: k_knn_wide<3><<<blocks, THREADS, 0, st>>>(X, XT, n, d, roles, qrow, qsplit, p, K, Kp, out_d, out_i); break;
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
