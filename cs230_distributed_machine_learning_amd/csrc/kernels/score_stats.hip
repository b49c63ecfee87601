// score_stats.hip -- the statistics every label / sum based scorer needs, for all fits of a batch
// in one launch (multi-metric GridSearchCV scoring; docs/MULTIMETRIC.md).
//
// The held-out row ids and predictions of F fits lie concatenated (fit f owns entries
// [fit_row_off[f], fit_row_off[f + 1])).  grid.y is the fit and grid.x tiles that fit's entries
// in tiles of kTile; a block whose tile starts past its fit's end returns, so fits of unequal
// size (CV folds and a holdout split together) share one launch.
//
//   classification   out int64 [F][C * C + 1]: the confusion matrix cm[t * C + p], then the number
//                    of entries that could not be counted (a prediction or target outside [0, C),
//                    a row id outside [0, n)).  Counts leave a block as 64-bit integer atomics:
//                    integer sums are the same bits in any order.
//                      C <= kSmallC  k_fit_stats_cls_reg<C>: C * C compare-and-count registers per
//                                    lane (fully unrolled), summed over the wave by xor-shuffles
//                      C <= 64       k_fit_stats_cls_lds: one LDS histogram of C * C counters per
//                                    wave (ds_add_u32), 4 * C * C * 4 bytes <= 64 KiB
//   regression       out double [F][14] (kRegSlots; the table in docs/MULTIMETRIC.md).  No
//                    floating-point atomics: a lane adds its entries in order, the lanes of a wave
//                    are added by the xor-shuffle tree, the four waves ascending, and the block
//                    writes its 14 partials; k_fit_stats_reg_reduce adds a fit's blocks in block
//                    order.  ../runtime/score_stats_cpu.cpp adds in the same order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "wave_ops.h"

namespace dml {

#define FS_PTR(T, v) ((T*)(__attribute__((address_space(1))) T*)(uintptr_t)(v))

constexpr int kTile = 4096;      // entries of a fit per block (16 per lane)
constexpr int kSmallC = 4;       // register counters up to this many classes
constexpr int kMaxC = 64;        // LDS histograms up to this many classes
constexpr int kRegSlots = 14;
constexpr int kWantLog = 1, kWantPoisson = 2, kWantGamma = 4;

struct FitStatsArgs {
  int64_t rows;         // int32 [total]: dataset row id of every entry
  int64_t fit_row_off;  // int64 [F + 1]
  int64_t pred;         // int32 [total] class ids / float [total] values
  int64_t ycls;         // int32 [n] (classification)
  int64_t yreg;         // float [n] (regression)
  int64_t n;            // length of ycls / yreg
  int64_t C;            // classes; 0: regression
  int64_t F;
  int64_t max_rows;     // entries of the longest fit (sizes grid.x)
  int64_t want;         // regression: kWantLog | kWantPoisson | kWantGamma
  int64_t part;         // regression: double [F][ceil(max_rows / kTile)][14]
  int64_t out;
  int64_t f0;           // first fit of this launch (the entry point sets it)
};

// the tile of this block: false when it starts past the fit's end
__device__ __forceinline__ bool fs_tile(const FitStatsArgs& a, int f, int64_t* t0, int64_t* t1) {
  const int64_t* roff = FS_PTR(const int64_t, a.fit_row_off);
  const int64_t r0 = roff[f], r1 = roff[f + 1];
  *t0 = r0 + (int64_t)blockIdx.x * kTile;
  *t1 = *t0 + kTile < r1 ? *t0 + kTile : r1;
  return *t0 < r1;
}

// cell of one entry: t * C + p, or -1 when it cannot be counted
__device__ __forceinline__ int fs_cell(const FitStatsArgs& a, int64_t i, int C) {
  const int32_t row = FS_PTR(const int32_t, a.rows)[i];
  const int32_t p = FS_PTR(const int32_t, a.pred)[i];
  if ((uint64_t)(int64_t)row >= (uint64_t)a.n) return -1;
  const int32_t t = FS_PTR(const int32_t, a.ycls)[row];
  return ((uint32_t)t < (uint32_t)C && (uint32_t)p < (uint32_t)C) ? t * C + p : -1;
}

template <int C>
__global__ __launch_bounds__(256) void k_fit_stats_cls_reg(FitStatsArgs a) {
  constexpr int CC = C * C;
  __shared__ uint32_t red[4][CC + 1];
  const int f = (int)a.f0 + blockIdx.y;
  int64_t t0, t1;
  if (!fs_tile(a, f, &t0, &t1)) return;
  uint32_t cnt[CC + 1];
#pragma unroll
  for (int j = 0; j <= CC; ++j) cnt[j] = 0;
  for (int64_t i = t0 + threadIdx.x; i < t1; i += 256) {
    const int cell = fs_cell(a, i, C);
#pragma unroll
    for (int j = 0; j < CC; ++j) cnt[j] += cell == j ? 1u : 0u;
    cnt[CC] += cell < 0 ? 1u : 0u;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j <= CC; ++j) {
    const uint32_t s = wave::sum(cnt[j], lane);
    if (lane == 0) red[w][j] = s;
  }
  __syncthreads();
  if (threadIdx.x <= CC) {
    const int j = threadIdx.x;
    const unsigned long long s = (unsigned long long)red[0][j] + red[1][j] + red[2][j] + red[3][j];
    if (s) atomicAdd(FS_PTR(unsigned long long, a.out) + (int64_t)f * (CC + 1) + j, s);
  }
}

__global__ __launch_bounds__(256) void k_fit_stats_cls_lds(FitStatsArgs a) {
  extern __shared__ uint32_t fs_hist[];   // [4][C * C]
  const int C = (int)a.C, CC = C * C;
  const int f = (int)a.f0 + blockIdx.y;
  int64_t t0, t1;
  if (!fs_tile(a, f, &t0, &t1)) return;   // block-uniform: before any barrier
  for (int j = threadIdx.x; j < 4 * CC; j += 256) fs_hist[j] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t* mine = fs_hist + w * CC;
  uint32_t bad = 0;
  for (int64_t i = t0 + threadIdx.x; i < t1; i += 256) {
    const int cell = fs_cell(a, i, C);
    if (cell >= 0) atomicAdd(mine + cell, 1u);
    else bad += 1;
  }
  unsigned long long* out = FS_PTR(unsigned long long, a.out) + (int64_t)f * (CC + 1);
  bad = wave::sum(bad, lane);
  if (lane == 0 && bad) atomicAdd(out + CC, (unsigned long long)bad);
  __syncthreads();
  for (int j = threadIdx.x; j < CC; j += 256) {
    const unsigned long long s = (unsigned long long)fs_hist[j] + fs_hist[CC + j] + fs_hist[2 * CC + j] + fs_hist[3 * CC + j];
    if (s) atomicAdd(out + j, s);
  }
}

__global__ __launch_bounds__(256) void k_fit_stats_reg(FitStatsArgs a, int64_t gx) {
#pragma clang fp contract(off)
  __shared__ double red[4][kRegSlots];
  const int f = (int)a.f0 + blockIdx.y;
  int64_t t0, t1;
  if (!fs_tile(a, f, &t0, &t1)) return;
  const bool want_log = (a.want & kWantLog) != 0, want_poi = (a.want & kWantPoisson) != 0,
             want_gam = (a.want & kWantGamma) != 0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0, s8 = 0.0, s9 = 0.0,
         s10 = 0.0, s11 = 0.0, s12 = 0.0, s13 = 0.0;
  for (int64_t i = t0 + threadIdx.x; i < t1; i += 256) {
    const int32_t row = FS_PTR(const int32_t, a.rows)[i];
    if ((uint64_t)(int64_t)row >= (uint64_t)a.n) continue;   // not counted: slot 0 tells the caller
    const double y = (double)FS_PTR(const float, a.yreg)[row];
    const double p = (double)FS_PTR(const float, a.pred)[i];
    const double e = p - y, ae = fabs(e);
    s0 += 1.0;
    s1 += y;
    s2 += y * y;
    s3 += e;
    s4 += e * e;
    s5 += ae;
    s6 = fmax(s6, ae);
    s7 += ae / fmax(fabs(y), 2.220446049250313e-16);
    const bool bad_log = y <= -1.0 || p <= -1.0, bad_poi = y < 0.0 || p <= 0.0, bad_gam = y <= 0.0 || p <= 0.0;
    s9 += bad_log ? 1.0 : 0.0;
    s11 += bad_poi ? 1.0 : 0.0;
    s13 += bad_gam ? 1.0 : 0.0;
    if (want_log && !bad_log) {
      const double d = log1p(y) - log1p(p);
      s8 += d * d;
    }
    if (want_poi && !bad_poi) {
      const double xl = y > 0.0 ? y * log(y / p) : 0.0;
      s10 += 2.0 * (xl - y + p);
    }
    if (want_gam && !bad_gam) s12 += 2.0 * (log(p / y) + y / p - 1.0);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#define FS_WAVE_SUM(j, v)                     \
  {                                           \
    const double t = wave::sum(v, lane);      \
    if (lane == 0) red[w][j] = t;             \
  }
  FS_WAVE_SUM(0, s0) FS_WAVE_SUM(1, s1) FS_WAVE_SUM(2, s2) FS_WAVE_SUM(3, s3) FS_WAVE_SUM(4, s4) FS_WAVE_SUM(5, s5)
  FS_WAVE_SUM(7, s7) FS_WAVE_SUM(8, s8) FS_WAVE_SUM(9, s9) FS_WAVE_SUM(10, s10) FS_WAVE_SUM(11, s11)
  FS_WAVE_SUM(12, s12) FS_WAVE_SUM(13, s13)
#undef FS_WAVE_SUM
  s6 = fmax(s6, wave::shfl_xor<32>(s6, lane)); s6 = fmax(s6, wave::shfl_xor<16>(s6, lane));
  s6 = fmax(s6, wave::shfl_xor<8>(s6, lane)); s6 = fmax(s6, wave::shfl_xor<4>(s6, lane));
  s6 = fmax(s6, wave::shfl_xor<2>(s6, lane)); s6 = fmax(s6, wave::shfl_xor<1>(s6, lane));
  if (lane == 0) red[w][6] = s6;
  __syncthreads();
  if (threadIdx.x < kRegSlots) {
    const int j = threadIdx.x;
    const double v = j == 6 ? fmax(fmax(fmax(red[0][j], red[1][j]), red[2][j]), red[3][j])
                            : ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
    FS_PTR(double, a.part)[((int64_t)f * gx + blockIdx.x) * kRegSlots + j] = v;
  }
}

// out[f][j] = the fit's block partials added (slot 6: maximised) in block order, one thread per
// (f, j): the same sum every run.  A fit without entries gets zeros.
__global__ __launch_bounds__(256) void k_fit_stats_reg_reduce(FitStatsArgs a, int64_t gx) {
#pragma clang fp contract(off)
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= a.F * kRegSlots) return;
  const int64_t f = q / kRegSlots;
  const int j = (int)(q % kRegSlots);
  const int64_t* roff = FS_PTR(const int64_t, a.fit_row_off);
  const int64_t len = roff[f + 1] - roff[f];
  int64_t nb = len > 0 ? (len + kTile - 1) / kTile : 0;
  if (nb > gx) nb = gx;
  const double* part = FS_PTR(const double, a.part) + f * gx * kRegSlots + j;
  double acc = 0.0;
  for (int64_t b = 0; b < nb; ++b) {
    const double v = part[b * kRegSlots];
    acc = j == 6 ? fmax(acc, v) : acc + v;
  }
  FS_PTR(double, a.out)[q] = acc;
}

}  // namespace dml

using namespace dml;

extern "C" {

int dml_fit_stats_sizeof_args() { return (int)sizeof(FitStatsArgs); }
int dml_fit_stats_tile() { return kTile; }
int dml_fit_stats_small_c() { return kSmallC; }
int dml_fit_stats_max_c() { return kMaxC; }

// 0: launched; 1: a HIP error; 2: bad arguments.  Classification zeroes `out` itself.
int dml_fit_stats(FitStatsArgs* a, hipStream_t st) {
  if (a->F <= 0) return 0;
  if (!a->fit_row_off || !a->out || a->C < 0 || a->C > kMaxC || a->C == 1 || a->max_rows < 0 || a->n < 0 ||
      a->n > 2147483647LL)
    return 2;
  if (a->max_rows > 0 && (!a->rows || !a->pred || !(a->C ? a->ycls : a->yreg))) return 2;
  const int64_t gx = (a->max_rows + kTile - 1) / kTile;
  if (gx > 2147483647LL) return 2;
  const bool reg = a->C == 0;
  if (reg && gx > 0 && !a->part) return 2;
  if (!reg &&
      hipMemsetAsync((void*)(uintptr_t)a->out, 0, (size_t)a->F * (size_t)(a->C * a->C + 1) * 8, st) != hipSuccess)
    return 1;
  FitStatsArgs b = *a;
  for (int64_t f0 = 0; gx > 0 && f0 < a->F; f0 += 65535) {   // grid.y holds at most 65535 fits
    b.f0 = f0;
    const dim3 grid((unsigned)gx, (unsigned)(a->F - f0 < 65535 ? a->F - f0 : 65535));
    if (reg) k_fit_stats_reg<<<grid, 256, 0, st>>>(b, gx);
    else if (a->C == 2) k_fit_stats_cls_reg<2><<<grid, 256, 0, st>>>(b);
    else if (a->C == 3) k_fit_stats_cls_reg<3><<<grid, 256, 0, st>>>(b);
    else if (a->C == 4) k_fit_stats_cls_reg<4><<<grid, 256, 0, st>>>(b);
    else k_fit_stats_cls_lds<<<grid, 256, (size_t)(4 * a->C * a->C * 4), st>>>(b);
  }
  if (reg) {
    b.f0 = 0;
    k_fit_stats_reg_reduce<<<(unsigned)((a->F * kRegSlots + 255) / 256), 256, 0, st>>>(b, gx);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // extern "C"
