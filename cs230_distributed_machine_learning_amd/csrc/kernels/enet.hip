// enet.hip -- batched Gram coordinate descent for Lasso / ElasticNet (docs/ELASTIC_NET.md).
//
// sklearn's enet_coordinate_descent_gram (sklearn/linear_model/_cd_fast.pyx): float64, cyclic,
// started from w = 0, for F problems in one launch.  The problems of a grid search share a few
// Gram matrices (one per split and fit_intercept), so Q stays in L2 while every
// (candidate, split) pair walks it.
//
// One wave owns one problem and there is no workgroup barrier: H = Q w and w live in the wave's
// slice of LDS, lane l owns entries l, l + 64, ... of both and is the only lane that ever reads
// or writes them.  A coordinate step reads the row Q[ii] from global memory (coalesced), the
// step's scalars (w[ii], H[ii]) come from the owner lane by v_readlane, and every lane computes
// the new coefficient redundantly.  A finished wave exits; nothing waits on it.
//
// Determinism (the host twin ../runtime/enet_cpu.cpp gives the same bits): the two H updates are
// explicit fma, every other operation is separately rounded (fp contract off below), and the
// gap's reductions add each lane's strided entries in ascending order, then wave::sum's xor tree.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "enet_args.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace dml {

constexpr int kEnetLdsBytes = 64 * 1024;          // dynamic LDS of one workgroup
constexpr int kEnetMaxD = kEnetLdsBytes / 16;     // H and w of one problem: 16 bytes per feature
constexpr int kEnetMaxWaves = 4;                  // problems per workgroup where they fit

static inline int enet_waves(int64_t d) {
  const int64_t fit = kEnetLdsBytes / (16 * d);
  return (int)(fit < 1 ? 0 : (fit > kEnetMaxWaves ? kEnetMaxWaves : fit));
}

#define EN_PTR(T, v) reinterpret_cast<T*>(static_cast<uintptr_t>(v))

__device__ __forceinline__ double en_max(double v, int lane) {
  v = fmax(v, wave::shfl_xor<32>(v, lane)); v = fmax(v, wave::shfl_xor<16>(v, lane));
  v = fmax(v, wave::shfl_xor<8>(v, lane));  v = fmax(v, wave::shfl_xor<4>(v, lane));
  v = fmax(v, wave::shfl_xor<2>(v, lane));  v = fmax(v, wave::shfl_xor<1>(v, lane));
  return v;
}

// a wave-uniform index the compiler must keep in a vector register (so the load through it is a
// vector load)
__device__ __forceinline__ int en_vector_index(int i) {
  asm volatile("" : "+v"(i));
  return i;
}

// the Grams are read through global-address-space pointers: a generic (flat) load would count on
// the LDS counter as well, and every LDS wait of a step would then wait for the prefetch too
typedef const double __attribute__((address_space(1))) * en_gptr;

constexpr int kEnetRing = 3;   // register sets of the row prefetch: the row of step ii + 2 is in flight

// NE > 0: d <= 64 * NE, and the rows of the next TWO coordinates are in flight while a step
// computes (a row's address does not depend on the iterate, so its load leaves the step's
// dependency chain).  A sweep runs ceil(d / 3) * 3 steps, the ones past d empty, so that the
// register set of a step is a compile-time constant; the last steps of a sweep load rows 0 and 1
// for the next one.  NE == 0: any d up to kEnetMaxD, the row is read where it is used.
template <int NE>
__global__ __launch_bounds__(64 * kEnetMaxWaves) void k_enet_cd(EnetArgs a) {
  extern __shared__ __attribute__((aligned(16))) double en_lds[];
  const int lane = wave::lane_id();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int waves = (int)(blockDim.x >> 6);
  const int64_t f = (int64_t)blockIdx.x * waves + wv;
  if (f >= a.F) return;
  const int d = (int)a.d;
  double* __restrict__ wout = EN_PTR(double, a.w) + f * d;
  const int g = EN_PTR(const int32_t, a.gram_id)[f];
  if (g < 0 || g >= a.G) {   // never a read outside the Grams: the problem is reported unsolved
    for (int j = lane; j < d; j += 64) wout[j] = 0.0;
    if (lane == 0) {
      EN_PTR(double, a.gap)[f] = __builtin_nan("");
      EN_PTR(double, a.tol_eff)[f] = 0.0;
      EN_PTR(int32_t, a.n_iter)[f] = -1;
    }
    return;
  }
  const en_gptr Q = (en_gptr)(uintptr_t)a.Q + (int64_t)g * d * d;
  const en_gptr q = (en_gptr)(uintptr_t)a.q + (int64_t)g * d;
  const double yn = EN_PTR(const double, a.ynorm2)[g];
  const double l1 = EN_PTR(const double, a.l1)[f], l2 = EN_PTR(const double, a.l2)[f];
  const bool positive = EN_PTR(const int32_t, a.positive)[f] != 0;
  const int max_iter = EN_PTR(const int32_t, a.max_iter)[f];
  const double tol = EN_PTR(const double, a.tol)[f];
  const double tol_eff = tol * yn;
  double* H = en_lds + (size_t)wv * 2 * d;
  double* w = H + d;
  for (int j = lane; j < d; j += 64) {
    H[j] = 0.0;
    w[j] = 0.0;
  }
  double gap = tol + 1.0;
  int n_iter = 0;
  constexpr int NR = NE > 0 ? NE : 1;
  double ring[kEnetRing][NR];            // row entries lane, lane + 64, ... of the steps in flight
  double ring_qd[kEnetRing], ring_qv[kEnetRing];   // their diagonal and q entry
  // row `r` into register set S; the diagonal and q entry as VECTOR loads (every lane the same
  // address): a scalar load would share the LDS counter.  Every load is unconditional, at a
  // clamped address (an entry past d, or the row of an empty step, is loaded and never used):
  // straight-line code lets the compiler count the loads in flight and wait for exactly the
  // ones a step needs.
  auto fetch = [&](auto slot, int r) {
    constexpr int S = decltype(slot)::value;
    const en_gptr row = Q + (int64_t)(r < d ? r : 0) * d;
    if constexpr (NE > 0) {
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        const int j = lane + 64 * k;
        ring[S][k] = row[j < d ? j : d - 1];
      }
    }
    const int vr = en_vector_index(r < d ? r : 0);
    ring_qd[S] = row[vr];
    ring_qv[S] = q[vr];
  };
  const int d3 = (d + kEnetRing - 1) / kEnetRing * kEnetRing;
  fetch(std::integral_constant<int, 0>{}, 0);
  fetch(std::integral_constant<int, 1>{}, 1);
  for (int it = 0; it < max_iter; ++it) {
    n_iter = it + 1;
    double w_max = 0.0, d_w_max = 0.0;
    auto step = [&](auto slot, int ii) {
      constexpr int S = decltype(slot)::value;
      const int nx = ii + 2;   // the step two ahead: its row goes into the set this step's predecessor left
      fetch(std::integral_constant<int, (S + 2) % kEnetRing>{}, nx < d3 ? nx : nx - d3);
      const double qii = ring_qd[S];
      if (ii < d && qii != 0.0) {   // wave-uniform
        const int owner = ii & 63;
        // every lane reads the entry of its own in ii's group of 64 (none past d); the owner's
        // is the step's
        const int mine = (ii & ~63) | lane;
        const double w_ii = wave::bcast(mine < d ? w[mine] : 0.0, owner);
        double hii = wave::bcast(mine < d ? H[mine] : 0.0, owner);
        if (w_ii != 0.0) hii = fma(-w_ii, qii, hii);
        const double tmp = ring_qv[S] - hii;
        double wn;
        if (positive && tmp < 0.0) {
          wn = 0.0;
        } else {
          const double m = fabs(tmp) - l1;
          const double s = tmp > 0.0 ? 1.0 : (tmp < 0.0 ? -1.0 : 0.0);
          wn = (s * (m > 0.0 ? m : 0.0)) / (qii + l2);
        }
        if (lane == owner) w[ii] = wn;
        if (w_ii != 0.0 || wn != 0.0) {   // wave-uniform
          const double na = -w_ii;
          if constexpr (NE > 0) {
#pragma unroll
            for (int k = 0; k < NE; ++k) {
              const int j = lane + 64 * k;
              if (j < d) {
                double h = H[j];
                if (w_ii != 0.0) h = fma(na, ring[S][k], h);
                if (wn != 0.0) h = fma(wn, ring[S][k], h);
                H[j] = h;
              }
            }
          } else {
            const en_gptr row = Q + (int64_t)ii * d;
            for (int j = lane; j < d; j += 64) {
              const double r = row[j];
              double h = H[j];
              if (w_ii != 0.0) h = fma(na, r, h);
              if (wn != 0.0) h = fma(wn, r, h);
              H[j] = h;
            }
          }
        }
        const double d_w_ii = fabs(wn - w_ii);
        if (d_w_ii > d_w_max) d_w_max = d_w_ii;
        if (fabs(wn) > w_max) w_max = fabs(wn);
      }
    };
    for (int base = 0; base < d3; base += kEnetRing) {
      step(std::integral_constant<int, 0>{}, base);
      step(std::integral_constant<int, 1>{}, base + 1);
      step(std::integral_constant<int, 2>{}, base + 2);
    }
    if (w_max == 0.0 || d_w_max / w_max < tol || it == max_iter - 1) {
      double s_qw = 0.0, s_wh = 0.0, s_ww = 0.0, s_l1 = 0.0;
      double dual = positive ? -INFINITY : 0.0;
      for (int j = lane; j < d; j += 64) {
        const double wj = w[j], hj = H[j], qj = q[j];
        s_qw = s_qw + wj * qj;
        s_wh = s_wh + wj * hj;
        s_ww = s_ww + wj * wj;
        s_l1 = s_l1 + fabs(wj);
        double x = (qj - hj) - l2 * wj;
        if (!positive) x = fabs(x);
        if (x > dual) dual = x;
      }
      const double q_dot_w = wave::sum(s_qw, lane);
      dual = en_max(dual, lane);
      const double wH = wave::sum(s_wh, lane);
      const double R = (yn + wH) - 2.0 * q_dot_w;
      const double wn2 = wave::sum(s_ww, lane);
      const double l1n = wave::sum(s_l1, lane);
      double c;
      if (dual > l1) {
        c = l1 / dual;
        const double A = R * (c * c);
        gap = 0.5 * (R + A);
      } else {
        c = 1.0;
        gap = R;
      }
      gap = gap + (((l1 * l1n - c * yn) + c * q_dot_w) + ((0.5 * l2) * (1.0 + c * c)) * wn2);
      if (gap < tol_eff) break;
    }
  }
  for (int j = lane; j < d; j += 64) wout[j] = w[j];
  if (lane == 0) {
    EN_PTR(double, a.gap)[f] = gap;
    EN_PTR(double, a.tol_eff)[f] = tol_eff;
    EN_PTR(int32_t, a.n_iter)[f] = n_iter;
  }
}

}  // namespace dml

using namespace dml;

extern "C" {

int dml_enet_sizeof_args() { return (int)sizeof(EnetArgs); }
// the largest d one launch solves, and the problems one workgroup holds at a given d
int dml_enet_max_d() { return kEnetMaxD; }
int dml_enet_problems_per_block(int64_t d) { return d < 1 ? 0 : enet_waves(d); }

// 0: launched; 1: a HIP error; 2: bad arguments; 3: d > dml_enet_max_d() (nothing was launched:
// the caller solves the batch with dml_cpu_enet_cd).
static int enet_launch(EnetArgs* a, hipStream_t st, bool prefetch);
int dml_enet_cd(EnetArgs* a, hipStream_t st) { return enet_launch(a, st, true); }
// the same solve by k_enet_cd<0> (rows read where they are used) at every d: the baseline of the
// row prefetch in scripts/bench_enet.py; the same bits
int dml_enet_cd_plain(EnetArgs* a, hipStream_t st) { return enet_launch(a, st, false); }

static int enet_launch(EnetArgs* a, hipStream_t st, bool prefetch) {
  if (a->F < 0 || a->d < 1 || a->G < 0) return kEnetBadArgs;
  if (a->d > kEnetMaxD) return kEnetDTooLarge;
  if (a->F == 0) return kEnetOk;
  if (!a->Q || !a->q || !a->ynorm2 || !a->gram_id || !a->l1 || !a->l2 || !a->positive || !a->max_iter || !a->tol ||
      !a->w || !a->gap || !a->tol_eff || !a->n_iter || a->G < 1)
    return kEnetBadArgs;
  const int waves = enet_waves(a->d);
  const int64_t blocks = (a->F + waves - 1) / waves;
  if (blocks > 2147483647LL) return kEnetBadArgs;
  const dim3 grid((unsigned)blocks), block(64 * waves);
  const size_t lds = (size_t)waves * 16 * (size_t)a->d;
  const int64_t ne = prefetch ? (a->d + 63) / 64 : 1000;
  if (ne == 1) k_enet_cd<1><<<grid, block, lds, st>>>(*a);
  else if (ne == 2) k_enet_cd<2><<<grid, block, lds, st>>>(*a);
  else if (ne == 3) k_enet_cd<3><<<grid, block, lds, st>>>(*a);
  else if (ne == 4) k_enet_cd<4><<<grid, block, lds, st>>>(*a);
  else if (ne <= 8) k_enet_cd<8><<<grid, block, lds, st>>>(*a);
  else if (ne <= 16) k_enet_cd<16><<<grid, block, lds, st>>>(*a);
  else k_enet_cd<0><<<grid, block, lds, st>>>(*a);
  return hipGetLastError() == hipSuccess ? kEnetOk : kEnetHipError;
}

}  // extern "C"
