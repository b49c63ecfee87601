// svm_prob.hip — SVC(probability=True): batched Platt scaling and pairwise coupling.
//
// libsvm's probability layer (what sklearn's SVC(probability=True) runs per fit):
//   k_platt_fit    sigmoid_train (Lin, Lin, Weng 2007) -- one 256-thread workgroup per
//                  one-vs-one machine; Newton's method with backtracking on (A, B), the five
//                  sums and the objective reduced over the workgroup in float64.
//   k_pair_proba   multiclass_probability (Wu, Lin, Weng 2004, second method) -- one wave
//                  per held-out row, lane t owns class t (k <= 64); the sequential sweep
//                  broadcasts lane t's step to the wave.
// Host twins: csrc/runtime/svm_prob_cpu.cpp (same recurrences; the coupling in the same
// order, the sigmoid fit with a different summation order).  f64 exp / log1p are software
// routines on gfx950 (tens of VALU instructions each), so every element evaluates exp once
// per pass and derives p, q and the objective term from it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "wave_ops.h"

// the host twins are built with -ffp-contract=off: keep a*b+c as two roundings here too
#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
enum { kConverged = 0, kIterCap = 1, kLineSearchFailed = 2 };

// sums of N values over the workgroup; every thread returns with the same totals
template <int N>
__device__ void block_sum(double (&v)[N], double* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = dml::wave::sum(v[q], lane);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) red[q * NW + wid] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) {
    double r = red[q * NW];
    for (int w = 1; w < NW; ++w) r += red[q * NW + w];
    v[q] = r;
  }
  __syncthreads();
}

__device__ double platt_objective(const double* __restrict__ dec, const double* __restrict__ lab, int64_t L,
                                  double hi, double lo, double A, double B, double* red) {
  double f[1] = {0.0};
  for (int64_t i = threadIdx.x; i < L; i += NT) {
    const double t = lab[i] > 0 ? hi : lo;
    const double z = dec[i] * A + B;
    f[0] += z >= 0 ? t * z + log1p(exp(-z)) : (t - 1.0) * z + log1p(exp(z));
  }
  block_sum(f, red);
  return f[0];
}

__global__ __launch_bounds__(NT) void k_platt_fit(const double* __restrict__ dec_all,
                                                  const double* __restrict__ lab_all,
                                                  const int64_t* __restrict__ off_len, double* __restrict__ AB,
                                                  int64_t* __restrict__ iters_status) {
  __shared__ double red[5 * NW];
  const int64_t mi = blockIdx.x;
  const double* dec = dec_all + off_len[2 * mi];
  const double* lab = lab_all + off_len[2 * mi];
  const int64_t L = off_len[2 * mi + 1];
  double pr[1] = {0.0};
  for (int64_t i = threadIdx.x; i < L; i += NT) pr[0] += lab[i] > 0 ? 1.0 : 0.0;
  block_sum(pr, red);   // a count: exact in any order
  const double prior1 = pr[0], prior0 = (double)L - prior1;
  const double hi = (prior1 + 1.0) / (prior1 + 2.0), lo = 1.0 / (prior0 + 2.0);
  double A = 0.0, B = log((prior0 + 1.0) / (prior1 + 1.0));
  double f = platt_objective(dec, lab, L, hi, lo, A, B, red);
  // every value that steers the loops below comes out of block_sum, identical in all
  // threads: the control flow is uniform and every __syncthreads() is reached by all
  int64_t iter = 0, status = kIterCap;
  for (; iter < 100; ++iter) {
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // h11, h22, h21, g1, g2
    for (int64_t i = threadIdx.x; i < L; i += NT) {
      const double t = lab[i] > 0 ? hi : lo;
      const double dv = dec[i];
      const double z = dv * A + B;
      double p, q;
      if (z >= 0) {
        const double e = exp(-z);
        p = e / (1.0 + e);
        q = 1.0 / (1.0 + e);
      } else {
        const double e = exp(z);
        p = 1.0 / (1.0 + e);
        q = e / (1.0 + e);
      }
      const double d2 = p * q, d1 = t - p;
      s[0] += dv * dv * d2;
      s[1] += d2;
      s[2] += dv * d2;
      s[3] += dv * d1;
      s[4] += d1;
    }
    block_sum(s, red);
    const double h11 = 1e-12 + s[0], h22 = 1e-12 + s[1], h21 = s[2], g1 = s[3], g2 = s[4];
    if (fabs(g1) < 1e-5 && fabs(g2) < 1e-5) {
      status = kConverged;
      break;
    }
    const double det = h11 * h22 - h21 * h21;
    const double dA = -(h22 * g1 - h21 * g2) / det, dB = -(-h21 * g1 + h11 * g2) / det;
    const double gd = g1 * dA + g2 * dB;
    double step = 1.0;
    bool accepted = false;
    while (step >= 1e-10) {
      const double nA = A + step * dA, nB = B + step * dB;
      const double nf = platt_objective(dec, lab, L, hi, lo, nA, nB, red);
      if (nf < f + 1e-4 * step * gd) {
        A = nA;
        B = nB;
        f = nf;
        accepted = true;
        break;
      }
      step /= 2.0;
    }
    if (!accepted) {
      status = kLineSearchFailed;
      break;
    }
  }
  if (threadIdx.x == 0) {
    AB[2 * mi] = A;
    AB[2 * mi + 1] = B;
    iters_status[2 * mi] = iter;
    iters_status[2 * mi + 1] = status;
  }
}

__device__ __forceinline__ double wave_max(double v, int lane) {
  v = fmax(v, dml::wave::shfl_xor<32>(v, lane)); v = fmax(v, dml::wave::shfl_xor<16>(v, lane));
  v = fmax(v, dml::wave::shfl_xor<8>(v, lane)); v = fmax(v, dml::wave::shfl_xor<4>(v, lane));
  v = fmax(v, dml::wave::shfl_xor<2>(v, lane)); v = fmax(v, dml::wave::shfl_xor<1>(v, lane));
  return v;
}

// One wave per row.  r[a][b] of the row lives in the wave's LDS slab, pitch k + 1; Q is
// never stored: Q[t][j] = -r[j][t] r[t][j], and lane t keeps Q[t][t], p[t] and Qp[t].
__global__ void k_pair_proba(const double* __restrict__ dec, const double* __restrict__ AB, int64_t m, int k,
                             int wpb, double* __restrict__ out, int32_t* __restrict__ iters) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int S = k + 1;
  double* R = lds + (size_t)wid * k * S;
  const int64_t row = (int64_t)blockIdx.x * wpb + wid;
  const bool live = row < m;
  if (live) {
    int pi0 = 0;   // index of pair (a, a + 1)
    for (int a = 0; a < k; ++a) {
      const int b = a + 1 + lane;
      if (b < k) {
        const int pi = pi0 + lane;
        const double z = dec[(int64_t)pi * m + row] * AB[2 * pi] + AB[2 * pi + 1];
        double s;
        if (z >= 0) {
          const double e = exp(-z);
          s = e / (1.0 + e);
        } else {
          s = 1.0 / (1.0 + exp(z));
        }
        s = s < 1e-7 ? 1e-7 : (s > 1.0 - 1e-7 ? 1.0 - 1e-7 : s);
        R[a * S + b] = s;
        R[b * S + a] = 1.0 - s;
      }
      pi0 += k - 1 - a;
    }
  }
  __syncthreads();   // the only barrier; what follows is wave-local
  if (!live) return;
  const bool act = lane < k;
  const int t = act ? lane : 0;   // idle lanes shadow lane 0 (their values are never read)
  double Qtt = 0.0;
  for (int j = 0; j < k; ++j)
    if (j != t) {
      const double x = R[j * S + t];
      Qtt += x * x;
    }
  double p = act ? 1.0 / (double)k : 0.0;
  const int max_iter = k > 100 ? k : 100;
  const double eps = 0.005 / (double)k;
  int iter = 0;
  for (; iter < max_iter; ++iter) {
    double Qp = 0.0;
    for (int j = 0; j < k; ++j) {
      const double pj = dml::wave::bcast(p, j);
      const double Qtj = j == t ? Qtt : -R[j * S + t] * R[t * S + j];
      Qp += Qtj * pj;
    }
    const double pq = p * Qp;
    double pQp = 0.0;
    for (int j = 0; j < k; ++j) pQp += dml::wave::bcast(pq, j);
    const double max_error = wave_max(act ? fabs(Qp - pQp) : 0.0, lane);
    if (max_error < eps) break;
    for (int s = 0; s < k; ++s) {
      const double Qps = dml::wave::bcast(Qp, s), Qss = dml::wave::bcast(Qtt, s);
      const double diff = (-Qps + pQp) / Qss;
      if (lane == s) p += diff;
      pQp = (pQp + diff * (diff * Qss + 2.0 * Qps)) / (1.0 + diff) / (1.0 + diff);
      const double Qsj = t == s ? Qtt : -R[t * S + s] * R[s * S + t];
      Qp = (Qp + diff * Qsj) / (1.0 + diff);
      p /= (1.0 + diff);
    }
  }
  if (act) out[row * k + lane] = p;
  if (iters && lane == 0) iters[row] = iter;
}

}  // namespace

extern "C" {

// dec / lab: held-out decision values and labels (+1 / -1) of n machines, concatenated;
// off_len [n][2] = (offset, L).  AB [n][2] = (A, B); iters_status [n][2].
int dml_svm_platt_fit(const double* dec, const double* lab, const int64_t* off_len, int64_t n, double* AB,
                      int64_t* iters_status, void* stream) {
  if (n <= 0) return 0;
  k_platt_fit<<<(unsigned)n, NT, 0, (hipStream_t)stream>>>(dec, lab, off_len, AB, iters_status);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// dec [npairs][m] (pair (a, b), a < b, lexicographic; positive towards a), AB [npairs][2]
// -> out [m][k]; iters [m] (may be null).  k <= 64 only (2: no such kernel).
int dml_svm_pair_proba(const double* dec, const double* AB, int64_t m, int64_t k, double* out, int32_t* iters,
                       void* stream) {
  if (k < 1 || k > 64) return 2;
  if (m <= 0) return 0;
  const size_t slab = (size_t)k * (k + 1) * sizeof(double);   // <= 33280 B
  const int wpb = slab * 4 <= 65536 ? 4 : 1;
  const int64_t blocks = (m + wpb - 1) / wpb;
  k_pair_proba<<<(unsigned)blocks, 64 * wpb, slab * wpb, (hipStream_t)stream>>>(dec, AB, m, (int)k, wpb, out, iters);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // extern "C"
