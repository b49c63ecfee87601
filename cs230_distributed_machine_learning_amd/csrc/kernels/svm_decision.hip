// svm_decision.hip — the post-solve phase of every SVC / SVR dual problem of a job in three
// launches: rho + support-vector compaction, decision values of the held-out rows, votes.
//
// Reference: libsvm's Solver::calculate_rho, svm_predict_values and the one-vs-one vote of
// svm_predict (what sklearn SVC / SVR run per fit; aws-prod/worker/worker.py:40,47).
//
// k_svm_rho       one workgroup per problem.  rho in double, its free-variable sum reduced in a
//                 fixed order (per-thread strided partials, wave butterfly, waves in index
//                 order); the rows with coef != 0 compacted in ascending order by a block prefix
//                 scan (no atomics) into sv_idx / sv_coef at the problem's roff.
// k_svm_decision  one workgroup per (problem, tile of kSvmDecQT query rows) of a host-built
//                 work list.  Lanes own support vectors (lane t: compacted SVs t, t + 256, ...);
//                 the tile's query rows sit in LDS as doubles, feature-chunked (kSvmDecFC), so
//                 any d is served with 16 KiB of LDS.  Per feature a lane loads its SV's value
//                 once (feature-major rowset block, through the compacted index) and runs it
//                 against the QT broadcast queries: QT float64 accumulators, sum (q - s)^2 for
//                 RBF (the direct difference form: no cancellation), sum q s otherwise.  The
//                 kernel function is applied in double and coef * k joins QT float64 running
//                 sums; at the end a wave butterfly, the waves in index order, and
//                 out[opos] = sum - rho.  FP64 vector arithmetic throughout: the matrix cores'
//                 FP64 peak is the vector peak on this part and they would force the
//                 |a|^2 + |b|^2 - 2ab form.
// k_svm_vote      one thread per (fit, test row): libsvm's vote over the fit's pairs (dv > 0
//                 votes for the pair's first class), first maximum.
//
// The host twins (../runtime/svm_cpu.cpp) do the same arithmetic in the same order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "svm_args.h"
#include "wave_ops.h"

namespace {

using dml::SvmDecArgs;
using dml::SvmProb;
constexpr int NT = dml::kSvmDecNT;
constexpr int QT = dml::kSvmDecQT;
constexpr int FC = dml::kSvmDecFC;
constexpr int NW = NT / 64;

// every lane of the wave ends with the same sum; the twin repeats the pairing
__device__ __forceinline__ double wave_sum(double v, int lane) { return dml::wave::sum(v, lane); }

__device__ __forceinline__ double wave_min(double v, int lane) {
  v = fmin(v, dml::wave::shfl_xor<32>(v, lane)); v = fmin(v, dml::wave::shfl_xor<16>(v, lane));
  v = fmin(v, dml::wave::shfl_xor<8>(v, lane)); v = fmin(v, dml::wave::shfl_xor<4>(v, lane));
  v = fmin(v, dml::wave::shfl_xor<2>(v, lane)); v = fmin(v, dml::wave::shfl_xor<1>(v, lane));
  return v;
}

__global__ __launch_bounds__(NT) void k_svm_rho(const SvmProb* __restrict__ probs, const float* __restrict__ yv,
                                                const double* __restrict__ Cv, const double* __restrict__ alpha,
                                                const double* __restrict__ Gv, int32_t* __restrict__ sv_idx,
                                                double* __restrict__ sv_coef, double* __restrict__ rho_out,
                                                int32_t* __restrict__ nsv_out) {
  __shared__ double s_sum[NW], s_ub[NW], s_lb[NW];
  __shared__ int s_free[NW], s_cnt[NW];
  const SvmProb p = probs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* y = yv + p.voff;
  const double* C = Cv + p.voff;
  const double* a = alpha + p.voff;
  const double* g = Gv + p.voff;
  // ---- rho (libsvm calculate_rho) ----
  double fsum = 0.0, ub = INFINITY, nlb = INFINITY;   // nlb = -lb: one min reduction serves both
  int nfree = 0;
  for (int64_t t = tid; t < p.L; t += NT) {
    const double yt = (double)y[t], yg = yt * g[t];
    const bool upper = a[t] >= C[t], lower = a[t] <= 0.0;
    if (!upper && !lower) {
      fsum += yg;
      ++nfree;
    } else {
      if ((upper && yt < 0) || (lower && yt > 0)) ub = fmin(ub, yg);
      if ((upper && yt > 0) || (lower && yt < 0)) nlb = fmin(nlb, -yg);
    }
  }
  fsum = wave_sum(fsum, lane);
  ub = wave_min(ub, lane);
  nlb = wave_min(nlb, lane);
  nfree = dml::wave::sum(nfree, lane);
  if (lane == 0) { s_sum[wid] = fsum; s_ub[wid] = ub; s_lb[wid] = nlb; s_free[wid] = nfree; }
  __syncthreads();
  if (tid == 0) {
    double fs = s_sum[0], u = s_ub[0], nl = s_lb[0];
    int nf = s_free[0];
    for (int w = 1; w < NW; ++w) { fs += s_sum[w]; u = fmin(u, s_ub[w]); nl = fmin(nl, s_lb[w]); nf += s_free[w]; }
    rho_out[blockIdx.x] = nf > 0 ? fs / (double)nf : (u + -nl) / 2;
  }
  // ---- support vectors: ascending positions with coef != 0 ----
  int32_t* idx = sv_idx + p.roff;
  double* cf = sv_coef + p.roff;
  int base = 0;   // support vectors found in the earlier passes
  for (int64_t r0 = 0; r0 < p.nrows; r0 += NT) {
    const int64_t r = r0 + tid;
    double c = 0.0;
    if (r < p.nrows) c = p.svr ? a[r] - a[p.nrows + r] : a[r] * (double)y[r];
    const int flag = c != 0.0;
    const int incl = dml::wave::incl_scan(flag);
    if (lane == 63) s_cnt[wid] = incl;
    __syncthreads();
    int before = base;
    for (int w = 0; w < wid; ++w) before += s_cnt[w];
    if (flag) {
      idx[before + incl - 1] = (int32_t)r;
      cf[before + incl - 1] = c;
    }
    for (int w = 0; w < NW; ++w) base += s_cnt[w];
    __syncthreads();
  }
  if (tid == 0) nsv_out[blockIdx.x] = base;
}

// stage features [f0, f0 + fc) of the tile's query rows as doubles: xs[f * QT + q]
__device__ __forceinline__ void stage_queries(double* xs, const float* __restrict__ X, int64_t d,
                                              const int64_t* __restrict__ qr, int nq, int64_t f0, int fc) {
  for (int i = threadIdx.x; i < QT * fc; i += NT) {
    const int q = i / fc, f = i - q * fc;   // consecutive threads read consecutive features of a row
    xs[f * QT + q] = q < nq ? (double)X[qr[q] * d + f0 + f] : 0.0;
  }
}

__device__ __forceinline__ double kfun64(int kernel, double gamma, double coef0, int degree, double acc) {
  switch (kernel) {
    case dml::KRBF: return exp(-gamma * acc);
    case dml::KPOLY: {
      const double b = gamma * acc + coef0;
      double r = 1.0;
      for (int i = 0; i < degree; ++i) r *= b;
      return r;
    }
    case dml::KSIG: return tanh(gamma * acc + coef0);
    default: return acc;
  }
}

// one support vector's features [f0, f0 + fc) against the staged queries
template <bool RBF>
__device__ __forceinline__ void accumulate(double (&acc)[QT], const double* xs, const float* __restrict__ col,
                                           int64_t nrows, int fc) {
#pragma unroll 4
  for (int f = 0; f < fc; ++f) {
    const double s = (double)col[(int64_t)f * nrows];
    const double* xq = xs + f * QT;
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      if (RBF) {
        const double t = xq[q] - s;
        acc[q] = __builtin_fma(t, t, acc[q]);
      } else {
        acc[q] = __builtin_fma(xq[q], s, acc[q]);
      }
    }
  }
}

__global__ __launch_bounds__(NT) void k_svm_decision(const float* __restrict__ Xrs, const float* __restrict__ X,
                                                     int64_t d, const SvmProb* __restrict__ probs,
                                                     const int32_t* __restrict__ work,
                                                     const int64_t* __restrict__ qinfo,
                                                     const int64_t* __restrict__ qrows,
                                                     const int64_t* __restrict__ opos,
                                                     const int32_t* __restrict__ sv_idx,
                                                     const double* __restrict__ sv_coef,
                                                     const double* __restrict__ rho, const int32_t* __restrict__ nsv_all,
                                                     double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double xs[FC * QT];
  __shared__ double red[NW][QT];
  const int k = work[2 * blockIdx.x], tile = work[2 * blockIdx.x + 1];
  const SvmProb p = probs[k];
  const int64_t qoff = qinfo[2 * k], qn = qinfo[2 * k + 1];
  const int64_t q0 = (int64_t)tile * QT;
  if (q0 >= qn) return;
  const int nq = (int)(qn - q0 < QT ? qn - q0 : QT);
  const int64_t* qr = qrows + qoff + q0;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nsv = nsv_all[k];
  const int32_t* idx = sv_idx + p.roff;
  const double* cf = sv_coef + p.roff;
  const float* base = Xrs + p.xoff;
  const int nchunk = (int)((d + FC - 1) / FC);
  const int kernel = (int)p.kernel, degree = (int)p.degree;
  double sum[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) sum[q] = 0.0;
  for (int j0 = 0; j0 < nsv; j0 += NT) {
    const int j = j0 + tid;
    const bool active = j < nsv;
    const int64_t r = active ? idx[j] : 0;
    double acc[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) acc[q] = 0.0;
    for (int c = 0; c < nchunk; ++c) {
      const int64_t f0 = (int64_t)c * FC;
      const int fc = (int)(d - f0 < FC ? d - f0 : FC);
      if (nchunk > 1 || j0 == 0) {   // one chunk: the tile stays staged for every pass
        __syncthreads();
        stage_queries(xs, X, d, qr, nq, f0, fc);
        __syncthreads();
      }
      if (active) {
        const float* col = base + f0 * p.nrows + r;
        if (kernel == dml::KRBF) accumulate<true>(acc, xs, col, p.nrows, fc);
        else accumulate<false>(acc, xs, col, p.nrows, fc);
      }
    }
    if (active) {
      const double cj = cf[j];
#pragma unroll
      for (int q = 0; q < QT; ++q)
        sum[q] = __builtin_fma(cj, kfun64(kernel, p.gamma, p.coef0, degree, acc[q]), sum[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < QT; ++q) {
    const double v = dml::wave::sum(sum[q], lane);
    if (lane == 0) red[wid][q] = v;
  }
  __syncthreads();
  if (tid < nq) {
    double v = red[0][tid];
    for (int w = 1; w < NW; ++w) v += red[w][tid];
    out[opos[qoff + q0 + tid]] = v - rho[k];
  }
}

__global__ __launch_bounds__(NT) void k_svm_vote(const double* __restrict__ dec, const int64_t* __restrict__ fit_tab,
                                                 const int64_t* __restrict__ pair_off, int64_t F, int nc,
                                                 int64_t max_m, int32_t* __restrict__ pred) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= F * max_m) return;
  const int64_t fit = i / max_m, row = i - fit * max_m;
  if (row >= fit_tab[2 * fit]) return;
  const int64_t* po = pair_off + fit * ((int64_t)nc * (nc - 1) / 2);
  int best = 0, best_votes = -1;
  for (int c = 0; c < nc; ++c) {
    int votes = 0;
    // pair (a, b), a < b, is entry a nc - a (a + 1) / 2 + (b - a - 1) of the fit's table
    for (int b = c + 1; b < nc; ++b) {
      const int64_t o = po[c * nc - c * (c + 1) / 2 + (b - c - 1)];
      if (o >= 0 && dec[o + row] > 0) ++votes;
    }
    for (int a = 0; a < c; ++a) {
      const int64_t o = po[a * nc - a * (a + 1) / 2 + (c - a - 1)];
      if (o >= 0 && !(dec[o + row] > 0)) ++votes;
    }
    if (votes > best_votes) { best_votes = votes; best = c; }
  }
  pred[fit_tab[2 * fit + 1] + row] = best;
}

}  // namespace

extern "C" {

int dml_svm_dec_sizeof_args() { return (int)sizeof(SvmDecArgs); }
int dml_svm_dec_query_tile() { return QT; }

// rho, nsv, sv_idx, sv_coef of every problem (nothing is read back)
int dml_svm_rho_sv(const SvmDecArgs* a, hipStream_t st) {
  if (a->nprob <= 0) return dml::kSvmDecOk;
  k_svm_rho<<<(unsigned)a->nprob, NT, 0, st>>>((const SvmProb*)a->probs, (const float*)a->y, (const double*)a->C,
                                               (const double*)a->alpha, (const double*)a->G, (int32_t*)a->sv_idx,
                                               (double*)a->sv_coef, (double*)a->rho, (int32_t*)a->nsv);
  return hipGetLastError() == hipSuccess ? dml::kSvmDecOk : dml::kSvmDecHipError;
}

// out[opos[.]] = decision value of every query of every problem on the work list
int dml_svm_decision(const SvmDecArgs* a, hipStream_t st) {
  if (a->nwork <= 0) return dml::kSvmDecOk;
  if (a->d < 1 || a->nwork > 0x7fffffff) return dml::kSvmDecBadArgs;
  k_svm_decision<<<(unsigned)a->nwork, NT, 0, st>>>(
      (const float*)a->Xrs, (const float*)a->X, a->d, (const SvmProb*)a->probs, (const int32_t*)a->work,
      (const int64_t*)a->qinfo, (const int64_t*)a->qrows, (const int64_t*)a->opos, (const int32_t*)a->sv_idx,
      (const double*)a->sv_coef, (const double*)a->rho, (const int32_t*)a->nsv, (double*)a->out);
  return hipGetLastError() == hipSuccess ? dml::kSvmDecOk : dml::kSvmDecHipError;
}

int dml_svm_vote(const SvmDecArgs* a, hipStream_t st) {
  const int64_t n = a->F * a->max_m;
  if (n <= 0) return dml::kSvmDecOk;
  if (a->n_classes < 2) return dml::kSvmDecBadArgs;
  k_svm_vote<<<(unsigned)((n + NT - 1) / NT), NT, 0, st>>>((const double*)a->out, (const int64_t*)a->fit_tab,
                                                           (const int64_t*)a->pair_off, a->F, (int)a->n_classes,
                                                           a->max_m, (int32_t*)a->pred);
  return hipGetLastError() == hipSuccess ? dml::kSvmDecOk : dml::kSvmDecHipError;
}

}  // extern "C"
