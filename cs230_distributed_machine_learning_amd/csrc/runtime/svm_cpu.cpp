// svm_cpu.cpp — the batched SMO solver of svm.hip on the host (no-GPU path and oracle).
//
// Same dual algorithm as libsvm's Solver (what sklearn SVC/SVR run per fit, reference
// aws-prod/worker/worker.py:40,47): WSS3 second-order working-set selection, analytic
// two-variable update, gradient maintenance, eps stopping rule, later index wins ties.
// Problems are independent and run in parallel with OpenMP.
//
// Below the solver: the host twins of svm_decision.hip (rho + support-vector compaction,
// decision values, votes) -- the same arithmetic in the same summation order (per-lane strided
// partials, the wave butterfly, the waves in index order), so they are the kernels' oracle
// and the implementation of the batched post-solve phase on a CPU device.
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "svm_args.h"

namespace {

using dml::KLIN;
using dml::KPOLY;
using dml::KRBF;
using dml::KSIG;
using dml::SvmDecArgs;
using dml::SvmProb;
constexpr double kTau = 1e-12;
constexpr double kInf = 1e300;

float kfun(int kernel, double gamma, double coef0, int degree, float acc) {
  switch (kernel) {
    case KRBF: return (float)std::exp(-gamma * (double)acc);
    case KPOLY: {
      const double b = gamma * (double)acc + coef0;
      double r = 1.0;
      for (int i = 0; i < degree; ++i) r *= b;
      return (float)r;
    }
    case KSIG: return (float)std::tanh(gamma * (double)acc + coef0);
    default: return acc;
  }
}

void column(const SvmProb& p, const float* X, int64_t d, int64_t src, float* col) {
  const float* base = X + p.xoff;
  for (int64_t r = 0; r < p.nrows; ++r) {
    float acc = 0.f;
    if (p.kernel == KRBF) {
      for (int64_t f = 0; f < d; ++f) {
        const float t = base[f * p.nrows + src] - base[f * p.nrows + r];
        acc = std::fma(t, t, acc);
      }
    } else {
      for (int64_t f = 0; f < d; ++f) acc = std::fma(base[f * p.nrows + src], base[f * p.nrows + r], acc);
    }
    col[r] = kfun((int)p.kernel, p.gamma, p.coef0, (int)p.degree, acc);
  }
}

void solve(SvmProb& p, const float* X, int64_t d, const float* yv, const double* Cv, const float* qd, double* alpha,
           double* G) {
  const int64_t L = p.L, nr = p.nrows;
  const float* y = yv + p.voff;
  const double* C = Cv + p.voff;
  double* a = alpha + p.voff;
  double* g = G + p.voff;
  const float* QD = qd + p.roff;
  std::vector<float> Ki(nr), Kj(nr);
  auto rowof = [&](int64_t t) { return (p.svr && t >= nr) ? t - nr : t; };
  int64_t it = p.iters;
  int status = 2;
  while (it < p.max_iter) {
    double Gmax = -kInf;
    int64_t i = -1;
    for (int64_t t = 0; t < L; ++t) {
      const bool up = y[t] > 0 ? a[t] < C[t] : a[t] > 0;
      if (up && -y[t] * g[t] >= Gmax) { Gmax = -y[t] * g[t]; i = t; }
    }
    if (i < 0) { status = 1; break; }
    const double yi = y[i];
    const int64_t ri = rowof(i);
    column(p, X, d, ri, Ki.data());
    double Gmax2 = -kInf, odmin = kInf;
    int64_t j = -1;
    const double QDi = QD[ri];
    for (int64_t t = 0; t < L; ++t) {
      const double yt = y[t];
      const int64_t rt = rowof(t);
      const double kit = Ki[rt];
      if (yt > 0) {
        if (a[t] > 0) {
          const double gd = Gmax + g[t];
          if (g[t] >= Gmax2) Gmax2 = g[t];
          if (gd > 0) {
            const double qc = QDi + QD[rt] - 2.0 * yi * (yi * yt * kit);
            const double od = qc > 0 ? -(gd * gd) / qc : -(gd * gd) / kTau;
            if (od <= odmin) { odmin = od; j = t; }
          }
        }
      } else {
        if (a[t] < C[t]) {
          const double gd = Gmax - g[t];
          if (-g[t] >= Gmax2) Gmax2 = -g[t];
          if (gd > 0) {
            const double qc = QDi + QD[rt] + 2.0 * yi * (yi * yt * kit);
            const double od = qc > 0 ? -(gd * gd) / qc : -(gd * gd) / kTau;
            if (od <= odmin) { odmin = od; j = t; }
          }
        }
      }
    }
    if (Gmax + Gmax2 < p.eps || j < 0) { status = 1; break; }
    const double yj = y[j];
    const int64_t rj = rowof(j);
    column(p, X, d, rj, Kj.data());
    const double Ci = C[i], Cj = C[j];
    const double Qij = yi * yj * (double)Ki[rj];
    const double QDj = QD[rj];
    const double oai = a[i], oaj = a[j];
    double ai = oai, aj = oaj;
    if (yi != yj) {
      double qc = QDi + QDj + 2.0 * Qij;
      if (qc <= 0) qc = kTau;
      const double delta = (-g[i] - g[j]) / qc;
      const double diff = ai - aj;
      ai += delta; aj += delta;
      if (diff > 0) { if (aj < 0) { aj = 0; ai = diff; } }
      else { if (ai < 0) { ai = 0; aj = -diff; } }
      if (diff > Ci - Cj) { if (ai > Ci) { ai = Ci; aj = Ci - diff; } }
      else { if (aj > Cj) { aj = Cj; ai = Cj + diff; } }
    } else {
      double qc = QDi + QDj - 2.0 * Qij;
      if (qc <= 0) qc = kTau;
      const double delta = (g[i] - g[j]) / qc;
      const double sum = ai + aj;
      ai -= delta; aj += delta;
      if (sum > Ci) { if (ai > Ci) { ai = Ci; aj = sum - Ci; } }
      else { if (aj < 0) { aj = 0; ai = sum; } }
      if (sum > Cj) { if (aj > Cj) { aj = Cj; ai = sum - Cj; } }
      else { if (ai < 0) { ai = 0; aj = sum; } }
    }
    a[i] = ai; a[j] = aj;
    const double dai = ai - oai, daj = aj - oaj;
    for (int64_t t = 0; t < L; ++t) {
      const int64_t rt = rowof(t);
      g[t] += y[t] * (yi * (double)Ki[rt] * dai + yj * (double)Kj[rt] * daj);
    }
    ++it;
  }
  p.iters = it;
  p.status = status;
}

// ---- twins of svm_decision.hip ---------------------------------------------------------------
constexpr int NT = dml::kSvmDecNT, QT = dml::kSvmDecQT, NW = NT / 64;

// dml::wave::sum over one wave's 64 lane values: v += v[lane ^ 32], ^ 16, ... ^ 1 (lane 0's result)
double butterfly_sum(double* v) {
  for (int m = 32; m >= 1; m >>= 1) {
    double nv[64];
    for (int l = 0; l < 64; ++l) nv[l] = v[l] + v[l ^ m];
    std::copy(nv, nv + 64, v);
  }
  return v[0];
}

// the workgroup's reduction of its 256 per-lane partials: butterfly per wave, waves in index order
double block_sum(double* lanes) {
  double r = butterfly_sum(lanes);
  for (int w = 1; w < NW; ++w) r += butterfly_sum(lanes + 64 * w);
  return r;
}

void rho_sv(const SvmProb& p, const SvmDecArgs& a, int64_t k) {
  const float* y = (const float*)a.y + p.voff;
  const double* C = (const double*)a.C + p.voff;
  const double* al = (const double*)a.alpha + p.voff;
  const double* g = (const double*)a.G + p.voff;
  const double inf = std::numeric_limits<double>::infinity();
  double fsum[NT], ub = inf, lb = -inf;
  int64_t nfree = 0;
  for (int t0 = 0; t0 < NT; ++t0) {
    fsum[t0] = 0.0;
    for (int64_t t = t0; t < p.L; t += NT) {
      const double yt = (double)y[t], yg = yt * g[t];
      const bool upper = al[t] >= C[t], lower = al[t] <= 0.0;
      if (!upper && !lower) {
        fsum[t0] += yg;
        ++nfree;
      } else {
        if ((upper && yt < 0) || (lower && yt > 0)) ub = std::fmin(ub, yg);   // fmin / fmax as the kernel: a NaN is ignored
        if ((upper && yt > 0) || (lower && yt < 0)) lb = std::fmax(lb, yg);
      }
    }
  }
  const double fs = block_sum(fsum);
  ((double*)a.rho)[k] = nfree > 0 ? fs / (double)nfree : (ub + lb) / 2;
  int32_t* idx = (int32_t*)a.sv_idx + p.roff;
  double* cf = (double*)a.sv_coef + p.roff;
  int32_t n = 0;
  for (int64_t r = 0; r < p.nrows; ++r) {
    const double c = p.svr ? al[r] - al[p.nrows + r] : al[r] * (double)y[r];
    if (c != 0.0) { idx[n] = (int32_t)r; cf[n] = c; ++n; }
  }
  ((int32_t*)a.nsv)[k] = n;
}

double kfun64(int kernel, double gamma, double coef0, int degree, double acc) {
  switch (kernel) {
    case KRBF: return std::exp(-gamma * acc);
    case KPOLY: {
      const double b = gamma * acc + coef0;
      double r = 1.0;
      for (int i = 0; i < degree; ++i) r *= b;
      return r;
    }
    case KSIG: return std::tanh(gamma * acc + coef0);
    default: return acc;
  }
}

// one (problem, query tile) workgroup of k_svm_decision
void decision_tile(const SvmDecArgs& a, int64_t w) {
  const int32_t* work = (const int32_t*)a.work;
  const int64_t k = work[2 * w], tile = work[2 * w + 1];
  const SvmProb& p = ((const SvmProb*)a.probs)[k];
  const int64_t* qinfo = (const int64_t*)a.qinfo;
  const int64_t qoff = qinfo[2 * k], qn = qinfo[2 * k + 1], q0 = tile * QT, d = a.d;
  if (q0 >= qn) return;
  const int nq = (int)std::min<int64_t>(QT, qn - q0);
  const int64_t* qr = (const int64_t*)a.qrows + qoff + q0;
  const int64_t* op = (const int64_t*)a.opos + qoff + q0;
  const int32_t nsv = ((const int32_t*)a.nsv)[k];
  const int32_t* idx = (const int32_t*)a.sv_idx + p.roff;
  const double* cf = (const double*)a.sv_coef + p.roff;
  const float* base = (const float*)a.Xrs + p.xoff;
  const float* X = (const float*)a.X;
  const double rho = ((const double*)a.rho)[k];
  for (int q = 0; q < nq; ++q) {
    const float* xq = X + qr[q] * d;
    double lanes[NT];
    for (int t = 0; t < NT; ++t) {
      double sum = 0.0;
      for (int64_t j = t; j < nsv; j += NT) {
        const float* col = base + idx[j];
        double acc = 0.0;
        if (p.kernel == KRBF) {
          for (int64_t f = 0; f < d; ++f) {
            const double df = (double)xq[f] - (double)col[f * p.nrows];
            acc = std::fma(df, df, acc);
          }
        } else {
          for (int64_t f = 0; f < d; ++f) acc = std::fma((double)xq[f], (double)col[f * p.nrows], acc);
        }
        sum = std::fma(cf[j], kfun64((int)p.kernel, p.gamma, p.coef0, (int)p.degree, acc), sum);
      }
      lanes[t] = sum;
    }
    ((double*)a.out)[op[q]] = block_sum(lanes) - rho;
  }
}

}  // namespace

extern "C" {

int dml_cpu_svm_dec_sizeof_args() { return (int)sizeof(SvmDecArgs); }

int dml_cpu_svm_rho_sv(const SvmDecArgs* a) {
  const SvmProb* P = (const SvmProb*)a->probs;
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t k = 0; k < a->nprob; ++k) rho_sv(P[k], *a, k);
  return dml::kSvmDecOk;
}

int dml_cpu_svm_decision(const SvmDecArgs* a) {
  if (a->nwork > 0 && a->d < 1) return dml::kSvmDecBadArgs;
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t w = 0; w < a->nwork; ++w) decision_tile(*a, w);
  return dml::kSvmDecOk;
}

int dml_cpu_svm_vote(const SvmDecArgs* a) {
  if (a->F * a->max_m <= 0) return dml::kSvmDecOk;
  if (a->n_classes < 2) return dml::kSvmDecBadArgs;
  const int nc = (int)a->n_classes;
  const double* dec = (const double*)a->out;
  const int64_t* tab = (const int64_t*)a->fit_tab;
  for (int64_t fit = 0; fit < a->F; ++fit) {
    const int64_t* po = (const int64_t*)a->pair_off + fit * ((int64_t)nc * (nc - 1) / 2);
    int32_t* pred = (int32_t*)a->pred + tab[2 * fit + 1];
    for (int64_t row = 0; row < tab[2 * fit]; ++row) {
      int best = 0, best_votes = -1;
      for (int c = 0; c < nc; ++c) {
        int votes = 0;
        for (int b = c + 1; b < nc; ++b) {
          const int64_t o = po[c * nc - c * (c + 1) / 2 + (b - c - 1)];
          if (o >= 0 && dec[o + row] > 0) ++votes;
        }
        for (int a_ = 0; a_ < c; ++a_) {
          const int64_t o = po[a_ * nc - a_ * (a_ + 1) / 2 + (c - a_ - 1)];
          if (o >= 0 && !(dec[o + row] > 0)) ++votes;
        }
        if (votes > best_votes) { best_votes = votes; best = c; }
      }
      pred[row] = best;
    }
  }
  return dml::kSvmDecOk;
}

int dml_cpu_svm_sizeof_prob() { return (int)sizeof(SvmProb); }

void dml_cpu_svm_smo(const float* X, int64_t d, void* probs, int64_t nprob, const float* y, const double* C,
                     const float* qd, double* alpha, double* G) {
  SvmProb* P = (SvmProb*)probs;
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t k = 0; k < nprob; ++k)
    if (P[k].status == 0) solve(P[k], X, d, y, C, qd, alpha, G);
}

}  // extern "C"
