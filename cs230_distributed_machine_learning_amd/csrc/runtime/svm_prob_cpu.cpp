// svm_prob_cpu.cpp — SVC(probability=True) on the host: the twins of svm_prob.hip.
//
// libsvm's probability layer as scikit-learn ships it: sigmoid_train (Lin, Lin, Weng 2007:
// Newton's method with backtracking on the regularised Platt objective) per one-vs-one
// machine, and multiclass_probability (Wu, Lin, Weng 2004, second method) per row.  All
// float64, every sum in index order, so the results are libsvm's up to the last place of
// exp / log1p.  Machines / rows are independent and run in parallel with OpenMP.
#include <stdint.h>

#include <cmath>
#include <vector>

namespace {

enum { kConverged = 0, kIterCap = 1, kLineSearchFailed = 2 };

double platt_objective(const double* dec, const double* lab, int64_t L, double hi, double lo, double A, double B) {
  double f = 0.0;
  for (int64_t i = 0; i < L; ++i) {
    const double t = lab[i] > 0 ? hi : lo;
    const double z = dec[i] * A + B;
    f += z >= 0 ? t * z + std::log1p(std::exp(-z)) : (t - 1.0) * z + std::log1p(std::exp(z));
  }
  return f;
}

void platt_fit_one(const double* dec, const double* lab, int64_t L, double* AB, int64_t* st) {
  double prior1 = 0.0;
  for (int64_t i = 0; i < L; ++i) prior1 += lab[i] > 0 ? 1.0 : 0.0;
  const double prior0 = (double)L - prior1;
  const double hi = (prior1 + 1.0) / (prior1 + 2.0), lo = 1.0 / (prior0 + 2.0);
  double A = 0.0, B = std::log((prior0 + 1.0) / (prior1 + 1.0));
  double f = platt_objective(dec, lab, L, hi, lo, A, B);
  int64_t iter = 0, status = kIterCap;
  for (; iter < 100; ++iter) {
    double h11 = 1e-12, h22 = 1e-12, h21 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int64_t i = 0; i < L; ++i) {
      const double t = lab[i] > 0 ? hi : lo;
      const double z = dec[i] * A + B;
      double p, q;
      if (z >= 0) {
        const double e = std::exp(-z);
        p = e / (1.0 + e);
        q = 1.0 / (1.0 + e);
      } else {
        const double e = std::exp(z);
        p = 1.0 / (1.0 + e);
        q = e / (1.0 + e);
      }
      const double d2 = p * q, d1 = t - p;
      h11 += dec[i] * dec[i] * d2;
      h22 += d2;
      h21 += dec[i] * d2;
      g1 += dec[i] * d1;
      g2 += d1;
    }
    if (std::fabs(g1) < 1e-5 && std::fabs(g2) < 1e-5) {
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
      const double nf = platt_objective(dec, lab, L, hi, lo, nA, nB);
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
  AB[0] = A;
  AB[1] = B;
  st[0] = iter;
  st[1] = status;
}

// r[a][b] of one row, k x k row-major (the diagonal is not used)
void pair_matrix(const double* dec, const double* AB, int64_t m, int64_t k, int64_t row, double* r) {
  int64_t pi = 0;
  for (int64_t a = 0; a < k; ++a)
    for (int64_t b = a + 1; b < k; ++b, ++pi) {
      const double z = dec[pi * m + row] * AB[2 * pi] + AB[2 * pi + 1];
      double s;
      if (z >= 0) {
        const double e = std::exp(-z);
        s = e / (1.0 + e);
      } else {
        s = 1.0 / (1.0 + std::exp(z));
      }
      s = s < 1e-7 ? 1e-7 : (s > 1.0 - 1e-7 ? 1.0 - 1e-7 : s);
      r[a * k + b] = s;
      r[b * k + a] = 1.0 - s;
    }
}

int coupling(const double* r, int64_t k, double* p, double* Q, double* Qp) {
  const int max_iter = k > 100 ? (int)k : 100;
  const double eps = 0.005 / (double)k;
  for (int64_t t = 0; t < k; ++t) {
    p[t] = 1.0 / (double)k;
    double qtt = 0.0;
    for (int64_t j = 0; j < k; ++j) {
      if (j == t) continue;
      qtt += r[j * k + t] * r[j * k + t];
      Q[t * k + j] = -r[j * k + t] * r[t * k + j];
    }
    Q[t * k + t] = qtt;
  }
  int iter = 0;
  for (; iter < max_iter; ++iter) {
    double pQp = 0.0;
    for (int64_t t = 0; t < k; ++t) {
      double s = 0.0;
      for (int64_t j = 0; j < k; ++j) s += Q[t * k + j] * p[j];
      Qp[t] = s;
      pQp += p[t] * s;
    }
    double max_error = 0.0;
    for (int64_t t = 0; t < k; ++t) max_error = std::fmax(max_error, std::fabs(Qp[t] - pQp));
    if (max_error < eps) break;
    for (int64_t t = 0; t < k; ++t) {
      const double qtt = Q[t * k + t];
      const double diff = (-Qp[t] + pQp) / qtt;
      p[t] += diff;
      pQp = (pQp + diff * (diff * qtt + 2.0 * Qp[t])) / (1.0 + diff) / (1.0 + diff);
      for (int64_t j = 0; j < k; ++j) {
        Qp[j] = (Qp[j] + diff * Q[t * k + j]) / (1.0 + diff);
        p[j] /= (1.0 + diff);
      }
    }
  }
  return iter;
}

}  // namespace

extern "C" {

// dec / lab: the machines' held-out decision values and labels (+1 / -1), concatenated;
// off_len [n][2] = (offset, L) per machine.  AB [n][2] = (A, B); iters_status [n][2].
int dml_cpu_svm_platt_fit(const double* dec, const double* lab, const int64_t* off_len, int64_t n, double* AB,
                          int64_t* iters_status) {
#pragma omp parallel for schedule(dynamic)
  for (int64_t i = 0; i < n; ++i)
    platt_fit_one(dec + off_len[2 * i], lab + off_len[2 * i], off_len[2 * i + 1], AB + 2 * i, iters_status + 2 * i);
  return 0;
}

// dec [npairs][m] (pair (a, b), a < b, in lexicographic order; positive towards a), AB
// [npairs][2] -> out [m][k]; iters [m] (may be null): coupling iterations per row.
int dml_cpu_svm_pair_proba(const double* dec, const double* AB, int64_t m, int64_t k, double* out, int32_t* iters) {
  if (k < 1) return 1;
#pragma omp parallel
  {
    std::vector<double> r((size_t)(k * k)), Q((size_t)(k * k)), Qp((size_t)k);
#pragma omp for schedule(static)
    for (int64_t row = 0; row < m; ++row) {
      pair_matrix(dec, AB, m, k, row, r.data());
      const int it = coupling(r.data(), k, out + row * k, Q.data(), Qp.data());
      if (iters) iters[row] = it;
    }
  }
  return 0;
}

}  // extern "C"
