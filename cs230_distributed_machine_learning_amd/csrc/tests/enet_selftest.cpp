// enet_selftest.cpp -- ../runtime/enet_cpu.cpp under AddressSanitizer / UBSan (build.py
// build_enet_selftest; tests/test_enet_selftest.py runs it as a plain executable).
// Every result is checked against a straight scalar coordinate descent written here (plain
// loops, sequential sums): d = 1, d = 65, an all-zero Gram, max_iter = 1, positive, F = 0,
// problems of two Grams interleaved.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "enet_args.h"

extern "C" {
int dml_cpu_enet_sizeof_args();
int dml_cpu_enet_cd(const dml::EnetArgs* a);
}

namespace {

int failures = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

uint32_t rng_state = 2463534242u;
double rnd() {   // uniform in (-1, 1)
  rng_state = rng_state * 1664525u + 1013904223u;
  return (double)(rng_state >> 8) / 8388608.0 - 1.0;
}

struct Problem {
  int g;
  double l1, l2;
  int positive, max_iter;
  double tol;
};

// straight scalar loop: sklearn's algorithm with plain sequential sums
void scalar_cd(int d, const double* Q, const double* q, double yn, const Problem& p, std::vector<double>& w,
               double* gap_out, int* n_iter_out) {
  std::vector<double> H(d, 0.0);
  w.assign(d, 0.0);
  double gap = p.tol + 1.0;
  const double tol_eff = p.tol * yn;
  int n_iter = 0;
  for (int it = 0; it < p.max_iter; ++it) {
    n_iter = it + 1;
    double w_max = 0.0, d_w_max = 0.0;
    for (int ii = 0; ii < d; ++ii) {
      const double qii = Q[ii * d + ii];
      if (qii == 0.0) continue;
      const double w_ii = w[ii];
      if (w_ii != 0.0)
        for (int j = 0; j < d; ++j) H[j] -= w_ii * Q[ii * d + j];
      const double tmp = q[ii] - H[ii];
      if (p.positive && tmp < 0.0) {
        w[ii] = 0.0;
      } else {
        const double s = tmp > 0.0 ? 1.0 : (tmp < 0.0 ? -1.0 : 0.0);
        w[ii] = s * fmax(fabs(tmp) - p.l1, 0.0) / (qii + p.l2);
      }
      if (w[ii] != 0.0)
        for (int j = 0; j < d; ++j) H[j] += w[ii] * Q[ii * d + j];
      d_w_max = fmax(d_w_max, fabs(w[ii] - w_ii));
      w_max = fmax(w_max, fabs(w[ii]));
    }
    if (w_max == 0.0 || d_w_max / w_max < p.tol || it == p.max_iter - 1) {
      double qw = 0.0, wH = 0.0, ww = 0.0, l1n = 0.0, dual = p.positive ? -INFINITY : 0.0;
      for (int j = 0; j < d; ++j) {
        qw += w[j] * q[j];
        wH += w[j] * H[j];
        ww += w[j] * w[j];
        l1n += fabs(w[j]);
        const double x = q[j] - H[j] - p.l2 * w[j];
        dual = fmax(dual, p.positive ? x : fabs(x));
      }
      const double R = yn + wH - 2.0 * qw;
      double c = 1.0;
      if (dual > p.l1) {
        c = p.l1 / dual;
        gap = 0.5 * (R + R * c * c);
      } else {
        gap = R;
      }
      gap += p.l1 * l1n - c * yn + c * qw + 0.5 * p.l2 * (1.0 + c * c) * ww;
      if (gap < tol_eff) break;
    }
  }
  *gap_out = gap;
  *n_iter_out = n_iter;
}

// a Gram of n random rows (column `zero_col` constant 0 when >= 0)
void make_gram(int n, int d, int zero_col, std::vector<double>& Q, std::vector<double>& q, double* yn) {
  std::vector<double> X((size_t)n * d), y(n);
  for (auto& v : X) v = rnd();
  for (int i = 0; i < n; ++i) {
    if (zero_col >= 0) X[(size_t)i * d + zero_col] = 0.0;
    y[i] = 2.0 * X[(size_t)i * d] - (d > 2 ? 1.5 * X[(size_t)i * d + 2] : 0.0) + 0.1 * rnd();
  }
  Q.assign((size_t)d * d, 0.0);
  q.assign(d, 0.0);
  *yn = 0.0;
  for (int i = 0; i < n; ++i) {
    *yn += y[i] * y[i];
    for (int a = 0; a < d; ++a) {
      q[a] += X[(size_t)i * d + a] * y[i];
      for (int b = 0; b < d; ++b) Q[(size_t)a * d + b] += X[(size_t)i * d + a] * X[(size_t)i * d + b];
    }
  }
}

void run_case(int d, int G, bool zero_gram, const std::vector<Problem>& probs) {
  const int n = 200;
  std::vector<double> Q, q, yn(G);
  for (int g = 0; g < G; ++g) {
    std::vector<double> Qg, qg;
    make_gram(n, d, d > 4 ? 3 : -1, Qg, qg, &yn[g]);
    if (zero_gram && g == 0) Qg.assign(Qg.size(), 0.0);
    Q.insert(Q.end(), Qg.begin(), Qg.end());
    q.insert(q.end(), qg.begin(), qg.end());
  }
  const int64_t F = (int64_t)probs.size();
  std::vector<int32_t> gid(F), pos(F), mi(F), n_iter(F, -7);
  std::vector<double> l1(F), l2(F), tol(F), w((size_t)F * d, 99.0), gap(F, -1.0), tol_eff(F, -1.0);
  for (int64_t f = 0; f < F; ++f) {
    gid[f] = probs[f].g; pos[f] = probs[f].positive; mi[f] = probs[f].max_iter;
    l1[f] = probs[f].l1; l2[f] = probs[f].l2; tol[f] = probs[f].tol;
  }
  dml::EnetArgs a{};
  a.Q = (int64_t)(uintptr_t)Q.data(); a.q = (int64_t)(uintptr_t)q.data(); a.ynorm2 = (int64_t)(uintptr_t)yn.data();
  a.gram_id = (int64_t)(uintptr_t)gid.data(); a.l1 = (int64_t)(uintptr_t)l1.data(); a.l2 = (int64_t)(uintptr_t)l2.data();
  a.positive = (int64_t)(uintptr_t)pos.data(); a.max_iter = (int64_t)(uintptr_t)mi.data();
  a.tol = (int64_t)(uintptr_t)tol.data(); a.w = (int64_t)(uintptr_t)w.data(); a.gap = (int64_t)(uintptr_t)gap.data();
  a.tol_eff = (int64_t)(uintptr_t)tol_eff.data(); a.n_iter = (int64_t)(uintptr_t)n_iter.data();
  a.F = F; a.d = d; a.G = G;
  CHECK(dml_cpu_enet_cd(&a) == dml::kEnetOk);
  for (int64_t f = 0; f < F; ++f) {
    std::vector<double> wr;
    double gr;
    int nr;
    const int g = probs[f].g;
    scalar_cd(d, Q.data() + (size_t)g * d * d, q.data() + (size_t)g * d, yn[g], probs[f], wr, &gr, &nr);
    // the scalar loop sums in another order: agreement to rounding, the same sweep count on
    // these well-separated cases
    CHECK(n_iter[f] == nr);
    CHECK(tol_eff[f] == probs[f].tol * yn[g]);
    CHECK(fabs(gap[f] - gr) <= 1e-9 * yn[g]);
    double wmax = 0.0, dev = 0.0;
    for (int j = 0; j < d; ++j) {
      wmax = fmax(wmax, fabs(wr[j]));
      dev = fmax(dev, fabs(wr[j] - w[(size_t)f * d + j]));
      if (probs[f].positive) CHECK(w[(size_t)f * d + j] >= 0.0);
    }
    CHECK(dev <= 1e-9 * fmax(wmax, 1e-300));
    if (d > 4) CHECK(w[(size_t)f * d + 3] == 0.0);   // the constant column is skipped
    if (zero_gram && g == 0) CHECK(wmax == 0.0);   // every coordinate skipped
  }
}

}  // namespace

int main() {
  CHECK(dml_cpu_enet_sizeof_args() == (int)sizeof(dml::EnetArgs));
  const int n = 200;
  // l1 is alpha * n: 0.05 * n keeps a few coefficients, 50 * n none
  const std::vector<Problem> mix = {
      {0, 0.05 * n, 0.0, 0, 1000, 1e-4},      {1, 0.02 * n, 0.02 * n, 0, 1000, 1e-4},
      {0, 0.05 * n, 0.0, 1, 1000, 1e-4},      {1, 0.05 * n, 0.0, 0, 1, 1e-4},
      {0, 50.0 * n, 0.0, 0, 1000, 1e-4},      {1, 0.001 * n, 0.0, 0, 100000, 1e-10},
      {0, 0.0, 0.3 * n, 0, 1000, 1e-4},       {1, 0.01 * n, 0.01 * n, 1, 2, 1e-4},
  };
  run_case(1, 2, false, mix);
  run_case(65, 2, false, mix);
  run_case(7, 2, true, mix);    // Gram 0 all zero
  run_case(3, 2, false, {});    // F = 0
  {   // bad arguments are refused before anything is read
    dml::EnetArgs a{};
    a.F = 1; a.d = 0; a.G = 1;
    CHECK(dml_cpu_enet_cd(&a) == dml::kEnetBadArgs);
    a.d = 3;
    CHECK(dml_cpu_enet_cd(&a) == dml::kEnetBadArgs);   // null pointers
  }
  if (failures) {
    fprintf(stderr, "enet_selftest: %d check(s) failed\n", failures);
    return 1;
  }
  printf("enet_selftest: ok\n");
  return 0;
}
