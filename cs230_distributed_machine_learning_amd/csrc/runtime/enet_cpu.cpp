// enet_cpu.cpp -- host twin of csrc/kernels/enet.hip (dml_enet_cd): sklearn's
// enet_coordinate_descent_gram (sklearn/linear_model/_cd_fast.pyx), float64, cyclic, started
// from w = 0, for F problems that share G Gram matrices; OpenMP over problems.
//
// It is the CPU data path's solver and the kernel's reference: w, gap and n_iter are bit-equal
// to the kernel's.  What makes that hold:
//   * the two H updates of a coordinate are explicit fused multiply-adds (std::fma here, fma on
//     the device), everything else is separately rounded (the library is built with
//     -ffp-contract=off, the kernel under `#pragma clang fp contract(off)`);
//   * a reduction of the gap adds, per wave lane l = 0..63, the terms of entries l, l + 64, ...
//     in ascending order and then combines the 64 partials by the xor-shuffle tree
//     (masks 32, 16, 8, 4, 2, 1) -- the order of the kernel's wave::sum.
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "enet_args.h"

namespace {

using dml::EnetArgs;

template <typename T>
inline T* ptr(int64_t v) {
  return reinterpret_cast<T*>(static_cast<uintptr_t>(v));
}

// H[j] = fma(b, row[j], fma(a, row[j], H[j])), each half only when its factor is nonzero
void axpy2_generic(int64_t d, double a, double b, const double* row, double* H) {
  for (int64_t j = 0; j < d; ++j) {
    double h = H[j];
    if (a != 0.0) h = std::fma(a, row[j], h);
    if (b != 0.0) h = std::fma(b, row[j], h);
    H[j] = h;
  }
}

#if defined(__x86_64__) && defined(__GNUC__)
// the same fused operations as hardware instructions (a fused multiply-add is exactly rounded
// either way, so both variants give the same bits)
__attribute__((target("avx2,fma"))) void axpy2_fma(int64_t d, double a, double b, const double* row, double* H) {
  if (a != 0.0 && b != 0.0) {
    for (int64_t j = 0; j < d; ++j) H[j] = __builtin_fma(b, row[j], __builtin_fma(a, row[j], H[j]));
  } else if (a != 0.0) {
    for (int64_t j = 0; j < d; ++j) H[j] = __builtin_fma(a, row[j], H[j]);
  } else if (b != 0.0) {
    for (int64_t j = 0; j < d; ++j) H[j] = __builtin_fma(b, row[j], H[j]);
  }
}
bool have_fma() {
  static const bool v = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
  return v;
}
#else
void axpy2_fma(int64_t d, double a, double b, const double* row, double* H) { axpy2_generic(d, a, b, row, H); }
bool have_fma() { return false; }
#endif

// the kernel's wave reduction: 64 lane partials combined by the xor tree
double tree_sum(double* p) {
  double t[64];
  for (int m = 32; m >= 1; m >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = p[l] + p[l ^ m];
    for (int l = 0; l < 64; ++l) p[l] = t[l];
  }
  return p[0];
}

template <typename Term>
double lane_sum(int64_t d, Term term) {
  double p[64];
  for (int l = 0; l < 64; ++l) {
    double s = 0.0;
    for (int64_t j = l; j < d; j += 64) s = s + term(j);
    p[l] = s;
  }
  return tree_sum(p);
}

void solve_one(const EnetArgs& a, int64_t f, double* H) {
  const int64_t d = a.d;
  const int32_t g = ptr<const int32_t>(a.gram_id)[f];
  const double* Q = ptr<const double>(a.Q) + (int64_t)g * d * d;
  const double* q = ptr<const double>(a.q) + (int64_t)g * d;
  const double yn = ptr<const double>(a.ynorm2)[g];
  const double l1 = ptr<const double>(a.l1)[f], l2 = ptr<const double>(a.l2)[f];
  const bool positive = ptr<const int32_t>(a.positive)[f] != 0;
  const int32_t max_iter = ptr<const int32_t>(a.max_iter)[f];
  const double tol = ptr<const double>(a.tol)[f];
  const double tol_eff = tol * yn;
  double* w = ptr<double>(a.w) + f * d;
  const bool hw_fma = have_fma();
  for (int64_t j = 0; j < d; ++j) w[j] = H[j] = 0.0;
  double gap = tol + 1.0;
  int32_t n_iter = 0;
  for (int32_t it = 0; it < max_iter; ++it) {
    n_iter = it + 1;
    double w_max = 0.0, d_w_max = 0.0;
    for (int64_t ii = 0; ii < d; ++ii) {
      const double* row = Q + ii * d;
      const double qii = row[ii];
      if (qii == 0.0) continue;
      const double w_ii = w[ii];
      double hii = H[ii];
      if (w_ii != 0.0) hii = std::fma(-w_ii, qii, hii);
      const double tmp = q[ii] - hii;
      double wn;
      if (positive && tmp < 0.0) {
        wn = 0.0;
      } else {
        const double m = fabs(tmp) - l1;
        const double s = tmp > 0.0 ? 1.0 : (tmp < 0.0 ? -1.0 : 0.0);
        wn = (s * (m > 0.0 ? m : 0.0)) / (qii + l2);
      }
      w[ii] = wn;
      if (w_ii != 0.0 || wn != 0.0) {
        if (hw_fma) axpy2_fma(d, -w_ii, wn, row, H);
        else axpy2_generic(d, -w_ii, wn, row, H);
      }
      const double d_w_ii = fabs(wn - w_ii);
      if (d_w_ii > d_w_max) d_w_max = d_w_ii;
      if (fabs(wn) > w_max) w_max = fabs(wn);
    }
    if (w_max == 0.0 || d_w_max / w_max < tol || it == max_iter - 1) {
      const double q_dot_w = lane_sum(d, [&](int64_t j) { return w[j] * q[j]; });
      double dual = positive ? -INFINITY : 0.0;
      for (int64_t j = 0; j < d; ++j) {
        double x = (q[j] - H[j]) - l2 * w[j];
        if (!positive) x = fabs(x);
        if (x > dual) dual = x;
      }
      const double wH = lane_sum(d, [&](int64_t j) { return w[j] * H[j]; });
      const double R = (yn + wH) - 2.0 * q_dot_w;
      const double wn2 = lane_sum(d, [&](int64_t j) { return w[j] * w[j]; });
      const double l1n = lane_sum(d, [&](int64_t j) { return fabs(w[j]); });
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
  ptr<double>(a.gap)[f] = gap;
  ptr<double>(a.tol_eff)[f] = tol_eff;
  ptr<int32_t>(a.n_iter)[f] = n_iter;
}

}  // namespace

extern "C" {

int dml_cpu_enet_sizeof_args() { return (int)sizeof(EnetArgs); }

// 0: solved; 2: bad arguments.  No limit on d.
int dml_cpu_enet_cd(const EnetArgs* a) {
  if (a->F < 0 || a->d < 1 || a->G < 0) return dml::kEnetBadArgs;
  if (a->F == 0) return dml::kEnetOk;
  if (!a->Q || !a->q || !a->ynorm2 || !a->gram_id || !a->l1 || !a->l2 || !a->positive || !a->max_iter || !a->tol ||
      !a->w || !a->gap || !a->tol_eff || !a->n_iter || a->G < 1)
    return dml::kEnetBadArgs;
  const int32_t* gid = ptr<const int32_t>(a->gram_id);
  for (int64_t f = 0; f < a->F; ++f)
    if (gid[f] < 0 || gid[f] >= a->G) return dml::kEnetBadArgs;
#pragma omp parallel
  {
    std::vector<double> H((size_t)a->d);
#pragma omp for schedule(dynamic, 1)
    for (int64_t f = 0; f < a->F; ++f) solve_one(*a, f, H.data());
  }
  return dml::kEnetOk;
}

}  // extern "C"
