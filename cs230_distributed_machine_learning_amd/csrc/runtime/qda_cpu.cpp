// qda_cpu.cpp -- host twin of csrc/kernels/qda.hip (docs/QDA.md): plain C++ float64, the
// reference of the kernels' GPU tests.
//
// dml_cpu_qda_class_moments adds in the kernel's order: a cell's rows are cut into slabs of
// kQdaSlabRows, partition p takes slabs p, p + parts, ... and adds their rows in ascending order,
// one fused multiply-add per row and entry (the matrix instruction's step over 4 rows is taken as
// 4 fused multiply-adds in row order); the partitions are then added in ascending order from 0.
// dml_cpu_qda_score is the formula as written, in no particular order of the kernel's.
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "qda_args.h"

namespace {

using dml::QdaMomArgs;
using dml::QdaScoreArgs;

template <typename T>
inline T* ptr(int64_t v) {
  return reinterpret_cast<T*>(static_cast<uintptr_t>(v));
}

inline int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }

}  // namespace

extern "C" {

int dml_cpu_qda_sizeof_mom_args() { return (int)sizeof(QdaMomArgs); }
int dml_cpu_qda_sizeof_score_args() { return (int)sizeof(QdaScoreArgs); }

// 0: done; 2: bad arguments.  No limit on d.  `part` is not used.
int dml_cpu_qda_class_moments(const QdaMomArgs* a) {
  if (a->n < 0 || a->d < 1 || a->n_cells < 0 || a->ld < a->d || a->parts < 1 || a->parts > dml::kQdaMaxParts)
    return dml::kQdaBadArgs;
  if (a->n_cells == 0) return dml::kQdaOk;
  if (!a->shift || !a->perm || !a->cell_off || !a->out || (a->n > 0 && !a->X)) return dml::kQdaBadArgs;
  const int64_t d = a->d, Dp = up16(d + 1), P = a->parts, n = a->n;
  const float* X = ptr<const float>(a->X);
  const double* shift = ptr<const double>(a->shift);
  const int32_t* perm = ptr<const int32_t>(a->perm);
  const int64_t* cell_off = ptr<const int64_t>(a->cell_off);
  for (int64_t cell = 0; cell <= a->n_cells; ++cell)
    if (cell_off[cell] < 0 || cell_off[cell] > n || (cell > 0 && cell_off[cell] < cell_off[cell - 1]))
      return dml::kQdaBadArgs;
  for (int64_t i = 0; i < n; ++i)
    if (perm[i] < 0 || perm[i] >= n) return dml::kQdaBadArgs;
#pragma omp parallel
  {
    std::vector<double> acc((size_t)(Dp * Dp)), z((size_t)Dp);
#pragma omp for schedule(dynamic, 1)
    for (int64_t cell = 0; cell < a->n_cells; ++cell) {
      double* out = ptr<double>(a->out) + cell * Dp * Dp;
      for (int64_t e = 0; e < Dp * Dp; ++e) out[e] = 0.0;
      const int64_t r0 = cell_off[cell], r1 = cell_off[cell + 1];
      const int64_t n_slabs = (r1 - r0 + dml::kQdaSlabRows - 1) / dml::kQdaSlabRows;
      for (int64_t p = 0; p < P; ++p) {
        for (int64_t e = 0; e < Dp * Dp; ++e) acc[e] = 0.0;
        for (int64_t s = p; s < n_slabs; s += P) {
          const int64_t b = r0 + s * dml::kQdaSlabRows;
          for (int64_t pos = b; pos < b + dml::kQdaSlabRows && pos < r1; ++pos) {
            const float* x = X + (int64_t)perm[pos] * a->ld;
            for (int64_t c = 0; c < Dp; ++c) z[c] = c < d ? (double)x[c] - shift[c] : (c == d ? 1.0 : 0.0);
            for (int64_t i = 0; i < Dp; ++i)
              for (int64_t j = i / 16 * 16; j < Dp; ++j) acc[i * Dp + j] = std::fma(z[i], z[j], acc[i * Dp + j]);
          }
        }
        for (int64_t i = 0; i < Dp; ++i)
          for (int64_t j = i / 16 * 16; j < Dp; ++j) out[i * Dp + j] = out[i * Dp + j] + acc[i * Dp + j];
      }
    }
  }
  return dml::kQdaOk;
}

// 0: done; 2: bad arguments.  No limit on d or NC.
int dml_cpu_qda_score(const QdaScoreArgs* a) {
  if (a->n < 0 || a->d < 1 || a->S < 0 || a->C < 1 || a->NC < 1 || a->total_rows < 0 || a->ld < a->d)
    return dml::kQdaBadArgs;
  if (a->S == 0 || a->total_rows == 0) return dml::kQdaOk;
  if (!a->X || !a->rows || !a->row_off || !a->mu || !a->V || !a->inv || !a->cst || !a->pred) return dml::kQdaBadArgs;
  const int64_t d = a->d, C = a->C, NC = a->NC, S = a->S, total = a->total_rows;
  const float* X = ptr<const float>(a->X);
  const int32_t* rows = ptr<const int32_t>(a->rows);
  const int64_t* row_off = ptr<const int64_t>(a->row_off);
  for (int64_t s = 0; s <= S; ++s)
    if (row_off[s] < 0 || row_off[s] > total || (s > 0 && row_off[s] < row_off[s - 1])) return dml::kQdaBadArgs;
  for (int64_t i = 0; i < total; ++i)
    if (rows[i] < 0 || rows[i] >= a->n) return dml::kQdaBadArgs;
  const double* mu = ptr<const double>(a->mu);
  const double* V = ptr<const double>(a->V);
  const double* inv = ptr<const double>(a->inv);
  const double* cst = ptr<const double>(a->cst);
  int32_t* pred = ptr<int32_t>(a->pred);
  double* dec = ptr<double>(a->dec);
  for (int64_t s = 0; s < S; ++s) {
#pragma omp parallel
    {
      std::vector<double> z((size_t)d), best((size_t)NC);
      std::vector<int32_t> bestc((size_t)NC);
#pragma omp for schedule(static)
      for (int64_t i = row_off[s]; i < row_off[s + 1]; ++i) {
        const float* x = X + (int64_t)rows[i] * a->ld;
        for (int64_t k = 0; k < NC; ++k) {
          best[k] = -INFINITY;
          bestc[k] = 0;
        }
        for (int64_t c = 0; c < C; ++c) {
          const double* m = mu + (s * C + c) * d;
          const double* Vc = V + (s * C + c) * d * d;
          for (int64_t j = 0; j < d; ++j) z[j] = 0.0;
          for (int64_t k = 0; k < d; ++k) {
            const double xm = (double)x[k] - m[k];
            for (int64_t j = 0; j < d; ++j) z[j] += xm * Vc[k * d + j];
          }
          for (int64_t k = 0; k < NC; ++k) {
            const double* w = inv + ((s * NC + k) * C + c) * d;
            double q = 0.0;
            for (int64_t j = 0; j < d; ++j) q += z[j] * z[j] * w[j];
            const double v = cst[(s * NC + k) * C + c] - 0.5 * q;
            if (dec) dec[(k * total + i) * C + c] = v;
            if (v > best[k]) {
              best[k] = v;
              bestc[k] = (int32_t)c;
            }
          }
        }
        for (int64_t k = 0; k < NC; ++k) pred[k * total + i] = bestc[k];
      }
    }
  }
  return dml::kQdaOk;
}

}  // extern "C"
