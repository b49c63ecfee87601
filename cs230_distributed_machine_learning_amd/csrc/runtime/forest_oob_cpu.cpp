// forest_oob_cpu.cpp -- out-of-bag prediction of a kept fit on the host: the twin of
// ../kernels/predict.hip k_oob_cls / k_oob_reg.  Same definition, same order of every
// floating-point operation (trees ascending, classes ascending, float sums for the class
// fractions, a double sum for the regression means), so the two agree bit for bit; this is
// the CPU data path and the reference the GPU test compares against.
#include <stdint.h>
#include <vector>
#include "../kernels/forest_common.h"

using namespace dml;

extern "C" {

// rows[n_rows]: dataset row ids (the fit's training rows); trees [t0, t1) of the pool, read
// down to depth_cap levels (<= 0: whole trees).  out: float [n_rows][C] (classification) or
// [n_rows] (regression); pred: int32 [n_rows] (classification, may be null); cnt: int32 [n_rows].
void dml_cpu_forest_oob(const uint8_t* Xb, int64_t ld, const NodeRec* nodes, const double* val, int64_t VC,
                        int64_t is_reg, int64_t C, const TreeSpec* specs, int32_t t0, int32_t t1,
                        const int32_t* rows, int64_t n_rows, int32_t depth_cap, float* out, int32_t* pred,
                        int32_t* cnt) {
  const int cap = depth_cap > 0 ? depth_cap : 1 << 20;
#pragma omp parallel
  {
    std::vector<float> p(is_reg ? 1 : (size_t)C);
#pragma omp for schedule(static)
    for (int64_t i = 0; i < n_rows; ++i) {
      const int32_t row = rows[i];
      const uint8_t* xr = Xb + (int64_t)row * ld;
      const uint64_t rk = boot_row_key((uint32_t)row);
      for (size_t k = 0; k < p.size(); ++k) p[k] = 0.f;
      double acc = 0.0;
      int n = 0;
      for (int t = t0; t < t1; ++t) {
        if (!boot_is_oob(specs[t], rk)) continue;
        int node = t;
        NodeRec nr = nodes[node];
        for (int steps = 0; nr.split >= 0 && steps < cap; ++steps) {
          node = nr.left + (xr[nr.split >> 8] > (nr.split & 255) ? 1 : 0);
          nr = nodes[node];
        }
        const double* v = val + (int64_t)node * VC;
        if (is_reg) {
          if (v[0] > 0.0) { acc += v[1] / v[0]; ++n; }
          continue;
        }
        ++n;
        double W = 0.0;
        for (int k = 0; k < C; ++k) W += v[k];
        if (W > 0.0) {
          const double inv = 1.0 / W;
          for (int k = 0; k < C; ++k) p[k] += (float)(v[k] * inv);
        }
      }
      cnt[i] = n;
      if (is_reg) {
        out[i] = n ? (float)(acc / n) : 0.f;
        continue;
      }
      int best = 0;
      float bv = p[0];
      for (int k = 1; k < C; ++k)
        if (p[k] > bv) { bv = p[k]; best = k; }
      if (pred) pred[i] = best;
      const float nt = (float)n;
      for (int k = 0; k < C; ++k) out[i * C + k] = n ? p[k] / nt : 0.f;
    }
  }
}

// boot_weight and boot_is_oob of one (tree, row): the test of their agreement
void dml_boot_weight_oob(const TreeSpec* spec, uint32_t row, uint32_t* out) {
  out[0] = boot_weight(*spec, row);
  out[1] = boot_is_oob(*spec, boot_row_key(row)) ? 1u : 0u;
}

}  // extern "C"
