// forest_pd_cpu.cpp -- one-way partial dependence of a kept fit on the host: the twin of
// ../kernels/predict.hip k_pd_cls / k_pd_reg / k_pd_reduce.  Same definition and the same order of
// every floating-point operation: a row's value is k_predict_cls / k_predict_reg's (trees
// ascending, classes ascending, float sums for the class fractions, a double sum for the
// regression means); the 256 values of a block are added as the kernel adds them (the xor-shuffle
// tree over the 64 lanes of a wave, then the four waves ascending) and the blocks in block order,
// so the sums agree with the kernel's to the last bit.  The `walked` count follows the kernel's
// skip rule (per group of `group` lock-step trees, the bin interval of feature f over which no
// tree of the group changes its leaf).  This is the CPU data path and the reference the GPU test
// compares against.
#include <stdint.h>
#include <vector>
#include "../kernels/forest_common.h"

using namespace dml;

namespace {

struct Walk {
  const uint8_t* Xb;
  int64_t ld;
  const NodeRec* nodes;
  const double* val;
  int64_t VC, C;
  bool is_reg;
  int t0, t1, cap;
};

struct Step {   // one visited split node of a baseline walk
  int32_t feat;
  int16_t split;
  int16_t right;
};

// leaf of tree t for bins xr with feature f's bin replaced by sub (f < 0: nothing replaced);
// path (optional) collects the visited split nodes
inline int leaf_of(const Walk& w, const uint8_t* xr, int t, int f, int sub, std::vector<Step>* path) {
  int node = t;
  NodeRec nr = w.nodes[node];
  for (int steps = 0; nr.split >= 0 && steps < w.cap; ++steps) {
    const int feat = nr.split >> 8, thr = nr.split & 255;
    const int bin = feat == f ? sub : xr[feat];
    const int b = bin > thr ? 1 : 0;
    if (path) path->push_back(Step{feat, (int16_t)thr, (int16_t)b});
    node = nr.left + b;
    nr = w.nodes[node];
  }
  return node;
}

// the forest's value for one row from one leaf per tree: v[0 .. C) class fractions (float32), or
// v[0] the float32 mean
inline void value_of(const Walk& w, const int* leaf, float* v) {
  const int T = w.t1 - w.t0;
  if (w.is_reg) {
    double acc = 0.0;
    int n = 0;
    for (int t = 0; t < T; ++t) {
      const double* q = w.val + (int64_t)leaf[t] * w.VC;
      if (q[0] > 0.0) { acc += q[1] / q[0]; ++n; }
    }
    v[0] = n ? (float)(acc / n) : 0.f;
    return;
  }
  for (int k = 0; k < w.C; ++k) v[k] = 0.f;
  for (int t = 0; t < T; ++t) {
    const double* q = w.val + (int64_t)leaf[t] * w.VC;
    double W = 0.0;
    for (int k = 0; k < w.C; ++k) W += q[k];
    if (W > 0.0) {
      const double inv = 1.0 / W;
      for (int k = 0; k < w.C; ++k) v[k] += (float)(q[k] * inv);
    }
  }
  const float nt = (float)T;
  for (int k = 0; k < w.C; ++k) v[k] = v[k] / nt;
}

// the kernel's block sum of 256 lane values: lanes by xor-shuffle (offsets 32 .. 1), then the
// four waves ascending
inline double block_sum(double* lane) {
  for (int wv = 0; wv < 4; ++wv) {
    double* s = lane + 64 * wv;
    for (int off = 32; off >= 1; off >>= 1)
      for (int i = 0; i < off; ++i) s[i] = s[i] + s[i + off];
  }
  return lane[0] + lane[64] + lane[128] + lane[192];
}

}  // namespace

extern "C" {

// rows[n_rows]: dataset row ids; features: int32 [F] feature ids or -1 (the baseline slot);
// sub_bins: uint8 [F][Gmax], of which slot fi uses the first n_grid[fi]; trees [t0, t1) of the
// pool, read down to depth_cap levels (<= 0: whole trees).  The targets are classes
// [c0, c0 + n_targets) (regression: the one mean).  part: scratch [ceil(n_rows / 256)][F][Gmax]
// [n_targets], out: [F][Gmax][n_targets] -- double sums over the rows (entries past n_grid are
// not written); rows_out (optional): float [F][Gmax][n_rows][n_targets]; walked (optional):
// uint64 [F] (row, tree, grid point) slots that were walked a second time.
void dml_cpu_forest_pd(const uint8_t* Xb, int64_t ld, const NodeRec* nodes, const double* val, int64_t VC,
                       int64_t is_reg, int64_t C, int32_t t0, int32_t t1, const int32_t* rows, int64_t n_rows,
                       int32_t depth_cap, const int32_t* features, int64_t F, const uint8_t* sub_bins, int64_t Gmax,
                       const int32_t* n_grid, int64_t n_targets, int64_t c0, int32_t group, int32_t no_skip,
                       double* part, double* out, float* rows_out, uint64_t* walked) {
  const Walk w{Xb, ld, nodes, val, VC, C, is_reg != 0, t0, t1, depth_cap > 0 ? depth_cap : 1 << 20};
  const int T = t1 - t0, U = group > 0 ? group : 8, NG = (T + U - 1) / U;
  const int64_t blocks = (n_rows + 255) / 256, NT = n_targets, FGN = F * Gmax * NT;
  if (walked)
    for (int64_t fi = 0; fi < F; ++fi) walked[fi] = 0;
#pragma omp parallel
  {
    std::vector<float> v(is_reg ? 1 : (size_t)C);
    std::vector<int> base((size_t)256 * T), leaf(T);
    std::vector<Step> path;
    std::vector<int64_t> path_off((size_t)256 * T + 1);
    std::vector<uint8_t> hit((size_t)256 * T);
    std::vector<int> lo((size_t)256 * NG), hi((size_t)256 * NG);
    std::vector<double> lane((size_t)256 * NT);
    std::vector<uint64_t> nw(F, 0);
#pragma omp for schedule(dynamic)
    for (int64_t b = 0; b < blocks; ++b) {
      const int64_t i0 = b * 256;
      const int live = (int)(i0 + 256 < n_rows ? 256 : n_rows - i0);
      path.clear();
      for (int r = 0; r < live; ++r) {
        const uint8_t* xr = Xb + (int64_t)rows[i0 + r] * ld;
        for (int t = 0; t < T; ++t) {
          path_off[(size_t)r * T + t] = (int64_t)path.size();
          base[(size_t)r * T + t] = leaf_of(w, xr, t0 + t, -1, 0, &path);
        }
      }
      path_off[(size_t)live * T] = (int64_t)path.size();
      for (int64_t fi = 0; fi < F; ++fi) {
        const int f = features[fi];
        // per row: which trees visit a node on f, and per group the bins that keep every leaf
        for (int r = 0; r < live; ++r) {
          for (int g = 0; g < NG; ++g) { lo[(size_t)r * NG + g] = 0; hi[(size_t)r * NG + g] = 255; }
          for (int t = 0; t < T; ++t) {
            bool h = false;
            int& l = lo[(size_t)r * NG + t / U];
            int& u = hi[(size_t)r * NG + t / U];
            for (int64_t q = path_off[(size_t)r * T + t]; q < path_off[(size_t)r * T + t + 1]; ++q) {
              if (path[q].feat != f) continue;
              h = true;
              if (path[q].right) { if (path[q].split + 1 > l) l = path[q].split + 1; }
              else if (path[q].split < u) u = path[q].split;
            }
            hit[(size_t)r * T + t] = (no_skip || h) ? 1 : 0;
          }
        }
        for (int64_t g = 0; g < n_grid[fi]; ++g) {
          const int sub = sub_bins[fi * Gmax + g];
          for (size_t j = 0; j < lane.size(); ++j) lane[j] = 0.0;
          for (int r = 0; r < live; ++r) {
            const uint8_t* xr = Xb + (int64_t)rows[i0 + r] * ld;
            for (int t = 0; t < T; ++t) {
              const bool in = sub >= lo[(size_t)r * NG + t / U] && sub <= hi[(size_t)r * NG + t / U];
              const bool again = hit[(size_t)r * T + t] && (no_skip || !in);
              leaf[t] = again ? leaf_of(w, xr, t0 + t, f, sub, nullptr) : base[(size_t)r * T + t];
              if (again) ++nw[fi];
            }
            value_of(w, leaf.data(), v.data());
            for (int64_t k = 0; k < NT; ++k) {
              const float x = v[is_reg ? 0 : c0 + k];
              lane[(size_t)k * 256 + r] = (double)x;
              if (rows_out) rows_out[((fi * Gmax + g) * n_rows + i0 + r) * NT + k] = x;
            }
          }
          for (int64_t k = 0; k < NT; ++k)
            part[b * FGN + (fi * Gmax + g) * NT + k] = block_sum(lane.data() + (size_t)k * 256);
        }
      }
    }
    if (walked) {
#pragma omp critical
      for (int64_t fi = 0; fi < F; ++fi) walked[fi] += nw[fi];
    }
  }
  for (int64_t fi = 0; fi < F; ++fi)
    for (int64_t g = 0; g < n_grid[fi]; ++g)
      for (int64_t k = 0; k < NT; ++k) {
        const int64_t j = (fi * Gmax + g) * NT + k;
        double s = 0.0;
        for (int64_t b = 0; b < blocks; ++b) s += part[b * FGN + j];
        out[j] = s;
      }
}

}  // extern "C"
