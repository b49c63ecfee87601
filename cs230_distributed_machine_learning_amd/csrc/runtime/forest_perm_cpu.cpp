// forest_perm_cpu.cpp -- permutation-importance score statistics of a kept fit on the host:
// the twin of ../kernels/predict.hip k_perm_cls / k_perm_reg.  Same definition and the same
// order of every floating-point operation of a prediction (trees ascending, classes ascending,
// float sums for the class fractions, a double sum for the regression means), so the
// predictions agree bit for bit and the match counts are equal; the squared errors are summed
// per block of 256 rows in row order and the blocks in block order (the kernel sums a block's
// rows by lane shuffles), so the SSE agrees to rounding.  This is the CPU data path and the
// reference the GPU test compares against.
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

// leaf of tree t for bins xr with feature f's bin replaced by sub (f < 0: nothing replaced);
// feats (optional) collects the features of the visited split nodes
inline int leaf_of(const Walk& w, const uint8_t* xr, int t, int f, int sub, std::vector<int32_t>* feats) {
  int node = t;
  NodeRec nr = w.nodes[node];
  for (int steps = 0; nr.split >= 0 && steps < w.cap; ++steps) {
    const int feat = nr.split >> 8;
    if (feats) feats->push_back(feat);
    const int bin = feat == f ? sub : xr[feat];
    node = nr.left + (bin > (nr.split & 255) ? 1 : 0);
    nr = w.nodes[node];
  }
  return node;
}

// the forest's prediction from one leaf per tree: class id (first maximum) or the float mean
inline void predict_leaves(const Walk& w, const int* leaf, std::vector<float>& p, int32_t* cls, float* reg) {
  if (w.is_reg) {
    double acc = 0.0;
    int n = 0;
    for (int t = w.t0; t < w.t1; ++t) {
      const double* v = w.val + (int64_t)leaf[t - w.t0] * w.VC;
      if (v[0] > 0.0) { acc += v[1] / v[0]; ++n; }
    }
    *reg = n ? (float)(acc / n) : 0.f;
    return;
  }
  for (int k = 0; k < w.C; ++k) p[k] = 0.f;
  for (int t = w.t0; t < w.t1; ++t) {
    const double* v = w.val + (int64_t)leaf[t - w.t0] * w.VC;
    double W = 0.0;
    for (int k = 0; k < w.C; ++k) W += v[k];
    if (W > 0.0) {
      const double inv = 1.0 / W;
      for (int k = 0; k < w.C; ++k) p[k] += (float)(v[k] * inv);
    }
  }
  int best = 0;
  float bv = p[0];
  for (int k = 1; k < w.C; ++k)
    if (p[k] > bv) { bv = p[k]; best = k; }
  *cls = best;
}

}  // namespace

extern "C" {

// rows[n_rows]: dataset row ids (the fit's held-out rows); perm: int32 [K][n_rows] positions in
// rows[]; features: int32 [F] feature ids or -1 (a slot that equals the baseline); trees
// [t0, t1) of the pool, read down to depth_cap levels (<= 0: whole trees).  part: scratch
// [ceil(n_rows / 256)][F][K], out: [F][K] -- int64 match counts (classification, ycls by
// dataset row) or double squared errors (regression, yreg); pred (optional): [F][K][n_rows]
// int32 class / float prediction; walked (optional): uint64 [F] (row, tree, repeat) slots that
// were walked a second time.
void dml_cpu_forest_perm(const uint8_t* Xb, int64_t ld, const NodeRec* nodes, const double* val, int64_t VC,
                         int64_t is_reg, int64_t C, int32_t t0, int32_t t1, const int32_t* rows, int64_t n_rows,
                         int32_t depth_cap, const int32_t* perm, int64_t K, const int32_t* features, int64_t F,
                         const int32_t* ycls, const float* yreg, void* part, void* out, void* pred,
                         uint64_t* walked) {
  const Walk w{Xb, ld, nodes, val, VC, C, is_reg != 0, t0, t1, depth_cap > 0 ? depth_cap : 1 << 20};
  const int T = t1 - t0;
  const int64_t blocks = (n_rows + 255) / 256, FK = F * K;
  int64_t* part_i = (int64_t*)part;
  double* part_d = (double*)part;
  if (walked)
    for (int64_t fi = 0; fi < F; ++fi) walked[fi] = 0;
#pragma omp parallel
  {
    std::vector<float> p(is_reg ? 1 : (size_t)C);
    std::vector<int> base(T), leaf(T);
    std::vector<int32_t> path, path_off(T + 1);
    std::vector<uint64_t> nw(F, 0);
#pragma omp for schedule(dynamic)
    for (int64_t b = 0; b < blocks; ++b) {
      for (int64_t j = 0; j < FK; ++j) {
        if (is_reg) part_d[b * FK + j] = 0.0;
        else part_i[b * FK + j] = 0;
      }
      const int64_t i1 = b * 256 + 256 < n_rows ? b * 256 + 256 : n_rows;
      for (int64_t i = b * 256; i < i1; ++i) {
        const int32_t row = rows[i];
        const uint8_t* xr = Xb + (int64_t)row * ld;
        path.clear();
        for (int t = 0; t < T; ++t) {
          path_off[t] = (int32_t)path.size();
          base[t] = leaf_of(w, xr, t0 + t, -1, 0, &path);
        }
        path_off[T] = (int32_t)path.size();
        int32_t bcls = 0;
        float breg = 0.f;
        predict_leaves(w, base.data(), p, &bcls, &breg);
        for (int64_t fi = 0; fi < F; ++fi) {
          const int f = features[fi];
          for (int64_t k = 0; k < K; ++k) {
            int32_t pc = bcls;
            float pr = breg;
            const int sub = f >= 0 ? Xb[(int64_t)rows[perm[k * n_rows + i]] * ld + f] : 0;
            if (f >= 0 && sub != xr[f]) {
              bool any = false;
              for (int t = 0; t < T; ++t) {
                bool hit = false;
                for (int32_t q = path_off[t]; q < path_off[t + 1]; ++q) hit |= path[q] == f;
                leaf[t] = hit ? leaf_of(w, xr, t0 + t, f, sub, nullptr) : base[t];
                if (hit) { any = true; ++nw[fi]; }
              }
              if (any) predict_leaves(w, leaf.data(), p, &pc, &pr);
            }
            if (is_reg) {
              const double er = (double)pr - (double)yreg[row];
              part_d[b * FK + fi * K + k] += er * er;
              if (pred) ((float*)pred)[(fi * K + k) * n_rows + i] = pr;
            } else {
              part_i[b * FK + fi * K + k] += pc == ycls[row] ? 1 : 0;
              if (pred) ((int32_t*)pred)[(fi * K + k) * n_rows + i] = pc;
            }
          }
        }
      }
    }
    if (walked) {
#pragma omp critical
      for (int64_t fi = 0; fi < F; ++fi) walked[fi] += nw[fi];
    }
  }
  for (int64_t j = 0; j < FK; ++j) {
    if (is_reg) {
      double s = 0.0;
      for (int64_t b = 0; b < blocks; ++b) s += part_d[b * FK + j];
      ((double*)out)[j] = s;
    } else {
      int64_t s = 0;
      for (int64_t b = 0; b < blocks; ++b) s += part_i[b * FK + j];
      ((int64_t*)out)[j] = s;
    }
  }
}

}  // extern "C"
