// predict.hip — batched forest inference and fused per-fit scoring (K6 + K10).
//
// The reference predicts once per fit and scores with sklearn metrics
// (aws-prod/worker/worker.py:322-323 accuracy, :336-338 r2/mse, and inside
// cross_val_score :326/:341).  Here one launch predicts the held-out rows of EVERY
// fit of a batch (grid.y = fit), each thread walking all trees of its fit for one
// row against the HBM-resident binned matrix; a second launch reduces per-fit score
// statistics (correct count / SSE / sum y / sum y^2) so the host gets F x 4 doubles.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

// int64 argument fields -> GLOBAL address-space pointers (flat loads otherwise)
#define GPTR(T, v) ((T*)(__attribute__((address_space(1))) T*)(uintptr_t)(v))
#include "forest_common.h"

namespace dml {

struct PredictArgs {
  int64_t Xb, ld;
  int64_t nodes, node_val, VC, is_reg, n_classes;
  int64_t fit_tree_off;  // int32[F+1]: trees of fit f are [off[f], off[f+1]) (tree t's root = node t)
  int64_t fit_row_off;   // int64[F+1]: rows of fit f in rows[] are [off[f], off[f+1])
  int64_t rows;          // int32[]: row indices to predict
  int64_t out_pred;      // int32 class id (cls) or float (reg), aligned with rows[]
  int64_t out_proba;     // float [len(rows)][C] or 0
  int64_t F, max_rows;
  int64_t d;          // features (bins per row actually read)
  int64_t lds_pitch;  // set by dml_forest_predict: LDS row stride, 0 = no staging
  int64_t fit_row_off_host;   // optional host copy of fit_row_off (per-fit grid sizes)
  int64_t fit_skip;           // optional int32[F] device mask: fits already predicted (early) are skipped
  int64_t fit_depth_cap;      // optional int32[F]: fit f reads its trees only down to this depth (<= 0: all);
                              // prefix fits of a deeper grown forest (models/base.py prefix_groups)
  int64_t toptab;             // optional NodeRec[trees][kTopSlots]: every tree's first kTopLv levels in heap
                              // order (k_top_fill), walked from LDS; 0 = every level from the node pool
  int64_t max_trees;          // max trees of one fit (k_top_fill grid)
};

// The first kTopLv levels of a tree are shared by every row that walks it: they are
// gathered once per predict into a heap-ordered table (slot s: children 2s+1 / 2s+2;
// a slot under a leaf holds {-1, -1}), and a block copies the table of the U trees it is
// walking into LDS with one coalesced read.  Those levels then cost LDS reads instead of
// dependent 8-B gathers through TA / L2 (the walk's first levels are L2 hits, so the
// saving is address-processing and latency, not HBM bytes).
#ifndef DML_PRED_TOP_LV
#define DML_PRED_TOP_LV 7
#endif
constexpr int kTopLv = DML_PRED_TOP_LV;
constexpr int kTopSlots = 1 << kTopLv;   // 2^kTopLv - 1 used + 1 pad
static_assert(kTopLv >= 1 && kTopSlots <= 256, "ops/forest_ops.py TOP_SLOTS_MAX allocates 256 slots per tree");

// leaf of U consecutive trees [t0, t0 + u_n) for one row, walked in lock-step: the U
// dependent node-load chains are independent, so U requests are in flight per thread
// instead of one (tree traversal is latency-bound)
// top (LDS, [kPredU][kTopSlots]) or nullptr: the group's top-level table (see kTopLv)
// kMasked (the out-of-bag walk): slot u is walked only when bit u of `mask` is set -- a masked
// slot starts as a leaf record and issues no load (its leaf[u] stays the root and is not read)
template <int kPredU, bool kMasked = false>
__device__ __forceinline__ void leaves_u(const NodeRec* __restrict__ nodes, const uint8_t* __restrict__ xr, int t0,
                                         int u_n, int (&leaf)[kPredU], int cap, const NodeRec* top,
                                         uint32_t mask = ~0u) {
  NodeRec nr[kPredU];
  int sl[kPredU];
#pragma unroll
  for (int u = 0; u < kPredU; ++u) {
    leaf[u] = t0 + u;
    sl[u] = 0;
    const bool walk = u < u_n && (!kMasked || ((mask >> u) & 1u));
    nr[u] = walk ? (top ? top[u * kTopSlots] : nodes[leaf[u]]) : NodeRec{-1, -1};
  }
  for (int steps = 0; steps < cap; ++steps) {   // step s: every unfinished tree at depth s
    bool any = false;
#pragma unroll
    for (int u = 0; u < kPredU; ++u) any |= nr[u].split >= 0;
    if (!any) break;
    if (top && steps + 1 < kTopLv) {   // depth steps + 1 is in the LDS table (uniform branch)
#pragma unroll
      for (int u = 0; u < kPredU; ++u) {
        if (nr[u].split >= 0) {
          const int b = xr[nr[u].split >> 8] > (nr[u].split & 255) ? 1 : 0;
          leaf[u] = nr[u].left + b;
          sl[u] = 2 * sl[u] + 1 + b;
          nr[u] = top[u * kTopSlots + sl[u]];
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < kPredU; ++u) {
        if (nr[u].split >= 0) {
          leaf[u] = nr[u].left + (xr[nr[u].split >> 8] > (nr[u].split & 255) ? 1 : 0);
          nr[u] = nodes[leaf[u]];
        }
      }
    }
  }
}

// the top-level table of every tree of the launch's fits: one wave per tree, one level per
// round (lane i < 2^l fills slot 2^l - 1 + i from its parent's record)
__global__ __launch_bounds__(256) void k_top_fill(PredictArgs a) {
  __shared__ NodeRec recs[4][kTopSlots];
  const int f = blockIdx.y;
  if (a.fit_skip && (GPTR(const int32_t, a.fit_skip))[f]) return;
  const int32_t* toff = GPTR(const int32_t, a.fit_tree_off);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t = toff[f] + (int)blockIdx.x * 4 + w;
  if (t >= toff[f + 1]) return;   // wave-uniform; the rounds below synchronise within the wave only
  const NodeRec* nodes = GPTR(const NodeRec, a.nodes);
  NodeRec* r = recs[w];
  if (lane == 0) r[0] = nodes[t];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int l = 1; l < kTopLv; ++l) {
    const int n = 1 << l;
    for (int i = lane; i < n; i += 64) {
      const int s = n - 1 + i;
      const NodeRec pr = r[(s - 1) >> 1];
      r[s] = pr.split >= 0 ? nodes[pr.left + ((s - 1) & 1)] : NodeRec{-1, -1};
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  NodeRec* out = GPTR(NodeRec, a.toptab) + (int64_t)t * kTopSlots;
  for (int s = lane; s < kTopSlots; s += 64) out[s] = s < kTopSlots - 1 ? r[s] : NodeRec{-1, -1};
}

// copy the top tables of trees [t, t + u_n) into LDS (block-wide; every thread of the block calls)
template <int kPredU>
__device__ __forceinline__ void load_top(const PredictArgs& a, NodeRec* top, int t, int u_n) {
  __syncthreads();   // the previous group's walks are done with the table
  const uint4* src = (const uint4*)(GPTR(const NodeRec, a.toptab) + (int64_t)t * kTopSlots);
  uint4* dst = (uint4*)top;
  for (int k = threadIdx.x; k < kPredU * kTopSlots / 2; k += 256)
    if (k < u_n * (kTopSlots / 2)) dst[k] = src[k];
  __syncthreads();
}

// depth cap of fit f (1 << 20: none)
__device__ __forceinline__ int depth_cap(const PredictArgs& a, int f) {
  const int c = a.fit_depth_cap ? (GPTR(const int32_t, a.fit_depth_cap))[f] : 0;
  return c > 0 ? c : 1 << 20;
}

// The block's 256 rows are staged in LDS once (dword stride odd -> a wave whose lanes
// read the same feature hits distinct banks), so the ~25 bin reads per tree walk are LDS
// reads and the only vector-memory traffic of the walk is the node-record chain.
// PredictArgs.lds_pitch = row stride in bytes (multiple of 4, <= ld), 0 = read bins from HBM.
__device__ __forceinline__ const uint8_t* stage_rows(const PredictArgs& a, uint8_t* xs, int64_t r0, int64_t nr) {
  const int P = (int)a.lds_pitch, W = P >> 2;
  const int64_t b0 = (int64_t)blockIdx.x * 256;
  __shared__ int32_t srow[256];
  const int64_t i = b0 + threadIdx.x;
  srow[threadIdx.x] = i < nr ? (GPTR(const int32_t, a.rows))[r0 + i] : -1;
  __syncthreads();
  const uint8_t* X = GPTR(const uint8_t, a.Xb);
  for (int k = threadIdx.x; k < 256 * W; k += 256) {
    const int r = k / W, w = k - r * W;
    const int32_t row = srow[r];
    if (row >= 0) ((uint32_t*)xs)[k] = *(const uint32_t*)(X + (int64_t)row * a.ld + 4 * w);
  }
  __syncthreads();
  return xs + threadIdx.x * P;
}

// byte offset of the top table in the dynamic LDS (after the staged rows, 16-B aligned)
__device__ __forceinline__ int64_t top_lds_off(const PredictArgs& a) { return (a.lds_pitch * 256 + 15) & ~15; }

template <int MAXC, int kPredU>
__global__ __launch_bounds__(256) void k_predict_cls(PredictArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t xs_lds[];
  const int f = blockIdx.y;
  if (a.fit_skip && (GPTR(const int32_t, a.fit_skip))[f]) return;
  const int32_t* toff = GPTR(const int32_t, a.fit_tree_off);
  const int64_t* roff = GPTR(const int64_t, a.fit_row_off);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = roff[f], nr = roff[f + 1] - r0;
  if ((int64_t)blockIdx.x * 256 >= nr) return;
  // with the top table every thread stays to the end (block-wide table loads); a thread
  // past the fit's rows walks nothing and writes nothing
  const bool live = i < nr;
  NodeRec* top = a.toptab ? (NodeRec*)(xs_lds + top_lds_off(a)) : nullptr;
  const uint8_t* xr;
  if (a.lds_pitch) {
    xr = stage_rows(a, xs_lds, r0, nr);
    if (!live && !top) return;
  } else {
    if (!live && !top) return;
    xr = GPTR(const uint8_t, a.Xb) + (int64_t)(GPTR(const int32_t, a.rows))[r0 + (live ? i : 0)] * a.ld;
  }
  const int C = (int)a.n_classes;
  const int cap = depth_cap(a, f);
  const NodeRec* nodes = GPTR(const NodeRec, a.nodes);
  const double* val = GPTR(const double, a.node_val);
  float p[MAXC];
#pragma unroll
  for (int k = 0; k < MAXC; ++k) p[k] = 0.f;
  const int tend = toff[f + 1];
  for (int t = toff[f]; t < tend; t += kPredU) {
    int leaf[kPredU];
    const int u_all = min(kPredU, tend - t), u_n = live ? u_all : 0;
    if (top) load_top<kPredU>(a, top, t, u_all);
    leaves_u<kPredU>(nodes, xr, t, u_n, leaf, cap, top);
    // accumulate in tree order (bit-identical to the host predictor)
#pragma unroll
    for (int u = 0; u < kPredU; ++u) {
      if (u >= u_n) break;
      const double* v = val + (int64_t)leaf[u] * a.VC;
      double W = 0.0;
#pragma unroll
      for (int k = 0; k < MAXC; ++k)
        if (k < C) W += v[k];
      if (W > 0.0) {
        const double inv = 1.0 / W;
#pragma unroll
        for (int k = 0; k < MAXC; ++k)
          if (k < C) p[k] += (float)(v[k] * inv);
      }
    }
  }
  if (!live) return;
  int best = 0;
  float bv = p[0];
#pragma unroll
  for (int k = 1; k < MAXC; ++k)
    if (k < C && p[k] > bv) { bv = p[k]; best = k; }
  (GPTR(int32_t, a.out_pred))[r0 + i] = best;
  if (a.out_proba) {
    const float nt = (float)(toff[f + 1] - toff[f]);
    float* op = GPTR(float, a.out_proba) + (r0 + i) * C;
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
      if (k < C) op[k] = p[k] / nt;
  }
}

template <int kPredU>
__global__ __launch_bounds__(256) void k_predict_reg(PredictArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t xs_lds[];
  const int f = blockIdx.y;
  if (a.fit_skip && (GPTR(const int32_t, a.fit_skip))[f]) return;
  const int32_t* toff = GPTR(const int32_t, a.fit_tree_off);
  const int64_t* roff = GPTR(const int64_t, a.fit_row_off);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = roff[f], nr = roff[f + 1] - r0;
  if ((int64_t)blockIdx.x * 256 >= nr) return;
  // with the top table every thread stays to the end (block-wide table loads); a thread
  // past the fit's rows walks nothing and writes nothing
  const bool live = i < nr;
  NodeRec* top = a.toptab ? (NodeRec*)(xs_lds + top_lds_off(a)) : nullptr;
  const uint8_t* xr;
  if (a.lds_pitch) {
    xr = stage_rows(a, xs_lds, r0, nr);
    if (!live && !top) return;
  } else {
    if (!live && !top) return;
    xr = GPTR(const uint8_t, a.Xb) + (int64_t)(GPTR(const int32_t, a.rows))[r0 + (live ? i : 0)] * a.ld;
  }
  const NodeRec* nodes = GPTR(const NodeRec, a.nodes);
  const double* val = GPTR(const double, a.node_val);
  const int cap = depth_cap(a, f);
  double acc = 0.0;
  int nt = 0;
  const int tend = toff[f + 1];
  for (int t = toff[f]; t < tend; t += kPredU) {
    int leaf[kPredU];
    const int u_all = min(kPredU, tend - t), u_n = live ? u_all : 0;
    if (top) load_top<kPredU>(a, top, t, u_all);
    leaves_u<kPredU>(nodes, xr, t, u_n, leaf, cap, top);
#pragma unroll
    for (int u = 0; u < kPredU; ++u) {
      if (u >= u_n) break;
      const double* v = val + (int64_t)leaf[u] * a.VC;
      if (v[0] > 0.0) { acc += v[1] / v[0]; ++nt; }
    }
  }
  if (!live) return;
  (GPTR(float, a.out_pred))[r0 + i] = nt ? (float)(acc / nt) : 0.f;
}

// ---- out-of-bag prediction of a kept fit ----------------------------------------------
// The predict walk over the fit's TRAINING rows, where tree t takes part in row r's
// average iff boot_weight(specs[t], r) == 0 (forest_common.h boot_is_oob: recomputed from
// the tree seed and the row id, nothing stored).  Every thread of a block still walks the
// same U consecutive trees (so the block-wide LDS top table works); the in-bag slots of a
// lane are masked in leaves_u and load nothing.  ../runtime/forest_oob_cpu.cpp is the same
// loop in the same order on the host: the outputs agree bit for bit.
struct OobArgs {
  int64_t Xb, ld, d;
  int64_t nodes, node_val, VC, is_reg, n_classes;
  int64_t specs;         // TreeSpec[] of the pool (indexed by pool tree id)
  int64_t fit_tree_off;  // int32[2] device: the fit's pool trees [t0, t1)
  int64_t fit_row_off;   // int64[2] device: {0, n_rows}
  int64_t t0, t1;
  int64_t rows, n_rows;  // int32[n_rows]: dataset row ids (the split's training rows, ascending)
  int64_t depth_cap;     // <= 0: whole trees
  int64_t out;           // float [n_rows][C] (classification) or [n_rows] (regression)
  int64_t out_pred;      // int32 [n_rows] (classification): first maximum of the row's sums
  int64_t out_cnt;       // int32 [n_rows]: trees that left the row out
  int64_t toptab;        // NodeRec[t1][kTopSlots] scratch or 0
};

struct OobTail {   // what the OOB kernels take besides the predict block
  const TreeSpec* specs;
  int32_t* cnt;
  int cap;
};

// bit u set: tree t + u (u < u_n) left the row out
template <int kPredU>
__device__ __forceinline__ uint32_t oob_mask(const TreeSpec* __restrict__ specs, int t, int u_n, uint64_t row_key) {
  uint32_t m = 0;
#pragma unroll
  for (int u = 0; u < kPredU; ++u)
    if (u < u_n && boot_is_oob(specs[t + u], row_key)) m |= 1u << u;   // specs[t + u]: wave-uniform address
  return m;
}

template <int MAXC, int kPredU>
__global__ __launch_bounds__(256) void k_oob_cls(PredictArgs a, OobTail e) {
  extern __shared__ __attribute__((aligned(16))) uint8_t xs_lds[];
  const int32_t* toff = GPTR(const int32_t, a.fit_tree_off);
  const int64_t* roff = GPTR(const int64_t, a.fit_row_off);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = roff[0], nr = roff[1] - r0;
  if ((int64_t)blockIdx.x * 256 >= nr) return;
  const bool live = i < nr;
  NodeRec* top = a.toptab ? (NodeRec*)(xs_lds + top_lds_off(a)) : nullptr;
  const uint8_t* xr;
  if (a.lds_pitch) {
    xr = stage_rows(a, xs_lds, r0, nr);
    if (!live && !top) return;
  } else {
    if (!live && !top) return;
    xr = nullptr;
  }
  const int32_t row = (GPTR(const int32_t, a.rows))[r0 + (live ? i : 0)];
  if (!a.lds_pitch) xr = GPTR(const uint8_t, a.Xb) + (int64_t)row * a.ld;
  const uint64_t rk = boot_row_key((uint32_t)row);
  const int C = (int)a.n_classes;
  const NodeRec* nodes = GPTR(const NodeRec, a.nodes);
  const double* val = GPTR(const double, a.node_val);
  float p[MAXC];
#pragma unroll
  for (int k = 0; k < MAXC; ++k) p[k] = 0.f;
  int cnt = 0;
  const int tend = toff[1];
  for (int t = toff[0]; t < tend; t += kPredU) {
    int leaf[kPredU];
    const int u_all = min(kPredU, tend - t), u_n = live ? u_all : 0;
    if (top) load_top<kPredU>(a, top, t, u_all);
    const uint32_t m = oob_mask<kPredU>(e.specs, t, u_n, rk);
    leaves_u<kPredU, true>(nodes, xr, t, u_n, leaf, e.cap, top, m);
    // accumulate in tree order (bit-identical to the host twin)
#pragma unroll
    for (int u = 0; u < kPredU; ++u) {
      if (!((m >> u) & 1u)) continue;
      ++cnt;
      const double* v = val + (int64_t)leaf[u] * a.VC;
      double W = 0.0;
#pragma unroll
      for (int k = 0; k < MAXC; ++k)
        if (k < C) W += v[k];
      if (W > 0.0) {
        const double inv = 1.0 / W;
#pragma unroll
        for (int k = 0; k < MAXC; ++k)
          if (k < C) p[k] += (float)(v[k] * inv);
      }
    }
  }
  if (!live) return;
  int best = 0;
  float bv = p[0];
#pragma unroll
  for (int k = 1; k < MAXC; ++k)
    if (k < C && p[k] > bv) { bv = p[k]; best = k; }
  (GPTR(int32_t, a.out_pred))[r0 + i] = best;
  e.cnt[r0 + i] = cnt;
  const float nt = (float)cnt;
  float* op = GPTR(float, a.out_proba) + (r0 + i) * C;
#pragma unroll
  for (int k = 0; k < MAXC; ++k)
    if (k < C) op[k] = cnt ? p[k] / nt : 0.f;
}

template <int kPredU>
__global__ __launch_bounds__(256) void k_oob_reg(PredictArgs a, OobTail e) {
  extern __shared__ __attribute__((aligned(16))) uint8_t xs_lds[];
  const int32_t* toff = GPTR(const int32_t, a.fit_tree_off);
  const int64_t* roff = GPTR(const int64_t, a.fit_row_off);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = roff[0], nr = roff[1] - r0;
  if ((int64_t)blockIdx.x * 256 >= nr) return;
  const bool live = i < nr;
  NodeRec* top = a.toptab ? (NodeRec*)(xs_lds + top_lds_off(a)) : nullptr;
  const uint8_t* xr;
  if (a.lds_pitch) {
    xr = stage_rows(a, xs_lds, r0, nr);
    if (!live && !top) return;
  } else {
    if (!live && !top) return;
    xr = nullptr;
  }
  const int32_t row = (GPTR(const int32_t, a.rows))[r0 + (live ? i : 0)];
  if (!a.lds_pitch) xr = GPTR(const uint8_t, a.Xb) + (int64_t)row * a.ld;
  const uint64_t rk = boot_row_key((uint32_t)row);
  const NodeRec* nodes = GPTR(const NodeRec, a.nodes);
  const double* val = GPTR(const double, a.node_val);
  double acc = 0.0;
  int cnt = 0;
  const int tend = toff[1];
  for (int t = toff[0]; t < tend; t += kPredU) {
    int leaf[kPredU];
    const int u_all = min(kPredU, tend - t), u_n = live ? u_all : 0;
    if (top) load_top<kPredU>(a, top, t, u_all);
    const uint32_t m = oob_mask<kPredU>(e.specs, t, u_n, rk);
    leaves_u<kPredU, true>(nodes, xr, t, u_n, leaf, e.cap, top, m);
#pragma unroll
    for (int u = 0; u < kPredU; ++u) {
      if (!((m >> u) & 1u)) continue;
      const double* v = val + (int64_t)leaf[u] * a.VC;
      if (v[0] > 0.0) { acc += v[1] / v[0]; ++cnt; }
    }
  }
  if (!live) return;
  (GPTR(float, a.out_pred))[r0 + i] = cnt ? (float)(acc / cnt) : 0.f;
  e.cnt[r0 + i] = cnt;
}

// ---- permutation importance of a kept fit on its held-out rows ------------------------------
// For feature f (grid.y, from features[]) and repeat k, row i is predicted from its own bins
// except that feature f's bin comes from row rows[perm[k][i]]; the score statistic of every
// (f, k) is reduced per block.  The prediction rule is k_predict_cls / k_predict_reg's (trees
// ascending, the same float / double sums), so a tree whose leaf does not change adds the same
// value: per group of U trees the baseline is walked once, recording for each slot whether a
// visited node splits on f (`hit`), and a repeat walks again only the hit slots of a row whose
// substituted bin differs from its own.  features[] may hold -1 (no node splits on it): that
// slot's statistics are the baseline's.  ../runtime/forest_perm_cpu.cpp is the host twin.
struct PermArgs {
  int64_t Xb, ld, d;
  int64_t nodes, node_val, VC, is_reg, n_classes;
  int64_t fit_tree_off;  // int32[2] device: the fit's pool trees [t0, t1)
  int64_t fit_row_off;   // int64[2] device: {0, n_rows}
  int64_t t0, t1;
  int64_t rows, n_rows;  // int32[n_rows]: dataset row ids (the split's held-out rows, ascending)
  int64_t depth_cap;     // <= 0: whole trees
  int64_t perm, K;       // int32 [K][n_rows]: positions in rows[]
  int64_t features, F;   // int32 [F]: feature ids, or -1
  int64_t ycls, yreg;    // targets by dataset row id: int32 (classification) / float (regression)
  int64_t part;          // scratch [blocks][F][K]: int64 match counts / double squared errors
  int64_t out;           // [F][K]: the block partials summed in block order
  int64_t out_pred;      // optional [F][K][n_rows]: int32 class / float prediction
  int64_t out_walked;    // optional uint64 [F]: (row, tree, repeat) slots walked a second time
  int64_t toptab;        // NodeRec[t1][kTopSlots] scratch or 0
  int64_t no_skip;       // A/B: walk every tree again for every repeat
};

struct PermTail {   // what the permutation kernels take besides the predict block
  const int32_t* perm;
  const int32_t* features;
  const void* y;
  void* part;
  void* pred;
  unsigned long long* walked;
  int K, F, cap, no_skip;
};

// repeats whose accumulators a thread holds at once (K_chunk x MAXC floats stay in registers)
constexpr int perm_chunk(int maxc) { return maxc <= 4 ? 8 : maxc <= 8 ? 4 : maxc <= 16 ? 2 : 1; }

// leaves_u's masked walk for the permutation kernels.  kRecord: the baseline walk, which sets bit
// u of `hit` when a visited node of slot u splits on feature f.  Otherwise feature f's bin is
// `sub` (substituted in the compare: the rows may not be staged, and a staged byte stays as it is).
template <int kPredU, bool kRecord>
__device__ __forceinline__ void leaves_perm_u(const NodeRec* __restrict__ nodes, const uint8_t* __restrict__ xr, int t0,
                                              int u_n, int (&leaf)[kPredU], int cap, const NodeRec* top, uint32_t mask,
                                              int f, int sub, uint32_t& hit) {
  NodeRec nr[kPredU];
  int sl[kPredU];
#pragma unroll
  for (int u = 0; u < kPredU; ++u) {
    leaf[u] = t0 + u;
    sl[u] = 0;
    const bool walk = u < u_n && ((mask >> u) & 1u);
    nr[u] = walk ? (top ? top[u * kTopSlots] : nodes[leaf[u]]) : NodeRec{-1, -1};
  }
  for (int steps = 0; steps < cap; ++steps) {
    bool any = false;
#pragma unroll
    for (int u = 0; u < kPredU; ++u) any |= nr[u].split >= 0;
    if (!any) break;
    const bool in_top = top && steps + 1 < kTopLv;
#pragma unroll
    for (int u = 0; u < kPredU; ++u) {
      if (nr[u].split >= 0) {
        const int feat = nr[u].split >> 8;
        int bin = xr[feat];
        if (kRecord) {
          if (feat == f) hit |= 1u << u;
        } else if (feat == f) {
          bin = sub;
        }
        const int b = bin > (nr[u].split & 255) ? 1 : 0;
        leaf[u] = nr[u].left + b;
        if (in_top) {
          sl[u] = 2 * sl[u] + 1 + b;
          nr[u] = top[u * kTopSlots + sl[u]];
        } else {
          nr[u] = nodes[leaf[u]];
        }
      }
    }
  }
}

// the substituted bins of one row for repeats [k0, k0 + KC): feature f of row rows[perm[k][i]]
template <int KC>
__device__ __forceinline__ void perm_subs(const PredictArgs& a, const PermTail& e, int64_t i, int64_t nr, int f, int own,
                                          bool live, int k0, int (&sub)[KC]) {
#pragma unroll
  for (int kk = 0; kk < KC; ++kk) {
    sub[kk] = own;
    if (live && f >= 0 && k0 + kk < e.K) {
      const int32_t j = e.perm[(int64_t)(k0 + kk) * nr + i];
      sub[kk] = (GPTR(const uint8_t, a.Xb))[(int64_t)(GPTR(const int32_t, a.rows))[j] * a.ld + f];
    }
  }
}

// block sum of one value per thread for each repeat of a chunk, in a fixed order (lanes by
// xor-shuffle, then the four waves ascending) -> part[block][f][k]
template <class T, int KC>
__device__ __forceinline__ void perm_block_sums(const PermTail& e, T (&v)[KC], T (*red)[KC], int k0) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int kk = 0; kk < KC; ++kk) {
    T s = v[kk];
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[w][kk] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < KC && k0 + (int)threadIdx.x < e.K) {
    const int kk = threadIdx.x;
    ((T*)e.part)[((int64_t)blockIdx.x * e.F + blockIdx.y) * e.K + k0 + kk] =
        red[0][kk] + red[1][kk] + red[2][kk] + red[3][kk];
  }
  __syncthreads();   // red is free for the next chunk
}

__device__ __forceinline__ void perm_count_walked(const PermTail& e, int nw) {
  if (!e.walked) return;
  for (int off = 32; off >= 1; off >>= 1) nw += __shfl_xor(nw, off);
  if ((threadIdx.x & 63) == 0 && nw) atomicAdd(e.walked + blockIdx.y, (unsigned long long)nw);
}

template <int MAXC, int kPredU>
__global__ __launch_bounds__(256) void k_perm_cls(PredictArgs a, PermTail e) {
  constexpr int KC = perm_chunk(MAXC);
  extern __shared__ __attribute__((aligned(16))) uint8_t xs_lds[];
  __shared__ long long red[4][KC];
  const int32_t* toff = GPTR(const int32_t, a.fit_tree_off);
  const int64_t* roff = GPTR(const int64_t, a.fit_row_off);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = roff[0], nr = roff[1] - r0;
  if ((int64_t)blockIdx.x * 256 >= nr) return;
  // every thread of a block with rows stays to the end (block-wide table loads and sums); a
  // thread past the rows walks nothing and adds nothing
  const bool live = i < nr;
  NodeRec* top = a.toptab ? (NodeRec*)(xs_lds + top_lds_off(a)) : nullptr;
  const uint8_t* xr = a.lds_pitch ? stage_rows(a, xs_lds, r0, nr) : nullptr;
  const int32_t row = (GPTR(const int32_t, a.rows))[r0 + (live ? i : 0)];
  if (!a.lds_pitch) xr = GPTR(const uint8_t, a.Xb) + (int64_t)row * a.ld;
  const int f = e.features[blockIdx.y];
  const int own = f >= 0 ? xr[f] : 0;
  const int32_t label = ((const int32_t*)e.y)[row];
  const int C = (int)a.n_classes;
  const NodeRec* nodes = GPTR(const NodeRec, a.nodes);
  const double* val = GPTR(const double, a.node_val);
  const int tend = toff[1];
  int nw = 0;
  for (int k0 = 0; k0 < e.K; k0 += KC) {
    int sub[KC];
    perm_subs<KC>(a, e, i, nr, f, own, live, k0, sub);
    float p[KC][MAXC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
#pragma unroll
      for (int k = 0; k < MAXC; ++k) p[kk][k] = 0.f;
    for (int t = toff[0]; t < tend; t += kPredU) {
      int base[kPredU];
      const int u_all = min(kPredU, tend - t), u_n = live ? u_all : 0;
      if (top) load_top<kPredU>(a, top, t, u_all);
      uint32_t hit = 0;
      leaves_perm_u<kPredU, true>(nodes, xr, t, u_n, base, e.cap, top, ~0u, f, 0, hit);
      if (e.no_skip) hit = (1u << u_n) - 1u;
      // narrow class counts: the baseline leaves' fractions are computed once per group and
      // added as they are for every repeat that keeps the leaf (the same floats, so the same sums)
      constexpr bool kKeep = MAXC <= 4;
      float bc[kKeep ? kPredU : 1][MAXC];
      uint32_t bok = 0;
      if (kKeep) {
#pragma unroll
        for (int u = 0; u < kPredU; ++u) {
          if (u >= u_n) continue;
          const double* v = val + (int64_t)base[u] * a.VC;
          double W = 0.0;
#pragma unroll
          for (int k = 0; k < MAXC; ++k)
            if (k < C) W += v[k];
          if (W > 0.0) {
            const double inv = 1.0 / W;
            bok |= 1u << u;
#pragma unroll
            for (int k = 0; k < MAXC; ++k)
              if (k < C) bc[kKeep ? u : 0][k] = (float)(v[k] * inv);
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < KC; ++kk) {
        if (k0 + kk >= e.K) break;
        int lk[kPredU];
        const uint32_t m = (sub[kk] != own || e.no_skip) ? hit : 0u;
        if (m) {
          uint32_t none = 0;
          leaves_perm_u<kPredU, false>(nodes, xr, t, u_n, lk, e.cap, top, m, f, sub[kk], none);
          nw += __popc(m);
        }
        // accumulate in tree order (bit-identical to the predict kernels and the host twin)
#pragma unroll
        for (int u = 0; u < kPredU; ++u) {   // no break: a constant trip count keeps lk / base in registers
          if (u >= u_n) continue;
          if (kKeep && !((m >> u) & 1u)) {
            if ((bok >> u) & 1u) {
#pragma unroll
              for (int k = 0; k < MAXC; ++k)
                if (k < C) p[kk][k] += bc[kKeep ? u : 0][k];
            }
            continue;
          }
          const double* v = val + (int64_t)(((m >> u) & 1u) ? lk[u] : base[u]) * a.VC;
          double W = 0.0;
#pragma unroll
          for (int k = 0; k < MAXC; ++k)
            if (k < C) W += v[k];
          if (W > 0.0) {
            const double inv = 1.0 / W;
#pragma unroll
            for (int k = 0; k < MAXC; ++k)
              if (k < C) p[kk][k] += (float)(v[k] * inv);
          }
        }
      }
    }
    long long hitc[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
      int best = 0;
      float bv = p[kk][0];
#pragma unroll
      for (int k = 1; k < MAXC; ++k)
        if (k < C && p[kk][k] > bv) { bv = p[kk][k]; best = k; }
      const bool on = live && k0 + kk < e.K;
      hitc[kk] = on && best == label ? 1 : 0;
      if (on && e.pred) ((int32_t*)e.pred)[((int64_t)blockIdx.y * e.K + k0 + kk) * nr + i] = best;
    }
    perm_block_sums<long long, KC>(e, hitc, red, k0);
  }
  perm_count_walked(e, nw);
}

template <int kPredU>
__global__ __launch_bounds__(256) void k_perm_reg(PredictArgs a, PermTail e) {
  constexpr int KC = 8;
  extern __shared__ __attribute__((aligned(16))) uint8_t xs_lds[];
  __shared__ double red[4][KC];
  const int32_t* toff = GPTR(const int32_t, a.fit_tree_off);
  const int64_t* roff = GPTR(const int64_t, a.fit_row_off);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = roff[0], nr = roff[1] - r0;
  if ((int64_t)blockIdx.x * 256 >= nr) return;
  const bool live = i < nr;   // as in k_perm_cls: every thread stays
  NodeRec* top = a.toptab ? (NodeRec*)(xs_lds + top_lds_off(a)) : nullptr;
  const uint8_t* xr = a.lds_pitch ? stage_rows(a, xs_lds, r0, nr) : nullptr;
  const int32_t row = (GPTR(const int32_t, a.rows))[r0 + (live ? i : 0)];
  if (!a.lds_pitch) xr = GPTR(const uint8_t, a.Xb) + (int64_t)row * a.ld;
  const int f = e.features[blockIdx.y];
  const int own = f >= 0 ? xr[f] : 0;
  const double y = ((const float*)e.y)[row];
  const NodeRec* nodes = GPTR(const NodeRec, a.nodes);
  const double* val = GPTR(const double, a.node_val);
  const int tend = toff[1];
  int nw = 0;
  for (int k0 = 0; k0 < e.K; k0 += KC) {
    int sub[KC];
    perm_subs<KC>(a, e, i, nr, f, own, live, k0, sub);
    double acc[KC];
    int nt[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) { acc[kk] = 0.0; nt[kk] = 0; }
    for (int t = toff[0]; t < tend; t += kPredU) {
      int base[kPredU];
      const int u_all = min(kPredU, tend - t), u_n = live ? u_all : 0;
      if (top) load_top<kPredU>(a, top, t, u_all);
      uint32_t hit = 0;
      leaves_perm_u<kPredU, true>(nodes, xr, t, u_n, base, e.cap, top, ~0u, f, 0, hit);
      if (e.no_skip) hit = (1u << u_n) - 1u;
      // the baseline leaves' means, computed once per group (as k_perm_cls keeps its fractions)
      double bq[kPredU];
      uint32_t bok = 0;
#pragma unroll
      for (int u = 0; u < kPredU; ++u) {
        if (u >= u_n) continue;
        const double* v = val + (int64_t)base[u] * a.VC;
        if (v[0] > 0.0) { bq[u] = v[1] / v[0]; bok |= 1u << u; }
      }
#pragma unroll
      for (int kk = 0; kk < KC; ++kk) {
        if (k0 + kk >= e.K) break;
        int lk[kPredU];
        const uint32_t m = (sub[kk] != own || e.no_skip) ? hit : 0u;
        if (m) {
          uint32_t none = 0;
          leaves_perm_u<kPredU, false>(nodes, xr, t, u_n, lk, e.cap, top, m, f, sub[kk], none);
          nw += __popc(m);
        }
#pragma unroll
        for (int u = 0; u < kPredU; ++u) {
          if (u >= u_n) continue;
          if (!((m >> u) & 1u)) {
            if ((bok >> u) & 1u) { acc[kk] += bq[u]; ++nt[kk]; }
            continue;
          }
          const double* v = val + (int64_t)(((m >> u) & 1u) ? lk[u] : base[u]) * a.VC;
          if (v[0] > 0.0) { acc[kk] += v[1] / v[0]; ++nt[kk]; }
        }
      }
    }
    double se[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
      const float pr = nt[kk] ? (float)(acc[kk] / nt[kk]) : 0.f;
      const bool on = live && k0 + kk < e.K;
      const double er = (double)pr - y;
      se[kk] = on ? er * er : 0.0;
      if (on && e.pred) ((float*)e.pred)[((int64_t)blockIdx.y * e.K + k0 + kk) * nr + i] = pr;
    }
    perm_block_sums<double, KC>(e, se, red, k0);
  }
  perm_count_walked(e, nw);
}

// out[f][k] = the block partials added in block order (one thread per (f, k): the same sum every run)
template <class T>
__global__ __launch_bounds__(256) void k_perm_reduce(const T* __restrict__ part, T* __restrict__ out, int64_t blocks,
                                                     int64_t FK) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= FK) return;
  T s = 0;
  for (int64_t b = 0; b < blocks; ++b) s += part[b * FK + j];
  out[j] = s;
}

// ---- one-way partial dependence of a kept fit over its training rows -------------------------
// For feature f (grid.y, a slot of features[]) and grid point g, every row is predicted from its
// own bins except that feature f's bin is sub_bins[slot][g] -- the same for every row, so it is
// read once per block, not gathered -- and the values (k_predict_cls's out_proba / k_predict_reg's
// out_pred, bit for bit) are summed over the rows.  The block shape and the hit-skip are the
// permutation kernels'; the skip test is an interval: the baseline walk of a group of U trees
// also records the bins [lo, hi] of feature f over which no slot of the group changes its leaf
// (lo: the largest split + 1 among the f-nodes where the row went right, hi: the smallest split
// among those where it went left; the row's own bin lies inside), and a grid point whose bin is
// inside adds the baseline leaves' values without walking.  Every slot adds the same value in
// tree order whether it was walked again or not.  ../runtime/forest_pd_cpu.cpp is the host twin.
struct PdArgs {
  int64_t Xb, ld, d;
  int64_t nodes, node_val, VC, is_reg, n_classes;
  int64_t fit_tree_off;  // int32[2] device: the fit's pool trees [t0, t1)
  int64_t fit_row_off;   // int64[2] device: {0, n_rows}
  int64_t t0, t1;
  int64_t rows, n_rows;  // int32[n_rows]: dataset row ids
  int64_t depth_cap;     // <= 0: whole trees
  int64_t features, F;   // int32 [F]: feature ids, or -1 (the baseline slot)
  int64_t sub_bins, Gmax;   // uint8 [F][Gmax]: the bins to substitute
  int64_t n_grid;        // int32 [F]: slot s uses sub_bins[s][0 .. n_grid[s])
  int64_t n_targets, c0; // the values summed: classes [c0, c0 + n_targets) (regression: 1, 0)
  int64_t part, f_chunk; // scratch double [blocks][f_chunk][Gmax][n_targets]: the slots are launched
                         // f_chunk at a time, so the partials stay within what the caller allows
  int64_t out;           // double [F][Gmax][n_targets]: the block partials summed in block order
  int64_t out_rows;      // optional float [F][Gmax][n_rows][n_targets]: the per-row values
  int64_t out_walked;    // optional uint64 [F]: (row, tree, grid point) slots walked a second time
  int64_t toptab;        // NodeRec[t1][kTopSlots] scratch or 0
  int64_t no_skip;       // A/B: walk every tree again for every grid point
};

struct PdTail {   // what the partial-dependence kernels take besides the predict block
  const int32_t* features;
  const uint8_t* sub;
  const int32_t* n_grid;
  double* part;
  float* rows_out;
  unsigned long long* walked;
  int Gmax, Fc, f0, NT, c0, cap, no_skip;
};

// leaves_perm_u's recording walk, which also narrows [lo, hi] at every visited node on feature f
template <int kPredU>
__device__ __forceinline__ void leaves_pd_u(const NodeRec* __restrict__ nodes, const uint8_t* __restrict__ xr, int t0,
                                            int u_n, int (&leaf)[kPredU], int cap, const NodeRec* top, int f,
                                            uint32_t& hit, int& lo, int& hi) {
  NodeRec nr[kPredU];
  int sl[kPredU];
#pragma unroll
  for (int u = 0; u < kPredU; ++u) {
    leaf[u] = t0 + u;
    sl[u] = 0;
    nr[u] = u < u_n ? (top ? top[u * kTopSlots] : nodes[leaf[u]]) : NodeRec{-1, -1};
  }
  for (int steps = 0; steps < cap; ++steps) {
    bool any = false;
#pragma unroll
    for (int u = 0; u < kPredU; ++u) any |= nr[u].split >= 0;
    if (!any) break;
    const bool in_top = top && steps + 1 < kTopLv;
#pragma unroll
    for (int u = 0; u < kPredU; ++u) {
      if (nr[u].split >= 0) {
        const int feat = nr[u].split >> 8, thr = nr[u].split & 255;
        const int b = xr[feat] > thr ? 1 : 0;
        if (feat == f) {
          hit |= 1u << u;
          lo = b ? max(lo, thr + 1) : lo;
          hi = b ? hi : min(hi, thr);
        }
        leaf[u] = nr[u].left + b;
        if (in_top) {
          sl[u] = 2 * sl[u] + 1 + b;
          nr[u] = top[u * kTopSlots + sl[u]];
        } else {
          nr[u] = nodes[leaf[u]];
        }
      }
    }
  }
}

// block sum of one double per thread in a fixed order: lanes by xor-shuffle, lane 0 of wave w
// leaves it in red[w * stride]; the caller adds the four waves ascending after a barrier
__device__ __forceinline__ void pd_wave_sum(double s, double* red, int stride) {
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * stride] = s;
}

__device__ __forceinline__ void pd_count_walked(const PdTail& e, int fs, int nw) {
  if (!e.walked) return;
  for (int off = 32; off >= 1; off >>= 1) nw += __shfl_xor(nw, off);
  if ((threadIdx.x & 63) == 0 && nw) atomicAdd(e.walked + fs, (unsigned long long)nw);
}

template <int MAXC, int kPredU>
__global__ __launch_bounds__(256) void k_pd_cls(PredictArgs a, PdTail e) {
  constexpr int KC = perm_chunk(MAXC);
  extern __shared__ __attribute__((aligned(16))) uint8_t xs_lds[];
  __shared__ double red[4][KC * MAXC];
  const int32_t* toff = GPTR(const int32_t, a.fit_tree_off);
  const int64_t* roff = GPTR(const int64_t, a.fit_row_off);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = roff[0], nr = roff[1] - r0;
  if ((int64_t)blockIdx.x * 256 >= nr) return;
  // every thread of a block with rows stays to the end (block-wide table loads and sums); a
  // thread past the rows walks nothing and adds nothing
  const bool live = i < nr;
  NodeRec* top = a.toptab ? (NodeRec*)(xs_lds + top_lds_off(a)) : nullptr;
  const uint8_t* xr = a.lds_pitch ? stage_rows(a, xs_lds, r0, nr) : nullptr;
  const int32_t row = (GPTR(const int32_t, a.rows))[r0 + (live ? i : 0)];
  if (!a.lds_pitch) xr = GPTR(const uint8_t, a.Xb) + (int64_t)row * a.ld;
  const int fs = e.f0 + (int)blockIdx.y;
  const int f = e.features[fs];
  const int ng = e.n_grid[fs];
  const uint8_t* subs = e.sub + (int64_t)fs * e.Gmax;
  const int C = (int)a.n_classes;
  const NodeRec* nodes = GPTR(const NodeRec, a.nodes);
  const double* val = GPTR(const double, a.node_val);
  const int tend = toff[1];
  const float ntf = (float)(tend - toff[0]);
  int nw = 0;
  for (int g0 = 0; g0 < ng; g0 += KC) {
    int sub[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) sub[kk] = g0 + kk < ng ? subs[g0 + kk] : 0;   // uniform over the block
    float p[KC][MAXC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
#pragma unroll
      for (int k = 0; k < MAXC; ++k) p[kk][k] = 0.f;
    for (int t = toff[0]; t < tend; t += kPredU) {
      int base[kPredU];
      const int u_all = min(kPredU, tend - t), u_n = live ? u_all : 0;
      if (top) load_top<kPredU>(a, top, t, u_all);
      uint32_t hit = 0;
      int lo = 0, hi = 255;
      leaves_pd_u<kPredU>(nodes, xr, t, u_n, base, e.cap, top, f, hit, lo, hi);
      if (e.no_skip) hit = (1u << u_n) - 1u;
      // narrow class counts: the baseline leaves' fractions are computed once per group and added
      // as they are for every grid point that keeps the leaf (the same floats, so the same sums)
      constexpr bool kKeep = MAXC <= 4;
      float bc[kKeep ? kPredU : 1][MAXC];
      uint32_t bok = 0;
      if (kKeep) {
#pragma unroll
        for (int u = 0; u < kPredU; ++u) {
          if (u >= u_n) continue;
          const double* v = val + (int64_t)base[u] * a.VC;
          double W = 0.0;
#pragma unroll
          for (int k = 0; k < MAXC; ++k)
            if (k < C) W += v[k];
          if (W > 0.0) {
            const double inv = 1.0 / W;
            bok |= 1u << u;
#pragma unroll
            for (int k = 0; k < MAXC; ++k)
              if (k < C) bc[kKeep ? u : 0][k] = (float)(v[k] * inv);
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < KC; ++kk) {
        if (g0 + kk >= ng) break;
        int lk[kPredU];
#ifdef DML_PD_PLAIN_SKIP   // A/B build: the permutation kernels' test, the row's own bin alone
        const bool inside = sub[kk] == (f >= 0 ? xr[f] : 0);
#else
        const bool inside = sub[kk] >= lo && sub[kk] <= hi;
#endif
        const uint32_t m = (!inside || e.no_skip) ? hit : 0u;
        if (m) {
          uint32_t none = 0;
          leaves_perm_u<kPredU, false>(nodes, xr, t, u_n, lk, e.cap, top, m, f, sub[kk], none);
          nw += __popc(m);
        }
        // accumulate in tree order (bit-identical to the predict kernels and the host twin)
#pragma unroll
        for (int u = 0; u < kPredU; ++u) {   // no break: a constant trip count keeps lk / base in registers
          if (u >= u_n) continue;
          if (kKeep && !((m >> u) & 1u)) {
            if ((bok >> u) & 1u) {
#pragma unroll
              for (int k = 0; k < MAXC; ++k)
                if (k < C) p[kk][k] += bc[kKeep ? u : 0][k];
            }
            continue;
          }
          const double* v = val + (int64_t)(((m >> u) & 1u) ? lk[u] : base[u]) * a.VC;
          double W = 0.0;
#pragma unroll
          for (int k = 0; k < MAXC; ++k)
            if (k < C) W += v[k];
          if (W > 0.0) {
            const double inv = 1.0 / W;
#pragma unroll
            for (int k = 0; k < MAXC; ++k)
              if (k < C) p[kk][k] += (float)(v[k] * inv);
          }
        }
      }
    }
    // the values of this chunk's grid points: k_predict_cls's out_proba for classes [c0, c0 + NT)
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
      const bool on = live && g0 + kk < ng;
#pragma unroll
      for (int k = 0; k < MAXC; ++k) {
        if (k < e.c0 || k >= e.c0 + e.NT) continue;   // uniform
        const float q = p[kk][k] / ntf;
        if (on && e.rows_out)
          e.rows_out[(((int64_t)fs * e.Gmax + g0 + kk) * nr + i) * e.NT + (k - e.c0)] = q;
        pd_wave_sum(on ? (double)q : 0.0, &red[0][kk * MAXC + k], KC * MAXC);
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < KC * MAXC) {
      const int j = threadIdx.x, kk = j / MAXC, k = j - kk * MAXC;
      if (g0 + kk < ng && k >= e.c0 && k < e.c0 + e.NT)
        e.part[((((int64_t)blockIdx.x * e.Fc + blockIdx.y) * e.Gmax) + g0 + kk) * e.NT + (k - e.c0)] =
            red[0][j] + red[1][j] + red[2][j] + red[3][j];
    }
    __syncthreads();   // red is free for the next chunk
  }
  pd_count_walked(e, fs, nw);
}

template <int kPredU>
__global__ __launch_bounds__(256) void k_pd_reg(PredictArgs a, PdTail e) {
  constexpr int KC = 8;
  extern __shared__ __attribute__((aligned(16))) uint8_t xs_lds[];
  __shared__ double red[4][KC];
  const int32_t* toff = GPTR(const int32_t, a.fit_tree_off);
  const int64_t* roff = GPTR(const int64_t, a.fit_row_off);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r0 = roff[0], nr = roff[1] - r0;
  if ((int64_t)blockIdx.x * 256 >= nr) return;
  const bool live = i < nr;   // as in k_pd_cls: every thread stays
  NodeRec* top = a.toptab ? (NodeRec*)(xs_lds + top_lds_off(a)) : nullptr;
  const uint8_t* xr = a.lds_pitch ? stage_rows(a, xs_lds, r0, nr) : nullptr;
  const int32_t row = (GPTR(const int32_t, a.rows))[r0 + (live ? i : 0)];
  if (!a.lds_pitch) xr = GPTR(const uint8_t, a.Xb) + (int64_t)row * a.ld;
  const int fs = e.f0 + (int)blockIdx.y;
  const int f = e.features[fs];
  const int ng = e.n_grid[fs];
  const uint8_t* subs = e.sub + (int64_t)fs * e.Gmax;
  const NodeRec* nodes = GPTR(const NodeRec, a.nodes);
  const double* val = GPTR(const double, a.node_val);
  const int tend = toff[1];
  int nw = 0;
  for (int g0 = 0; g0 < ng; g0 += KC) {
    int sub[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) sub[kk] = g0 + kk < ng ? subs[g0 + kk] : 0;   // uniform over the block
    double acc[KC];
    int nt[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) { acc[kk] = 0.0; nt[kk] = 0; }
    for (int t = toff[0]; t < tend; t += kPredU) {
      int base[kPredU];
      const int u_all = min(kPredU, tend - t), u_n = live ? u_all : 0;
      if (top) load_top<kPredU>(a, top, t, u_all);
      uint32_t hit = 0;
      int lo = 0, hi = 255;
      leaves_pd_u<kPredU>(nodes, xr, t, u_n, base, e.cap, top, f, hit, lo, hi);
      if (e.no_skip) hit = (1u << u_n) - 1u;
      // the baseline leaves' means, computed once per group (as k_pd_cls keeps its fractions)
      double bq[kPredU];
      uint32_t bok = 0;
#pragma unroll
      for (int u = 0; u < kPredU; ++u) {
        if (u >= u_n) continue;
        const double* v = val + (int64_t)base[u] * a.VC;
        if (v[0] > 0.0) { bq[u] = v[1] / v[0]; bok |= 1u << u; }
      }
#pragma unroll
      for (int kk = 0; kk < KC; ++kk) {
        if (g0 + kk >= ng) break;
        int lk[kPredU];
#ifdef DML_PD_PLAIN_SKIP   // A/B build: the permutation kernels' test, the row's own bin alone
        const bool inside = sub[kk] == (f >= 0 ? xr[f] : 0);
#else
        const bool inside = sub[kk] >= lo && sub[kk] <= hi;
#endif
        const uint32_t m = (!inside || e.no_skip) ? hit : 0u;
        if (m) {
          uint32_t none = 0;
          leaves_perm_u<kPredU, false>(nodes, xr, t, u_n, lk, e.cap, top, m, f, sub[kk], none);
          nw += __popc(m);
        }
#pragma unroll
        for (int u = 0; u < kPredU; ++u) {
          if (u >= u_n) continue;
          if (!((m >> u) & 1u)) {
            if ((bok >> u) & 1u) { acc[kk] += bq[u]; ++nt[kk]; }
            continue;
          }
          const double* v = val + (int64_t)lk[u] * a.VC;
          if (v[0] > 0.0) { acc[kk] += v[1] / v[0]; ++nt[kk]; }
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
      const float q = nt[kk] ? (float)(acc[kk] / nt[kk]) : 0.f;
      const bool on = live && g0 + kk < ng;
      if (on && e.rows_out) e.rows_out[((int64_t)fs * e.Gmax + g0 + kk) * nr + i] = q;
      pd_wave_sum(on ? (double)q : 0.0, &red[0][kk], KC);
    }
    __syncthreads();
    if ((int)threadIdx.x < KC && g0 + (int)threadIdx.x < ng) {
      const int kk = threadIdx.x;
      e.part[(((int64_t)blockIdx.x * e.Fc + blockIdx.y) * e.Gmax) + g0 + kk] =
          red[0][kk] + red[1][kk] + red[2][kk] + red[3][kk];
    }
    __syncthreads();   // red is free for the next chunk
  }
  pd_count_walked(e, fs, nw);
}

// out[f0 + s][g][k] = the block partials of slot s added in block order (one thread per entry:
// the same sum every run); entries past a slot's n_grid are left as they are
__global__ __launch_bounds__(256) void k_pd_reduce(const double* __restrict__ part, double* __restrict__ out,
                                                   const int32_t* __restrict__ n_grid, int64_t blocks, int Fc, int f0,
                                                   int Gmax, int NT) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, FGN = (int64_t)Fc * Gmax * NT;
  if (j >= FGN) return;
  const int s = (int)(j / ((int64_t)Gmax * NT)), g = (int)(j / NT) % Gmax;
  if (g >= n_grid[f0 + s]) return;
  double acc = 0.0;
  for (int64_t b = 0; b < blocks; ++b) acc += part[b * FGN + j];
  out[(int64_t)f0 * Gmax * NT + j] = acc;
}

// per-fit score statistics: out[f] = {match_count or SSE, sum y, sum y^2, n}
struct ScoreArgs {
  int64_t rows;        // int32[] row ids
  int64_t fit_row_off; // int64[F+1]
  int64_t pred;        // int32 (cls) / float (reg)
  int64_t ycls, yreg, is_reg;
  int64_t out;         // double [F][4]
  int64_t F;
};

__global__ __launch_bounds__(256) void k_scores(ScoreArgs a) {
  const int f = blockIdx.x;
  const int64_t* roff = GPTR(const int64_t, a.fit_row_off);
  const int64_t r0 = roff[f], r1 = roff[f + 1];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const int32_t* rows = GPTR(const int32_t, a.rows);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) {
    const int32_t row = rows[i];
    if (a.is_reg) {
      const double y = (GPTR(const float, a.yreg))[row];
      const double e = (double)(GPTR(const float, a.pred))[i] - y;
      s0 += e * e; s1 += y; s2 += y * y;
    } else {
      s0 += (GPTR(const int32_t, a.pred))[i] == (GPTR(const int32_t, a.ycls))[row] ? 1.0 : 0.0;
    }
  }
  __shared__ double red[3][4];
  for (int off = 32; off >= 1; off >>= 1) {
    s0 += __shfl_xor(s0, off); s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = s0; red[1][w] = s1; red[2][w] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = GPTR(double, a.out) + 4 * f;
    o[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    o[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    o[2] = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    o[3] = (double)(r1 - r0);
  }
}

// leaf index of every row for every tree (boosting line search / raw-score update):
// leaf[t * n + row]; trees t = t0 .. t0+T-1 have their roots at node t.
__global__ __launch_bounds__(256) void k_apply(const uint8_t* __restrict__ Xb, int64_t ld, int64_t n,
                                               const NodeRec* __restrict__ nodes, int32_t t0,
                                               int32_t* __restrict__ leaf) {
  const int t = blockIdx.y;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const uint8_t* xr = Xb + row * ld;
  int node = t0 + t;
  NodeRec nr = nodes[node];
  for (int steps = 0; nr.split >= 0 && steps < 1 << 20; ++steps) {
    node = nr.left + (xr[nr.split >> 8] > (nr.split & 255) ? 1 : 0);
    nr = nodes[node];
  }
  leaf[(int64_t)t * n + row] = node;
}

// ---- sklearn-style split thresholds -------------------------------------------------
// A histogram split "bin <= b_lo" equals sklearn's "x <= (x_left_max + x_right_min) / 2"
// on the training rows; held-out rows between the two values are routed like sklearn
// only if the threshold sits at the midpoint.  For features whose bins are exact values
// (<= 256 distinct), pass 1 finds b_hi = min bin among each internal node's right-going
// in-bag training rows, pass 2 moves the split bin to the last bin value <= midpoint.
__global__ __launch_bounds__(256) void k_refine_hi(const uint8_t* __restrict__ Xb, int64_t ld, int64_t n,
                                                   const NodeRec* __restrict__ nodes,
                                                   const TreeSpec* __restrict__ specs,
                                                   const uint8_t* __restrict__ roles, uint32_t* hi) {
  const int t = blockIdx.y;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const TreeSpec& s = specs[t];
  if (roles[(int64_t)s.split * n + row] != 1 || boot_weight(s, (uint32_t)row) == 0) return;
  const uint8_t* xr = Xb + row * ld;
  int node = t;
  NodeRec nr = nodes[node];
  for (int steps = 0; nr.split >= 0 && steps < 1 << 20; ++steps) {
    const uint32_t b = xr[nr.split >> 8];
    if (b > (uint32_t)(nr.split & 255)) {
      if (b < hi[node]) atomicMin(&hi[node], b);
      node = nr.left + 1;
    } else {
      node = nr.left;
    }
    nr = nodes[node];
  }
}

__global__ __launch_bounds__(256) void k_refine_split(NodeRec* nodes, int64_t P, int64_t d, const uint32_t* __restrict__ hi,
                                                      const float* __restrict__ vals, const uint8_t* __restrict__ exact) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const NodeRec nr = nodes[i];
  if (nr.split < 0 || (nr.split >> 8) >= d) return;
  const int f = nr.split >> 8, blo = nr.split & 255;
  const uint32_t bhi = hi[i];
  if (!exact[f] || bhi > 255u || (int)bhi <= blo) return;
  const float* v = vals + (int64_t)f * 256;
  double m = (double)v[blo] / 2.0 + (double)v[bhi] / 2.0;
  if (m == (double)v[bhi] || !(m == m)) m = (double)v[blo];
  int b = blo;
  while (b + 1 < (int)bhi && (double)v[b + 1] <= m) ++b;
  nodes[i].split = f * 256 + b;
}

// U trees walked in lock-step per thread (memory-level parallelism of the dependent
// node-load chains); DML_PRED_U=4/16 select the other widths (A/B)
// LDS row stride for staged predict rows: whole dwords, odd dword count (conflict-free
// when the lanes of a wave read the same feature), within the row pitch; 0 disables
static int64_t predict_pitch(const PredictArgs* a) {
  static const bool off = getenv("DML_PRED_NO_STAGE") != nullptr;
  int64_t w = (a->d + 3) / 4;
  if ((w & 1) == 0) ++w;
  if (off || a->d <= 0 || 4 * ((a->d + 3) / 4) > a->ld || (a->ld & 3) || 256 * 4 * w > 64 * 1024) return 0;
  return 4 * w;
}

template <int U>
static int launch_predict(PredictArgs* a, hipStream_t st) {
  dim3 grid((unsigned)((a->max_rows + 255) / 256), (unsigned)a->F);
  a->lds_pitch = predict_pitch(a);
  size_t lds = (size_t)a->lds_pitch * 256;
  static const bool top_off = getenv("DML_PRED_NO_TOP") != nullptr;
  PredictArgs b = *a;   // the launch's copy: the top table only when it fits the LDS
  const size_t lds_top = ((lds + 15) & ~(size_t)15) + (size_t)U * kTopSlots * sizeof(NodeRec);
  if (top_off || lds_top > 64 * 1024 || a->max_trees <= 0) b.toptab = 0;
  if (b.toptab) {
    k_top_fill<<<dim3((unsigned)((b.max_trees + 3) / 4), (unsigned)b.F), 256, 0, st>>>(b);
    lds = lds_top;
  }
  a = &b;
  if (a->is_reg) {
    k_predict_reg<U><<<grid, 256, lds, st>>>(*a);
  } else {
    const int C = (int)a->n_classes;
    if (C <= 2) k_predict_cls<2, U><<<grid, 256, lds, st>>>(*a);
    else if (C <= 4) k_predict_cls<4, U><<<grid, 256, lds, st>>>(*a);
    else if (C <= 8) k_predict_cls<8, U><<<grid, 256, lds, st>>>(*a);
    else if (C <= 16) k_predict_cls<16, U><<<grid, 256, lds, st>>>(*a);
    else if (C <= 32) k_predict_cls<32, U><<<grid, 256, lds, st>>>(*a);
    else if (C <= 64) k_predict_cls<64, U><<<grid, 256, lds, st>>>(*a);
    else return 5;
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// one launch over the kept fit's training rows: launch_predict's LDS layout (staged rows, top
// table of the U trees being walked) with F = 1
template <int U>
static int launch_oob(const OobArgs* o, hipStream_t st) {
  PredictArgs a{};
  a.Xb = o->Xb; a.ld = o->ld; a.d = o->d;
  a.nodes = o->nodes; a.node_val = o->node_val; a.VC = o->VC; a.is_reg = o->is_reg; a.n_classes = o->n_classes;
  a.fit_tree_off = o->fit_tree_off; a.fit_row_off = o->fit_row_off; a.rows = o->rows;
  a.out_pred = o->is_reg ? o->out : o->out_pred;
  a.out_proba = o->is_reg ? 0 : o->out;
  a.F = 1; a.max_rows = o->n_rows; a.max_trees = o->t1 - o->t0;
  a.toptab = o->toptab;
  a.lds_pitch = predict_pitch(&a);
  size_t lds = (size_t)a.lds_pitch * 256;
  static const bool top_off = getenv("DML_PRED_NO_TOP") != nullptr;
  const size_t lds_top = ((lds + 15) & ~(size_t)15) + (size_t)U * kTopSlots * sizeof(NodeRec);
  if (top_off || lds_top > 64 * 1024) a.toptab = 0;
  if (a.toptab) {
    k_top_fill<<<dim3((unsigned)((a.max_trees + 3) / 4), 1), 256, 0, st>>>(a);
    lds = lds_top;
  }
  const OobTail e{GPTR(const TreeSpec, o->specs), GPTR(int32_t, o->out_cnt),
                  o->depth_cap > 0 ? (int)o->depth_cap : 1 << 20};
  const dim3 grid((unsigned)((o->n_rows + 255) / 256), 1);
  if (o->is_reg) {
    k_oob_reg<U><<<grid, 256, lds, st>>>(a, e);
  } else {
    const int C = (int)o->n_classes;
    if (C <= 2) k_oob_cls<2, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 4) k_oob_cls<4, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 8) k_oob_cls<8, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 16) k_oob_cls<16, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 32) k_oob_cls<32, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 64) k_oob_cls<64, U><<<grid, 256, lds, st>>>(a, e);
    else return 5;
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// launch_oob's LDS layout with grid.y = feature; the kernels' own static LDS (stage_rows' row
// list and the block sums) counts against the 64 KiB the dynamic part may fill
template <int U>
static int launch_perm(const PermArgs* o, hipStream_t st) {
  PredictArgs a{};
  a.Xb = o->Xb; a.ld = o->ld; a.d = o->d;
  a.nodes = o->nodes; a.node_val = o->node_val; a.VC = o->VC; a.is_reg = o->is_reg; a.n_classes = o->n_classes;
  a.fit_tree_off = o->fit_tree_off; a.fit_row_off = o->fit_row_off; a.rows = o->rows;
  a.F = 1; a.max_rows = o->n_rows; a.max_trees = o->t1 - o->t0;
  a.toptab = o->toptab;
  constexpr size_t kStatic = 256 * sizeof(int32_t) + 4 * 8 * sizeof(double);
  a.lds_pitch = predict_pitch(&a);
  if ((size_t)a.lds_pitch * 256 + kStatic > 64 * 1024) a.lds_pitch = 0;
  size_t lds = (size_t)a.lds_pitch * 256;
  static const bool top_off = getenv("DML_PRED_NO_TOP") != nullptr;
  const size_t lds_top = ((lds + 15) & ~(size_t)15) + (size_t)U * kTopSlots * sizeof(NodeRec);
  if (top_off || lds_top + kStatic > 64 * 1024) a.toptab = 0;
  if (a.toptab) {
    k_top_fill<<<dim3((unsigned)((a.max_trees + 3) / 4), 1), 256, 0, st>>>(a);
    lds = lds_top;
  }
  static const bool no_skip = getenv("DML_PERM_NO_SKIP") != nullptr;
  const PermTail e{GPTR(const int32_t, o->perm), GPTR(const int32_t, o->features),
                   o->is_reg ? (const void*)GPTR(const float, o->yreg) : (const void*)GPTR(const int32_t, o->ycls),
                   GPTR(uint8_t, o->part), o->out_pred ? GPTR(uint8_t, o->out_pred) : nullptr,
                   o->out_walked ? GPTR(unsigned long long, o->out_walked) : nullptr,
                   (int)o->K, (int)o->F, o->depth_cap > 0 ? (int)o->depth_cap : 1 << 20,
                   (no_skip || o->no_skip) ? 1 : 0};
  const int64_t blocks = (o->n_rows + 255) / 256, FK = o->F * o->K;
  const dim3 grid((unsigned)blocks, (unsigned)o->F);
  const unsigned rgrid = (unsigned)((FK + 255) / 256);
  if (o->is_reg) {
    k_perm_reg<U><<<grid, 256, lds, st>>>(a, e);
    k_perm_reduce<double><<<rgrid, 256, 0, st>>>(GPTR(const double, o->part), GPTR(double, o->out), blocks, FK);
  } else {
    const int C = (int)o->n_classes;
    if (C <= 2) k_perm_cls<2, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 4) k_perm_cls<4, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 8) k_perm_cls<8, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 16) k_perm_cls<16, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 32) k_perm_cls<32, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 64) {
      // 64 class sums with 16 lock-step walks: the slot loops are too large to unroll and the leaf
      // arrays would live in scratch -- dml_forest_perm sends these through the 8-wide walk
      if constexpr (U < 16) k_perm_cls<64, U><<<grid, 256, lds, st>>>(a, e);
      else return 5;
    } else return 5;
    k_perm_reduce<long long><<<rgrid, 256, 0, st>>>(GPTR(const long long, o->part), GPTR(long long, o->out), blocks, FK);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// launch_perm's LDS layout with grid.y = a slot of features[]; the slots go f_chunk at a time, each
// chunk's partials reduced into out before the next chunk overwrites them (one stream: in order)
template <int U>
static int launch_pd(const PdArgs* o, hipStream_t st) {
  PredictArgs a{};
  a.Xb = o->Xb; a.ld = o->ld; a.d = o->d;
  a.nodes = o->nodes; a.node_val = o->node_val; a.VC = o->VC; a.is_reg = o->is_reg; a.n_classes = o->n_classes;
  a.fit_tree_off = o->fit_tree_off; a.fit_row_off = o->fit_row_off; a.rows = o->rows;
  a.F = 1; a.max_rows = o->n_rows; a.max_trees = o->t1 - o->t0;
  a.toptab = o->toptab;
  // stage_rows' row list and the largest block-sum table (KC * MAXC <= 64 doubles per wave)
  constexpr size_t kStatic = 256 * sizeof(int32_t) + 4 * 64 * sizeof(double);
  a.lds_pitch = predict_pitch(&a);
  if ((size_t)a.lds_pitch * 256 + kStatic > 64 * 1024) a.lds_pitch = 0;
  size_t lds = (size_t)a.lds_pitch * 256;
  static const bool top_off = getenv("DML_PRED_NO_TOP") != nullptr;
  const size_t lds_top = ((lds + 15) & ~(size_t)15) + (size_t)U * kTopSlots * sizeof(NodeRec);
  if (top_off || lds_top + kStatic > 64 * 1024) a.toptab = 0;
  if (a.toptab) {
    k_top_fill<<<dim3((unsigned)((a.max_trees + 3) / 4), 1), 256, 0, st>>>(a);
    lds = lds_top;
  }
  static const bool no_skip = getenv("DML_PD_NO_SKIP") != nullptr;
  const int C = (int)o->n_classes;
  const int64_t blocks = (o->n_rows + 255) / 256;
  for (int64_t f0 = 0; f0 < o->F; f0 += o->f_chunk) {
    const int Fc = (int)(o->F - f0 < o->f_chunk ? o->F - f0 : o->f_chunk);
    const PdTail e{GPTR(const int32_t, o->features), GPTR(const uint8_t, o->sub_bins), GPTR(const int32_t, o->n_grid),
                   GPTR(double, o->part), o->out_rows ? GPTR(float, o->out_rows) : nullptr,
                   o->out_walked ? GPTR(unsigned long long, o->out_walked) : nullptr,
                   (int)o->Gmax, Fc, (int)f0, (int)o->n_targets, (int)o->c0,
                   o->depth_cap > 0 ? (int)o->depth_cap : 1 << 20, (no_skip || o->no_skip) ? 1 : 0};
    const dim3 grid((unsigned)blocks, (unsigned)Fc);
    if (o->is_reg) k_pd_reg<U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 2) k_pd_cls<2, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 4) k_pd_cls<4, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 8) k_pd_cls<8, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 16) k_pd_cls<16, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 32) k_pd_cls<32, U><<<grid, 256, lds, st>>>(a, e);
    else if (C <= 64) {
      // as launch_perm: 64 class sums run the 8-wide walk (dml_forest_pd), or the leaf arrays spill
      if constexpr (U < 16) k_pd_cls<64, U><<<grid, 256, lds, st>>>(a, e);
      else return 5;
    } else return 5;
    const int64_t FGN = (int64_t)Fc * o->Gmax * o->n_targets;
    k_pd_reduce<<<(unsigned)((FGN + 255) / 256), 256, 0, st>>>(GPTR(const double, o->part), GPTR(double, o->out),
                                                             GPTR(const int32_t, o->n_grid), blocks, Fc, (int)f0,
                                                             (int)o->Gmax, (int)o->n_targets);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// max_leaf_nodes: one lane per limited tree replays sklearn's best-first order over the
// grown tree (forest_common.h best_first_prune); the frontier heap lives in global
// scratch, ``cap`` entries per lane.  Trees with limit 0 are left alone.
__global__ void k_prune_best_first(NodeRec* nodes, const double* vals, int64_t VC, int C, int is_reg,
                                   const TreeSpec* specs, const int32_t* limit, int32_t t0, int32_t T,
                                   FrontierEnt* heap, int64_t cap, int32_t* leaves) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  const int t = t0 + i;   // tree t's root is pool node t
  const int L = limit[t];
  if (L <= 0 || L > cap) { if (leaves) leaves[t] = -1; return; }
  const int n = best_first_prune(nodes, vals, VC, C, is_reg != 0, specs[t].criterion, t, L, heap + (int64_t)i * cap);
  if (leaves) leaves[t] = n;
}

}  // namespace dml

using namespace dml;

extern "C" {

int dml_forest_prune(NodeRec* nodes, const double* vals, int64_t VC, int32_t C, int32_t is_reg,
                     const TreeSpec* specs, const int32_t* limit, int32_t t0, int32_t T, void* heap, int64_t cap,
                     int32_t* leaves, hipStream_t st) {
  if (T <= 0) return 0;
  if (cap <= 0 || heap == nullptr) return 2;
  k_prune_best_first<<<(unsigned)((T + 63) / 64), 64, 0, st>>>(nodes, vals, VC, C, is_reg, specs, limit, t0, T,
                                                               static_cast<FrontierEnt*>(heap), cap, leaves);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

int dml_forest_refine(const uint8_t* Xb, int64_t ld, int64_t n, int64_t d, NodeRec* nodes, int64_t P,
                      const TreeSpec* specs, int32_t T, const uint8_t* roles, const float* vals, const uint8_t* exact,
                      uint32_t* hi, hipStream_t st) {
  if (P <= 0 || T <= 0) return 0;
  if (hipMemsetAsync(hi, 0xFF, (size_t)P * 4, st) != hipSuccess) return 1;
  dim3 g1((unsigned)((n + 255) / 256), (unsigned)T);
  k_refine_hi<<<g1, 256, 0, st>>>(Xb, ld, n, nodes, specs, roles, hi);
  k_refine_split<<<(unsigned)((P + 255) / 256), 256, 0, st>>>(nodes, P, d, hi, vals, exact);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}


int dml_forest_apply(const uint8_t* Xb, int64_t ld, int64_t n, const dml::NodeRec* nodes, int32_t t0, int32_t T,
                     int32_t* leaf, hipStream_t st) {
  if (n <= 0 || T <= 0) return 0;
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)T);
  dml::k_apply<<<grid, 256, 0, st>>>(Xb, ld, n, nodes, t0, leaf);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

int dml_predict_sizeof_args() { return (int)sizeof(PredictArgs); }

int dml_forest_predict(PredictArgs* a, hipStream_t st) {
  if (a->F <= 0 || a->max_rows <= 0) return 0;
  static const int u = [] { const char* e = getenv("DML_PRED_U"); return e ? atoi(e) : 8; }();
  if (u == 16) return launch_predict<16>(a, st);
  if (u == 4) return launch_predict<4>(a, st);
  return launch_predict<8>(a, st);
}

// predict fit f alone (its trees and held-out rows; outputs stay at their absolute rows) --
// the forest builder calls this for a fit whose trees are complete while deeper fits of the
// same build are still growing (forest.hip early predict)
int dml_forest_predict_fit(const PredictArgs* a, int32_t f, hipStream_t st) {
  if (f < 0 || f >= a->F) return 2;
  const int64_t* roff = (const int64_t*)a->fit_row_off_host;
  PredictArgs b = *a;
  b.fit_tree_off = a->fit_tree_off + 4 * (int64_t)f;   // int32[F+1] device array, advanced to fit f
  b.fit_row_off = a->fit_row_off + 8 * (int64_t)f;     // int64[F+1]
  b.F = 1;
  b.fit_skip = 0;
  if (a->fit_depth_cap) b.fit_depth_cap = a->fit_depth_cap + 4 * (int64_t)f;
  b.max_rows = roff ? roff[f + 1] - roff[f] : a->max_rows;
  return dml_forest_predict(&b, st);
}

int dml_oob_sizeof_args() { return (int)sizeof(OobArgs); }

// out-of-bag prediction of one kept fit over its training rows (k_oob_cls / k_oob_reg)
int dml_forest_oob(const OobArgs* o, hipStream_t st) {
  if (o->n_rows <= 0) return 0;
  if (o->t1 <= o->t0 || o->t0 < 0) return 2;
  static const int u = [] { const char* e = getenv("DML_PRED_U"); return e ? atoi(e) : 8; }();
  if (u == 16) return launch_oob<16>(o, st);
  if (u == 4) return launch_oob<4>(o, st);
  return launch_oob<8>(o, st);
}

int dml_perm_sizeof_args() { return (int)sizeof(PermArgs); }

// permutation-importance score statistics of one kept fit over its held-out rows
// (k_perm_cls / k_perm_reg, then k_perm_reduce)
int dml_forest_perm(const PermArgs* o, hipStream_t st) {
  if (o->n_rows <= 0 || o->F <= 0 || o->K <= 0) return 0;
  if (o->t1 <= o->t0 || o->t0 < 0 || o->F > 65535 || !o->part || !o->out) return 2;
  static const int u = [] { const char* e = getenv("DML_PRED_U"); return e ? atoi(e) : 8; }();
  if (u == 16 && (o->is_reg || o->n_classes <= 32)) return launch_perm<16>(o, st);
  if (u == 4) return launch_perm<4>(o, st);
  return launch_perm<8>(o, st);
}

int dml_pd_sizeof_args() { return (int)sizeof(PdArgs); }

// partial-dependence sums of one kept fit over its rows (k_pd_cls / k_pd_reg, then k_pd_reduce,
// f_chunk slots of features[] per launch)
int dml_forest_pd(const PdArgs* o, hipStream_t st) {
  if (o->n_rows <= 0 || o->F <= 0) return 0;
  if (o->t1 <= o->t0 || o->t0 < 0 || o->f_chunk < 1 || o->f_chunk > 65535 || o->Gmax < 1 || !o->part || !o->out ||
      !o->features || !o->sub_bins || !o->n_grid)
    return 2;
  if (o->n_targets < 1 || o->c0 < 0 || (o->is_reg ? o->n_targets != 1 || o->c0 != 0 : o->c0 + o->n_targets > o->n_classes))
    return 2;
  static const int u = [] { const char* e = getenv("DML_PRED_U"); return e ? atoi(e) : 8; }();
  if (u == 16 && (o->is_reg || o->n_classes <= 32)) return launch_pd<16>(o, st);
  if (u == 4) return launch_pd<4>(o, st);
  return launch_pd<8>(o, st);
}

int dml_scores(ScoreArgs* a, hipStream_t st) {
  if (a->F <= 0) return 0;
  k_scores<<<(unsigned)a->F, 256, 0, st>>>(*a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // extern "C"
