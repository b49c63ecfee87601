// qda.hip -- QuadraticDiscriminantAnalysis for every (candidate, split) of a job (docs/QDA.md).
//
// Float64 throughout on v_mfma_f64_16x16x4f64; the float32 table is widened on load.  The MFMA
// operand map used below (as in linear.hip): lane l gives A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15], and holds D[i = (l >> 4) + 4 g][j = l & 15] in element g.
//
// k_qda_class_moments: every row belongs to one (fold bucket, class) cell; the host passes the
//   rows grouped by cell.  Workgroup (cell, strip ti, partition p) walks slabs p, p + parts, ...
//   of the cell's rows; a slab is 32 rows of z = [x - shift, 1] staged once in LDS as float64 and
//   read by the 4 waves, wave w owning the tiles (ti, ti + w + 4 q) of the strip.  Column d of z
//   makes the count and the column sums part of the same product.  Each workgroup stores its
//   tiles; k_qda_moments_reduce adds the partitions in ascending order.  No atomics: the result
//   repeats run to run, and the host twin (../runtime/qda_cpu.cpp) adds in the same order.
//
// k_qda_score: workgroup (row tile of 32 held-out rows, split).  The rows' x go to LDS once, as
//   float32.  Per class c the workgroup forms Z^T = V_c^T (x - mu_c)^T: V_c streams through LDS
//   in slabs of 16 components' rows (k), double-buffered (the next slab's global loads are in
//   flight while the current one feeds the MFMAs); wave w accumulates the 16 x 16 tiles
//   (columns 16 (w >> 1 + 2 q), rows 16 (w & 1)).  Computing the TRANSPOSE puts Z in the B-operand
//   layout of a second product: the squares, still in registers, are contracted with the
//   candidates' 1 / variance table (A operand, 16 candidates per tile) -- q[cand][row].  The two
//   waves of a row tile are added through LDS in a fixed order, the owner adds the candidate's
//   constant and keeps a running (max, argmax) per (row, candidate) in registers; ties keep the
//   lower class.
//
// Limits: d <= 128 (kQdaMaxD), <= 32 candidates per launch (kQdaMaxCand), any number of classes,
// up to 2^31 - 1 rows.  LDS of k_qda_score at d = 128: 2 x 16 KiB V slabs + 16.1 KiB rows + 8 KiB
// wave sums + 1 KiB mean = 57.1 KiB, two workgroups per CU (160 KiB); less at smaller d (the
// arrays are sized by roundup(d, 16)).  k_qda_class_moments at d = 128: 36 KiB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "qda_args.h"

namespace dml {

typedef double qd_f64x4 __attribute__((ext_vector_type(4)));

#define QD_PTR(T, v) reinterpret_cast<T*>(static_cast<uintptr_t>(v))

__host__ __device__ __forceinline__ int qd_up16(int64_t v) { return (int)((v + 15) / 16 * 16); }

__global__ __launch_bounds__(256) void k_qda_class_moments(QdaMomArgs a) {
  extern __shared__ __attribute__((aligned(16))) double qd_zs[];   // [kQdaSlabRows][Dp]
  const int cell = blockIdx.x, ti = blockIdx.y, p = blockIdx.z;
  const int d = (int)a.d, Dp = qd_up16(a.d + 1), T = Dp / 16, P = (int)a.parts;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* __restrict__ X = QD_PTR(const float, a.X);
  const double* __restrict__ shift = QD_PTR(const double, a.shift);
  const int32_t* __restrict__ perm = QD_PTR(const int32_t, a.perm);
  const int64_t* __restrict__ cell_off = QD_PTR(const int64_t, a.cell_off);
  int64_t r0 = cell_off[cell], r1 = cell_off[cell + 1];
  if (r0 < 0) r0 = 0;
  if (r1 > a.n) r1 = a.n;            // never a read outside perm
  const int64_t n_slabs = r1 > r0 ? (r1 - r0 + kQdaSlabRows - 1) / kQdaSlabRows : 0;
  qd_f64x4 acc[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) acc[q] = qd_f64x4{0.0, 0.0, 0.0, 0.0};
  for (int64_t s = p; s < n_slabs; s += P) {
    __syncthreads();   // the previous slab has been read
    for (int idx = threadIdx.x; idx < kQdaSlabRows * Dp; idx += 256) {
      const int r = idx / Dp, c = idx - r * Dp;
      const int64_t pos = r0 + s * kQdaSlabRows + r;
      double v = 0.0;
      if (pos < r1) {
        const int64_t row = perm[pos];
        if (row >= 0 && row < a.n) v = c < d ? (double)X[row * a.ld + c] - shift[c] : (c == d ? 1.0 : 0.0);
      }
      qd_zs[idx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kQdaSlabRows / 4; ++kk) {
      const double* zr = qd_zs + (kk * 4 + (lane >> 4)) * Dp;
      const double av = zr[ti * 16 + (lane & 15)];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int tj = ti + wv + 4 * q;
        if (tj < T) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, zr[tj * 16 + (lane & 15)], acc[q], 0, 0, 0);
      }
    }
  }
  double* __restrict__ part = QD_PTR(double, a.part) + ((int64_t)cell * P + p) * Dp * Dp;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int tj = ti + wv + 4 * q;
    if (tj < T) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        part[(int64_t)(ti * 16 + (lane >> 4) + 4 * g) * Dp + tj * 16 + (lane & 15)] = acc[q][g];
    }
  }
}

// out[cell][row][col] = part[cell][0][row][col] + part[cell][1][row][col] + ... (tiles ti <= tj; 0 below)
__global__ __launch_bounds__(256) void k_qda_moments_reduce(QdaMomArgs a) {
  const int Dp = qd_up16(a.d + 1), P = (int)a.parts;
  const int64_t per = (int64_t)Dp * Dp, total = a.n_cells * per;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t cell = i / per, e = i - cell * per;
  const int row = (int)(e / Dp), col = (int)(e - (int64_t)row * Dp);
  double s = 0.0;
  if (row / 16 <= col / 16) {
    const double* __restrict__ part = QD_PTR(const double, a.part) + cell * P * per + e;
    for (int p = 0; p < P; ++p) s = s + part[p * per];
  }
  QD_PTR(double, a.out)[i] = s;
}

__global__ __launch_bounds__(256) void k_qda_score(QdaScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) double qd_lds[];
  const int d = (int)a.d, Dp = qd_up16(a.d), T = Dp / 16, C = (int)a.C, NC = (int)a.NC;
  const int xp = Dp + 1;   // pitch of the row tile (floats): rows 16 apart fall in different banks
  double* Vs = qd_lds;                                   // [2][16][Dp]
  double* red = Vs + 2 * 16 * Dp;                        // [2 row tiles][2 cand tiles][4][64]
  double* mus = red + 2 * 2 * 4 * 64;                    // [Dp]
  float* xs = reinterpret_cast<float*>(mus + Dp);        // [kQdaRowTile][xp]
  const int s = blockIdx.y;
  const int64_t* __restrict__ row_off = QD_PTR(const int64_t, a.row_off);
  const int64_t roff = row_off[s];
  const int64_t nrows = row_off[s + 1] - roff;
  const int64_t t0 = (int64_t)blockIdx.x * kQdaRowTile;
  if (t0 >= nrows || roff < 0 || roff + nrows > a.total_rows) return;   // block-uniform, before any barrier
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int rt = wv & 1, th = wv >> 1;
  const float* __restrict__ X = QD_PTR(const float, a.X);
  const int32_t* __restrict__ rows = QD_PTR(const int32_t, a.rows) + roff + t0;
  for (int idx = threadIdx.x; idx < kQdaRowTile * Dp; idx += 256) {
    const int r = idx / Dp, k = idx - r * Dp;
    float v = 0.f;
    if (t0 + r < nrows && k < d) {
      const int64_t row = rows[r];
      if (row >= 0 && row < a.n) v = X[row * a.ld + k];
    }
    xs[r * xp + k] = v;
  }
  double best[2][4];
  int bestc[2][4];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      best[ct][g] = -INFINITY;
      bestc[ct][g] = 0;
    }
  const int KS = Dp / 16;
  const int my_row = 16 * rt + (lane & 15);              // the row this lane's results belong to
  const bool row_ok = t0 + my_row < nrows;
  const int64_t grow = roff + t0 + my_row;               // its place in rows / pred / dec
  for (int c = 0; c < C; ++c) {
    const double* __restrict__ Vc = QD_PTR(const double, a.V) + ((int64_t)s * C + c) * d * d;
    const double* __restrict__ muc = QD_PTR(const double, a.mu) + ((int64_t)s * C + c) * d;
    double regs[8];
    // slab ks of V_c (rows k = 16 ks .. 16 ks + 15, zero past d) into registers / from them into LDS
    auto fetch = [&](int ks) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = threadIdx.x + 256 * u;
        const int kr = idx / Dp, j = idx - kr * Dp, k = ks * 16 + kr;
        regs[u] = (idx < 16 * Dp && k < d && j < d) ? Vc[(int64_t)k * d + j] : 0.0;
      }
    };
    auto stash = [&](int buf) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = threadIdx.x + 256 * u;
        if (idx < 16 * Dp) Vs[buf * 16 * Dp + idx] = regs[u];
      }
    };
    fetch(0);
    __syncthreads();   // the previous class is done with mus, Vs and red (and xs is written)
    if ((int)threadIdx.x < Dp) mus[threadIdx.x] = (int)threadIdx.x < d ? muc[threadIdx.x] : 0.0;
    stash(0);
    __syncthreads();
    qd_f64x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = qd_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + 1 < KS) fetch(ks + 1);
      const double* vb = Vs + (ks & 1) * 16 * Dp;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int kr = kk * 4 + (lane >> 4), k = ks * 16 + kr;
        const double b = (double)xs[my_row * xp + k] - mus[k];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int tj = th + 2 * q;
          if (tj < T) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(vb[kr * Dp + tj * 16 + (lane & 15)], b, acc[q], 0, 0, 0);
        }
      }
      if (ks + 1 < KS) stash((ks + 1) & 1);
      __syncthreads();
    }
    // acc[q][g] = Z[row my_row][component 16 tj + (lane >> 4) + 4 g]: the B operand of the contraction
    qd_f64x4 q2[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      q2[ct] = qd_f64x4{0.0, 0.0, 0.0, 0.0};
      if (ct * 16 < NC) {
        const int cand = ct * 16 + (lane & 15);
        const bool cand_ok = cand < NC;
        const double* __restrict__ ip =
            QD_PTR(const double, a.inv) + (((int64_t)s * NC + (cand_ok ? cand : 0)) * C + c) * d;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int tj = th + 2 * q;
          if (tj < T) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int col = 16 * tj + 4 * g + (lane >> 4);
              const double w = (cand_ok && col < d) ? ip[col] : 0.0;
              const double z = acc[q][g];
              q2[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(w, z * z, q2[ct], 0, 0, 0);
            }
          }
        }
      }
    }
    // q2[ct][g] = this wave's share of q[candidate 16 ct + (lane >> 4) + 4 g][row my_row]
    if (th == 1) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) red[((rt * 2 + ct) * 4 + g) * 64 + lane] = q2[ct][g];
    }
    __syncthreads();
    if (th == 0) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int cand = ct * 16 + (lane >> 4) + 4 * g;
          if (cand < NC && row_ok) {
            const double q = q2[ct][g] + red[((rt * 2 + ct) * 4 + g) * 64 + lane];
            const double v = QD_PTR(const double, a.cst)[((int64_t)s * NC + cand) * C + c] - 0.5 * q;
            if (a.dec) QD_PTR(double, a.dec)[((int64_t)cand * a.total_rows + grow) * C + c] = v;
            if (v > best[ct][g]) {
              best[ct][g] = v;
              bestc[ct][g] = c;
            }
          }
        }
    }
  }
  if (th == 0 && row_ok) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cand = ct * 16 + (lane >> 4) + 4 * g;
        if (cand < NC) QD_PTR(int32_t, a.pred)[(int64_t)cand * a.total_rows + grow] = bestc[ct][g];
      }
  }
}

}  // namespace dml

using namespace dml;

extern "C" {

int dml_qda_sizeof_mom_args() { return (int)sizeof(QdaMomArgs); }
int dml_qda_sizeof_score_args() { return (int)sizeof(QdaScoreArgs); }
int dml_qda_max_d() { return kQdaMaxD; }
int dml_qda_max_candidates() { return kQdaMaxCand; }

// 0: launched; 1: a HIP error; 2: bad arguments; 3: d above dml_qda_max_d() (nothing was launched).
int dml_qda_class_moments(const QdaMomArgs* a, hipStream_t st) {
  if (a->n < 0 || a->d < 1 || a->n_cells < 0 || a->ld < a->d || a->parts < 1 || a->parts > kQdaMaxParts)
    return kQdaBadArgs;
  if (a->d > kQdaMaxD) return kQdaTooLarge;
  if (a->n_cells == 0) return kQdaOk;
  if (!a->shift || !a->perm || !a->cell_off || !a->part || !a->out || (a->n > 0 && !a->X) ||
      a->n > 2147483647LL || a->n_cells > 2147483647LL)
    return kQdaBadArgs;
  const int Dp = qd_up16(a->d + 1);
  const dim3 grid((unsigned)a->n_cells, (unsigned)(Dp / 16), (unsigned)a->parts);
  k_qda_class_moments<<<grid, 256, (size_t)kQdaSlabRows * Dp * sizeof(double), st>>>(*a);
  const int64_t total = a->n_cells * Dp * Dp;
  k_qda_moments_reduce<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(*a);
  return hipGetLastError() == hipSuccess ? kQdaOk : kQdaHipError;
}

int dml_qda_score(const QdaScoreArgs* a, hipStream_t st) {
  if (a->n < 0 || a->d < 1 || a->S < 0 || a->C < 1 || a->NC < 1 || a->max_rows < 0 || a->total_rows < 0 ||
      a->ld < a->d || a->max_rows > a->total_rows)
    return kQdaBadArgs;
  if (a->d > kQdaMaxD || a->NC > kQdaMaxCand) return kQdaTooLarge;
  if (a->S == 0 || a->max_rows == 0) return kQdaOk;
  if (!a->X || !a->rows || !a->row_off || !a->mu || !a->V || !a->inv || !a->cst || !a->pred ||
      a->total_rows > 2147483647LL || a->S > 65535)
    return kQdaBadArgs;
  const int Dp = qd_up16(a->d);
  const size_t lds = (size_t)(2 * 16 * Dp + 2 * 2 * 4 * 64 + Dp) * sizeof(double) +
                     (size_t)kQdaRowTile * (Dp + 1) * sizeof(float);
  const dim3 grid((unsigned)((a->max_rows + kQdaRowTile - 1) / kQdaRowTile), (unsigned)a->S);
  k_qda_score<<<grid, 256, lds, st>>>(*a);
  return hipGetLastError() == hipSuccess ? kQdaOk : kQdaHipError;
}

}  // extern "C"
