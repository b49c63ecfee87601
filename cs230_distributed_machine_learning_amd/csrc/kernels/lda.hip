// lda.hip -- LinearDiscriminantAnalysis for every (candidate, split) of a job (docs/LDA.md).
//
// The class moments come from qda.hip's k_qda_class_moments; this unit adds the two passes over
// the rows that the moments cannot give.  Float64 throughout, the float32 table widened on load.
//
// k_lda_lw_stat: the Ledoit-Wolf statistic of shrinkage="auto", sum over a class's training rows
//   of (sum_j ((x_j - m_j) / s_j)^2)^2, for every (cell, split) at once.  Workgroup (cell,
//   partition p) stages the cell's class tables (mean and 1 / variance, zero for the splits in
//   which the cell's bucket does not train) of up to 16 splits in LDS once, then walks blocks
//   p, p + parts, ... of 16 rows: wave w takes rows 4 w .. 4 w + 3 of a block, 16 lanes per row.
//   A lane widens its columns j = (lane & 15) + 16 u of x once and loops over the splits with the
//   tables read from LDS, so x is read once per row however many splits there are.  The 16-lane
//   sum is a DPP butterfly (wave_ops.h), after which every lane of the row holds q; q^2 is added
//   per (lane group, split) in registers in ascending row order, the 16 lane groups of the
//   workgroup are added through LDS in a fixed order, and k_lda_stat_reduce adds the partitions
//   in ascending order.  No atomics: the result repeats bit for bit.
//
// k_lda_score: workgroup (tile of 64 held-out rows, split), 4 waves, wave w owning rows
//   16 w .. 16 w + 15.  The x tile goes to LDS once with coalesced loads (float32); each wave
//   lifts its B operands (x^T, Dp / 4 doubles per lane) into registers and keeps them for the
//   whole kernel, after which the tile's LDS is reused for W.  The product is computed
//   TRANSPOSED on v_mfma_f64_16x16x4f64 (operand map at the top of qda.hip),
//   D^T[col][row] = W x^T, over column tiles of 16 with col = class * NCp + candidate.  W's
//   column slabs stream through LDS double-buffered, stored k-major at a pitch of 17 so that both
//   the coalesced stores and the A-operand reads spread over the banks; the next slab's global
//   loads are in flight during the current slab's MFMAs.  Lane l holds row l & 15 and columns
//   (l >> 4) + 4 g: element g of every tile belongs to one candidate (for NCp >= 4, up to
//   relabelling of g), so the running (max, class) lives in registers, classes ascending.  The
//   four elements are merged in the lane where they share a candidate (NCp <= 8), and for NCp = 2
//   and 1 the lane groups l >> 4 are merged once after the last tile by two cross-lane exchanges.
//   Ties keep the lower class everywhere.  Padded candidates and rows past a split's end are
//   never written.
//
// Limits: d <= 128 (kLdaMaxD), <= 16 candidates per scoring launch, <= 16 splits per statistic
// launch, any number of classes, up to 2^31 - 1 rows.  LDS at d = 128: k_lda_score 34 KiB (the W
// slabs; the 33 KiB row tile lives in the same bytes before them), k_lda_lw_stat 34 KiB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lda_args.h"
#include "wave_ops.h"

namespace dml {

typedef double ld_f64x4 __attribute__((ext_vector_type(4)));

#define LD_PTR(T, v) reinterpret_cast<T*>(static_cast<uintptr_t>(v))

constexpr int kLdaWPitch = 17;       // doubles between consecutive k rows of a W slab in LDS
constexpr int kLdaNoClass = 0x7fffffff;

__host__ __device__ __forceinline__ int ld_up16(int64_t v) { return (int)((v + 15) / 16 * 16); }

__global__ __launch_bounds__(256) void k_lda_lw_stat(LdaStatArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ld_lds[];
  const int cell = blockIdx.x, p = blockIdx.y;
  const int d = (int)a.d, Dp = ld_up16(a.d), T = Dp / 16, S = (int)a.S, C = (int)a.C, P = (int)a.parts;
  double* ms = ld_lds;                 // [S][Dp] class means
  double* ws = ms + S * Dp;            // [S][Dp] 1 / variance, 0 where the bucket does not train
  double* red = ws + S * Dp;           // [kLdaMaxSplits][16 lane groups]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lg = lane >> 4, lj = lane & 15;
  const int bucket = cell / C, cls = cell - bucket * C;
  const int32_t* __restrict__ train = LD_PTR(const int32_t, a.train) + (int64_t)bucket * S;
  const double* __restrict__ mean = LD_PTR(const double, a.mean);
  const double* __restrict__ w = LD_PTR(const double, a.w);
  for (int idx = threadIdx.x; idx < S * Dp; idx += 256) {
    const int s = idx / Dp, j = idx - s * Dp;
    const bool ok = j < d && train[s] != 0;
    const int64_t at = ((int64_t)s * C + cls) * d + j;
    ms[idx] = ok ? mean[at] : 0.0;
    ws[idx] = ok ? w[at] : 0.0;
  }
  __syncthreads();
  const float* __restrict__ X = LD_PTR(const float, a.X);
  const int32_t* __restrict__ perm = LD_PTR(const int32_t, a.perm);
  const int64_t* __restrict__ cell_off = LD_PTR(const int64_t, a.cell_off);
  int64_t r0 = cell_off[cell], r1 = cell_off[cell + 1];
  if (r0 < 0) r0 = 0;
  if (r1 > a.n) r1 = a.n;            // never a read outside perm
  const int64_t n_blk = r1 > r0 ? (r1 - r0 + 15) / 16 : 0;
  double acc[kLdaMaxSplits];
#pragma unroll
  for (int s = 0; s < kLdaMaxSplits; ++s) acc[s] = 0.0;
  for (int64_t blk = p; blk < n_blk; blk += P) {
    const int64_t pos = r0 + blk * 16 + wv * 4 + lg;
    int64_t row = pos < r1 ? (int64_t)perm[pos] : -1;
    if (row >= a.n) row = -1;
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = lj + 16 * u;
      x[u] = (row >= 0 && j < d) ? (double)X[row * a.ld + j] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < kLdaMaxSplits; ++s) {
      if (s < S) {
        double q = 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (u < T) {
            const double c = x[u] - ms[s * Dp + lj + 16 * u];
            q += ws[s * Dp + lj + 16 * u] * (c * c);
          }
        }
        q += wave::shfl_xor<8>(q, lane);
        q += wave::shfl_xor<4>(q, lane);
        q += wave::shfl_xor<2>(q, lane);
        q += wave::shfl_xor<1>(q, lane);
        if (row >= 0) acc[s] += q * q;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < kLdaMaxSplits; ++s)
    if (s < S && lj == 0) red[s * 16 + wv * 4 + lg] = acc[s];
  __syncthreads();
  if ((int)threadIdx.x < S) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t = t + red[threadIdx.x * 16 + k];
    LD_PTR(double, a.part)[((int64_t)cell * P + p) * S + threadIdx.x] = t;
  }
}

// out[cell][s] = part[cell][0][s] + part[cell][1][s] + ...
__global__ __launch_bounds__(256) void k_lda_stat_reduce(LdaStatArgs a) {
  const int S = (int)a.S, P = (int)a.parts;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_cells * S) return;
  const int64_t cell = i / S, s = i - cell * S;
  const double* __restrict__ part = LD_PTR(const double, a.part) + cell * P * S + s;
  double t = 0.0;
  for (int p = 0; p < P; ++p) t = t + part[(int64_t)p * S];
  LD_PTR(double, a.out)[i] = t;
}

// (bv, bc) <- the better of (bv, bc) and (ov, oc): the larger value, the lower class on a tie
__device__ __forceinline__ void ld_merge(double& bv, int& bc, double ov, int oc) {
  if (ov > bv || (ov == bv && oc < bc)) {
    bv = ov;
    bc = oc;
  }
}

template <int KS>   // k-steps (of 4 features) a lane keeps of its row: Dp <= 4 KS
__global__ __launch_bounds__(256) void k_lda_score(LdaScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ld_lds[];
  constexpr int NR = KS / 4;   // doubles of a W slab (16 x Dp) per thread
  const int d = (int)a.d, Dp = ld_up16(a.d), C = (int)a.C, NC = (int)a.NC, NCp = (int)a.NCp;
  const int sh = 31 - __builtin_clz((unsigned)NCp);
  const int xp = Dp + 1;   // pitch of the row tile (floats): rows 16 apart fall in different banks
  double* Ws = ld_lds;                                 // [2][Dp][kLdaWPitch], after the row tile is lifted
  float* xs = reinterpret_cast<float*>(ld_lds);        // [kLdaRowTile][xp], until then
  const int s = blockIdx.y;
  const int64_t* __restrict__ row_off = LD_PTR(const int64_t, a.row_off);
  const int64_t roff = row_off[s];
  const int64_t nrows = row_off[s + 1] - roff;
  const int64_t t0 = (int64_t)blockIdx.x * kLdaRowTile;
  if (t0 >= nrows || roff < 0 || roff + nrows > a.total_rows) return;   // block-uniform, before any barrier
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lg = lane >> 4, lj = lane & 15;
  const int ncols = C * NCp, NT = (ncols + 15) / 16;
  const double* __restrict__ Wsp = LD_PTR(const double, a.W) + (int64_t)s * ncols * d;
  const double* __restrict__ bsp = LD_PTR(const double, a.b) + (int64_t)s * ncols;
  double regs[NR];
  // slab t of W (columns 16 t .. 16 t + 15, zero past the last column and past d) into registers /
  // from them into LDS, k-major
  auto fetch = [&](int t) {
#pragma unroll
    for (int u = 0; u < NR; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int col = idx / Dp, k = idx - col * Dp, gc = t * 16 + col;
      regs[u] = (idx < 16 * Dp && k < d && gc < ncols) ? Wsp[(int64_t)gc * d + k] : 0.0;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < NR; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int col = idx / Dp, k = idx - col * Dp;
      if (idx < 16 * Dp) Ws[(buf * Dp + k) * kLdaWPitch + col] = regs[u];
    }
  };
  fetch(0);
  const float* __restrict__ X = LD_PTR(const float, a.X);
  const int32_t* __restrict__ rows = LD_PTR(const int32_t, a.rows) + roff + t0;
  for (int idx = threadIdx.x; idx < kLdaRowTile * Dp; idx += 256) {
    const int r = idx / Dp, k = idx - r * Dp;
    float v = 0.f;
    if (t0 + r < nrows && k < d) {
      const int64_t row = rows[r];
      if (row >= 0 && row < a.n) v = X[row * a.ld + k];
    }
    xs[r * xp + k] = v;
  }
  __syncthreads();
  const int my_row = 16 * wv + lj;                       // the row this lane's results belong to
  const bool row_ok = t0 + my_row < nrows;
  const int64_t grow = roff + t0 + my_row;               // its place in rows / pred / dec
  double xb[KS];                                         // B operand: x[my_row][4 kk + lg]
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) xb[kk] = 4 * kk < Dp ? (double)xs[my_row * xp + 4 * kk + lg] : 0.0;
  __syncthreads();   // every wave has lifted its rows: the tile's bytes now hold W slabs
  stash(0);
  __syncthreads();
  double best[4];
  int bestc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    best[g] = -INFINITY;
    bestc[g] = kLdaNoClass;
  }
  double* __restrict__ dec = LD_PTR(double, a.dec);
  for (int t = 0; t < NT; ++t) {
    if (t + 1 < NT) fetch(t + 1);
    const double* wb = Ws + (t & 1) * Dp * kLdaWPitch;
    ld_f64x4 acc = ld_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
      if (4 * kk < Dp)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wb[(4 * kk + lg) * kLdaWPitch + lj], xb[kk], acc, 0, 0, 0);
    // acc[g] = x[my_row] . W[column 16 t + lg + 4 g]
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int col = 16 * t + lg + 4 * g, cls = col >> sh, cand = col & (NCp - 1);
      if (cls < C) {
        const double v = acc[g] + bsp[col];
        if (dec && row_ok && cand < NC) dec[((int64_t)cand * a.total_rows + grow) * C + cls] = v;
        if (v > best[g]) {
          best[g] = v;
          bestc[g] = cls;
        }
      }
    }
    if (t + 1 < NT) stash((t + 1) & 1);
    __syncthreads();
  }
  // elements g and g + 2 share a candidate when NCp <= 8, all four when NCp <= 4; lane groups lg
  // and lg ^ 2 when NCp <= 2, all of them when NCp = 1
  if (NCp <= 8) {
    ld_merge(best[0], bestc[0], best[2], bestc[2]);
    ld_merge(best[1], bestc[1], best[3], bestc[3]);
  }
  if (NCp <= 4) ld_merge(best[0], bestc[0], best[1], bestc[1]);
  if (NCp <= 2) ld_merge(best[0], bestc[0], wave::shfl_xor<32>(best[0], lane), wave::shfl_xor<32>(bestc[0], lane));
  if (NCp == 1) ld_merge(best[0], bestc[0], wave::shfl_xor<16>(best[0], lane), wave::shfl_xor<16>(bestc[0], lane));
  if (row_ok) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cand = lg + 4 * g;
      if (4 * g < NCp && cand < NC)   // no value above -inf (or only NaN): class 0, as argmax gives
        LD_PTR(int32_t, a.pred)[(int64_t)cand * a.total_rows + grow] = bestc[g] == kLdaNoClass ? 0 : bestc[g];
    }
  }
}

}  // namespace dml

using namespace dml;

extern "C" {

int dml_lda_sizeof_stat_args() { return (int)sizeof(LdaStatArgs); }
int dml_lda_sizeof_score_args() { return (int)sizeof(LdaScoreArgs); }
int dml_lda_max_d() { return kLdaMaxD; }
int dml_lda_max_candidates() { return kLdaMaxCand; }
int dml_lda_max_splits() { return kLdaMaxSplits; }

// 0: launched; 1: a HIP error; 2: bad arguments; 3: d, S or NC above the limit (nothing was launched).
int dml_lda_lw_stat(const LdaStatArgs* a, hipStream_t st) {
  if (a->n < 0 || a->d < 1 || a->n_cells < 0 || a->C < 1 || a->S < 1 || a->ld < a->d || a->parts < 1 ||
      a->parts > kLdaMaxParts || a->n_cells % a->C != 0)
    return kLdaBadArgs;
  if (a->d > kLdaMaxD || a->S > kLdaMaxSplits) return kLdaTooLarge;
  if (a->n_cells == 0) return kLdaOk;
  if (!a->perm || !a->cell_off || !a->train || !a->mean || !a->w || !a->part || !a->out || (a->n > 0 && !a->X) ||
      a->n > 2147483647LL || a->n_cells > 2147483647LL)
    return kLdaBadArgs;
  const int Dp = ld_up16(a->d);
  const size_t lds = (size_t)(2 * a->S * Dp + kLdaMaxSplits * 16) * sizeof(double);
  k_lda_lw_stat<<<dim3((unsigned)a->n_cells, (unsigned)a->parts), 256, lds, st>>>(*a);
  const int64_t total = a->n_cells * a->S;
  k_lda_stat_reduce<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(*a);
  return hipGetLastError() == hipSuccess ? kLdaOk : kLdaHipError;
}

int dml_lda_score(const LdaScoreArgs* a, hipStream_t st) {
  if (a->n < 0 || a->d < 1 || a->S < 0 || a->C < 1 || a->NC < 1 || a->NCp < a->NC || (a->NCp & (a->NCp - 1)) != 0 ||
      a->max_rows < 0 || a->total_rows < 0 || a->ld < a->d || a->max_rows > a->total_rows)
    return kLdaBadArgs;
  if (a->d > kLdaMaxD || a->NCp > kLdaMaxCand) return kLdaTooLarge;
  if (a->S == 0 || a->max_rows == 0) return kLdaOk;
  if (!a->X || !a->rows || !a->row_off || !a->W || !a->b || !a->pred || a->total_rows > 2147483647LL ||
      a->S > 65535 || a->C > (1 << 24))
    return kLdaBadArgs;
  const int Dp = ld_up16(a->d);
  const size_t w_bytes = (size_t)2 * Dp * kLdaWPitch * sizeof(double);
  const size_t x_bytes = (size_t)kLdaRowTile * (Dp + 1) * sizeof(float);
  const size_t lds = w_bytes > x_bytes ? w_bytes : x_bytes;
  const dim3 grid((unsigned)((a->max_rows + kLdaRowTile - 1) / kLdaRowTile), (unsigned)a->S);
  if (Dp <= 16)
    k_lda_score<4><<<grid, 256, lds, st>>>(*a);
  else if (Dp <= 32)
    k_lda_score<8><<<grid, 256, lds, st>>>(*a);
  else if (Dp <= 64)
    k_lda_score<16><<<grid, 256, lds, st>>>(*a);
  else
    k_lda_score<32><<<grid, 256, lds, st>>>(*a);
  return hipGetLastError() == hipSuccess ? kLdaOk : kLdaHipError;
}

}  // extern "C"
