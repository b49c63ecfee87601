// rank_stats.hip -- the statistics of the ranking and probability scorers (roc_auc*,
// average_precision, neg_log_loss, neg_brier_score, top_k_accuracy) for all fits of a batch,
// without leaving the device once per fit (docs/RANK_SCORES.md).
//
// Inputs as score_stats.hip: the held-out row ids of F fits concatenated (fit f owns entries
// [fit_row_off[f], fit_row_off[f + 1])), the table's class ids, and per entry K float32 scores
// (row-major [total][K]).  A problem is one (fit, column): p = f * K + j, positive class pos0 + j.
//
//   k_rank_partition   key = order-preserving uint32 of (score + 0.0f); the problem's keys go into
//                      its own range [fit_row_off[f] * K + j * len, + len) of the key buffer,
//                      negatives from the front and positives from the back.  Two integer cursors
//                      per problem (out[p][0] = n_neg, out[p][1] = n_pos), advanced by one 64-bit
//                      atomic per wave and side; lanes find their slot by ballot and popcount.
//   segmented sort     LSD radix sort of every side of every problem, keys only: 4 passes of 8 bits
//                      over ping-pong buffers, each pass three launches (k_seg_hist, k_seg_scan,
//                      k_seg_scatter).  No block waits for another block: the launches are ordered
//                      by the stream alone.  dml_seg_sort_u32 exposes it for plain segments.
//   k_rank_reduce      per sorted positive two binary searches in the sorted negatives give U2
//                      (an integer: one 64-bit atomic per block), and the first of every tie group
//                      adds its term of the average precision.  AP takes no floating-point
//                      atomics: lane in order, xor-shuffle tree, the four waves ascending, block
//                      partials, k_rank_ap_reduce adds a problem's blocks in block order.
//   k_proba_stats      per fit: n, sum log p_y, the Brier sum, top-2 hits, bad; doubles in the same
//                      fixed order (k_proba_reduce), counts as integer atomics.
// ../runtime/rank_stats_cpu.cpp is the host twin (std::sort per segment; sums in this order).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "wave_ops.h"

namespace dml {

#define RS_PTR(T, v) ((T*)(__attribute__((address_space(1))) T*)(uintptr_t)(v))

constexpr int kRsTile = 4096;       // keys / entries per block: 4 waves x 16 rounds x 64 lanes
constexpr int kRsRounds = 16;
constexpr int kRsWaveKeys = kRsRounds * 64;
constexpr int kRsMaxC = 64;
constexpr int kRankSlots = 4;       // n_neg, n_pos, U2, AP (double bits)
constexpr int kProbaSlots = 5;      // n, sum log p_y (double bits), Brier sum (double bits), top-2 hits, bad
constexpr int kWantAP = 1;
constexpr int kWantLogLoss = 1, kWantBrier = 2, kWantTop2 = 4;
constexpr int64_t kMaxGridY = 65535;

struct RankStatsArgs {
  int64_t rows;         // int32 [total]
  int64_t fit_row_off;  // int64 [F + 1]
  int64_t score;        // float [total][K]
  int64_t ycls;         // int32 [n]
  int64_t n;
  int64_t C;            // classes of ycls
  int64_t K;            // score columns (rank: 1 or C; proba: C)
  int64_t pos0;         // rank: the positive class of column j is pos0 + j
  int64_t F;
  int64_t max_rows;     // entries of the longest fit
  int64_t want;
  int64_t keys;         // rank: uint32 [total * K]
  int64_t tmp;          // rank: uint32 [total * K]
  int64_t hist;         // rank: uint32 [min(2 F K, 65535)][ceil(max_rows / tile)][256]
  int64_t part;         // rank: double [F K][gx]; proba: double [F][gx][2]
  int64_t out;          // rank: 8-byte slots [F K][4]; proba: [F][5]
  int64_t bad;          // rank: int64 [F]
  int64_t phase;        // rank: 0 all; 1 partition, 2 sort, 3 reduce only (timing)
  int64_t f0;           // first fit / problem of this launch (the entry point sets it)
};

// one pass of the sort (internal)
struct SegSortArgs {
  int64_t src, dst;      // uint32 key buffers of this pass
  int64_t seg_off;       // int64 [S + 1]; 0: the segments are the two sides of rank problems
  int64_t fit_row_off;   // rank problems: as RankStatsArgs
  int64_t K;
  int64_t cur;           // rank problems: out (the cursors)
  int64_t hist;
  int64_t gx;
  int64_t s0;            // first segment of this launch
  int64_t shift;
};

__device__ __forceinline__ uint32_t rs_key(float s) {
  const uint32_t u = __builtin_bit_cast(uint32_t, s + 0.0f);   // -0.0 -> +0.0: equal scores, equal keys
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// lanes below this one whose bit is set
__device__ __forceinline__ uint32_t rs_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ uint64_t rs_ballot(bool b) { return __builtin_amdgcn_ballot_w64(b); }

// the key range of problem p, and where its fit's entries start
__device__ __forceinline__ void rs_problem(const int64_t* roff, int64_t K, int64_t p, int64_t* base, int64_t* len) {
  const int64_t f = p / K, j = p - f * K;
  const int64_t r0 = roff[f];
  *len = roff[f + 1] - r0;
  *base = r0 * K + j * *len;
}

__device__ __forceinline__ void ss_bounds(const SegSortArgs& a, int64_t s, int64_t* b, int64_t* e) {
  if (a.seg_off) {
    const int64_t* off = RS_PTR(const int64_t, a.seg_off);
    *b = off[s];
    *e = off[s + 1];
    return;
  }
  const int64_t p = s >> 1;
  int64_t base, len;
  rs_problem(RS_PTR(const int64_t, a.fit_row_off), a.K, p, &base, &len);
  const int64_t* cur = RS_PTR(const int64_t, a.cur) + p * kRankSlots;
  if (s & 1) {
    *b = base + len - cur[1];
    *e = base + len;
  } else {
    *b = base;
    *e = base + cur[0];
  }
}

__global__ __launch_bounds__(256) void k_rank_partition(RankStatsArgs a) {
  const int64_t f = a.f0 + blockIdx.y;
  const int64_t* roff = RS_PTR(const int64_t, a.fit_row_off);
  const int64_t r0 = roff[f], r1 = roff[f + 1], len = r1 - r0;
  const int64_t t0 = r0 + (int64_t)blockIdx.x * kRsTile;
  if (t0 >= r1) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t w0 = t0 + (int64_t)w * kRsWaveKeys + lane;
  const int C = (int)a.C, K = (int)a.K, pos0 = (int)a.pos0;
  int32_t tgt[kRsRounds];   // class of the entry; -1: cannot be placed; -2: past the fit's end
  uint32_t nbad = 0;
#pragma unroll
  for (int r = 0; r < kRsRounds; ++r) {
    const int64_t i = w0 + r * 64;
    int32_t t = -2;
    if (i < r1) {
      const int32_t row = RS_PTR(const int32_t, a.rows)[i];
      t = -1;
      if ((uint64_t)(int64_t)row < (uint64_t)a.n) {
        const int32_t y = RS_PTR(const int32_t, a.ycls)[row];
        if ((uint32_t)y < (uint32_t)C) t = y;
      }
      nbad += t == -1 ? 1u : 0u;
    }
    tgt[r] = t;
  }
  const float* score = RS_PTR(const float, a.score);
  for (int j = 0; j < K; ++j) {
    uint32_t key[kRsRounds];
    uint32_t side = 0;   // 2 bits per round: 1 negative, 2 positive
    uint32_t cn = 0, cp = 0;
#pragma unroll
    for (int r = 0; r < kRsRounds; ++r) {
      const int64_t i = w0 + r * 64;
      uint32_t st = 0, k = 0;
      if (tgt[r] >= 0) {
        const float s = score[i * K + j];
        if (s != s) {
          nbad += 1;
        } else {
          k = rs_key(s);
          st = tgt[r] == pos0 + j ? 2u : 1u;
        }
      }
      key[r] = k;
      side |= st << (2 * r);
      cn += (uint32_t)__popcll(rs_ballot(st == 1u));
      cp += (uint32_t)__popcll(rs_ballot(st == 2u));
    }
    unsigned long long* cur = RS_PTR(unsigned long long, a.out) + (f * K + j) * kRankSlots;
    unsigned long long bn = 0, bp = 0;
    if (lane == 0) {
      if (cn) bn = atomicAdd(cur, (unsigned long long)cn);
      if (cp) bp = atomicAdd(cur + 1, (unsigned long long)cp);
    }
    bn = wave::bcast(bn, 0);
    bp = wave::bcast(bp, 0);
    uint32_t* kb = RS_PTR(uint32_t, a.keys) + r0 * K + (int64_t)j * len;
#pragma unroll
    for (int r = 0; r < kRsRounds; ++r) {
      const uint32_t st = (side >> (2 * r)) & 3u;
      const uint64_t mn = rs_ballot(st == 1u), mp = rs_ballot(st == 2u);
      if (st == 1u) kb[(int64_t)bn + rs_below(mn)] = key[r];
      if (st == 2u) kb[len - 1 - ((int64_t)bp + rs_below(mp))] = key[r];
      bn += (unsigned long long)__popcll(mn);
      bp += (unsigned long long)__popcll(mp);
    }
  }
  nbad = wave::sum(nbad, lane);
  if (lane == 0 && nbad) atomicAdd(RS_PTR(unsigned long long, a.bad) + f, (unsigned long long)nbad);
}

// hist[segment of this launch][tile][digit]
__global__ __launch_bounds__(256) void k_seg_hist(SegSortArgs a) {
  __shared__ uint32_t h[4][256];
  int64_t b, e;
  ss_bounds(a, a.s0 + blockIdx.y, &b, &e);
  const int64_t t0 = b + (int64_t)blockIdx.x * kRsTile;
  if (t0 >= e) return;   // block-uniform: before any barrier
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) h[q][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t* src = RS_PTR(const uint32_t, a.src);
  const int64_t w0 = t0 + (int64_t)w * kRsWaveKeys + lane;
  const int shift = (int)a.shift;
  uint32_t key[kRsRounds];
#pragma unroll
  for (int r = 0; r < kRsRounds; ++r) {
    const int64_t i = w0 + r * 64;
    key[r] = i < e ? src[i] : 0u;
  }
#pragma unroll
  for (int r = 0; r < kRsRounds; ++r)
    if (w0 + r * 64 < e) atomicAdd(&h[w][(key[r] >> shift) & 255u], 1u);
  __syncthreads();
  const int d = threadIdx.x;
  RS_PTR(uint32_t, a.hist)[((int64_t)blockIdx.y * a.gx + blockIdx.x) * 256 + d] = h[0][d] + h[1][d] + h[2][d] + h[3][d];
}

// one block per segment: the tile histograms -> exclusive offsets, digit-major, then tile
__global__ __launch_bounds__(256) void k_seg_scan(SegSortArgs a) {
  __shared__ uint32_t wsum[4];
  int64_t b, e;
  ss_bounds(a, a.s0 + blockIdx.x, &b, &e);
  if (b >= e) return;
  int64_t nt = (e - b + kRsTile - 1) / kRsTile;
  if (nt > a.gx) nt = a.gx;   // only with a max_len below the longest segment: stay inside the table
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t* h = RS_PTR(uint32_t, a.hist) + (int64_t)blockIdx.x * a.gx * 256 + threadIdx.x;
  uint32_t tot = 0;
  for (int64_t t = 0; t < nt; ++t) tot += h[t * 256];
  const uint32_t incl = wave::incl_scan(tot);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  uint32_t run = incl - tot;
  for (int q = 0; q < w; ++q) run += wsum[q];
  for (int64_t t = 0; t < nt; ++t) {
    const uint32_t c = h[t * 256];
    h[t * 256] = run;
    run += c;
  }
}

// stable scatter of one tile: a key's place is its digit's offset (k_seg_scan), plus the keys of
// that digit in earlier waves of the tile, plus those in earlier rounds of its wave (the wave's
// counters in LDS), plus those in lower lanes of its round (8 ballots on the digit's bits)
__global__ __launch_bounds__(256) void k_seg_scatter(SegSortArgs a) {
  __shared__ uint32_t cnt[4][256];
  int64_t b, e;
  ss_bounds(a, a.s0 + blockIdx.y, &b, &e);
  const int64_t t0 = b + (int64_t)blockIdx.x * kRsTile;
  if (t0 >= e) return;   // block-uniform: before any barrier
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) cnt[q][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t* src = RS_PTR(const uint32_t, a.src);
  const int64_t w0 = t0 + (int64_t)w * kRsWaveKeys + lane;
  const int shift = (int)a.shift;
  uint32_t key[kRsRounds], rk[kRsRounds];
#pragma unroll
  for (int r = 0; r < kRsRounds; ++r) {
    const int64_t i = w0 + r * 64;
    key[r] = i < e ? src[i] : 0xFFFFFFFFu;
  }
  volatile uint32_t* mine = cnt[w];
#pragma unroll
  for (int r = 0; r < kRsRounds; ++r) {
    const bool valid = w0 + r * 64 < e;
    const uint32_t d = (key[r] >> shift) & 255u;
    uint64_t peers = rs_ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1u;
      const uint64_t m = rs_ballot(one);
      peers &= one ? m : ~m;
    }
    const uint32_t below = rs_below(peers);
    const uint32_t pre = mine[d];   // the wave's LDS accesses complete in program order
    if (valid && below == 0) mine[d] = pre + (uint32_t)__popcll(peers);
    rk[r] = pre + below;
  }
  __syncthreads();
  {
    const int d = threadIdx.x;
    const uint32_t o = RS_PTR(const uint32_t, a.hist)[((int64_t)blockIdx.y * a.gx + blockIdx.x) * 256 + d];
    const uint32_t c0 = cnt[0][d], c1 = cnt[1][d], c2 = cnt[2][d];
    cnt[0][d] = o;
    cnt[1][d] = o + c0;
    cnt[2][d] = o + c0 + c1;
    cnt[3][d] = o + c0 + c1 + c2;
  }
  __syncthreads();
  uint32_t* dst = RS_PTR(uint32_t, a.dst) + b;
#pragma unroll
  for (int r = 0; r < kRsRounds; ++r) {
    if (w0 + r * 64 < e) dst[cnt[w][(key[r] >> shift) & 255u] + rk[r]] = key[r];
  }
}

// first index in [lo, hi) whose key is >= v (upper = false) or > v (upper = true)
__device__ __forceinline__ int64_t rs_bound(const uint32_t* k, int64_t lo, int64_t hi, uint32_t v, bool upper) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const uint32_t x = k[mid];
    if (upper ? x <= v : x < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_rank_reduce(RankStatsArgs a, int64_t gx) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  __shared__ unsigned long long ured[4];
  const int64_t p = a.f0 + blockIdx.y;
  unsigned long long* cur = RS_PTR(unsigned long long, a.out) + p * kRankSlots;
  const int64_t n_neg = (int64_t)cur[0], n_pos = (int64_t)cur[1];
  const int64_t t0 = (int64_t)blockIdx.x * kRsTile;
  if (t0 >= n_pos) return;   // block-uniform: before any barrier
  const int64_t t1 = t0 + kRsTile < n_pos ? t0 + kRsTile : n_pos;
  int64_t base, len;
  rs_problem(RS_PTR(const int64_t, a.fit_row_off), a.K, p, &base, &len);
  const uint32_t* neg = RS_PTR(const uint32_t, a.keys) + base;
  const uint32_t* pos = neg + (len - n_pos);
  const bool want_ap = (a.want & kWantAP) != 0;
  unsigned long long u2 = 0;
  double ap = 0.0;
  for (int64_t i = t0 + threadIdx.x; i < t1; i += 256) {
    const uint32_t v = pos[i];
    const int64_t lt = rs_bound(neg, 0, n_neg, v, false);
    const int64_t le = rs_bound(neg, lt, n_neg, v, true);
    u2 += (unsigned long long)(2 * lt + (le - lt));
    if (want_ap && (i == 0 || pos[i - 1] != v)) {
      const int64_t m = rs_bound(pos, i, n_pos, v, true) - i;
      const int64_t tp = n_pos - i, fp = n_neg - lt;
      ap += (double)m / (double)n_pos * ((double)tp / (double)(tp + fp));
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u2 = wave::sum(u2, lane);
  ap = wave::sum(ap, lane);
  if (lane == 0) {
    ured[w] = u2;
    red[w] = ap;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long s = ured[0] + ured[1] + ured[2] + ured[3];
    if (s) atomicAdd(cur + 2, s);
    if (want_ap) RS_PTR(double, a.part)[p * gx + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

// out[p][3] = the problem's block partials in block order; one thread per problem
__global__ __launch_bounds__(256) void k_rank_ap_reduce(RankStatsArgs a, int64_t gx) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.F * a.K) return;
  double* out = RS_PTR(double, a.out) + p * kRankSlots;
  const int64_t n_pos = RS_PTR(const int64_t, a.out)[p * kRankSlots + 1];
  int64_t nb = (n_pos + kRsTile - 1) / kRsTile;
  if (nb > gx) nb = gx;
  const double* part = RS_PTR(const double, a.part) + p * gx;
  double acc = 0.0;
  for (int64_t b = 0; b < nb; ++b) acc += part[b];
  out[3] = acc;
}

__global__ __launch_bounds__(256) void k_proba_stats(RankStatsArgs a, int64_t gx) {
#pragma clang fp contract(off)
  __shared__ double red[4][2];
  __shared__ uint32_t cred[4][3];
  const int64_t f = a.f0 + blockIdx.y;
  const int64_t* roff = RS_PTR(const int64_t, a.fit_row_off);
  const int64_t r0 = roff[f], r1 = roff[f + 1];
  const int64_t t0 = r0 + (int64_t)blockIdx.x * kRsTile;
  if (t0 >= r1) return;   // block-uniform: before any barrier
  const int64_t t1 = t0 + kRsTile < r1 ? t0 + kRsTile : r1;
  const int C = (int)a.C;
  const bool want_log = (a.want & kWantLogLoss) != 0, want_brier = (a.want & kWantBrier) != 0,
             want_top = (a.want & kWantTop2) != 0;
  const double eps = 2.220446049250313e-16;
  double sl = 0.0, sb = 0.0;
  uint32_t cn = 0, ct = 0, cb = 0;
  for (int64_t i = t0 + threadIdx.x; i < t1; i += 256) {
    const int32_t row = RS_PTR(const int32_t, a.rows)[i];
    int32_t y = -1;
    if ((uint64_t)(int64_t)row < (uint64_t)a.n) y = RS_PTR(const int32_t, a.ycls)[row];
    if ((uint32_t)y >= (uint32_t)C) {
      cb += 1;
      continue;
    }
    const float* p = RS_PTR(const float, a.score) + i * C;
    const float py = p[y];
    int ahead = 0;
    bool nan = false;
    double br = 0.0;
    for (int k = 0; k < C; ++k) {
      const float pk = p[k];
      nan = nan || pk != pk;
      ahead += (pk > py || (pk == py && k > y)) ? 1 : 0;
      if (want_brier) {
        const double d = (double)pk - (k == y ? 1.0 : 0.0);
        br += d * d;
      }
    }
    if (nan) {
      cb += 1;
      continue;
    }
    cn += 1;
    if (want_log) sl += log(fmin(fmax((double)py, eps), 1.0 - eps));
    if (want_brier) {
      if (C == 2) {   // binary: the positive class's squared error
        const double d = (double)p[1] - (double)y;
        br = d * d;
      }
      sb += br;
    }
    if (want_top) ct += ahead < 2 ? 1u : 0u;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  sl = wave::sum(sl, lane);
  sb = wave::sum(sb, lane);
  cn = wave::sum(cn, lane);
  ct = wave::sum(ct, lane);
  cb = wave::sum(cb, lane);
  if (lane == 0) {
    red[w][0] = sl;
    red[w][1] = sb;
    cred[w][0] = cn;
    cred[w][1] = ct;
    cred[w][2] = cb;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int j = threadIdx.x;
    RS_PTR(double, a.part)[(f * gx + blockIdx.x) * 2 + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  } else if (threadIdx.x < 5) {
    const int j = threadIdx.x - 2;
    const unsigned long long s = (unsigned long long)cred[0][j] + cred[1][j] + cred[2][j] + cred[3][j];
    const int slot = j == 0 ? 0 : (j == 1 ? 3 : 4);
    if (s) atomicAdd(RS_PTR(unsigned long long, a.out) + f * kProbaSlots + slot, s);
  }
}

// out[f][1], out[f][2] = the fit's block partials in block order; one thread per (fit, sum)
__global__ __launch_bounds__(256) void k_proba_reduce(RankStatsArgs a, int64_t gx) {
#pragma clang fp contract(off)
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= a.F * 2) return;
  const int64_t f = q >> 1;
  const int j = (int)(q & 1);
  const int64_t* roff = RS_PTR(const int64_t, a.fit_row_off);
  const int64_t len = roff[f + 1] - roff[f];
  int64_t nb = len > 0 ? (len + kRsTile - 1) / kRsTile : 0;
  if (nb > gx) nb = gx;
  const double* part = RS_PTR(const double, a.part) + f * gx * 2 + j;
  double acc = 0.0;
  for (int64_t b = 0; b < nb; ++b) acc += part[b * 2];
  RS_PTR(double, a.out)[f * kProbaSlots + 1 + j] = acc;
}

// the 4 passes: keys -> tmp -> keys -> tmp -> keys
static int seg_sort_launch(SegSortArgs s, int64_t S, hipStream_t st) {
  const int64_t keys = s.src, tmp = s.dst;
  for (int pass = 0; pass < 4 && s.gx > 0; ++pass) {
    s.src = (pass & 1) ? tmp : keys;
    s.dst = (pass & 1) ? keys : tmp;
    s.shift = 8 * pass;
    for (int64_t s0 = 0; s0 < S; s0 += kMaxGridY) {   // grid.y holds at most 65535 segments
      s.s0 = s0;
      const unsigned ny = (unsigned)(S - s0 < kMaxGridY ? S - s0 : kMaxGridY);
      k_seg_hist<<<dim3((unsigned)s.gx, ny), 256, 0, st>>>(s);
      k_seg_scan<<<ny, 256, 0, st>>>(s);
      k_seg_scatter<<<dim3((unsigned)s.gx, ny), 256, 0, st>>>(s);
    }
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace dml

using namespace dml;

extern "C" {

int dml_rank_stats_sizeof_args() { return (int)sizeof(RankStatsArgs); }
int dml_rank_stats_tile() { return kRsTile; }
int dml_rank_stats_max_c() { return kRsMaxC; }

// bytes of the histogram workspace of a sort of S segments, the longest of max_len keys
int64_t dml_seg_sort_hist_bytes(int64_t S, int64_t max_len) {
  const int64_t gx = (max_len + kRsTile - 1) / kRsTile;
  return (S < kMaxGridY ? S : kMaxGridY) * gx * 256 * 4;
}

// Sorts every segment [seg_off[s], seg_off[s + 1]) of `keys` ascending, in place (`tmp`: as many
// keys; `hist`: dml_seg_sort_hist_bytes).  seg_off is device memory.  0: launched; 1: a HIP
// error; 2: bad arguments.
int dml_seg_sort_u32(void* keys, const int64_t* seg_off, int64_t S, int64_t max_len, void* tmp, void* hist,
                     hipStream_t st) {
  if (S <= 0 || max_len <= 0) return 0;
  if (!keys || !seg_off || !tmp || !hist || max_len > 2147483647LL) return 2;
  SegSortArgs s = {};
  s.src = (int64_t)(uintptr_t)keys;
  s.dst = (int64_t)(uintptr_t)tmp;
  s.seg_off = (int64_t)(uintptr_t)seg_off;
  s.hist = (int64_t)(uintptr_t)hist;
  s.gx = (max_len + kRsTile - 1) / kRsTile;
  return seg_sort_launch(s, S, st);
}

// 0: launched; 1: a HIP error; 2: bad arguments.  Zeroes `out` and `bad` itself.
int dml_rank_stats(RankStatsArgs* a, hipStream_t st) {
  if (a->F <= 0) return 0;
  if (!a->fit_row_off || !a->out || !a->bad || a->C < 2 || a->K < 1 || a->pos0 < 0 || a->max_rows < 0 || a->n < 0 ||
      a->n > 2147483647LL || a->max_rows > 2147483647LL || a->phase < 0 || a->phase > 3)
    return 2;
  const int64_t gx = (a->max_rows + kRsTile - 1) / kRsTile;
  const int64_t P = a->F * a->K;
  if (gx > 0 && (!a->rows || !a->score || !a->ycls || !a->keys || !a->tmp || !a->hist)) return 2;
  if ((a->want & kWantAP) && gx > 0 && !a->part) return 2;
  RankStatsArgs b = *a;
  if (a->phase <= 1) {
    if (hipMemsetAsync((void*)(uintptr_t)a->out, 0, (size_t)P * kRankSlots * 8, st) != hipSuccess ||
        hipMemsetAsync((void*)(uintptr_t)a->bad, 0, (size_t)a->F * 8, st) != hipSuccess)
      return 1;
    for (int64_t f0 = 0; gx > 0 && f0 < a->F; f0 += kMaxGridY) {
      b.f0 = f0;
      const dim3 grid((unsigned)gx, (unsigned)(a->F - f0 < kMaxGridY ? a->F - f0 : kMaxGridY));
      k_rank_partition<<<grid, 256, 0, st>>>(b);
    }
  }
  if (a->phase == 0 || a->phase == 2) {
    SegSortArgs s = {};
    s.src = a->keys;
    s.dst = a->tmp;
    s.fit_row_off = a->fit_row_off;
    s.K = a->K;
    s.cur = a->out;
    s.hist = a->hist;
    s.gx = gx;
    if (seg_sort_launch(s, 2 * P, st) != 0) return 1;
  }
  if (a->phase == 0 || a->phase == 3) {
    for (int64_t p0 = 0; gx > 0 && p0 < P; p0 += kMaxGridY) {
      b.f0 = p0;
      const dim3 grid((unsigned)gx, (unsigned)(P - p0 < kMaxGridY ? P - p0 : kMaxGridY));
      k_rank_reduce<<<grid, 256, 0, st>>>(b, gx);
    }
    if (a->want & kWantAP) {
      b.f0 = 0;
      k_rank_ap_reduce<<<(unsigned)((P + 255) / 256), 256, 0, st>>>(b, gx);
    }
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// 0: launched; 1: a HIP error; 2: bad arguments.  Zeroes `out` itself.
int dml_proba_stats(RankStatsArgs* a, hipStream_t st) {
  if (a->F <= 0) return 0;
  if (!a->fit_row_off || !a->out || a->C < 2 || a->C > kRsMaxC || a->K != a->C || a->max_rows < 0 || a->n < 0 ||
      a->n > 2147483647LL)
    return 2;
  const int64_t gx = (a->max_rows + kRsTile - 1) / kRsTile;
  if (gx > 2147483647LL) return 2;
  if (gx > 0 && (!a->rows || !a->score || !a->ycls || !a->part)) return 2;
  if (hipMemsetAsync((void*)(uintptr_t)a->out, 0, (size_t)a->F * kProbaSlots * 8, st) != hipSuccess) return 1;
  RankStatsArgs b = *a;
  for (int64_t f0 = 0; gx > 0 && f0 < a->F; f0 += kMaxGridY) {
    b.f0 = f0;
    const dim3 grid((unsigned)gx, (unsigned)(a->F - f0 < kMaxGridY ? a->F - f0 : kMaxGridY));
    k_proba_stats<<<grid, 256, 0, st>>>(b, gx);
  }
  b.f0 = 0;
  k_proba_reduce<<<(unsigned)((a->F * 2 + 255) / 256), 256, 0, st>>>(b, gx);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // extern "C"
