// rank_stats_cpu.cpp -- the statistics of the ranking and probability scorers on the host: the
// twin of ../kernels/rank_stats.hip (dml_rank_stats, dml_proba_stats, dml_seg_sort_u32).  Same
// arguments, one per field, same outputs.  The kernel's radix sort is replaced by std::sort per
// segment: sorted keys are unique, so the two agree bit for bit.  Every floating-point sum is
// added in the kernel's order: a lane adds its entries of the tile in order, the 64 lanes of a
// wave by the xor-shuffle tree (offsets 32 .. 1), the four waves ascending, a problem's (fit's)
// blocks in block order.  This file is built with -ffp-contract=off.  The sum of logarithms can
// differ from the kernel's by the ulps between the host's and the device's log.
// This is the CPU data path and the reference the GPU test compares against.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace {

constexpr int kTile = 4096;
constexpr int kMaxC = 64;
constexpr int kRankSlots = 4;
constexpr int kProbaSlots = 5;
constexpr int kWantAP = 1;
constexpr int kWantLogLoss = 1, kWantBrier = 2, kWantTop2 = 4;

// lane 0 of the kernel's wave sum, then the four waves ascending
inline double block_sum(double* lane) {
  for (int wv = 0; wv < 4; ++wv) {
    double* s = lane + 64 * wv;
    for (int off = 32; off >= 1; off >>= 1)
      for (int i = 0; i < off; ++i) s[i] = s[i] + s[i + off];
  }
  return ((lane[0] + lane[64]) + lane[128]) + lane[192];
}

inline uint32_t rs_key(float s) {
  const float z = s + 0.0f;   // -0.0 -> +0.0
  uint32_t u;
  memcpy(&u, &z, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

inline void put_double(int64_t* slot, double v) { memcpy(slot, &v, 8); }

}  // namespace

extern "C" {

int dml_cpu_rank_stats_tile() { return kTile; }

// sorts every segment [seg_off[s], seg_off[s + 1]) of keys ascending, in place
int dml_cpu_seg_sort_u32(uint32_t* keys, const int64_t* seg_off, int64_t S) {
  if (S <= 0) return 0;
  if (!keys || !seg_off) return 2;
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t s = 0; s < S; ++s)
    if (seg_off[s + 1] > seg_off[s]) std::sort(keys + seg_off[s], keys + seg_off[s + 1]);
  return 0;
}

// The fields of rank_stats.hip RankStatsArgs, one by one (no workspace).  out: 8-byte slots
// [F * K][4] = n_neg, n_pos, U2, AP (double bits); bad: int64 [F].  Returns 0, or 2 for arguments
// the kernel refuses too.
int dml_cpu_rank_stats(const int32_t* rows, const int64_t* fit_row_off, const float* score, const int32_t* ycls,
                       int64_t n, int64_t C, int64_t K, int64_t pos0, int64_t F, int64_t max_rows, int64_t want,
                       int64_t* out, int64_t* bad) {
  if (F <= 0) return 0;
  if (!fit_row_off || !out || !bad || C < 2 || K < 1 || pos0 < 0 || max_rows < 0 || n < 0 || n > 2147483647LL ||
      max_rows > 2147483647LL)
    return 2;
  if (max_rows > 0 && (!rows || !score || !ycls)) return 2;
  const int64_t gx = (max_rows + kTile - 1) / kTile;
  const bool want_ap = (want & kWantAP) != 0;
  memset(out, 0, (size_t)(F * K) * kRankSlots * 8);
  memset(bad, 0, (size_t)F * 8);
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t f = 0; f < F; ++f) {
    const int64_t r0 = fit_row_off[f];
    int64_t r1 = fit_row_off[f + 1];
    if (r1 > r0 + gx * kTile) r1 = r0 + gx * kTile;   // the launch's reach
    std::vector<int32_t> tgt((size_t)(r1 - r0));
    int64_t nbad = 0;
    for (int64_t i = r0; i < r1; ++i) {
      const int32_t row = rows[i];
      int32_t t = -1;
      if ((uint64_t)(int64_t)row < (uint64_t)n) {
        const int32_t y = ycls[row];
        if ((uint32_t)y < (uint32_t)C) t = y;
      }
      nbad += t < 0 ? 1 : 0;
      tgt[(size_t)(i - r0)] = t;
    }
    std::vector<uint32_t> neg, pos;
    for (int64_t j = 0; j < K; ++j) {
      neg.clear();
      pos.clear();
      for (int64_t i = r0; i < r1; ++i) {
        const int32_t t = tgt[(size_t)(i - r0)];
        if (t < 0) continue;
        const float s = score[i * K + j];
        if (s != s) {
          nbad += 1;
          continue;
        }
        (t == pos0 + j ? pos : neg).push_back(rs_key(s));
      }
      std::sort(neg.begin(), neg.end());
      std::sort(pos.begin(), pos.end());
      const int64_t n_neg = (int64_t)neg.size(), n_pos = (int64_t)pos.size();
      uint64_t u2 = 0;
      double ap = 0.0;
      for (int64_t t0 = 0; t0 < n_pos; t0 += kTile) {
        const int64_t t1 = t0 + kTile < n_pos ? t0 + kTile : n_pos;
        double lane[256];
        for (int t = 0; t < 256; ++t) {
          lane[t] = 0.0;
          for (int64_t i = t0 + t; i < t1; i += 256) {
            const uint32_t v = pos[(size_t)i];
            const int64_t lt = std::lower_bound(neg.begin(), neg.end(), v) - neg.begin();
            const int64_t le = std::upper_bound(neg.begin() + lt, neg.end(), v) - neg.begin();
            u2 += (uint64_t)(2 * lt + (le - lt));
            if (want_ap && (i == 0 || pos[(size_t)(i - 1)] != v)) {
              const int64_t m = (std::upper_bound(pos.begin() + i, pos.end(), v) - pos.begin()) - i;
              const int64_t tp = n_pos - i, fp = n_neg - lt;
              lane[t] += (double)m / (double)n_pos * ((double)tp / (double)(tp + fp));
            }
          }
        }
        if (want_ap) ap += block_sum(lane);
      }
      int64_t* o = out + (f * K + j) * kRankSlots;
      o[0] = n_neg;
      o[1] = n_pos;
      o[2] = (int64_t)u2;
      put_double(o + 3, ap);
    }
    bad[f] = nbad;
  }
  return 0;
}

// out: 8-byte slots [F][5] = n, sum log p_y (double bits), Brier sum (double bits), top-2 hits, bad
int dml_cpu_proba_stats(const int32_t* rows, const int64_t* fit_row_off, const float* score, const int32_t* ycls,
                        int64_t n, int64_t C, int64_t F, int64_t max_rows, int64_t want, int64_t* out) {
  if (F <= 0) return 0;
  if (!fit_row_off || !out || C < 2 || C > kMaxC || max_rows < 0 || n < 0 || n > 2147483647LL) return 2;
  if (max_rows > 0 && (!rows || !score || !ycls)) return 2;
  const int64_t gx = (max_rows + kTile - 1) / kTile;
  const bool want_log = (want & kWantLogLoss) != 0, want_brier = (want & kWantBrier) != 0,
             want_top = (want & kWantTop2) != 0;
  const double eps = 2.220446049250313e-16;
#pragma omp parallel for schedule(static)
  for (int64_t f = 0; f < F; ++f) {
    const int64_t r0 = fit_row_off[f], r1 = fit_row_off[f + 1];
    int64_t cn = 0, ct = 0, cb = 0;
    double asl = 0.0, asb = 0.0;
    for (int64_t b = 0; b < gx; ++b) {
      const int64_t t0 = r0 + b * kTile, t1 = t0 + kTile < r1 ? t0 + kTile : r1;
      if (t0 >= r1) break;
      double sl[256], sb[256];
      for (int t = 0; t < 256; ++t) {
        sl[t] = 0.0;
        sb[t] = 0.0;
        for (int64_t i = t0 + t; i < t1; i += 256) {
          const int32_t row = rows[i];
          int32_t y = -1;
          if ((uint64_t)(int64_t)row < (uint64_t)n) y = ycls[row];
          if ((uint32_t)y >= (uint32_t)C) {
            cb += 1;
            continue;
          }
          const float* p = score + i * C;
          const float py = p[y];
          int ahead = 0;
          bool nan = false;
          double br = 0.0;
          for (int k = 0; k < (int)C; ++k) {
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
          if (want_log) sl[t] += log(fmin(fmax((double)py, eps), 1.0 - eps));
          if (want_brier) {
            if (C == 2) {
              const double d = (double)p[1] - (double)y;
              br = d * d;
            }
            sb[t] += br;
          }
          if (want_top) ct += ahead < 2 ? 1 : 0;
        }
      }
      asl += block_sum(sl);
      asb += block_sum(sb);
    }
    int64_t* o = out + f * kProbaSlots;
    o[0] = cn;
    put_double(o + 1, asl);
    put_double(o + 2, asb);
    o[3] = ct;
    o[4] = cb;
  }
  return 0;
}

}  // extern "C"
