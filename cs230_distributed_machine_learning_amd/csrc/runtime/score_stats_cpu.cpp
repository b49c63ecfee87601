// score_stats_cpu.cpp -- per-fit score statistics on the host: the twin of
// ../kernels/score_stats.hip (dml_fit_stats).  Same arguments, one per field, same outputs, and
// the same order of every floating-point sum: a lane adds its entries of the tile in order, the 64
// lanes of a wave are added by the xor-shuffle tree (offsets 32 .. 1), the four waves ascending,
// and a fit's blocks in block order -- so the counts and the sums of slots 0-6 agree with the
// kernel's to the last bit (this file is built with -ffp-contract=off; the kernel turns
// contraction off for the same terms).  The slots that divide or take logarithms differ from the
// kernel's only by the ulps between the host's and the device's division / log / log1p.
// This is the CPU data path and the reference the GPU test compares against.
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace {

constexpr int kTile = 4096;
constexpr int kMaxC = 64;
constexpr int kRegSlots = 14;
constexpr int kWantLog = 1, kWantPoisson = 2, kWantGamma = 4;

// lane 0 of the kernel's wave sum, then the four waves ascending
inline double block_sum(double* lane) {
  for (int wv = 0; wv < 4; ++wv) {
    double* s = lane + 64 * wv;
    for (int off = 32; off >= 1; off >>= 1)
      for (int i = 0; i < off; ++i) s[i] = s[i] + s[i + off];
  }
  return ((lane[0] + lane[64]) + lane[128]) + lane[192];
}

inline double block_max(const double* lane) {
  double m = 0.0;
  for (int t = 0; t < 256; ++t) m = fmax(m, lane[t]);
  return m;
}

}  // namespace

extern "C" {

int dml_cpu_fit_stats_tile() { return kTile; }

// The fields of score_stats.hip FitStatsArgs, one by one (part may be null: the block partials
// are added as they are produced).  Returns 0, or 2 for arguments the kernel refuses too.
int dml_cpu_fit_stats(const int32_t* rows, const int64_t* fit_row_off, const void* pred, const int32_t* ycls,
                      const float* yreg, int64_t n, int64_t C, int64_t F, int64_t max_rows, int64_t want,
                      double* part, void* out) {
  if (F <= 0) return 0;
  if (!fit_row_off || !out || C < 0 || C > kMaxC || C == 1 || max_rows < 0 || n < 0 || n > 2147483647LL) return 2;
  if (max_rows > 0 && (!rows || !pred || !(C ? (const void*)ycls : (const void*)yreg))) return 2;
  const int64_t gx = (max_rows + kTile - 1) / kTile;
  if (C > 0) {
    const int64_t CC = C * C;
    int64_t* o = (int64_t*)out;
    memset(o, 0, (size_t)F * (size_t)(CC + 1) * 8);
    const int32_t* p = (const int32_t*)pred;
#pragma omp parallel for schedule(static)
    for (int64_t f = 0; f < F; ++f) {
      int64_t* of = o + f * (CC + 1);
      int64_t r1 = fit_row_off[f + 1];
      if (r1 > fit_row_off[f] + gx * kTile) r1 = fit_row_off[f] + gx * kTile;   // the launch's reach
      for (int64_t i = fit_row_off[f]; i < r1; ++i) {
        const int32_t row = rows[i], pv = p[i];
        int64_t cell = -1;
        if ((uint64_t)(int64_t)row < (uint64_t)n) {
          const int32_t t = ycls[row];
          if ((uint32_t)t < (uint32_t)C && (uint32_t)pv < (uint32_t)C) cell = (int64_t)t * C + pv;
        }
        of[cell >= 0 ? cell : CC] += 1;
      }
    }
    return 0;
  }
  const float* p = (const float*)pred;
  double* o = (double*)out;
  const bool want_log = (want & kWantLog) != 0, want_poi = (want & kWantPoisson) != 0,
             want_gam = (want & kWantGamma) != 0;
#pragma omp parallel for schedule(static)
  for (int64_t f = 0; f < F; ++f) {
    const int64_t r0 = fit_row_off[f], r1 = fit_row_off[f + 1];
    double acc[kRegSlots];
    for (int j = 0; j < kRegSlots; ++j) acc[j] = 0.0;
    for (int64_t b = 0; b < gx; ++b) {
      const int64_t t0 = r0 + b * kTile, t1 = t0 + kTile < r1 ? t0 + kTile : r1;
      if (t0 >= r1) break;
      double s[kRegSlots][256];
      for (int j = 0; j < kRegSlots; ++j)
        for (int t = 0; t < 256; ++t) s[j][t] = 0.0;
      for (int t = 0; t < 256; ++t) {
        for (int64_t i = t0 + t; i < t1; i += 256) {
          const int32_t row = rows[i];
          if ((uint64_t)(int64_t)row >= (uint64_t)n) continue;
          const double y = (double)yreg[row], pv = (double)p[i];
          const double e = pv - y, ae = fabs(e);
          s[0][t] += 1.0;
          s[1][t] += y;
          s[2][t] += y * y;
          s[3][t] += e;
          s[4][t] += e * e;
          s[5][t] += ae;
          s[6][t] = fmax(s[6][t], ae);
          s[7][t] += ae / fmax(fabs(y), 2.220446049250313e-16);
          const bool bad_log = y <= -1.0 || pv <= -1.0, bad_poi = y < 0.0 || pv <= 0.0,
                     bad_gam = y <= 0.0 || pv <= 0.0;
          s[9][t] += bad_log ? 1.0 : 0.0;
          s[11][t] += bad_poi ? 1.0 : 0.0;
          s[13][t] += bad_gam ? 1.0 : 0.0;
          if (want_log && !bad_log) {
            const double d = log1p(y) - log1p(pv);
            s[8][t] += d * d;
          }
          if (want_poi && !bad_poi) {
            const double xl = y > 0.0 ? y * log(y / pv) : 0.0;
            s[10][t] += 2.0 * (xl - y + pv);
          }
          if (want_gam && !bad_gam) s[12][t] += 2.0 * (log(pv / y) + y / pv - 1.0);
        }
      }
      for (int j = 0; j < kRegSlots; ++j) {
        const double v = j == 6 ? block_max(s[j]) : block_sum(s[j]);
        if (part) part[(f * gx + b) * kRegSlots + j] = v;
        acc[j] = j == 6 ? fmax(acc[j], v) : acc[j] + v;
      }
    }
    for (int j = 0; j < kRegSlots; ++j) o[f * kRegSlots + j] = acc[j];
  }
  return 0;
}

}  // extern "C"
