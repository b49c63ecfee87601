// gbrt_stats_cpu.cpp -- per-stage loss / score statistics of gradient-boosting fits on the host:
// the twin of ../kernels/gbrt.hip k_gb_stage_stats / k_gb_stage_stats_reduce.  Same definition,
// same outputs (the block partials included) and the same order of every floating-point sum: a
// block's 256 terms are added as the kernel adds them (the xor-shuffle tree over the 64 lanes of
// a wave, then the four waves ascending) and the blocks as the kernel's reduction adds them (16
// at a time in block order, level by level), so the counts and the squared-error sums agree with
// the kernel's to the last bit (this file is built with -ffp-contract=off; the kernel turns
// contraction off for the same terms).  The loss sums differ from the kernel's only by the ulps
// between the host's and the device's exp / log / log1p.
// This is the CPU data path and the reference the GPU test compares against.
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace {

enum GbLoss : int32_t { kGbSq = 0, kGbAbs = 1, kGbHuber = 2, kGbQuant = 3, kGbLog = 4, kGbExp = 5 };

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

inline uint64_t bits(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  return u;
}

inline double from_bits(uint64_t u) {
  double v;
  memcpy(&v, &u, 8);
  return v;
}

}  // namespace

extern "C" {

// The arguments of gbrt.hip GbStatsArgs, one by one (val / delta may be null).
void dml_cpu_gbrt_stage_stats(int64_t n, int64_t K, int64_t A, const double* raw, const int32_t* ycls,
                              const double* yreg, const uint8_t* roles, const uint8_t* inbag, const uint8_t* val,
                              const int32_t* fit_raw, const int32_t* fit_loss, const int32_t* fit_role,
                              const int32_t* fit_inbag, const int32_t* fit_val, const int32_t* fit_out,
                              const int32_t* fit_dpos, const double* fit_alpha, const double* delta, uint64_t* part,
                              uint64_t* stats, int64_t stage, int64_t n_stages) {
  if (A <= 0 || n <= 0) return;
  const int64_t blocks = (n + 255) / 256, E = A * 9;
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t b = 0; b < blocks; ++b) {
    for (int64_t fa = 0; fa < A; ++fa) {
      double ls[3][256], ss[3][256];
      long long cnt[3] = {0, 0, 0}, hit[3] = {0, 0, 0};
      for (int c = 0; c < 3; ++c)
        for (int t = 0; t < 256; ++t) { ls[c][t] = 0.0; ss[c][t] = 0.0; }
      const int loss = fit_loss[fa];
      const bool is_cls = loss == kGbLog || loss == kGbExp;
      const int vrow = val ? fit_val[fa] : -1;
      for (int t = 0; t < 256; ++t) {
        const int64_t r = b * 256 + t;
        if (r >= n) break;
        const uint8_t role = roles[(int64_t)fit_role[fa] * n + r];
        const bool isval = vrow >= 0 && val[(int64_t)vrow * n + r] != 0;
        int cat = -1;
        if (role == 2) cat = 2;
        else if (role == 1 && !isval) cat = inbag[(int64_t)fit_inbag[fa] * n + r] ? 0 : 1;
        if (cat < 0) continue;
        const double* rw = raw + (int64_t)fit_raw[fa] * n + r;
        double term, se = 0.0;
        bool match = false;
        if (!is_cls) {
          const double dl = delta ? delta[fit_dpos[fa]] : 0.0, al = fit_alpha[fa];
          const double x = rw[0], y = yreg[r];
          const double e = x - y;
          se = e * e;
          const double d = y - x, ad = fabs(d);
          if (loss == kGbSq) term = 0.5 * d * d;
          else if (loss == kGbAbs) term = ad;
          else if (loss == kGbQuant) term = d >= 0.0 ? al * d : (al - 1.0) * d;
          else term = ad <= dl ? 0.5 * d * d : dl * (ad - 0.5 * dl);
        } else {
          const int y = ycls[r];
          if (K == 1) {
            const double z = rw[0];
            match = (z >= 0.0 ? 1 : 0) == y;
            if (loss == kGbExp) term = exp(y ? -z : z);
            else term = fmax(z, 0.0) + log1p(exp(-fabs(z))) - (y ? z : 0.0);
          } else {
            double mx = -INFINITY, ry = 0.0, s = 0.0;
            int arg = 0;
            for (int64_t k = 0; k < K; ++k) {
              const double v = rw[k * n];
              if (v > mx) { mx = v; arg = (int)k; }   // strict: the first maximum
              if (k == y) ry = v;
            }
            for (int64_t k = 0; k < K; ++k) s += exp(rw[k * n] - mx);
            match = arg == y;
            term = (mx + log(s)) - ry;
          }
        }
        ls[cat][t] = term;
        ss[cat][t] = se;
        cnt[cat] += 1;
        hit[cat] += match ? 1 : 0;
      }
      uint64_t* out = part + (b * A + fa) * 9;
      for (int c = 0; c < 3; ++c) {
        out[3 * c] = (uint64_t)cnt[c];
        out[3 * c + 1] = is_cls ? (uint64_t)hit[c] : bits(block_sum(ss[c]));
        out[3 * c + 2] = bits(block_sum(ls[c]));
      }
    }
  }
  // the kernel's reduction: groups of 16 added in order, level by level, each level's sums
  // behind the previous one's in part, until one group is left
  const uint64_t* in = part;
  uint64_t* next = part + blocks * E;
  for (int64_t n_in = blocks;;) {
    const int64_t groups = (n_in + 15) / 16;
    for (int64_t g = 0; g < groups; ++g) {
      const int64_t b0 = g * 16, b1 = b0 + 16 < n_in ? b0 + 16 : n_in;
      for (int64_t j = 0; j < E; ++j) {
        const int64_t fa = j / 9;
        const int q = (int)(j % 3);
        const int loss = fit_loss[fa];
        const bool as_int = q == 0 || (q == 1 && (loss == kGbLog || loss == kGbExp));
        uint64_t res;
        if (as_int) {
          long long acc = 0;
          for (int64_t b = b0; b < b1; ++b) acc += (long long)in[b * E + j];
          res = (uint64_t)acc;
        } else {
          double acc = 0.0;
          for (int64_t b = b0; b < b1; ++b) acc += from_bits(in[b * E + j]);
          res = bits(acc);
        }
        if (groups == 1) stats[((int64_t)fit_out[fa] * n_stages + stage) * 9 + j % 9] = res;
        else next[g * E + j] = res;
      }
    }
    if (groups == 1) break;
    in = next;
    next += groups * E;
    n_in = groups;
  }
}

}  // extern "C"
