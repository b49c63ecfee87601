// rank_stats_selftest.cpp -- ../runtime/rank_stats_cpu.cpp under AddressSanitizer / UBSan
// (build.py build_rank_selftest; tests/test_rank_stats_selftest.py runs it as a plain executable).
// The statistics are checked against direct O(n^2) counts: an empty fit, a one-sided fit, a fit
// longer than a tile, K = 3 columns, a bad row id and a NaN score, and the segmented sort.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

extern "C" {
int dml_cpu_rank_stats_tile();
int dml_cpu_seg_sort_u32(uint32_t* keys, const int64_t* seg_off, int64_t S);
int dml_cpu_rank_stats(const int32_t* rows, const int64_t* fit_row_off, const float* score, const int32_t* ycls,
                       int64_t n, int64_t C, int64_t K, int64_t pos0, int64_t F, int64_t max_rows, int64_t want,
                       int64_t* out, int64_t* bad);
int dml_cpu_proba_stats(const int32_t* rows, const int64_t* fit_row_off, const float* score, const int32_t* ycls,
                        int64_t n, int64_t C, int64_t F, int64_t max_rows, int64_t want, int64_t* out);
}

namespace {

int failures = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

uint32_t rng_state = 12345u;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

double as_double(int64_t v) {
  double d;
  memcpy(&d, &v, 8);
  return d;
}

// direct statistics of one (fit, column)
void direct(const std::vector<float>& s, const std::vector<int>& lab, int64_t* n_neg, int64_t* n_pos, uint64_t* u2,
            double* ap) {
  *n_neg = *n_pos = 0;
  *u2 = 0;
  for (size_t i = 0; i < s.size(); ++i) (lab[i] ? *n_pos : *n_neg) += 1;
  double acc = 0.0;
  for (size_t i = 0; i < s.size(); ++i) {
    if (!lab[i]) continue;
    int64_t tp = 0, fp = 0, m = 0;
    bool first = true;   // the first positive with this score, in index order, carries the term
    for (size_t q = 0; q < s.size(); ++q) {
      if (!lab[q]) {
        if (s[q] < s[i]) *u2 += 2;
        else if (s[q] == s[i]) *u2 += 1;
        if (s[q] >= s[i]) ++fp;
      } else {
        if (s[q] >= s[i]) ++tp;
        if (s[q] == s[i]) {
          ++m;
          if (q < i) first = false;
        }
      }
    }
    if (first) acc += (double)m / (double)*n_pos * ((double)tp / (double)(tp + fp));
  }
  *ap = acc;
}

void test_sort() {
  const int tile = dml_cpu_rank_stats_tile();
  const int64_t lens[] = {0, 1, 2, 65, tile + 1};
  std::vector<int64_t> off(1, 0);
  for (int64_t l : lens) off.push_back(off.back() + l);
  std::vector<uint32_t> keys((size_t)off.back() + 3);   // three keys past the last segment stay put
  for (auto& k : keys) k = rnd() * 977u;
  std::vector<uint32_t> ref = keys;
  for (size_t s = 0; s + 1 < off.size(); ++s) std::sort(ref.begin() + off[s], ref.begin() + off[s + 1]);
  CHECK(dml_cpu_seg_sort_u32(keys.data(), off.data(), (int64_t)off.size() - 1) == 0);
  CHECK(keys == ref);
  CHECK(dml_cpu_seg_sort_u32(nullptr, off.data(), 0) == 0);
}

void test_rank(int K) {
  const int tile = dml_cpu_rank_stats_tile();
  const int C = K == 1 ? 2 : K, pos0 = K == 1 ? 1 : 0;
  const int64_t n = 300;
  std::vector<int32_t> y((size_t)n);
  for (auto& v : y) v = (int32_t)(rnd() % (uint32_t)C);
  // fits: empty, one-sided (only class 0), mixed, longer than a tile
  const int64_t lens[] = {0, 20, 130, tile + 77};
  const int F = 4;
  std::vector<int64_t> off(1, 0);
  for (int64_t l : lens) off.push_back(off.back() + l);
  const int64_t total = off.back();
  std::vector<int32_t> rows((size_t)total);
  for (int64_t i = 0; i < total; ++i) {
    int32_t r = (int32_t)(rnd() % (uint32_t)n);
    if (i >= off[1] && i < off[2])
      while (y[(size_t)r] != 0) r = (r + 1) % (int32_t)n;
    rows[(size_t)i] = r;
  }
  std::vector<float> score((size_t)(total * K));
  for (auto& v : score) v = (float)((int)(rnd() % 21u) - 10) / 10.0f;   // ties, both signs
  score[(size_t)(off[2] * K)] = -0.0f;
  score[(size_t)((off[2] + 1) * K)] = 0.0f;
  std::vector<int64_t> out((size_t)(F * K * 4)), bad((size_t)F);
  int64_t max_rows = 0;
  for (int64_t l : lens) max_rows = std::max(max_rows, l);
  CHECK(dml_cpu_rank_stats(rows.data(), off.data(), score.data(), y.data(), n, C, K, pos0, F, max_rows, 1, out.data(),
                           bad.data()) == 0);
  for (int f = 0; f < F; ++f) {
    CHECK(bad[(size_t)f] == 0);
    for (int j = 0; j < K; ++j) {
      std::vector<float> s;
      std::vector<int> lab;
      for (int64_t i = off[(size_t)f]; i < off[(size_t)f + 1]; ++i) {
        s.push_back(score[(size_t)(i * K + j)]);
        lab.push_back(y[(size_t)rows[(size_t)i]] == pos0 + j);
      }
      int64_t n_neg, n_pos;
      uint64_t u2;
      double ap;
      direct(s, lab, &n_neg, &n_pos, &u2, &ap);
      const int64_t* o = out.data() + (f * K + j) * 4;
      CHECK(o[0] == n_neg && o[1] == n_pos && (uint64_t)o[2] == u2);
      CHECK(fabs(as_double(o[3]) - ap) <= 1e-12 * fabs(ap));
      if (f == 0) CHECK(n_neg == 0 && n_pos == 0);
      if (f == 1 && K == 1) CHECK(n_pos == 0 && n_neg == 20);
    }
  }
  // a bad row id and a NaN score are counted for their fit and not placed
  std::vector<int32_t> rows2 = rows;
  std::vector<float> score2 = score;
  rows2[(size_t)off[2] + 5] = (int32_t)n;
  rows2[(size_t)off[3] + 9] = -1;
  score2[(size_t)((off[3] + 11) * K)] = NAN;
  CHECK(dml_cpu_rank_stats(rows2.data(), off.data(), score2.data(), y.data(), n, C, K, pos0, F, max_rows, 0, out.data(),
                           bad.data()) == 0);
  CHECK(bad[0] == 0 && bad[1] == 0 && bad[2] == 1 && bad[3] == 2);
  CHECK(out[(size_t)(2 * K * 4)] + out[(size_t)(2 * K * 4 + 1)] == lens[2] - 1);
  CHECK(dml_cpu_rank_stats(rows.data(), off.data(), score.data(), y.data(), n, 1, K, pos0, F, max_rows, 0, out.data(),
                           bad.data()) == 2);
}

void test_proba(int C) {
  const int tile = dml_cpu_rank_stats_tile();
  const int64_t n = 200;
  std::vector<int32_t> y((size_t)n);
  for (auto& v : y) v = (int32_t)(rnd() % (uint32_t)C);
  const int64_t lens[] = {0, 3, tile + 5};
  const int F = 3;
  std::vector<int64_t> off(1, 0);
  for (int64_t l : lens) off.push_back(off.back() + l);
  const int64_t total = off.back();
  std::vector<int32_t> rows((size_t)total);
  for (auto& r : rows) r = (int32_t)(rnd() % (uint32_t)n);
  std::vector<float> p((size_t)(total * C));
  for (int64_t i = 0; i < total; ++i) {
    float sum = 0.0f;
    for (int k = 0; k < C; ++k) sum += (p[(size_t)(i * C + k)] = (float)(rnd() % 5u));   // ties and zeros
    for (int k = 0; k < C; ++k) p[(size_t)(i * C + k)] = sum > 0 ? p[(size_t)(i * C + k)] / sum : 1.0f / (float)C;
  }
  std::vector<int64_t> out((size_t)(F * 5));
  CHECK(dml_cpu_proba_stats(rows.data(), off.data(), p.data(), y.data(), n, C, F, tile + 5, 7, out.data()) == 0);
  const double eps = 2.220446049250313e-16;
  for (int f = 0; f < F; ++f) {
    double sl = 0.0, sb = 0.0;
    int64_t top = 0;
    for (int64_t i = off[(size_t)f]; i < off[(size_t)f + 1]; ++i) {
      const int t = y[(size_t)rows[(size_t)i]];
      const float* pi = p.data() + i * C;
      sl += log(std::min(std::max((double)pi[t], eps), 1.0 - eps));
      int ahead = 0;
      double br = 0.0;
      for (int k = 0; k < C; ++k) {
        ahead += pi[k] > pi[t] || (pi[k] == pi[t] && k > t);
        const double d = (double)pi[k] - (k == t);
        br += d * d;
      }
      if (C == 2) br = ((double)pi[1] - t) * ((double)pi[1] - t);
      sb += br;
      top += ahead < 2;
    }
    const int64_t* o = out.data() + f * 5;
    CHECK(o[0] == lens[f] && o[3] == top && o[4] == 0);
    CHECK(fabs(as_double(o[1]) - sl) <= 1e-12 * fabs(sl));
    CHECK(fabs(as_double(o[2]) - sb) <= 1e-12 * fabs(sb));
  }
  rows[(size_t)off[2] + 1] = (int32_t)n + 7;
  CHECK(dml_cpu_proba_stats(rows.data(), off.data(), p.data(), y.data(), n, C, F, tile + 5, 0, out.data()) == 0);
  CHECK(out[2 * 5 + 4] == 1 && out[2 * 5] == lens[2] - 1 && out[1 * 5 + 4] == 0);
}

}  // namespace

int main() {
  test_sort();
  test_rank(1);
  test_rank(3);
  test_proba(2);
  test_proba(3);
  if (failures) {
    fprintf(stderr, "rank stats selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("rank stats selftest ok\n");
  return 0;
}
