// svm_args.h -- records shared by the SVM kernels (svm.hip, svm_decision.hip) and their host
// twins (../runtime/svm_cpu.cpp).  Every field is 64 bits wide (pointers as integers), as the
// other argument blocks.
#pragma once
#include <stdint.h>

namespace dml {

enum { KLIN = 0, KPOLY = 1, KRBF = 2, KSIG = 3 };

// one dual problem
struct SvmProb {
  int64_t xoff;      // feature-major rows of this problem's rowset: X[xoff + f * nrows + r]
  int64_t roff;      // per-row arrays (qd, sv_idx, sv_coef): at [roff, roff + nrows)
  int64_t nrows;     // rows in the rowset
  int64_t L;         // dual variables (nrows for SVC, 2 nrows for epsilon-SVR)
  int64_t voff;      // per-variable arrays: y, C, alpha, G at [voff, voff + L)
  int64_t koff;      // kernel-column scratch: 2 * nrows floats at koff
  int64_t kernel, degree;
  double gamma, coef0, eps;
  int64_t max_iter;  // total iteration budget
  int64_t iters;     // in/out: iterations done so far
  int64_t status;    // in/out: 0 running, 1 optimal, 2 iteration limit
  int64_t svr;       // 1: variable t uses row t mod nrows
  int64_t coff;      // split solver: kernel-column cache, S * nrows floats at coff
  int64_t moff;      // split solver: per-workgroup cache maps, B * (nrows + 2 S) ints at moff
};

// post-solve phase (svm_decision.hip): rho + support-vector compaction, decision values, votes
struct SvmDecArgs {
  int64_t probs;     // const SvmProb [nprob]
  int64_t nprob;
  int64_t y;         // const float  [sum L]
  int64_t C;         // const double [sum L]
  int64_t alpha;     // const double [sum L]
  int64_t G;         // const double [sum L]
  int64_t sv_idx;    // int32  [sum nrows]  rho_sv out: ascending rowset positions with coef != 0, at roff
  int64_t sv_coef;   // double [sum nrows]  rho_sv out: their coefficients, at roff
  int64_t rho;       // double [nprob]      rho_sv out
  int64_t nsv;       // int32  [nprob]      rho_sv out
  int64_t Xrs;       // const float: the problems' feature-major rowset blocks (SvmProb::xoff)
  int64_t X;         // const float [n][d]: the row-major table the query rows come from
  int64_t d;
  int64_t work;      // const int32 [nwork][2]: (problem, query tile) per workgroup
  int64_t nwork;
  int64_t qinfo;     // const int64 [nprob][2]: (qoff, qn) of each problem in qrows / opos
  int64_t qrows;     // const int64: table row of every query
  int64_t opos;      // const int64: slot of every query's decision value in out
  int64_t out;       // double: decision values
  // votes: one thread per (fit, test row)
  int64_t fit_tab;   // const int64 [F][2]: (test rows m, offset of the fit's predictions in pred)
  int64_t pair_off;  // const int64 [F][n_classes (n_classes - 1) / 2]: offset of the pair's m values in out, < 0: no machine
  int64_t F, n_classes, max_m;
  int64_t pred;      // int32: voted class (first maximum)
};

constexpr int kSvmDecOk = 0;
constexpr int kSvmDecHipError = 1;
constexpr int kSvmDecBadArgs = 2;

// work split of k_svm_decision, mirrored by the host twin's summation order
constexpr int kSvmDecNT = 256;   // lanes of a workgroup; lane t owns support vectors t, t + 256, ...
constexpr int kSvmDecQT = 8;     // query rows per workgroup
constexpr int kSvmDecFC = 256;   // features staged in LDS at a time

}  // namespace dml
