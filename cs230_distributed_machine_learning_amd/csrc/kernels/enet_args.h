// enet_args.h -- argument block shared by the batched Gram coordinate-descent solver
// (enet.hip dml_enet_cd) and its host twin (../runtime/enet_cpu.cpp dml_cpu_enet_cd).
// Every field is 64 bits wide (pointers as integers), as the other argument blocks.
#pragma once
#include <stdint.h>

namespace dml {

struct EnetArgs {
  int64_t Q;         // const double [G][d][d]  Gram matrices X^T X (row-major, symmetric)
  int64_t q;         // const double [G][d]     X^T y
  int64_t ynorm2;    // const double [G]        y^T y
  int64_t gram_id;   // const int32  [F]        Gram of every problem
  int64_t l1;        // const double [F]        alpha * l1_ratio * n_train
  int64_t l2;        // const double [F]        alpha * (1 - l1_ratio) * n_train
  int64_t positive;  // const int32  [F]
  int64_t max_iter;  // const int32  [F]
  int64_t tol;       // const double [F]        the unscaled tolerance
  int64_t w;         // double [F][d]           out: coefficients (started from 0)
  int64_t gap;       // double [F]              out: last duality gap
  int64_t tol_eff;   // double [F]              out: tol * ynorm2
  int64_t n_iter;    // int32  [F]              out: sweeps run
  int64_t F, d, G;
};

// return codes of both entries
constexpr int kEnetOk = 0;
constexpr int kEnetHipError = 1;
constexpr int kEnetBadArgs = 2;
constexpr int kEnetDTooLarge = 3;   // one problem's H and w do not fit a workgroup's LDS (device entry only)

}  // namespace dml
