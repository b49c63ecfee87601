// qda_args.h -- argument blocks of csrc/kernels/qda.hip and its host twin
// csrc/runtime/qda_cpu.cpp (docs/QDA.md).  Every field is an int64 (pointers as integers), the
// layout utils/native.py mirrors with ctypes.
#pragma once
#include <stdint.h>

namespace dml {

// Per-cell moments of z = [x - shift, 1]: a cell is one (fold bucket, class) pair, its rows are
// perm[cell_off[cell] .. cell_off[cell + 1]).
struct QdaMomArgs {
  int64_t X, ld, n, d;      // float32 [n, ld] table, d <= ld columns used
  int64_t shift;            // float64 [d]
  int64_t perm;             // int32 [n]: row ids grouped by cell
  int64_t cell_off;         // int64 [n_cells + 1]
  int64_t n_cells;
  int64_t parts;            // row partitions of a cell (1..kQdaMaxParts): partition p takes slabs p, p + parts, ...
  int64_t part;             // float64 [n_cells, parts, Dp, Dp] workspace, Dp = roundup(d + 1, 16)
  int64_t out;              // float64 [n_cells, Dp, Dp]: tiles with ti <= tj hold the moments, the rest 0
};

// Decision values and predictions of every held-out row of S splits for NC candidates.
struct QdaScoreArgs {
  int64_t X, ld, n, d;
  int64_t rows;             // int32 [total_rows]: the splits' held-out rows, split after split
  int64_t row_off;          // int64 [S + 1] offsets into rows
  int64_t S, max_rows;      // max_rows: the longest split's row count (sizes the grid)
  int64_t total_rows;
  int64_t C, NC;
  int64_t mu;               // float64 [S, C, d] class means
  int64_t V;                // float64 [S, C, d, d]: V[k][j], column j = component j (dropped ones 0)
  int64_t inv;              // float64 [S, NC, C, d]: 1 / variance of component j (dropped ones 0)
  int64_t cst;              // float64 [S, NC, C]: -0.5 sum log variance + log prior
  int64_t pred;             // int32 [NC, total_rows]
  int64_t dec;              // float64 [NC, total_rows, C] or 0
};

constexpr int kQdaOk = 0, kQdaHipError = 1, kQdaBadArgs = 2, kQdaTooLarge = 3;
constexpr int kQdaMaxD = 128;        // features of one launch (both kernels)
constexpr int kQdaMaxCand = 32;      // candidates of one scoring launch
constexpr int kQdaMaxParts = 16;
constexpr int kQdaSlabRows = 32;     // rows of one LDS slab of the moments kernel
constexpr int kQdaRowTile = 32;      // held-out rows of one scoring workgroup

}  // namespace dml
