// lda_args.h -- argument blocks of csrc/kernels/lda.hip (docs/LDA.md).  Every field is an int64
// (pointers as integers), the layout utils/native.py mirrors with ctypes.
#pragma once
#include <stdint.h>

namespace dml {

// Ledoit-Wolf row statistic.  A cell is one (fold bucket, class) pair, cell = bucket * C + class,
// its rows are perm[cell_off[cell] .. cell_off[cell + 1]) (the grouping of QdaMomArgs).
// stat[cell][s] = sum over the cell's rows of q^2, q = sum_j w[s][class][j] (x_j - mean[s][class][j])^2,
// for the splits s whose train[bucket][s] is non-zero; 0 for the others.
struct LdaStatArgs {
  int64_t X, ld, n, d;      // float32 [n, ld] table, d <= ld columns used
  int64_t perm;             // int32 [n]: row ids grouped by cell
  int64_t cell_off;         // int64 [n_cells + 1]
  int64_t n_cells, C;       // n_cells is a multiple of C
  int64_t train;            // int32 [n_cells / C, S]
  int64_t S;                // splits of this launch (1..kLdaMaxSplits)
  int64_t mean, w;          // float64 [S, C, d]
  int64_t parts;            // row partitions of a cell (1..kLdaMaxParts): partition p takes row blocks p, p + parts, ...
  int64_t part;             // float64 [n_cells, parts, S] workspace
  int64_t out;              // float64 [n_cells, S]
};

// Linear scores and predictions of every held-out row of S splits for NC candidates:
// dec[cand][row][c] = W[s][c][cand] . x + b[s][c][cand].
struct LdaScoreArgs {
  int64_t X, ld, n, d;
  int64_t rows;             // int32 [total_rows]: the splits' held-out rows, split after split
  int64_t row_off;          // int64 [S + 1] offsets into rows
  int64_t S, max_rows;      // max_rows: the longest split's row count (sizes the grid)
  int64_t total_rows;
  int64_t C, NC, NCp;       // NCp: NC padded to a power of two (1, 2, 4, 8 or 16)
  int64_t W;                // float64 [S, C, NCp, d]
  int64_t b;                // float64 [S, C, NCp]
  int64_t pred;             // int32 [NC, total_rows]
  int64_t dec;              // float64 [NC, total_rows, C] or 0
};

constexpr int kLdaOk = 0, kLdaHipError = 1, kLdaBadArgs = 2, kLdaTooLarge = 3;
constexpr int kLdaMaxD = 128;        // features of one launch (both kernels)
constexpr int kLdaMaxCand = 16;      // candidates of one scoring launch
constexpr int kLdaMaxSplits = 16;    // splits of one statistic launch
constexpr int kLdaMaxParts = 16;
constexpr int kLdaRowTile = 64;      // held-out rows of one scoring workgroup

}  // namespace dml
