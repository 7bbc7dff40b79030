// nmf_shapes.h — what nmf.hip (entry points, LDS-history sizing) and nmf_kernels.inc (the launchers of one rank and storage
// type) must agree on: the arguments of one launch and the table of register footprints.
#pragma once
#include "fz_common.h"

namespace fz {

struct NmfArgs {
  const void *x;            // matrices: storage type of the launcher (FZ_AT)
  const float *u0, *v0;
  const void *gy;           // FZ_AT
  const float *gu, *gv;
  void *y;                  // FZ_AT
  float *uo, *vo;
  void *gx;                 // FZ_AT
  int64_t nmat;
  int M, N, T, G, solver;
  float eps;
  hipStream_t stream;
};

}  // namespace fz

// X(MP, NPL, largest M, largest N): MP padded rows, a lane holds NPL columns.  Taken in this order, the first row that
// holds the matrix: the smallest register footprint (a 8x150 matrix of the 160x192x160 / patch (5,6,5) configuration in
// the 8x512 family spends 70 % of its work on padding; 8x192 is that patch of BASELINE configs[4]).
#define FZ_NMF_SHAPES(X) \
  X(8, 1, 8, 64)         \
  X(8, 2, 8, 128)        \
  X(8, 3, 8, 192)        \
  X(8, 4, 8, 256)        \
  X(8, 8, 8, 512)        \
  X(16, 1, 16, 64)       \
  X(16, 4, 16, 256)      \
  X(32, 1, 32, 64)       \
  X(32, 2, 32, 128)
