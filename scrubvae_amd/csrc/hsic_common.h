// The kernel values every kernel of hsic.hip must share bit for bit: the moments pass (row sums, totals) and the cross sums under
// every permutation take K and L from these two expressions.  Comes after pair_tiles.h, whose #pragma clang fp contract(off)
// covers it.
#pragma once

#include "pair_tiles.h"

namespace svae {

// Gaussian kernel value of a pair at squared distance s (pair_tile, or the same feature-order sum): exp((-s) / h).  No sqrt round
// trip, unlike mmd_value: it would be paid per pair and permutation.
__device__ __forceinline__ double hsic_value(double s, double h) { return exp(-s / h); }

// delta kernel value of a pair of integer labels
__device__ __forceinline__ double hsic_delta(int a, int b) { return a == b ? 1.0 : 0.0; }

}  // namespace svae
