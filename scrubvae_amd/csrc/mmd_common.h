// The two expressions mmd.hip and mmd_null.hip must share bit for bit: mmd_permutation_test promises mmd_estimate's statistic
// and a null in its arithmetic.  Comes after pair_tiles.h, whose #pragma clang fp contract(off) covers it.
#pragma once

#include "pair_tiles.h"

namespace svae {

// kernel value of a pair at squared distance s (pair_tile): exp((-(dist * dist)) / h), dist = sqrt(s) as scipy's pdist rounds it
__device__ __forceinline__ double mmd_value(double s, double h) {
  const double dist = sqrt(s);
  const double dd = dist * dist;
  return exp(-dd / h);
}

// kxx + kyy - 2 kxy from the three kernel sums: over the pairs inside a side of na rows, inside the other of nb rows, across.
// out4 (or null) receives {kxx, kyy, kxy, the statistic}.  Symmetric in the sides: the same bits with a and b swapped.
__device__ __forceinline__ double mmd_statistic(double sxx, double syy, double sxy, int na, int nb, double* out4) {
  const double kxx = sxx / ((double)na * (double)(na - 1) / 2.0);
  const double kyy = syy / ((double)nb * (double)(nb - 1) / 2.0);
  const double kxy = sxy / ((double)na * (double)nb);
  const double t = (kxx + kyy) - 2.0 * kxy;
  if (out4) {
    out4[0] = kxx;
    out4[1] = kyy;
    out4[2] = kxy;
    out4[3] = t;
  }
  return t;
}

}  // namespace svae
