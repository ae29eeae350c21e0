// sqdist.h -- squared Euclidean distances in fp64 with a stated summation order, shared by
// select.hip (numpy's order) and knn.hip (numpy's and the KD-tree's).
//
// Every term is a rounded difference and a rounded square, no FMA.  hipcc's default fuses a
// product into a following sum, also through the header's __dmul_rn / __dadd_rn (plain
// operators there), so a file that includes this header is compiled with contraction off
// (the pragma below reaches the rest of the including file) and the rounded operations are
// the local mul_rn / add_rn / sub_rn.
#pragma once

#pragma clang fp contract(off)

__device__ __forceinline__ double mul_rn(double a, double b) { return a * b; }
__device__ __forceinline__ double add_rn(double a, double b) { return a + b; }
__device__ __forceinline__ double sub_rn(double a, double b) { return a - b; }

// |x - y|^2 in numpy's order for np.linalg.norm(A - x, axis=1) on a C-contiguous array
// (add.reduce along a contiguous axis): d < 8 left to right; d >= 8 eight accumulators over
// elements 0..7, every further full block of eight added lane-wise,
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the d % 8 tail one by one.  y(k) reads element
// k of the other row.
template <int D, class Y>
__device__ __forceinline__ double sqdist(const double (&x)[D], Y y) {
  double s[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double df = sub_rn(y(k), x[k]);
    s[k] = mul_rn(df, df);
  }
  if constexpr (D < 8) {
    double res = s[0];
#pragma unroll
    for (int k = 1; k < D; ++k) res = add_rn(res, s[k]);
    return res;
  } else {
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = s[j];
#pragma unroll
    for (int b = 8; b + 8 <= D; b += 8)
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = add_rn(r[j], s[b + j]);
    double res = add_rn(add_rn(add_rn(r[0], r[1]), add_rn(r[2], r[3])),
                        add_rn(add_rn(r[4], r[5]), add_rn(r[6], r[7])));
#pragma unroll
    for (int k = D - D % 8; k < D; ++k) res = add_rn(res, s[k]);
    return res;
  }
}

// |x - y|^2 in the order of scipy's KD-tree (sqeuclidean_distance_double): four accumulators
// a0..a3 from 0, every full block of four elements added lane-wise, s = ((a0+a1)+a2)+a3, then
// the d % 4 tail one by one.
template <int D, class Y>
__device__ __forceinline__ double sqdist_kd(const double (&x)[D], Y y) {
  double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int b = 0; b + 4 <= D; b += 4)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double df = sub_rn(x[b + j], y(b + j));
      a[j] = add_rn(a[j], mul_rn(df, df));
    }
  double res = add_rn(add_rn(add_rn(a[0], a[1]), a[2]), a[3]);
#pragma unroll
  for (int k = D - D % 4; k < D; ++k) {
    const double df = sub_rn(x[k], y(k));
    res = add_rn(res, mul_rn(df, df));
  }
  return res;
}
