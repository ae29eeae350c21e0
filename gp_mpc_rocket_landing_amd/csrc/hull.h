// hull.h -- the batched convex-hull projection (hull.hip) as other units launch it.
#pragma once
#include "internal.h"

#define HULL_MAXD 32        // features of a vertex
#define HULL_MAXK 64        // vertices of a set: one a lane
#define HULL_WAVES 4        // queries a workgroup serves: one a wave
#define HULL_MAX_ITER 4096  // the most cycles a caller may ask for

// One launch: B queries X (B x d), every pointer a device pointer.  Vertex i < nv[b] of query b
// is row gidx[b * kmax + i] of V when gidx is given (V: a resident table of d-wide rows), else
// row i of V (shared) or row b * kmax + i; q (may be null) is indexed as V's rows.  nv null:
// kmax vertices for every query.  Outputs as gpmpc_hull_project; qhull is written when q is given.
struct HullArgs {
  const double *V, *q, *X;
  const int *nv, *gidx;
  int B, kmax, d, shared;
  double tol;
  int max_iter;
  double *lambda, *proj, *dist, *gap, *qhull;
  int *iters, *status;
};
hipError_t launch_hull(hipStream_t s, const HullArgs &a);
