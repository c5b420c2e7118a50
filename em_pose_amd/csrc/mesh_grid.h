// Grid of the kernels of mesh_rows.hip / mesh_bf16.hip: a workgroup of `nw` waves per `bm` frames; with fewer than one
// workgroup per CU the mesh's tiles are split over grid.y (at least one tile per wave).  Host only.
#pragma once
#include <hip/hip_runtime.h>

namespace empose {

inline dim3 mesh_rows_grid(int T, int V, int bm, int nw) {
  const int bx = (T + bm - 1) / bm;
  const int n_tiles = (V + 31) / 32;
  int by = bx >= 256 ? 1 : (256 + bx - 1) / bx;
  const int max_by = (n_tiles + nw - 1) / nw;
  if (by > max_by) by = max_by;
  return dim3(bx, by);
}

}  // namespace empose
