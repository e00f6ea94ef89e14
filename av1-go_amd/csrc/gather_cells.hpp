// gather_cells.hpp — a 16-byte cell of a plane's row, one lane's share, as the filtering gathers (deint_kernels.hip, grain_kernels.hip)
// load and store it: whole (dwordx4) where the plane's rows are whole 16-byte units, else dword by dword and the last cell partly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace av1mi {
namespace {

// the cell at byte `off` of a row of rb bytes; dwords beyond the row, and all of an inactive lane's, are 0
__device__ __forceinline__ void load_cell(const char *row, uint32_t off, uint32_t rb, bool whole, bool active, uint32_t c[4]) {
  c[0] = c[1] = c[2] = c[3] = 0;
  if (!active) return;
  if (whole) {
    const uint4 v = *reinterpret_cast<const uint4 *>(row + off);
    c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (off + 4u * q < rb) c[q] = *reinterpret_cast<const uint32_t *>(row + off + 4u * q);
  }
}
__device__ __forceinline__ void store_cell(char *row, uint32_t off, uint32_t rb, bool whole, bool active, const uint32_t c[4]) {
  if (!active) return;
  if (whole) *reinterpret_cast<uint4 *>(row + off) = make_uint4(c[0], c[1], c[2], c[3]);
  else {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (off + 4u * q < rb) *reinterpret_cast<uint32_t *>(row + off + 4u * q) = c[q];
  }
}

}  // namespace
}  // namespace av1mi
