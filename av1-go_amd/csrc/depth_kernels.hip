// depth_kernels.hip — depth reduction: the 10-bit planar planes the input chain leaves become the 8-bit planes that are coded
// (include/av1mi.h "depth reduction"; numpy twin: tests/depth_ref.py).
//
//   k_depth_reduce   out of place and pointwise: 3 bytes in and 1.5 bytes out per luma sample, nothing else.  A lane owns a CELL of 16 output
//                    bytes of one row and reads the 32 input bytes under it: two dwordx4 loads, one dwordx4 store.  The 8-bit rows start
//                    only at multiples of 8 bytes (luma, W8) and 4 bytes (chroma, W8 / 2), so the vector types are declared 4-byte aligned,
//                    as in input_kernels.hip and tonemap_kernels.hip.  A row whose width is no multiple of 16 ends in a short cell of 4, 8
//                    or 12 samples (the widths are multiples of 4), moved in QUADS: a dwordx2 load and a dword store each.  The batch is
//                    one plane of frames x height rows per plane (the heights are even, so a row's parity in the batch is its parity in
//                    its frame).  One launch covers the three planes: a workgroup belongs to one plane, chosen from blockIdx by uniform
//                    branches (selects on the kernel's scalar arguments, no indexed argument array), and a lane to one cell of it.
//                    The threshold of a row is two numbers, for even and odd x; both samples of a dword take theirs in one pass.
#include <hip/hip_runtime.h>

#include "av1mi_internal.hpp"

namespace av1mi {
namespace {

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

constexpr int kCell = 16;      // output bytes = samples of a cell

struct DepthPlane { int w, cpr; unsigned rows, blocks; };      // a batch plane: samples per row, cells per row, rows, workgroups
struct DepthArgs {
  const uint16_t *in[3]; uint8_t *out[3];
  DepthPlane y, c;
  int mode;
};

// two samples of a dword (even x in the low half) -> their two output bytes in bits 0 .. 15; te / to: the thresholds at even / odd x
__device__ __forceinline__ uint32_t reduce2(uint32_t d, uint32_t te, uint32_t to) {
  const uint32_t a = min(((d & 0xFFFFu) + te) >> 2, 255u), b = min(((d >> 16) + to) >> 2, 255u);
  return a | (b << 8);
}
__device__ __forceinline__ uint32_t reduce4(uint32_t d0, uint32_t d1, uint32_t te, uint32_t to) { return reduce2(d0, te, to) | (reduce2(d1, te, to) << 16); }

__global__ __launch_bounds__(256) void k_depth_reduce(DepthArgs A) {
  // plane and block inside the plane: uniform
  unsigned b = blockIdx.x;
  const bool luma = b < A.y.blocks;
  if (!luma) b -= A.y.blocks;
  const int p = luma ? 0 : b < A.c.blocks ? 1 : 2;
  if (p == 2) b -= A.c.blocks;
  const DepthPlane G = luma ? A.y : A.c;
  const uint16_t *in = p == 0 ? A.in[0] : p == 1 ? A.in[1] : A.in[2];      // (selects: no indexed kernel argument)
  uint8_t *out = p == 0 ? A.out[0] : p == 1 ? A.out[1] : A.out[2];
  const unsigned idx = b * 256u + threadIdx.x;
  const unsigned row = idx / (unsigned)G.cpr;
  if (row >= G.rows) return;
  const int x0 = (int)(idx - row * (unsigned)G.cpr) * kCell, n = G.w - x0 < kCell ? G.w - x0 : kCell;
  // T = { { 0, 2 }, { 3, 1 } }, t_p(x, y) = T[y & 1][(x + p) & 1]; x0 is even, so a dword's low half sits at an even x
  uint32_t te = 2, to = 2;
  if (A.mode == AV1MI_DEPTH_ORDERED) {
    const uint32_t t0 = row & 1 ? 3 : 0, t1 = row & 1 ? 1 : 2;
    te = p & 1 ? t1 : t0; to = p & 1 ? t0 : t1;
  }
  const uint16_t *src = in + (size_t)row * G.w + x0;
  uint8_t *dst = out + (size_t)row * G.w + x0;
  if (n == kCell) {
    const u32x4_a4 a = *(const u32x4_a4 *)src, c = *(const u32x4_a4 *)(src + 8);
    *(u32x4_a4 *)dst = u32x4_a4{ reduce4(a.x, a.y, te, to), reduce4(a.z, a.w, te, to), reduce4(c.x, c.y, te, to), reduce4(c.z, c.w, te, to) };
  } else {
#pragma unroll
    for (int q = 0; q < 3; q++)
      if (4 * q < n) {
        const u32x2_a4 a = *(const u32x2_a4 *)(src + 4 * q);
        ((uint32_t *)dst)[q] = reduce4(a.x, a.y, te, to);
      }
  }
}

}  // namespace

hipError_t launch_depth_reduce(int mode, int w, int h, int frames, const void *const in[3], void *const out[3], hipStream_t s) {
  if ((mode != AV1MI_DEPTH_ROUND && mode != AV1MI_DEPTH_ORDERED) || w < 8 || h < 8 || (w & 7) || (h & 7) || w > 16384 || h > 16384 || frames < 1)
    return hipErrorInvalidValue;
  DepthArgs A;
  A.mode = mode;
  for (int p = 0; p < 3; p++) { A.in[p] = (const uint16_t *)in[p]; A.out[p] = (uint8_t *)out[p]; }
  size_t total = 0;
  auto plane = [&](DepthPlane &G, int pw, int ph, int count) {
    const size_t rows = (size_t)ph * frames;
    G.w = pw; G.cpr = (pw + kCell - 1) / kCell;
    const size_t cells = rows * G.cpr, blocks = (cells + 255) / 256;
    if (rows > 0x7FFFFFFFu || cells > 0xFFFFFFFFull - 256) return false;      // (the cell index is 32 bits and runs past the end by under a workgroup)
    G.rows = (unsigned)rows; G.blocks = (unsigned)blocks;
    total += blocks * count;
    return true;
  };
  if (!plane(A.y, w, h, 1) || !plane(A.c, w / 2, h / 2, 2) || total > 0x7FFFFFFFu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_depth_reduce, dim3((unsigned)total), dim3(256), 0, s, A);
  return hipGetLastError();
}

}  // namespace av1mi
