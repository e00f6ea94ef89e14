// motion_common.hpp — the device routines every kernel that finds or follows motion shares (inter_kernels.hip, mc_kernels.hip,
// me_coarse_kernels.hip, scene_kernels.hip, grain_kernels.hip): the rules a decoder or a numpy reference holds them to — the AV1 sub-pel
// taps, which plane a P frame predicts from, edge extension, the 8-bit view of deeper samples — each stated once.
#pragma once
#include "av1mi_internal.hpp"

namespace av1mi {

// AV1 spec §7.11.3.4 Subpel_Filters: 6 families x 16 phases x 8 taps.  Rows 0 (regular 8-tap) and 4 (regular 4-tap) are the ones the
// encoder policy uses (k_inter_pipe); k_mc takes them all.  static: the library is built one object per .hip file without relocatable
// device code, so every translation unit that reads the table holds its own copy.
static __constant__ int16_t kSubpel[6][16][8] = {
  { { 0, 0, 0, 128, 0, 0, 0, 0 }, { 0, 2, -6, 126, 8, -2, 0, 0 }, { 0, 2, -10, 122, 18, -4, 0, 0 }, { 0, 2, -12, 116, 28, -8, 2, 0 },
    { 0, 2, -14, 110, 38, -10, 2, 0 }, { 0, 2, -14, 102, 48, -12, 2, 0 }, { 0, 2, -16, 94, 58, -12, 2, 0 }, { 0, 2, -14, 84, 66, -12, 2, 0 },
    { 0, 2, -14, 76, 76, -14, 2, 0 }, { 0, 2, -12, 66, 84, -14, 2, 0 }, { 0, 2, -12, 58, 94, -16, 2, 0 }, { 0, 2, -12, 48, 102, -14, 2, 0 },
    { 0, 2, -10, 38, 110, -14, 2, 0 }, { 0, 2, -8, 28, 116, -12, 2, 0 }, { 0, 0, -4, 18, 122, -10, 2, 0 }, { 0, 0, -2, 8, 126, -6, 2, 0 } },
  { { 0, 0, 0, 128, 0, 0, 0, 0 }, { 0, 2, 28, 62, 34, 2, 0, 0 }, { 0, 0, 26, 62, 36, 4, 0, 0 }, { 0, 0, 22, 62, 40, 4, 0, 0 },
    { 0, 0, 20, 60, 42, 6, 0, 0 }, { 0, 0, 18, 58, 44, 8, 0, 0 }, { 0, 0, 16, 56, 46, 10, 0, 0 }, { 0, -2, 16, 54, 48, 12, 0, 0 },
    { 0, -2, 14, 52, 52, 14, -2, 0 }, { 0, 0, 12, 48, 54, 16, -2, 0 }, { 0, 0, 10, 46, 56, 16, 0, 0 }, { 0, 0, 8, 44, 58, 18, 0, 0 },
    { 0, 0, 6, 42, 60, 20, 0, 0 }, { 0, 0, 4, 40, 62, 22, 0, 0 }, { 0, 0, 4, 36, 62, 26, 0, 0 }, { 0, 0, 2, 34, 62, 28, 2, 0 } },
  { { 0, 0, 0, 128, 0, 0, 0, 0 }, { -2, 2, -6, 126, 8, -2, 2, 0 }, { -2, 6, -12, 124, 16, -6, 4, -2 }, { -2, 8, -18, 120, 26, -10, 6, -2 },
    { -4, 10, -22, 116, 38, -14, 6, -2 }, { -4, 10, -22, 108, 48, -18, 8, -2 }, { -4, 10, -24, 100, 60, -20, 8, -2 },
    { -4, 10, -24, 90, 70, -22, 10, -2 }, { -4, 12, -24, 80, 80, -24, 12, -4 }, { -2, 10, -22, 70, 90, -24, 10, -4 },
    { -2, 8, -20, 60, 100, -24, 10, -4 }, { -2, 8, -18, 48, 108, -22, 10, -4 }, { -2, 6, -14, 38, 116, -22, 10, -4 },
    { -2, 6, -10, 26, 120, -18, 8, -2 }, { -2, 4, -6, 16, 124, -12, 6, -2 }, { 0, 2, -2, 8, 126, -6, 2, -2 } },
  { { 0, 0, 0, 128, 0, 0, 0, 0 }, { 0, 0, 0, 120, 8, 0, 0, 0 }, { 0, 0, 0, 112, 16, 0, 0, 0 }, { 0, 0, 0, 104, 24, 0, 0, 0 },
    { 0, 0, 0, 96, 32, 0, 0, 0 }, { 0, 0, 0, 88, 40, 0, 0, 0 }, { 0, 0, 0, 80, 48, 0, 0, 0 }, { 0, 0, 0, 72, 56, 0, 0, 0 },
    { 0, 0, 0, 64, 64, 0, 0, 0 }, { 0, 0, 0, 56, 72, 0, 0, 0 }, { 0, 0, 0, 48, 80, 0, 0, 0 }, { 0, 0, 0, 40, 88, 0, 0, 0 },
    { 0, 0, 0, 32, 96, 0, 0, 0 }, { 0, 0, 0, 24, 104, 0, 0, 0 }, { 0, 0, 0, 16, 112, 0, 0, 0 }, { 0, 0, 0, 8, 120, 0, 0, 0 } },
  { { 0, 0, 0, 128, 0, 0, 0, 0 }, { 0, 0, -4, 126, 8, -2, 0, 0 }, { 0, 0, -8, 122, 18, -4, 0, 0 }, { 0, 0, -10, 116, 28, -6, 0, 0 },
    { 0, 0, -12, 110, 38, -8, 0, 0 }, { 0, 0, -12, 102, 48, -10, 0, 0 }, { 0, 0, -14, 94, 58, -10, 0, 0 }, { 0, 0, -12, 84, 66, -10, 0, 0 },
    { 0, 0, -12, 76, 76, -12, 0, 0 }, { 0, 0, -10, 66, 84, -12, 0, 0 }, { 0, 0, -10, 58, 94, -14, 0, 0 }, { 0, 0, -10, 48, 102, -12, 0, 0 },
    { 0, 0, -8, 38, 110, -12, 0, 0 }, { 0, 0, -6, 28, 116, -10, 0, 0 }, { 0, 0, -4, 18, 122, -8, 0, 0 }, { 0, 0, -2, 8, 126, -4, 0, 0 } },
  { { 0, 0, 0, 128, 0, 0, 0, 0 }, { 0, 0, 30, 62, 34, 2, 0, 0 }, { 0, 0, 26, 62, 36, 4, 0, 0 }, { 0, 0, 22, 62, 40, 4, 0, 0 },
    { 0, 0, 20, 60, 42, 6, 0, 0 }, { 0, 0, 18, 58, 44, 8, 0, 0 }, { 0, 0, 16, 56, 46, 10, 0, 0 }, { 0, 0, 14, 54, 48, 12, 0, 0 },
    { 0, 0, 12, 52, 52, 12, 0, 0 }, { 0, 0, 12, 48, 54, 14, 0, 0 }, { 0, 0, 10, 46, 56, 16, 0, 0 }, { 0, 0, 8, 44, 58, 18, 0, 0 },
    { 0, 0, 6, 42, 60, 20, 0, 0 }, { 0, 0, 4, 40, 62, 22, 0, 0 }, { 0, 0, 4, 36, 62, 26, 0, 0 }, { 0, 0, 2, 34, 62, 30, 0, 0 } },
};
// the table's family for a filter type along a dimension of `dim` samples: blocks up to 4 wide or high take the 4-tap families
__device__ __forceinline__ int mc_filter_index(int type, int dim) {
  if (dim <= 4) { if (type == 0 || type == 2) return 4; if (type == 1) return 5; }
  return type;
}

typedef short s16x2 __attribute__((ext_vector_type(2)));
// The first v_dot2 of an accumulation with its start value as an operand.  The compiler always picks the two-address form
// (v_dot2c: accumulator = destination) and initialises every accumulator with a v_mov first — one extra instruction per output
// sample in loops that are nothing but dot products; the three-address VOP3P form takes the start value from an SGPR.
__device__ __forceinline__ int dot2_start(uint32_t a, uint32_t b, int start_uniform) {
  int d;
  asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(start_uniform));
  return d;
}

// the plane frame f predicts from: the restored one, or (ref_sel given and 0 for this frame and plane) the CDEF output — the
// restoration on / off decision of the previous frame (lr_kernel.hip k_lr_decide) without a copy
// (the flag is read as the aligned dword that holds it: f is uniform in a workgroup, so this is a scalar load)
__device__ __forceinline__ const void *ref_plane(const InterLaunch &L, int f, int p) {
  if (!L.ref_sel) return L.ref[p];
  const int i = f * 3 + p;
  const uint32_t w = reinterpret_cast<const uint32_t *>(L.ref_sel)[i >> 2];
  return ((w >> (8 * (i & 3))) & 0xffu) ? L.ref[p] : L.ref_alt[p];
}

// One dword of the quarter plane: Q[y][x0 .. x0 + 3], Q = (sum of the 4x4 samples' 8-bit views (sample >> sh) + 8) >> 4, from four rows of 16
// samples of a plane of w columns (x0 a multiple of 4, 4 x0 < w, 4 y + 3 inside the plane).  A row is one 16-byte load at 8 bits, two
// above; the last group of a row whose width is not a multiple of 16 replicates the true last column (the quarter plane's padding).
template <typename Pix> __device__ __forceinline__ uint32_t quarter_dword(const Pix *plane, int stride, int w, int sh, int x0, int y) {
  uint32_t sum[4] = { 8, 8, 8, 8 };
  const int ix = 4 * x0;                                       // first of the row's 16 input samples
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const Pix *row = plane + row_off(4 * y + r, stride) + ix;
    if (ix + 15 < w) {
      uint32_t d[4 * (int)sizeof(Pix)];
      __builtin_memcpy(d, row, sizeof(d));
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if constexpr (sizeof(Pix) == 1) sum[k] = __builtin_amdgcn_sad_u8(d[k], 0u, sum[k]);
        else {
          // two samples per dword: their 8-bit views side by side, added as packed halves (8 x 255 per half at most here)
          const uint32_t t = ((d[2 * k] >> sh) & 0x00ff00ffu) + ((d[2 * k + 1] >> sh) & 0x00ff00ffu);
          sum[k] += (t & 0xffffu) + (t >> 16);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++) sum[k >> 2] += (uint32_t)(row[min(k, w - 1 - ix)] >> sh) & 0xffu;
    }
  }
  return (sum[0] >> 4) | ((sum[1] >> 4) << 8) | ((sum[2] >> 4) << 16) | ((sum[3] >> 4) << 24);
}

// One dword of NS samples of plane row `row`, columns x .. x + NS - 1 clamped into [0, w) (the spec's edge extension): one load where
// the group lies inside the row (any address: the hardware takes it), sample by sample where it sticks out.  By default the samples
// fill the dword as they lie in memory.  NS = 4 of 16-bit samples packs their 8-bit views (sample >> sh) & 0xff instead, the form the
// integer search scores (sh is 0 wherever the samples fill the dword).
template <typename Pix, int NS = 4 / (int)sizeof(Pix)> __device__ __forceinline__ uint32_t row_dword(const Pix *row, int x, int w, int sh = 0) {
  constexpr int BITS = 32 / NS;
  if (x >= 0 && x + NS <= w) {
    uint32_t v[NS * (int)sizeof(Pix) / 4];
    __builtin_memcpy(v, row + x, sizeof(v));
    if constexpr (NS * sizeof(Pix) == 4) return v[0];
    else return ((v[0] >> sh) & 0xff) | (((v[0] >> (16 + sh)) & 0xff) << 8) | (((v[1] >> sh) & 0xff) << 16) | (((v[1] >> (16 + sh)) & 0xff) << 24);
  }
  uint32_t u = 0;
#pragma unroll
  for (int k = 0; k < NS; k++) u |= ((uint32_t)(row[min(max(x + k, 0), w - 1)] >> sh) & (0xffffffffu >> (32 - BITS))) << (BITS * k);
  return u;
}

// One window row of N samples from plane row `row`, columns x0 .. x0 + N - 1, into the dword-aligned LDS row `dst`.
// Inside the plane it is one unaligned vector load (the hardware takes any address) and N * sizeof(Pix) / 4 dword stores;
// rows that stick out clamp sample by sample (the spec's edge extension).
template <int N, typename Pix> __device__ __forceinline__ void stage_window_row(const Pix *row, int x0, int w, Pix *dst) {
  constexpr int ND = N * (int)sizeof(Pix) / 4;
  uint32_t u[ND];
  if (x0 >= 0 && x0 + N <= w) __builtin_memcpy(u, row + x0, sizeof(u));
  else {
    constexpr int PER = 4 / (int)sizeof(Pix);
#pragma unroll
    for (int d = 0; d < ND; d++) {
      u[d] = 0;
#pragma unroll
      for (int k = 0; k < PER; k++) u[d] |= (uint32_t)row[min(max(x0 + d * PER + k, 0), w - 1)] << (k * 8 * (int)sizeof(Pix));
    }
  }
  uint32_t *q = reinterpret_cast<uint32_t *>(dst);
#pragma unroll
  for (int d = 0; d < ND; d++) q[d] = u[d];
}

}  // namespace av1mi
