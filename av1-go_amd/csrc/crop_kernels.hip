// crop_kernels.hip — the crop window of the GOP session and the black-bar analysis (include/av1mi.h "crop window", "bar detection").
// Three gfx950 kernels:
//
//   k_crop_copy     the window of the planar 4:2:0 planes at the fed size -> the coded planes, ONE launch for the three planes of all
//                   stacked frames; the window's own last column / row is replicated into the coded planes' padding.  A lane owns 16
//                   bytes of one output row.  The window starts at any even luma column, so a source row starts at any even byte
//                   (8-bit luma), any byte (8-bit chroma) or any 2 / 4 bytes (16-bit): the 16-byte load is declared with the SAMPLE's
//                   alignment and nothing more (the idiom of k_scale's staging and of mc_kernels.hip: the hardware takes a global
//                   dwordx4 load at any byte address; there is no flat access and no LDS behind it).  A group that reaches beyond the
//                   window is read sample by sample with clamped coordinates: nothing outside the window is ever read.  The stores go
//                   to the coded planes, whose rows are whole dwords: 16 bytes declared 4-byte aligned, or single dwords at a row's end.
//   k_crop_sums     every luma sample of the analysed frames is read ONCE and feeds both families of sums.  A workgroup owns a tile of
//                   kTileUnits 16-byte units x kTileRows rows of one frame; a wave reads 64 consecutive units of one row (1 KiB,
//                   coalesced), the four waves take rows r, r + 1, r + 2, r + 3 and step by four.  Per lane the m8 views of its unit's
//                   columns are accumulated over its 16 rows as PACKED 16-bit pairs (16 x 255 fits); a row's sum is reduced across the
//                   wave's lanes and written by one lane.  After the rows the four waves' column accumulators meet in LDS and leave the
//                   workgroup as one partial per column.  No atomics: every partial has one writer.
//   k_crop_margins  one workgroup per frame: row(y) and col(x) are the partials added in an order fixed by geometry, compared with
//                   limit * w / limit * h, and the four margins are integer minima (LDS atomicMin: the order changes nothing).
// Arithmetic: include/av1mi.h; restated in numpy by tests/crop_ref.py.  Reference tree: nothing (transcode.go:120).
#include <string.h>
#include "av1mi_internal.hpp"

namespace av1mi {

namespace {
constexpr int kTileUnits = 64;      // 16-byte units of a row per workgroup: one per lane of a wave
constexpr int kTileRows = 64;       // rows per workgroup: 16 per wave (packed 16-bit column accumulators hold 257 rows of 255)

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct CropCopyPlane {
  int origin;                 // of the window in the source plane: y * stride + x, samples
  int src_stride, src_rows;   // the source plane's buffer: samples per row, rows per frame
  int win_w, win_h;           // the window in this plane
  int dst_w, dst_h;           // the coded plane (= its stride and rows per frame)
  int groups;                 // 16-byte groups of a destination row (the last may be partial)
};
struct CropCopyLaunch {
  const void *src[3]; void *dst[3];
  CropCopyPlane pl[3];
  unsigned first_wg1, first_wg2;      // the first workgroup of the U and of the V plane
  int frames;
};

template <typename Pix>
__global__ __launch_bounds__(256) void k_crop_copy(CropCopyLaunch L) {
  constexpr int G = 16 / (int)sizeof(Pix);
  const unsigned bid = blockIdx.x;
  const int p = bid < L.first_wg1 ? 0 : bid < L.first_wg2 ? 1 : 2;
  const CropCopyPlane d = p == 0 ? L.pl[0] : p == 1 ? L.pl[1] : L.pl[2];      // (selects: no indexed kernel argument)
  const Pix *src = reinterpret_cast<const Pix *>(p == 0 ? L.src[0] : p == 1 ? L.src[1] : L.src[2]);
  Pix *dst = reinterpret_cast<Pix *>(p == 0 ? L.dst[0] : p == 1 ? L.dst[1] : L.dst[2]);
  const unsigned item = (bid - (p == 0 ? 0u : p == 1 ? L.first_wg1 : L.first_wg2)) * 256u + threadIdx.x;
  const unsigned per_frame = (unsigned)d.groups * (unsigned)d.dst_h;
  const unsigned f = item / per_frame;
  if (f >= (unsigned)L.frames) return;
  const unsigned rem = item - f * per_frame, y = rem / (unsigned)d.groups;
  const int x0 = (int)(rem - y * (unsigned)d.groups) * G;
  const Pix *rp = src + (size_t)f * d.src_rows * d.src_stride + d.origin + row_off(min((int)y, d.win_h - 1), d.src_stride);
  uint32_t o[4];
  if (x0 + G <= d.win_w) {
    __builtin_memcpy(o, rp + x0, 16);      // alignment: the sample's
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      o[q] = 0;
#pragma unroll
      for (int m = 0; m < G / 4; m++) o[q] |= (uint32_t)rp[min(x0 + q * (G / 4) + m, d.win_w - 1)] << (m * 8 * (int)sizeof(Pix));
    }
  }
  Pix *out = dst + ((size_t)f * d.dst_h + y) * d.dst_w + x0;
  const int n = d.dst_w - x0;      // samples of this group inside the coded plane: whole dwords
  if (n >= G) {
    *reinterpret_cast<u32x4_a4 *>(out) = u32x4_a4{ o[0], o[1], o[2], o[3] };
  } else {
#pragma unroll
    for (int q = 0; q < 3; q++)
      if (q * (G / 4) < n) reinterpret_cast<uint32_t *>(out)[q] = o[q];
  }
}

// ------------------------------------------------------------------------------------------ bar detection
// the unit's columns as packed 16-bit pairs: NR registers.  8-bit: dword k holds samples 4 k .. 4 k + 3; register 2 k = samples 4 k
// (low half) and 4 k + 2 (high half), register 2 k + 1 = samples 4 k + 1 and 4 k + 3.  16-bit: register k = samples 2 k and 2 k + 1.
template <typename Pix> struct CropRegs { static constexpr int NR = sizeof(Pix) == 1 ? 8 : 4; };

// grid: tiles_x x tiles_y x frames, in xcd_tile order
template <typename Pix>
__global__ __launch_bounds__(256) void k_crop_sums(const Pix *luma, uint32_t *rowpart, uint32_t *colpart, int stride, int rows, int w, int h, int sh, int tiles_x,
                                                   int tiles_y, int frames) {
  constexpr int G = 16 / (int)sizeof(Pix), NR = CropRegs<Pix>::NR;
  __shared__ uint32_t s_col[4][NR][kTileUnits];
  const Tile3 tl = xcd_tile((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)frames);
  const int f = tl.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = (tl.x * kTileUnits + lane) * G, y0 = tl.y * kTileRows;
  const Pix *in = luma + (size_t)f * rows * stride;
  uint32_t acc[NR];
#pragma unroll
  for (int k = 0; k < NR; k++) acc[k] = 0;
  for (int r = wave; r < kTileRows; r += 4) {
    const int y = y0 + r;
    if (y >= h) break;      // (uniform in the wave)
    uint32_t t[NR], rs = 0;
#pragma unroll
    for (int k = 0; k < NR; k++) t[k] = 0;
    if (x0 < w) {
      const Pix *row = in + row_off(y, stride) + x0;
      if (x0 + G <= w) {
        uint32_t d[4];
        __builtin_memcpy(d, row, 16);
        if constexpr (sizeof(Pix) == 1) {
#pragma unroll
          for (int k = 0; k < 4; k++) { t[2 * k] = d[k] & 0x00ff00ffu; t[2 * k + 1] = (d[k] >> 8) & 0x00ff00ffu; }
        } else {
#pragma unroll
          for (int k = 0; k < 4; k++) t[k] = (d[k] >> sh) & 0x00ff00ffu;
        }
      } else {      // the unit that holds the last true column: sample by sample, nothing at or beyond column w
#pragma unroll
        for (int j = 0; j < G; j++) {
          const uint32_t v = x0 + j < w ? ((uint32_t)row[j] >> sh) & 0xffu : 0u;
          if constexpr (sizeof(Pix) == 1) t[2 * (j >> 2) + (j & 1)] |= v << (16 * ((j >> 1) & 1));
          else t[j >> 1] |= v << (16 * (j & 1));
        }
      }
#pragma unroll
      for (int k = 0; k < NR; k++) { acc[k] += t[k]; rs += (t[k] & 0xffffu) + (t[k] >> 16); }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) rs += __shfl_xor(rs, m, 64);
    if (lane == 0) rowpart[((size_t)f * h + y) * tiles_x + tl.x] = rs;
  }
#pragma unroll
  for (int k = 0; k < NR; k++) s_col[wave][k][lane] = acc[k];
  __syncthreads();
  // a partial per column of the tile: the four waves' halves added
  for (int c = tid; c < kTileUnits * G; c += 256) {
    const int u = c / G, j = c - u * G;
    const int reg = sizeof(Pix) == 1 ? 2 * (j >> 2) + (j & 1) : j >> 1, half = sizeof(Pix) == 1 ? (j >> 1) & 1 : j & 1;
    uint32_t s = 0;
#pragma unroll
    for (int wv = 0; wv < 4; wv++) s += (s_col[wv][reg][u] >> (16 * half)) & 0xffffu;
    const int x = tl.x * kTileUnits * G + c;
    if (x < w) colpart[((size_t)f * tiles_y + tl.y) * w + x] = s;
  }
}

// one workgroup per frame
__global__ __launch_bounds__(256) void k_crop_margins(const uint32_t *rowpart, const uint32_t *colpart, av1mi_crop_record *out, int w, int h, int tiles_x, int tiles_y,
                                                      uint32_t limit) {
  __shared__ uint32_t s_m[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (tid < 4) s_m[tid] = tid < 2 ? (uint32_t)h : (uint32_t)w;
  __syncthreads();
  for (int y = tid; y < h; y += 256) {
    uint32_t s = 0;
    for (int t = 0; t < tiles_x; t++) s += rowpart[((size_t)f * h + y) * tiles_x + t];
    if (s > limit * (uint32_t)w) { atomicMin(&s_m[0], (uint32_t)y); atomicMin(&s_m[1], (uint32_t)(h - 1 - y)); }
  }
  for (int x = tid; x < w; x += 256) {
    uint32_t s = 0;
    for (int t = 0; t < tiles_y; t++) s += colpart[((size_t)f * tiles_y + t) * w + x];
    if (s > limit * (uint32_t)h) { atomicMin(&s_m[2], (uint32_t)x); atomicMin(&s_m[3], (uint32_t)(w - 1 - x)); }
  }
  __syncthreads();
  if (tid == 0) {
    av1mi_crop_record r;
    r.top = s_m[0]; r.bottom = s_m[1]; r.left = s_m[2]; r.right = s_m[3];
    out[f] = r;
  }
}

}  // namespace

CropLayout crop_layout(int bd, int w, int h, int frames) {
  CropLayout L;
  const int G = bd == 8 ? 16 : 8;
  L.tiles_x = ((w + G - 1) / G + kTileUnits - 1) / kTileUnits; L.tiles_y = (h + kTileRows - 1) / kTileRows;
  L.off_cols = (size_t)frames * h * L.tiles_x * 4;
  L.bytes = L.off_cols + (size_t)frames * L.tiles_y * w * 4;
  return L;
}

hipError_t launch_crop_analyse(const CropAnalyseLaunch &A, hipStream_t s) {
  if (A.frames <= 0) return hipSuccess;
  const CropLayout L = crop_layout(A.bd, A.w, A.h, A.frames);
  uint32_t *rowpart = (uint32_t *)A.scratch, *colpart = (uint32_t *)((char *)A.scratch + L.off_cols);
  const size_t grid = (size_t)L.tiles_x * L.tiles_y * A.frames;
  if (grid > 0x7FFFFFFFu) return hipErrorInvalidValue;
  if (A.bd == 8)
    hipLaunchKernelGGL(k_crop_sums<uint8_t>, dim3((unsigned)grid), dim3(256), 0, s, (const uint8_t *)A.luma, rowpart, colpart, A.stride, A.rows, A.w, A.h, 0, L.tiles_x,
                       L.tiles_y, A.frames);
  else
    hipLaunchKernelGGL(k_crop_sums<uint16_t>, dim3((unsigned)grid), dim3(256), 0, s, (const uint16_t *)A.luma, rowpart, colpart, A.stride, A.rows, A.w, A.h, A.bd - 8,
                       L.tiles_x, L.tiles_y, A.frames);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_crop_margins, dim3((unsigned)A.frames), dim3(256), 0, s, rowpart, colpart, A.out, A.w, A.h, L.tiles_x, L.tiles_y, (uint32_t)A.limit);
  return hipGetLastError();
}

hipError_t launch_crop_copy(const CropWindow &W, int bd, int dst_w, int dst_h, int frames, const void *const *src, void *const *dst, hipStream_t s) {
  if (frames < 1) return hipErrorInvalidValue;
  CropCopyLaunch L;
  memset(&L, 0, sizeof(L));
  const int bps = bd == 8 ? 1 : 2, fw8 = (W.frame_w + 7) & ~7, fh8 = (W.frame_h + 7) & ~7;
  size_t wgs[3];
  for (int p = 0; p < 3; p++) {
    const int ss = p > 0;
    CropCopyPlane &d = L.pl[p];
    L.src[p] = src[p]; L.dst[p] = dst[p];
    d.src_stride = fw8 >> ss; d.src_rows = fh8 >> ss;
    d.origin = (W.y >> ss) * d.src_stride + (W.x >> ss);
    d.win_w = W.w >> ss; d.win_h = W.h >> ss; d.dst_w = dst_w >> ss; d.dst_h = dst_h >> ss;
    d.groups = (d.dst_w * bps + 15) / 16;
    wgs[p] = ((size_t)d.groups * d.dst_h * frames + 255) / 256;
    if (wgs[p] * 256 > 0xFFFFFFFFu) return hipErrorInvalidValue;      // (items are counted in 32 bits)
  }
  if (wgs[0] + wgs[1] + wgs[2] > 0x7FFFFFFFu) return hipErrorInvalidValue;
  L.first_wg1 = (unsigned)wgs[0]; L.first_wg2 = (unsigned)(wgs[0] + wgs[1]); L.frames = frames;
  const dim3 grid((unsigned)(wgs[0] + wgs[1] + wgs[2])), block(256);
  if (bd == 8) hipLaunchKernelGGL(k_crop_copy<uint8_t>, grid, block, 0, s, L);
  else hipLaunchKernelGGL(k_crop_copy<uint16_t>, grid, block, 0, s, L);
  return hipGetLastError();
}

}  // namespace av1mi
