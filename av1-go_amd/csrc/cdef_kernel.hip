// cdef_kernel.hip — SURVEY.md §8a row K6: CDEF of 4:2:0 frames, one 64x64 luma superblock (+ its 32x32 U and V
// blocks) per workgroup, frames of a segment along blockIdx.z.
//
// The workgroup stages the deblocked luma block with a 2-sample halo (and both chroma blocks likewise) in LDS as
// uint16, samples outside the picture stored as 0xFFFF = "not available" (taps skip them, as the spec's
// CdefAvailable: in the packed filter a marked tap is replaced by the centre sample).  Wave 0 then runs the direction search, one 8x8 block per lane with every bin index a
// compile-time constant; afterwards all 256 lanes filter: 16 luma + 8 chroma samples each, 12 taps per sample
// read from LDS.  Output goes to separate planes, so taps never see filtered samples and superblocks are
// independent.  HBM traffic: b*S read + b*S written (= 2b*S of SURVEY.md §8d); halo re-reads hit L2.
//
// Restates AV1 spec §7.15 and libaom cdef_find_dir_c / cdef_filter_block_c / constrain(); the reference has no
// counterpart (internal/ffmpeg/transcode.go:120).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "av1mi_internal.hpp"
#include "cdef_filter.hpp"

namespace av1mi {

template <typename Pix>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_cdef(CdefLaunch L) {
  constexpr int YS = 64 + 4 + 2, CSZ = 32 + 4 + 2;   // LDS row strides (halo 2 each side, +2 pad)
  __shared__ __attribute__((aligned(16))) uint16_t ty[(64 + 4) * YS + 8];
  __shared__ __attribute__((aligned(16))) uint16_t tc[2][(32 + 4) * CSZ + 8];
  __shared__ uint8_t bskip[64];   // skip flag of each 8x8 block of the superblock (1 also for blocks outside the picture)
  // per 8x8 block, from the direction search (cdef_block_params)
  __shared__ uint32_t bpar[64];
  __shared__ __attribute__((aligned(16))) int32_t offy[8 * kTapEntries], offc[8 * kTapEntries];   // tap tables for the two tile strides
  const int tid = threadIdx.x;
  if (tid < 48) cdef_fill_offsets<YS>(offy, tid); else if (tid >= 64 && tid < 112) cdef_fill_offsets<CSZ>(offc, tid - 64);
  const Tile3 tl = xcd_tile((L.w + 63) / 64, (L.h + 63) / 64, L.nframes);
  const int sbx = tl.x, sby = tl.y, f = tl.z;
  constexpr int bd = sizeof(Pix) == 1 ? 8 : 10, cs = bd - 8;   // the launch picks the instantiation by L.bd (8 or 10)
  const Pix *sy = reinterpret_cast<const Pix *>(L.src[0]) + (size_t)f * L.h * L.stride_y;
  Pix *dy = reinterpret_cast<Pix *>(L.dst[0]) + (size_t)f * L.h * L.stride_y;
  const int cw = L.w / 2, chh = L.h / 2;
  // the superblock's strength set, requested before the tile loads so that its latency hides behind them (one aligned dword)
  const int sbw = (L.w + 63) / 64;
  const uint32_t st32 = *reinterpret_cast<const uint32_t *>(L.sb_strength + ((size_t)f * L.sb_frame_stride + (size_t)sby * sbw + sbx) * 4);
  // the 64 skip flags once, next to the tiles: the filter loops read one per quad, and as a global load each of those sat
  // in front of a branch with its whole latency exposed
  if (tid >= 192) {
    const int b = tid - 192, fy8 = sby * 8 + (b >> 3), fx8 = sbx * 8 + (b & 7);
    bskip[b] = (fy8 < (L.h >> 3) && fx8 < (L.w >> 3)) ? L.skip8[(size_t)f * L.skip_frame_stride + (size_t)fy8 * (L.w >> 3) + fx8] : (uint8_t)1;
  }
  // every tap of this superblock inside the picture?  (then the tile holds no 0xFFFF mark: vector staging, no mark handling)
  const bool interior = sbx > 0 && sby > 0 && sbx * 64 + 66 <= L.w && sby * 64 + 66 <= L.h;
  // stage luma 68x68 and chroma 36x36 x2 (local (0,0) = picture (sb*64-2, sb*64-2))
  if (interior) {
    // no bounds to check: 4-sample aligned loads starting 4 samples left of the block (18 per row luma, 10 chroma); the tile
    // keeps only the 2-sample halo, so local column = aligned column - 2.  The four samples are two uint16 pairs = two dword
    // stores: samples 0,1 go to tile columns 4g - 2, 4g - 1 and samples 2,3 to 4g, 4g + 1 (even columns, even row stride);
    // the first pair of a row and the last lie outside.  All of a lane's loads (5 luma + 3 chroma items) are issued before
    // its first LDS store, so their latencies overlap instead of adding up.
    constexpr int NY = 68 * 18, NC = 2 * 36 * 10, KY = (NY + 255) / 256, KC = (NC + 255) / 256;
    uint2 vy[KY], vc[KC];
#pragma unroll
    for (int k = 0; k < KY; k++) {
      const int i = tid + 256 * k;
      if (i < NY) {
        const int r = i / 18, g = i - r * 18;
        const Pix *q = sy + row_off(sby * 64 - 2 + r, L.stride_y) + sbx * 64 - 4 + g * 4;
        if constexpr (sizeof(Pix) == 1) vy[k].x = *reinterpret_cast<const uint32_t *>(q);
        else vy[k] = *reinterpret_cast<const uint2 *>(q);
      }
    }
#pragma unroll
    for (int k = 0; k < KC; k++) {
      const int i = tid + 256 * k;
      if (i < NC) {
        const int pl = i / 360, j = i - pl * 360, r = j / 10, g = j - r * 10;
        const Pix *q = reinterpret_cast<const Pix *>(L.src[1 + pl]) + (size_t)f * chh * L.stride_uv + row_off(sby * 32 - 2 + r, L.stride_uv) + sbx * 32 - 4 + g * 4;
        if constexpr (sizeof(Pix) == 1) vc[k].x = *reinterpret_cast<const uint32_t *>(q);
        else vc[k] = *reinterpret_cast<const uint2 *>(q);
      }
    }
    auto pairs = [](uint2 v, uint32_t &lo, uint32_t &hi) {
      if constexpr (sizeof(Pix) == 1) { lo = __builtin_amdgcn_perm(0u, v.x, 0x0c010c00u); hi = __builtin_amdgcn_perm(0u, v.x, 0x0c030c02u); }
      else { lo = v.x; hi = v.y; }
    };
#pragma unroll
    for (int k = 0; k < KY; k++) {
      const int i = tid + 256 * k;
      if (i < NY) {
        const int r = i / 18, g = i - r * 18;
        uint32_t lo, hi;
        pairs(vy[k], lo, hi);
        uint32_t *d = reinterpret_cast<uint32_t *>(ty + r * YS + g * 4 - 2);
        if (g > 0) d[0] = lo;
        if (g < 17) d[1] = hi;
      }
    }
#pragma unroll
    for (int k = 0; k < KC; k++) {
      const int i = tid + 256 * k;
      if (i < NC) {
        const int pl = i / 360, j = i - pl * 360, r = j / 10, g = j - r * 10;
        uint32_t lo, hi;
        pairs(vc[k], lo, hi);
        uint32_t *d = reinterpret_cast<uint32_t *>(tc[pl] + r * CSZ + g * 4 - 2);
        if (g > 0) d[0] = lo;
        if (g < 9) d[1] = hi;
      }
    }
  } else {
    for (int i = tid; i < 68 * 68; i += 256) {
      const int r = i / 68, c = i - r * 68;
      const int fy = sby * 64 - 2 + r, fx = sbx * 64 - 2 + c;
      ty[r * YS + c] = (fy >= 0 && fy < L.h && fx >= 0 && fx < L.w) ? (uint16_t)sy[row_off(fy, L.stride_y) + fx] : (uint16_t)0xFFFF;
    }
    for (int i = tid; i < 2 * 36 * 36; i += 256) {
      const int pl = i / (36 * 36), j = i - pl * 36 * 36, r = j / 36, c = j - r * 36;
      const int fy = sby * 32 - 2 + r, fx = sbx * 32 - 2 + c;
      const Pix *sc = reinterpret_cast<const Pix *>(L.src[1 + pl]) + (size_t)f * chh * L.stride_uv;
      tc[pl][r * CSZ + c] = (fy >= 0 && fy < chh && fx >= 0 && fx < cw) ? (uint16_t)sc[row_off(fy, L.stride_uv) + fx] : (uint16_t)0xFFFF;
    }
  }
  __syncthreads();
  const bool enabled = (st32 & 255) != 255;
  // direction search: lane b of wave 0 owns 8x8 block b (raster within the superblock)
  if (tid < 64 && enabled) {
    const int by = tid >> 3, bx = tid & 7;
    if (sby * 64 + by * 8 < L.h && sbx * 64 + bx * 8 < L.w) bpar[tid] = cdef_block_params<YS>(ty + (2 + by * 8) * YS + 2 + bx * 8, cs, (int)(st32 & 255) << cs, L.damping + cs);
  }
  __syncthreads();
  // filter: all 256 lanes, with the strengths of the superblock (uniform) and what follows from them alone
  const CdefSb S = cdef_sb_params(st32, L.damping, cs);
  cdef_filter_luma<Pix, YS>(ty + 2 * YS + 2, dy, L.stride_y, sbx, sby, L.w, L.h, S, interior, bskip, bpar, offy, tid);
  cdef_filter_chroma<Pix, CSZ>(tc[0] + 2 * CSZ + 2, tc[1] + 2 * CSZ + 2, reinterpret_cast<Pix *>(L.dst[1]) + (size_t)f * chh * L.stride_uv,
                               reinterpret_cast<Pix *>(L.dst[2]) + (size_t)f * chh * L.stride_uv, L.stride_uv, sbx, sby, L.w, L.h, S, interior, bskip, bpar, offc, tid);
}


hipError_t launch_cdef(const CdefLaunch &L, hipStream_t s) {
  const dim3 grid((unsigned)(((L.w + 63) / 64) * ((L.h + 63) / 64) * L.nframes));   // 1-D: k_cdef orders the tiles itself (xcd_tile)
  if (L.bd == 8) hipLaunchKernelGGL(k_cdef<uint8_t>, grid, dim3(256), 0, s, L);
  else hipLaunchKernelGGL(k_cdef<uint16_t>, grid, dim3(256), 0, s, L);
  return hipGetLastError();
}

}  // namespace av1mi
