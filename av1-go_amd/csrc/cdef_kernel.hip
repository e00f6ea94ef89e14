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
  const int chh = L.h / 2;
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
  cdef_stage_tiles<Pix, YS, CSZ>(ty, tc, sy, reinterpret_cast<const Pix *>(L.src[1]) + (size_t)f * chh * L.stride_uv,
                                 reinterpret_cast<const Pix *>(L.src[2]) + (size_t)f * chh * L.stride_uv, L.stride_y, L.stride_uv, sbx, sby, L.w, L.h, interior, tid);
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
