// deblock_cdef_kernel.hip — SURVEY.md §8a rows K5 + K6 in one pass over the reconstruction: the deblocking loop filter and CDEF of
// 4:2:0 frames, one 64x64 luma superblock (+ its 32x32 U and V blocks) per workgroup, frames of a segment along the grid.
//
// k_deblock writes the deblocked planes to HBM only for k_cdef to read them back; both stage the same superblock in LDS as uint16.
// Here the workgroup stages the UNFILTERED reconstruction once, deblocks it in place (deblock_filter.hpp: the source k_deblock
// runs), marks what lies outside the picture with CDEF's 0xFFFF, and runs CDEF on that tile (cdef_filter.hpp: the source k_cdef
// runs).  Of the deblocked planes it stores only the rows loop restoration reads (below).  HBM traffic: b*S read + b*S written,
// against 4b*S of the two kernels, and one staging instead of two.
//
// Halo.  CDEF wants the deblocked superblock plus 2 samples on every side: window W = [-2, 66) in superblock coordinates, both axes.
// A deblocking filter lies on the grid of the narrower of the two transform blocks it separates and modifies less than half of that
// block on either side: an edge at a multiple of 4 that is no multiple of 8 separates 4-sample transforms (filter 4: modifies 2 per
// side, reads 2), at a multiple of 8 but not 16 at most 8-sample ones (filter 8: modifies 3, reads 4), at a multiple of 16 any
// (filter 14: modifies 6, reads 7).  So the edges that can modify a sample of W are those at 0, 4, ..., 64 — the edge at -4 modifies
// [-6, -3], at -8 [-11, -6], at -16 [-22, -11], and at 68 [66, 69], at 72 [69, 74], at 80 [74, 85]: all outside W.  That is exactly
// the edge set k_deblock filters for its 64-sample window.  Pass 1 (horizontal edges at y in [0, 64]) reads rows [-7, 71) of the
// columns of W, as pass 0 left them; pass 0 (vertical edges at x in [0, 64]) is exact on columns W by the same count, is run on
// every staged row, and reads columns [-7, 71).  So unfiltered samples in [-8, 72) x [-8, 72) are all that is ever read: the
// 8-sample halo of k_deblock covers W, and the only widening is pass 1's column range (the window's 64 columns + 2 either side).
// Chroma (4:2:0): transforms of 4 to 16 samples (32x32 luma blocks), and lf_edge gives chroma filter 4 (modifies 2, reads 2) or
// filter 6 (modifies 2, reads 3), never 8 or 14.  Edges that modify W = [-2, 34): 0, 4, ..., 32 (the edge at -4 modifies [-6, -3],
// at 36 [34, 37]); they read [-3, 35) in both passes: a halo of 3, staged as 4 to keep the tile in whole mode-info units.
//
// One tile per plane: 80 x 80 luma, 40 x 40 per chroma plane, rows LW + 2 samples apart.  That is an odd number of dwords (41, 21),
// which the column walks of deblocking want (64 banks of 4 bytes: lanes a row apart hit different banks) and k_cdef's tiles have
// too (35, 19); it is even in samples and the superblock's corner is 8-byte aligned in it, which the packed CDEF taps want (aligned
// dword pairs, cdef_quad_packed).
//
// Rows of the deblocked planes that k_lr reads (lr_kernel.hip, the staging rule of its halo rows): for a stripe with first row
// sstart = 64 k - 8 (luma; 32 k - 4 chroma) and last row send = sstart + 63 (31), rows sstart - 2, sstart - 1 of the stripe above and
// send + 1, send + 2 of the stripe below — luma rows 64 k - 10 .. 64 k - 7, chroma rows 32 k - 6 .. 32 k - 3, for every k >= 1 with
// 64 k - 8 < h (32 k - 4 < h / 2): the stripe below exists.  With h a multiple of 8 all four rows are then inside the picture.  They
// are local rows 54 .. 57 (26 .. 29) of superblock row k - 1: one owner each.  Nothing else of the deblocked planes is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "av1mi_internal.hpp"
#include "deblock_filter.hpp"
#include "cdef_filter.hpp"

namespace av1mi {

// SHARP0: sharpness 0, the only value the encoder loops use (as in k_deblock)
template <typename Pix, bool SHARP0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_deblock_cdef(DeblockCdefLaunch L) {
  typedef LfTile<64, 64, 8> GY;
  typedef LfTile<32, 32, 4> GC;
  constexpr int YS = GY::LS, CS = GC::LS;
  // (+8: the packed taps read whole dword triples, up to two dwords past the last sample they use)
  __shared__ __attribute__((aligned(16))) uint16_t ty[GY::LH * YS + 8];
  __shared__ __attribute__((aligned(16))) uint16_t tc[2][GC::LH * CS + 8];
  __shared__ uint32_t misy[GY::MH * GY::MW], misc[GC::MH * GC::MW];   // deblocking mode info: luma, chroma (U and V share it)
  __shared__ uint8_t bskip[64];   // skip flag of each 8x8 block of the superblock (1 also for blocks outside the picture)
  __shared__ uint32_t bpar[64];   // per 8x8 block, from the direction search (cdef_block_params)
  __shared__ __attribute__((aligned(16))) int32_t offy[8 * kTapEntries], offc[8 * kTapEntries];   // tap tables for the two tile strides
  const int tid = threadIdx.x;
  if (tid < 48) cdef_fill_offsets<YS>(offy, tid); else if (tid >= 64 && tid < 112) cdef_fill_offsets<CS>(offc, tid - 64);
  const Tile3 tl = xcd_tile((L.w + 63) / 64, (L.h + 63) / 64, L.nframes);
  const int sbx = tl.x, sby = tl.y, f = tl.z;
  constexpr int bd = sizeof(Pix) == 1 ? 8 : 10, cs = bd - 8;   // the launch picks the instantiation by L.bd (8 or 10)
  const int cw = L.w / 2, chh = L.h / 2;
  const int sharp = SHARP0 ? 0 : L.sharpness;
  // the superblock's strength set and the 64 skip flags, requested before the tile loads so that their latency hides behind them
  const int sbw = (L.w + 63) / 64;
  const uint32_t st32 = *reinterpret_cast<const uint32_t *>(L.sb_strength + ((size_t)f * L.sb_frame_stride + (size_t)sby * sbw + sbx) * 4);
  if (tid >= 192) {
    const int b = tid - 192, fy8 = sby * 8 + (b >> 3), fx8 = sbx * 8 + (b & 7);
    bskip[b] = (fy8 < (L.h >> 3) && fx8 < (L.w >> 3)) ? L.skip8[(size_t)f * L.skip_frame_stride + (size_t)fy8 * (L.w >> 3) + fx8] : (uint8_t)1;
  }
  // (a) stage the unfiltered reconstruction and the mode info: plane coordinates of LDS (0, 0)
  const int X0 = sbx * 64 - GY::HALO, Y0 = sby * 64 - GY::HALO, CX0 = sbx * 32 - GC::HALO, CY0 = sby * 32 - GC::HALO;
  {
    const Pix *ry = reinterpret_cast<const Pix *>(L.rec[0]) + (size_t)f * L.h * L.rec_stride_y;
    const Pix *ru = reinterpret_cast<const Pix *>(L.rec[1]) + (size_t)f * chh * L.rec_stride_uv;
    const Pix *rv = reinterpret_cast<const Pix *>(L.rec[2]) + (size_t)f * chh * L.rec_stride_uv;
    uint32_t mivy[GY::NMI], mivc[GC::NMI];
    uint2 vy[GY::NIT], vu[GC::NIT], vv[GC::NIT];
    unsigned dy_, du_, dv_;
    // all of a lane's loads (7 luma + 2 x 4 chroma items, 3 mode-info words) before its first LDS store
    lf_mi_load<GY>(mivy, L.mi_y + (size_t)f * L.mi_frame_stride_y, L.mi_stride_y, X0, Y0, L.w, L.h, tid);
    lf_mi_load<GC>(mivc, L.mi_uv + (size_t)f * L.mi_frame_stride_uv, L.mi_stride_uv, CX0, CY0, cw, chh, tid);
    lf_stage_load<Pix, GY>(vy, dy_, ry, L.rec_stride_y, X0, Y0, L.w, L.h, tid);
    lf_stage_load<Pix, GC>(vu, du_, ru, L.rec_stride_uv, CX0, CY0, cw, chh, tid);
    lf_stage_load<Pix, GC>(vv, dv_, rv, L.rec_stride_uv, CX0, CY0, cw, chh, tid);
    lf_mi_store<GY>(misy, mivy, tid);
    lf_mi_store<GC>(misc, mivc, tid);
    lf_stage_store<Pix, GY>(ty, vy, dy_, tid);
    lf_stage_store<Pix, GC>(tc[0], vu, du_, tid);
    lf_stage_store<Pix, GC>(tc[1], vv, dv_, tid);
  }
  __syncthreads();
  // (b) deblock in place.  A chroma pass has 360 / 324 lines for 256 lanes: V starts half a workgroup further on, so that the
  // second round of U and of V fall on different waves
  const int tid2 = (tid + 128) & 255;
  lf_pass0<GY, false, bd>(ty, misy, X0, Y0, L.h, sharp, tid);
  lf_pass0<GC, true, bd>(tc[0], misc, CX0, CY0, chh, sharp, tid);
  lf_pass0<GC, true, bd>(tc[1], misc, CX0, CY0, chh, sharp, tid2);
  __syncthreads();
  lf_pass1<GY, false, bd, 2>(ty, misy, X0, Y0, L.w, sharp, tid);
  lf_pass1<GC, true, bd, 2>(tc[0], misc, CX0, CY0, cw, sharp, tid);
  lf_pass1<GC, true, bd, 2>(tc[1], misc, CX0, CY0, cw, sharp, tid2);
  __syncthreads();
  // the rows of the deblocked planes that k_lr reads (file header): waves 0 and 1; every other lane goes on
  if (tid < 64) {
    const int r = 54 + (tid >> 4), c = (tid & 15) * 4, fx = sbx * 64 + c;
    if (sby * 64 + 56 < L.h && fx < L.w) {
      const uint16_t *p = ty + (GY::HALO + r) * YS + GY::HALO + c;
      const int o[4] = { p[0], p[1], p[2], p[3] };
      cdef_store4<Pix>(reinterpret_cast<Pix *>(L.dbl[0]) + (size_t)f * L.h * L.dbl_stride_y + row_off(sby * 64 + r, L.dbl_stride_y) + fx, o);
    }
  } else if (tid < 128) {
    const int i = tid - 64, pl = i >> 5, r = 26 + ((i >> 3) & 3), c = (i & 7) * 4, fx = sbx * 32 + c;
    if (sby * 32 + 28 < chh && fx < cw) {
      const uint16_t *p = tc[pl] + (GC::HALO + r) * CS + GC::HALO + c;
      const int o[4] = { p[0], p[1], p[2], p[3] };
      cdef_store4<Pix>(reinterpret_cast<Pix *>(L.dbl[1 + pl]) + (size_t)f * chh * L.dbl_stride_uv + row_off(sby * 32 + r, L.dbl_stride_uv) + fx, o);
    }
  }
  // (c) every tap of this superblock inside the picture?  Otherwise mark what lies outside (staging replicated the border there,
  // which deblocking wants and CDEF does not: taps skip marked samples, spec CdefAvailable)
  const bool interior = sbx > 0 && sby > 0 && sbx * 64 + 66 <= L.w && sby * 64 + 66 <= L.h;
  if (!interior) {
    for (int i = tid; i < 68 * 68; i += 256) {
      const int r = i / 68, c = i - r * 68;
      const int fy = sby * 64 - 2 + r, fx = sbx * 64 - 2 + c;
      if (fy < 0 || fy >= L.h || fx < 0 || fx >= L.w) ty[(GY::HALO - 2 + r) * YS + GY::HALO - 2 + c] = (uint16_t)0xFFFF;
    }
    for (int i = tid; i < 2 * 36 * 36; i += 256) {
      const int pl = i / (36 * 36), j = i - pl * 36 * 36, r = j / 36, c = j - r * 36;
      const int fy = sby * 32 - 2 + r, fx = sbx * 32 - 2 + c;
      if (fy < 0 || fy >= chh || fx < 0 || fx >= cw) tc[pl][(GC::HALO - 2 + r) * CS + GC::HALO - 2 + c] = (uint16_t)0xFFFF;
    }
  }
  __syncthreads();
  // (d) CDEF as in k_cdef: direction search, lane b of wave 0 owns 8x8 block b (raster within the superblock) ...
  const CdefSb S = cdef_sb_params(st32, L.damping, cs);
  const uint16_t *ty0 = ty + GY::HALO * YS + GY::HALO;
  if (tid < 64 && S.enabled) {
    const int by = tid >> 3, bx = tid & 7;
    if (sby * 64 + by * 8 < L.h && sbx * 64 + bx * 8 < L.w) bpar[tid] = cdef_block_params<YS>(ty0 + by * 8 * YS + bx * 8, cs, S.ypri0, S.dampy);
  }
  __syncthreads();
  // ... then all 256 lanes filter
  cdef_filter_luma<Pix, YS>(ty0, reinterpret_cast<Pix *>(L.dst[0]) + (size_t)f * L.h * L.dst_stride_y, L.dst_stride_y, sbx, sby, L.w, L.h, S, interior, bskip, bpar, offy, tid);
  cdef_filter_chroma<Pix, CS>(tc[0] + GC::HALO * CS + GC::HALO, tc[1] + GC::HALO * CS + GC::HALO, reinterpret_cast<Pix *>(L.dst[1]) + (size_t)f * chh * L.dst_stride_uv,
                              reinterpret_cast<Pix *>(L.dst[2]) + (size_t)f * chh * L.dst_stride_uv, L.dst_stride_uv, sbx, sby, L.w, L.h, S, interior, bskip, bpar, offc, tid);
}

hipError_t launch_deblock_cdef(const DeblockCdefLaunch &L, hipStream_t s) {
  const dim3 grid((unsigned)(((L.w + 63) / 64) * ((L.h + 63) / 64) * L.nframes));   // 1-D: the kernel orders the tiles itself (xcd_tile)
  const bool s0 = L.sharpness == 0;
  if (L.bd == 8) { if (s0) hipLaunchKernelGGL((k_deblock_cdef<uint8_t, true>), grid, dim3(256), 0, s, L); else hipLaunchKernelGGL((k_deblock_cdef<uint8_t, false>), grid, dim3(256), 0, s, L); }
  else           { if (s0) hipLaunchKernelGGL((k_deblock_cdef<uint16_t, true>), grid, dim3(256), 0, s, L); else hipLaunchKernelGGL((k_deblock_cdef<uint16_t, false>), grid, dim3(256), 0, s, L); }
  return hipGetLastError();
}

}  // namespace av1mi
