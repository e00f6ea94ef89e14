// deblock_kernels.hip — SURVEY.md §8a row K5: the AV1 deblocking loop filter as ONE gfx950 kernel per plane.
//
// A workgroup owns a TW x TH window of output samples.  It stages the window plus an 8-sample halo of the
// UNFILTERED source plane in LDS (coalesced row loads, uint16 per sample), runs pass 0 (vertical edges) on
// every edge that can reach the window or the rows pass 1 will read, then pass 1 (horizontal edges) on the
// window's columns, and writes the window back as whole rows.  Source and destination planes differ, so
// neighbouring workgroups never see each other's output; edges in the halo are recomputed, never exchanged.
// Within a pass edges are independent (a filter never reaches past half of the narrower transform block),
// so lanes filter in place in LDS without ordering.
// HBM traffic: b*S read + b*S written = the 2b*S of SURVEY.md §8d (halo re-reads come from L2).
//
// Restates AV1 spec §7.14 and libaom aom_dsp/loopfilter.c (highbd_filter4/6/8/14 and their masks); the
// reference has no counterpart (internal/ffmpeg/transcode.go:120 names the external encoder only).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "av1mi_internal.hpp"
#include "deblock_filter.hpp"

namespace av1mi {

// CHROMA: the plane's filter-length rule (a launch is one plane); SHARP0: sharpness 0, the only value the encoder loops use
// (other values take the run-time path) — both fold the per-line limit arithmetic.
template <typename Pix, int TW, int TH, bool CHROMA, bool SHARP0>
__global__ __launch_bounds__(256) void k_deblock(DeblockLaunch L) {
  // Halo of 8: an edge needs at most p6..q6 (13-tap filter) plus the flatness tests up to p6/q6; an edge whose filter can
  // reach the window lies in [0, TW] x [0, TH], so source samples in [-8, TW + 8) x [-8, TH + 8) are all that is ever read
  typedef LfTile<TW, TH, 8> G;
  __shared__ __attribute__((aligned(16))) uint16_t tile[G::LH * G::LS];
  __shared__ uint32_t mis[G::MH * G::MW];
  const int tid = threadIdx.x;
  const Tile3 tl = xcd_tile((L.w + TW - 1) / TW, (L.h + TH - 1) / TH, L.nframes);
  const int X0 = tl.x * TW - G::HALO, Y0 = tl.y * TH - G::HALO;   // frame coords of LDS (0,0)
  // frame tl.z of a stack of frames: planes are stacked vertically, mode info per frame or shared
  const Pix *src = reinterpret_cast<const Pix *>(L.src) + (size_t)tl.z * L.h * L.src_stride;
  const uint32_t *mi = L.mi + (size_t)tl.z * L.mi_frame_stride;
  constexpr int BD = sizeof(Pix) == 1 ? 8 : 10;
  const int sharp = SHARP0 ? 0 : L.sharpness;
  // mode-info units requested first, stored after the sample loads have been issued too; all of a lane's loads first, then its
  // LDS stores (as one loop every load was waited for before the next one was issued)
  {
    uint32_t miv[G::NMI];
    uint2 v[G::NIT];
    unsigned done;
    lf_mi_load<G>(miv, mi, L.mi_stride, X0, Y0, L.w, L.h, tid);
    lf_stage_load<Pix, G>(v, done, src, L.src_stride, X0, Y0, L.w, L.h, tid);
    lf_mi_store<G>(mis, miv, tid);
    lf_stage_store<Pix, G>(tile, v, done, tid);
  }
  __syncthreads();
  lf_pass0<G, CHROMA, BD>(tile, mis, X0, Y0, L.h, sharp, tid);
  __syncthreads();
  lf_pass1<G, CHROMA, BD, 0>(tile, mis, X0, Y0, L.w, sharp, tid);
  __syncthreads();
  constexpr int HALO = G::HALO, LS = G::LS;
  // write the window, 4 samples per lane per step
  Pix *dst = reinterpret_cast<Pix *>(L.dst) + (size_t)tl.z * L.h * L.dst_stride;
  for (int i = tid; i < TH * (TW / 4); i += 256) {
    const int wy = i / (TW / 4), wx = (i % (TW / 4)) * 4;
    const int fy = Y0 + HALO + wy, fx = X0 + HALO + wx;
    if (fy >= L.h || fx >= L.w) continue;   // w, h are multiples of 4
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(tile + (HALO + wy) * LS + HALO + wx);
    const uint32_t lo = s32[0], hi = s32[1];
    Pix *o = dst + (size_t)fy * L.dst_stride + fx;
    if constexpr (sizeof(Pix) == 1) *reinterpret_cast<uint32_t *>(o) = __builtin_amdgcn_perm(hi, lo, 0x06040200u);
    else *reinterpret_cast<uint2 *>(o) = make_uint2(lo, hi);
  }
}

hipError_t launch_deblock(const DeblockLaunch &L, hipStream_t s) {
  constexpr int TW = 64, TH = 64;
  const dim3 grid((unsigned)(((L.w + TW - 1) / TW) * ((L.h + TH - 1) / TH) * L.nframes));   // 1-D: the kernel orders the tiles (xcd_tile)
  const dim3 blk(256);
#define AV1MI_DBL(PIX, C, S0) hipLaunchKernelGGL((k_deblock<PIX, TW, TH, C, S0>), grid, blk, 0, s, L)
  const bool c = L.is_chroma != 0, s0 = L.sharpness == 0;
  if (L.bd == 8) { if (c) { if (s0) AV1MI_DBL(uint8_t, true, true); else AV1MI_DBL(uint8_t, true, false); }
                   else   { if (s0) AV1MI_DBL(uint8_t, false, true); else AV1MI_DBL(uint8_t, false, false); } }
  else           { if (c) { if (s0) AV1MI_DBL(uint16_t, true, true); else AV1MI_DBL(uint16_t, true, false); }
                   else   { if (s0) AV1MI_DBL(uint16_t, false, true); else AV1MI_DBL(uint16_t, false, false); } }
#undef AV1MI_DBL
  return hipGetLastError();
}

}  // namespace av1mi
