// cdef_search_kernel.hip — the CDEF search (include/av1mi.h "CDEF search"): which of 2, 4 or 8 candidate strength sets brings a
// 64x64 superblock closest to the source.  One 256-lane workgroup per (frame, superblock), frames along the grid like k_cdef.
//
//   STAGE       the deblocked luma tile and the two chroma tiles into LDS, once, by k_cdef's own staging (cdef_stage_tiles: the same
//               shapes, the same 0xFFFF marks outside the picture);
//   PARAMETERS  direction and variance of every 8x8 block, once (wave 0, a block per lane: cdef_block_dirvar) — they do not depend on
//               the strengths — and from them every candidate's per-block record (cdef_block_pack: 2 per lane at 8 candidates);
//   SOURCE      each lane's 16 luma + 8 chroma source samples into registers, once, with how many of each four lie inside the TRUE
//               frame size (search_sse.hpp: SbSource, and the error and the sums below);
//   CANDIDATES  per candidate the filter items of cdef_filter.hpp, whose sink adds the squared difference to the source into a
//               register (a lane's 24 samples: below 2^25), reduced over the wave (below 2^31) into LDS;
//   PICK        the workgroup owns its superblock: thread 0 adds the four waves' sums in 64 bits, takes the arg-min (lowest sum, then
//               lowest index) and writes the eight sums, the chosen set's four strength bytes and the index.  No atomics, no zeroing.
//
// LDS: k_cdef's 16 KB + 2 KB of per-candidate block records.  The VALU work is up to eight filter passes per staging.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "av1mi_internal.hpp"
#include "cdef_filter.hpp"
#include "search_sse.hpp"

namespace av1mi {

template <typename Pix>
__global__ __launch_bounds__(256) void k_cdef_search(CdefSearchLaunch L) {
  constexpr int YS = 64 + 4 + 2, CSZ = 32 + 4 + 2;   // k_cdef's tiles
  __shared__ __attribute__((aligned(16))) uint16_t ty[(64 + 4) * YS + 8];
  __shared__ __attribute__((aligned(16))) uint16_t tc[2][(32 + 4) * CSZ + 8];
  __shared__ uint8_t bskip[64];
  __shared__ uint32_t dirvar[64], bpar[8][64];
  __shared__ __attribute__((aligned(16))) int32_t offy[8 * kTapEntries], offc[8 * kTapEntries];
  __shared__ uint32_t wsum[8][4];
  const int tid = threadIdx.x;
  if (tid < 48) cdef_fill_offsets<YS>(offy, tid); else if (tid >= 64 && tid < 112) cdef_fill_offsets<CSZ>(offc, tid - 64);
  const int sbw = (L.w + 63) / 64, sbh = (L.h + 63) / 64;
  const Tile3 tl = xcd_tile(sbw, sbh, L.nframes);
  const int sbx = tl.x, sby = tl.y, f = tl.z;
  constexpr int bd = sizeof(Pix) == 1 ? 8 : 10, cs = bd - 8;
  const size_t oy = (size_t)f * L.h * L.stride_y, oc = (size_t)f * (L.h / 2) * L.stride_uv;
  if (tid >= 192) {
    const int b = tid - 192, fy8 = sby * 8 + (b >> 3), fx8 = sbx * 8 + (b & 7);
    bskip[b] = (fy8 < (L.h >> 3) && fx8 < (L.w >> 3)) ? L.skip8[(size_t)f * L.skip_frame_stride + (size_t)fy8 * (L.w >> 3) + fx8] : (uint8_t)1;
  }
  const bool interior = sbx > 0 && sby > 0 && sbx * 64 + 66 <= L.w && sby * 64 + 66 <= L.h;
  cdef_stage_tiles<Pix, YS, CSZ>(ty, tc, reinterpret_cast<const Pix *>(L.src[0]) + oy, reinterpret_cast<const Pix *>(L.src[1]) + oc,
                                 reinterpret_cast<const Pix *>(L.src[2]) + oc, L.stride_y, L.stride_uv, sbx, sby, L.w, L.h, interior, tid);
  SbSource<Pix> src;      // SOURCE: the lane's samples, and how many of each four count
  src.load(L.orig, oy, oc, L.stride_y, L.stride_uv, sbx, sby, L.w, L.h, L.tw, L.th, tid);
  __syncthreads();
  // direction and variance: lane b of wave 0 owns 8x8 block b (raster within the superblock); 0 for a block outside the picture
  if (tid < 64) {
    const int by = tid >> 3, bx = tid & 7;
    dirvar[tid] = (sby * 64 + by * 8 < L.h && sbx * 64 + bx * 8 < L.w) ? cdef_block_dirvar<YS>(ty + (2 + by * 8) * YS + 2 + bx * 8, cs) : 0u;
  }
  __syncthreads();
  for (int i = tid; i < L.ncand * 64; i += 256) bpar[i >> 6][i & 63] = cdef_block_pack(dirvar[i & 63], cs, (int)(L.sets[i >> 6] & 255) << cs, L.damping + cs);
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < L.ncand; c++) {
    const CdefSb S = cdef_sb_params(L.sets[c], L.damping, cs);
    uint32_t e = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
      cdef_luma_item<YS>(tid + 256 * k, ty + 2 * YS + 2, sbx, sby, L.w, L.h, S, interior, bskip, bpar[c], offy,
                         [&](int, int, const int (&o)[4]) { e += sq_diff4<Pix>(o, src.sy[k], src.ny[k]); });
#pragma unroll
    for (int k = 0; k < 2; k++)
      cdef_chroma_item<CSZ>(tid + 256 * k, tc[0] + 2 * CSZ + 2, tc[1] + 2 * CSZ + 2, sbx, sby, L.w, L.h, S, interior, bskip, bpar[c], offc,
                            [&](int, int, int, const int (&o)[4]) { e += sq_diff4<Pix>(o, src.sc[k], src.nc[k]); });
    e = wave_sum(e);
    if ((tid & 63) == 0) wsum[c][tid >> 6] = e;
  }
  __syncthreads();
  if (tid == 0) {
    const size_t sb = (size_t)f * sb_count(L.w, L.h) + (size_t)sby * sbw + sbx;
    unsigned long long best = 0;
    int pick = 0;
    for (int c = 0; c < 8; c++) {
      const unsigned long long s = c < L.ncand ? wave_sums_total(wsum[c]) : 0ull;
      L.sse[sb * 8 + c] = s;
      if (c < L.ncand && (c == 0 || s < best)) { best = s; pick = c; }
    }
    *reinterpret_cast<uint32_t *>(L.strength + sb * 4) = L.sets[pick];
    L.idx[sb] = (uint8_t)pick;
  }
}

hipError_t launch_cdef_search(const CdefSearchLaunch &L, hipStream_t s) {
  const dim3 grid((unsigned)(sb_count(L.w, L.h) * L.nframes));   // 1-D: the kernel orders the tiles itself (xcd_tile)
  if (L.bd == 8) hipLaunchKernelGGL(k_cdef_search<uint8_t>, grid, dim3(256), 0, s, L);
  else hipLaunchKernelGGL(k_cdef_search<uint16_t>, grid, dim3(256), 0, s, L);
  return hipGetLastError();
}

}  // namespace av1mi
