// lf_search_kernel.hip — the deblocking search (include/av1mi.h "deblocking search"): which of 8 candidate levels around the policy's
// brings a frame's deblocked planes closest to the source, luma and chroma apart.
//
// k_lf_search: one 256-lane workgroup per (frame, superblock), frames along the grid like k_deblock_cdef, whose tiles these are.
//   STAGE       the UNFILTERED 80 x 80 luma tile, the two 40 x 40 chroma tiles and the mode-info words under them into LDS, once, by
//               deblock_filter.hpp's own staging (lf_stage_load / store, lf_mi_load / store: the calls of k_deblock_cdef);
//   SOURCE      each lane's 16 luma + 8 chroma source samples of the inner 64 x 64 / 2 x 32 x 32 into registers, once, with how many of
//               each four lie inside the TRUE frame size (search_sse.hpp: SbSource, and the error and the sums below);
//   CANDIDATES  per candidate: the pristine tiles copied to work tiles (LDS to LDS, 16 bytes a lane and trip), the two level bytes of
//               the LDS mode-info words replaced (k_mi_levels' rule: a word that carries bit 24 is held; so is the 0xFFFFFFFF of a unit
//               outside the plane), lf_pass0 / lf_pass1 as k_deblock runs them (window only: EXT 0), then the lane's squared
//               differences (16 + 8 samples: below 2^25), reduced over the wave (below 2^31) into LDS.  A group (luma, chroma) whose
//               levels equal an earlier candidate's is not run again: its sum is that candidate's;
//   TABLE       lanes 0 .. 15 add the four waves' sums in 64 bits and write the superblock's sixteen sums [2][8]: every entry of the
//               table has one writer, so there are no atomics and no zeroing launch.
// The windows are exact by the argument in deblock_cdef_kernel.hip's header: edges at 0, 4, ..., 64 (32) are all that can modify the
// inner window, and a halo of 8 (4) covers what they read.
//
// k_lf_pick: one workgroup per frame adds the table over the frame's superblocks (lane = stripe of superblocks x column, then the 16
// stripes in order: integer sums, any order gives the same bits), takes the two arg-mins (lowest sum, then lowest index) and writes
// the sixteen sums, the two indices and the four header levels.
//
// LDS: 2 x 13.1 KB luma (pristine, work) + 2 x 6.7 KB chroma + 2 KB mode info + the wave sums = 41.9 KB: three workgroups a CU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "av1mi_internal.hpp"
#include "deblock_filter.hpp"
#include "search_sse.hpp"

namespace av1mi {

// N16 x 16 bytes LDS to LDS, and the level bytes of N mode-info words
template <int N16> __device__ __forceinline__ void lf_copy16(uint16_t *dst, const uint16_t *src, int tid) {
  for (int i = tid; i < N16; i += 256) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
}
template <int N> __device__ __forceinline__ void lf_patch_levels(uint32_t *mis, uint32_t bits, int tid) {
  for (int i = tid; i < N; i += 256) {
    const uint32_t v = mis[i];
    if (!(v & (1u << 24))) mis[i] = (v & ~0x00FFFF00u) | bits;
  }
}

// SHARP0: sharpness 0, the only value the policy gives (as in k_deblock)
template <typename Pix, bool SHARP0>
__global__ __launch_bounds__(256) void k_lf_search(LfSearchLaunch L) {
  typedef LfTile<64, 64, 8> GY;
  typedef LfTile<32, 32, 4> GC;
  constexpr int YS = GY::LS, CS = GC::LS, NY = GY::LH * YS, NC = GC::LH * CS;
  static_assert(NY * 2 % 16 == 0 && NC * 2 % 16 == 0, "the tiles are copied 16 bytes at a time");
  __shared__ __attribute__((aligned(16))) uint16_t py[NY], wy[NY];             // luma: pristine, work
  __shared__ __attribute__((aligned(16))) uint16_t pc[2 * NC], wc[2 * NC];     // U then V
  __shared__ uint32_t misy[GY::MH * GY::MW], misc[GC::MH * GC::MW];
  __shared__ uint32_t wsum[2][8][4];                                           // [luma / chroma][candidate][wave]
  const int tid = threadIdx.x;
  const int sbw = (L.w + 63) / 64, sbh = (L.h + 63) / 64;
  const Tile3 tl = xcd_tile(sbw, sbh, L.nframes);
  const int sbx = tl.x, sby = tl.y, f = tl.z;
  constexpr int bd = sizeof(Pix) == 1 ? 8 : 10;      // the launch picks the instantiation by L.bd (8 or 10)
  const int cw = L.w / 2, chh = L.h / 2;
  const int sharp = SHARP0 ? 0 : L.sharpness;
  const size_t oy = (size_t)f * L.h * L.stride_y, oc = (size_t)f * chh * L.stride_uv;
  const int X0 = sbx * 64 - GY::HALO, Y0 = sby * 64 - GY::HALO, CX0 = sbx * 32 - GC::HALO, CY0 = sby * 32 - GC::HALO;
  // STAGE: all of a lane's loads before its first LDS store, as in k_deblock_cdef
  {
    const Pix *ry = reinterpret_cast<const Pix *>(L.rec[0]) + oy, *ru = reinterpret_cast<const Pix *>(L.rec[1]) + oc, *rv = reinterpret_cast<const Pix *>(L.rec[2]) + oc;
    uint32_t mivy[GY::NMI], mivc[GC::NMI];
    uint2 vy[GY::NIT], vu[GC::NIT], vv[GC::NIT];
    unsigned dy_, du_, dv_;
    lf_mi_load<GY>(mivy, L.mi_y + (size_t)f * L.mi_frame_stride_y, L.mi_stride_y, X0, Y0, L.w, L.h, tid);
    lf_mi_load<GC>(mivc, L.mi_uv + (size_t)f * L.mi_frame_stride_uv, L.mi_stride_uv, CX0, CY0, cw, chh, tid);
    lf_stage_load<Pix, GY>(vy, dy_, ry, L.stride_y, X0, Y0, L.w, L.h, tid);
    lf_stage_load<Pix, GC>(vu, du_, ru, L.stride_uv, CX0, CY0, cw, chh, tid);
    lf_stage_load<Pix, GC>(vv, dv_, rv, L.stride_uv, CX0, CY0, cw, chh, tid);
    lf_mi_store<GY>(misy, mivy, tid);
    lf_mi_store<GC>(misc, mivc, tid);
    lf_stage_store<Pix, GY>(py, vy, dy_, tid);
    lf_stage_store<Pix, GC>(pc, vu, du_, tid);
    lf_stage_store<Pix, GC>(pc + NC, vv, dv_, tid);
  }
  SbSource<Pix> src;      // SOURCE: the lane's samples, and how many of each four count
  src.load(L.orig, oy, oc, L.stride_y, L.stride_uv, sbx, sby, L.w, L.h, L.tw, L.th, tid);
  __syncthreads();
  // CANDIDATES (every condition on c is the launch's: the whole workgroup takes the same way to every barrier)
  const int tid2 = (tid + 128) & 255;      // V's lines start half a workgroup further on than U's (k_deblock_cdef)
#pragma unroll 1
  for (int c = 0; c < 8; c++) {
    const bool luma = L.first[0][c] == c, chroma = L.first[1][c] == c;
    if (!luma && !chroma) continue;
    if (luma) {
      lf_copy16<NY * 2 / 16>(wy, py, tid);
      lf_patch_levels<GY::MH * GY::MW>(misy, (uint32_t)L.lvl[c][0] << 8 | (uint32_t)L.lvl[c][1] << 16, tid);
    }
    if (chroma) {
      lf_copy16<2 * NC * 2 / 16>(wc, pc, tid);
      lf_patch_levels<GC::MH * GC::MW>(misc, (uint32_t)L.lvl[c][2] << 8 | (uint32_t)L.lvl[c][2] << 16, tid);
    }
    __syncthreads();
    if (luma) lf_pass0<GY, false, bd>(wy, misy, X0, Y0, L.h, sharp, tid);
    if (chroma) {
      lf_pass0<GC, true, bd>(wc, misc, CX0, CY0, chh, sharp, tid);
      lf_pass0<GC, true, bd>(wc + NC, misc, CX0, CY0, chh, sharp, tid2);
    }
    __syncthreads();
    if (luma) lf_pass1<GY, false, bd, 0>(wy, misy, X0, Y0, L.w, sharp, tid);
    if (chroma) {
      lf_pass1<GC, true, bd, 0>(wc, misc, CX0, CY0, cw, sharp, tid);
      lf_pass1<GC, true, bd, 0>(wc + NC, misc, CX0, CY0, cw, sharp, tid2);
    }
    __syncthreads();
    uint32_t ey = 0, ec = 0;
    if (luma) {
#pragma unroll
      for (int k = 0; k < 4; k++) ey += sq_diff4<Pix>(wy + (GY::HALO + sb_luma_row(tid + 256 * k)) * YS + GY::HALO + sb_luma_col(tid + 256 * k), src.sy[k], src.ny[k]);
    }
    if (chroma) {
#pragma unroll
      for (int k = 0; k < 2; k++) ec += sq_diff4<Pix>(wc + k * NC + (GC::HALO + sb_chroma_row(tid)) * CS + GC::HALO + sb_chroma_col(tid), src.sc[k], src.nc[k]);
    }
    ey = wave_sum(ey); ec = wave_sum(ec);
    if ((tid & 63) == 0) {
      if (luma) wsum[0][c][tid >> 6] = ey;
      if (chroma) wsum[1][c][tid >> 6] = ec;
    }
    __syncthreads();      // the sums are in LDS, and the work tiles are free for the next candidate
  }
  // TABLE: a lane per entry; a twin's entry is the sum of the candidate it repeats
  if (tid < 16) {
    const int g = tid >> 3, c = tid & 7, first = L.first[g][c];
    const size_t sb = (size_t)f * sb_count(L.w, L.h) + (size_t)sby * sbw + sbx;
    L.table[sb * 16 + tid] = wave_sums_total(wsum[g][first]);
  }
}

__global__ __launch_bounds__(256) void k_lf_pick(LfSearchLaunch L) {
  __shared__ unsigned long long part[16][16], total[16];
  const int tid = threadIdx.x, f = blockIdx.x, col = tid & 15, stripe = tid >> 4;
  const size_t nsb = (size_t)sb_count(L.w, L.h);
  const unsigned long long *t = L.table + (size_t)f * nsb * 16;
  unsigned long long s = 0;
  for (size_t sb = stripe; sb < nsb; sb += 16) s += t[sb * 16 + col];
  part[stripe][col] = s;
  __syncthreads();
  if (tid < 16) {
    s = 0;
    for (int k = 0; k < 16; k++) s += part[k][tid];
    total[tid] = s;
    L.sse[(size_t)f * 16 + tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    int pick[2];
    for (int g = 0; g < 2; g++) {
      pick[g] = 0;
      for (int c = 1; c < 8; c++) if (total[g * 8 + c] < total[g * 8 + pick[g]]) pick[g] = c;
      L.choice[(size_t)f * 2 + g] = (uint8_t)pick[g];
    }
    // (one aligned dword: what k_mi_levels_frames reads)
    *reinterpret_cast<uint32_t *>(L.levels + (size_t)f * 4) =
        (uint32_t)L.lvl[pick[0]][0] | (uint32_t)L.lvl[pick[0]][1] << 8 | (uint32_t)L.lvl[pick[1]][2] << 16 | (uint32_t)L.lvl[pick[1]][3] << 24;
  }
}

hipError_t launch_lf_search(const LfSearchLaunch &L, hipStream_t s) {
  const dim3 grid((unsigned)(sb_count(L.w, L.h) * L.nframes));   // 1-D: the kernel orders the tiles itself (xcd_tile)
  const bool s0 = L.sharpness == 0;
  if (L.bd == 8) { if (s0) hipLaunchKernelGGL((k_lf_search<uint8_t, true>), grid, dim3(256), 0, s, L); else hipLaunchKernelGGL((k_lf_search<uint8_t, false>), grid, dim3(256), 0, s, L); }
  else           { if (s0) hipLaunchKernelGGL((k_lf_search<uint16_t, true>), grid, dim3(256), 0, s, L); else hipLaunchKernelGGL((k_lf_search<uint16_t, false>), grid, dim3(256), 0, s, L); }
  return hipGetLastError();
}
hipError_t launch_lf_pick(const LfSearchLaunch &L, hipStream_t s) {
  hipLaunchKernelGGL(k_lf_pick, dim3((unsigned)L.nframes), dim3(256), 0, s, L);
  return hipGetLastError();
}

}  // namespace av1mi
