// noise_kernels.hip — the temporal noise of a source, measured on pairs of consecutive frames (include/av1mi.h "noise records"), from
// which the host plans the denoiser's strength (host/noiseplan.hpp).  Two gfx950 kernels:
//
//   k_noise_blocks  every luma sample of both planes of a pair that lies in a whole 8x8 block is read ONCE.  A workgroup owns a tile of
//                   kTileUnits 16-byte units x kTileBlockRows rows of blocks of one pair; a wave owns one row of blocks (8 lines), a lane
//                   one unit of each of its lines in both planes: 16 loads of 16 bytes in flight per lane, a wave's load of a line 1 KiB
//                   and coalesced.  A unit is two blocks wide at 8 bits and one at 16, so a block's S and M are sums over ONE lane's
//                   registers: no shuffle, no LDS reduction.  8 bits: v_sad_u8 against the other plane (S) and against 0 (M), two
//                   instructions per dword; 16 bits: v_sad_u16 the same way, M on the samples shifted to their m8 view first (shift,
//                   mask, sad).  The block's bin is counted in the workgroup's LDS histogram by an integer atomic (the order changes
//                   nothing), and the histogram leaves the workgroup as 256 partials, one writer each.
//                   A unit is loaded whole, 16 bytes at once; where the rows are whole 16-byte units that load is aligned, in rows that
//                   are not (8-bit widths that are 8 mod 16) it starts on every second row 8 bytes off.  An 8-bit unit whose second block
//                   is cut by the true width gives its first block's 8 bytes alone: nothing at or beyond the whole blocks is read.
//   k_noise_sum     one workgroup per pair, lane i owns bin i: the workgroups' partials added in an order fixed by geometry.  eligible
//                   is the sum of the bins (every eligible block is in exactly one).
// Arithmetic: include/av1mi.h; restated in numpy by tests/noise_ref.py.  Reference tree: nothing (transcode.go:120).
#include "av1mi_internal.hpp"

namespace av1mi {

namespace {
constexpr int kBins = 256;            // of a record's histogram: one per lane of a workgroup
constexpr int kTileUnits = 64;        // 16-byte units of a row per workgroup: one per lane of a wave
constexpr int kTileBlockRows = 4;     // rows of 8x8 blocks per workgroup: one per wave
constexpr uint32_t kLumaLow = 16 * 64, kLumaHigh = 235 * 64;      // a block is eligible iff its M lies in the nominal video range

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

// The lane's unit of one line.  full: all 16 bytes belong to whole blocks: ONE 16-byte load, declared with a dword's alignment and nothing
// more (crop_kernels.hip's idiom: the hardware takes a global dwordx4 load at any dword; rows that are whole 16-byte units make it an
// aligned one).  Else (8 bits only) the unit's first block alone: its 8 bytes, the second block's dwords zeros.
__device__ __forceinline__ void load_unit(const char *p, bool full, uint32_t c[4]) {
  if (full) {
    const u32x4_a4 v = *reinterpret_cast<const u32x4_a4 *>(p);
    c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
  } else {
    const u32x2_a4 v = *reinterpret_cast<const u32x2_a4 *>(p);
    c[0] = v.x; c[1] = v.y; c[2] = c[3] = 0;
  }
}

// grid: tiles_x x tiles_y x pairs, in xcd_tile order.  bw x bh: the whole blocks of the true size.  part: [pair][tile][bin]
template <typename Pix>
__global__ __launch_bounds__(256) void k_noise_blocks(const Pix *luma, uint32_t *part, int stride, int rows, int bw, int bh, int sh, int tiles_x, int tiles_y, int pairs) {
  constexpr int NB = sizeof(Pix) == 1 ? 2 : 1;      // blocks of a unit
  constexpr int DW = 4 / NB;                        // dwords of a block's line
  __shared__ uint32_t s_hist[kBins];
  const Tile3 tl = xcd_tile((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)pairs);
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  s_hist[tid] = 0;
  __syncthreads();
  const int by = tl.y * kTileBlockRows + (int)wave;      // (uniform in the wave)
  const uint32_t cx = (uint32_t)tl.x * kTileUnits + lane;
  const int nb = min(max(bw - (int)cx * NB, 0), NB);     // the unit's blocks that lie wholly inside the true width
  if (by < bh && nb > 0) {
    const uint32_t rb = (uint32_t)stride * (uint32_t)sizeof(Pix);
    const bool full = nb == NB;
    const size_t plane = (size_t)rows * rb;
    const char *a = reinterpret_cast<const char *>(luma) + (size_t)tl.z * 2 * plane + (size_t)(by * 8) * rb + (size_t)cx * 16u, *b = a + plane;
    const uint32_t keep = (0xffffu >> sh) * 0x00010001u;      // (16-bit) the m8 view of a dword's two samples
    uint32_t va[8][4], vb[8][4];
    if (full) {      // (ONE branch around the sixteen loads, not one around each)
#pragma unroll
      for (int r = 0; r < 8; r++) { load_unit(a + (size_t)r * rb, true, va[r]); load_unit(b + (size_t)r * rb, true, vb[r]); }
    } else {
#pragma unroll
      for (int r = 0; r < 8; r++) { load_unit(a + (size_t)r * rb, false, va[r]); load_unit(b + (size_t)r * rb, false, vb[r]); }
    }
    uint32_t S[NB], M[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) S[k] = M[k] = 0;
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if constexpr (sizeof(Pix) == 1) {
          S[q / DW] = __builtin_amdgcn_sad_u8(va[r][q], vb[r][q], S[q / DW]);
          M[q / DW] = __builtin_amdgcn_sad_u8(va[r][q], 0u, M[q / DW]);
        } else {
          S[0] = __builtin_amdgcn_sad_u16(va[r][q], vb[r][q], S[0]);
          M[0] = __builtin_amdgcn_sad_u16((va[r][q] >> sh) & keep, 0u, M[0]);
        }
      }
#pragma unroll
    for (int k = 0; k < NB; k++)
      if (k < nb && M[k] >= kLumaLow && M[k] <= kLumaHigh) atomicAdd(&s_hist[min((S[k] >> sh) >> 2, (uint32_t)kBins - 1u)], 1u);
  }
  __syncthreads();
  part[((size_t)tl.z * tiles_y * tiles_x + (size_t)tl.y * tiles_x + tl.x) * kBins + tid] = s_hist[tid];
}

// one workgroup per pair, lane i = bin i
__global__ __launch_bounds__(256) void k_noise_sum(const uint32_t *part, av1mi_noise_record *out, unsigned per_pair, uint32_t blocks) {
  __shared__ uint32_t s_eligible;
  const unsigned f = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_eligible = 0;
  __syncthreads();
  uint32_t s = 0;
  for (unsigned t = 0; t < per_pair; t++) s += part[((size_t)f * per_pair + t) * kBins + tid];
  out[f].hist[tid] = s;
  atomicAdd(&s_eligible, s);      // (an integer sum: the order changes nothing)
  __syncthreads();
  if (tid == 0) { out[f].eligible = s_eligible; out[f].blocks = blocks; }
}

}  // namespace

NoiseLayout noise_layout(int bd, int w, int h, int pairs) {
  NoiseLayout L;
  const int nb = bd == 8 ? 2 : 1;
  L.bw = w / 8; L.bh = h / 8;
  L.tiles_x = ((L.bw + nb - 1) / nb + kTileUnits - 1) / kTileUnits; L.tiles_y = (L.bh + kTileBlockRows - 1) / kTileBlockRows;
  L.bytes = (size_t)L.tiles_x * L.tiles_y * (size_t)pairs * kBins * 4;
  return L;
}

hipError_t launch_noise_analyse(const NoiseAnalyseLaunch &A, hipStream_t s) {
  if (A.pairs <= 0) return hipSuccess;
  const NoiseLayout L = noise_layout(A.bd, A.w, A.h, A.pairs);
  uint32_t *part = (uint32_t *)A.scratch;
  const size_t per_pair = (size_t)L.tiles_x * L.tiles_y, grid = per_pair * A.pairs;
  if (grid > 0x7FFFFFFFu) return hipErrorInvalidValue;
  if (grid > 0) {      // (a true size under 8 x 8 has no block: the records are zeros)
    if (A.bd == 8)
      hipLaunchKernelGGL(k_noise_blocks<uint8_t>, dim3((unsigned)grid), dim3(256), 0, s, (const uint8_t *)A.luma, part, A.stride, A.rows, L.bw, L.bh, 0, L.tiles_x, L.tiles_y,
                         A.pairs);
    else
      hipLaunchKernelGGL(k_noise_blocks<uint16_t>, dim3((unsigned)grid), dim3(256), 0, s, (const uint16_t *)A.luma, part, A.stride, A.rows, L.bw, L.bh, A.bd - 8, L.tiles_x,
                         L.tiles_y, A.pairs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_noise_sum, dim3((unsigned)A.pairs), dim3(256), 0, s, part, A.out, (unsigned)per_pair, (uint32_t)L.bw * (uint32_t)L.bh);
  return hipGetLastError();
}

}  // namespace av1mi
