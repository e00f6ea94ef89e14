// levels_kernels.hip — k_mi_levels: the GOP session's side information follows the batch's quantiser (av1mi_gop_set_base_q_idx).
//
// The deblocking mode-info maps and the CDEF strength records are built on the host at av1mi_gop_open from the levels of ONE
// quantiser (gop_session.hip side_information).  A batch with another quantiser needs other levels in them, and nothing else: the
// geometry — transform sizes, edge bits, the "off screen: never filtered" words of a true size that is not a multiple of 8, the
// 32x32 / 16x16 transforms of a key frame's complete superblock rows — stays where the host put it.  So the kernel PATCHES the words
// in place on the main stream, ordered behind the previous batch's filters (the last readers) and in front of this batch's:
//     word = (word & keep) | bits        unless (word & hold) != 0
// A mode-info map:   keep = everything but the two level bytes (bits 8..23), bits = the levels, hold = bit 24 ("skipped inter block":
//                    in these maps only the off-screen words carry it, and their level stays 0).
// A CDEF record set: one dword per superblock, keep = hold = 0, bits = the four strength bytes.
// One launch covers up to three arrays (blockIdx.y), one dword per lane and trip, 16-byte accesses over the multiple-of-four head of
// an array and single dwords over what is left.  A plain streaming kernel of a few hundred kilobytes at the most, launched only when
// the quantiser changes: it has to be correct and asynchronous, not fast.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "av1mi_internal.hpp"

namespace av1mi {

__global__ __launch_bounds__(256) void k_mi_levels(LevelsLaunch L) {
  const LevelsLaunch::Array A = L.a[blockIdx.y];
  const uint32_t keep = A.keep, bits = A.bits, hold = A.hold;
  auto patch = [&](uint32_t v) { return (v & hold) ? v : ((v & keep) | bits); };
  const size_t n4 = A.n / 4, step = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint4 *p4 = reinterpret_cast<uint4 *>(A.words);      // (hipMalloc'd: 256-byte aligned)
  for (size_t i = first; i < n4; i += step) {
    uint4 v = p4[i];
    v.x = patch(v.x); v.y = patch(v.y); v.z = patch(v.z); v.w = patch(v.w);
    p4[i] = v;
  }
  for (size_t i = n4 * 4 + first; i < A.n; i += step) A.words[i] = patch(A.words[i]);
}

hipError_t launch_mi_levels(const LevelsLaunch &L, hipStream_t s) {
  if (L.arrays < 1 || L.arrays > 3) return hipErrorInvalidValue;
  size_t most = 0;
  for (int k = 0; k < L.arrays; k++) {
    if (!L.a[k].words) return hipErrorInvalidValue;
    most = L.a[k].n > most ? L.a[k].n : most;
  }
  // a lane per 16 bytes of the longest array, at most 256 workgroups (the loops stride over the rest)
  size_t blocks = (most / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : blocks > 256 ? 256 : blocks;
  hipLaunchKernelGGL(k_mi_levels, dim3((unsigned)blocks, (unsigned)L.arrays), dim3(256), 0, s, L);
  return hipGetLastError();
}

// The grid-wide sibling for the deblocking search (lf_search_kernel.hip): every frame of a batch gets a map of its own, the base map's
// words with the level bytes the search picked for THAT frame.  The bytes are read from levels[frame] in device memory (k_lf_pick wrote
// them on the same stream: no host round trip), the words from the base maps with their strides, and written densely.  blockIdx.y: luma
// / chroma map, blockIdx.z: the frame; a dword per lane and trip.
__global__ __launch_bounds__(256) void k_mi_levels_frames(LevelsFramesLaunch L) {
  const int k = blockIdx.y, f = blockIdx.z;
  if (!L.out[k]) return;
  const uint32_t lv = *reinterpret_cast<const uint32_t *>(L.levels + (size_t)f * 4);      // luma vertical, luma horizontal, U, V
  const uint32_t bits = k == 0 ? (lv & 0xFFFFu) << 8 : ((lv >> 16) & 255u) << 8 | ((lv >> 16) & 255u) << 16;      // (U and V share the chroma map: U's level)
  const uint32_t keep = ~0x00FFFF00u, hold = 1u << 24;
  const int cols = L.cols[k];
  const size_t n = (size_t)L.rows[k] * cols, step = (size_t)gridDim.x * blockDim.x;
  const uint32_t *base = L.base[k] + (size_t)f * L.frame_stride[k];
  uint32_t *out = L.out[k] + (size_t)f * n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const size_t r = i / cols;
    const uint32_t v = base[r * L.stride[k] + (i - r * cols)];
    out[i] = (v & hold) ? v : ((v & keep) | bits);
  }
}

hipError_t launch_mi_levels_frames(const LevelsFramesLaunch &L, hipStream_t s) {
  if (!L.levels || L.nframes < 1 || L.nframes > 65535 || (!L.out[0] && !L.out[1])) return hipErrorInvalidValue;
  size_t most = 0;
  for (int k = 0; k < 2; k++) {
    if (L.out[k] && (!L.base[k] || L.cols[k] < 1 || L.rows[k] < 1 || L.stride[k] < L.cols[k])) return hipErrorInvalidValue;
    const size_t n = L.out[k] ? (size_t)L.rows[k] * L.cols[k] : 0;
    most = n > most ? n : most;
  }
  size_t blocks = (most + 255) / 256;      // a lane per dword of the larger map, at most 256 workgroups a frame (the loop strides over the rest)
  blocks = blocks < 1 ? 1 : blocks > 256 ? 256 : blocks;
  hipLaunchKernelGGL(k_mi_levels_frames, dim3((unsigned)blocks, 2u, (unsigned)L.nframes), dim3(256), 0, s, L);
  return hipGetLastError();
}

}  // namespace av1mi
