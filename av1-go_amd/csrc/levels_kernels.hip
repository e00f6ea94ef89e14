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

}  // namespace av1mi
