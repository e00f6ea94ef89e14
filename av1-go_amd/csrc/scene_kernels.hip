// scene_kernels.hip — the scene analysis and the frame gather behind av1mi_gop_config.store_frames (include/av1mi.h "scene analysis").
// Four gfx950 kernels:
//
//   k_scene_down    the quarter planes of a stack of luma planes: k_me_down's arithmetic (me_coarse_kernels.hip) on ONE plane per frame.
//                   That kernel's grid is (source, reference) x frames and reads an InterLaunch; this sibling takes a plain pointer, so
//                   the search's instantiations stay what they are.  A lane owns four output samples: four rows of 16 input samples and
//                   ONE dword stored.
//   k_scene_blocks  per block of 8x8 quarter samples (32x32 luma) of frame f: inter = the smallest SAD against Q_{f-1} displaced by
//                   [-2, 2]^2, intra = the SAD against the block's own mean.  A workgroup owns (frame, block row, a run of up to kRun
//                   blocks): the 8 rows of Q_f and the 12-row window of Q_{f-1}, both clamped into the plane, are staged in LDS as whole
//                   dwords.  An item is (block, dy): per block row two source dwords against four window dwords, the five dx side by
//                   side: dx -2 .. 1 on one v_qsad_pk_u16_u8 per source dword, dx 2 on v_sad_u8.  The packed 16-bit accumulators hold a
//                   block's whole SAD (64 x 255 = 16 320).  The minimum over a block's five items is an LDS atomic (a minimum of integers:
//                   the order changes nothing).  Results per block go to scratch.
//   k_scene_sum     one workgroup per frame adds the blocks' pairs in an order fixed by geometry and writes the record.
//   k_frames_gather the planes of a batch from a table of per-(segment, plane) source pointers into the stacked fed buffers, ONE
//                   launch; a null pointer is a flat slot and is written as zeros.  A lane owns 16 bytes, a wave a contiguous run.
// Arithmetic: include/av1mi.h; restated in numpy by tests/scene_ref.py.  Reference tree: nothing (transcode.go:120).
#include "motion_common.hpp"

namespace av1mi {

namespace {
constexpr int kRun = 48;                         // blocks of a block row per workgroup: 48 x 5 = 240 items for 256 lanes
constexpr int kCurStride = kRun * 8 + 8;         // bytes: 98 dwords, an odd number of dword pairs (rows start two banks apart)
constexpr int kWinStride = kRun * 8 + 8 + 8;     // the window has 4 columns more on either side: (kRun * 8 + 8) bytes used, 100 dwords
constexpr int kGatherUnroll = 4;                 // 16-byte units per lane of k_frames_gather
}

SceneLayout scene_layout(int w, int h, int frames) {
  SceneLayout L;
  L.qw = w / 4; L.qh = h / 4; L.qs = (L.qw + 3) & ~3;
  L.nbx = (w + 31) / 32; L.nby = (h + 31) / 32;
  const size_t planes = ((size_t)L.qs * L.qh * (size_t)frames + 15) & ~(size_t)15;
  L.off_blocks = planes;
  L.bytes = planes + (size_t)L.nbx * L.nby * (size_t)frames * 8;
  return L;
}

// ------------------------------------------------------------------------------------------ quarter planes
// grid: (workgroups per plane) x frames, in xcd_tile order: the frame is uniform in a workgroup
template <typename Pix>
__global__ __launch_bounds__(256) void k_scene_down(const Pix *luma, uint8_t *q, int w, int h, int sh, int qh, int qs, int wgs, int frames) {
  const Tile3 tl = xcd_tile((unsigned)wgs, 1u, (unsigned)frames);
  const int f = tl.z, ng = qs >> 2;
  const int item = tl.x * 256 + (int)threadIdx.x;
  if (item >= ng * qh) return;
  const int y = item / ng, x0 = (item - y * ng) * 4;           // output samples (x0 .. x0 + 3, y)
  uint8_t *out = q + (size_t)f * qs * qh + (size_t)y * qs + x0;
  *reinterpret_cast<uint32_t *>(out) = quarter_dword<Pix>(luma + (size_t)f * h * w, w, w, sh, x0, y);
}

// ------------------------------------------------------------------------------------------ blocks
// grid: runs x block rows x frames
__global__ __launch_bounds__(256) void k_scene_blocks(const uint8_t *q, uint2 *blocks, int qw, int qh, int qs, int nbx, int nby, int runs, int frames) {
  __shared__ __attribute__((aligned(16))) uint8_t cur[8 * kCurStride];
  __shared__ __attribute__((aligned(16))) uint8_t win[12 * kWinStride];
  __shared__ uint32_t s_inter[kRun];
  const Tile3 tl = xcd_tile((unsigned)runs, (unsigned)nby, (unsigned)frames);
  const int f = tl.z, by = tl.y, b0 = tl.x * kRun, nb = min(kRun, nbx - b0), tid = threadIdx.x;
  const int x0 = 8 * b0;                                        // first column of the run
  const uint8_t *qf = q + (size_t)f * qs * qh;
  // staging, a dword per lane and step.  cur: 8 rows of 2 nb dwords, dword i = columns x0 + 4 i ..; win (f > 0): 12 rows (-2 .. 9) of
  // 2 nb + 2 dwords, dword j = columns x0 - 4 + 4 j ..: a block's window starts on a dword.  Every coordinate clamped into the plane.
  const int cd = 2 * nb, wd = 2 * nb + 2, ncur = 8 * cd, nwin = f > 0 ? 12 * wd : 0;
  for (int i = tid; i < ncur + nwin; i += 256) {
    if (i < ncur) {
      const int r = i / cd, c = i - r * cd;
      const int y = min(8 * by + r, qh - 1);
      *reinterpret_cast<uint32_t *>(cur + r * kCurStride + 4 * c) = row_dword(qf + (size_t)y * qs, x0 + 4 * c, qw);
    } else {
      const int j = i - ncur, r = j / wd, c = j - r * wd;
      const int y = min(max(8 * by - 2 + r, 0), qh - 1);
      *reinterpret_cast<uint32_t *>(win + r * kWinStride + 4 * c) = row_dword(qf - (size_t)qs * qh + (size_t)y * qs, x0 - 4 + 4 * c, qw);
    }
  }
  if (tid < kRun) s_inter[tid] = f > 0 ? 0xFFFFFFFFu : 0u;
  __syncthreads();
  // items (dy, block): consecutive lanes take consecutive blocks, 8 bytes apart in either array
  if (f > 0) {
    for (int it = tid; it < 5 * nb; it += 256) {
      const int dyi = it / nb, b = it - dyi * nb;               // dy = dyi - 2
      unsigned long long acc = 0;
      uint32_t acc4 = 0;
#pragma unroll
      for (int r = 0; r < 8; r++) {
        const uint2 c = *reinterpret_cast<const uint2 *>(cur + r * kCurStride + 8 * b);
        // columns 8 b - 4 .. 8 b + 11 of the run, as two 8-byte reads (a block's window starts 8 bytes, not 16, after its neighbour's)
        const uint2 v = *reinterpret_cast<const uint2 *>(win + (r + dyi) * kWinStride + 8 * b);
        const uint2 t = *reinterpret_cast<const uint2 *>(win + (r + dyi) * kWinStride + 8 * b + 8);
        // the window from column 8 b - 2 on: a0 = columns -2 .. 1, a1 = 2 .. 5, a2 = 6 .. 9 (relative to the block)
        const uint32_t a0 = __builtin_amdgcn_alignbyte(v.y, v.x, 2), a1 = __builtin_amdgcn_alignbyte(t.x, v.y, 2), a2 = __builtin_amdgcn_alignbyte(t.y, t.x, 2);
        acc = __builtin_amdgcn_qsad_pk_u16_u8((unsigned long long)a0 | ((unsigned long long)a1 << 32), c.x, acc);      // dx -2 .. 1
        acc = __builtin_amdgcn_qsad_pk_u16_u8((unsigned long long)a1 | ((unsigned long long)a2 << 32), c.y, acc);
        acc4 = __builtin_amdgcn_sad_u8(a1, c.x, acc4);                                                                  // dx 2
        acc4 = __builtin_amdgcn_sad_u8(a2, c.y, acc4);
      }
      uint32_t best = acc4;
#pragma unroll
      for (int i = 0; i < 4; i++) best = min(best, (uint32_t)(acc >> (16 * i)) & 0xffffu);
      atomicMin(&s_inter[b], best);
    }
  }
  __syncthreads();
  if (tid < nb) {
    uint32_t sum = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint2 c = *reinterpret_cast<const uint2 *>(cur + r * kCurStride + 8 * tid);
      sum = __builtin_amdgcn_sad_u8(c.x, 0u, sum);
      sum = __builtin_amdgcn_sad_u8(c.y, 0u, sum);
    }
    const uint32_t m = ((sum + 32) >> 6) * 0x01010101u;
    uint32_t intra = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint2 c = *reinterpret_cast<const uint2 *>(cur + r * kCurStride + 8 * tid);
      intra = __builtin_amdgcn_sad_u8(c.x, m, intra);
      intra = __builtin_amdgcn_sad_u8(c.y, m, intra);
    }
    blocks[((size_t)f * nby + by) * nbx + b0 + tid] = make_uint2(s_inter[tid], intra);
  }
}

// one workgroup per frame: lane i adds blocks i, i + 256, ..., then the lanes' sums are folded in halves
__global__ __launch_bounds__(256) void k_scene_sum(const uint2 *blocks, av1mi_scene_record *out, int per_frame) {
  __shared__ unsigned long long s_a[256], s_b[256];
  const int f = blockIdx.x, tid = threadIdx.x;
  unsigned long long a = 0, b = 0;
  for (int i = tid; i < per_frame; i += 256) {
    const uint2 v = blocks[(size_t)f * per_frame + i];
    a += v.x; b += v.y;
  }
  s_a[tid] = a; s_b[tid] = b;
  __syncthreads();
  for (int n = 128; n > 0; n >>= 1) {
    if (tid < n) { s_a[tid] += s_a[tid + n]; s_b[tid] += s_b[tid + n]; }
    __syncthreads();
  }
  if (tid == 0) {
    av1mi_scene_record r;
    r.inter_sad = s_a[0]; r.intra_sad = s_b[0]; r.blocks = (uint32_t)per_frame; r.reserved = 0;
    out[f] = r;
  }
}

hipError_t launch_scene(const SceneLaunch &S, hipStream_t s) {
  if (S.frames <= 0) return hipSuccess;
  const SceneLayout L = scene_layout(S.w, S.h, S.frames);
  uint8_t *q = (uint8_t *)S.scratch;
  uint2 *blocks = (uint2 *)(q + L.off_blocks);
  const int wgs = ((L.qs >> 2) * L.qh + 255) / 256;
  const size_t g1 = (size_t)wgs * S.frames, runs = (size_t)(L.nbx + kRun - 1) / kRun, g2 = runs * L.nby * S.frames;
  if (g1 > 0x7FFFFFFFu || g2 > 0x7FFFFFFFu) return hipErrorInvalidValue;
  const int sh = S.bd - 8;
  if (S.bd == 8) hipLaunchKernelGGL(k_scene_down<uint8_t>, dim3((unsigned)g1), dim3(256), 0, s, (const uint8_t *)S.luma, q, S.w, S.h, sh, L.qh, L.qs, wgs, S.frames);
  else hipLaunchKernelGGL(k_scene_down<uint16_t>, dim3((unsigned)g1), dim3(256), 0, s, (const uint16_t *)S.luma, q, S.w, S.h, sh, L.qh, L.qs, wgs, S.frames);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_scene_blocks, dim3((unsigned)g2), dim3(256), 0, s, q, blocks, L.qw, L.qh, L.qs, L.nbx, L.nby, (int)runs, S.frames);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_scene_sum, dim3((unsigned)S.frames), dim3(256), 0, s, blocks, S.out, L.nbx * L.nby);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ gather
struct GatherGeom {
  void *dst[3];
  uint32_t bytes[3];      // of one segment's plane, multiples of 4
  uint32_t wgs[3];        // workgroups per (segment, plane)
  uint32_t per_seg;       // wgs[0] + wgs[1] + wgs[2]
  int segments;
};

// grid: per_seg x segments.  Segment and plane are uniform in a workgroup; the workgroup owns a run of 256 * kGatherUnroll units of 16
// bytes, a wave 64 consecutive units of it at a time.  A plane that is not whole units (never the session's: its planes are multiples
// of 16 bytes) is moved in single dwords, four per lane.
__global__ __launch_bounds__(256) void k_frames_gather(GatherGeom G, const void *const *table) {
  const unsigned seg = blockIdx.x / G.per_seg;
  unsigned wg = blockIdx.x - seg * G.per_seg;
  int p = 0;
  if (wg >= G.wgs[0]) { wg -= G.wgs[0]; p = 1; }
  if (p == 1 && wg >= G.wgs[1]) { wg -= G.wgs[1]; p = 2; }
  const uint32_t bytes = p == 0 ? G.bytes[0] : p == 1 ? G.bytes[1] : G.bytes[2];
  const char *src = (const char *)table[seg * 3 + p];
  char *dst = (char *)(p == 0 ? G.dst[0] : p == 1 ? G.dst[1] : G.dst[2]) + (size_t)seg * bytes;
  const bool whole = !(bytes & 15u);
  const uint32_t units = (bytes + 15u) >> 4;
#pragma unroll
  for (int k = 0; k < kGatherUnroll; k++) {
    const uint32_t u = (wg * kGatherUnroll + k) * 256u + threadIdx.x;
    if (u >= units) break;
    if (whole) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (src) v = *reinterpret_cast<const uint4 *>(src + (size_t)u * 16);
      *reinterpret_cast<uint4 *>(dst + (size_t)u * 16) = v;
    } else {
      for (uint32_t o = u * 16u; o < min(u * 16u + 16u, bytes); o += 4)
        *reinterpret_cast<uint32_t *>(dst + o) = src ? *reinterpret_cast<const uint32_t *>(src + o) : 0u;
    }
  }
}

hipError_t launch_frames_gather(const size_t plane_bytes[3], int segments, const void *const *table, void *const dst[3], hipStream_t s) {
  GatherGeom G;
  G.per_seg = 0; G.segments = segments;
  for (int p = 0; p < 3; p++) {
    if (plane_bytes[p] > 0x7FFFFFF0u || (plane_bytes[p] & 3)) return hipErrorInvalidValue;
    G.dst[p] = dst[p]; G.bytes[p] = (uint32_t)plane_bytes[p];
    G.wgs[p] = (uint32_t)((((plane_bytes[p] + 15) >> 4) + 256 * kGatherUnroll - 1) / (256 * kGatherUnroll));
    G.per_seg += G.wgs[p];
  }
  if (segments <= 0 || !G.per_seg) return hipSuccess;
  if ((size_t)G.per_seg * segments > 0x7FFFFFFFu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_frames_gather, dim3(G.per_seg * (unsigned)segments), dim3(256), 0, s, G, table);
  return hipGetLastError();
}

}  // namespace av1mi
