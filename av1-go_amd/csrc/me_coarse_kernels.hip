// me_coarse_kernels.hip — the optional coarse motion search in front of k_me_int (include/av1mi.h "motion search"): a search centre
// per 64x64 tile of every stacked frame, found on quarter-resolution planes, so that the +-search_range integer search follows
// motion of up to coarse_range + search_range samples per frame.  Two gfx950 kernels:
//
//   k_me_down    both quarter planes of all stacked frames in one launch: Q[y][x] = (sum of the 4x4 samples' 8-bit views + 8) >> 4 for
//                the source luma and for the luma plane each frame predicts from (ref_plane: restored or CDEF).  A lane owns four
//                output samples: four rows of 16 input samples (one 16-byte load per row at 8 bits, two at 10) and ONE dword stored.
//   k_me_coarse  per tile the 16x16 block of the source's quarter plane against every displacement in [-Rc, Rc]^2 of the reference's,
//                SAD over all 256 samples.  Block and clamped window ((16 + 2 Rc)^2, rows padded to whole dwords) in LDS; a lane owns
//                (dy, four adjacent dx) and scores them with one v_qsad_pk_u16_u8 per four source samples, as k_me_int does; the 16-bit
//                packed accumulators hold the whole SAD (at most 256 x 255 = 65 280).  kTiles tiles share a workgroup and form ONE
//                item space, so the waves are full whatever Rc is (a tile alone has 3 items at Rc = 1, 297 at Rc = 16); the minimum
//                of (SAD << 16 | rank) per tile is an LDS atomic.
// The quarter planes live in a scratch area (me_layout) with rows padded to a multiple of 4 bytes, so that every store and
// every aligned window group is a dword; the padding columns hold the replicated last column and are never scored.
// Arithmetic and tie rules: include/av1mi.h; restated in numpy by tests/me_ref.py.  Reference tree: nothing (transcode.go:120).
#include "motion_common.hpp"

namespace av1mi {

namespace {
constexpr int kTiles = 4;          // tiles per workgroup of k_me_coarse
constexpr int kMaxRc = 16;
constexpr int kWinRows = 16 + 2 * kMaxRc, kWinStride = 4 * ((2 * kMaxRc + 1 + 3) / 4) + 20;      // 48 rows of 56 bytes
}

MeLayout me_layout(int w, int h, int nframes) {
  MeLayout M;
  M.qw = w / 4; M.qh = h / 4; M.qs = (M.qw + 3) & ~3;
  M.tiles = ((w + 63) / 64) * ((h + 63) / 64);
  const size_t plane = ((size_t)M.qs * M.qh * (size_t)nframes + 15) & ~(size_t)15;
  M.off_ref = plane; M.off_centres = 2 * plane;
  M.bytes = 2 * plane + (((size_t)M.tiles * (size_t)nframes * 4 + 15) & ~(size_t)15);
  return M;
}

// ------------------------------------------------------------------------------------------ quarter planes
// grid: (workgroups per plane) x 2 planes x nframes, in xcd_tile order: the frame and the plane are uniform in a workgroup
template <typename Pix>
__global__ __launch_bounds__(256) void k_me_down(InterLaunch L, uint8_t *qsrc, uint8_t *qref, int qw, int qh, int qs, int wgs) {
  constexpr int sh = sizeof(Pix) == 1 ? 0 : 2;
  const Tile3 tl = xcd_tile((unsigned)wgs, 2u, (unsigned)L.nframes);
  const int f = tl.z, pl = tl.y, ng = qs >> 2;
  const int item = tl.x * 256 + (int)threadIdx.x;
  if (item >= ng * qh) return;
  const int y = item / ng, x0 = (item - y * ng) * 4;           // output samples (x0 .. x0 + 3, y)
  const Pix *in = reinterpret_cast<const Pix *>(pl ? ref_plane(L, f, 0) : L.src[0]) + (size_t)f * L.h * L.stride_y;
  uint8_t *out = (pl ? qref : qsrc) + (size_t)f * qs * qh + (size_t)y * qs + x0;
  *reinterpret_cast<uint32_t *>(out) = quarter_dword<Pix>(in, L.stride_y, L.w, sh, x0, y);
}

// ------------------------------------------------------------------------------------------ coarse search
__global__ __launch_bounds__(256) void k_me_coarse(const uint8_t *qsrc, const uint8_t *qref, int16_t *centres, int qw, int qh, int qs, int sbw,
                                                    int sbh, int ntiles, int Rc) {
  __shared__ __attribute__((aligned(16))) uint8_t win[kTiles][kWinRows * kWinStride];
  __shared__ __attribute__((aligned(16))) uint8_t blk[kTiles][256];
  __shared__ uint32_t s_best[kTiles];
  const int tid = threadIdx.x;
  const int NC = 2 * Rc + 1, NG = (NC + 3) >> 2;          // displacements per row, groups of four dx starting at -Rc
  const int WR = 16 + 2 * Rc, WD = NG + 4;                // window rows; dwords per window row: columns -Rc .. 4 NG + 15 - Rc (clamped beyond +Rc)
  const int t0 = (int)xcd_swizzle(blockIdx.x, gridDim.x) * kTiles;
  const int per_frame = sbw * sbh;
  // staging, a dword per lane and step: the source block (16 rows of 4 dwords) and the window of every tile of the workgroup;
  // all coordinates clamped into the quarter plane (edge replication; covers partial tiles too)
  const int wdw = WR * WD, per_tile = 64 + wdw;
  for (int i = tid; i < kTiles * per_tile; i += 256) {
    const int k = i / per_tile, j = i - k * per_tile, t = t0 + k;
    if (t >= ntiles) break;
    const int f = t / per_frame, rem = t - f * per_frame, ty = rem / sbw, tx = rem - ty * sbw;
    const bool is_blk = j < 64;
    const int r = is_blk ? j >> 2 : (j - 64) / WD, c = is_blk ? (j & 3) * 4 : ((j - 64) - r * WD) * 4;
    const int fy = min(max(16 * ty + r - (is_blk ? 0 : Rc), 0), qh - 1), fx = 16 * tx + c - (is_blk ? 0 : Rc);
    const uint8_t *row = (is_blk ? qsrc : qref) + (size_t)f * qs * qh + (size_t)fy * qs;
    // (a window group starts at any byte, fx = 16 tx + c - Rc: inside the plane it is still one load of its four bytes)
    *reinterpret_cast<uint32_t *>(is_blk ? blk[k] + r * 16 + c : win[k] + r * kWinStride + c) = row_dword(row, fx, qw);
  }
  if (tid < kTiles) s_best[tid] = 0xFFFFFFFFu;
  __syncthreads();
  // items: (tile, dy, dx group).  An item reads, per block row, five window dwords and the row's four source dwords (the same
  // address in every lane of a tile: a broadcast) and issues four QSADs: 64 per item, four candidates each.
  const int items = NC * NG;
  for (int u = tid; u < kTiles * items; u += 256) {
    const int k = u / items, it = u - k * items;
    if (t0 + k >= ntiles) break;
    const int dyi = it / NG, g = it - dyi * NG;            // dy = dyi - Rc, dx = 4 g - Rc + {0, 1, 2, 3}
    const uint8_t *p = win[k] + dyi * kWinStride + 4 * g;
    unsigned long long acc = 0;
#pragma unroll 4
    for (int r = 0; r < 16; r++) {
      const uint32_t *q = reinterpret_cast<const uint32_t *>(p + r * kWinStride);
      const uint4 s = *reinterpret_cast<const uint4 *>(blk[k] + r * 16);
      const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
      acc = __builtin_amdgcn_qsad_pk_u16_u8((unsigned long long)w0 | ((unsigned long long)w1 << 32), s.x, acc);
      acc = __builtin_amdgcn_qsad_pk_u16_u8((unsigned long long)w1 | ((unsigned long long)w2 << 32), s.y, acc);
      acc = __builtin_amdgcn_qsad_pk_u16_u8((unsigned long long)w2 | ((unsigned long long)w3 << 32), s.z, acc);
      acc = __builtin_amdgcn_qsad_pk_u16_u8((unsigned long long)w3 | ((unsigned long long)w4 << 32), s.w, acc);
    }
    // key = SAD << 16 | rank: (0, 0) ranks first, the others in raster order; a dx beyond +Rc (the last group's padding) is left out
    unsigned best = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int dxi = 4 * g + i;
      const unsigned sad = (unsigned)(acc >> (16 * i)) & 0xffffu;
      const unsigned rank = (dyi == Rc && dxi == Rc) ? 0u : (unsigned)(1 + dyi * NC + dxi);
      if (dxi < NC) best = min(best, (sad << 16) | rank);
    }
    atomicMin(&s_best[k], best);
  }
  __syncthreads();
  if (tid < kTiles && t0 + tid < ntiles) {
    const int rank = (int)(s_best[tid] & 0xffffu);
    const int dy = rank ? (rank - 1) / NC - Rc : 0, dx = rank ? (rank - 1) % NC - Rc : 0;
    // one int16 pair per tile and frame, stored as the dword it is
    reinterpret_cast<uint32_t *>(centres)[t0 + tid] = (uint32_t)(uint16_t)(int16_t)(4 * dx) | ((uint32_t)(uint16_t)(int16_t)(4 * dy) << 16);
  }
}

// quarter planes + centres of L's stacked frames into `scratch` (me_layout(L.w, L.h, L.nframes).bytes, 16-byte aligned); Rc = coarse_range / 4
hipError_t launch_me_coarse(const InterLaunch &L, int coarse_range, void *scratch, hipStream_t s) {
  if (L.nframes <= 0) return hipSuccess;
  const MeLayout M = me_layout(L.w, L.h, L.nframes);
  uint8_t *qsrc = (uint8_t *)scratch, *qref = qsrc + M.off_ref;
  int16_t *centres = (int16_t *)(qsrc + M.off_centres);
  const int wgs = ((M.qs >> 2) * M.qh + 255) / 256;
  const dim3 g1((unsigned)(wgs * 2 * L.nframes));
  if (L.bd == 8) hipLaunchKernelGGL(k_me_down<uint8_t>, g1, dim3(256), 0, s, L, qsrc, qref, M.qw, M.qh, M.qs, wgs);
  else hipLaunchKernelGGL(k_me_down<uint16_t>, g1, dim3(256), 0, s, L, qsrc, qref, M.qw, M.qh, M.qs, wgs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int ntiles = M.tiles * L.nframes;
  hipLaunchKernelGGL(k_me_coarse, dim3((unsigned)((ntiles + kTiles - 1) / kTiles)), dim3(256), 0, s, qsrc, qref, centres, M.qw, M.qh, M.qs,
                     (L.w + 63) / 64, (L.h + 63) / 64, ntiles, coarse_range / 4);
  return hipGetLastError();
}

}  // namespace av1mi
