// telecine_kernels.hip — inverse telecine (include/av1mi.h "inverse telecine"): the field-match records of a run of frames, and the weave
// gather that stands where k_frames_gather (scene_kernels.hip) stands in a session that weaves.  Three gfx950 kernels:
//
//   k_telecine_rows    a workgroup owns a tile of kTilePairs line pairs (an even line and the odd line under it) x 64 cells of 16 bytes,
//                      and a chunk of up to kChunk consecutive frames of the run, which it WALKS: a wave owns kPairs pairs of the tile,
//                      a lane one cell of each of their lines.  The three candidates of frame f share B's lines, and T_c of frame f is
//                      T_n of f - 1 and T_p of f + 1: the even lines live in three register sets that roll as the walk advances, and the
//                      odd lines of frame f stay to be B_{f-1} of the next step.  So per frame a lane loads its even lines once (as T_n),
//                      its odd lines once, and one halo line (the odd line above its first pair, another wave's or workgroup's: an L2
//                      hit, its owner loads it in the same step).  A chunk's first step loads two frames more (T_p / T_c and B_{f-1}):
//                      the run is cut into chunks so that a short tile count still fills the device.  Per (frame, tile, wave) ONE lane
//                      writes four 32-bit partials (a lane's share of a frame is at most kPairs x 16 x 510, a wave's 64 times that).
//                      No LDS, no barrier, no atomics.
//   k_telecine_sum     one workgroup per frame adds the partials in an order fixed by geometry and writes the record; frame 0 of the
//                      run gets bdiff = 2^64 - 1.
//   k_telecine_gather  the weave: an item is (segment, plane, band of kBand output rows, group of 64 cells), a wave owns an item
//                      (gather_cells.hpp's geometry, cells and padding rule, shared with the deinterlacer); output row y is row
//                      min(y, h - 1) of the top source where that row is even, else of the bottom source: a straight copy of cells,
//                      dwordx4 where the plane's rows are whole 16-byte units, else dwords.
// Columns at or beyond the true width: a cell that straddles it is loaded whole (inside the buffer's row) and its samples beyond the
// edge are masked out of the sums / replaced by the last true column; rows at or beyond the true height are never loaded.  So no value
// at or beyond the true size enters a result.
// Arithmetic: include/av1mi.h; restated in numpy by tests/telecine_ref.py.  Reference tree: nothing (transcode.go:120).
#include "av1mi_internal.hpp"
#include "gather_cells.hpp"

namespace av1mi {

namespace {
constexpr int kPairs = 2;                    // line pairs per wave
constexpr int kTilePairs = 4 * kPairs;       // ... per workgroup: 16 rows
constexpr int kChunk = 16;                   // frames a workgroup walks

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }
}  // namespace

TelecineLayout telecine_layout(int bd, int w, int h, int frames) {
  TelecineLayout L;
  const int ns = bd == 8 ? 16 : 8;
  L.tiles_x = ((w + ns - 1) / ns + 63) / 64;
  L.tiles_y = ((h + 1) / 2 + kTilePairs - 1) / kTilePairs;
  L.chunks = (frames + kChunk - 1) / kChunk;
  L.per_frame = (size_t)L.tiles_x * L.tiles_y * 4;
  L.bytes = L.per_frame * (size_t)frames * 16;
  return L;
}

// grid: tiles_x x tiles_y x chunks, in xcd_tile order.  part: [frame][tile][wave] of uint4 (comb p, c, n, bdiff)
template <typename Pix>
__global__ __launch_bounds__(256) void k_telecine_rows(const Pix *luma, uint4 *part, int stride, int rows, int w, int h, int sh, int tiles_x, int tiles_y, int chunks,
                                                       int frames) {
  constexpr int NS = 16 / (int)sizeof(Pix);
  const Tile3 tl = xcd_tile((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)chunks);
  const unsigned lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t rb = (uint32_t)stride * (uint32_t)sizeof(Pix);
  const uint32_t cx = (uint32_t)tl.x * 64u + lane, off = cx * 16u;
  const bool active = off < (uint32_t)w * (uint32_t)sizeof(Pix), whole = !(rb & 15u);      // active: the cell holds a true column
  const int lastj = w - 1 - (int)cx * NS;             // samples j <= lastj of the cell are true columns
  const int k0 = (tl.y * 4 + (int)wave) * kPairs;     // the wave's first pair: lines 2 k0, 2 k0 + 1
  const int f0 = tl.z * kChunk, f1 = min(f0 + kChunk, frames);
  const size_t frame_bytes = (size_t)rows * rb;
  const char *base = reinterpret_cast<const char *>(luma);
  // line y of frame f: the lane's cell, zeros for a line at or beyond the true height (uniform in the wave) and for an inactive lane
  auto line = [&](int f, int y, uint32_t c[4]) { load_cell(base + (size_t)f * frame_bytes + (size_t)y * rb, off, rb, whole, active && y < h, c); };

  uint32_t Tp[kPairs][4], Tc[kPairs][4], Tn[kPairs][4], Bo[kPairs][4], Bq[kPairs][4], Bh[4] = { 0, 0, 0, 0 };
#pragma unroll
  for (int i = 0; i < kPairs; i++) {
    line(max(f0 - 1, 0), 2 * (k0 + i), Tp[i]);
    line(f0, 2 * (k0 + i), Tc[i]);
    line(max(f0 - 1, 0), 2 * (k0 + i) + 1, Bq[i]);
  }
#pragma unroll 1
  for (int f = f0; f < f1; f++) {
    const bool next = f + 1 < frames;                 // else T_n = T_c (uniform)
#pragma unroll
    for (int i = 0; i < kPairs; i++) {
      if (next) line(f + 1, 2 * (k0 + i), Tn[i]);
      else { Tn[i][0] = Tc[i][0]; Tn[i][1] = Tc[i][1]; Tn[i][2] = Tc[i][2]; Tn[i][3] = Tc[i][3]; }
      line(f, 2 * (k0 + i) + 1, Bo[i]);
    }
    if (k0 >= 1) line(f, 2 * k0 - 1, Bh);
    uint32_t cp = 0, cc = 0, cn = 0, bd = 0;
#pragma unroll
    for (int i = 0; i < kPairs; i++) {
      const int y = 2 * (k0 + i);
      const uint32_t *up = i == 0 ? Bh : Bo[i > 0 ? i - 1 : 0], *dn = Bo[i];
      if (y >= 2 && y <= h - 2) {                     // (uniform in the wave)
#pragma unroll
        for (int j = 0; j < NS; j++) {
          const int u = elem<Pix>(up, j) >> sh, d = elem<Pix>(dn, j) >> sh, e = iabs(u - d) + 8, s = u + d;
          const bool in = j <= lastj;
          const int a = iabs(2 * (elem<Pix>(Tp[i], j) >> sh) - s) - e, b = iabs(2 * (elem<Pix>(Tc[i], j) >> sh) - s) - e, c = iabs(2 * (elem<Pix>(Tn[i], j) >> sh) - s) - e;
          cp += in ? (uint32_t)max(a, 0) : 0u; cc += in ? (uint32_t)max(b, 0) : 0u; cn += in ? (uint32_t)max(c, 0) : 0u;
        }
      }
      if (f > 0 && y + 1 < h) {
#pragma unroll
        for (int j = 0; j < NS; j++) bd += j <= lastj ? (uint32_t)iabs((elem<Pix>(Bo[i], j) >> sh) - (elem<Pix>(Bq[i], j) >> sh)) : 0u;
      }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      cp += __shfl_xor(cp, m, 64); cc += __shfl_xor(cc, m, 64); cn += __shfl_xor(cn, m, 64); bd += __shfl_xor(bd, m, 64);
    }
    if (lane == 0) part[((size_t)f * tiles_y * tiles_x + (size_t)tl.y * tiles_x + tl.x) * 4 + wave] = make_uint4(cp, cc, cn, bd);
#pragma unroll
    for (int i = 0; i < kPairs; i++)
#pragma unroll
      for (int q = 0; q < 4; q++) { Tp[i][q] = Tc[i][q]; Tc[i][q] = Tn[i][q]; Bq[i][q] = Bo[i][q]; }
  }
}

// one workgroup per frame: lane i adds partials i, i + 256, ..., then the lanes' sums are folded in halves
__global__ __launch_bounds__(256) void k_telecine_sum(const uint4 *part, av1mi_telecine_record *out, unsigned per_frame) {
  __shared__ unsigned long long s[4][256];
  const int f = blockIdx.x, tid = threadIdx.x;
  unsigned long long a[4] = { 0, 0, 0, 0 };
  for (unsigned i = tid; i < per_frame; i += 256) {
    const uint4 v = part[(size_t)f * per_frame + i];
    a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) s[k][tid] = a[k];
  __syncthreads();
  for (int n = 128; n > 0; n >>= 1) {
    if (tid < n) {
#pragma unroll
      for (int k = 0; k < 4; k++) s[k][tid] += s[k][tid + n];
    }
    __syncthreads();
  }
  if (tid == 0) {
    av1mi_telecine_record r;
    r.comb[0] = s[0][0]; r.comb[1] = s[1][0]; r.comb[2] = s[2][0];
    r.bdiff = f == 0 ? ~0ull : s[3][0];
    out[f] = r;
  }
}

hipError_t launch_telecine_analyse(const TelecineLaunch &A, hipStream_t s) {
  if (A.frames <= 0) return hipSuccess;
  const TelecineLayout L = telecine_layout(A.bd, A.w, A.h, A.frames);
  const size_t grid = (size_t)L.tiles_x * L.tiles_y * L.chunks;
  if (grid > 0x7FFFFFFFu || L.per_frame > 0x7FFFFFFFu) return hipErrorInvalidValue;
  uint4 *part = (uint4 *)A.scratch;
  if (A.bd == 8)
    hipLaunchKernelGGL(k_telecine_rows<uint8_t>, dim3((unsigned)grid), dim3(256), 0, s, (const uint8_t *)A.luma, part, A.stride, A.rows, A.w, A.h, 0, L.tiles_x, L.tiles_y,
                       L.chunks, A.frames);
  else
    hipLaunchKernelGGL(k_telecine_rows<uint16_t>, dim3((unsigned)grid), dim3(256), 0, s, (const uint16_t *)A.luma, part, A.stride, A.rows, A.w, A.h, A.bd - 8, L.tiles_x,
                       L.tiles_y, L.chunks, A.frames);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_telecine_sum, dim3((unsigned)A.frames), dim3(256), 0, s, part, A.out, (unsigned)L.per_frame);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ the weave
namespace {
// gather_plane() of gather_cells.hpp for a table of TWO pointers per (segment, plane): C = the top source, N = the bottom source
__device__ __forceinline__ GatherPlane weave_plane(const BandGeom G, const void *const *table) {
  const unsigned seg = blockIdx.x / G.per_seg;
  unsigned wg = blockIdx.x - seg * G.per_seg;
  int p = 0;
  if (wg >= G.wgs[0]) { wg -= G.wgs[0]; p = 1; }
  if (p == 1 && wg >= G.wgs[1]) { wg -= G.wgs[1]; p = 2; }
#define PL(a) (p == 0 ? G.a[0] : p == 1 ? G.a[1] : G.a[2])
  GatherPlane W;
  W.seg = seg; W.wg = wg; W.p = p;
  W.rb = PL(row_bytes); W.cells = PL(cells); W.groups = PL(groups); W.items = PL(items);
  W.rows = PL(rows); W.w = PL(w); W.h = PL(h);
  W.dst = (char *)PL(dst) + (size_t)seg * PL(plane_bytes);
#undef PL
  const char *const *tab = reinterpret_cast<const char *const *>(table) + ((size_t)seg * 3 + p) * 2;
  W.P = nullptr; W.C = tab[0]; W.N = tab[1];
  return W;
}
}  // namespace

// grid: per_seg x segments; 4 waves = 4 consecutive items of one (segment, plane)
template <typename Pix>
__global__ __launch_bounds__(256) void k_telecine_gather(BandGeom G, const void *const *table) {
  constexpr int NS = 16 / (int)sizeof(Pix);
  const GatherPlane W = weave_plane(G, table);
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const unsigned item = W.wg * 4u + wave;
  if (item >= W.items) return;                   // (uniform in the wave; the kernel has no barrier)
  const GatherBand B = gather_band<NS>(W, item, lane);
  if (!W.C) { zero_band(W, B); return; }
  // four rows at a time: their loads are issued before the first of their stores (a band is kBand = 16 rows)
#pragma unroll 1
  for (int y0 = B.r0; y0 < B.r1; y0 += 4) {
    uint32_t c[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int y = y0 + k, ye = min(y, W.h - 1);
      if (y >= B.r1) break;                        // (uniform)
      const char *row = ((ye & 1) ? W.N : W.C) + (size_t)ye * W.rb;      // (h == 1: ye = 0, the top source)
      if (B.lastj >= 0) load_cell(row, B.off, W.rb, B.whole, B.active, c[k]);
      else if (B.active) {                         // a cell that lies wholly in the padding: the row's last true column
        uint32_t e = reinterpret_cast<const Pix *>(row)[W.w - 1];
        e = sizeof(Pix) == 1 ? e * 0x01010101u : e * 0x00010001u;
        c[k][0] = c[k][1] = c[k][2] = c[k][3] = e;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int y = y0 + k;
      if (y >= B.r1) break;
      if (B.lastj >= 0) pass_cell<Pix>(W, B, y, c[k]);
      else store_cell(W.dst + (size_t)y * W.rb, B.off, W.rb, B.whole, B.active, c[k]);
    }
  }
}

hipError_t launch_telecine_gather(const GatherPlanes &L, hipStream_t s) {
  BandGeom G;
  if (hipError_t e = band_geometry(L, false, G)) return e;
  if (L.segments <= 0 || !G.per_seg) return hipSuccess;
  const dim3 grid(G.per_seg * (unsigned)L.segments);
  if (L.bd == 8) hipLaunchKernelGGL(k_telecine_gather<uint8_t>, grid, dim3(256), 0, s, G, L.table);
  else hipLaunchKernelGGL(k_telecine_gather<uint16_t>, grid, dim3(256), 0, s, G, L.table);
  return hipGetLastError();
}

}  // namespace av1mi
