// gather_cells.hpp — the frame that the filtering gathers share (k_deint_gather in deint_kernels.hip; k_denoise_gather and
// k_denoise_mc_gather in grain_kernels.hip): kernels that build a batch's fed buffers from the frame store and filter on the way.
//
//   cells     a 16-byte cell of a plane's row, one lane's share, loaded and stored whole (dwordx4) where the plane's rows are whole 16-byte
//             units, else dword by dword and the last cell partly: load_cell, store_cell; pack_cell and pass_cell for the padding rule.
//   geometry  BandGeom, the part of the kernel argument that all of them read, and band_geometry(), which fills it from a GatherPlanes
//             (av1mi_internal.hpp) and refuses what the kernels cannot take.
//   decode    gather_plane(): blockIdx.x -> (segment, plane, workgroup in the plane), that plane's scalars and its P, C, N.
//             gather_band(): item -> band and group, the lane's cell in it.  Neither returns from the kernel: the callers branch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "av1mi_internal.hpp"

namespace av1mi {
namespace {

constexpr int kBand = 16;      // output rows per item (even)

struct BandGeom {
  void *dst[3];
  uint32_t plane_bytes[3];     // of one segment's plane in the destination (= a frame's plane in the store)
  uint32_t row_bytes[3];       // multiples of 4
  int32_t rows[3];             // buffer rows
  int32_t w[3], h[3];          // true size in samples
  uint32_t cells[3];           // 16-byte cells per row (the last one may be partial)
  uint32_t groups[3];          // groups of 64 cells per row
  uint32_t items[3];           // groups x bands
  uint32_t wgs[3];             // workgroups per (segment, plane)
  uint32_t per_seg;
};

// the geometry of a launch over L's planes: an item is (band of kBand rows, group of 64 cells), a workgroup four items;
// hipErrorInvalidValue for what the kernels cannot take.  cell_rule: the last cell of a row must start inside the true width.  That does
// NOT follow from plane_w - true_w < 8 (8-bit rows of 20 samples with 13 true ones: the second cell starts at sample 16), and
// av1mi_deinterlace_gather takes such planes, so it is an option: the denoising kernels need it, the deinterlacer does not ask for it.
inline hipError_t band_geometry(const GatherPlanes &L, bool cell_rule, BandGeom &G) {
  const uint32_t bps = L.bd == 8 ? 1 : 2;
  G.per_seg = 0;
  for (int p = 0; p < 3; p++) {
    const size_t rb = (size_t)L.plane_w[p] * bps, bytes = rb * (size_t)L.plane_h[p];
    const bool have = L.plane_w[p] > 0 && L.plane_h[p] > 0;
    if (bytes > 0x7FFFFFF0u || (rb & 3)) return hipErrorInvalidValue;
    if (have && (L.true_w[p] < 1 || L.true_h[p] < 1 || L.true_w[p] > L.plane_w[p] || L.true_h[p] > L.plane_h[p] || L.plane_w[p] - L.true_w[p] >= 8 ||
                 L.plane_h[p] - L.true_h[p] >= 8))
      return hipErrorInvalidValue;
    G.dst[p] = L.dst[p]; G.plane_bytes[p] = have ? (uint32_t)bytes : 0; G.row_bytes[p] = (uint32_t)rb; G.rows[p] = L.plane_h[p]; G.w[p] = L.true_w[p]; G.h[p] = L.true_h[p];
    G.cells[p] = have ? (uint32_t)((rb + 15) >> 4) : 0;
    if (cell_rule && have && (size_t)(G.cells[p] - 1) * (16 / bps) > (size_t)L.true_w[p] - 1) return hipErrorInvalidValue;
    G.groups[p] = (G.cells[p] + 63) / 64;
    G.items[p] = have ? G.groups[p] * (uint32_t)((L.plane_h[p] + kBand - 1) / kBand) : 0;
    G.wgs[p] = (G.items[p] + 3) / 4;
    G.per_seg += G.wgs[p];
  }
  if (L.segments > 0 && (size_t)G.per_seg * L.segments > 0x7FFFFFFFu) return hipErrorInvalidValue;
  return hipSuccess;
}

// what a workgroup of a gather works on (grid: per_seg x segments); uniform in the workgroup
struct GatherPlane {
  unsigned seg, wg;            // the segment, the workgroup within (segment, plane)
  int p;
  uint32_t rb, cells, groups, items;
  int rows, w, h;
  char *dst;                   // the segment's plane in the destination
  const char *P, *C, *N;       // ... and in the frames before, at and after it (C null = a flat slot)
};
// (G by value, and plane p's elements selected, not indexed: an array of the kernel's argument that is indexed by a variable, or read
// through a reference on either side of a branch, goes to scratch)
__device__ __forceinline__ GatherPlane gather_plane(const BandGeom G, const void *const *table) {
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
  const char *const *tab = reinterpret_cast<const char *const *>(table) + ((size_t)seg * 3 + p) * 3;
  W.P = tab[0]; W.C = tab[1]; W.N = tab[2];
  return W;
}

// a lane's cell in an item of W (item < W.items), NS samples wide
struct GatherBand {
  uint32_t cx, off;            // the cell in its row, and its first byte
  bool active, whole;          // the cell exists; the plane's rows are whole cells
  int r0, r1;                  // the band's output rows [r0, r1)
  int x0, lastj;               // the cell's first sample, and the sample OF THE CELL that is the last true column (>= NS: the cell is all true)
};
template <int NS>
__device__ __forceinline__ GatherBand gather_band(const GatherPlane &W, unsigned item, unsigned lane) {
  GatherBand B;
  const unsigned band = item / W.groups, grp = item - band * W.groups;
  B.cx = grp * 64u + lane; B.off = B.cx * 16u;
  B.active = B.cx < W.cells; B.whole = !(W.rb & 15u);
  B.r0 = (int)band * kBand; B.r1 = min(B.r0 + kBand, W.rows);
  B.x0 = (int)B.cx * NS;
  B.lastj = W.w - 1 - B.x0;
  return B;
}

// the cell at byte `off` of a row of rb bytes; dwords beyond the row, and all of an inactive lane's, are 0
__device__ __forceinline__ void load_cell(const char *row, uint32_t off, uint32_t rb, bool whole, bool active, uint32_t c[4]) {
  c[0] = c[1] = c[2] = c[3] = 0;
  if (!active) return;
  if (whole) {
    const uint4 v = *reinterpret_cast<const uint4 *>(row + off);
    c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (off + 4u * q < rb) c[q] = *reinterpret_cast<const uint32_t *>(row + off + 4u * q);
  }
}
__device__ __forceinline__ void store_cell(char *row, uint32_t off, uint32_t rb, bool whole, bool active, const uint32_t c[4]) {
  if (!active) return;
  if (whole) *reinterpret_cast<uint4 *>(row + off) = make_uint4(c[0], c[1], c[2], c[3]);
  else {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (off + 4u * q < rb) *reinterpret_cast<uint32_t *>(row + off + 4u * q) = c[q];
  }
}

// sample i of packed dwords
template <typename Pix>
__device__ __forceinline__ int elem(const uint32_t *d, int i) {
  if constexpr (sizeof(Pix) == 1) return (int)((d[i >> 2] >> (8 * (i & 3))) & 0xffu);
  else return (int)((d[i >> 1] >> (16 * (i & 1))) & 0xffffu);
}
// samples of a cell -> its dwords, the columns beyond the true width (sample index above `lastj`) repeating the last true one
template <typename Pix, int NS, typename T>
__device__ __forceinline__ void pack_cell(T o[NS], int lastj, uint32_t c[4]) {
#pragma unroll
  for (int j = 1; j < NS; j++) o[j] = j > lastj ? o[j - 1] : o[j];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    if constexpr (sizeof(Pix) == 1) c[q] = (uint32_t)o[4 * q] | (uint32_t)o[4 * q + 1] << 8 | (uint32_t)o[4 * q + 2] << 16 | (uint32_t)o[4 * q + 3] << 24;
    else c[q] = (uint32_t)o[2 * q] | (uint32_t)o[2 * q + 1] << 16;
  }
}

// a flat slot: the band's output rows are zeros
__device__ __forceinline__ void zero_band(const GatherPlane &W, const GatherBand &B) {
  const uint32_t z[4] = { 0, 0, 0, 0 };
  for (int y = B.r0; y < B.r1; y++) store_cell(W.dst + (size_t)y * W.rb, B.off, W.rb, B.whole, B.active, z);
}
// output row y takes the cell c of a source row as it is, its padding repeating the last true column
template <typename Pix>
__device__ __forceinline__ void pass_cell(const GatherPlane &W, const GatherBand &B, int y, uint32_t c[4]) {
  constexpr int NS = 16 / (int)sizeof(Pix);
  if (B.lastj < NS - 1) {                        // the cell reaches into the padding
    int o[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) o[j] = elem<Pix>(c, j);
    pack_cell<Pix, NS>(o, B.lastj, c);
  }
  store_cell(W.dst + (size_t)y * W.rb, B.off, W.rb, B.whole, B.active, c);
}

}  // namespace
}  // namespace av1mi
