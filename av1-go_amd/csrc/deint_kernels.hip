// deint_kernels.hip — the deinterlacing gather behind av1mi_gop_config.deinterlace (include/av1mi.h "deinterlacing"): k_deint_gather
// stands where k_frames_gather (scene_kernels.hip) stands in a session that does not deinterlace.  ONE launch builds the fed buffers of
// a batch from the frame store, and on the way replaces the lines of every frame's second field.
//
//   work      an item is (segment, plane, band of kBand output rows, group of 64 cells); a cell is 16 bytes of a row, one lane's.  A wave
//             owns an item, a workgroup four consecutive items of one (segment, plane): both are uniform in a workgroup.
//   rows      the wave walks down its band.  Per kept row it holds a SET in registers: the C row's cell with 3 samples on either side, and
//             the cells of the same row of P and N.  A missing row y needs the sets of rows up and dn plus the cells P[y] and C[y]; the set
//             that was dn becomes up two rows later, so inside a band every row of C, P and N is loaded once (a band re-reads the one kept
//             row above it).  Kept rows are stored from the set's own cell: a straight copy.
//   columns   the 3 samples beside a cell are the neighbouring lanes' edge dwords, moved by ds_bpermute_b32 (the LDS crossbar; no LDS
//             memory is allocated).  Lanes 0 and 63 of a wave, whose neighbour is another wave's, load those dwords (1 at 8 bits, 2 at 16)
//             from memory.  At the plane's true edge the window is clamped in registers; nothing beyond the buffer's row is read.
//   tails     a plane whose rows are whole 16-byte units moves in dwordx4; any other (rows are always whole dwords) in single dwords,
//             the last cell of a row partly.
//   padding   output columns beyond the true width repeat the last true column's OUTPUT, output rows beyond the true height the last
//             true row's: both by construction (a row y >= h is computed as row h - 1).  The input's padding is never used.
//   fields    k_deint_gather<Pix, true> is the field-rate launch (av1mi_gop_config.deinterlace_fields): a phase per segment, 0 = the frame's
//             first field (the same-rate filter), 1 = its second (the opposite parity kept, t0 / t1 from C / N).  The phase is read once
//             per workgroup and only picks a parity and two row pointers: the row loop, its loads and its arithmetic are shared.
// The launch geometry, the decode of blockIdx.x and of an item, the cells and the padding rule are gather_cells.hpp's, shared with the
// denoising gathers (grain_kernels.hip); here: the sets, the window and the filter.
// Arithmetic: include/av1mi.h; restated in numpy by tests/deinterlace_ref.py.  Reference tree: nothing (transcode.go:120).
#include <type_traits>
#include "av1mi_internal.hpp"
#include "gather_cells.hpp"

namespace av1mi {

namespace {
struct DeintGeom : BandGeom { int parity; };
// the field-rate launch (include/av1mi.h "field-rate output"): a phase per segment beside the session's parity; only its low bit is read
struct DeintFieldsGeom : DeintGeom { const uint8_t *phase; };

// one kept row as the filter needs it: the C row's cell with HD dwords on either side (c[HD .. HD + 3] is the cell), and the cells of the
// same row of P and N
template <int ND>
struct RowSet { uint32_t c[ND], p[4], n[4]; };

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

}  // namespace

// grid: per_seg x segments; 4 waves = 4 consecutive items of one (segment, plane).  FIELDS: the segment's phase (uniform in the workgroup)
// picks the kept parity and the temporal pair (P, C) or (C, N) once, in front of the row loop; the loop itself is the same-rate one
template <typename Pix, bool FIELDS>
__global__ __launch_bounds__(256) void k_deint_gather(typename std::conditional<FIELDS, DeintFieldsGeom, DeintGeom>::type G, const void *const *table) {
  constexpr int NS = 16 / (int)sizeof(Pix);      // samples per cell
  constexpr int HD = (int)sizeof(Pix);           // dwords that hold 3 samples beside a cell (they hold 4)
  constexpr int ND = 4 + 2 * HD;
  constexpr int NW = NS + 6;                     // the window: samples x0 - 3 .. x0 + NS + 2
  const GatherPlane W = gather_plane(G, table);
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const unsigned item = W.wg * 4u + wave;
  if (item >= W.items) return;                   // (uniform in the wave; the kernel has no barrier)
  const GatherBand B = gather_band<NS>(W, item, lane);
  if (!W.C) { zero_band(W, B); return; }
  const uint32_t rb = W.rb, cells = W.cells, cx = B.cx, off = B.off;
  const bool active = B.active, whole = B.whole;
  const char *P = W.P, *C = W.C, *N = W.N;
  int k = G.parity;
  const char *T0 = P, *T1 = C;                   // the rows of t0 and t1: one field before and one field after the missing one
  if constexpr (FIELDS) {
    const int phi = __builtin_amdgcn_readfirstlane(G.phase[W.seg] & 1);
    k ^= phi;
    T0 = phi ? C : P; T1 = phi ? N : C;
  }
  const int h = W.h, lastj = B.lastj;
  const bool first_cell = cx == 0, edge = first_cell || lastj < NS + 2;

  // the set of kept row r
  auto load_set = [&](RowSet<ND> &S, int r) {
    const size_t ro = (size_t)r * rb;
    uint32_t cell[4];
    load_cell(C + ro, off, rb, whole, active, cell);
    load_cell(P + ro, off, rb, whole, active, S.p);
    load_cell(N + ro, off, rb, whole, active, S.n);
#pragma unroll
    for (int q = 0; q < 4; q++) S.c[HD + q] = cell[q];
#pragma unroll
    for (int q = 0; q < HD; q++) {               // every lane of the wave is here: the branch around load_set is uniform
      S.c[q] = __shfl_up(cell[4 - HD + q], 1);
      S.c[HD + 4 + q] = __shfl_down(cell[q], 1);
    }
    if (lane == 0 && active && cx > 0) {         // the neighbours are another wave's
#pragma unroll
      for (int q = 0; q < HD; q++) S.c[q] = *reinterpret_cast<const uint32_t *>(C + ro + off - 4u * (HD - q));
    }
    if (lane == 63 && cx + 1 < cells) {
#pragma unroll
      for (int q = 0; q < HD; q++) S.c[HD + 4 + q] = off + 16u + 4u * q < rb ? *reinterpret_cast<const uint32_t *>(C + ro + off + 16u + 4u * q) : 0u;
    }
  };
  // the window of a set's C row, clamped at the true edge
  auto window = [&](const RowSet<ND> &S, int W[NW]) {
#pragma unroll
    for (int i = 0; i < NW; i++) W[i] = elem<Pix>(S.c, i + (4 / (int)sizeof(Pix)) * HD - 3);
    if (edge) {
      if (first_cell) W[0] = W[1] = W[2] = W[3];
#pragma unroll
      for (int i = 4; i < NW; i++) W[i] = i > lastj + 3 ? W[i - 1] : W[i];
    }
  };

  RowSet<ND> up, dn;
  int held_up = -1, held_dn = -1;
#pragma unroll 1
  for (int y = B.r0; y < B.r1; y++) {
    const int ye = min(y, h - 1);
    if (h == 1 || (ye & 1) == k) {               // a kept row
      if (ye != held_dn) { load_set(dn, ye); held_dn = ye; }
      uint32_t c[4] = { dn.c[HD], dn.c[HD + 1], dn.c[HD + 2], dn.c[HD + 3] };
      pass_cell<Pix>(W, B, y, c);
      continue;
    }
    const int ur = ye >= 1 ? ye - 1 : ye + 1, dr = ye + 1 <= h - 1 ? ye + 1 : ye - 1;
    if (ur != held_up) {
      if (ur == held_dn) up = dn; else load_set(up, ur);
      held_up = ur;
    }
    if (dr != held_dn) {
      if (dr == ur) dn = up; else load_set(dn, dr);
      held_dn = dr;
    }
    uint32_t py[4], cy[4];
    load_cell(T0 + (size_t)ye * rb, off, rb, whole, active, py);
    load_cell(T1 + (size_t)ye * rb, off, rb, whole, active, cy);
    int A[NW], B[NW], o[NS];
    window(up, A);
    window(dn, B);
#pragma unroll
    for (int j = 0; j < NS; j++) {
      const int c = j + 3;
      int best = iabs(A[c - 1] - B[c - 1]) + iabs(A[c] - B[c]) + iabs(A[c + 1] - B[c + 1]), ba = A[c], bb = B[c];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int d = i == 0 ? -1 : i == 1 ? 1 : i == 2 ? -2 : 2;
        const int sc = iabs(A[c - 1 + d] - B[c - 1 - d]) + iabs(A[c + d] - B[c - d]) + iabs(A[c + 1 + d] - B[c + 1 - d]);
        const bool better = sc < best;
        best = better ? sc : best; ba = better ? A[c + d] : ba; bb = better ? B[c - d] : bb;
      }
      const int s = (ba + bb + 1) >> 1;
      const int t0 = elem<Pix>(py, j), t1 = elem<Pix>(cy, j), t = (t0 + t1 + 1) >> 1;
      int m = (iabs(t0 - t1) + 1) >> 1;
      m = max(m, (iabs(elem<Pix>(up.p, j) - A[c]) + iabs(elem<Pix>(dn.p, j) - B[c]) + 1) >> 1);
      m = max(m, (iabs(elem<Pix>(up.n, j) - A[c]) + iabs(elem<Pix>(dn.n, j) - B[c]) + 1) >> 1);
      o[j] = min(max(s, t - m), t + m);
    }
    uint32_t c[4];
    pack_cell<Pix, NS>(o, lastj, c);
    store_cell(W.dst + (size_t)y * rb, off, rb, whole, active, c);
  }
}

hipError_t launch_deint_gather(const DeintLaunch &L, hipStream_t s) {
  DeintGeom G;
  G.parity = L.parity;
  if (hipError_t e = band_geometry(L, false, G)) return e;
  if (L.segments <= 0 || !G.per_seg) return hipSuccess;
  const dim3 grid(G.per_seg * (unsigned)L.segments);
  if (L.bd == 8) hipLaunchKernelGGL((k_deint_gather<uint8_t, false>), grid, dim3(256), 0, s, G, L.table);
  else hipLaunchKernelGGL((k_deint_gather<uint16_t, false>), grid, dim3(256), 0, s, G, L.table);
  return hipGetLastError();
}

hipError_t launch_deint_gather_fields(const DeintFieldsLaunch &L, hipStream_t s) {
  DeintFieldsGeom G;
  G.parity = L.parity; G.phase = L.phase;
  if (hipError_t e = band_geometry(L, false, G)) return e;
  if (L.segments <= 0 || !G.per_seg) return hipSuccess;
  const dim3 grid(G.per_seg * (unsigned)L.segments);
  if (L.bd == 8) hipLaunchKernelGGL((k_deint_gather<uint8_t, true>), grid, dim3(256), 0, s, G, L.table);
  else hipLaunchKernelGGL((k_deint_gather<uint16_t, true>), grid, dim3(256), 0, s, G, L.table);
  return hipGetLastError();
}

}  // namespace av1mi
