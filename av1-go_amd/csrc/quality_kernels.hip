// quality_kernels.hip — the quality records of include/av1mi.h (av1mi_quality): per (frame, plane) the exact squared error and the sum
// of the 8x8-window, step-4 SSIM values between the source and the decoded picture; arithmetic in quality.hpp, shared with the host.
//
// k_quality_tiles.  One launch covers the three planes of all stacked frames.  A workgroup of 256 lanes owns a TILE of one plane of
// one frame: 256 bytes x 64 rows (64 x 16 blocks of 4x4 at 8 bits, 32 x 16 at 10), i.e. 16 x 16 CELLS of 16 bytes x 4 rows, one per
// lane: four 16-byte loads from each of the two planes, a wave-instruction reads four runs of 256 contiguous bytes.  A lane turns
// its cell into the sums of its 4 / 2 blocks (s1, s2, ss, s12) in LDS.  The windows a tile owns start at its blocks and reach one
// block to the right and below, so 33 lanes then add the overlap: one block column to the right (4-sample loads), one cell row
// below.  After the barrier every lane evaluates 4 / 2 windows (four LDS blocks added, the formula in double) and the workgroup
// reduces.  The squared error needs no second pass over the samples: sum (a - b)^2 = ss - 2 s12 of the OWNED cells.
//
// Edges.  Nothing beyond the true size W x H of the plane is read: a cell that crosses W (or whose rows cross H) loads sample by
// sample and takes 0 for both planes beyond — 0 - 0 adds nothing to the squared error, and the blocks such a cell fills are partial
// ones, which no window uses (windows run over the whole blocks, floor(W / 4) x floor(H / 4)).  No frame reads another's rows.
//
// Reproducible sums.  No atomics: a workgroup writes its partial pair (squared error, SSIM sum) to its own scratch entry, indexed by
// the TILE (not by where the workgroup ran), and k_quality_sum — one workgroup per (frame, plane) — adds a plane's entries in a fixed
// order: lane l takes entries l, l + 256, ..., then the same shuffle / LDS tree as in the tile kernel.  The order of the double
// additions is a function of the geometry alone, so two runs give the same bits.
//
// Against the guides.  Per 16 / 8 sample pairs a lane issues 2 x 16 bytes of loads, ~6 integer operations per pair and one double
// division per 16 pairs, so the plan is a kernel that streams; whether it reaches the copy rate is a measurement, not a property of
// the plan: the numbers (and what nobody has measured) are in DESIGN.md, section 5.00-ter.  16-byte loads at 4-byte alignment (a chroma
// row of an 8-bit frame is a multiple of 4 bytes, not 16).  13.3 KB LDS in SoA dword arrays with a row pitch of 65.  The window reads
// (ds_read_b32) have the lanes of a half-wave on 32 consecutive dwords of one row: conflict-free.  The block-sum stores
// (ds_write_b32: 32 banks, half-waves) are at o = cy * 65 + cx * NB + k, lanes NB dwords apart and two rows per half-wave: at 10 bits
// (NB = 2) banks 2 cx + cy cover all 32, conflict-free; at 8 bits (NB = 4) lanes cx and cx + 8 meet on a bank, a 2-way conflict on
// 12 stores per lane and tile, left as it is beside 128 bytes of global loads per lane.  Registers and occupancy are whatever the
// compiler reports for the source as it stands (tools/bench_quality.py --resources-only prints the report and records it beside the
// timings; no scratch is a requirement).  Tile ids go through xcd_swizzle so that the tiles sharing an overlap row mostly share an L2.
#include "av1mi_internal.hpp"
#include "quality.hpp"

namespace av1mi {
namespace {

namespace q = av1mi::quality;
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

enum { kCellsX = 16, kCellsY = 16, kTileRows = 4 * kCellsY, kLanes = kCellsX * kCellsY };

// the 16 bytes of row `y` of a cell at sample x (T samples), zero where the cell leaves the true size W x H
template <typename T>
__device__ __forceinline__ void load_row(const T *plane, int stride, int W, int H, int x, int y, uint32_t (&d)[4]) {
  constexpr int N = 16 / (int)sizeof(T);
  if (y >= H || x >= W) { d[0] = d[1] = d[2] = d[3] = 0; return; }
  const T *p = plane + row_off(y, stride) + x;
  if (x + N <= W) {
    const u32x4_a4 v = *(const u32x4_a4 *)p;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  } else {
    d[0] = d[1] = d[2] = d[3] = 0;
    constexpr int PER = 4 / (int)sizeof(T);      // samples per dword
#pragma unroll
    for (int i = 0; i < N; i++)
      if (x + i < W) d[i / PER] |= (uint32_t)p[i] << (8 * (int)sizeof(T) * (i % PER));
  }
}
// sample i of a row's dwords
template <typename T>
__device__ __forceinline__ uint32_t sample(const uint32_t (&d)[4], int i) {
  return sizeof(T) == 1 ? (d[i >> 2] >> (8 * (i & 3))) & 0xFFu : (d[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
}

struct Red { double d[kLanes / 64]; unsigned long long u[kLanes / 64]; };
struct Lds {
  // block sums of the tile + one column / row of overlap, [row][column], SoA; pitch = the widest tile's blocks + 1
  uint32_t s12p[(kCellsY + 1) * 65];      // s1 | s2 << 16
  uint32_t ss[(kCellsY + 1) * 65];
  uint32_t sab[(kCellsY + 1) * 65];
  Red red;
};
// a tile's partial pair in the scratch buffer
struct Part { unsigned long long sse; double ssim_sum; };

// a cell of NB blocks at (sample x, row y): sums into LDS at block (bx, by); returns the cell's squared error
template <typename T, int NB>
__device__ __forceinline__ uint32_t cell_sums(Lds &L, const T *a, const T *b, int stride, int W, int H, int x, int y, int bx, int by) {
  q::Sums s[NB];
#pragma unroll
  for (int k = 0; k < NB; k++) s[k] = q::Sums{ 0, 0, 0, 0 };
  uint32_t ra[4][4], rb[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++) { load_row<T>(a, stride, W, H, x, y + r, ra[r]); load_row<T>(b, stride, W, H, x, y + r, rb[r]); }
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int k = 0; k < NB; k++)
#pragma unroll
      for (int i = 0; i < 4; i++) q::add_sample(s[k], sample<T>(ra[r], 4 * k + i), sample<T>(rb[r], 4 * k + i));
  uint32_t sse = 0;
#pragma unroll
  for (int k = 0; k < NB; k++) {
    const int o = by * 65 + bx + k;
    L.s12p[o] = s[k].s1 | (s[k].s2 << 16); L.ss[o] = s[k].ss; L.sab[o] = s[k].s12;
    sse += q::sums_sse(s[k]);
  }
  return sse;
}
// one block at (sample x, row y), whole (the caller checked x + 4 <= W, y + 4 <= H): 4-sample loads
template <typename T>
__device__ __forceinline__ void block_sums(Lds &L, const T *a, const T *b, int stride, int x, int y, int bx, int by) {
  q::Sums s = { 0, 0, 0, 0 };
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const T *pa = a + row_off(y + r, stride) + x, *pb = b + row_off(y + r, stride) + x;
#pragma unroll
    for (int i = 0; i < 4; i++) q::add_sample(s, pa[i], pb[i]);
  }
  const int o = by * 65 + bx;
  L.s12p[o] = s.s1 | (s.s2 << 16); L.ss[o] = s.ss; L.sab[o] = s.s12;
}

// workgroup sums in a fixed order: xor-shuffle tree inside a wave, then wave 0 .. 3 in turn; the result is valid in lane 0
__device__ __forceinline__ void wg_reduce(Red &R, double &d, unsigned long long &u) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { d += __shfl_xor(d, m, 64); u += __shfl_xor(u, m, 64); }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { R.d[wave] = d; R.u[wave] = u; }
  __syncthreads();
  d = R.d[0]; u = R.u[0];
#pragma unroll
  for (int k = 1; k < kLanes / 64; k++) { d += R.d[k]; u += R.u[k]; }
}

}  // namespace

struct QualityGeom {
  const void *src[3], *dec0[3], *dec1[3];
  const uint8_t *sel;               // [frame * 3 + plane]: 0 reads dec1, anything else dec0; null = dec0
  int W[3], H[3], stride[3], rows[3];      // true size, buffer stride and rows per frame of plane 0 / 1 / 2 (samples)
  int tx[3], ty[3];                 // tiles of a plane
  int tiles_frame, frames, bd;
};

namespace {

template <typename T>
__global__ __launch_bounds__(256) void k_quality_tiles(QualityGeom G, Part *part) {
  constexpr int NB = 4 / (int)sizeof(T);             // blocks per cell
  constexpr int TBX = kCellsX * NB;                  // blocks per tile row
  __shared__ Lds L;
  const unsigned tile = xcd_swizzle(blockIdx.x, gridDim.x);
  const int f = (int)(tile / (unsigned)G.tiles_frame);
  int r = (int)(tile - (unsigned)f * (unsigned)G.tiles_frame);
  const int n0 = G.tx[0] * G.ty[0], n1 = G.tx[1] * G.ty[1];
  const int p = r < n0 ? 0 : r < n0 + n1 ? 1 : 2;
  r -= p == 0 ? 0 : p == 1 ? n0 : n0 + n1;
  const int W = p ? G.W[1] : G.W[0], H = p ? G.H[1] : G.H[0], stride = p ? G.stride[1] : G.stride[0], rows = p ? G.rows[1] : G.rows[0];
  const int ntx = p ? G.tx[1] : G.tx[0];
  const int tyi = r / ntx, txi = r - tyi * ntx;
  const bool first = !G.sel || G.sel[f * 3 + p];
  const size_t frame_off = (size_t)f * row_off(rows, stride);
  const T *a = (const T *)(p == 0 ? G.src[0] : p == 1 ? G.src[1] : G.src[2]) + frame_off;
  const T *b = (const T *)(first ? (p == 0 ? G.dec0[0] : p == 1 ? G.dec0[1] : G.dec0[2]) : (p == 0 ? G.dec1[0] : p == 1 ? G.dec1[1] : G.dec1[2])) + frame_off;
  const int bx0 = txi * TBX, by0 = tyi * kCellsY;    // the tile's first block
  const int nbx = W >> 2, nby = H >> 2;              // whole blocks of the plane

  const int tid = threadIdx.x, cx = tid & (kCellsX - 1), cy = tid >> 4;
  unsigned long long sse = cell_sums<T, NB>(L, a, b, stride, W, H, 4 * (bx0 + cx * NB), 4 * (by0 + cy), cx * NB, cy);
  // the overlap (whole blocks only; a window never uses another): lanes 0 .. 15 the column right of the tile, lanes 64 .. 79 the cell row
  // below it, lane 128 the corner
  if (tid < kCellsY) {
    if (bx0 + TBX < nbx && by0 + tid < nby) block_sums<T>(L, a, b, stride, 4 * (bx0 + TBX), 4 * (by0 + tid), TBX, tid);
  } else if (tid >= 64 && tid < 64 + kCellsX) {
    if (by0 + kCellsY < nby) (void)cell_sums<T, NB>(L, a, b, stride, W, H, 4 * (bx0 + (tid - 64) * NB), 4 * (by0 + kCellsY), (tid - 64) * NB, kCellsY);
  } else if (tid == 128) {
    if (bx0 + TBX < nbx && by0 + kCellsY < nby) block_sums<T>(L, a, b, stride, 4 * (bx0 + TBX), 4 * (by0 + kCellsY), TBX, kCellsY);
  }
  __syncthreads();
  // windows: (x, y) of the tile's blocks with x + 1 < nbx and y + 1 < nby
  const int64_t c1 = q::ssim_c1(G.bd), c2 = q::ssim_c2(G.bd);
  double sum = 0;
#pragma unroll
  for (int k = 0; k < NB; k++) {
    const int wi = tid + k * kLanes, wy = wi / TBX, wx = wi - wy * TBX;
    if (bx0 + wx + 1 < nbx && by0 + wy + 1 < nby) {
      const int o = wy * 65 + wx;
      const uint32_t p0 = L.s12p[o], p1 = L.s12p[o + 1], p2 = L.s12p[o + 65], p3 = L.s12p[o + 66];
      q::Sums w;
      w.s1 = (p0 & 0xFFFFu) + (p1 & 0xFFFFu) + (p2 & 0xFFFFu) + (p3 & 0xFFFFu);
      w.s2 = (p0 >> 16) + (p1 >> 16) + (p2 >> 16) + (p3 >> 16);
      w.ss = L.ss[o] + L.ss[o + 1] + L.ss[o + 65] + L.ss[o + 66];
      w.s12 = L.sab[o] + L.sab[o + 1] + L.sab[o + 65] + L.sab[o + 66];
      sum += q::window_ssim(w, c1, c2);
    }
  }
  wg_reduce(L.red, sum, sse);
  if (tid == 0) part[tile] = Part{ sse, sum };
}

// one workgroup per (frame, plane): its tiles' partial pairs added in a fixed order -> the record
__global__ __launch_bounds__(256) void k_quality_sum(QualityGeom G, const Part *part, av1mi_quality *out) {
  __shared__ Red R;
  const int f = blockIdx.x / 3, p = blockIdx.x - 3 * f;
  const int n0 = G.tx[0] * G.ty[0], n1 = G.tx[1] * G.ty[1];
  const size_t first = (size_t)f * G.tiles_frame + (p == 0 ? 0 : p == 1 ? n0 : n0 + n1);
  const int n = p ? n1 : n0;
  double sum = 0;
  unsigned long long sse = 0;
  for (int i = threadIdx.x; i < n; i += kLanes) {
    sse += part[first + i].sse;
    sum += part[first + i].ssim_sum;
  }
  wg_reduce(R, sum, sse);
  if (threadIdx.x == 0) {
    const int W = p ? G.W[1] : G.W[0], H = p ? G.H[1] : G.H[0];
    av1mi_quality r;
    r.sse = sse; r.ssim_sum = sum; r.samples = (uint32_t)W * (uint32_t)H; r.windows = (uint32_t)((W / 4 - 1) * (H / 4 - 1));
    out[blockIdx.x] = r;
  }
}

QualityGeom geometry(const QualityLaunch &Q) {
  QualityGeom G;
  const int tile_w = 256 / (Q.bd == 8 ? 1 : 2);      // samples: 256 bytes
  for (int p = 0; p < 3; p++) {
    G.src[p] = Q.src[p]; G.dec0[p] = Q.dec0[p]; G.dec1[p] = Q.dec1 ? Q.dec1[p] : nullptr;
    G.W[p] = q::plane_dim(Q.w, p); G.H[p] = q::plane_dim(Q.h, p); G.stride[p] = q::plane_buf(Q.w, p); G.rows[p] = q::plane_buf(Q.h, p);
    G.tx[p] = (G.W[p] + tile_w - 1) / tile_w; G.ty[p] = (G.H[p] + kTileRows - 1) / kTileRows;
  }
  G.sel = Q.dec1 ? Q.sel : nullptr;
  G.tiles_frame = G.tx[0] * G.ty[0] + 2 * G.tx[1] * G.ty[1];
  G.frames = Q.frames; G.bd = Q.bd;
  return G;
}

}  // namespace

size_t quality_scratch_bytes(int bd, int w, int h, int frames) {
  const int tile_w = 256 / (bd == 8 ? 1 : 2);
  size_t tiles = 0;
  for (int p = 0; p < 3; p++)
    tiles += (size_t)((q::plane_dim(w, p) + tile_w - 1) / tile_w) * ((q::plane_dim(h, p) + kTileRows - 1) / kTileRows);
  return tiles * (size_t)frames * sizeof(Part);
}

hipError_t launch_quality(const QualityLaunch &Q, hipStream_t s) {
  const QualityGeom G = geometry(Q);
  const size_t tiles = (size_t)G.tiles_frame * G.frames;
  if (tiles > 0x7FFFFFFFu) return hipErrorInvalidValue;
  if (Q.bd == 8) hipLaunchKernelGGL(k_quality_tiles<uint8_t>, dim3((unsigned)tiles), dim3(kLanes), 0, s, G, (Part *)Q.scratch);
  else hipLaunchKernelGGL(k_quality_tiles<uint16_t>, dim3((unsigned)tiles), dim3(kLanes), 0, s, G, (Part *)Q.scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_quality_sum, dim3((unsigned)G.frames * 3), dim3(kLanes), 0, s, G, (const Part *)Q.scratch, Q.out);
  return hipGetLastError();
}

}  // namespace av1mi
