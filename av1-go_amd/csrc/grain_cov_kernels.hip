// grain_cov_kernels.hip — the grain covariance behind av1mi_gop_config.grain_cov (include/av1mi.h "grain covariance"): k_grain_cov runs
// AFTER either denoising gather, reads what it was fed (the C entries of its table) and what it wrote, and adds up the products of the
// residual r = C - out with its neighbours at the 52 offsets dy = 0 .. 3, dx = -6 .. 6; k_grain_cov_sum adds the workgroups' partials.
//
//   work      the gathers' items, from gather_cells.hpp (band_geometry with the cell rule, gather_plane, gather_band, load_cell): an item
//             is (segment, plane, band of kBand rows, group of 64 cells of 16 bytes), a wave owns an item and walks down its band, a
//             workgroup holds four consecutive items of one (segment, plane).  The same geometry as k_denoise_gather's, so the same
//             argument check; after k_denoise_mc_gather it is merely another tiling of the same planes.
//   residual  r is 0 beyond the true size: with that ONE rule the definition's "both samples inside w x h" needs no case of its own, a
//             product with a sample outside is 0.  Per row a lane computes r of its cell as packed 16-bit halves (|r| <= 1023) and
//             writes it to its wave's ring of FOUR rows in LDS (rows y .. y + 3 of the anchor row y); lanes 0 and 63 also write the
//             neighbouring cell on either side (another wave's, or zeros at the plane's edge): a halo of a whole cell where six samples
//             would do, so that it is load_cell's unit.  A row enters the ring once per band; a band re-reads the three rows below it.
//             The ring is a wave's own: AV1MI_GROUP_SYNC orders its writes and reads, no workgroup barrier stands in the loop
//             (the four waves' bands may differ in length).
//   products  per anchor row and dy a lane reads the NS + 12 halves around its cell as dwords, forms the dwords that start at odd
//             samples with v_alignbit_b32, and adds TWO products per instruction: v_dot2_i32_i16 (__builtin_amdgcn_sdot2) of an anchor
//             pair (x, x + 1) with the pair (x + dx, x + dx + 1).  The ISA for gfx950 shows 13 x NP v_dot2_i32_i16 per dy (416 in the
//             8-bit kernel, NP = 8 pairs; 208 at 10 bits), multiplies only in the rows' addresses, the 52 accumulators in VGPRs, no
//             scratch; 247 VGPRs, so two waves per SIMD: the windows of all four dy are live at once after unrolling.
//   width     a lane's accumulator takes kBand rows x NS samples = at most 16 x 16 = 256 products of at most 1023^2 < 2^20: below 2^28,
//             it stays in 32 bits.  Everything past the lane is 64 bits: the wave's sum by six exchanges of 64-bit values, the
//             workgroup's in LDS (integer atomics), the partial in scratch and k_grain_cov_sum.  All integers, so every order of
//             addition gives the same bytes.
//   ends      none of its own: an end of a run has out = C, a flat slot C = null (zeros) and out = zeros; r = 0 everywhere.
// Arithmetic: include/av1mi.h; restated in numpy by tests/grain_cov_ref.py.  Reference tree: nothing (it has no denoiser).
#include "gather_cells.hpp"

namespace av1mi {

namespace {
constexpr int kCovDy = 4, kCovDx = 13, kCovSums = kCovDy * kCovDx;      // av1mi_grain_cov_record: sum[dy][dx + 6]

struct CovGeom : BandGeom {
  long long *partials;         // per workgroup kCovSums sums, [blockIdx.x]
};

typedef short ss2 __attribute__((ext_vector_type(2)));

// r = C - out of the cell cx of row y as packed halves (sample 2 q in the low half of dword q), 0 beyond the true width and for a cell or
// a row that does not exist.  C null: zeros were fed
template <typename Pix, int NS>
__device__ __forceinline__ void residual_cell(const GatherPlane &W, const char *C, int y, uint32_t cx, bool row_ok, uint32_t r[NS / 2]) {
  constexpr int NP = NS / 2;
  const bool active = row_ok && cx < W.cells;
  const bool whole = !(W.rb & 15u);
  const size_t ro = (size_t)(row_ok ? y : 0) * W.rb;
  uint32_t c[4] = { 0, 0, 0, 0 }, o[4];
  if (C) load_cell(C + ro, cx * 16u, W.rb, whole, active, c);
  load_cell(W.dst + ro, cx * 16u, W.rb, whole, active, o);
  const int lastj = W.w - 1 - (int)cx * NS;      // the sample OF THE CELL that is the last true column
#pragma unroll
  for (int q = 0; q < NP; q++) {
    uint32_t a, b;
    if constexpr (sizeof(Pix) == 1) {
      const uint32_t cd = c[q >> 1] >> (16 * (q & 1)), od = o[q >> 1] >> (16 * (q & 1));
      a = (cd & 0xffu) | ((cd & 0xff00u) << 8);
      b = (od & 0xffu) | ((od & 0xff00u) << 8);
    } else {
      a = c[q]; b = o[q];
    }
    uint32_t d = __builtin_bit_cast(uint32_t, (ss2)(__builtin_bit_cast(ss2, a) - __builtin_bit_cast(ss2, b)));
    if (2 * q > lastj) d = 0;
    else if (2 * q + 1 > lastj) d &= 0xffffu;
    r[q] = active ? d : 0u;
  }
}
}  // namespace

// grid: per_seg x segments; 4 waves = 4 consecutive items of one (segment, plane)
template <typename Pix>
__global__ __launch_bounds__(256) void k_grain_cov(CovGeom G, const void *const *table) {
  constexpr int NS = 16 / (int)sizeof(Pix);      // samples per cell
  constexpr int NP = NS / 2;                     // dwords of packed halves per cell
  constexpr int ROW = 66 * NP;                   // dwords of a ring row: a halo cell, the wave's 64 cells, a halo cell
  constexpr int WIN = NP + 6;                    // dwords of a lane's window: six samples, its cell, six samples
  __shared__ uint32_t s_ring[4][4][ROW];
  __shared__ unsigned long long s_sum[kCovSums];
  const GatherPlane W = gather_plane(G, table);
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (threadIdx.x < kCovSums) s_sum[threadIdx.x] = 0;
  __syncthreads();
  const unsigned item = W.wg * 4u + wave;
  if (item < W.items) {                          // (uniform in the wave)
    const GatherBand B = gather_band<NS>(W, item, lane);
    const int h = W.h, y1 = min(B.r1, h);        // anchor rows [r0, y1)
    const char *C = W.C;
    uint32_t (*ring)[ROW] = s_ring[wave];
    // row yy (< h) enters the ring: every lane its cell, lanes 0 and 63 the cells beside the wave's
    auto put_row = [&](int yy) {
      uint32_t *row = ring[yy & 3];
      uint32_t r[NP];
      residual_cell<Pix, NS>(W, C, yy, B.cx, true, r);
#pragma unroll
      for (int q = 0; q < NP; q++) row[NP * (1 + (int)lane) + q] = r[q];
      if (lane == 0 || lane == 63) {
        const bool left = lane == 0;
        residual_cell<Pix, NS>(W, C, yy, left ? B.cx - 1u : B.cx + 1u, left ? B.cx > 0 : true, r);      // (cx + 1 >= cells: no such cell, zeros)
#pragma unroll
        for (int q = 0; q < NP; q++) row[(left ? 0 : 65 * NP) + q] = r[q];
      }
    };
    int acc[kCovDy][kCovDx];
#pragma unroll
    for (int dy = 0; dy < kCovDy; dy++)
#pragma unroll
      for (int dx = 0; dx < kCovDx; dx++) acc[dy][dx] = 0;
    if (B.r0 < y1) {
      for (int yy = B.r0; yy < min(B.r0 + 3, h); yy++) put_row(yy);
#pragma unroll 1
      for (int y = B.r0; y < y1; y++) {
        if (y + 3 < h) put_row(y + 3);           // (into the slot of row y - 1, whose reads are behind the fence below)
        AV1MI_GROUP_SYNC();
        uint32_t own[NP];
#pragma unroll
        for (int q = 0; q < NP; q++) own[q] = ring[y & 3][NP * (1 + (int)lane) + q];
#pragma unroll
        for (int dy = 0; dy < kCovDy; dy++) {
          if (y + dy < h) {                      // (uniform; a row beyond the true height holds no sample)
            const uint32_t *win = &ring[(y + dy) & 3][NP * (1 + (int)lane) - 3];      // the dword of sample x0 - 6
            uint32_t ev[WIN], od[WIN - 1];
#pragma unroll
            for (int k = 0; k < WIN; k++) ev[k] = win[k];
#pragma unroll
            for (int k = 0; k < WIN - 1; k++) od[k] = __builtin_amdgcn_alignbit(ev[k + 1], ev[k], 16);      // the pair that starts one sample later
#pragma unroll
            for (int q = 0; q < NP; q++) {
              const ss2 a = __builtin_bit_cast(ss2, own[q]);
#pragma unroll
              for (int d = 0; d < kCovDx; d++) {             // dx = d - 6: the pair at window sample 2 q + d
                const uint32_t b = (d & 1) ? od[q + (d >> 1)] : ev[q + (d >> 1)];
                acc[dy][d] = __builtin_amdgcn_sdot2(a, __builtin_bit_cast(ss2, b), acc[dy][d], false);
              }
            }
          }
        }
        AV1MI_GROUP_SYNC();
      }
    }
    // the wave's sums, 64 bits from here on: lane e keeps sum e
    long long mine = 0;
#pragma unroll
    for (int dy = 0; dy < kCovDy; dy++)
#pragma unroll
      for (int dx = 0; dx < kCovDx; dx++) {
        long long v = acc[dy][dx];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        if ((int)lane == dy * kCovDx + dx) mine = v;
      }
    if (lane < (unsigned)kCovSums) atomicAdd(&s_sum[lane], (unsigned long long)mine);
  }
  __syncthreads();
  if (threadIdx.x < kCovSums) G.partials[(size_t)blockIdx.x * kCovSums + threadIdx.x] = (long long)s_sum[threadIdx.x];
}

// grid: segments x 3; the partials of (segment, plane) are those of its workgroups, [first, first + n)
__global__ __launch_bounds__(256) void k_grain_cov_sum(CovGeom G, av1mi_grain_cov_record *out) {
  __shared__ long long s_part[4][64];
  const unsigned seg = blockIdx.x / 3, p = blockIdx.x - seg * 3;
  const unsigned first = seg * G.per_seg + (p > 0 ? G.wgs[0] : 0) + (p > 1 ? G.wgs[1] : 0), n = G.wgs[p];
  const unsigned e = threadIdx.x & 63u, part = threadIdx.x >> 6;
  long long sum = 0;
  if (e < (unsigned)kCovSums)
    for (unsigned i = part; i < n; i += 4) sum += G.partials[(size_t)(first + i) * kCovSums + e];
  s_part[part][e] = sum;
  __syncthreads();
  if (threadIdx.x < (unsigned)kCovSums) (&out[blockIdx.x].sum[0][0])[threadIdx.x] = s_part[0][e] + s_part[1][e] + s_part[2][e] + s_part[3][e];
}

size_t grain_cov_scratch_bytes(const GatherPlanes &L) {
  CovGeom G;
  if ((L.bd != 8 && L.bd != 10) || band_geometry(L, true, G) != hipSuccess || L.segments <= 0) return 0;
  return (size_t)G.per_seg * L.segments * kCovSums * sizeof(long long);
}

hipError_t launch_grain_cov(const GrainCovLaunch &L, hipStream_t s) {
  static_assert(sizeof(av1mi_grain_cov_record) == kCovSums * sizeof(long long), "av1mi_grain_cov_record is 4 x 13 sums");
  CovGeom G;
  if (L.bd != 8 && L.bd != 10) return hipErrorInvalidValue;
  if (hipError_t e = band_geometry(L, true, G)) return e;
  if (L.segments <= 0) return hipSuccess;
  if (!L.cov || !L.table) return hipErrorInvalidValue;
  if (!G.per_seg) return hipMemsetAsync(L.cov, 0, (size_t)L.segments * 3 * sizeof(av1mi_grain_cov_record), s);      // no plane at all
  if (!L.scratch) return hipErrorInvalidValue;
  G.partials = (long long *)L.scratch;
  const dim3 grid(G.per_seg * (unsigned)L.segments);
  if (L.bd == 8) hipLaunchKernelGGL(k_grain_cov<uint8_t>, grid, dim3(256), 0, s, G, L.table);
  else hipLaunchKernelGGL(k_grain_cov<uint16_t>, grid, dim3(256), 0, s, G, L.table);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(k_grain_cov_sum, dim3(3u * (unsigned)L.segments), dim3(256), 0, s, G, L.cov);
  return hipGetLastError();
}

}  // namespace av1mi
