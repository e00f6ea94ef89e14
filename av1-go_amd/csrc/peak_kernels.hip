// peak_kernels.hip — the light level of a PQ source, measured per frame as the histogram of M = max(R', G', B') (include/av1mi.h "peak
// records"), from which the host plans the tone map's peak (host/peakplan.hpp).  Two gfx950 kernels:
//
//   k_peak_rows   a workgroup owns a STRIP of kStripPairs pairs of luma rows of one frame and walks its cells; a lane owns a CELL as in
//                 k_tone_map: 16 bytes (8 samples) of two adjacent luma rows and the 8-byte halves of U and V above them, four 2x2 quads.
//                 Buffer widths are multiples of 8 and the planes 16-byte aligned, so every luma load is ONE aligned 16-byte unit and every
//                 chroma load one aligned 8-byte unit (chroma rows are whole 8-byte units, not always whole 16-byte ones); a chroma
//                 sample is loaded once per quad.  The one cell of a row that the true width cuts, and the second row of a last pair
//                 that the true height cuts, are loaded sample by sample below the true size: nothing at or beyond it is read.
//                 Steps 1 and 2 of "tone mapping" per pixel, in 32-bit integers, and the pixel counts in the workgroup's 1024-bin LDS
//                 histogram by an integer atomic (the order changes nothing).  The histogram leaves the workgroup as 1024 partials, one
//                 writer each.
//                 Contention: flat content puts every lane of a wave on one LDS counter.  The remedy chosen here is MERGING EQUAL
//                 NEIGHBOURS IN A LANE: a lane walks its 16 pixels quad by quad and keeps (code, count); only a change of code, and the
//                 end of the cell, cost an atomic.  A flat cell is one atomic of 16 instead of sixteen of 1.  The alternative, one
//                 sub-histogram per wave (16 KB of LDS, the lanes of ONE wave still on one counter), has not been measured by anybody.
//   k_peak_sum    one workgroup per frame, lane i owns bins 4 i .. 4 i + 3: the strips' partials added in strip order (fixed by
//                 geometry); the record is 4-byte aligned, so it is written in dwords.
// Arithmetic: include/av1mi.h; restated in numpy by tests/peak_ref.py.  Reference tree: nothing (its encoder child never tone-maps by content).
#include "av1mi_internal.hpp"

namespace av1mi {

namespace {
constexpr int kBins = 1024;          // of a record's histogram: four per lane of a workgroup
constexpr int kStripPairs = 8;       // pairs of luma rows per workgroup: 16 rows

// (code, count) of the lane's run of equal neighbours; a change of code flushes the run into the histogram
struct Run { int code; uint32_t n; };
__device__ __forceinline__ void count(uint32_t *hist, Run &r, int M) {
  if (M == r.code) { r.n++; return; }
  if (r.n) atomicAdd(&hist[r.code], r.n);
  r.code = M; r.n = 1;
}

// steps 1 and 2 of "tone mapping": with Y, U, V <= 1023 every product and sum below fits 32 bits (|y| < 2^25, |BU * u| < 2^25)
__device__ __forceinline__ int max_rgb(int Y, int u, int v) {
  const int y = AV1MI_TONE_TO_RGB_Y * (Y - 64) + 8192;
  const int R = min(max((y + AV1MI_TONE_TO_RGB_RV * v) >> 14, 0), 1023);
  const int G = min(max((y - AV1MI_TONE_TO_RGB_GV * v - AV1MI_TONE_TO_RGB_GU * u) >> 14, 0), 1023);
  const int B = min(max((y + AV1MI_TONE_TO_RGB_BU * u) >> 14, 0), 1023);
  return max(max(R, G), B);
}

// grid: strips x frames.  w8 x h8: the buffers' luma size; tw x th: the true size; part: [frame][strip][bin]
__global__ __launch_bounds__(256) void k_peak_rows(const uint16_t *Yp, const uint16_t *Up, const uint16_t *Vp, uint32_t *part, int w8, int h8, int tw, int th) {
  __shared__ __attribute__((aligned(16))) uint32_t s_hist[kBins];
  const unsigned tid = threadIdx.x, strip = blockIdx.x, frame = blockIdx.y;
  ((uint4 *)s_hist)[tid] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const int cw8 = w8 >> 1, cells_x = (tw + 7) >> 3, pairs = (th + 1) >> 1;
  const int pr0 = (int)strip * kStripPairs, npr = min(kStripPairs, pairs - pr0);
  const uint16_t *fy = Yp + (size_t)frame * w8 * h8, *fu = Up + (size_t)frame * cw8 * (h8 >> 1), *fv = Vp + (size_t)frame * cw8 * (h8 >> 1);
  Run run = { 0, 0 };
  for (int c = (int)tid; c < cells_x * npr; c += 256) {
    const int pr = pr0 + c / cells_x, cx = c % cells_x;
    const int nx = min(8, tw - cx * 8), ny = min(2, th - 2 * pr);      // the cell's samples and rows below the true size (>= 1 each)
    const uint16_t *y0 = fy + (size_t)(2 * pr) * w8 + cx * 8, *y1 = y0 + w8, *pu = fu + (size_t)pr * cw8 + cx * 4, *pv = fv + (size_t)pr * cw8 + cx * 4;
    uint32_t l0[4], l1[4] = { 0, 0, 0, 0 }, U[4], V[4];      // per quad: a row's two samples in a dword; the quad's U and V
    if (nx == 8) {
      const uint4 a = *(const uint4 *)y0;
      const uint2 cu = *(const uint2 *)pu, cv = *(const uint2 *)pv;
      l0[0] = a.x; l0[1] = a.y; l0[2] = a.z; l0[3] = a.w;
      if (ny == 2) { const uint4 b = *(const uint4 *)y1; l1[0] = b.x; l1[1] = b.y; l1[2] = b.z; l1[3] = b.w; }
      U[0] = cu.x & 0xffffu; U[1] = cu.x >> 16; U[2] = cu.y & 0xffffu; U[3] = cu.y >> 16;
      V[0] = cv.x & 0xffffu; V[1] = cv.x >> 16; V[2] = cv.y & 0xffffu; V[3] = cv.y >> 16;
    } else {      // the row's last cell, cut by the true width: its samples one by one
#pragma unroll
      for (int q = 0; q < 4; q++) {
        l0[q] = 0; U[q] = V[q] = 0;
        if (2 * q < nx) { l0[q] = y0[2 * q]; U[q] = pu[q]; V[q] = pv[q]; }
        if (2 * q + 1 < nx) l0[q] |= (uint32_t)y0[2 * q + 1] << 16;
        if (ny == 2) {
          if (2 * q < nx) l1[q] = y1[2 * q];
          if (2 * q + 1 < nx) l1[q] |= (uint32_t)y1[2 * q + 1] << 16;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (2 * q >= nx) continue;
      const int u = (int)min(U[q], 1023u) - 512, v = (int)min(V[q], 1023u) - 512;
      const bool right = 2 * q + 1 < nx;
      count(s_hist, run, max_rgb((int)min(l0[q] & 0xffffu, 1023u), u, v));
      if (right) count(s_hist, run, max_rgb((int)min(l0[q] >> 16, 1023u), u, v));
      if (ny == 2) {
        count(s_hist, run, max_rgb((int)min(l1[q] & 0xffffu, 1023u), u, v));
        if (right) count(s_hist, run, max_rgb((int)min(l1[q] >> 16, 1023u), u, v));
      }
    }
  }
  if (run.n) atomicAdd(&s_hist[run.code], run.n);
  __syncthreads();
  ((uint4 *)(part + ((size_t)frame * gridDim.x + strip) * kBins))[tid] = ((const uint4 *)s_hist)[tid];
}

// one workgroup per frame, lane i = bins 4 i .. 4 i + 3
__global__ __launch_bounds__(256) void k_peak_sum(const uint32_t *part, av1mi_peak_record *out, unsigned strips, uint32_t pixels) {
  const unsigned f = blockIdx.x, tid = threadIdx.x;
  const uint4 *p = (const uint4 *)(part + (size_t)f * strips * kBins) + tid;
  uint4 s = make_uint4(0, 0, 0, 0);
  for (unsigned t = 0; t < strips; t++) { const uint4 v = p[(size_t)t * (kBins / 4)]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
  uint32_t *h = out[f].hist + 4 * tid;      // (records are 4-byte aligned: dword stores)
  h[0] = s.x; h[1] = s.y; h[2] = s.z; h[3] = s.w;
  if (tid == 0) out[f].pixels = pixels;
}

}  // namespace

PeakLayout peak_layout(int th, int frames) {
  PeakLayout L;
  L.strips = ((th + 1) / 2 + kStripPairs - 1) / kStripPairs;
  L.bytes = (size_t)L.strips * (size_t)frames * kBins * 4;
  return L;
}

hipError_t launch_peak_analyse(const PeakAnalyseLaunch &A, hipStream_t s) {
  if (A.frames <= 0) return hipSuccess;
  if (A.frames > 65535 || A.tw < 1 || A.th < 1 || A.tw > A.w8 || A.th > A.h8 || (A.w8 & 7) || (A.h8 & 7)) return hipErrorInvalidValue;
  const PeakLayout L = peak_layout(A.th, A.frames);
  uint32_t *part = (uint32_t *)A.scratch;
  hipLaunchKernelGGL(k_peak_rows, dim3((unsigned)L.strips, (unsigned)A.frames), dim3(256), 0, s, (const uint16_t *)A.y, (const uint16_t *)A.u, (const uint16_t *)A.v, part, A.w8,
                     A.h8, A.tw, A.th);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_peak_sum, dim3((unsigned)A.frames), dim3(256), 0, s, part, A.out, (unsigned)L.strips, (uint32_t)A.tw * (uint32_t)A.th);
  return hipGetLastError();
}

}  // namespace av1mi
