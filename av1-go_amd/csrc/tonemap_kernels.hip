// tonemap_kernels.hip — tone mapping of the planar source planes in place (include/av1mi.h "tone mapping"; numpy twin: tests/tonemap_ref.py).
//
//   k_tone_map   a lane owns a CELL: 16 bytes (8 samples) of two adjacent luma rows and the 8-byte halves of U and V above them, i.e. four
//                2x2 quads.  dwordx4 / dwordx2 loads and stores declared 4-byte aligned (a width that is a multiple of 4 puts luma rows at 8
//                and chroma rows at 4 bytes); a row's last cell is a half cell (dwordx2 / dword) where the width is not a multiple of 8.
//                A row pair never straddles frames (the height is even), so the batch is one plane of frames * height rows.  The tables
//                (11.8 KB) are copied to LDS once per workgroup, and the workgroups stride over the batch's cells.  Everything a lane reads
//                it alone writes: in place is safe.  The work per quad is ~12 LDS lookups and ~40 integer multiplies (nine of them 64-bit);
//                HBM traffic is 3 bytes in + 3 out per luma sample.
//
// av1mi_tone_map_tables is plain host code: doubles, libm, no device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "av1mi_internal.hpp"

namespace av1mi {
namespace {

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

constexpr int kLin = 0, kGain = 1024, kLo = 2048, kHi = 2048 + AV1MI_TONE_LO, kWords = kHi + AV1MI_TONE_HI + 3;
static_assert(kWords % 4 == 0 && offsetof(av1mi_tone_tables, to_rgb) == kWords * 4, "the kernel copies the tables' first kWords words as dwordx4");
constexpr int kMaxGroups = 2048;      // workgroups of a launch: 8 per CU of 256, each with its copy of the tables

__device__ __forceinline__ uint32_t oetf(const uint32_t *s, uint32_t c) {      // step 6
  if (c < AV1MI_TONE_LO) return s[kLo + c];
  const int k = 31 - __clz((int)c), sh = k - 6, i = (k - 9) * 64 + (int)(c >> sh) - 64;
  const uint32_t f = c & ((1u << sh) - 1u);
  const uint32_t v = s[kHi + i] * ((1u << sh) - f) + s[kHi + i + 1] * f;
  return min((v + (1u << (sh + 5))) >> (sh + 6), 1023u);
}

// one pixel: Y with the quad's u, v -> the output Y; the pixel's Cb / Cr sums are added to *cb, *cr
__device__ __forceinline__ uint32_t pixel(const uint32_t *s, int Y, int u, int v, int *cb, int *cr) {
  constexpr int G[3][3] = AV1MI_TONE_GAMUT, K[3][3] = AV1MI_TONE_TO_YUV;
  const int y = AV1MI_TONE_TO_RGB_Y * (Y - 64) + 8192;
  const int R = min(max((y + AV1MI_TONE_TO_RGB_RV * v) >> 14, 0), 1023);
  const int Gc = min(max((y - AV1MI_TONE_TO_RGB_GV * v - AV1MI_TONE_TO_RGB_GU * u) >> 14, 0), 1023);
  const int B = min(max((y + AV1MI_TONE_TO_RGB_BU * u) >> 14, 0), 1023);
  const int M = max(max(R, Gc), B);
  const int64_t r = s[kLin + R], g = s[kLin + Gc], b = s[kLin + B];
  const uint64_t gain = s[kGain + M];
  int o[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int64_t c = max((G[i][0] * r + G[i][1] * g + G[i][2] * b + 8192) >> 14, (int64_t)0);
    const uint64_t t = ((uint64_t)c * gain + 32768u) >> 16;
    o[i] = (int)oetf(s, (uint32_t)min(t, (uint64_t)25600));
  }
  *cb += K[1][0] * o[0] + K[1][1] * o[1] + K[1][2] * o[2];
  *cr += K[2][0] * o[0] + K[2][1] * o[1] + K[2][2] * o[2];
  return (uint32_t)min(max(64 + ((K[0][0] * o[0] + K[0][1] * o[1] + K[0][2] * o[2] + 8192) >> 14), 0), 1023);
}

// quad q of a cell: its two luma dwords (a row's two samples each), its U and V -> the same, mapped
__device__ __forceinline__ void quad(const uint32_t *s, uint32_t &l0, uint32_t &l1, uint32_t &U, uint32_t &V) {
  const int u = (int)(U & 1023u) - 512, v = (int)(V & 1023u) - 512;
  int cb = 0, cr = 0;
  const uint32_t a = pixel(s, l0 & 1023u, u, v, &cb, &cr), b = pixel(s, (l0 >> 16) & 1023u, u, v, &cb, &cr);
  const uint32_t c = pixel(s, l1 & 1023u, u, v, &cb, &cr), d = pixel(s, (l1 >> 16) & 1023u, u, v, &cb, &cr);
  l0 = a | (b << 16); l1 = c | (d << 16);
  U = (uint32_t)min(max(512 + ((cb + 32768) >> 16), 0), 1023);
  V = (uint32_t)min(max(512 + ((cr + 32768) >> 16), 0), 1023);
}

__global__ __launch_bounds__(256) void k_tone_map(uint16_t *Yp, uint16_t *Up, uint16_t *Vp, const uint32_t *tables, int w, int cells_x, uint32_t cells) {
  __shared__ __attribute__((aligned(16))) uint32_t s[kWords];
  for (int i = threadIdx.x; i < kWords / 4; i += 256) ((uint4 *)s)[i] = ((const uint4 *)tables)[i];
  __syncthreads();
  const int cw = w >> 1;
  for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < cells; c += gridDim.x * 256u) {
    const uint32_t pr = c / (uint32_t)cells_x;
    const int cx = (int)(c - pr * (uint32_t)cells_x);
    const bool whole = cx * 8 + 8 <= w;      // else the row's last four samples: half a cell
    uint16_t *y0 = Yp + (size_t)pr * 2 * w + cx * 8, *y1 = y0 + w, *pu = Up + (size_t)pr * cw + cx * 4, *pv = Vp + (size_t)pr * cw + cx * 4;
    uint32_t l0[4], l1[4], U[4], V[4];
    if (whole) {
      const u32x4_a4 a = *(const u32x4_a4 *)y0, b = *(const u32x4_a4 *)y1;
      const u32x2_a4 cu = *(const u32x2_a4 *)pu, cv = *(const u32x2_a4 *)pv;
#pragma unroll
      for (int q = 0; q < 4; q++) { l0[q] = a[q]; l1[q] = b[q]; U[q] = cu[q >> 1] >> (16 * (q & 1)); V[q] = cv[q >> 1] >> (16 * (q & 1)); }
    } else {
      const u32x2_a4 a = *(const u32x2_a4 *)y0, b = *(const u32x2_a4 *)y1;
      const uint32_t cu = *(const uint32_t *)pu, cv = *(const uint32_t *)pv;
#pragma unroll
      for (int q = 0; q < 2; q++) { l0[q] = a[q]; l1[q] = b[q]; U[q] = cu >> (16 * q); V[q] = cv >> (16 * q); }
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (q < 2 || whole) quad(s, l0[q], l1[q], U[q], V[q]);
    if (whole) {
      u32x4_a4 a, b;
      u32x2_a4 cu, cv;
#pragma unroll
      for (int q = 0; q < 4; q++) { a[q] = l0[q]; b[q] = l1[q]; }
      cu[0] = U[0] | (U[1] << 16); cu[1] = U[2] | (U[3] << 16); cv[0] = V[0] | (V[1] << 16); cv[1] = V[2] | (V[3] << 16);
      *(u32x4_a4 *)y0 = a; *(u32x4_a4 *)y1 = b; *(u32x2_a4 *)pu = cu; *(u32x2_a4 *)pv = cv;
    } else {
      u32x2_a4 a, b;
      a[0] = l0[0]; a[1] = l0[1]; b[0] = l1[0]; b[1] = l1[1];
      *(u32x2_a4 *)y0 = a; *(u32x2_a4 *)y1 = b; *(uint32_t *)pu = U[0] | (U[1] << 16); *(uint32_t *)pv = V[0] | (V[1] << 16);
    }
  }
}

// ---- the curve and the transfer functions, in doubles (tests/tonemap_ref.py has the same lines)
const double kM1 = 2610.0 / 16384, kM2 = 2523.0 / 4096 * 128, kC1 = 3424.0 / 4096, kC2 = 2413.0 / 4096 * 32, kC3 = 2392.0 / 4096 * 32;
double pq_eotf(double e) { const double p = pow(e, 1.0 / kM2); return 10000.0 * pow(std::max(p - kC1, 0.0) / (kC2 - kC3 * p), 1.0 / kM1); }
double pq_inv(double l) { const double y = pow(l / 10000.0, kM1); return pow((kC1 + kC2 * y) / (1.0 + kC3 * y), kM2); }
double eetf(double e, double peak) {      // BT.2390, black level 0
  const double src = pq_inv(peak), e1 = std::min(e / src, 1.0), mx = pq_inv(100.0) / src, ks = 1.5 * mx - 0.5;
  if (e1 < ks) return e1 * src;
  const double t = std::min(std::max((e1 - ks) / (1.0 - ks), 0.0), 1.0), t2 = t * t, t3 = t2 * t;
  return ((2 * t3 - 3 * t2 + 1) * ks + (t3 - 2 * t2 + t) * (1 - ks) + (-2 * t3 + 3 * t2) * mx) * src;
}
double oetf709(double l) { return l < 0.018 ? 4.5 * l : 1.099 * pow(l, 0.45) - 0.099; }

}  // namespace

hipError_t launch_tone_map(int w, int h, int frames, void *const planes[3], const void *tables, hipStream_t s) {
  if (w < 4 || h < 2 || (w & 3) || (h & 1) || frames < 1) return hipErrorInvalidValue;
  const int cells_x = (w + 7) / 8;
  const uint64_t cells = (uint64_t)cells_x * (uint64_t)(h / 2) * (uint64_t)frames;
  if (cells > 0xFFFFFFFFull - (uint64_t)kMaxGroups * 256) return hipErrorInvalidValue;      // (the cell counter is 32 bits and steps past the end once)
  const unsigned groups = (unsigned)std::min<uint64_t>((cells + 255) / 256, kMaxGroups);
  hipLaunchKernelGGL(k_tone_map, dim3(groups), dim3(256), 0, s, (uint16_t *)planes[0], (uint16_t *)planes[1], (uint16_t *)planes[2], (const uint32_t *)tables, w,
                     cells_x, (uint32_t)cells);
  return hipGetLastError();
}

}  // namespace av1mi

extern "C" int av1mi_tone_map_tables(int peak, av1mi_tone_tables *out) {
  using namespace av1mi;
  if (!out || peak < 100 || peak > 10000) return AV1MI_E_INVAL;
  memset(out, 0, sizeof(*out));
  for (int m = 0; m < 1024; m++) {
    const double e = m / 1023.0, l = pq_eotf(e);
    out->lin[m] = (uint32_t)floor(l * 256.0 + 0.5);
    out->gain[m] = (uint32_t)floor((l > 0 ? pq_eotf(eetf(e, peak)) / l : 1.0) * 65536.0 + 0.5);
    auto light = [&](int i) { return std::min<uint64_t>(((uint64_t)out->lin[i] * out->gain[i] + 32768u) >> 16, 25600u); };      // step 5 on the neutral axis
    while (m && light(m) < light(m - 1)) out->gain[m]++;
  }
  for (int c = 0; c < AV1MI_TONE_LO; c++) out->oetf_lo[c] = (uint32_t)floor(oetf709(c / 25600.0) * 1023.0 + 0.5);
  for (int i = 0; i < AV1MI_TONE_HI; i++) {
    const int k = 9 + i / 64, x = (64 + i % 64) << (k - 6);      // (i = 384: k = 15, x = 2^15)
    out->oetf_hi[i] = (uint32_t)floor(oetf709(x / 25600.0) * 1023.0 * 64.0 + 0.5);
  }
  const int32_t to_rgb[5] = { AV1MI_TONE_TO_RGB_Y, AV1MI_TONE_TO_RGB_RV, AV1MI_TONE_TO_RGB_GV, AV1MI_TONE_TO_RGB_GU, AV1MI_TONE_TO_RGB_BU };
  const int32_t gamut[3][3] = AV1MI_TONE_GAMUT, to_yuv[3][3] = AV1MI_TONE_TO_YUV;
  memcpy(out->to_rgb, to_rgb, sizeof(to_rgb)); memcpy(out->gamut, gamut, sizeof(gamut)); memcpy(out->to_yuv, to_yuv, sizeof(to_yuv));
  out->peak = peak;
  return AV1MI_OK;
}
