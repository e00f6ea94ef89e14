// quality.hpp — the arithmetic of the quality records (include/av1mi.h "quality"): squared error and the 8x8-window, step-4 SSIM of
// the x264 / FFmpeg `ssim` filter, per plane.  ONE statement of it for the device kernel (quality_kernels.hip, hipcc) and the host
// twin + the command line's report (host/, g++), the way av1_ops.hpp is shared: what the GPU counts is what the CPU tests pinned.
//
// Everything up to the last step is integer arithmetic, so it cannot differ between compilers; the last step converts four integers
// below 2^35 to double (exact), forms ONE product above, ONE below and ONE IEEE division: no addition follows a product, so there is
// nothing to contract into an FMA and a window's value is the same bits on every IEEE machine.  Only the ORDER in which windows are
// added differs between implementations (and is fixed inside each of them).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/av1mi.h"

#if defined(__HIPCC__)
#define AV1MI_Q_HD __host__ __device__ __forceinline__
#else
#define AV1MI_Q_HD inline
#endif

namespace av1mi {
namespace quality {

// c1 = floor(0.01^2 L^2 64 + 0.5), c2 = floor(0.03^2 L^2 64 63 + 0.5), L = 2^bd - 1, in integers: floor(n / 10000 + 1 / 2) =
// (n + 5000) / 10000.  8 bit: 416, 235963.  10 bit: 6698, 3797644.
AV1MI_Q_HD int64_t ssim_c1(int bd) { const int64_t L = (1 << bd) - 1; return (L * L * 64 + 5000) / 10000; }
AV1MI_Q_HD int64_t ssim_c2(int bd) { const int64_t L = (1 << bd) - 1; return (9 * L * L * 64 * 63 + 5000) / 10000; }

// the sums of one 4x4 block; of a window = four blocks added.  10 bit: s1, s2 <= 64 * 1023 < 2^16, ss <= 64 * 2 * 1023^2 < 2^28.
struct Sums { uint32_t s1, s2, ss, s12; };      // sum a, sum b, sum (a^2 + b^2), sum a b
AV1MI_Q_HD void add_sample(Sums &s, uint32_t a, uint32_t b) { s.s1 += a; s.s2 += b; s.ss += a * a + b * b; s.s12 += a * b; }
// sum (a - b)^2 of the samples behind the sums
AV1MI_Q_HD uint32_t sums_sse(const Sums &s) { return s.ss - 2 * s.s12; }

AV1MI_Q_HD double window_ssim(const Sums &w, int64_t c1, int64_t c2) {
  const int64_t s1 = w.s1, s2 = w.s2;      // s1^2 passes 2^32 at 10 bits
  const int64_t vars = 64 * (int64_t)w.ss - s1 * s1 - s2 * s2, covar = 64 * (int64_t)w.s12 - s1 * s2;
  const double a = (double)(2 * s1 * s2 + c1), b = (double)(2 * covar + c2), c = (double)(s1 * s1 + s2 * s2 + c1), d = (double)(vars + c2);
  return (a * b) / (c * d);
}

// the true size of plane p (0 luma, 1 / 2 chroma) of a 4:2:0 frame of true luma size w x h, and of its buffer (that size rounded up to 8)
AV1MI_Q_HD int plane_dim(int n, int p) { return p ? (n + 1) / 2 : n; }
AV1MI_Q_HD int plane_buf(int n, int p) { const int c = (n + 7) & ~7; return p ? c / 2 : c; }

// ---- derived figures (host) ----------------------------------------------------------------------------------------------------
inline double psnr_from_sse(double sse, double samples, int bd) {
  const double L = (double)((1 << bd) - 1);
  return sse == 0 ? INFINITY : 10.0 * log10(L * L * samples / sse);
}

// ---- the CPU twin of the kernel: plain loops over one plane ----------------------------------------------------------------------
template <typename T>
void plane_host(const T *a, const T *b, int stride, int W, int H, int bd, av1mi_quality *out) {
  const int nbx = W / 4, nby = H / 4;
  uint64_t sse = 0;
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      const int64_t d = (int64_t)a[(size_t)y * stride + x] - (int64_t)b[(size_t)y * stride + x];
      sse += (uint64_t)(d * d);
    }
  const int64_t c1 = ssim_c1(bd), c2 = ssim_c2(bd);
  // two rows of block sums at a time
  Sums *rows = new Sums[(size_t)2 * (nbx > 0 ? nbx : 1)];
  auto block_row = [&](int by, Sums *dst) {
    for (int bx = 0; bx < nbx; bx++) {
      Sums s = { 0, 0, 0, 0 };
      for (int y = 0; y < 4; y++)
        for (int x = 0; x < 4; x++) add_sample(s, a[(size_t)(4 * by + y) * stride + 4 * bx + x], b[(size_t)(4 * by + y) * stride + 4 * bx + x]);
      dst[bx] = s;
    }
  };
  double sum = 0;
  uint32_t windows = 0;
  if (nby > 0) block_row(0, rows);
  for (int by = 0; by + 1 < nby; by++) {
    Sums *r0 = rows + (size_t)(by & 1) * nbx, *r1 = rows + (size_t)((by + 1) & 1) * nbx;
    block_row(by + 1, r1);
    for (int bx = 0; bx + 1 < nbx; bx++) {
      const Sums w = { r0[bx].s1 + r0[bx + 1].s1 + r1[bx].s1 + r1[bx + 1].s1, r0[bx].s2 + r0[bx + 1].s2 + r1[bx].s2 + r1[bx + 1].s2,
                       r0[bx].ss + r0[bx + 1].ss + r1[bx].ss + r1[bx + 1].ss, r0[bx].s12 + r0[bx + 1].s12 + r1[bx].s12 + r1[bx + 1].s12 };
      sum += window_ssim(w, c1, c2);
      windows++;
    }
  }
  delete[] rows;
  out->sse = sse; out->ssim_sum = sum; out->samples = (uint32_t)W * (uint32_t)H; out->windows = windows;
}

// the argument rules of av1mi_quality_planes / av1mi_quality_planes_host: null = fine
inline const char *geometry_error(int bd, int w, int h, int frames) {
  if (bd != 8 && bd != 10) return "bit depth must be 8 or 10";
  if (w < 16 || h < 16) return "a true luma size under 16x16 has a plane without a window";
  if (w > 16384 || h > 16384) return "frame larger than 16384x16384";
  if (frames < 1 || frames > 65536) return "frames must be 1 .. 65536";
  return nullptr;
}

// `frames` stacked frames of three planes; sel / dec1 may be null (see av1mi_quality_planes)
inline int planes_host(int bd, int w, int h, int frames, const void *const src[3], const void *const dec0[3], const void *const dec1[3], const uint8_t *sel,
                       av1mi_quality *out) {
  if (geometry_error(bd, w, h, frames) || !src || !dec0 || !out || (sel && !dec1)) return AV1MI_E_INVAL;
  for (int p = 0; p < 3; p++)
    if (!src[p] || !dec0[p] || (sel && !dec1[p])) return AV1MI_E_INVAL;
  for (int f = 0; f < frames; f++)
    for (int p = 0; p < 3; p++) {
      const int W = plane_dim(w, p), H = plane_dim(h, p), stride = plane_buf(w, p);
      const size_t off = (size_t)f * plane_buf(h, p) * stride;
      const void *dec = sel && !sel[f * 3 + p] ? dec1[p] : dec0[p];
      if (bd == 8) plane_host((const uint8_t *)src[p] + off, (const uint8_t *)dec + off, stride, W, H, bd, &out[f * 3 + p]);
      else plane_host((const uint16_t *)src[p] + off, (const uint16_t *)dec + off, stride, W, H, bd, &out[f * 3 + p]);
    }
  return AV1MI_OK;
}

// ---- the report of the command line (INTEGRATION.md "stats file"): the eight figures of one frame or of the summary ---------------
struct Figures { double psnr[4], ssim[4]; };      // Y, U, V, all
// one frame from its three records
inline Figures frame_figures(const av1mi_quality q[3], int bd) {
  Figures f;
  double sse = 0, n = 0;
  for (int p = 0; p < 3; p++) {
    f.psnr[p] = psnr_from_sse((double)q[p].sse, (double)q[p].samples, bd);
    f.ssim[p] = q[p].ssim_sum / (double)q[p].windows;
    sse += (double)q[p].sse; n += (double)q[p].samples;
  }
  f.psnr[3] = psnr_from_sse(sse, n, bd);
  f.ssim[3] = (4 * f.ssim[0] + f.ssim[1] + f.ssim[2]) / 6;
  return f;
}
// the summary over frames: PSNR from the summed squared error, SSIM the mean of the frame values
struct Summary {
  uint64_t sse[3] = { 0, 0, 0 }, samples[3] = { 0, 0, 0 };
  double ssim[4] = { 0, 0, 0, 0 };
  long frames = 0;
  void add(const av1mi_quality q[3], int bd) {
    const Figures f = frame_figures(q, bd);
    for (int p = 0; p < 3; p++) { sse[p] += q[p].sse; samples[p] += q[p].samples; }
    for (int k = 0; k < 4; k++) ssim[k] += f.ssim[k];
    frames++;
  }
  Figures figures(int bd) const {
    Figures f;
    for (int p = 0; p < 3; p++) f.psnr[p] = psnr_from_sse((double)sse[p], (double)samples[p], bd);
    f.psnr[3] = psnr_from_sse((double)sse[0] + (double)sse[1] + (double)sse[2], (double)samples[0] + (double)samples[1] + (double)samples[2], bd);
    for (int k = 0; k < 4; k++) f.ssim[k] = frames ? ssim[k] / (double)frames : 0;
    return f;
  }
};
// " psnr_y:… psnr_u:… psnr_v:… psnr_all:… ssim_y:… ssim_u:… ssim_v:… ssim_all:…" (six decimals, inf where the squared error is 0) into buf
inline int format_figures(const Figures &f, char *buf, size_t cap) {
  static const char *const names[4] = { "y", "u", "v", "all" };
  size_t n = 0;
  for (int k = 0; k < 8 && n < cap; k++) {
    const double v = k < 4 ? f.psnr[k] : f.ssim[k - 4];
    int m;
    if (isinf(v)) m = snprintf(buf + n, cap - n, " %s_%s:inf", k < 4 ? "psnr" : "ssim", names[k & 3]);
    else m = snprintf(buf + n, cap - n, " %s_%s:%.6f", k < 4 ? "psnr" : "ssim", names[k & 3], v);
    if (m < 0) break;
    n += (size_t)m;
  }
  return (int)n;
}

}  // namespace quality
}  // namespace av1mi

// ---- exported by libav1mi_host.so (host/capi_host.cpp; no GPU) --------------------------------------------------------------------
extern "C" {
// av1mi_quality_planes (include/av1mi.h) on HOST pointers: the same records from the same arithmetic, in plain loops
int av1mi_quality_planes_host(int bit_depth, int width, int height, int frames, const void *const src[3], const void *const dec0[3], const void *const dec1[3],
                              const uint8_t *select, av1mi_quality *out);
// 10 log10(L^2 samples / sse), L = 2^bit_depth - 1; inf when sse == 0
double av1mi_quality_psnr(const av1mi_quality *q, int bit_depth);
// ssim_sum / windows
double av1mi_quality_ssim(const av1mi_quality *q);
}
