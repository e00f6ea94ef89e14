// scale_kernels.hip — the resampler of the input stage (include/av1mi.h "scaling"): source frames of one size -> the planar planes
// of the coded size, Lanczos-3 in 14-bit integer coefficients, horizontally then vertically, bit exact by definition.  Host part:
// av1mi_scale_filter (the coefficient table, no GPU needed) and the plan that holds the tables of one geometry on the device.
//
// Kernel.  One launch covers the three planes of all stacked frames.  A workgroup owns a tile of tile_w x tile_h OUTPUT samples of one
// plane of one frame (frames never mix: rows are clamped inside the frame), in three phases with a barrier between them:
//   stage       the source window the tile needs -> LDS as int16, 8 samples per lane and step: one unaligned vector load inside the
//               plane (the window-as-dwords idiom of mc_kernels.hip), sample by sample with clamped coordinates where the window sticks
//               out (edge replication at the TRUE size: nothing beyond it is ever read);
//   horizontal  lane = output column (its taps in registers for all rows), rows strided over the waves: T / 2 + 1 aligned LDS dwords,
//               a 16-bit funnel shift where the window starts on an odd sample, T / 2 v_dot2_i32_i16 -> int16 intermediate in LDS
//               (rows padded by 16 bytes);
//   vertical    lane = 16 bytes of one output row: two intermediate rows per step as ds_read_b128, interleaved into (row, row + 1)
//               pairs with v_perm_b32, v_dot2_i32_i16 against the row's packed taps, clamp, one 16-byte store.
// The tables (first tap + packed coefficient pairs per output column / row, per plane) live in one device allocation together with the
// per-plane geometry; everything a workgroup derives from them is wave-uniform.  Entries for the padding of a coded size that is not
// the target (coded = target rounded up to 8) repeat the last true column / row, so the padding is filled by the same code.
// Algorithmic bytes: b * (S_src + S_dst); arithmetic: T_h * (rows of the window) + T_v multiply-adds per output sample.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "av1mi_internal.hpp"

namespace av1mi {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

struct ScalePlaneDesc {      // 16 ints per plane at the head of the table
  int src_w, src_h;          // true size of the source plane
  int src_stride, src_rows;  // its buffer: samples per row, rows per frame
  int dst_w, dst_h;          // coded size of the destination plane (= its stride and rows per frame)
  int taps_h, taps_v;
  int tiles_x, tiles_y;
  int origin, reserved;      // a crop window: where it starts in the source plane (y * src_stride + x samples; src_w x src_h is then the window)
  int first_h, coef_h, first_v, coef_v;      // dword offsets into the table
};
static_assert(sizeof(ScalePlaneDesc) == 64, "table layout");

struct ScaleLaunch {
  const void *src[3]; void *dst[3];
  const uint32_t *tab;
  int first_wg1, first_wg2;      // the first workgroup of the U and of the V plane (luma starts at 0)
  int tile_w_log2, tile_h, win_stride, win_rows, max_val;
};

template <typename Pix>
__device__ __forceinline__ void widen8(const void *p, uint32_t (&o)[4]) {
  if (sizeof(Pix) == 2) {
    __builtin_memcpy(o, p, 16);
  } else {
    uint32_t a[2];
    __builtin_memcpy(a, p, 8);
#pragma unroll
    for (int i = 0; i < 2; i++) {      // bytes 0, 1 and 2, 3 of a dword -> two uint16 each (0x0c selects a zero byte)
      o[2 * i] = __builtin_amdgcn_perm(0u, a[i], 0x0c010c00u);
      o[2 * i + 1] = __builtin_amdgcn_perm(0u, a[i], 0x0c030c02u);
    }
  }
}

template <typename Pix, int TAPS>      // TAPS: both passes of all planes use this many taps; 0 = the counts are run-time values (<= 24)
__global__ __launch_bounds__(256) void k_scale(ScaleLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr int G = 16 / (int)sizeof(Pix);      // samples per lane in the vertical pass
  constexpr int NP = TAPS ? TAPS / 2 : 12;      // coefficient pairs held in registers
  const unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const ScalePlaneDesc *D = reinterpret_cast<const ScalePlaneDesc *>(L.tab);
  const int p = bid < (unsigned)L.first_wg1 ? 0 : bid < (unsigned)L.first_wg2 ? 1 : 2;
  const ScalePlaneDesc d = D[p];
  const Pix *src = reinterpret_cast<const Pix *>(p == 0 ? L.src[0] : p == 1 ? L.src[1] : L.src[2]);      // (selects: no indexed kernel argument)
  Pix *dst = reinterpret_cast<Pix *>(p == 0 ? L.dst[0] : p == 1 ? L.dst[1] : L.dst[2]);
  const int t = (int)bid - (p == 0 ? 0 : p == 1 ? L.first_wg1 : L.first_wg2), per = d.tiles_x * d.tiles_y;
  const int f = t / per, rem = t - f * per, ty = rem / d.tiles_x, tx = rem - ty * d.tiles_x;
  const int twl = L.tile_w_log2, tile_w = 1 << twl;
  const int j0 = tx << twl, i0 = ty * L.tile_h;
  const int tw = min(tile_w, d.dst_w - j0), th = min(L.tile_h, d.dst_h - i0);
  const int nph = TAPS ? NP : d.taps_h >> 1, npv = TAPS ? NP : d.taps_v >> 1;
  const int *fh = reinterpret_cast<const int *>(L.tab) + d.first_h, *fv = reinterpret_cast<const int *>(L.tab) + d.first_v;
  // the source window of the tile: columns x0 .. (x0 even, so that a sample pair is an aligned LDS dword), rows y0 ..
  const int x0 = fh[j0] & ~1, nx = fh[j0 + tw - 1] + 2 * nph - x0;
  const int y0 = fv[i0], ny = fv[i0 + th - 1] + 2 * npv - y0;
  const int wsd = L.win_stride >> 1;                      // window row stride in dwords (a multiple of 4)
  const int isd = (tile_w + 8) >> 1;                      // intermediate row stride in dwords
  uint32_t *win = lds;
  uint32_t *inter = lds + L.win_rows * wsd;
  const int tid = threadIdx.x;

  // ---- stage: 8 samples per lane and step
  {
    const int ncx = (nx + 7) >> 3;
    for (int c = tid; c < ny * ncx; c += 256) {
      const int row = c / ncx, cx = c - row * ncx, sx = x0 + 8 * cx;
      const Pix *rp = src + d.origin + (size_t)(f * d.src_rows + min(max(y0 + row, 0), d.src_h - 1)) * d.src_stride;
      uint32_t o[4];
      if (sx >= 0 && sx + 7 < d.src_w) {
        widen8<Pix>(rp + sx, o);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          o[i] = (uint32_t)rp[min(max(sx + 2 * i, 0), d.src_w - 1)] | ((uint32_t)rp[min(max(sx + 2 * i + 1, 0), d.src_w - 1)] << 16);
      }
      *reinterpret_cast<u32x4 *>(win + row * wsd + cx * 4) = u32x4{ o[0], o[1], o[2], o[3] };
    }
  }
  __syncthreads();

  // ---- horizontal: lane = output column of the tile, rows strided
  {
    const int j = tid & (tile_w - 1);
    if (j < tw) {
      const int o = fh[j0 + j] - x0, od = o >> 1;
      const uint32_t sh = (uint32_t)(o & 1) << 4;
      const uint32_t *cp = L.tab + d.coef_h + (size_t)(j0 + j) * nph;
      uint32_t cf[NP];
#pragma unroll
      for (int k = 0; k < NP; k++) cf[k] = k < nph ? cp[k] : 0u;
      int16_t *im = reinterpret_cast<int16_t *>(inter);
      for (int row = tid >> twl; row < ny; row += 256 >> twl) {
        const uint32_t *wr = win + row * wsd + od;
        int acc = 1 << 9;
        uint32_t lo = wr[0];
#pragma unroll
        for (int k = 0; k < NP; k++) {
          if (!TAPS && k >= nph) break;
          const uint32_t hi = wr[k + 1];
          acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, __builtin_amdgcn_alignbit(hi, lo, sh)), __builtin_bit_cast(s16x2, cf[k]), acc, false);
          lo = hi;
        }
        im[row * (isd * 2) + j] = (int16_t)(acc >> 10);
      }
    }
  }
  __syncthreads();

  // ---- vertical: lane = G samples (16 bytes) of one output row
  {
    const int gl = twl - (sizeof(Pix) == 2 ? 3 : 4);      // log2 of the 16-byte groups per tile row
    for (int it = tid; it < (th << gl); it += 256) {
      const int i = it >> gl, c0 = (it & ((1 << gl) - 1)) * G;
      if (c0 >= tw) continue;
      const uint32_t *cp = L.tab + d.coef_v + (size_t)(i0 + i) * npv;
      const uint32_t *ir = inter + (fv[i0 + i] - y0) * isd + (c0 >> 1);
      int acc[G];
#pragma unroll
      for (int m = 0; m < G; m++) acc[m] = 1 << 17;
#pragma unroll
      for (int k = 0; k < NP; k++) {
        if (!TAPS && k >= npv) break;
        const s16x2 cf = __builtin_bit_cast(s16x2, cp[k]);
        uint32_t a[G / 2], b[G / 2];
#pragma unroll
        for (int q = 0; q < G / 8; q++) {
          const u32x4 va = *reinterpret_cast<const u32x4 *>(ir + (2 * k) * isd + 4 * q), vb = *reinterpret_cast<const u32x4 *>(ir + (2 * k + 1) * isd + 4 * q);
          a[4 * q] = va.x; a[4 * q + 1] = va.y; a[4 * q + 2] = va.z; a[4 * q + 3] = va.w;
          b[4 * q] = vb.x; b[4 * q + 1] = vb.y; b[4 * q + 2] = vb.z; b[4 * q + 3] = vb.w;
        }
#pragma unroll
        for (int m = 0; m < G / 2; m++) {      // (row 2k, row 2k + 1) of column 2m and of column 2m + 1
          acc[2 * m] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, __builtin_amdgcn_perm(b[m], a[m], 0x05040100u)), cf, acc[2 * m], false);
          acc[2 * m + 1] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, __builtin_amdgcn_perm(b[m], a[m], 0x07060302u)), cf, acc[2 * m + 1], false);
        }
      }
      uint32_t o[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        o[q] = 0;
#pragma unroll
        for (int m = 0; m < G / 4; m++)
          o[q] |= (uint32_t)min(max(acc[q * (G / 4) + m] >> 18, 0), L.max_val) << (m * 8 * (int)sizeof(Pix));
      }
      Pix *out = dst + (size_t)(f * d.dst_h + i0 + i) * d.dst_w + j0 + c0;
      const int n = tw - c0;      // samples of this group inside the plane: a multiple of 4
      if (n >= G) {
        *reinterpret_cast<u32x4_a4 *>(out) = u32x4_a4{ o[0], o[1], o[2], o[3] };
      } else if (sizeof(Pix) == 2) {      // 4 samples = 8 bytes
        *reinterpret_cast<u32x2_a4 *>(out) = u32x2_a4{ o[0], o[1] };
      } else {                            // 4, 8 or 12 samples, 4 bytes each
#pragma unroll
        for (int q = 0; q < 3; q++)
          if (4 * q < n) reinterpret_cast<uint32_t *>(out)[q] = o[q];
      }
    }
  }
}

// Lanczos-3 window
double lanczos3(double x) {
  const double kPi = 3.14159265358979323846;
  if (x < 0) x = -x;
  if (x >= 3.0) return 0.0;
  if (x == 0.0) return 1.0;
  const double a = kPi * x, b = a / 3.0;
  return (sin(a) / a) * (sin(b) / b);
}

}  // namespace

// the table of include/av1mi.h for n source -> m output samples (no limits checked here: the planes of a frame may be smaller than
// what the public entry point accepts); coef: m rows of T int16
int scale_taps(int n, int m) { return 2 * (int)((3L * (n > m ? n : m) + m - 1) / m); }
void scale_filter_rows(int n, int m, int32_t *first, int16_t *coef) {
  const int T = scale_taps(n, m);
  const double s = (double)(n > m ? n : m) / (double)m;
  std::vector<double> w((size_t)T);
  for (int j = 0; j < m; j++) {
    const long num = (2L * j + 1) * n - m;      // centre c = num / (2 m)
    const long fl = num >= 0 ? num / (2L * m) : -((-num + 2L * m - 1) / (2L * m));
    const int f0 = (int)fl - T / 2 + 1;
    const double c = (double)num / (double)(2L * m);
    double sum = 0;
    for (int k = 0; k < T; k++) { w[(size_t)k] = lanczos3(((double)(f0 + k) - c) / s); sum += w[(size_t)k]; }
    int16_t *row = coef + (size_t)j * T;
    int total = 0, big = 0;
    for (int k = 0; k < T; k++) {
      const int q = (int)floor(w[(size_t)k] / sum * 16384.0 + 0.5);
      row[k] = (int16_t)q;
      total += q;
      if (abs(q) > abs((int)row[big])) big = k;
    }
    row[big] = (int16_t)(row[big] + (16384 - total));
    first[j] = f0;
  }
}

const char *scale_geometry_error(int sw, int sh, int dw, int dh) {
  if (sw < 16 || sh < 16 || dw < 16 || dh < 16) return "scaling needs source and target of at least 16x16";
  if (sw > 4096 || sh > 4096 || dw > 4096 || dh > 4096) return "scaling takes sources and targets up to 4096x4096";
  if (sw > 4 * dw || dw > 4 * sw || sh > 4 * dh || dh > 4 * sh) return "scaling ratio outside [1/4, 4]";
  // the half-size chroma planes of an odd target can fall just outside
  if ((sw + 1) / 2 > 4 * (dw / 2) || (sh + 1) / 2 > 4 * (dh / 2)) return "scaling ratio of the chroma planes outside [1/4, 4]";
  return nullptr;
}

struct ScalePlan {
  int bd = 0, sw = 0, sh = 0, dw = 0, dh = 0;
  void *d_tab = nullptr;
  int tile_w_log2 = 6, tile_h = 16, win_stride = 0, win_rows = 0, taps = 0;
  int tiles_per_frame[3] = {};
  size_t lds_bytes = 0;
};

bool scale_plan_is(const ScalePlan *P, int bd, int sw, int sh, int dw, int dh) {
  return P && P->bd == bd && P->sw == sw && P->sh == sh && P->dw == dw && P->dh == dh;
}
void scale_plan_destroy(ScalePlan *P) {
  if (!P) return;
  if (P->d_tab) (void)hipFree(P->d_tab);
  delete P;
}

// sw x sh: the true luma size of the source (its buffers are that rounded up to 8); dw x dh: the target luma size (the destination
// planes are that rounded up to 8).  Sizes and ratios are checked by the callers.
hipError_t scale_plan_create(int bd, int sw, int sh, int dw, int dh, ScalePlan **out, const CropWindow *window) {
  *out = nullptr;
  ScalePlan *P = new (std::nothrow) ScalePlan();
  if (!P) return hipErrorOutOfMemory;
  P->bd = bd; P->sw = sw; P->sh = sh; P->dw = dw; P->dh = dh;
  // (a window: the strides are those of the frames it lies in)
  const int sw8 = ((window ? window->frame_w : sw) + 7) & ~7, sh8 = ((window ? window->frame_h : sh) + 7) & ~7, cw = (dw + 7) & ~7, ch = (dh + 7) & ~7;
  struct Dir { int n = 0, m = 0, coded = 0, taps = 0; std::vector<int32_t> first; std::vector<int16_t> coef; };
  Dir dir[3][2];
  int taps_all = -1;
  for (int p = 0; p < 3; p++)
    for (int v = 0; v < 2; v++) {
      Dir &d = dir[p][v];
      const int ns = v ? sh : sw, nd = v ? dh : dw, nc = v ? ch : cw;
      d.n = p ? (ns + 1) / 2 : ns; d.m = p ? nd / 2 : nd; d.coded = p ? nc / 2 : nc;
      d.taps = scale_taps(d.n, d.m);
      if (d.taps > 24) { delete P; return hipErrorInvalidValue; }      // (a chroma plane just beyond 4:1 under an odd target)
      taps_all = taps_all < 0 || taps_all == d.taps ? d.taps : 0;
      d.first.resize((size_t)d.coded); d.coef.resize((size_t)d.coded * d.taps);
      scale_filter_rows(d.n, d.m, d.first.data(), d.coef.data());
      for (int j = d.m; j < d.coded; j++) {      // the padding of the coded size repeats the last true column / row
        d.first[(size_t)j] = d.first[(size_t)d.m - 1];
        memcpy(&d.coef[(size_t)j * d.taps], &d.coef[(size_t)(d.m - 1) * d.taps], (size_t)d.taps * 2);
      }
    }
  P->taps = taps_all == 6 || taps_all == 12 ? taps_all : 0;
  // the tile: as large as 64 KiB of LDS allow (window + intermediate of the worst tile of any plane)
  int twl = cw >= 128 ? 7 : 6, th = 16;
  for (;;) {
    int max_nx = 0, max_ny = 0;
    for (int p = 0; p < 3; p++) {
      const Dir &H = dir[p][0], &V = dir[p][1];
      for (int j0 = 0; j0 < H.coded; j0 += 1 << twl) {
        const int j1 = (j0 + (1 << twl) < H.coded ? j0 + (1 << twl) : H.coded) - 1;
        const int nx = H.first[(size_t)j1] + H.taps - (H.first[(size_t)j0] & ~1);
        if (nx > max_nx) max_nx = nx;
      }
      for (int i0 = 0; i0 < V.coded; i0 += th) {
        const int i1 = (i0 + th < V.coded ? i0 + th : V.coded) - 1;
        const int ny = V.first[(size_t)i1] + V.taps - V.first[(size_t)i0];
        if (ny > max_ny) max_ny = ny;
      }
    }
    // a row: the window rounded up to whole 8-sample steps, + 8 for the dword the funnel shift reads beyond an odd start
    P->win_stride = ((max_nx + 7) & ~7) + 8;
    P->win_rows = max_ny;
    P->lds_bytes = (size_t)P->win_rows * ((size_t)P->win_stride + (size_t)(1 << twl) + 8) * 2;
    if (P->lds_bytes <= 64 * 1024) break;
    if (th > 8) th = 8; else if (twl > 6) twl = 6; else if (th > 2) th /= 2; else { delete P; return hipErrorInvalidValue; }
  }
  P->tile_w_log2 = twl; P->tile_h = th;
  std::vector<uint32_t> tab(48);
  ScalePlaneDesc desc[3];
  memset(desc, 0, sizeof(desc));
  for (int p = 0; p < 3; p++) {
    const Dir &H = dir[p][0], &V = dir[p][1];
    ScalePlaneDesc &d = desc[p];
    d.src_w = H.n; d.src_h = V.n; d.src_stride = p ? sw8 / 2 : sw8; d.src_rows = p ? sh8 / 2 : sh8;
    if (window) d.origin = (p ? window->y / 2 : window->y) * d.src_stride + (p ? window->x / 2 : window->x);
    d.dst_w = H.coded; d.dst_h = V.coded; d.taps_h = H.taps; d.taps_v = V.taps;
    d.tiles_x = (H.coded + (1 << twl) - 1) >> twl; d.tiles_y = (V.coded + th - 1) / th;
    P->tiles_per_frame[p] = d.tiles_x * d.tiles_y;
    auto put = [&](const void *src, size_t bytes) { const size_t at = tab.size(); tab.resize(at + (bytes + 3) / 4); memcpy(&tab[at], src, bytes); return (int)at; };
    d.first_h = put(H.first.data(), H.first.size() * 4); d.coef_h = put(H.coef.data(), H.coef.size() * 2);
    d.first_v = put(V.first.data(), V.first.size() * 4); d.coef_v = put(V.coef.data(), V.coef.size() * 2);
  }
  memcpy(tab.data(), desc, sizeof(desc));
  hipError_t e = hipMalloc(&P->d_tab, tab.size() * 4);
  if (e == hipSuccess) e = hipMemcpy(P->d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { scale_plan_destroy(P); return e; }
  *out = P;
  return hipSuccess;
}

hipError_t launch_scale(const ScalePlan *P, int frames, const void *const *src, void *const *dst, hipStream_t s) {
  if (!P || frames < 1) return hipErrorInvalidValue;
  ScaleLaunch L;
  memset(&L, 0, sizeof(L));
  for (int p = 0; p < 3; p++) { L.src[p] = src[p]; L.dst[p] = dst[p]; }
  L.tab = (const uint32_t *)P->d_tab;
  L.tile_w_log2 = P->tile_w_log2; L.tile_h = P->tile_h; L.win_stride = P->win_stride; L.win_rows = P->win_rows;
  L.max_val = (1 << P->bd) - 1;
  L.first_wg1 = P->tiles_per_frame[0] * frames; L.first_wg2 = L.first_wg1 + P->tiles_per_frame[1] * frames;
  const unsigned total = (unsigned)(L.first_wg2 + P->tiles_per_frame[2] * frames);
  const dim3 grid(total), block(256);
  const size_t lds = P->lds_bytes;
  using Kernel = void (*)(ScaleLaunch);
  static const Kernel kernels[2][3] = { { k_scale<uint8_t, 0>, k_scale<uint8_t, 6>, k_scale<uint8_t, 12> }, { k_scale<uint16_t, 0>, k_scale<uint16_t, 6>, k_scale<uint16_t, 12> } };
  hipLaunchKernelGGL(kernels[P->bd != 8][P->taps == 6 ? 1 : P->taps == 12 ? 2 : 0], grid, block, lds, s, L);
  return hipGetLastError();
}

}  // namespace av1mi

extern "C" int av1mi_scale_filter(int src_n, int dst_n, int *taps, int32_t *first, int16_t *coef) {
  if (!taps || src_n < 8 || dst_n < 8 || src_n > 4096 || dst_n > 4096 || src_n > 4 * dst_n || dst_n > 4 * src_n) return AV1MI_E_INVAL;
  *taps = av1mi::scale_taps(src_n, dst_n);
  if (!first) return AV1MI_OK;
  if (!coef) return AV1MI_E_INVAL;
  av1mi::scale_filter_rows(src_n, dst_n, first, coef);
  return AV1MI_OK;
}
