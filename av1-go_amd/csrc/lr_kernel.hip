// lr_kernel.hip — SURVEY.md §8a row K7: loop restoration (Wiener and self-guided) of one plane, frames of a
// segment along blockIdx.z.
//
// A workgroup owns the intersection of one 64-row stripe (32 for 4:2:0 chroma; stripes are offset 8 luma rows
// upwards, AV1 spec §7.17) with one column band no wider than a restoration unit, so every sample it writes has
// the same stripe limits AND the same unit parameters: no divergence.  It stages that block plus a 3-sample halo
// in LDS through the spec's get_source_sample rule, then runs the Wiener or the self-guided filter on it: the
// phases, each described where it is written, are in lr_filter.hpp.
// Reads two planes, writes one: algorithmic HBM traffic 2b*S (SURVEY.md §8d counts b read + b written; the
// deblocked rows are 4 of every 64).  Restates spec §7.17.3/4/6 and libaom av1_highbd_wiener_convolve_add_src_c /
// av1_selfguided_restoration_c; the reference has no counterpart (internal/ffmpeg/transcode.go:120).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "av1_ops.hpp"
#include "lr_filter.hpp"

namespace av1mi {

// Workgroup `bid` of the plane's `nwg`.  SUBY: vertical subsampling of the plane (0 luma, 1 chroma of 4:2:0) — stripe height and
// offset become constants.  A device function over the workgroup's LDS, which the kernel declares: k_lr runs it for one plane,
// k_lr_yuv for the three planes of 4:2:0 frames in one launch.
template <typename Pix, int SUBY, bool SGR>
__device__ __forceinline__ void lr_tile(const LrLaunch &L, unsigned bid, unsigned nwg, LrLds<SGR> &lds) {
  constexpr int bd = sizeof(Pix) == 1 ? 8 : 10;              // the launch picks the instantiation by L.bd (8 or 10)
  const LrGeom G(L.w, L.h, SUBY, L.unit_size, L.nframes);
  const Tile3 tl = xcd_tile(G.bands, G.stripes, L.nframes, bid, nwg);
  const int X0 = tl.x * G.tile_w, stripe = tl.y, f = tl.z;
  LrTile<Pix> T;
  T.stride = L.stride; T.w = L.w; T.h = L.h; T.X0 = X0; T.sstart = G.first_row(stripe); T.send = T.sstart + G.stripe_h - 1;
  T.y0 = max(T.sstart, 0); T.y1 = min(T.send, L.h - 1);      // rows this workgroup writes
  if (T.y0 > T.y1 || X0 >= L.w) return;
  // Two-pass form of the decision: the workgroups that have nothing to do leave before they load anything (uniform per workgroup,
  // before any barrier).
  const bool sampled = G.sampled(X0, stripe);
  if (L.pass == 1 && !sampled) return;
  if (L.pass == 2 && (sampled || !L.keep[(size_t)f * L.keep_stride])) return;
  T.bw = min(G.tile_w, L.w - X0); T.bh = T.y1 - T.y0 + 1;
  const size_t frame = (size_t)f * L.h * L.stride;
  T.cdef = reinterpret_cast<const Pix *>(L.cdef) + frame; T.dbl = reinterpret_cast<const Pix *>(L.dbl) + frame;
  T.out = reinterpret_cast<Pix *>(L.out) + frame;
  T.orig = L.orig && sampled ? reinterpret_cast<const Pix *>(L.orig) + frame : nullptr;
  const LrUnit U = lr_unit(L.units + ((size_t)f * L.unit_frame_stride + G.unit_index(X0, T.y0)) * 8);
  const int type = (!SGR && U.type == 2) ? 0 : U.type;
  LrErr err;
  if (type == 0) lr_copy(T, err);
  else {
    if (X0 >= 4 && X0 + T.bw + 4 <= L.w && !(T.bw & 3)) lr_stage_aligned(T, lds.src);
    else lr_stage_clamped(T, lds.src);
    __syncthreads();
    if (type != 1) { if constexpr (SGR) lr_sgr<Pix, bd>(T, lds, err, U); }
    else if (!(T.bw & 3)) lr_wiener_packed<Pix, bd>(T, lds, err, U);
    else lr_wiener_scalar<Pix, bd>(T, lds, err, U);
  }
  // (uniform: no decision asked for, or a tile outside the sample.  Every thread of a workgroup that comes here at all comes here:
  // uniform control flow up to the returns, and there is a barrier inside)
  if (T.orig) err.finish(lds, L, f, stripe);
}

template <typename Pix, int SUBY, bool SGR = true>
__global__ __launch_bounds__(256) void k_lr(LrLaunch L) {
  __shared__ LrLds<SGR> lds;
  lr_tile<Pix, SUBY, SGR>(L, blockIdx.x, gridDim.x, lds);
}
// the three planes' grids end to end: the plane, and with it SUBY, from the workgroup's index (uniform per workgroup)
template <typename Pix, bool SGR>
__global__ __launch_bounds__(256) void k_lr_yuv(LrYuvLaunch Y) {
  __shared__ LrLds<SGR> lds;
  const unsigned b = blockIdx.x;
  if (b < Y.first[1]) lr_tile<Pix, 0, SGR>(Y.plane[0], b, Y.first[1], lds);
  else if (b < Y.first[2]) lr_tile<Pix, 1, SGR>(Y.plane[1], b - Y.first[1], Y.first[2] - Y.first[1], lds);
  else lr_tile<Pix, 1, SGR>(Y.plane[2], b - Y.first[2], gridDim.x - Y.first[2], lds);
}

// Restoration stays on for frame f of plane p when it lowered the squared error: on[f * on_stride + p] = sum over the stripes.
// thread = (frame, plane) of nplanes = 1 (geometry y) or 3 (4:2:0: y, c, c; the planes' sums end to end, lr_first_pair).  clear: the sums
// a thread has read it leaves ZERO, what the next call's pass 1 adds into (it is their only reader; capi.hip lr_yuv_decide_with: the rule)
__global__ __launch_bounds__(64) void k_lr_decide(unsigned long long *sse, LrGeom y, LrGeom c, int nplanes, uint8_t *on, int on_stride, bool clear) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= y.nframes * nplanes) return;
  const int f = i / nplanes, p = i - nplanes * f, stripes = p ? c.stripes : y.stripes;
  unsigned long long *q = sse + 2 * (lr_first_pair(y, c, p) + (size_t)f * stripes);
  unsigned long long a = 0, b = 0;
  for (int s = 0; s < stripes; s++) { a += q[2 * s]; b += q[2 * s + 1]; if (clear) q[2 * s] = q[2 * s + 1] = 0; }
  on[(size_t)f * on_stride + p] = a < b;
}
hipError_t launch_lr_decide(unsigned long long *sse, const LrGeom &y, const LrGeom &c, int nplanes, uint8_t *on, int on_stride, bool clear, hipStream_t s) {
  hipLaunchKernelGGL(k_lr_decide, dim3((unsigned)((y.nframes * nplanes + 63) / 64)), dim3(64), 0, s, sse, y, c, nplanes, on, on_stride, clear);
  return hipGetLastError();
}

// ---- The restoration search (av1mi.h "restoration search").  k_lr_search: k_lr_yuv's tiles — a stripe x a band of 64 columns, the
// three planes' grids end to end — each staged once through the get_source_sample rule, then per horizontal filter the int16
// intermediate and one vertical pass over it that sums the squared error of every vertical filter's output against the source.  No
// sample is stored: a workgroup's nine sums go by 64-bit integer atomic adds into its unit's entry of the cost table (a unit spans
// several tiles: the stripes split it at rows 64 k - 8, and edge units are up to 1.5 units long).
template <typename Pix, int SUBY>
__device__ __forceinline__ void lr_search_tile(const LrSearchLaunch &S, int p, unsigned bid, unsigned nwg, LrLds<false> &lds) {
  constexpr int bd = sizeof(Pix) == 1 ? 8 : 10;
  const LrGeom G(S.w[p], S.h[p], SUBY, S.unit_size, S.nframes);
  const Tile3 tl = xcd_tile(G.bands, G.stripes, S.nframes, bid, nwg);
  const int X0 = tl.x * G.tile_w, f = tl.z;
  LrTile<Pix> T;
  T.stride = S.stride[p]; T.w = G.w; T.h = G.h; T.X0 = X0; T.sstart = G.first_row(tl.y); T.send = T.sstart + G.stripe_h - 1;
  T.y0 = max(T.sstart, 0); T.y1 = min(T.send, G.h - 1);
  if (T.y0 > T.y1 || X0 >= G.w) return;      // (uniform per workgroup, before any barrier)
  T.bw = min(G.tile_w, G.w - X0); T.bh = T.y1 - T.y0 + 1;
  const size_t frame = (size_t)f * G.h * T.stride;
  T.cdef = reinterpret_cast<const Pix *>(S.cdef[p]) + frame; T.dbl = reinterpret_cast<const Pix *>(S.dbl[p]) + frame;
  T.orig = reinterpret_cast<const Pix *>(S.orig[p]) + frame; T.out = nullptr;
  if (X0 >= 4 && X0 + T.bw + 4 <= G.w && !(T.bw & 3)) lr_stage_aligned(T, lds.src);
  else lr_stage_clamped(T, lds.src);
  __syncthreads();
  const LrSearchTaps F = lr_search_taps(S.taps[p ? 1 : 0]);
  unsigned err[kLrCands] = {};
  // candidate 3 v + h: the horizontal filters one after the other, under each the vertical ones (the pair (0, 0) is left out)
  auto passes = [&](auto &&horizontal, auto &&vertical_all, auto &&vertical_from1) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < kLrFilters; h++) {
      if (h) __syncthreads();      // the last vertical pass has read the intermediate
      horizontal(F.f[h]);
      __syncthreads();
      unsigned e[kLrFilters] = {};
      if (h) vertical_all(e); else vertical_from1(e);
#pragma unroll
      for (int v = 0; v < kLrFilters; v++) err[3 * v + h] += e[v];
    }
  };
  if (!(T.bw & 3)) {
    uint2 sv[2][2];
    lr_search_source(T, sv);
    err[0] = lr_search_none_packed(lds.src, T.bw, T.bh, sv);
    passes([&](const int (&hf)[7]) __attribute__((always_inline)) { lr_wiener_h_packed<bd>(lds.src, lds.inter(), T.bw, T.bh, hf); },
           [&](unsigned (&e)[kLrFilters]) __attribute__((always_inline)) { lr_search_v_packed<bd, 0>(lds.inter(), T.bw, T.bh, F, sv, e); },
           [&](unsigned (&e)[kLrFilters]) __attribute__((always_inline)) { lr_search_v_packed<bd, 1>(lds.inter(), T.bw, T.bh, F, sv, e); });
  } else {
    err[0] = lr_search_none_scalar(T, lds.src);
    passes([&](const int (&hf)[7]) __attribute__((always_inline)) { lr_wiener_h_scalar<bd>(lds.src, lds.inter(), T.bw, T.bh, hf); },
           [&](unsigned (&e)[kLrFilters]) __attribute__((always_inline)) { lr_search_v_scalar<Pix, bd, 0>(T, lds.inter(), F, e); },
           [&](unsigned (&e)[kLrFilters]) __attribute__((always_inline)) { lr_search_v_scalar<Pix, bd, 1>(T, lds.inter(), F, e); });
  }
  lr_search_finish(lds, err, S.sums + ((size_t)f * S.units_frame + S.unit_first[p] + G.unit_index(X0, T.y0)) * kLrCands);
}
template <typename Pix>
__global__ __launch_bounds__(256) void k_lr_search(LrSearchLaunch S) {
  __shared__ LrLds<false> lds;
  const unsigned b = blockIdx.x;
  if (b < S.first[1]) lr_search_tile<Pix, 0>(S, 0, b, S.first[1], lds);
  else if (b < S.first[2]) lr_search_tile<Pix, 1>(S, 1, b - S.first[1], S.first[2] - S.first[1], lds);
  else lr_search_tile<Pix, 1>(S, 2, b - S.first[2], gridDim.x - S.first[2], lds);
}
// k_lr_pick: one lane per unit of a frame's three planes.  J_c = SSE_c + lambda * bits_c in 64-bit integers, the lowest J wins, the
// lowest index on a tie; the unit's 8-byte record into its plane's array, the chosen index into choice
__global__ __launch_bounds__(64) void k_lr_pick(LrSearchLaunch S) {
  const unsigned i = blockIdx.x * 64 + threadIdx.x;
  if (i >= (unsigned)S.nframes * S.units_frame) return;
  const unsigned f = i / S.units_frame, u = i - f * S.units_frame;
  const int p = u < S.unit_first[1] ? 0 : u < S.unit_first[2] ? 1 : 2, cls = p ? 1 : 0;
  const unsigned nunits = (p == 2 ? S.units_frame : S.unit_first[p + 1]) - S.unit_first[p];
  const unsigned long long *sse = S.sums + (size_t)i * kLrCands;
  int best = 0;
  long long bestj = 0;
  for (int c = 0; c < kLrCands; c++) {
    const long long j = (long long)sse[c] + S.lambda * S.bits[cls][c];
    if (c == 0 || j < bestj) { best = c; bestj = j; }
  }
  typedef signed char i8x8 __attribute__((ext_vector_type(8)));
  i8x8 rec = { 0, 0, 0, 0, 0, 0, 0, 0 };
  if (best) {
    const int8_t *v = S.taps[cls][best / 3], *h = S.taps[cls][best % 3];
    rec = i8x8{ 1, v[0], v[1], v[2], h[0], h[1], h[2], 0 };
  }
  *reinterpret_cast<i8x8 *>(S.units[p] + ((size_t)f * nunits + (u - S.unit_first[p])) * 8) = rec;
  S.choice[i] = (uint8_t)best;
}
hipError_t launch_lr_search(LrSearchLaunch &S, hipStream_t s) {
  unsigned n = 0;
  for (int p = 0; p < 3; p++) { S.first[p] = n; n += LrGeom(S.w[p], S.h[p], p ? 1 : 0, S.unit_size, S.nframes).workgroups(); }
  if (S.bd == 8) hipLaunchKernelGGL(k_lr_search<uint8_t>, dim3(n), dim3(256), 0, s, S);
  else hipLaunchKernelGGL(k_lr_search<uint16_t>, dim3(n), dim3(256), 0, s, S);
  return hipGetLastError();
}
hipError_t launch_lr_pick(const LrSearchLaunch &S, hipStream_t s) {
  const unsigned n = (unsigned)S.nframes * S.units_frame;
  hipLaunchKernelGGL(k_lr_pick, dim3((n + 63) / 64), dim3(64), 0, s, S);
  return hipGetLastError();
}
// The candidates (av1mi.h states the table): the 1-D filters I, D, L per plane class as (tap0, tap1, tap2)
static const int8_t kLrSearchTaps[2][3][3] = { { { 0, 0, 0 }, { 3, -7, 15 }, { 0, 2, 14 } }, { { 0, 0, 0 }, { 0, -7, 15 }, { 0, 2, 14 } } };
void lr_search_tables(LrSearchLaunch *S) {
  memcpy(S->taps, kLrSearchTaps, sizeof(kLrSearchTaps));
  for (int cls = 0; cls < 2; cls++)
    for (int c = 0; c < kLrCands; c++) S->bits[cls][c] = lr_search_bits(cls, c);
}
void lr_search_record(int chroma, int c, int8_t rec[8]) {
  memset(rec, 0, 8);
  if (c < 1 || c >= kLrCands) return;
  const int8_t *v = kLrSearchTaps[chroma ? 1 : 0][c / 3], *h = kLrSearchTaps[chroma ? 1 : 0][c % 3];
  rec[0] = 1;
  for (int i = 0; i < 3; i++) { rec[1 + i] = v[i]; rec[4 + i] = h[i]; }
}
// bits_c: one for the use_wiener symbol, and the literal bits the coder's own syntax function (av1_ops.hpp tok_signed_subexp_ref)
// emits for the record's taps against the default reference taps — what tok_lr codes with one superblock per tile
namespace { struct BitCounter { int n = 0; void lit(unsigned, int nbits) { n += nbits; } }; }
int lr_search_bits(int chroma, int c) {
  int8_t u[8];
  lr_search_record(chroma, c, u);
  BitCounter k;
  if (u[0] == 1) av1ops::tok_wiener_taps(k, av1ops::lr_record_word(u), chroma != 0);
  return 1 + k.n;
}

// A frame whose true size (vw x vh) is not a multiple of 8 is coded at the size rounded up (w x h, at most 7 more columns / rows).
// A decoder clamps motion-compensation and restoration reads at the TRUE last column / row (spec 7.11.3.4 lastX / lastY, 7.17
// PlaneEndX / PlaneEndY); the kernels clamp at the coded size.  Replicating the true edge into the padding makes both read the
// same values.  One thread per padded sample: first the columns right of vw for the rows above vh, then whole rows below vh
// (which copy row vh - 1 with ITS columns already clamped).
template <typename Pix> __global__ __launch_bounds__(256) void k_extend(Pix *plane, int stride, int w, int h, int vw, int vh, int nframes) {
  const int pw = w - vw, ph = h - vh;                 // padding columns / rows
  const long per = (long)pw * vh + (long)ph * w;      // padded samples of a frame
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per * nframes) return;
  const int f = (int)(i / per);
  const long k = i - (long)f * per;
  Pix *p = plane + (size_t)f * h * stride;
  int x, y;
  if (k < (long)pw * vh) { y = (int)(k / pw); x = vw + (int)(k - (long)y * pw); }
  else { const long r = k - (long)pw * vh; y = vh + (int)(r / w); x = (int)(r - (long)(y - vh) * w); }
  p[(size_t)y * stride + x] = p[(size_t)min(y, vh - 1) * stride + min(x, vw - 1)];
}
hipError_t launch_extend(void *plane, int stride, int w, int h, int vw, int vh, int bd, int nframes, hipStream_t s) {
  const long n = ((long)(w - vw) * vh + (long)(h - vh) * w) * nframes;
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (bd == 8) hipLaunchKernelGGL(k_extend<uint8_t>, grid, dim3(256), 0, s, (uint8_t *)plane, stride, w, h, vw, vh, nframes);
  else hipLaunchKernelGGL(k_extend<uint16_t>, grid, dim3(256), 0, s, (uint16_t *)plane, stride, w, h, vw, vh, nframes);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_zero16(uint4 *p, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = make_uint4(0, 0, 0, 0);
}
hipError_t launch_zero16(void *p, size_t bytes, hipStream_t s) {      // bytes: a multiple of 16
  const size_t n = bytes / 16;
  if (n) hipLaunchKernelGGL(k_zero16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint4 *)p, n);
  return hipGetLastError();
}
hipError_t launch_lr(const LrLaunch &L, hipStream_t s) {
  const dim3 grid(LrGeom(L).workgroups());   // 1-D: the kernel orders the tiles (xcd_tile)
#define AV1MI_LR(PIX, SUBY) do { if (L.no_sgr) hipLaunchKernelGGL((k_lr<PIX, SUBY, false>), grid, dim3(256), 0, s, L); \
                                  else hipLaunchKernelGGL((k_lr<PIX, SUBY, true>), grid, dim3(256), 0, s, L); } while (0)
  if (L.ss) { if (L.bd == 8) AV1MI_LR(uint8_t, 1); else AV1MI_LR(uint16_t, 1); }
  else { if (L.bd == 8) AV1MI_LR(uint8_t, 0); else AV1MI_LR(uint16_t, 0); }
#undef AV1MI_LR
  return hipGetLastError();
}
hipError_t launch_lr_yuv(LrYuvLaunch &Y, hipStream_t s) {
  if (Y.plane[0].ss != 0 || Y.plane[1].ss != 1 || Y.plane[2].ss != 1) return hipErrorInvalidValue;
  unsigned n = 0;
  for (int p = 0; p < 3; p++) { Y.first[p] = n; n += LrGeom(Y.plane[p]).workgroups(); }
  const LrLaunch &L = Y.plane[0];
  const dim3 grid(n);
#define AV1MI_LR3(PIX) do { if (L.no_sgr) hipLaunchKernelGGL((k_lr_yuv<PIX, false>), grid, dim3(256), 0, s, Y); \
                            else hipLaunchKernelGGL((k_lr_yuv<PIX, true>), grid, dim3(256), 0, s, Y); } while (0)
  if (L.bd == 8) AV1MI_LR3(uint8_t); else AV1MI_LR3(uint16_t);
#undef AV1MI_LR3
  return hipGetLastError();
}

}  // namespace av1mi
