// lr_filter.hpp — loop restoration (AV1 spec §7.17) of one tile staged in LDS: the unit's parameters, the spec's get_source_sample
// row rule, the two staging routes, the Wiener filter (packed and scalar), the self-guided filter, the output routines and the
// on/off decision's error sums.  The phases of lr_tile (lr_kernel.hip), each a piece over the LDS of a 256-lane workgroup; k_lr and
// k_lr_yuv run the same source.  The geometry (LrGeom) stands beside LrLaunch in av1mi_internal.hpp, for the host as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "av1mi_internal.hpp"

namespace av1mi {

// Sgr_Params (spec 7.17.3): { r0, eps0, r1, eps1 }; s = ((1 << 20) + n*n*eps / 2) / (n*n*eps) is derived in the kernel
__device__ constexpr int kSgrParams[16][4] = {
  { 2, 12, 1, 4 }, { 2, 15, 1, 6 }, { 2, 18, 1, 8 }, { 2, 21, 1, 9 }, { 2, 24, 1, 10 }, { 2, 29, 1, 11 },
  { 2, 36, 1, 12 }, { 2, 45, 1, 13 }, { 2, 56, 1, 14 }, { 2, 68, 1, 15 }, { 0, 0, 1, 5 }, { 0, 0, 1, 8 },
  { 0, 0, 1, 11 }, { 0, 0, 1, 14 }, { 2, 30, 0, 0 }, { 2, 75, 0, 0 } };

// SGR: the launch may hold self-guided units.  Without them (the encoder's policy: Wiener or none) the A / B planes of that path
// are not allocated — 9 instead of 27 KB of scratch, 20 instead of 38 KB of LDS per workgroup, 8 instead of 4 workgroups per CU —
// and a unit of type 2 would be copied unfiltered (the caller promises there is none: LrLaunch::no_sgr).
// The buffers are sized by the 64 x 64 tile whatever the subsampling is, so luma and chroma workgroups of the merged launch use the
// same 20 KB (38 KB with self-guided units) and the occupancy of the luma launch stands.
// src: (bh + 6) rows of stride kLrSS, tile column 0 = X0 - 4; scratch: the Wiener intermediate, int16 (bh + 6) x kLrMaxW, or the
// self-guided A (u16) and B (i32) planes, (bh + 2) x (bw + 2) of row stride kLrAS
constexpr int kLrMaxH = 64, kLrMaxW = 64, kLrSS = kLrMaxW + 16, kLrAS = kLrMaxW + 2 + 2;
template <bool SGR> struct LrLds {
  __attribute__((aligned(16))) uint16_t src[(kLrMaxH + 6) * kLrSS];
  __attribute__((aligned(16))) unsigned char scratch[SGR ? (kLrMaxH + 2) * kLrAS * 2 + (kLrMaxH + 2) * kLrAS * 4 : (kLrMaxH + 6) * kLrMaxW * 2];
  unsigned long long sse[2][4];
  __device__ int16_t *inter() { return reinterpret_cast<int16_t *>(scratch); }
  __device__ uint16_t *A() { return reinterpret_cast<uint16_t *>(scratch); }
  __device__ int32_t *B() { return reinterpret_cast<int32_t *>(scratch + (kLrMaxH + 2) * kLrAS * 2); }
};

// a unit's 8 parameter bytes: the type (0 none, 1 Wiener, 2 self-guided), then three vertical and three horizontal taps (Wiener: the
// symmetric 7-tap filters vf, hf) or the parameter set and the two projection weights (self-guided).  One load, up front.
struct LrUnit { int type, vf[7], hf[7], set, w0, w1; };
__device__ __forceinline__ LrUnit lr_unit(const int8_t *p) {
  typedef signed char i8x8 __attribute__((ext_vector_type(8)));
  const i8x8 b = *reinterpret_cast<const i8x8 *>(p);
  LrUnit U = { b[0], {}, {}, b[1] & 15, b[2], b[3] };
#pragma unroll
  for (int i = 0; i < 3; i++) { U.vf[i] = U.vf[6 - i] = b[1 + i]; U.hf[i] = U.hf[6 - i] = b[4 + i]; }
  U.vf[3] = 128 - 2 * (b[1] + b[2] + b[3]); U.hf[3] = 128 - 2 * (b[4] + b[5] + b[6]);
  return U;
}

// The spec's get_source_sample row rule: row y clamped to the picture; inside the stripe the CDEF output, up to two rows beyond it
// the DEBLOCKED frame, further rows replicate those
struct LrRow { bool deblocked; int y; };
__device__ __forceinline__ LrRow lr_source_row(int y, int sstart, int send, int h) {
  y = min(max(y, 0), h - 1);
  if (y < sstart) return { true, max(sstart - 2, y) };
  if (y > send) return { true, min(send + 2, y) };
  return { false, y };
}

// One workgroup's tile: frame f's planes, the bw x bh block at (X0, y0) that it writes, the first and last row of its stripe.
// orig: the source plane when the decision's sums run over this tile, else null (uniform per workgroup)
template <typename Pix> struct LrTile {
  const Pix *cdef, *dbl, *orig; Pix *out;
  int stride, w, h, X0, y0, y1, bw, bh, sstart, send;
  __device__ __forceinline__ size_t at(int r, int c) const { return row_off(y0 + r, stride) + X0 + c; }      // sample (r, c) of the block in its plane
  __device__ __forceinline__ const Pix *source_row(int y) const {
    const LrRow s = lr_source_row(y, sstart, send, h);
    const Pix *c = cdef, *d = dbl;      // (both read first: chosen by address, the two members kept the whole tile in scratch memory)
    return (s.deblocked ? d : c) + row_off(s.y, stride);
  }
};

// The on/off decision's two sums: squared error of the restored samples and of the CDEF samples this workgroup covers, against the
// source; per lane in 32 bits (16 samples x 2^20), per wave and stripe into 64-bit words (finish)
struct LrErr {
  unsigned lr = 0, cd = 0;
  __device__ __forceinline__ void add(int o, int c, int sv) { const int a = o - sv, b = c - sv; lr += (unsigned)(a * a); cd += (unsigned)(b * b); }
  template <bool SGR> __device__ __forceinline__ void finish(LrLds<SGR> &lds, const LrLaunch &L, int f, int stripe) const {
    unsigned long long a = lr, b = cd;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_down(a, d, 64); b += __shfl_down(b, d, 64); }
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { lds.sse[0][tid >> 6] = a; lds.sse[1][tid >> 6] = b; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long *dst = L.sse + ((size_t)f * L.sse_stripes + stripe) * 2;
      atomicAdd(dst, lds.sse[0][0] + lds.sse[0][1] + lds.sse[0][2] + lds.sse[0][3]);
      atomicAdd(dst + 1, lds.sse[1][0] + lds.sse[1][1] + lds.sse[1][2] + lds.sse[1][3]);
    }
  }
};

// Output: sample (r, c) of the block, and with the decision on its error and the error of the CDEF sample cd against the source
template <typename Pix> __device__ __forceinline__ void lr_put1(const LrTile<Pix> &T, LrErr &err, int r, int c, int o, int cd) {
  T.out[T.at(r, c)] = (Pix)o;
  if (T.orig) err.add(o, cd, T.orig[T.at(r, c)]);
}
// ... four samples from column c (a multiple of 4) on: one store and one source load each where the address is aligned (it is when
// the plane's rows are 4-sample aligned), the four CDEF samples as one read of the LDS tile
template <typename Pix> __device__ __forceinline__ void lr_put4(const LrTile<Pix> &T, const uint16_t *src, LrErr &err, int r, int c, const int (&o)[4]) {
  typedef Pix Pix4 __attribute__((ext_vector_type(4)));
  typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
  Pix *d = T.out + T.at(r, c);
  if (T.orig) {
    const Pix *sp = T.orig + T.at(r, c);
    const u16x4 cd = *reinterpret_cast<const u16x4 *>(src + (r + 3) * kLrSS + c + 4);
    Pix4 sv;
    if (((uintptr_t)sp & (sizeof(Pix4) - 1)) == 0) sv = *reinterpret_cast<const Pix4 *>(sp);
    else sv = Pix4{ sp[0], sp[1], sp[2], sp[3] };
#pragma unroll
    for (int k = 0; k < 4; k++) err.add(o[k], cd[k], sv[k]);
  }
  const Pix4 v = { (Pix)o[0], (Pix)o[1], (Pix)o[2], (Pix)o[3] };
  if (((uintptr_t)d & (sizeof(Pix4) - 1)) == 0) *reinterpret_cast<Pix4 *>(d) = v;
  else { d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3]; }
}
// no restoration: copy the CDEF output
template <typename Pix> __device__ __forceinline__ void lr_copy(const LrTile<Pix> &T, LrErr &err) {
  for (int i = threadIdx.x; i < T.bh * T.bw; i += 256) {
    const int r = i / T.bw, c = i - r * T.bw;
    const Pix v = T.cdef[T.at(r, c)];
    lr_put1(T, err, r, c, v, v);
  }
}

// Staging: (bh + 6) rows x (bw + 8) columns of source samples, local row 0 == y0 - 3, local column 0 == X0 - 4 (4-aligned).
// The aligned route: no horizontal clamping and whole 4-sample groups (X0 >= 4, X0 + bw + 4 <= w, bw % 4 == 0).
template <typename Pix> __device__ __forceinline__ void lr_stage_aligned(const LrTile<Pix> &T, uint16_t *src) {
  const int tid = threadIdx.x, bh = T.bh;
  // item -> (row, group) by reciprocal multiplication (exact: items < 2^11 and (i + 0.5) / ng is never within 0.5 / ng of an
  // integer); an integer division by a run-time value is ~25 VALU instructions, and "full ? i / const : i / ng" evaluated both
  const float inv_ng = 1.0f / (float)((T.bw + 8) / 4);
  const int ng = (T.bw + 8) / 4, nmain = bh * ng, nhalo = 6 * ng;
  // All of a lane's loads first, then all of its LDS stores (as one loop every load was waited for before the next was issued,
  // and the kernel spent most of its time in those waits: waves stalled 64 % of their cycles by PMC).  The bh rows of the
  // block itself lie inside the stripe and the picture: plain CDEF rows, no clamping — at most 64 x 18 items = 5 per lane;
  // only the 3 + 3 halo rows go through the stripe rule — at most 108 items = 1 per lane.  The 8-byte loads need no alignment
  // check: the hardware takes any address.
  constexpr int NMAIN = (kLrMaxH * ((kLrMaxW + 8) / 4) + 255) / 256, NHALO = (6 * ((kLrMaxW + 8) / 4) + 255) / 256;
  uint2 o[NMAIN + NHALO];
  auto each_item = [&](auto &&body) __attribute__((always_inline)) {      // body(slot of o, row among the block's / the halo's, group, halo?) for this lane's items
#pragma unroll
    for (int k = 0; k < NMAIN + NHALO; k++) {
      const bool halo = k >= NMAIN;
      const int i = tid + 256 * (halo ? k - NMAIN : k);
      if (i < (halo ? nhalo : nmain)) { const int r = (int)(((float)i + 0.5f) * inv_ng); body(k, r, i - r * ng, halo); }
    }
  };
  each_item([&](int k, int r, int g, bool halo) __attribute__((always_inline)) {
    // (halo rows y0 - 3 .. y0 - 1 and y1 + 1 .. y1 + 3)
    const Pix *q = (halo ? T.source_row(r < 3 ? T.y0 - 3 + r : T.y1 - 2 + r) : T.cdef + row_off(T.y0, T.stride) + row_off(r, T.stride)) + T.X0 - 4 + 4 * g;
    if constexpr (sizeof(Pix) == 1) o[k].x = *reinterpret_cast<const uint32_t *>(q);
    else o[k] = *reinterpret_cast<const uint2 *>(q);
  });
  each_item([&](int k, int r, int g, bool halo) __attribute__((always_inline)) {
    uint2 w = o[k];
    if constexpr (sizeof(Pix) == 1) { const uint32_t u = w.x; w.x = __builtin_amdgcn_perm(0u, u, 0x0c010c00u); w.y = __builtin_amdgcn_perm(0u, u, 0x0c030c02u); }
    *reinterpret_cast<uint2 *>(src + __mul24(halo ? (r < 3 ? r : bh + r) : r + 3, kLrSS) + 4 * g) = w;
  });
}
// ... and the clamped route, sample by sample: columns X0 - 3 .. X0 + bw + 2 clamped to the picture
template <typename Pix> __device__ __forceinline__ void lr_stage_clamped(const LrTile<Pix> &T, uint16_t *src) {
  for (int i = threadIdx.x; i < (T.bh + 6) * (T.bw + 6); i += 256) {
    const int r = i / (T.bw + 6), c = i - r * (T.bw + 6);
    src[r * kLrSS + c + 1] = T.source_row(T.y0 - 3 + r)[min(max(T.X0 - 3 + c, 0), T.w - 1)];
  }
}

// Wiener (spec 7.17.4): 7-tap rows -> int16 intermediate in LDS -> 7-tap columns, rounds 3 / 11
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 lr_pk(int a, int b) { return __builtin_bit_cast(s16x2, (uint32_t)(a & 0xffff) | ((uint32_t)b << 16)); }
// The packed route (bw % 4 == 0): both passes on v_dot2_i32_i16 (two taps per instruction; samples and the clipped intermediate fit
// int16, the sums are exact in int32).  Horizontal: four outputs per lane from six aligned dwords of the source row (window columns
// c .. c + 11, the taps of output k start at column c + 1 + k): outputs 1 and 3 use the dwords as they are, outputs 0 and 2 the
// same dwords funnel-shifted by one sample.  Tap pairs (h0,h1) (h2,h3) (h4,h5) (h6,0).
// The horizontal pass of that route on its own (the restoration search runs it once per horizontal filter): the (bh + 6) x bw
// intermediate of the staged tile under the taps hf
template <int BD> __device__ __forceinline__ void lr_wiener_h_packed(const uint16_t *src, int16_t *inter, int bw, int bh, const int (&hf)[7]) {
  constexpr int offset = 1 << (BD + 3), limit = (1 << (BD + 5)) - 1;
  const s16x2 H0 = lr_pk(hf[0], hf[1]), H1 = lr_pk(hf[2], hf[3]), H2 = lr_pk(hf[4], hf[5]), H3 = lr_pk(hf[6], 0);
  const int q4 = bw / 4;
  const float inv_q4 = 1.0f / (float)q4;
  for (int i = threadIdx.x; i < (bh + 6) * q4; i += 256) {
    const int r = (int)(((float)i + 0.5f) * inv_q4), c = (i - r * q4) * 4;
    const uint2 *p = reinterpret_cast<const uint2 *>(src + __mul24(r, kLrSS) + c);   // (r * SS became a 64-bit multiply-add)
    const uint2 a = p[0], b = p[1], e = p[2];
    const uint32_t d[6] = { a.x, a.y, b.x, b.y, e.x, e.y };
    uint32_t A[6];
#pragma unroll
    for (int m = 1; m < 6; m++) A[m] = __builtin_amdgcn_alignbit(d[m], d[m - 1], 16);   // columns (c + 2m - 1, c + 2m)
    int o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      // output k: columns c + 1 + k .. c + 7 + k
      const uint32_t *w = (k & 1) ? d + (k + 1) / 2 : A + k / 2 + 1;
      int sum = 4;
      sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, w[0]), H0, sum, false);
      sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, w[1]), H1, sum, false);
      sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, w[2]), H2, sum, false);
      sum = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, w[3]), H3, sum, false);
      o[k] = min(max(sum >> 3, -offset), limit - offset);
    }
    uint2 w; w.x = (uint32_t)(o[0] & 0xffff) | ((uint32_t)o[1] << 16); w.y = (uint32_t)(o[2] & 0xffff) | ((uint32_t)o[3] << 16);
    *reinterpret_cast<uint2 *>(inter + r * kLrMaxW + c) = w;
  }
}
template <typename Pix, int BD, bool SGR> __device__ __forceinline__ void lr_wiener_packed(const LrTile<Pix> &T, LrLds<SGR> &lds, LrErr &err, const LrUnit &U) {
  const uint16_t *src = lds.src;
  int16_t *inter = lds.inter();
  const int q4 = T.bw / 4, hp = (T.bh + 1) >> 1;
  const float inv_q4 = 1.0f / (float)q4;
  lr_wiener_h_packed<BD>(src, inter, T.bw, T.bh, U.hf);
  __syncthreads();
  // Vertical: a lane produces rows 2 rp and 2 rp + 1 of four columns from intermediate rows 2 rp .. 2 rp + 7, interleaved once into
  // row pairs per column; the even row pairs its taps (v0,v1) (v2,v3) (v4,v5) (v6,0), the odd row the same row pairs with the taps
  // moved up by one row: (0,v0) (v1,v2) (v3,v4) (v5,v6).
  const s16x2 VE[4] = { lr_pk(U.vf[0], U.vf[1]), lr_pk(U.vf[2], U.vf[3]), lr_pk(U.vf[4], U.vf[5]), lr_pk(U.vf[6], 0) };
  const s16x2 VO[4] = { lr_pk(0, U.vf[0]), lr_pk(U.vf[1], U.vf[2]), lr_pk(U.vf[3], U.vf[4]), lr_pk(U.vf[5], U.vf[6]) };
  for (int i = threadIdx.x; i < hp * q4; i += 256) {
    const int rp = (int)(((float)i + 0.5f) * inv_q4), c = (i - rp * q4) * 4, r = 2 * rp;
    int se[4] = { 1024, 1024, 1024, 1024 }, so[4] = { 1024, 1024, 1024, 1024 };
#pragma unroll
    for (int j = 0; j < 4; j++) {
      // rows r + 2j, r + 2j + 1 (the last pair of an odd-height block reads one row past the intermediate: inside the
      // scratch buffer, and only the odd output row, which is not stored then, depends on it)
      const uint2 x = *reinterpret_cast<const uint2 *>(inter + (r + 2 * j) * kLrMaxW + c);
      const uint2 y = *reinterpret_cast<const uint2 *>(inter + (r + 2 * j + 1) * kLrMaxW + c);
      const uint32_t pr[4] = { __builtin_amdgcn_perm(y.x, x.x, 0x05040100u), __builtin_amdgcn_perm(y.x, x.x, 0x07060302u),
                               __builtin_amdgcn_perm(y.y, x.y, 0x05040100u), __builtin_amdgcn_perm(y.y, x.y, 0x07060302u) };
#pragma unroll
      for (int k = 0; k < 4; k++) {
        se[k] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, pr[k]), VE[j], se[k], false);
        so[k] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, pr[k]), VO[j], so[k], false);
      }
    }
#pragma unroll
    for (int half = 0; half < 2; half++) {
      if (r + half >= T.bh) break;
      int o[4];
#pragma unroll
      for (int k = 0; k < 4; k++) o[k] = min(max((half ? so[k] : se[k]) >> 11, 0), (1 << BD) - 1);
      lr_put4(T, src, err, r + half, c, o);
    }
  }
}
// the scalar route: any width
template <int BD> __device__ __forceinline__ void lr_wiener_h_scalar(const uint16_t *src, int16_t *inter, int bw, int bh, const int (&hf)[7]) {
  constexpr int offset = 1 << (BD + 3), limit = (1 << (BD + 5)) - 1;
  for (int i = threadIdx.x; i < (bh + 6) * bw; i += 256) {
    const int r = i / bw, c = i - r * bw;
    const uint16_t *p = src + r * kLrSS + c + 1;
    int sum = 0;
#pragma unroll
    for (int t = 0; t < 7; t++) sum += hf[t] * p[t];
    inter[r * kLrMaxW + c] = (int16_t)min(max((sum + 4) >> 3, -offset), limit - offset);
  }
}
template <typename Pix, int BD, bool SGR> __device__ __forceinline__ void lr_wiener_scalar(const LrTile<Pix> &T, LrLds<SGR> &lds, LrErr &err, const LrUnit &U) {
  const int tid = threadIdx.x, bw = T.bw, bh = T.bh;
  int16_t *inter = lds.inter();
  lr_wiener_h_scalar<BD>(lds.src, inter, bw, bh, U.hf);
  __syncthreads();
  for (int i = tid; i < bh * bw; i += 256) {
    const int r = i / bw, c = i - r * bw;
    int sum = 0;
#pragma unroll
    for (int t = 0; t < 7; t++) sum += U.vf[t] * inter[(r + t) * kLrMaxW + c];
    lr_put1(T, err, r, c, min(max((sum + 1024) >> 11, 0), (1 << BD) - 1), lds.src[(r + 3) * kLrSS + c + 4]);
  }
}

// ---- The restoration search (av1mi.h "restoration search"): the squared error of every candidate over one staged tile against the
// source, nothing stored.  A candidate above 0 is a (vertical, horizontal) pair of the plane class's three 1-D filters: pair (v, h) is
// candidate 3 v + h.  Pair (0, 0) would be the identity; its place, candidate 0, holds "none": the CDEF samples' own error.
// One horizontal pass per horizontal filter (lr_wiener_h_packed / _scalar), then ONE vertical pass that runs the vertical filters
// over the same loads of the intermediate, into error sums only.  Per lane the sums are 32 bits: at most 16 samples x 2^20.
constexpr int kLrFilters = 3, kLrCands = 9;
struct LrSearchTaps { int f[kLrFilters][7]; };      // the symmetric 7-tap form of the class's filters
__device__ __forceinline__ LrSearchTaps lr_search_taps(const int8_t (&t)[kLrFilters][3]) {
  LrSearchTaps F;
#pragma unroll
  for (int k = 0; k < kLrFilters; k++) {
#pragma unroll
    for (int i = 0; i < 3; i++) F.f[k][i] = F.f[k][6 - i] = t[k][i];
    F.f[k][3] = 128 - 2 * (t[k][0] + t[k][1] + t[k][2]);
  }
  return F;
}
// The packed route's source samples, loaded once and kept for the three vertical passes: item i = tid + 256 k of the vertical pass
// (k < 2: a tile has at most 32 row pairs x 16 column groups) is rows 2 rp, 2 rp + 1 of four columns; sv[k][half] = those four samples
// of the source as 16-bit halves, where the row exists
template <typename Pix> __device__ __forceinline__ void lr_search_source(const LrTile<Pix> &T, uint2 (&sv)[2][2]) {
  typedef Pix Pix4 __attribute__((ext_vector_type(4)));
  const int q4 = T.bw / 4, hp = (T.bh + 1) >> 1;
  const float inv_q4 = 1.0f / (float)q4;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int i = threadIdx.x + 256 * k;
#pragma unroll
    for (int half = 0; half < 2; half++) {
      sv[k][half] = make_uint2(0, 0);
      if (i >= hp * q4) continue;
      const int rp = (int)(((float)i + 0.5f) * inv_q4), c = (i - rp * q4) * 4, r = 2 * rp + half;
      if (r >= T.bh) continue;
      const Pix *sp = T.orig + T.at(r, c);
      Pix4 v;
      if (((uintptr_t)sp & (sizeof(Pix4) - 1)) == 0) v = *reinterpret_cast<const Pix4 *>(sp);
      else v = Pix4{ sp[0], sp[1], sp[2], sp[3] };
      sv[k][half] = make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
    }
  }
}
__device__ __forceinline__ int lr_search_sample(const uint2 &s, int k) { return (int)(((k & 2) ? s.y : s.x) >> ((k & 1) * 16) & 0xffffu); }
// candidate 0 over the lane's items: the staged CDEF samples against the source
__device__ __forceinline__ unsigned lr_search_none_packed(const uint16_t *src, int bw, int bh, const uint2 (&sv)[2][2]) {
  const int q4 = bw / 4, hp = (bh + 1) >> 1;
  const float inv_q4 = 1.0f / (float)q4;
  unsigned e = 0;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int i = threadIdx.x + 256 * k;
    if (i >= hp * q4) continue;
    const int rp = (int)(((float)i + 0.5f) * inv_q4), c = (i - rp * q4) * 4;
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const int r = 2 * rp + half;
      if (r >= bh) continue;
      const uint2 cd = *reinterpret_cast<const uint2 *>(src + (r + 3) * kLrSS + c + 4);
#pragma unroll
      for (int m = 0; m < 4; m++) { const int d = lr_search_sample(cd, m) - lr_search_sample(sv[k][half], m); e += (unsigned)(d * d); }
    }
  }
  return e;
}
// The vertical pass of the search, packed: lr_wiener_packed's row pairs and tap pairs, the vertical filters FIRST .. 2 over one set of
// loads, err[v] += the squared error of filter v's output.  (The last pair of an odd-height block: see lr_wiener_packed; its odd row
// is not counted.)
template <int BD, int FIRST> __device__ __forceinline__ void lr_search_v_packed(const int16_t *inter, int bw, int bh, const LrSearchTaps &F, const uint2 (&sv)[2][2],
                                                                               unsigned (&err)[kLrFilters]) {
  const int q4 = bw / 4, hp = (bh + 1) >> 1;
  const float inv_q4 = 1.0f / (float)q4;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int i = threadIdx.x + 256 * k;
    if (i >= hp * q4) continue;
    const int rp = (int)(((float)i + 0.5f) * inv_q4), c = (i - rp * q4) * 4, r = 2 * rp;
    uint32_t pr[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint2 x = *reinterpret_cast<const uint2 *>(inter + (r + 2 * j) * kLrMaxW + c);
      const uint2 y = *reinterpret_cast<const uint2 *>(inter + (r + 2 * j + 1) * kLrMaxW + c);
      pr[j][0] = __builtin_amdgcn_perm(y.x, x.x, 0x05040100u); pr[j][1] = __builtin_amdgcn_perm(y.x, x.x, 0x07060302u);
      pr[j][2] = __builtin_amdgcn_perm(y.y, x.y, 0x05040100u); pr[j][3] = __builtin_amdgcn_perm(y.y, x.y, 0x07060302u);
    }
#pragma unroll
    for (int v = FIRST; v < kLrFilters; v++) {
      const int (&vf)[7] = F.f[v];
      const s16x2 VE[4] = { lr_pk(vf[0], vf[1]), lr_pk(vf[2], vf[3]), lr_pk(vf[4], vf[5]), lr_pk(vf[6], 0) };
      const s16x2 VO[4] = { lr_pk(0, vf[0]), lr_pk(vf[1], vf[2]), lr_pk(vf[3], vf[4]), lr_pk(vf[5], vf[6]) };
      int se[4] = { 1024, 1024, 1024, 1024 }, so[4] = { 1024, 1024, 1024, 1024 };
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int m = 0; m < 4; m++) {
          se[m] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, pr[j][m]), VE[j], se[m], false);
          so[m] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, pr[j][m]), VO[j], so[m], false);
        }
#pragma unroll
      for (int half = 0; half < 2; half++) {
        if (r + half >= bh) continue;
#pragma unroll
        for (int m = 0; m < 4; m++) {
          const int d = min(max((half ? so[m] : se[m]) >> 11, 0), (1 << BD) - 1) - lr_search_sample(sv[k][half], m);
          err[v] += (unsigned)(d * d);
        }
      }
    }
  }
}
// ... and the scalar route, any width: the source sample by sample from memory
template <typename Pix> __device__ __forceinline__ unsigned lr_search_none_scalar(const LrTile<Pix> &T, const uint16_t *src) {
  unsigned e = 0;
  for (int i = threadIdx.x; i < T.bh * T.bw; i += 256) {
    const int r = i / T.bw, c = i - r * T.bw, d = (int)src[(r + 3) * kLrSS + c + 4] - (int)T.orig[T.at(r, c)];
    e += (unsigned)(d * d);
  }
  return e;
}
template <typename Pix, int BD, int FIRST> __device__ __forceinline__ void lr_search_v_scalar(const LrTile<Pix> &T, const int16_t *inter, const LrSearchTaps &F,
                                                                                             unsigned (&err)[kLrFilters]) {
  for (int i = threadIdx.x; i < T.bh * T.bw; i += 256) {
    const int r = i / T.bw, c = i - r * T.bw, sv = T.orig[T.at(r, c)];
    int x[7];
#pragma unroll
    for (int t = 0; t < 7; t++) x[t] = inter[(r + t) * kLrMaxW + c];
#pragma unroll
    for (int v = FIRST; v < kLrFilters; v++) {
      int sum = 0;
#pragma unroll
      for (int t = 0; t < 7; t++) sum += F.f[v][t] * x[t];
      const int d = min(max((sum + 1024) >> 11, 0), (1 << BD) - 1) - sv;
      err[v] += (unsigned)(d * d);
    }
  }
}
// The workgroup's nine sums into the unit's entry of the cost table: per wave in 32 bits (64 lanes x 2^24), the four waves and the
// tiles of a unit in 64 — integer adds, so the table does not depend on the order the tiles finish in.  Uses the intermediate's LDS,
// which every lane has left (the barrier).
__device__ __forceinline__ void lr_search_finish(LrLds<false> &lds, const unsigned (&err)[kLrCands], unsigned long long *dst) {
  const int tid = threadIdx.x;
  unsigned *red = reinterpret_cast<unsigned *>(lds.scratch);      // [candidate][wave]
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kLrCands; c++) {
    unsigned a = err[c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_down(a, d, 64);
    if ((tid & 63) == 0) red[c * 4 + (tid >> 6)] = a;
  }
  __syncthreads();
  if (tid < kLrCands) atomicAdd(dst + tid, (unsigned long long)red[tid * 4] + red[tid * 4 + 1] + red[tid * 4 + 2] + red[tid * 4 + 3]);
}

// Self-guided (spec 7.17.3): box sums (r = 2 on odd rows, then r = 1) -> A (u16) / B (i32) in LDS -> 3x3 weighted a*x + b, both
// passes kept in registers, projection with (w0, w1, 128 - w0 - w1).
// The box sums of one pass: A/B at local (i, j) for i in -1..bh, j in -1..bw; stored at [(i+1) * kLrAS + (j+1)]
template <int BD> __device__ __forceinline__ void lr_sgr_box(const uint16_t *src, uint16_t *Abuf, int32_t *Bbuf, int bw, int bh, int y0, int pass, int r, int eps) {
  const unsigned n = (2 * r + 1) * (2 * r + 1), n2e = n * n * (unsigned)eps;
  const unsigned sfac = ((1u << 20) + n2e / 2) / n2e, one_by_n = ((1u << 12) + n / 2) / n;
  for (int q = threadIdx.x; q < (bh + 2) * (bw + 2); q += 256) {
    const int i = q / (bw + 2) - 1, j = q % (bw + 2) - 1;
    if (pass == 0 && !((y0 + i) & 1)) continue;            // the r = 2 pass only ever reads odd rows
    const uint16_t *p = src + (i + 3) * kLrSS + (j + 4);
    unsigned a = 0, b = 0;
    for (int dy = -r; dy <= r; dy++)
      for (int dx = -r; dx <= r; dx++) { const unsigned v = p[dy * kLrSS + dx]; a += v * v; b += v; }
    const unsigned as = BD == 8 ? a : (a + 8) >> 4, d = BD == 8 ? b : (b + 2) >> 2;
    const unsigned pv = as * n > d * d ? as * n - d * d : 0;
    const unsigned z = (unsigned)(((unsigned long long)pv * sfac + (1u << 19)) >> 20);
    const unsigned a2 = z >= 255 ? 256 : z == 0 ? 1 : ((z << 8) + z / 2) / (z + 1);
    Abuf[(i + 1) * kLrAS + j + 1] = (uint16_t)a2;
    Bbuf[(i + 1) * kLrAS + j + 1] = (int32_t)(((256 - a2) * b * one_by_n + (1u << 11)) >> 12);
  }
}
// the weighted 3x3 sum of A and B around sample (i, j) of the block, applied to the sample x
__device__ __forceinline__ int lr_sgr_weighted(const uint16_t *Abuf, const int32_t *Bbuf, int i, int j, bool odd_row, int pass, int x) {
  constexpr int AS = kLrAS;
  auto sum = [&](auto *p) -> int {      // one plane's weights: r = 2 has values on odd rows only
    p += (i + 1) * AS + j + 1;
    if (pass != 0) return 4 * (p[0] + p[-1] + p[1] + p[-AS] + p[AS]) + 3 * (p[-AS - 1] + p[-AS + 1] + p[AS - 1] + p[AS + 1]);
    if (odd_row) return 6 * p[0] + 5 * (p[-1] + p[1]);
    return 6 * (p[-AS] + p[AS]) + 5 * (p[-AS - 1] + p[-AS + 1] + p[AS - 1] + p[AS + 1]);
  };
  const int shift = pass == 0 && odd_row ? 4 : 5;
  return (sum(Abuf) * x + sum(Bbuf) + (1 << (shift + 3))) >> (shift + 4);   // Round2(v, SGR_BITS 8 + shift - RST_BITS 4)
}
template <typename Pix, int BD> __device__ __forceinline__ void lr_sgr(const LrTile<Pix> &T, LrLds<true> &lds, LrErr &err, const LrUnit &U) {
  const int tid = threadIdx.x, bw = T.bw, bh = T.bh, set = U.set, w2 = 128 - U.w0 - U.w1;
  const uint16_t *src = lds.src;
  int flt[2][16];   // this lane's samples: index k <-> sample tid + 256 k of the block (row-major)
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    const int r = kSgrParams[set][2 * pass];
    if (r == 0) continue;   // uniform across the workgroup
    lr_sgr_box<BD>(src, lds.A(), lds.B(), bw, bh, T.y0, pass, r, kSgrParams[set][2 * pass + 1]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int q = tid + 256 * k;
      if (q >= bh * bw) continue;
      const int i = q / bw, j = q - i * bw;
      flt[pass][k] = lr_sgr_weighted(lds.A(), lds.B(), i, j, (T.y0 + i) & 1, pass, src[(i + 3) * kLrSS + j + 4]);
    }
    __syncthreads();
  }
  const int r0 = kSgrParams[set][0], r1 = kSgrParams[set][2];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int q = tid + 256 * k;
    if (q >= bh * bw) continue;
    const int i = q / bw, j = q - i * bw;
    const int x = src[(i + 3) * kLrSS + j + 4], u = x << 4;
    int v = U.w1 * u;
    v += U.w0 * (r0 ? flt[0][k] : u);
    v += w2 * (r1 ? flt[1][k] : u);
    lr_put1(T, err, i, j, min(max((v + 1024) >> 11, 0), (1 << BD) - 1), x);
  }
}

}  // namespace av1mi
