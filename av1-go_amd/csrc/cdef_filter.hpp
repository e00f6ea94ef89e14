// cdef_filter.hpp — CDEF (AV1 spec §7.15) of one 64x64 luma superblock and its two 32x32 chroma blocks on tiles staged in LDS: the
// direction search, the tap tables, the packed filter, and the filter items of a 256-lane workgroup with a sink for their output.
// Shared by k_cdef (cdef_kernel.hip: deblocked planes from HBM), k_deblock_cdef (deblock_cdef_kernel.hip: the tile deblocked in
// place) and k_cdef_search (cdef_search_kernel.hip: squared error against the source per candidate strength set), so all three run
// the same source.  A tile holds 0xFFFF where a sample lies outside the picture.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "av1mi_internal.hpp"

namespace av1mi {

__device__ constexpr int8_t kCdefDir[8][2][2] = {
  { { -1, 1 }, { -2, 2 } }, { { 0, 1 }, { -1, 2 } }, { { 0, 1 }, { 0, 2 } }, { { 0, 1 }, { 1, 2 } },
  { { 1, 1 }, { 2, 2 } },   { { 1, 0 }, { 2, 1 } },  { { 1, 0 }, { 2, 0 } }, { { 1, 0 }, { 2, -1 } } };

__device__ __forceinline__ int msb(unsigned v) { return 31 - __clz(v); }
// Four horizontally adjacent samples at once with packed 16-bit VALU (v_pk_*_i16: two samples per lane-op).  SENT = the
// tile may hold 0xFFFF "outside the picture" marks (picture-border superblocks): two more ops per tap pair.
// p: 4-byte aligned centre pointer (first of the four samples) in an LDS tile with even row stride LS.
typedef short v2s __attribute__((ext_vector_type(2)));
typedef unsigned short v2u __attribute__((ext_vector_type(2)));
// constrain() on two samples: clamp(diff, -t, t) with t = max(0, thr - (|diff| >> shift)) — the same value as
// sign(diff) * min(|diff|, t) (spec 7.15.2), written so that it is a saturating subtract and a min/max pair
__device__ __forceinline__ v2s pk_constrain(v2s diff, v2u thr, v2u shift) {
  const v2u mag = __builtin_bit_cast(v2u, __builtin_elementwise_max(diff, -diff));
  const v2s t = __builtin_bit_cast(v2s, __builtin_elementwise_sub_sat(thr, mag >> shift));
  return __builtin_elementwise_max(__builtin_elementwise_min(diff, t), -t);
}
// Tap table of one direction in a tile of row stride LS, ready to use: for each of the six tap positions j (primary k = 0, 1;
// secondary dir + 2, k = 0, 1; secondary dir + 6, k = 0, 1) three int32: the BYTE offset of the aligned dword pair that holds
// the four samples at +offset, the same for the mirrored tap at -offset, and the funnel shift (16 when the offset is odd).
// A quad reads its direction's 18 entries with five LDS loads and adds them to its centre address; derived per quad from
// int16 sample offsets this was ~45 of the ~450 instructions of a quad.
constexpr int kTapEntries = 20;   // 18 used, row padded to a multiple of 4 dwords
template <int LS> __device__ __forceinline__ void cdef_fill_offsets(int32_t *tab, int i) {   // i in [0, 8 * 6)
  const int dir = i / 6, j = i - dir * 6;
  const int d = j < 2 ? dir : j < 4 ? (dir + 2) & 7 : (dir + 6) & 7, k = j & 1;
  const int o = kCdefDir[d][k][0] * LS + kCdefDir[d][k][1], odd = o & 1;
  tab[dir * kTapEntries + 3 * j] = 2 * (o - odd);
  tab[dir * kTapEntries + 3 * j + 1] = 2 * (-o - odd);
  tab[dir * kTapEntries + 3 * j + 2] = odd * 16;
}
// pshift / sshift: max(0, damping - msb(strength)) (0 for strength 0); pt0, pt1: the primary tap weights (4, 2) or (3, 3)
template <bool SENT>
__device__ __forceinline__ void cdef_quad_packed(const uint16_t *p, const int32_t *otab, int pri, int sec, int pshift, int sshift, int pt0, int pt1, v2s *out) {
  const uint32_t *c32 = reinterpret_cast<const uint32_t *>(p);
  const v2s x0 = __builtin_bit_cast(v2s, c32[0]), x1 = __builtin_bit_cast(v2s, c32[1]);
  v2s s0 = { 0, 0 }, s1 = { 0, 0 }, mx0 = x0, mx1 = x1, mn0 = x0, mn1 = x1;
  int ot[kTapEntries];
#pragma unroll
  for (int i = 0; i < kTapEntries; i += 4) {
    const int4 v = *reinterpret_cast<const int4 *>(otab + i);
    ot[i] = v.x; ot[i + 1] = v.y; ot[i + 2] = v.z; ot[i + 3] = v.w;
  }
  // one tap position and its mirror image share weight and strength: constrain both, add, one multiply-add per pair
  auto taps = [&](int j, int thr, int shift, int w) {
    const v2u th = { (unsigned short)thr, (unsigned short)thr }, sh = { (unsigned short)shift, (unsigned short)shift };
    v2s c0 = { 0, 0 }, c1 = { 0, 0 };
#pragma unroll
    for (int sg = 0; sg < 2; sg++) {
      // the four samples at p +- offset .. + 3 as two packed pairs; the offset may be odd: funnel-shift three aligned dwords
      const uint32_t *q = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(p) + ot[3 * j + sg]);
      const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
      v2s a0 = __builtin_bit_cast(v2s, __builtin_amdgcn_alignbit(d1, d0, ot[3 * j + 2]));
      v2s a1 = __builtin_bit_cast(v2s, __builtin_amdgcn_alignbit(d2, d1, ot[3 * j + 2]));
      if constexpr (SENT) {
        // picture-border superblocks: 0xFFFF marks a sample outside the picture (CdefAvailable = 0).  Valid samples are
        // < 2^15, so the sign bit is the mark; a marked tap is replaced by the centre sample: difference 0, and it cannot
        // move the min/max clamp — exactly "skip the tap"
        // (the sign splat goes through inline asm: written as a0 >> 15 the compiler recognises a per-element select and emits
        // a compare + v_cndmask per HALF, six instructions per pair instead of shift + v_bfi)
        uint32_t m0, m1;
        asm("v_pk_ashrrev_i16 %0, 15, %1 op_sel_hi:[0,1]" : "=v"(m0) : "v"(__builtin_bit_cast(uint32_t, a0)));
        asm("v_pk_ashrrev_i16 %0, 15, %1 op_sel_hi:[0,1]" : "=v"(m1) : "v"(__builtin_bit_cast(uint32_t, a1)));
        a0 = __builtin_bit_cast(v2s, (__builtin_bit_cast(uint32_t, x0) & m0) | (__builtin_bit_cast(uint32_t, a0) & ~m0));
        a1 = __builtin_bit_cast(v2s, (__builtin_bit_cast(uint32_t, x1) & m1) | (__builtin_bit_cast(uint32_t, a1) & ~m1));
      }
      c0 += pk_constrain(a0 - x0, th, sh); c1 += pk_constrain(a1 - x1, th, sh);
      mx0 = __builtin_elementwise_max(mx0, a0); mx1 = __builtin_elementwise_max(mx1, a1);
      mn0 = __builtin_elementwise_min(mn0, a0); mn1 = __builtin_elementwise_min(mn1, a1);
    }
    const v2s ww = { (short)w, (short)w };
    s0 += ww * c0; s1 += ww * c1;
  };
  // secondary strength 0 (uniform in a superblock; the policy's value for inter frames at mid quantisers): its eight taps
  // contribute nothing to the sum, and without them the result lies between the centre and a primary tap, so that they do not
  // take part in the min / max clamp changes nothing either (libaom's cdef_filter_8_1 drops the clamp altogether)
  if (sec) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      taps(k, pri, pshift, k ? pt1 : pt0);
      taps(2 + k, sec, sshift, k ? 1 : 2);
      taps(4 + k, sec, sshift, k ? 1 : 2);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 2; k++) taps(k, pri, pshift, k ? pt1 : pt0);
  }
  const v2s eight = { 8, 8 }, four = { 4, 4 }, fifteen = { 15, 15 };
  const v2s y0 = x0 + ((s0 + (s0 >> fifteen) + eight) >> four), y1 = x1 + ((s1 + (s1 >> fifteen) + eight) >> four);
  out[0] = __builtin_elementwise_min(__builtin_elementwise_max(y0, mn0), mx0);
  out[1] = __builtin_elementwise_min(__builtin_elementwise_max(y1, mn1), mx1);
}

// What the superblock's strength set { y_pri, y_sec, uv_pri, uv_sec } and the damping give on their own (uniform in the workgroup)
struct CdefSb {
  bool enabled;
  int ypri0, ysec, upri, usec, dampy, dampc;
  int ysshift, usshift, upshift, upar;
};
__device__ __forceinline__ CdefSb cdef_sb_params(uint32_t st32, int damping, int cs) {
  const int st[4] = { (int)(st32 & 255), (int)((st32 >> 8) & 255), (int)((st32 >> 16) & 255), (int)(st32 >> 24) };
  CdefSb s;
  s.enabled = st[0] != 255;
  s.ypri0 = st[0] << cs; s.ysec = (st[1] == 3 ? 4 : st[1]) << cs;
  s.upri = st[2] << cs; s.usec = (st[3] == 3 ? 4 : st[3]) << cs;
  s.dampy = damping + cs; s.dampc = damping + cs - 1;
  s.ysshift = s.ysec ? max(0, s.dampy - msb((unsigned)s.ysec)) : 0; s.usshift = s.usec ? max(0, s.dampc - msb((unsigned)s.usec)) : 0;
  s.upshift = s.upri ? max(0, s.dampc - msb((unsigned)s.upri)) : 0; s.upar = (s.upri >> cs) & 1;
  return s;
}

// Direction search of the 8x8 luma block at p (rows YS apart), every bin index a compile-time constant: the block's direction
// (bits 0-2) and its variance (from bit 3).  Neither depends on the strengths, so the CDEF search runs this once per block for all of
// its candidate sets; cdef_block_pack adds what a strength set makes of them.
template <int YS> __device__ __forceinline__ uint32_t cdef_block_dirvar(const uint16_t *p, int cs) {
  // squares of sums of at most 8 values in [-128, 127] (<= 2^20) times weights <= 840: 24-bit multiplies (a 32-bit integer
  // multiply is four passes)
  constexpr int div_table[9] = { 0, 840, 420, 280, 210, 168, 140, 120, 105 };
  // (pinned by inline asm: the compiler, which can bound the sums, turned __mul24(v, v) back into v_mul_lo_u32 / v_mad_u64_u32)
  auto sq = [](int v) { int d; asm("v_mul_i32_i24 %0, %1, %1" : "=v"(d) : "v"(v)); return d; };
  auto cost_diag = [&](const int (&s)[15]) {      // directions 0 and 4: 15 lines of 1 .. 8 .. 1 samples
    int c = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) c += (int)__umul24((unsigned)(sq(s[i]) + sq(s[14 - i])), (unsigned)div_table[i + 1]);
    return c + (int)__umul24((unsigned)sq(s[7]), 105u);
  };
  auto cost_straight = [&](const int (&s)[8]) {   // directions 2 and 6: 8 lines of 8 samples
    int c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) c += sq(s[i]);
    return (int)__umul24((unsigned)c, 105u);
  };
  auto cost_skew = [&](const int (&s)[11]) {      // the odd directions: 11 lines of 2, 4, 6, 8 x 5, 6, 4, 2 samples
    int c = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) c += sq(s[3 + j]);
    c = (int)__umul24((unsigned)c, 105u);
#pragma unroll
    for (int j = 0; j < 3; j++) c += (int)__umul24((unsigned)(sq(s[j]) + sq(s[10 - j])), (unsigned)div_table[2 * j + 2]);
    return c;
  };
  // The line sums of four directions at a time: 45 accumulators.  All eight in one walk over the block are 90 live values beside
  // the addresses, more than the 96 registers of five waves per SIMD hold, and the surplus went to scratch memory; the second
  // walk costs 64 more LDS reads per block.  (The sums are integers: the order of the additions changes nothing.)
  int cost[8];
#pragma unroll
  for (int half = 0; half < 2; half++) {
    int diag[15], skew_a[11], straight[8], skew_b[11];
#pragma unroll
    for (int k = 0; k < 15; k++) diag[k] = 0;
#pragma unroll
    for (int k = 0; k < 11; k++) skew_a[k] = skew_b[k] = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) straight[k] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int x = (p[i * YS + j] >> cs) - 128;
        if (half == 0) { diag[i + j] += x; skew_a[i + j / 2] += x; straight[i] += x; skew_b[3 + i - j / 2] += x; }          // directions 0, 1, 2, 3
        else { diag[7 + i - j] += x; skew_a[3 - i / 2 + j] += x; straight[j] += x; skew_b[i / 2 + j] += x; }                // directions 4, 5, 6, 7
      }
    cost[4 * half] = cost_diag(diag); cost[4 * half + 1] = cost_skew(skew_a); cost[4 * half + 2] = cost_straight(straight); cost[4 * half + 3] = cost_skew(skew_b);
    if (half == 0) asm volatile("" ::: "memory");   // keeps the second walk's loads behind the first half's sums
  }
  int best = 0, best_cost = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) if (cost[i] > best_cost) { best_cost = cost[i]; best = i; }
  int opp = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) if (i == ((best + 4) & 7)) opp = cost[i];
  return (uint32_t)best | ((uint32_t)((best_cost - opp) >> 10) << 3);
}
// Everything a quad of the block needs, once per block instead of once per quad (16 luma + 8 chroma quads per block): luma primary
// strength after the variance adjustment (bits 0-7), its damping shift (8-11), the luma filter direction (12-14), the primary tap
// parity (15), the block's direction itself (16-18: chroma)
__device__ __forceinline__ uint32_t cdef_block_pack(uint32_t dirvar, int cs, int ypri0, int dampy) {
  const int best = (int)(dirvar & 7), var = (int)(dirvar >> 3);
  const int vs = (var >> 6) ? min(msb((unsigned)(var >> 6)), 12) : 0;
  const int pri = var ? (ypri0 * (4 + vs) + 8) >> 4 : 0;             // spec 7.15.2: luma primary strength adjusted by the variance
  const int pshift = pri ? max(0, dampy - msb((unsigned)pri)) : 0;
  const int ydir = ypri0 == 0 ? 0 : best;
  return (uint32_t)pri | ((uint32_t)pshift << 8) | ((uint32_t)ydir << 12) | ((uint32_t)((pri >> cs) & 1) << 15) | ((uint32_t)best << 16);
}
template <int YS> __device__ __forceinline__ uint32_t cdef_block_params(const uint16_t *p, int cs, int ypri0, int dampy) {
  return cdef_block_pack(cdef_block_dirvar<YS>(p, cs), cs, ypri0, dampy);
}

template <typename Pix> __device__ __forceinline__ void cdef_store4(Pix *d, const int (&o)[4]) {
  if constexpr (sizeof(Pix) == 1) *reinterpret_cast<uint32_t *>(d) = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
  else { uint2 u; u.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16); u.y = (uint32_t)o[2] | ((uint32_t)o[3] << 16); *reinterpret_cast<uint2 *>(d) = u; }
}

// THE FILTER, stated once: item q of a 256-lane workgroup's superblock is four horizontally adjacent samples, and what becomes of the
// four filtered samples is the SINK's business — k_cdef and k_deblock_cdef store them to the output planes (CdefStore), k_cdef_search
// adds their squared difference to the source into a register.  ty0 / tu0, tv0: the tile sample of the block's top-left corner (4-byte
// aligned, rows YS / CS apart, both even); (sbx, sby): the superblock; w, h: the luma picture.  interior: the tiles hold no 0xFFFF
// mark.  bskip: skip flag of each 8x8 block of the superblock (1 also for blocks outside the picture); bpar: see cdef_block_pack;
// offy / offc: the tap tables of the two tile strides (cdef_fill_offsets).  An item outside the picture reaches no sink.
// luma 64x64: q in [0, 64 * 16) -> (row, group of 4 columns); sink(fy, fx, o)
template <int YS, class Sink>
__device__ __forceinline__ void cdef_luma_item(int q, const uint16_t *ty0, int sbx, int sby, int w, int h, const CdefSb &S, bool interior,
                                               const uint8_t *bskip, const uint32_t *bpar, const int32_t *offy, Sink &&sink) {
  const int r = q >> 4, c = (q & 15) * 4;
  const int fy = sby * 64 + r, fx = sbx * 64 + c;
  if (fy >= h || fx >= w) return;
  const int b = (r >> 3) * 8 + (c >> 3);
  const bool skip = !S.enabled || bskip[b];
  const uint16_t *p = ty0 + r * YS + c;
  int o[4];
  if (skip) { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3]; }
  else {
    const uint32_t bp = bpar[b];
    const int pri = bp & 255, pshift = (bp >> 8) & 15, par = (bp >> 15) & 1;
    const int32_t *ot = offy + ((bp >> 12) & 7) * kTapEntries;
    v2s r[2];
    if (interior) cdef_quad_packed<false>(p, ot, pri, S.ysec, pshift, S.ysshift, par ? 3 : 4, par ? 3 : 2, r);
    else cdef_quad_packed<true>(p, ot, pri, S.ysec, pshift, S.ysshift, par ? 3 : 4, par ? 3 : 2, r);
    o[0] = r[0].x; o[1] = r[0].y; o[2] = r[1].x; o[3] = r[1].y;
  }
  sink(fy, fx, o);
}
// chroma 2 x 32x32: q in [0, 2 * 32 * 8) -> (plane, row, group of 4 columns); sink(pl, fy, fx, o)
template <int CS, class Sink>
__device__ __forceinline__ void cdef_chroma_item(int q, const uint16_t *tu0, const uint16_t *tv0, int sbx, int sby, int w, int h, const CdefSb &S, bool interior,
                                                 const uint8_t *bskip, const uint32_t *bpar, const int32_t *offc, Sink &&sink) {
  const int cw = w / 2, chh = h / 2;
  const int pl = q >> 8, r = (q >> 3) & 31, c = (q & 7) * 4;
  const int fy = sby * 32 + r, fx = sbx * 32 + c;
  if (fy >= chh || fx >= cw) return;
  const int b = (r >> 2) * 8 + (c >> 2);
  const bool skip = !S.enabled || bskip[b];
  const uint16_t *p = (pl ? tv0 : tu0) + r * CS + c;
  int o[4];
  if (skip) { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3]; }
  else {
    const int32_t *ot = offc + (S.upri == 0 ? 0 : (int)((bpar[b] >> 16) & 7)) * kTapEntries;
    v2s r[2];
    if (interior) cdef_quad_packed<false>(p, ot, S.upri, S.usec, S.upshift, S.usshift, S.upar ? 3 : 4, S.upar ? 3 : 2, r);
    else cdef_quad_packed<true>(p, ot, S.upri, S.usec, S.upshift, S.usshift, S.upar ? 3 : 4, S.upar ? 3 : 2, r);
    o[0] = r[0].x; o[1] = r[0].y; o[2] = r[1].x; o[3] = r[1].y;
  }
  sink(pl, fy, fx, o);
}

// The filter loops of the two kernels that store: dy / du, dv: frame f's output planes.
// luma 64x64 -> 16 samples per lane (4 rows x 4 columns)
template <typename Pix, int YS>
__device__ __forceinline__ void cdef_filter_luma(const uint16_t *ty0, Pix *dy, int stride_y, int sbx, int sby, int w, int h, const CdefSb &S, bool interior,
                                                 const uint8_t *bskip, const uint32_t *bpar, const int32_t *offy, int tid) {
  for (int q = tid; q < 64 * 16; q += 256)
    cdef_luma_item<YS>(q, ty0, sbx, sby, w, h, S, interior, bskip, bpar, offy,
                       [&](int fy, int fx, const int (&o)[4]) { cdef_store4<Pix>(dy + row_off(fy, stride_y) + fx, o); });
}
// chroma 2 x 32x32 -> 2 x 4 samples per lane
template <typename Pix, int CS>
__device__ __forceinline__ void cdef_filter_chroma(const uint16_t *tu0, const uint16_t *tv0, Pix *du, Pix *dv, int stride_uv, int sbx, int sby, int w, int h, const CdefSb &S,
                                                   bool interior, const uint8_t *bskip, const uint32_t *bpar, const int32_t *offc, int tid) {
  for (int q = tid; q < 2 * 32 * 8; q += 256)
    cdef_chroma_item<CS>(q, tu0, tv0, sbx, sby, w, h, S, interior, bskip, bpar, offc,
                         [&](int pl, int fy, int fx, const int (&o)[4]) { cdef_store4<Pix>((pl ? dv : du) + row_off(fy, stride_uv) + fx, o); });
}

// Staging of a superblock from whole planes in memory (k_cdef, k_cdef_search): luma 68x68 into ty (rows YS apart) and chroma 36x36 x 2
// into tc (rows CSZ apart), local (0, 0) = picture (sb * 64 - 2, sb * 64 - 2) (chroma: sb * 32 - 2); sy / su / sv: frame f's planes.
// interior: every tap of the superblock lies inside the picture; otherwise what lies outside is stored as 0xFFFF.
template <typename Pix, int YS, int CSZ, int TCN>
__device__ __forceinline__ void cdef_stage_tiles(uint16_t *ty, uint16_t (*tc)[TCN], const Pix *sy, const Pix *su, const Pix *sv, int stride_y, int stride_uv, int sbx, int sby,
                                                 int w, int h, bool interior, int tid) {
  const int cw = w / 2, chh = h / 2;
  if (interior) {
    // no bounds to check: 4-sample aligned loads starting 4 samples left of the block (18 per row luma, 10 chroma); the tile
    // keeps only the 2-sample halo, so local column = aligned column - 2.  The four samples are two uint16 pairs = two dword
    // stores: samples 0,1 go to tile columns 4g - 2, 4g - 1 and samples 2,3 to 4g, 4g + 1 (even columns, even row stride);
    // the first pair of a row and the last lie outside.  All of a lane's loads (5 luma + 3 chroma items) are issued before
    // its first LDS store, so their latencies overlap instead of adding up.
    constexpr int NY = 68 * 18, NC = 2 * 36 * 10, KY = (NY + 255) / 256, KC = (NC + 255) / 256;
    uint2 vy[KY], vc[KC];
#pragma unroll
    for (int k = 0; k < KY; k++) {
      const int i = tid + 256 * k;
      if (i < NY) {
        const int r = i / 18, g = i - r * 18;
        const Pix *q = sy + row_off(sby * 64 - 2 + r, stride_y) + sbx * 64 - 4 + g * 4;
        if constexpr (sizeof(Pix) == 1) vy[k].x = *reinterpret_cast<const uint32_t *>(q);
        else vy[k] = *reinterpret_cast<const uint2 *>(q);
      }
    }
#pragma unroll
    for (int k = 0; k < KC; k++) {
      const int i = tid + 256 * k;
      if (i < NC) {
        const int pl = i / 360, j = i - pl * 360, r = j / 10, g = j - r * 10;
        const Pix *q = (pl ? sv : su) + row_off(sby * 32 - 2 + r, stride_uv) + sbx * 32 - 4 + g * 4;
        if constexpr (sizeof(Pix) == 1) vc[k].x = *reinterpret_cast<const uint32_t *>(q);
        else vc[k] = *reinterpret_cast<const uint2 *>(q);
      }
    }
    auto pairs = [](uint2 v, uint32_t &lo, uint32_t &hi) {
      if constexpr (sizeof(Pix) == 1) { lo = __builtin_amdgcn_perm(0u, v.x, 0x0c010c00u); hi = __builtin_amdgcn_perm(0u, v.x, 0x0c030c02u); }
      else { lo = v.x; hi = v.y; }
    };
#pragma unroll
    for (int k = 0; k < KY; k++) {
      const int i = tid + 256 * k;
      if (i < NY) {
        const int r = i / 18, g = i - r * 18;
        uint32_t lo, hi;
        pairs(vy[k], lo, hi);
        uint32_t *d = reinterpret_cast<uint32_t *>(ty + r * YS + g * 4 - 2);
        if (g > 0) d[0] = lo;
        if (g < 17) d[1] = hi;
      }
    }
#pragma unroll
    for (int k = 0; k < KC; k++) {
      const int i = tid + 256 * k;
      if (i < NC) {
        const int pl = i / 360, j = i - pl * 360, r = j / 10, g = j - r * 10;
        uint32_t lo, hi;
        pairs(vc[k], lo, hi);
        uint32_t *d = reinterpret_cast<uint32_t *>(tc[pl] + r * CSZ + g * 4 - 2);
        if (g > 0) d[0] = lo;
        if (g < 9) d[1] = hi;
      }
    }
  } else {
    for (int i = tid; i < 68 * 68; i += 256) {
      const int r = i / 68, c = i - r * 68;
      const int fy = sby * 64 - 2 + r, fx = sbx * 64 - 2 + c;
      ty[r * YS + c] = (fy >= 0 && fy < h && fx >= 0 && fx < w) ? (uint16_t)sy[row_off(fy, stride_y) + fx] : (uint16_t)0xFFFF;
    }
    for (int i = tid; i < 2 * 36 * 36; i += 256) {
      const int pl = i / (36 * 36), j = i - pl * 36 * 36, r = j / 36, c = j - r * 36;
      const int fy = sby * 32 - 2 + r, fx = sbx * 32 - 2 + c;
      const Pix *sc = pl ? sv : su;
      tc[pl][r * CSZ + c] = (fy >= 0 && fy < chh && fx >= 0 && fx < cw) ? (uint16_t)sc[row_off(fy, stride_uv) + fx] : (uint16_t)0xFFFF;
    }
  }
}

}  // namespace av1mi
