// subpel.hpp — the separable sub-pel FIR of AV1 spec §7.11.3.4 (8 taps at 1/16-sample phases, rounding by 3 bits after the rows and by 11
// after the columns) as the device routines its two users share: k_mc (mc_kernels.hip, any block size and filter family) and
// k_inter_pipe (inter_kernels.hip, the candidates of the quarter-sample round and the chroma blocks).  First the pieces both are
// made of — the funnel-shifted row read, the 8-bit horizontal pass, the packing of the intermediate, the row-pair interleave — then
// the routines only k_inter_pipe uses, which filter one 8x8 or 4x4 block from a window in LDS.
// The 10-bit horizontal pass is NOT shared: k_mc takes all eight taps of any family (four v_dot2), k_inter_pipe only ever the regular
// family, whose taps 0 and 7 are zero (three v_dot2 over the x 32 table, v_perm pack); each says so where it stands.
#pragma once
#include "motion_common.hpp"

namespace av1mi {

// ND dwords of samples starting `ox` samples into the dword-aligned LDS row q: ND + 1 aligned dword reads and a funnel shift each,
// instead of a read per sample (part of the LDS diet that mc_rows7's comment tells of).  ox in [0, 4 / sizeof(ES)).
template <int ND, typename ES> __device__ __forceinline__ void row_dwords(const uint32_t *q, int ox, uint32_t *a) {
  uint32_t w[ND + 1];
#pragma unroll
  for (int i = 0; i <= ND; i++) w[i] = q[i];
#pragma unroll
  for (int i = 0; i < ND; i++) {
    if constexpr (sizeof(ES) == 1) a[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], ox);
    else a[i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], ox * 16);
  }
}

// Horizontal pass at 8 bits: CH sums of 8 taps over the CH + 7 samples in the dwords a[], rounding constant 4 included.
// 8 taps = two v_dot4_i32_i8 on the samples biased to signed bytes (p - 128), except tap 3 (it reaches 128, one more than a signed
// byte holds), which is a separate multiply-add on the unbiased sample.  The bias is paid back in the accumulator: sum over t != 3 of
// f_t * 128 = 128 * (128 - f_3).
template <int CH> __device__ __forceinline__ void fir8_u8(const uint32_t *a, const int *fx, int *sum) {
  static_assert(CH == 4 || CH == 8, "a[] holds at most four dwords, CH is a multiple of 4");
  constexpr int NA = (CH + 10) / 4;              // dwords that hold the CH + 7 samples
  uint32_t b[NA];
#pragma unroll
  for (int i = 0; i < NA; i++) b[i] = a[i] ^ 0x80808080u;
  const int F0 = (fx[0] & 255) | ((fx[1] & 255) << 8) | ((fx[2] & 255) << 16);
  const int F1 = (fx[4] & 255) | ((fx[5] & 255) << 8) | ((fx[6] & 255) << 16) | ((fx[7] & 255) << 24);
  const int acc0 = 4 + 128 * (128 - fx[3]);
  uint32_t d[CH + 4];
#pragma unroll
  for (int c = 0; c < CH + 4; c++) d[c] = (c & 3) ? __builtin_amdgcn_alignbyte(b[(c >> 2) + 1], b[c >> 2], c & 3) : b[c >> 2];
#pragma unroll
  for (int c = 0; c < CH; c++) {
    const int p3 = (int)((a[(c + 3) >> 2] >> (((c + 3) & 3) * 8)) & 255);
    sum[c] = __builtin_amdgcn_sdot4(F0, (int)d[c], __builtin_amdgcn_sdot4(F1, (int)d[c + 4], acc0 + fx[3] * p3, false), false);
  }
}

// CH horizontal sums -> CH / 2 dwords of the int16 intermediate, (s + 4) >> 3 with the 4 already in s (|value| < 2^15 for bd <= 10)
template <int CH> __device__ __forceinline__ void pack_intermediate(const int *sum, uint32_t *o) {
#pragma unroll
  for (int c = 0; c < CH; c++) {
    const uint32_t h = (uint32_t)(sum[c] >> 3) & 0xffff;
    o[c >> 1] = (c & 1) ? (o[c >> 1] | (h << 16)) : h;
  }
}

// Two rows of the intermediate, two columns a dword each, as the row pairs of the two columns: the operands of the vertical v_dot2
__device__ __forceinline__ void row_pair(uint32_t x, uint32_t y, uint32_t &lo, uint32_t &hi) {
  lo = __builtin_amdgcn_perm(y, x, 0x05040100u);   // (x.lo, y.lo)
  hi = __builtin_amdgcn_perm(y, x, 0x07060302u);   // (x.hi, y.hi)
}

// ------------------------------------------------------------------------------------------ k_inter_pipe only
// N consecutive samples starting `ox` samples into a dword-aligned LDS row
template <int N, typename ES> __device__ __forceinline__ void row_samples(const ES *row, int ox, int *v) {
  constexpr int PER = 4 / (int)sizeof(ES), ND = (N + PER - 1) / PER;
  uint32_t a[ND];
  row_dwords<ND, ES>(reinterpret_cast<const uint32_t *>(row), ox, a);
#pragma unroll
  for (int i = 0; i < N; i++) v[i] = (a[i / PER] >> ((i % PER) * 8 * (int)sizeof(ES))) & (sizeof(ES) == 1 ? 255u : 0xffffu);
}

// 2-D sub-pel prediction of row `lane` of a B x B block from a window in LDS (origin = integer position - 4, i.e. the
// window starts 4 samples left of / above the integer-vector block): posx/posy = displacement from the window's block
// origin in 1/16 samples, in [-16, 15].  im: (B+7) x B int16 scratch of the group.  Two group syncs: after the rows, after the columns.
// T0, T1: the filter family's non-zero taps are T0 .. T1 - 1 (the 4-tap families of blocks <= 4 wide: 2 .. 5; the other taps
// are exactly 0, so leaving them out changes nothing but the work: 7 intermediate rows of 4 taps instead of 11 of 8).
template <int B, typename ES, int T0 = 0, int T1 = 8>
__device__ __forceinline__ void mc_row(const ES *win, int ws, int16_t *im, int lane, int posx, int posy, const int16_t (*filt)[8], int bd,
                                       int *out) {
  const int ox = 4 + (posx >> 4) - 3, oy = 4 + (posy >> 4) - 3;   // window column / row of tap 0 of sample (0,0)
  constexpr int NT = T1 - T0, NR = B + NT - 1, PER = 4 / (int)sizeof(ES);
  int fx[NT], fy[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) { fx[t] = filt[posx & 15][T0 + t]; fy[t] = filt[posy & 15][T0 + t]; }
#pragma unroll
  for (int it = 0; it < (NR + B - 1) / B; it++) {   // intermediate rows T0 .. T0 + NR - 1 over B lanes
    const int j = T0 + lane + it * B;
    if (j < T0 + NR) {
      int v[NR];
      const int o = ox + T0;                        // first sample of the row that a non-zero tap touches
      row_samples<NR, ES>(win + (oy + j) * ws + (o & ~(PER - 1)), o & (PER - 1), v);
#pragma unroll
      for (int c = 0; c < B; c++) {
        int s = 0;
#pragma unroll
        for (int t = 0; t < NT; t++) s += fx[t] * v[c + t];
        im[j * B + c] = (int16_t)((s + 4) >> 3);
      }
    }
  }
  AV1MI_GROUP_SYNC();
  const int maxpix = (1 << bd) - 1;
#pragma unroll
  for (int c = 0; c < B; c++) {
    int s = 0;
#pragma unroll
    for (int t = 0; t < NT; t++) s += fy[t] * (int)im[(lane + T0 + t) * B + c];
    out[c] = min(max((s + 1024) >> 11, 0), maxpix);
  }
  AV1MI_GROUP_SYNC();
}

// The same filter split in two, so that the candidates of a refinement round that share a horizontal phase share its
// (more expensive) horizontal pass: mc_h16 filters all 16 rows of the luma window for one horizontal displacement,
// mc_rows7 + mc_v7 produce row `lane` of the prediction for the vertical displacements from that intermediate.
// `filt`: the regular 8-tap table at 8 bits, the same times 32 at 10.
template <typename ES>
__device__ __forceinline__ void mc_h16(const ES *win, int ws, int16_t *im, int lane, int posx, const int16_t (*filt)[8]) {
  const int ox = 4 + (posx >> 4) - 3;            // 0 or 1
  int fx[8];
  if constexpr (sizeof(ES) == 1) {
#pragma unroll
    for (int t = 0; t < 8; t++) fx[t] = filt[posx & 15][t];
  }
  constexpr int PER = 4 / (int)sizeof(ES), ND = 16 / PER;
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int j = lane + it * 8;
    uint32_t a[ND], o[4];                        // the row's 16 samples from ox on
    row_dwords<ND, ES>(reinterpret_cast<const uint32_t *>(win + j * ws), ox, a);
    if constexpr (sizeof(ES) == 1) {
      int sum[8];
      fir8_u8<8>(a, fx, sum);
      pack_intermediate<8>(sum, o);
    } else {
      // 10-bit, this kernel's own: the regular filter has SIX taps (taps 0 and 7 are 0 at every phase), so sample pairs (m, m + 1)
      // for m = 1..12 (odd m by funnel shift) against the tap pairs (t1, t2) (t3, t4) (t5, t6) are three v_dot2_i32_i16 per sample
      // where k_mc's any-family pass takes four
      uint32_t pm[13];
#pragma unroll
      for (int m = 1; m < 13; m++) pm[m] = (m & 1) ? __builtin_amdgcn_alignbit(a[(m + 1) >> 1], a[m >> 1], 16) : a[m >> 1];
      // the tap row is 8 int16 = (t0, t1) (t2, t3) (t4, t5) (t6, t7) as they lie in memory: the pairs one tap further by funnel shift
      const uint4 fq = *reinterpret_cast<const uint4 *>(filt[posx & 15]);
      const uint32_t g1 = __builtin_amdgcn_alignbit(fq.y, fq.x, 16), g2 = __builtin_amdgcn_alignbit(fq.z, fq.y, 16), g3 = __builtin_amdgcn_alignbit(fq.w, fq.z, 16);
      int sum[8];
#pragma unroll
      for (int c = 0; c < 8; c++) {
        int acc = dot2_start(pm[c + 1], g1, 128);   // taps x 32 (see below): the rounding constant 4 x 32
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, pm[c + 3]), __builtin_bit_cast(s16x2, g2), acc, false);
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, pm[c + 5]), __builtin_bit_cast(s16x2, g3), acc, false);
        sum[c] = acc;
      }
      // `filt` is the x 32 table, (32 s + 128) >> 8 == (s + 4) >> 3: the int16 result is bytes 1..2 of the accumulator, and
      // one v_perm shifts and packs two of them (|32 s| < 2^23: no overflow)
#pragma unroll
      for (int k = 0; k < 4; k++) o[k] = __builtin_amdgcn_perm((uint32_t)sum[2 * k + 1], (uint32_t)sum[2 * k], 0x06050201u);
    }
    *reinterpret_cast<uint4 *>(im + j * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}
// mc_h16 for a whole-sample horizontal position (posx = 0): phase 0 is the identity, (128 p + 4) >> 3 = 16 p exactly.
template <typename ES>
__device__ __forceinline__ void mc_h16_copy(const ES *win, int ws, int16_t *im, int lane) {
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int j = lane + it * 8;
    uint32_t o[4];
    if constexpr (sizeof(ES) == 2) {
      const uint4 a = *reinterpret_cast<const uint4 *>(win + j * ws + 4);        // samples 4 .. 11 of the row, two per dword
      o[0] = a.x << 4; o[1] = a.y << 4; o[2] = a.z << 4; o[3] = a.w << 4;         // p < 2^12: no carry between the halves
    } else {
      const uint2 a = *reinterpret_cast<const uint2 *>(win + j * ws + 4);
      o[0] = __builtin_amdgcn_perm(0u, a.x, 0x0c010c00u) << 4; o[1] = __builtin_amdgcn_perm(0u, a.x, 0x0c030c02u) << 4;
      o[2] = __builtin_amdgcn_perm(0u, a.y, 0x0c010c00u) << 4; o[3] = __builtin_amdgcn_perm(0u, a.y, 0x0c030c02u) << 4;
    }
    *reinterpret_cast<uint4 *>(im + j * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}
// The vertical displacements of one refinement round differ by less than a sample and the regular filter has six taps (1..6),
// so row `lane` of all of them reads intermediate rows lane + 1 .. lane + 7: those seven rows (16 bytes each) are loaded ONCE
// per horizontal position (mc_rows7) and every vertical candidate is a 7-tap sum over them — the six taps of its phase shifted
// by its integer part, a zero at the other end (mc_v7).  The first version of k_inter_pipe was LDS-bound (LDS busy 85 % of the
// kernel by PMC); this cut the reads of the vertical pass from 8 per candidate to 7 per three candidates.
// After the LDS diet the kernel is VALU-bound, so the vertical sums run on v_dot2_i32_i16: the rows are interleaved once per
// horizontal position into row PAIRS per column, pr[kp][c] = (row 2kp + 1, row 2kp + 2) of column c ("row 8" = a constant), and
// a candidate is 4 dot2 per sample instead of 7 multiply-adds + 7 extracts (exact: int16 x int16 into int32).
__device__ __forceinline__ void mc_rows7(const int16_t *im, int lane, uint32_t (*pr)[8]) {
  uint4 rw[8];
#pragma unroll
  for (int k = 0; k < 7; k++) rw[k] = *reinterpret_cast<const uint4 *>(im + (lane + 1 + k) * 8);
  rw[7] = make_uint4(0x00020002u, 0x00020002u, 0x00020002u, 0x00020002u);   // "row 8" = the constant 2: carries mc_v7's rounding term
#pragma unroll
  for (int kp = 0; kp < 4; kp++) {
    const uint32_t x[4] = { rw[2 * kp].x, rw[2 * kp].y, rw[2 * kp].z, rw[2 * kp].w };
    const uint32_t y[4] = { rw[2 * kp + 1].x, rw[2 * kp + 1].y, rw[2 * kp + 1].z, rw[2 * kp + 1].w };
#pragma unroll
    for (int d = 0; d < 4; d++) row_pair(x[d], y[d], pr[kp][2 * d], pr[kp][2 * d + 1]);
  }
}
// `filt32` holds the taps times 32: (32 s + 32768) >> 16 == (s + 1024) >> 11 exactly, and the result is then the high half of
// the accumulator — one v_perm takes the high halves of two sums, shift and pack in one instruction (the products stay far
// inside int32: |intermediate| < 2^15, sum of |taps| x 32 < 2^13).  Returns row `lane` of the prediction as four packed pairs.
__device__ __forceinline__ void mc_v7(const uint32_t (*pr)[8], int posy, const int16_t (*filt32)[8], int bd, uint32_t *ow) {
  const int oy = 4 + (posy >> 4) - 3;            // 0 or 1
  // the taps over rows lane + 1 .. lane + 7 as pairs.  The tap row lies in memory as (t0, t1) (t2, t3) (t4, t5) (t6, t7), t0 = t7 = 0:
  //   oy = 1 (rows 2 .. 7 carry t1 .. t6): (0, t1) (t2, t3) (t4, t5) (t6, .)   = the row as it lies;
  //   oy = 0 (rows 1 .. 6 carry t1 .. t6): (t1, t2) (t3, t4) (t5, t6) (0, .)   = one funnel shift per pair.
  // The last pair's second row is the constant 2 (mc_rows7) and its tap 16384: 2 x 16384 = 32768 is the rounding term, so the
  // accumulators start at 0 — an inline constant of the first dot2 instead of a v_mov of a literal per column.
  const uint4 fq = *reinterpret_cast<const uint4 *>(filt32[posy & 15]);
  const uint32_t g[4] = { oy ? fq.x : __builtin_amdgcn_alignbit(fq.y, fq.x, 16), oy ? fq.y : __builtin_amdgcn_alignbit(fq.z, fq.y, 16),
                          oy ? fq.z : __builtin_amdgcn_alignbit(fq.w, fq.z, 16), (oy ? (fq.w & 0xFFFFu) : 0u) | 0x40000000u };
  int s[8];
#pragma unroll
  for (int kp = 0; kp < 4; kp++) {
    const s16x2 gp = __builtin_bit_cast(s16x2, g[kp]);
#pragma unroll
    for (int c = 0; c < 8; c++)
      s[c] = kp == 0 ? dot2_start(pr[kp][c], g[kp], 0) : __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, pr[kp][c]), gp, s[c], false);
  }
  const s16x2 zero = { 0, 0 }, top = { (short)((1 << bd) - 1), (short)((1 << bd) - 1) };
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const s16x2 v = __builtin_bit_cast(s16x2, __builtin_amdgcn_perm((uint32_t)s[2 * j + 1], (uint32_t)s[2 * j], 0x07060302u));
    ow[j] = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_elementwise_max(v, zero), top));
  }
}

}  // namespace av1mi
