// input_kernels.hip — the input stage in front of the block pipeline (include/av1mi.h enum av1mi_input_format): one streaming
// kernel turns a wire / surface format (10-bit packed planes, P010, NV12) into the planar planes every other kernel reads, and the
// host-side helpers that define and produce those formats (av1mi_input_plane_bytes, av1mi_input_pack; no GPU needed).
//
// The kernel is pure bandwidth (PACKED10 1.25 B in + 2 B out per sample, P010 2 + 2, NV12 1 + 1), so all it has to get right is the
// access shape: a lane owns one UNIT, consecutive lanes consecutive units, every wave-instruction reads or writes one contiguous run,
// 16 bytes per lane wherever the format's granularity allows it.  Units (all planes of a batch are whole numbers of them, because
// width and height are multiples of 8: a plane has a multiple of 64 luma / 16 chroma samples):
//   PACKED10   16 samples of one plane: 20 bytes in (dwordx4 + dword at 4-byte alignment), 32 bytes out (2 x dwordx4)
//   P010       luma: 8 samples, 16 bytes in and out;  chroma: 8 (U, V) pairs, 32 bytes in, 16 bytes to each of U and V
//   NV12       luma: 16 samples, 16 bytes in and out; chroma: 16 pairs, 32 bytes in, 16 bytes to each of U and V
// The three planes share one launch: the unit index runs over luma first, then chroma; the grid is capped and strides over the units.
// Further down: k_chroma_convert, the stage behind it for sources that are not 4:2:0 or deeper than the coded depth.
#include <string.h>
#include "av1mi_internal.hpp"

namespace av1mi {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));     // a 16-byte load from a 4-byte aligned address

// 16 samples of 10 bits = five little-endian dwords -> eight dwords of two uint16 samples each.  Sample i sits at bit 10 i of the 160:
// every index below is a compile-time constant, a sample that straddles two dwords is one 64-bit shift (v_alignbit_b32).
__device__ __forceinline__ void unpack16(const uint32_t (&w)[5], uint32_t (&o)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint32_t s[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int bit = 10 * (2 * k + j), d = bit >> 5, sh = bit & 31;
      s[j] = (sh <= 22 ? w[d] >> sh : (uint32_t)((((uint64_t)w[d + 1] << 32) | w[d]) >> sh)) & 0x3FFu;
    }
    o[k] = s[0] | (s[1] << 16);
  }
}

template <int F>
__global__ __launch_bounds__(256) void k_input_convert(InputLaunch L) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < L.units; u += stride) {
    if (F == AV1MI_INPUT_PACKED10) {
      // which plane: luma units first, then U, then V (wave-uniform except in the two waves that straddle a boundary)
      const int p = u < L.units_y ? 0 : u < L.units_y + L.units_c ? 1 : 2;
      const size_t i = u - (p == 0 ? 0 : p == 1 ? L.units_y : L.units_y + L.units_c);
      const char *src = (const char *)(p == 0 ? L.in[0] : p == 1 ? L.in[1] : L.in[2]) + i * 20;      // (selects: no indexed kernel argument)
      const u32x4_a4 a = *(const u32x4_a4 *)src;
      const uint32_t w[5] = { a.x, a.y, a.z, a.w, *(const uint32_t *)(src + 16) };
      uint32_t o[8];
      unpack16(w, o);
      u32x4 *dst = (u32x4 *)((char *)(p == 0 ? L.out[0] : p == 1 ? L.out[1] : L.out[2]) + i * 32);
      dst[0] = u32x4{ o[0], o[1], o[2], o[3] };
      dst[1] = u32x4{ o[4], o[5], o[6], o[7] };
    } else if (u < L.units_y) {      // semi-planar formats, luma: 16 bytes in, 16 bytes out
      u32x4 a = ((const u32x4 *)L.in[0])[u];
      if (F == AV1MI_INPUT_P010) a = (a >> 6) & 0x03FF03FFu;      // the value sits in bits 15..6 of each half; the low 6 bits are ignored
      ((u32x4 *)L.out[0])[u] = a;
    } else {                         // chroma: 32 bytes of interleaved pairs -> 16 bytes of U, 16 bytes of V
      const size_t i = u - L.units_y;
      const u32x4 a = ((const u32x4 *)L.in[1])[2 * i], b = ((const u32x4 *)L.in[1])[2 * i + 1];
      const uint32_t d[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
      uint32_t ou[4], ov[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t lo = d[2 * k], hi = d[2 * k + 1];
        if (F == AV1MI_INPUT_P010) {      // dword = U | V << 16
          ou[k] = ((lo >> 6) & 0x3FFu) | ((hi << 10) & 0x03FF0000u);
          ov[k] = (lo >> 22) | ((hi >> 6) & 0x03FF0000u);
        } else {                          // dword = U0 | V0 << 8 | U1 << 16 | V1 << 24: bytes 0, 2 of both -> U, bytes 1, 3 -> V (v_perm_b32)
          ou[k] = __builtin_amdgcn_perm(hi, lo, 0x06040200u);
          ov[k] = __builtin_amdgcn_perm(hi, lo, 0x07050301u);
        }
      }
      ((u32x4 *)L.out[1])[i] = u32x4{ ou[0], ou[1], ou[2], ou[3] };
      ((u32x4 *)L.out[2])[i] = u32x4{ ov[0], ov[1], ov[2], ov[3] };
    }
  }
}

// ---- chroma formats (include/av1mi.h "chroma formats"): a 4:2:2 / 4:4:4 / grey or 12-bit source -> the 4:2:0 planes that are coded.
// Pure bandwidth again (4:4:4 10-bit: 4 B in + 1 B out per luma sample of chroma, 12-bit adds 2 + 2 of luma), same access discipline:
// a lane owns one CELL = 16 bytes of one output row (16 samples of uint8, 8 of uint16; the last cell of a row may be short, rows are
// multiples of 4 bytes), consecutive lanes consecutive cells, rows following each other — the output planes have no row padding, so a
// wave stores one contiguous run, and loads one contiguous run per source row it needs (1 for a copy, 2 for 4:2:2, 2 x 32 bytes per
// lane for 4:4:4), dwordx4 at the rows' 4-byte alignment.  Frame and plane are uniform per workgroup (the grid is frames x (luma blocks
// + 2 x chroma blocks)), so no wave mixes frames at the vertical clamp.  The 4:4:4 filter needs ONE sample outside a lane's own 32
// bytes, the column left of them: the vertical sum of the neighbouring lane's last column, handed over through a 256-entry LDS row
// (the first lane of a workgroup reads its two samples from memory instead).  Lanes whose cell reaches past the TRUE width take the
// sample-by-sample clamped path; the vertical clamp is two row indices per lane and costs nothing.
struct ChromaGeo {      // one plane of one frame: the source buffer, the true source size, the output plane, its cells and workgroups
  int in_stride, in_rows, wp, hp, out_w, out_rows, cpr;
  unsigned blocks;
};
struct ChromaArgs {
  const void *in[3]; void *out[3];
  ChromaGeo y, c;       // y.blocks == 0: the luma plane is not converted (equal depths)
  unsigned blocks_per_frame;
};

template <typename Pix, int S>
__device__ __forceinline__ uint32_t chroma_round(uint32_t v) {
  constexpr uint32_t kMax = sizeof(Pix) == 1 ? 255u : 1023u;
  if (S == 0) return v;
  const uint32_t r = (v + (1u << (S > 0 ? S - 1 : 0))) >> S;
  return r < kMax ? r : kMax;
}
// sample i of a run of little-endian dwords / N samples -> the cell's four dwords
template <typename Pix>
__device__ __forceinline__ uint32_t chroma_sample(const uint32_t *w, int i) {
  return sizeof(Pix) == 1 ? (w[i >> 2] >> (8 * (i & 3))) & 0xFFu : (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
}
template <typename Pix>
__device__ __forceinline__ void chroma_pack(const uint32_t *v, uint32_t (&o)[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++)
    o[k] = sizeof(Pix) == 1 ? v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24) : v[2 * k] | (v[2 * k + 1] << 16);
}
// the cell's first n samples (n * sizeof(Pix) a multiple of 4) to a 4-byte aligned address: one dwordx4 for a whole cell
template <typename Pix>
__device__ __forceinline__ void chroma_store(Pix *dst, const uint32_t (&o)[4], int n) {
  constexpr int N = 16 / (int)sizeof(Pix);
  if (n == N) { *(u32x4_a4 *)dst = u32x4_a4{ o[0], o[1], o[2], o[3] }; return; }
#pragma unroll
  for (int k = 0; k < 3; k++)
    if (k * (N / 4) < n) ((uint32_t *)dst)[k] = o[k];
}

template <typename Pix, int CHROMA, int D>
__global__ __launch_bounds__(256) void k_chroma_convert(ChromaArgs A) {
  constexpr int N = 16 / (int)sizeof(Pix);
  __shared__ uint32_t left_of[256];      // 4:4:4: the vertical sum of every lane's last column
  // frame, plane and block inside the plane: uniform
  unsigned b = blockIdx.x;
  const unsigned f = b / A.blocks_per_frame;
  b -= f * A.blocks_per_frame;
  const bool luma = b < A.y.blocks;
  if (!luma) b -= A.y.blocks;
  const int p = luma ? 0 : b < A.c.blocks ? 1 : 2;
  if (p == 2) b -= A.c.blocks;
  const ChromaGeo G = luma ? A.y : A.c;
  const Pix *in = (const Pix *)(p == 0 ? A.in[0] : p == 1 ? A.in[1] : A.in[2]) + (size_t)f * G.in_rows * G.in_stride;      // (selects: no indexed kernel argument)
  Pix *out = (Pix *)(p == 0 ? A.out[0] : p == 1 ? A.out[1] : A.out[2]) + (size_t)f * G.out_rows * G.out_w;
  const unsigned idx = b * 256u + threadIdx.x;
  const bool active = idx < (unsigned)(G.out_rows * G.cpr);
  const int row = active ? (int)(idx / (unsigned)G.cpr) : 0, cell = active ? (int)(idx - (unsigned)row * G.cpr) : 0;
  const int x0 = cell * N, n = G.out_w - x0 < N ? G.out_w - x0 : N;      // the cell's samples: a short last cell where the row is no multiple of 16 bytes
  Pix *dst = out + (size_t)row * G.out_w + x0;
  uint32_t v[N], o[4];

  if (luma || CHROMA == AV1MI_CHROMA_420) {               // S = in(x, y), s = d
    if (!active) return;
    const Pix *r0 = in + (size_t)(row < G.hp - 1 ? row : G.hp - 1) * G.in_stride;
    if (x0 + N <= G.wp) {
      const u32x4_a4 a = *(const u32x4_a4 *)(r0 + x0);
      const uint32_t w[4] = { a.x, a.y, a.z, a.w };
#pragma unroll
      for (int i = 0; i < N; i++) v[i] = chroma_round<Pix, D>(chroma_sample<Pix>(w, i));
    } else {
#pragma unroll
      for (int i = 0; i < N; i++) { const int x = x0 + i; v[i] = chroma_round<Pix, D>(r0[x < G.wp - 1 ? x : G.wp - 1]); }
    }
  } else if (CHROMA == AV1MI_CHROMA_400) {                // flat chroma
    if (!active) return;
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = sizeof(Pix) == 1 ? 128u : 512u;
  } else {
    const int y0 = 2 * row < G.hp - 1 ? 2 * row : G.hp - 1, y1 = 2 * row + 1 < G.hp - 1 ? 2 * row + 1 : G.hp - 1;
    const Pix *r0 = in + (size_t)y0 * G.in_stride, *r1 = in + (size_t)y1 * G.in_stride;
    if (CHROMA == AV1MI_CHROMA_422) {                     // S = in(x, 2 y) + in(x, 2 y + 1), s = 1 + d
      if (!active) return;
      if (x0 + N <= G.wp) {
        const u32x4_a4 a = *(const u32x4_a4 *)(r0 + x0), c = *(const u32x4_a4 *)(r1 + x0);
        const uint32_t w0[4] = { a.x, a.y, a.z, a.w }, w1[4] = { c.x, c.y, c.z, c.w };
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = chroma_round<Pix, 1 + D>(chroma_sample<Pix>(w0, i) + chroma_sample<Pix>(w1, i));
      } else {
#pragma unroll
        for (int i = 0; i < N; i++) { const int x = x0 + i < G.wp - 1 ? x0 + i : G.wp - 1; v[i] = chroma_round<Pix, 1 + D>((uint32_t)r0[x] + r1[x]); }
      }
    } else {                                              // 4:4:4: S = sum over both rows of in(2 x - 1) + 2 in(2 x) + in(2 x + 1), s = 3 + d
      const int c0 = 2 * x0;
      const bool fast = active && c0 + 2 * N <= G.wp;
      uint32_t s[2 * N];                                  // vertical sums of the lane's own 2 N columns
      if (fast) {
        const u32x4_a4 a0 = *(const u32x4_a4 *)(r0 + c0), a1 = *(const u32x4_a4 *)(r0 + c0 + N);
        const u32x4_a4 b0 = *(const u32x4_a4 *)(r1 + c0), b1 = *(const u32x4_a4 *)(r1 + c0 + N);
        const uint32_t w0[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w }, w1[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
#pragma unroll
        for (int i = 0; i < 2 * N; i++) s[i] = chroma_sample<Pix>(w0, i) + chroma_sample<Pix>(w1, i);
        left_of[threadIdx.x] = s[2 * N - 1];
      }
      __syncthreads();      // (reached by every lane of the workgroup: nothing above returns on this path)
      if (!active) return;
      if (fast) {
        // the column left of the cell: the row's first cell clamps to its own first column; otherwise the previous lane holds it — the
        // same row's previous cell, which lies wholly inside the true width as well — except for the workgroup's first lane
        uint32_t l = s[0];
        if (cell != 0) l = threadIdx.x != 0 ? left_of[threadIdx.x - 1] : (uint32_t)r0[c0 - 1] + r1[c0 - 1];
#pragma unroll
        for (int i = 0; i < N; i++) { v[i] = chroma_round<Pix, 3 + D>(l + 2 * s[2 * i] + s[2 * i + 1]); l = s[2 * i + 1]; }
      } else {
        const int last = G.wp - 1;
#pragma unroll
        for (int i = 0; i < N; i++) {
          const int c = c0 + 2 * i, cl = c - 1 < 0 ? 0 : c - 1 < last ? c - 1 : last, cm = c < last ? c : last, cr = c + 1 < last ? c + 1 : last;
          v[i] = chroma_round<Pix, 3 + D>((uint32_t)r0[cl] + r1[cl] + 2 * ((uint32_t)r0[cm] + r1[cm]) + r0[cr] + r1[cr]);
        }
      }
    }
  }
  chroma_pack<Pix>(v, o);
  chroma_store<Pix>(dst, o, n);
}

}  // namespace

const char *chroma_format_error(int chroma, int src_bd, int bd) {
  if (chroma < AV1MI_CHROMA_420 || chroma > AV1MI_CHROMA_400) return "source_chroma unknown (0 4:2:0, 1 4:2:2, 2 4:4:4, 3 grey)";
  if (!((src_bd == 8 && bd == 8) || (src_bd == 10 && bd == 10) || (src_bd == 12 && bd == 10))) return "a source is coded 8 -> 8, 10 -> 10 or 12 -> 10 bits";
  return nullptr;
}

hipError_t launch_chroma_convert(const ChromaLaunch &L, hipStream_t s) {
  if (chroma_format_error(L.chroma, L.src_bd, L.bd) || L.w < 1 || L.h < 1 || L.w > 16384 || L.h > 16384 || L.frames < 1) return hipErrorInvalidValue;
  const int W8 = (L.w + 7) & ~7, H8 = (L.h + 7) & ~7, sz = L.src_bd == 8 ? 1 : 2, d = L.src_bd - L.bd;
  ChromaArgs A;
  memset(&A, 0, sizeof(A));
  for (int p = 0; p < 3; p++) { A.in[p] = L.in[p]; A.out[p] = L.out[p]; }
  auto cells = [&](ChromaGeo &G) { G.cpr = (G.out_w * sz + 15) / 16; G.blocks = (unsigned)(((size_t)G.out_rows * G.cpr + 255) / 256); };
  A.y = ChromaGeo{ W8, H8, L.w, L.h, W8, H8, 0, 0 };
  cells(A.y);
  if (!d) A.y.blocks = 0;
  A.c = L.chroma == AV1MI_CHROMA_444 ? ChromaGeo{ W8, H8, L.w, L.h, W8 / 2, H8 / 2, 0, 0 }
      : L.chroma == AV1MI_CHROMA_422 ? ChromaGeo{ W8 / 2, H8, (L.w + 1) / 2, L.h, W8 / 2, H8 / 2, 0, 0 }
                                     : ChromaGeo{ W8 / 2, H8 / 2, (L.w + 1) / 2, (L.h + 1) / 2, W8 / 2, H8 / 2, 0, 0 };
  cells(A.c);
  A.blocks_per_frame = A.y.blocks + 2 * A.c.blocks;
  const size_t total = (size_t)A.blocks_per_frame * L.frames;
  if (total > 0x7FFFFFFFu) return hipErrorInvalidValue;
  const dim3 grid((unsigned)total), block(256);
#define CHROMA_CASE(Pix, C, D) hipLaunchKernelGGL((k_chroma_convert<Pix, C, D>), grid, block, 0, s, A)
#define CHROMA_LAYOUTS(Pix, D)                                                 \
  switch (L.chroma) {                                                          \
    case AV1MI_CHROMA_420: CHROMA_CASE(Pix, AV1MI_CHROMA_420, D); break;       \
    case AV1MI_CHROMA_422: CHROMA_CASE(Pix, AV1MI_CHROMA_422, D); break;       \
    case AV1MI_CHROMA_444: CHROMA_CASE(Pix, AV1MI_CHROMA_444, D); break;       \
    default: CHROMA_CASE(Pix, AV1MI_CHROMA_400, D); break;                     \
  }
  if (L.src_bd == 8) { CHROMA_LAYOUTS(uint8_t, 0) }
  else if (d == 0) { CHROMA_LAYOUTS(uint16_t, 0) }
  else { CHROMA_LAYOUTS(uint16_t, 2) }
#undef CHROMA_LAYOUTS
#undef CHROMA_CASE
  return hipGetLastError();
}

hipError_t launch_input_convert(int format, InputLaunch L, hipStream_t s) {
  // ny luma and nc chroma samples per plane -> units (see the head of this file)
  const size_t per_y = format == AV1MI_INPUT_P010 ? 8 : 16, per_c = per_y;
  L.units_y = L.ny / per_y; L.units_c = L.nc / per_c;
  L.units = L.units_y + (format == AV1MI_INPUT_PACKED10 ? 2 * L.units_c : L.units_c);
  if (!L.units) return hipSuccess;
  // memory-bound: 2048 workgroups of 256 lanes (8 per CU) stride over the units
  const size_t want = (L.units + 255) / 256;
  const dim3 grid((unsigned)(want < 2048 ? want : 2048)), block(256);
  switch (format) {
    case AV1MI_INPUT_PACKED10: hipLaunchKernelGGL(k_input_convert<AV1MI_INPUT_PACKED10>, grid, block, 0, s, L); break;
    case AV1MI_INPUT_P010: hipLaunchKernelGGL(k_input_convert<AV1MI_INPUT_P010>, grid, block, 0, s, L); break;
    case AV1MI_INPUT_NV12: hipLaunchKernelGGL(k_input_convert<AV1MI_INPUT_NV12>, grid, block, 0, s, L); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace av1mi

// ---- the formats on the host: sizes and packing (plain C++, the loops are written for the compiler's vectoriser) ---------------

namespace {

bool format_valid(int format, int bit_depth) {
  switch (format) {
    case AV1MI_INPUT_PLANAR: return bit_depth == 8 || bit_depth == 10;
    case AV1MI_INPUT_PACKED10: case AV1MI_INPUT_P010: return bit_depth == 10;
    case AV1MI_INPUT_NV12: return bit_depth == 8;
    default: return false;
  }
}

// n samples (a multiple of 16) -> n * 5 / 4 bytes, sixteen samples (the unit the kernel reads) = 20 bytes per step.  Four samples are
// one 64-bit load; two masks and a shift close the 6-bit gaps pairwise, one more joins the two 20-bit halves into a 40-bit group; four
// groups are stored as 8 + 8 + 4 bytes.  A step touches nothing outside its own 20 bytes.  (Little-endian host, like every byte
// layout of this ABI.)
inline uint64_t group40(const uint16_t *s) {
  uint64_t x;
  memcpy(&x, s, 8);
  const uint64_t t = (x & 0x000003FF000003FFull) | ((x & 0x03FF000003FF0000ull) >> 6);
  return (t & 0xFFFFFu) | ((t >> 32) << 20);
}
void pack10(const uint16_t *__restrict s, uint8_t *__restrict o, size_t n) {
  for (size_t k = 0; k < n / 16; k++) {
    const uint64_t g0 = group40(s + 16 * k), g1 = group40(s + 16 * k + 4), g2 = group40(s + 16 * k + 8), g3 = group40(s + 16 * k + 12);
    const uint64_t a = g0 | g1 << 40, b = g1 >> 24 | g2 << 16 | g3 << 56;
    const uint32_t c = (uint32_t)(g3 >> 8);
    memcpy(o + 20 * k, &a, 8); memcpy(o + 20 * k + 8, &b, 8); memcpy(o + 20 * k + 16, &c, 4);
  }
}
template <typename T, int SHIFT>
void interleave(const T *__restrict u, const T *__restrict v, T *__restrict o, size_t n) {
  for (size_t i = 0; i < n; i++) { o[2 * i] = (T)(u[i] << SHIFT); o[2 * i + 1] = (T)(v[i] << SHIFT); }
}

}  // namespace

extern "C" {

size_t av1mi_input_plane_bytes(int format, int bit_depth, int plane, int width, int rows) {
  if (!format_valid(format, bit_depth) || plane < 0 || plane > 2 || width <= 0 || rows <= 0 || (width & 7) || (rows & 7)) return 0;
  const size_t ny = (size_t)width * rows, n = plane ? ny / 4 : ny;
  switch (format) {
    case AV1MI_INPUT_PLANAR: return n * (bit_depth == 8 ? 1 : 2);
    case AV1MI_INPUT_PACKED10: return n * 5 / 4;
    default: {      // semi-planar: luma, then (U, V) pairs
      const size_t bps = format == AV1MI_INPUT_P010 ? 2 : 1;
      return plane == 0 ? n * bps : plane == 1 ? 2 * n * bps : 0;
    }
  }
}

size_t av1mi_source_plane_bytes(int source_chroma, int source_bit_depth, int plane, int width, int rows) {
  if (source_chroma < AV1MI_CHROMA_420 || source_chroma > AV1MI_CHROMA_400 || (source_bit_depth != 8 && source_bit_depth != 10 && source_bit_depth != 12) || plane < 0 ||
      plane > 2 || width <= 0 || rows <= 0 || (width & 7) || (rows & 7))
    return 0;
  const size_t ny = (size_t)width * rows * (source_bit_depth == 8 ? 1 : 2);
  if (plane == 0) return ny;
  return source_chroma == AV1MI_CHROMA_444 ? ny : source_chroma == AV1MI_CHROMA_422 ? ny / 2 : source_chroma == AV1MI_CHROMA_420 ? ny / 4 : 0;
}

int av1mi_input_pack(int format, int bit_depth, int width, int rows, const void *y, const void *u, const void *v, void *out0, void *out1, void *out2) {
  if (!av1mi_input_plane_bytes(format, bit_depth, 0, width, rows) || !y || !u || !v || !out0 || !out1) return AV1MI_E_INVAL;
  const size_t ny = (size_t)width * rows, nc = ny / 4;
  switch (format) {
    case AV1MI_INPUT_PLANAR:
      if (!out2) return AV1MI_E_INVAL;
      memcpy(out0, y, ny * (bit_depth == 8 ? 1 : 2)); memcpy(out1, u, nc * (bit_depth == 8 ? 1 : 2)); memcpy(out2, v, nc * (bit_depth == 8 ? 1 : 2));
      break;
    case AV1MI_INPUT_PACKED10:
      if (!out2) return AV1MI_E_INVAL;
      pack10((const uint16_t *)y, (uint8_t *)out0, ny); pack10((const uint16_t *)u, (uint8_t *)out1, nc); pack10((const uint16_t *)v, (uint8_t *)out2, nc);
      break;
    case AV1MI_INPUT_P010: {
      const uint16_t *s = (const uint16_t *)y;
      uint16_t *o = (uint16_t *)out0;
      for (size_t i = 0; i < ny; i++) o[i] = (uint16_t)(s[i] << 6);
      interleave<uint16_t, 6>((const uint16_t *)u, (const uint16_t *)v, (uint16_t *)out1, nc);
      break;
    }
    default:
      memcpy(out0, y, ny);
      interleave<uint8_t, 0>((const uint8_t *)u, (const uint8_t *)v, (uint8_t *)out1, nc);
      break;
  }
  return AV1MI_OK;
}

}  // extern "C"
