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

}  // namespace

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
