// search_sse.hpp — the source samples of a 64x64 superblock and the squared error against them, for the searches that try candidates on a
// superblock held in LDS (k_cdef_search, k_lf_search): one 256-lane workgroup per superblock, a lane owns 16 luma + 8 chroma samples, four
// at a time.  SOURCE is SbSource::load; the error of four samples sq_diff4 (a lane's 24 samples: below 2^25); the sums wave_sum (below
// 2^31), then wave_sums_total over the four waves' partials in 64 bits.
#pragma once
#include "av1mi_internal.hpp"

namespace av1mi {

// The lane's items.  Luma item q = tid + 256 k (k < 4) is row q >> 4, columns (q & 15) * 4 .. + 3 of the superblock; chroma item k (k < 2)
// is plane k, row (tid >> 3) & 31, columns (tid & 7) * 4 .. + 3.  These are the samples cdef_filter.hpp's cdef_luma_item / cdef_chroma_item
// hand item tid + 256 k: k_cdef_search's sinks rely on it.
__device__ __forceinline__ int sb_luma_row(int q) { return q >> 4; }
__device__ __forceinline__ int sb_luma_col(int q) { return (q & 15) * 4; }
__device__ __forceinline__ int sb_chroma_row(int tid) { return (tid >> 3) & 31; }
__device__ __forceinline__ int sb_chroma_col(int tid) { return (tid & 7) * 4; }

// four samples as they lie in memory
template <typename Pix> struct Samples4 { uint32_t w[sizeof(Pix) == 1 ? 1 : 2]; };
template <typename Pix> __device__ __forceinline__ Samples4<Pix> load_samples4(const Pix *p) {
  Samples4<Pix> v;
  if constexpr (sizeof(Pix) == 1) v.w[0] = *reinterpret_cast<const uint32_t *>(p);
  else { const uint2 u = *reinterpret_cast<const uint2 *>(p); v.w[0] = u.x; v.w[1] = u.y; }
  return v;
}
template <typename Pix> __device__ __forceinline__ int sample_at(const Samples4<Pix> &v, int i) {
  if constexpr (sizeof(Pix) == 1) return (int)((v.w[0] >> (8 * i)) & 255u);
  else return (int)((v.w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
}
// the squared difference of the first n of four samples (a select, no branch)
template <typename Pix> __device__ __forceinline__ uint32_t sq_diff4(const int (&o)[4], const Samples4<Pix> &s, int n) {
  uint32_t e = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) { const int d = o[i] - sample_at<Pix>(s, i); e += i < n ? (uint32_t)(d * d) : 0u; }
  return e;
}
// ... with the four samples in an LDS tile (uint16, the first at an even index)
template <typename Pix> __device__ __forceinline__ uint32_t sq_diff4(const uint16_t *t, const Samples4<Pix> &s, int n) {
  const uint32_t *t32 = reinterpret_cast<const uint32_t *>(t);      // (two dwords: the rows are an odd number of dwords apart)
  const uint2 u = { t32[0], t32[1] };
  const int o[4] = { (int)(u.x & 0xFFFFu), (int)(u.x >> 16), (int)(u.y & 0xFFFFu), (int)(u.y >> 16) };
  return sq_diff4<Pix>(o, s, n);
}

// SOURCE: the lane's samples of superblock (sbx, sby), and how many of each four count: those inside the TRUE size tw x th, chroma
// (t + 1) / 2 — the rule stands here and nowhere else.  orig: the source planes, oy / oc the frame's offset in them; w x h: the coded size
template <typename Pix> struct SbSource {
  Samples4<Pix> sy[4], sc[2];
  int ny[4], nc[2];
  __device__ __forceinline__ void load(const void *const (&orig)[3], size_t oy, size_t oc, int stride_y, int stride_uv, int sbx, int sby, int w, int h, int tw, int th, int tid) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int q = tid + 256 * k, fy = sby * 64 + sb_luma_row(q), fx = sbx * 64 + sb_luma_col(q);
      ny[k] = fy < th ? min(max(tw - fx, 0), 4) : 0;
      sy[k] = fy < h && fx < w ? load_samples4(reinterpret_cast<const Pix *>(orig[0]) + oy + row_off(fy, stride_y) + fx) : Samples4<Pix>{};
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int fy = sby * 32 + sb_chroma_row(tid), fx = sbx * 32 + sb_chroma_col(tid);
      nc[k] = fy < (th + 1) / 2 ? min(max((tw + 1) / 2 - fx, 0), 4) : 0;
      sc[k] = fy < h / 2 && fx < w / 2 ? load_samples4(reinterpret_cast<const Pix *>(orig[1 + k]) + oc + row_off(fy, stride_uv) + fx) : Samples4<Pix>{};
    }
  }
};

// a lane's sum over its wave (every lane gets it), and the workgroup's total from the four waves' partials
__device__ __forceinline__ uint32_t wave_sum(uint32_t e) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) e += __shfl_xor(e, d, 64);
  return e;
}
__device__ __forceinline__ unsigned long long wave_sums_total(const uint32_t (&w)[4]) { return (unsigned long long)w[0] + w[1] + w[2] + w[3]; }

}  // namespace av1mi
