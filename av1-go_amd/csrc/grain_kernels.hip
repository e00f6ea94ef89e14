// grain_kernels.hip — the denoising gather behind av1mi_gop_config.denoise (include/av1mi.h "denoising", "grain records"): k_denoise_gather
// stands where k_frames_gather / k_deint_gather stand, and measures what it removes on the way; k_grain_sum adds the measurements up.
//
//   work      k_deint_gather's, from gather_cells.hpp (band_geometry, gather_plane, gather_band, the cells): an item is (segment, plane,
//             band of kBand output rows, group of 64 cells of 16 bytes), a wave owns an item and walks down its band, a workgroup holds
//             four consecutive items of one (segment, plane).
//   rows      per row and per neighbour frame F the wave computes A = |C - F| of its cell as PACKED 16-bit halves (v_pk_max / min / sub)
//             and the horizontal 3-sums H = A(x - 1) + A(x) + A(x + 1), two samples per add (no half can carry: 3 x 4095).  H of three
//             rows is held rolling (previous, current, next); D = their sum (<= 9 x 4095 < 2^16).  Inside a band every row of C, P and
//             N is loaded once; a band re-reads one row above and one below it.
//   columns   A(x0 - 1) and A(x0 + NS) are the neighbouring lanes': one dword (P's half, N's half) moved up and one moved down per row
//             by ds_bpermute_b32.  Lanes 0 and 63, whose neighbour is another wave's, load that one dword of C, P and N.  At the
//             true edge the last true column's A is replicated in registers; nothing beyond the true size is read into the result.
//   samples   weights, output and the residual are per sample in 32 bits: num <= 48 x 4095 does not fit a half.  K[den] comes from a
//             register of lane den - 16 (ds_bpermute_b32 again: no LDS memory for it).
//   records   a lane adds r^2 and 1 into a (bin, sum, count) triple of its own while the bin stays the same, and flushes it into its
//             wave's 16 bins in LDS (integer atomics: the order cannot matter) when the bin changes and at the end of the band; the
//             workgroup's four sets become ONE partial in scratch; k_grain_sum adds the partials of a (segment, plane).  All integers,
//             so every order of addition gives the same bytes.
//   ends      a frame at an end of its run (P or N is C itself) and a flat slot (C null) are the gather alone: copied, resp. zeros,
//             and their partials are zero.
// Arithmetic: include/av1mi.h; restated in numpy by tests/denoise_ref.py.  Reference tree: nothing (it has no denoiser).
// GrainBins and GrainLane are the records' LDS bins and a lane's open triple, for both denoising gathers.
// Below them: k_denoise_search and k_denoise_mc_gather, the motion-compensated pair that av1mi_gop_config.denoise_range launches instead.
#include "gather_cells.hpp"
#include "motion_common.hpp"

namespace av1mi {

namespace {
struct GrainGeom : BandGeom {
  uint32_t cut, recip;         // 27 T and floor(2^32 / (27 T)) + 1
  int bin_shift;               // bit_depth - 4
  av1mi_grain_bin *partials;   // per workgroup 16 bins, [blockIdx.x]; null = nothing is measured
};

// the records of a workgroup of either denoising gather (in LDS): 16 bins per wave.  The barriers between clear(), the lanes' flushes and
// store() are the kernel's
struct GrainBins {
  unsigned long long sum[4][16];
  uint32_t cnt[4][16];
  __device__ __forceinline__ void clear() {
    if (threadIdx.x < 64) { sum[threadIdx.x >> 4][threadIdx.x & 15] = 0; cnt[threadIdx.x >> 4][threadIdx.x & 15] = 0; }
  }
  // the four waves' sets become ONE partial, the workgroup's
  __device__ __forceinline__ void store(av1mi_grain_bin *partials) const {
    if (threadIdx.x < 16) {
      av1mi_grain_bin b;
      b.sum_sq = sum[0][threadIdx.x] + sum[1][threadIdx.x] + sum[2][threadIdx.x] + sum[3][threadIdx.x];
      b.count = cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
      b.reserved = 0;
      partials[(size_t)blockIdx.x * 16 + threadIdx.x] = b;
    }
  }
};
// a lane's open (bin, sum, count) triple: the kernel adds residuals to it while the bin stays the same and flushes it into the wave's bins
// when the bin changes and at the end.  (The update itself stays in the kernels' loops: as a member function it is optimised on its own
// before it is inlined, and costs the plain gather three register moves per sample.)
struct GrainLane {
  int bin = -1;
  unsigned long long acc = 0; uint32_t cnt = 0;
  __device__ __forceinline__ void flush(GrainBins &S, unsigned wave) {
    if (bin >= 0) { atomicAdd(&S.sum[wave][bin], acc); atomicAdd(&S.cnt[wave][bin], cnt); }
    acc = 0; cnt = 0;
  }
};

// K[den - 16] = round(65536 / den), den = 16 .. 48 (include/av1mi.h prints it)
__device__ const uint32_t kRecipDen[33] = { 4096, 3855, 3641, 3449, 3277, 3121, 2979, 2849, 2731, 2621, 2521, 2427, 2341, 2260, 2185, 2114, 2048,
                                            1986, 1928, 1872, 1820, 1771, 1725, 1680, 1638, 1598, 1560, 1524, 1489, 1456, 1425, 1394, 1365 };

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
// |a - b| of both 16-bit halves
__device__ __forceinline__ uint32_t pk_absdiff(uint32_t a, uint32_t b) {
  const us2 x = __builtin_bit_cast(us2, a), y = __builtin_bit_cast(us2, b);
  return __builtin_bit_cast(uint32_t, (us2)(__builtin_elementwise_max(x, y) - __builtin_elementwise_min(x, y)));
}
// the samples of a cell as 16-bit halves: NP dwords, sample 2 q in the low half of dword q
template <typename Pix, int NP>
__device__ __forceinline__ void halves(const uint32_t c[4], uint32_t o[NP]) {
  if constexpr (sizeof(Pix) == 1) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      o[2 * q] = (c[q] & 0xffu) | ((c[q] & 0xff00u) << 8);
      o[2 * q + 1] = ((c[q] >> 16) & 0xffu) | ((c[q] >> 24) << 16);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++) o[q] = c[q];
  }
}
__device__ __forceinline__ uint32_t half_of(const uint32_t *v, int j) { return (v[j >> 1] >> (16 * (j & 1))) & 0xffffu; }
template <typename Pix>
__device__ __forceinline__ uint32_t last_sample(uint32_t d) { return sizeof(Pix) == 1 ? d >> 24 : d >> 16; }
template <typename Pix>
__device__ __forceinline__ uint32_t first_sample(uint32_t d) { return sizeof(Pix) == 1 ? d & 0xffu : d & 0xffffu; }

// the halves beyond sample lastj take the value of sample lastj (>= 0), without indexing registers by a variable
template <int NP>
__device__ __forceinline__ void replicate_halves(uint32_t v[NP], int lastj) {
  uint32_t e = v[0] & 0xffffu;
#pragma unroll
  for (int j = 1; j < 2 * NP; j++) {
    e = j <= lastj ? half_of(v, j) : e;
    v[j >> 1] = (v[j >> 1] & ~(0xffffu << (16 * (j & 1)))) | e << (16 * (j & 1));
  }
}
template <int NP>
struct GrainRow { uint32_t c[4], p[4], n[4], hp[NP], hn[NP]; };      // the cells of a row and its horizontal 3-sums against P and N

}  // namespace

// grid: per_seg x segments; 4 waves = 4 consecutive items of one (segment, plane)
template <typename Pix>
__global__ __launch_bounds__(256) void k_denoise_gather(GrainGeom G, const void *const *table) {
  constexpr int NS = 16 / (int)sizeof(Pix);      // samples per cell
  constexpr int NP = NS / 2;                     // dwords of packed halves per cell
  __shared__ GrainBins s_bins;
  const GatherPlane W = gather_plane(G, table);
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const bool measure = G.partials != nullptr;
  if (measure) {
    s_bins.clear();
    __syncthreads();
  }
  const unsigned item = W.wg * 4u + wave;
  if (item < W.items) {                          // (uniform in the wave)
    const GatherBand B = gather_band<NS>(W, item, lane);
    const uint32_t rb = W.rb, cells = W.cells, cx = B.cx, off = B.off;
    const bool active = B.active, whole = B.whole;
    const int h = W.h, lastj = B.lastj;          // (cx * NS <= w - 1 in every active lane: band_geometry's cell rule)
    const char *P = W.P, *C = W.C, *N = W.N;
    if (!C) zero_band(W, B);
    else if (P == C || N == C) {                 // an end of the run: the frame passes through, its padding replicating its edge
      for (int y = B.r0; y < B.r1; y++) {
        uint32_t c[4];
        load_cell(C + (size_t)min(y, h - 1) * rb, off, rb, whole, active, c);
        pass_cell<Pix>(W, B, y, c);
      }
    } else {
      const uint32_t kden = kRecipDen[lane < 33 ? lane : 32];
      const bool left_edge = cx == 0, right_edge = lastj <= NS - 1;      // the neighbour column lies beyond the true width: clamped
      // row r: its cells, and the horizontal 3-sums of |C - F| with the columns clamped to the true width
      auto load_row = [&](GrainRow<NP> &R, int r) {
        const size_t ro = (size_t)r * rb;
        load_cell(C + ro, off, rb, whole, active, R.c);
        load_cell(P + ro, off, rb, whole, active, R.p);
        load_cell(N + ro, off, rb, whole, active, R.n);
        uint32_t hc[NP], hf[NP], ap[NP], an[NP];
        halves<Pix, NP>(R.c, hc);
        halves<Pix, NP>(R.p, hf);
#pragma unroll
        for (int q = 0; q < NP; q++) ap[q] = pk_absdiff(hc[q], hf[q]);
        halves<Pix, NP>(R.n, hf);
#pragma unroll
        for (int q = 0; q < NP; q++) an[q] = pk_absdiff(hc[q], hf[q]);
        if (lastj < NS - 1) {                    // the cell reaches into the padding: the last true column's value goes on
          replicate_halves<NP>(ap, lastj);
          replicate_halves<NP>(an, lastj);
        }
        // the neighbours' columns: (P's, N's) in one dword each way.  Every lane of the wave is here
        uint32_t lft = __shfl_up((ap[NP - 1] >> 16) | (an[NP - 1] & 0xffff0000u), 1);
        uint32_t rgt = __shfl_down((ap[0] & 0xffffu) | (an[0] << 16), 1);
        if (lane == 0 && active && cx > 0) {     // the neighbours are another wave's
          const uint32_t c = last_sample<Pix>(*reinterpret_cast<const uint32_t *>(C + ro + off - 4u));
          const uint32_t a = last_sample<Pix>(*reinterpret_cast<const uint32_t *>(P + ro + off - 4u)), b = last_sample<Pix>(*reinterpret_cast<const uint32_t *>(N + ro + off - 4u));
          lft = (c > a ? c - a : a - c) | (c > b ? c - b : b - c) << 16;
        }
        if (lane == 63 && cx + 1 < cells) {
          const uint32_t c = first_sample<Pix>(*reinterpret_cast<const uint32_t *>(C + ro + off + 16u));
          const uint32_t a = first_sample<Pix>(*reinterpret_cast<const uint32_t *>(P + ro + off + 16u)), b = first_sample<Pix>(*reinterpret_cast<const uint32_t *>(N + ro + off + 16u));
          rgt = (c > a ? c - a : a - c) | (c > b ? c - b : b - c) << 16;
        }
        if (left_edge) lft = (ap[0] & 0xffffu) | (an[0] << 16);
        if (right_edge) rgt = (ap[NP - 1] >> 16) | (an[NP - 1] & 0xffff0000u);
        const uint32_t lp = lft << 16, ln = lft & 0xffff0000u, rp = rgt & 0xffffu, rn = rgt >> 16;      // left: in the high half; right: in the low half
#pragma unroll
        for (int q = 0; q < NP; q++) {
          R.hp[q] = ap[q] + __builtin_amdgcn_alignbit(ap[q], q ? ap[q - 1] : lp, 16) + __builtin_amdgcn_alignbit(q + 1 < NP ? ap[q + 1] : rp, ap[q], 16);
          R.hn[q] = an[q] + __builtin_amdgcn_alignbit(an[q], q ? an[q - 1] : ln, 16) + __builtin_amdgcn_alignbit(q + 1 < NP ? an[q + 1] : rn, an[q], 16);
        }
      };

      GrainRow<NP> cur, nxt;
      uint32_t php[NP], phn[NP], out[4] = { 0, 0, 0, 0 };
      GrainLane open;
      int held = -1;
#pragma unroll 1
      for (int y = B.r0; y < B.r1; y++) {
        const int ye = min(y, h - 1);
        if (ye != held) {
          if (held < 0) {                        // the band's first row: cur <- the row above it, nxt <- the row itself
            load_row(cur, max(ye - 1, 0));
            if (ye >= 1) load_row(nxt, ye); else nxt = cur;
          }
#pragma unroll
          for (int q = 0; q < NP; q++) { php[q] = cur.hp[q]; phn[q] = cur.hn[q]; }
          cur = nxt;
          if (ye + 1 <= h - 1) load_row(nxt, ye + 1);      // (else the row below is the row itself: nxt stays)
          held = ye;
          uint32_t cc[NP], pp[NP], nn[NP], o[NS];
          halves<Pix, NP>(cur.c, cc);
          halves<Pix, NP>(cur.p, pp);
          halves<Pix, NP>(cur.n, nn);
#pragma unroll
          for (int j = 0; j < NS; j++) {
            const uint32_t dp = php[j >> 1] + cur.hp[j >> 1] + nxt.hp[j >> 1], dn = phn[j >> 1] + cur.hn[j >> 1] + nxt.hn[j >> 1];      // (both halves; no carry)
            const uint32_t Dp = (dp >> (16 * (j & 1))) & 0xffffu, Dn = (dn >> (16 * (j & 1))) & 0xffffu;
            const uint32_t wp = 16u - __umulhi(16u * min(Dp, G.cut), G.recip), wn = 16u - __umulhi(16u * min(Dn, G.cut), G.recip);
            const uint32_t c = half_of(cc, j), num = 16u * c + wp * half_of(pp, j) + wn * half_of(nn, j);
            const uint32_t k = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((wp + wn) << 2), (int)kden);
            o[j] = (num * k + 32768u) >> 16;
            if (measure && active && y < h && j <= lastj && wp + wn >= 24u) {
              const int b = (int)(o[j] >> G.bin_shift);
              if (b != open.bin) { open.flush(s_bins, wave); open.bin = b; }
              const int r = (int)c - (int)o[j];
              open.acc += (uint32_t)(r * r); open.cnt++;
            }
          }
          pack_cell<Pix, NS>(o, lastj, out);
        }
        store_cell(W.dst + (size_t)y * rb, off, rb, whole, active, out);
      }
      if (measure) open.flush(s_bins, wave);
    }
  }
  if (measure) {
    __syncthreads();
    s_bins.store(G.partials);
  }
}

// grid: segments x 3; the partials of (segment, plane) are those of its workgroups, [first, first + n)
__global__ __launch_bounds__(256) void k_grain_sum(GrainGeom G, av1mi_grain_record *out) {
  __shared__ unsigned long long s_sum[16][16];
  __shared__ uint32_t s_cnt[16][16];
  const unsigned seg = blockIdx.x / 3, p = blockIdx.x - seg * 3;
  const unsigned first = seg * G.per_seg + (p > 0 ? G.wgs[0] : 0) + (p > 1 ? G.wgs[1] : 0), n = G.wgs[p];
  const unsigned b = threadIdx.x & 15u, part = threadIdx.x >> 4;
  unsigned long long sum = 0; uint32_t cnt = 0;
  for (unsigned i = part; i < n; i += 16) {
    const av1mi_grain_bin v = G.partials[(size_t)(first + i) * 16 + b];
    sum += v.sum_sq; cnt += v.count;
  }
  s_sum[part][b] = sum; s_cnt[part][b] = cnt;
  __syncthreads();
  if (threadIdx.x < 16) {
    av1mi_grain_bin o; o.sum_sq = 0; o.count = 0; o.reserved = 0;
    for (int i = 0; i < 16; i++) { o.sum_sq += s_sum[i][b]; o.count += s_cnt[i][b]; }
    out[blockIdx.x].bin[b] = o;
  }
}

namespace {
// the geometry of a launch; hipErrorInvalidValue for what the kernel cannot take
hipError_t grain_geometry(const DenoiseLaunch &L, GrainGeom &G) {
  if (L.strength < 1 || L.strength > 16 || (L.bd != 8 && L.bd != 10)) return hipErrorInvalidValue;
  G.cut = 27u * ((uint32_t)L.strength << (L.bd - 8)); G.recip = (uint32_t)((1ull << 32) / G.cut) + 1u; G.bin_shift = L.bd - 4;
  G.partials = nullptr;
  return band_geometry(L, true, G);
}
}  // namespace

size_t grain_scratch_bytes(const DenoiseLaunch &L) {
  GrainGeom G;
  if (grain_geometry(L, G) != hipSuccess || L.segments <= 0) return 0;
  return (size_t)G.per_seg * L.segments * 16 * sizeof(av1mi_grain_bin);
}

hipError_t launch_denoise_gather(const DenoiseLaunch &L, hipStream_t s) {
  GrainGeom G;
  if (hipError_t e = grain_geometry(L, G)) return e;
  if (L.segments <= 0 || !G.per_seg) return hipSuccess;
  if (L.records && !L.scratch) return hipErrorInvalidValue;
  G.partials = L.records ? (av1mi_grain_bin *)L.scratch : nullptr;
  const dim3 grid(G.per_seg * (unsigned)L.segments);
  if (L.bd == 8) hipLaunchKernelGGL(k_denoise_gather<uint8_t>, grid, dim3(256), 0, s, G, L.table);
  else hipLaunchKernelGGL(k_denoise_gather<uint16_t>, grid, dim3(256), 0, s, G, L.table);
  if (hipError_t e = hipGetLastError()) return e;
  if (L.records) hipLaunchKernelGGL(k_grain_sum, dim3(3u * (unsigned)L.segments), dim3(256), 0, s, G, L.records);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Motion-compensated denoising (include/av1mi.h "motion-compensated denoising"): k_denoise_search gives every 16x16 luma block a vector
// towards P and one towards N; k_denoise_mc_gather stands in k_denoise_gather's place and compares every sample with its DISPLACED
// neighbours.  The partial records and k_grain_sum are the plain gather's.
//
//   search    a wave owns (block, F): the block (zeros beyond its true part) and F's clamped window of (16 + 2 range)^2 samples lie in
//             LDS as whole dwords.  A lane owns a candidate (dy, dx) at a time and walks down the block's rows: the window row's dwords
//             from the candidate's first byte on come through v_alignbyte_b32, the columns beyond the true width are masked to zero on
//             both sides, and v_sad_u8 (four samples) / v_sad_u16 (two) add into ONE 32-bit accumulator (256 x 1023 + the bias < 2^19).
//             The key (cost << 11 | rank) goes through an LDS atomicMin; a workgroup holds two blocks and stores one dword per block.
//   gather    a wave owns a block's samples in ONE plane (16 >> ssx by 16 >> ssy of them, plus the padding beyond the true size at the
//             plane's right and bottom edge: at most 23 x 23), a workgroup four blocks side by side.  C and the displaced P and N of the
//             block's 18 x 18 neighbourhood go to LDS once (coordinates clamped as the definition clamps them), |C - P| and |C - N| as the
//             two halves of a dword, so that D_P and D_N of a sample are nine dword adds (9 x 1023 fits a half).  The output is
//             assembled in LDS and leaves in 16-byte units where the block's row run allows them, in dwords elsewhere.
// Arithmetic restated in numpy by tests/denoise_mc_ref.py.
namespace {
struct McGeom {
  int w0, h0;                  // the luma plane's true size
  int nbx, nby;                // blocks across and down
  uint32_t rb0;                // bytes of a luma row
  uint32_t pairs;              // the search's workgroups per segment: two blocks each
  uint32_t strips;             // the gather's workgroups per block row: four blocks each
  uint32_t t_luma;             // strength << (bit_depth - 8)
  int ssx[3], ssy[3];          // the planes' subsampling against luma
  uint32_t *vectors;           // [segment * blocks + block]: dx_p | dy_p << 8 | dx_n << 16 | dy_n << 24 (av1mi_denoise_vec)
};

template <typename Pix>
__device__ __forceinline__ uint32_t sample_at(const char *plane, uint32_t rb, int x, int y) { return reinterpret_cast<const Pix *>(plane + (size_t)y * rb)[x]; }
__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }
// idx / d for idx * d < 2^16, rcp = 65536 / d + 1 (the error of rcp, at most d / 65536 per unit, cannot reach the next integer)
__device__ __forceinline__ uint32_t div_small(uint32_t idx, uint32_t rcp) { return (idx * rcp) >> 16; }
}  // namespace

// grid: pairs x segments; wave = (block pair * 2 + (wave >> 1), F = wave & 1 ? N : P)
template <typename Pix, int RANGE>
__global__ __launch_bounds__(256) void k_denoise_search(McGeom M, const void *const *table) {
  constexpr int BPS = (int)sizeof(Pix), SPD = 4 / BPS;      // samples per dword
  constexpr int WIN = 16 + 2 * RANGE;                       // the window's rows, and samples per row
  constexpr int WDW = WIN / SPD + 1;                        // dwords of a window row in LDS (+ 1: the funnel's last high dword, zero)
  constexpr int CDW = 16 / SPD;                             // dwords of a block row
  constexpr int SIDE = 2 * RANGE + 1, CAND = SIDE * SIDE, CENTRE = RANGE * SIDE + RANGE;
  __shared__ uint32_t s_win[4][WIN * WDW];
  __shared__ uint32_t s_blk[4][16 * CDW];
  __shared__ uint32_t s_key[4];
  const unsigned seg = blockIdx.x / M.pairs, pair = blockIdx.x - seg * M.pairs;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const unsigned nblk = (unsigned)(M.nbx * M.nby);
  const char *const *tab = reinterpret_cast<const char *const *>(table) + (size_t)seg * 9;      // the luma plane's P, C, N
  const char *P = tab[0], *C = tab[1], *N = tab[2];
  uint32_t *vec = M.vectors + (size_t)seg * nblk;
  if (!C || P == C || N == C) {                  // a flat slot, an end of the run: not searched (uniform in the workgroup)
    if (threadIdx.x < 2 && pair * 2 + threadIdx.x < nblk) vec[pair * 2 + threadIdx.x] = 0;
    return;
  }
  const unsigned blk = pair * 2 + (wave >> 1);
  const bool live = blk < nblk;
  const char *F = (wave & 1) ? N : P;
  const int by = live ? (int)blk / M.nbx : 0, bx = live ? (int)blk - by * M.nbx : 0;
  const int bw = min(16, M.w0 - bx * 16), bh = min(16, M.h0 - by * 16);      // the block's true part
  if (threadIdx.x < 4) s_key[threadIdx.x] = 0xffffffffu;
  if (live) {
    for (int i = (int)lane; i < 16 * CDW; i += 64) {
      const int r = i / CDW, q = i - r * CDW;
      uint32_t d = 0;
      if (r < bh) {
#pragma unroll
        for (int k = 0; k < SPD; k++)
          if (q * SPD + k < bw) d |= sample_at<Pix>(C, M.rb0, bx * 16 + q * SPD + k, by * 16 + r) << (8 * BPS * k);
      }
      s_blk[wave][i] = d;
    }
    for (int i = (int)lane; i < WIN * WDW; i += 64) {
      const int r = i / WDW, q = i - r * WDW;
      uint32_t d = 0;
      if (q < WDW - 1) {
        const int y = clampi(by * 16 - RANGE + r, M.h0 - 1), x = bx * 16 - RANGE + q * SPD;
        d = row_dword(reinterpret_cast<const Pix *>(F + (size_t)y * M.rb0), x, M.w0);
      }
      s_win[wave][i] = d;
    }
  }
  __syncthreads();
  if (live) {
    uint32_t mask[CDW];                          // the block's true columns
#pragma unroll
    for (int q = 0; q < CDW; q++) {
      mask[q] = 0;
#pragma unroll
      for (int k = 0; k < SPD; k++)
        if (q * SPD + k < bw) mask[q] |= (BPS == 1 ? 0xffu : 0xffffu) << (8 * BPS * k);
    }
    const uint32_t bias = ((uint32_t)(bw * bh) * M.t_luma) >> 2;
    uint32_t best = 0xffffffffu;
    for (int c = (int)lane; c < CAND; c += 64) {
      const int dyi = c / SIDE, dxi = c - dyi * SIDE;      // dy + RANGE, dx + RANGE
      const int q0 = (dxi * BPS) >> 2;
      const uint32_t sh = (uint32_t)(dxi * BPS) & 3u;
      uint32_t sad = 0;
#pragma unroll 1
      for (int r = 0; r < bh; r++) {
        const uint32_t *wr = &s_win[wave][(dyi + r) * WDW + q0];
        const uint32_t *br = &s_blk[wave][r * CDW];
        uint32_t lo = wr[0];
#pragma unroll
        for (int q = 0; q < CDW; q++) {
          const uint32_t hi = wr[q + 1];
          const uint32_t f = __builtin_amdgcn_alignbyte(hi, lo, sh) & mask[q];
          if constexpr (BPS == 1) sad = __builtin_amdgcn_sad_u8(br[q], f, sad);
          else sad = __builtin_amdgcn_sad_u16(br[q], f, sad);
          lo = hi;
        }
      }
      const uint32_t rank = c < CENTRE ? (uint32_t)c + 1u : c > CENTRE ? (uint32_t)c : 0u;
      best = min(best, ((sad + (rank ? bias : 0u)) << 11) | rank);
    }
    atomicMin(&s_key[wave], best);
  }
  __syncthreads();
  if (threadIdx.x < 2 && pair * 2 + threadIdx.x < nblk) {
    uint32_t v = 0;
#pragma unroll
    for (int f = 0; f < 2; f++) {
      const int rank = (int)(s_key[threadIdx.x * 2 + f] & 2047u);
      const int c = rank == 0 ? CENTRE : rank <= CENTRE ? rank - 1 : rank;
      const int dy = c / SIDE - RANGE, dx = c - (c / SIDE) * SIDE - RANGE;
      v |= (((uint32_t)dx & 0xffu) | ((uint32_t)dy & 0xffu) << 8) << (16 * f);
    }
    vec[pair * 2 + threadIdx.x] = v;
  }
}

// grid: per_seg x segments; workgroup = (segment, plane, block row, four blocks across), a wave per block
template <typename Pix>
__global__ __launch_bounds__(256) void k_denoise_mc_gather(GrainGeom G, McGeom M, const void *const *table) {
  constexpr int BPS = (int)sizeof(Pix);
  constexpr int TS = 18;                         // the neighbourhood tile's side
  constexpr int RMAX = 23, RS = 32;              // the output region's rows at most, and its row stride in samples (whole 16-byte units)
  __shared__ uint16_t s_c[4][TS * TS], s_p[4][TS * TS], s_n[4][TS * TS];
  __shared__ uint32_t s_a[4][TS * TS];
  __shared__ __attribute__((aligned(16))) Pix s_o[4][RMAX * RS];
  __shared__ GrainBins s_bins;
  const GatherPlane W = gather_plane(G, table);
  const unsigned seg = W.seg, wg = W.wg;
  const uint32_t rb = W.rb;
  const int rows = W.rows, w = W.w, h = W.h;
  const int ssx = W.p == 0 ? M.ssx[0] : W.p == 1 ? M.ssx[1] : M.ssx[2], ssy = W.p == 0 ? M.ssy[0] : W.p == 1 ? M.ssy[1] : M.ssy[2];
  char *dst = W.dst;
  const char *P = W.P, *C = W.C, *N = W.N;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const bool measure = G.partials != nullptr;
  s_bins.clear();                                // (the barrier below stands before the first flush)
  const bool flat = !C, middle = C && P != C && N != C;      // (uniform in the workgroup)
  const int brow = (int)(wg / M.strips), bx = (int)(wg - (unsigned)brow * M.strips) * 4 + (int)wave;
  const bool live = bx < M.nbx;
  const int bwp = 16 >> ssx, bhp = 16 >> ssy;
  const int x0 = bx * bwp, y0 = brow * bhp;
  // the true part tw x th (<= 16 x 16) and the region written rw x rh: the plane's last blocks take its padding with them
  const int tw = live ? min(bwp, w - x0) : 0, th = live ? min(bhp, h - y0) : 0;
  const int rw = live ? (bx == M.nbx - 1 ? (int)(rb / BPS) - x0 : bwp) : 0, rh = live ? (brow == M.nby - 1 ? rows - y0 : bhp) : 0;
  if (live && middle) {
    const uint32_t v = M.vectors[(size_t)seg * (unsigned)(M.nbx * M.nby) + (unsigned)(brow * M.nbx + bx)];
    const int vxp = (int)(int8_t)(v & 0xffu) >> ssx, vyp = (int)(int8_t)((v >> 8) & 0xffu) >> ssy;      // (arithmetic shifts: floor)
    const int vxn = (int)(int8_t)((v >> 16) & 0xffu) >> ssx, vyn = (int)(int8_t)(v >> 24) >> ssy;
    const int ew = tw + 2, n = ew * (th + 2);
    const uint32_t rcp = 65536u / (uint32_t)ew + 1u;
    for (int e = (int)lane; e < n; e += 64) {
      const int j = (int)div_small((uint32_t)e, rcp), i = e - j * ew;
      const int cx = clampi(x0 - 1 + i, w - 1), cy = clampi(y0 - 1 + j, h - 1);
      const uint32_t c = sample_at<Pix>(C, rb, cx, cy);
      const uint32_t a = sample_at<Pix>(P, rb, clampi(cx + vxp, w - 1), clampi(cy + vyp, h - 1)), b = sample_at<Pix>(N, rb, clampi(cx + vxn, w - 1), clampi(cy + vyn, h - 1));
      const int t = j * TS + i;
      s_c[wave][t] = (uint16_t)c; s_p[wave][t] = (uint16_t)a; s_n[wave][t] = (uint16_t)b;
      s_a[wave][t] = (c > a ? c - a : a - c) | (c > b ? c - b : b - c) << 16;
    }
  }
  __syncthreads();
  if (live) {
    const uint32_t kden = kRecipDen[lane < 33 ? lane : 32];
    const uint32_t rcp = 65536u / (uint32_t)rw + 1u;
    const int n = rw * rh;
    GrainLane open;
    for (int e0 = 0; e0 < n; e0 += 64) {         // (every lane of the wave walks the loop: ds_bpermute below reads lanes' registers)
      const int e = min(e0 + (int)lane, n - 1);
      const bool mine = e0 + (int)lane < n;
      const int ry = (int)div_small((uint32_t)e, rcp), rx = e - ry * rw;
      const int tx = min(rx, tw - 1), ty = min(ry, th - 1);      // the padding repeats the true part's edge
      uint32_t o = 0;
      if (middle) {
        const uint32_t *a = &s_a[wave][ty * TS + tx];
        const uint32_t d = a[0] + a[1] + a[2] + a[TS] + a[TS + 1] + a[TS + 2] + a[2 * TS] + a[2 * TS + 1] + a[2 * TS + 2];      // (both halves; no carry)
        const uint32_t Dp = d & 0xffffu, Dn = d >> 16;
        const uint32_t wp = 16u - __umulhi(16u * min(Dp, G.cut), G.recip), wn = 16u - __umulhi(16u * min(Dn, G.cut), G.recip);
        const int t = (ty + 1) * TS + tx + 1;
        const uint32_t c = s_c[wave][t], num = 16u * c + wp * s_p[wave][t] + wn * s_n[wave][t];
        const uint32_t k = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((wp + wn) << 2), (int)kden);
        o = (num * k + 32768u) >> 16;
        if (measure && mine && rx < tw && ry < th && wp + wn >= 24u) {
          const int b = (int)(o >> G.bin_shift);
          if (b != open.bin) { open.flush(s_bins, wave); open.bin = b; }
          const int r = (int)c - (int)o;
          open.acc += (uint32_t)(r * r); open.cnt++;
        }
      } else if (!flat) o = sample_at<Pix>(C, rb, x0 + tx, y0 + ty);      // an end of the run passes through
      if (mine) s_o[wave][ry * RS + rx] = (Pix)o;
    }
    if (measure) open.flush(s_bins, wave);
  }
  __syncthreads();
  if (live) {
    const int rbytes = rw * BPS;                 // of the region's row: whole dwords, as the plane's rows and x0 * BPS are
    const bool wide = !(rb & 15u) && !((x0 * BPS) & 15) && !(rbytes & 15);
    const int units = wide ? rbytes >> 4 : rbytes >> 2, n = units * rh;
    const uint32_t rcp = 65536u / (uint32_t)units + 1u;
    char *at = dst + (size_t)y0 * rb + (size_t)x0 * BPS;
    for (int e = (int)lane; e < n; e += 64) {
      const int ry = (int)div_small((uint32_t)e, rcp), u = e - ry * units;
      const char *from = reinterpret_cast<const char *>(&s_o[wave][ry * RS]);
      if (wide) *reinterpret_cast<uint4 *>(at + (size_t)ry * rb + u * 16) = *reinterpret_cast<const uint4 *>(from + u * 16);
      else *reinterpret_cast<uint32_t *>(at + (size_t)ry * rb + u * 4) = *reinterpret_cast<const uint32_t *>(from + u * 4);
    }
  }
  if (measure) s_bins.store(G.partials);
}

namespace {
// the geometry of the motion-compensated launches: the plain gather's checks, then blocks in place of bands
hipError_t mc_geometry(const DenoiseMcLaunch &L, GrainGeom &G, McGeom &M) {
  if (hipError_t e = grain_geometry(L, G)) return e;
  if ((L.range != 4 && L.range != 8) || L.plane_w[0] <= 0 || L.plane_h[0] <= 0) return hipErrorInvalidValue;
  M.w0 = L.true_w[0]; M.h0 = L.true_h[0]; M.nbx = (M.w0 + 15) / 16; M.nby = (M.h0 + 15) / 16;
  M.rb0 = G.row_bytes[0]; M.pairs = ((uint32_t)(M.nbx * M.nby) + 1) / 2; M.strips = ((uint32_t)M.nbx + 3) / 4;
  M.t_luma = (uint32_t)L.strength << (L.bd - 8); M.vectors = (uint32_t *)L.vectors;
  G.per_seg = 0;
  for (int p = 0; p < 3; p++) {
    const bool have = L.plane_w[p] > 0 && L.plane_h[p] > 0;
    M.ssx[p] = have && L.plane_w[p] < L.plane_w[0]; M.ssy[p] = have && L.plane_h[p] < L.plane_h[0];
    // a chroma plane's true size is the luma plane's, halved upwards where it is subsampled: every block then has samples in it
    if (have && (L.true_w[p] != (M.w0 + M.ssx[p]) >> M.ssx[p] || L.true_h[p] != (M.h0 + M.ssy[p]) >> M.ssy[p])) return hipErrorInvalidValue;
    G.wgs[p] = have ? (uint32_t)M.nby * M.strips : 0;
    G.per_seg += G.wgs[p];
  }
  if (L.segments > 0 && ((size_t)G.per_seg * L.segments > 0x7FFFFFFFu || (size_t)M.pairs * L.segments > 0x7FFFFFFFu)) return hipErrorInvalidValue;
  return hipSuccess;
}
}  // namespace

size_t denoise_mc_scratch_bytes(const DenoiseMcLaunch &L) {
  GrainGeom G; McGeom M;
  if (mc_geometry(L, G, M) != hipSuccess || L.segments <= 0) return 0;
  return (size_t)G.per_seg * L.segments * 16 * sizeof(av1mi_grain_bin);
}
size_t denoise_mc_vector_bytes(const DenoiseMcLaunch &L) {
  GrainGeom G; McGeom M;
  if (mc_geometry(L, G, M) != hipSuccess || L.segments <= 0) return 0;
  return (size_t)M.nbx * M.nby * L.segments * sizeof(av1mi_denoise_vec);
}

hipError_t launch_denoise_mc_gather(const DenoiseMcLaunch &L, hipStream_t s) {
  GrainGeom G; McGeom M;
  if (hipError_t e = mc_geometry(L, G, M)) return e;
  if (L.segments <= 0) return hipSuccess;        // (per_seg > 0: mc_geometry asks for a luma plane)
  if (!L.vectors || (L.records && !L.scratch)) return hipErrorInvalidValue;
  G.partials = L.records ? (av1mi_grain_bin *)L.scratch : nullptr;
  const dim3 search(M.pairs * (unsigned)L.segments), grid(G.per_seg * (unsigned)L.segments);
  if (L.bd == 8 && L.range == 4) hipLaunchKernelGGL((k_denoise_search<uint8_t, 4>), search, dim3(256), 0, s, M, L.table);
  else if (L.bd == 8) hipLaunchKernelGGL((k_denoise_search<uint8_t, 8>), search, dim3(256), 0, s, M, L.table);
  else if (L.range == 4) hipLaunchKernelGGL((k_denoise_search<uint16_t, 4>), search, dim3(256), 0, s, M, L.table);
  else hipLaunchKernelGGL((k_denoise_search<uint16_t, 8>), search, dim3(256), 0, s, M, L.table);
  if (hipError_t e = hipGetLastError()) return e;
  if (L.bd == 8) hipLaunchKernelGGL(k_denoise_mc_gather<uint8_t>, grid, dim3(256), 0, s, G, M, L.table);
  else hipLaunchKernelGGL(k_denoise_mc_gather<uint16_t>, grid, dim3(256), 0, s, G, M, L.table);
  if (hipError_t e = hipGetLastError()) return e;
  if (L.records) hipLaunchKernelGGL(k_grain_sum, dim3(3u * (unsigned)L.segments), dim3(256), 0, s, G, L.records);
  return hipGetLastError();
}

}  // namespace av1mi
