// inter_kernels.hip — the inter (P-frame) block pipeline of BASELINE config 3 as two gfx950 kernels:
//
//   k_me_int     integer motion search.  One workgroup per 64x64 luma tile: source tile and the reference window
//                (tile + search range, coordinates clamped = the spec's edge extension) staged in LDS; one 8x8 block
//                per wave at a time, ONE CANDIDATE VECTOR PER LANE, the 64 source samples broadcast from LDS;
//                (SAD, raster rank) packed into one integer and min-reduced across the wave with xor-shuffles.
//   k_inter_pipe per block, 8 lanes of one wave (8 blocks per wave, no dependency between blocks), seven phases, a function each:
//                1 the block of this group; 2 luma window into LDS; 3 score of the integer vector; 4 half-pel refinement scored
//                with the bilinear filter (= rounded averages, no filter passes); 5 quarter-pel refinement with the real 8-tap
//                sub-pel filter (K4 arithmetic, subpel.hpp); 6 luma and 7 chroma motion compensation + the shared residual tail
//                (K1 + K8 + K2, block_code.hpp), skip flag and final vector.
// Inter blocks only depend on the PREVIOUS frame, so a P frame is embarrassingly parallel; the serial dependency is
// frame-to-frame inside a GOP and the pipeline batches the t-th frames of many segments into one launch.
// HBM traffic per sample (k_inter_pipe): source b + reference window (L2-served after first touch) ~b + reconstruction
// b + levels 2.
//
// Arithmetic: AV1 spec §7.11.3.4 (subpel.hpp, shared with mc_kernels.hip) + §7.13.3 / §7.12.3; search policy is this project's own and
// mirrored by oracle/av1o_pipeline.c:av1o_inter_encode_frame.  Reference tree: nothing (transcode.go:120).
#include "block_code.hpp"
#include "subpel.hpp"

namespace av1mi {

// ------------------------------------------------------------------------------------------ integer search
// The search runs on the 8 most significant bits of the samples (10-bit content is shifted down by 2: encoder policy,
// mirrored by the oracle), which lets one v_qsad_pk_u16_u8 score FOUR horizontally adjacent candidate vectors against
// four source samples at once.  A lane owns (dy, group of 4 dx): per block row it reads 12 reference bytes (three
// aligned dwords) and issues two QSADs with the row's two source dwords, which all lanes read from the same LDS address.
// RC: the search range as a compile-time constant (0 = take L.range at run time): with the default +-8 every quotient, item
// count and validity bound below is a constant.
// CEN: the search runs around a centre per tile and frame (L.centres, the coarse search of me_coarse_kernels.hip; multiples of 4, so
// the window's groups of four stay aligned): the window is staged around tile origin + centre, the displacements d rank as without
// one ((0, 0) = the centre itself first) and the vector written is centre + d.  Without it the kernel is the one it was.
template <typename Pix, int RC, bool CEN>
__global__ __launch_bounds__(256) void k_me_int(InterLaunch L) {
  // window row stride in bytes: 41 dwords.  The window reads are ds_read2_b32 / ds_read_b32 (32 banks per 32-lane group); a lane
  // reads dword (by 8 + 3 dp + r) 41 + 2 bx + g (+ 0, 1, 2): 3 x 41 = 27 mod 32, so the six dy triples of a block start 5 banks
  // apart (0, 27, 22, 17, 12, 7) and their five dx groups fill the gaps: 30 distinct banks.  That holds per BLOCK, so a block's
  // 30 items are padded to 32 (one 32-lane group = one block; 16 x 32 items are the same 8 rounds as 16 x 30).  With 35-dword
  // rows and 30 items per block every group straddled two blocks and two triples shared a bank: SQ_LDS_BANK_CONFLICT was 55 % of
  // the LDS cycles.
  constexpr int MAXR = 16, WS = 164;
  static_assert(WS >= 64 + 2 * MAXR + 4 && WS % 4 == 0, "window row must hold tile + range and be whole dwords");
  __shared__ __attribute__((aligned(16))) uint8_t win[(64 + 2 * MAXR) * WS];
  __shared__ __attribute__((aligned(16))) uint8_t srct[64 * 64];
  __shared__ uint32_t s_best[64];                    // per 8x8 block: min of SAD << 16 | rank
  constexpr int sh = sizeof(Pix) == 1 ? 0 : 2;
  const int tid = threadIdx.x, R = RC ? RC : L.range, R4 = (R + 3) & ~3, NC = 2 * R + 1;
  const int WDX = 64 + 2 * R4 + 4, WDY = 64 + 2 * R + 2;    // window columns start at x - R4 (4-aligned), rows at y - R; two more rows for the unused part of the last dy triple
  const int sbw = (L.w + 63) / 64;
  const Tile3 tl = xcd_tile(sbw, (L.h + 63) / 64, L.nframes);
  const int f = tl.z, sby = tl.y, sbx = tl.x;
  int cx = 0, cy = 0;
  if constexpr (CEN) {      // (uniform in the workgroup: a scalar load of the pair)
    const uint32_t c = reinterpret_cast<const uint32_t *>(L.centres)[(f * ((L.h + 63) / 64) + sby) * sbw + sbx];
    cx = (int16_t)(c & 0xffffu); cy = (int16_t)(c >> 16);
  }
  const Pix *src = reinterpret_cast<const Pix *>(L.src[0]) + (size_t)f * L.h * L.stride_y;
  const Pix *ref = reinterpret_cast<const Pix *>(ref_plane(L, f, 0)) + (size_t)f * L.h * L.stride_y;
  // staging, four samples per lane per step as one dword of their 8-bit views (the window starts on a 4-sample boundary and its width
  // is a multiple of 4)
  const int wg = WDX >> 2;
  for (int i = tid; i < WDY * wg; i += 256) {
    const int r = i / wg, c = (i - r * wg) * 4;
    const int fy = min(max(sby * 64 - R + r + cy, 0), L.h - 1), fx = sbx * 64 - R4 + c + cx;
    *reinterpret_cast<uint32_t *>(win + r * WS + c) = row_dword<Pix, 4>(ref + row_off(fy, L.stride_y), fx, L.w, sh);
  }
  for (int i = tid; i < 64 * 16; i += 256) {
    const int r = i >> 4, c = (i & 15) * 4;
    const int fy = min(sby * 64 + r, L.h - 1), fx = sbx * 64 + c;
    *reinterpret_cast<uint32_t *>(srct + r * 64 + c) = row_dword<Pix, 4>(src + row_off(fy, L.stride_y), fx, L.w, sh);      // (fx >= 0: only the right side ever clamps)
  }
  if (tid < 64) s_best[tid] = 0xFFFFFFFFu;
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const int bw = L.w / 8, bh = L.h / 8;
  const int NG = (2 * R4) / 4 + 1;                 // groups of four dx starting at -R4
  constexpr int HD = 3;                            // vertical displacements per item
  const int NP = (NC + HD - 1) / HD;               // triples of vertical displacements (the last one may hold fewer)
  const int items = NP * NG;                       // (dy triple, dx group) items per block
  const int per = RC == 8 ? 32 : items;            // lanes per block: padded to a 32-lane group when the count is known to be 30
  int16_t *mvs = L.mvs + (size_t)f * bw * bh * 2;
  // A lane scores THREE vertically adjacent displacements of four horizontal ones: they share six of their eight window
  // rows, so ten rows of three dwords and ONE copy of the source block's even rows are read for 24 QSADs (pairs: nine rows and a source
  // copy per 32; the QSADs are half of the kernel's cycles, the reads and the per-item arithmetic the other half, and +-8 is
  // 17 = 6 x 3 - 1 rows: as little padding as pairs).  The 16 blocks of a wave form ONE item space (16 x per): with +-8 a
  // block has 30 items, which alone would leave a 64-lane wave half empty; the per-block minimum is an LDS atomic instead of a
  // wave reduction.
  // item -> (block, dy pair, dx group) by reciprocal multiplication: u < 16 x 144 and (u + 0.5) / per is never closer than
  // 0.5 / per to an integer, far outside float rounding, so the truncation is the exact quotient (an integer division by a
  // run-time divisor is ~25 instructions, and there are two per item)
  const float inv_per = 1.0f / (float)per, inv_ng = 1.0f / (float)NG;
  // what an item (dy triple dp, dx group g) contributes whatever the block: its window offset, the ranks of its 12 displacements
  // (~0 = outside +-R) and whether it holds the zero vector.  With 32 items per block a lane has the SAME item in every round, so
  // all of it is computed once, before the loop (the compiler does not hoist it out of the rounds' conditional bodies by itself).
  struct Item { int off; unsigned rk[HD][4]; unsigned not_zero_item; };
  auto make_item = [&](int t) {
    Item it;
    const int dp = (int)(((float)t + 0.5f) * inv_ng), g = t - __mul24(dp, NG);    // dy = 3 dp - R + {0, 1, 2}, dx0 = -R4 + 4 g
    it.off = __mul24(HD * dp, WS) + 4 * g;
    // rank: (0,0) ranks first (0), the others in raster order (1 + (dy + R) NC + dx + R < 1024); dx_i = 4 g - R4 + i is in range for
    // i in [imin, imax]; row h of the triple exists when 3 dp + h < NC
    const int imin = R4 - R - 4 * g, imax = R4 + R - 4 * g;
    const unsigned rank0 = (unsigned)(__mul24(HD * dp, NC) + 4 * g - R4 + R + 1);
#pragma unroll
    for (int h = 0; h < HD; h++)
#pragma unroll
      for (int i = 0; i < 4; i++)
        it.rk[h][i] = (rank0 + h * NC + i) | (unsigned)(((i - imin) | (imax - i)) >> 31) | (unsigned)((NC - 1 - h - HD * dp) >> 31);
    it.not_zero_item = (dp == R / HD && g == (R4 >> 2)) ? 0u : 0xFFFFFFFFu;     // dy index R = row R % 3 of triple R / 3, dx index R4 = sample 0 of group R4 >> 2
    return it;
  };
  Item fixed = {};
  if constexpr (RC == 8) fixed = make_item(lane & 31);
  for (int u0 = 0; u0 < 16 * per; u0 += 64) {
    const int u = u0 + lane;
    if (u < 16 * per) {
      // (with 32 items per block the item of a lane — its dy triple, dx group, ranks and validity masks — is the same in every round:
      // written so that the compiler sees it and keeps them in registers across the unrolled rounds)
      const int bi = RC == 8 ? (u0 >> 5) + (lane >> 5) : (int)(((float)u + 0.5f) * inv_per), t = RC == 8 ? (lane & 31) : u - __mul24(bi, per), b = wave + 4 * bi;   // (plain products here became 64-bit multiply-adds)
      const int by = b >> 3, bx = b & 7;
      if (t < items && sbx * 8 + bx < bw && sby * 8 + by < bh) {
        const Item it = RC == 8 ? fixed : make_item(t);
        const uint8_t *p = win + __mul24(by * 8, WS) + bx * 8 + it.off;
        const uint8_t *s = srct + (by * 8) * 64 + bx * 8;
        // the SAD runs over the block's EVEN rows (policy; the oracle's block_sad8): half the QSADs, the same vectors on the test clips
        uint2 sr[4];
#pragma unroll
        for (int r = 0; r < 4; r++) sr[r] = *reinterpret_cast<const uint2 *>(s + 2 * r * 64);
        unsigned long long acc[HD] = { 0, 0, 0 };
#pragma unroll
        for (int r = 0; r < 8 + HD - 1; r++) {
          const uint32_t *q = reinterpret_cast<const uint32_t *>(p + r * WS);   // row 3 dp + r <= 2 R + 11: inside the staged window
          // (q1, q2) as a 64-bit operand costs two register moves per row — an even-aligned pair — but reading the row as two overlapping
          // 8-byte pieces instead is slower: +23 % LDS instructions, 0.300 -> 0.311 ms)
          const unsigned long long w01 = (unsigned long long)q[0] | ((unsigned long long)q[1] << 32);
          const unsigned long long w12 = (unsigned long long)q[1] | ((unsigned long long)q[2] << 32);
#pragma unroll
          for (int h = 0; h < HD; h++)
            if (r - h >= 0 && r - h < 8 && ((r - h) & 1) == 0) {
              acc[h] = __builtin_amdgcn_qsad_pk_u16_u8(w01, sr[(r - h) >> 1].x, acc[h]);
              acc[h] = __builtin_amdgcn_qsad_pk_u16_u8(w12, sr[(r - h) >> 1].y, acc[h]);
            }
        }
        // key = SAD << 16 | rank; ties keep the lower rank; a displacement outside +-R has rank ~0, which turns its key into ~0 under
        // the OR.  With the SAD in the upper half a candidate's key is ONE instruction from the packed QSAD result:
        // (word << 16) | rank or (word & 0xFFFF0000) | rank.
        unsigned best = 0xFFFFFFFFu;
#pragma unroll
        for (int h = 0; h < HD; h++) {
          const uint32_t lo = (uint32_t)acc[h], hi = (uint32_t)(acc[h] >> 32);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const uint32_t word = i < 2 ? lo : hi;
            best = min(best, ((i & 1) ? (word & 0xFFFF0000u) : (word << 16)) | it.rk[h][i]);
          }
        }
        {
          const int hz = R % HD;      // the zero vector
          const unsigned sz = (unsigned)(hz == 0 ? acc[0] : hz == 1 ? acc[1] : acc[2]) << 16;
          best = min(best, sz | it.not_zero_item);
        }
        atomicMin(&s_best[b], best);
      }
    }
  }
  __syncthreads();
  if (tid < 64) {
    const int by = tid >> 3, bx = tid & 7;
    const int fbx = sbx * 8 + bx, fby = sby * 8 + by;
    if (fbx < bw && fby < bh) {
      const int rank = s_best[tid] & 0xFFFF;
      const int dy = rank ? (rank - 1) / NC - R : 0, dx = rank ? (rank - 1) % NC - R : 0;
      mvs[((size_t)fby * bw + fbx) * 2] = (int16_t)((cx + dx) * 8);
      mvs[((size_t)fby * bw + fbx) * 2 + 1] = (int16_t)((cy + dy) * 8);
    }
  }
}

// ------------------------------------------------------------------------------------------ refinement + coding
__host__ __device__ constexpr int cmax3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
constexpr int kInterGroups = 32;                 // groups (blocks) per workgroup of k_inter_pipe

// ONE LDS region per group, reused by the phases of a block (each ends with a group sync before the next one writes):
//   luma search     window (YW x YWS samples) | intermediate (16 x 8 int16)
//   luma residual   transpose buffer (8 x 12 int32) over the dead window / intermediate
//   chroma          two windows (CWR x CWS samples) | intermediates (2 x (11 x 4 + 4) int16); then the two transpose buffers
//                   (2 x 32 int32) over the dead windows
// Separate arrays cost 66 KB per workgroup at 10 bits = 2 waves per SIMD; the shared region is 29 KB (912 bytes per block: the luma
// phase sets it since the chroma windows hold 7 rows instead of 12) = the 5 waves per SIMD the VGPRs allow.
template <typename ES> struct InterRegion {
  static constexpr int YW = 16, YWS = 20;        // luma window 16 x 16 (integer vector -4 .. +11); rows are whole dwords
  static constexpr int CW = 12, CWS = 16;        // chroma window columns: chroma integer position -4 .. +7; rows are whole dwords
  static constexpr int CWR0 = 3, CWR = 7;        // ... of which the 4-tap family reads rows 3 .. 9 only: those are stored
  static constexpr int YWIN_BYTES = YW * YWS * (int)sizeof(ES), CWIN_BYTES = 2 * CWR * CWS * (int)sizeof(ES);
  static constexpr int IMY_BYTES = 16 * 8 * 2, IMC_BYTES = 2 * (11 * 4 + 4) * 2, TY_BYTES = 8 * 12 * 4, TC_BYTES = 2 * 32 * 4;
  static constexpr int REG_RAW = cmax3(YWIN_BYTES + IMY_BYTES, CWIN_BYTES + IMC_BYTES, TY_BYTES > TC_BYTES ? TY_BYTES : TC_BYTES);
  // per-group stride = 16 bytes past a multiple of 128: the groups of a wave run in lockstep at equal offsets and so start 4 banks apart
  static constexpr int REG_BYTES = ((REG_RAW + 127) / 128) * 128 + 16;
  static_assert(YWIN_BYTES % 16 == 0 && CWIN_BYTES % 16 == 0, "intermediates and transpose buffers need 16-byte alignment");
  unsigned char *base;                           // of this group's region: 16-byte aligned, which the compiler is told at every use
  __device__ __forceinline__ unsigned char *at(int off) const { return static_cast<unsigned char *>(__builtin_assume_aligned(base, 16)) + off; }
  __device__ __forceinline__ ES *luma_win() const { return reinterpret_cast<ES *>(at(0)); }
  __device__ __forceinline__ int16_t *luma_im() const { return reinterpret_cast<int16_t *>(at(YWIN_BYTES)); }
  __device__ __forceinline__ int32_t *luma_T() const { return reinterpret_cast<int32_t *>(at(0)); }
  // window of chroma plane pl (0 U, 1 V): row r at chroma_win(pl) + r * CWS, rows CWR0 .. CWR0 + CWR - 1 exist
  __device__ __forceinline__ ES *chroma_win(int pl) const { return reinterpret_cast<ES *>(at(0)) + pl * CWR * CWS - CWR0 * CWS; }
  __device__ __forceinline__ int16_t *chroma_im(int pl) const { return reinterpret_cast<int16_t *>(at(CWIN_BYTES)) + pl * (11 * 4 + 4); }
  __device__ __forceinline__ int32_t *chroma_T(int pl) const { return reinterpret_cast<int32_t *>(at(0)) + pl * 32; }
};

// What the phases of one block share.  The chroma planes are not here: lanes 0-3 of a group work on U and 4-7 on V, so their pointers
// are per lane and phase 7 makes them — held from the start they would be six registers through the whole search.
template <typename Pix> struct InterBlock {
  int f, blk, x, y, lane;                        // frame, block of the frame in raster order, its luma origin, lane of the block's 8
  const Pix *src_y, *ref_y;                      // luma planes of frame f
  Pix *rec_y;
  InterRegion<Pix> reg;
  // the block among the blocks of all frames: where its vector and its skip flag are
  __device__ __forceinline__ bool present(const InterLaunch &L) const { return blk < (L.w / 8) * (L.h / 8); }
  __device__ __forceinline__ size_t index(const InterLaunch &L) const { return (size_t)f * (L.w / 8) * (L.h / 8) + blk; }
};

// rows are compared as packed pairs (v_sad_u16: two samples per instruction, both bit depths) and the running best
// prediction is kept packed: four selects per candidate; it is unpacked once after the search
__device__ __forceinline__ void pack_pairs(const int *o, uint32_t *w) {
#pragma unroll
  for (int j = 0; j < 4; j++) w[j] = (uint32_t)o[2 * j] | ((uint32_t)o[2 * j + 1] << 16);
}
__device__ __forceinline__ int block_sad(const uint32_t *sp, const uint32_t *w) {
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) v = __builtin_amdgcn_sad_u16(sp[j], w[j], v);
  return group_sum<8>((int)v);
}
// A 3x3 refinement round picks the minimum of (SAD, rank): candidate k = iy * 3 + ix has rank k + 1, except the centre (k = 4), which
// has rank 0 and so keeps ties — the oracle's raster-order visit with strict improvement.  round_winner: the winning key's offset
// from the centre, each of -1, 0, 1 times `step`.
__device__ __forceinline__ unsigned round_key(int sad, int k) { return ((unsigned)sad << 4) | (unsigned)(k == 4 ? 0 : k + 1); }
__device__ __forceinline__ void round_winner(unsigned key, int step, int &dx, int &dy) {
  const int rk = (int)(key & 15u), kk = rk - 1, wy = (kk * 11) >> 5, wx = kk - 3 * wy;   // kk / 3 for kk in 0..8
  dx = rk ? (wx - 1) * step : 0;
  dy = rk ? (wy - 1) * step : 0;
}

// Phase 1, the block of this group.  No LDS, no memory access but the kernel's arguments; the kernel leaves right after it when
// B.present(L) is false (the groups past the last block in a frame's last workgroup).  The context is filled whole before that test:
// filled on one path only, its members reach the phases merged with "undefined" and the compiler forgets the region's alignment
// (64-bit LDS accesses of the window became pairs of 32-bit ones, 110 instructions more).
// workgroups in XCD-aware order: vertically adjacent block rows (their windows overlap by 8 of 16 rows) share an L2
// frame = a whole number of workgroups (launch_inter_pipe): the frame index is a 32-bit division of the workgroup id — scalar
// code — and the block row a reciprocal multiplication with a one-step correction.  (As blk_all / (bw * bh) in 64 bits and two
// more integer divisions per lane this line was 117 vector instructions, 5 % of the kernel.)
template <typename Pix> __device__ __forceinline__ void inter_block_of_group(const InterLaunch &L, unsigned char *regions, InterBlock<Pix> &B) {
  const int grp = threadIdx.x >> 3, bw = L.w / 8, bh = L.h / 8;
  const unsigned wpf = (unsigned)(bw * bh + kInterGroups - 1) / kInterGroups, wg = xcd_swizzle(blockIdx.x, gridDim.x);
  B.lane = threadIdx.x & 7;
  B.f = (int)(wg / wpf); B.blk = (int)(wg - (unsigned)B.f * wpf) * kInterGroups + grp;
  int by = (int)((float)B.blk * __builtin_amdgcn_rcpf((float)bw)), bx = B.blk - by * bw;       // blk < 2^22: the estimate is within 1
  if (bx < 0) { by--; bx += bw; } else if (bx >= bw) { by++; bx -= bw; }
  B.x = bx * 8; B.y = by * 8;
  B.reg.base = regions + grp * InterRegion<Pix>::REG_BYTES;
  B.src_y = reinterpret_cast<const Pix *>(L.src[0]) + (size_t)B.f * L.h * L.stride_y;
  B.ref_y = reinterpret_cast<const Pix *>(ref_plane(L, B.f, 0)) + (size_t)B.f * L.h * L.stride_y;
  B.rec_y = reinterpret_cast<Pix *>(L.rec[0]) + (size_t)B.f * L.h * L.stride_y;
}

// Phase 2, the luma window: samples (x + imx - 4 .. +11, y + imy - 4 .. +11) around the integer vector (imx, imy) from k_me_int
// (multiples of 8), clamped into the plane; and the block's source row as samples s[] and as pairs sp[].
// Enters with the region free; leaves with the window written and synced.
template <typename Pix>
__device__ __forceinline__ void inter_stage_luma(const InterLaunch &L, const InterBlock<Pix> &B, int &imx, int &imy, int *s, uint32_t *sp) {
  using Reg = InterRegion<Pix>;
  const int16_t *mvs = L.mvs + B.index(L) * 2;
  imx = mvs[0] >> 3; imy = mvs[1] >> 3;
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int r = B.lane + it * 8;
    const int fy = min(max(B.y + imy - 4 + r, 0), L.h - 1);
    stage_window_row<Reg::YW, Pix>(B.ref_y + row_off(fy, L.stride_y), B.x + imx - 4, L.w, B.reg.luma_win() + r * Reg::YWS);
  }
  load_row<8>(B.src_y + row_off(B.y + B.lane, L.stride_y) + B.x, s);
  AV1MI_GROUP_SYNC();
  pack_pairs(s, sp);
}

// Phase 3, candidate 0, the integer vector itself: returns its SAD.  Window synced on entry, only read.
// (phase 0 of the 8-tap filter is the identity: taps 0 0 0 128 0 0 0 0, and (128 p + 4) >> 3 = 16 p, (128 * 16 p + 1024) >> 11
// = p exactly — so the integer position is a copy of the window's centre)
template <typename Pix> __device__ __forceinline__ int inter_score_integer(const InterBlock<Pix> &B, const uint32_t *sp) {
  int bp[8];
  uint32_t w[4];
  row_samples<8, Pix>(B.reg.luma_win() + (B.lane + 4) * InterRegion<Pix>::YWS + 4, 0, bp);
  pack_pairs(bp, w);
  return block_sad(sp, w);
}

// Phase 4, the half-sample round, scored with the BILINEAR filter (encoder policy, mirrored by the oracle; libaom's USE_2_TAPS search):
// at phase 8 its taps are (64, 64), and through the spec's two rounding stages ((s + 4) >> 3, then (s + 1024) >> 11) the
// prediction is EXACTLY the rounded average of the 2 (one direction) or 4 (both) samples around the position.  So this round
// needs no filter passes at all: three window rows of ten samples per lane and adds.  Which half-sample neighbourhood a
// block lies in is decided as well this way as with the 8-tap filter (coded bytes and PSNR unchanged); the
// quarter-sample round scores every position, its centre included, with the real filter.
// centre_sad: phase 3's; (bfx, bfy): the winner in 1/8 samples relative to the integer vector.  Window synced on entry, only read.
template <typename Pix>
__device__ __forceinline__ void inter_half_round(const InterBlock<Pix> &B, const uint32_t *sp, int centre_sad, int &bfx, int &bfy) {
  // packed 16-bit arithmetic (v_pk_add_u16 / v_pk_lshrrev_b16: two samples per lane-op; sums of four 10-bit samples fit):
  // P[j][k][i] = the sample pair at columns 3 + k + 2 i, 4 + k + 2 i of window row lane + 3 + j (block row -1 .. +1, columns
  // -1 + k ..), straight from the window's dwords — the sample-by-sample form unpacked 30 samples, averaged in 32 bits and packed
  // every candidate again for the SAD
  typedef unsigned short v2u __attribute__((ext_vector_type(2)));
  v2u P[3][3][4];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const uint32_t *r32 = reinterpret_cast<const uint32_t *>(B.reg.luma_win() + (B.lane + 3 + j) * InterRegion<Pix>::YWS);
    uint32_t w[3][4];
    if constexpr (sizeof(Pix) == 2) {
      uint32_t D[6];                               // columns 2 .. 13
#pragma unroll
      for (int i = 0; i < 6; i++) D[i] = r32[1 + i];
#pragma unroll
      for (int i = 0; i < 4; i++) { w[0][i] = __builtin_amdgcn_alignbit(D[i + 1], D[i], 16); w[1][i] = D[i + 1]; w[2][i] = __builtin_amdgcn_alignbit(D[i + 2], D[i + 1], 16); }
    } else {
      const uint32_t B0 = r32[0], B1 = r32[1], B2 = r32[2], B3 = r32[3];     // columns 0 .. 15, one byte each
      w[0][0] = __builtin_amdgcn_perm(B1, B0, 0x0c040c03u); w[0][1] = __builtin_amdgcn_perm(0u, B1, 0x0c020c01u);
      w[0][2] = __builtin_amdgcn_perm(B2, B1, 0x0c040c03u); w[0][3] = __builtin_amdgcn_perm(0u, B2, 0x0c020c01u);
      w[1][0] = __builtin_amdgcn_perm(0u, B1, 0x0c010c00u); w[1][1] = __builtin_amdgcn_perm(0u, B1, 0x0c030c02u);
      w[1][2] = __builtin_amdgcn_perm(0u, B2, 0x0c010c00u); w[1][3] = __builtin_amdgcn_perm(0u, B2, 0x0c030c02u);
      w[2][0] = w[0][1]; w[2][1] = w[0][2]; w[2][2] = w[0][3]; w[2][3] = __builtin_amdgcn_perm(B3, B2, 0x0c040c03u);
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int i = 0; i < 4; i++) P[j][k][i] = __builtin_bit_cast(v2u, w[k][i]);
  }
  v2u H[3][2][4];                                // horizontal pair sums: columns (k, k + 1) of row j
#pragma unroll
  for (int j = 0; j < 3; j++)
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int i = 0; i < 4; i++) H[j][k][i] = P[j][k][i] + P[j][k + 1][i];
  const v2u one = { 1, 1 }, two = { 2, 2 };
  unsigned bestkey = round_key(centre_sad, 4);
#pragma unroll
  for (int iy = 0; iy < 3; iy++) {
#pragma unroll
    for (int ix = 0; ix < 3; ix++) {
      if (ix == 1 && iy == 1) continue;
      const int r0 = iy == 0 ? 0 : 1, r1 = iy == 2 ? 2 : 1, k = ix == 0 ? 0 : 1;   // the 1, 2 or 4 samples averaged
      uint32_t ow[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        v2u o;
        if (iy == 1) o = (H[1][k][i] + one) >> one;
        else if (ix == 1) o = (P[r0][1][i] + P[r1][1][i] + one) >> one;
        else o = (H[r0][k][i] + H[r1][k][i] + two) >> two;
        ow[i] = __builtin_bit_cast(uint32_t, o);
      }
      bestkey = min(bestkey, round_key(block_sad(sp, ow), iy * 3 + ix));
    }
  }
  round_winner(bestkey, 4, bfx, bfy);
}

// Phase 5, the quarter-sample round with the real 8-tap filter: the centre (bfx, bfy) (re-scored: rank 0) and its 8 neighbours, column
// by column, one horizontal pass per column.  Every position goes through the same (key, prediction) update, so the order of
// evaluation does not matter.  (bfx, bfy) becomes the winner and bpp its prediction row, packed.  filt: the kernel's tables in LDS.
// Enters with the window synced and the intermediate free; a column is pass, sync, reads, sync, so it leaves the region free.
template <typename Pix>
__device__ __forceinline__ void inter_quarter_round(const InterBlock<Pix> &B, const int16_t (*filt)[16][8], const uint32_t *sp, int &bfx, int &bfy,
                                                    uint32_t *bpp) {
  constexpr int step = 2, bd = sizeof(Pix) == 1 ? 8 : 10;
  const int cx = bfx, cy = bfy;
  int16_t *im = B.reg.luma_im();
  unsigned bestkey = 0xFFFFFFFFu;
#pragma unroll 1
  for (int ix = 0; ix < 3; ix++) {
    const int fx = cx + (ix - 1) * step;
    mc_h16<Pix>(B.reg.luma_win(), InterRegion<Pix>::YWS, im, B.lane, fx * 2, sizeof(Pix) == 2 ? filt[2] : filt[0]);
    AV1MI_GROUP_SYNC();
    uint32_t pr[4][8];
    mc_rows7(im, B.lane, pr);
#pragma unroll
    for (int iy = 0; iy < 3; iy++) {     // unrolled: the three vertical candidates of a column overlap
      const int fy = cy + (iy - 1) * step;
      uint32_t ow[4];
      mc_v7(pr, fy * 2, filt[2], bd, ow);
      const unsigned key = round_key(block_sad(sp, ow), iy * 3 + ix);
      const bool better = key < bestkey;
      bestkey = min(bestkey, key);
#pragma unroll
      for (int j = 0; j < 4; j++) bpp[j] = better ? ow[j] : bpp[j];
    }
    AV1MI_GROUP_SYNC();
  }
  round_winner(bestkey, step, bfx, bfy);
  bfx += cx; bfy += cy;
}

// Phase 6, luma: the final vector (1/8 luma samples) written, the residual of source row s[] against prediction row bpp coded
// (levels, reconstruction stored).  Returns non-zero when the row holds a level.  The transpose buffer lies over window and
// intermediate: enters with the region free, leaves it read but NOT synced.
template <typename Pix>
__device__ __forceinline__ int inter_code_luma(const InterLaunch &L, const InterBlock<Pix> &B, const int *s, const uint32_t *bpp, int mvx, int mvy) {
  int bp[8], rec[8];
#pragma unroll
  for (int j = 0; j < 4; j++) { bp[2 * j] = bpp[j] & 0xffff; bp[2 * j + 1] = bpp[j] >> 16; }
  int16_t *mvs = L.mvs + B.index(L) * 2;
  if (B.lane == 0) { mvs[0] = (int16_t)mvx; mvs[1] = (int16_t)mvy; }
  const int nz = code_residual<8, Pix, false, kAcRoundInter>(B.reg.luma_T(), B.lane, s, bp, L.dc_q, L.ac_q, L.dc_quant, L.ac_quant,
                                                             L.lev[0] + (size_t)B.f * L.w * L.h + (size_t)B.blk * 64 + B.lane * 8, rec);
  store_row<8>(B.rec_y + row_off(B.y + B.lane, L.stride_y) + B.x, rec);
  return nz;
}

// Phase 7, chroma: lanes 0-3 code the U block, lanes 4-7 the V block (4x4 each, 4-tap regular filter rows `filt4`): two 7-row windows
// staged, mc_row, residual, store.  The vector in 1/16 chroma samples is the luma vector in 1/8 luma samples.
// Enters with the luma transpose buffer read but not synced (its first act is that sync); leaves the chroma buffers read.
template <typename Pix>
__device__ __forceinline__ int inter_code_chroma(const InterLaunch &L, const InterBlock<Pix> &B, const int16_t (*filt4)[8], int mvx, int mvy) {
  using Reg = InterRegion<Pix>;
  constexpr int bd = sizeof(Pix) == 1 ? 8 : 10;
  const int pl = B.lane >> 2, cl = B.lane & 3;
  const int cw = L.w / 2, chh = L.h / 2, cx0 = B.x / 2, cy0 = B.y / 2;
  const Pix *src_c = reinterpret_cast<const Pix *>(L.src[1 + pl]) + (size_t)B.f * chh * L.stride_uv;
  const Pix *ref_c = reinterpret_cast<const Pix *>(ref_plane(L, B.f, 1 + pl)) + (size_t)B.f * chh * L.stride_uv;
  Pix *rec_c = reinterpret_cast<Pix *>(L.rec[1 + pl]) + (size_t)B.f * chh * L.stride_uv;
  const int cix = mvx >> 4, ciy = mvy >> 4;         // integer chroma displacement (floor)
  Pix *wc = B.reg.chroma_win(pl);
  AV1MI_GROUP_SYNC();                               // the luma transpose buffer has been read: the region is free
  // the 4-tap family reads window rows 3 .. 9 only (mc_row<4, ES, 2, 6>: taps 2 .. 5 of rows -1 .. +5 around the block)
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int r = 3 + cl + it * 4;
    if (r <= 9) {
      const int fy = min(max(cy0 + ciy - 4 + r, 0), chh - 1);
      stage_window_row<Reg::CW, Pix>(ref_c + row_off(fy, L.stride_uv), cx0 + cix - 4, cw, wc + r * Reg::CWS);
    }
  }
  int sc[4], pc[4], rc[4];
  load_row<4>(src_c + row_off(cy0 + cl, L.stride_uv) + cx0, sc);
  AV1MI_GROUP_SYNC();
  mc_row<4, Pix, 2, 6>(wc, Reg::CWS, B.reg.chroma_im(pl), cl, mvx & 15, mvy & 15, filt4, bd, pc);
  const int nz = code_residual<4, Pix, false, kAcRoundInter>(B.reg.chroma_T(pl), cl, sc, pc, L.dc_q, L.ac_q, L.dc_quant, L.ac_quant,
                                                             L.lev[1 + pl] + (size_t)B.f * cw * chh + (size_t)B.blk * 16 + cl * 4, rc);
  store_row<4>(rec_c + row_off(cy0 + cl, L.stride_uv) + cx0, rc);
  return nz;
}

template <typename Pix>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_inter_pipe(InterLaunch L) {
  __shared__ __attribute__((aligned(16))) unsigned char regions[kInterGroups * InterRegion<Pix>::REG_BYTES];
  // the two filter families this policy uses, copied next to the windows: a lane's taps depend on its block's vector, and a
  // per-lane indexed read of __constant__ memory is a vector memory load (hundreds of cycles) in front of every candidate
  __shared__ __attribute__((aligned(16))) int16_t s_filt[3][16][8];   // regular 8-tap, regular 4-tap, regular 8-tap x 32 (mc_h16 at 10 bits, mc_v7)
  if (threadIdx.x < 128) {
    const int t = threadIdx.x;
    reinterpret_cast<uint32_t *>(s_filt)[t] = reinterpret_cast<const uint32_t *>(kSubpel[t < 64 ? 0 : 4])[t & 63];
    s_filt[2][t >> 3][t & 7] = (int16_t)(kSubpel[0][t >> 3][t & 7] * 32);
  }
  __syncthreads();
  InterBlock<Pix> B;
  inter_block_of_group(L, regions, B);                               // 1
  if (!B.present(L)) return;
  int s[8], imx, imy, bfx, bfy;
  uint32_t sp[4], bpp[4];
  inter_stage_luma(L, B, imx, imy, s, sp);                           // 2
  const int sad0 = inter_score_integer(B, sp);                       // 3
  inter_half_round(B, sp, sad0, bfx, bfy);                           // 4
  inter_quarter_round(B, s_filt, sp, bfx, bfy, bpp);                 // 5
  const int mvx = imx * 8 + bfx, mvy = imy * 8 + bfy;                // final vector, 1/8 luma samples
  int nz = inter_code_luma(L, B, s, bpp, mvx, mvy);                  // 6
  nz |= inter_code_chroma(L, B, s_filt[1], mvx, mvy);                // 7
  nz = group_or<8>(nz);
  if (B.lane == 0) L.skip[B.index(L)] = nz == 0;
}

// integer search: writes L.mvs (whole-sample vectors), which k_inter_pipe then refines
hipError_t launch_me_int(const InterLaunch &L, hipStream_t s) {
  if (L.nframes <= 0) return hipSuccess;
  const int sbs = ((L.w + 63) / 64) * ((L.h + 63) / 64);
  const dim3 g1((unsigned)(sbs * L.nframes));   // 1-D: the kernel orders the tiles (xcd_tile)
  // the instantiation by (bit depth, range known at compile time, centres given)
  using Kernel = void (*)(InterLaunch);
  static const Kernel kernels[2][2][2] = { { { k_me_int<uint8_t, 0, false>, k_me_int<uint8_t, 0, true> }, { k_me_int<uint8_t, 8, false>, k_me_int<uint8_t, 8, true> } },
                                           { { k_me_int<uint16_t, 0, false>, k_me_int<uint16_t, 0, true> }, { k_me_int<uint16_t, 8, false>, k_me_int<uint16_t, 8, true> } } };
  hipLaunchKernelGGL(kernels[L.bd != 8][L.range == 8][L.centres != nullptr], g1, dim3(256), 0, s, L);
  return hipGetLastError();
}
hipError_t launch_inter_pipe(const InterLaunch &L, hipStream_t s) {
  if (L.nframes <= 0) return hipSuccess;
  const long long wpf = ((long long)(L.w / 8) * (L.h / 8) + 31) / 32;       // workgroups per frame (32 blocks each)
  const dim3 g2((unsigned)(wpf * L.nframes));
  if (L.bd == 8) hipLaunchKernelGGL(k_inter_pipe<uint8_t>, g2, dim3(256), 0, s, L);
  else hipLaunchKernelGGL(k_inter_pipe<uint16_t>, g2, dim3(256), 0, s, L);
  return hipGetLastError();
}

}  // namespace av1mi
