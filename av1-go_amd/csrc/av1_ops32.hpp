// av1_ops32.hpp — the tile syntax of KEY FRAMES IN 32x32 BLOCKS (av1mi_gop_config.key_block_size = 32) as the same op
// stream av1_ops.hpp makes of 8x8 blocks: list words + grouped entries, after which the chains, the range coder and the gather of
// av1_entropy_kernels.hip (and their CPU twins) run unchanged.  A tile is one complete 64x64 superblock: PARTITION_SPLIT, four 32x32
// blocks (PARTITION_NONE), luma transform 32x32 (DCT_DCT, not coded: the 32x32 set holds nothing else), chroma 16x16 with the transform
// type implied by the mode, TX_MODE_LARGEST.
// ONE WAVE OF 64 LANES PER TILE, THE UNIT OF PARALLEL WORK A SCAN RANGE OF A TRANSFORM BLOCK (tok_tile32): the tile's levels are read
// once, by all lanes, into four-bit magnitude maps; every context of coeffs() is a function of that map alone (av1_ops.hpp
// tok_coeffs_pass1 / _pass2), so lane j tokenizes 16 luma or 4 chroma scan positions of the transform block at hand and only the PLACE of
// its output — in the list, and in each CDF slot's entries in decoding order — is computed across the lanes.  Nothing is written to
// memory but the list and the entries themselves.
// The syntax this band shares with the 8x8 one (restoration, key-frame modes, coefficients) is av1_ops.hpp's, with this band's slot
// set (kSlots32); here: the slots, the 16x16 / 32x32 scan tables and magnitude map, the sinks and the tile's order.
// Shared source: hipcc runs it across a wave, g++ as a loop over the lanes (the CPU twin, host/av1_opstream.cpp), verified there byte
// for byte against the general block writer (host/av1_blockstream.cpp, itself verified by dav1d).
#pragma once
#include "av1_ops.hpp"

namespace av1ops {

enum SlotK32 : int {
  K_SKIP = 0,                    // context 0 (key frames code skip = 0)
  K_PART32 = 1,                  // context 0: the neighbours inside the tile are 32x32 blocks too
  K_PART64 = 2,                  // context 0: nothing of the tile lies above or to the left of a superblock
  K_USE_WIENER = 3,
  K_TXB_SKIP_Y = 4,              // all_zero, luma: context 0 (the transform covers the block)
  K_TXB_SKIP_C = 5,              // [3] chroma: contexts 7, 8, 9
  K_EOB_Y = 8,                   // eob_pt_1024
  K_EOB_C = 9,                   // eob_pt_256
  K_EOBX_Y = 10,                 // [9] eob_extra
  K_EOBX_C = 19,                 // [7]
  K_DC_SIGN_Y = 26,              // [3]
  K_DC_SIGN_C = 29,              // [3]
  K_BASE_EOB_Y = 32,             // [4]
  K_BASE_EOB_C = 36,             // [4]
  K_BASE_Y = 40,                 // [26]
  K_BASE_C = 66,                 // [26]
  K_BR_Y = 92,                   // [21]
  K_BR_C = 113,                  // [21]
  K_KF_Y_MODE = 134,             // [5][5]
  K_UV_MODE = 159,               // [13] chroma-from-luma allowed (blocks up to 32x32)
  K_ANGLE = 172,                 // [8]
  K_END = 180
};
static_assert((int)K_END <= (int)S_MAX, "the slot arrays of the coder are sized by S_MAX");

constexpr BandSlots kSlots32 = { K_USE_WIENER, K_KF_Y_MODE, K_UV_MODE, K_ANGLE, K_TXB_SKIP_Y, K_TXB_SKIP_C, K_EOB_Y, K_EOB_C, K_EOBX_Y, K_EOBX_C,
                                 K_DC_SIGN_Y, K_DC_SIGN_C, K_BASE_EOB_Y, K_BASE_EOB_C, K_BASE_Y, K_BASE_C, K_BR_Y, K_BR_C, 11, 9 };

AV1_HD int slot_nsym_k32(int s) {
  if (const int n = coeff_nsym<kSlots32>(s)) return n;
  if (s == K_SKIP || s == K_USE_WIENER) return 2;
  if (s < K_KF_Y_MODE) return 10;
  if (s < K_UV_MODE) return 13;
  if (s < K_ANGLE) return 14;
  return 7;
}

// Default_Scan_16x16 / Default_Scan_32x32 (zig-zag: odd diagonals downwards): the scan index of a position has a closed form (the
// diagonals before its own, then its place on the diagonal); the other direction is a table
template <int N> AV1_HD int scan_index32(int pos) {
  const int r = pos / N, c = pos % N, d = r + c;
  const int before = d < N ? d * (d + 1) / 2 : N * N - (2 * N - 1 - d) * (2 * N - d) / 2;
  const int rmin = imax(0, d - N + 1), rmax = imin(d, N - 1);
  return before + ((d & 1) ? r - rmin : rmax - r);
}
struct ScanTables32 { uint16_t s32[1024]; uint8_t s16[256]; };
// thread `tid` of `nthreads` fills its share
AV1_HD void fill_scan_tables32(ScanTables32 *t, int tid = 0, int nthreads = 1) {
  for (int pos = tid; pos < 1024; pos += nthreads) t->s32[scan_index32<32>(pos)] = (uint16_t)pos;
  for (int pos = tid; pos < 256; pos += nthreads) t->s16[scan_index32<16>(pos)] = (uint8_t)pos;
}
// a transform block's magnitude map: min(|level|, 15), FOUR BITS each, rows of 32 + 4 entries (18 bytes), N + 2 rows (the context
// templates reach two rows / columns beyond a level), then one sign bit per level
enum { kMag32Stride = 36 };
template <int N> struct Mag32 { enum { kNibbleBytes = (N + 2) * kMag32Stride / 2, kBytes = kNibbleBytes + N * N / 8 }; };      // 740 (N = 32), 356 (N = 16)
static_assert(Mag32<32>::kBytes % 4 == 0 && Mag32<16>::kBytes % 4 == 0, "maps follow each other on dwords");
struct TokScratch32 { uint8_t *mag; const ScanTables32 *scan; };

#if defined(__HIP_DEVICE_COMPILE__)
#define AV1_SHARED_ADD(p, v) atomicAdd(p, v)
#define AV1_SHARED_MAX(p, v) atomicMax(p, v)
#else       // the twin's lanes run one after the other
#define AV1_SHARED_ADD(p, v) (*(p) += (v))
#define AV1_SHARED_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#endif

// the magnitude map of av1_ops.hpp for N = 16, 32, loaded by many lanes: load8 takes eight levels (the map is zero beforehand)
template <int N> struct MagMap<N, false> {
  enum { LG = N == 16 ? 4 : 5, MS = kMag32Stride };
  uint8_t *mag, *sgn;
  const ScanTables32 *scan;
  AV1_HD MagMap(const TokScratch32 &ts) : mag(ts.mag), sgn(ts.mag + Mag32<N>::kNibbleBytes), scan(ts.scan) {}
  // levels [8 r, 8 r + 8) into the map; returns 1 + the highest scan index of a non-zero level among them (0: none), adds their sum to *cul
  AV1_HD int load8(const int16_t *lev, int r, int *cul) {
    struct alignas(16) L8 { int16_t v[8]; } q = *reinterpret_cast<const L8 *>(lev + 8 * r);
    unsigned packed = 0, signs = 0;
    int eob = 0, sum = 0;
    for (int j = 0; j < 8; j++) {
      const int v = q.v[j], a = iabs(v);
      if (v) eob = imax(eob, scan_index32<N>(8 * r + j) + 1);
      sum += a;
      packed |= (unsigned)(a > 15 ? 15 : a) << (4 * j);
      signs |= (unsigned)(v < 0) << j;
    }
    if (!sum) return 0;
    // eight levels of one row, from an even column on: two 16-bit stores (a row of 18 bytes starts on an even address only)
    const int at = (((8 * r) >> LG) * MS + ((8 * r) & (N - 1))) >> 1;
    *reinterpret_cast<u16a *>(mag + at) = (uint16_t)packed;
    *reinterpret_cast<u16a *>(mag + at + 2) = (uint16_t)(packed >> 16);
    sgn[r] = (uint8_t)signs;
    *cul += sum;
    return eob;
  }
  AV1_HD int pos(int c) const { return N == 16 ? (int)scan->s16[c] : (int)scan->s32[c]; }
  AV1_HD int at(int i) const { return (mag[i >> 1] >> ((i & 1) << 2)) & 15; }
  AV1_HD int neg(int p) const { return (sgn[p >> 3] >> (p & 7)) & 1; }
};

// ------------------------------------------------------------------------------------------------ the tile's wave
// tok_tile32 is written against a WAVE W of kLanes32 lanes:
//   W::Var<T>            a value per lane that lives across phases (a register on the GPU, an array in the twin); v[lane]
//   w.each(f)            f(lane) for every lane, then a barrier: what a phase wrote to the tile's memory is visible to the next
//   w.scan(v) -> total   v[lane] becomes the sum of the lanes before it
//   w.first(v)           lane 0's value, to all
//   w.ballot(v) -> mask  bit `lane` = v[lane] != 0 (64 bits)
// Values that are the same in every lane (what scan and first return, what is read from the tile's memory after a barrier) are
// plain variables.
enum { kLanes32 = 64, kBlocks32 = 4, kTile32MagBytes = kBlocks32 * (Mag32<32>::kBytes + 2 * Mag32<16>::kBytes) };
template <class T, int kStore> struct LaneVar {
  T v[kStore];
  AV1_HD T &operator[](int lane) { return v[kStore == 1 ? 0 : lane]; }
};
// PASS 1 of a transform block takes one ROUND: the lanes hold consecutive ranges of its scan positions, highest first.  The symbols of
// a round fall into 51 slots (base_eob, base, br of the plane); a lane counts its own per slot (bytes: at most 16 x 4 of a slot), a
// prefix over the lanes per slot + the slot's running position in the tile gives each lane its places in the grouped entries (16 bits,
// written over the counts), and the lanes tokenize their ranges a second time, now writing.
enum { kRoundSlots = 4 + 26 + 21, kRoundStride = 33 };      // a slot's row: 64 byte counts, then 64 16-bit positions in their place; 33 dwords: rows on different banks
AV1_HD int round_slot(int slot, bool chroma) {
  const int be = chroma ? K_BASE_EOB_C : K_BASE_EOB_Y, ba = chroma ? K_BASE_C : K_BASE_Y, br = chroma ? K_BR_C : K_BR_Y;
  return slot >= br ? 30 + slot - br : slot >= ba ? 4 + slot - ba : slot - be;
}
AV1_HD int round_slot_global(int rs, bool chroma) {
  const int be = chroma ? K_BASE_EOB_C : K_BASE_EOB_Y, ba = chroma ? K_BASE_C : K_BASE_Y, br = chroma ? K_BR_C : K_BR_Y;
  return rs >= 30 ? br + rs - 30 : rs >= 4 ? ba + rs - 4 : be + rs;
}
struct RoundCounts { uint32_t w[kLanes32 / 4]; };

// what a tile's wave keeps in LDS (the twin: in memory): 15.7 KB
struct Tile32Mem {
  ScanTables32 scan;
  alignas(16) uint8_t mag[kTile32MagBytes];       // per block: luma, U, V
  uint32_t round[kRoundSlots * kRoundStride];
  uint32_t run[K_END];                            // per slot: first its symbols in the tile, then the place of its next entry
  int eob[kBlocks32 * 3], cul[kBlocks32 * 3];     // per transform block: 1 + the last non-zero level's scan index, sum |level|
};
AV1_HD TokScratch32 tile_scratch32(Tile32Mem &S, int b, int p) {
  return { S.mag + b * (Mag32<32>::kBytes + 2 * Mag32<16>::kBytes) + (p ? Mag32<32>::kBytes + (p - 1) * Mag32<16>::kBytes : 0), &S.scan };
}

// the sinks of the syntax (sym / split / lit, as av1_ops.hpp's Sink).  A literal of more than 11 bits is several list words.
AV1_HD int lit_words(int nbits) { return (nbits + 10) / 11; }
template <class F> AV1_HD void lit_pieces(unsigned v, int nbits, F put) {
  while (nbits > 11) { nbits -= 11; put(op_lit(11, (v >> nbits) & 0x7FFu)); }
  if (nbits > 0) put(op_lit(nbits, v & ((1u << nbits) - 1u)));
}
struct WordSink32 {              // list words only
  int n;
  AV1_HD void sym(int, int) { n++; }
  AV1_HD void lit(unsigned, int nbits) { n += lit_words(nbits); }
};
struct TotalSink32 {             // + the tile's symbols per slot (all lanes add to the same counters)
  uint32_t *tot; int n;
  AV1_HD void sym(int slot, int) { AV1_SHARED_ADD(&tot[slot], 1u); n++; }
  AV1_HD void split(int, int slot) { sym(slot, 0); }
  AV1_HD void lit(unsigned, int nbits) { n += lit_words(nbits); }
};
struct CountSink32 {             // a round's counts: the lane's column of bytes
  uint8_t *col; bool chroma; int n;
  AV1_HD void sym(int slot, int) { col[round_slot(slot, chroma) * (kRoundStride * 4)]++; n++; }
  AV1_HD void lit(unsigned, int nbits) { n += lit_words(nbits); }
};
struct EmitSink32 {              // a round's output: the lane's column of positions
  u16a *col; bool chroma; int n; op_t *list; uint32_t *grouped;
  AV1_HD void sym(int slot, int s) { u16a &p = col[round_slot(slot, chroma) * (kRoundStride * 2)]; grouped[p] = ((uint32_t)n << 4) | (uint32_t)s; p++; n++; }
  AV1_HD void lit(unsigned v, int nbits) { lit_pieces(v, nbits, [&](op_t o) { list[n++] = o; }); }
};
struct DirectSink32 {            // output of the one lane that is alone with its slots: the slots' running positions themselves
  uint32_t *run; int n; op_t *list; uint32_t *grouped;
  AV1_HD void sym(int slot, int s) { grouped[run[slot]++] = ((uint32_t)n << 4) | (uint32_t)s; n++; }
  AV1_HD void split(int kind, int slot) { sym(slot, kind ? kSplitVert : kSplitHorz); }      // split_or_horz / split_or_vert = 1 at a frame edge
  AV1_HD void lit(unsigned v, int nbits) { lit_pieces(v, nbits, [&](op_t o) { list[n++] = o; }); }
};

AV1_HD long block_index32(const FrameView &f, int sbr, int sbc, int b) { return (long)(sbr * 2 + (b >> 1)) * (f.w8 / 4) + sbc * 2 + (b & 1); }

// what precedes the coefficients of block b (0..3, raster = decoding order) of the tile = superblock (sbr, sbc).  f.y_mode / f.uv_mode:
// the band's modes, one per 32x32 block in raster order (w8 / 4 per row); f.lev_*: block-contiguous over the same grid (1024 luma,
// 256 + 256 chroma levels per block)
template <class K> AV1_HD void tok_block32_head(const FrameView &f, K &k, int sbr, int sbc, int b, bool half) {
  const int w32 = f.w8 / 4, by = b >> 1, bx = b & 1;
  const long i = block_index32(f, sbr, sbc, b);
  if (b == 0) {
    tok_lr<kSlots32>(f, k, sbr, sbc);
    if (half) k.split(1, K_PART64);              // no room for a 64-wide block: split_or_vert = 1 (the band's rows are always complete)
    else k.sym(K_PART64, 3);                     // PARTITION_SPLIT
  }
  k.sym(K_PART32, 0);                            // PARTITION_NONE
  k.sym(K_SKIP, 0);
  if (b == 0 && f.cdef_bits) k.lit(cdef_index(f, sbr, sbc), f.cdef_bits);      // read_cdef: with the tile's first block (key frames: skip = 0)
  tok_kf_modes<kSlots32>(k, f.y_mode[i], f.uv_mode[i], by ? f.y_mode[i - w32] : 0, bx ? f.y_mode[i - 1] : 0);
}
// what the neighbours of a transform block read of it: min(63, sum |level|) and the DC's sign class (0 none / 1 negative / 2 positive)
AV1_HD void tile_sum32(Tile32Mem &S, int b, int p, int *cul, int *dc) {
  const TokScratch32 ts = tile_scratch32(S, b, p);
  *cul = imin(S.cul[b * 3 + p], 63);
  *dc = (ts.mag[0] & 15) ? ((ts.mag[p ? (int)Mag32<16>::kNibbleBytes : (int)Mag32<32>::kNibbleBytes] & 1) ? 1 : 2) : 0;
}
struct TbCtx32 { int ac, ad, lc, ld; };
AV1_HD TbCtx32 tile_ctx32(Tile32Mem &S, int b, int p) {
  TbCtx32 c = { 0, 0, 0, 0 };
  if (b >> 1) tile_sum32(S, b - 2, p, &c.ac, &c.ad);
  if (b & 1) tile_sum32(S, b - 1, p, &c.lc, &c.ld);
  return c;
}
// the leading symbols of plane p of block b, after the block's head when the plane is the first: the lane that opens the round
template <int N, class K> AV1_HD void tok_tb32_open(const FrameView &f, K &k, Tile32Mem &S, int sbr, int sbc, int b, int p, bool half) {
  if (p == 0) tok_block32_head(f, k, sbr, sbc, b, half);
  const TbCtx32 c = tile_ctx32(S, b, p);
  tok_coeffs_lead<N, kSlots32>(k, p != 0, S.eob[b * 3 + p], c.ac, c.ad, c.lc, c.ld, -1, 0);      // DCT_DCT is the only 32x32 type; chroma: implied
}
AV1_HD const int16_t *tile_levels32(const FrameView &f, long i, int p) { return p == 0 ? f.lev_y + i * 1024 : (p == 1 ? f.lev_u : f.lev_v) + i * 256; }
// range `ri` of a transform block: kRange scan positions (16 luma, 4 chroma: 64 ranges cover the block)
template <int N> struct Range32 {
  enum { kRange = N * N / kLanes32 };
  AV1_HD static int count(int eob) { return (eob + kRange - 1) / kRange; }
  template <class K> AV1_HD static void pass1(K &k, Tile32Mem &S, const int16_t *lev, int b, int p, int eob, int ri) {
    const MagMap<N> M(tile_scratch32(S, b, p));
    tok_coeffs_pass1<N, kSlots32>(k, M, p != 0, lev, eob, imin(eob, (ri + 1) * kRange) - 1, ri * kRange);
  }
  template <class K> AV1_HD static void pass2(K &k, Tile32Mem &S, const int16_t *lev, int b, int p, int eob, int ri) {
    const MagMap<N> M(tile_scratch32(S, b, p));
    const TbCtx32 c = ri == 0 ? tile_ctx32(S, b, p) : TbCtx32{ 0, 0, 0, 0 };      // the DC's sign context: scan position 0 only
    tok_coeffs_pass2<N, kSlots32>(k, M, p != 0, lev, c.ad, c.ld, ri * kRange, imin(eob, (ri + 1) * kRange));
  }
};

// one transform block of the counting sweep: every lane its range of both passes, lane 0 what opens the round
template <int N> AV1_HD void tok_tb32_total(const FrameView &f, TotalSink32 &k, Tile32Mem &S, int lane, int sbr, int sbc, int b, int p, bool half) {
  const int eob = S.eob[b * 3 + p];
  const int16_t *lev = tile_levels32(f, block_index32(f, sbr, sbc, b), p);
  if (lane == 0) tok_tb32_open<N>(f, k, S, sbr, sbc, b, p, half);
  if (lane < Range32<N>::count(eob)) { Range32<N>::pass1(k, S, lev, b, p, eob, lane); Range32<N>::pass2(k, S, lev, b, p, eob, lane); }
}

// one transform block of the emitting sweep; `words`: the tile's list words so far (returns them with the block's)
template <int N, class W>
AV1_HD int tok_tb32_emit(W &w, Tile32Mem &S, const FrameView &f, int sbr, int sbc, int b, int p, bool half, int words, op_t *list, uint32_t *grouped) {
  typedef typename W::template Var<int> LaneInt;
  typedef Range32<N> R;
  const int eob = S.eob[b * 3 + p], nr = R::count(eob);
  const int16_t *lev = tile_levels32(f, block_index32(f, sbr, sbc, b), p);
  const bool chroma = p != 0;
  LaneInt n, opened;
  if (nr <= 1) {       // at most one range (an all-zero block: one symbol): lane 0 writes the block in one go
    w.each([&](int lane) {
      if (lane) return;
      DirectSink32 k = { S.run, words, list, grouped };
      tok_tb32_open<N>(f, k, S, sbr, sbc, b, p, half);
      if (nr) { R::pass1(k, S, lev, b, p, eob, 0); R::pass2(k, S, lev, b, p, eob, 0); }
      n[lane] = k.n;
    });
    return w.first(n);
  }
  // pass 1, counted: lane j has range nr - 1 - j; lane 0 writes what opens the round (slots no range touches) and counts its words in
  w.each([&](int lane) {
    int c = 0, o = 0;
    if (lane == 0) {
      DirectSink32 k = { S.run, words, list, grouped };
      tok_tb32_open<N>(f, k, S, sbr, sbc, b, p, half);
      o = k.n - words;
    }
    if (lane < ((nr + 3) & ~3)) {       // (the prefix reads whole dwords of counts)
      uint8_t *col = reinterpret_cast<uint8_t *>(S.round) + lane;
      for (int rs = 0; rs < kRoundSlots; rs++) col[rs * (kRoundStride * 4)] = 0;
      if (lane < nr) {
        CountSink32 k = { col, chroma, 0 };
        R::pass1(k, S, lev, b, p, eob, nr - 1 - lane);
        c = k.n;
      }
    }
    opened[lane] = o; n[lane] = c + o;
  });
  const int words1 = w.scan(n);
  // lane rs takes slot rs of the round: its counts into registers, then the positions in their place
  typename W::template Var<RoundCounts> cnt;
  const int nd = (nr + 3) >> 2;
  w.each([&](int lane) {
    if (lane >= kRoundSlots) return;
    RoundCounts &c = cnt[lane];
    AV1_UNROLL
    for (int q = 0; q < kLanes32 / 4; q++) c.w[q] = q < nd ? S.round[lane * kRoundStride + q] : 0u;
  });
  w.each([&](int lane) {
    if (lane >= kRoundSlots) return;
    const RoundCounts &c = cnt[lane];
    const int slot = round_slot_global(lane, chroma);
    uint32_t run = S.run[slot];
    AV1_UNROLL
    for (int q = 0; q < kLanes32 / 4; q++) {
      if (q >= nd) continue;
      const uint32_t u = c.w[q], p0 = run, p1 = p0 + (u & 0xFF), p2 = p1 + ((u >> 8) & 0xFF), p3 = p2 + ((u >> 16) & 0xFF);
      run = p3 + (u >> 24);
      S.round[lane * kRoundStride + 2 * q] = p0 | (p1 << 16); S.round[lane * kRoundStride + 2 * q + 1] = p2 | (p3 << 16);
    }
    S.run[slot] = run;
  });
  w.each([&](int lane) {
    if (lane >= nr) return;
    EmitSink32 k = { reinterpret_cast<u16a *>(S.round) + lane, chroma, words + n[lane] + opened[lane], list, grouped };
    R::pass1(k, S, lev, b, p, eob, nr - 1 - lane);
  });
  words += words1;
  // pass 2: lane j has range j; literals, but for the DC's sign (lane 0, alone with its slot)
  w.each([&](int lane) {
    WordSink32 k = { 0 };
    if (lane < nr) R::pass2(k, S, lev, b, p, eob, lane);
    n[lane] = k.n;
  });
  const int words2 = w.scan(n);
  w.each([&](int lane) {
    if (lane >= nr) return;
    DirectSink32 k = { S.run, words + n[lane], list, grouped };
    R::pass2(k, S, lev, b, p, eob, lane);
  });
  return words + words2;
}

// THE TILE'S AREAS.  A tile tokenizer (tok_tile32 here, tok_tile8 of av1_ops8.hpp) knows the tile's list words and grouped entries after
// its counting pass, before it writes one of them, and asks an object `out` for the places:
//   out.reserve(words, entries, &a, &b)   one lane, once per tile that fits: two handles
//   out.list(a) / out.grouped(b)          every lane: the areas behind the handles (>= words, >= entries; 16-byte aligned)
//   out.slot(sl, total, base)             a slot's entries: `total` from grouped[base] on; called for every slot below S_MAX
//   out.refuse(sl)                        the tile does not fit: slot sl has no entries
// The GPU kernels reserve whole cache lines of a pool all tiles share (av1_entropy_kernels.hip); the CPU twin hands out the caller's
// pointers:
struct CallerAreas {
  op_t *list_; uint32_t *grouped_; uint16_t *slot_total, *slot_base;
  AV1_HD void reserve(int, int, int *a, int *b) const { *a = 0; *b = 0; }
  AV1_HD op_t *list(int) const { return list_; }
  AV1_HD uint32_t *grouped(int) const { return grouped_; }
  AV1_HD void slot(int sl, uint16_t total, uint16_t base) const { slot_total[sl] = total; slot_base[sl] = base; }
  AV1_HD void refuse(int sl) const { slot_total[sl] = 0; }
};

// THE TILE = superblock (sbr, sbc) of a key frame's 32x32 band: its literals into list[0 .. words), its adaptive symbols into `grouped`
// (slot sl: total entries from base on, bases on multiples of kListAlign), totals and bases of all S_MAX slots to `out`, which also places
// the list and the entries.  Returns the list words, the same in every lane; -1 when the tile has more than ops_cap words or more than
// 65 535 entries: then all totals and bases are 0, nothing has been reserved and neither list nor grouped has been written.  (No other
// capacity: a lane's counts of a round fit their bytes.)
template <class W, class O>
AV1_HD int tok_tile32(W &w, Tile32Mem &S, const FrameView &f, int sbr, int sbc, uint32_t ops_cap, O &out) {
  typedef typename W::template Var<int> LaneInt;
  const bool half = sbc * 8 + 4 >= f.w8;         // the frame ends after the superblock's left 32 columns (width % 64 == 32): blocks 1 and 3 are not coded
  w.each([&](int lane) {
    fill_scan_tables32(&S.scan, lane, kLanes32);
    for (int i = lane; i < kTile32MagBytes / 4; i += kLanes32) reinterpret_cast<u32a *>(S.mag)[i] = 0;
    for (int i = lane; i < K_END; i += kLanes32) S.run[i] = 0;
    if (lane < kBlocks32 * 3) { S.eob[lane] = 0; S.cul[lane] = 0; }
  });
  // the levels, once: 128 groups of eight per luma block (two per lane), 32 + 32 per chroma pair (one per lane)
  w.each([&](int lane) {
    AV1_UNROLL
    for (int b = 0; b < kBlocks32; b++) {
      if (half && (b & 1)) continue;
      const long i = block_index32(f, sbr, sbc, b);
      int eob = 0, cul = 0;
      MagMap<32> Y(tile_scratch32(S, b, 0));
      eob = Y.load8(f.lev_y + i * 1024, lane, &cul);
      eob = imax(eob, Y.load8(f.lev_y + i * 1024, lane + kLanes32, &cul));
      if (cul) { AV1_SHARED_MAX(&S.eob[b * 3], eob); AV1_SHARED_ADD(&S.cul[b * 3], cul); }
      const int p = 1 + (lane >> 5);
      MagMap<16> C(tile_scratch32(S, b, p));
      cul = 0;
      eob = C.load8((p == 1 ? f.lev_u : f.lev_v) + i * 256, lane & 31, &cul);
      if (cul) { AV1_SHARED_MAX(&S.eob[b * 3 + p], eob); AV1_SHARED_ADD(&S.cul[b * 3 + p], cul); }
    }
  });
  // the counting sweep: symbols per slot, list words
  LaneInt n;
  w.each([&](int lane) {
    TotalSink32 k = { S.run, 0 };
    for (int b = 0; b < kBlocks32; b++) {
      if (half && (b & 1)) continue;
      tok_tb32_total<32>(f, k, S, lane, sbr, sbc, b, 0, half);
      tok_tb32_total<16>(f, k, S, lane, sbr, sbc, b, 1, half);
      tok_tb32_total<16>(f, k, S, lane, sbr, sbc, b, 2, half);
    }
    n[lane] = k.n;
  });
  const int words = w.scan(n);
  // place the slots: lane j has slots 3 j .. 3 j + 2
  enum { kOwn = (K_END + kLanes32 - 1) / kLanes32 };
  w.each([&](int lane) {
    int mine = 0;
    for (int q = 0; q < kOwn; q++) if (lane * kOwn + q < K_END) mine += (int)((S.run[lane * kOwn + q] + kListAlign - 1) & ~(uint32_t)(kListAlign - 1));
    n[lane] = mine;
  });
  const int entries = w.scan(n);
  const bool fits = (uint32_t)words <= ops_cap && entries <= 65535;
  w.each([&](int lane) {
    uint32_t run = (uint32_t)n[lane];
    for (int q = 0; q < kOwn; q++) {
      const int sl = lane * kOwn + q;
      if (sl >= K_END) break;
      const uint32_t tot = S.run[sl];
      out.slot(sl, (uint16_t)(fits ? tot : 0u), (uint16_t)(fits ? run : 0u));
      S.run[sl] = run;
      run += (tot + kListAlign - 1) & ~(uint32_t)(kListAlign - 1);
    }
    for (int sl = K_END + lane; sl < S_MAX; sl += kLanes32) out.slot(sl, 0, 0);
  });
  if (!fits) return -1;
  LaneInt at_list, at_grouped;
  w.each([&](int lane) { if (lane == 0) out.reserve(words, entries, &at_list[lane], &at_grouped[lane]); });
  op_t *const list = out.list(w.first(at_list));
  uint32_t *const grouped = out.grouped(w.first(at_grouped));
  // the emitting sweep, transform block by transform block in decoding order
  int at = 0;
  for (int b = 0; b < kBlocks32; b++) {
    if (half && (b & 1)) continue;
    at = tok_tb32_emit<32>(w, S, f, sbr, sbc, b, 0, half, at, list, grouped);
    at = tok_tb32_emit<16>(w, S, f, sbr, sbc, b, 1, half, at, list, grouped);
    at = tok_tb32_emit<16>(w, S, f, sbr, sbc, b, 2, half, at, list, grouped);
  }
  return at;
}

}  // namespace av1ops
