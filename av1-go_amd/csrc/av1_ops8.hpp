// av1_ops8.hpp — THE TILE TOKENIZER OF 8x8 BLOCKS (tok_tile8): every P frame's tiles, and the rows of a key frame below its 32x32
// band.  One wave of 64 lanes per tile, a lane per block in z-order, written against the wave of av1_ops32.hpp (each / scan / Var):
// hipcc runs it across a wave (k_av1_tokens), g++ as a loop over the lanes (the CPU twin, host/av1_opstream.cpp).
//   SUMMARIES  every lane reads what its block's neighbours need of its levels (block_levels_summary: the DC signs, chroma zero or
//              not) into the tile's memory — the contexts across blocks come from there, not from a pass over the batch's levels;
//   TOKENIZE   once per block (tok_block): 16-bit records + per (slot, block) byte counts;
//   PLACE      counts -> the slots' totals and bases, and a ROW for every slot the tile uses;
//   REPLAY     records -> list words and grouped entries, through 16-bit running positions [rows][64 blocks].  The positions of
//              kReplaySlots rows fit the tile's memory: a tile that uses no more slots than that (a P tile at the usual quantisers
//              uses 60-90 of 199) replays its records ONCE; only a tile that uses more takes two passes, half of its rows each.
#pragma once
#include "av1_ops32.hpp"

namespace av1ops {

enum { kLanes8 = kBlocksPerTile, kReplaySlots = (S_MAX + 1) / 2, kOwn8 = (S_MAX + kLanes8 - 1) / kLanes8 };
static_assert(2 * kReplaySlots >= S_MAX && S_MAX <= 256 && kOwn8 * kLanes8 >= S_MAX && 4 * kLanes8 >= S_MAX, "rows are bytes; two passes cover every slot");

// what a tile's wave keeps in LDS (the twin: in memory): 19.9 KB.  The byte counts share their place with the positions that replace
// them: a lane keeps the counts of its slots in registers across the switch.
struct Tile8Mem {
  union {
    struct { uint8_t cnt[S_MAX * kBlocksPerTile]; alignas(16) uint8_t mag[kBlocksPerTile * kMagBytes]; } p1;    // while tokenizing
    uint16_t pos[kReplaySlots * kBlocksPerTile];                                                               // while replaying
  };
  uint16_t total[S_MAX], base[S_MAX];
  uint8_t row[(S_MAX + 3) & ~3];          // per slot the tile uses: its row among the used slots, in slot order
  uint8_t sums[kBlocksPerTile];           // [by * 8 + bx] block_levels_summary
  ScanTables scan;
};
struct SlotCounts8 { uint32_t w[kOwn8][kBlocksPerTile / 4]; };      // the counts of a lane's slots (lane, lane + 64, ...), four blocks a dword

// block `blk`: its records -> list words (from index `first`) and grouped entries.  pos = [rows][64 blocks] running positions of the
// rows [row_lo, row_lo + kReplaySlots); `literals`: this pass writes the literals too
AV1_HD void replay_block8(const uint16_t *rec, int nrec, uint16_t *pos, const uint8_t *row, int blk, int first, op_t *list, uint32_t *grouped, int row_lo,
                          bool literals) {
  int n = first;
  for (int i0 = 0; i0 < nrec; i0 += 8) {        // eight records per load (a dependent 2-byte load per record is a memory round trip each)
    struct alignas(16) R8 { uint32_t w[4]; } q = *reinterpret_cast<const R8 *>(rec + i0);
    AV1_UNROLL      // (fully unrolled the eight records are register halves; indexed at run time the array lived in scratch memory)
    for (int j = 0; j < 8; j++, n++) {
      if (i0 + j >= nrec) break;
      const unsigned r = (q.w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
      if (r & 0x8000u) { if (literals) list[n] = op_lit((int)((r >> 11) & 15), r & 0x7FFu); }
      else {
        const unsigned rw = (unsigned)row[r >> 4] - (unsigned)row_lo;
        if (rw < (unsigned)kReplaySlots) { uint16_t &p = pos[rw * kBlocksPerTile + blk]; grouped[p] = ((uint32_t)n << 4) | (r & 15u); p++; }
      }
    }
  }
}

// THE TILE = superblock (sbr, sbc) of 8x8 blocks: its literals into list[0 .. words), its adaptive symbols into `grouped` (slot sl:
// total entries from base on, bases on multiples of kListAlign, slots in order), totals and bases of all S_MAX slots to `out`.  The list
// and the entries lie where `out` places them once the tile's word and entry counts are known (av1_ops32.hpp: the tile's areas).
// rec: kBlocksPerTile * kBlockRecords records of scratch.  Returns the list words, the same in every lane; -1 when the tile has more
// than ops_cap words or more than 65 535 entries, or a block more than kBlockRecords records or more than 255 symbols of one slot:
// then every slot has been refused, nothing has been reserved and nothing else has been written.
template <class W, class O>
AV1_HD int tok_tile8(W &w, Tile8Mem &S, const FrameView &f, int sbr, int sbc, uint16_t *rec, uint32_t ops_cap, O &out) {
  typedef typename W::template Var<int> LaneInt;
  const int nslots = f.key ? S_KEY_END : S_INTER_END;
  w.each([&](int lane) {
    for (int i = lane; i < S_MAX * kBlocksPerTile / 4; i += kLanes8) reinterpret_cast<u32a *>(S.p1.cnt)[i] = 0;
    if (lane == 0) fill_scan_tables(&S.scan);
    int bx, by;
    demorton8((unsigned)lane, &bx, &by);
    const int r8 = sbr * 8 + by, c8 = sbc * 8 + bx;
    S.sums[by * 8 + bx] = (uint8_t)(r8 < f.h8 && c8 < f.w8 ? block_levels_summary(f, r8 * f.w8 + c8) : 0u);
  });
  // read_cdef: the superblock's index goes with the tile's first block in coding order (= lane order) that is not skipped — block 0 of
  // a key frame; in a P frame a ballot over the lanes' "inside the frame and coded" says which, and none when the tile is all skipped
  int cdef_zi = -1;
  if (f.cdef_bits) {
    if (f.key) cdef_zi = 0;
    else {
      LaneInt coded;
      w.each([&](int lane) {
        int bx, by;
        demorton8((unsigned)lane, &bx, &by);
        const int r8 = sbr * 8 + by, c8 = sbc * 8 + bx;
        coded[lane] = r8 < f.h8 && c8 < f.w8 && !f.skip[r8 * f.w8 + c8];
      });
      const uint64_t m = w.ballot(coded);
      cdef_zi = m ? __builtin_ctzll(m) : -1;
    }
  }
  // tokenize: records, counts; a lane's list words, and "a block overflowed" above them
  LaneInt nrec, first;
  w.each([&](int lane) {
    const TokScratch ts = { S.p1.mag + lane * kMagBytes, &S.scan };
    Sink k = { rec + (size_t)lane * kBlockRecords, S.p1.cnt, lane, 0, 0, false };
    tok_block(f, k, ts, sbr, sbc, lane, S.sums, cdef_zi);
    nrec[lane] = k.nrec;
    first[lane] = k.n | (k.overflow ? 1 << 24 : 0);       // (a block has fewer than 2^16 words)
  });
  const int sum = w.scan(first), words = sum & 0xFFFFFF;
  bool fits = (uint32_t)words <= ops_cap && !(sum >> 24);
  // place.  Lane j owns slots j, j + 64, ...: their counts into registers, their totals to everybody
  typename W::template Var<SlotCounts8> cnt;
  if (fits) w.each([&](int lane) {
    SlotCounts8 &c = cnt[lane];
    AV1_UNROLL
    for (int q = 0; q < kOwn8; q++) {
      const int sl = lane + kLanes8 * q;
      int tot = 0;
      AV1_UNROLL
      for (int i = 0; i < kBlocksPerTile / 4; i++) {
        const uint32_t u = sl < nslots ? reinterpret_cast<const u32a *>(S.p1.cnt)[sl * (kBlocksPerTile / 4) + i] : 0u;
        c.w[q][i] = u;
#if defined(__HIP_DEVICE_COMPILE__)
        tot = (int)__builtin_amdgcn_sad_u8(u, 0u, (unsigned)tot);      // the four counts of the dword in one instruction
#else
        tot += (int)((u & 0xFF) + ((u >> 8) & 0xFF) + ((u >> 16) & 0xFF) + (u >> 24));
#endif
      }
      if (sl < S_MAX) S.total[sl] = (uint16_t)tot;
    }
  });
  // lane j places slots [4 j, 4 j + 4): slots follow each other on 16-byte boundaries, used slots take the rows in turn
  LaneInt ent, used;
  if (fits) w.each([&](int lane) {
    int e = 0, u = 0;
    for (int q = 0; q < 4; q++) {
      const int sl = 4 * lane + q;
      if (sl < nslots) { e += (S.total[sl] + kListAlign - 1) & ~(kListAlign - 1); u += S.total[sl] != 0; }
    }
    ent[lane] = e; used[lane] = u;
  });
  const int entries = fits ? w.scan(ent) : 0, rows = fits ? w.scan(used) : 0;
  fits = fits && entries <= 65535;
  if (!fits) {
    w.each([&](int lane) { for (int sl = lane; sl < S_MAX; sl += kLanes8) out.refuse(sl); });
    return -1;
  }
  LaneInt at_list, at_grouped;
  w.each([&](int lane) { if (lane == 0) out.reserve(words, entries, &at_list[lane], &at_grouped[lane]); });
  op_t *const list = out.list(w.first(at_list));
  uint32_t *const grouped = out.grouped(w.first(at_grouped));
  w.each([&](int lane) {
    int run = ent[lane], r = used[lane];
    for (int q = 0; q < 4; q++) {
      const int sl = 4 * lane + q;
      if (sl >= nslots) break;
      const int tot = S.total[sl];
      S.base[sl] = (uint16_t)run; S.row[sl] = (uint8_t)r;
      run += (tot + kListAlign - 1) & ~(kListAlign - 1); r += tot != 0;
    }
  });
  const int npass = rows <= kReplaySlots ? 1 : 2;
  for (int pass = 0; pass < npass; pass++) {
    const int row_lo = pass * kReplaySlots;
    // (every count is in a register, and the pass before has used its positions up: the positions overwrite them)
    w.each([&](int lane) {
      const SlotCounts8 &c = cnt[lane];
      AV1_UNROLL
      for (int q = 0; q < kOwn8; q++) {
        const int sl = lane + kLanes8 * q;
        if (sl >= S_MAX) continue;
        if (pass == 0) { const bool on = sl < nslots; out.slot(sl, on ? S.total[sl] : (uint16_t)0, on ? S.base[sl] : (uint16_t)0); }
        if (sl >= nslots || !S.total[sl]) continue;
        const unsigned rw = (unsigned)S.row[sl] - (unsigned)row_lo;
        if (rw >= (unsigned)kReplaySlots) continue;
        int run = S.base[sl];
        AV1_UNROLL
        for (int i = 0; i < kBlocksPerTile / 4; i++) {
          const uint32_t u = c.w[q][i];
          const int p0 = run, p1 = p0 + (int)(u & 0xFF), p2 = p1 + (int)((u >> 8) & 0xFF), p3 = p2 + (int)((u >> 16) & 0xFF);
          run = p3 + (int)(u >> 24);
          u32a *d = reinterpret_cast<u32a *>(S.pos + rw * kBlocksPerTile + 4 * i);
          d[0] = (uint32_t)p0 | ((uint32_t)p1 << 16); d[1] = (uint32_t)p2 | ((uint32_t)p3 << 16);
        }
      }
    });
    w.each([&](int lane) {
      replay_block8(rec + (size_t)lane * kBlockRecords, nrec[lane], S.pos, S.row, lane, first[lane] & 0xFFFFFF, list, grouped, row_lo, pass == 0);
    });
  }
  return words;
}

}  // namespace av1ops
