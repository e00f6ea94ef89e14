// av1_tile_syntax.hpp — the part of the AV1 tile syntax that does not depend on block geometry, stated once for both host
// writers (av1_bitstream.cpp: 8x8 blocks; av1_blockstream.cpp: every block and transform size): a tile's coder state and
// its reset, the subexponential codes, the loop restoration units, motion vector components, the CDEF index, the
// chroma-from-luma alphas, the transform type and the coefficients of one transform block (general in width, height and
// class).  What a writer adds is the partition tree, the mode info of its blocks and the position of each transform block.
// Written from the AV1 Bitstream & Decoding Process Specification; section numbers in the comments are the specification's.
// No mutable statics: tiles are written by several threads, each with a writer of its own.  Internal to libav1mi_host.so.
#pragma once
#include <map>

#include "av1_bitstream_core.hpp"

namespace av1mi_host {
namespace av1 {
namespace core {

enum { T_V_DCT = 10, T_H_DCT, T_V_ADST, T_H_ADST, T_V_FLIPADST, T_H_FLIPADST };      // the 1-D types, after T_IDTX
enum { CLASS_2D, CLASS_HORIZ, CLASS_VERT };
inline int tx_class_of(int t) {
  return (t == T_V_DCT || t == T_V_ADST || t == T_V_FLIPADST) ? CLASS_VERT : (t == T_H_DCT || t == T_H_ADST || t == T_H_FLIPADST) ? CLASS_HORIZ : CLASS_2D;
}
// symbol of a transform type inside each set (inverse of Tx_Type_Intra_Inv_Set1/2, Tx_Type_Inter_Inv_Set1/2/3, 5.11.47); -1 = not in the set.
// Sets as get_tx_set (5.11.48) numbers them here: 0 DCT only, 1 INTRA_1, 2 INTRA_2, 3 INTER_1, 4 INTER_2, 5 INTER_3
static const int8_t kIntraSet1Sym[16] = { 1, 5, 6, 4, -1, -1, -1, -1, -1, 0, 2, 3, -1, -1, -1, -1 };
static const int8_t kIntraSet2Sym[16] = { 1, 3, 4, 2, -1, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1 };
static const int8_t kInterSet1Sym[16] = { 7, 8, 9, 12, 10, 11, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6 };
static const int8_t kInterSet2Sym[16] = { 3, 4, 5, 8, 6, 7, 9, 10, 11, 0, 1, 2, -1, -1, -1, -1 };
static const int8_t kInterSet3Sym[16] = { 1, -1, -1, -1, -1, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1 };
inline const int8_t *tx_set_syms(int set) {
  return set == 1 ? kIntraSet1Sym : set == 2 ? kIntraSet2Sym : set == 3 ? kInterSet1Sym : set == 4 ? kInterSet2Sym : kInterSet3Sym;
}

// get_scan (5.11.41): positions pos = row * tw + col of the (at most 32 x 32) coded area; kind 0 default, 1 row-major (mrow), 2 column-major (mcol)
inline const std::vector<uint16_t> &scan_of(int tw, int th, int kind) {
  static thread_local std::map<int, std::vector<uint16_t>> cache;      // (per thread: tiles are written by several)
  const int key = (tw << 16) | (th << 4) | kind;
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  std::vector<uint16_t> s;
  s.reserve((size_t)tw * th);
  if (kind == 1) {
    for (int i = 0; i < tw * th; i++) s.push_back((uint16_t)i);
  } else if (kind == 2) {
    for (int c = 0; c < tw; c++) for (int r = 0; r < th; r++) s.push_back((uint16_t)(r * tw + c));
  } else {
    for (int d = 0; d < tw + th - 1; d++) {
      // square: zig-zag (odd diagonals run downwards, even ones upwards); tall: every diagonal downwards; wide: every diagonal upwards
      const bool down = tw == th ? (d & 1) : th > tw;
      for (int i = 0; i <= d; i++) {
        const int r = down ? i : d - i, c = d - r;
        if (r < th && c < tw) s.push_back((uint16_t)(r * tw + c));
      }
    }
  }
  return cache.emplace(key, std::move(s)).first->second;
}

// a transform size and class as the coefficient syntax sees them.  Looking the scan up costs a map search: a writer whose
// transform sizes are fixed makes its Txbs once per tile
struct Txb {
  int w, h;            // the transform's size, 4..64
  int tw, th;          // the coded area: at most 32 x 32
  int sq, txs_ctx;     // Tx_Size_Sqr; txSzCtx = (Tx_Size_Sqr + Tx_Size_Sqr_Up + 1) >> 1
  int cls;
  const uint16_t *scan;
  Txb() {}
  Txb(int w_, int h_, int cls_) : w(w_), h(h_), tw(std::min(w_, 32)), th(std::min(h_, 32)), cls(cls_) {
    sq = floor_log2((uint32_t)std::min(w, h)) - 2;
    txs_ctx = (sq + floor_log2((uint32_t)std::max(w, h)) - 2 + 1) >> 1;
    scan = scan_of(tw, th, cls == CLASS_VERT ? 1 : cls == CLASS_HORIZ ? 2 : 0).data();
  }
};

struct TileSyntax {
  FrameInfo fi;
  const av1mi_obu_frame &f;
  RangeEnc ec;
  Cdfs cdf;
  bool adapt = true;
  int mi_r0 = 0, mi_r1 = 0, mi_c0 = 0, mi_c1 = 0;        // tile bounds in 4x4 units
  // Above{Level,Dc}Context per plane: 4-sample units of the plane, tile relative (position x4 of the plane is entry x4 - (mi_c0 >> ss)),
  // with room for a 64-wide block that hangs over the frame's edge.  Left...: superblock relative (entry y4 & (15 >> ss))
  std::vector<uint8_t> a_lvl[3], a_dc[3];
  uint8_t l_lvl[3][32], l_dc[3][32];
  int ref_wiener[3][2][3], ref_sgr[3][2];                // RefLrWiener / RefSgrXqd (5.11.58)
  bool cdef_coded = false;

  explicit TileSyntax(const FrameInfo &fi_) : fi(fi_), f(*fi_.f) {}
  inline void sym(uint16_t *icdf, int n, int s) { put_symbol(ec, icdf, n, s, adapt); }

  // the start of decode_tile (5.11.2): tile bounds, symbol coder, default CDFs, clear_above_context, the restoration references
  void reset_tile(int tr, int tc) {
    mi_r0 = tr * fi.tile_h_sb * 16; mi_r1 = std::min(mi_r0 + fi.tile_h_sb * 16, fi.mi_rows);
    mi_c0 = tc * fi.tile_w_sb * 16; mi_c1 = std::min(mi_c0 + fi.tile_w_sb * 16, fi.mi_cols);
    ec = RangeEnc();
    cdf = default_cdfs(fi.qcat);
    adapt = !f.disable_cdf_update;
    for (int p = 0; p < 3; p++) {
      a_lvl[p].assign((size_t)(mi_c1 - mi_c0) + 48, 0); a_dc[p].assign((size_t)(mi_c1 - mi_c0) + 48, 0);
      for (int k = 0; k < 2; k++) { ref_wiener[p][k][0] = 3; ref_wiener[p][k][1] = -7; ref_wiener[p][k][2] = 15; }      // Wiener_Taps_Mid
      ref_sgr[p][0] = -32; ref_sgr[p][1] = 31;                                                                          // Sgrproj_Xqd_Mid
    }
  }
  void clear_left_context() { memset(l_lvl, 0, sizeof(l_lvl)); memset(l_dc, 0, sizeof(l_dc)); }

  // ---- subexponential codes with a reference, written with equiprobable bools (5.11.58, 4.10.10 structure)
  void put_ns(int n, int v) {               // NS(n) by literals
    const int w = floor_log2((uint32_t)n) + 1, m = (1 << w) - n;
    if (v < m) ec.literal((uint32_t)v, w - 1);
    else { ec.literal((uint32_t)((v + m) >> 1), w - 1); ec.literal((uint32_t)((v + m) & 1), 1); }
  }
  void put_subexp(int num_syms, int k, int v) {   // decode_subexp_bool
    int i = 0, mk = 0;
    for (;;) {
      const int b2 = i ? k + i - 1 : k, a = 1 << b2;
      if (num_syms <= mk + 3 * a) { put_ns(num_syms - mk, v - mk); return; }
      const int more = v >= mk + a;
      ec.literal((uint32_t)more, 1);
      if (!more) { ec.literal((uint32_t)(v - mk), b2); return; }
      i++; mk += a;
    }
  }
  static int recenter(int r, int v) { return v > 2 * r ? v : v >= r ? 2 * (v - r) : 2 * (r - v) - 1; }   // inverse of inverse_recenter
  void put_signed_subexp_with_ref(int v, int low, int high, int k, int r) {   // decode_signed_subexp_with_ref_bool
    const int mx = high - low; v -= low; r -= low;
    put_subexp(mx, k, (r << 1) <= mx ? recenter(r, v) : recenter(mx - 1 - r, mx - 1 - v));
  }

  // ---- read_lr / read_lr_unit (5.11.57, 5.11.58): the restoration units of the superblock at (mi_r, mi_c)
  void write_lr(int mi_r, int mi_c) {
    for (int p = 0; p < 3; p++) {
      if (!f.lr_type[p]) continue;
      const int ss = p ? 1 : 0, us = fi.lr_size[p];
      const int row0 = (mi_r * (4 >> ss) + us - 1) / us, row1 = std::min(((mi_r + 16) * (4 >> ss) + us - 1) / us, fi.lr_rows[p]);
      const int col0 = (mi_c * (4 >> ss) + us - 1) / us, col1 = std::min(((mi_c + 16) * (4 >> ss) + us - 1) / us, fi.lr_cols[p]);
      for (int ur = row0; ur < row1; ur++)
        for (int uc = col0; uc < col1; uc++) lr_unit(p, f.lr_units[p] + ((size_t)ur * fi.lr_cols[p] + uc) * 8);
    }
  }
  void lr_unit(int p, const int8_t *u) {
    const int type = u[0];   // 0 none, 1 Wiener, 2 self-guided
    if (f.lr_type[p] == 1) sym(cdf.use_wiener, 2, type == 1);
    else if (f.lr_type[p] == 2) sym(cdf.use_sgrproj, 2, type == 2);
    else sym(cdf.switchable_restore, 3, type);
    if (type == 1 && f.lr_type[p] != 2) {
      static const int kMin[3] = { -5, -23, -17 }, kMax[3] = { 10, 8, 46 }, kK[3] = { 1, 2, 3 };   // Wiener_Taps_Min / Max / K
      for (int pass = 0; pass < 2; pass++)
        for (int j = p ? 1 : 0; j < 3; j++) {
          const int v = u[1 + pass * 3 + j];
          put_signed_subexp_with_ref(v, kMin[j], kMax[j] + 1, kK[j], ref_wiener[p][pass][j]);
          ref_wiener[p][pass][j] = v;
        }
    } else if (type == 2 && f.lr_type[p] != 1) {
      static const int8_t kRadius[16][2] = { { 2, 1 }, { 2, 1 }, { 2, 1 }, { 2, 1 }, { 2, 1 }, { 2, 1 }, { 2, 1 }, { 2, 1 }, { 2, 1 }, { 2, 1 },
                                             { 0, 1 }, { 0, 1 }, { 0, 1 }, { 0, 1 }, { 2, 0 }, { 2, 0 } };   // Sgr_Params radii
      static const int kMin[2] = { -96, -32 }, kMax[2] = { 31, 95 };
      const int set = u[1];
      ec.literal((uint32_t)set, 4);
      for (int i = 0; i < 2; i++) {
        int v = u[2 + i];
        if (kRadius[set][i]) put_signed_subexp_with_ref(v, kMin[i], kMax[i] + 1, 4, ref_sgr[p][i]);
        else v = i == 0 ? 0 : std::min(std::max(128 - ref_sgr[p][0], kMin[1]), kMax[1]);
        ref_sgr[p][i] = v;
      }
    }
  }

  // ---- read_cdef (5.11.56): the index is coded with the first non-skipped block of the 64x64 superblock sb
  void write_cdef(int sb, int skip) {
    if (skip || cdef_coded) return;
    ec.literal(f.cdef_idx ? f.cdef_idx[sb] : 0, f.cdef_bits);
    cdef_coded = true;
  }
  // ---- read_cfl_alphas (5.11.45); not both zero, each at most 16 in magnitude
  void write_cfl_alphas(int alpha_u, int alpha_v) {
    const int su = alpha_u == 0 ? 0 : alpha_u < 0 ? 1 : 2, sv = alpha_v == 0 ? 0 : alpha_v < 0 ? 1 : 2;   // CFL_SIGN_ZERO / NEG / POS
    sym(cdf.cfl_sign, 8, su * 3 + sv - 1);
    if (su) sym(cdf.cfl_alpha[(su - 1) * 3 + sv], 16, std::abs(alpha_u) - 1);
    if (sv) sym(cdf.cfl_alpha[(sv - 1) * 3 + su], 16, std::abs(alpha_v) - 1);
  }
  // ---- is_inter with its context (9.3); above_intra / left_intra: the neighbour is available and intra
  void write_is_inter(bool au, bool al, bool above_intra, bool left_intra, int is_inter) {
    int ctx;
    if (au && al) ctx = (left_intra && above_intra) ? 3 : (left_intra || above_intra);
    else if (au || al) ctx = 2 * (au ? above_intra : left_intra);
    else ctx = 0;
    sym(cdf.is_inter[ctx], 2, is_inter);
  }
  // ---- read_mv_component (5.11.33).  Without allow_high_precision_mv (hp false) the eighth-sample bit is implied 1: diff is even
  void write_mv_comp(MvCompCdf &m, int diff, bool hp) {
    sym(m.sign, 2, diff < 0);
    const int off = std::abs(diff) - 1;
    const int cls = (off >> 3) < 2 ? 0 : floor_log2((uint32_t)(off >> 3));
    sym(m.cls, 11, cls);
    if (cls == 0) {
      sym(m.class0, 2, off >> 3);
      sym(m.class0_fr[off >> 3], 4, (off >> 1) & 3);
      if (hp) sym(m.class0_hp, 2, off & 1);
    } else {
      const int o = off - (2 << (cls + 2)), d = o >> 3;
      for (int i = 0; i < cls; i++) sym(m.bits[i], 2, (d >> i) & 1);
      sym(m.fr, 4, (o >> 1) & 3);
      if (hp) sym(m.hp, 2, o & 1);
    }
  }

  // ---- transform_type (5.11.47) of a luma transform block whose set (get_tx_set, numbered as above) holds more than DCT_DCT
  void transform_type(int set, int sq, int y_mode, int tx_type) {
    switch (set) {
      case 1: sym(cdf.intra_tx1[sq][y_mode], 7, kIntraSet1Sym[tx_type]); break;
      case 2: sym(cdf.intra_tx2[sq][y_mode], 5, kIntraSet2Sym[tx_type]); break;
      case 3: sym(cdf.inter_tx1[sq], 16, kInterSet1Sym[tx_type]); break;
      case 4: sym(cdf.inter_tx2, 12, kInterSet2Sym[tx_type]); break;
      default: sym(cdf.inter_tx3[sq], 2, kInterSet3Sym[tx_type]); break;
    }
  }

  // ---- coeffs (5.11.39) of one transform block: all_zero with the context the caller derived (it depends on the block around the
  // transform), the transform type (plane 0, set > 0), end of block, levels, signs, and the contexts later blocks read.  The block's
  // context entries start at a_*[plane][ax] / l_*[plane][ly]; nw x nh of them (units of 4 samples) lie inside the frame.  lev: the
  // tw x th coded area, row-major.  Returns eob.
  int coeffs(int plane, const Txb &t, const int16_t *lev, int all_zero_ctx, int ax, int ly, int nw, int nh, int set, int tx_type, int y_mode) {
    const int ptype = plane > 0, tw = t.tw, nc = tw * t.th, bwl = floor_log2((uint32_t)tw), cls = t.cls, txs_ctx = t.txs_ctx;
    const uint16_t *scan = t.scan;
    uint8_t *al = a_lvl[plane].data() + ax, *ad = a_dc[plane].data() + ax, *ll = l_lvl[plane] + ly, *ld = l_dc[plane] + ly;
    int eob = 0;
    for (int k = nc - 1; k >= 0; k--) if (lev[scan[k]]) { eob = k + 1; break; }
    put_symbol_n<2>(ec, cdf.txb_skip[txs_ctx][all_zero_ctx], eob == 0, adapt);
    int cul = 0, dc_cat = 0;
    if (eob) {
      if (plane == 0 && set > 0) transform_type(set, t.sq, y_mode, tx_type);
      // eob_pt_*, eob_extra, eob_extra_bit
      const int eob_pt = eob < 3 ? eob : floor_log2((uint32_t)(eob - 1)) + 2;   // eob in (2^(pt-2), 2^(pt-1)]
      const int ectx2 = cls == CLASS_2D ? 0 : 1;
      switch (bwl + floor_log2((uint32_t)t.th) - 4) {      // eobMultisize
        case 0: put_symbol_n<5>(ec, cdf.eob16[ptype][ectx2], eob_pt - 1, adapt); break;
        case 1: put_symbol_n<6>(ec, cdf.eob32[ptype][ectx2], eob_pt - 1, adapt); break;
        case 2: put_symbol_n<7>(ec, cdf.eob64[ptype][ectx2], eob_pt - 1, adapt); break;
        case 3: put_symbol_n<8>(ec, cdf.eob128[ptype][ectx2], eob_pt - 1, adapt); break;
        case 4: put_symbol_n<9>(ec, cdf.eob256[ptype][ectx2], eob_pt - 1, adapt); break;
        case 5: put_symbol_n<10>(ec, cdf.eob512[ptype][ectx2], eob_pt - 1, adapt); break;
        default: put_symbol_n<11>(ec, cdf.eob1024[ptype][ectx2], eob_pt - 1, adapt); break;
      }
      if (eob_pt >= 3) {
        const int off = eob - ((1 << (eob_pt - 2)) + 1);
        int shift = eob_pt - 3;
        put_symbol_n<2>(ec, cdf.eob_extra[txs_ctx][ptype][eob_pt - 3], (off >> shift) & 1, adapt);
        for (shift--; shift >= 0; shift--) ec.bool_eq((off >> shift) & 1);
      }
      // levels, last to first.  mag = min(|level|, 15) with a zero border of 4 on the right and bottom (the 1-D classes look 4 ahead);
      // only positions below eob are ever non-zero, so only those are written
      constexpr int MS = 36;
      uint8_t mag[MS * MS];
      memset(mag, 0, (size_t)MS * (t.th + 4));
      for (int k = 0; k < eob; k++) {
        const int pos = scan[k], a = std::abs((int)lev[pos]);
        mag[(pos >> bwl) * MS + (pos & (tw - 1))] = (uint8_t)(a > 15 ? 15 : a);
      }
      uint16_t(*base_cdf)[5] = cdf.base[txs_ctx][ptype];
      uint16_t(*br_cdf)[5] = cdf.br[std::min(txs_ctx, 3)][ptype];
      auto c3 = [](int v) { return v > 3 ? 3 : v; };
      for (int k = eob - 1; k >= 0; k--) {
        const int pos = scan[k], row = pos >> bwl, col = pos & (tw - 1);
        const uint8_t *m = mag + row * MS + col;
        const int a = std::abs((int)lev[pos]);
        if (k == eob - 1) {
          const int ectx = k == 0 ? 0 : k <= nc / 8 ? 1 : k <= nc / 4 ? 2 : 3;
          put_symbol_n<3>(ec, cdf.base_eob[txs_ctx][ptype][ectx], (a > 3 ? 3 : a) - 1, adapt);
        } else {
          // get_coeff_base_ctx (9.3): five neighbours, each capped at 3
          int mm;
          if (cls == CLASS_2D) mm = c3(m[1]) + c3(m[MS]) + c3(m[MS + 1]) + c3(m[2]) + c3(m[2 * MS]);
          else if (cls == CLASS_HORIZ) mm = c3(m[1]) + c3(m[MS]) + c3(m[2]) + c3(m[3]) + c3(m[4]);
          else mm = c3(m[1]) + c3(m[MS]) + c3(m[2 * MS]) + c3(m[3 * MS]) + c3(m[4 * MS]);
          int bctx = std::min((mm + 1) >> 1, 4);
          if (cls == CLASS_2D) {
            if (pos == 0) bctx = 0;
            else if (t.w < t.h && row < 2) bctx += 11;     // Coeff_Base_Ctx_Offset[txSz]: tall transforms (32x64 too), first two rows
            else if (t.w > t.h && col < 2) bctx += 16;     // wide transforms, first two columns
            else bctx += row + col < 2 ? 1 : row + col < 4 ? 6 : 21;
          } else {
            bctx += 26 + 5 * std::min(cls == CLASS_VERT ? row : col, 2);      // Coeff_Base_Pos_Ctx_Offset
          }
          put_symbol_n<4>(ec, base_cdf[bctx], a > 3 ? 3 : a, adapt);
        }
        if (a > 2) {     // coeff_br: up to four increments of 0..3
          int mm = m[1] + m[MS] + (cls == CLASS_2D ? m[MS + 1] : cls == CLASS_HORIZ ? m[2] : m[2 * MS]);
          mm = std::min((mm + 1) >> 1, 6);
          int rctx;
          if (pos == 0) rctx = mm;
          else if (cls == CLASS_2D) rctx = (row < 2 && col < 2) ? mm + 7 : mm + 14;
          else rctx = (cls == CLASS_HORIZ ? col : row) == 0 ? mm + 7 : mm + 14;
          int rem = a - 3;
          for (int i = 0; i < 4; i++) {
            const int kk = rem > 3 ? 3 : rem;
            put_symbol_n<4>(ec, br_cdf[rctx], kk, adapt);
            rem -= kk;
            if (kk < 3) break;
          }
        }
      }
      // signs and Golomb remainders, first to last
      for (int k = 0; k < eob; k++) {
        const int pos = scan[k], v = lev[pos];
        if (!v) continue;
        const int a = std::abs(v);
        if (k == 0) {
          int sg = 0;
          for (int i = 0; i < nw; i++) sg += (ad[i] == 2) - (ad[i] == 1);
          for (int i = 0; i < nh; i++) sg += (ld[i] == 2) - (ld[i] == 1);
          put_symbol_n<2>(ec, cdf.dc_sign[ptype][sg < 0 ? 1 : sg > 0 ? 2 : 0], v < 0, adapt);
          dc_cat = v < 0 ? 1 : 2;
        } else {
          ec.bool_eq(v < 0);
        }
        if (a > 14) {    // read_golomb: x = a - 14 >= 1, length - 1 zeros then x in `length` bits
          const uint32_t x = (uint32_t)(a - 14);
          const int len = floor_log2(x) + 1;
          ec.literal(0, len - 1);
          ec.literal(x, len);
        }
        cul += a;
      }
      cul = std::min(cul, 63);
    }
    for (int i = 0; i < nw; i++) { al[i] = (uint8_t)cul; ad[i] = (uint8_t)dc_cat; }
    for (int i = 0; i < nh; i++) { ll[i] = (uint8_t)cul; ld[i] = (uint8_t)dc_cat; }
    return eob;
  }
};

}  // namespace core
}  // namespace av1
}  // namespace av1mi_host
