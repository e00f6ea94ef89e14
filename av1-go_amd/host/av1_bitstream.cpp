// av1_bitstream.cpp — see av1_bitstream.hpp.  Written from the AV1 Bitstream & Decoding Process Specification; section
// numbers in the comments are the specification's.  The default CDF tables come from av1_default_cdfs.inc (generated,
// tools/extract_av1_cdfs.py).  Conformance is checked by decoding with dav1d (tests/test_av1_conformance.py).
// This file holds what is particular to frames of 8x8 blocks: the partition tree split down to 8x8, the mode info of such a block and
// the MV prediction list among them.  The tile's coder state and everything below the block (restoration units, CDEF index,
// chroma-from-luma alphas, vector components, transform type, coefficients) is TileSyntax (av1_tile_syntax.hpp), shared with the
// general block writer (av1_blockstream.cpp).
#include "av1_bitstream.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "av1_tile_syntax.hpp"

namespace av1mi_host {
namespace av1 {
namespace {
using namespace core;

// ------------------------------------------------------------------------------------------------ one tile
struct MvCand { int16_t x, y; int weight; };

struct TileEnc : TileSyntax {
  int r8_0, r8_1, c8_0, c8_1;          // tile bounds in 8x8 blocks
  Txb txb[2][3];                       // the 4x4 (chroma) and 8x8 (luma) transforms of each class, made once per tile

  TileEnc(const FrameInfo &fi_, int tr, int tc) : TileSyntax(fi_) {
    reset_tile(tr, tc);
    r8_0 = mi_r0 >> 1; r8_1 = mi_r1 >> 1; c8_0 = mi_c0 >> 1; c8_1 = mi_c1 >> 1;
    for (int cls = 0; cls < 3; cls++) { txb[0][cls] = Txb(4, 4, cls); txb[1][cls] = Txb(8, 8, cls); }
  }
  inline int blk(int r8, int c8) const { return r8 * fi.w8 + c8; }
  inline bool avail_u(int r8) const { return r8 - 1 >= r8_0; }
  inline bool avail_l(int c8) const { return c8 - 1 >= c8_0; }
  inline int skip_of(int b) const { return f.skip ? f.skip[b] : 0; }
  inline int inter_of(int b) const { return fi.key ? 0 : (f.is_inter ? f.is_inter[b] : 1); }

  // ---- decode_tile (5.11.2)
  void run() {
    for (int r8 = r8_0; r8 < r8_1; r8 += 8) {
      clear_left_context();
      for (int c8 = c8_0; c8 < c8_1; c8 += 8) {
        cdef_coded = false;                                                 // clear_cdef
        write_lr(r8 * 2, c8 * 2);
        partition(r8 * 2, c8 * 2, 64);
      }
    }
    ec.finish();
  }

  // ---- decode_partition (5.11.4): always split down to 8x8
  void partition(int r, int c, int bsize) {
    if (r >= fi.mi_rows || c >= fi.mi_cols) return;
    const int half = bsize >> 3;      // halfBlock4x4
    const bool has_rows = r + half < fi.mi_rows, has_cols = c + half < fi.mi_cols;
    const bool au = (r >> 1) - 1 >= r8_0, al = (c >> 1) - 1 >= c8_0;
    if (bsize == 8) {
      sym(cdf.part8[0], 4, 0);        // PARTITION_NONE; the neighbours are 8x8 too, so the context is 0
      block(r >> 1, c >> 1);
      return;
    }
    // neighbours are 8x8 blocks, narrower than this one: ctx = left * 2 + above (9.3)
    uint16_t *pc = (bsize == 16 ? cdf.part16 : bsize == 32 ? cdf.part32 : cdf.part64)[(al ? 2 : 0) + (au ? 1 : 0)];
    if (has_rows && has_cols) {
      sym(pc, 10, 3);                 // PARTITION_SPLIT
    } else if (has_rows || has_cols) {
      // split_or_horz / split_or_vert: the probability of "split" gathers every partition type that splits the missing way
      auto prob = [&](int k) { return (uint32_t)((k ? pc[k - 1] : 32768) - pc[k]); };
      uint32_t psum;
      if (has_cols) psum = prob(2) + prob(3) + prob(4) + prob(6) + prob(7) + prob(9);   // VERT SPLIT HORZ_A VERT_A VERT_B VERT_4
      else psum = prob(1) + prob(3) + prob(4) + prob(5) + prob(6) + prob(8);            // HORZ SPLIT HORZ_A HORZ_B VERT_A HORZ_4
      ec.encode(psum, 0, 1, 2);       // the bit is 1 (split), cdf { 32768 - psum, 32768 }: no adaptation
    }
    const int q = bsize >> 1;
    partition(r, c, q); partition(r, c + half, q); partition(r + half, c, q); partition(r + half, c + half, q);
  }

  // ---- decode_block (5.11.5) of one 8x8 block
  void block(int r8, int c8) {
    const int b = blk(r8, c8);
    const bool au = avail_u(r8), al = avail_l(c8);
    const int skip = skip_of(b);
    if (fi.key) intra_frame_mode_info(r8, c8, b, au, al, skip);
    else inter_frame_mode_info(r8, c8, b, au, al, skip);
    // read_block_tx_size: TX_MODE_LARGEST, nothing coded.  residual (5.11.34): one 8x8 luma and two 4x4 chroma transform blocks, whose
    // context entries (units of 4 samples, tile / superblock relative) start at:
    const int x4 = (c8 - c8_0) * 2, y4 = (r8 & 7) * 2, cx4 = c8 - c8_0, cy4 = r8 & 7;
    if (skip) {   // reset_block_context
      a_lvl[0][x4] = a_lvl[0][x4 + 1] = a_dc[0][x4] = a_dc[0][x4 + 1] = 0;
      l_lvl[0][y4] = l_lvl[0][y4 + 1] = l_dc[0][y4] = l_dc[0][y4 + 1] = 0;
      for (int p = 1; p < 3; p++) a_lvl[p][cx4] = a_dc[p][cx4] = l_lvl[p][cy4] = l_dc[p][cy4] = 0;
      return;
    }
    const int is_inter = inter_of(b);
    const int tx_type = f.tx_type ? f.tx_type[b] : (int)T_DCT_DCT;
    const int set = is_inter ? (f.reduced_tx_set ? 5 : 3) : (f.reduced_tx_set ? 2 : 1);      // get_tx_set (5.11.48) of an 8x8 transform
    // all_zero context (9.3): 0 where the transform covers the whole block (luma)
    const int eob_y = coeffs(0, txb[1][tx_class_of(tx_type)], f.lev_y + (size_t)b * 64, 0, x4, y4, 2, 2, set, tx_type, f.y_mode ? f.y_mode[b] : 0);
    // compute_tx_type (5.11.40): the chroma blocks of an inter block take the coded luma type (a 4x4's inter set holds what an 8x8's
    // does); those of an intra block follow the mode, always of the 2-D class
    const Txb &tc = txb[0][is_inter && eob_y ? tx_class_of(tx_type) : (int)CLASS_2D];
    for (int p = 1; p < 3; p++) {
      const int above = a_lvl[p][cx4] | a_dc[p][cx4], left = l_lvl[p][cy4] | l_dc[p][cy4];
      coeffs(p, tc, (p == 1 ? f.lev_u : f.lev_v) + (size_t)b * 16, 7 + (above != 0) + (left != 0), cx4, cy4, 1, 1, 0, 0, 0);
    }
  }

  void write_skip(int b, bool au, bool al, int skip) {
    const int ctx = (au ? skip_of(b - fi.w8) : 0) + (al ? skip_of(b - 1) : 0);
    sym(cdf.skip[ctx], 2, skip);
  }
  // ---- intra_frame_mode_info (5.11.7)
  void intra_frame_mode_info(int r8, int c8, int b, bool au, bool al, int skip) {
    write_skip(b, au, al, skip);
    write_cdef((r8 >> 3) * fi.sb_cols + (c8 >> 3), skip);
    const int ym = f.y_mode[b];
    const int actx = kIntraModeContext[au ? f.y_mode[b - fi.w8] : (int)DC_PRED], lctx = kIntraModeContext[al ? f.y_mode[b - 1] : (int)DC_PRED];
    sym(cdf.kf_y_mode[actx][lctx], 13, ym);
    intra_tail(b, ym);
  }
  // intra_angle_info_y, uv_mode, read_cfl_alphas, intra_angle_info_uv (5.11.42 ..): shared by intra blocks of both frame types
  void intra_tail(int b, int ym) {
    if (is_directional(ym)) sym(cdf.angle_delta[ym - V_PRED], 7, (f.angle_y ? f.angle_y[b] : 0) + 3);
    const int uvm = f.uv_mode[b];
    sym(cdf.uv_mode_cfl[ym], 14, uvm);          // an 8x8 block allows chroma from luma
    if (uvm == UV_CFL_PRED) {
      write_cfl_alphas(f.cfl_alpha ? f.cfl_alpha[2 * b] : 0, f.cfl_alpha ? f.cfl_alpha[2 * b + 1] : 0);
    } else if (is_directional(uvm)) {
      sym(cdf.angle_delta[uvm - V_PRED], 7, (f.angle_uv ? f.angle_uv[b] : 0) + 3);
    }
  }

  void inter_frame_mode_info(int r8, int c8, int b, bool au, bool al, int skip);   // below
  void mv_stack(int r8, int c8, MvCand *stack, int *num, int *new_ctx, int *ref_ctx);
};

// ---- inter frames.  Tool set: single reference LAST_FRAME, modes NEWMV / NEARESTMV / NEARMV / GLOBALMV (whichever codes the
// encoder's vector), no segmentation, no skip mode, no compound, simple translation, fixed interpolation filter; intra blocks
// are allowed.  All blocks are 8x8, so every candidate of the MV prediction list has weight 2 * len = 4 (7.10.2.2 - 7.10.2.4).
inline unsigned morton8(unsigned x, unsigned y) {   // z-order index inside a superblock of 8 x 8 blocks
  unsigned m = 0;
  for (int i = 0; i < 3; i++) m |= ((x >> i) & 1u) << (2 * i) | ((y >> i) & 1u) << (2 * i + 1);
  return m;
}

// find_mv_stack (7.10.2) for a single-reference block: the list, its weights, and the mode contexts
void TileEnc::mv_stack(int r8, int c8, MvCand *stack, int *num_out, int *new_ctx, int *ref_ctx) {
  int num = 0, new_count = 0;
  bool found = false;
  auto inside = [&](int r, int c) { return r >= r8_0 && r < r8_1 && c >= c8_0 && c < c8_1; };
  auto add = [&](int r, int c, bool count_new) {     // add_ref_mv_candidate + search_stack_process (7.10.2.7, 7.10.2.8), weight 4
    if (!inside(r, c)) return;
    const int nb = blk(r, c);
    if (!inter_of(nb)) return;                        // intra neighbour: no candidate
    const int16_t mx = f.mv[2 * nb], my = f.mv[2 * nb + 1];   // already at quarter-sample precision: lower_mv_precision is the identity
    if (count_new && (*fi.newmv)[(size_t)nb]) new_count++;
    found = true;
    int i = 0;
    for (; i < num; i++) if (stack[i].x == mx && stack[i].y == my) break;
    if (i < num) stack[i].weight += 4;
    else if (num < 8) { stack[num].x = mx; stack[num].y = my; stack[num].weight = 4; num++; }
  };
  add(r8 - 1, c8, true);                              // scan_row(-1)
  const bool above0 = found; found = false;
  add(r8, c8 - 1, true);                              // scan_col(-1)
  const bool left0 = found; found = false;
  {   // scan_point(-1, bw4): the top-right block counts only if it has been decoded already
    const int tr = r8 - 1, tc = c8 + 1;
    bool decoded = false;
    if (inside(tr, tc)) {
      if ((tr >> 3) < (r8 >> 3)) decoded = true;                       // superblock row above
      else if ((tc >> 3) == (c8 >> 3)) decoded = morton8(tc & 7, tr & 7) < morton8(c8 & 7, r8 & 7);
    }
    if (decoded) add(tr, tc, true);
  }
  bool above = above0 || found; found = false;
  const int close = (above ? 1 : 0) + (left0 ? 1 : 0);
  const int num_nearest = num, num_new = new_count;
  for (int i = 0; i < num_nearest; i++) stack[i].weight += 640;   // REF_CAT_LEVEL
  // (no temporal candidates: use_ref_frame_mvs = 0, ZeroMvContext = 0)
  add(r8 - 1, c8 - 1, false);                         // scan_point(-1, -1)
  above = above || found; found = false;
  bool left = left0;
  add(r8 - 2, c8, false); above = above || found; found = false;      // scan_row(-3)
  add(r8, c8 - 2, false); left = left || found; found = false;        // scan_col(-3)
  add(r8 - 3, c8, false); above = above || found; found = false;      // scan_row(-5)
  add(r8, c8 - 3, false); left = left || found; found = false;        // scan_col(-5)
  const int total = (above ? 1 : 0) + (left ? 1 : 0);
  // sorting process (7.10.2.11): the nearest entries, then the rest, each by descending weight (stable bubble sort)
  auto sort_range = [&](int a, int b) {
    for (int len = b; len > a;) {
      int nr = a;
      for (int i = a + 1; i < len; i++)
        if (stack[i - 1].weight < stack[i].weight) { std::swap(stack[i - 1], stack[i]); nr = i; }
      len = nr;
    }
  };
  sort_range(0, num_nearest);
  sort_range(num_nearest, num);
  // extra search process (7.10.2.12): adds vectors of neighbours that use OTHER reference frames; every inter block here uses
  // LAST_FRAME, so its vector is in the list already.  Context and clamping process (7.10.2.14):
  if (close == 0) { *new_ctx = std::min(total, 1); *ref_ctx = total; }
  else if (close == 1) { *new_ctx = 3 - std::min(num_new, 1); *ref_ctx = 2 + total; }
  else { *new_ctx = 5 - std::min(num_new, 1); *ref_ctx = 5; }
  const int mi_r = r8 * 2, mi_c = c8 * 2;
  const int border = 128 + 2 * 4 * 8;                 // MV_BORDER + block size in 1/8 samples
  const int top = -(mi_r * 4 * 8) - border, bottom = (fi.mi_rows - 2 - mi_r) * 4 * 8 + border;
  const int lft = -(mi_c * 4 * 8) - border, right = (fi.mi_cols - 2 - mi_c) * 4 * 8 + border;
  for (int i = 0; i < num; i++) {
    stack[i].y = (int16_t)std::min(std::max<int>(stack[i].y, top), bottom);
    stack[i].x = (int16_t)std::min(std::max<int>(stack[i].x, lft), right);
  }
  for (int i = num; i < 2; i++) { stack[i].x = stack[i].y = 0; stack[i].weight = 0; }   // GlobalMvs: identity
  *num_out = num;
}

void TileEnc::inter_frame_mode_info(int r8, int c8, int b, bool au, bool al, int skip) {
  write_skip(b, au, al, skip);      // inter_segment_id, read_skip_mode: nothing to code
  write_cdef((r8 >> 3) * fi.sb_cols + (c8 >> 3), skip);
  const int is_inter = inter_of(b);
  write_is_inter(au, al, au && !inter_of(b - fi.w8), al && !inter_of(b - 1), is_inter);
  if (!is_inter) {   // intra_block_mode_info (5.11.22): y_mode with the size-group context (Size_Group[BLOCK_8X8] = 1)
    const int ym = f.y_mode[b];
    sym(cdf.y_mode[1], 13, ym);
    intra_tail(b, ym);
    (*fi.newmv)[(size_t)b] = 0;
    return;
  }
  // read_ref_frames (5.11.25): single_ref_p1 = 0, single_ref_p3 = 0, single_ref_p4 = 0 -> LAST_FRAME.  The contexts compare
  // counts of neighbouring references (9.3): only LAST_FRAME ever occurs, so each is 1 (no inter neighbour) or 2.
  const int n_last = (au && inter_of(b - fi.w8) ? 1 : 0) + (al && inter_of(b - 1) ? 1 : 0);
  const int rctx = n_last ? 2 : 1;
  sym(cdf.single_ref[rctx][0], 2, 0);
  sym(cdf.single_ref[rctx][2], 2, 0);
  sym(cdf.single_ref[rctx][3], 2, 0);
  MvCand st[8];
  int num, new_ctx, ref_ctx;
  mv_stack(r8, c8, st, &num, &new_ctx, &ref_ctx);
  const int mx = f.mv[2 * b], my = f.mv[2 * b + 1];
  // the cheapest mode that reproduces the encoder's vector: NEARESTMV, NEARMV (index 1..3), GLOBALMV, else NEWMV
  int mode = 3, ref_idx = 0;      // 0 NEARESTMV, 1 NEARMV, 2 GLOBALMV, 3 NEWMV
  if (st[0].x == mx && st[0].y == my) mode = 0;
  else {
    for (int i = 1; i < std::max(num, 2) && i < 4; i++)
      if (st[i].x == mx && st[i].y == my) { mode = 1; ref_idx = i; break; }
    if (mode == 3 && mx == 0 && my == 0) mode = 2;
  }
  sym(cdf.new_mv[new_ctx], 2, mode != 3);
  if (mode != 3) {
    sym(cdf.zero_mv[0], 2, mode != 2);
    if (mode != 2) sym(cdf.ref_mv[ref_ctx], 2, mode == 1);
  }
  auto drl_ctx = [&](int i) {     // drl_mode context from the weights of entries i and i + 1 (9.3)
    const bool a = st[i].weight >= 640, c = st[i + 1].weight >= 640;
    return a && c ? 0 : a ? 1 : !c ? 2 : 0;
  };
  if (mode == 3) {
    // NEWMV: the predictor is entry RefMvIdx of the list; pick the closest of the entries the syntax can name (0..2)
    const int nsel = std::min(num, 3);
    long best = -1;
    for (int i = 0; i < std::max(nsel, 1); i++) {
      const long c = std::abs(mx - st[i].x) + std::abs(my - st[i].y);
      if (best < 0 || c < best) { best = c; ref_idx = i; }
    }
    for (int i = 0; i < 2; i++)
      if (num > i + 1) {
        sym(cdf.drl[drl_ctx(i)], 2, ref_idx != i);
        if (ref_idx == i) break;
      }
    const int pred = num <= 1 ? 0 : ref_idx;            // assign_mv (5.11.26)
    const int dx = mx - st[pred].x, dy = my - st[pred].y;   // read_mv (5.11.32): component 0 is the row (vertical) difference
    sym(cdf.mv_joint, 4, (dx ? 1 : 0) + (dy ? 2 : 0));
    if (dy) write_mv_comp(cdf.mv[0], dy, false);      // quarter-sample precision: the differences are even
    if (dx) write_mv_comp(cdf.mv[1], dx, false);
  } else if (mode == 1) {
    for (int i = 1; i < 3; i++)
      if (num > i + 1) {
        sym(cdf.drl[drl_ctx(i)], 2, ref_idx != i);
        if (ref_idx == i) break;
      }
  }
  (*fi.newmv)[(size_t)b] = mode == 3;
  // read_interintra_mode, read_motion_mode, read_compound_type, interpolation filter: nothing to code with this tool set
}


}  // namespace

// ------------------------------------------------------------------------------------------------ public
std::vector<uint8_t> temporal_delimiter_obu() { return make_obu(2, {}); }

std::vector<uint8_t> sequence_header_obu(const SequenceParams &sp) {   // sequence_header_obu (5.5.1)
  BitWriter w;
  w.put(0, 3);      // seq_profile 0: 4:2:0, 8 / 10 bit
  w.put(0, 1);      // still_picture
  w.put(0, 1);      // reduced_still_picture_header
  w.put(0, 1);      // timing_info_present_flag
  w.put(0, 1);      // initial_display_delay_present_flag
  w.put(0, 5);      // operating_points_cnt_minus_1
  w.put(0, 12);     // operating_point_idc[0]
  w.put(31, 5);     // seq_level_idx[0] = 31: "maximum parameters" (one tile per superblock exceeds every numbered level's tile count)
  w.put(0, 1);      // seq_tier[0]
  const int wb = floor_log2((uint32_t)std::max(sp.width - 1, 1)) + 1, hb = floor_log2((uint32_t)std::max(sp.height - 1, 1)) + 1;
  w.put((uint32_t)(wb - 1), 4); w.put((uint32_t)(hb - 1), 4);
  w.put((uint32_t)(sp.width - 1), wb); w.put((uint32_t)(sp.height - 1), hb);
  w.put(0, 1);      // frame_id_numbers_present_flag
  w.put(0, 1);      // use_128x128_superblock
  w.put(0, 1);      // enable_filter_intra
  w.put(1, 1);      // enable_intra_edge_filter
  w.put(0, 1);      // enable_interintra_compound
  w.put(0, 1);      // enable_masked_compound
  w.put(0, 1);      // enable_warped_motion
  w.put(0, 1);      // enable_dual_filter
  w.put(0, 1);      // enable_order_hint
  w.put(0, 1);      // seq_choose_screen_content_tools
  w.put(0, 1);      // seq_force_screen_content_tools = 0 (so seq_force_integer_mv = SELECT_INTEGER_MV, not coded)
  w.put(0, 1);      // enable_superres
  w.put(1, 1);      // enable_cdef
  w.put(1, 1);      // enable_restoration
  write_color_config(w, sp);
  w.put(sp.film_grain ? 1 : 0, 1);      // film_grain_params_present
  w.trailing_bits();
  return make_obu(1, w.b);
}


const char *colour_error(const av1mi_colour &c) {
  if (c.primaries < 0 || c.primaries > 255 || c.transfer < 0 || c.transfer > 255 || c.matrix < 0 || c.matrix > 255) return "colour: a code point does not fit in eight bits";
  if (c.matrix == 0) return "colour: matrix_coefficients 0 (identity) implies 4:4:4 (the spec's sRGB case), which is not coded";
  if (c.full_range != 0 && c.full_range != 1) return "colour: full_range must be 0 or 1";
  return nullptr;
}

static std::vector<uint8_t> metadata_obu(int type, BitWriter &w) {   // metadata_obu (5.8.1): metadata_type leb128, the payload, trailing bits
  w.trailing_bits();
  std::vector<uint8_t> p;
  put_leb128(p, (uint64_t)type);
  p.insert(p.end(), w.b.begin(), w.b.end());
  return make_obu(5, p);
}
std::vector<uint8_t> metadata_obu_hdr_cll(const av1mi_colour &c) {   // metadata_hdr_cll (5.8.3)
  BitWriter w;
  w.put(c.max_cll, 16); w.put(c.max_fall, 16);
  return metadata_obu(1, w);
}
std::vector<uint8_t> metadata_obu_hdr_mdcv(const av1mi_colour &c) {  // metadata_hdr_mdcv (5.8.4)
  BitWriter w;
  for (int i = 0; i < 3; i++) { w.put(c.primary_x[i], 16); w.put(c.primary_y[i], 16); }
  w.put(c.white_x, 16); w.put(c.white_y, 16);
  w.put(c.luminance_max >> 16, 16); w.put(c.luminance_max & 0xFFFF, 16);      // (the writer's put takes up to 32 bits; two halves keep the shifts plain)
  w.put(c.luminance_min >> 16, 16); w.put(c.luminance_min & 0xFFFF, 16);
  return metadata_obu(2, w);
}
void append_sequence_obus(const SequenceParams &sp, std::vector<uint8_t> *out) {
  const std::vector<uint8_t> sh = sequence_header_obu(sp);
  out->insert(out->end(), sh.begin(), sh.end());
  if (sp.colour.have_cll) { const std::vector<uint8_t> m = metadata_obu_hdr_cll(sp.colour); out->insert(out->end(), m.begin(), m.end()); }
  if (sp.colour.have_mdcv) { const std::vector<uint8_t> m = metadata_obu_hdr_mdcv(sp.colour); out->insert(out->end(), m.begin(), m.end()); }
}

bool frame_obu_from_tiles(const av1mi_obu_frame &f, const uint8_t *payloads, const uint32_t *sizes, int ntiles, std::vector<uint8_t> *out,
                          std::string *err) {
  if (!check(f, err, false)) return false;
  const FrameInfo fi = frame_info(f);
  if (ntiles != fi.tile_cols * fi.tile_rows) { if (err) *err = "tile count does not match the frame"; return false; }
  std::vector<const uint8_t *> data((size_t)ntiles);
  std::vector<size_t> size((size_t)ntiles);
  for (int t = 0; t < ntiles; t++) {
    if (sizes[t] == 0) { if (err) *err = "empty tile payload"; return false; }
    data[(size_t)t] = payloads; size[(size_t)t] = sizes[t]; payloads += sizes[t];
  }
  return assemble_frame(fi, data.data(), size.data(), out);
}

bool frame_obu(const av1mi_obu_frame &f, int threads, std::vector<uint8_t> *out, std::string *err) {
  if (!check(f, err)) return false;
  FrameInfo fi = frame_info(f);
  std::vector<uint8_t> newmv((size_t)fi.w8 * fi.h8, 0);
  fi.newmv = &newmv;
  const int ntiles = fi.tile_cols * fi.tile_rows;
  std::vector<std::vector<uint8_t>> tiles((size_t)ntiles);
  std::atomic<int> next(0);
  auto work = [&] {
    for (int t; (t = next.fetch_add(1)) < ntiles;) {
      TileEnc te(fi, t / fi.tile_cols, t % fi.tile_cols);
      te.run();
      tiles[(size_t)t].swap(te.ec.out);
    }
  };
  const int nt = std::max(1, std::min(threads, ntiles));
  if (nt == 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    for (int i = 0; i < nt; i++) pool.emplace_back(work);
    for (auto &t : pool) t.join();
  }
  std::vector<const uint8_t *> data((size_t)ntiles);
  std::vector<size_t> size((size_t)ntiles);
  for (int t = 0; t < ntiles; t++) { data[(size_t)t] = tiles[(size_t)t].data(); size[(size_t)t] = tiles[(size_t)t].size(); }
  return assemble_frame(fi, data.data(), size.data(), out);
}

bool temporal_unit(const av1mi_obu_frame &f, bool with_sequence_header, int threads, std::vector<uint8_t> *out, std::string *err) {
  std::vector<uint8_t> fr;
  if (!frame_obu(f, threads, &fr, err)) return false;
  *out = temporal_delimiter_obu();
  if (with_sequence_header) append_sequence_obus(sequence_params(f), out);
  out->insert(out->end(), fr.begin(), fr.end());
  return true;
}

std::vector<uint8_t> range_code_raw(const uint32_t *fl, const uint32_t *fh, const uint8_t *sym, const uint8_t *nsym, size_t count) {
  RangeEnc ec;
  for (size_t i = 0; i < count; i++) ec.encode(fl[i], fh[i], sym[i], nsym[i]);
  ec.finish();
  return ec.out;
}

}  // namespace av1
}  // namespace av1mi_host
