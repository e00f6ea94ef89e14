// av1_opstream.cpp — the CPU twin of the GPU tile entropy coder: the three-stage formulation of csrc/av1_ops.hpp (tokenize per
// block with all contexts from neighbour data; one adaptation chain per CDF slot; one serial range-coder pass per tile) run on
// the host, so that its logic is checked byte for byte against the block-sequential writer of av1_bitstream.cpp on every
// machine, GPU or not (tests/test_av1_opstream.py).  Also the reference the GPU kernels' output is compared with.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../csrc/av1_ops_cdfs.hpp"
#include "../csrc/av1_ops8.hpp"
#include "av1_bitstream.hpp"

namespace av1mi_host {
namespace av1 {

// true when the description stays inside the GPU coder's tool set (what the GPU block pipeline produces)
bool opstream_supported(const av1mi_obu_frame &f, std::string *why) {
  auto no = [&](const char *m) { if (why) *why = m; return false; };
  if (f.cdef_bits < 0 || f.cdef_bits > 3) return no("cdef_bits outside 0 .. 3");      // (a null cdef_idx is index 0 everywhere, as in the host writers)
  if (f.reduced_tx_set || f.disable_cdf_update) return no("reduced_tx_set / disable_cdf_update must be 0");
  if (f.tile_cols_log2 >= 0 || f.tile_rows_log2 >= 0) return no("one superblock per tile only");
  if (f.angle_y || f.angle_uv || f.cfl_alpha || f.tx_type || f.is_inter) return no("angle deltas, chroma from luma, transform types and intra blocks in inter frames are host-writer only");
  if (f.frame_type == 0 && f.skip) return no("key frames are coded with skip = 0");
  for (int p = 0; p < 3; p++) if (f.lr_type[p] > 1) return no("Wiener restoration only");
  if (f.lr_unit_shift || f.lr_uv_shift) return no("64x64 restoration units only");
  return true;
}

namespace {
// stages 2 and 3 of a tile whose list holds the literals and whose adaptive symbols are grouped by slot (totals, bases): one chain per
// slot from the default CDFs `image` (the GPU: one lane per (tile, slot)), the serial range coder over the finished list (the GPU: one
// lane per tile)
bool code_list(std::vector<av1ops::op_t> &list, const std::vector<uint32_t> &grouped, int nslots, const uint16_t *total, const uint16_t *base,
               const av1ops::SlotTable &tab, const uint16_t *image, std::vector<uint8_t> *out, std::string *err) {
  using namespace av1ops;
  const int nops = (int)list.size();
  for (int sl = 0; sl < nslots; sl++)
    if (total[sl]) run_chain(&image[tab.off[sl]], tab.nsym[sl], &grouped[(size_t)base[sl]], total[sl], list.data());
  out->resize((size_t)nops * 2 + 64);       // a step adds at most 15 bits
  Coder c;
  uint16_t stage[Coder::kStage];
  c.init(out->data(), (int)out->size(), stage);
  for (int i = 0; i < nops; i++) code_word(c, list[(size_t)i]);
  const int n = c.finish();
  if (n < 0) { if (err) *err = "tile payload overflow"; return false; }
  out->resize((size_t)n);
  return true;
}
// the wave of the tile tokenizers (av1_ops32.hpp tok_tile32, av1_ops8.hpp tok_tile8) as a loop: the lanes of a phase one after the other
struct WaveLoop {
  template <class T> using Var = av1ops::LaneVar<T, av1ops::kLanes32>;
  template <class F> void each(F f) { for (int lane = 0; lane < av1ops::kLanes32; lane++) f(lane); }
  int scan(Var<int> &v) {
    int run = 0;
    for (int lane = 0; lane < av1ops::kLanes32; lane++) { const int x = v.v[lane]; v.v[lane] = run; run += x; }
    return run;
  }
  int first(Var<int> &v) { return v.v[0]; }
  uint64_t ballot(Var<int> &v) {
    uint64_t m = 0;
    for (int lane = 0; lane < av1ops::kLanes32; lane++) m |= (uint64_t)(v.v[lane] != 0) << lane;
    return m;
  }
};
void frame_view_of(const av1mi_obu_frame &f, av1ops::FrameView *v) {
  memset(v, 0, sizeof(*v));
  v->w8 = f.width / 8; v->h8 = f.height / 8; v->key = f.frame_type == 0;
  v->y_mode = f.y_mode; v->uv_mode = f.uv_mode; v->mv = f.mv; v->skip = f.skip; v->lev_y = f.lev_y; v->lev_u = f.lev_u; v->lev_v = f.lev_v;
  v->cdef_bits = f.cdef_bits; v->cdef_idx = f.cdef_bits ? f.cdef_idx : nullptr;
  for (int p = 0; p < 3; p++) {
    v->lr_on[p] = f.lr_type[p] == 1;
    const int ph = p ? (visible_height(f) + 1) >> 1 : visible_height(f), pw = p ? (visible_width(f) + 1) >> 1 : visible_width(f);
    v->lr_rows[p] = std::max((ph + 32) / 64, 1); v->lr_cols[p] = std::max((pw + 32) / 64, 1);
  }
}
// the op-stream coder reads a unit's own record where the plane's records differ (FrameView::lr_units: the restoration search's
// choice, Wiener or none), and the one shared record per plane class where they are all alike (what the session's policy produces:
// the path the GPU coder takes with null arrays, so the two are compared on every frame of that kind)
bool lr_units_of(const av1mi_obu_frame &f, av1ops::FrameView *v, std::string *err) {
  bool shared = true;
  for (int p = 0; p < 3; p++) {
    if (!v->lr_on[p]) continue;
    const int8_t *u = f.lr_units[p];
    const size_t n = (size_t)v->lr_rows[p] * v->lr_cols[p];
    for (size_t i = 0; i < n; i++) {
      if (u[i * 8] != 0 && u[i * 8] != 1) { if (err) *err = "Wiener restoration units only"; return false; }
      if (memcmp(u, u + i * 8, 8)) shared = false;
    }
    if (p == 2 && v->lr_on[1] && memcmp(u, f.lr_units[1], 8)) shared = false;
  }
  for (int p = 0; p < 3; p++) {
    if (!v->lr_on[p]) continue;
    if (shared) memcpy(v->lr_unit[p ? 1 : 0], f.lr_units[p], 8);
    else v->lr_units[p] = f.lr_units[p];
  }
  return true;
}
}  // namespace

// tile payloads (range-coded, finished) of a frame through tokenize + code; tiles in raster order
// key_rows32 > 0: a key frame whose first key_rows32 luma rows (whole superblock rows) are coded in 32x32 blocks (av1_ops32.hpp; the
// symbol arrays in the session's layout: those rows' modes one per 32x32 block from entry 0, levels block-contiguous over the 32x32
// grid; the rows below in the 8x8 layout at their usual places)
bool opstream_tiles(const av1mi_obu_frame &f, std::vector<std::vector<uint8_t>> *tiles, std::string *err, int key_rows32) {
  using namespace av1ops;
  if (!opstream_supported(f, err)) return false;
  if (key_rows32 && (f.frame_type != 0 || (key_rows32 & 63) || key_rows32 > f.height || (f.width & 31))) { if (err) *err = "bad 32x32 band"; return false; }
  FrameView v;
  frame_view_of(f, &v);
  std::vector<uint8_t> zskip;
  if (!v.key && !v.skip) { zskip.assign((size_t)v.w8 * v.h8, 0); v.skip = zskip.data(); }
  if (!lr_units_of(f, &v, err)) return false;
  const size_t nb = (size_t)v.w8 * v.h8;
  std::vector<BlockInfo> info(nb);
  v.info = info.data();
  for (size_t b = 0; b < nb; b++) memset(&info[b], 0, sizeof(BlockInfo));
  if (!v.key) for (int r = 0; r < v.h8; r++) for (int c = 0; c < v.w8; c++) inter_mode_decision(v, r, c, &info[(size_t)r * v.w8 + c]);
  const int qcat = q_category(f.base_q_idx);
  SlotTable tab;
  const std::vector<uint16_t> image = default_slot_image(v.key != 0, qcat, &tab);
  const int sbr_n = (v.h8 + 7) / 8, sbc_n = (v.w8 + 7) / 8;
  tiles->assign((size_t)sbr_n * sbc_n, {});
  const int nslots = v.key ? S_KEY_END : S_INTER_END;
  // what a tile's wave of 8x8 blocks keeps in LDS, its records, and its outputs
  std::vector<Tile8Mem> mem8(1);
  std::vector<uint16_t> rec((size_t)kBlocksPerTile * kBlockRecords);
  const uint32_t ops_cap8 = 1u << 20;        // (no tile has as many words)
  std::vector<op_t> list8(ops_cap8);
  std::vector<uint32_t> grouped8(65536 + kListAlign);
  // AV1MI_TOK_STATS=1 (diagnostic): the capacities a frame would need — records per block, symbols of one slot in one block, list
  // words per tile — to stderr; tiles over capacity are skipped instead of failing the call
  const bool stats = getenv("AV1MI_TOK_STATS") != nullptr;
  int st_rec = 0, st_cnt = 0, st_ops = 0, st_over = 0; long st_ops_sum = 0;
  // the 32x32 band's own slot table and default CDFs, and what a tile's wave keeps in LDS
  SlotTable tab32;
  const std::vector<uint16_t> image32 = key_rows32 ? default_slot_image_k32(qcat, &tab32) : std::vector<uint16_t>();
  std::vector<Tile32Mem> mem32(key_rows32 ? 1 : 0);
  const uint32_t ops_cap32 = 1u << 20;       // (no tile has as many words: 4 x 1536 coefficients)
  std::vector<op_t> list32(key_rows32 ? ops_cap32 : 0);
  std::vector<uint32_t> grouped32(key_rows32 ? 65536 : 0);
  for (int sbr = 0; sbr < sbr_n; sbr++)
    for (int sbc = 0; sbc < sbc_n; sbc++) {
      if (sbr * 64 < key_rows32) {
        // a tile of the 32x32 band: the lanes of its wave over scan ranges (tok_tile32), then the same chains and the same range coder
        WaveLoop wave;
        uint16_t base[S_MAX], total[S_MAX];
        CallerAreas out = { list32.data(), grouped32.data(), total, base };
        const int words = tok_tile32(wave, mem32[0], v, sbr, sbc, ops_cap32, out);
        if (words < 0) { if (err) *err = "tile too large for 16-bit entry positions"; return false; }
        std::vector<op_t> list(list32.begin(), list32.begin() + words);
        if (!code_list(list, grouped32, K_END, total, base, tab32, image32.data(), &(*tiles)[(size_t)sbr * sbc_n + sbc], err)) return false;
        continue;
      }
      // stage 1 (av1_ops8.hpp tok_tile8, the GPU: a lane per block): summaries, records + counts, place, replay
      WaveLoop wave;
      uint16_t base[S_MAX], total[S_MAX];
      CallerAreas out = { list8.data(), grouped8.data(), total, base };
      const int words = tok_tile8(wave, mem8[0], v, sbr, sbc, rec.data(), ops_cap8, out);
      if (stats) {       // the blocks once more, one by one, for what the tile's call does not tell
        std::vector<uint8_t> cnt((size_t)S_MAX * kBlocksPerTile, 0);
        const TokScratch ts = { mem8[0].p1.mag, &mem8[0].scan };
        int ops = 0;
        for (int zi = 0; zi < kBlocksPerTile; zi++) {
          Sink k = { rec.data(), cnt.data(), zi, 0, 0, false };
          tok_block(v, k, ts, sbr, sbc, zi, mem8[0].sums, -1);
          st_rec = std::max(st_rec, k.nrec); ops += k.n;
        }
        for (uint8_t c : cnt) st_cnt = std::max(st_cnt, (int)c);
        st_ops = std::max(st_ops, ops); st_ops_sum += ops;
        if (words < 0) { st_over++; continue; }
      }
      if (words < 0) { if (err) *err = "a tile exceeds the tokenizer's capacities (records or symbols of a slot per block, entries per tile)"; return false; }
      std::vector<op_t> list(list8.begin(), list8.begin() + words);
      if (!code_list(list, grouped8, nslots, total, base, tab, image.data(), &(*tiles)[(size_t)sbr * sbc_n + sbc], err)) return false;
    }
  if (stats)
    fprintf(stderr, "[av1mi tok stats] %d tiles: records per block <= %d (capacity %d), symbols of a slot in a block <= %d (255), list words per tile <= %d, mean %.0f; %d tiles over a block capacity\n",
            sbr_n * sbc_n, st_rec, (int)kBlockRecords, st_cnt, st_ops, (double)st_ops_sum / (sbr_n * sbc_n), st_over);
  return true;
}

int opstream_slots() { return av1ops::S_MAX; }

// One tile of 8x8 blocks (key or inter frame) through tok_tile8 into the caller's areas, as the GPU kernel calls it (tests: the
// capacity of the list is the caller's): returns the list words, -1 when the tile is refused (then nothing but the totals is written),
// -2 for a frame outside the tool set
int opstream_tile8(const av1mi_obu_frame &f, int sbr, int sbc, uint32_t ops_cap, uint32_t *list, uint32_t *grouped, uint16_t *slot_total, uint16_t *slot_base,
                   std::string *err) {
  using namespace av1ops;
  if (!opstream_supported(f, err) || sbr < 0 || sbc < 0 || sbr * 64 >= f.height || sbc * 64 >= f.width) return -2;
  FrameView v;
  frame_view_of(f, &v);
  std::vector<uint8_t> zskip;
  if (!v.key && !v.skip) { zskip.assign((size_t)v.w8 * v.h8, 0); v.skip = zskip.data(); }
  if (!lr_units_of(f, &v, err)) return -2;
  std::vector<BlockInfo> info(v.key ? 0 : (size_t)v.w8 * v.h8);
  v.info = info.data();
  if (!v.key) for (int r = 0; r < v.h8; r++) for (int c = 0; c < v.w8; c++) { memset(&info[(size_t)r * v.w8 + c], 0, sizeof(BlockInfo)); inter_mode_decision(v, r, c, &info[(size_t)r * v.w8 + c]); }
  std::vector<Tile8Mem> mem(1);
  std::vector<uint16_t> rec((size_t)kBlocksPerTile * kBlockRecords);
  WaveLoop wave;
  CallerAreas out = { list, grouped, slot_total, slot_base };
  return tok_tile8(wave, mem[0], v, sbr, sbc, rec.data(), ops_cap, out);
}

// One tile of a key frame's 32x32 band through tok_tile32 into the caller's areas, as the GPU kernel calls it (tests: the capacity of
// the list is the caller's): returns the list words, -1 when the tile does not fit (then nothing but the totals and bases is written),
// -2 for a frame outside the tool set
int opstream_tile32(const av1mi_obu_frame &f, int sbr, int sbc, uint32_t ops_cap, uint32_t *list, uint32_t *grouped, uint16_t *slot_total, uint16_t *slot_base,
                    std::string *err) {
  using namespace av1ops;
  if (!opstream_supported(f, err) || f.frame_type != 0 || (f.width & 31) || sbr < 0 || sbc < 0 || (sbr + 1) * 64 > f.height || sbc * 64 >= f.width) return -2;
  FrameView v;
  frame_view_of(f, &v);
  if (!lr_units_of(f, &v, err)) return -2;
  std::vector<Tile32Mem> mem(1);
  WaveLoop wave;
  CallerAreas out = { list, grouped, slot_total, slot_base };
  return tok_tile32(wave, mem[0], v, sbr, sbc, ops_cap, out);
}

}  // namespace av1
}  // namespace av1mi_host
