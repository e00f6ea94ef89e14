// session_unit.cpp — a collected batch's segment becomes a temporal unit: the frame description the bitstream writer takes
// (DescribeSessionFrame) and the three ways to the bytes (SessionTemporalUnit): GPU-coded tiles wrapped in a frame header, a key frame in
// 32x32 blocks through the general block writer, everything else through the 8x8 writer on the host cores.  Declared in backend.hpp;
// backend.cpp calls it for every frame a job writes, capi_host.cpp exports it (include/av1mi_host.h av1mi_session_temporal_unit).
#include <cstring>
#include <string>
#include <vector>
#include "backend.hpp"
#include "av1_bitstream.hpp"

namespace av1mi_host {

void DescribeSessionFrame(const av1mi_gop_frame &fr, int seg, int width, int height, int bit_depth, SessionFrameDesc *d, int visible_width, int visible_height) {
  const av1mi_frame_params &p = fr.params;
  av1mi_obu_frame &f = d->f;
  memset(&f, 0, sizeof(f));
  f.width = width; f.height = height; f.bit_depth = bit_depth; f.frame_type = p.frame_type; f.base_q_idx = p.base_q_idx;
  f.visible_width = visible_width; f.visible_height = visible_height;
  for (int i = 0; i < 4; i++) f.lf_level[i] = fr.lf_levels ? fr.lf_levels[(size_t)seg * 4 + i] : p.lf_level[i];      // (lf_levels: a session with the deblocking search)
  f.lf_sharpness = p.lf_sharpness; f.cdef_damping = p.cdef_damping; f.cdef_bits = 0; f.cdef_y[0] = p.cdef_y; f.cdef_uv[0] = p.cdef_uv;
  if (fr.cdef_bits) {      // a session with the CDEF search: the batch's strength sets and the segment's index per superblock
    f.cdef_bits = fr.cdef_bits;
    memcpy(f.cdef_y, fr.cdef_y, 8); memcpy(f.cdef_uv, fr.cdef_uv, 8);
    if (fr.cdef_idx) f.cdef_idx = fr.cdef_idx + (size_t)seg * ((width + 63) / 64) * ((height + 63) / 64);
  }
  auto units = [&](int n) { const int u = (n + p.lr_unit_size / 2) / p.lr_unit_size; return u > 1 ? u : 1; };
  const int vw = visible_width ? visible_width : width, vh = visible_height ? visible_height : height;      // the units tile the TRUE frame
  const size_t uy = (size_t)units(vh) * units(vw), uc = (size_t)units((vh + 1) / 2) * units((vw + 1) / 2);
  d->lr_y.resize(uy * 8); d->lr_uv.resize(uc * 8);
  for (size_t i = 0; i < uy; i++) memcpy(&d->lr_y[i * 8], p.lr_unit_y, 8);
  for (size_t i = 0; i < uc; i++) memcpy(&d->lr_uv[i * 8], p.lr_unit_uv, 8);
  // restoration per plane: the policy's type where the encoder kept it ON for this segment's frame (fr.lr_on), NONE elsewhere
  const uint8_t *on = fr.lr_on ? fr.lr_on + (size_t)seg * 3 : nullptr;
  f.lr_type[0] = (!on || on[0]) ? p.lr_unit_y[0] : 0;
  f.lr_type[1] = (!on || on[1]) ? p.lr_unit_uv[0] : 0;
  f.lr_type[2] = (!on || on[2]) ? p.lr_unit_uv[0] : 0;
  f.lr_unit_shift = p.lr_unit_size == 64 ? 0 : p.lr_unit_size == 128 ? 1 : 2; f.lr_uv_shift = 0;
  f.lr_units[0] = d->lr_y.data(); f.lr_units[1] = f.lr_units[2] = d->lr_uv.data();
  // a session with the restoration search: the segment's own records per plane (the session keeps the true size's grid of units)
  for (int q = 0; q < 3; q++)
    if (fr.lr_units[q] && (size_t)fr.lr_units_per_frame[q] == (q ? uc : uy)) f.lr_units[q] = fr.lr_units[q] + (size_t)seg * fr.lr_units_per_frame[q] * 8;
  f.tile_cols_log2 = f.tile_rows_log2 = -1;      // one superblock per tile: the independence the GPU pipeline's prediction assumes
  const size_t nb = fr.blocks_per_frame, o = (size_t)seg * nb;
  if (fr.y_mode) { f.y_mode = fr.y_mode + o; f.uv_mode = fr.uv_mode + o; }       // the symbols are absent when the tiles were coded on the GPU
  if (fr.mv) { f.mv = fr.mv + o * 2; f.skip = fr.skip + o; }
  if (fr.lev_y) { f.lev_y = fr.lev_y + o * 64; f.lev_u = fr.lev_u + o * 16; f.lev_v = fr.lev_v + o * 16; }     // absent when the tiles were coded on the GPU
}

// A key frame of a key_block_size 32 session (av1mi_gop_frame.key_block_size == 32): 32x32 blocks over the complete superblock rows,
// 8x8 blocks in a last partial row — written by the general block writer (av1_blockstream.cpp) from the session's symbols.
static bool Key32TemporalUnit(const av1mi_gop_frame &fr, int seg, const SessionFrameDesc &desc, int width, int height, bool with_sequence_header, int threads,
                              std::vector<uint8_t> *out, std::string *err) {
  if (!fr.y_mode || !fr.lev_y) { if (err) *err = "a key frame in 32x32 blocks needs its symbols (gpu_entropy 0)"; return false; }
  const int hA = (height / 64) * 64, mi_rows = height / 4, mi_cols = width / 4;
  const size_t ny = (size_t)width * height, nc = ny / 4;
  const uint8_t *my = fr.y_mode + (size_t)seg * fr.key_modes_stride, *muv = fr.uv_mode + (size_t)seg * fr.key_modes_stride;
  std::vector<int16_t> lev(ny + 2 * nc);
  memcpy(lev.data(), fr.lev_y + (size_t)seg * ny, ny * 2);
  memcpy(lev.data() + ny, fr.lev_u + (size_t)seg * nc, nc * 2);
  memcpy(lev.data() + ny + nc, fr.lev_v + (size_t)seg * nc, nc * 2);
  std::vector<uint8_t> parts;
  std::vector<av1mi_obu_block> blocks;
  auto block = [&](int r, int c, int bsize, int mode_y, int mode_uv, size_t oy, size_t oc) {
    av1mi_obu_block b;
    memset(&b, 0, sizeof(b));
    b.mi_row = (uint16_t)r; b.mi_col = (uint16_t)c; b.bsize = (uint8_t)bsize; b.y_mode = (uint8_t)mode_y; b.uv_mode = (uint8_t)mode_uv;
    b.tx_type_off = 0;                                   // every luma transform is DCT_DCT: one shared entry
    b.lev_off[0] = (uint32_t)oy; b.lev_off[1] = (uint32_t)(ny + oc); b.lev_off[2] = (uint32_t)(ny + nc + oc);
    blocks.push_back(b);
  };
  const int w32 = width / 32, w8 = width / 8;
  std::vector<size_t> starts;          // per tile (= superblock): its first block, its first partition symbol; the writer's threads start there
  for (int sr = 0; sr * 16 < mi_rows; sr++)
    for (int sc = 0; sc * 16 < mi_cols; sc++) {
      starts.push_back(blocks.size()); starts.push_back(parts.size());
      if (sr * 64 < hA) {                                // PARTITION_SPLIT at 64x64, four 32x32 blocks (two where the frame ends mid-superblock)
        parts.push_back(3);
        for (int k = 0; k < 4; k++) {
          const int r32 = sr * 2 + (k >> 1), c32 = sc * 2 + (k & 1);
          if (c32 >= w32) continue;
          const size_t i = (size_t)r32 * w32 + c32;
          parts.push_back(0);
          block(r32 * 8, c32 * 8, 9 /* BLOCK_32X32 */, my[i], muv[i], i * 1024, i * 256);
        }
      } else {                                           // the last, partial superblock row: split down to 8x8 wherever the frame reaches
        const size_t oyB = (size_t)hA * width, ocB = oyB / 4;
        const uint8_t *myB = my + fr.key_modes_band, *muvB = muv + fr.key_modes_band;
        for (int k = 0; k < 64; k++) {                   // z-order over the superblock's 8x8 blocks; a level's symbol precedes its first block
          int bx = 0, by = 0;
          for (int i = 0; i < 3; i++) { bx |= ((k >> (2 * i)) & 1) << i; by |= ((k >> (2 * i + 1)) & 1) << i; }
          const int r = sr * 16 + by * 2, c = sc * 16 + bx * 2;
          for (int n8 = 8; n8 >= 2; n8 >>= 1)            // 64, 32, 16: PARTITION_SPLIT at every level that starts here, inside the frame
            if (!(bx & (n8 - 1)) && !(by & (n8 - 1)) && r < mi_rows && c < mi_cols) parts.push_back(3);
          if (r >= mi_rows || c >= mi_cols) continue;
          parts.push_back(0);
          const size_t i = (size_t)(r / 2 - hA / 8) * w8 + c / 2;
          block(r, c, 3 /* BLOCK_8X8 */, myB[i], muvB[i], oyB + i * 64, ocB + i * 16);
        }
      }
    }
  av1mi_obu_blocks d;
  memset(&d, 0, sizeof(d));
  d.hdr = desc.f;
  const uint8_t dct = 0;
  d.partition = parts.data(); d.n_partition = parts.size(); d.blocks = blocks.data(); d.n_blocks = blocks.size(); d.tx_type = &dct; d.levels = lev.data();
  starts.push_back(blocks.size()); starts.push_back(parts.size());
  std::string werr;
  if (!av1::blocks_temporal_unit(d, with_sequence_header, out, &werr, threads, reinterpret_cast<const size_t (*)[2]>(starts.data()))) {
    if (err) *err = "bitstream writer: " + werr;
    return false;
  }
  return true;
}

bool SessionTemporalUnit(const av1mi_gop_frame &fr, int seg, int width, int height, int bit_depth, int visible_width, int visible_height,
                         bool with_sequence_header, int threads, std::vector<uint8_t> *out, std::string *err, bool film_grain_present,
                         const av1mi_film_grain *film_grain, const av1mi_colour *colour) {
  SessionFrameDesc desc;
  DescribeSessionFrame(fr, seg, width, height, bit_depth, &desc, visible_width, visible_height);
  desc.f.film_grain_present = film_grain_present; desc.f.film_grain = film_grain; desc.f.colour = colour;
  std::string werr;
  if (fr.tile_size) {      // tiles coded on the GPU: frame header + tile group around them
    const uint32_t *sz = fr.tile_size + (size_t)seg * fr.tiles_per_frame;
    size_t off = 0;
    for (size_t i = 0; i < (size_t)seg * fr.tiles_per_frame; i++) off += fr.tile_size[i];
    std::vector<uint8_t> frame;
    if (!av1::frame_obu_from_tiles(desc.f, fr.tile_payload + off, sz, fr.tiles_per_frame, &frame, &werr)) { if (err) *err = "bitstream assembly: " + werr; return false; }
    *out = av1::temporal_delimiter_obu();
    if (with_sequence_header) av1::append_sequence_obus(av1::sequence_params(desc.f), out);
    out->insert(out->end(), frame.begin(), frame.end());
    return true;
  }
  if (fr.key_block_size == 32) return Key32TemporalUnit(fr, seg, desc, width, height, with_sequence_header, threads, out, err);      // symbols of a key frame in 32x32 blocks
  if (!av1::temporal_unit(desc.f, with_sequence_header, threads, out, &werr)) { if (err) *err = "bitstream writer: " + werr; return false; }
  return true;
}

}  // namespace av1mi_host
