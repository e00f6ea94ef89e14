// av1_ops_cdfs.hpp — the default CDF image of a tile in the slot layout of av1_ops.hpp (8x8 blocks) or av1_ops32.hpp (the 32x32
// band), built from the specification's default tables (host/av1_default_cdfs.inc).  Host code only (the GPU coder uploads the image
// once per context).
#pragma once
#include <vector>
#include "av1_ops.hpp"
#include "av1_ops32.hpp"
#include "../host/av1_default_cdfs.inc"

namespace av1ops {

// a slot image in the layout of table t: cdfs[t.off[slot] ..]: nsym - 1 inverse values, then the counter (0), then padding;
// put(slot, spec CDF, nsym) fills one slot
struct SlotImage {
  const SlotTable &t;
  std::vector<uint16_t> img;
  explicit SlotImage(const SlotTable &tab) : t(tab), img((size_t)tab.words, 0) {}
  void operator()(int slot, const uint16_t *spec, int nsym) {
    for (int i = 0; i < nsym - 1; i++) img[t.off[slot] + i] = (uint16_t)(32768 - spec[i]);
  }
};

// the coefficient slots of band B: luma in transform-size context txs_y (plane type 0), chroma in txs_c (plane type 1); eob_y /
// eob_c: the eob_pt CDFs of the two transform sizes
template <const BandSlots &B>
inline void put_coeff_cdfs(SlotImage &put, int qcat, int txs_y, int txs_c, const uint16_t *eob_y, const uint16_t *eob_c) {
  put(B.txb_skip_y, Default_Txb_Skip_Cdf[qcat][txs_y][0], 2);
  for (int i = 0; i < 3; i++) put(B.txb_skip_c + i, Default_Txb_Skip_Cdf[qcat][txs_c][7 + i], 2);
  put(B.eob_y, eob_y, B.eob_y_n);
  put(B.eob_c, eob_c, B.eob_c_n);
  for (int i = 0; i < B.eob_y_n - 2; i++) put(B.eobx_y + i, Default_Eob_Extra_Cdf[qcat][txs_y][0][i], 2);
  for (int i = 0; i < B.eob_c_n - 2; i++) put(B.eobx_c + i, Default_Eob_Extra_Cdf[qcat][txs_c][1][i], 2);
  for (int i = 0; i < 3; i++) { put(B.dc_sign_y + i, Default_Dc_Sign_Cdf[qcat][0][i], 2); put(B.dc_sign_c + i, Default_Dc_Sign_Cdf[qcat][1][i], 2); }
  for (int i = 0; i < 4; i++) { put(B.base_eob_y + i, Default_Coeff_Base_Eob_Cdf[qcat][txs_y][0][i], 3); put(B.base_eob_c + i, Default_Coeff_Base_Eob_Cdf[qcat][txs_c][1][i], 3); }
  for (int i = 0; i < 26; i++) { put(B.base_y + i, Default_Coeff_Base_Cdf[qcat][txs_y][0][i], 4); put(B.base_c + i, Default_Coeff_Base_Cdf[qcat][txs_c][1][i], 4); }
  for (int i = 0; i < 21; i++) { put(B.br_y + i, Default_Coeff_Br_Cdf[qcat][txs_y][0][i], 4); put(B.br_c + i, Default_Coeff_Br_Cdf[qcat][txs_c][1][i], 4); }
}
// the key-frame mode slots of band B
template <const BandSlots &B> inline void put_kf_mode_cdfs(SlotImage &put) {
  for (int a = 0; a < 5; a++) for (int l = 0; l < 5; l++) put(B.kf_y_mode + a * 5 + l, Default_Intra_Frame_Y_Mode_Cdf[a][l], 13);
  for (int m = 0; m < 13; m++) put(B.uv_mode + m, Default_Uv_Mode_Cfl_Allowed_Cdf[m], 14);
  for (int i = 0; i < 8; i++) put(B.angle + i, Default_Angle_Delta_Cdf[i], 7);
}

// the tiles of 8x8 blocks: luma 8x8 (transform-size context 1), chroma 4x4 (context 0)
inline std::vector<uint16_t> default_slot_image(bool key, int qcat, SlotTable *t) {
  build_slot_table(key, t);
  SlotImage put(*t);
  for (int i = 0; i < 3; i++) put(S_SKIP + i, Default_Skip_Cdf[i], 2);
  put(S_PART8, Default_Partition_W8_Cdf[0], 4);
  for (int i = 0; i < 4; i++) { put(S_PART16 + i, Default_Partition_W16_Cdf[i], 10); put(S_PART32 + i, Default_Partition_W32_Cdf[i], 10); put(S_PART64 + i, Default_Partition_W64_Cdf[i], 10); }
  put(S_USE_WIENER, Default_Use_Wiener_Cdf[0], 2);
  put_coeff_cdfs<kSlots8>(put, qcat, 1, 0, Default_Eob_Pt_64_Cdf[qcat][0][0], Default_Eob_Pt_16_Cdf[qcat][1][0]);
  if (key) {
    put_kf_mode_cdfs<kSlots8>(put);
    for (int m = 0; m < 13; m++) put(S_INTRA_TX + m, Default_Intra_Tx_Type_Set1_Cdf[1][m], 7);
  } else {
    for (int i = 0; i < 4; i++) put(S_IS_INTER + i, Default_Is_Inter_Cdf[i], 2);
    static const int kBit[3] = { 0, 2, 3 };      // single_ref_p1, p3, p4
    for (int c = 0; c < 2; c++) for (int k = 0; k < 3; k++) put(S_SINGLE_REF + c * 3 + k, Default_Single_Ref_Cdf[1 + c][kBit[k]], 2);
    for (int i = 0; i < 6; i++) { put(S_NEW_MV + i, Default_New_Mv_Cdf[i], 2); put(S_REF_MV + i, Default_Ref_Mv_Cdf[i], 2); }
    put(S_ZERO_MV, Default_Zero_Mv_Cdf[0], 2);
    for (int i = 0; i < 3; i++) put(S_DRL + i, Default_Drl_Mode_Cdf[i], 2);
    put(S_MV_JOINT, Default_Mv_Joint_Cdf[0], 4);
    for (int c = 0; c < 2; c++) {
      const int b = S_MV_COMP + c * 16;
      put(b + MVC_CLASS, Default_Mv_Class_Cdf[0], 11);
      put(b + MVC_CLASS0, Default_Mv_Class0_Bit_Cdf[0], 2);
      put(b + MVC_CLASS0_FR, Default_Mv_Class0_Fr_Cdf[0], 4);
      put(b + MVC_CLASS0_FR + 1, Default_Mv_Class0_Fr_Cdf[1], 4);
      put(b + MVC_SIGN, Default_Mv_Sign_Cdf[0], 2);
      for (int i = 0; i < 10; i++) put(b + MVC_BITS + i, Default_Mv_Bit_Cdf[i], 2);
      put(b + MVC_FR, Default_Mv_Fr_Cdf[0], 4);
    }
    put(S_INTER_TX, Default_Inter_Tx_Type_Set1_Cdf[1], 16);
  }
  return put.img;
}

// the tiles of a key frame's 32x32 band (av1_ops32.hpp): luma 32x32 (transform-size context 3), chroma 16x16 (context 2)
inline std::vector<uint16_t> default_slot_image_k32(int qcat, SlotTable *t) {
  build_slot_table(K_END, slot_nsym_k32, t);
  SlotImage put(*t);
  put(K_SKIP, Default_Skip_Cdf[0], 2);
  put(K_PART32, Default_Partition_W32_Cdf[0], 10); put(K_PART64, Default_Partition_W64_Cdf[0], 10);
  put(K_USE_WIENER, Default_Use_Wiener_Cdf[0], 2);
  put_coeff_cdfs<kSlots32>(put, qcat, 3, 2, Default_Eob_Pt_1024_Cdf[qcat][0][0], Default_Eob_Pt_256_Cdf[qcat][1][0]);
  put_kf_mode_cdfs<kSlots32>(put);
  return put.img;
}

}  // namespace av1ops
