// chains_rank.hpp — the order in which k_av1_chains walks the CDF slots of a group of 64 tiles: LONGEST EXPECTED CHAIN FIRST, so that
// a group's long chains start together and finish together and the short slots of this group and the next fill the tail.  One table
// per launch flavour (each has its own slot numbering): entry k is the slot the group's k-th workgroup walks.  The order is static:
// the slots sorted by the entries they received over all tiles of the default workload (bench.py: 4K 10-bit, q index 128; the sums
// are in profiles/chains_l2_parent_vs_change.json), ties and slots without entries in slot order.  Any permutation gives the same
// bytes; only the memory traffic depends on it.
#pragma once
#include <stdint.h>
#include "av1_ops32.hpp"

namespace av1mi {
using av1ops::S_INTER_END; using av1ops::S_KEY_END; using av1ops::K_END;

// inter frames
__device__ constexpr uint8_t kChainsRankInter[S_INTER_END] = {
   66,  51,  67,  77,  52,  22,   3, 139, 146, 147, 148, 155,  17,  19,   0,  71, 161, 154,  73,  21,
  198,  45,  46,  78,  47,  18,  72,  20,  44,  40,  34,  41,  42,  30,  27, 159,  29,  28, 152,   1,
   38,  43,   7,  31,  26,  25,  39,  35,  36,  24,  37,  92,  23,   6,   5, 151, 165,  93,  53,  32,
   33,  48, 182, 186, 183, 153, 166, 170, 167, 168,   2,   4,   8,   9,  10,  11,  12, 143, 144, 145,
  149, 185,  68, 184,  16,  74,  54,  94,  79,  49, 163,  50, 162,  55, 113, 106, 112,  99, 107, 100,
   69, 114, 105, 164, 108, 101,  98,  75, 115, 119, 109, 102,  80, 120, 126, 118,  70, 127, 116,  97,
  111, 110, 103, 169, 124, 187, 197,  76, 171, 181, 172, 121, 125, 122, 128, 132, 188, 123, 133, 104,
  129, 173, 130, 189, 131,  13,  14,  15,  56,  57,  58,  59,  60,  61,  62,  63,  64,  65,  81,  82,
   83,  84,  85,  86,  87,  88,  89,  90,  91,  95,  96, 117, 134, 135, 136, 137, 138, 140, 141, 142,
  150, 156, 157, 158, 160, 174, 175, 176, 177, 178, 179, 180, 190, 191, 192, 193, 194, 195, 196
};
// key frames, the tiles of 8x8 blocks
__device__ constexpr uint8_t kChainsRankKey8[S_KEY_END] = {
   67,  66,  77,  78,  68,  55,  54,  73,  22,  71,  50,  44,  53,  20,  74, 113,  30, 112,   0,   3,
   17,  21,  45,  40, 103, 110, 114,  29,  69,  27, 108,  36,  35, 107,  34, 109,  19, 115,  52, 126,
  120,  92, 106,  26,  33,  31,  32, 121,  75,  93,  43,  79, 116, 102,  72, 127, 119, 101, 182, 183,
   70, 180, 184,  49, 175, 196, 122, 100, 178,   7, 117, 139, 181, 177, 111, 173, 194, 179, 105, 143,
  174, 195,  28, 176, 197, 170, 191, 125, 159, 141, 172, 193, 168, 189,   6, 165, 186, 164, 185,  99,
  140, 166, 187, 144, 149, 169, 190, 123,  42, 163, 171, 192, 154,  18,   5, 128, 167, 188, 153,  76,
  161, 160, 142,  48, 162, 151, 133, 150, 148, 124,   4,   8,   9,  10,  11,  12, 146, 152, 147,  51,
  158,  98, 118, 145,  94, 156,  80, 155, 132, 157, 104, 129,  41, 134,  47,  39,  25,  81,  97, 130,
   95,  46, 131, 135,   1,   2,  13,  14,  15,  16,  23,  24,  37,  38,  56,  57,  58,  59,  60,  61,
   62,  63,  64,  65,  82,  83,  84,  85,  86,  87,  88,  89,  90,  91,  96, 136, 137, 138
};
// key frames, the tiles of the 32x32 band
__device__ constexpr uint8_t kChainsRankKey32[K_END] = {
   61,  87,  62,  65,  88, 112,  63,  64,  89,  91,  90, 109, 110, 108,  76, 111, 133, 130, 129, 131,
   50, 107, 132, 126, 128,  71, 105, 119,  98,   9,  66,  39,  45,  25, 125,   0,   1,   4,   6,   8,
   35,  40, 124,  29,  30, 123,  31,  18,  75, 106,   5,   7, 118,  17, 159, 127, 134, 117,  26, 104,
   27,  24, 122,  97,  28, 172, 103,   2,  96, 116, 173,  95, 102, 139, 160, 168, 136, 135, 161, 115,
  144,   3,  74, 121, 177,  94, 101,  70, 175, 176, 169, 170, 179, 174, 165, 178, 154,  49, 114, 138,
  167,  93, 100,  44, 137, 164,  69, 162,  73, 166, 141, 163, 142, 120, 140,  48, 171, 156, 157,  43,
  113, 143, 147, 155, 145, 146,  92,  99,  68, 158, 148,  47,  72,  42,  38,  67,  23,  41,  46,  10,
   11,  12,  13,  14,  15,  16,  19,  20,  21,  22,  32,  33,  34,  36,  37,  51,  52,  53,  54,  55,
   56,  57,  58,  59,  60,  77,  78,  79,  80,  81,  82,  83,  84,  85,  86, 149, 150, 151, 152, 153
};

// a table that is no permutation would skip a slot (its tuples never written) and walk another twice
template <int N> constexpr bool chains_rank_is_permutation(const uint8_t (&r)[N]) {
  bool seen[N] = {};
  for (int i = 0; i < N; i++) {
    if (r[i] >= N || seen[r[i]]) return false;
    seen[r[i]] = true;
  }
  return true;
}
static_assert(chains_rank_is_permutation(kChainsRankInter) && chains_rank_is_permutation(kChainsRankKey8) && chains_rank_is_permutation(kChainsRankKey32),
              "every slot of a flavour exactly once");

}  // namespace av1mi
