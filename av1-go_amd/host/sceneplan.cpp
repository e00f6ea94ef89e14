// sceneplan.cpp — see sceneplan.hpp.
#include "sceneplan.hpp"
#include <cstdlib>

extern "C" {

int av1mi_scene_is_cut(const av1mi_scene_record *rec, int scenecut) {
  if (!rec || scenecut < 1 || scenecut > 99 || rec->intra_sad == 0) return 0;
  // both sums stay below 2^50 at any frame size the session takes: the products fit 64 bits
  return 100ull * rec->inter_sad >= (uint64_t)(100 - scenecut) * rec->intra_sad ? 1 : 0;
}

int av1mi_plan_gops(int n, int G, int S, int min_len, const uint8_t *cut, int32_t *start, int32_t *len) {
  if (G < 1 || S < 1 || n < 1 || (long long)n > (long long)S * G || !cut || !start || !len) return -1;
  const int reach = G / 2;
  if (min_len <= 0) min_len = G / 4 > 1 ? G / 4 : 1;
  if (min_len > G - reach) return -1;
  const int K = (n + G - 1) / G;
  start[0] = 0;
  for (int k = 1; k < K; k++) {
    const int at = k * G, lo = start[k - 1] + min_len, hi = start[k - 1] + G + reach;
    int best = -1;
    for (int f = at - reach; f <= at + reach && f <= n - 1 && f <= hi; f++)
      if (f >= lo && cut[f] && (best < 0 || abs(f - at) < abs(best - at))) best = f;      // (strictly nearer: ties stay with the earlier cut)
    start[k] = best < 0 ? at : best;
  }
  for (int k = 0; k < K; k++) len[k] = (k + 1 < K ? start[k + 1] : n) - start[k];
  for (int k = K; k < S; k++) { start[k] = n; len[k] = 0; }
  return K;
}

}  // extern "C"
