// filmgrain.cpp — grain records -> film grain parameters; the model, the measured gain and the rules are in filmgrain.hpp
#include "filmgrain.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace av1mi_host {

namespace {
int scaling_of(uint64_t sum_sq, uint32_t count, int bit_depth, double gain) {
  const double rms = std::sqrt((double)sum_sq / (double)count) / (double)(1 << (bit_depth - 8));
  return (int)std::min(255.0, std::floor(rms * kResidualToGrain / gain + 0.5));
}
}  // namespace

bool FilmGrainFromRecords(const av1mi_grain_record *records, int bit_depth, int frame_index, av1mi_film_grain *out) {
  if (!records || !out || (bit_depth != 8 && bit_depth != 10)) return false;
  av1mi_film_grain g;
  memset(&g, 0, sizeof(g));
  g.grain_seed = (int32_t)((((uint32_t)frame_index + 1u) * 40503u) & 0xffffu);
  g.grain_scaling_minus_8 = 1;
  g.overlap_flag = 1;
  g.ar_coeffs_cb_plus_128[0] = g.ar_coeffs_cr_plus_128[0] = 128;
  g.cb_mult = g.cr_mult = 192; g.cb_luma_mult = g.cr_luma_mult = 128; g.cb_offset = g.cr_offset = 256;
  // luma: the bins that hold enough samples, the 14 fullest of them
  int bins[AV1MI_GRAIN_BINS], n = 0;
  for (int i = 0; i < AV1MI_GRAIN_BINS; i++) if (records[0].bin[i].count >= kMinCount) bins[n++] = i;
  while (n > 14) {
    int drop = 0;
    for (int k = 1; k < n; k++) if (records[0].bin[bins[k]].count < records[0].bin[bins[drop]].count) drop = k;
    for (int k = drop; k + 1 < n; k++) bins[k] = bins[k + 1];
    n--;
  }
  g.num_y_points = n;
  for (int k = 0; k < n; k++) {
    const av1mi_grain_bin &b = records[0].bin[bins[k]];
    g.point_y_value[k] = (uint8_t)(16 * bins[k] + 8);
    g.point_y_scaling[k] = (uint8_t)scaling_of(b.sum_sq, b.count, bit_depth, kGainLuma);
  }
  if (n) {      // chroma: one constant function per plane
    for (int p = 1; p < 3; p++) {
      uint64_t sum = 0, count = 0;
      for (int i = 0; i < AV1MI_GRAIN_BINS; i++) { sum += records[p].bin[i].sum_sq; count += records[p].bin[i].count; }
      if (count < kMinCount) continue;
      const uint8_t s = (uint8_t)scaling_of(sum, (uint32_t)std::min<uint64_t>(count, 0xffffffffu), bit_depth, kGainChroma);
      uint8_t *value = p == 1 ? g.point_cb_value : g.point_cr_value, *scaling = p == 1 ? g.point_cb_scaling : g.point_cr_scaling;
      (p == 1 ? g.num_cb_points : g.num_cr_points) = 2;
      value[0] = 0; value[1] = 255; scaling[0] = scaling[1] = s;
    }
  }
  g.apply_grain = n > 0;
  *out = g;
  return true;
}

int FilmGrainMidGrey(const av1mi_film_grain &g) {
  if (!g.apply_grain || !g.num_y_points) return 0;
  const int n = g.num_y_points, x = 128;
  if (x <= g.point_y_value[0]) return g.point_y_scaling[0];
  for (int k = 1; k < n; k++)
    if (x <= g.point_y_value[k]) {
      const int x0 = g.point_y_value[k - 1], x1 = g.point_y_value[k], s0 = g.point_y_scaling[k - 1], s1 = g.point_y_scaling[k];
      return s0 + ((s1 - s0) * (x - x0) + (x1 - x0) / 2) / (x1 - x0);
    }
  return g.point_y_scaling[n - 1];
}

}  // namespace av1mi_host
