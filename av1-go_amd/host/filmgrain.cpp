// filmgrain.cpp — grain records -> film grain parameters; the model, the measured gain and the rules are in filmgrain.hpp
#include "filmgrain.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace av1mi_host {

namespace {
int scaling_of(uint64_t sum_sq, uint32_t count, int bit_depth, double gain) {
  const double rms = std::sqrt((double)sum_sq / (double)count) / (double)(1 << (bit_depth - 8));
  return (int)std::min(255.0, std::floor(rms * kResidualToGrain / gain + 0.5));
}
bool white(const av1mi_grain_record *records, int bit_depth, int frame_index, const double amp[3], av1mi_film_grain *out);
}  // namespace

bool FilmGrainFromRecords(const av1mi_grain_record *records, int bit_depth, int frame_index, av1mi_film_grain *out) {
  const double one[3] = { 1.0, 1.0, 1.0 };
  return white(records, bit_depth, frame_index, one, out);
}

namespace {
// the parameters with white grain; amp[plane]: what the template's variance is raised by on its way (sqrt(G); 1 = white), which the
// scaling values are divided by
bool white(const av1mi_grain_record *records, int bit_depth, int frame_index, const double amp[3], av1mi_film_grain *out) {
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
    g.point_y_scaling[k] = (uint8_t)scaling_of(b.sum_sq, b.count, bit_depth, kGainLuma * amp[0]);
  }
  if (n) {      // chroma: one constant function per plane
    for (int p = 1; p < 3; p++) {
      uint64_t sum = 0, count = 0;
      for (int i = 0; i < AV1MI_GRAIN_BINS; i++) { sum += records[p].bin[i].sum_sq; count += records[p].bin[i].count; }
      if (count < kMinCount) continue;
      const uint8_t s = (uint8_t)scaling_of(sum, (uint32_t)std::min<uint64_t>(count, 0xffffffffu), bit_depth, kGainChroma * amp[p]);
      uint8_t *value = p == 1 ? g.point_cb_value : g.point_cr_value, *scaling = p == 1 ? g.point_cb_scaling : g.point_cr_scaling;
      (p == 1 ? g.num_cb_points : g.num_cr_points) = 2;
      value[0] = 0; value[1] = 255; scaling[0] = scaling[1] = s;
    }
  }
  g.apply_grain = n > 0;
  *out = g;
  return true;
}

// the causal neighbours of a lag in the spec's order
int neighbours(int lag, int dx[24], int dy[24]) {
  int n = 0;
  for (int y = -lag; y <= 0; y++)
    for (int x = -lag; x <= lag && !(y == 0 && x == 0); x++) { dx[n] = x; dy[n] = y; n++; }
  return n;
}
}  // namespace

bool ArSolve(const av1mi_grain_cov_record &cov, int lag, double *a) {
  if (lag < 1 || lag > 3 || cov.sum[0][6] <= 0) return false;
  const double c0 = (double)cov.sum[0][6];
  auto rho = [&](int x, int y) { if (y < 0) { x = -x; y = -y; } return (double)cov.sum[y][x + 6] / c0; };
  int dx[24], dy[24];
  const int n = neighbours(lag, dx, dy);
  double m[24][25];
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) m[i][j] = rho(dx[i] - dx[j], dy[i] - dy[j]) + (i == j ? kArRidge : 0.0);
    m[i][n] = rho(dx[i], dy[i]);
  }
  for (int k = 0; k < n; k++) {
    int piv = k;
    for (int i = k + 1; i < n; i++) if (std::fabs(m[i][k]) > std::fabs(m[piv][k])) piv = i;
    if (!(std::fabs(m[piv][k]) > 1e-12)) return false;
    if (piv != k) for (int j = k; j <= n; j++) std::swap(m[k][j], m[piv][j]);
    for (int i = k + 1; i < n; i++) {
      const double f = m[i][k] / m[k][k];
      for (int j = k; j <= n; j++) m[i][j] -= f * m[k][j];
    }
  }
  for (int i = n - 1; i >= 0; i--) {
    double v = m[i][n];
    for (int j = i + 1; j < n; j++) v -= m[i][j] * a[j];
    a[i] = v / m[i][i];
    if (!std::isfinite(a[i])) return false;
  }
  return true;
}

double ArGain(const int *c, int lag, int shift) {
  if (lag == 0) return 1.0;
  constexpr int K = 32, W = 2 * K + 1, M = 3;      // rows 0 .. K, columns -K .. K, a margin of zeros for the neighbours beyond
  static thread_local double h[K + 1 + M][W + 2 * M];
  int dx[24], dy[24];
  const int n = neighbours(lag, dx, dy);
  const double unit = 1.0 / (double)(1 << shift);
  for (auto &row : h) for (double &v : row) v = 0.0;
  double total = 0.0, inner = 0.0;
  for (int y = 0; y <= K; y++)
    for (int x = -K; x <= K; x++) {
      double v = x == 0 && y == 0 ? 1.0 : 0.0;
      for (int i = 0; i < n; i++) v += c[i] * unit * h[y + dy[i] + M][x + dx[i] + K + M];
      h[y + M][x + K + M] = v;
      total += v * v;
      if (y <= K / 2 && x >= -K / 2 && x <= K / 2) inner += v * v;
      if (!std::isfinite(total) || total > 1e12) return -1.0;
    }
  return total - inner > 1e-3 * total ? -1.0 : total;
}

namespace {
// the white templates of one size, made once (their values do not depend on the filter): `runs` templates of H x W, and the sum of squares
// of the part blocks are cut from
struct WhiteTemplates {
  int H, W, from, runs;
  std::vector<short> v;
  double before = 0.0;
  WhiteTemplates(bool chroma) : H(chroma ? 38 : 73), W(chroma ? 44 : 82), from(chroma ? 6 : 9), runs(chroma ? 3 * kTemplateRuns : kTemplateRuns) {
    uint64_t state = chroma ? 0xD1B54A32D192ED03ull : 0x9E3779B97F4A7C15ull;
    auto uniform = [&]() {      // xorshift64*, the top 53 bits, in (0, 1]
      state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
      return ((double)((state * 0x2545F4914F6CDD1Dull) >> 11) + 1.0) / 9007199254740992.0;
    };
    v.resize((size_t)runs * H * W);
    for (size_t k = 0; k < v.size(); k += 2) {      // Box-Muller, two values a time (H x W is even)
      const double m = std::sqrt(-2.0 * std::log(uniform())) * kTemplateSigma, a = 2.0 * M_PI * uniform();
      v[k] = (short)std::floor(m * std::cos(a) + 0.5); v[k + 1] = (short)std::floor(m * std::sin(a) + 0.5);
    }
    for (int r = 0; r < runs; r++)
      for (int y = from; y < H; y++)
        for (int x = from; x < W - 3; x++) { const double s = v[((size_t)r * H + y) * W + x]; before += s * s; }
  }
};
}  // namespace

double ArTemplateGain(const int *c, int lag, int shift, bool chroma) {
  if (lag == 0) return 1.0;
  static const WhiteTemplates luma_templates(false), chroma_templates(true);      // (initialised once, by whichever thread comes first)
  const WhiteTemplates &T = chroma ? chroma_templates : luma_templates;
  const int H = T.H, W = T.W;
  int dx[24], dy[24], off[24];
  const int n = neighbours(lag, dx, dy);
  for (int i = 0; i < n; i++) off[i] = dy[i] * W + dx[i];
  std::vector<int> t((size_t)H * W);
  double after = 0.0;
  for (int r = 0; r < T.runs; r++) {
    for (int k = 0; k < H * W; k++) t[(size_t)k] = T.v[(size_t)r * H * W + k];
    for (int y = 3; y < H; y++)
      for (int x = 3; x < W - 3; x++) {      // (x + dx in [0, W), y + dy >= 0: inside the template)
        int *at = &t[(size_t)y * W + x], sum = 0;
        for (int i = 0; i < n; i++) sum += c[i] * at[off[i]];
        *at = std::min(std::max(*at + ((sum + (1 << (shift - 1))) >> shift), -128), 127);
      }
    for (int y = T.from; y < H; y++) for (int x = T.from; x < W - 3; x++) { const double s = t[(size_t)y * W + x]; after += s * s; }
  }
  return after / T.before;
}

bool FilmGrainFromRecordsAr(const av1mi_grain_record *records, const av1mi_grain_cov_record *cov, int bit_depth, int frame_index, int lag, av1mi_film_grain *out) {
  if (!records || !cov || !out || (bit_depth != 8 && bit_depth != 10) || lag < 0 || lag > 3) return false;
  int l[3], q[3][24], shift = 9;
  double a[3][24], amp[3] = { 1.0, 1.0, 1.0 };
  for (int p = 0; p < 3; p++) {
    uint64_t count = 0;
    for (int i = 0; i < AV1MI_GRAIN_BINS; i++) count += records[p].bin[i].count;
    l[p] = count >= kMinCount && cov[p].sum[0][6] > 0 ? lag : 0;
  }
  // every plane at its lag; a plane that fails a rule steps down and everything is derived again (the shift is common to the three)
  for (bool again = true; again;) {
    again = false;
    for (int p = 0; p < 3 && !again; p++) {
      if (!l[p]) continue;
      if (!ArSolve(cov[p], l[p], a[p])) { l[p]--; again = true; break; }
      const int n = 2 * l[p] * (l[p] + 1);
      for (int i = 0; i < n; i++) {
        const double c = std::floor(a[p][i] * 64.0 + 0.5);
        if (c < -128.0 || c > 127.0) { l[p]--; again = true; break; }      // does not fit at the smallest shift
      }
    }
    if (again) continue;
    for (shift = 9; shift > 6; shift--) {
      bool fits = true;
      for (int p = 0; p < 3; p++)
        for (int i = 0; i < 2 * l[p] * (l[p] + 1); i++) {
          const double c = std::floor(a[p][i] * (double)(1 << shift) + 0.5);
          if (c < -128.0 || c > 127.0) fits = false;
        }
      if (fits) break;
    }
    for (int p = 0; p < 3 && !again; p++) {
      amp[p] = 1.0;
      if (!l[p]) continue;
      const int n = 2 * l[p] * (l[p] + 1);
      for (int i = 0; i < n; i++) q[p][i] = (int)std::floor(a[p][i] * (double)(1 << shift) + 0.5);
      const double G = ArGain(q[p], l[p], shift);
      if (!(G > 0.0) || G > kArMaxGain) { l[p]--; again = true; break; }
      amp[p] = std::sqrt(ArTemplateGain(q[p], l[p], shift, p > 0));      // what the decoder's template comes out with, clip and all
    }
  }
  if (!white(records, bit_depth, frame_index, amp, out)) return false;
  const int coded = out->apply_grain ? std::max(l[0], std::max(out->num_cb_points ? l[1] : 0, out->num_cr_points ? l[2] : 0)) : 0;
  if (!coded) {      // no plane is coloured (or no grain at all): the white parameters, scaling values undivided
    const double one[3] = { 1.0, 1.0, 1.0 };
    return white(records, bit_depth, frame_index, one, out);
  }
  // the divided values are small numbers, a step of which is a larger share: one more bit of scaling where every value still fits
  {
    const double half[3] = { amp[0] / 2.0, amp[1] / 2.0, amp[2] / 2.0 };
    av1mi_film_grain fine;
    bool fits = white(records, bit_depth, frame_index, half, &fine);
    for (int k = 0; k < fine.num_y_points; k++) fits = fits && fine.point_y_scaling[k] < 255;
    fits = fits && (!fine.num_cb_points || fine.point_cb_scaling[0] < 255) && (!fine.num_cr_points || fine.point_cr_scaling[0] < 255);
    if (fits) { *out = fine; out->grain_scaling_minus_8 = 2; }
  }
  out->ar_coeff_lag = coded;
  out->ar_coeff_shift_minus_6 = shift - 6;
  int cdx[24], cdy[24];
  const int cn = neighbours(coded, cdx, cdy);
  for (int p = 0; p < 3; p++) {
    uint8_t *dst = p == 0 ? out->ar_coeffs_y_plus_128 : p == 1 ? out->ar_coeffs_cb_plus_128 : out->ar_coeffs_cr_plus_128;
    int pdx[24], pdy[24];
    const int pn = l[p] ? neighbours(l[p], pdx, pdy) : 0;
    for (int i = 0; i < cn; i++) {      // the plane's own neighbourhood inside the coded one, zeros around it
      int v = 0;
      for (int j = 0; j < pn; j++) if (pdx[j] == cdx[i] && pdy[j] == cdy[i]) v = q[p][j];
      dst[i] = (uint8_t)(v + 128);
    }
    if (p) dst[cn] = 128;      // the luma grain's share: none
  }
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
