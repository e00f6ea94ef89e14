// peakplan_check.cpp — peakplan.hpp alone in a program of its own, to be built with the host sanitizers (make peakplan_check: address +
// undefined behaviour) and run: the rule's edge cases on hand-made histograms — an all-black frame, one bright pixel under and over skip,
// code 1023, counts near 2^32, frames 0 — and the sample's slots.  Exit code 0 = every case gave what the header says.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>
#include "peakplan.hpp"

using namespace av1mi_host;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "peakplan_check: line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static av1mi_peak_record rec(std::initializer_list<std::pair<int, uint32_t>> bins) {
  av1mi_peak_record r;
  memset(&r, 0, sizeof(r));
  uint64_t sum = 0;
  for (const auto &b : bins) { r.hist[b.first] = b.second; sum += b.second; }
  r.pixels = (uint32_t)sum;
  return r;
}

int main() {
  // lin[]: the PQ EOTF of code / 1023 in 2^-8 cd/m2 (include/av1mi.h "tone mapping", step 3)
  static uint32_t lin[1024];
  const double m1 = 2610.0 / 16384, m2 = 2523.0 / 4096 * 128, c1 = 3424.0 / 4096, c2 = 2413.0 / 4096 * 32, c3 = 2392.0 / 4096 * 32;
  for (int c = 0; c < 1024; c++) {
    const double p = pow(c / 1023.0, 1.0 / m2);
    lin[c] = (uint32_t)floor(10000.0 * pow(std::max(p - c1, 0.0) / (c2 - c3 * p), 1.0 / m1) * 256.0 + 0.5);
  }
  CHECK(lin[0] == 0 && lin[1023] == 2560000u);
  int32_t code[4] = { -7, -7, -7, -7 };
  // an all-black frame: code 0, the floor
  av1mi_peak_record r[4];
  r[0] = rec({ { 0, 64 * 64 } });
  CHECK(PeakFrameCode(r[0]) == 0 && PlanPeak(r, 1, lin, code) == 400 && code[0] == 0);
  // a frame under 16384 pixels skips nothing: one bright pixel is the code
  r[0] = rec({ { 0, 64 * 64 - 1 }, { 900, 1 } });
  CHECK(PeakFrameCode(r[0]) == 900 && PlanPeak(r, 1, lin, nullptr) == PeakOfCode(900, lin));
  // 32768 pixels: skip = 2.  Two bright pixels are let go, the third is not
  r[0] = rec({ { 100, 32768 - 2 }, { 900, 2 } });
  CHECK(PeakFrameCode(r[0]) == 100);
  r[0] = rec({ { 100, 32768 - 3 }, { 900, 3 } });
  CHECK(PeakFrameCode(r[0]) == 900);
  r[0] = rec({ { 100, 32768 - 3 }, { 800, 1 }, { 900, 2 } });      // (the tail is cumulative: the third pixel from the top decides)
  CHECK(PeakFrameCode(r[0]) == 800);
  // 3840 x 2160: skip = 506
  r[0] = rec({ { 300, 3840 * 2160 - 506 }, { 1000, 506 } });
  CHECK((r[0].pixels >> 14) == 506 && PeakFrameCode(r[0]) == 300);
  r[0] = rec({ { 300, 3840 * 2160 - 507 }, { 1000, 507 } });
  CHECK(PeakFrameCode(r[0]) == 1000);
  // code 1023: the cap; and the round-up of lin
  r[0] = rec({ { 1023, 4096 } });
  CHECK(PeakFrameCode(r[0]) == 1023 && PlanPeak(r, 1, lin, code) == 10000 && code[0] == 1023);
  CHECK(PeakOfCode(1023, lin) == 10000 && PeakOfCode(0, lin) == 400);
  { uint32_t one[1024] = { 0 }; one[5] = 400 * 256 + 1; one[6] = 400 * 256; one[7] = 0xFFFFFFFFu; CHECK(PeakOfCode(5, one) == 401 && PeakOfCode(6, one) == 400 && PeakOfCode(7, one) == 10000); }
  // counts near 2^32: the tail must not wrap
  r[0] = rec({});
  r[0].hist[1] = 0xFFFFFFFFu; r[0].hist[1000] = 0x3FFFFu; r[0].hist[1001] = 1; r[0].pixels = 0xFFFFFFFFu;      // skip = 0x3FFFF
  CHECK(PeakFrameCode(r[0]) == 1000);
  // the file: the maximum over the frames, whatever their order
  r[0] = rec({ { 200, 4096 } }); r[1] = rec({ { 700, 4096 } }); r[2] = rec({ { 500, 4096 } }); r[3] = rec({ { 0, 4096 } });
  CHECK(PlanPeak(r, 4, lin, code) == PeakOfCode(700, lin) && code[0] == 200 && code[1] == 700 && code[2] == 500 && code[3] == 0);
  CHECK(PeakOfCode(700, lin) > 400 && PeakOfCode(700, lin) < 10000);
  // refusals: frames 0 and below, no records, no table, a record without pixels
  CHECK(PlanPeak(r, 0, lin, nullptr) == -1 && PlanPeak(r, -1, lin, nullptr) == -1 && PlanPeak(nullptr, 1, lin, nullptr) == -1 && PlanPeak(r, 1, nullptr, nullptr) == -1);
  r[1] = rec({});
  CHECK(PlanPeak(r, 2, lin, nullptr) == -1);
  // the sample's slots: the crop sampler's
  CHECK(PeakSampleFrames(-1) == 0 && PeakSampleFrames(0) == 0 && PeakSampleFrames(8) == 8 && PeakSampleFrames(1000) == 32);
  CHECK(PeakSampleSlot(0, 8) == 0 && PeakSampleSlot(7, 8) == 7 && PeakSampleSlot(31, 1000) == 968 && PeakSampleSlot(31, 2000000000l) == 1937500000l);
  if (failures) return 1;
  printf("peakplan_check: all cases as the header says\n");
  return 0;
}
