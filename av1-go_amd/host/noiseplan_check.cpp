// noiseplan_check.cpp — noiseplan.hpp alone in a program of its own, to be built with the host sanitizers (make noiseplan_check: address +
// undefined behaviour) and run: the plan cases of tests/test_noise_plan.py on hand-made histograms, plus the all-zero and the all-bin-255
// record, the counts a 32-bit sum would lose, and the pair slots.  Exit code 0 = every case gave what the header says.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>
#include "noiseplan.hpp"

using namespace av1mi_host;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "noiseplan_check: line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static av1mi_noise_record rec(std::initializer_list<std::pair<int, uint32_t>> bins, long blocks = -1, long eligible = -1) {
  av1mi_noise_record r;
  memset(&r, 0, sizeof(r));
  uint64_t sum = 0;
  for (const auto &b : bins) { r.hist[b.first] = b.second; sum += b.second; }
  r.eligible = eligible < 0 ? (uint32_t)sum : (uint32_t)eligible;
  r.blocks = blocks < 0 ? r.eligible : (uint32_t)blocks;
  return r;
}

int main() {
  // the quartile index at counted = 1, 4, 5; bin 255 is no part of it
  CHECK(NoisePairLevel(rec({ { 40, 1 } })) == 40);
  CHECK(NoisePairLevel(rec({ { 10, 1 }, { 20, 1 }, { 30, 1 }, { 40, 1 } })) == 10);
  CHECK(NoisePairLevel(rec({ { 10, 1 }, { 20, 1 }, { 30, 1 }, { 40, 1 }, { 50, 1 } })) == 20);
  CHECK(NoisePairLevel(rec({ { 10, 1 }, { 20, 1 }, { 30, 3 }, { 255, 15 } })) == 20);
  CHECK(NoisePairLevel(rec({ { 0, 2 }, { 254, 7 } })) == 254);
  // validity
  CHECK(NoisePairLevel(rec({ { 30, 25 }, { 255, 75 } })) == 30);
  CHECK(NoisePairLevel(rec({ { 30, 24 }, { 255, 76 } })) == -1);
  CHECK(NoisePairLevel(rec({ { 30, 6 } }, 96)) == 30);
  CHECK(NoisePairLevel(rec({ { 30, 6 } }, 112)) == -1);
  CHECK(NoisePairLevel(rec({}, 8)) == -1);
  CHECK(NoisePairLevel(rec({}, 1000)) == -1);                 // the all-zero histogram
  CHECK(NoisePairLevel(rec({ { 255, 1000 } })) == -1);        // the all-bin-255 histogram
  // counts near 2^32: 4 x counted must not wrap
  CHECK(NoisePairLevel(rec({ { 7, 0xFFFFFFFFu } }, 0xFFFFFFFFl, 0xFFFFFFFFl)) == 7);
  CHECK(NoisePairLevel(rec({ { 7, 0x40000000u }, { 9, 0xBFFFFFFFu } }, 0xFFFFFFFFl, 0xFFFFFFFFl)) == 7);
  // the file: no pair, no valid pair, the index at n = 1, 4, 5, 16
  int32_t q[16], s16 = 99;
  CHECK(PlanDenoise(nullptr, 0, nullptr, &s16) == 0 && s16 == -1);
  CHECK(PlanDenoise(nullptr, 1, nullptr, nullptr) == -1 && PlanDenoise(nullptr, -1, nullptr, nullptr) == -1);
  av1mi_noise_record r[16];
  r[0] = rec({ { 255, 50 } }); r[1] = rec({ { 100, 1 }, { 255, 50 } });
  CHECK(PlanDenoise(r, 2, q, &s16) == 0 && s16 == -1 && q[0] == -1 && q[1] == -1);
  const int four[5] = { 90, 50, 70, 60, 80 };
  for (int i = 0; i < 5; i++) r[i] = rec({ { four[i], 10 } });
  CHECK(PlanDenoise(r, 1, q, &s16) == NoiseStrength(NoiseSigma16(90)) && s16 == NoiseSigma16(90) && q[0] == 90);
  CHECK(PlanDenoise(r, 4, nullptr, &s16) >= 0 && s16 == NoiseSigma16(50));
  CHECK(PlanDenoise(r, 5, nullptr, &s16) >= 0 && s16 == NoiseSigma16(60));
  for (int i = 0; i < 16; i++) r[i] = rec({ { 115 - i, 10 } });
  CHECK(PlanDenoise(r, 16, q, &s16) >= 0 && s16 == NoiseSigma16(103) && q[15] == 100);
  // the floor and the cap
  CHECK(NoiseSigma16(8) == 7 && NoiseSigma16(9) == 8 && NoiseSigma16(254) == 225);
  r[0] = rec({ { 8, 10 } }); CHECK(PlanDenoise(r, 1, nullptr, nullptr) == 0);
  r[0] = rec({ { 9, 10 } }); CHECK(PlanDenoise(r, 1, nullptr, nullptr) == 1);
  r[0] = rec({ { 254, 10 } }); CHECK(PlanDenoise(r, 1, nullptr, nullptr) == 16);
  CHECK(NoiseStrength(7) == 0 && NoiseStrength(8) == 1 && NoiseStrength(64) == 6 && NoiseStrength(160) == 15 && NoiseStrength(170) == 16 && NoiseStrength(4000) == 16);
  // the pair slots
  CHECK(NoiseSamplePairs(-1) == 0 && NoiseSamplePairs(0) == 0 && NoiseSamplePairs(1) == 0 && NoiseSamplePairs(3) == 1 && NoiseSamplePairs(1000) == 16);
  CHECK(NoisePairSlot(0, 3) == 0 && NoisePairSlot(1, 5) == 1 && NoisePairSlot(15, 1000) == 499 && NoisePairSlot(15, 32) == 15 && NoisePairSlot(15, 2000000000l) == 999999999l);
  if (failures) return 1;
  printf("noiseplan_check: all cases as the header says\n");
  return 0;
}
