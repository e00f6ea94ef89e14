// sceneplan.hpp — where the GOPs of a group start when the scene analysis (include/av1mi.h "scene analysis") has found cuts: the cut
// rule on a frame's record, and the planner that moves GOP boundaries onto cuts.  Pure functions, exported by libav1mi_host.so; the
// reference has no counterpart (its encoder child decides, internal/ffmpeg/transcode.go:120).
#pragma once
#include <stdint.h>
#include "../../include/av1mi.h"

// -av1mi_scenecut without a number's worth of opinion: the middle of the range of sensitivities that find every cut and no false one on
// the two clips of tests/scene_clips.py (DEFAULT_CLIPS): 1 .. 30, DESIGN 5.00-sexies
#define AV1MI_SCENECUT_DEFAULT 15

extern "C" {
// 1 when the frame of `rec` is a cut at sensitivity scenecut (1 .. 99): 100 inter_sad >= (100 - scenecut) intra_sad and intra_sad > 0
int av1mi_scene_is_cut(const av1mi_scene_record *rec, int scenecut);
// The window's n frames (1 <= n <= S G) are split into K = ceil(n / G) GOPs; returns K, or -1 for arguments outside these rules.
// cut[f] != 0 marks frame f of the window as a cut.  start[0] = 0.  For k = 1 .. K - 1 in order the boundary is the cut nearest to k G
// among the cuts f with start[k - 1] + min_len <= f <= min(n - 1, start[k - 1] + G + G / 2) and |f - k G| <= G / 2, ties going to the
// earlier cut; without such a cut it is k G.  len[k] = start[k + 1] - start[k], the last GOP ends with the window.  So every frame
// belongs to exactly one GOP, lengths lie in [min_len, G + G / 2] except a last GOP cut short by the end of the input, and without cuts
// the plan is the fixed layout start[k] = k G.  (The bound start[k - 1] + G + G / 2 is what keeps a GOP that started early on one cut
// from ending late on the next.)  min_len: 1 .. G - G / 2, or <= 0 for the default max(1, G / 4).  start and len hold S entries;
// entries from K on are set to (n, 0).
int av1mi_plan_gops(int n, int G, int S, int min_len, const uint8_t *cut, int32_t *start, int32_t *len);
}
