// av1_entropy_kernels.hip — K9 for the REAL syntax: the AV1 tile entropy coder on the GPU.  SURVEY.md §8a row H1 keeps entropy
// coding on the host cores and §8e names it the scaling risk; measured (profiles/): the host writer on the box's 16
// cores sustains ~100 4K frames/s while the block pipeline produces 4 900 — so the same syntax also runs here, and what crosses
// PCIe is the coded tile payloads (0.7 MB per 4K frame) instead of 25 MB of int16 levels.
//
// The syntax is av1_ops.hpp + av1_ops32.hpp (key frames in 32x32 blocks; shared source with the host's CPU twin, byte-identical
// to the dav1d-verified writer), in three stages:
//   k_av1_info     inter frames, thread per block: the mode that codes the block's vector
//   k_av1_tokens   workgroup per tile, thread per block in z-order (av1_ops8.hpp): the block's syntax elements, counted, placed,
//                  written — literals into the tile's list, adaptive symbols as entries grouped by CDF slot
//   k_av1_chains   a slot's CDF evolves with that slot's symbols only: one lane per (tile, slot) walks the slot's entries with the
//                  CDF in registers and writes, at each element's place in the list, the tuple (icdf[s - 1], icdf[s], n - s) the
//                  range coder needs.  The serial dependency of a tile drops from all its symbols (4000-8000) to its longest
//                  chain (700-1300), and the chains of ALL tiles run side by side
//   k_av1_code     ONE LANE PER TILE: the serial range coder over the finished list.  No CDFs: its state is five registers.
//                  Each workgroup also writes the sum of its 64 tiles' payload sizes.
//   k_av1_gather   tile payloads -> one contiguous buffer in tile order (the host adds the frame header and the tile-size fields:
//                  they depend on the largest tile, host/av1_bitstream.cpp frame_obu_from_tiles).  A tile's workgroup finds its
//                  offset from the group sums; the last tile's writes the total and the status, and the caller's pinned mirrors
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "av1_ops_cdfs.hpp"
#include "av1_ops8.hpp"
#include "av1mi_internal.hpp"
#include "chains_rank.hpp"

namespace av1mi {
using namespace av1ops;

struct Av1EntLaunch {
  FrameView fv;                 // pointers of frame 0; frame f adds f * per-frame strides
  int nframes, sbr_n, sbc_n;
  BlockInfo *info;              // nframes * blocks
  // The lists (literal ops, tuples) and the entries of the adaptive symbols, grouped by slot, are two POOLS of the size every tile at its
  // capacity would need, handed out DENSELY: a tile's wave reserves whole 128-byte lines for the words and entries it has counted
  // (PoolAreas), so what a batch touches lies at the pools' fronts, in the order the tiles arrive there, and no two tiles share a line
  // (the tiles of different groups are completed on different XCDs, whose L2s know nothing of one another).  Every tile's range is at
  // most its capacity rounded up to lines, which ops_cap and grouped_cap cover: a pool cannot run out before a tile does.
  op_t *ops; uint32_t ops_cap;
  uint32_t *grouped; uint32_t grouped_cap;
  uint32_t *list_off, *grouped_off;          // per tile: where its list / its entries start, in lines of kPoolLine words
  uint32_t *cursors;                         // [0] the lists' next free line, [1] the entries'; from [kTicketRowFirst] the chains' tickets: all zero at the start of a batch
  uint16_t *slot_total, *slot_base;          // per tile x S_MAX: entries of the slot, position of its first entry
  uint16_t *rec;                             // per tile of 8x8 blocks x 64 blocks x kBlockRecords: the tokenizer's records
  uint32_t *nops;               // per tile
  uint8_t *slots; uint32_t slot_cap;   // per tile payload slot
  uint32_t *tile_size;          // per tile: payload bytes (0 = overflow)
  uint64_t *group_sum;          // per workgroup of k_av1_code (64 tiles): the sum of its tiles' sizes
  uint64_t *total;              // the job's d_total: [0] all tiles' bytes; the status is the word behind it
  Av1EntMirrors mir;            // optional pinned mirrors of sizes, total + status and lr_on_frame (av1mi_internal.hpp)
  uint32_t *status;             // bit 0: a tile's op list overflowed, bit 1: a payload slot overflowed, bit 2: out_cap too small
  uint8_t *out; uint64_t out_cap;
  const uint16_t *cdf_image; int cdf_words;   // default slot image of this frame type / q category
  SlotTable tab;
  const uint16_t *cdf_image32; SlotTable tab32;   // the same for the tiles of a key frame's 32x32 band
  const uint8_t *lr_on_frame;   // optional: [frame * 3 + plane], 0 = restoration of the plane is off in that frame
  size_t lr_units_stride[3];    // fv.lr_units[p] != null: units between the frames of plane p's records
  size_t cdef_idx_stride;       // fv.cdef_idx != null: bytes between the frames' CDEF indices
  // key frames in 32x32 blocks (av1_ops32.hpp): the first sb_rows32 superblock rows of every frame are tiles of that kind, with their
  // own slot table and default CDFs; `band` selects which tiles a chains launch walks (0 all, 1 the 32x32 band, 2 the rows below)
  int sb_rows32, band, nslots;
  int chains_cap, chains_waves; // how k_av1_chains' residency is limited (kChainsCap*), and to how many workgroups per CU
};

// frame f of the launch; kKey: 1 / 0 = the launch is known to hold key / inter frames (the choice at run time between the two sets of
// pointers put them into scratch memory)
template <int kKey = -1> __device__ __forceinline__ FrameView frame_view(const Av1EntLaunch &L, int f) {
  FrameView v = L.fv;
  const long nb = (long)v.w8 * v.h8;
  if (kKey < 0 ? v.key != 0 : kKey != 0) { v.y_mode += nb * f; v.uv_mode += nb * f; }
  else { v.mv += nb * 2 * f; v.skip += nb * f; }
  v.lev_y += nb * 64 * f; v.lev_u += nb * 16 * f; v.lev_v += nb * 16 * f;
  v.info = L.info + nb * f;
  if (L.lr_on_frame) for (int p = 0; p < 3; p++) v.lr_on[p] = v.lr_on[p] && L.lr_on_frame[f * 3 + p];
  for (int p = 0; p < 3; p++) if (v.lr_units[p]) v.lr_units[p] += L.lr_units_stride[p] * 8 * (size_t)f;
  if (v.cdef_idx) v.cdef_idx += L.cdef_idx_stride * (size_t)f;
  return v;
}

// the areas of tile t (av1_ops32.hpp: the tile's areas) out of the launch's pools
constexpr uint32_t kPoolLine = 32;      // words: 128 bytes
struct PoolAreas {
  const Av1EntLaunch &L; size_t t;
  __device__ __forceinline__ void reserve(int words, int entries, int *a, int *b) const {
    const uint32_t la = atomicAdd(L.cursors, ((uint32_t)words + kPoolLine - 1) / kPoolLine), lb = atomicAdd(L.cursors + 1, ((uint32_t)entries + kPoolLine - 1) / kPoolLine);
    L.list_off[t] = la; L.grouped_off[t] = lb;
    *a = (int)la; *b = (int)lb;
  }
  __device__ __forceinline__ op_t *list(int a) const { return L.ops + (size_t)(uint32_t)a * kPoolLine; }
  __device__ __forceinline__ uint32_t *grouped(int b) const { return L.grouped + (size_t)(uint32_t)b * kPoolLine; }
  __device__ __forceinline__ void slot(int sl, uint16_t total, uint16_t base) const { L.slot_total[t * S_MAX + sl] = total; L.slot_base[t * S_MAX + sl] = base; }
  __device__ __forceinline__ void refuse(int sl) const { L.slot_total[t * S_MAX + sl] = 0; }
};

// inter frames only: the tokenizer of a key frame reads nothing of a block's info
__global__ __launch_bounds__(256) void k_av1_info(Av1EntLaunch L) {
  const long nb = (long)L.fv.w8 * L.fv.h8, i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nb * L.nframes) return;
  const int f = (int)(i / nb), b = (int)(i - (long)f * nb);
  const FrameView v = frame_view<0>(L, f);
  BlockInfo o = {};
  inter_mode_decision(v, b / v.w8, b % v.w8, &o);
  L.info[nb * f + b] = o;
}

// The wave of a tile tokenizer (av1_ops32.hpp: each / scan / first / Var): one workgroup of 64 lanes
struct TileWave {
  template <class T> using Var = LaneVar<T, 1>;
  template <class F> __device__ __forceinline__ void each(F f) { f((int)threadIdx.x); __syncthreads(); }
  __device__ __forceinline__ int scan(Var<int> &v) {
    const int lane = (int)threadIdx.x, x = v.v[0];
    int inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(inc, d, 64);
      if (lane >= d) inc += y;
    }
    v.v[0] = inc - x;
    return __shfl(inc, 63, 64);
  }
  __device__ __forceinline__ int first(Var<int> &v) { return __shfl(v.v[0], 0, 64); }
  __device__ __forceinline__ uint64_t ballot(Var<int> &v) { return __ballot(v.v[0] != 0); }
};

// The tiles of 8x8 blocks: ONE WAVE PER TILE, a lane per block in z-order (av1_ops8.hpp tok_tile8): the neighbours' level summaries into
// LDS, TOKENIZE once (records + counts; every read of a coefficient after the first goes to the lane's LDS copy of the block), PLACE (the
// counts of the tile's 64 blocks -> where each block's entries of each slot go), REPLAY (records -> list words and grouped entries) —
// once for a tile that uses at most kReplaySlots slots, in two passes otherwise.  19.9 KB of LDS per wave: eight waves per CU, what the
// registers allow.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 8))) void k_av1_tokens(Av1EntLaunch L) {
  const int tiles = L.sbr_n * L.sbc_n, t = blockIdx.x, f = t / tiles, tt = t - f * tiles, sbr = tt / L.sbc_n, sbc = tt - sbr * L.sbc_n;
  if (sbr < L.sb_rows32) return;           // a tile of the 32x32 band: k_av1_tokens32
  const FrameView v = frame_view(L, f);
  __shared__ Tile8Mem S;
  const int below = tiles - L.sb_rows32 * L.sbc_n;      // the records are this band's alone: the frame's tiles below the 32x32 band
  uint16_t *rec = L.rec + ((size_t)f * below + (tt - (tiles - below))) * kBlocksPerTile * kBlockRecords;
  TileWave w;
  PoolAreas out = { L, (size_t)t };
  const int n = tok_tile8(w, S, v, sbr, sbc, rec, L.ops_cap, out);
  if (threadIdx.x == 0) {
    if (n < 0) atomicOr(L.status, 1u);
    L.nops[t] = n < 0 ? 0u : (uint32_t)n;
  }
}

// The tiles of a key frame's 32x32 band: ONE WAVE PER TILE, the lanes over scan ranges of the transform block at hand (av1_ops32.hpp
// tok_tile32: the levels are read once into magnitude maps in LDS, a counting sweep gives the slots' totals and bases, an emitting
// sweep writes list words and grouped entries straight to their places) — after which the chains, the range coder and the gather treat
// the tile like any other.  No records in memory (L.rec is the 8x8 band's).  15.7 KB of LDS per wave: ten waves per CU.
__global__ __launch_bounds__(64) void k_av1_tokens32(Av1EntLaunch L) {
  __shared__ Tile32Mem S;
  const int tiles = L.sbr_n * L.sbc_n, band = L.sb_rows32 * L.sbc_n, f = blockIdx.x / band, tt = blockIdx.x - f * band, sbr = tt / L.sbc_n, sbc = tt - sbr * L.sbc_n;
  const size_t t = (size_t)f * tiles + tt;          // (the band's tiles are a frame's first)
  const FrameView v = frame_view<1>(L, f);
  TileWave w;
  PoolAreas out = { L, t };
  const int n = tok_tile32(w, S, v, sbr, sbc, L.ops_cap, out);
  if (threadIdx.x == 0) {
    if (n < 0) atomicOr(L.status, 1u);
    L.nops[t] = n < 0 ? 0u : (uint32_t)n;
  }
}

// CHAINS: workgroup = one CDF slot of 64 consecutive tiles, one lane per tile.  The slot is the same for the whole wave (no
// divergence between alphabet sizes) and its chains are about equally long in neighbouring tiles, so the lanes stay busy — a
// tile's own slots differ in length by three orders of magnitude.  Small alphabets keep the CDF in registers, large ones in LDS.
// (Measured: a workgroup that walks several slots one after the other is slower — fewer, longer waves; about half of this
// kernel's time is the 4-byte scatter of the tuples into the lists.)
//
// RESIDENCY is bounded by the GRID.  The 64 lists of a group are completed word by word by all the group's slots, and the traffic stays
// near one read and one write per word only while their lines (about 1 MB per group, grouped entries included) stay in the XCD's 4 MB
// L2.  Left alone, an XCD holds 1 024 of these waves: the short slots retire at once, so the resident set fills with the long slots of
// many groups.  Two limiters, chosen per context (AV1MI_CHAINS_CAP, AV1MI_CHAINS_WAVES = W workgroups per CU):
//   tickets  a fixed grid of 8 XCDs x 32 CUs x W workgroups; each takes (group, slot) items of its XCD from a counter until the XCD's
//            groups are used up.  An XCD never has more than 32 W items open, and the kernel holds its 2 KB of LDS per workgroup and
//            nothing else: the LDS-using kernels of the other streams can start beside it.  NO WORKGROUP WAITS FOR ANOTHER: the counter
//            is a work queue, a workgroup that is never scheduled costs nothing, one that comes late finds the queue empty and leaves.
//   lds      one workgroup per item, and dynamic LDS nobody uses, sized so that W workgroups fit a CU (nominally: the hardware rounds
//            an allocation up to its granule, which may make it one fewer).  At W = 12 that is the CU's whole LDS: while chains waves
//            sit on a CU no workgroup of a kernel that uses LDS starts there.
// Either way an XCD opens its groups in turn and a group's slots longest first, and every (group, slot) is walked exactly once, so the
// bytes are the same.  Measured at 4K, q index 128: DESIGN 5.0-quater (lds: 2.5 GB per launch uncapped, 1.8 GB at 12 waves, 0.95 GB at
// 4) and 5.0-septies (tickets, profiles/chains_tickets_parent_vs_change.json): under lds the session is fastest at 12, because fewer
// waves still lock the CUs; under tickets the kernel alone is fastest at 6 (0.65 ms against 0.77) and the SESSION at 2, where the
// chains take twice as long beside the other kernels and the block pipeline, which is the longer queue, gets the CUs.  At 1 the
// chains become the longer queue.  Default: tickets, W = 2.
enum { kChainsInter = 0, kChainsKey8 = 1, kChainsKey32 = 2 };      // the launch flavours: each has its slot table and its rank
enum { kChainsCapLds = 0, kChainsCapTickets = 1 };
constexpr int kChainsStaticLds = 64 * 16 * 2, kCuLds = 160 << 10, kChainsXcds = 8, kChainsCusPerXcd = 32;
constexpr int kChainsDefaultCap = kChainsCapTickets, kChainsDefaultWaves = 2;
// the tickets live behind the batch's cursor line and are zeroed with it, by the one memset per batch: a row of eight counters, one per
// XCD, for each of a batch's two launches, EVERY COUNTER ON A 128-BYTE LINE OF ITS OWN.  (Measured: with the eight counters of a row in
// one line the 76 000 draws of a launch queue up behind one another at the memory side and the kernel alone takes 0.4 ms longer.)
constexpr int kTicketStride = 32, kTicketRowFirst = kTicketStride, kTicketRowBand32 = kTicketRowFirst + kChainsXcds * kTicketStride;
static unsigned chains_dynamic_lds(int waves) { return waves > 0 && kCuLds / waves > kChainsStaticLds ? (unsigned)(kCuLds / waves - kChainsStaticLds) : 0u; }

// one item: slot rank[k] of tile group g, a lane per tile
__device__ __forceinline__ void chains_item(const Av1EntLaunch &L, int ntiles_all, int flavour, int g, int k, uint16_t *s_big) {
  const int lane = threadIdx.x, t = g * 64 + lane;
  // the group's slots longest expected chain first (chains_rank.hpp)
  const int sl = (flavour == kChainsInter ? kChainsRankInter : flavour == kChainsKey8 ? kChainsRankKey8 : kChainsRankKey32)[k];
  const int n = L.tab.nsym[sl], off = L.tab.off[sl];
  int cnt = 0, base = 0;
  bool mine = t < ntiles_all;
  if (mine && L.band) { const int tiles = L.sbr_n * L.sbc_n, sbr = (t % tiles) / L.sbc_n; mine = (sbr < L.sb_rows32) == (L.band == 1); }
  if (mine) { cnt = L.slot_total[(size_t)t * S_MAX + sl]; base = L.slot_base[(size_t)t * S_MAX + sl]; }
  if (!__any(cnt > 0)) return;
  // (a tile without entries in the slot may be one that was refused and has no areas: its offsets are read by nobody)
  op_t *list = L.ops + (cnt > 0 ? (size_t)L.list_off[t] * kPoolLine : 0);
  const uint32_t *grouped = L.grouped + (cnt > 0 ? (size_t)L.grouped_off[t] * kPoolLine : 0) + base;
  if (n <= 4) {
    const uint32_t *iw = reinterpret_cast<const uint32_t *>(L.cdf_image) + (off >> 1);
    uint64_t cdf = (uint64_t)iw[0] | ((uint64_t)iw[1] << 32);
    // sixteen entries (four 16-byte loads) per round, requested a whole round ahead: the chain is serial and a load takes
    // longer than four of its steps
    const uint4 *g4 = reinterpret_cast<const uint4 *>(grouped);
    const uint4 z = make_uint4(0, 0, 0, 0);
    uint4 c0 = cnt > 0 ? g4[0] : z, c1 = cnt > 4 ? g4[1] : z, c2 = cnt > 8 ? g4[2] : z, c3 = cnt > 12 ? g4[3] : z;
    auto four = [&](const uint4 &v, int e) {
      if (e < cnt) list[v.x >> 4] = small_step(cdf, (int)(v.x & 15), n);
      if (e + 1 < cnt) list[v.y >> 4] = small_step(cdf, (int)(v.y & 15), n);
      if (e + 2 < cnt) list[v.z >> 4] = small_step(cdf, (int)(v.z & 15), n);
      if (e + 3 < cnt) list[v.w >> 4] = small_step(cdf, (int)(v.w & 15), n);
    };
#pragma unroll 1
    for (int e = 0; e < cnt; e += 16) {
      const uint4 *nx = g4 + (e >> 2) + 4;
      const uint4 n0 = e + 16 < cnt ? nx[0] : z, n1 = e + 20 < cnt ? nx[1] : z, n2 = e + 24 < cnt ? nx[2] : z, n3 = e + 28 < cnt ? nx[3] : z;
      four(c0, e); four(c1, e + 4); four(c2, e + 8); four(c3, e + 12);
      c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
  } else {
    uint16_t *cdf = s_big + lane * 16;
    {
      const uint4 *iw = reinterpret_cast<const uint4 *>(L.cdf_image + off);
      uint4 *d = reinterpret_cast<uint4 *>(cdf);
      d[0] = iw[0];
      d[1] = n > 8 ? iw[1] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll 1
    for (int e = 0; e < cnt; e++) {
      const uint32_t v = grouped[e];
      const int s = (int)(v & 15);
      list[v >> 4] = s >= kSplitHorz ? split_tuple(cdf, s) : big_step(cdf, s, n);
    }
  }
}

// tickets: one row of kChainsXcds counters, zero at the start of the batch (the fixed grid takes items from them), or null (one
// workgroup per item: a grid of ((ngroups + 7) / 8) * 8 * nslots workgroups)
__global__ __launch_bounds__(64) void k_av1_chains(Av1EntLaunch L, int ntiles_all, int ngroups, int flavour, uint32_t *tickets) {
  // workgroups are dealt to the eight XCDs in turn (id % 8), each with its own L2: all slots of a tile group go to ONE XCD, one
  // after the other, so the 64 lists the group's chains complete word by word stay in that L2 as long as possible.  (Were they dealt
  // otherwise, the items would still be walked exactly once each, only on other L2s.)
  const int xcd = blockIdx.x & (kChainsXcds - 1), nslots = L.nslots;
  __shared__ __attribute__((aligned(16))) uint16_t s_big[64 * 16];      // a lane's own 16 words, written afresh by every item that uses them
  uint32_t j = blockIdx.x >> 3;
  for (;;) {
    if (tickets) {       // the workgroup is one wave: lane 0 draws, the wave reads its lane — no barrier, and nothing to wait for
      uint32_t drawn = 0;
      if (threadIdx.x == 0) drawn = atomicAdd(tickets + xcd * kTicketStride, 1u);
      j = (uint32_t)__shfl((int)drawn, 0, 64);
    }
    const int g = (int)(j / (uint32_t)nslots) * kChainsXcds + xcd, k = (int)(j % (uint32_t)nslots);
    if (g >= ngroups) return;
    chains_item(L, ntiles_all, flavour, g, k, s_big);
    if (!tickets) return;
  }
}

// 64 lanes (tiles) per workgroup; per lane in LDS a ring of 64 list words and the coder's byte stage (32 x 16 bits).
//
// The chain is serial and the lanes of a wave are at different places of different tiles: what counts is the latency of one step.
//  * one interval update per step for every lane, whatever the word: a tuple, or one bit of a literal;
//  * NO global memory in the steady state (a wait for memory on gfx9 waits for every outstanding vector-memory operation,
//    stores included).  Words come from the LDS ring, bytes go to the LDS stage; both meet global memory in rare PHASES the whole
//    wave takes together: 32 words per lane are requested into registers in one phase and written to the ring in the next (the
//    loads have long landed), the stages are stored.  A phase is due when a lane has fewer than 24 words staged or a stage is
//    nearly full; that is looked at every eight steps.
constexpr int kRingOps = 64, kLaneWords = kRingOps * 2 + Coder::kStage + 8;     // uint16 per lane; + 8: the lanes start on different banks

__global__ __launch_bounds__(64) void k_av1_code(Av1EntLaunch L, int ntiles_all) {
  // (Measured, round 3: s_setprio(3) for these lone latency-bound waves changes nothing, with four or with eight hardware queues —
  // they do not lose issue slots to co-resident waves; what the streams compete for is residency: LDS and wave slots per CU.)
  __shared__ __attribute__((aligned(16))) uint16_t s_lane[64 * kLaneWords];
  const int lane = threadIdx.x, t = blockIdx.x * 64 + lane;
  const bool live = t < ntiles_all;
  uint32_t *ring = reinterpret_cast<uint32_t *>(s_lane + lane * kLaneWords);
  Coder c;
  c.init(L.slots + (size_t)(live ? t : 0) * L.slot_cap, (int)L.slot_cap, s_lane + lane * kLaneWords + kRingOps * 2);
  const int n = live ? (int)L.nops[t] : 0;
  const uint4 *ops4 = reinterpret_cast<const uint4 *>(L.ops + (n ? (size_t)L.list_off[t] * kPoolLine : 0));
  // words [w - 64, w) are in the ring; `pend`: words [w, w + 32) are on their way into r0..r7
  uint4 r0, r1, r2, r3, r4, r5, r6, r7;
  r0 = r1 = r2 = r3 = r4 = r5 = r6 = r7 = make_uint4(0, 0, 0, 0);
  int w = 0;
  bool pend = false;
  auto request = [&]() {
    const uint4 *p = ops4 + (w >> 2);
    if (w < n) r0 = p[0];
    if (w + 4 < n) r1 = p[1];
    if (w + 8 < n) r2 = p[2];
    if (w + 12 < n) r3 = p[3];
    if (w + 16 < n) r4 = p[4];
    if (w + 20 < n) r5 = p[5];
    if (w + 24 < n) r6 = p[6];
    if (w + 28 < n) r7 = p[7];
    pend = w < n;
  };
  auto take = [&]() {
    uint4 *q = reinterpret_cast<uint4 *>(ring + (w & 32));
    q[0] = r0; q[1] = r1; q[2] = r2; q[3] = r3; q[4] = r4; q[5] = r5; q[6] = r6; q[7] = r7;
    w += 32;
  };
  request();
  if (pend) { take(); request(); }
  int i = 0, lit_left = 0;
  // the word of this step and the next two in registers; the ring read of a step is issued before its arithmetic and used after
  // it (read and moved back to back, every step waited a whole LDS latency)
  uint32_t op = ring[0], op_next = ring[1], op_next2 = ring[2];
  for (;;) {
    // the checks every eight steps: a lane advances by at most eight words and eight stage entries in between
    if (!__any(lit_left > 0 || i < n)) break;
    if (__any((pend && w - i < 24) || c.ns >= Coder::kStage - 8)) {      // a phase
      if (pend && w - i <= 32) { take(); request(); }
      c.spill();
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
      if (lit_left > 0 || i < n) {
        const uint32_t fetched = ring[(i + 3) & (kRingOps - 1)];      // requested first, used last: the word an advance shifts in
        uint32_t tup = op;
        if (lit_left == 0 && (op >> 31)) lit_left = (int)((op >> 27) & 15);
        if (lit_left > 0) {         // one equiprobable bit: the tuples of (icdf 16384 | 0, symbol 1 of 2) and (32768 | 16384, symbol 0 of 2)
          lit_left--;
          tup = (op >> lit_left) & 1 ? (1u << 19) | (256u << 9) : (2u << 19) | (512u << 9) | 256u;
        }
        c.encode_tuple(tup);
        if (lit_left == 0) { i++; op = op_next; op_next = op_next2; op_next2 = fetched; }
      }
    }
  }
  int sz = 0;
  if (live) {
    sz = n ? c.finish() : -1;          // n == 0: the list overflowed (k_av1_tokens), nothing to code
    if (sz < 0) { if (n) atomicOr(L.status, 2u); sz = 0; }
    L.tile_size[t] = (uint32_t)sz;
  }
  // the group's bytes (64 x slot_cap fits 32 bits), for the gather's offsets; a lane without a tile adds nothing
  unsigned sum = (unsigned)sz;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, d, 64);
  if (lane == 0) L.group_sum[blockIdx.x] = sum;
}

// one workgroup per tile; `out` may be pinned host memory (the GOP session hands the payloads straight to the host this way):
// bytes up to the first 16-byte boundary of the destination, then aligned 16-byte stores, then the tail.
// The tile's offset is the bytes of all tiles before it: the sums of the groups below its own (k_av1_code) plus the sizes of its own
// group's tiles below it — at most groups / 64 + 1 coalesced loads per lane and one wave reduction, in 64 bits.  The last tile's
// workgroup therefore knows the total: it sets status bit 2 where that exceeds out_cap (bits 0 and 1 were set by kernels that have
// finished), and writes total and status to the job's d_total.  Where the caller gave pinned mirrors (Av1EntMirrors) every workgroup
// stores its tile's size there and the last one total, status and the restoration flags: plain stores, ordered for the host by the
// event behind this launch like the payloads themselves.
__global__ __launch_bounds__(64) void k_av1_gather(Av1EntLaunch L, int ntiles_all) {
  const int t = blockIdx.x, lane = threadIdx.x, g = t >> 6;
  uint64_t off = 0;
  for (int i = lane; i < g; i += 64) off += L.group_sum[i];
  if (g * 64 + lane < t) off += L.tile_size[g * 64 + lane];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) off += __shfl_xor(off, d, 64);
  const uint32_t n = L.tile_size[t];
  if (lane == 0 && L.mir.h_tile_size) L.mir.h_tile_size[t] = n;
  if (t == ntiles_all - 1) {
    if (lane == 0) {
      const uint64_t total = off + n;
      uint32_t status = *L.status;
      if (total > L.out_cap) status |= 4u;
      L.total[0] = total; *L.status = status;
      if (L.mir.h_total) { L.mir.h_total[0] = total; L.mir.h_total[1] = status; }
    }
    if (L.mir.h_lr_on && L.lr_on_frame)
      for (uint32_t i = lane; i < L.mir.lr_on_bytes; i += 64) L.mir.h_lr_on[i] = L.lr_on_frame[i];
  }
  if (off + n > L.out_cap) return;
  const uint8_t *src = L.slots + (size_t)t * L.slot_cap;
  uint8_t *dst = L.out + off;
  const uint32_t head = min(n, (uint32_t)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15)), body = (n - head) >> 4, tail0 = head + (body << 4);
  if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
  for (uint32_t i = threadIdx.x; i < body; i += 64) {
    uint4 v;
    __builtin_memcpy(&v, src + head + 16 * i, 16);       // the source is not aligned with the destination
    *reinterpret_cast<uint4 *>(dst + head + 16 * i) = v;
  }
  if (tail0 + threadIdx.x < n) dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
}

hipError_t launch_av1_front(av1mi_ctx *ctx, const Av1EntLaunch &L, hipStream_t s) {
  const long nb = (long)L.fv.w8 * L.fv.h8 * L.nframes;
  const int ntiles_all = L.sbr_n * L.sbc_n * L.nframes, ngroups = (ntiles_all + 63) / 64;
  ProfToken t = ctx_prof_begin(ctx, AV1MI_K_ENTROPY_TOKENS, s);
  if (!L.fv.key) hipLaunchKernelGGL(k_av1_info, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, L);
  if (L.sb_rows32 < L.sbr_n) hipLaunchKernelGGL(k_av1_tokens, dim3((unsigned)ntiles_all), dim3(64), 0, s, L);
  if (L.sb_rows32) hipLaunchKernelGGL(k_av1_tokens32, dim3((unsigned)(L.sb_rows32 * L.sbc_n * L.nframes)), dim3(64), 0, s, L);
  ctx_prof_end(ctx, t, s);
  t = ctx_prof_begin(ctx, AV1MI_K_ENTROPY_CHAINS, s);
  Av1EntLaunch C = L;
  C.nslots = L.fv.key ? S_KEY_END : S_INTER_END; C.band = L.sb_rows32 ? 2 : 0;
  const bool by_tickets = L.chains_cap == kChainsCapTickets;
  const unsigned lds = by_tickets ? 0u : chains_dynamic_lds(L.chains_waves);
  auto chains = [&](int flavour, int ticket_row) {
    const unsigned grid = by_tickets ? (unsigned)(kChainsXcds * kChainsCusPerXcd * L.chains_waves) : (unsigned)(((ngroups + 7) / 8) * 8 * C.nslots);
    hipLaunchKernelGGL(k_av1_chains, dim3(grid), dim3(64), lds, s, C, ntiles_all, ngroups, flavour, by_tickets ? L.cursors + ticket_row : nullptr);
  };
  if (L.sb_rows32 < L.sbr_n) chains(L.fv.key ? kChainsKey8 : kChainsInter, kTicketRowFirst);
  if (L.sb_rows32) {       // the 32x32 band's tiles: their slot table and default CDFs
    C.nslots = K_END; C.band = 1; C.tab = L.tab32; C.cdf_image = L.cdf_image32;
    chains(kChainsKey32, kTicketRowBand32);
  }
  ctx_prof_end(ctx, t, s);
  return hipGetLastError();
}
hipError_t launch_av1_back(av1mi_ctx *ctx, const Av1EntLaunch &L, hipStream_t s) {
  const int ntiles_all = L.sbr_n * L.sbc_n * L.nframes;
  ProfToken t = ctx_prof_begin(ctx, AV1MI_K_ENTROPY, s);
  hipLaunchKernelGGL(k_av1_code, dim3((unsigned)((ntiles_all + 63) / 64)), dim3(64), 0, s, L, ntiles_all);
  ctx_prof_end(ctx, t, s);
  t = ctx_prof_begin(ctx, AV1MI_K_ENTROPY_PACK, s);
  hipLaunchKernelGGL(k_av1_gather, dim3((unsigned)ntiles_all), dim3(64), 0, s, L, ntiles_all);
  ctx_prof_end(ctx, t, s);
  return hipGetLastError();
}

}  // namespace av1mi

// ------------------------------------------------------------------------------------------------ C ABI
struct av1mi_av1ent_state {      // per-context scratch of the coder, grown on demand (owned through av1mi_av1_entropy_release)
  void *info = nullptr, *ops[2] = { nullptr, nullptr }, *nops[2] = { nullptr, nullptr }, *grouped = nullptr, *grouped_off = nullptr, *slot_tb = nullptr, *rec = nullptr, *slots = nullptr, *group_sum = nullptr, *status = nullptr;
  size_t info_b = 0, ops_b[2] = { 0, 0 }, nops_b[2] = { 0, 0 }, grouped_b = 0, grouped_off_b = 0, slot_tb_b = 0, rec_b = 0, slots_b = 0, group_sum_b = 0;
  // the lists (ops; nops with the lists' offsets behind them) exist twice: job k uses set k & 1, so the front half of job k + 1 may run beside the back half of job k
  hipEvent_t lists_ready[2] = { nullptr, nullptr }, lists_free[2] = { nullptr, nullptr };
  bool free_recorded[2] = { false, false };
  unsigned long jobs = 0;
  av1mi::Av1EntLaunch pending[2];             // a job whose back half (range coder, gather) is still to be launched (av1_entropy_back)
  bool pending_valid[2] = { false, false };
  size_t last_tiles = 0;          // tiles of the most recent job (av1mi_av1_entropy_last_list_words)
  uint16_t *d_image[2][4] = {};   // [key][qcat] default CDF images
  uint16_t *d_image32[4] = {};    // [qcat] the 32x32 band's
  av1ops::SlotTable tab32;        // the 32x32 band's slot table (the same for every q category)
  int image_words[2] = { 0, 0 };
  av1ops::SlotTable tab[2];
  // k_av1_chains' residency limiter, read once when the context's coder state is made.  Diagnostics, like AV1MI_CODER_STREAMS:
  // AV1MI_CHAINS_CAP = lds | tickets, AV1MI_CHAINS_WAVES = workgroups per CU (1..32); anything else leaves the default
  int chains_cap = av1mi::kChainsDefaultCap, chains_waves = av1mi::kChainsDefaultWaves;
};

namespace {
constexpr size_t kCursorBytes = 128 * (1 + 2 * av1mi::kChainsXcds);      // the pools' cursor line, then a line per ticket counter
static_assert((av1mi::kTicketRowBand32 + av1mi::kChainsXcds * av1mi::kTicketStride) * sizeof(uint32_t) <= kCursorBytes && av1mi::kTicketRowFirst >= 2, "the tickets lie in the zeroed area, behind the pool cursors");
int grow(av1mi_ctx *ctx, void **p, size_t *have, size_t need) {
  if (*have >= need) return AV1MI_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr; *have = 0;
  if (hipMalloc(p, need) != hipSuccess) return av1mi::ctx_fail(ctx, AV1MI_E_NOMEM, "AV1 entropy scratch: hipMalloc(%zu) failed", need);
  *have = need;
  return AV1MI_OK;
}
}  // namespace

extern "C" {

// Capacities, sized on the densest content measured (tools: AV1MI_TOK_STATS in host/av1_opstream.cpp; 4K 10-bit noise-dominated key
// frames at the reference's quality 23: <= 485 records in a block before the tile's restoration / CDEF syntax, which rides on the
// tile's first block — 512 overflowed there —, <= 22 394 list words in a tile).  Not the syntax's worst case (~820 records per block,
// ~52 000 words per tile): a tile beyond them raises a status bit and the session hands the batch to the host writer.
uint32_t av1mi_av1_entropy_ops_per_tile(void) { return 32768; }
uint32_t av1mi_av1_entropy_slot_bytes(void) { return 16384; }

}  // extern "C"

int av1mi::av1_entropy_front(av1mi_ctx *ctx, const av1mi_av1_entropy_job *j, hipStream_t front, int *ticket, const av1mi_av1_entropy_units *units,
                             const av1mi_av1_entropy_cdef *cdef) {
  if (!ctx || !ticket) return AV1MI_E_INVAL;
  *ticket = -1;
  if (!j) return av1mi::ctx_fail(ctx, AV1MI_E_INVAL, "null job");
  if (hipSetDevice(av1mi::ctx_device(ctx)) != hipSuccess) return av1mi::ctx_fail(ctx, AV1MI_E_DEVICE, "hipSetDevice failed");
  if (j->width <= 0 || j->height <= 0 || (j->width & 7) || (j->height & 7) || j->width > 4096 || j->height > 4096)
    return av1mi::ctx_fail(ctx, AV1MI_E_INVAL, "frame %dx%d must be a multiple of 8, at most 4096x4096", j->width, j->height);
  if (j->nframes < 0 || j->nframes > 4096 || j->base_q_idx < 1 || j->base_q_idx > 255) return av1mi::ctx_fail(ctx, AV1MI_E_INVAL, "bad nframes / base_q_idx");
  const void *need[] = { j->d_lev_y, j->d_lev_u, j->d_lev_v, j->d_out, j->d_tile_size, j->d_total, j->key ? (const void *)j->d_modes_y : (const void *)j->d_mvs,
                         j->key ? (const void *)j->d_modes_uv : (const void *)j->d_skip };
  for (const void *p : need) if (!p) return av1mi::ctx_fail(ctx, AV1MI_E_INVAL, "null device pointer");
  if (units) {      // all three planes' records or none, each read as 64-bit words
    const bool any = units->d_units[0] || units->d_units[1] || units->d_units[2], all = units->d_units[0] && units->d_units[1] && units->d_units[2];
    if (any && !all) return av1mi::ctx_fail(ctx, AV1MI_E_INVAL, "restoration units: the records of all three planes, or of none");
    for (int p = 0; p < 3; p++) if ((uintptr_t)units->d_units[p] & 7) return av1mi::ctx_fail(ctx, AV1MI_E_INVAL, "restoration units: misaligned device pointer (8 bytes)");
  }
  if (cdef && (cdef->cdef_bits < 0 || cdef->cdef_bits > 3)) return av1mi::ctx_fail(ctx, AV1MI_E_INVAL, "CDEF indices: cdef_bits %d outside 0 .. 3", cdef->cdef_bits);
  if (j->nframes == 0) return AV1MI_OK;
  av1mi_av1ent_state *st = av1mi::ctx_av1ent(ctx);
  if (!st) return av1mi::ctx_fail(ctx, AV1MI_E_NOMEM, "AV1 entropy state");
  const int key = j->key ? 1 : 0, qcat = av1ops::q_category(j->base_q_idx);
  if (!st->d_image[key][qcat]) {
    av1ops::SlotTable tab;
    const std::vector<uint16_t> img = av1ops::default_slot_image(key != 0, qcat, &tab);
    st->tab[key] = tab; st->image_words[key] = tab.words;
    if (hipMalloc((void **)&st->d_image[key][qcat], img.size() * 2) != hipSuccess ||
        hipMemcpy(st->d_image[key][qcat], img.data(), img.size() * 2, hipMemcpyHostToDevice) != hipSuccess)
      return av1mi::ctx_fail(ctx, AV1MI_E_DEVICE, "uploading the default CDF image failed");
  }
  if (j->key_rows32 && (!key || (j->key_rows32 & 63) || j->key_rows32 > j->height || (j->width & 31)))
    return av1mi::ctx_fail(ctx, AV1MI_E_INVAL, "key_rows32 %d: whole superblock rows of a key frame whose width is a multiple of 32", j->key_rows32);
  if (j->key_rows32 && !st->d_image32[qcat]) {
    const std::vector<uint16_t> img = av1ops::default_slot_image_k32(qcat, &st->tab32);
    if (hipMalloc((void **)&st->d_image32[qcat], img.size() * 2) != hipSuccess ||
        hipMemcpy(st->d_image32[qcat], img.data(), img.size() * 2, hipMemcpyHostToDevice) != hipSuccess)
      return av1mi::ctx_fail(ctx, AV1MI_E_DEVICE, "uploading the default CDF image failed");
  }
  av1mi::Av1EntLaunch L;
  memset(&L, 0, sizeof(L));
  L.sb_rows32 = j->key_rows32 / 64;
  if (j->key_rows32) { L.tab32 = st->tab32; L.cdf_image32 = st->d_image32[qcat]; }
  L.fv.w8 = j->width / 8; L.fv.h8 = j->height / 8; L.fv.key = key;
  L.fv.y_mode = j->d_modes_y; L.fv.uv_mode = j->d_modes_uv; L.fv.mv = j->d_mvs; L.fv.skip = j->d_skip;
  L.fv.lev_y = j->d_lev_y; L.fv.lev_u = j->d_lev_u; L.fv.lev_v = j->d_lev_v;
  for (int p = 0; p < 3; p++) {
    L.fv.lr_on[p] = j->lr_on[p] != 0;
    const int vh = j->visible_height ? j->visible_height : j->height, vw = j->visible_width ? j->visible_width : j->width;   // the units tile the TRUE frame
    const int ph = p ? (vh + 1) / 2 : vh, pw = p ? (vw + 1) / 2 : vw;
    L.fv.lr_rows[p] = (ph + 32) / 64 > 1 ? (ph + 32) / 64 : 1; L.fv.lr_cols[p] = (pw + 32) / 64 > 1 ? (pw + 32) / 64 : 1;
  }
  memcpy(L.fv.lr_unit[0], j->lr_unit_y, 8); memcpy(L.fv.lr_unit[1], j->lr_unit_uv, 8);
  L.nframes = j->nframes; L.sbr_n = (L.fv.h8 + 7) / 8; L.sbc_n = (L.fv.w8 + 7) / 8;
  const size_t nb = (size_t)L.fv.w8 * L.fv.h8 * j->nframes, nt = (size_t)L.sbr_n * L.sbc_n * j->nframes;
  L.ops_cap = av1mi_av1_entropy_ops_per_tile(); L.slot_cap = av1mi_av1_entropy_slot_bytes();
  L.grouped_cap = L.ops_cap + av1ops::kListAlign * av1ops::S_MAX;      // every slot's entries start on 16 bytes
  const int par = (int)(st->jobs++ & 1);
  st->last_tiles = nt;
  int rc;
  if ((rc = grow(ctx, &st->info, &st->info_b, nb * sizeof(av1ops::BlockInfo))) ||
      (rc = grow(ctx, &st->ops[par], &st->ops_b[par], nt * L.ops_cap * sizeof(av1ops::op_t))) || (rc = grow(ctx, &st->nops[par], &st->nops_b[par], nt * 8)) ||
      (rc = grow(ctx, &st->grouped, &st->grouped_b, nt * L.grouped_cap * sizeof(uint32_t))) || (rc = grow(ctx, &st->grouped_off, &st->grouped_off_b, nt * 4)) ||
      (rc = grow(ctx, &st->slot_tb, &st->slot_tb_b, kCursorBytes + nt * av1ops::S_MAX * 4)) ||
      (rc = grow(ctx, &st->rec, &st->rec_b, (size_t)(L.sbr_n - L.sb_rows32) * L.sbc_n * j->nframes * av1ops::kBlocksPerTile * av1ops::kBlockRecords * sizeof(uint16_t))) ||
      (rc = grow(ctx, &st->slots, &st->slots_b, nt * L.slot_cap)) || (rc = grow(ctx, &st->group_sum, &st->group_sum_b, ((nt + 63) / 64) * 8)))
    return rc;
  L.info = (av1ops::BlockInfo *)st->info; L.ops = (av1ops::op_t *)st->ops[par]; L.nops = (uint32_t *)st->nops[par]; L.grouped = (uint32_t *)st->grouped;
  L.list_off = L.nops + nt; L.grouped_off = (uint32_t *)st->grouped_off;
  L.cursors = (uint32_t *)st->slot_tb;        // the pools' cursors: a line of their own in front of the slot tables
  L.slot_total = (uint16_t *)((uint8_t *)st->slot_tb + kCursorBytes); L.slot_base = L.slot_total + nt * av1ops::S_MAX; L.rec = (uint16_t *)st->rec; L.slots = (uint8_t *)st->slots;
  L.group_sum = (uint64_t *)st->group_sum;
  L.tile_size = j->d_tile_size; L.out = j->d_out; L.out_cap = j->out_cap;
  L.total = j->d_total; L.status = (uint32_t *)(j->d_total + 1);
  L.cdf_image = st->d_image[key][qcat]; L.cdf_words = st->image_words[key]; L.tab = st->tab[key];
  L.lr_on_frame = j->d_lr_on;
  L.chains_cap = st->chains_cap; L.chains_waves = st->chains_waves;
  if (units) for (int p = 0; p < 3; p++) { L.fv.lr_units[p] = units->d_units[p]; L.lr_units_stride[p] = units->frame_stride[p]; }
  if (cdef && cdef->cdef_bits) { L.fv.cdef_bits = cdef->cdef_bits; L.fv.cdef_idx = cdef->d_idx; L.cdef_idx_stride = cdef->frame_stride; }
#define E_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return av1mi::ctx_fail(ctx, AV1MI_E_DEVICE, "%s: %s", #call, hipGetErrorString(e_)); } while (0)
  for (hipEvent_t *ev : { &st->lists_ready[par], &st->lists_free[par] }) if (!*ev) E_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  if (st->free_recorded[par]) E_HIP(hipStreamWaitEvent(front, st->lists_free[par], 0));      // the coder of two jobs ago still reads this set of lists
  E_HIP(hipMemsetAsync(j->d_total, 0, 16, front));
  E_HIP(hipMemsetAsync(L.cursors, 0, kCursorBytes, front));
  E_HIP(av1mi::launch_av1_front(ctx, L, front));
  E_HIP(hipEventRecord(st->lists_ready[par], front));
  st->pending[par] = L; st->pending_valid[par] = true;
  *ticket = par;
  return AV1MI_OK;
}

// the back half of the job `ticket` names (av1_entropy_front): the serial range coder and the gather, which also delivers sizes,
// total and status (to the job's device arrays, and to the pinned mirrors where the caller gives them)
int av1mi::av1_entropy_back(av1mi_ctx *ctx, int ticket, hipStream_t back, const Av1EntMirrors *mirrors) {
  if (!ctx || ticket < 0 || ticket > 1) return AV1MI_E_INVAL;
  av1mi_av1ent_state *st = av1mi::ctx_av1ent(ctx);
  if (!st || !st->pending_valid[ticket]) return av1mi::ctx_fail(ctx, AV1MI_E_INVAL, "no entropy job pending under this ticket");
  av1mi::Av1EntLaunch L = st->pending[ticket];
  if (mirrors) L.mir = *mirrors;
  E_HIP(hipStreamWaitEvent(back, st->lists_ready[ticket], 0));
  E_HIP(av1mi::launch_av1_back(ctx, L, back));
  E_HIP(hipEventRecord(st->lists_free[ticket], back)); st->free_recorded[ticket] = true;
  st->pending_valid[ticket] = false;
#undef E_HIP
  return AV1MI_OK;
}

int av1mi::av1_entropy_submit(av1mi_ctx *ctx, const av1mi_av1_entropy_job *j, hipStream_t front, hipStream_t back, const Av1EntMirrors *mirrors,
                              const av1mi_av1_entropy_units *units, const av1mi_av1_entropy_cdef *cdef) {
  int ticket = -1;
  const int rc = av1_entropy_front(ctx, j, front, &ticket, units, cdef);
  if (rc != AV1MI_OK || ticket < 0) return rc;      // (an empty job has no back half)
  return av1_entropy_back(ctx, ticket, back, mirrors);
}

extern "C" {

int av1mi_av1_entropy_encode_sides(av1mi_ctx *ctx, const av1mi_av1_entropy_job *j, const av1mi_av1_entropy_units *units, const av1mi_av1_entropy_cdef *cdef,
                                   void *stream_handle) {
  if (!ctx) return AV1MI_E_INVAL;
  hipStream_t s = stream_handle ? (hipStream_t)stream_handle : av1mi::ctx_stream(ctx);
  return av1mi::av1_entropy_submit(ctx, j, s, s, nullptr, units, cdef);
}
int av1mi_av1_entropy_encode_units(av1mi_ctx *ctx, const av1mi_av1_entropy_job *j, const av1mi_av1_entropy_units *units, void *stream_handle) {
  if (!ctx) return AV1MI_E_INVAL;
  hipStream_t s = stream_handle ? (hipStream_t)stream_handle : av1mi::ctx_stream(ctx);
  return av1mi::av1_entropy_submit(ctx, j, s, s, nullptr, units);
}
int av1mi_av1_entropy_encode_on(av1mi_ctx *ctx, const av1mi_av1_entropy_job *j, void *stream_handle) {
  if (!ctx) return AV1MI_E_INVAL;
  hipStream_t s = stream_handle ? (hipStream_t)stream_handle : av1mi::ctx_stream(ctx);
  return av1mi::av1_entropy_submit(ctx, j, s, s);
}

int av1mi_av1_entropy_encode(av1mi_ctx *ctx, const av1mi_av1_entropy_job *j) { return av1mi_av1_entropy_encode_on(ctx, j, nullptr); }

int av1mi_av1_entropy_last_list_words(av1mi_ctx *ctx, uint64_t *words) {
  if (!ctx || !words) return AV1MI_E_INVAL;
  *words = 0;
  av1mi_av1ent_state *st = av1mi::ctx_av1ent(ctx);
  if (!st || !st->jobs || !st->last_tiles) return AV1MI_OK;
  if (hipSetDevice(av1mi::ctx_device(ctx)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return av1mi::ctx_fail(ctx, AV1MI_E_DEVICE, "synchronising failed");
  std::vector<uint32_t> n(st->last_tiles);
  if (hipMemcpy(n.data(), st->nops[(st->jobs - 1) & 1], n.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return av1mi::ctx_fail(ctx, AV1MI_E_DEVICE, "reading the list sizes failed");
  for (uint32_t v : n) *words += v;
  return AV1MI_OK;
}

}  // extern "C"

namespace av1mi {
void av1ent_free(av1mi_av1ent_state *st) {
  if (!st) return;
  for (void *p : { st->info, st->ops[0], st->ops[1], st->nops[0], st->nops[1], st->grouped, st->grouped_off, st->slot_tb, st->rec, st->slots, st->group_sum }) if (p) (void)hipFree(p);
  for (hipEvent_t ev : { st->lists_ready[0], st->lists_ready[1], st->lists_free[0], st->lists_free[1] }) if (ev) (void)hipEventDestroy(ev);
  for (auto &k : st->d_image) for (uint16_t *p : k) if (p) (void)hipFree(p);
  for (uint16_t *p : st->d_image32) if (p) (void)hipFree(p);
  delete st;
}
av1mi_av1ent_state *av1ent_new() {
  av1mi_av1ent_state *st = new (std::nothrow) av1mi_av1ent_state();
  if (!st) return st;
  if (const char *e = getenv("AV1MI_CHAINS_CAP")) st->chains_cap = !strcmp(e, "tickets") ? kChainsCapTickets : !strcmp(e, "lds") ? kChainsCapLds : st->chains_cap;
  if (const char *e = getenv("AV1MI_CHAINS_WAVES")) { const int w = atoi(e); if (w >= 1 && w <= 32) st->chains_waves = w; }
  return st;
}
}  // namespace av1mi
