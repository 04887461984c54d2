// The launch selection of the split-fp16 convolution (x3_select.h): host-only.  Every heuristic
// that picks a conv_x3_f16 / conv_x3_wr instance for a launch lives here, as one function of the
// launch descriptor, the device's CU count and the ISLPOSE_* switches.
#include "x3_select.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace isl {

// ---------------------------------------------------------------------------
// The switches.  Their meanings stand with the heuristics that read them, below and in
// runtime.cpp (plan_steps); conv.hip reads ISLPOSE_CONV_STAGING and conv_x3.hip hands
// ISLPOSE_X3_ABL to its development kernels.  The run_key rows keep their order: a graph's run
// key hashes them in it.
// ---------------------------------------------------------------------------
static const X3SwitchDef kSwitches[] = {
    {"ISLPOSE_X3_DEEP", &X3Switches::deep, 2, "01", true},
    {"ISLPOSE_RGB_CONV", &X3Switches::rgb_conv, 1, "0", true},
    {"ISLPOSE_FUSED_POOL", &X3Switches::fused_pool, 1, "0", true},
    {"ISLPOSE_POOL_INPUT", &X3Switches::pool_input, 1, "0", true},
    {"ISLPOSE_CONV_STAGING", &X3Switches::conv_staging, 0, nullptr, true},
    {"ISLPOSE_X3_TILES", &X3Switches::tiles_small, 0, "s", true},
    {"ISLPOSE_X3_UNION", &X3Switches::union_mode, 1, nullptr, true},
    {"ISLPOSE_X3_HALF64", &X3Switches::half64, 1, "0", true},
    {"ISLPOSE_X3_WIDE7", &X3Switches::wide7, 2, nullptr, true},
    {"ISLPOSE_X3_ACROSS", &X3Switches::across, -1, nullptr, true},
    {"ISLPOSE_X3_S8", &X3Switches::s8, 1, nullptr, true},
    {"ISLPOSE_X3_FUSE67", &X3Switches::fuse67, -1, "0123", true},
    {"ISLPOSE_X3_G2", &X3Switches::g2, 1, "0", true},
    {"ISLPOSE_X3_PX64", &X3Switches::px64, 2, nullptr, true},
    {"ISLPOSE_X3_HALFSMALL", &X3Switches::halfsmall, 1, "0", true},
    {"ISLPOSE_X3_WR", &X3Switches::wr, 1, nullptr, true},
    {"ISLPOSE_X3_WR_WN", &X3Switches::wr_wn, 1, "2", true},
    {"ISLPOSE_C12", &X3Switches::c12, 1, "02", true},
    {"ISLPOSE_X3_TAIL", &X3Switches::tail, 1, "0", true},
    {"ISLPOSE_X3_SMALL7", &X3Switches::small7, 2, nullptr, true},
    {"ISLPOSE_X3_W2", &X3Switches::w2, 2, "012", true},
    {"ISLPOSE_X3_S7W96", &X3Switches::s7w96, 1, "0", true},
    {"ISLPOSE_A16_DMA", &X3Switches::a16_dma, 1, "0", true},
#ifdef ISLPOSE_DEV
    {"ISLPOSE_X3_HALFCO", &X3Switches::halfco, 2, "01", true},
    {"ISLPOSE_X3_PPS2", &X3Switches::pps2, 0, "1", true},
    {"ISLPOSE_X3_M16", &X3Switches::m16, 0, "1", true},
    {"ISLPOSE_X3_WINO", &X3Switches::x3_wino, 0, "1", true},
    {"ISLPOSE_X3_ABL", &X3Switches::abl, 0, nullptr, true},
    // (a run with the fold on is never replayed from a graph)
    {"ISLPOSE_X3_FOLD", &X3Switches::fold, 0, "1", false},
#endif
};

const X3SwitchDef* x3_switch_table(int* count) {
  *count = (int)(sizeof(kSwitches) / sizeof(kSwitches[0]));
  return kSwitches;
}

X3Switches x3_switches() {
  X3Switches sw{};
  sw.halfco = 2;   // (the defaults of the development switches in a product build)
  for (const X3SwitchDef& d : kSwitches) {
    const char* e = getenv(d.name);
    int v = d.def;
    if (e && !d.first) v = atoi(e);
    else if (e && e[0] && strchr(d.first, e[0])) v = isdigit((unsigned char)e[0]) ? e[0] - '0' : 1;
    sw.*d.field = v;
  }
  return sw;
}

// ---------------------------------------------------------------------------
// The instances (x3_instances.h) as the host sees them: packed tuple -> forms.
// ---------------------------------------------------------------------------
namespace {
struct Inst {
  bool wr;
  int ks, a, b, c, d, var, occ, forms;
};
const Inst kInstances[] = {
#define X3_F16(KS, A, B, C, D, VAR, OCC, FORMS) {false, KS, A, B, C, D, VAR, OCC, FORMS},
#define X3_WR(KS, WN, DEPTH, FORMS) {true, KS, 0, 0, 0, WN, DEPTH, 0, FORMS},
#include "x3_instances.h"
#undef X3_F16
#undef X3_WR
};
}  // namespace

int x3_instance_forms(const X3Choice& ch) {
  const bool wr = ch.family == X3Choice::WR;
  if (ch.family != X3Choice::F16 && ch.family != X3Choice::FUSED67 && !wr) return 0;
  const int var = wr ? ch.depth : ch.var & ~(X3V_F16 | X3V_A16);
  for (const Inst& i : kInstances)
    if (i.wr == wr && i.ks == ch.ks && i.a == ch.waves_m && i.b == ch.waves_n && i.c == ch.wm && i.d == ch.wn &&
        i.var == var && i.occ == ch.occ)
      return i.forms;
  return 0;
}

bool x3_fits(const ConvLaunch& c) { return c.in_pad >= c.ks / 2; }

bool x3_fused67_fits(int cout6, int cout7) {
  return (cout6 == 128 || cout6 == 256 || cout6 == 512) && cout7 > 0 && cout7 <= 64;
}

// 1x1 layers with 256k output channels and an even number of chunk pairs (Mconv6 of
// every stage: 384/288 -> 512/256) also pack their split filters for 256-channel
// tiles.  On big grids they run 16 waves of 64co x 64px over 256 pixels with two chunk
// pairs per K step (VAR 4096: 24 MFMAs per wave between barriers instead of 12, and
// the input read for half as many channel tiles): +7-12 % (tools/archive/gpu_k1.sh).  Small
// grids (K ranges, the 128-pixel family) keep the 128-channel packing: 256-channel
// tiles there halve the blocks and lost 30 %.
bool x3_wide1_layer(int ks, int cout, int cin_phys) {
  return ks == 1 && cout % 256 == 0 && ((cin_phys / 8 + 1) / 2) % 2 == 0;
}

// fp16 products per MAC a launch executes: three (fp32-accurate), one under ISL_PREC_FP16
static double x3_products(const ConvLaunch& c) { return c.f16 ? 1.0 : 3.0; }

bool x3_rgb_fits(const ConvLaunch& c) {
  return c.ks == 3 && c.cin_chunks == 1 && c.cout <= RGB_BCO && c.in_pad >= 1 && !c.hpool;
}

X3Choice x3_choose_rgb(const ConvLaunch& c) {
  X3Choice ch;
  if (!x3_rgb_fits(c)) {
    ch.error = "conv_x3_rgb: needs a 3x3 layer with one input chunk, <= 64 outputs and rgb-packed weights";
    return ch;
  }
  if (c.act16 && (!c.f16 || c.out32)) {
    ch.error = "conv_x3_rgb: fp16 activation storage needs the one-term form (and is no net output)";
    return ch;
  }
  ch.family = X3Choice::RGB;
  ch.ks = 3;
  ch.bpx = RGB_TILE;
  ch.var = X3V_RGB | (c.f16 ? X3V_F16 : 0) | (c.act16 ? X3V_A16 : 0);
  ch.act16 = c.f16 != 0;
  ch.mfma_flops = x3_products(c) * 2.0 * RGB_BCO * 32.0 * (double)((c.H * c.W + RGB_TILE - 1) / RGB_TILE) * RGB_TILE * c.n;
  ch.code = x3_variant_code(ch.var, 3, ch.bpx, RGB_BCO);
  return ch;
}

double conv_x3_rgb_mfma_flops(const ConvLaunch& c) { return x3_choose_rgb(c).mfma_flops; }

// Tail tiles.  A chip-filling grid of full tiles takes ceil(blocks / CUs) rounds of one block per
// CU, its last round often part-empty (Mode N's 92x164 layers: 1920 blocks, 7.5 rounds -> 8; the
// layer time follows the rounds, tools/round_probe.py).  Where it pays by the estimate below, each
// frame's first full_tiles tiles fill whole rounds and the rest of its pixels run as tail tiles of
// ttpx pixels (a multiple of 128, so that the MFMA-skipping waves past the tile stay spread over
// the SIMDs), dispatched after them.  The plan prices a tail block at 0.3 + 0.7 ttpx / tpx of a
// full one; measured, a 256-pixel tail of the 512-pixel row union costs ~0.85 (its weight slabs,
// staging and barriers stay: profiles/r05/r5tl), so only clear wins are taken (>= 0.25 round by
// the estimate).  Every output keeps its MFMA sequence: same bits.
// ISLPOSE_X3_TAIL=0: one tiling (A/B).
X3Tail x3_tail_plan(int n, int HW, int co_tiles, int px_tiles, int tpx, int nblocks, int cus_, const X3Switches& sw) {
  X3Tail a;
  a.nblocks = nblocks;
  if (!sw.tail) return a;
  const long long cus = cus_, per = (long long)n * co_tiles;
  const long long R0 = (per * px_tiles + cus - 1) / cus;
  const int full_max = HW / tpx;
  const long long Rf = per * full_max / cus;        // whole rounds the full tiles can fill
  if (Rf < 1 || R0 < 2) return a;
  const int F = (int)(Rf * cus / per);
  const long long NF = per * F;
  if (F < 1 || NF % 8) return a;                    // (each class is spread over the 8 XCDs)
  const int rem = HW - F * tpx;
  double best = (double)R0 - 0.25;
  for (int t = 128; t < tpx; t += 128) {
    const int TT = (rem + t - 1) / t;
    const long long NT = per * TT;
    const double est = (double)NF / cus + (double)((NT + cus - 1) / cus) * (0.3 + 0.7 * t / tpx);
    if (est < best && NF + NT <= 0x7fffffff) {
      best = est;
      a.nb_full = (int)NF; a.full_tiles = F; a.tail_tiles = TT; a.ttpx = t;
      a.nblocks = (int)(NF + NT);
    }
  }
  return a;
}

namespace {

// The decision for one launch of the generic kernels.  c is the launch with its K-range count
// (c.ksplit) as launch_conv_x3 sets it; `ws`: the ranges run across blocks.
struct Sel {
  ConvLaunch c;
  const int cus;
  const X3Switches& sw;
  bool ws = false;

  bool small_tiles() const { return sw.tiles_small != 0; }

  // Canonical K ranges of a layer, from its shape alone (never the batch): the small
  // stage layers (<= 1024 pixels per frame: Mode R's 23x41 body stages, the 184 px hand
  // scale) sum their chunk pairs in S ranges, so that a batch-1 frame can spread them
  // over S blocks (split-K) and a large batch can keep them in one block, with the same
  // bits.  Every range is ceil(pairs / S) pairs long and non-empty.
  int canonical_ranges() const {
    // 3x3 / 7x7 layers: ranges of >= 2 chunk pairs; 1x1 layers: >= 4 pairs (64 channels), so
    // that a range of an Mconv7 is one wave's share of the fused pair (VAR 16) and the two
    // executions of the pair give the same bits
    const int pairs = (c.cin_chunks + 1) / 2, per = c.ks == 1 ? 4 : 2;
    if (!c.allow_split || c.H * c.W > 1024 || pairs < 2 * per) return 1;
    int S = std::min(8, pairs / per);
    while (S > 1 && (S - 1) * ((pairs + S - 1) / S) >= pairs) --S;
    return S;
  }

  // Small grids (the 128-pixel family) with 128-channel tiles on two 64-channel blocks of 4
  // waves each (VAR 256): by default the 1x1 / 3x3 layers whose K ranges are split across
  // blocks (grids below one block per CU: batch-1 Mode R, +4 % frames/s), where doubling the
  // grid buys more than the second staging of the input costs; with one block per CU (Mode R
  // batch 32) it loses 10-20 % (profiles/r03/halfco_ab/).  Same bits either way.
  // ISLPOSE_X3_HALFCO (development build only; A/B of profiles/r03/halfco_ab/): =0 off, =1 every
  // 128-channel launch of the family (measured slower at one block per CU, so not in the product).
  bool halfco() const {
    if (c.ks > 7 || c.fold) return false;
    if (c.ks == 7) return c.ksplit > 1 && ws && small7();
    if (sw.halfco == 0) return false;
    if (sw.halfco == 1) return true;
    return c.ks <= 3 && c.ksplit > 1 && ws;
  }

  // Small 7x7 grids (a frame's hand crops per call: one or two crops at the 46^2 - 92^2 hand
  // scales, or the 23^2 scale's across-block K ranges), under one 128-pixel block per CU: the
  // 128-channel tiles run as two 64-channel blocks on 64-pixel tiles (VAR 256, 4 waves of 32co x
  // 32px, two blocks per CU): 4x the blocks, each output the same MFMA sequence (same ranges, same
  // K order), so the same bits as the batched crops.  ISLPOSE_X3_SMALL7=0 off (A/B).
  bool small7() const {
    if (c.ks != 7 || c.bco != 128 || c.fold || c.vin || c.hpool) return false;
    if (sw.small7 == 0) return false;
    const int tpx = tile_pixels(c, 128, x3_segmax(128));
    const long long blocks = (long long)c.n * ((c.H * c.W + tpx - 1) / tpx) * std::max(1, c.ksplit);
    return blocks < cus;
  }
  // ... with the operands two K steps ahead (VAR 128: a ring of three 28 KiB weight slabs, one
  // block per CU) where the 64-pixel grid still fits one block per CU: the 46^2 / 69^2 scales
  // of one crop 55 -> 48 us per layer; past one round (92^2: 266 blocks) the two resident
  // blocks of the plain loop win (profiles/r05/r5s7b/).  ISLPOSE_X3_SMALL7=1: never, 3: always.
  bool small7_deep() const {
    const int m = sw.small7;
    if (m < 2) return false;
    if (m >= 3) return true;
    const int tpx = tile_pixels(c, 64, x3_segmax(64));
    return (long long)c.n * ((c.H * c.W + tpx - 1) / tpx) * 2 * std::max(1, c.ksplit) <= cus;
  }
  // ... on 96-pixel tiles (6 waves of 32co x 32px, two steps ahead) where the 64-pixel grid takes
  // more than one round of one block per CU and the 96-pixel grid takes one: one crop at the
  // 92^2 (736 px) hand scale, 266 -> 178 blocks (the 64-pixel plain loop left 10 CUs with two
  // blocks, every layer waiting on them).  No K range is split: the same bits.
  // ISLPOSE_X3_S7W96=0 off (A/B).
  bool small7_96() const {
    if (!sw.s7w96 || sw.small7 != 2 || c.ksplit > 1) return false;
    const long long HW = (long long)c.H * c.W;
    const int t64 = tile_pixels(c, 64, x3_segmax(64)), t96 = tile_pixels(c, 96, x3_segmax(96));
    return c.n * ((HW + t64 - 1) / t64) * 2 > cus && c.n * ((HW + t96 - 1) / t96) * 2 <= cus;
  }

  // Small grids (the 128-pixel family) with two K groups per block (VAR 32, 16 waves: the first
  // and second half of the canonical K ranges side by side, one block per CU): every 128-channel
  // 1x1 / 3x3 launch whose K ranges run in one block (Mode R's 23x41 stage layers and conv4_x at
  // batch >= 32; 5-6 % faster than the one-group loops there, profiles/r04/r4b/).  The 96-channel
  // form (two groups of 6 waves of 32co x 64px) measured 7 % slower than the deep-prefetch loop on
  // the c96 stage layers and is not built.  The one-group form keeps both halves' sums and the
  // range's in registers (153 VGPRs: one 8-wave block per CU) where two groups hold one each (122:
  // 16 waves per CU).
  // ISLPOSE_X3_G2=0: the one-group loops (A/B).
  bool g2() const {
    if (c.ks > 3 || c.bco != 128 || c.fold || c.vin || c.ksplit < 2 || ws) return false;
    return sw.g2 != 0;
  }

  // Small grids whose K ranges run across blocks (batch-1 Mode R's 23x41 stage layers: 8 pixel
  // tiles x S ranges, far under one block per CU) on 64-pixel tiles: the 96-channel tiles as 6
  // waves of 32co x 32px (not 12 on 128 pixels), the half-channel blocks of the 128-channel tiles
  // (VAR 256) as 4 waves of 32co x 32px (not 4 of 64co x 32px on 128 pixels) -- twice the blocks,
  // each with half the MFMAs and staging per K step.  Each output sees the same MFMA sequence (same
  // ranges, same K order): same bits.  Batch-1 Mode R net 1.955 -> 1.828 ms (profiles/r04/r4ai/).
  // ISLPOSE_X3_PX64=0: the 128-pixel blocks, =1: the 96-channel tiles only (A/B).
  bool px64() const {
    if (c.ks > 3 || c.bco != 96 || c.fold || c.vin || c.ksplit < 2 || !ws) return false;
    return sw.px64 >= 1;
  }

  // Small 3x3 grids without K ranges (batch-1 conv2_x / conv3_x: at most half a block per CU) on
  // half-channel blocks (VAR 256): twice the blocks; same MFMA sequence per output, same bits.
  // Batch-1 Mode R net 1.828 -> 1.817 ms; the 1x1 layers (the two-launch Mconv6) measured slower
  // and the deep-prefetch form level (profiles/r04/r4ai/).  ISLPOSE_X3_HALFSMALL=0 off (A/B).
  bool halfsmall() const {
    if (!sw.halfsmall || c.ks != 3 || c.bco != 128 || c.fold || c.vin || c.ksplit > 1) return false;
    const int tpx = tile_pixels(c, 128, x3_segmax(128));
    const long long blocks = (long long)c.n * ((c.H * c.W + tpx - 1) / tpx) * ((c.cout + c.bco - 1) / c.bco);
    return 2 * blocks <= cus;
  }

  // Small grids (the 128-pixel family) with the inputs and weights prefetched two K steps
  // ahead (VAR 128): by default the 3x3 layers whose grid has at most one block per CU and
  // whose K ranges (if any) run in one block -- Mode R's 23x41 stage layers at batch 32, -5 to
  // -12 % per layer in the net (profiles/r03/deep_ab/).  Its ring of three weight slabs (98 KiB)
  // allows one block per CU, so grids with more blocks lose the second resident block (conv4_x
  // at batch 32: +12-16 %), and the 1x1 layers lost 25-30 %.  ISLPOSE_X3_DEEP=0 off, =1 every
  // 1x1 / 3x3 launch of the family, across-block ranges included (A/B).
  bool deep() const {
    if (c.fold || c.vin || (c.bco != 128 && c.bco != 96) || c.ks > 3) return false;
    if (sw.deep == 0) return false;
    if (sw.deep == 1) return true;
    if (c.ks != 3 || (c.ksplit > 1 && ws)) return false;
    const int tpx = tile_pixels(c, 128, x3_segmax(128));
    const long long blocks = (long long)c.n * ((c.H * c.W + tpx - 1) / tpx) * ((c.cout + c.bco - 1) / c.bco);
    return blocks <= cus;
  }

  // Small grids (the 128-pixel family) with two chunk pairs per K step (VAR 4096): a step's
  // MFMAs double against its barrier and its L2 round trip.  Only for layers with canonical K
  // ranges (they never run the big-tile kernels, whose one-pair order the other layers must
  // keep for batch-invariant bits), an even number of pairs in every range, and one channel
  // tile (c512 lost 7 %).  Per layer (tools/convbench, 23x41 at batch 32) c128 -3 %, c96 -8 %,
  // c384 / c288 -1.5 % time, but the whole of Mode R moved by +-1 % (batch 32 +0.5 %, batch 1
  // -1.2 %, profiles/r03/pps2_ab/), so it is rejected: development build only, ISLPOSE_X3_PPS2=1.
  bool pps2() const {
    // the fold A/B (ISLPOSE_X3_FOLD=1) runs its consumers on one-pair steps, so every layer of a
    // frame keeps one order at every batch size only with PPS2 off there
    if (!sw.pps2 || sw.fold || c.ks > 3 || c.vin || (c.bco != 128 && c.bco != 96) || c.cout > c.bco) return false;
    const int S = canonical_ranges(), pairs = (c.cin_chunks + 1) / 2;
    if (S < 2 || c.ksplit != S) return false;
    const int pps = (pairs + S - 1) / S;
    return pairs % 2 == 0 && pps % 2 == 0;
  }

  // Tile families.  3x3 / 1x1 layers: 512-pixel tiles (16 waves per block, one
  // block per CU): the weight slab of a K step is then shared by 4x the pixels,
  // which cut the L2->LDS bytes per FLOP ~2x and measured +10 % over the 128-pixel
  // tiles (r01); 16 rather than 8 waves for the narrow (96/64/32-channel) tiles
  // +2-9 %.  7x7 layers keep 128-pixel tiles (their slab is 2.3x larger), and so do
  // layers with canonical K ranges (their second accumulator set needs the 128-pixel
  // family's register budget).  512-pixel tiles are used only when they fill the
  // chip: a layer with fewer such blocks than CUs runs ~2x faster on the 128-pixel,
  // 4-wave family (tools/archive/gpu_tiles.sh).  ISLPOSE_X3_TILES=s: never (A/B).

  // 64-channel 3x3 layers off the row union (full-resolution conv1_2 / hand conv1_2: 12 K
  // steps) run 256-pixel blocks of 8 waves (64co x 32px each), two blocks per CU, so that one
  // block's prologue and epilogue overlap the other's K loop: -4 to -5 % against the 16-wave
  // 512-pixel block (tools/archive/gpu_mid.sh; the 128-channel layers stay on 512 pixels, where every
  // 256-pixel shape lost 4-7 %).  ISLPOSE_X3_HALF64=0: the 512-pixel block (A/B).
  bool half64() const { return sw.half64 && c.ks == 3 && c.bco == 64 && !row_union(); }

  int big_bpx() const { return (c.ks == 1 && c.bco == 256) || half64() ? 256 : 512; }

  bool big_tiles() const {
    if (c.ks > 3 || small_tiles() || canonical_ranges() > 1) return false;
    const int bpx = big_bpx(), tpx = tile_pixels(c, bpx, x3_segmax(bpx));
    const long long px_tiles = (c.H * c.W + tpx - 1) / tpx;
    return (long long)c.n * px_tiles * ((c.cout + c.bco - 1) / c.bco) >= cus;
  }

  // pixels per 7x7 tile (128, 256 or 384), chosen per launch by grid quantisation: rounds
  // of one block per CU, a round of 256- / 384-pixel blocks costing X3_WIDE7_COST /
  // X3_W384_COST of a 128-pixel round.  ISLPOSE_X3_WIDE7=0|1|3 forces 128 / 256 / 384 (A/B).
  int bpx_7x7() const {
    if (c.ks != 7 || c.bco != 128 || small_tiles() || canonical_ranges() > 1) return 128;
    const int mode = sw.wide7;
    if (mode != 2) return mode == 1 ? 256 : mode == 3 ? 384 : 128;
    const long long HW = (long long)c.H * c.W, co = (c.cout + 127) / 128;
    int best = 128;
    double best_t = 0.0;
    for (int bpx : {128, 256, 384}) {
      const int t = tile_pixels(c, bpx, x3_segmax(bpx));
      const long long b = c.n * ((HW + t - 1) / t) * co;
      const double cost = bpx == 128 ? 1.0 : bpx == 256 ? X3_WIDE7_COST : X3_W384_COST;
      const double tt = (double)((b + cus - 1) / cus) * cost;
      if (bpx == 128 || tt < best_t) { best = bpx; best_t = tt; }
    }
    return best;
  }

  // Row-union staging (VAR 512) when the longest union run of any 512-pixel tile fits.
  // longest row-union run (pixels) over the 512-pixel tiles of a layer
  int union_run() const {
    const int P = c.ks / 2, Wi = c.W + 2 * c.in_pad, HW = c.H * c.W;
    const int tpx = tile_pixels(c, 512, x3_segmax(512));
    int span = 0;
    for (int m0 = 0; m0 < HW; m0 += tpx) {
      const int ml = std::min(m0 + tpx, HW) - 1;
      span = std::max(span, (ml / c.W - m0 / c.W) * Wi + (ml % c.W - m0 % c.W));
    }
    return span + 2 * P * Wi + 2 * P + 1;
  }

  // ISLPOSE_X3_UNION: 0: no row union (A/B), 1: row union (default), 4: row union with s_memtime
  // stamps (development; needs ConvLaunch::dbg, set only by tools/convbench)
  bool row_union() const {
    if (sw.union_mode == 0 || c.ks != 3 || small_tiles() || canonical_ranges() > 1) return false;
    return union_run() <= x3_segu_max();
  }

  // The row union on v_mfma_f32_16x16x32_f16 (VAR 131072) for 128-channel tiles with an even
  // number of chunk pairs: rejected (profiles/r03/m16_ab/), development build only,
  // ISLPOSE_X3_M16=1.
  bool m16() const { return sw.m16 && c.ks == 3 && c.bco == 128 && ((c.cin_chunks + 1) / 2) % 2 == 0; }

  // K-range plan of a launch on the 128-pixel family: S ranges, computed across S blocks
  // per tile (split-K, partials through the workspace) when the plain grid has fewer
  // blocks than CUs, else in one block (tools/archive/gpu_across.sh: across wins 10-50 % at
  // 64-160 blocks, in-block wins 20-70 % at 256-1024 -- same bits either way;
  // ISLPOSE_X3_ACROSS=0|1 forces it, A/B).  With isl_net_set_split_k(net, 2) (latency
  // mode) layers without canonical ranges also split when their grid is that small --
  // an adaptive S that depends on the batch, so those layers' bits then do too.
  void ranges(int* S_, bool* across_) const {
    *S_ = 1;
    *across_ = false;
    if (big_tiles() || bpx_7x7() != 128) return;
    const int tpx = tile_pixels(c, 128, x3_segmax(128));
    const long long blocks = (long long)c.n * ((c.H * c.W + tpx - 1) / tpx) * ((c.cout + c.bco - 1) / c.bco);
    const int pairs = (c.cin_chunks + 1) / 2;
    *S_ = canonical_ranges();
    if (*S_ > 1) {
      *across_ = sw.across >= 0 ? sw.across == 1 : blocks < cus;
      return;
    }
    if (c.allow_split == 2 && 2 * blocks <= cus && pairs >= 4) {
      int S = (int)std::min<long long>({8, pairs / 2, (cus + blocks - 1) / blocks});
      while (S > 1 && (S - 1) * ((pairs + S - 1) / S) >= pairs) --S;
      *S_ = S;
      *across_ = S > 1;
    }
  }

  // The conv_x3_f16 instance of the launch (VAR without its form bits); false: no variant
  bool pick(X3Choice& ch) const {
    const int KS = c.ks;
    const bool big = big_tiles();
    auto set = [&](int a, int b, int wm, int wn, int var, int occ) {
      ch.waves_m = a; ch.waves_n = b; ch.wm = wm; ch.wn = wn; ch.var = var; ch.occ = occ;
      return true;
    };
    if (KS == 3 && big && row_union()) {
#ifdef ISLPOSE_DEV
      if (sw.union_mode == 4 && c.dbg) {   // development build only (tools/convbench)
        if (c.bco == 128) return set(2, 8, 2, 2, 512 | 16384, 4);
        if (c.bco == 96) return set(1, 16, 3, 1, 512 | 16384, 4);
      }
      if (!c.f16 && c.bco == 128 && m16()) return set(2, 8, 2, 2, 512 | 131072 | (c.vin ? 32768 : 0), 4);   // (three-term only)
#endif
      if (c.vin) {
        if (c.bco == 128) return set(2, 8, 2, 2, 512 | 32768, 4);
        ch.error = "conv_x3: pooled-input staging without a variant (x3_vin_ok)";
        return false;
      }
      switch (c.bco) {
        case 128: return set(2, 8, 2, 2, 512, 4);
        case 96: return set(1, 16, 3, 1, 512, 4);
        case 64: return set(2, 8, 1, 2, 512, 4);
        case 32: return set(1, 16, 1, 1, 512, 4);
      }
    }
    if (KS == 1 && c.bco == 256 && big) return set(4, 4, 2, 2, 4096, 1);
    if (KS <= 3 && big) {
      if (KS == 3 && c.vin) {
        if (c.bco == 128) return set(2, 8, 2, 2, 32768, 4);
        if (half64()) return set(1, 8, 2, 1, 32768, 2);
      }
      if (c.vin) {
        ch.error = "conv_x3: pooled-input staging without a variant (x3_vin_ok)";
        return false;
      }
      if (half64()) return set(1, 8, 2, 1, 0, 2);   // 8 waves of 64co x 32px, 256 px
      switch (c.bco) {
        case 128: return set(2, 8, 2, 2, 0, 4);   // 16 waves, 64co x 64px each
        case 96: return set(1, 16, 3, 1, 0, 4);   // 16 waves, 96co x 32px
        case 64: return set(2, 8, 1, 2, 0, 4);    // 16 waves, 32co x 64px
        case 32: return set(1, 16, 1, 1, 0, 4);   // 16 waves, 32co x 32px
      }
    }
    // 128-channel 7x7 tiles without K ranges: 8 waves of 64co x 64px on 256 pixels, or
    // of 64co x 32px on 128 pixels (one block per CU either way: the 56 KiB weight
    // slabs; 8 waves measured 2-6 % over 4 waves of 64co x 64px / x 128px)
    if (KS == 7 && c.ksplit <= 1 && c.bco == 128) {
      if (small7()) {   // 64co x 64px blocks (=2: the steps' operands two steps ahead)
        if (small7_96()) return set(2, 3, 1, 1, 256 | 128, 1);
        if (small7_deep()) return set(2, 2, 1, 1, 256 | 128, 1);
        return set(2, 2, 1, 1, 256, 4);
      }
      const int bpx = bpx_7x7();
      if (bpx == 384) return set(2, 6, 2, 2, 65536, 1);   // 12 waves, 384 px, one input buffer
      if (bpx == 256) return set(2, 4, 2, 2, 0, 1);
      return set(2, 4, 2, 1, 0, 1);
    }
    const bool ranged = c.ksplit > 1 && !ws;      // in-block ranges
    const bool split = c.ksplit > 1 && ws;        // across blocks
    const int kr = split ? 2048 : ranged ? 1024 : 0;
    // 128- / 96-channel tiles of the 128-pixel family: 8 waves of 64co x 32px / 12 waves of
    // 32co x 32px rather than 4 waves of 64co x 64px / 96co x 32px.  These grids are small
    // (Mode R's 23x41 stages: one block per CU at batch 32), and two or three waves per
    // SIMD hide the staging: -8 to -22 % on the 23x41 3x3 stage layers, -12 to -31 % on
    // their 1x1 layers, -5 to -14 % on the hand's 23^2 7x7 layers, -20 % on its 23^2 c512
    // layers (tools/archive/gpu_s8.sh, gpu_s8b.sh).  ISLPOSE_X3_S8=0: the 4-wave layouts (A/B).
    if (sw.s8) {
#ifdef ISLPOSE_DEV
      if (KS <= 3 && c.fold) {   // consumers of folded split-K partials (x3_fold_ok)
        if (c.bco == 128) return set(2, 4, 2, 1, kr | 8192, 2);
        if (c.bco == 96) return set(3, 4, 1, 1, kr | 8192, 2);
        ch.error = "conv_x3: fold without a variant (x3_fold_ok)";
        return false;
      }
#else
      if (c.fold) {
        ch.error = "conv_x3: the split-K fold is a development-build variant";
        return false;
      }
#endif
      if (KS <= 3 && g2()) return set(2, 4, 2, 1, 1024 | 32, 1);   // two K groups of 8 waves
      if (KS <= 3 && !split && !ranged && halfsmall()) return set(1, 4, 2, 1, 256, 4);
      if (KS <= 3 && deep()) {   // prefetch two K steps ahead
        if (c.bco == 128) return set(2, 4, 2, 1, kr | 128, 1);
        if (c.bco == 96) return set(3, 4, 1, 1, kr | 128, 1);
      }
#ifdef ISLPOSE_DEV
      if (KS <= 3 && pps2()) {   // two chunk pairs per K step: twice the MFMAs between barriers
        if (c.bco == 128) return set(2, 4, 2, 1, kr | 4096, 2);
        if (c.bco == 96) return set(3, 4, 1, 1, kr | 4096, 2);
      }
#endif
      if (c.bco == 128 && halfco()) {   // two blocks of 4 waves (64co x 32px) per 128-channel tile
        if (KS == 7 && split && small7_deep()) return set(2, 2, 1, 1, 2048 | 256 | 128, 1);
        if (split && sw.px64 >= 2) return set(2, 2, 1, 1, 2048 | 256, 4);
        if (split) return set(1, 4, 2, 1, 2048 | 256, 4);
#ifdef ISLPOSE_DEV
        if (ranged) return set(1, 4, 2, 1, 1024 | 256, 4);
#endif
        if (!ranged) return set(1, 4, 2, 1, 256, 4);
      }
      if (c.bco == 128) return set(2, 4, 2, 1, kr, 2);   // 8 waves of 64co x 32px
      if (c.bco == 96) {                                  // 12 waves of 32co x 32px (6 on 64-pixel tiles: px64)
        if (split && px64()) return set(3, 2, 1, 1, 2048, 4);
        return set(3, 4, 1, 1, kr, 2);
      }
    }
    switch (c.bco) {
      case 128: return set(2, 2, 2, 2, kr, 2);
      case 96: return set(1, 4, 3, 1, kr, 2);
      case 64: return set(1, 4, 2, 1, kr, 2);
      case 32: return set(1, 4, 1, 1, kr, 2);
    }
    ch.error = "conv_x3: unsupported tile";
    return false;
  }
};

}  // namespace

X3Choice x3_choose(const ConvLaunch& c0, int cus, const X3Switches& sw) {
  X3Choice ch;
  ch.ks = c0.ks;
  const int fv = c0.act16 ? X3V_F16 | X3V_A16 : c0.f16 ? X3V_F16 : 0;
  // (fp16 storage is planned per run: never with the fold, nor -- the fused pair apart -- under the
  // A/B mode that runs the other small grids on the wave-range kernel)
  const bool a16_pair = c0.f16 && !c0.fold && !c0.fold_out, a16_run = a16_pair && sw.wr != 2;
  auto none = [&](const char* why) {
    ch = X3Choice();
    ch.ks = c0.ks;
    ch.error = why;
    return ch;
  };
  if (!x3_fits(c0)) return none("conv_x3: input ring narrower than kernel radius");
  Sel s{c0, cus, sw};
  ConvLaunch& c = s.c;
  if (c.cout7 > 0) {
    // The fused 1x1 pair, one tile of every Mconv6 channel: 16 waves of 64co x 64px, 8 x 2
    // (512 channels, 128 pixels), 4 x 4 (256, 256) or 2 x 8 (128, 512).  No K ranges: the pair
    // always runs fused, at every batch size, so a frame's bits do not depend on its batch.
    // (two chunk pairs per K step with one input buffer, VAR 4096 | 65536, measured level with
    // this loop in Mode N and Mode R, profiles/r04/r4c/ops_*_pps1.txt: not built)
    if (c.ks != 1 || !x3_fused67_fits(c.cout, c.cout7)) return none("conv_x3: fused 1x1 pair outside its shapes");
    ch.family = X3Choice::FUSED67;
    ch.waves_m = c.cout / 64; ch.waves_n = 16 / ch.waves_m; ch.wm = ch.wn = 2; ch.occ = 4;
    ch.var = 16 | fv;
    ch.bpx = ch.waves_n * 64;
    const double px = std::ceil((double)c.H * c.W / tile_pixels(c, ch.bpx, x3_segmax(ch.bpx))) * ch.bpx * c.n;
    const double k6 = ((c.cin_chunks + 1) / 2) * 16.0;
    ch.mfma_flops = x3_products(c) * 2.0 * px * ((double)c.cout * k6 + 32.0 * ((c.cout7 + 31) / 32) * c.cout);
    // (the 512-channel tile does not fit the 4-bit tile field: it records cout / 2, decode_variant
    // doubles it back for VAR 16)
    ch.code = x3_variant_code(ch.var, 1, ch.bpx, c.cout / 2);
    ch.act16 = a16_pair && !c.hpool && !c.vin && (x3_instance_forms(ch) & 4);
    return ch;
  }
  if (c.ks != 1 && c.ks != 3 && c.ks != 7) return none("conv_x3: unsupported kernel size");
  s.ranges(&ch.S, &ch.across_blocks);
  c.ksplit = ch.S;
  // the tile the FLOP count assumes: the family's nominal one
  const int nominal = s.big_tiles() ? s.big_bpx() : s.bpx_7x7();
  const double co = (double)((c.cout + c.bco - 1) / c.bco) * c.bco;
  const double px = std::ceil((double)c.H * c.W / tile_pixels(c, nominal, x3_segmax(nominal))) * nominal;
  ch.mfma_flops = x3_products(c) * 2.0 * co * (((c.cin_chunks + 1) / 2) * 16.0) * c.ks * c.ks * px * c.n;
  // conv_x3_wr for the launches whose K ranges would run across blocks, by default those with at
  // most 4 ranges of a 1x1 / 3x3 layer: with 8 a block's 8 waves load 2x the operand bytes per CU
  // of the split-K blocks (no sharing between ranges), and in the net the c384 / c288 stage layers
  // ran 20-35 % slower on it (profiles/r05/r5c/ops_*.txt); a 7x7 range is 98 taps long for one
  // wave (the hand's 184-pixel scale: C3 109.4 -> 107.5 frames/s on it, profiles/r05/r5n/).
  // ISLPOSE_X3_WR=0: the split-K launches + x3_splitk_reduce (A/B), =2: also the small grids
  // without K ranges (one wave per block summing the whole K; A/B), =3: every range count;
  // ISLPOSE_X3_WR_WN=2: 64-pixel tiles (two 32-pixel accumulator tiles per wave sharing the weight
  // fragments).
  const bool wr_ranges = ch.across_blocks && !c.fold_out && (sw.wr >= 3 || (sw.wr >= 1 && ch.S <= 4 && c.ks <= 3));
  const bool wr_plain = sw.wr == 2 && ch.S == 1 && c.ks <= 3 && !c.hpool && !c.vin && !c.fold && !s.big_tiles() &&
                        s.bpx_7x7() == 128;
  if (wr_ranges || wr_plain) {
    ch.family = X3Choice::WR;
    if (wr_plain && !wr_ranges) ch.S = 1;
    ch.wn = sw.wr_wn == 2 ? 2 : 1;
    ch.depth = sw.wr_wn == 2 ? 8 : 12;
    ch.bpx = 32 * ch.wn;
    ch.var = 8 | (ch.S > 1 ? 1024 : 0) | (c.f16 ? X3V_F16 : 0);
    ch.code = x3_variant_code(ch.var, c.ks, ch.bpx, 32);
    return ch;
  }
  s.ws = ch.across_blocks;
  if (!s.pick(ch)) return none(ch.error);
  if (c.vin && !(ch.var & 32768)) return none("conv_x3: pooled-input staging without a variant (x3_vin_ok)");
  ch.family = X3Choice::F16;
  ch.var |= fv;
  const int bco = ch.waves_m * ch.wm * 32;
  ch.bpx = ch.waves_n * ch.wn * 32;
  if (ch.across_blocks) ch.ws_floats = (size_t)ch.S * c.n * ((c.cout + 7) / 8) * 8 * c.H * c.W;
  ch.code = x3_variant_code(ch.var, c.ks, ch.bpx, bco);
  ch.act16 = a16_run && (x3_instance_forms(ch) & 4);
  return ch;
}

// Launches with a pooled-input variant (VAR 32768): 3x3 layers on the 512-pixel family
// with 128-channel tiles (row union or generic) or the 256-pixel 64-channel blocks -- the
// layers after the body's and hand's pools at batch sizes that fill the chip.  Others
// take vpool2_kernel + the plain variant.
bool x3_vin_ok(const ConvLaunch& c, int cus, const X3Switches& sw) {
  ConvLaunch v = c;
  v.vin = 1;
  return c.in_coff == 0 && (long long)(c.H + 2 * c.in_pad) * (c.W + 2 * c.in_pad) < (1 << 20) &&
         x3_choose(v, cus, sw).family == X3Choice::F16;
}

bool x3_hpool_ok(const ConvLaunch& c, int cus, const X3Switches& sw) {
  return x3_fits(c) && !(c.W & 1) && !x3_choose(c, cus, sw).across_blocks;
}

bool x3_wide1(const ConvLaunch& c, int cus, const X3Switches& sw) {
  return c.bco == 256 && x3_wide1_layer(c.ks, c.cout, c.cin_chunks * 8) && (x3_choose(c, cus, sw).var & 4096);
}

bool x3_act16_ok(const ConvLaunch& c, int cus, const X3Switches& sw) { return x3_choose(c, cus, sw).act16; }

double conv_x3_mfma_flops(const ConvLaunch& c, int cus, const X3Switches& sw) { return x3_choose(c, cus, sw).mfma_flops; }

double conv_x3_fused67_mfma_flops(const ConvLaunch& c, int cus, const X3Switches& sw) {
  return x3_choose(c, cus, sw).mfma_flops;
}

int x3_split_ranges(const ConvLaunch& c, bool* across_blocks, int cus, const X3Switches& sw) {
  const X3Choice ch = x3_choose(c, cus, sw);
  if (across_blocks) *across_blocks = ch.across_blocks;
  return ch.S;
}

size_t x3_splitk_ws_floats(const ConvLaunch& c, int cus, const X3Switches& sw) { return x3_choose(c, cus, sw).ws_floats; }

bool x3_fold_ok(const ConvLaunch& c, int cus, const X3Switches& sw) {
  const Sel s{c, cus, sw};
  return sw.s8 && x3_fits(c) && c.ks <= 3 && !c.vin && !c.hpool && (c.bco == 128 || c.bco == 96) && !s.big_tiles() &&
         (long long)(c.H + 2 * c.in_pad) * (c.W + 2 * c.in_pad) < (1 << 20);
}

// The pair runs fused where its grid has at least half a block per CU; smaller grids (batch-1
// Mode R: 8 pixel tiles) take the two launches (Mconv6 then Mconv7 with its K ranges split
// across blocks), whose bits are the fused kernel's (the runtime's permuted Mconv6 output order,
// pack_x3 with the Mconv7 channel map; x3_canonical_order over the waves).
bool x3_fused67_grid(const ConvLaunch& c, int cus) {
  const int bpx = c.cout == 512 ? 128 : c.cout == 256 ? 256 : 512;
  const int tpx = tile_pixels(c, bpx, x3_segmax(bpx));
  return 2 * ((long long)c.n * ((c.H * c.W + tpx - 1) / tpx)) >= cus;
}

}  // namespace isl
