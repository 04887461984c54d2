// The host-side decisions of the post-processing (post_plan.h): host-only.  The switches, the
// plans of the body and hand posts and their scratch layouts.
#include "post_plan.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace isl {

// ---------------------------------------------------------------------------
// The switches (A/B and tests; every one is read per call).  On unless set to 0:
//   ISLPOSE_FUSED_BLUR   the resize inside the blur where the plan allows it
//   ISLPOSE_BLUR_LIST    a live-tile list for the blur; 0: the band-maxima early out inside
//                        every tile's block
//   ISLPOSE_BLUR_BANDS   single scale, materialised planes: the band maxima of the final resize
//                        (blur early out)
//   ISLPOSE_RESIZE_SKIP  two-stage frames: stage-2 tiles that no live window reads are skipped
//                        (stage2_need_kernel), which takes the band-maxima V4 form of both stages
//   ISLPOSE_RESIZE_V4    the four-column vertical pass of the resize; 0: the one-column pass
//                        everywhere
//   ISLPOSE_LIMB_SPLIT   the pair scoring over Z blocks per limb; 0: one block per limb
//   ISLPOSE_LIMB_LDS     large pair sets ranked and matched in LDS; 0: the per-thread pair loop
//   ISLPOSE_ASM_REG      the assembly's merge in registers; 0: the table merge only
// ISLPOSE_BLUR_EXACT=1: every live tile on the fp64 passes, without the fp32 filter; =2: the
// filter with a margin so wide that nearly every live tile falls back (the same mask bits either
// way).  ISLPOSE_LIMB_Z=z: z blocks per limb, 1..64.
// Development build only, off unless set to 1:
//   ISLPOSE_FUSED_WIDE   two-stage frames whose stage-2 scale needs the wide LDS window (Mode R
//                        at 368 x 656) resize on the fly in blur_nms too.  Measured slower than
//                        materialising the planes (Mode R batch-32 post 1.54 -> 1.61 ms, batch 1
//                        0.19 -> 0.22 ms, profiles/r03/wide/): two 72 KB blocks per CU and a
//                        28-row horizontal pass per tile cost more than the 0.8 GB write and re-read
//   ISLPOSE_TILE_PROF    the blur launches stamp their tiles (isl_dev_tile_prof)
//   ISLPOSE_ASM_PROF     assemble_kernel stamps its phases per frame (isl_dev_asm_prof)
// ---------------------------------------------------------------------------
static const PostSwitchDef kSwitches[] = {
    {"ISLPOSE_FUSED_BLUR", &PostSwitches::fused_blur, 1, "0", 0, 0},
    {"ISLPOSE_BLUR_LIST", &PostSwitches::blur_list, 1, "0", 0, 0},
    {"ISLPOSE_BLUR_BANDS", &PostSwitches::blur_bands, 1, "0", 0, 0},
    {"ISLPOSE_BLUR_EXACT", &PostSwitches::blur_exact, 0, "12", 0, 0},
    {"ISLPOSE_RESIZE_SKIP", &PostSwitches::resize_skip, 1, "0", 0, 0},
    {"ISLPOSE_RESIZE_V4", &PostSwitches::resize_v4, 1, "0", 0, 0},
    {"ISLPOSE_LIMB_SPLIT", &PostSwitches::limb_split, 1, "0", 0, 0},
    {"ISLPOSE_LIMB_Z", &PostSwitches::limb_z, 0, nullptr, 1, 64},
    {"ISLPOSE_LIMB_LDS", &PostSwitches::limb_lds, 1, "0", 0, 0},
    {"ISLPOSE_ASM_REG", &PostSwitches::asm_reg, 1, "0", 0, 0},
#ifdef ISLPOSE_DEV
    {"ISLPOSE_FUSED_WIDE", &PostSwitches::fused_wide, 0, "1", 0, 0},
    {"ISLPOSE_TILE_PROF", &PostSwitches::tile_prof, 0, "1", 0, 0},
    {"ISLPOSE_ASM_PROF", &PostSwitches::asm_prof, 0, "1", 0, 0},
#endif
};

const PostSwitchDef* post_switch_table(int* count) {
  *count = (int)(sizeof(kSwitches) / sizeof(kSwitches[0]));
  return kSwitches;
}

PostSwitches post_switches() {
  PostSwitches sw{};
  for (const PostSwitchDef& d : kSwitches) {
    const char* e = getenv(d.name);
    int v = d.def;
    if (e && !d.first) v = std::max(d.lo, std::min(d.hi, atoi(e)));
    else if (e && e[0] && strchr(d.first, e[0])) v = e[0] - '0';
    sw.*d.field = v;
  }
  return sw;
}

// ---------------------------------------------------------------------------
// The plans
// ---------------------------------------------------------------------------
int fit_rows(int ty, double scy, bool identity) {
  if (!identity)
    while (ty > 1 && (ty - 1) * scy + 5.0 > (double)RS_MAXR) --ty;
  return ty;
}
int resize_rows(double scy, bool identity) { return fit_rows(RS_TY, scy, identity); }

isl_resize_plan resize_form(double scy, bool identity, int ow, int mode, bool want_bm, const PostSwitches& sw) {
  isl_resize_plan f{};
  f.launched = 1;
  f.identity = identity;
  f.ty = resize_rows(scy, identity);
  const bool v4 = mode == 1 && !identity && ow % 4 == 0 && f.ty % 4 == 0 && sw.resize_v4;
  f.bm = want_bm && mode == 1 && f.ty % BM_ROWS == 0;
  f.v4 = f.bm ? v4 && f.ty == 4 * BM_ROWS : v4;
  // 128-column blocks unless 256 pads less (it never does); the BM and V4 forms are 128 wide
  f.cols = f.bm || f.v4 || (ow + 127) / 128 * 128 <= (ow + RS_TX - 1) / RS_TX * RS_TX ? 128 : RS_TX;
  return f;
}

bool plan_geom_ok(int nscales, const isl_scale_geom* geom) {
  if (nscales <= 0 || nscales > MAX_SCALES || !geom) return false;
  for (int si = 0; si < nscales; ++si)
    if (geom[si].net_h < 8 || geom[si].net_w < 8 || geom[si].valid_h < 1 || geom[si].valid_w < 1) return false;
  return true;
}

void body_post_plan(int kind, int n, int H, int W, int nscales, const isl_scale_geom* geom, const PostSwitches& sw,
                    isl_body_post_plan* p) {
  memset(p, 0, sizeof(*p));
  const int nlimbs = kind == ISL_BODY25 ? 24 : 19;
  const isl_scale_geom& g0 = geom[0];
  const bool multi = nscales > 1;
  // single scale with the net input at frame size (one x8 resize): fuse resize + blur,
  // no full-resolution heat planes
  // single scale, two stages (Mode R on large frames: 184 x 327 -> 1080 x 1920): the
  // second resize is a strong upsampling whose full-resolution planes cost more HBM
  // traffic than the on-the-fly resize; fused too when a blur tile's source window fits
  // the LDS window (~1/5.2 and below; at 368 x 656, scale 1/2, it does not)
  // (the wide window takes stage-2 scales down to ~1/2: Mode R at 368 x 656)
  auto window_fits = [&](int rows, int cols) {
    return 41.0 * g0.valid_h / H + 6.0 <= rows && 217.0 * g0.valid_w / W + 6.0 <= cols;
  };
  const bool two = !multi && !(g0.valid_h == H && g0.valid_w == W);
  const bool fuse2_small = two && window_fits(NMS_SRC_ROWS, NMS_SRC_COLS);
  p->env_fused_wide = sw.fused_wide;
  p->env_fused_blur = sw.fused_blur;
  const bool fuse2 = two && (fuse2_small || (window_fits(NMS_WSRC_ROWS, NMS_WSRC_COLS) && p->env_fused_wide));
  const bool fused = !multi && (!two || fuse2) && p->env_fused_blur;
  p->multi = multi;
  p->two_stage = two;
  p->fuse2 = fuse2;
  p->wide = fuse2 && !fuse2_small;
  p->fused = fused;
  p->env_blur_list = sw.blur_list;
  p->env_blur_bands = sw.blur_bands;
  const bool bands = !fused && !multi && p->env_blur_bands;
  p->env_resize_skip = sw.resize_skip;
  p->env_resize_v4 = sw.resize_v4;
  p->env_blur_exact = sw.blur_exact;
  p->env_limb_lds = sw.limb_lds;
  p->env_asm_reg = sw.asm_reg;
  const double scy2 = 1.0 / ((double)H / g0.valid_h);
  const isl_resize_plan s1bm = resize_form(1.0 / 8.0, false, g0.valid_w, 1, true, sw);
  const isl_resize_plan s2bm = resize_form(scy2, false, W, 1, true, sw);
  p->skip2 = !fused && !multi && two && bands && p->env_blur_list && p->env_resize_skip && s1bm.bm && s1bm.v4 &&
             s2bm.bm && s2bm.v4;
  p->stage2_ty = resize_rows(scy2, false);
  int acc_ty = RA_TY;
  for (int si = 0; si < nscales; ++si) {
    const isl_scale_geom& g = geom[si];
    const bool two_stage = !(g.valid_h == H && g.valid_w == W);
    p->scale_two_stage[si] = two_stage;
    // stage 1: cv2.resize(fx=fy=8); stage 2: cv2.resize(crop, (W, H)), scale = 1 / (H / valid_h)
    if (two_stage) p->stage1[si] = resize_form(1.0 / 8.0, false, g.valid_w, 1, p->skip2, sw);
    const double scy = two_stage ? 1.0 / ((double)H / g.valid_h) : 1.0 / 8.0;
    if (multi) acc_ty = fit_rows(acc_ty, scy, false);   // every scale's final resize, one fp64 pass
    else if (!fused) p->final_rs[si] = resize_form(scy, false, W, 1, bands, sw);
  }
  p->acc_ty = multi ? acc_ty : 0;
  if (multi) p->blur = ISL_BLUR_MULTI_F64;
  else if (fused) p->blur = ISL_BLUR_FUSED_LIVE;
  else if (p->final_rs[0].bm && p->env_blur_list) p->blur = ISL_BLUR_BAND_LIVE;
  else p->blur = ISL_BLUR_DENSE;
  p->blur_bandmax = p->blur == ISL_BLUR_DENSE && p->final_rs[0].bm;
  // a frame per call: the scoring over Z blocks per limb (MODE 1), then ranks and matches (MODE 2).
  // A 1080p frame's scoring: 10 / 32 / 64 blocks per limb 70.7 / 34.5 / 40.5 us
  // (profiles/r06/lk/lz/); each pair is scored whole by one block, so the slicing changes no sum
  p->limb_z = !sw.limb_split || n * nlimbs >= 128 ? 1
              : sw.limb_z ? sw.limb_z : std::max(1, std::min(32, 1024 / (n * nlimbs)));
}

void hand_post_plan(int h, int w, int nscales, const isl_scale_geom* geom, const PostSwitches& sw,
                    isl_hand_post_plan* p) {
  memset(p, 0, sizeof(*p));
  int ty = RA_TY;
  for (int si = 0; si < nscales; ++si) {
    const isl_scale_geom& g = geom[si];
    const bool two_stage = !(g.valid_h == h && g.valid_w == w);
    p->two_stage[si] = two_stage;
    p->identity[si] = 0;   // both the x8 and the stage-2 source are interpolated
    if (two_stage) p->stage1[si] = resize_form(1.0 / 8.0, false, g.valid_w, 1, false, sw);
    // rows per tile: every scale's source window fits the LDS rows
    ty = fit_rows(ty, two_stage ? 1.0 / ((double)h / g.valid_h) : 1.0 / 8.0, p->identity[si]);
  }
  p->acc_ty = ty;
  p->cc_lds = (long long)h * w <= CC_LDS_MAX;
  p->cc_rows = std::max(1, CC_CHUNK / w);
  p->cc_chunks = (h + p->cc_rows - 1) / p->cc_rows;
}

// ---------------------------------------------------------------------------
// The scratch layouts
// ---------------------------------------------------------------------------
namespace {
// lays the regions out in the order of the calls
struct Carve {
  size_t at = 0;
  void operator()(PostRegion& r, size_t bytes) {
    r.off = at;
    r.bytes = bytes;
    at += r.padded();
  }
};
// the stage-1 planes of every scale whose valid size is not the output's
size_t mid_bytes(int n, int nparts, int h, int w, int nscales, const isl_scale_geom* geom) {
  size_t b = 0;
  for (int si = 0; si < nscales; ++si)
    if (!(geom[si].valid_h == h && geom[si].valid_w == w))
      b += (size_t)n * geom[si].valid_h * geom[si].valid_w * nparts * 4;
  return b;
}
size_t blur_tiles(int n, int nparts, int h, int w) {
  return (size_t)((w + NMS_TX - 1) / NMS_TX) * ((h + NMS_TY - 1) / NMS_TY) * n * nparts;
}
}  // namespace

BodyPostLayout body_post_layout(const isl_body_post_plan& plan, int kind, int n, int H, int W, int nscales,
                                const isl_scale_geom* geom, const isl_caps& caps) {
  const int nparts = kind == ISL_BODY25 ? 25 : 18, nlimbs = kind == ISL_BODY25 ? 24 : 19;
  const int words = (W + 63) / 64;
  const bool skip2 = plan.skip2;
  BodyPostLayout l{};
  l.n_tiles = blur_tiles(n, nparts, H, W);
  // The band maxima are sized by the switch, as they always were: also where the final resize
  // cannot write them (its rows per tile no multiple of BM_ROWS), and the live list with them.
  const bool bands = !plan.fused && !plan.multi && plan.env_blur_bands;
  const bool live = plan.fused || (bands && plan.env_blur_list);
  const isl_scale_geom& g0 = geom[0];
  const int ty2 = plan.stage2_ty, ry_tiles = (H + ty2 - 1) / ty2, rx_tiles = (W + 127) / 128;
  Carve carve;
  carve(l.heat, plan.fused ? 0 : (size_t)n * nparts * H * W * (plan.multi ? 8 : 4));
  carve(l.mid, mid_bytes(n, nparts, H, W, nscales, geom));
  carve(l.mask, (size_t)n * nparts * H * words * 8);
  carve(l.pairs, (size_t)n * nlimbs * caps.max_pairs * (8 + 4 + 4));
  carve(l.used, (size_t)n * nlimbs * 2 * caps.max_peaks);
  carve(l.live, live ? (l.n_tiles + 1) * sizeof(int) : 0);
  carve(l.bandmax, bands ? (size_t)n * nparts * ((H + BM_ROWS - 1) / BM_ROWS) * words * 4 : 0);
  carve(l.amb, (l.n_tiles + 1) * sizeof(int));
  carve(l.bm1, skip2 ? (size_t)n * nparts * ((g0.valid_h + BM_ROWS - 1) / BM_ROWS) * ((g0.valid_w + 63) / 64) * 4 : 0);
  carve(l.live_mid, skip2 ? l.n_tiles : 0);
  carve(l.need, skip2 ? (size_t)n * nparts * ry_tiles * rx_tiles : 0);
  l.total = carve.at;
  return l;
}

HandPostLayout hand_post_layout(const isl_hand_post_plan& plan, int n, int h, int w, int nscales,
                                const isl_scale_geom* geom) {
  const int nparts = 21;
  const size_t P = (size_t)h * w;
  const int words = (w + 63) / 64;
  HandPostLayout l{};
  Carve carve;
  carve(l.avg, (size_t)n * nparts * P * 8);
  carve(l.mid, mid_bytes(n, nparts, h, w, nscales, geom));
  carve(l.mask, (size_t)n * nparts * h * words * 8);
  carve(l.parent, (size_t)n * nparts * P * 4);
  carve(l.vals, (size_t)n * nparts * P * 8);
  carve(l.stats, (size_t)n * nparts * sizeof(CcStats));
  carve(l.chunks, (size_t)n * nparts * plan.cc_chunks * sizeof(CcChunk));
  carve(l.bsum, (size_t)n * nparts * CC_KFAST * (P / 8192 + 1) * 8);
  carve(l.amb, (blur_tiles(n, nparts, h, w) + 1) * 4);
  l.total = carve.at;
  return l;
}

}  // namespace isl
