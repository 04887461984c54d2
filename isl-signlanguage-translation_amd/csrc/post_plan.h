// The host-side decisions of the post-processing (post.hip): host-only.  The constants that size
// tiles and scratch, the ISLPOSE_* switches of the post in one table, the plans (which kernel
// forms and which blur branch a post takes) and the scratch layouts, each written once:
// allocation and launch read the same struct.  Pure host arithmetic, no HIP headers and no
// device -- tools/post_plan.cpp and tests/test_post_plan.py hold it to a golden file on the CPU.
#pragma once
#include <cstddef>

#include "islpose.h"

namespace isl {

// ---------------------------------------------------------------------------
// Sizing constants (the kernels that read them: post.hip)
// ---------------------------------------------------------------------------
// resize_sep_kernel: a block covers RS_TY output rows x RS_TX (or 128) output columns of one
// plane; RS_MAXR source rows fit its LDS window
constexpr int RS_TY = 64, RS_TX = 256, RS_MAXR = 40;   // 64 rows: amortise the horizontal pass
constexpr int BM_ROWS = 16;   // rows per band of the band maxima (resize_sep_kernel BM)
constexpr int RA_TY = 16;     // resize_acc_kernel: output rows per block (fp64 accumulators in registers)
// blur_nms_kernel's tile: 16 output rows x 192 output columns (3 mask words)
constexpr int NMS_TY = 16, NMS_TX = 192;
// its fused source window (FUSED = true), and the wide one (development build)
constexpr int NMS_SRC_ROWS = 16;
constexpr int NMS_SRC_COLS = 48;                   // source columns (218 / 8 + 5 = 33 at scale 1/8; 42 at 1/5.9)
constexpr int NMS_WSRC_ROWS = 28;
constexpr int NMS_WSRC_COLS = 120;
constexpr int MAX_SCALES = 8;
static_assert(ISL_PLAN_SCALES == MAX_SCALES, "the plan structs hold one slot per scale");
constexpr int CC_LDS_MAX = 36864;   // plane pixels whose parent array fits LDS (144 KB)
constexpr int CC_CHUNK = 4096;      // pixels per row chunk of the large-plane path
constexpr int CC_WMAX = 8192;       // widest plane the large-plane path takes (LDS chunk parents)
constexpr int CC_MAXC = 64;         // candidate components kept per plane
constexpr int CC_KFAST = 4;         // candidate components of the fast finish (cc_count_kernel)
constexpr int ASM_LDS_ROWS = 256;   // subset rows that fit the LDS table (256 x 27 doubles = 55 KB)
constexpr int ASM_CONN_CACHE = 512;   // x 5 doubles = 20 KB

// per-plane results of the large-plane pre-pass
struct CcStats {
  int count;                        // foreground pixels
  int ncand;                        // components whose approximate sum reaches the candidate bar
  unsigned long long maxbits;       // largest approximate component sum (bits of a positive double)
  int cand[CC_MAXC];                // their roots, unordered
};
// per (plane, chunk): the candidates' pixel counts and first maxima
struct CcChunk {
  int count[CC_KFAST];
  int besti[CC_KFAST];
  double bestv[CC_KFAST];
};

// ---------------------------------------------------------------------------
// The switches of the post, read per call: every entry of a post reads the table once
// (post_switches) and passes the struct down.  Their meanings stand with the code that reads
// them, in post_plan.cpp and post.hip.
// ---------------------------------------------------------------------------
struct PostSwitches {
  int fused_blur, blur_list, blur_bands, blur_exact, resize_skip, resize_v4, limb_split;
  int limb_z;   // 0: unset (the plan picks the blocks per limb)
  int limb_lds, asm_reg;
  // read in development builds only (ISLPOSE_DEV); off elsewhere
  int fused_wide, tile_prof, asm_prof;
};
struct PostSwitchDef {
  const char* name;
  int PostSwitches::*field;
  int def;             // the value when the variable is unset or has none of `first`
  const char* first;   // the first characters that count, each a digit and its value;
                       // null: any value, through atoi, clamped to lo..hi
  int lo, hi;
};
const PostSwitchDef* post_switch_table(int* count);
PostSwitches post_switches();

// ---------------------------------------------------------------------------
// The plans
// ---------------------------------------------------------------------------
// rows per tile: `ty` lowered until the source window of a resize of vertical scale scy fits
// the LDS rows
int fit_rows(int ty, double scy, bool identity);
int resize_rows(double scy, bool identity);   // output rows per resize tile
// The form launch_resize runs for a source of vertical scale scy onto ow columns; want_bm: the
// caller has a band-maxima buffer for it (mode 1).
isl_resize_plan resize_form(double scy, bool identity, int ow, int mode, bool want_bm, const PostSwitches& sw);
bool plan_geom_ok(int nscales, const isl_scale_geom* geom);
// What isl_body_post_opts chooses on the host for n frames of H x W (no device work): the
// post launches from this plan, and isl_debug_body_post_plan returns it.
void body_post_plan(int kind, int n, int H, int W, int nscales, const isl_scale_geom* geom, const PostSwitches& sw,
                    isl_body_post_plan* p);
// What hand_post_launch chooses on the host for crops of h x w (no device work): the launch
// follows this plan, and isl_debug_hand_post_plan returns it.
void hand_post_plan(int h, int w, int nscales, const isl_scale_geom* geom, const PostSwitches& sw,
                    isl_hand_post_plan* p);

// ---------------------------------------------------------------------------
// The scratch layouts: the regions of one post in the order they lie in the scratch buffer,
// each starting at a multiple of 256 bytes.  A region the plan does not use has no bytes (and
// the offset of the next one).  `total`: the end of the last region, rounded up alike.
// ---------------------------------------------------------------------------
struct PostRegion {
  size_t off, bytes;
  size_t padded() const { return (bytes + 255) / 256 * 256; }   // the bytes up to the next region
};
struct BodyPostLayout {
  PostRegion heat;       // full-resolution heat planes (fp64 for several scales); none when fused
  PostRegion mid;        // the stage-1 planes of every two-stage scale
  PostRegion mask;       // peak mask, one bit per pixel
  PostRegion pairs;      // limb_kernel: scores, keep flags and order of the candidate pairs
  PostRegion used;       // limb_kernel: used flags of the peaks
  PostRegion live;       // live-tile list: count, then tiles
  PostRegion bandmax;    // band maxima of the final resize
  PostRegion amb;        // the blur filter's undecided tiles: count, then tiles
  PostRegion bm1;        // skip2: band maxima of the stage-1 planes
  PostRegion live_mid;   // skip2: blur tiles that can be live (stage2_need_kernel)
  PostRegion need;       // skip2: stage-2 resize tiles a live window reads
  size_t total;
  size_t n_tiles;        // blur tiles of the call
};
BodyPostLayout body_post_layout(const isl_body_post_plan& plan, int kind, int n, int H, int W, int nscales,
                                const isl_scale_geom* geom, const isl_caps& caps);
struct HandPostLayout {
  PostRegion avg;      // fp64 average planes
  PostRegion mid;      // every scale's stage-1 planes (they stay until the fused average)
  PostRegion mask;     // peak mask
  PostRegion parent;   // component parents
  PostRegion vals;     // component sums, then the compacted candidate values
  PostRegion stats;    // CcStats per plane
  PostRegion chunks;   // CcChunk per (plane, chunk)
  PostRegion bsum;     // np.sum's 8192-element buffer sums per candidate
  PostRegion amb;      // the blur filter's undecided tiles
  size_t total;
};
HandPostLayout hand_post_layout(const isl_hand_post_plan& plan, int n, int h, int w, int nscales,
                                const isl_scale_geom* geom);

}  // namespace isl
