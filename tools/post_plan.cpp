// The plans and scratch layouts of the post-processing on the CPU (tests/test_post_plan.py): the
// host-only decisions (csrc/post_plan.cpp) behind a command line.
//
//   post_plan FILE       every line of FILE is "case" or "case | ..."; prints "case | plan | layout"
//                        for each (tests/golden/post_plans.txt holds such lines).  The ISLPOSE_*
//                        switches are read from the tool's own environment, as a post reads them.
//   post_plan --switches the switch table, one "NAME default values" per line
//
// case:   body KIND n H W nscales  net_h net_w valid_h valid_w (per scale)  max_peaks max_pairs
//         max_conns max_rows             (KIND: body25 or coco)
//         hand n h w nscales  net_h net_w valid_h valid_w (per scale)
// plan:   every field of isl_body_post_plan / isl_hand_post_plan, the resize plans as
//         launched:ty:cols:v4:bm:identity per scale and the switches as read as env=fused_blur,
//         fused_wide,blur_list,blur_bands,resize_skip,resize_v4,blur_exact,limb_lds,asm_reg
// layout: the regions in their order as name=offset+bytes, then total (and the blur tiles)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "post_plan.h"

using namespace isl;

static std::string trim(const std::string& s) {
  const size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
  return a == std::string::npos ? "" : s.substr(a, b - a + 1);
}

static std::string resizes(const isl_resize_plan* r, int k) {
  std::string out;
  char b[64];
  for (int i = 0; i < k; ++i) {
    snprintf(b, sizeof b, "%s%d:%d:%d:%d:%d:%d", i ? "," : "", r[i].launched, r[i].ty, r[i].cols, r[i].v4, r[i].bm,
             r[i].identity);
    out += b;
  }
  return out;
}

static std::string ints(const int32_t* v, int k) {
  std::string out;
  for (int i = 0; i < k; ++i) out += (i ? "," : "") + std::to_string(v[i]);
  return out;
}

struct Named { const char* name; const PostRegion* r; };
static std::string regions(const std::vector<Named>& rs, size_t total) {
  std::string out;
  char b[96];
  for (const Named& x : rs) {
    snprintf(b, sizeof b, "%s=%zu+%zu ", x.name, x.r->off, x.r->bytes);
    out += b;
  }
  snprintf(b, sizeof b, "total=%zu", total);
  return out + b;
}

static bool read_geoms(std::istringstream& in, int nscales, std::vector<isl_scale_geom>* g) {
  if (nscales < 1 || nscales > MAX_SCALES) return false;
  g->resize(nscales);
  for (isl_scale_geom& x : *g)
    if (!(in >> x.net_h >> x.net_w >> x.valid_h >> x.valid_w)) return false;
  return plan_geom_ok(nscales, g->data());
}

static bool run_case(const std::string& text, const PostSwitches& sw, std::string* out) {
  static const char* kBlur[] = {"MULTI_F64", "FUSED_LIVE", "BAND_LIVE", "DENSE"};
  std::istringstream in(text);
  std::string what;
  in >> what;
  std::vector<isl_scale_geom> g;
  char b[1024];
  if (what == "body") {
    std::string kname;
    int n, H, W, ns;
    isl_caps caps{};
    if (!(in >> kname >> n >> H >> W >> ns) || (kname != "body25" && kname != "coco") || n < 1 || H < 1 || W < 1 ||
        !read_geoms(in, ns, &g) || !(in >> caps.max_peaks >> caps.max_pairs >> caps.max_conns >> caps.max_rows))
      return false;
    const int kind = kname == "body25" ? ISL_BODY25 : ISL_COCO;
    isl_body_post_plan p;
    body_post_plan(kind, n, H, W, ns, g.data(), sw, &p);
    const BodyPostLayout l = body_post_layout(p, kind, n, H, W, ns, g.data(), caps);
    snprintf(b, sizeof b,
             "multi=%d two_stage=%d fused=%d fuse2=%d wide=%d skip2=%d blur=%s blur_bandmax=%d acc_ty=%d stage2_ty=%d "
             "limb_z=%d env=%d,%d,%d,%d,%d,%d,%d,%d,%d scale_two_stage=%s stage1=%s final=%s",
             p.multi, p.two_stage, p.fused, p.fuse2, p.wide, p.skip2, kBlur[p.blur], p.blur_bandmax, p.acc_ty,
             p.stage2_ty, p.limb_z, p.env_fused_blur, p.env_fused_wide, p.env_blur_list, p.env_blur_bands,
             p.env_resize_skip, p.env_resize_v4, p.env_blur_exact, p.env_limb_lds, p.env_asm_reg,
             ints(p.scale_two_stage, ns).c_str(), resizes(p.stage1, ns).c_str(), resizes(p.final_rs, ns).c_str());
    *out = std::string(b) + " | " +
           regions({{"heat", &l.heat}, {"mid", &l.mid}, {"mask", &l.mask}, {"pairs", &l.pairs}, {"used", &l.used},
                    {"live", &l.live}, {"bandmax", &l.bandmax}, {"amb", &l.amb}, {"bm1", &l.bm1},
                    {"live_mid", &l.live_mid}, {"need", &l.need}},
                   l.total) +
           " tiles=" + std::to_string(l.n_tiles);
    return true;
  }
  if (what == "hand") {
    int n, h, w, ns;
    if (!(in >> n >> h >> w >> ns) || n < 1 || h < 1 || w < 1 || !read_geoms(in, ns, &g)) return false;
    isl_hand_post_plan p;
    hand_post_plan(h, w, ns, g.data(), sw, &p);
    const HandPostLayout l = hand_post_layout(p, n, h, w, ns, g.data());
    snprintf(b, sizeof b, "two_stage=%s identity=%s stage1=%s acc_ty=%d cc_lds=%d cc_rows=%d cc_chunks=%d",
             ints(p.two_stage, ns).c_str(), ints(p.identity, ns).c_str(), resizes(p.stage1, ns).c_str(), p.acc_ty,
             p.cc_lds, p.cc_rows, p.cc_chunks);
    *out = std::string(b) + " | " +
           regions({{"avg", &l.avg}, {"mid", &l.mid}, {"mask", &l.mask}, {"parent", &l.parent}, {"vals", &l.vals},
                    {"stats", &l.stats}, {"chunks", &l.chunks}, {"bsum", &l.bsum}, {"amb", &l.amb}},
                   l.total);
    return true;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "--switches")) {
    int n = 0;
    const PostSwitchDef* defs = post_switch_table(&n);
    for (int i = 0; i < n; ++i) {
      if (defs[i].first) printf("%s %d %s\n", defs[i].name, defs[i].def, defs[i].first);
      else printf("%s %d %d..%d\n", defs[i].name, defs[i].def, defs[i].lo, defs[i].hi);
    }
    return 0;
  }
  if (argc < 2) { fprintf(stderr, "usage: post_plan FILE | --switches\n"); return 2; }
  std::ifstream f(argv[1]);
  if (!f) { fprintf(stderr, "post_plan: cannot read %s\n", argv[1]); return 2; }
  const PostSwitches sw = post_switches();
  std::string line;
  while (std::getline(f, line)) {
    if (trim(line).empty() || line[0] == '#' || line[0] == '[') continue;
    const std::string text = trim(line.substr(0, line.find('|')));
    std::string out;
    if (!run_case(text, sw, &out)) { fprintf(stderr, "post_plan: bad case: %s\n", text.c_str()); return 2; }
    printf("%s | %s\n", text.c_str(), out.c_str());
  }
  return 0;
}
