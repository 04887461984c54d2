// What launch_conv_x3 would run for a launch, on the CPU (tests/test_x3_select.py): the host-only
// launch selection (csrc/x3_select.cpp) behind a command line.
//
//   x3_choice FILE [cus]   every line of FILE is "descriptor | switches | ..."; prints
//                          "descriptor | switches | choice" for each (tests/golden/x3_choices.txt
//                          holds such lines with the choices the kernels' launchers recorded)
//   x3_choice --instances  the instances of csrc/x3_instances.h, one per line and form
//   x3_choice --sweep      walks a synthetic grid of launches and switches and checks that the
//                          instance table is closed under the decision; exit status 1 if not
//
// descriptor: name=value pairs of the ConvLaunch fields the decision reads (pointers as 0 / 1),
// and rgb=1 for a conv_x3_rgb launch.  switches: NAME=value pairs, with or without the ISLPOSE_
// prefix (every other switch of the table is unset).  choice: f16<...> / wr<...> / rgb<...> are
// conv_x3_f16, conv_x3_wr and conv_x3_rgb with their template arguments, S the K ranges, x=1 when
// they run across blocks, code the variant code.  cus: the device's compute units (default 256).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "x3_select.h"

using namespace isl;

static ConvLaunch blank() {
  ConvLaunch c{};
  c.ks = 3; c.cin_chunks = 16; c.cout = 128; c.bco = 128; c.n = 1; c.H = 46; c.W = 82; c.in_pad = 1;
  return c;
}

static std::string describe(const ConvLaunch& c, bool rgb) {
  char b[512];
  snprintf(b, sizeof b,
           "ks=%d cin_chunks=%d cout=%d bco=%d n=%d H=%d W=%d in_pad=%d allow_split=%d f16=%d act16=%d hpool=%d vin=%d "
           "fold=%d fold_out=%d cout7=%d dbg=%d out32=%d rgb=%d",
           c.ks, c.cin_chunks, c.cout, c.bco, c.n, c.H, c.W, c.in_pad, c.allow_split, c.f16, c.act16, c.hpool, c.vin,
           c.fold ? 1 : 0, c.fold_out, c.cout7, c.dbg ? 1 : 0, c.out32 ? 1 : 0, rgb ? 1 : 0);
  return b;
}

static bool parse(const std::string& text, ConvLaunch* c, bool* rgb) {
  static const X3Fold fold{};
  static unsigned long long dbg;
  static float out32;
  *c = blank();
  *rgb = false;
  std::istringstream in(text);
  std::string tok;
  while (in >> tok) {
    const size_t eq = tok.find('=');
    if (eq == std::string::npos) return false;
    const std::string k = tok.substr(0, eq);
    const int v = atoi(tok.c_str() + eq + 1);
    if (k == "ks") c->ks = v;
    else if (k == "cin_chunks") c->cin_chunks = v;
    else if (k == "cout") c->cout = v;
    else if (k == "bco") c->bco = v;
    else if (k == "n") c->n = v;
    else if (k == "H") c->H = v;
    else if (k == "W") c->W = v;
    else if (k == "in_pad") c->in_pad = v;
    else if (k == "allow_split") c->allow_split = v;
    else if (k == "f16") c->f16 = v;
    else if (k == "act16") c->act16 = v;
    else if (k == "hpool") c->hpool = v;
    else if (k == "vin") c->vin = v;
    else if (k == "fold") c->fold = v ? &fold : nullptr;
    else if (k == "fold_out") c->fold_out = v;
    else if (k == "cout7") c->cout7 = v;
    else if (k == "dbg") c->dbg = v ? &dbg : nullptr;
    else if (k == "out32") c->out32 = v ? &out32 : nullptr;
    else if (k == "rgb") *rgb = v != 0;
    else return false;
  }
  return true;
}

static void set_switches(const std::string& text) {
  int n = 0;
  const X3SwitchDef* defs = x3_switch_table(&n);
  for (int i = 0; i < n; ++i) unsetenv(defs[i].name);
  std::istringstream in(text);
  std::string tok;
  while (in >> tok) {
    const size_t eq = tok.find('=');
    if (eq == std::string::npos) continue;
    const std::string name = tok.substr(0, eq);   // (with or without the ISLPOSE_ prefix)
    setenv((name.compare(0, 8, "ISLPOSE_") ? "ISLPOSE_" + name : name).c_str(), tok.c_str() + eq + 1, 1);
  }
}

static std::string show(const X3Choice& ch) {
  char b[256];
  switch (ch.family) {
    case X3Choice::NONE: return "none";
    case X3Choice::F16: case X3Choice::FUSED67:
      snprintf(b, sizeof b, "f16<%d,%d,%d,%d,%d,%d,%d> S=%d x=%d code=%d", ch.ks, ch.waves_m, ch.waves_n, ch.wm,
               ch.wn, ch.var, ch.occ, ch.S, ch.across_blocks ? 1 : 0, ch.code);
      return b;
    case X3Choice::WR:
      snprintf(b, sizeof b, "wr<%d,%d,%d,%d> S=%d x=%d code=%d", ch.ks, ch.wn, ch.depth, (ch.var & X3V_F16) ? 1 : 0,
               ch.S, ch.across_blocks ? 1 : 0, ch.code);
      return b;
    case X3Choice::RGB:
      snprintf(b, sizeof b, "rgb<%d,%d,%d> S=1 x=0 code=%d", ch.bpx, (ch.var & X3V_F16) ? 1 : 0,
               (ch.var & X3V_A16) ? 1 : 0, ch.code);
      return b;
  }
  return "none";
}

static std::string trim(const std::string& s) {
  const size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
  return a == std::string::npos ? "" : s.substr(a, b - a + 1);
}

static int run_file(const char* path, int cus) {
  std::ifstream f(path);
  if (!f) { fprintf(stderr, "x3_choice: cannot read %s\n", path); return 2; }
  std::string line;
  while (std::getline(f, line)) {
    if (trim(line).empty() || line[0] == '#') continue;
    const size_t p1 = line.find('|'), p2 = p1 == std::string::npos ? p1 : line.find('|', p1 + 1);
    if (p2 == std::string::npos) { fprintf(stderr, "x3_choice: bad line: %s\n", line.c_str()); return 2; }
    const std::string desc = trim(line.substr(0, p1)), sws = trim(line.substr(p1 + 1, p2 - p1 - 1));
    ConvLaunch c;
    bool rgb;
    if (!parse(desc, &c, &rgb)) { fprintf(stderr, "x3_choice: bad descriptor: %s\n", desc.c_str()); return 2; }
    set_switches(sws);
    const X3Choice ch = rgb ? x3_choose_rgb(c) : x3_choose(c, cus, x3_switches());
    printf("%s | %s | %s\n", desc.c_str(), sws.c_str(), show(ch).c_str());
  }
  return 0;
}

static void print_instances() {
#define X3_F16(KS, A, B, C, D, VAR, OCC, FORMS)                                                                   \
  for (int f = 0; f < 3; ++f)                                                                                     \
    if ((FORMS) >> f & 1) printf("f16<%d,%d,%d,%d,%d,%d,%d>\n", KS, A, B, C, D, (VAR) | (f == 0 ? 0 : f == 1 ? 2 : 3), OCC);
#define X3_WR(KS, WN, DEPTH, FORMS) \
  for (int f = 0; f < 2; ++f)       \
    if ((FORMS) >> f & 1) printf("wr<%d,%d,%d,%d>\n", KS, WN, DEPTH, f);
#include "x3_instances.h"
#undef X3_F16
#undef X3_WR
}

// The table is closed under the decision: for every point of the grid the choice is an instance
// in the requested form or none with an error text; the fp16-storage answer is the instance's
// form; a workspace is asked for exactly by the across-block launches off the wave-range kernel.
static int sweep() {
  int n = 0;
  const X3SwitchDef* defs = x3_switch_table(&n);
  // every switch singly, at each of its documented values (and one undocumented)
  std::vector<std::string> settings = {""};
  for (int i = 0; i < n; ++i) {
    const std::string name = defs[i].name;
    std::vector<std::string> vals;
    if (defs[i].first) {
      for (const char* p = defs[i].first; *p; ++p) vals.push_back(std::string(1, *p));
      vals.push_back(defs[i].first[0] == 's' ? "b" : "7");
    } else {
      vals = {"-1", "0", "1", "2", "3", "4"};
    }
    for (const std::string& v : vals) settings.push_back(name + "=" + v);
  }
  struct Plane { int H, W; };
  const Plane planes[] = {{1, 1}, {5, 1}, {64, 2}, {33, 7}, {23, 23}, {23, 41}, {46, 46}, {46, 82}, {92, 92},
                          {92, 164}, {184, 328}, {368, 656}};
  const int bcos[] = {32, 64, 96, 128, 256}, chunks[] = {1, 2, 3, 4, 8, 12, 16, 24, 32, 36, 48, 64}, ns[] = {1, 2, 16, 32};
  long long points = 0, bad = 0;
  auto fail = [&](const ConvLaunch& c, const std::string& sws, const X3Choice& ch, const char* what) {
    if (++bad <= 20) fprintf(stderr, "sweep: %s: %s | %s | %s\n", what, describe(c, false).c_str(), sws.c_str(), show(ch).c_str());
  };
  for (const std::string& sws : settings) {
    set_switches(sws);
    const X3Switches sw = x3_switches();
    for (int ks : {1, 3, 7})
      for (int bco : bcos)
        for (int cc : chunks)
          for (const Plane& p : planes)
            for (int nn : ns)
              for (int form = 0; form < 3; ++form)
                for (int split = 0; split < 3; ++split)
                  for (int extra = 0; extra < 4; ++extra) {   // plain, hpool, vin, the fused pair
                    ConvLaunch c = blank();
                    c.ks = ks; c.bco = bco; c.cin_chunks = cc; c.H = p.H; c.W = p.W; c.n = nn;
                    c.in_pad = ks == 7 ? 3 : 1;
                    c.cout = bco == 256 ? 512 : bco == 128 ? 128 : bco;
                    c.f16 = form > 0; c.act16 = form > 1;
                    c.allow_split = split;
                    c.hpool = extra == 1; c.vin = extra == 2;
                    if (extra == 3) {
                      if (ks != 1 || bco < 128) continue;
                      c.cout7 = 52; c.cout = bco == 256 ? 256 : 128 * (1 + 3 * (cc & 1));   // 128, 256, 512
                    }
                    ++points;
                    const X3Choice ch = x3_choose(c, 256, sw);
                    const int forms = x3_instance_forms(ch);
                    if (ch.family == X3Choice::NONE) {
                      if (!ch.error || !ch.error[0]) fail(c, sws, ch, "none without an error text");
                      if (ch.act16 || ch.ws_floats) fail(c, sws, ch, "none with a plan");
                      continue;
                    }
                    const int want = ch.family == X3Choice::WR ? (c.f16 ? 2 : 1) : 1 << form;
                    // (a launch on fp16 buffers the choice gives no such form is refused by
                    // launch_conv_x3 before the table is read: the run never plans it)
                    if (!(forms & want) && !(c.act16 && !ch.act16)) fail(c, sws, ch, "not an instance in this form");
                    if (!forms) fail(c, sws, ch, "not an instance");
                    // (the one exception: ISLPOSE_X3_WR=2 keeps every launch but the fused pair on fp32 buffers)
                    const bool a16 = c.f16 && (forms & 4) && (extra == 3 || sw.wr != 2);
                    if (x3_act16_ok(c, 256, sw) != a16) fail(c, sws, ch, "x3_act16_ok is not the instance's fp16-storage form");
                    if ((ch.ws_floats != 0) != (ch.across_blocks && ch.family != X3Choice::WR)) fail(c, sws, ch, "workspace");
                  }
  }
  printf("sweep: %lld points, %zu switch settings, %lld violations\n", points, settings.size(), bad);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "--instances")) { print_instances(); return 0; }
  if (argc >= 2 && !strcmp(argv[1], "--sweep")) return sweep();
  if (argc < 2) { fprintf(stderr, "usage: x3_choice FILE [cus] | --instances | --sweep\n"); return 2; }
  return run_file(argv[1], argc > 2 ? atoi(argv[2]) : 256);
}
