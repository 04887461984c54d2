// Digests of the weight packs (csrc/pack.cpp) of a fixed list of small synthetic layers: the
// smallest shapes at which each layout's index expressions can go wrong.  Host only, no device:
//   make tools/pack_digest && tools/pack_digest
// One line per pack: case, kind, element count, 2^-s (bit pattern), FNV-1a 64 of the bytes.
// tests/test_pack.py compares the output with tests/golden/pack_digests.txt, which was recorded
// from the pack functions as they stood in runtime.cpp (profiles/packs/README.md).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pack.h"

using namespace isl;

// weights in [-amp, amp) from an integer LCG (Knuth's MMIX constants), exact in fp32
static void fill(std::vector<float>& v, size_t n, uint64_t seed, float amp) {
  uint64_t s = seed;
  v.resize(n);
  for (float& x : v) {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    x = (float)((int)(s >> 40) - (1 << 23)) / (float)(1 << 23) * amp;
  }
}

static PackLayer layer(int cin, int cout, int k, int act, std::vector<Seg> cmap, int cin_phys, int bco, uint64_t seed,
                       float amp) {
  PackLayer c;
  c.cin = cin; c.cout = cout; c.k = k; c.act = act;
  c.cmap = cmap; c.cin_phys = cin_phys; c.bco = bco;
  fill(c.w, (size_t)cout * cin * k * k, seed, amp);
  fill(c.b, cout, seed + 1, 1.f);
  if (act == PACK_ACT_PRELU) fill(c.s, cout, seed + 2, 0.25f);
  return c;
}

static void line(const char* name, const char* kind, size_t elems, float inv, const void* data, size_t bytes) {
  uint64_t h = 1469598103934665603ULL;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ ((const unsigned char*)data)[i]) * 1099511628211ULL;
  uint32_t bits;
  memcpy(&bits, &inv, 4);
  printf("%s %s %zu %08x %016llx\n", name, kind, elems, bits, (unsigned long long)h);
}

static void pack(const char* name, const PackLayer& c, int kind, bool hi_only = false) {
  float inv = 1.f;
  const HostPack p = build_pack(c, kind, hi_only, &inv);
  line(name, (std::string(pack_name(kind)) + (hi_only ? ".hi" : "")).c_str(), p.elems(), inv, p.data(), p.bytes());
}

static void param(const char* name, const PackLayer& c, int which, const char* kind) {
  const std::vector<float> v = build_param(c, which, param_pad(c));
  line(name, kind, v.size(), 1.f, v.data(), v.size() * sizeof(float));
}

int main() {
  // 3x3, 20 logical channels in 40 physical with a gap: 5 chunks, 3 pairs, the last half empty;
  // cout 52 on 32-channel tiles (a partial tile), and as one tile of all 52 (the fused pair's form)
  PackLayer seg = layer(20, 52, 3, 1, {{0, 0, 12}, {12, 24, 8}}, 40, 32, 1, 0.37f);
  seg.fuse6 = true;
  auto seg_packs = [](const char* name, const PackLayer& c) {
    pack(name, c, PK_DIRECT);
    pack(name, c, PK_X3);
    pack(name, c, PK_X3, true);
    pack(name, c, PK_X3F);
    pack(name, c, PK_X3F, true);
  };
  seg_packs("seg3x3", seg);

  // 3x3 on the Winograd kernels: 3 chunks (a half-empty pair) with a gap, one 64-channel tile
  PackLayer wino = layer(20, 64, 3, 1, {{0, 0, 12}, {12, 16, 8}}, 24, 64, 2, 1.9f);
  wino.wbco = 64;
  pack("wino3x3", wino, PK_WINO);
  pack("wino3x3", wino, PK_WINO_F16);
#ifdef ISLPOSE_DEV
  pack("wino3x3", wino, PK_WINO_X3);
#endif

  const PackLayer rgb = layer(3, 64, 3, 1, {{0, 0, 3}}, 8, 64, 3, 0.011f);
  pack("rgb", rgb, PK_RGB);
  pack("rgb", rgb, PK_RGB, true);

  // the fusable 1x1 pair: Mconv6 (rows, bias, slopes in the fused K order) ...
  PackLayer m6 = layer(16, 64, 1, PACK_ACT_PRELU, {{0, 0, 16}}, 16, 64, 4, 3.f);
  m6.fuse6 = true;
  pack("pair6", m6, PK_X3P);
  pack("pair6", m6, PK_X3P, true);
  param("pair6", m6, PB_BIAS_PERM, "bias_perm");
  param("pair6", m6, PB_SLOPE_PERM, "slope_perm");
  param("pair6", m6, PB_BIAS, "bias");
  param("pair6", m6, PB_SLOPE, "slope");
  // ... and Mconv7, 26 channels: a partial 32-row tile
  PackLayer m7 = layer(64, 26, 1, 0, {{0, 0, 64}}, 64, 32, 5, 0.6f);
  m7.fuse7 = true;
  pack("pair7", m7, PK_X3F7);
  pack("pair7", m7, PK_X3F7, true);
  pack("pair7", m7, PK_X3P);
  pack("pair7", m7, PK_X3P, true);

  const PackLayer c7 = layer(8, 32, 7, 1, {{0, 0, 8}}, 8, 32, 6, 0.05f);
  pack("conv7x7", c7, PK_X3);

  // all-zero weights: exponent 0, 2^-s = 1
  PackLayer zero = seg;
  zero.w.assign(zero.w.size(), 0.f);
  seg_packs("zero", zero);

  // max|w| exactly a power of two: the frexp boundary
  PackLayer pow2 = seg;
  pow2.w[777] = -2.f;
  seg_packs("pow2", pow2);

  // 1x1 with 256-channel tiles: cout % 256 == 0 and an even number of chunk pairs
  PackLayer wide = layer(24, 256, 1, 1, {{0, 0, 24}}, 24, 128, 7, 0.8f);
  wide.x3_wide = true;
  pack("wide1x1", wide, PK_X3);
  pack("wide1x1", wide, PK_X3_WIDE);
  pack("wide1x1", wide, PK_X3_WIDE, true);
  return 0;
}
