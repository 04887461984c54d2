// Weight packing (pack.h): OIHW fp32 filters into the layouts the conv kernels read.  The
// layout comments here are the specification the kernels are written against.  Compiled with
// -ffp-contract=off: every pack is a fixed sequence of roundings.
#include "pack.h"

#include <algorithm>
#include <cmath>

namespace isl {

// Physical input channel -> logical (the concat order of the reference), -1 for a gap; n
// entries (the pair layouts pad cin_phys to whole chunk pairs).
static std::vector<int> phys_to_logical(const PackLayer& c, int n) {
  std::vector<int> p2l(n, -1);
  for (const Seg& s : c.cmap)
    for (int i = 0; i < s.len; ++i) p2l[s.phys + i] = s.logical + i;
  return p2l;
}

static int chunk_pairs(const PackLayer& c) { return (c.cin_phys / 8 + 1) / 2; }

// The per-layer power of two of the split packs: s with mx * 2^s in [2^13, 2^14), 0 for mx = 0
static int pow2_exp(double mx) {
  int e = 0;
  if (mx > 0.0) {
    std::frexp(mx, &e);            // mx = f * 2^e, f in [0.5, 1)
    e = 14 - e;                    // mx * 2^e in [2^13, 2^14)
  }
  return e;
}

static int weight_exp(const PackLayer& c) {
  float mx = 0.f;
  for (float v : c.w) mx = std::max(mx, std::fabs(v));
  return pow2_exp(mx);
}

// w = hi + lo (both fp16, round to nearest) into the [hi|lo] planes of a split pack: hi at
// `at`, lo one plane of `group` values further
static void put_split(std::vector<_Float16>& out, size_t at, size_t group, float w) {
  const _Float16 hi = (_Float16)w;
  out[at] = hi;
  out[at + group] = (_Float16)(w - (float)hi);
}

// U = G g G^T of one 3x3 filter, in double; U[4 * row + col]
static void wino_transform(const float* g, double* U) {
  static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  double t[4][3];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 3; ++j) t[i][j] = G[i][0] * g[0 * 3 + j] + G[i][1] * g[1 * 3 + j] + G[i][2] * g[2 * 3 + j];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) U[4 * i + j] = t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2];
}

// Repack OIHW weights into [co_tile][chunk][ky][kx][plane(2)][BCO][4] (see conv.hip).
static std::vector<float> pack_weights(const PackLayer& c) {
  const int ks = c.k, bco = c.bco, chunks = c.cin_phys / 8;
  const int co_tiles = (c.cout + bco - 1) / bco;
  const std::vector<int> p2l = phys_to_logical(c, c.cin_phys);
  std::vector<float> out((size_t)co_tiles * chunks * ks * ks * 2 * bco * 4, 0.f);
  size_t idx = 0;
  for (int ct = 0; ct < co_tiles; ++ct)
    for (int ch = 0; ch < chunks; ++ch)
      for (int ky = 0; ky < ks; ++ky)
        for (int kx = 0; kx < ks; ++kx)
          for (int pl = 0; pl < 2; ++pl)
            for (int i = 0; i < bco; ++i)
              for (int e = 0; e < 4; ++e, ++idx) {
                const int co = ct * bco + i, lci = p2l[ch * 8 + pl * 4 + e];
                if (co < c.cout && lci >= 0) out[idx] = c.w[(((size_t)co * c.cin + lci) * ks + ky) * ks + kx];
              }
  return out;
}

// U = G g G^T of every (co, physical ci) 3x3 filter, in double, rounded once to
// fp32; layout [co_tile][chunk][xi = 4*row + col][plane][BCO][4] (wino.hip).
static std::vector<float> pack_wino(const PackLayer& c) {
  const int bco = c.wbco, chunks = c.cin_phys / 8, co_tiles = c.cout / bco;
  const std::vector<int> p2l = phys_to_logical(c, c.cin_phys);
  std::vector<float> out((size_t)co_tiles * chunks * 16 * 2 * bco * 4, 0.f);
  for (int co = 0; co < c.cout; ++co)
    for (int pc = 0; pc < c.cin_phys; ++pc) {
      const int lci = p2l[pc];
      if (lci < 0) continue;
      double U[16];
      wino_transform(&c.w[((size_t)co * c.cin + lci) * 9], U);
      const int ct = co / bco, i_co = co % bco, ch = pc / 8, pl = (pc % 8) / 4, e = pc % 4;
      for (int xi = 0; xi < 16; ++xi)
        out[((((size_t)ct * chunks + ch) * 16 + xi) * 2 + pl) * bco * 4 + (size_t)i_co * 4 + e] = (float)U[xi];
    }
  return out;
}

// Split-fp16 filters for conv_x3.hip: w * 2^s = hi + lo (both fp16, round to
// nearest), 2^s chosen per layer so that max|w| * 2^s lies in [2^13, 2^14);
// layout [co_tile][chunk pair][ky][kx][hi|lo][h][BCO][8], h = chunk of the pair.
static std::vector<_Float16> pack_x3(const PackLayer& c, int bco, float* inv_scale) {
  const int ks = c.k, pairs = chunk_pairs(c);
  const int co_tiles = (c.cout + bco - 1) / bco;
  const std::vector<int> p2l = phys_to_logical(c, pairs * 16);
  const int e = weight_exp(c);
  const float scale = std::ldexp(1.f, e);
  *inv_scale = std::ldexp(1.f, -e);
  const size_t group = (size_t)2 * bco * 8;
  std::vector<_Float16> out((size_t)co_tiles * pairs * ks * ks * 2 * group, (_Float16)0.f);
  for (int ct = 0; ct < co_tiles; ++ct)
    for (int pr = 0; pr < pairs; ++pr)
      for (int ky = 0; ky < ks; ++ky)
        for (int kx = 0; kx < ks; ++kx)
          for (int h = 0; h < 2; ++h)
            for (int i = 0; i < bco; ++i)
              for (int j = 0; j < 8; ++j) {
                const int co = ct * bco + i, lci = p2l[pr * 16 + h * 8 + j];
                if (co >= c.cout || lci < 0) continue;
                const size_t base = ((((size_t)(ct * pairs + pr) * ks + ky) * ks + kx) * 2) * 2 * bco;
                put_split(out, (base + (size_t)h * bco + i) * 8 + j, group,
                          c.w[(((size_t)co * c.cin + lci) * ks + ky) * ks + kx] * scale);
              }
  return out;
}

// The split-fp16 Winograd packs: U = G g G^T per (co, physical ci) in double, scaled by a
// per-layer 2^s (max|U| * 2^s in [2^13, 2^14), as pack_x3), rounded once to fp32 and split
// hi + lo.  `out` is the zeroed pack, at(co, pc, xi) the position of a hi value, its lo `group`
// values further.
template <class At>
static void pack_wino_split(const PackLayer& c, std::vector<_Float16>& out, size_t group, float* inv_scale, At at) {
  const int pcs = chunk_pairs(c) * 16;
  const std::vector<int> p2l = phys_to_logical(c, pcs);
  std::vector<double> U((size_t)c.cout * pcs * 16, 0.0);   // [co][pc][xi]
  double mx = 0.0;
  for (int co = 0; co < c.cout; ++co)
    for (int pc = 0; pc < pcs; ++pc) {
      if (p2l[pc] < 0) continue;
      double* u = &U[((size_t)co * pcs + pc) * 16];
      wino_transform(&c.w[((size_t)co * c.cin + p2l[pc]) * 9], u);
      for (int xi = 0; xi < 16; ++xi) mx = std::max(mx, std::fabs(u[xi]));
    }
  const int e = pow2_exp(mx);
  const double scale = std::ldexp(1.0, e);
  *inv_scale = std::ldexp(1.f, -e);
  for (int co = 0; co < c.cout; ++co)
    for (int pc = 0; pc < pcs; ++pc) {
      if (p2l[pc] < 0) continue;
      for (int xi = 0; xi < 16; ++xi)
        put_split(out, at(co, pc, xi), group, (float)(U[((size_t)co * pcs + pc) * 16 + xi] * scale));
    }
}

// Split-fp16 Winograd filters for wino_f16.hip (pack_wino_split);
// layout [co_block 64][pair][xi 16][co tile i 2][hi|lo][h][32][8] -- one wave's
// filters of a K step are 4 contiguous 1 KiB pieces (i, hi|lo), lane = h * 32 + co.
static std::vector<_Float16> pack_wino_f16(const PackLayer& c, float* inv_scale) {
  const int pairs = chunk_pairs(c), cob = c.cout / 64;
  std::vector<_Float16> out((size_t)cob * pairs * 16 * 2 * 2 * 2 * 32 * 8, (_Float16)0.f);
  pack_wino_split(c, out, 2 * 32 * 8, inv_scale, [&](int co, int pc, int xi) {
    const int cb = co / 64, i = (co % 64) / 32, r = co % 32, pr = pc / 16, h = (pc % 16) / 8, k = pc % 8;
    const size_t base = ((((size_t)cb * pairs + pr) * 16 + xi) * 2 + i) * 2;
    return ((base * 2 + h) * 32 + r) * 8 + k;
  });
  return out;
}

#ifdef ISLPOSE_DEV
// Split-fp16 Winograd filters for wino_x3.hip (pack_wino_split);
// layout [co_tile][pair][xi][hi|lo][h][64][8], h = chunk of the pair.
static std::vector<_Float16> pack_wino_x3(const PackLayer& c, float* inv_scale) {
  constexpr int BCO = PACK_WINO_X3_BCO;
  const int pairs = chunk_pairs(c), co_tiles = (c.cout + BCO - 1) / BCO;
  std::vector<_Float16> out((size_t)co_tiles * pairs * 16 * 2 * 2 * BCO * 8, (_Float16)0.f);
  pack_wino_split(c, out, 2 * BCO * 8, inv_scale, [&](int co, int pc, int xi) {
    const int ct = co / BCO, i_co = co % BCO, pr = pc / 16, h = (pc % 16) / 8, k = pc % 8;
    const size_t base = (((size_t)ct * pairs + pr) * 16 + xi) * 2;
    return ((base * 2 + h) * BCO + i_co) * 8 + k;
  });
  return out;
}
#endif

bool rgb_layer(const PackLayer& c) {
  return c.k == 3 && c.cin == 3 && c.cin_phys == 8 && c.cout <= 64 && c.cmap.size() == 1 && c.cmap[0].phys == 0 &&
         c.cmap[0].logical == 0 && c.cmap[0].len == 3;
}

// conv1_1 filters for conv_x3_rgb: K = 9 ky + 3 kx + c (27 real, padded to 32),
// k = 16 kk + 8 h + j, layout [kk][hi|lo][h][64][8]; the same 2^s as pack_x3.
static std::vector<_Float16> pack_x3_rgb(const PackLayer& c, float* inv_scale) {
  const int e = weight_exp(c);
  const float scale = std::ldexp(1.f, e);
  *inv_scale = std::ldexp(1.f, -e);
  const size_t group = (size_t)2 * 64 * 8;
  std::vector<_Float16> out(2 * 2 * group, (_Float16)0.f);
  for (int k = 0; k < 27; ++k) {
    const int ky = k / 9, kx = (k % 9) / 3, ci = k % 3, kk = k / 16, h = (k % 16) / 8, j = k % 8;
    for (int co = 0; co < c.cout; ++co)
      put_split(out, ((((size_t)kk * 2 + 0) * 2 + h) * 64 + co) * 8 + j, group,
                c.w[(((size_t)co * 3 + ci) * 3 + ky) * 3 + kx] * scale);
  }
  return out;
}

// Mconv7 of a fused 1x1 pair (conv_x3 VAR 16): the K order of Mconv6's accumulator
// registers.  K block kb = 2 g + q covers Mconv6 channels [32 g, 32 g + 32) half q; its slot j
// of lane half h is register 8 q + j of that 32-row D tile, i.e. channel
// 32 g + 16 q + 8 (j >> 2) + 4 h + (j & 3).  Layout [row tile t][kb][hi|lo][h][32][8], the same
// 2^s as pack_x3 (max|w| * 2^s in [2^13, 2^14)).
static std::vector<_Float16> pack_x3_f7(const PackLayer& c, float* inv_scale) {
  const int e = weight_exp(c);
  const float scale = std::ldexp(1.f, e);
  *inv_scale = std::ldexp(1.f, -e);
  const int nt = (c.cout + 31) / 32, kbs = c.cin / 16;
  const size_t group = (size_t)2 * 32 * 8;
  std::vector<_Float16> out((size_t)nt * kbs * 2 * group, (_Float16)0.f);
  for (int t = 0; t < nt; ++t)
    for (int kb = 0; kb < kbs; ++kb)
      for (int h = 0; h < 2; ++h)
        for (int row = 0; row < 32; ++row)
          for (int j = 0; j < 8; ++j) {
            const int co = 32 * t + row;
            if (co >= c.cout) continue;
            const int ch = 32 * (kb >> 1) + 16 * (kb & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
            const size_t base = ((size_t)(t * kbs + kb) * 2) * 64;
            put_split(out, (base + h * 32 + row) * 8 + j, group, c.w[(size_t)co * c.cin + ch] * scale);
          }
  return out;
}

// Mconv6 output channel order of a fusable pair's two-launch form: physical channel
// 16 p + 8 h + j (chunk h of pair p, element j) holds the channel that sits in slot j of lane
// half h of the fused kernel's K block p (pack_x3_f7): 32 g + 16 q + 8 (j >> 2) + 4 h + (j & 3),
// p = 2 g + q.  Mconv7 then stages exactly the fused kernel's B fragments.
int f7_logical(int phys) {
  const int p = phys >> 4, h = (phys >> 3) & 1, j = phys & 7, g = p >> 1, q = p & 1;
  return 32 * g + 16 * q + 8 * (j >> 2) + 4 * h + (j & 3);
}

// The permuted copies of a fusable pair's layers (two-launch form): Mconv6 with its output
// rows (weights, bias, slopes) in f7_logical order, Mconv7 with the matching channel map
PackLayer f7_permuted(const PackLayer& c) {
  PackLayer p = c;
  if (c.fuse6) {
    const size_t per = (size_t)c.cin * c.k * c.k;
    for (int ph = 0; ph < c.cout; ++ph) {
      const int lg = f7_logical(ph);
      std::copy(c.w.begin() + lg * per, c.w.begin() + (lg + 1) * per, p.w.begin() + ph * per);
      p.b[ph] = c.b[lg];
      if (c.act == PACK_ACT_PRELU) p.s[ph] = c.s[lg];
    }
  } else {
    p.cmap.clear();
    for (int ph = 0; ph < c.cin; ++ph) p.cmap.push_back({f7_logical(ph), ph, 1});
  }
  return p;
}

// The hi halves of a split pack whose [hi|lo] dimension has `group` fp16 values per plane
// (pack_x3: 2 * bco * 8, pack_x3_rgb: 2 * 64 * 8): the planes [.. ][hi] in order, i.e. the same
// layout without that dimension and the same 2^s -- the filters rounded once to fp16 (RNE)
static std::vector<_Float16> pack_hi_only(const std::vector<_Float16>& split, size_t group) {
  std::vector<_Float16> out(split.size() / 2);
  for (size_t g = 0; g < out.size() / group; ++g)
    std::copy(split.begin() + 2 * g * group, split.begin() + (2 * g + 1) * group, out.begin() + g * group);
  return out;
}

const char* pack_name(int kind) {
  static const char* const names[] = {"direct", "wino", "x3", "x3_wide", "rgb", "x3f", "x3f7", "x3p", "wino_f16", "wino_x3"};
  return names[kind];
}

bool owns_pack(const PackLayer& c, int kind) {
  switch (kind) {
    case PK_DIRECT:
    case PK_X3: return true;
    case PK_WINO: return c.wbco != 0;
    case PK_X3_WIDE: return c.x3_wide;
    case PK_RGB: return rgb_layer(c);
    case PK_X3F: return c.fuse6 && c.bco != c.cout;
    case PK_X3F7: return c.fuse7;
    case PK_X3P: return c.fuse6 || c.fuse7;
    case PK_WINO_F16: return c.k == 3 && c.cout % 64 == 0 && !rgb_layer(c);
#ifdef ISLPOSE_DEV
    case PK_WINO_X3: return c.k == 3 && c.cout % 4 == 0;
#endif
  }
  return false;
}

bool pack_has_hi(int kind) { return kind >= PK_X3 && kind <= PK_X3P; }

HostPack build_pack(const PackLayer& c, int kind, bool hi_only, float* inv) {
  HostPack p;
  int tile = 0;   // channels per [hi|lo] plane and chunk of a pack_has_hi kind
  *inv = 1.f;
  switch (kind) {
    case PK_DIRECT: p.f32 = pack_weights(c); break;
    case PK_WINO: p.f32 = pack_wino(c); break;
    case PK_X3: p.f16 = pack_x3(c, tile = c.bco, inv); break;
    case PK_X3_WIDE: p.f16 = pack_x3(c, tile = 256, inv); break;
    case PK_RGB: p.f16 = pack_x3_rgb(c, inv); tile = 64; break;
    case PK_X3F: p.f16 = pack_x3(c, tile = c.cout, inv); break;
    case PK_X3F7: p.f16 = pack_x3_f7(c, inv); tile = 32; break;
    case PK_X3P: p.f16 = pack_x3(f7_permuted(c), tile = c.bco, inv); break;
    case PK_WINO_F16: p.f16 = pack_wino_f16(c, inv); break;
#ifdef ISLPOSE_DEV
    case PK_WINO_X3: p.f16 = pack_wino_x3(c, inv); break;
#endif
  }
  if (hi_only && tile) p.f16 = pack_hi_only(p.f16, (size_t)2 * tile * 8);
  return p;
}

size_t param_pad(const PackLayer& c) {
  return (size_t)std::max((c.cout + c.bco - 1) / c.bco * c.bco, (c.cout + 255) / 256 * 256);
}

std::vector<float> build_param(const PackLayer& c, int which, size_t n) {
  if (which >= PB_BIAS_PERM) return build_param(f7_permuted(c), which - PB_BIAS_PERM, n);
  std::vector<float> out(n, 0.f);
  if (which == PB_BIAS) std::copy(c.b.begin(), c.b.end(), out.begin());
  else if (c.act == PACK_ACT_PRELU) std::copy(c.s.begin(), c.s.end(), out.begin());
  return out;
}

}  // namespace isl
