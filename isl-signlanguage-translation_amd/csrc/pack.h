// Host-only weight packing: the host view of a conv layer and the filter layouts the kernels
// read.  Pure host arithmetic, no HIP headers and no device -- tools/pack_digest.cpp and
// tests/test_pack.py hold every layout to recorded digests on the CPU.
#pragma once
#include <cstddef>
#include <vector>

namespace isl {

struct Seg {
  int logical, phys, len;  // logical input channels [logical, logical+len) live at physical offset phys
};

constexpr int PACK_ACT_PRELU = 2;     // ACT_PRELU of internal.h
constexpr int PACK_WINO_X3_BCO = 64;  // WINO_X3_BCO of internal.h

// What the packers read of a layer (ConvLayer of runtime.cpp derives from it)
struct PackLayer {
  int cin = 0, cout = 0, k = 0, act = 0;
  std::vector<float> w, b, s;
  std::vector<Seg> cmap;
  int cin_phys = 0, bco = 0;
  bool x3_wide = false;          // 1x1 layer with a second split-fp16 packing for 256-channel tiles
  int wbco = 0;                  // Winograd tile (3x3 layers), 0 = direct only
  // the fused 1x1 pair (conv_x3 VAR 16): fuse6 marks the first layer (Mconv6), fuse7 the second
  bool fuse6 = false, fuse7 = false;
};

// The filter packs of a layer; each layout is specified at its function in pack.cpp.
enum PackKind {
  PK_DIRECT,     // fp32, conv.hip
  PK_WINO,       // fp32 Winograd-transformed, wino.hip (wbco)
  PK_X3,         // split-fp16, conv_x3.hip, tiles of bco channels; its 2^s is the layer's
  PK_X3_WIDE,    // the same for 256-channel tiles (x3_wide layers; per launch, x3_wide1)
  PK_RGB,        // conv1_1: K packed as the 27 real (ky, kx, c) values
  PK_X3F,        // Mconv6 of a fused pair as one tile of all its channels (when bco < cout)
  PK_X3F7,       // Mconv7 of a fused pair in the fused K order
  PK_X3P,        // the pair's two-launch form: Mconv6 rows / Mconv7 channel map in that order
  PK_WINO_F16,   // split-fp16 Winograd filters of wino_f16.hip
#ifdef ISLPOSE_DEV
  PK_WINO_X3,    // split-fp16 Winograd filters of wino_x3.hip
#endif
  PK_COUNT
};
const char* pack_name(int kind);

// conv1_1: 3 input channels at the head of one chunk, 3x3, <= 64 outputs
bool rgb_layer(const PackLayer& c);
// The one statement of which packs a layer owns ...
bool owns_pack(const PackLayer& c, int kind);
// ... and which of them have a hi-only form (ISL_PREC_FP16: the split packs of conv_x3.hip)
bool pack_has_hi(int kind);

struct HostPack {
  std::vector<float> f32;        // PK_DIRECT, PK_WINO
  std::vector<_Float16> f16;     // every other kind
  size_t elems() const { return f32.size() + f16.size(); }
  size_t bytes() const { return f32.size() * sizeof(float) + f16.size() * sizeof(_Float16); }
  const void* data() const { return f16.empty() ? (const void*)f32.data() : (const void*)f16.data(); }
};

// The host bytes of one pack; hi_only: its hi halves alone (pack_has_hi kinds).  *inv: the 2^-s
// of a split pack (PK_RGB: the layer's, as PK_X3), 1 for the fp32 kinds.
HostPack build_pack(const PackLayer& c, int kind, bool hi_only, float* inv);

// Bias and PReLU slopes (zero without PReLU), zero-padded to n floats; *_PERM: of the fused
// pair's Mconv6 in its two-launch channel order (f7_permuted)
enum ParamBuf { PB_BIAS, PB_SLOPE, PB_BIAS_PERM, PB_SLOPE_PERM, PB_COUNT };
std::vector<float> build_param(const PackLayer& c, int which, size_t n);
// the padding that covers every tile width of the layer (c.bco; 256 for x3_wide layers)
size_t param_pad(const PackLayer& c);

int f7_logical(int phys);
PackLayer f7_permuted(const PackLayer& c);

}  // namespace isl
