// Which kernel a split-fp16 convolution launch runs: the whole decision, in host-only code (no
// HIP headers; x3_select.cpp, as pack.cpp is).  conv_x3.hip launches what x3_choose() returns,
// the runtime plans around the same choice, and tools/x3_choice prints it without a device.
#pragma once
#include <cstddef>

namespace isl {

// One input chunk of a split-fp16 conv whose producer left split-K partial sums instead
// of its output (ConvLaunch::fold, conv_x3 VAR 8192): the consumer's staging sums them in
// range order and applies the producer's epilogue, exactly as x3_splitk_reduce would have
// (the reduce launch is skipped).  ws == nullptr: the chunk is read from the buffer.
struct X3Fold {
  const float* ws;          // partials of this chunk: + n * fstride + m * 8 + k * sstride (range k)
  long long fstride, sstride;
  const float* bias;        // 8 values of the chunk
  const float* slope;       // 8 PReLU slopes (act == ACT_PRELU)
  float scale;              // the producer's 2^-s
  int S, act, pad_;
};

// One convolution launch.
struct ConvLaunch {
  const float* in;  int in_pad, in_cs, in_coff;
  float* out;       int out_pad, out_cs, out_coff;
  const float* wpk;            // packed weights  [co_tile][chunk][ky][kx][plane][BCO][4]
  const float* bias;           // [co_tiles*BCO]
  const float* slope;          // [co_tiles*BCO] or null
  int n, H, W;
  int ks;                      // 1, 3, 7
  int cin_chunks;              // physical input channels / 8
  int cout;                    // real output channels
  int bco;                     // output channels per block tile (32, 64, 96, 128)
  int act;
  // split-fp16 path (conv_x3.hip)
  const void* wx3 = nullptr;   // pre-split weights [co_tile][pair][ky][kx][hi|lo][h][BCO][8] fp16
  float wscale_inv = 1.f;      // 2^-s, the inverse of the per-layer weight scale
  int* range_flag = nullptr;   // raised when an output leaves the fp16 split range
  // ISL_PREC_FP16: one fp16 product per MAC.  wx3 then holds the hi halves alone -- the same
  // layouts without their [hi|lo] dimension (runtime.cpp pack_hi_only) -- and the kernels
  // round the activations to fp16 once at staging; launch_conv_x3 (the fused pair included: wx3f7
  // is then the hi-only pack_x3_f7), launch_conv_x3_rgb and launch_conv_x3_c12 (both launches set it)
  int f16 = 0;
  // ISL_ACT_FP16 (with f16 only): `in` and `out` are fp16 buffers (Act::esize 2; the strides in
  // elements are the same), the staging copies the stored roundings and the epilogue stores
  // RNE(v) after its range check on the fp32 value.  launch_conv_x3_rgb reads its fp32 net input
  // as ever and writes fp16.  out32 (a layer that writes a net output): the unrounded fp32
  // values also go to channels [0, cout) of this fp32 buffer of out32_cs channels, ring out32_pad
  int act16 = 0;
  float* out32 = nullptr;
  int out32_pad = 0, out32_cs = 0;
  // split-K workspace (conv_x3 on grids too small to fill the GPU); null = no split
  float* ws = nullptr;
  size_t ws_floats = 0;
  int ksplit = 1;              // set by launch_conv_x3
  int allow_split = 0;         // the net's split-K switch (isl_net_set_split_k)
  unsigned long long* dbg = nullptr;   // development stamps (tools/convbench), never set by the runtime
  // Half of a following 2x2 max-pool (conv_x3 only, even W): the epilogue writes the
  // max of each horizontal pixel pair into `out` as an unpadded [n][chunk][H][W/2][8]
  // buffer (out_pad 0); launch_vpool2 then takes the max of row pairs.
  int hpool = 0;
  // The other half (conv_x3 only): `in` is such a pair-max buffer [n][chunk][2H][W][8] of
  // the pool whose H x W output this conv reads; its staging takes the max of each row
  // pair on the fly (the ring, in_pad wide, reads as zeros), so the pool kernel and its
  // output buffer are skipped.  in_pad / in_cs / in_coff describe the pooled buffer.
  int vin = 0;
  // Split-K fold (conv_x3 only).  fold: device table [cin_chunks] of X3Fold for this conv's
  // input chunks (a consumer); fold_out: this conv's across-block partial sums are consumed
  // by folding consumers, so its x3_splitk_reduce launch is skipped (a producer).
  const X3Fold* fold = nullptr;
  int fold_out = 0;

  // The fused 1x1 pair (conv_x3 VAR 16; Mconv6 -> Mconv7 of a stage, model.py:108-109):
  // cout7 > 0 makes this launch the pair.  The fields above describe Mconv6 (wx3 packed for a
  // tile of all its cout channels) with `out` / out_* describing Mconv7's output; these
  // describe Mconv7 (wx3f7 = pack_x3_f7, K in the order of Mconv6's accumulator registers).
  const void* wx3f7 = nullptr;
  const float* bias7 = nullptr;
  const float* slope7 = nullptr;
  float wscale7_inv = 1.f;
  int cout7 = 0, act7 = 0;
};

// Pixels per tile of the flattened-raster conv kernels: BPX, or fewer when the
// image is so narrow that a BPX-pixel tile's padded input row segment (which
// crosses up to (W+BPX-2)/W image rows, each adding 2*in_pad ring pixels) would
// overflow the kernel's LDS segment capacity `segcap`.
inline int tile_pixels(const ConvLaunch& c, int bpx, int segcap) {
  const int P = c.ks / 2;
  for (int t = bpx; t > 1; --t)
    if (t - 1 + 2 * c.in_pad * ((c.W + t - 2) / c.W) + 2 * P + 1 <= segcap) return t;
  return 1;
}

// LDS segment capacity (pixels) of a conv_x3_f16 block of bpx pixels, and of the row union
constexpr int x3_segmax(int bpx) { return bpx + 64; }
constexpr int x3_segu_max() { return 856; }

// conv1_1 of every net (conv_x3_rgb): 64 output channels, 256-pixel blocks: 3 % faster than 512
// (more blocks resident per CU), 128 lost 16 % (tools/archive/gpu_rgb_bpx.sh)
constexpr int RGB_BCO = 64, RGB_TILE = 256;

// 7x7 layers on 256-pixel tiles (8 waves of 64co x 64px, 156 KiB of LDS) or on
// 128-pixel tiles (8 waves of 64co x 32px): one block per CU either way (a step's
// weight slab is 56 KiB).  The 256-pixel block does twice the work for ~1.72x the
// time of a 128-pixel block (half the weight bytes per MFMA), so the choice is per
// launch, by grid quantisation: rounds of one block per CU, a 256-pixel block costing
// X3_WIDE7_COST 128-pixel blocks.  Both pack the weights for 128-channel tiles.
// Round 6 re-measured the three forms on the hand's batch-32 grids of C3 (op tables,
// profiles/r06/w7ab/): 69^2 x 32 ran 11.93 / 10.89 / 11.36 ms over its twenty 7x7 stage
// layers on 128 / 256 / 384 pixels (5 / 3 / 2 rounds), i.e. 1.52 and 2.38 128-pixel rounds
// per round; with the round-2 costs (1.74, 2.58; tools/archive/gpu_wide7.sh, gpu_w384.sh)
// the estimate kept 69^2 on 128 pixels.  92^2 (384) and 46^2 (384) choose as before.
constexpr double X3_WIDE7_COST = 1.52;
// a round of 384-pixel blocks (12 waves, one input buffer)
constexpr double X3_W384_COST = 2.38;

// Which conv_x3 variant a launch runs (isl_net_op_info): the template's VAR bits (1 fp16
// activation storage, 512 row
// union, 1024 in-block K ranges, 2048 split-K across blocks, 4096 two pairs per step,
// 32768 pooled-input staging, 65536 one input buffer), X3V_RGB for conv_x3_rgb, the tile
// (pixels / 32 at bits 20-24, output channels / 32 at bits 25-28) and the kernel radius
// (ks / 2) at bits 29-30.
constexpr int X3V_RGB = 1 << 18;
constexpr int X3V_FOLD_OUT = 1 << 19;   // a split-K producer whose reduce was folded into its consumers
constexpr int X3V_C12 = 4;              // conv1_1 -> conv1_2 -> pair-max in one launch (conv_c12.hip)
constexpr int X3V_W2 = 64;              // split-fp16 Winograd F(2x2, 3x3) (wino_f16.hip)
constexpr int X3V_F16 = 2;              // one-term fp16 products (ISL_PREC_FP16; a template VAR bit too)
constexpr int X3V_A16 = 1;              // reads / writes fp16 activations (ISL_ACT_FP16; a template VAR bit, with X3V_F16)

constexpr int x3_variant_code(int var, int ks, int bpx, int bco) {
  return (var & 0xfffff) | ((bpx / 32) << 20) | ((bco / 32) << 25) | ((ks / 2) << 29);
}

// The ISLPOSE_* switches of the launch selection and of the plan around it, read from the
// environment by x3_switches() alone.  A run reads them once (plan_steps); a graph's run key
// hashes the same table (x3_switch_table).
struct X3Switches {
  int deep, rgb_conv, fused_pool, pool_input, conv_staging, tiles_small, union_mode, half64, wide7, across, s8,
      fuse67, g2, px64, halfsmall, wr, wr_wn, c12, tail, small7, w2, s7w96, a16_dma;
  // read in development builds only (ISLPOSE_DEV); their defaults elsewhere
  int halfco, pps2, m16, x3_wino, abl, fold;
};
struct X3SwitchDef {
  const char* name;
  int X3Switches::*field;
  int def;             // the value when the variable is unset or has none of `first`
  const char* first;   // the first characters that count: a digit is its value, a letter is 1;
                       // null: any value, through atoi
  bool run_key;        // hashed into a graph's run key (name=value, in table order)
};
const X3SwitchDef* x3_switch_table(int* count);
X3Switches x3_switches();

// What launch_conv_x3 runs for a launch.
struct X3Choice {
  enum Family {
    NONE,      // no kernel: `error` says why
    F16,       // conv_x3_f16<ks, waves_m, waves_n, wm, wn, var, occ>
    FUSED67,   // the same kernel's VAR 16 instances: the fused 1x1 pair (ConvLaunch::cout7)
    WR,        // conv_x3_wr<ks, wn, depth, f16>
    RGB,       // conv_x3_rgb<bpx, f16, act16>
  };
  Family family = NONE;
  const char* error = nullptr;
  int ks = 0, waves_m = 0, waves_n = 0, wm = 0, wn = 0, occ = 0, depth = 0;
  int var = 0;                  // with the form bits (X3V_F16, X3V_A16) of the launch
  int S = 1;                    // K ranges
  bool across_blocks = false;   // ... each in a block of its own (split-K, or the waves of conv_x3_wr)
  int bpx = 0;                  // pixels per block tile
  size_t ws_floats = 0;         // split-K workspace the launch needs
  bool act16 = false;           // the run may plan this launch on fp16 buffers (x3_act16_ok)
  double mfma_flops = 0.0;      // tile padding included
  int code = 0;                 // x3_variant_code
};
// cus: the device's compute units (conv_x3.hip device_cus), the only thing taken from the device
X3Choice x3_choose(const ConvLaunch& c, int cus, const X3Switches& sw);
X3Choice x3_choose_rgb(const ConvLaunch& c);
// The forms csrc/x3_instances.h builds of a choice's kernel (1 three-term, 2 one-term, 4 fp16
// storage); 0: no such instance
int x3_instance_forms(const X3Choice& ch);

// Tail tiles of a chip-filling grid of full tiles (x3_select.cpp)
struct X3Tail {
  int nb_full = 0, full_tiles = 0, tail_tiles = 0, ttpx = 0, nblocks = 0;
};
X3Tail x3_tail_plan(int n, int HW, int co_tiles, int px_tiles, int tpx, int nblocks, int cus, const X3Switches& sw);

// Split-fp16 (3 x fp16 MFMA = fp32-accurate) direct convolution: same tiles as
// launch_conv; x3_fits() says whether the input segment of a pixel tile fits.
bool x3_fits(const ConvLaunch& c);
// 1x1 layers with x3_wide1_layer() also carry filters packed for 256-channel tiles,
// used for a launch when x3_wide1(c with bco 256) says its grid is big enough.
bool x3_wide1_layer(int ks, int cout, int cin_phys);
bool x3_wide1(const ConvLaunch& c, int cus, const X3Switches& sw);
// whether launch_conv_x3 has a pooled-input (ConvLaunch::vin) variant for this launch
bool x3_vin_ok(const ConvLaunch& c, int cus, const X3Switches& sw);
// conv1_1 (3 input channels in one chunk, 3x3, <= 64 outputs): K packed as the 27
// real (ky, kx, c) values; c.wx3 then holds the pack_x3_rgb filters [kk][hi|lo][h][64][8].
bool x3_rgb_fits(const ConvLaunch& c);
// whether launch_conv_x3 would run c (f16 set, the fields as at its launch) on a kernel with an
// fp16-storage form (ConvLaunch::act16): every one-term conv_x3_f16 variant (the fused 1x1 pair
// included) x3_instances.h lists with that form; not the wave-range kernel
bool x3_act16_ok(const ConvLaunch& c, int cus, const X3Switches& sw);
// whether launch_conv_x3 can run c with hpool (even W, not split across blocks)
bool x3_hpool_ok(const ConvLaunch& c, int cus, const X3Switches& sw);
double conv_x3_mfma_flops(const ConvLaunch& c, int cus, const X3Switches& sw);
double conv_x3_rgb_mfma_flops(const ConvLaunch& c);
// whether launch_conv_x3 has a fused-pair variant for a 1x1 layer of cout6 outputs followed by
// a 1x1 layer of cout7 outputs reading all of them (VAR 16)
bool x3_fused67_fits(int cout6, int cout7);
// whether a fusable pair's launch has the grid for the fused kernel (else two launches)
bool x3_fused67_grid(const ConvLaunch& c, int cus);
// MFMA FLOPs a fused-pair launch executes (both layers, tile padding included)
double conv_x3_fused67_mfma_flops(const ConvLaunch& c, int cus, const X3Switches& sw);
// floats of split-K workspace launch_conv_x3 would use for c (0 = no split)
size_t x3_splitk_ws_floats(const ConvLaunch& c, int cus, const X3Switches& sw);
// K ranges launch_conv_x3 would use for c: S, and whether they run across blocks (split-K
// through the workspace) -- the producers a consumer can fold
int x3_split_ranges(const ConvLaunch& c, bool* across_blocks, int cus, const X3Switches& sw);
// whether launch_conv_x3 would run c on its generic loop (the loop that can fold)
bool x3_fold_ok(const ConvLaunch& c, int cus, const X3Switches& sw);

}  // namespace isl
