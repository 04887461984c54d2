// Internal declarations shared by the libislpose translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "x3_select.h"

namespace isl {

// Activation buffer: float32 in 8-channel chunks ("NC8HW8"), with a zero ring of
// `pad` pixels around every frame, i.e. element (n, y, x, c) lives at
//   base + ((n*(cs/8) + c/8) * (H+2p) + y+p) * (W+2p) * 8 + (x+p) * 8 + c%8.
// A chunk of consecutive pixels is contiguous, so every kernel that walks pixels
// for a K step of 8 channels reads whole cache lines.  Convolutions read/write
// channel slices [coff, coff+C) (coff a multiple of 8) of such buffers, which is
// how every torch.cat of the reference becomes zero-copy.
// esize 2 (ISL_ACT_FP16, an fp16-storage arena): the same layout with fp16 elements -- `base`
// then points at _Float16 values, every element offset is unchanged.  The net input, the net
// outputs (buffers of their own there, runtime.cpp) and the split-K / fold workspaces are fp32
// in every arena; only the kernels with an fp16-storage form (ConvLaunch::act16, the *16 pool
// launches) read or write an esize-2 buffer.
struct Act {
  float* base = nullptr;
  int n = 0, H = 0, W = 0, pad = 0, cs = 0;   // cs: channel capacity, a multiple of 8
  int esize = 4;                              // bytes per element: 4 (fp32) or 2 (fp16)
  size_t chunk_elems() const { return (size_t)(H + 2 * pad) * (W + 2 * pad) * 8; }
  size_t frame_elems() const { return chunk_elems() * (cs / 8); }
  size_t bytes() const { return frame_elems() * n * (size_t)esize; }
};

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_PRELU = 2 };

// ConvLaunch (one convolution launch), X3Fold and tile_pixels live in x3_select.h: the host-only
// launch selection of the split-fp16 kernels reads them without a HIP header.

// Returns the block tile width (output channels) the conv kernels use for cout.
int conv_bco_for(int cout);
hipError_t launch_conv(const ConvLaunch& c, hipStream_t s);
// Winograd F(2x2,3x3) path for 3x3 layers: output channels per block tile
// (64 or 96), or 0 when cout does not fit one of them; `c.wpk` then holds
// the transformed filters [co_tile][chunk][xi 16][plane 2][BCO][4].
int wino_bco_for(int cout);
hipError_t launch_wino(const ConvLaunch& c, hipStream_t s);
// Split-fp16 (3 x fp16 MFMA = fp32-accurate) direct convolution (conv_x3.hip).  What a launch
// runs is x3_choose's decision (x3_select.h, with every predicate the runtime plans by); the
// launch takes the plan's choice, or makes it from the switches (isl_debug_conv, tools/convbench).
hipError_t launch_conv_x3(const ConvLaunch& c, const X3Choice& ch, const X3Switches& sw, hipStream_t s);
hipError_t launch_conv_x3(const ConvLaunch& c, const X3Switches& sw, hipStream_t s);
hipError_t launch_conv_x3_rgb(const ConvLaunch& c, hipStream_t s);
// compute units of the current device (cached; 256 where the query fails): x3_choose's `cus`
int device_cus();
// conv1_1 -> conv1_2 -> pair-max (conv_c12.hip): l1 = conv1_1 (rgb-packed wx3), l2 = conv1_2 with
// its hpool output.  f16 on both: the one-term form from the hi-only packs of both layers; act16
// on both: l2.out is an fp16 buffer (the net input stays fp32)
bool x3_c12_fits(const ConvLaunch& l1, const ConvLaunch& l2);
hipError_t launch_conv_x3_c12(const ConvLaunch& l1, const ConvLaunch& l2, hipStream_t s);
double conv_x3_c12_mfma_flops(const ConvLaunch& l1);
// Split-fp16 Winograd F(2x2,3x3) (wino_x3.hip): 3x3 layers with cout % 4 == 0;
// c.wx3 then holds the split transformed filters [co_tile][pair][xi][hi|lo][h][64][8].
hipError_t launch_wino_x3(const ConvLaunch& c, hipStream_t s);
double wino_x3_mfma_flops(const ConvLaunch& c);
constexpr int WINO_X3_BCO = 64;
// Split-fp16 Winograd F(2x2, 3x3) on 64-channel x 64-tile blocks (wino_f16.hip): 3x3 layers with
// cout % 64 == 0, no fused pool / pooled input / fold, >= 32 tiles per row, > 1024 pixels per
// frame; c.wx3 holds the pack_wino_f16 filters and c.wscale_inv their 2^-s.
bool wino_f16_fits(const ConvLaunch& c);
hipError_t launch_wino_f16(const ConvLaunch& c, hipStream_t s);
double wino_f16_mfma_flops(const ConvLaunch& c);
// FLOPs the matrix cores execute for one launch (tile padding included)
double conv_mfma_flops(const ConvLaunch& c);
double wino_mfma_flops(const ConvLaunch& c);

hipError_t launch_maxpool2(const Act& in, const Act& out, int C, hipStream_t s);
// adds 1 to *trips when *flag is set (stream-ordered range-guard count)
hipError_t launch_range_count(const int* flag, unsigned long long* trips, hipStream_t s);
// second half of a fused 2x2 max-pool: row pairs of a horizontally pooled buffer
// (ConvLaunch::hpool, [n][chunk][H][W/2][8]) into the padded next buffer
hipError_t launch_vpool2(const Act& half, const Act& out, int C, hipStream_t s);
// (both pools take fp16 buffers too -- in and out of one Act::esize; the max of roundings is
// the rounding of the max)
// range_flag: raised for an input element outside the fp16 split range (null: no check kept)
hipError_t launch_pack_nchw(const float* x, int n, int C, int h, int w, const Act& out, int* range_flag, hipStream_t s);
hipError_t launch_unpack_nchw(const Act& in, int coff, int C, float* y, hipStream_t s);
// Pre-processing of a batch of images described by a device table of entries
// (preprocess_entry: byte offset of the image in `frames`, its size, the
// resized size and 1/fx); row_bytes = bytes per row of the frame array.
hipError_t launch_preprocess_tab(const uint8_t* frames, long long row_bytes, const void* d_tab, int n,
                                 const Act& out, hipStream_t s);
size_t preprocess_entry_bytes();
void preprocess_entry(void* dst, long long off, int sh, int sw, int rh, int rw, double scale, int flip = 0);

struct MapSrc {            // one single-stage cubic resize, sampled per output element
  const float* base;       // element (f, c, y, x) at base + f*fs + chan(c) + y*ys + x*xs,
  long long fs, cstr, ys, xs;   //   chan(c) = (c >> cshift) * cbig + (c & (2^cshift - 1)) * cstr
  long long cbig;          // chunk stride of a chunked (arena) map; planar maps: cshift = 30, cbig = 0
  int cshift;
  int sh, sw;              // source size (tap clamping)
  int dh, dw;              // destination size of this resize
  double scy, scx;         // source pixels per destination pixel (1/inv_scale)
  int cn;                  // channels of the image OpenCV resized (SIMD body / tail split)
  int identity;            // dsize == ssize: plain copy
};

void set_error(const std::string& msg);


}  // namespace isl

struct isl_net;
namespace isl {
int net_kind(const isl_net* net);
int net_device(const isl_net* net);
// low-resolution output `which` (0 = out0 / PAF, 1 = out1 / heat) of the last run, as a MapSrc
int net_low_res(isl_net* net, int which, MapSrc* m);
// grow-only device scratch owned by the net (nullptr + error on failure)
void* net_scratch(isl_net* net, size_t bytes);
size_t net_scratch_size(const isl_net* net);
// streams on which isl_hand_post_crops runs its crops side by side, forked from and
// joined back into the caller's stream; a grow-only scratch per lane
constexpr int ISL_POST_LANES = 4;
struct PostLanes {
  hipStream_t stream[ISL_POST_LANES];
  hipEvent_t fork, join[ISL_POST_LANES];
  void* scratch[ISL_POST_LANES];
  size_t bytes[ISL_POST_LANES];
  // the batch's stage-1 maps (written on the caller's stream, read by the lanes): a buffer
  // of their own, released by `mid_free` (recorded on the caller's stream after the lanes
  // joined); the next writer waits on it, whatever stream it runs on
  void* mid;
  size_t mid_bytes;
  hipEvent_t mid_free;
  bool mid_used;
};
// created on first use (nullptr + error on failure), destroyed with the net
PostLanes* net_post_lanes(isl_net* net);
}  // namespace isl
