// 3x3 convolution (stride 1, pad 1) as Winograd F(2x2, 3x3) on the gfx950 FP16 matrix
// cores with split-fp16 (x3) products: the fp32-accurate arithmetic of conv_x3.hip on the
// 16 Winograd GEMMs, for the 3x3 layers of src/model.py:25-64 (make_layers /
// make_layers_Mconv) on chip-filling grids.
//
//   U = G g G^T   per (co, ci), host, double, x 2^s, split hi + lo     (pack_wino_f16)
//   V = B^T d B   per (tile, ci), in the kernel from the staged input, fp32, then split
//   M[xi] = sum_ci U[xi][co][ci] V[xi][ci][tile]   16 GEMMs, 3 fp16 MFMAs per product
//   Y = A^T M A   the 2x2 outputs of a tile, x 2^-s + bias, activation, range check
//
// 16 products per 2x2 outputs instead of 36: 2.25x fewer MFMAs than conv_x3_f16.  The
// transforms are exact-coefficient (0, +-1 for B and A; G's 1/2 in double on the host), so
// the accuracy class is that of conv_x3 (rel err ~1e-6 vs the fp64 forward).
//
// Round 1's split-fp16 Winograd (wino_x3.hip, development build) lost 1.3-1.8x: 4 waves
// of 64 channels computed all 16 V values of a tile per thread (184 VALU per (tile, channel),
// redone for every 64-channel block) into a single-buffered 128 KB step.  This kernel is built
// the other way round, so that no operand of the K loop is shared through LDS except the raw
// input:
//
//   * Block = 8 waves (512 threads, one block per CU, two waves per SIMD) for 64 output channels
//     x 64 tiles x all 16 GEMMs.  Wave w owns the two GEMMs xi0 = 4 r + 2 cp, xi1 = xi0 + 1
//     (r = w >> 1 a row of V, cp = w & 1 a column pair): 2 x 2 x 2 accumulator tiles of 32 x 32,
//     128 registers.  U[xi0], U[xi1] of the block are used by that wave alone, so its A fragments
//     go straight from L2 into registers (8 x 16 B per lane and K step, loaded one step ahead
//     into the other of two register sets by counted inline-asm loads) -- no LDS, no barrier for
//     the filters.
//   * V[xi0], V[xi1] are also used by that wave alone: the wave builds its B fragments itself
//     from the staged fp32 input.  B^T's rows have two nonzeros each, so a row of V is the
//     combination t[col] = d[ra][col] + sr d[rb][col] (sr = +-1), shared by the pair over three
//     column slots: V(xi0) = tX - tY, V(xi1) = tY + sz tZ -- 6 pixels, 3 + 2 packed fma per
//     4 channels for the two values, then the split (v_cvt_pk_f16_f32 + v_fma_mix, 1.5 VALU per
//     value).  sr and sz are wave-uniform and sit in scalar register pairs.
//   * The raw input of a K step (a chunk pair) arrives by LDS-DMA into a ring of three slots, two
//     steps ahead, one barrier per step.  The block's 64 tiles are consecutive in "band order" (a
//     band = two tile rows, walked column-pair by column-pair), so they touch at most two bands
//     and the staged run is 6 rows x (64 + 4) columns whatever the image width (26 KB per step).
//     Layout [chunk half h][channel quad q][row 6][column parity][34] x 16 B: the lanes of
//     a wave (consecutive band slots) read ds_read_b128s (lane pairs 2k, 2k+1 differ by two
//     rows = 32 banks, lane pairs by 16 B).
//   * A K step is four groups (tile half j, channel quad Q) of six ds_read_b128, 22 VALU and,
//     behind each Q = 1 group, the 12 MFMAs of j.  The reads run one group ahead of their use:
//     the first group's at the top of the step; the
//     next group's as soon as the current group's row combinations are formed and its 24 raw
//     registers are free.  Reads and their waits are inline asm, tied by operands to the work
//     they stand behind, so the wait of a group finds its pixels landed behind the previous
//     group's splits and MFMAs instead of straight behind the reads (what hipcc places).
//   * The step's 12 vector-memory instructions (8 filter loads of pair k + 1, 4 DMA pieces of pair
//     k + 2) are spread over the step, one at a time, each inline asm tied between two neighbours:
//     two filter loads behind the splits of group (0, 0), four behind every second MFMA of the
//     j = 0 burst, two behind the splits of group (1, 0), the four pieces behind every third MFMA
//     of the j = 1 burst.  Issued together at the top of the step, behind the barrier, they cost
//     the eight waves 750-1700 cycles of issue before the first VALU (a quarter of the step,
//     DESIGN 4.3j).  The filter loads write the idle register set; the counted waits are
//     vmcnt(6) in front of the first MFMA and vmcnt(12) in front of the barrier.
//   * Epilogue: the waves' M tiles meet in LDS (two rounds of 32 channels, 128 KB), one
//     thread per (4 channels, tile) sums them in a fixed order into the 2x2 outputs.
//
// Per K step and CU (8 waves of 24 MFMAs): 1536 MFMA cycles per SIMD, 192 KB of LDS reads
// (24 ds_read_b128 per wave), ~130 VALU per wave and 64 KB of filters + 26 KB of input from
// L2.  242 VGPRs, no spills, two waves per SIMD.  Eligible launches (wino_f16_fits): 3x3,
// cout % 64 == 0, no fused pool or pooled-input staging, at least 32 tiles per row and > 1024
// pixels per frame (no canonical K ranges: those layers keep conv_x3's batch-invariant sums).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "internal.h"

namespace isl {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct W2Args {
  const float* in;
  float* out;
  const f16x8* upk;             // [co_block][pair][xi][i 2][hi|lo][h][32] x 8 fp16 (pack_wino_f16)
  const float* bias;
  const float* slope;
  int* range_flag;
  unsigned long long* dbg;      // STAMP (development): block 0's s_memtime segment sums, [wave 8][8]
  long long in_fs, in_chs, out_fs, out_chs;   // frame / chunk strides (floats)
  float wscale_inv;             // 2^-s
  int in_pad, out_pad, H, W, TH, TW, pairs, cin_chunks, co_blocks, bpf, act, nblocks;
};

constexpr int RS = 34;                  // 16-byte units per staged (row, column parity): 68 columns
constexpr int QS = 6 * 2 * RS;          // per (chunk half, channel quad): 6 rows x 2 parities
constexpr int HS = 13 * 64;             // per chunk half: 2 quads (816 units) in 13 whole DMA pieces
constexpr int BUF = 32 * 64;            // 2048 units (32 KiB): 32 DMA pieces of 64 units, 2 per wave

// v = hi + lo for 4 fp32 values as dwords of 2 fp16 each (h01 = hi of v.x, v.y; ...): hi by the
// packed RNE conversion, lo = (f16)(v - (f32)hi) in one v_fma_mix per value (-1 * hi + v: the
// difference is exact in fp32, Sterbenz), written straight into its half of the dword -- the bits of
// conv_x3's x3_split8 in 1.5 instead of 3 VALU per value and no repacking moves.
__device__ __forceinline__ void split_dw(const f32x4& v, unsigned& h01, unsigned& h23, unsigned& l01, unsigned& l23) {
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h01) : "v"(v.x), "v"(v.y));
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h23) : "v"(v.z), "v"(v.w));
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l01) : "v"(h01), "v"(v.x));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l01) : "v"(h01), "v"(v.y));
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l23) : "v"(h23), "v"(v.z));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l23) : "v"(h23), "v"(v.w));
}

// the six raw pixels (4 channels each) of one (tile half, channel quad): rows ra / rb x column slots X, Y, Z
struct W2Raw {
  f32x4 aX, aY, aZ, bX, bY, bZ;
};
// s * b + a with the +-1 multiplier s in a scalar register pair: the v_pk_fma_f32 of the vector form
__device__ __forceinline__ f32x2 pk_fma_s(unsigned long long s, f32x2 b, f32x2 a) {
  f32x2 d;
  asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "s"(s), "v"(b), "v"(a));
  return d;
}
__device__ __forceinline__ f32x2 lo2(const f32x4& v) { return f32x2{v.x, v.y}; }
__device__ __forceinline__ f32x2 hi2(const f32x4& v) { return f32x2{v.z, v.w}; }

// ABL (development build only, tools/convbench "w2" with ISLPOSE_W2_ABL): timing ablations --
// 1 no MFMAs, 2 no transform (no raw LDS reads, no VALU; constant B), 4 no filter loads, 8 no
// raw-input DMA, 16 no epilogue (the accumulators are folded into one store so that nothing
// upstream is dead code), 32 (on the PF = 1 loop) no raw LDS reads (the transform's VALU and the
// MFMAs stay; the pixels come from registers the compiler cannot fold -- what the reads' round
// trips cost); 64 + k (k = 1, 4, 8, 12, 16) ablation k on the PF = 1 loop.  Wrong results;
// libislpose.so has ABL = 0 only.
// PF: 1 = the raw pixels of a channel quad are read one quad ahead (below), 0 = read where they are
// used (the development build's reference for interleaved A/B runs).
// MV (PF = 1): where a K step issues its 12 vector-memory instructions, the 8 filter loads of pair
// k + 1 and the 4 DMA pieces of pair k + 2 (w2_slot below).  0 = all at the top of the step, behind
// the first group's reads (the loop before; development build, tools/convbench "w2t"); 1 = the
// filter loads behind the first eight MFMAs of the j = 0 burst, the pieces behind every second
// MFMA of the j = 1 burst; 2 = spread over the whole step: two filter loads behind the splits of
// each Q = 0 group, four in the j = 0 burst, the pieces in the j = 1 burst; 3 = two pieces behind
// the splits of each Q = 0 group, four filter loads in each burst.  libislpose.so has W2_MV only.
// STAMP (development build, tools/convbench with CONVBENCH_W2STAMP=1): s_memtime stamps at eight
// points of the K step, summed per segment in scalar registers; block 0 stores its sums once,
// behind the loop.  The stamps fence the scheduler and drain the LDS reads in flight: read the
// segments' differences between builds, not the run time.
constexpr int W2_MV = 2;
// what stands behind MFMA m (0 .. 11) of burst j: -1 nothing, 0 .. 7 filter load n, 8 + e DMA piece e
constexpr int w2_slot(int mv, int j, int m) {
  if (mv == 1) return j == 0 ? (m < 8 ? m : -1) : (m < 8 && m % 2 == 0 ? 8 + m / 2 : -1);
  if (mv == 2) return j == 0 ? (m < 8 && m % 2 == 0 ? 2 + m / 2 : -1) : (m % 3 == 0 ? 8 + m / 3 : -1);
  if (mv == 3) return m < 8 && m % 2 == 0 ? 4 * j + m / 2 : -1;
  return -1;
}
// what stands behind split s (0, 1) of the Q = 0 group of tile half j
constexpr int w2_gslot(int mv, int j, int s) { return mv == 2 ? 6 * j + s : mv == 3 ? 8 + 2 * j + s : -1; }
// The counted waits (derivation at the K loop).  In front of the first MFMA, A(k) landed: the
// vector-memory instructions younger than A(k)'s last load.  In front of the barrier, raw(k+1)
// landed: those younger than its last piece.  MV 3 ends a step with filter loads, so its pieces have
// four more behind them, and its prologue has to drain (there raw(1) has nothing behind it).
constexpr int w2_wait_a(int mv) { return mv == 0 ? 16 : mv == 1 ? 4 : mv == 2 ? 6 : 2; }
constexpr int w2_wait_raw(int mv) { return mv == 3 ? 16 : 12; }
template <int ABL, int PF, int MV = W2_MV, bool STAMP = false>
__global__ void __launch_bounds__(512, 1) wino_f16(W2Args a) {
  static_assert(PF == 1 || (MV == 0 && !STAMP), "the issue placements and the stamps are those of the PF = 1 loop");
  // [0, 3 BUF): the raw-input ring; [0, 8192): the M exchange of the epilogue; then the epilogue's
  // bias and PReLU slopes (64 + 64 floats)
  __shared__ f32x4 smem[8192 + 32];

  // XCD-aware order (conv_x3): the channel blocks of a tile block, then neighbouring tile
  // blocks, on one XCD, so the staged input is read from one L2
  int bid = blockIdx.x;
  {
    const int nb = a.nblocks, q = nb >> 3, r = nb & 7, xcd = bid & 7, k = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  const int co_b = bid % a.co_blocks;
  const int rest = bid / a.co_blocks;
  const int fb = rest % a.bpf;
  const int n = rest / a.bpf;

  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

  // the epilogue's bias and slopes, staged once (read after the K loop's last barrier)
  if (tid < 64) {
    float* eb = (float*)(smem + 8192);
    eb[tid] = a.bias[co_b * 64 + tid];
    eb[64 + tid] = a.act == ACT_PRELU ? a.slope[co_b * 64 + tid] : 0.f;
  }

  // the block's 64 band slots s0 .. s0 + 63: band b = tile rows 2b, 2b + 1; slot u of a band =
  // tile (2b + (u & 1), u >> 1).  They lie in band ba and, past its end, in band bb = ba + 1
  // (TW >= 32); segment 0 = band ba's columns from txlo0, segment 1 = band bb's from 0
  const int BW = 2 * a.TW, s0 = fb * 64;
  const int ba = s0 / BW, bb = (s0 + 63) / BW;
  const bool two = bb > ba;
  const int txlo0 = (s0 - ba * BW) >> 1;
  const int txhi0 = two ? a.TW - 1 : (s0 + 63 - ba * BW) >> 1;
  const int w0 = 2 * (txhi0 - txlo0 + 1) + 2;                    // staged columns of segment 0
  const int w1 = two ? 2 * (((s0 + 63 - bb * BW) >> 1) + 1) + 2 : 0;
  const int Hp = a.H + 2 * a.in_pad, Wp = a.W + 2 * a.in_pad;
  const float* in_f = a.in + (size_t)n * a.in_fs;

  // Raw-input pieces of this wave: p = w + 8 e (e < 4), 64 units each.  Piece p stages chunk half
  // hp = p / 13 of the pair (13 pieces = 832 units per half: [q][row 6][parity][34] + 16 spare);
  // pieces 26 .. 31 are spare (they reload pixel 0 into the buffer's tail).  Lane unit -> (q, row,
  // parity, half column) -> the padded input pixel; rows / columns past the buffer, which only
  // feed discarded outputs, are clamped.  The chunk is wave-uniform: a uniform base plus a
  // 32-bit lane offset.
  unsigned doff[4];
  int dch[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int p = w + 8 * e;
    const int hp = p < 26 ? p / 13 : 0;
    const int u = (p - 13 * hp) * 64 + lane;             // unit within the half's region
    int t = u / RS;
    const int hc = u - t * RS;
    const int par = t & 1;
    t >>= 1;
    const int row = t % 6;
    const int qq = t / 6;
    const int v = 2 * hc + par;
    const bool s1 = v >= w0;
    const int vl = s1 ? v - w0 : v;
    const bool ok = p < 26 && qq < 2 && vl < (s1 ? w1 : w0);
    const int band = s1 ? bb : ba, txlo = s1 ? 0 : txlo0;
    const int rp = min(4 * band - 1 + row + a.in_pad, Hp - 1);
    const int cp = min(2 * txlo - 1 + vl + a.in_pad, Wp - 1);
    doff[e] = ok ? (unsigned)((rp * Wp + cp) * 8 + qq * 4) * 4u : 0u;   // bytes (< 2^32: wino_f16_fits)
    dch[e] = __builtin_amdgcn_readfirstlane(hp);
  }

  // This wave's two GEMMs: xi0 = 4 r + 2 cp, xi1 = xi0 + 1 (one row r of V, a column pair).
  // V[r][c] = (d[ra][ca] + sc d[ra][cb]) + sr (d[rb][ca] + sc d[rb][cb]); B^T rows: d0 - d2,
  // d1 + d2, d2 - d1, d1 - d3.  The row combination t[col] = d[ra][col] + sr d[rb][col] is
  // shared by the pair, over three column slots X, Y, Z: V(xi0) = tX - tY, V(xi1) = tY + sz tZ
  // (cp 0: columns 0, 2, 1, sz = +1 -- d0 - d2, d2 + d1; cp 1: columns 2, 1, 3, sz = -1 --
  // d2 - d1, d1 - d3): 6 pixels, 3 + 2 fma per channel for the two values, no selects.
  const int wr = w >> 1, cpr = w & 1;
  const int ra = wr == 0 ? 0 : wr == 2 ? 2 : 1, rb = wr == 3 ? 3 : wr == 2 ? 1 : 2;
  const float sr = wr == 1 ? 1.f : -1.f, sz = cpr ? -1.f : 1.f;
  const f32x4 srv = f32x4{sr, sr, sr, sr}, szv = f32x4{sz, sz, sz, sz};
  // PF: the +-1 multipliers as scalar register pairs (wave-uniform), operands of v_pk_fma_f32
  const unsigned sru = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, sr));
  const unsigned szu = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, sz));
  const unsigned long long sr2 = (unsigned long long)sru << 32 | sru, sz2 = (unsigned long long)szu << 32 | szu;
  const unsigned lds0 = (unsigned)(__UINTPTR_TYPE__)(__attribute__((address_space(3))) void*)smem;
  const int cX = cpr ? 2 : 0, cY = cpr ? 1 : 2, cZ = cpr ? 3 : 1;
  auto toff = [&](int row, int col) { return (row * 2 + (col & 1)) * RS + (col >> 1); };
  const int to_aX = toff(ra, cX), to_aY = toff(ra, cY), to_aZ = toff(ra, cZ);
  const int to_bX = toff(rb, cX), to_bY = toff(rb, cY), to_bZ = toff(rb, cZ);
  // per tile tile j the lane's unit base in a raw buffer (chunk half h, quad 0, row 2 typ, parity 0)
  int tb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int s = s0 + 32 * j + l32;
    const int band = s / BW, u = s - band * BW, tx = u >> 1, typ = u & 1;
    const int hc0 = band > ba ? (w0 >> 1) + tx : tx - txlo0;
    tb[j] = h * HS + 2 * typ * 2 * RS + hc0;
  }

  // Filters U[co_b][pair k][xi][i][hi|lo][h][32 co]: this wave's xi0 and xi1 are 8 contiguous
  // 1 KiB pieces (xi, i, hi|lo); lane offset h * 32 + co.  Loaded by inline asm (so the
  // compiler, which drains every outstanding load at the first use of an ordinary load while a
  // LDS-DMA is in flight, does not see them) and waited for with counted vmcnt below.
  const unsigned uvoff = (unsigned)lane * 16;
  auto load_a = [&](f16x8 (&A)[2][2][2], int k) __attribute__((always_inline)) {
    if constexpr ((ABL & 4) != 0) return;
    const f16x8* u0 = a.upk + ((size_t)(co_b * a.pairs + k) * 16 + 4 * wr + 2 * cpr) * 256;
    const f16x8* u1 = u0 + 256;
    asm volatile(
        "global_load_dwordx4 %0, %8, %9 offset:0\n\t"
        "global_load_dwordx4 %1, %8, %9 offset:1024\n\t"
        "global_load_dwordx4 %2, %8, %9 offset:2048\n\t"
        "global_load_dwordx4 %3, %8, %9 offset:3072\n\t"
        "global_load_dwordx4 %4, %8, %10 offset:0\n\t"
        "global_load_dwordx4 %5, %8, %10 offset:1024\n\t"
        "global_load_dwordx4 %6, %8, %10 offset:2048\n\t"
        "global_load_dwordx4 %7, %8, %10 offset:3072"
        : "=v"(A[0][0][0]), "=v"(A[0][0][1]), "=v"(A[0][1][0]), "=v"(A[0][1][1]), "=v"(A[1][0][0]),
          "=v"(A[1][0][1]), "=v"(A[1][1][0]), "=v"(A[1][1][1])
        : "v"(uvoff), "s"(u0), "s"(u1)
        : "memory");
  };
  // the raw input of pair k into ring slot sl (4 pieces of 64 units; counted by vmcnt)
  auto dma = [&](int k, int sl) __attribute__((always_inline)) {
    if constexpr ((ABL & 8) != 0) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ch = min(2 * k + dch[e], a.cin_chunks - 1);   // a missing odd chunk: zero filters
      const float* src = in_f + (size_t)ch * a.in_chs;
      unsigned d = doff[e];
      asm volatile("" : "+v"(d));   // widened per use: four registers across the loop, not eight
      __builtin_amdgcn_global_load_lds((const void*)((const char*)src + (size_t)d),
                                       (__attribute__((address_space(3))) void*)(smem + sl * BUF + (w + 8 * e) * 64),
                                       16, 0, 0);
    }
  };

  // MV != 0: one vector-memory instruction of the step, n = 0 .. 7 filter load n of pair k1 into
  // the idle register set (xi = n >> 2, i, hi|lo), n = 8 + e DMA piece e of pair k2 into ring slot
  // sl.  t0, t1 are in-out operands the asm does not touch: the values it has to stand behind and
  // in front of (the accumulator of the MFMA before it and of the one after it, or a split's
  // fragment dwords).  The DMA is asm as well (M0 = the piece's LDS address), so that it stays put.
  auto vmem1 = [&](auto nc, f16x8 (&An)[2][2][2], int k1, int k2, int sl, auto& t0, auto& t1) __attribute__((always_inline)) {
    constexpr int n = decltype(nc)::value;
    if constexpr (n < 0) {
    } else if constexpr (n < 8) {
      if constexpr ((ABL & 4) != 0) return;
      const f16x8* u = a.upk + ((size_t)(co_b * a.pairs + k1) * 16 + 4 * wr + 2 * cpr + (n >> 2)) * 256;
      asm volatile("global_load_dwordx4 %0, %3, %4 offset:%5"
                   : "=v"(An[n >> 2][(n >> 1) & 1][n & 1]), "+v"(t0), "+v"(t1)
                   : "v"(uvoff), "s"(u), "n"((n & 3) * 1024)
                   : "memory");
    } else {
      if constexpr ((ABL & 8) != 0) return;
      constexpr int e = n - 8;
      const int ch = min(2 * k2 + dch[e], a.cin_chunks - 1);
      const float* src = in_f + (size_t)ch * a.in_chs;
      const unsigned dv = doff[e];
      const unsigned m0v = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(sl * BUF + (w + 8 * e) * 64) * 16u);
      asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %4"
                   : "+v"(t0), "+v"(t1)
                   : "v"(dv), "s"(m0v), "s"(src)
                   : "memory");   // (M0 is a reserved register: hipcc sets it in front of each use of its own)
    }
  };
  // STAMP: segment i = the time from the stamp before it (in program order) to stamp i
  unsigned long long tsum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
  auto stamp = [&](int i) __attribute__((always_inline)) {
    if constexpr (STAMP) {
      __builtin_amdgcn_sched_barrier(0);
      unsigned long long t;
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
      if (i >= 0) tsum[i] += t - tprev;
      tprev = t;
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  f32x16 acc[2][2][2];   // [xi][i][j]
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[x][i][j][r] = 0.f;
  // Range: V = B^T d B reaches 4 x the input, so inputs below 65504 can give |V| >= 65520.  Such
  // a V splits to hi = +-inf and lo = v - hi = -+inf; the three products hi Uhi + lo Uhi + hi Ulo
  // are inf - inf (0 inf for a zero filter), so every output fed by that V is NaN, for every
  // output channel.  A ReLU would store that NaN as 0: the epilogue therefore tests the value
  // before the activation for NaN / inf and the stored value for its magnitude, and either
  // raises the range flag (the host then recomputes on the fp32 kernels).  |V| in [65504, 65520)
  // splits exactly.

  // PF = 1: the K step's four (tile half j, channel quad Q) groups in the order (0, 0), (0, 1),
  // (1, 0), (1, 1), the same V values, splits and MFMAs as below in the same order.  The six
  // ds_read_b128 of a group are issued one group ahead: those of (0, 0) at the top of the step,
  // in front of the step's filter loads and DMA; those of group g + 1 as soon as the row
  // combinations t of group g are formed and its raw registers are dead, so that they land behind
  // group g's differences and splits and, after a Q = 1 group, behind the 12 MFMAs of j.  Reads
  // and waits are inline asm (the compiler would put s_waitcnt lgkmcnt(0) straight behind each
  // read); one group is outstanding at a wait, so its count is 0.  Every read of a step has landed
  // before the step's barrier: the ring's hazards are those of PF = 0.
  const unsigned oaX = lds0 + 16 * to_aX, oaY = lds0 + 16 * to_aY, oaZ = lds0 + 16 * to_aZ;
  const unsigned obX = lds0 + 16 * to_bX, obY = lds0 + 16 * to_bY, obZ = lds0 + 16 * to_bZ;
  // t: the issuing group's six row combinations, input operands of the reads' asm (which does not
  // use them), so that the reads stand behind them (null at the step's top)
  auto rd = [&](W2Raw& r, int sl, int j, auto qc, f32x2* t) __attribute__((always_inline)) {
    constexpr int OFF = decltype(qc)::value * QS * 16;
    if constexpr ((ABL & 32) != 0) {
      // whatever the 24 registers hold (earlier pixels and fragments): no read, nothing to fold
      asm volatile("" : "=v"(r.aX), "=v"(r.bX), "=v"(r.aY), "=v"(r.bY), "=v"(r.aZ), "=v"(r.bZ));
      return;
    }
    unsigned b = (unsigned)(tb[j] + sl * BUF) * 16;
    asm volatile("" : "+v"(b));   // the pixel addresses are formed per group (not held across it)
    const unsigned paX = b + oaX, paY = b + oaY, paZ = b + oaZ, pbX = b + obX, pbY = b + obY, pbZ = b + obZ;
#define W2_READS                           \
  "ds_read_b128 %0, %6 offset:%12\n\t"     \
  "ds_read_b128 %1, %7 offset:%12\n\t"     \
  "ds_read_b128 %2, %8 offset:%12\n\t"     \
  "ds_read_b128 %3, %9 offset:%12\n\t"     \
  "ds_read_b128 %4, %10 offset:%12\n\t"    \
  "ds_read_b128 %5, %11 offset:%12"
    if (t)
      asm volatile(W2_READS
                   : "=&v"(r.aX), "=&v"(r.bX), "=&v"(r.aY), "=&v"(r.bY), "=&v"(r.aZ), "=&v"(r.bZ)
                   : "v"(paX), "v"(pbX), "v"(paY), "v"(pbY), "v"(paZ), "v"(pbZ), "n"(OFF), "v"(t[0]), "v"(t[1]),
                     "v"(t[2]), "v"(t[3]), "v"(t[4]), "v"(t[5])
                   : "memory");
    else
      asm volatile(W2_READS
                   : "=&v"(r.aX), "=&v"(r.bX), "=&v"(r.aY), "=&v"(r.bY), "=&v"(r.aZ), "=&v"(r.bZ)
                   : "v"(paX), "v"(pbX), "v"(paY), "v"(pbY), "v"(paZ), "v"(pbZ), "n"(OFF)
                   : "memory");
#undef W2_READS
  };
  // An, k1, k2, sl2 (MV != 0): the idle filter register set and what the step loads -- the filters
  // of pair k1 into An, the raw input of pair k2 into ring slot sl2
  auto compute_pf = [&](f16x8 (&A)[2][2][2], int sl, W2Raw r, f16x8 (&An)[2][2][2], int k1, int k2, int sl2) __attribute__((always_inline)) {
    unsigned Bd[2][2][4];   // [xi][hi|lo] x 4 dwords, quad Q in dwords 2Q, 2Q + 1
    auto group = [&](auto jc, auto qc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value, Q = decltype(qc)::value;
      // The wait for this group's pixels.  Its in-out operands keep it behind the work the reads
      // are meant to land behind (the asm does not touch them): after a Q = 0 group that group's
      // eight fragment dwords, after a Q = 1 group the first two accumulators of its MFMAs (six of
      // the twelve; the other six may run beside this group's VALU).
      if constexpr ((ABL & 32) != 0) {
      } else if constexpr (j == 0 && Q == 0) {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(r.aX), "+v"(r.bX), "+v"(r.aY), "+v"(r.bY), "+v"(r.aZ), "+v"(r.bZ)
                     :
                     : "memory");
      } else if constexpr (Q == 1) {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(r.aX), "+v"(r.bX), "+v"(r.aY), "+v"(r.bY), "+v"(r.aZ), "+v"(r.bZ), "+v"(Bd[0][0][0]),
                       "+v"(Bd[0][0][1]), "+v"(Bd[0][1][0]), "+v"(Bd[0][1][1]), "+v"(Bd[1][0][0]), "+v"(Bd[1][0][1]),
                       "+v"(Bd[1][1][0]), "+v"(Bd[1][1][1])
                     :
                     : "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(r.aX), "+v"(r.bX), "+v"(r.aY), "+v"(r.bY), "+v"(r.aZ), "+v"(r.bZ), "+v"(acc[0][0][0]),
                       "+v"(acc[0][1][0])
                     :
                     : "memory");
      }
      f32x2 t[6];
      t[0] = pk_fma_s(sr2, lo2(r.bX), lo2(r.aX)), t[1] = pk_fma_s(sr2, hi2(r.bX), hi2(r.aX));
      t[2] = pk_fma_s(sr2, lo2(r.bY), lo2(r.aY)), t[3] = pk_fma_s(sr2, hi2(r.bY), hi2(r.aY));
      t[4] = pk_fma_s(sr2, lo2(r.bZ), lo2(r.aZ)), t[5] = pk_fma_s(sr2, hi2(r.bZ), hi2(r.aZ));
      // the next group's reads, into the raw registers that died just above
      if constexpr (Q == 0) rd(r, sl, j, std::integral_constant<int, 1>{}, t);
      else if constexpr (j == 0) rd(r, sl, 1, std::integral_constant<int, 0>{}, t);
      // nothing of the group's remaining work (nor its MFMAs) is scheduled in front of the reads
      if constexpr (j == 0 || Q == 0) __builtin_amdgcn_sched_barrier(0);
      const f32x2 v00 = t[0] - t[2], v01 = t[1] - t[3];
      const f32x2 v10 = pk_fma_s(sz2, t[4], t[2]), v11 = pk_fma_s(sz2, t[5], t[3]);
      split_dw(f32x4{v00.x, v00.y, v01.x, v01.y}, Bd[0][0][2 * Q], Bd[0][0][2 * Q + 1], Bd[0][1][2 * Q], Bd[0][1][2 * Q + 1]);
      split_dw(f32x4{v10.x, v10.y, v11.x, v11.y}, Bd[1][0][2 * Q], Bd[1][0][2 * Q + 1], Bd[1][1][2 * Q], Bd[1][1][2 * Q + 1]);
      if constexpr (Q == 0 && MV != 0) {
        // behind the group's two splits (tied to their hi dwords)
        vmem1(std::integral_constant<int, w2_gslot(MV, j, 0)>{}, An, k1, k2, sl2, Bd[0][0][0], Bd[0][0][1]);
        vmem1(std::integral_constant<int, w2_gslot(MV, j, 1)>{}, An, k1, k2, sl2, Bd[1][0][0], Bd[1][0][1]);
      }
      if constexpr (Q == 1) {
        f16x8 Bh[2], Bl[2];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
          Bh[x] = __builtin_bit_cast(f16x8, u32x4{Bd[x][0][0], Bd[x][0][1], Bd[x][0][2], Bd[x][0][3]});
          Bl[x] = __builtin_bit_cast(f16x8, u32x4{Bd[x][1][0], Bd[x][1][1], Bd[x][1][2], Bd[x][1][3]});
        }
        if constexpr (MV != 0 && j == 0) {
          // A(k) landed (MV = 0: at the top of the step): the filter loads of this step stand
          // behind this wait, except those w2_gslot puts into group (0, 0)
          if constexpr (STAMP) stamp(1);
          if constexpr ((ABL & 4) == 0)
            asm volatile("s_waitcnt vmcnt(%8)"
                         : "+v"(A[0][0][0]), "+v"(A[0][0][1]), "+v"(A[0][1][0]), "+v"(A[0][1][1]), "+v"(A[1][0][0]),
                           "+v"(A[1][0][1]), "+v"(A[1][1][0]), "+v"(A[1][1][1])
                         : "n"(w2_wait_a(MV))
                         : "memory");
          if constexpr (STAMP) stamp(2);
        }
        if constexpr (STAMP) stamp(j == 0 ? 3 : 5);
        if constexpr (MV == 0) {
#pragma unroll
          for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              if constexpr ((ABL & 1) != 0) continue;
              acc[x][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[x][i][0], Bh[x], acc[x][i][j], 0, 0, 0);
              acc[x][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[x][i][0], Bl[x], acc[x][i][j], 0, 0, 0);
              acc[x][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[x][i][1], Bh[x], acc[x][i][j], 0, 0, 0);
            }
        } else {
          // The same three MFMAs per accumulator in the same order, written out in the order hipcc
          // issues them above (per xi the two chains i = 0, 1 alternately), each followed by what
          // w2_slot puts behind it, tied to its accumulator and to that of the MFMA after it.
          auto half = [&](auto xc) __attribute__((always_inline)) {
            constexpr int x = decltype(xc)::value;
            auto mf = [&](auto mc, auto ic, const f16x8& af, const f16x8& bf, f32x16& nxt) __attribute__((always_inline)) {
              constexpr int m = decltype(mc)::value, i = decltype(ic)::value;
              if constexpr ((ABL & 1) == 0) acc[x][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc[x][i][j], 0, 0, 0);
              vmem1(std::integral_constant<int, w2_slot(MV, j, 6 * x + m)>{}, An, k1, k2, sl2, acc[x][i][j], nxt);
            };
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, 1>;
            mf(std::integral_constant<int, 0>{}, I0{}, A[x][0][0], Bh[x], acc[x][1][j]);
            mf(std::integral_constant<int, 1>{}, I1{}, A[x][1][0], Bh[x], acc[x][0][j]);
            mf(std::integral_constant<int, 2>{}, I0{}, A[x][0][0], Bl[x], acc[x][1][j]);
            mf(std::integral_constant<int, 3>{}, I1{}, A[x][1][0], Bl[x], acc[x][0][j]);
            mf(std::integral_constant<int, 4>{}, I0{}, A[x][0][1], Bh[x], acc[x][1][j]);
            mf(std::integral_constant<int, 5>{}, I1{}, A[x][1][1], Bh[x], acc[1][0][j]);   // (xi 1: none follows)
          };
          half(std::integral_constant<int, 0>{});
          half(std::integral_constant<int, 1>{});
        }
        if constexpr (STAMP) stamp(j == 0 ? 4 : 6);
      }
    };
    group(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
    group(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
    group(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
    group(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
  };

  // PF = 0.  per tile tile j: both GEMMs' B fragments (the transform) from ring slot sl, then 12 MFMAs
  auto compute = [&](const f16x8 (&A)[2][2][2], int sl) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int b = tb[j] + sl * BUF;
      asm volatile("" : "+v"(b));   // the pixel addresses are formed per step (not held across it)
      // B fragments as dwords (2 fp16 each): [xi][hi|lo] x 4 dwords, quad Q in dwords 2Q, 2Q + 1
      unsigned Bd[2][2][4];
      if constexpr ((ABL & 2) != 0) {
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int hl = 0; hl < 2; ++hl)
#pragma unroll
            for (int d = 0; d < 4; ++d) Bd[x][hl][d] = 0x3c003c00u;
      } else {
        auto quad = [&](auto qc) __attribute__((always_inline)) {
          constexpr int Q = decltype(qc)::value;
          const f32x4 aX = smem[b + to_aX + Q * QS], aY = smem[b + to_aY + Q * QS], aZ = smem[b + to_aZ + Q * QS];
          const f32x4 bX = smem[b + to_bX + Q * QS], bY = smem[b + to_bY + Q * QS], bZ = smem[b + to_bZ + Q * QS];
          // (vector forms: each f32x4 op becomes two v_pk_*_f32 on the registers ds_read_b128 filled)
          const f32x4 tX = __builtin_elementwise_fma(srv, bX, aX);
          const f32x4 tY = __builtin_elementwise_fma(srv, bY, aY);
          const f32x4 tZ = __builtin_elementwise_fma(srv, bZ, aZ);
          const f32x4 v0 = tX - tY;
          const f32x4 v1 = __builtin_elementwise_fma(szv, tZ, tY);
          split_dw(v0, Bd[0][0][2 * Q], Bd[0][0][2 * Q + 1], Bd[0][1][2 * Q], Bd[0][1][2 * Q + 1]);
          split_dw(v1, Bd[1][0][2 * Q], Bd[1][0][2 * Q + 1], Bd[1][1][2 * Q], Bd[1][1][2 * Q + 1]);
        };
        quad(std::integral_constant<int, 0>{});
        quad(std::integral_constant<int, 1>{});
      }
      f16x8 Bh[2], Bl[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        Bh[x] = __builtin_bit_cast(f16x8, u32x4{Bd[x][0][0], Bd[x][0][1], Bd[x][0][2], Bd[x][0][3]});
        Bl[x] = __builtin_bit_cast(f16x8, u32x4{Bd[x][1][0], Bd[x][1][1], Bd[x][1][2], Bd[x][1][3]});
      }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if constexpr ((ABL & 1) != 0) continue;
          acc[x][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[x][i][0], Bh[x], acc[x][i][j], 0, 0, 0);
          acc[x][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[x][i][0], Bl[x], acc[x][i][j], 0, 0, 0);
          acc[x][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[x][i][1], Bh[x], acc[x][i][j], 0, 0, 0);
        }
    }
  };

  // K loop, one step per chunk pair k, one barrier per step.  Per step each wave issues the
  // filters of pair k + 1 (8 loads, into the other register set) and the raw input of pair k + 2
  // (4 LDS-DMA pieces, ring slot (k + 2) % 3) while it transforms and multiplies pair k.  At the
  // top of a step the wave's queue holds A(k) 8, raw(k+1) 4, in that order (the prologue leaves
  // it so), and every placement issues all of A(k+1) before raw(k+2).  Ring slot (k + 2) % 3 was
  // last read in step k - 1, behind whose barrier the step stands: a piece is safe anywhere in it.
  // Counted waits (loads past the last pair repeat it, so the counts are the same on every step):
  //   before the first MFMA: A(k) landed -- younger: raw(k+1) 4 and what the step has issued by
  //     then: MV 0 all 12 -> vmcnt(16); MV 1 nothing -> vmcnt(4); MV 2 two loads -> vmcnt(6)
  //   before the barrier: raw(k+1) landed -- younger: A(k+1) 8, raw(k+2) 4 -> vmcnt(12)
  // The registers of A(k+1) are idle from the last MFMA of step k - 1 to the load that writes them.
  f16x8 AS[2][2][2][2];   // two register sets [set][xi][i][hi|lo]
  load_a(AS[0], 0);
  dma(0, 0);
  dma(min(1, a.pairs - 1), 1);
  if constexpr (MV == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // raw(0) landed (raw(1) may not)
  __syncthreads();                                       // (and the epilogue constants are staged)
  __builtin_amdgcn_sched_barrier(0);
  auto step = [&](int k, f16x8 (&A)[2][2][2], f16x8 (&An)[2][2][2]) __attribute__((always_inline)) {
    W2Raw r0;
    const int k1 = min(k + 1, a.pairs - 1), k2 = min(k + 2, a.pairs - 1);
    stamp(0);
    if constexpr (PF != 0) rd(r0, k % 3, 0, std::integral_constant<int, 0>{}, nullptr);
    if constexpr (MV == 0) {
      load_a(An, k1);
      dma(k2, (k + 2) % 3);
      __builtin_amdgcn_sched_barrier(0);
      stamp(1);
      if constexpr ((ABL & 4) == 0)
        asm volatile("s_waitcnt vmcnt(16)"
                     : "+v"(A[0][0][0]), "+v"(A[0][0][1]), "+v"(A[0][1][0]), "+v"(A[0][1][1]), "+v"(A[1][0][0]),
                       "+v"(A[1][0][1]), "+v"(A[1][1][0]), "+v"(A[1][1][1])
                     :
                     : "memory");
      stamp(2);
    }
    if constexpr (PF != 0) compute_pf(A, k % 3, r0, An, k1, k2, (k + 2) % 3);
    else compute(A, k % 3);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" : : "n"(w2_wait_raw(MV)) : "memory");
    stamp(7);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  stamp(-1);
  for (int k = 0; k < a.pairs; k += 2) {
    step(k, AS[0], AS[1]);
    if (k + 1 < a.pairs) step(k + 1, AS[1], AS[0]);
  }
  // every filter register the asm loads wrote stays allocated until the loads have landed (the
  // last step's loads are never used: without this their registers could be reused while in flight)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"
               : "+v"(AS[0][0][0][0]), "+v"(AS[0][0][0][1]), "+v"(AS[0][0][1][0]), "+v"(AS[0][0][1][1]),
                 "+v"(AS[0][1][0][0]), "+v"(AS[0][1][0][1]), "+v"(AS[0][1][1][0]), "+v"(AS[0][1][1][1]),
                 "+v"(AS[1][0][0][0]), "+v"(AS[1][0][0][1]), "+v"(AS[1][0][1][0]), "+v"(AS[1][0][1][1]),
                 "+v"(AS[1][1][0][0]), "+v"(AS[1][1][0][1]), "+v"(AS[1][1][1][0]), "+v"(AS[1][1][1][1])
               :
               : "memory");
  __syncthreads();
  if constexpr (STAMP) {
    if (blockIdx.x == 0 && lane == 0)
#pragma unroll
      for (int i = 0; i < 8; ++i) a.dbg[w * 8 + i] = tsum[i];
  }

  bool bad = false;
  if constexpr ((ABL & 16) != 0) {
    // keep the accumulators live: one value per lane
    float sum = 0.f;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) sum += acc[x][i][j][r];
    if (sum == 1.2345f || bad) atomicOr(a.range_flag, 1);
    return;
  }
  // epilogue: M tiles through LDS, per round i (32 channels) [xi][j][q][h][32] x f32x4 (128 KB);
  // thread (j, q, h, tile) sums its 4 channels' 16 values in a fixed order into the 2x2 outputs
  f32x4* xm = smem;
  f32x4 nonfin = {0.f, 0.f, 0.f, 0.f};   // NaN where a value in front of the activation was NaN or +-inf
  const float* eb = (const float*)(smem + 8192);
  const int Wo = a.W + 2 * a.out_pad;
  float* out_f = a.out + (size_t)n * a.out_fs;
  const int rn = tid & 31, rh = (tid >> 5) & 1, rq = (tid >> 6) & 3, rj = tid >> 8;
  const int rs = s0 + 32 * rj + rn, rband = rs / BW, ru = rs - rband * BW, rtx = ru >> 1, rty = 2 * rband + (ru & 1);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          xm[((((2 * w + x) * 2 + j) * 4 + q) * 2 + h) * 32 + l32] =
              f32x4{acc[x][i][j][4 * q], acc[x][i][j][4 * q + 1], acc[x][i][j][4 * q + 2], acc[x][i][j][4 * q + 3]};
    __syncthreads();
    {
      const f32x4* mp = xm + ((rj * 4 + rq) * 2 + rh) * 32 + rn;   // + xi * 8 KiB (512 units)
      // Y = A^T M A: rows R0[c] = M0c + M1c + M2c, R1[c] = M1c - M2c - M3c; then the columns
      f32x4 R0[4], R1[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 m0 = mp[(0 + c) * 512], m1 = mp[(4 + c) * 512], m2 = mp[(8 + c) * 512], m3 = mp[(12 + c) * 512];
        R0[c] = (m0 + m1) + m2;
        R1[c] = (m1 - m2) - m3;
      }
      f32x4 Y[2][2];
      Y[0][0] = (R0[0] + R0[1]) + R0[2];
      Y[0][1] = (R0[1] - R0[2]) - R0[3];
      Y[1][0] = (R1[0] + R1[1]) + R1[2];
      Y[1][1] = (R1[1] - R1[2]) - R1[3];
      const int cl = i * 32 + 8 * rq + 4 * rh, co = co_b * 64 + cl;
      const f32x4 bv = *(const f32x4*)(eb + cl);
      const f32x4 sl = *(const f32x4*)(eb + 64 + cl);
      if (rty < a.TH) {
        float* oc = out_f + (size_t)(co >> 3) * a.out_chs + (co & 7);
#pragma unroll
        for (int yy = 0; yy < 2; ++yy)
#pragma unroll
          for (int xx = 0; xx < 2; ++xx) {
            const int y = 2 * rty + yy, x = 2 * rtx + xx;
            if (y >= a.H || x >= a.W) continue;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = Y[yy][xx][e] * a.wscale_inv + bv[e];
            // an overflowed V arrives here as NaN (or +-inf); the ReLU below would store 0 for NaN
            // and -inf, in range, so a non-finite value raises the flag before the activation:
            // 0 v is +-0 for a number and NaN otherwise, summed here and tested once at the end
            nonfin = __builtin_elementwise_fma(v, f32x4{0.f, 0.f, 0.f, 0.f}, nonfin);
            if (a.act == ACT_RELU) {
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
            } else if (a.act == ACT_PRELU) {
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = v[e] >= 0.f ? v[e] : v[e] * sl[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) bad |= !(__builtin_fabsf(v[e]) < 65504.f);
            *(f32x4*)(oc + (size_t)((y + a.out_pad) * Wo + x + a.out_pad) * 8) = v;
          }
      }
    }
    __syncthreads();
  }
  bad |= !((nonfin[0] + nonfin[1]) + (nonfin[2] + nonfin[3]) == 0.f);
  if (bad) atomicOr(a.range_flag, 1);
}

int g_wino_blocks(const ConvLaunch& c, int* bpf) {
  const int TH = (c.H + 1) / 2, TW = (c.W + 1) / 2, nbands = (TH + 1) / 2;
  *bpf = (nbands * 2 * TW + 63) / 64;
  return c.n * *bpf * (c.cout / 64);
}

}  // namespace

bool wino_f16_fits(const ConvLaunch& c) {
  return c.ks == 3 && c.in_pad >= 1 && c.cout % 64 == 0 && c.cout > 0 && !c.hpool && !c.vin && !c.fold &&
         c.cout7 == 0 && (c.W + 1) / 2 >= 32 && (long long)c.H * c.W > 1024 &&
         !((c.in_cs | c.in_coff | c.out_cs | c.out_coff) & 7) && (long long)(c.H + 2 * c.in_pad) * (c.W + 2 * c.in_pad) * 8 < (1ll << 30);
}

hipError_t launch_wino_f16(const ConvLaunch& c, hipStream_t s) {
  if (!wino_f16_fits(c)) { set_error("wino_f16: launch not eligible"); return hipErrorInvalidValue; }
  if (!c.wx3 || !c.range_flag) { set_error("wino_f16: split filters / range flag missing"); return hipErrorInvalidValue; }
  W2Args a{};
  a.in_chs = (long long)(c.H + 2 * c.in_pad) * (c.W + 2 * c.in_pad) * 8;
  a.out_chs = (long long)(c.H + 2 * c.out_pad) * (c.W + 2 * c.out_pad) * 8;
  a.in_fs = a.in_chs * (c.in_cs / 8);
  a.out_fs = a.out_chs * (c.out_cs / 8);
  a.in = c.in + (c.in_coff / 8) * a.in_chs;
  a.out = c.out + (c.out_coff / 8) * a.out_chs;
  a.upk = (const f16x8*)c.wx3;
  a.bias = c.bias;
  a.slope = c.slope;
  a.range_flag = c.range_flag;
  a.wscale_inv = c.wscale_inv;
  a.in_pad = c.in_pad;
  a.out_pad = c.out_pad;
  a.H = c.H;
  a.W = c.W;
  a.TH = (c.H + 1) / 2;
  a.TW = (c.W + 1) / 2;
  a.pairs = (c.cin_chunks + 1) / 2;
  a.cin_chunks = c.cin_chunks;
  a.co_blocks = c.cout / 64;
  a.act = c.act;
  const long long nb = g_wino_blocks(c, &a.bpf);
  if (nb <= 0 || nb > 0x7fffffff) { set_error("wino_f16: bad grid"); return hipErrorInvalidValue; }
  a.nblocks = (int)nb;
#ifdef ISLPOSE_DEV
  // ablations 1 .. 31 are those of the PF = 0 loop, 32 and 64 + k those of the PF = 1 loop with its
  // loads at the top of the step (MV = 0); ISLPOSE_W2_PF=0 runs the PF = 0 loop whole
  const int abl = getenv("ISLPOSE_W2_ABL") ? atoi(getenv("ISLPOSE_W2_ABL")) : 0;
  switch (abl) {
#define W2ABL(k) case k: hipLaunchKernelGGL((wino_f16<k, 0, 0>), dim3(a.nblocks), dim3(512), 0, s, a); return hipGetLastError();
    W2ABL(1) W2ABL(2) W2ABL(3) W2ABL(4) W2ABL(6) W2ABL(8) W2ABL(12) W2ABL(14) W2ABL(16) W2ABL(31)
#undef W2ABL
    case 65: hipLaunchKernelGGL((wino_f16<1, 1, 0>), dim3(a.nblocks), dim3(512), 0, s, a); return hipGetLastError();
    case 68: hipLaunchKernelGGL((wino_f16<4, 1, 0>), dim3(a.nblocks), dim3(512), 0, s, a); return hipGetLastError();
    case 72: hipLaunchKernelGGL((wino_f16<8, 1, 0>), dim3(a.nblocks), dim3(512), 0, s, a); return hipGetLastError();
    case 76: hipLaunchKernelGGL((wino_f16<12, 1, 0>), dim3(a.nblocks), dim3(512), 0, s, a); return hipGetLastError();
    case 80: hipLaunchKernelGGL((wino_f16<16, 1, 0>), dim3(a.nblocks), dim3(512), 0, s, a); return hipGetLastError();
    case 32: hipLaunchKernelGGL((wino_f16<32, 1, 0>), dim3(a.nblocks), dim3(512), 0, s, a); return hipGetLastError();
    default: break;
  }
  if (getenv("ISLPOSE_W2_PF") && atoi(getenv("ISLPOSE_W2_PF")) == 0) {
    hipLaunchKernelGGL((wino_f16<0, 0, 0>), dim3(a.nblocks), dim3(512), 0, s, a);
    return hipGetLastError();
  }
  // ISLPOSE_W2_MV=0 .. 3: where the step issues its loads (default W2_MV); with c.dbg the stamped build
  const int mv = getenv("ISLPOSE_W2_MV") ? atoi(getenv("ISLPOSE_W2_MV")) : W2_MV;
  a.dbg = c.dbg;
  if (mv < 0 || mv > 3) { set_error("wino_f16: ISLPOSE_W2_MV out of range"); return hipErrorInvalidValue; }
#define W2MV(m)                                                                                    \
  if (mv == m) {                                                                                   \
    if (c.dbg) hipLaunchKernelGGL((wino_f16<0, 1, m, true>), dim3(a.nblocks), dim3(512), 0, s, a);  \
    else hipLaunchKernelGGL((wino_f16<0, 1, m>), dim3(a.nblocks), dim3(512), 0, s, a);             \
    return hipGetLastError();                                                                      \
  }
  W2MV(0) W2MV(1) W2MV(2) W2MV(3)
#undef W2MV
#endif
  hipLaunchKernelGGL((wino_f16<0, 1>), dim3(a.nblocks), dim3(512), 0, s, a);
  return hipGetLastError();
}

double wino_f16_mfma_flops(const ConvLaunch& c) {
  int bpf = 0;
  const double nb = g_wino_blocks(c, &bpf);
  return nb * 16.0 * 64 * 64 * 16.0 * ((c.cin_chunks + 1) / 2) * 2 * 3;
}

}  // namespace isl
