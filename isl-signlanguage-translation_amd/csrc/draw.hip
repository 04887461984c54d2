// isl_draw: stick-model overlays on resident uint8 frames in one launch (include/islpose.h,
// DESIGN.md section 4.2j).  The reference draws them on the host, one full-canvas copy and
// alpha blend per limb (util.draw_bodypose / drawStickmodel, src/util.py:47-96,308-358) and a
// matplotlib figure for the hands; here a pixel applies, in list order, the primitives that
// cover it.  All arithmetic is 64-bit integer: no floating point runs on the device.
//
// A block owns one DRAW_TW x DRAW_TH pixel tile of one frame.  It walks the frame's list in
// batches of DRAW_CHUNK entries: each thread tests one entry's conservative box (made on the
// host, clipped to the frame) against the tile, a ballot prefix keeps the hits in list order in
// LDS, and every thread then applies the batch's hits to its DRAW_PX consecutive pixels, whose
// state stays in registers across batches -- so a list of any length works.  A tile nothing
// hits leaves after the cull when the call is in place, and is a plain copy (or zeros)
// otherwise.  Memory-bound by design: the floor is 2*H*W*3 bytes per frame out of place, the
// bytes of the touched runs in place (measured at 60 % of the copy kernel's rate: the blocks
// that carry the drawing, not the bytes, set the time -- DESIGN.md section 4.2j).  A thread's 8 pixels are 24 bytes: three 8-byte accesses
// when the run lies whole in its row and starts on an 8-byte address, six dwords on a 4-byte
// address (source and destination each decide for themselves), bytes otherwise (odd 3*W,
// unaligned bases, the row's last run).  Out of place the loads are issued before the cull.
#include "internal.h"
#include "islpose.h"

#include <cmath>
#include <cstring>
#include <mutex>

namespace isl {

constexpr int DRAW_BLOCK = 256, DRAW_PX = 8, DRAW_TW = 128, DRAW_TH = 16, DRAW_CHUNK = DRAW_BLOCK;
static_assert(DRAW_TW / DRAW_PX * DRAW_TH == DRAW_BLOCK, "one thread per 8-pixel run of the tile");

// The device's form of an isl_draw_prim (col = color[0] | color[1] << 8 | color[2] << 16 |
// blend << 24) and its conservative box, inclusive and clipped to the frame; an empty box is
// {32767, 32767, -1, -1}, which no tile meets.
struct DrawRec {
  int32_t kind, p[4], c, s, r2;
  uint32_t col;
};
struct DrawBox {
  int16_t x0, y0, x1, y1;
};

__device__ __forceinline__ bool draw_covers(const DrawRec& r, int x, int y) {
  const long long dx = x - r.p[0], dy = y - r.p[1];
  if (r.kind == 0) {
    const long long u = dx * r.c + dy * r.s, v = dy * r.c - dx * r.s;
    const long long a = r.p[2], b = r.p[3];
    if ((u < 0 ? -u : u) > (a << 14) || (v < 0 ? -v : v) > (b << 14)) return false;
    return u * u * (b * b) + v * v * (a * a) <= (a * a * b * b) << 28;
  }
  const long long r2 = r.r2;
  if (dx * dx + dy * dy <= r2) return true;
  if (r.kind == 1) return false;
  const long long ex = x - r.p[2], ey = y - r.p[3];
  if (ex * ex + ey * ey <= r2) return true;
  const long long ddx = r.p[2] - r.p[0], ddy = r.p[3] - r.p[1];
  const long long L2 = ddx * ddx + ddy * ddy;
  const long long t = dx * ddx + dy * ddy, cr = dx * ddy - dy * ddx;
  return L2 > 0 && t >= 0 && t <= L2 && cr * cr <= r2 * L2;   // L2 = 0: the disc
}

__device__ __forceinline__ uint32_t draw_colour(uint32_t px, uint32_t col) {
  if (!(col >> 24)) return col & 0xffffffu;
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const uint32_t v = (px >> (8 * ch)) & 255u, k = (col >> (8 * ch)) & 255u;
    out |= ((4u * v + 6u * k + 5u) / 10u) << (8 * ch);
  }
  return out;
}

// grid (tiles_x * tiles_y, min(n, 65535)): blockIdx.y strides over the frames.  src may equal
// dst (in place: a thread reads and writes only its own pixels' bytes), hence no __restrict__.
__global__ __launch_bounds__(DRAW_BLOCK) void draw_kernel(const uint8_t* src, uint8_t* dst,
                                                          int n, int H, int W, int tiles_x,
                                                          const DrawRec* __restrict__ recs,
                                                          const DrawBox* __restrict__ boxes,
                                                          const int32_t* __restrict__ first) {
  __shared__ DrawRec s_rec[DRAW_CHUNK];
  __shared__ DrawBox s_box[DRAW_CHUNK];
  __shared__ int s_cnt[DRAW_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int tx0 = tx * DRAW_TW, ty0 = ty * DRAW_TH;
  const int tx1 = min(tx0 + DRAW_TW, W) - 1, ty1 = min(ty0 + DRAW_TH, H) - 1;
  const int y = ty0 + tid / (DRAW_TW / DRAW_PX), x0 = tx0 + (tid % (DRAW_TW / DRAW_PX)) * DRAW_PX;
  const int npx = y < H ? min(max(W - x0, 0), DRAW_PX) : 0;      // the thread's pixels inside the frame
  const bool in_place = src == dst;
  const long long L = 3ll * H * W;
  for (int f = blockIdx.y; f < n; f += gridDim.y) {
    const long long row = (long long)f * L + 3ll * ((long long)y * W + x0);   // used only when npx > 0
    uint32_t px[DRAW_PX];
    bool loaded = false, touched = false;
    auto load = [&]() {
#pragma unroll
      for (int q = 0; q < DRAW_PX; ++q) px[q] = 0u;
      if (!src || npx == 0) return;
      const uint8_t* a = src + row;
      if (npx == DRAW_PX && ((uintptr_t)a & 3) == 0) {
        uint32_t e[7];
        if (((uintptr_t)a & 7) == 0) {
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const uint2 t = reinterpret_cast<const uint2*>(a)[d];
            e[2 * d] = t.x;
            e[2 * d + 1] = t.y;
          }
        } else {
#pragma unroll
          for (int d = 0; d < 6; ++d) e[d] = reinterpret_cast<const uint32_t*>(a)[d];
        }
        e[6] = 0u;
#pragma unroll
        for (int q = 0; q < DRAW_PX; ++q) {
          const int b = 3 * q, d = b >> 2, sh = 8 * (b & 3);
          px[q] = (uint32_t)((((uint64_t)e[d + 1] << 32) | e[d]) >> sh) & 0xffffffu;
        }
      } else {
#pragma unroll
        for (int q = 0; q < DRAW_PX; ++q)
          if (q < npx) px[q] = a[3 * q] | ((uint32_t)a[3 * q + 1] << 8) | ((uint32_t)a[3 * q + 2] << 16);
      }
    };
    if (!in_place) {                                          // needed whatever the cull finds: issue it first
      load();
      loaded = true;
    }
    const int lo = first[f], hi = first[f + 1];
    for (int base = lo; base < hi; base += DRAW_CHUNK) {
      const int i = base + tid;
      bool hit = false;
      DrawBox bx;
      if (i < hi) {
        bx = boxes[i];
        hit = bx.x0 <= tx1 && bx.x1 >= tx0 && bx.y0 <= ty1 && bx.y1 >= ty0;
      }
      const unsigned long long votes = __ballot(hit);
      if (lane == 0) s_cnt[wave] = __popcll(votes);
      __syncthreads();
      int off = 0, nhit = 0;
#pragma unroll
      for (int k = 0; k < DRAW_BLOCK / 64; ++k) {
        if (k < wave) off += s_cnt[k];
        nhit += s_cnt[k];
      }
      if (hit) {
        const int slot = off + __popcll(votes & ((1ull << lane) - 1ull));
        s_rec[slot] = recs[i];
        s_box[slot] = bx;
      }
      __syncthreads();
      if (nhit) {                                             // block-uniform
        if (!loaded) {
          load();
          loaded = true;
        }
        for (int k = 0; k < nhit; ++k) {
          const DrawBox b = s_box[k];
          if (npx == 0 || y < b.y0 || y > b.y1 || x0 > b.x1 || x0 + DRAW_PX - 1 < b.x0) continue;
          const DrawRec r = s_rec[k];
#pragma unroll
          for (int q = 0; q < DRAW_PX; ++q)
            if (q < npx && draw_covers(r, x0 + q, y)) {
              px[q] = draw_colour(px[q], r.col);
              touched = true;
            }
        }
      }
      __syncthreads();                                        // the next batch refills the LDS
    }
    if (!loaded) continue;                                    // in place and nothing hit the tile: never written
    if (npx == 0 || (in_place && !touched)) continue;
    uint8_t* a = dst + row;
    if (npx == DRAW_PX && ((uintptr_t)a & 3) == 0) {
      uint32_t w[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int q = 0; q < DRAW_PX; ++q)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int b = 3 * q + ch;
          w[b >> 2] |= ((px[q] >> (8 * ch)) & 255u) << (8 * (b & 3));
        }
      if (((uintptr_t)a & 7) == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) reinterpret_cast<uint2*>(a)[d] = make_uint2(w[2 * d], w[2 * d + 1]);
      } else {
#pragma unroll
        for (int d = 0; d < 6; ++d) reinterpret_cast<uint32_t*>(a)[d] = w[d];
      }
    } else {
#pragma unroll
      for (int q = 0; q < DRAW_PX; ++q)
        if (q < npx) {
          a[3 * q] = (uint8_t)px[q];
          a[3 * q + 1] = (uint8_t)(px[q] >> 8);
          a[3 * q + 2] = (uint8_t)(px[q] >> 16);
        }
    }
  }
}

namespace {

// The table's way to the device: the pinned + device ring of isl_augment (csrc/augment.hip),
// with a ring of its own.  One slot holds the call's records, boxes and `first`.
constexpr int DRAW_SLOTS = 8, DRAW_MAX_DEV = 64;
struct DrawSlot {
  void* pin = nullptr;
  void* dev = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
};
struct DrawRing {
  DrawSlot slot[DRAW_SLOTS];
  unsigned next = 0;
};
std::mutex g_draw_mu;
DrawRing g_draw_ring[DRAW_MAX_DEV];

int draw_fail(int code, const std::string& msg) {
  set_error("isl_draw: " + msg);
  return code;
}

#define DRAW_HIP(expr)                                                                   \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) return draw_fail(ISL_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

constexpr int DRAW_COORD = 16384;

bool coord_ok(int32_t v) { return v >= -DRAW_COORD && v <= DRAW_COORD; }

// Conservative inclusive box of a valid primitive, clipped to the frame.  A covered pixel of a
// stick has |u| <= A = a*2^14 and |v| <= B = b*2^14 and lies in the ellipse (u/A)^2 + (v/B)^2
// <= 1; with N = c^2 + s^2, dx = (c*u - s*v) / N and dy = (s*u + c*v) / N, whose maxima over
// the ellipse are sqrt(c^2*A^2 + s^2*B^2) / N and sqrt(s^2*A^2 + c^2*B^2) / N.  They are
// evaluated in fp64 (relative error ~1e-16 on values < 2^41) and widened by one pixel.  N = 0
// covers every pixel.  Any c, s in range is handled, not only those of an angle.
DrawBox draw_box(const isl_draw_prim& q, int H, int W) {
  long long x0, y0, x1, y1;
  if (q.kind == 0) {
    const double c = q.c, s = q.s, N = c * c + s * s;
    if (N == 0.0) {
      x0 = y0 = 0;
      x1 = W - 1;
      y1 = H - 1;
    } else {
      const double A = 16384.0 * q.p[2], B = 16384.0 * q.p[3];
      const double hx = std::min(std::sqrt(c * c * A * A + s * s * B * B) / N, 65536.0);
      const double hy = std::min(std::sqrt(s * s * A * A + c * c * B * B) / N, 65536.0);
      const long long ix = (long long)std::ceil(hx) + 1, iy = (long long)std::ceil(hy) + 1;
      x0 = q.p[0] - ix;
      x1 = q.p[0] + ix;
      y0 = q.p[1] - iy;
      y1 = q.p[1] + iy;
    }
  } else {
    long long r = 0;
    while (r * r < q.r2) ++r;                               // ceil(sqrt(r2)) <= 64
    const bool seg = q.kind == 2;
    x0 = std::min(q.p[0], seg ? q.p[2] : q.p[0]) - r;
    x1 = std::max(q.p[0], seg ? q.p[2] : q.p[0]) + r;
    y0 = std::min(q.p[1], seg ? q.p[3] : q.p[1]) - r;
    y1 = std::max(q.p[1], seg ? q.p[3] : q.p[1]) + r;
  }
  x0 = std::max(x0, 0ll);
  y0 = std::max(y0, 0ll);
  x1 = std::min(x1, (long long)W - 1);
  y1 = std::min(y1, (long long)H - 1);
  if (x0 > x1 || y0 > y1) return DrawBox{32767, 32767, -1, -1};
  return DrawBox{(int16_t)x0, (int16_t)y0, (int16_t)x1, (int16_t)y1};
}

size_t round16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace
}  // namespace isl

using namespace isl;

extern "C" int isl_draw(const uint8_t* d_src, uint8_t* d_dst, int n, int H, int W, const isl_draw_prim* prims,
                        const int32_t* first, void* stream) {
  if (!d_dst) return draw_fail(ISL_E_ARG, "NULL d_dst");
  if (n < 0) return draw_fail(ISL_E_ARG, "n = " + std::to_string(n) + " is negative");
  if (H <= 0 || W <= 0 || H > 16384 || W > 16384 || (long long)H * W > (1ll << 29))
    return draw_fail(ISL_E_ARG, "bad shape H = " + std::to_string(H) + ", W = " + std::to_string(W) +
                                    " (1 <= H, W <= 16384, H * W <= 2^29)");
  const unsigned long long L = 3ull * H * W;
  if (d_src && d_src != d_dst) {
    const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + (uintptr_t)(L * n);
    const uintptr_t t0 = (uintptr_t)d_dst, t1 = t0 + (uintptr_t)(L * n);
    if (s0 < t1 && t0 < s1) return draw_fail(ISL_E_ARG, "d_dst overlaps d_src without being equal to it");
  }
  if (n == 0) return ISL_OK;
  if (!first) return draw_fail(ISL_E_ARG, "NULL first");
  if (first[0] != 0) return draw_fail(ISL_E_ARG, "first[0] = " + std::to_string(first[0]) + " must be 0");
  for (int f = 0; f < n; ++f)
    if (first[f + 1] < first[f])
      return draw_fail(ISL_E_ARG, "first decreases at frame " + std::to_string(f) + ": " + std::to_string(first[f]) +
                                      " -> " + std::to_string(first[f + 1]));
  const int total = first[n];
  if (total > (1 << 20)) return draw_fail(ISL_E_ARG, std::to_string(total) + " primitives exceed 2^20 per call");
  if (total > 0 && !prims) return draw_fail(ISL_E_ARG, "NULL prims");
  for (int k = 0; k < total; ++k) {
    const isl_draw_prim& q = prims[k];
    const std::string at = "primitive " + std::to_string(k) + ": ";
    if (q.kind < 0 || q.kind > 2) return draw_fail(ISL_E_ARG, at + "unknown kind " + std::to_string(q.kind));
    if (q.blend > 1) return draw_fail(ISL_E_ARG, at + "blend " + std::to_string(q.blend) + " must be 0 or 1");
    if (q.reserved) return draw_fail(ISL_E_ARG, at + "reserved field must be zero");
    if (!coord_ok(q.p[0]) || !coord_ok(q.p[1]) || (q.kind == 2 && (!coord_ok(q.p[2]) || !coord_ok(q.p[3]))))
      return draw_fail(ISL_E_ARG, at + "coordinate outside [-16384, 16384]");
    if (q.kind == 0) {
      if (q.p[2] < 1 || q.p[2] > 4096 || q.p[3] < 1 || q.p[3] > 16)
        return draw_fail(ISL_E_ARG, at + "half axes a = " + std::to_string(q.p[2]) + ", b = " + std::to_string(q.p[3]) +
                                        " outside [1, 4096] x [1, 16]");
      if (q.c < -16384 || q.c > 16384 || q.s < -16384 || q.s > 16384)
        return draw_fail(ISL_E_ARG, at + "c, s outside [-16384, 16384]");
    } else if (q.r2 < 0 || q.r2 > 4096) {
      return draw_fail(ISL_E_ARG, at + "r2 = " + std::to_string(q.r2) + " outside [0, 4096]");
    }
  }
  if (total == 0 && d_src == d_dst) return ISL_OK;         // in place, nothing to draw

  int dev = 0;
  DRAW_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= DRAW_MAX_DEV) return draw_fail(ISL_E_ARG, "device index " + std::to_string(dev) + " not supported");
  hipStream_t s = (hipStream_t)stream;
  const size_t off_box = round16((size_t)total * sizeof(DrawRec));
  const size_t off_first = off_box + round16((size_t)total * sizeof(DrawBox));
  const size_t bytes = off_first + (size_t)(n + 1) * sizeof(int32_t);
  std::lock_guard<std::mutex> lock(g_draw_mu);
  DrawRing& ring = g_draw_ring[dev];
  DrawSlot& sl = ring.slot[ring.next % DRAW_SLOTS];
  if (sl.ev) DRAW_HIP(hipEventSynchronize(sl.ev));        // the slot's previous launch has read its table
  if (bytes > sl.bytes) {
    if (sl.pin) DRAW_HIP(hipHostFree(sl.pin));
    if (sl.dev) DRAW_HIP(hipFree(sl.dev));
    sl.pin = sl.dev = nullptr;
    sl.bytes = 0;
    const size_t cap = (bytes + 4095) / 4096 * 4096;
    DRAW_HIP(hipHostMalloc(&sl.pin, cap, hipHostMallocDefault));
    DRAW_HIP(hipMalloc(&sl.dev, cap));
    sl.bytes = cap;
  }
  if (!sl.ev) DRAW_HIP(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
  DrawRec* recs = reinterpret_cast<DrawRec*>(sl.pin);
  DrawBox* boxes = reinterpret_cast<DrawBox*>((char*)sl.pin + off_box);
  for (int k = 0; k < total; ++k) {
    const isl_draw_prim& q = prims[k];
    recs[k] = DrawRec{q.kind, {q.p[0], q.p[1], q.p[2], q.p[3]}, q.c, q.s, q.r2,
                      (uint32_t)q.color[0] | ((uint32_t)q.color[1] << 8) | ((uint32_t)q.color[2] << 16) |
                          ((uint32_t)q.blend << 24)};
    boxes[k] = draw_box(q, H, W);
  }
  memcpy((char*)sl.pin + off_first, first, (size_t)(n + 1) * sizeof(int32_t));
  DRAW_HIP(hipMemcpyAsync(sl.dev, sl.pin, bytes, hipMemcpyHostToDevice, s));
  const int tiles_x = (W + DRAW_TW - 1) / DRAW_TW, tiles_y = (H + DRAW_TH - 1) / DRAW_TH;
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)std::min(n, 65535));
  hipLaunchKernelGGL(draw_kernel, grid, dim3(DRAW_BLOCK), 0, s, d_src, d_dst, n, H, W, tiles_x,
                     (const DrawRec*)sl.dev, (const DrawBox*)((const char*)sl.dev + off_box),
                     (const int32_t*)((const char*)sl.dev + off_first));
  DRAW_HIP(hipGetLastError());
  DRAW_HIP(hipEventRecord(sl.ev, s));
  ring.next++;
  return ISL_OK;
}
