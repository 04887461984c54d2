// isl_augment: augmented copies of resident uint8 frames in one launch (include/islpose.h,
// DESIGN.md section 4.2h): dst[k] = variant(src[item[k].src], item[k]) -- a nearest-neighbour
// rotation about the image centre, then a solarize, with an optional channel reversal at the
// load.  The reference builds these on the host per frame (extract_featuressingle.py:49-52,
// 116-120: torchvision v2.RandomRotation / v2.RandomSolarize) before each model call.
//
// Memory-bound by design: the floor is 2*H*W*3 bytes per item.  An item is one flat run of
// 3*H*W bytes; a thread owns one aligned 16-byte store of it.  16 bytes at byte offset b start
// in pixel b / 3 at channel b % 3 <= 2 and end at most 18 bytes later, so they lie in exactly 6
// consecutive pixels: the thread evaluates those 6 (12.5 % more pixel evaluations than pixels),
// packs their 18 bytes and stores the 16 it owns.  Adjacent lanes own adjacent stores and read
// adjacent source pixels along the rotated row.  The source is read in aligned dwords: five or
// six for the 18 consecutive bytes of an item that does not rotate, one or two per pixel of one
// that does (byte loads ran the copy at half the rate: 18 load instructions per store).  The bytes in front of the first aligned
// address and behind the last whole store (an item's base need not be aligned: 3*H*W is any
// number) go one by one in the thread behind the last store.
#include "internal.h"
#include "islpose.h"

#include <cmath>
#include <cstring>
#include <mutex>

namespace isl {

// Source pixel index (row-major) of output pixel (row j, column i) of `it`, -1 for a filled
// pixel.  The coordinate arithmetic is the header's, fp64, evaluated per pixel from (i, j) --
// never incrementally along a row -- so the bits are numpy's (the build has -ffp-contract=off).
__device__ __forceinline__ int aug_source(int i, int j, int H, int W, const isl_aug_item& it, double cx, double cy) {
  if (!it.rotate) return j * W + i;
  const double dx = (double)i - cx, dy = (double)j - cy;
  const double xs = (it.c * dx + it.s * dy) + cx;
  const double ys = ((-it.s) * dx + it.c * dy) + cy;
  const double xr = rint(xs), yr = rint(ys);            // half to even
  const bool in = xr >= 0.0 && xr < (double)W && yr >= 0.0 && yr < (double)H;
  return in ? (int)yr * W + (int)xr : -1;
}

// A raw source pixel b0 | b1 << 8 | b2 << 16 (0 for a filled one) -> the channel reversal,
// then the solarize (filled pixels go through it too).
__device__ __forceinline__ uint32_t aug_finish(uint32_t raw, const isl_aug_item& it) {
  uint32_t v0 = raw & 255u, v1 = (raw >> 8) & 255u, v2 = (raw >> 16) & 255u;
  if (it.swap_rb) {
    const uint32_t t = v0;
    v0 = v2;
    v2 = t;
  }
  const uint32_t thr = (uint32_t)it.threshold;          // 256: never reached
  v0 = v0 >= thr ? 255u - v0 : v0;
  v1 = v1 >= thr ? 255u - v1 : v1;
  v2 = v2 >= thr ? 255u - v2 : v2;
  return v0 | (v1 << 8) | (v2 << 16);
}

// The wide path reads the source in aligned dwords, each of which holds at least one byte it
// needs: such a dword may reach up to 3 bytes past either end of the source array, but never
// leaves the 4-byte word -- hence the page -- of a byte that belongs to it.
__device__ __forceinline__ uint32_t aug_load_pixel(const uint8_t* __restrict__ sf, int p) {
  const uintptr_t a = (uintptr_t)sf + 3ull * (unsigned)p;
  const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const int sh = (int)(a & 3);
  const uint32_t lo = q[0];
  const uint32_t hi = sh >= 2 ? q[1] : 0u;              // q[1] holds byte a + 2 then
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh)) & 0xffffffu;
}

constexpr int AUG_BLOCK = 256;

// grid (ceil((L / 16 + 1) / AUG_BLOCK), m): blockIdx.y is the item
__global__ __launch_bounds__(AUG_BLOCK) void augment_kernel(const uint8_t* __restrict__ src,
                                                            uint8_t* __restrict__ dst,
                                                            const isl_aug_item* __restrict__ tab, int H, int W) {
  const isl_aug_item it = tab[blockIdx.y];
  const long long L = (long long)H * W * 3;             // bytes of one frame (<= 3 * 2^29)
  const uint8_t* sf = src + (long long)it.src * L;
  uint8_t* df = dst + (long long)blockIdx.y * L;
  const double cx = (W - 1) * 0.5, cy = (H - 1) * 0.5;
  long long head = (long long)((16 - ((uintptr_t)df & 15)) & 15);   // bytes before the first aligned one
  if (head > L) head = L;
  const long long nvec = (L - head) >> 4;               // whole aligned 16-byte stores
  const long long g = (long long)blockIdx.x * AUG_BLOCK + threadIdx.x;
  if (g > nvec) return;
  if (g < nvec) {
    const long long b0 = head + 16 * g;                 // b0 + 15 <= L - 1
    const int p0 = (int)(b0 / 3), o = (int)(b0 - 3ll * p0);
    // pixel p0 + 5 starts at byte b0 + 15 - o <= b0 + 15 <= L - 1, so all 6 pixels exist
    uint32_t raw[6];
    if (it.rotate) {
      int j = p0 / W, i = p0 - j * W;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int p = aug_source(i, j, H, W, it, cx, cy);
        raw[q] = p >= 0 ? aug_load_pixel(sf, p) : 0u;
        if (++i == W) {
          i = 0;
          ++j;
        }
      }
    } else {
      // no rotation: the 18 bytes of the 6 pixels are the source's own bytes [3 * p0, 3 * p0 + 18)
      const uintptr_t a = (uintptr_t)sf + 3ull * (unsigned)p0;
      const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
      const int sh = (int)(a & 3);
      uint32_t e[6];
#pragma unroll
      for (int d = 0; d < 5; ++d) e[d] = q[d];          // q[4] starts at or before byte a + 16
      e[5] = sh == 3 ? q[5] : 0u;                        // q[5] holds byte a + 17 then
      uint32_t u[5];
#pragma unroll
      for (int d = 0; d < 5; ++d) u[d] = (uint32_t)((((uint64_t)e[d + 1] << 32) | e[d]) >> (8 * sh));
      raw[0] = u[0] & 0xffffffu;                                             // pixel q at bit 24 * q
      raw[1] = (uint32_t)((((uint64_t)u[1] << 32) | u[0]) >> 24) & 0xffffffu;
      raw[2] = (uint32_t)((((uint64_t)u[2] << 32) | u[1]) >> 16) & 0xffffffu;
      raw[3] = u[2] >> 8;
      raw[4] = u[3] & 0xffffffu;
      raw[5] = (uint32_t)((((uint64_t)u[4] << 32) | u[3]) >> 24) & 0xffffffu;
    }
    uint32_t w[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const uint32_t v = aug_finish(raw[q], it);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int n = 3 * q + ch;
        w[n >> 2] |= ((v >> (8 * ch)) & 255u) << (8 * (n & 3));
      }
    }
    uint4 out;
    const int sh = 8 * o;
    out.x = (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> sh);
    out.y = (uint32_t)((((uint64_t)w[2] << 32) | w[1]) >> sh);
    out.z = (uint32_t)((((uint64_t)w[3] << 32) | w[2]) >> sh);
    out.w = (uint32_t)((((uint64_t)w[4] << 32) | w[3]) >> sh);
    *reinterpret_cast<uint4*>(df + b0) = out;
    return;
  }
  // g == nvec: the scalar head [0, head) and tail [head + 16 * nvec, L), at most 30 bytes,
  // read byte by byte
  const long long tail0 = head + 16 * nvec;
  const long long nscalar = head + (L - tail0);
  for (long long t = 0; t < nscalar; ++t) {
    const long long b = t < head ? t : tail0 + (t - head);
    const int p = (int)(b / 3), ch = (int)(b - 3ll * p);
    const int j = p / W, i = p - j * W;
    const int ps = aug_source(i, j, H, W, it, cx, cy);
    uint32_t raw = 0;
    if (ps >= 0) {
      const uint8_t* px = sf + 3ll * ps;
      raw = px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
    }
    df[b] = (uint8_t)(aug_finish(raw, it) >> (8 * ch));
  }
}

namespace {

// The item table's way to the device: a ring of pinned + device buffer pairs per device.  A
// call copies its records into a slot's pinned buffer, enqueues the copy and the launch, and
// records the slot's event behind the launch; the slot is refilled only once that event has
// completed, so the host waits for the stream only when AUG_SLOTS calls are still in flight.
constexpr int AUG_SLOTS = 8, AUG_MAX_DEV = 64;
struct AugSlot {
  void* pin = nullptr;
  void* dev = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
};
struct AugRing {
  AugSlot slot[AUG_SLOTS];
  unsigned next = 0;
};
std::mutex g_aug_mu;
AugRing g_aug_ring[AUG_MAX_DEV];

int aug_fail(int code, const std::string& msg) {
  set_error("isl_augment: " + msg);
  return code;
}

#define AUG_HIP(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) return aug_fail(ISL_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

}  // namespace
}  // namespace isl

using namespace isl;

extern "C" int isl_augment(const uint8_t* d_src, int n_src, int H, int W, uint8_t* d_dst,
                           const isl_aug_item* items, int m, void* stream) {
  if (m < 0) return aug_fail(ISL_E_ARG, "m = " + std::to_string(m) + " is negative");
  if (m == 0) return ISL_OK;
  if (!d_src || !d_dst || !items) return aug_fail(ISL_E_ARG, "NULL buffer");
  if (n_src <= 0 || H <= 0 || W <= 0 || (long long)H * W > (1ll << 29))
    return aug_fail(ISL_E_ARG, "bad shape n_src = " + std::to_string(n_src) + ", H = " + std::to_string(H) +
                                   ", W = " + std::to_string(W) + " (H * W <= 2^29)");
  if (m > 65535) return aug_fail(ISL_E_ARG, "m = " + std::to_string(m) + " exceeds 65535 items per call");
  for (int k = 0; k < m; ++k) {
    const isl_aug_item& it = items[k];
    const std::string at = "item " + std::to_string(k) + ": ";
    if (it.src < 0 || it.src >= n_src)
      return aug_fail(ISL_E_ARG, at + "src index " + std::to_string(it.src) + " outside [0, " + std::to_string(n_src) + ")");
    if (it.threshold < 0 || it.threshold > 256)
      return aug_fail(ISL_E_ARG, at + "threshold " + std::to_string(it.threshold) + " outside [0, 256]");
    if ((it.rotate & ~1) || (it.swap_rb & ~1)) return aug_fail(ISL_E_ARG, at + "rotate and swap_rb must be 0 or 1");
    if (it.rotate && !(std::isfinite(it.c) && std::isfinite(it.s))) return aug_fail(ISL_E_ARG, at + "c and s must be finite");
    if (it.reserved[0] || it.reserved[1]) return aug_fail(ISL_E_ARG, at + "reserved fields must be zero");
  }
  const unsigned long long L = (unsigned long long)H * W * 3;
  const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + (uintptr_t)(L * n_src);
  const uintptr_t t0 = (uintptr_t)d_dst, t1 = t0 + (uintptr_t)(L * m);
  if (s0 < t1 && t0 < s1) return aug_fail(ISL_E_ARG, "d_dst overlaps d_src");

  int dev = 0;
  AUG_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= AUG_MAX_DEV) return aug_fail(ISL_E_ARG, "device index " + std::to_string(dev) + " not supported");
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)m * sizeof(isl_aug_item);
  std::lock_guard<std::mutex> lock(g_aug_mu);
  AugRing& ring = g_aug_ring[dev];
  AugSlot& sl = ring.slot[ring.next % AUG_SLOTS];
  if (sl.ev) AUG_HIP(hipEventSynchronize(sl.ev));        // the slot's previous launch has read its table
  if (bytes > sl.bytes) {
    if (sl.pin) AUG_HIP(hipHostFree(sl.pin));
    if (sl.dev) AUG_HIP(hipFree(sl.dev));
    sl.pin = sl.dev = nullptr;
    sl.bytes = 0;
    const size_t cap = (bytes + 4095) / 4096 * 4096;
    AUG_HIP(hipHostMalloc(&sl.pin, cap, hipHostMallocDefault));
    AUG_HIP(hipMalloc(&sl.dev, cap));
    sl.bytes = cap;
  }
  if (!sl.ev) AUG_HIP(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
  memcpy(sl.pin, items, bytes);
  AUG_HIP(hipMemcpyAsync(sl.dev, sl.pin, bytes, hipMemcpyHostToDevice, s));
  const unsigned long long threads = L / 16 + 1;        // every item's stores plus its scalar thread
  const dim3 grid((unsigned)((threads + AUG_BLOCK - 1) / AUG_BLOCK), (unsigned)m);
  hipLaunchKernelGGL(augment_kernel, grid, dim3(AUG_BLOCK), 0, s, d_src, d_dst, (const isl_aug_item*)sl.dev, H, W);
  AUG_HIP(hipGetLastError());
  AUG_HIP(hipEventRecord(sl.ev, s));
  ring.next++;
  return ISL_OK;
}
