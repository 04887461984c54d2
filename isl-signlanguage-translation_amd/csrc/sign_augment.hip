// isl_sign_augment: keypoint-space augmentation of the sign classifier's windows in one launch
// (include/islpose.h).  Output window k is item k's view of a resident row
// store: a resampled run of source rows (speed, temporal shift), frames dropped by a counter-based
// draw, and on every present (x, y) pair of a live frame an affine map plus an optional jitter.
//
// One workgroup per item; its lanes go over (frame, unit), a unit being one pair or one label of
// the row (n_body + 2 * n_slots * n_hand units per frame).  The lane of a pair loads x and y,
// computes both in fp64 in the order of the definition (the build has -ffp-contract=off, so no
// product is fused into a sum) and stores both; the lane of a label copies it.  Plain vector loads
// and stores only: no atomics, no LDS, no scratch.  An item that names rows outside the store is
// treated as "every frame masked", so no address outside [d_rows, d_rows + n_rows * F) is formed
// from it.
#include <cmath>
#include <string>

#include "internal.h"
#include "islpose.h"

namespace isl {

constexpr int SA_BLOCK = 256;
constexpr int SA_TMAX = 32, SA_FMAX = 256, SA_ITEMS_MAX = 65535;
constexpr float SA_DROP_MAX = 0.9f;
constexpr uint32_t SA_SITE_DROP = 16, SA_SITE_JITTER = 17;

struct SignAugArgs {
  const float* rows;
  int64_t n_rows;
  const isl_sign_aug_item* items;
  float* out;
  int F, T, nb, nh, npair, nunit;   // npair = nb + n_slots * nh; nunit = npair + n_slots * nh
  uint32_t thr_drop;                // a frame is dropped iff (k >> 40) < thr; 0: never
  double jitter;                    // 0: off
  uint64_t key;                     // sm(seed ^ step)
};

// the splitmix64 finaliser of section 4.2k (sign_train.hip's st_sm; a copy, so that file's code
// object stays as it was)
__host__ __device__ __forceinline__ uint64_t sa_sm(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint32_t sa_draw(uint64_t kw, uint32_t site, uint32_t index) {
  return (uint32_t)(sa_sm(kw ^ ((uint64_t)site << 32 | index)) >> 40);
}

__global__ __launch_bounds__(SA_BLOCK) void sign_augment_kernel(SignAugArgs a) {
  const isl_sign_aug_item it = a.items[blockIdx.x];
  const int T = a.T, F = a.F;
  float* out = a.out + (size_t)blockIdx.x * T * F;
  // row0 + nrows <= n_rows without forming the sum (nrows >= 1 and n_rows >= 0 are checked first)
  const bool item_ok = it.nrows >= 1 && it.q >= 8 && it.q <= 32 && it.row0 >= 0 && it.row0 <= a.n_rows - it.nrows;
  const float* src = a.rows + (item_ok ? (size_t)it.row0 * F : 0);
  const uint64_t kw = sa_sm(a.key ^ it.id);

  for (int i = threadIdx.x; i < T * a.nunit; i += SA_BLOCK) {
    const int t = i / a.nunit, u = i - t * a.nunit;
    // r = floor(num / 32) + start; num >= -31 * 32 + 16, so num + 2048 > 0 and the division is a floor
    const int num = (2 * t - (T - 1)) * it.q + 16 * (T - 1) + 16;
    const int64_t r = (int64_t)((num + 2048) / 32 - 64) + it.start;
    bool live = item_ok && r >= 0 && r < it.nrows;
    if (live && a.thr_drop) live = sa_draw(kw, SA_SITE_DROP, (uint32_t)t) >= a.thr_drop;
    const float* row = src + (live ? (size_t)r * F : 0);   // dereferenced only when live
    float* dst = out + (size_t)t * F;
    if (u >= a.npair) {                                    // a label: slot s, entry o
      const int v = u - a.npair, s = v / a.nh, o = v - s * a.nh;
      const int e = 2 * a.nb + s * 3 * a.nh + 2 * a.nh + o;
      dst[e] = live ? row[e] : 0.0f;
      continue;
    }
    int ex = u, ey = a.nb + u;                             // a body pair
    if (u >= a.nb) {                                       // a hand pair: slot s, entry o
      const int v = u - a.nb, s = v / a.nh, o = v - s * a.nh;
      ex = 2 * a.nb + s * 3 * a.nh + o;
      ey = ex + a.nh;
    }
    float X = 0.0f, Y = 0.0f;
    if (live) {
      const float x = row[ex], y = row[ey];
      if (x != 0.0f || y != 0.0f) {                        // a present pair (NaN counts as present)
        double dx = (it.m[0] * (double)x + it.m[1] * (double)y) + it.m[2];
        double dy = (it.m[3] * (double)x + it.m[4] * (double)y) + it.m[5];
        if (a.jitter > 0.0) {
          const uint32_t j = (uint32_t)(t * 512 + 2 * u);
          dx = dx + a.jitter * ((double)sa_draw(kw, SA_SITE_JITTER, j) * 0x1p-23 - 1.0);
          dy = dy + a.jitter * ((double)sa_draw(kw, SA_SITE_JITTER, j + 1) * 0x1p-23 - 1.0);
        }
        X = (float)dx;
        Y = (float)dy;
        if (X == 0.0f && Y == 0.0f) X = 0x1p-10f;          // a present point never turns absent
      }
    }
    dst[ex] = X;
    dst[ey] = Y;
  }
}

static int sa_fail(const std::string& msg) {
  set_error("isl_sign_augment: " + msg);
  return ISL_E_ARG;
}

}  // namespace isl

using namespace isl;

extern "C" int isl_sign_aug_opts_default(isl_sign_aug_opts* opts) {
  if (!opts) {
    set_error("isl_sign_aug_opts_default: NULL opts");
    return ISL_E_ARG;
  }
  *opts = isl_sign_aug_opts{};
  return ISL_OK;
}

extern "C" int isl_sign_augment(const float* d_rows, int64_t n_rows, int n_features, const isl_sign_aug_layout* layout,
                                const isl_sign_aug_item* d_items, int n_items, int window,
                                const isl_sign_aug_opts* opts, float* d_windows, void* stream) {
  if (n_items < 0 || n_items > SA_ITEMS_MAX)
    return sa_fail("n_items = " + std::to_string(n_items) + " outside [0, 65535]");
  if (n_items == 0) return ISL_OK;
  if (!d_rows || !layout || !d_items || !opts || !d_windows) return sa_fail("NULL pointer");
  if (n_rows < 0) return sa_fail("n_rows is negative");
  if (window < 1 || window > SA_TMAX || n_features < 1 || n_features > SA_FMAX)
    return sa_fail("window must be in [1, 32] and n_features in [1, 256]");
  if (layout->n_body < 0 || layout->n_slots < 0 || layout->n_hand < 0 || layout->reserved != 0)
    return sa_fail("layout counts must be >= 0 and its reserved field zero");
  // every count is at most n_features here or the size cannot match: compare in 64 bits
  const int64_t hand = (int64_t)layout->n_slots * layout->n_hand;
  if (2 * (int64_t)layout->n_body + 3 * hand != n_features)
    return sa_fail("layout (" + std::to_string(layout->n_body) + ", " + std::to_string(layout->n_slots) + ", " +
                   std::to_string(layout->n_hand) + ") does not have " + std::to_string(n_features) + " features");
  if (!(opts->drop >= 0.0f && opts->drop <= SA_DROP_MAX)) return sa_fail("drop must be a number in [0, 0.9]");
  if (!(std::isfinite(opts->jitter) && opts->jitter >= 0.0f)) return sa_fail("jitter must be finite and >= 0");
  for (int i = 0; i < 4; ++i)
    if (opts->reserved[i] != 0) return sa_fail("opts reserved fields must be zero");

  SignAugArgs a{};
  a.rows = d_rows;
  a.n_rows = n_rows;
  a.items = d_items;
  a.out = d_windows;
  a.F = n_features;
  a.T = window;
  a.nb = layout->n_body;
  a.nh = layout->n_hand;
  a.npair = layout->n_body + (int)hand;
  a.nunit = a.npair + (int)hand;
  // dropped iff (k >> 40) < round(drop * 2^24): the product is exact in fp64, halves round up
  a.thr_drop = (uint32_t)std::floor((double)opts->drop * 16777216.0 + 0.5);
  a.jitter = (double)opts->jitter;
  a.key = sa_sm(opts->seed ^ opts->step);
  hipLaunchKernelGGL(sign_augment_kernel, dim3((unsigned)n_items), dim3(SA_BLOCK), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string("isl_sign_augment: ") + hipGetErrorString(e));
    return ISL_E_HIP;
  }
  return ISL_OK;
}
