// Sign classifier of ISLSignPosTranslator (reference demo_isl_translate.py:72-100,
// called from src/ISL_Model_parameter.py:337): one workgroup per 20-frame window of
// 156-d keypoint features, the whole keras stack in one launch:
//
//   Masking(0) -> BatchNorm -> Bidirectional(LSTM 32, return_sequences)
//   -> Bidirectional(LSTM 32) -> elu -> Dense 32 -> BN -> elu -> Dense 32 -> BN
//   -> elu -> Dense n_classes + softmax                 (Dropouts: inference no-ops)
//
// Keras semantics kept: a frame is masked when every feature is exactly 0
// (Masking); masked steps carry (h, c) and, in the return_sequences layer, emit
// zeros (Bidirectional sets zero_output_for_mask = return_sequences); the
// backward direction walks the window in reverse and its sequence output is
// stored at the original time index; the mask propagates to the second layer.
// LSTM gates in keras order (i, f, c, o), sigmoid / tanh; BN eps = 1e-3.
//
// Thread map (1024 lanes = 16 waves): lane % 256 = direction * 128 + gate-row.  The
// input projection x_t @ K is split over four step ranges (lane / 256), one pass over
// K each (coalesced over the gate row, x broadcast from LDS); the recurrence (lanes
// < 256) keeps the lane's column of the
// recurrent kernel in 32 VGPRs and needs two barriers per step (gate
// activations, then the 64 (direction, unit) cell updates).  The work is tiny
// (≈2 MFLOP per window) and latency-bound; the point of the kernel is one launch
// per batch of windows instead of hundreds of framework ops.
#include <string>

#include "internal.h"
#include "islpose.h"
#include "sign_common.h"

namespace isl {

__global__ __launch_bounds__(SC_BLOCK) void sign_classify_kernel(SignArgs a) {
  __shared__ __attribute__((aligned(16))) float s_x[SC_TMAX * SC_FMAX];          // 32 KB: window, then BN'd
  __shared__ float s_z[SC_TMAX * SC_THREADS];       // 32 KB: projected gates
  __shared__ __attribute__((aligned(16))) float s_seq[SC_TMAX * 2 * SC_U];       //  8 KB: layer-1 sequence
  __shared__ float s_h[2][SC_U];
  __shared__ float s_act[2][SC_G];
  __shared__ int s_mask[SC_TMAX];
  __shared__ float s_v[2 * SC_U], s_y[SC_D], s_y2[SC_D];
  __shared__ float s_logit[SC_CMAX];
  __shared__ float s_red[SC_THREADS / 64];

  const int tid = threadIdx.x, lt = tid % SC_THREADS, tq = tid / SC_THREADS;
  const int d = lt / SC_G, g = lt % SC_G;
  const bool hw = tid < SC_THREADS;   // the head's lanes
  const int T = a.T, F = a.F, C = a.C;
  const float* x = a.x + (size_t)blockIdx.x * T * F;

  if (tid < SC_TMAX) s_mask[tid] = 0;
  __syncthreads();
  for (int i = tid; i < T * F; i += SC_BLOCK) {
    const float v = x[i];
    s_x[i] = v;
    if (v != 0.0f) s_mask[i / F] = 1;               // Masking(mask_value=0.)
  }
  __syncthreads();
  for (int i = tid; i < T * F; i += SC_BLOCK) s_x[i] = sc_bn(a.bn0, F, i % F, s_x[i]);
  __syncthreads();

  // layer 1: Bidirectional(LSTM(32, return_sequences=True))
  sc_project(s_x, F, T, a.k1[d], a.b1[d], g, tq, s_z + d * SC_G + g);
  __syncthreads();
  sc_recur<false>(s_z, s_mask, T, a.r1[d], d, g, tid, s_h, s_act, s_seq, s_v, SignTape{});

  // layer 2: Bidirectional(LSTM(32)) over the 64-wide sequence
  sc_project(s_seq, 2 * SC_U, T, a.k2[d], a.b2[d], g, tq, s_z + d * SC_G + g);
  __syncthreads();
  sc_recur<false>(s_z, s_mask, T, a.r2[d], d, g, tid, s_h, s_act, nullptr, s_v, SignTape{});

  // head: elu -> Dense -> BN -> elu -> Dense -> BN -> elu -> Dense + softmax
  if (tid < 2 * SC_U) s_v[tid] = sc_elu(s_v[tid]);
  __syncthreads();
  if (tid < SC_D) {
    float acc = 0.0f;
    for (int i = 0; i < 2 * SC_U; ++i) acc += s_v[i] * a.d1[i * SC_D + tid];
    s_y[tid] = sc_elu(sc_bn(a.bn1, SC_D, tid, acc));
  }
  __syncthreads();
  if (tid < SC_D) {
    float acc = 0.0f;
    for (int i = 0; i < SC_D; ++i) acc += s_y[i] * a.d2[i * SC_D + tid];
    s_y2[tid] = sc_elu(sc_bn(a.bn2, SC_D, tid, acc));
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int c = tid; hw && c < C; c += SC_THREADS) {
    const float acc = sc_logit(s_y2, a.d3, a.b3, C, c);
    s_logit[c] = acc;
    mx = fmaxf(mx, acc);
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if (hw && (tid & 63) == 0) s_red[tid / 64] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  __syncthreads();
  float sum = 0.0f;
  for (int c = tid; hw && c < C; c += SC_THREADS) {
    const float e = expf(s_logit[c] - mx);
    s_logit[c] = e;
    sum += e;
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (hw && (tid & 63) == 0) s_red[tid / 64] = sum;
  __syncthreads();
  sum = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  float* out = a.out + (size_t)blockIdx.x * C;
  for (int c = tid; hw && c < C; c += SC_THREADS) out[c] = s_logit[c] / sum;
}

}  // namespace isl

using namespace isl;

extern "C" int isl_sign_param_count(int n_features, int n_classes, int64_t* count) {
  if (n_features <= 0 || n_features > SC_FMAX || n_classes <= 0 || n_classes > SC_CMAX || !count) {
    set_error("isl_sign_param_count: n_features must be in [1, 256] and n_classes in [1, 1024]");
    return ISL_E_ARG;
  }
  *count = sign_layout(n_features, n_classes, nullptr, nullptr);
  return ISL_OK;
}

extern "C" int isl_sign_classify(const float* d_params, int n_features, int window, int n_classes,
                                 const float* d_windows, int batch, float* d_probs, void* stream) {
  if (batch == 0) return ISL_OK;
  if (!d_params || !d_windows || !d_probs || batch < 0 || window <= 0 || window > SC_TMAX || n_features <= 0 ||
      n_features > SC_FMAX || n_classes <= 0 || n_classes > SC_CMAX) {
    set_error("isl_sign_classify: bad argument (window <= 32, n_features <= 256, n_classes <= 1024)");
    return ISL_E_ARG;
  }
  SignArgs a{};
  a.x = d_windows;
  a.out = d_probs;
  a.T = window;
  a.F = n_features;
  a.C = n_classes;
  sign_layout(n_features, n_classes, &a, d_params);
  hipLaunchKernelGGL(sign_classify_kernel, dim3(batch), dim3(SC_BLOCK), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string("sign_classify_kernel: ") + hipGetErrorString(e));
    return ISL_E_HIP;
  }
  return ISL_OK;
}
