// Forward arithmetic of the sign classifier, shared by the inference kernel (sign.hip) and the
// training kernel (sign_train.hip): both run the same operations in the same order, so a
// window's logits at inference are those the training step differentiates (dropouts off).
//
// Thread map (1024 lanes = 16 waves): lane % 256 = direction * 128 + gate-row.  The
// input projection x_t @ K is split over four step ranges (lane / 256), one pass over
// K each (coalesced over the gate row, x broadcast from LDS); the recurrence (lanes
// < 256) keeps the lane's column of the recurrent kernel in 32 VGPRs and needs two
// barriers per step (gate activations, then the 64 (direction, unit) cell updates).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace isl {

constexpr int SC_U = 32;            // LSTM units (reference: LSTM(32))
constexpr int SC_G = 4 * SC_U;      // gate rows per direction
constexpr int SC_D = 32;            // Dense widths of the head
constexpr int SC_TMAX = 32;         // longest window
constexpr int SC_FMAX = 256;        // widest feature vector
constexpr int SC_CMAX = 1024;       // most classes
constexpr int SC_THREADS = 2 * SC_G;  // lanes of the recurrence: (direction, gate row)
constexpr int SC_BLOCK = 4 * SC_THREADS; // the projections also split the window in 4 step ranges
constexpr int SC_TQT = SC_TMAX / 4;      // steps per range
constexpr float SC_EPS = 1e-3f;     // keras BatchNormalization epsilon

struct SignArgs {
  const float* x;        // [batch, T, F]
  float* out;            // [batch, C] softmax probabilities
  int T, F, C;
  const float* bn0;      // gamma, beta, mean, var  [4][F]
  const float* k1[2];    // [F][4U]
  const float* r1[2];    // [U][4U]
  const float* b1[2];    // [4U]
  const float* k2[2];    // [2U][4U]
  const float* r2[2];
  const float* b2[2];
  const float* d1;       // [2U][D]
  const float* bn1;      // [4][D]
  const float* d2;       // [D][D]
  const float* bn2;      // [4][D]
  const float* d3;       // [D][C]
  const float* b3;       // [C]
};

// What the training kernel keeps of one layer's recurrence for its backward pass (the
// inference kernel passes none of it).  rm: the recurrent-dropout factor of each
// (direction, unit), 1 when off; hm: the carried h times rm, which the recurrent product reads;
// acts: the gate activations, written over the projected gates [T][2][4U] they came from;
// thm, tc: the carried h times rm, and the carried c, after each walk step [T][2][U].
struct SignTape {
  const float (*rm)[SC_U];
  float (*hm)[SC_U];
  float* acts;
  float* thm;
  float* tc;
};

__device__ __forceinline__ float sc_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }
__device__ __forceinline__ float sc_elu(float v) { return v > 0.0f ? v : expm1f(v); }
__device__ __forceinline__ float sc_bn(const float* p, int n, int j, float v) {
  // keras: (x - mean) * rsqrt(var + eps) * gamma + beta
  return (v - p[2 * n + j]) / sqrtf(p[3 * n + j] + SC_EPS) * p[j] + p[n + j];
}

// Logit of class c: the 32 products summed in order, then the bias.  The bias goes last: a sum
// that starts at b3[c] rounds every partial at the bias's magnitude, and a large bias (a softmax is
// blind to a shift common to all classes) then costs its ulp 32 times instead of once.
__device__ __forceinline__ float sc_logit(const float* y2, const float* d3, const float* b3, int C, int c) {
  float acc = 0.0f;
  for (int i = 0; i < SC_D; ++i) acc += y2[i] * d3[i * C + c];
  return acc + b3[c];
}

// z[t][d][g] = b[g] + sum_f in[t][f] * K[f][g] (one lane per (d, g, range of 8 steps)).
// A lone window is latency-bound: 1024 lanes on one CU, four K rows per iteration and
// 16-byte LDS reads of the inputs; the sum over f keeps its order.
__device__ void sc_project(const float* in, int F, int T, const float* K, const float* b, int g, int tq,
                           float* zrow) {
  const int tb = tq * SC_TQT;
  if (tb >= T) return;
  float acc[SC_TQT];
  const float bias = b[g];
#pragma unroll
  for (int k = 0; k < SC_TQT; ++k) acc[k] = bias;
  if ((F & 3) == 0) {
#pragma unroll 4
    for (int f = 0; f < F; f += 4) {
      const float w0 = K[(size_t)f * SC_G + g], w1 = K[(size_t)(f + 1) * SC_G + g];
      const float w2 = K[(size_t)(f + 2) * SC_G + g], w3 = K[(size_t)(f + 3) * SC_G + g];
#pragma unroll
      for (int k = 0; k < SC_TQT; ++k)
        if (tb + k < T) {
          const float4 v = *(const float4*)(in + (tb + k) * F + f);
          acc[k] = (((acc[k] + v.x * w0) + v.y * w1) + v.z * w2) + v.w * w3;
        }
    }
  } else {
    for (int f = 0; f < F; ++f) {
      const float w = K[(size_t)f * SC_G + g];
#pragma unroll
      for (int k = 0; k < SC_TQT; ++k)
        if (tb + k < T) acc[k] += in[(tb + k) * F + f] * w;
    }
  }
#pragma unroll
  for (int k = 0; k < SC_TQT; ++k)
    if (tb + k < T) zrow[(tb + k) * SC_THREADS] = acc[k];
}

// One bidirectional LSTM layer over s_z (projected inputs); seq != nullptr writes
// the return_sequences output [T][2U] (zeros at masked steps); h_last gets the
// final (carried) hidden state of each direction.  TRAIN: the recurrent product reads
// tape.hm (h times the recurrent-dropout factor) and the tape is filled.
template <bool TRAIN>
__device__ void sc_recur(const float* s_z, const int* s_mask, int T, const float* R, int d, int g, int tid,
                         float (*s_h)[SC_U], float (*s_act)[SC_G], float* seq, float* h_last,
                         const SignTape& tape) {
  const bool act = tid < SC_THREADS;     // the other lanes only keep the barriers
  float r[SC_U];
#pragma unroll
  for (int k = 0; k < SC_U; ++k) r[k] = act ? R[k * SC_G + g] : 0.0f;
  const int gate = g / SC_U;
  float c = 0.0f;
  if (tid < 2 * SC_U) {
    s_h[tid / SC_U][tid % SC_U] = 0.0f;
    if (TRAIN) tape.hm[tid / SC_U][tid % SC_U] = 0.0f;
  }
  __syncthreads();
  const float (*hsrc)[SC_U] = TRAIN ? tape.hm : s_h;
  for (int s = 0; s < T; ++s) {
    if (act) {
      const int t = d == 0 ? s : T - 1 - s;
      float z = s_z[t * SC_THREADS + d * SC_G + g];
#pragma unroll
      for (int k = 0; k < SC_U; ++k) z += hsrc[d][k] * r[k];
      const float a = gate == 2 ? tanhf(z) : sc_sigmoid(z);
      s_act[d][g] = a;
      if (TRAIN) tape.acts[t * SC_THREADS + d * SC_G + g] = a;
    }
    __syncthreads();
    if (tid < 2 * SC_U) {
      const int dd = tid / SC_U, u = tid % SC_U;
      const int tt = dd == 0 ? s : T - 1 - s;
      float h = 0.0f;
      if (s_mask[tt]) {
        c = s_act[dd][SC_U + u] * c + s_act[dd][u] * s_act[dd][2 * SC_U + u];
        h = s_act[dd][3 * SC_U + u] * tanhf(c);
        s_h[dd][u] = h;
        if (TRAIN) tape.hm[dd][u] = h * tape.rm[dd][u];
      }
      if (seq) seq[tt * 2 * SC_U + dd * SC_U + u] = h;
      if (TRAIN) {
        tape.tc[s * 2 * SC_U + tid] = c;
        tape.thm[s * 2 * SC_U + tid] = tape.hm[dd][u];
      }
    }
    __syncthreads();
  }
  if (tid < 2 * SC_U) h_last[tid] = s_h[tid / SC_U][tid % SC_U];
  __syncthreads();
}

// Offsets of keras `model.get_weights()` (Sequential order) in the flat buffer.
static int64_t sign_layout(int F, int C, SignArgs* a, const float* p) {
  int64_t o = 0;
  auto take = [&](int64_t n) { const float* q = p ? p + o : nullptr; o += n; return q; };
  const float* bn0 = take(4LL * F);
  const float *k1[2], *r1[2], *b1[2], *k2[2], *r2[2], *b2[2];
  for (int d = 0; d < 2; ++d) { k1[d] = take((int64_t)F * SC_G); r1[d] = take(SC_U * SC_G); b1[d] = take(SC_G); }
  for (int d = 0; d < 2; ++d) { k2[d] = take(2 * SC_U * SC_G); r2[d] = take(SC_U * SC_G); b2[d] = take(SC_G); }
  const float* d1 = take(2 * SC_U * SC_D);
  const float* bn1 = take(4 * SC_D);
  const float* d2 = take(SC_D * SC_D);
  const float* bn2 = take(4 * SC_D);
  const float* d3 = take((int64_t)SC_D * C);
  const float* b3 = take(C);
  if (a) {
    a->bn0 = bn0; a->d1 = d1; a->bn1 = bn1; a->d2 = d2; a->bn2 = bn2; a->d3 = d3; a->b3 = b3;
    for (int d = 0; d < 2; ++d) {
      a->k1[d] = k1[d]; a->r1[d] = r1[d]; a->b1[d] = b1[d];
      a->k2[d] = k2[d]; a->r2[d] = r2[d]; a->b2[d] = b2[d];
    }
  }
  return o;
}

}  // namespace isl
