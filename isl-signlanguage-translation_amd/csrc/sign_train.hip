// Training step of the sign classifier (isl_sign_grad): per window the
// forward of sign.hip with the training-time Dropouts, the sparse categorical cross-entropy, and
// the backward pass through both bidirectional LSTM layers, in one workgroup.
//
// The forward keeps in LDS what the backward needs (sign_common.h SignTape): per layer the gate
// activations, written over the projected gates they came from, and the carried (h, c) after every
// walk step; the normalised input; the layer-1 sequence after Dropout_A.  The backward overwrites
// the activations of a step with dz of that step, so after a layer's recurrence its [T][2][4U]
// buffer holds dz, from which the input-kernel gradients (sum over t of x_t[f] * dz_t[g]) and the
// gradient of the layer's input (K dz_t) are computed over all 1024 lanes.
//
// LDS at the limits (T 32, F 256, C 1024): input 32 KB, two gate buffers 64 KB, four (h, c) tapes
// 32 KB, sequence and its gradient 16 KB, logits 4 KB, about 4 KB of vectors: under 156 KB of the
// CU's 160 KB, one workgroup per CU.
//
// Every gradient element has one owner lane per workgroup.  Workgroup j of G = min(batch, 256)
// takes windows j, j + G, ... in order and adds each one's gradient, already scaled by w_b / B,
// into slice j of the workspace (the first window stores, the others read-modify-write); a second
// launch adds the G slices in index order.  No float atomics, no waits between workgroups.
#include <cmath>
#include <string>

#include "internal.h"
#include "islpose.h"
#include "sign_common.h"

namespace isl {

constexpr int ST_GMAX = 256;        // most workgroups (gradient slices)
constexpr float ST_RATE_MAX = 0.9f;

struct SignTrainArgs {
  SignArgs w;            // the parameters; w.x the windows, w.out unused
  const float* params;   // base of the parameters: a gradient sits at the same offset in its slice
  float* ws;             // G slices of P floats
  int64_t P;             // floats per slice
  const int32_t* labels;
  const float* weights;  // or nullptr
  const uint64_t* ids;   // or nullptr
  float* loss;
  int batch, G;
  float inv_batch;
  uint32_t thr_drop, thr_rec;     // keep iff (k >> 40) >= thr; 0: the site is off
  float scale_drop, scale_rec;    // 1.0f / (1.0f - rate); 1 when off
  uint64_t key;                   // sm(seed ^ step)
};

__host__ __device__ __forceinline__ uint64_t st_sm(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the factor of one dropout element: kw = sm(sm(seed ^ step) ^ sample_id)
__device__ __forceinline__ float st_keep(uint64_t kw, uint32_t site, uint32_t index, uint32_t thr, float scale) {
  const uint64_t k = st_sm(kw ^ ((uint64_t)site << 32 | index));
  return (uint32_t)(k >> 40) >= thr ? scale : 0.0f;
}

__device__ __forceinline__ void st_add(float* p, float v, bool first) { *p = first ? v : *p + v; }
__device__ __forceinline__ float st_delu(float pre) { return pre > 0.0f ? 1.0f : expf(pre); }   // d elu / d pre

// Backward of one bidirectional layer.  s_z: the gate activations [T][2][4U], replaced step by step
// with dz (zeros at masked steps).  Cell lanes (tid < 64: direction, unit) carry dh and dc; dh_init
// (or nullptr) is the gradient of the final carried h, dext (or nullptr) that of the sequence output
// [T][2U].  Lanes < 256 own, as (direction, gate row), the 32 recurrent-kernel gradients of their
// column and the bias gradient; lanes 256..511 compute, as (direction, unit, quarter of the gate
// rows), a quarter of dh_{t-1}[unit] = sum_g R[unit][g] dz[g], added across the four lanes by shuffles.
__device__ void st_recur_bwd(float* s_z, const int* s_mask, int T, const float* R, int d, int g, int tid,
                             const float* thm, const float* tc, const float (*rm)[SC_U], float (*s_dh)[SC_U],
                             const float* dh_init, const float* dext, float* gR, float* gb, bool first) {
  const bool bl = tid < SC_THREADS;              // owners of dR and db
  const bool hl = !bl && tid < 2 * SC_THREADS;   // the dh_{t-1} lanes
  const int ku = g / 4, kq = g % 4;              // their (unit, quarter)
  float rd[SC_U];                                // bl: dR[k][g]; hl: R[ku][4 j + kq] (four lanes, four banks)
#pragma unroll
  for (int j = 0; j < SC_U; ++j) rd[j] = hl ? R[ku * SC_G + 4 * j + kq] : 0.0f;
  float db = 0.0f;
  const int dd = tid / SC_U, u = tid % SC_U;     // cell lanes
  float dh = (tid < 2 * SC_U && dh_init) ? dh_init[tid] : 0.0f, dc = 0.0f;
  for (int s = T - 1; s >= 0; --s) {
    if (tid < 2 * SC_U) {
      const int tt = dd == 0 ? s : T - 1 - s;
      float* a = s_z + tt * SC_THREADS + dd * SC_G;
      float dzi = 0.0f, dzf = 0.0f, dzg = 0.0f, dzo = 0.0f;
      if (s_mask[tt]) {
        const float dht = dext ? dh + dext[tt * 2 * SC_U + tid] : dh;
        const float gi = a[u], gf = a[SC_U + u], gg = a[2 * SC_U + u], go = a[3 * SC_U + u];
        const float ct = tc[s * 2 * SC_U + tid], cp = s > 0 ? tc[(s - 1) * 2 * SC_U + tid] : 0.0f;
        const float tch = tanhf(ct);
        const float dct = dc + dht * go * (1.0f - tch * tch);
        dzo = dht * tch * go * (1.0f - go);
        dzi = dct * gg * gi * (1.0f - gi);
        dzf = dct * cp * gf * (1.0f - gf);
        dzg = dct * gi * (1.0f - gg * gg);
        dc = dct * gf;
      }
      a[u] = dzi;
      a[SC_U + u] = dzf;
      a[2 * SC_U + u] = dzg;
      a[3 * SC_U + u] = dzo;
    }
    __syncthreads();
    const int t = d == 0 ? s : T - 1 - s;
    const float* dz = s_z + t * SC_THREADS + d * SC_G;
    if (bl && s_mask[t]) {                       // uniform over a wave: d is
      const float mine = dz[g];
      db += mine;
      if (s > 0) {
        const float* hp = thm + (s - 1) * 2 * SC_U + d * SC_U;
#pragma unroll
        for (int k = 0; k < SC_U; ++k) rd[k] += hp[k] * mine;
      }
    }
    if (hl && s_mask[t]) {
      float p = 0.0f;
#pragma unroll
      for (int j = 0; j < SC_U; ++j) p += rd[j] * dz[4 * j + kq];
      p += __shfl_xor(p, 1);
      p += __shfl_xor(p, 2);
      if (kq == 0) s_dh[d][ku] = p * rm[d][ku];
    }
    __syncthreads();
    if (tid < 2 * SC_U && s_mask[dd == 0 ? s : T - 1 - s]) dh = s_dh[dd][u];
  }
  if (bl) {
#pragma unroll
    for (int k = 0; k < SC_U; ++k) st_add(gR + k * SC_G + g, rd[k], first);
    st_add(gb + g, db, first);
  }
  __syncthreads();
}

// Input-kernel gradient of one direction's gate row: gK[f][g] = sum_t in[t][f] * dz[t][d][g], the
// lane's step range of the projection now a range of 16 features out of every 64.
__device__ void st_dkernel(const float* in, int Fin, int T, const int* s_mask, const float* dzcol, int fq,
                           float* gK, bool first) {
  for (int f0 = fq * 16; f0 < Fin; f0 += 64) {
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
    for (int t = 0; t < T; ++t) {
      if (!s_mask[t]) continue;
      const float dz = dzcol[t * SC_THREADS];
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (f0 + j < Fin) acc[j] += in[t * Fin + f0 + j] * dz;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (f0 + j < Fin) st_add(gK + (size_t)(f0 + j) * SC_G, acc[j], first);
  }
}

// Gradient of a layer's input: acc[k] = sum_{d, g} K[d][f][g] * dz[t][d][g] at t = tq + 4 k, for the
// lane's feature f < Fin (the caller checks) and step range tq.
__device__ void st_dinput(const float* K0, const float* K1, int f, int tq, int T, const float* s_dz, float* acc) {
#pragma unroll
  for (int k = 0; k < SC_TQT; ++k) acc[k] = 0.0f;
  for (int d = 0; d < 2; ++d) {
    const float* K = (d == 0 ? K0 : K1) + (size_t)f * SC_G;
    for (int g4 = 0; g4 < SC_G; g4 += 4) {
      const float4 kv = make_float4(K[g4], K[g4 + 1], K[g4 + 2], K[g4 + 3]);
#pragma unroll
      for (int k = 0; k < SC_TQT; ++k) {
        const int t = tq + 4 * k;
        if (t < T) {
          const float4 v = *(const float4*)(s_dz + t * SC_THREADS + d * SC_G + g4);
          acc[k] = (((acc[k] + kv.x * v.x) + kv.y * v.y) + kv.z * v.z) + kv.w * v.w;
        }
      }
    }
  }
}

__global__ __launch_bounds__(SC_BLOCK) void sign_grad_kernel(SignTrainArgs a) {
  __shared__ __attribute__((aligned(16))) float s_x[SC_TMAX * SC_FMAX];        // 32 KB: window, then BN'd
  __shared__ __attribute__((aligned(16))) float s_z1[SC_TMAX * SC_THREADS];    // 32 KB: layer-1 gates -> acts -> dz
  __shared__ __attribute__((aligned(16))) float s_z2[SC_TMAX * SC_THREADS];    // 32 KB: layer-2 the same
  __shared__ float s_th1[SC_TMAX * 2 * SC_U], s_tc1[SC_TMAX * 2 * SC_U];       // 16 KB: carried h * rm, c per walk step
  __shared__ float s_th2[SC_TMAX * 2 * SC_U], s_tc2[SC_TMAX * 2 * SC_U];       // 16 KB
  __shared__ __attribute__((aligned(16))) float s_seq[SC_TMAX * 2 * SC_U];     //  8 KB: layer-1 sequence after Dropout_A
  __shared__ __attribute__((aligned(16))) float s_dseq[SC_TMAX * 2 * SC_U];    //  8 KB: its gradient; then BN0 partials
  __shared__ float s_logit[SC_CMAX];                                           //  4 KB: logits, then dL/dlogits
  __shared__ float s_h[2][SC_U], s_hm[2][SC_U], s_dh[2][SC_U];
  __shared__ float s_rm[4][SC_U];                  // recurrent-dropout factors: layer * 2 + direction
  __shared__ float s_act[2][SC_G];
  __shared__ int s_mask[SC_TMAX];
  __shared__ float s_v[2 * SC_U], s_hl[2 * SC_U], s_dv[2 * SC_U];
  __shared__ float s_y[SC_D], s_y2[SC_D], s_p1[SC_D], s_p2[SC_D], s_m1[SC_D], s_m2[SC_D];
  __shared__ float s_xh1[SC_D], s_xh2[SC_D], s_da[SC_D], s_dy[SC_D];
  __shared__ float s_red[SC_THREADS / 64];
  __shared__ float s_scale;

  const int tid = threadIdx.x, lt = tid % SC_THREADS, tq = tid / SC_THREADS;
  const int d = lt / SC_G, g = lt % SC_G;
  const bool hw = tid < SC_THREADS;   // the head's lanes
  const int T = a.w.T, F = a.w.F, C = a.w.C;
  const SignArgs& w = a.w;
  const size_t so = (size_t)blockIdx.x * a.P;       // this workgroup's gradient slice
  auto G_ = [&](const float* p) { return a.ws + so + (p - a.params); };

  bool first = true;
  for (int b = blockIdx.x; b < a.batch; b += a.G, first = false) {
    const float* x = w.x + (size_t)b * T * F;
    const uint64_t kw = st_sm(a.key ^ (a.ids ? a.ids[b] : (uint64_t)b));

    __syncthreads();                                // the previous window's LDS is no longer read
    if (tid < SC_TMAX) s_mask[tid] = 0;
    if (tid < 4 * SC_U) s_rm[tid / SC_U][tid % SC_U] = st_keep(kw, 3 + tid / SC_U, tid % SC_U, a.thr_rec, a.scale_rec);
    __syncthreads();
    for (int i = tid; i < T * F; i += SC_BLOCK) {
      const float v = x[i];
      s_x[i] = v;
      if (v != 0.0f) s_mask[i / F] = 1;               // Masking(mask_value=0.)
    }
    __syncthreads();
    for (int i = tid; i < T * F; i += SC_BLOCK) s_x[i] = sc_bn(w.bn0, F, i % F, s_x[i]);
    __syncthreads();

    // ---- forward: the arithmetic of sign_classify_kernel, taped
    sc_project(s_x, F, T, w.k1[d], w.b1[d], g, tq, s_z1 + d * SC_G + g);
    __syncthreads();
    sc_recur<true>(s_z1, s_mask, T, w.r1[d], d, g, tid, s_h, s_act, s_seq, s_v,
                   SignTape{s_rm, s_hm, s_z1, s_th1, s_tc1});
    if (a.thr_drop) {                                 // Dropout_A, index t * 64 + j
      for (int i = tid; i < T * 2 * SC_U; i += SC_BLOCK) s_seq[i] *= st_keep(kw, 0, i, a.thr_drop, a.scale_drop);
      __syncthreads();
    }
    sc_project(s_seq, 2 * SC_U, T, w.k2[d], w.b2[d], g, tq, s_z2 + d * SC_G + g);
    __syncthreads();
    sc_recur<true>(s_z2, s_mask, T, w.r2[d], d, g, tid, s_h, s_act, nullptr, s_v,
                   SignTape{s_rm + 2, s_hm, s_z2, s_th2, s_tc2});

    // head: elu -> Dense -> BN -> Dropout_B -> elu -> Dense -> BN -> elu -> Dropout_C -> Dense
    if (tid < 2 * SC_U) {
      s_hl[tid] = s_v[tid];
      s_v[tid] = sc_elu(s_v[tid]);
    }
    __syncthreads();
    if (tid < SC_D) {
      float acc = 0.0f;
      for (int i = 0; i < 2 * SC_U; ++i) acc += s_v[i] * w.d1[i * SC_D + tid];
      const float m = st_keep(kw, 1, tid, a.thr_drop, a.scale_drop);
      const float pre = sc_bn(w.bn1, SC_D, tid, acc) * m;
      s_xh1[tid] = (acc - w.bn1[2 * SC_D + tid]) / sqrtf(w.bn1[3 * SC_D + tid] + SC_EPS);
      s_m1[tid] = m;
      s_p1[tid] = pre;
      s_y[tid] = sc_elu(pre);
    }
    __syncthreads();
    if (tid < SC_D) {
      float acc = 0.0f;
      for (int i = 0; i < SC_D; ++i) acc += s_y[i] * w.d2[i * SC_D + tid];
      const float m = st_keep(kw, 2, tid, a.thr_drop, a.scale_drop);
      const float pre = sc_bn(w.bn2, SC_D, tid, acc);
      s_xh2[tid] = (acc - w.bn2[2 * SC_D + tid]) / sqrtf(w.bn2[3 * SC_D + tid] + SC_EPS);
      s_m2[tid] = m;
      s_p2[tid] = pre;
      s_y2[tid] = sc_elu(pre) * m;
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int c = tid; hw && c < C; c += SC_THREADS) {
      const float acc = sc_logit(s_y2, w.d3, w.b3, C, c);
      s_logit[c] = acc;
      mx = fmaxf(mx, acc);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (hw && (tid & 63) == 0) s_red[tid / 64] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    __syncthreads();
    float sum = 0.0f;
    for (int c = tid; hw && c < C; c += SC_THREADS) sum += expf(s_logit[c] - mx);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (hw && (tid & 63) == 0) s_red[tid / 64] = sum;
    __syncthreads();
    sum = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    const int label = a.labels[b];
    const bool valid = label >= 0 && label < C;
    if (tid == 0) {
      a.loss[b] = valid ? logf(sum) - (s_logit[label] - mx) : 0.0f;   // logsumexp - logit, the small term first
      s_scale = valid ? (a.weights ? a.weights[b] : 1.0f) * a.inv_batch : 0.0f;
    }
    __syncthreads();
    const float scale = s_scale;

    // ---- backward.  dL/dlogit = scale * (softmax - onehot)
    for (int c = tid; hw && c < C; c += SC_THREADS)
      s_logit[c] = scale * (expf(s_logit[c] - mx) / sum - (c == label ? 1.0f : 0.0f));
    if (first) {                                     // frozen statistics: mean and variance get no gradient
      if (tid < F) G_(w.bn0)[2 * F + tid] = G_(w.bn0)[3 * F + tid] = 0.0f;
      if (tid < SC_D) {
        G_(w.bn1)[2 * SC_D + tid] = G_(w.bn1)[3 * SC_D + tid] = 0.0f;
        G_(w.bn2)[2 * SC_D + tid] = G_(w.bn2)[3 * SC_D + tid] = 0.0f;
      }
    }
    __syncthreads();
    for (int i = tid; i < SC_D * C; i += SC_BLOCK) st_add(G_(w.d3) + i, s_y2[i / C] * s_logit[i % C], first);
    for (int c = tid; c < C; c += SC_BLOCK) st_add(G_(w.b3) + c, s_logit[c], first);
    {
      const int i = tid / 32, q = tid % 32;          // 32 lanes per unit of the last hidden layer
      float p = 0.0f;
      for (int c = q; c < C; c += 32) p += w.d3[i * C + c] * s_logit[c];
      for (int o = 16; o > 0; o >>= 1) p += __shfl_xor(p, o);
      if (q == 0) s_dy[i] = p;
    }
    __syncthreads();
    if (tid < SC_D) {
      const float db = s_dy[tid] * s_m2[tid] * st_delu(s_p2[tid]);
      st_add(G_(w.bn2) + tid, db * s_xh2[tid], first);
      st_add(G_(w.bn2) + SC_D + tid, db, first);
      s_da[tid] = db * (w.bn2[tid] / sqrtf(w.bn2[3 * SC_D + tid] + SC_EPS));
    }
    __syncthreads();
    {
      const int i = tid / 32, j = tid % 32;
      st_add(G_(w.d2) + tid, s_y[i] * s_da[j], first);
      float p = w.d2[tid] * s_da[j];
      for (int o = 16; o > 0; o >>= 1) p += __shfl_xor(p, o);
      if (j == 0) s_dy[i] = p;
    }
    __syncthreads();
    if (tid < SC_D) {
      const float db = s_dy[tid] * st_delu(s_p1[tid]) * s_m1[tid];
      st_add(G_(w.bn1) + tid, db * s_xh1[tid], first);
      st_add(G_(w.bn1) + SC_D + tid, db, first);
      s_da[tid] = db * (w.bn1[tid] / sqrtf(w.bn1[3 * SC_D + tid] + SC_EPS));
    }
    __syncthreads();
    for (int e = tid; e < 2 * SC_U * SC_D; e += SC_BLOCK) {
      const int i = e / 32, j = e % 32;
      st_add(G_(w.d1) + e, s_v[i] * s_da[j], first);
      float p = w.d1[e] * s_da[j];
      for (int o = 16; o > 0; o >>= 1) p += __shfl_xor(p, o);
      if (j == 0) s_dv[i] = p * st_delu(s_hl[i]);    // through the first elu: gradient of the last carried h
    }
    __syncthreads();

    // layer 2
    st_recur_bwd(s_z2, s_mask, T, w.r2[d], d, g, tid, s_th2, s_tc2, s_rm + 2, s_dh, s_dv, nullptr,
                 G_(w.r2[d]), G_(w.b2[d]), first);
    st_dkernel(s_seq, 2 * SC_U, T, s_mask, s_z2 + d * SC_G + g, tq, G_(w.k2[d]) + g, first);
    if (lt < 2 * SC_U) {                             // gradient of the sequence, through Dropout_A
      float acc[SC_TQT];
      st_dinput(w.k2[0], w.k2[1], lt, tq, T, s_z2, acc);
#pragma unroll
      for (int k = 0; k < SC_TQT; ++k) {
        const int t = tq + 4 * k;
        if (t < T) s_dseq[t * 2 * SC_U + lt] = acc[k] * st_keep(kw, 0, t * 2 * SC_U + lt, a.thr_drop, a.scale_drop);
      }
    }
    __syncthreads();

    // layer 1
    st_recur_bwd(s_z1, s_mask, T, w.r1[d], d, g, tid, s_th1, s_tc1, s_rm, s_dh, nullptr, s_dseq,
                 G_(w.r1[d]), G_(w.b1[d]), first);
    st_dkernel(s_x, F, T, s_mask, s_z1 + d * SC_G + g, tq, G_(w.k1[d]) + g, first);
    // BN0 gamma and beta: four partial sums over the steps per feature, added in order
    float pg = 0.0f, pb = 0.0f;
    if (lt < F) {
      float acc[SC_TQT];
      st_dinput(w.k1[0], w.k1[1], lt, tq, T, s_z1, acc);
      const float mean = w.bn0[2 * F + lt], sd = sqrtf(w.bn0[3 * F + lt] + SC_EPS);
#pragma unroll
      for (int k = 0; k < SC_TQT; ++k) {
        const int t = tq + 4 * k;
        if (t < T) {
          pg += acc[k] * ((x[t * F + lt] - mean) / sd);
          pb += acc[k];
        }
      }
    }
    __syncthreads();                                 // layer 1's reads of s_dseq are over
    s_dseq[tq * SC_THREADS + lt] = pg;
    s_dseq[SC_BLOCK + tq * SC_THREADS + lt] = pb;
    __syncthreads();
    if (tid < F) {
      const float* q = s_dseq + tid;
      st_add(G_(w.bn0) + tid, ((q[0] + q[SC_THREADS]) + q[2 * SC_THREADS]) + q[3 * SC_THREADS], first);
      q += SC_BLOCK;
      st_add(G_(w.bn0) + F + tid, ((q[0] + q[SC_THREADS]) + q[2 * SC_THREADS]) + q[3 * SC_THREADS], first);
    }
  }
}

// d_grad[i] = the sum of the G slices' element i, in slice order
__global__ __launch_bounds__(256) void sign_grad_reduce_kernel(const float* ws, int G, int64_t P, float* grad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float acc = ws[i];
  for (int j = 1; j < G; ++j) acc += ws[(size_t)j * P + i];
  grad[i] = acc;
}

static bool st_rate_ok(float r) { return r >= 0.0f && r <= ST_RATE_MAX; }   // false for nan

}  // namespace isl

using namespace isl;

extern "C" int isl_sign_train_opts_default(isl_sign_train_opts* opts) {
  if (!opts) {
    set_error("isl_sign_train_opts_default: NULL opts");
    return ISL_E_ARG;
  }
  *opts = isl_sign_train_opts{};
  opts->p_drop = 0.2f;      // demo_isl_translate.py:72-100: Dropout(0.2), recurrent_dropout=0.2
  opts->p_rec = 0.2f;
  return ISL_OK;
}

extern "C" int isl_sign_grad_workspace(int n_features, int n_classes, int batch, int64_t* bytes) {
  if (n_features <= 0 || n_features > SC_FMAX || n_classes <= 0 || n_classes > SC_CMAX || batch < 0 || !bytes) {
    set_error("isl_sign_grad_workspace: n_features must be in [1, 256], n_classes in [1, 1024], batch >= 0");
    return ISL_E_ARG;
  }
  const int64_t G = batch < ST_GMAX ? batch : ST_GMAX;
  *bytes = G * sign_layout(n_features, n_classes, nullptr, nullptr) * (int64_t)sizeof(float);
  return ISL_OK;
}

extern "C" int isl_sign_grad(const float* d_params, int n_features, int window, int n_classes,
                             const float* d_windows, const int32_t* d_labels, const float* d_weights,
                             const uint64_t* d_ids, int batch, const isl_sign_train_opts* opts, float* d_loss,
                             float* d_grad, void* d_workspace, void* stream) {
  bool ok = d_grad && batch >= 0 && window > 0 && window <= SC_TMAX && n_features > 0 && n_features <= SC_FMAX &&
            n_classes > 0 && n_classes <= SC_CMAX;
  if (ok && batch > 0) ok = d_params && d_windows && d_labels && d_loss && d_workspace;
  if (ok && opts) {
    ok = st_rate_ok(opts->p_drop) && st_rate_ok(opts->p_rec);
    for (int i = 0; i < 4; ++i) ok = ok && opts->reserved[i] == 0;
  }
  if (!ok) {
    set_error("isl_sign_grad: bad argument (window <= 32, n_features <= 256, n_classes <= 1024, rates in [0, 0.9], "
              "reserved zero, no NULL buffer)");
    return ISL_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  SignTrainArgs a{};
  a.P = sign_layout(n_features, n_classes, &a.w, d_params);
  if (batch == 0) {
    hipError_t e = hipMemsetAsync(d_grad, 0, (size_t)a.P * sizeof(float), st);
    if (e != hipSuccess) {
      set_error(std::string("isl_sign_grad: ") + hipGetErrorString(e));
      return ISL_E_HIP;
    }
    return ISL_OK;
  }
  a.params = d_params;
  a.ws = (float*)d_workspace;
  a.w.x = d_windows;
  a.w.T = window;
  a.w.F = n_features;
  a.w.C = n_classes;
  a.labels = d_labels;
  a.weights = d_weights;
  a.ids = d_ids;
  a.loss = d_loss;
  a.batch = batch;
  a.G = batch < ST_GMAX ? batch : ST_GMAX;
  a.inv_batch = 1.0f / (float)batch;
  a.scale_drop = a.scale_rec = 1.0f;
  uint64_t seed = 0, step = 0;
  if (opts) {
    seed = opts->seed;
    step = opts->step;
    // keep iff (k >> 40) >= round(rate * 2^24): the product is exact in fp64, halves round up
    a.thr_drop = (uint32_t)std::floor((double)opts->p_drop * 16777216.0 + 0.5);
    a.thr_rec = (uint32_t)std::floor((double)opts->p_rec * 16777216.0 + 0.5);
    if (a.thr_drop) a.scale_drop = 1.0f / (1.0f - opts->p_drop);
    if (a.thr_rec) a.scale_rec = 1.0f / (1.0f - opts->p_rec);
  }
  a.key = st_sm(seed ^ step);
  hipLaunchKernelGGL(sign_grad_kernel, dim3(a.G), dim3(SC_BLOCK), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    hipLaunchKernelGGL(sign_grad_reduce_kernel, dim3((unsigned)((a.P + 255) / 256)), dim3(256), 0, st,
                       (const float*)d_workspace, a.G, a.P, d_grad);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    set_error(std::string("isl_sign_grad: ") + hipGetErrorString(e));
    return ISL_E_HIP;
  }
  return ISL_OK;
}
