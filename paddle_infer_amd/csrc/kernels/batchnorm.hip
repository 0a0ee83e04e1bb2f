// Batch normalisation fused with the residual add and the activation (training and inference),
// NCHW and NHWC (channels-last) layouts, bf16 / f32 I/O with f32 statistics.
//
// Parity: reference `phi/kernels/gpu/batch_norm_kernel.cu` / `batch_norm_grad_kernel.cu`,
// `fluid/operators/fused/fused_bn_activation_op.cu` (bn + relu) and
// `fused_bn_add_activation_op.cu` (bn + residual add + relu, ResNet bottleneck tail).
//
// MI355X design: one pass for the statistics (per-thread Welford, workgroup merge, per-block
// partials [P][C] in HBM merged per channel with Chan's formula — exact for ResNet-scale N·H·W,
// no E[x²]-E[x]² cancellation), one fused normalise + add + act pass; backward = one reduction
// pass (Σ dz, Σ dz·x̂ with dz = dy ⊙ act'(y) read from the saved OUTPUT, so the residual is not
// needed) and one elementwise pass producing dx (and dz = d residual). Running statistics are
// updated on the device (no host sync). NCHW blocks walk one channel plane (coalesced along H·W);
// NHWC blocks walk rows with the lanes across channels.
#include "common.h"
#include <float.h>

namespace {

template <typename T> struct V;
template <> struct V<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct V<bf16_t> {
  static __device__ __forceinline__ float ld(const bf16_t* p) { return bf2f(*p); }
  static __device__ __forceinline__ void st(bf16_t* p, float v) { *p = f2bf(v); }
};

__device__ __forceinline__ void welford_merge(float& n, float& m, float& m2, float nb, float mb,
                                              float m2b) {
  if (nb == 0.f) return;
  const float nn = n + nb, d = mb - m;
  m += d * nb / nn;
  m2 += m2b + d * d * n * nb / nn;
  n = nn;
}

__device__ __forceinline__ void welford_add(float& n, float& m, float& m2, float v) {
  n += 1.f;
  const float d = v - m;
  m += d / n;
  m2 += d * (v - m);
}

// ------------------------------------------------------------------------ statistics (Welford)
// NCHW: grid (C, P); block b of channel c covers elements [b*chunk, (b+1)*chunk) of the N·S
// sequence of channel c. part: [3][P][C] (count, mean, M2).
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_nchw(const T* __restrict__ x, int N, int C, int S,
                                                     long long chunk, float* __restrict__ part) {
  const int c = blockIdx.x, b = blockIdx.y, P = gridDim.y;
  const long long M = (long long)N * S;
  const long long beg = b * chunk, end = min(M, beg + chunk);
  float n = 0.f, m = 0.f, m2 = 0.f;
  for (long long i = beg + threadIdx.x; i < end; i += 256)
    welford_add(n, m, m2, V<T>::ld(x + (i / S * C + c) * (long long)S + i % S));
  __shared__ float sn[256], sm[256], sm2[256];
  sn[threadIdx.x] = n; sm[threadIdx.x] = m; sm2[threadIdx.x] = m2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      float a = sn[threadIdx.x], am = sm[threadIdx.x], am2 = sm2[threadIdx.x];
      welford_merge(a, am, am2, sn[threadIdx.x + o], sm[threadIdx.x + o], sm2[threadIdx.x + o]);
      sn[threadIdx.x] = a; sm[threadIdx.x] = am; sm2[threadIdx.x] = am2;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[(0 * P + b) * C + c] = sn[0];
    part[(1 * P + b) * C + c] = sm[0];
    part[(2 * P + b) * C + c] = sm2[0];
  }
}

// NHWC: x [M][C]; grid (P). C ≥ 256: thread t owns channels t, t+256, …; C < 256 (C | 256):
// thread t owns channel t % C on rows t / C + k·(256 / C).
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_nhwc(const T* __restrict__ x, long long M, int C,
                                                     long long chunk, float* __restrict__ part) {
  const int b = blockIdx.x, P = gridDim.x, t = threadIdx.x;
  const long long beg = b * chunk, end = min(M, beg + chunk);
  __shared__ float sn[256], sm[256], sm2[256];
  if (C >= 256) {
    for (int c = t; c < C; c += 256) {
      float n = 0.f, m = 0.f, m2 = 0.f;
      for (long long r = beg; r < end; ++r) welford_add(n, m, m2, V<T>::ld(x + r * C + c));
      part[(0 * P + b) * C + c] = n;
      part[(1 * P + b) * C + c] = m;
      part[(2 * P + b) * C + c] = m2;
    }
    return;
  }
  const int rpi = 256 / C, c = t % C, r0 = t / C;
  float n = 0.f, m = 0.f, m2 = 0.f;
  for (long long r = beg + r0; r < end; r += rpi) welford_add(n, m, m2, V<T>::ld(x + r * C + c));
  sn[t] = n; sm[t] = m; sm2[t] = m2;
  __syncthreads();
  if (t < C) {
    for (int k = 1; k < rpi; ++k) welford_merge(n, m, m2, sn[t + k * C], sm[t + k * C], sm2[t + k * C]);
    part[(0 * P + b) * C + c] = n;
    part[(1 * P + b) * C + c] = m;
    part[(2 * P + b) * C + c] = m2;
  }
}

// per channel: merge partials → mean / rstd (saved for backward), running stats update, and the
// affine fold scale = γ·rstd, shift = β − mean·scale.
// one 256-thread block per channel: lanes merge strided partials, then an LDS tree merge.
__global__ __launch_bounds__(256) void bn_finalize(const float* __restrict__ part, int P, int C,
                                                   float eps, float momentum,
                                                   const float* __restrict__ gamma,
                                                   const float* __restrict__ beta,
                                                   float* __restrict__ run_mean,
                                                   float* __restrict__ run_var,
                                                   float* __restrict__ mean_out,
                                                   float* __restrict__ rstd_out,
                                                   float* __restrict__ scale,
                                                   float* __restrict__ shift) {
  const int c = blockIdx.x, t = threadIdx.x;
  float n = 0.f, m = 0.f, m2 = 0.f;
  for (int b = t; b < P; b += 256)
    welford_merge(n, m, m2, part[(0 * P + b) * C + c], part[(1 * P + b) * C + c],
                  part[(2 * P + b) * C + c]);
  __shared__ float sn[256], sm[256], sm2[256];
  sn[t] = n; sm[t] = m; sm2[t] = m2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      welford_merge(n, m, m2, sn[t + o], sm[t + o], sm2[t + o]);
      sn[t] = n; sm[t] = m; sm2[t] = m2;
    }
    __syncthreads();
  }
  if (t) return;
  const float var = n > 0.f ? m2 / n : 0.f;
  const float rstd = rsqrtf(var + eps);
  mean_out[c] = m;
  rstd_out[c] = rstd;
  if (run_mean) {  // Paddle: running = momentum·running + (1 − momentum)·batch (unbiased var)
    run_mean[c] = momentum * run_mean[c] + (1.f - momentum) * m;
    run_var[c] = momentum * run_var[c] + (1.f - momentum) * (n > 1.f ? m2 / (n - 1.f) : var);
  }
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  scale[c] = g * rstd;
  shift[c] = bt - m * g * rstd;
}

// bn_finalize over channel-major partials part[(k·C + c)·P + b] (the conv forward's per-tile
// statistics, piamd_conv2d_fwd): each channel's P partials are contiguous.
__global__ __launch_bounds__(256) void bn_finalize_t(const float* __restrict__ part, int P, int C,
                                                     float eps, float momentum,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ beta,
                                                     float* __restrict__ run_mean,
                                                     float* __restrict__ run_var,
                                                     float* __restrict__ mean_out,
                                                     float* __restrict__ rstd_out,
                                                     float* __restrict__ scale,
                                                     float* __restrict__ shift) {
  const int c = blockIdx.x, t = threadIdx.x;
  const float* pn = part + (long long)c * P;
  const float* pm = part + ((long long)C + c) * P;
  const float* pq = part + ((long long)2 * C + c) * P;
  float n = 0.f, m = 0.f, m2 = 0.f;
  for (int b = t; b < P; b += 256) welford_merge(n, m, m2, pn[b], pm[b], pq[b]);
  __shared__ float sn[256], sm[256], sm2[256];
  sn[t] = n; sm[t] = m; sm2[t] = m2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      welford_merge(n, m, m2, sn[t + o], sm[t + o], sm2[t + o]);
      sn[t] = n; sm[t] = m; sm2[t] = m2;
    }
    __syncthreads();
  }
  if (t) return;
  const float var = n > 0.f ? m2 / n : 0.f;
  const float rstd = rsqrtf(var + eps);
  mean_out[c] = m;
  rstd_out[c] = rstd;
  if (run_mean) {
    run_mean[c] = momentum * run_mean[c] + (1.f - momentum) * m;
    run_var[c] = momentum * run_var[c] + (1.f - momentum) * (n > 1.f ? m2 / (n - 1.f) : var);
  }
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  scale[c] = g * rstd;
  shift[c] = bt - m * g * rstd;
}

// inference fold from the running statistics (rstd_out for the backward)
__global__ void bn_fold(int C, float eps, const float* __restrict__ gamma,
                        const float* __restrict__ beta, const float* __restrict__ run_mean,
                        const float* __restrict__ run_var, float* __restrict__ scale,
                        float* __restrict__ shift, float* __restrict__ mean_out,
                        float* __restrict__ rstd_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float rstd = rsqrtf(run_var[c] + eps);
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  scale[c] = g * rstd;
  shift[c] = bt - run_mean[c] * g * rstd;
  if (mean_out) mean_out[c] = run_mean[c];
  if (rstd_out) rstd_out[c] = rstd;
}

__device__ __forceinline__ float bn_act(float z, int act) {
  return act == 1 ? fmaxf(z, 0.f) : act == 2 ? fminf(fmaxf(z, 0.f), 6.f) : z;
}

// y = act(x·scale[c] + shift[c] (+ res)); channel of element i: nchw → (i / S) % C, nhwc → i % C
template <typename T>
__global__ __launch_bounds__(256) void bn_apply(const T* __restrict__ x, const T* __restrict__ res,
                                                const float* __restrict__ scale,
                                                const float* __restrict__ shift, T* __restrict__ y,
                                                long long total, int C, int S, int nhwc, int act) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = nhwc ? (int)(i % C) : (int)((i / S) % C);
    float z = V<T>::ld(x + i) * scale[c] + shift[c];
    if (res) z += V<T>::ld(res + i);
    V<T>::st(y + i, bn_act(z, act));
  }
}

// ------------------------------------------------------------------------ backward
// dz = dy ⊙ act'(y) with y the forward output
template <typename T>
__device__ __forceinline__ float dz_of(const T* dy, const T* y, long long i, int act) {
  const float g = V<T>::ld(dy + i);
  if (act == 0) return g;
  const float yv = V<T>::ld(y + i);
  return (act == 1 ? yv > 0.f : (yv > 0.f && yv < 6.f)) ? g : 0.f;
}

// partials of Σ dz and Σ dz·x̂ per channel: part [2][P][C]
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_nchw(const T* __restrict__ dy,
                                                          const T* __restrict__ y,
                                                          const T* __restrict__ x,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, int N,
                                                          int C, int S, long long chunk, int act,
                                                          float* __restrict__ part) {
  const int c = blockIdx.x, b = blockIdx.y, P = gridDim.y;
  const long long M = (long long)N * S, beg = b * chunk, end = min(M, beg + chunk);
  const float mu = mean[c], rs = rstd[c];
  float s1 = 0.f, s2 = 0.f;
  for (long long i = beg + threadIdx.x; i < end; i += 256) {
    const long long idx = (i / S * C + c) * (long long)S + i % S;
    const float dz = dz_of(dy, y, idx, act);
    s1 += dz;
    s2 += dz * (V<T>::ld(x + idx) - mu) * rs;
  }
  __shared__ float r[2][4];
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0) { r[0][threadIdx.x >> 6] = s1; r[1][threadIdx.x >> 6] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[(0 * P + b) * C + c] = r[0][0] + r[0][1] + r[0][2] + r[0][3];
    part[(1 * P + b) * C + c] = r[1][0] + r[1][1] + r[1][2] + r[1][3];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_nhwc(const T* __restrict__ dy,
                                                          const T* __restrict__ y,
                                                          const T* __restrict__ x,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ rstd,
                                                          long long M, int C, long long chunk,
                                                          int act, float* __restrict__ part) {
  const int b = blockIdx.x, P = gridDim.x, t = threadIdx.x;
  const long long beg = b * chunk, end = min(M, beg + chunk);
  __shared__ float r1[256], r2[256];
  if (C >= 256) {
    for (int c = t; c < C; c += 256) {
      const float mu = mean[c], rs = rstd[c];
      float s1 = 0.f, s2 = 0.f;
      for (long long rr = beg; rr < end; ++rr) {
        const long long idx = rr * C + c;
        const float dz = dz_of(dy, y, idx, act);
        s1 += dz;
        s2 += dz * (V<T>::ld(x + idx) - mu) * rs;
      }
      part[(0 * P + b) * C + c] = s1;
      part[(1 * P + b) * C + c] = s2;
    }
    return;
  }
  const int rpi = 256 / C, c = t % C, r0 = t / C;
  const float mu = mean[c], rs = rstd[c];
  float s1 = 0.f, s2 = 0.f;
  for (long long rr = beg + r0; rr < end; rr += rpi) {
    const long long idx = rr * C + c;
    const float dz = dz_of(dy, y, idx, act);
    s1 += dz;
    s2 += dz * (V<T>::ld(x + idx) - mu) * rs;
  }
  r1[t] = s1; r2[t] = s2;
  __syncthreads();
  if (t < C) {
    for (int k = 1; k < rpi; ++k) { s1 += r1[t + k * C]; s2 += r2[t + k * C]; }
    part[(0 * P + b) * C + c] = s1;
    part[(1 * P + b) * C + c] = s2;
  }
}

// per channel (one block each): dβ = Σdz, dγ = Σ dz·x̂ (f32), and the dx pass as one FMA chain
// dx = A·dz + B·x + D with A = γ·rstd, B = −A·rstd·Σdz·x̂/M, D = A·(μ·rstd·Σdz·x̂ − Σdz)/M
// (training; eval: B = D = 0 — the running statistics are constants).
__global__ __launch_bounds__(256) void bn_bwd_finalize(const float* __restrict__ part, int P, int C,
                                                       float M, const float* __restrict__ gamma,
                                                       const float* __restrict__ mean,
                                                       const float* __restrict__ rstd,
                                                       float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta,
                                                       float* __restrict__ coef, int training) {
  const int c = blockIdx.x, t = threadIdx.x;
  float s1 = 0.f, s2 = 0.f;
  for (int b = t; b < P; b += 256) { s1 += part[(0 * P + b) * C + c]; s2 += part[(1 * P + b) * C + c]; }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  __shared__ float r[2][4];
  if ((t & 63) == 0) { r[0][t >> 6] = s1; r[1][t >> 6] = s2; }
  __syncthreads();
  if (t) return;
  s1 = r[0][0] + r[0][1] + r[0][2] + r[0][3];
  s2 = r[1][0] + r[1][1] + r[1][2] + r[1][3];
  if (dbeta) dbeta[c] = s1;
  if (dgamma) dgamma[c] = s2;
  const float rs = rstd[c], A = (gamma ? gamma[c] : 1.f) * rs;
  coef[c] = A;
  coef[C + c] = training ? -A * rs * s2 / M : 0.f;
  coef[2 * C + c] = training ? A * (mean[c] * rs * s2 - s1) / M : 0.f;
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply(const T* __restrict__ dy, const T* __restrict__ y,
                                                    const T* __restrict__ x,
                                                    const float* __restrict__ mean,
                                                    const float* __restrict__ rstd,
                                                    const float* __restrict__ coef, T* __restrict__ dx,
                                                    T* __restrict__ dres, long long total, int C,
                                                    int S, int nhwc, int act, int training) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = nhwc ? (int)(i % C) : (int)((i / S) % C);
    const float dz = dz_of(dy, y, i, act);
    if (dres) V<T>::st(dres + i, dz);
    float v = coef[c] * dz;
    if (training) v += coef[C + c] * V<T>::ld(x + i) + coef[2 * C + c];
    V<T>::st(dx + i, v);
  }
}

// ------------------------------------------------------------- vectorised NHWC (C % 8 == 0)
// 8 consecutive channels per thread (one 16-B bf16 / 2 × 16-B f32 load); a 256-thread block is
// RB = 256 / G rows × G = C/8 channel groups (G ≥ 256: one row per step, groups strided by 256).
template <typename T> __device__ __forceinline__ void ld8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void ld8<bf16_t>(const bf16_t* p, float (&v)[8]) {
  const u16x8 u = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = bf2f(u[j]);
}
template <> __device__ __forceinline__ void ld8<float>(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
}
template <typename T> __device__ __forceinline__ void st8(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void st8<bf16_t>(bf16_t* p, const float (&v)[8]) {
  u16x8 u;
#pragma unroll
  for (int j = 0; j < 8; ++j) u[j] = f2bf(v[j]);
  *reinterpret_cast<u16x8*>(p) = u;
}
template <> __device__ __forceinline__ void st8<float>(float* p, const float (&v)[8]) {
  f32x4 a, b;
#pragma unroll
  for (int j = 0; j < 4; ++j) { a[j] = v[j]; b[j] = v[4 + j]; }
  *reinterpret_cast<f32x4*>(p) = a;
  *reinterpret_cast<f32x4*>(p + 4) = b;
}

// Statistics: per thread shifted sums (shift = the block's first row — robust, no per-element
// divide), converted to (n, mean, M2) and Welford-merged over the block's row lanes.
constexpr int SR = 8;  // statistics rows in flight per lane
constexpr int RR = 4;  // backward-reduction rows in flight per lane (× 2-3 inputs)
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_nhwc8(const T* __restrict__ x, long long M, int C,
                                                      long long chunk, float* __restrict__ part) {
  const int b = blockIdx.x, P = gridDim.x, t = threadIdx.x, G = C / 8;
  const int RB = G >= 256 ? 1 : 256 / G;
  const long long beg = b * chunk, end = min(M, beg + chunk);
  __shared__ float sn[256], sm[256][9], sm2[256][9];
  for (int g0 = 0; g0 < G; g0 += (G >= 256 ? 256 : G)) {
    const int cg = G >= 256 ? g0 + t : t % G, rl = G >= 256 ? 0 : t / G;
    const bool live = cg < G && rl < RB && beg < end;
    float sh[8], s[8], q[8], n = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[j] = s[j] = q[j] = 0.f;
    if (live) {
      ld8(x + beg * C + cg * 8, sh);
      long long r = beg + rl;
      // SR rows per trip: SR independent 16-B loads in flight per lane (a single-row loop was
      // load-latency bound; 4 rows ran at 2.3 TB/s with 2 waves per SIMD)
      for (; r + (SR - 1) * RB < end; r += SR * RB) {
        float v[SR][8];
#pragma unroll
        for (int u = 0; u < SR; ++u) ld8(x + (r + u * RB) * C + cg * 8, v[u]);
#pragma unroll
        for (int u = 0; u < SR; ++u)
#pragma unroll
          for (int j = 0; j < 8; ++j) { const float d = v[u][j] - sh[j]; s[j] += d; q[j] += d * d; }
        n += (float)SR;
      }
      for (; r < end; r += RB) {
        float v[8];
        ld8(x + r * C + cg * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[j] - sh[j]; s[j] += d; q[j] += d * d; }
        n += 1.f;
      }
    }
    float mu[8], m2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mu[j] = n > 0.f ? sh[j] + s[j] / n : 0.f;
      m2[j] = n > 0.f ? fmaxf(q[j] - s[j] * s[j] / n, 0.f) : 0.f;
    }
    if (G < 256) {
      // tree over the RB row lanes of each channel group (pairs rl, rl + h): log2(RB) steps with
      // every live lane merging, instead of G lanes merging RB - 1 partials one after another
      sn[t] = n;
#pragma unroll
      for (int j = 0; j < 8; ++j) { sm[t][j] = mu[j]; sm2[t][j] = m2[j]; }
      __syncthreads();
      int h = 1;
      while (h < RB) h <<= 1;
      for (h >>= 1; h >= 1; h >>= 1) {
        if (rl < h && rl + h < RB && cg < G) {
          const int o = t + h * G;
          const float nb = sn[o];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float nn = n, mm = mu[j], qq = m2[j];
            welford_merge(nn, mm, qq, nb, sm[o][j], sm2[o][j]);
            mu[j] = mm; m2[j] = qq;
            sm[t][j] = mm; sm2[t][j] = qq;
          }
          n += nb;
          sn[t] = n;
        }
        __syncthreads();
      }
    }
    if (cg < G && rl == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = cg * 8 + j;
        part[(0 * P + b) * C + c] = n;
        part[(1 * P + b) * C + c] = mu[j];
        part[(2 * P + b) * C + c] = m2[j];
      }
    }
  }
}

// Backward partials Σ dz, Σ dz·(x − μ)·rstd per channel: part [2][P][C].
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_nhwc8(const T* __restrict__ dy,
                                                           const T* __restrict__ y,
                                                           const T* __restrict__ x,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ rstd,
                                                           long long M, int C, long long chunk,
                                                           int act, float* __restrict__ part,
                                                           const float* __restrict__ mscale,
                                                           const float* __restrict__ mshift) {
  const int b = blockIdx.x, P = gridDim.x, t = threadIdx.x, G = C / 8;
  const int RB = G >= 256 ? 1 : 256 / G;
  const long long beg = b * chunk, end = min(M, beg + chunk);
  // ReLU without a residual: the mask y > 0 is x·scale + shift > 0 with the forward's fold, so
  // the output y is not read (one tensor less per element)
  const bool xmask = act == 1 && mscale != nullptr;
  __shared__ float r1[256][9], r2[256][9];
  for (int g0 = 0; g0 < G; g0 += (G >= 256 ? 256 : G)) {
    const int cg = G >= 256 ? g0 + t : t % G, rl = G >= 256 ? 0 : t / G;
    const bool live = cg < G && rl < RB;
    float s1[8], s2[8], mu[8], msc[8], msh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s1[j] = s2[j] = 0.f;
      mu[j] = live ? mean[cg * 8 + j] : 0.f;
      msc[j] = live && xmask ? mscale[cg * 8 + j] : 0.f;
      msh[j] = live && xmask ? mshift[cg * 8 + j] : 0.f;
    }
    if (live) {
      long long r = beg + rl;
      // RR rows per trip (2·RR or 3·RR independent 16-B loads in flight per lane)
      for (; r + (RR - 1) * RB < end; r += RR * RB) {
        float g[RR][8], xv[RR][8], yv[RR][8];
#pragma unroll
        for (int u = 0; u < RR; ++u) {
          const long long i = (r + u * RB) * C + cg * 8;
          ld8(dy + i, g[u]);
          ld8(x + i, xv[u]);
          if (act && !xmask) ld8(y + i, yv[u]);
        }
#pragma unroll
        for (int u = 0; u < RR; ++u) {
          if (xmask) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (!(xv[u][j] * msc[j] + msh[j] > 0.f)) g[u][j] = 0.f;
          } else if (act) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (!(act == 1 ? yv[u][j] > 0.f : (yv[u][j] > 0.f && yv[u][j] < 6.f))) g[u][j] = 0.f;
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) { s1[j] += g[u][j]; s2[j] += g[u][j] * (xv[u][j] - mu[j]); }
        }
      }
      for (; r < end; r += RB) {
        const long long i = r * C + cg * 8;
        float g[8], xv[8];
        ld8(dy + i, g);
        ld8(x + i, xv);
        if (xmask) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (!(xv[j] * msc[j] + msh[j] > 0.f)) g[j] = 0.f;
        } else if (act) {
          float yv[8];
          ld8(y + i, yv);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (!(act == 1 ? yv[j] > 0.f : (yv[j] > 0.f && yv[j] < 6.f))) g[j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { s1[j] += g[j]; s2[j] += g[j] * (xv[j] - mu[j]); }
      }
    }
    if (G < 256) {  // tree over the RB row lanes (see bn_stats_nhwc8)
#pragma unroll
      for (int j = 0; j < 8; ++j) { r1[t][j] = s1[j]; r2[t][j] = s2[j]; }
      __syncthreads();
      int h = 1;
      while (h < RB) h <<= 1;
      for (h >>= 1; h >= 1; h >>= 1) {
        if (rl < h && rl + h < RB && cg < G) {
          const int o = t + h * G;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            s1[j] += r1[o][j];
            s2[j] += r2[o][j];
            r1[t][j] = s1[j];
            r2[t][j] = s2[j];
          }
        }
        __syncthreads();
      }
    }
    if (cg < G && rl == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = cg * 8 + j;
        part[(0 * P + b) * C + c] = s1[j];
        part[(1 * P + b) * C + c] = s2[j] * rstd[c];
      }
    }
  }
}

// per-channel coefficients of 8 consecutive elements: 8 channels c..c+7 (nhwc) or channel c
__device__ __forceinline__ void coef8(const float* __restrict__ a, int c, int nhwc, float (&v)[8]) {
  if (nhwc) {
    ld8<float>(a + c, v);
  } else {
    const float s = a[c];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = s;
  }
}

// 8 consecutive elements share one channel (nchw: S % 8 == 0) or are 8 channels (nhwc: C % 8 == 0)
__device__ __forceinline__ int chan8(long long i, int C, int S, int nhwc) {
  return nhwc ? (int)(i % C) : (int)((i / S) % C);
}

template <typename T>
__global__ __launch_bounds__(256) void bn_apply8(const T* __restrict__ x, const T* __restrict__ res,
                                                 const float* __restrict__ scale,
                                                 const float* __restrict__ shift, T* __restrict__ y,
                                                 long long total, int C, int S, int nhwc, int act) {
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < total;
       i += (long long)gridDim.x * blockDim.x * 8) {
    const int c = chan8(i, C, S, nhwc);
    float v[8], r[8], sc[8], sh[8];
    ld8(x + i, v);
    if (res) ld8(res + i, r);
    coef8(scale, c, nhwc, sc);
    coef8(shift, c, nhwc, sh);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float z = v[j] * sc[j] + sh[j];
      if (res) z += r[j];
      v[j] = bn_act(z, act);
    }
    st8(y + i, v);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply8(const T* __restrict__ dy, const T* __restrict__ y,
                                                     const T* __restrict__ x,
                                                     const float* __restrict__ mean,
                                                     const float* __restrict__ rstd,
                                                     const float* __restrict__ coef, T* __restrict__ dx,
                                                     T* __restrict__ dres, long long total, int C,
                                                     int S, int nhwc, int act, int training,
                                                     const float* __restrict__ mscale,
                                                     const float* __restrict__ mshift) {
  const bool xmask = act == 1 && mscale != nullptr;  // see bn_bwd_reduce_nhwc8
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < total;
       i += (long long)gridDim.x * blockDim.x * 8) {
    const int c = chan8(i, C, S, nhwc);
    float g[8], xv[8];
    ld8(dy + i, g);
    if (xmask || training) ld8(x + i, xv);
    if (xmask) {
      float sc[8], sh[8];
      coef8(mscale, c, nhwc, sc);
      coef8(mshift, c, nhwc, sh);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (!(xv[j] * sc[j] + sh[j] > 0.f)) g[j] = 0.f;
    } else if (act) {
      float yv[8];
      ld8(y + i, yv);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (!(act == 1 ? yv[j] > 0.f : (yv[j] > 0.f && yv[j] < 6.f))) g[j] = 0.f;
    }
    if (dres) st8(dres + i, g);
    float A[8];
    coef8(coef, c, nhwc, A);
    if (training) {
      float B[8], D[8];
      coef8(coef + C, c, nhwc, B);
      coef8(coef + 2 * C, c, nhwc, D);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = A[j] * g[j] + B[j] * xv[j] + D[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] *= A[j];
    }
    st8(dx + i, g);
  }
}

int parts_for(long long M) {
  long long p = (M + 4095) / 4096;
  return (int)(p < 1 ? 1 : (p > 512 ? 512 : p));
}

// vectorised NHWC: ≈ g_bn_elems elements per block (default 64 K), ≥ 16 rows each (the [P][C]
// partials stay ≤ 1/16 of the data), ≤ g_bn_parts ≤ MAX_PARTS blocks (default 512).
constexpr int MAX_PARTS = 2048;
long long g_bn_elems = 65536;
int g_bn_parts = 512;
int parts_for8(long long M, int C) {
  long long p = (M * C + g_bn_elems - 1) / g_bn_elems;
  const long long lim = M / 16;
  p = p > lim ? lim : p;
  p = p > g_bn_parts ? g_bn_parts : p;
  return (int)(p < 1 ? 1 : p);
}

}  // namespace

// Tuning hook for the NHWC statistics / reduction grid (elements per block, block cap ≤ 2048).
PIAMD_EXPORT int piamd_bn_set_parts(long long elems_per_block, int max_parts) {
  if (elems_per_block < 1024 || max_parts < 1 || max_parts > MAX_PARTS) return (int)hipErrorInvalidValue;
  g_bn_elems = elems_per_block;
  g_bn_parts = max_parts;
  return 0;
}

// Forward. x/res/y: [N, C, S] (nhwc = 0) or [N·S, C] (nhwc = 1); dtype 0 = f32, 1 = bf16.
// training: statistics of x → mean/rstd (f32 [C], saved for backward), running stats updated in
// place (momentum: Paddle convention); else the running statistics (mean/rstd still written).
// ws: f32 workspace of ≥ 2·C + 3·2048·C floats. act: 0 none, 1 relu, 2 relu6.
// nhwc requires C % 8 == 0 (vectorised path), C ≥ 256 or C | 256.
// ss (nullable): f32 [2][C] receives the affine fold (scale, shift) for piamd_bn_bwd's x-derived
// ReLU mask; otherwise the fold lives in ws.
// part_t (nullable, training only): precomputed channel-major statistics partials of x
// ([3][C][P_t] count / mean / M2, piamd_conv2d_fwd) — the statistics pass over x is skipped.
PIAMD_EXPORT int piamd_bn_fwd(int dtype, int nhwc, const void* x, const void* res, void* y, int N,
                              int C, int S, const float* gamma, const float* beta,
                              float* run_mean, float* run_var, float* mean, float* rstd,
                              float momentum, float eps, int training, int act, float* ws, float* ss,
                              const float* part_t, int P_t, hipStream_t st) {
  if (C < 1 || N < 1 || S < 1 || (nhwc && C % 8 && C < 256 && 256 % C) || (part_t && (!training || P_t < 1)))
    return (int)hipErrorInvalidValue;
  const long long M = (long long)N * S, total = M * C;
  const bool v8 = nhwc ? C % 8 == 0 : S % 8 == 0;
  float* scale = ss ? ss : ws;
  float* shift = scale + C;
  if (part_t) {
    hipLaunchKernelGGL(bn_finalize_t, dim3(C), dim3(256), 0, st, part_t, P_t, C, eps, momentum, gamma,
                       beta, run_mean, run_var, mean, rstd, scale, shift);
  } else if (training) {
    const int P = nhwc && C % 8 == 0 ? parts_for8(M, C) : parts_for(M);
    const long long chunk = (M + P - 1) / P;
    float* part = ws + 2 * C;
    if (nhwc && C % 8 == 0) {
      if (dtype) hipLaunchKernelGGL(bn_stats_nhwc8<bf16_t>, dim3(P), dim3(256), 0, st, (const bf16_t*)x, M, C, chunk, part);
      else hipLaunchKernelGGL(bn_stats_nhwc8<float>, dim3(P), dim3(256), 0, st, (const float*)x, M, C, chunk, part);
    } else if (nhwc) {
      if (dtype) hipLaunchKernelGGL(bn_stats_nhwc<bf16_t>, dim3(P), dim3(256), 0, st, (const bf16_t*)x, M, C, chunk, part);
      else hipLaunchKernelGGL(bn_stats_nhwc<float>, dim3(P), dim3(256), 0, st, (const float*)x, M, C, chunk, part);
    } else {
      if (dtype) hipLaunchKernelGGL(bn_stats_nchw<bf16_t>, dim3(C, P), dim3(256), 0, st, (const bf16_t*)x, N, C, S, chunk, part);
      else hipLaunchKernelGGL(bn_stats_nchw<float>, dim3(C, P), dim3(256), 0, st, (const float*)x, N, C, S, chunk, part);
    }
    hipLaunchKernelGGL(bn_finalize, dim3(C), dim3(256), 0, st, part, P, C, eps,
                       momentum, gamma, beta, run_mean, run_var, mean, rstd, scale, shift);
  } else {
    hipLaunchKernelGGL(bn_fold, dim3((C + 255) / 256), dim3(256), 0, st, C, eps, gamma, beta,
                       run_mean, run_var, scale, shift, mean, rstd);
  }
  if (v8) {
    const dim3 g8(stride_grid(total / 8, 256));
    if (dtype)
      hipLaunchKernelGGL(bn_apply8<bf16_t>, g8, dim3(256), 0, st, (const bf16_t*)x,
                         (const bf16_t*)res, scale, shift, (bf16_t*)y, total, C, S, nhwc, act);
    else
      hipLaunchKernelGGL(bn_apply8<float>, g8, dim3(256), 0, st, (const float*)x,
                         (const float*)res, scale, shift, (float*)y, total, C, S, nhwc, act);
    return (int)hipGetLastError();
  }
  const dim3 g(stride_grid(total, 256));
  if (dtype)
    hipLaunchKernelGGL(bn_apply<bf16_t>, g, dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)res,
                       scale, shift, (bf16_t*)y, total, C, S, nhwc, act);
  else
    hipLaunchKernelGGL(bn_apply<float>, g, dim3(256), 0, st, (const float*)x, (const float*)res,
                       scale, shift, (float*)y, total, C, S, nhwc, act);
  return (int)hipGetLastError();
}

// Backward. y = the forward OUTPUT (act' from it); dres (nullable) receives dz = ∂L/∂(bn + res).
// training = 0: the statistics are constants (dx = γ·rstd·dz). dgamma / dbeta: f32 [C]
// (nullable). ws: ≥ 3·C + 2·2048·C floats. ss (nullable): the forward's fold from
// piamd_bn_fwd — with ReLU, no residual and NHWC C % 8 == 0 the mask is x·scale + shift > 0
// (the forward's own test) and y is not read.
PIAMD_EXPORT int piamd_bn_bwd(int dtype, int nhwc, const void* dy, const void* y, const void* x,
                              void* dx, void* dres, int N, int C, int S, const float* gamma,
                              const float* mean, const float* rstd, float* dgamma, float* dbeta,
                              int training, int act, float* ws, const float* ss, hipStream_t st) {
  if (C < 1 || N < 1 || S < 1 || (nhwc && C % 8 && C < 256 && 256 % C))
    return (int)hipErrorInvalidValue;
  const float* msc = act == 1 && !dres && ss && nhwc && C % 8 == 0 ? ss : nullptr;
  const float* msh = msc ? ss + C : nullptr;
  const long long M = (long long)N * S, total = M * C;
  const bool v8 = nhwc ? C % 8 == 0 : S % 8 == 0;
  const int P = nhwc && C % 8 == 0 ? parts_for8(M, C) : parts_for(M);
  const long long chunk = (M + P - 1) / P;
  float* coef = ws;
  float* part = ws + 3 * C;
  if (nhwc && C % 8 == 0) {
    if (dtype) hipLaunchKernelGGL(bn_bwd_reduce_nhwc8<bf16_t>, dim3(P), dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)y, (const bf16_t*)x, mean, rstd, M, C, chunk, act, part, msc, msh);
    else hipLaunchKernelGGL(bn_bwd_reduce_nhwc8<float>, dim3(P), dim3(256), 0, st, (const float*)dy, (const float*)y, (const float*)x, mean, rstd, M, C, chunk, act, part, msc, msh);
  } else if (nhwc) {
    if (dtype) hipLaunchKernelGGL(bn_bwd_reduce_nhwc<bf16_t>, dim3(P), dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)y, (const bf16_t*)x, mean, rstd, M, C, chunk, act, part);
    else hipLaunchKernelGGL(bn_bwd_reduce_nhwc<float>, dim3(P), dim3(256), 0, st, (const float*)dy, (const float*)y, (const float*)x, mean, rstd, M, C, chunk, act, part);
  } else {
    if (dtype) hipLaunchKernelGGL(bn_bwd_reduce_nchw<bf16_t>, dim3(C, P), dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)y, (const bf16_t*)x, mean, rstd, N, C, S, chunk, act, part);
    else hipLaunchKernelGGL(bn_bwd_reduce_nchw<float>, dim3(C, P), dim3(256), 0, st, (const float*)dy, (const float*)y, (const float*)x, mean, rstd, N, C, S, chunk, act, part);
  }
  hipLaunchKernelGGL(bn_bwd_finalize, dim3(C), dim3(256), 0, st, part, P, C, (float)M, gamma,
                     mean, rstd, dgamma, dbeta, coef, training);
  if (v8) {
    const dim3 g8(stride_grid(total / 8, 256));
    if (dtype)
      hipLaunchKernelGGL(bn_bwd_apply8<bf16_t>, g8, dim3(256), 0, st, (const bf16_t*)dy,
                         (const bf16_t*)y, (const bf16_t*)x, mean, rstd, coef, (bf16_t*)dx,
                         (bf16_t*)dres, total, C, S, nhwc, act, training, msc, msh);
    else
      hipLaunchKernelGGL(bn_bwd_apply8<float>, g8, dim3(256), 0, st, (const float*)dy,
                         (const float*)y, (const float*)x, mean, rstd, coef, (float*)dx,
                         (float*)dres, total, C, S, nhwc, act, training, msc, msh);
    return (int)hipGetLastError();
  }
  const dim3 g(stride_grid(total, 256));
  if (dtype)
    hipLaunchKernelGGL(bn_bwd_apply<bf16_t>, g, dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)y,
                       (const bf16_t*)x, mean, rstd, coef, (bf16_t*)dx, (bf16_t*)dres, total, C, S,
                       nhwc, act, training);
  else
    hipLaunchKernelGGL(bn_bwd_apply<float>, g, dim3(256), 0, st, (const float*)dy, (const float*)y,
                       (const float*)x, mean, rstd, coef, (float*)dx, (float*)dres, total, C, S,
                       nhwc, act, training);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------- cross-rank (SyncBatchNorm)
// Reference `phi/kernels/gpu/sync_batch_norm_kernel.cu:192` / `sync_batch_norm_utils.h`. The
// framework's SyncBatchNorm runs these kernels around RCCL collectives issued from Python:
//   fwd: local (count, mean, M2) per channel → all-gather over ranks → piamd_bn_fwd with the
//        gathered triples as channel-major partials (Welford merge across ranks: no E[x²]−E[x]²
//        cancellation) → normalise + running statistics;
//   bwd: local Σdz, Σdz·x̂ → all-reduce → dx from the global sums (dγ / dβ stay the local sums,
//        the data-parallel gradient all-reduce sums them like any parameter gradient).
namespace {
__global__ __launch_bounds__(256) void bn_merge_stats(const float* __restrict__ part, int P, int C,
                                                      float* __restrict__ out) {
  const int c = blockIdx.x, t = threadIdx.x;
  float n = 0.f, m = 0.f, m2 = 0.f;
  for (int b = t; b < P; b += 256)
    welford_merge(n, m, m2, part[(0 * P + b) * C + c], part[(1 * P + b) * C + c],
                  part[(2 * P + b) * C + c]);
  __shared__ float sn[256], sm[256], sm2[256];
  sn[t] = n; sm[t] = m; sm2[t] = m2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      welford_merge(n, m, m2, sn[t + o], sm[t + o], sm2[t + o]);
      sn[t] = n; sm[t] = m; sm2[t] = m2;
    }
    __syncthreads();
  }
  if (t) return;
  out[c] = n;
  out[C + c] = m;
  out[2 * C + c] = m2;
}

__global__ __launch_bounds__(256) void bn_sum_parts2(const float* __restrict__ part, int P, int C,
                                                     float* __restrict__ out) {
  const int c = blockIdx.x, t = threadIdx.x;
  float s1 = 0.f, s2 = 0.f;
  for (int b = t; b < P; b += 256) { s1 += part[(0 * P + b) * C + c]; s2 += part[(1 * P + b) * C + c]; }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  __shared__ float r[2][4];
  if ((t & 63) == 0) { r[0][t >> 6] = s1; r[1][t >> 6] = s2; }
  __syncthreads();
  if (t) return;
  out[c] = r[0][0] + r[0][1] + r[0][2] + r[0][3];
  out[C + c] = r[1][0] + r[1][1] + r[1][2] + r[1][3];
}
}  // namespace

// Local statistics of x: out f32 [3][C] = (count, mean, M2) per channel. ws ≥ 3·2048·C floats.
PIAMD_EXPORT int piamd_bn_local_stats(int dtype, int nhwc, const void* x, int N, int C, int S,
                                      float* ws, float* out, hipStream_t st) {
  if (C < 1 || N < 1 || S < 1 || (nhwc && C % 8 && C < 256 && 256 % C)) return (int)hipErrorInvalidValue;
  const long long M = (long long)N * S;
  const int P = nhwc && C % 8 == 0 ? parts_for8(M, C) : parts_for(M);
  const long long chunk = (M + P - 1) / P;
  if (nhwc && C % 8 == 0) {
    if (dtype) hipLaunchKernelGGL(bn_stats_nhwc8<bf16_t>, dim3(P), dim3(256), 0, st, (const bf16_t*)x, M, C, chunk, ws);
    else hipLaunchKernelGGL(bn_stats_nhwc8<float>, dim3(P), dim3(256), 0, st, (const float*)x, M, C, chunk, ws);
  } else if (nhwc) {
    if (dtype) hipLaunchKernelGGL(bn_stats_nhwc<bf16_t>, dim3(P), dim3(256), 0, st, (const bf16_t*)x, M, C, chunk, ws);
    else hipLaunchKernelGGL(bn_stats_nhwc<float>, dim3(P), dim3(256), 0, st, (const float*)x, M, C, chunk, ws);
  } else {
    if (dtype) hipLaunchKernelGGL(bn_stats_nchw<bf16_t>, dim3(C, P), dim3(256), 0, st, (const bf16_t*)x, N, C, S, chunk, ws);
    else hipLaunchKernelGGL(bn_stats_nchw<float>, dim3(C, P), dim3(256), 0, st, (const float*)x, N, C, S, chunk, ws);
  }
  hipLaunchKernelGGL(bn_merge_stats, dim3(C), dim3(256), 0, st, ws, P, C, out);
  return (int)hipGetLastError();
}

// Local backward sums: out f32 [2][C] = (Σ dz, Σ dz·x̂). ws ≥ 2·2048·C floats.
PIAMD_EXPORT int piamd_bn_bwd_local_sums(int dtype, int nhwc, const void* dy, const void* y,
                                         const void* x, int N, int C, int S, const float* mean,
                                         const float* rstd, int act, float* ws, const float* ss,
                                         float* out, hipStream_t st) {
  if (C < 1 || N < 1 || S < 1 || (nhwc && C % 8 && C < 256 && 256 % C)) return (int)hipErrorInvalidValue;
  const float* msc = act == 1 && ss && nhwc && C % 8 == 0 ? ss : nullptr;
  const float* msh = msc ? ss + C : nullptr;
  const long long M = (long long)N * S;
  const int P = nhwc && C % 8 == 0 ? parts_for8(M, C) : parts_for(M);
  const long long chunk = (M + P - 1) / P;
  if (nhwc && C % 8 == 0) {
    if (dtype) hipLaunchKernelGGL(bn_bwd_reduce_nhwc8<bf16_t>, dim3(P), dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)y, (const bf16_t*)x, mean, rstd, M, C, chunk, act, ws, msc, msh);
    else hipLaunchKernelGGL(bn_bwd_reduce_nhwc8<float>, dim3(P), dim3(256), 0, st, (const float*)dy, (const float*)y, (const float*)x, mean, rstd, M, C, chunk, act, ws, msc, msh);
  } else if (nhwc) {
    if (dtype) hipLaunchKernelGGL(bn_bwd_reduce_nhwc<bf16_t>, dim3(P), dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)y, (const bf16_t*)x, mean, rstd, M, C, chunk, act, ws);
    else hipLaunchKernelGGL(bn_bwd_reduce_nhwc<float>, dim3(P), dim3(256), 0, st, (const float*)dy, (const float*)y, (const float*)x, mean, rstd, M, C, chunk, act, ws);
  } else {
    if (dtype) hipLaunchKernelGGL(bn_bwd_reduce_nchw<bf16_t>, dim3(C, P), dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)y, (const bf16_t*)x, mean, rstd, N, C, S, chunk, act, ws);
    else hipLaunchKernelGGL(bn_bwd_reduce_nchw<float>, dim3(C, P), dim3(256), 0, st, (const float*)dy, (const float*)y, (const float*)x, mean, rstd, N, C, S, chunk, act, ws);
  }
  hipLaunchKernelGGL(bn_sum_parts2, dim3(C), dim3(256), 0, st, ws, P, C, out);
  return (int)hipGetLastError();
}

// dx (and dres) from GLOBAL sums [2][C] over Mtot elements per channel. ws ≥ 3·C floats.
PIAMD_EXPORT int piamd_bn_bwd_apply_sums(int dtype, int nhwc, const void* dy, const void* y,
                                         const void* x, void* dx, void* dres, int N, int C, int S,
                                         const float* gamma, const float* mean, const float* rstd,
                                         int act, const float* sums, float Mtot, float* ws,
                                         const float* ss, hipStream_t st) {
  if (C < 1 || N < 1 || S < 1 || (nhwc && C % 8 && C < 256 && 256 % C)) return (int)hipErrorInvalidValue;
  const float* msc = act == 1 && !dres && ss && nhwc && C % 8 == 0 ? ss : nullptr;
  const float* msh = msc ? ss + C : nullptr;
  const long long total = (long long)N * S * C;
  const bool v8 = nhwc ? C % 8 == 0 : S % 8 == 0;
  float* coef = ws;
  hipLaunchKernelGGL(bn_bwd_finalize, dim3(C), dim3(256), 0, st, sums, 1, C, Mtot, gamma, mean, rstd,
                     (float*)nullptr, (float*)nullptr, coef, 1);
  if (v8) {
    const dim3 g8(stride_grid(total / 8, 256));
    if (dtype)
      hipLaunchKernelGGL(bn_bwd_apply8<bf16_t>, g8, dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)y,
                         (const bf16_t*)x, mean, rstd, coef, (bf16_t*)dx, (bf16_t*)dres, total, C, S,
                         nhwc, act, 1, msc, msh);
    else
      hipLaunchKernelGGL(bn_bwd_apply8<float>, g8, dim3(256), 0, st, (const float*)dy, (const float*)y,
                         (const float*)x, mean, rstd, coef, (float*)dx, (float*)dres, total, C, S,
                         nhwc, act, 1, msc, msh);
    return (int)hipGetLastError();
  }
  const dim3 g(stride_grid(total, 256));
  if (dtype)
    hipLaunchKernelGGL(bn_bwd_apply<bf16_t>, g, dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)y,
                       (const bf16_t*)x, mean, rstd, coef, (bf16_t*)dx, (bf16_t*)dres, total, C, S, nhwc,
                       act, 1);
  else
    hipLaunchKernelGGL(bn_bwd_apply<float>, g, dim3(256), 0, st, (const float*)dy, (const float*)y,
                       (const float*)x, mean, rstd, coef, (float*)dx, (float*)dres, total, C, S, nhwc,
                       act, 1);
  return (int)hipGetLastError();
}
