// The operators of the MINER baseline (reference manner/models/baselines/miner_module.py), f32, forward and backward:
//   PolyAttention        (manner/models/components/attention.py:60-84)    K additive attentions over the history
//   TargetAwareAttention (attention.py:102-116)                            candidate-aware mixture of the K scores
//   DotProduct           (click_predictors.py:9-12) as MINER calls it      [B, M, D] x [B, D, N] with M > 1
// The workload is small (B = 8 users, S <= 50, D = 256, Q = 200, K = 32, C ~ 40) and latency-bound: plain f32 VALU kernels on
// whole coalesced rows, the two nn.Linear products through manner_hip_linear / manner_hip_linear_backward.  Every reduction
// across rows runs in a fixed order (no floating-point atomics): two runs give the same bits.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace manner {
namespace {

constexpr int PA_MAX_S = 256, PA_MAX_K = 64, PA_MAX_Q = 512, PA_MAX_D = 1024;
constexpr int PA_KC = 16;        // context codes per workgroup of the forward / first backward kernel
constexpr int PA_SB = 8;         // history rows per workgroup of the second backward kernel
constexpr int TA_CT = 8;         // candidates per tile of the target-aware kernels

// N wave sums at once: the N exchange chains of a round are independent, so their cross-lane latency overlaps
template <int N>
__device__ __forceinline__ void wsum_n(float (&v)[N]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], o, 64);
  }
}
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_erf_grad(float v) {
  return 0.5f * (1.0f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}

// ---------------------------------------------------------------- PolyAttention
// The attention weights of user b for the codes [k0, k0 + kc): lg[kk][s] = softmax_s(logit[kk][s]),
//   logit[kk][s] = tanh(pre[s, :]) . codes[k0 + kk, :] + mean_t bias[s, t]        (pre = x W^T from the linear kernel).
// Two properties of the reference, kept exactly:
//  - attention.py:79 `weights.masked_fill_(~attn_mask.unsqueeze(dim=1), 1e-30)`: a masked slot gets the logit 1e-30, NOT -inf.  It
//    takes part in the softmax with a logit of about 0 and dilutes the real slots; its x row is weighted like any other.
//  - attention.py:75 `bias.mean(dim=2)`: the mean runs over ALL T columns of the batch-wide bias (every candidate of the whole
//    batch, the user's own zeroed by the caller), not over a per-user count.
// All 256 threads call it; it ends with a barrier.
__device__ __forceinline__ void poly_probs(const float* __restrict__ pre_b, const uint8_t* __restrict__ mask_b,
                                           const float* __restrict__ codes, const float* __restrict__ bias_b, int64_t T, int S, int Q,
                                           int k0, int kc, float* cs, float (*lg)[PA_MAX_S], float* bm) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < kc * Q; i += 256) cs[i] = codes[(size_t)k0 * Q + i];
  for (int s = wave; s < S; s += 4) {
    float t0 = 0.f, t1 = 0.f;
    if (bias_b) {
      const float* row = bias_b + (size_t)s * T;
      int64_t t = lane;
      for (; t + 64 < T; t += 128) { t0 += row[t]; t1 += row[t + 64]; }
      if (t < T) t0 += row[t];
    }
    const float tot = wsum(t0 + t1);
    if (lane == 0) bm[s] = bias_b ? tot / (float)T : 0.f;
  }
  __syncthreads();
  for (int s = wave; s < S; s += 4) {
    float a[PA_MAX_Q / 64];
#pragma unroll
    for (int j = 0; j < PA_MAX_Q / 64; ++j) {
      const int q = lane + 64 * j;
      a[j] = q < Q ? tanhf(pre_b[(size_t)s * Q + q]) : 0.f;
    }
    const bool live = mask_b[s] != 0;
    float v[PA_KC];
#pragma unroll
    for (int kk = 0; kk < PA_KC; ++kk) {
      v[kk] = 0.f;
      if (kk < kc) {
#pragma unroll
        for (int j = 0; j < PA_MAX_Q / 64; ++j) {
          const int q = lane + 64 * j;
          if (q < Q) v[kk] = fmaf(a[j], cs[kk * Q + q], v[kk]);
        }
      }
    }
    wsum_n(v);
#pragma unroll
    for (int kk = 0; kk < PA_KC; ++kk)
      if (lane == 0 && kk < kc) lg[kk][s] = live ? v[kk] + bm[s] : 1e-30f;
  }
  __syncthreads();
  for (int kk = wave; kk < kc; kk += 4) {
    float l[PA_MAX_S / 64], m = -INFINITY;
#pragma unroll
    for (int j = 0; j < PA_MAX_S / 64; ++j) {
      const int s = lane + 64 * j;
      l[j] = s < S ? lg[kk][s] : -INFINITY;
      m = fmaxf(m, l[j]);
    }
    m = wmax(m);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < PA_MAX_S / 64; ++j) {
      l[j] = lane + 64 * j < S ? expf(l[j] - m) : 0.f;
      sum += l[j];
    }
    sum = wsum(sum);
#pragma unroll
    for (int j = 0; j < PA_MAX_S / 64; ++j)
      if (lane + 64 * j < S) lg[kk][lane + 64 * j] = l[j] / sum;
  }
  __syncthreads();
}

// grid (B, ceil(K / PA_KC)): out[b, k, :] = sum_s p[k][s] x[b, s, :]
__global__ __launch_bounds__(256) void poly_fwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, const float* __restrict__ pre,
                                                       const float* __restrict__ codes, const float* __restrict__ bias, int64_t T, int S, int D,
                                                       int Q, int K, float* __restrict__ out) {
  __shared__ float cs[PA_KC * PA_MAX_Q];
  __shared__ float lg[PA_KC][PA_MAX_S];
  __shared__ float bm[PA_MAX_S];
  const int64_t b = blockIdx.x;
  const int k0 = blockIdx.y * PA_KC, kc = min(PA_KC, K - k0);
  poly_probs(pre + (size_t)b * S * Q, mask + (size_t)b * S, codes, bias ? bias + (size_t)b * S * T : nullptr, T, S, Q, k0, kc, cs, lg, bm);
  const float* xb = x + (size_t)b * S * D;
  for (int d = threadIdx.x; d < D; d += 256) {
    float e[PA_KC], o[PA_KC];                        // even / odd slots: two chains per output
#pragma unroll
    for (int kk = 0; kk < PA_KC; ++kk) e[kk] = o[kk] = 0.f;
    int s = 0;
    for (; s + 1 < S; s += 2) {
      const float x0 = xb[(size_t)s * D + d], x1 = xb[(size_t)(s + 1) * D + d];
#pragma unroll
      for (int kk = 0; kk < PA_KC; ++kk) { e[kk] = fmaf(lg[kk][s], x0, e[kk]); o[kk] = fmaf(lg[kk][s + 1], x1, o[kk]); }
    }
    if (s < S) {
      const float x0 = xb[(size_t)s * D + d];
#pragma unroll
      for (int kk = 0; kk < PA_KC; ++kk) e[kk] = fmaf(lg[kk][s], x0, e[kk]);
    }
#pragma unroll
    for (int kk = 0; kk < PA_KC; ++kk)
      if (kk < kc) out[((size_t)b * K + k0 + kk) * D + d] = e[kk] + o[kk];
  }
}

// Backward, first kernel, grid (B, ceil(K / PA_KC)): the weights again, then for dout [B, K, D]
//   dp[k][s] = dout[b, k, :] . x[b, s, :],  dlogit[k][s] = p (dp - sum_s p dp), 0 at a masked slot (masked_fill_ cuts the graph there).
// p and dlogit leave as [B, S, K] rows for the second kernel and for the weight-gradient kernel.
__global__ __launch_bounds__(256) void poly_bwd_probs_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                             const float* __restrict__ pre, const float* __restrict__ codes,
                                                             const float* __restrict__ bias, int64_t T, const float* __restrict__ dout, int S,
                                                             int D, int Q, int K, float* __restrict__ p_out, float* __restrict__ dl_out) {
  __shared__ float cs[PA_KC * PA_MAX_Q];
  __shared__ float lg[PA_KC][PA_MAX_S];
  __shared__ float bm[PA_MAX_S];
  static_assert(PA_MAX_S <= PA_MAX_Q, "dp reuses the staged codes");
  float (*dp)[PA_MAX_S] = reinterpret_cast<float (*)[PA_MAX_S]>(cs);      // the codes are spent once the weights stand
  const int64_t b = blockIdx.x;
  const int k0 = blockIdx.y * PA_KC, kc = min(PA_KC, K - k0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint8_t* mb = mask + (size_t)b * S;
  poly_probs(pre + (size_t)b * S * Q, mb, codes, bias ? bias + (size_t)b * S * T : nullptr, T, S, Q, k0, kc, cs, lg, bm);
  const float* xb = x + (size_t)b * S * D;
  const float* gb = dout + ((size_t)b * K + k0) * D;
  for (int s = wave; s < S; s += 4) {
    float xr[PA_MAX_D / 64];
#pragma unroll
    for (int j = 0; j < PA_MAX_D / 64; ++j) {
      const int d = lane + 64 * j;
      xr[j] = d < D ? xb[(size_t)s * D + d] : 0.f;
    }
    float v[PA_KC];
#pragma unroll
    for (int kk = 0; kk < PA_KC; ++kk) {
      v[kk] = 0.f;
      if (kk < kc) {                                 // rows past the chunk are not this user's (or not there at all)
#pragma unroll
        for (int j = 0; j < PA_MAX_D / 64; ++j) {
          const int d = lane + 64 * j;
          if (d < D) v[kk] = fmaf(xr[j], gb[(size_t)kk * D + d], v[kk]);
        }
      }
    }
    wsum_n(v);
#pragma unroll
    for (int kk = 0; kk < PA_KC; ++kk)
      if (lane == 0 && kk < kc) dp[kk][s] = v[kk];
  }
  __syncthreads();
  for (int kk = wave; kk < kc; kk += 4) {
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < PA_MAX_S / 64; ++j) {
      const int s = lane + 64 * j;
      if (s < S) dot = fmaf(lg[kk][s], dp[kk][s], dot);
    }
    dot = wsum(dot);
#pragma unroll
    for (int j = 0; j < PA_MAX_S / 64; ++j) {
      const int s = lane + 64 * j;
      if (s < S) dp[kk][s] = mb[s] ? lg[kk][s] * (dp[kk][s] - dot) : 0.f;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < S * kc; i += 256) {
    const int s = i / kc, kk = i - s * kc;
    const size_t at = ((size_t)b * S + s) * K + k0 + kk;
    p_out[at] = lg[kk][s];
    dl_out[at] = dp[kk][s];
  }
}

// Backward, second kernel, grid (B, ceil(S / PA_SB)): for the rows s of the tile
//   a = tanh(pre) (kept in `act` for d codes), d pre[s, q] = (sum_k dlogit[s, k] codes[k, q]) (1 - a^2)   written over pre,
//   add[s, d] = sum_k p[s, k] dout[b, k, d]          the weighted-sum route of d x; the linear backward adds the projection route.
__global__ __launch_bounds__(256) void poly_bwd_rows_kernel(float* __restrict__ pre, const float* __restrict__ codes, const float* __restrict__ dout,
                                                            const float* __restrict__ p, const float* __restrict__ dl, int S, int D, int Q, int K,
                                                            float* __restrict__ act, float* __restrict__ add) {
  __shared__ float ps[PA_SB][PA_MAX_K], ds[PA_SB][PA_MAX_K];
  const int64_t b = blockIdx.x;
  const int s0 = blockIdx.y * PA_SB, nr = min(PA_SB, S - s0);
  for (int i = threadIdx.x; i < PA_SB * K; i += 256) {
    const int ss = i / K, k = i - ss * K;
    const size_t at = ((size_t)b * S + s0 + ss) * K + k;
    ps[ss][k] = ss < nr ? p[at] : 0.f;
    ds[ss][k] = ss < nr ? dl[at] : 0.f;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < Q; q += 256) {
    float acc[PA_SB];
#pragma unroll
    for (int ss = 0; ss < PA_SB; ++ss) acc[ss] = 0.f;
    for (int k = 0; k < K; ++k) {
      const float c = codes[(size_t)k * Q + q];
#pragma unroll
      for (int ss = 0; ss < PA_SB; ++ss) acc[ss] = fmaf(ds[ss][k], c, acc[ss]);
    }
#pragma unroll
    for (int ss = 0; ss < PA_SB; ++ss)
      if (ss < nr) {
        const size_t at = ((size_t)b * S + s0 + ss) * Q + q;
        const float a = tanhf(pre[at]);
        act[at] = a;
        pre[at] = acc[ss] * (1.0f - a * a);
      }
  }
  const float* gb = dout + (size_t)b * K * D;
  for (int d = threadIdx.x; d < D; d += 256) {
    float acc[PA_SB];
#pragma unroll
    for (int ss = 0; ss < PA_SB; ++ss) acc[ss] = 0.f;
    for (int k = 0; k < K; ++k) {
      const float g = gb[(size_t)k * D + d];
#pragma unroll
      for (int ss = 0; ss < PA_SB; ++ss) acc[ss] = fmaf(ps[ss][k], g, acc[ss]);
    }
#pragma unroll
    for (int ss = 0; ss < PA_SB; ++ss)
      if (ss < nr) add[((size_t)b * S + s0 + ss) * D + d] = acc[ss];
  }
}

// ---------------------------------------------------------------- TargetAwareAttention
// The mixture weights of the candidates [c0, c0 + nc) of user b: lg[cc][k] = key[b, c, :] . proj[k, :], proj = gelu(pre) (GELU
// true: pre holds the Linear output, gelu applied here) or pre itself (GELU false: the caller has applied it).  Wave w takes the codes
// k = w, w + 4, ...; keys [TA_CT][D] sit in LDS (rows >= nc zero).  All 256 threads call it; it ends with a barrier.
template <bool GELU>
__device__ __forceinline__ void target_logits(const float* __restrict__ pre_b, int K, int D, int nc, const float (*keys)[PA_MAX_D],
                                              float (*lg)[PA_MAX_K]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = wave; k < K; k += 4) {
    float pk[PA_MAX_D / 64];
#pragma unroll
    for (int j = 0; j < PA_MAX_D / 64; ++j) {
      const int d = lane + 64 * j;
      const float v = d < D ? pre_b[(size_t)k * D + d] : 0.f;
      pk[j] = GELU ? gelu_erf(v) : v;
    }
    float v[TA_CT];
#pragma unroll
    for (int cc = 0; cc < TA_CT; ++cc) {
      v[cc] = 0.f;
      if (cc < nc) {
#pragma unroll
        for (int j = 0; j < PA_MAX_D / 64; ++j) {
          const int d = lane + 64 * j;
          if (d < D) v[cc] = fmaf(pk[j], keys[cc][d], v[cc]);
        }
      }
    }
    wsum_n(v);
#pragma unroll
    for (int cc = 0; cc < TA_CT; ++cc)
      if (lane == 0 && cc < nc) lg[cc][k] = v[cc];
  }
  __syncthreads();
}

// grid (B, ceil(C / TA_CT)): out[b, c] = sum_k softmax_k(lg[c][k]) value[b, c, k]   (attention.py:110-114: the softmax runs over the codes)
__global__ __launch_bounds__(256) void target_fwd_kernel(const float* __restrict__ pre, const float* __restrict__ key, const float* __restrict__ value,
                                                         int64_t C, int K, int D, float* __restrict__ out) {
  __shared__ float keys[TA_CT][PA_MAX_D];
  __shared__ float lg[TA_CT][PA_MAX_K];
  const int64_t b = blockIdx.x, c0 = (int64_t)blockIdx.y * TA_CT;
  const int nc = (int)min((int64_t)TA_CT, C - c0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < nc * D; i += 256) {
    const int cc = i / D, d = i - cc * D;
    keys[cc][d] = key[((size_t)b * C + c0 + cc) * D + d];
  }
  __syncthreads();
  target_logits<true>(pre + (size_t)b * K * D, K, D, nc, keys, lg);
  for (int cc = wave; cc < nc; cc += 4) {
    const float l = lane < K ? lg[cc][lane] : -INFINITY;
    const float m = wmax(l);
    const float e = lane < K ? expf(l - m) : 0.f;
    const float sum = wsum(e);
    const float v = lane < K ? value[((size_t)b * C + c0 + cc) * K + lane] : 0.f;
    const float o = wsum((e / sum) * v);
    if (lane == 0) out[(size_t)b * C + c0 + cc] = o;
  }
}

// Backward, grid (B): proj = gelu(pre) once, then tile by tile over the user's candidates, for dout [B, C]
//   w = softmax_k, d value[c, k] = dout[c] w,  dlogit[c, k] = w (dout[c] value[c, k] - sum_k w dout[c] value[c, k]),
//   d key[c, :] = sum_k dlogit[c, k] proj[k, :],  d proj[k, :] += sum_c dlogit[c, k] key[c, :]   (this workgroup alone owns the user's
//   rows of dproj: the tiles add in ascending order),  and at the end d pre = d proj gelu'(pre), written over dproj.
__global__ __launch_bounds__(256) void target_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ key, const float* __restrict__ value,
                                                         const float* __restrict__ dout, int64_t C, int K, int D, float* __restrict__ proj,
                                                         float* __restrict__ dproj, float* __restrict__ dkey, float* __restrict__ dvalue) {
  __shared__ float keys[TA_CT][PA_MAX_D];
  __shared__ float lg[TA_CT][PA_MAX_K];
  const int64_t b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* pre_b = pre + (size_t)b * K * D;
  float* proj_b = proj + (size_t)b * K * D;
  float* dproj_b = dproj + (size_t)b * K * D;
  for (int i = threadIdx.x; i < K * D; i += 256) proj_b[i] = gelu_erf(pre_b[i]);
  for (int64_t c0 = 0; c0 < C; c0 += TA_CT) {
    const int nc = (int)min((int64_t)TA_CT, C - c0);
    __syncthreads();                                 // proj is written; the last tile's readers of keys / lg are done
    for (int i = threadIdx.x; i < TA_CT * D; i += 256) {
      const int cc = i / D, d = i - cc * D;
      keys[cc][d] = cc < nc ? key[((size_t)b * C + c0 + cc) * D + d] : 0.f;
    }
    __syncthreads();
    target_logits<false>(proj_b, K, D, nc, keys, lg);
    for (int cc = wave; cc < TA_CT; cc += 4) {
      float dl = 0.f;
      if (cc < nc) {                                 // wave-uniform
        const size_t at = ((size_t)b * C + c0 + cc) * K + lane;
        const float l = lane < K ? lg[cc][lane] : -INFINITY;
        const float m = wmax(l);
        const float e = lane < K ? expf(l - m) : 0.f;
        const float w = e / wsum(e);
        const float g = dout[(size_t)b * C + c0 + cc];
        const float dw = lane < K ? g * value[at] : 0.f;
        const float dot = wsum(w * dw);
        dl = w * (dw - dot);
        if (lane < K) dvalue[at] = g * w;
      }
      if (lane < K) lg[cc][lane] = dl;
    }
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) {
      float acc[TA_CT];
#pragma unroll
      for (int cc = 0; cc < TA_CT; ++cc) acc[cc] = 0.f;
      for (int k = 0; k < K; ++k) {
        const float pv = proj_b[(size_t)k * D + d];
        float v = 0.f;
#pragma unroll
        for (int cc = 0; cc < TA_CT; ++cc) {
          acc[cc] = fmaf(lg[cc][k], pv, acc[cc]);
          v = fmaf(lg[cc][k], keys[cc][d], v);
        }
        const size_t at = (size_t)k * D + d;
        dproj_b[at] = c0 == 0 ? v : dproj_b[at] + v;
      }
#pragma unroll
      for (int cc = 0; cc < TA_CT; ++cc)
        if (cc < nc) dkey[((size_t)b * C + c0 + cc) * D + d] = acc[cc];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * D; i += 256) dproj_b[i] *= gelu_erf_grad(pre_b[i]);
}

// ---------------------------------------------------------------- batched dot product, M > 1
// out[b, m, n] = sum_d a[b, m, d] bm[b, d, n]; bm by element strides (the permuted [B, N, D] view of MINERModule.forward,
// miner_module.py:195-198, has sd == 1: a wave then reads whole rows).  One wave per output, a grid-stride loop over the outputs.
__global__ __launch_bounds__(256) void bmm_fwd_kernel(const float* __restrict__ a, const float* __restrict__ bm, int64_t total, int64_t M, int64_t N,
                                                      int D, int64_t sb, int64_t sd, int64_t sn, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < total; i += (int64_t)gridDim.x * 4) {
    const int64_t n = i % N, bmi = i / N, b = bmi / M;
    const float* ar = a + bmi * D;
    const float* br = bm + b * sb + n * sn;
    float v0 = 0.f, v1 = 0.f;
    int d = lane;
    for (; d + 64 < D; d += 128) { v0 = fmaf(ar[d], br[(int64_t)d * sd], v0); v1 = fmaf(ar[d + 64], br[(int64_t)(d + 64) * sd], v1); }
    if (d < D) v0 = fmaf(ar[d], br[(int64_t)d * sd], v0);
    const float v = wsum(v0 + v1);
    if (lane == 0) out[i] = v;
  }
}
// da[b, m, d] = sum_n g[b, m, n] bm[b, d, n]: one thread per element, d fastest
__global__ __launch_bounds__(256) void bmm_bwd_a_kernel(const float* __restrict__ g, const float* __restrict__ bm, int64_t total, int64_t M, int64_t N,
                                                        int D, int64_t sb, int64_t sd, int64_t sn, float* __restrict__ da) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t d = i % D, bmi = i / D, b = bmi / M;
    const float* gr = g + bmi * N;
    const float* br = bm + b * sb + d * sd;
    float v0 = 0.f, v1 = 0.f;
    int64_t n = 0;
    for (; n + 1 < N; n += 2) { v0 = fmaf(gr[n], br[n * sn], v0); v1 = fmaf(gr[n + 1], br[(n + 1) * sn], v1); }
    if (n < N) v0 = fmaf(gr[n], br[n * sn], v0);
    da[i] = v0 + v1;
  }
}
// dbm[b, d, n] = sum_m a[b, m, d] g[b, m, n], CONTIGUOUS [B, D, N] (the shape of the view the reference passes): n fastest
__global__ __launch_bounds__(256) void bmm_bwd_b_kernel(const float* __restrict__ g, const float* __restrict__ a, int64_t total, int64_t M, int64_t N,
                                                        int D, float* __restrict__ dbm) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i % N, bd = i / N, d = bd % D, b = bd / D;
    const float* ar = a + b * M * D + d;
    const float* gr = g + b * M * N + n;
    float v0 = 0.f, v1 = 0.f;
    int64_t m = 0;
    for (; m + 1 < M; m += 2) { v0 = fmaf(ar[m * D], gr[m * N], v0); v1 = fmaf(ar[(m + 1) * D], gr[(m + 1) * N], v1); }
    if (m < M) v0 = fmaf(ar[m * D], gr[m * N], v0);
    dbm[i] = v0 + v1;
  }
}

int poly_check(const char* who, int64_t B, int64_t S, int D, int Q, int K, const void* bias, int64_t T) {
  if (B < 0 || S < 1 || D < 1 || Q < 1 || K < 1) return fail(MANNER_HIP_E_INVALID, "%s: bad shape B=%lld S=%lld D=%d Q=%d K=%d", who, (long long)B, (long long)S, D, Q, K);
  if (S > PA_MAX_S) return fail(MANNER_HIP_E_INVALID, "%s: S=%lld unsupported (S <= %d)", who, (long long)S, PA_MAX_S);
  if (K > PA_MAX_K) return fail(MANNER_HIP_E_INVALID, "%s: K=%d unsupported (K <= %d)", who, K, PA_MAX_K);
  if (Q > PA_MAX_Q) return fail(MANNER_HIP_E_INVALID, "%s: Q=%d unsupported (Q <= %d)", who, Q, PA_MAX_Q);
  if (D > PA_MAX_D) return fail(MANNER_HIP_E_INVALID, "%s: D=%d unsupported (D <= %d)", who, D, PA_MAX_D);
  if (bias && T < 1) return fail(MANNER_HIP_E_INVALID, "%s: bias without columns (T >= 1)", who);
  if (B > 0x7fffffffll || B * S > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "%s: B*S exceeds the grid", who);
  return MANNER_HIP_OK;
}
int target_check(const char* who, int64_t B, int64_t C, int K, int D) {
  if (B < 0 || C < 0 || K < 1 || D < 1) return fail(MANNER_HIP_E_INVALID, "%s: bad shape B=%lld C=%lld K=%d D=%d", who, (long long)B, (long long)C, K, D);
  if (K > PA_MAX_K) return fail(MANNER_HIP_E_INVALID, "%s: K=%d unsupported (K <= %d)", who, K, PA_MAX_K);
  if (D > PA_MAX_D) return fail(MANNER_HIP_E_INVALID, "%s: D=%d unsupported (D <= %d)", who, D, PA_MAX_D);
  if (B > 0x7fffffffll || (C + TA_CT - 1) / TA_CT > 65535) return fail(MANNER_HIP_E_INVALID, "%s: B or C exceeds the grid", who);
  return MANNER_HIP_OK;
}
unsigned flat_grid(int64_t items, int per_block) {
  const int64_t blocks = (items + per_block - 1) / per_block;
  return (unsigned)(blocks < 65536 ? blocks : 65536);
}

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" {

size_t manner_hip_poly_attention_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t Q, int32_t K) {
  if (B <= 0 || S <= 0 || D <= 0 || Q <= 0 || K <= 0) return 0;
  return (size_t)(B * S) * (size_t)Q * sizeof(float) + 256;
}

int manner_hip_poly_attention(const float* x, const uint8_t* mask, const float* lin_w, const float* codes, const float* bias, int64_t T,
                              int64_t B, int64_t S, int32_t D, int32_t Q, int32_t K, float* out, void* workspace, size_t workspace_bytes,
                              manner_hip_stream_t stream) {
  int rc;
  if ((rc = poly_check("poly_attention", B, S, D, Q, K, bias, T))) return rc;
  if (B == 0) return MANNER_HIP_OK;
  if (!x || !mask || !lin_w || !codes || !out || !workspace) return fail(MANNER_HIP_E_INVALID, "poly_attention: null pointer");
  if (workspace_bytes < manner_hip_poly_attention_workspace_bytes(B, S, D, Q, K)) return fail(MANNER_HIP_E_WORKSPACE, "poly_attention: workspace too small");
  float* pre = static_cast<float*>(workspace);          // [B S, Q]
  if ((rc = manner_hip_linear(x, lin_w, nullptr, B * S, D, Q, pre, stream))) return rc;
  hipLaunchKernelGGL(poly_fwd_kernel, dim3((unsigned)B, (unsigned)((K + PA_KC - 1) / PA_KC)), dim3(256), 0, (hipStream_t)stream, x, mask, pre, codes,
                     bias, T, (int)S, D, Q, K, out);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

size_t manner_hip_poly_attention_backward_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t Q, int32_t K) {
  if (B <= 0 || S <= 0 || D <= 0 || Q <= 0 || K <= 0) return 0;
  const size_t R = (size_t)(B * S);
  const size_t part = std::max(wgrad_rows_part_floats(B * S, D, Q), wgrad_rows_part_floats(B * S, Q, K));
  return (R * (size_t)(2 * Q + D + 2 * K) + part) * sizeof(float) + 256;
}

int manner_hip_poly_attention_backward(const float* x, const uint8_t* mask, const float* lin_w, const float* codes, const float* bias, int64_t T,
                                       const float* grad_out, int64_t B, int64_t S, int32_t D, int32_t Q, int32_t K, float* grad_x, float* grad_w,
                                       float* grad_codes, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream) {
  int rc;
  if ((rc = poly_check("poly_attention_backward", B, S, D, Q, K, bias, T))) return rc;
  if (!grad_w || !grad_codes) return fail(MANNER_HIP_E_INVALID, "poly_attention_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {                                    // no user: the parameter gradients are sums over nothing
    MANNER_HIP_TRY(hipMemsetAsync(grad_w, 0, (size_t)Q * D * sizeof(float), s));
    MANNER_HIP_TRY(hipMemsetAsync(grad_codes, 0, (size_t)K * Q * sizeof(float), s));
    return MANNER_HIP_OK;
  }
  if (!x || !mask || !lin_w || !codes || !grad_out || !grad_x || !workspace) return fail(MANNER_HIP_E_INVALID, "poly_attention_backward: null pointer");
  if (workspace_bytes < manner_hip_poly_attention_backward_workspace_bytes(B, S, D, Q, K))
    return fail(MANNER_HIP_E_WORKSPACE, "poly_attention_backward: workspace too small");
  const int64_t R = B * S;
  float* pre = static_cast<float*>(workspace);          // [R, Q]: pre-activations, then d pre
  float* act = pre + (size_t)R * Q;                     // [R, Q]: tanh(pre)
  float* add = act + (size_t)R * Q;                     // [R, D]: the weighted-sum route of d x
  float* p = add + (size_t)R * D;                       // [R, K]
  float* dl = p + (size_t)R * K;                        // [R, K]
  float* part = dl + (size_t)R * K;                     // partial sums of the two weight gradients, one after the other
  if ((rc = manner_hip_linear(x, lin_w, nullptr, R, D, Q, pre, stream))) return rc;
  hipLaunchKernelGGL(poly_bwd_probs_kernel, dim3((unsigned)B, (unsigned)((K + PA_KC - 1) / PA_KC)), dim3(256), 0, s, x, mask, pre, codes, bias, T,
                     grad_out, (int)S, D, Q, K, p, dl);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(poly_bwd_rows_kernel, dim3((unsigned)B, (unsigned)((S + PA_SB - 1) / PA_SB)), dim3(256), 0, s, pre, codes, grad_out, p, dl, (int)S,
                     D, Q, K, act, add);
  MANNER_LAUNCH_CHECK();
  if ((rc = launch_wgrad_rows(dl, K, act, R, Q, K, part, grad_codes, Q, s))) return rc;
  if ((rc = launch_wgrad_rows(pre, Q, x, R, D, Q, part, grad_w, D, s))) return rc;
  return manner_hip_linear_backward(x, lin_w, pre, R, D, Q, add, grad_x, nullptr, nullptr, stream);
}

size_t manner_hip_target_attention_workspace_bytes(int64_t B, int32_t K, int32_t D) {
  if (B <= 0 || K <= 0 || D <= 0) return 0;
  return (size_t)(B * K) * (size_t)D * sizeof(float) + 256;
}

int manner_hip_target_attention(const float* query, const float* key, const float* value, const float* lin_w, int64_t B, int64_t C, int32_t K,
                                int32_t D, float* out, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream) {
  int rc;
  if ((rc = target_check("target_attention", B, C, K, D))) return rc;
  if (B == 0 || C == 0) return MANNER_HIP_OK;
  if (!query || !key || !value || !lin_w || !out || !workspace) return fail(MANNER_HIP_E_INVALID, "target_attention: null pointer");
  if (workspace_bytes < manner_hip_target_attention_workspace_bytes(B, K, D)) return fail(MANNER_HIP_E_WORKSPACE, "target_attention: workspace too small");
  float* pre = static_cast<float*>(workspace);          // [B K, D]
  if ((rc = manner_hip_linear(query, lin_w, nullptr, B * K, D, D, pre, stream))) return rc;
  hipLaunchKernelGGL(target_fwd_kernel, dim3((unsigned)B, (unsigned)((C + TA_CT - 1) / TA_CT)), dim3(256), 0, (hipStream_t)stream, pre, key, value, C, K,
                     D, out);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

size_t manner_hip_target_attention_backward_workspace_bytes(int64_t B, int32_t K, int32_t D) {
  if (B <= 0 || K <= 0 || D <= 0) return 0;
  return ((size_t)(B * K) * (size_t)D * 3 + wgrad_rows_part_floats(B * K, D, D)) * sizeof(float) + 256;
}

int manner_hip_target_attention_backward(const float* query, const float* key, const float* value, const float* lin_w, const float* grad_out,
                                         int64_t B, int64_t C, int32_t K, int32_t D, float* grad_query, float* grad_key, float* grad_value,
                                         float* grad_w, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream) {
  int rc;
  if ((rc = target_check("target_attention_backward", B, C, K, D))) return rc;
  if (!grad_w) return fail(MANNER_HIP_E_INVALID, "target_attention_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0 || C == 0) {                          // no candidate: nothing reaches the query or the weight (grad_key / grad_value are empty)
    MANNER_HIP_TRY(hipMemsetAsync(grad_w, 0, (size_t)D * D * sizeof(float), s));
    if (B > 0 && grad_query) MANNER_HIP_TRY(hipMemsetAsync(grad_query, 0, (size_t)(B * K) * D * sizeof(float), s));
    return MANNER_HIP_OK;
  }
  if (!query || !key || !value || !lin_w || !grad_out || !grad_query || !grad_key || !grad_value || !workspace)
    return fail(MANNER_HIP_E_INVALID, "target_attention_backward: null pointer");
  if (workspace_bytes < manner_hip_target_attention_backward_workspace_bytes(B, K, D))
    return fail(MANNER_HIP_E_WORKSPACE, "target_attention_backward: workspace too small");
  const int64_t R = B * K;
  float* pre = static_cast<float*>(workspace);          // [R, D]
  float* proj = pre + (size_t)R * D;                    // [R, D]: gelu(pre)
  float* dpre = proj + (size_t)R * D;                   // [R, D]: d proj, then d pre
  float* part = dpre + (size_t)R * D;
  if ((rc = manner_hip_linear(query, lin_w, nullptr, R, D, D, pre, stream))) return rc;
  hipLaunchKernelGGL(target_bwd_kernel, dim3((unsigned)B), dim3(256), 0, s, pre, key, value, grad_out, C, K, D, proj, dpre, grad_key, grad_value);
  MANNER_LAUNCH_CHECK();
  if ((rc = launch_wgrad_rows(dpre, D, query, R, D, D, part, grad_w, D, s))) return rc;
  return manner_hip_linear_backward(query, lin_w, dpre, R, D, D, nullptr, grad_query, nullptr, nullptr, stream);
}

int manner_hip_bmm(const float* a, const float* b, int64_t B, int64_t M, int64_t N, int32_t D, int64_t sb, int64_t sd, int64_t sn, float* out,
                   manner_hip_stream_t stream) {
  if (B < 0 || M < 0 || N < 0 || D <= 0) return fail(MANNER_HIP_E_INVALID, "bmm: bad shape");
  const int64_t total = B * M * N;
  if (total == 0) return MANNER_HIP_OK;
  if (!a || !b || !out) return fail(MANNER_HIP_E_INVALID, "bmm: null pointer");
  hipLaunchKernelGGL(bmm_fwd_kernel, dim3(flat_grid(total, 4)), dim3(256), 0, (hipStream_t)stream, a, b, total, M, N, D, sb, sd, sn, out);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_bmm_backward(const float* grad_out, const float* a, const float* b, int64_t B, int64_t M, int64_t N, int32_t D, int64_t sb,
                            int64_t sd, int64_t sn, float* grad_a, float* grad_b, manner_hip_stream_t stream) {
  if (B < 0 || M < 0 || N < 0 || D <= 0) return fail(MANNER_HIP_E_INVALID, "bmm_backward: bad shape");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return MANNER_HIP_OK;
  if ((M > 0 && !grad_a) || (N > 0 && !grad_b)) return fail(MANNER_HIP_E_INVALID, "bmm_backward: null pointer");
  if (M == 0 || N == 0) {                          // an empty product: the other operand's gradient is a sum over nothing
    if (M > 0) MANNER_HIP_TRY(hipMemsetAsync(grad_a, 0, (size_t)(B * M) * D * sizeof(float), s));
    if (N > 0) MANNER_HIP_TRY(hipMemsetAsync(grad_b, 0, (size_t)(B * N) * D * sizeof(float), s));
    return MANNER_HIP_OK;
  }
  if (!grad_out || !a || !b) return fail(MANNER_HIP_E_INVALID, "bmm_backward: null pointer");
  hipLaunchKernelGGL(bmm_bwd_a_kernel, dim3(flat_grid(B * M * D, 256)), dim3(256), 0, s, grad_out, b, B * M * D, M, N, D, sb, sd, sn, grad_a);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(bmm_bwd_b_kernel, dim3(flat_grid(B * D * N, 256)), dim3(256), 0, s, grad_out, a, B * D * N, M, N, D, grad_b);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // extern "C"
