// SURVEY §8f-3, the small operators of the training step: backward passes of nn.Linear and AdditiveAttention
// (manner/models/components/attention.py:12-29), nn.Embedding with padding_idx, and dropout on a flat tensor; the axis-0 multi-head
// attention of the entity branch, forward and backward, is axis0.hip; nn.Linear's data gradient and bias gradient are the shared row
// kernels of rows_f32.hip (launch_dx_rows, launch_colsum_rows), its weight gradient is here.  The tensors are small (entity dim 100, query dim 200, a few
// thousand rows): plain f32 VALU kernels, each one the textbook derivative of the forward kernel in entity.hip / scoring.hip.
// Composed into autograd Functions by manner_amd/train.py.
#include <math.h>

#include "train_common.h"

namespace manner {
namespace {

// dropout bits: train_common.h's generator (splitmix64 of (seed, site, index)); kept when bits >= thr
__global__ __launch_bounds__(256) void dropout_flat_kernel(const float* x, float* out, int64_t n, uint64_t seed, uint32_t site,
                                                           uint32_t thr, float scale) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = (thr == 0 || drop_bits(seed, site, (uint64_t)i) >= thr) ? x[i] * scale : 0.f;
}

// ---------------------------------------------------------------- nn.Linear backward: y = x W^T + b, x [R, K], W [O, K]
// dW[o, k] = sum_r dy[r, o] x[r, k]: grid (ceil(K / 256), O); rows gathered through `gather` when x is an embedding table
__global__ __launch_bounds__(256) void lin_bwd_w_kernel(const float* __restrict__ dy, const float* __restrict__ x, int64_t R, int K,
                                                        int O, float* __restrict__ dW) {
  const int k = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
  if (k >= K) return;
  float a0 = 0.f, a1 = 0.f;
  int64_t r = 0;
  for (; r + 1 < R; r += 2) {
    a0 = fmaf(dy[r * O + o], x[r * K + k], a0);
    a1 = fmaf(dy[(r + 1) * O + o], x[(r + 1) * K + k], a1);
  }
  if (r < R) a0 = fmaf(dy[r * O + o], x[r * K + k], a0);
  dW[(size_t)o * K + k] = a0 + a1;
}

// ---------------------------------------------------------------- AdditiveAttention backward (attention.py:21-27)
// pre [B, S, Q] = x W^T + b (from the linear kernel).  One workgroup per b: a = tanh(pre), w = softmax_s(a . q),
// out = sum_s w_s x_s.  Given dout [B, D]: dw_s = dout . x_s, dlogit_s = w_s (dw_s - sum w dw), dq += sum_s dlogit_s a_s,
// dpre = dlogit_s q (1 - a^2) (written over `pre`), w [B, S] kept for dx_s = w_s dout + dpre_s W.
constexpr int POOL_MAX_S = 1024;
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ x, float* __restrict__ pre, const float* __restrict__ query,
                                                       const float* __restrict__ dout, int S, int D, int Q, float* __restrict__ wout,
                                                       float* __restrict__ dq_part) {
  __shared__ float lg[POOL_MAX_S], dw[POOL_MAX_S];
  __shared__ float red[4];
  const int64_t b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* pb = pre + (size_t)b * S * Q;
  const float* xb = x + (size_t)b * S * D;
  const float* gb = dout + (size_t)b * D;
  for (int s = wave; s < S; s += 4) {                      // logits and dw, one wave per position
    float l = 0.f, d = 0.f;
    for (int j = lane; j < Q; j += 64) l = fmaf(tanhf(pb[(size_t)s * Q + j]), query[j], l);
    for (int c = lane; c < D; c += 64) d = fmaf(gb[c], xb[(size_t)s * D + c], d);
    l = wsum(l); d = wsum(d);
    if (lane == 0) { lg[s] = l; dw[s] = d; }
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int s = threadIdx.x; s < S; s += 256) mx = fmaxf(mx, lg[s]);
  mx = wmax(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float se = 0.f;
  for (int s = threadIdx.x; s < S; s += 256) se += expf(lg[s] - mx);
  se = wsum(se);
  if (lane == 0) red[wave] = se;
  __syncthreads();
  const float inv = 1.f / (red[0] + red[1] + red[2] + red[3]);
  __syncthreads();
  float c = 0.f;
  for (int s = threadIdx.x; s < S; s += 256) {
    const float w = expf(lg[s] - mx) * inv;
    lg[s] = w;                                             // lg now holds the weights
    c = fmaf(w, dw[s], c);
  }
  c = wsum(c);
  if (lane == 0) red[wave] = c;
  __syncthreads();
  c = red[0] + red[1] + red[2] + red[3];
  for (int s = threadIdx.x; s < S; s += 256) {
    wout[b * S + s] = lg[s];
    dw[s] = lg[s] * (dw[s] - c);                           // dlogit_s
  }
  __syncthreads();
  for (int j = threadIdx.x; j < Q; j += 256) {
    const float qj = query[j];
    float acc = 0.f;
    for (int s = 0; s < S; ++s) {
      const float a = tanhf(pb[(size_t)s * Q + j]);
      acc = fmaf(dw[s], a, acc);
      pb[(size_t)s * Q + j] = dw[s] * qj * (1.f - a * a);
    }
    dq_part[b * Q + j] = acc;
  }
}
// dq[j] = sum_b dq_part[b, j], in row order: the same bits on every run (f32 atomics across the rows were not)
__global__ __launch_bounds__(256) void pool_dq_kernel(const float* __restrict__ dq_part, int64_t B, int Q, float* __restrict__ dq) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= Q) return;
  float acc = 0.f;
  for (int64_t b = 0; b < B; ++b) acc += dq_part[b * Q + j];
  dq[j] = acc;
}
// add[b, s, :] = w[b, s] * dout[b, :]
__global__ __launch_bounds__(256) void pool_wdout_kernel(const float* __restrict__ w, const float* __restrict__ dout, int64_t R, int S,
                                                         int D, float* __restrict__ add) {
  const int64_t r = blockIdx.x;
  const int64_t b = r / S;
  const float ws = w[r];
  for (int c = threadIdx.x; c < D; c += 256) add[r * D + c] = ws * dout[b * D + c];
}

// ---------------------------------------------------------------- nn.Embedding
__global__ __launch_bounds__(256) void embedding_fwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table,
                                                            int64_t n_rows, int D, float* __restrict__ out, int32_t* __restrict__ status) {
  const int64_t r = blockIdx.x;
  int64_t id = ids[r];
  if (id < 0 || id >= n_rows) { if (threadIdx.x == 0 && status) atomicOr(status, MANNER_HIP_STATUS_INDEX); id = 0; }
  for (int c = threadIdx.x; c < D; c += 256) out[r * D + c] = table[id * D + c];
}
// dtable[ids[r]] += dy[r] (f32 atomics); rows equal to padding_idx receive nothing (nn.Embedding(padding_idx=...))
__global__ __launch_bounds__(256) void embedding_bwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dy, int64_t n_rows,
                                                            int D, int64_t padding_idx, float* __restrict__ dtable) {
  const int64_t r = blockIdx.x;
  const int64_t id = ids[r];
  if (id < 0 || id >= n_rows || id == padding_idx) return;
  for (int c = threadIdx.x; c < D; c += 256) atomicAdd(dtable + id * D + c, dy[r * D + c]);
}
// The same sums without atomics, for batches small enough that one scan of the ids per row costs nothing (an A-Module step has a few
// hundred entity slots): the first row that holds an id adds up every row holding it, in row order — one writer per table row, so
// the gradient is the same bits on every run.
constexpr int64_t EMBEDDING_ORDERED_MAX = 8192;
__global__ __launch_bounds__(256) void embedding_bwd_ordered_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dy, int R,
                                                                    int64_t n_rows, int D, int64_t padding_idx, float* __restrict__ dtable) {
  __shared__ unsigned long long s_mask[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x;
  const int64_t id = ids[r];
  if (id < 0 || id >= n_rows || id == padding_idx) return;        // (the whole workgroup)
  int seen = 0;
  for (int j = tid; j < r; j += 256) seen |= ids[j] == id;
  if (__syncthreads_or(seen)) return;
  for (int c0 = 0; c0 < D; c0 += 1024) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = r; j0 < R; j0 += 256) {
      const int j = j0 + tid;
      const unsigned long long m = __ballot(j < R && ids[j] == id);
      if (lane == 0) s_mask[wave] = m;
      __syncthreads();
      for (int w = 0; w < 4; ++w) {
        unsigned long long mm = s_mask[w];
        while (mm) {
          const float* src = dy + (size_t)(j0 + w * 64 + __builtin_ctzll(mm)) * D;
          mm &= mm - 1;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = c0 + q * 256 + tid;
            if (c < D) acc[q] += src[c];
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + q * 256 + tid;
      if (c < D) dtable[id * D + c] = acc[q];
    }
  }
}

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" {

int manner_hip_dropout(const float* x, float* out, int64_t n, uint64_t seed, uint32_t site, float p, manner_hip_stream_t stream) {
  if (n == 0) return MANNER_HIP_OK;
  if (!x || !out || n < 0 || !(p >= 0.f && p < 1.f)) return fail(MANNER_HIP_E_INVALID, "dropout: bad argument");
  const double t = (double)p * 4294967296.0;
  const uint32_t thr = p <= 0.f ? 0u : (t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t);
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(dropout_flat_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, x, out, n, seed,
                     site, thr, p <= 0.f ? 1.f : 1.f / (1.f - p));
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_linear_backward(const float* x, const float* weight, const float* grad_y, int64_t R, int32_t K, int32_t O,
                               const float* add_to_dx, float* grad_x, float* grad_w, float* grad_b, manner_hip_stream_t stream) {
  if (R < 0 || K <= 0 || O <= 0) return fail(MANNER_HIP_E_INVALID, "linear_backward: bad shape");
  hipStream_t s = (hipStream_t)stream;
  if (R == 0) {                                    // no rows: the parameter gradients are sums over nothing = 0 (grad_x is empty)
    if (grad_w) MANNER_HIP_TRY(hipMemsetAsync(grad_w, 0, (size_t)O * K * sizeof(float), s));
    if (grad_b) MANNER_HIP_TRY(hipMemsetAsync(grad_b, 0, (size_t)O * sizeof(float), s));
    return MANNER_HIP_OK;
  }
  if (!grad_y || (grad_x && !weight) || (grad_w && !x)) return fail(MANNER_HIP_E_INVALID, "linear_backward: null pointer");
  int rc;
  if (grad_x && (rc = launch_dx_rows(grad_y, O, weight, K, R, K, O, add_to_dx, nullptr, grad_x, s))) return rc;
  if (grad_w) {
    hipLaunchKernelGGL(lin_bwd_w_kernel, dim3((unsigned)((K + 255) / 256), (unsigned)O), dim3(256), 0, s, grad_y, x, R, K, O, grad_w);
    MANNER_LAUNCH_CHECK();
  }
  return grad_b ? launch_colsum_rows(grad_y, O, R, O, grad_b, s) : MANNER_HIP_OK;
}

size_t manner_hip_additive_pool_backward_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t Q) {
  if (B <= 0 || S <= 0 || D <= 0 || Q <= 0) return 0;
  return ((size_t)(B * S) * (size_t)(Q + D + 1) + (size_t)B * Q) * sizeof(float) + 1024;
}

int manner_hip_additive_pool_backward(const float* x, const float* lin_w, const float* lin_b, const float* query, const float* grad_out,
                                      int64_t B, int64_t S, int32_t D, int32_t Q, float* grad_x, float* grad_w, float* grad_b,
                                      float* grad_q, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream) {
  if (B < 0 || S < 0 || D <= 0 || Q <= 0) return fail(MANNER_HIP_E_INVALID, "additive_pool_backward: bad shape");
  if (B == 0 || S == 0) {                          // an empty batch / empty sequences: zero parameter gradients (grad_x is empty)
    hipStream_t s0 = (hipStream_t)stream;
    if (grad_w) MANNER_HIP_TRY(hipMemsetAsync(grad_w, 0, (size_t)Q * D * sizeof(float), s0));
    if (grad_b) MANNER_HIP_TRY(hipMemsetAsync(grad_b, 0, (size_t)Q * sizeof(float), s0));
    if (grad_q) MANNER_HIP_TRY(hipMemsetAsync(grad_q, 0, (size_t)Q * sizeof(float), s0));
    return MANNER_HIP_OK;
  }
  if (!x || !lin_w || !lin_b || !query || !grad_out || !grad_x || !grad_w || !grad_b || !grad_q || !workspace ||
      S > POOL_MAX_S || D <= 0 || Q <= 0)
    return fail(MANNER_HIP_E_INVALID, "additive_pool_backward: bad argument (S <= %d)", POOL_MAX_S);
  if (workspace_bytes < manner_hip_additive_pool_backward_workspace_bytes(B, S, D, Q))
    return fail(MANNER_HIP_E_WORKSPACE, "additive_pool_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t R = B * S;
  float* pre = static_cast<float*>(workspace);          // [R, Q]: pre-activations, then d pre
  float* add = pre + (size_t)R * Q;                     // [R, D]: w_s * dout
  float* w = add + (size_t)R * D;                       // [R]
  float* dq_part = w + R;                               // [B, Q]: each row's share of d query, summed in row order below
  int rc;
  if ((rc = manner_hip_linear(x, lin_w, lin_b, R, D, Q, pre, stream))) return rc;
  hipLaunchKernelGGL(pool_bwd_kernel, dim3((unsigned)B), dim3(256), 0, s, x, pre, query, grad_out, (int)S, D, Q, w, dq_part);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(pool_dq_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, dq_part, B, Q, grad_q);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(pool_wdout_kernel, dim3((unsigned)R), dim3(256), 0, s, w, grad_out, R, (int)S, D, add);
  MANNER_LAUNCH_CHECK();
  return manner_hip_linear_backward(x, lin_w, pre, R, D, Q, add, grad_x, grad_w, grad_b, stream);
}

int manner_hip_embedding(const int64_t* ids, int64_t R, const float* table, int64_t n_rows, int32_t D, float* out, int32_t* status,
                         manner_hip_stream_t stream) {
  if (R == 0) return MANNER_HIP_OK;
  if (!ids || !table || !out || R < 0 || n_rows <= 0 || D <= 0) return fail(MANNER_HIP_E_INVALID, "embedding: bad argument");
  hipLaunchKernelGGL(embedding_fwd_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, ids, table, n_rows, D, out, status);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_embedding_backward(const int64_t* ids, int64_t R, const float* grad_out, int64_t n_rows, int32_t D, int64_t padding_idx,
                                  float* grad_table, manner_hip_stream_t stream) {
  if (!grad_table || n_rows <= 0 || D <= 0) return fail(MANNER_HIP_E_INVALID, "embedding_backward: bad argument");
  hipStream_t s = (hipStream_t)stream;
  MANNER_HIP_TRY(hipMemsetAsync(grad_table, 0, (size_t)n_rows * D * sizeof(float), s));
  if (R == 0) return MANNER_HIP_OK;
  if (!ids || !grad_out || R < 0) return fail(MANNER_HIP_E_INVALID, "embedding_backward: bad argument");
  if (R <= EMBEDDING_ORDERED_MAX)
    hipLaunchKernelGGL(embedding_bwd_ordered_kernel, dim3((unsigned)R), dim3(256), 0, s, ids, grad_out, (int)R, n_rows, D, padding_idx,
                       grad_table);
  else
    hipLaunchKernelGGL(embedding_bwd_kernel, dim3((unsigned)R), dim3(256), 0, s, ids, grad_out, n_rows, D, padding_idx, grad_table);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // extern "C"
