// The auxiliary heads and losses of the aspect-aware baselines TANR-PLM and SentiRec-PLM (reference manner/models/baselines/
// tanr_plm_module.py:122-177, sentirec_plm_module.py:124-193), f32, forward and backward:
//   head_ce    nn.Linear(D, O) over every news row of the batch + nn.CrossEntropyLoss against its class: the mean of -log softmax(row)[t]
//   head_l1    nn.Linear(D, 1) + nn.L1Loss: the mean of |x . w + b - t|
//   senti_div  SentiRec's diversity regulariser relu(u_b s_bc score_bc).mean() over the dense [B, Cmax] block, on the ragged scores
// The two heads share one row walk: a workgroup stages the weight ONCE (LDS, when it fits) and its four waves walk a grid-stride loop of
// rows under it, one row per wave at a time, the row in registers.  No [N, O] logits reach HBM unless asked for; what the backward needs
// ([N, O] p - y, or [N] sign) is saved.  Every reduction across rows has a fixed order (no floating-point atomics) and every grid comes
// from the shape alone: two runs give the same bits on any CU count.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace manner {
namespace {

constexpr int AS_MAX_O = 64, AS_MAX_D = 1024;
constexpr int AS_J = AS_MAX_D / 64;                      // row elements per lane
constexpr int AS_WG_ROWS = 8, AS_MAX_WG = 512;           // rows a workgroup takes per trip of its grid-stride loop (two per wave: N is small and
                                                         // the chip wide); the grid's cap (two staged workgroups fit a CU)
constexpr int AS_CHUNK_ROWS = 32, AS_MAX_CHUNKS = 128;   // weight gradient: rows per partial sum at least; partial sums at most
constexpr size_t AS_STAGE_BYTES = 128 * 1024;            // a weight up to here is staged in LDS (160 KB per CU), a larger one is read through L2



// ---------------------------------------------------------------- the row heads, forward
// MODE 0: cross-entropy, the weight staged in LDS; 1: cross-entropy, the weight read where it lies; 2: L1 (O == 1, the weight row in
// registers).  Wave w of workgroup g takes the rows 8 (g + k G) + w + 4 i.  Per row: the row into registers, one dot product per class
// (four classes in flight, each a per-lane fma chain over d = lane + 64 j and a butterfly), class o's logit kept in lane o, then the
// softmax across the lanes.  rowloss [N] receives the row's loss, `saved` (may be NULL) p - y [N, O] or sign(residual) [N].
// A class outside [0, O) is never used as an index: it raises MANNER_HIP_STATUS_INDEX and its row counts as loss 0, gradient 0.
template <int MODE>
__global__ __launch_bounds__(256) void as_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                          const int64_t* __restrict__ cls, const float* __restrict__ tgt, int64_t N, int D, int O,
                                                          float* __restrict__ rowloss, float* __restrict__ saved, float* __restrict__ logits,
                                                          int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (MODE == 0) stage_weight(W, O * D, wl);
  float wr[AS_J];
  if (MODE == 2) {
#pragma unroll
    for (int j = 0; j < AS_J; ++j) wr[j] = lane + 64 * j < D ? W[lane + 64 * j] : 0.f;
  }
  const float bl = lane < O ? bias[lane] : 0.f;
  for (int64_t base = (int64_t)blockIdx.x * AS_WG_ROWS; base < N; base += (int64_t)gridDim.x * AS_WG_ROWS) {
    const int64_t end = base + AS_WG_ROWS < N ? base + AS_WG_ROWS : N;
    for (int64_t r = base + wave; r < end; r += 4) {
      float xr[AS_J];
#pragma unroll
      for (int j = 0; j < AS_J; ++j) xr[j] = lane + 64 * j < D ? x[(size_t)r * D + lane + 64 * j] : 0.f;
      if (MODE == 2) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < AS_J; ++j) a = fmaf(xr[j], wr[j], a);
        const float res = (wsum(a) + bias[0]) - tgt[r];
        if (lane == 0) {
          rowloss[r] = fabsf(res);
          if (saved) saved[r] = res > 0.f ? 1.f : (res < 0.f ? -1.f : res);      // sign(0) = 0, a NaN stays a NaN
        }
        continue;
      }
      const float* w = MODE == 0 ? wl : W;
      float mine = -INFINITY;                                   // the logit of class `lane`
      for (int o0 = 0; o0 < O; o0 += 4) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < AS_J; ++j) {
          if (64 * j < D) {                                      // wave-uniform; a lane past D holds x = 0 and reads column D - 1
            const int d = min(lane + 64 * j, D - 1);
#pragma unroll
            for (int c = 0; c < 4; ++c) a[c] = fmaf(xr[j], w[min(o0 + c, O - 1) * D + d], a[c]);
          }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float t = wsum(a[c]);
          if (lane == o0 + c && o0 + c < O) mine = t + bl;
        }
      }
      const int64_t t = cls[r];
      const bool bad = t < 0 || t >= O;
      const float m = wmax(mine);
      const float e = lane < O ? expf(mine - m) : 0.f;
      const float s = wsum(e);
      const float lt = __shfl(mine, bad ? 0 : (int)t, 64);
      if (lane < O) {
        if (saved) saved[(size_t)r * O + lane] = bad ? 0.f : e / s - (lane == (int)t ? 1.f : 0.f);
        if (logits) logits[(size_t)r * O + lane] = mine;
      }
      if (lane == 0) {
        rowloss[r] = bad ? 0.f : (logf(s) + m) - lt;
        if (bad && status) atomicOr(status, MANNER_HIP_STATUS_INDEX);
      }
    }
  }
}

// One workgroup: out[0] = (sum of v[0 .. n)) / denom.  Thread i adds the entries i, i + 256, ... in ascending order in f64, the 256
// sums meet in a fixed tree.
template <typename T>
__global__ __launch_bounds__(256) void as_mean_kernel(const T* __restrict__ v, int64_t n, double denom, float* __restrict__ out) {
  __shared__ double sm[256];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) a += (double)v[i];
  sm[threadIdx.x] = a;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(sm[0] / denom);
}

// ---------------------------------------------------------------- the row heads, backward
// d x[r, d] = (g / N) sum_o saved[r, o] W[o, d] (ascending o): the forward's row walk, lane o holding saved[r, o].  O == 1 is the L1 head.
template <bool STAGED>
__global__ __launch_bounds__(256) void as_head_dx_kernel(const float* __restrict__ g, const float* __restrict__ W, const float* __restrict__ saved,
                                                         int64_t N, int D, int O, float* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (STAGED) stage_weight(W, O * D, wl);
  const float* w = STAGED ? wl : W;
  const float coef = g[0] / (float)N;
  for (int64_t base = (int64_t)blockIdx.x * AS_WG_ROWS; base < N; base += (int64_t)gridDim.x * AS_WG_ROWS) {
    const int64_t end = base + AS_WG_ROWS < N ? base + AS_WG_ROWS : N;
    for (int64_t r = base + wave; r < end; r += 4) {
      const float mine = lane < O ? saved[(size_t)r * O + lane] : 0.f;
      float a[AS_J];
#pragma unroll
      for (int j = 0; j < AS_J; ++j) a[j] = 0.f;
      for (int o = 0; o < O; ++o) {
        const float t = __shfl(mine, o, 64);
#pragma unroll
        for (int j = 0; j < AS_J; ++j)
          if (64 * j < D) a[j] = fmaf(t, w[o * D + min(lane + 64 * j, D - 1)], a[j]);      // wave-uniform guard, clamped column
      }
#pragma unroll
      for (int j = 0; j < AS_J; ++j) {
        const int d = lane + 64 * j;
        if (d < D) dx[(size_t)r * D + d] = coef * a[j];
      }
    }
  }
}

// d W[o, d] = (g / N) sum_r saved[r, o] x[r, d] and d b[o] = (g / N) sum_r saved[r, o]: the bias is column d = D of the same
// contraction with x = 1.  One wave per (64 columns, chunk of rows): lane = column, the O classes in registers, the rows of the chunk
// in ascending order -> part [chunks, O, D + 1].
template <int OC>
__global__ __launch_bounds__(64) void as_head_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ saved, int64_t N, int D, int O,
                                                           int64_t chunk_rows, float* __restrict__ part) {
  const int lane = threadIdx.x;
  const int dd = blockIdx.x * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.y * chunk_rows, r1 = r0 + chunk_rows < N ? r0 + chunk_rows : N;
  float acc[OC];
#pragma unroll
  for (int c = 0; c < OC; ++c) acc[c] = 0.f;
  for (int64_t r = r0; r < r1; ++r) {
    const float xv = dd < D ? x[(size_t)r * D + dd] : (dd == D ? 1.f : 0.f);
    const float mine = lane < O ? saved[(size_t)r * O + lane] : 0.f;
#pragma unroll
    for (int c = 0; c < OC; ++c)
      if (c < O) acc[c] = fmaf(__shfl(mine, c, 64), xv, acc[c]);
  }
  if (dd <= D) {
#pragma unroll
    for (int c = 0; c < OC; ++c)
      if (c < O) part[((size_t)blockIdx.y * O + c) * (D + 1) + dd] = acc[c];
  }
}

// one thread per (o, column): the chunks in ascending order, times g / N
__global__ __launch_bounds__(256) void as_head_wreduce_kernel(const float* __restrict__ g, const float* __restrict__ part, int64_t N, int D, int O,
                                                              int chunks, float* __restrict__ dW, float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= O * (D + 1)) return;
  const int o = i / (D + 1), dd = i - o * (D + 1);
  float a = 0.f;
  for (int c = 0; c < chunks; ++c) a += part[(size_t)c * O * (D + 1) + i];
  a *= g[0] / (float)N;
  if (dd < D) {
    if (dW) dW[(size_t)o * D + dd] = a;
  } else if (db) {
    db[o] = a;
  }
}

// ---------------------------------------------------------------- SentiRec's diversity regulariser
// u_b = (sum of user b's history sentiment scores, ascending) / h_b — 0 / 0 = NaN for an empty history, as in the reference
__device__ __forceinline__ float hist_mean(const float* __restrict__ hs, int64_t h0, int64_t h1) {
  float a = 0.f;
  for (int64_t h = h0; h < h1; ++h) a += hs[h];
  return a / (float)(h1 - h0);
}
// relu as torch's: a NaN stays a NaN (fmaxf would drop it)
__device__ __forceinline__ float relu_nan(float v) { return v <= 0.f ? 0.f : v; }

// One wave per impression b: part[b] = sum over its candidates of relu((u_b s_t) score_t); the padded slots of the dense block add 0 for a
// user with a history.  A user WITHOUT one has u = NaN: each real candidate adds NaN and so does each padded slot of the reference
// (NaN * 0 * 0), and with c_max >= 1 the user has one or the other — its sum is NaN whatever its candidate count.  More candidates than
// c_max raise MANNER_HIP_STATUS_LENGTHS.
__global__ __launch_bounds__(64) void as_senti_div_fwd_kernel(const float* __restrict__ scores, const float* __restrict__ cs, const float* __restrict__ hs,
                                                              const int64_t* __restrict__ hist_off, const int64_t* __restrict__ cand_off, int64_t T,
                                                              int64_t NH, int64_t c_max, double* __restrict__ part, int32_t* __restrict__ status) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t h0 = clampi(hist_off[b], 0, NH), h1 = clampi(hist_off[b + 1], h0, NH);
  const int64_t c0 = clampi(cand_off[b], 0, T), c1 = clampi(cand_off[b + 1], c0, T);
  if (lane == 0 && c1 - c0 > c_max && status) atomicOr(status, MANNER_HIP_STATUS_LENGTHS);
  const float u = hist_mean(hs, h0, h1);
  float a = 0.f;
  for (int64_t t = c0 + lane; t < c1; t += 64) a += relu_nan((u * cs[t]) * scores[t]);
  if (lane == 0 && h1 == h0) a += u;                            // the NaN of the reference's padded slots
  const double tot = wsum((double)a);
  if (lane == 0) part[b] = tot;
}

// d score_t = (g / (B c_max)) u_b s_t where the product is > 0 (or NaN), 0 where it is <= 0
__global__ __launch_bounds__(64) void as_senti_div_bwd_kernel(const float* __restrict__ g, const float* __restrict__ scores, const float* __restrict__ cs,
                                                              const float* __restrict__ hs, const int64_t* __restrict__ hist_off,
                                                              const int64_t* __restrict__ cand_off, int64_t T, int64_t NH, double denom,
                                                              float* __restrict__ dscores) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t h0 = clampi(hist_off[b], 0, NH), h1 = clampi(hist_off[b + 1], h0, NH);
  const int64_t c0 = clampi(cand_off[b], 0, T), c1 = clampi(cand_off[b + 1], c0, T);
  const float u = hist_mean(hs, h0, h1);
  const float coef = g[0] / (float)denom;
  for (int64_t t = c0 + lane; t < c1; t += 64) {
    const float us = u * cs[t];
    dscores[t] = (us * scores[t]) <= 0.f ? 0.f : coef * us;
  }
}

int head_check(const char* who, int64_t N, int D, int O) {
  if (N < 0 || D < 1 || O < 1) return fail(MANNER_HIP_E_INVALID, "%s: bad shape N=%lld D=%d O=%d", who, (long long)N, D, O);
  if (O > AS_MAX_O) return fail(MANNER_HIP_E_INVALID, "%s: O=%d unsupported (O <= %d)", who, O, AS_MAX_O);
  if (D > AS_MAX_D) return fail(MANNER_HIP_E_INVALID, "%s: D=%d unsupported (D <= %d)", who, D, AS_MAX_D);
  return MANNER_HIP_OK;
}
unsigned walk_grid(int64_t N) {
  const int64_t g = (N + AS_WG_ROWS - 1) / AS_WG_ROWS;
  return (unsigned)(g < AS_MAX_WG ? g : AS_MAX_WG);
}
bool staged(int D, int O) { return O > 1 && (size_t)O * D * sizeof(float) <= AS_STAGE_BYTES; }
int64_t wgrad_chunks(int64_t N) {
  const int64_t c = (N + AS_CHUNK_ROWS - 1) / AS_CHUNK_ROWS;
  return c < AS_MAX_CHUNKS ? c : AS_MAX_CHUNKS;
}
size_t head_fwd_ws(int64_t N) { return N <= 0 ? 0 : (size_t)N * sizeof(float) + 256; }
size_t head_bwd_ws(int64_t N, int D, int O) { return N <= 0 ? 0 : (size_t)wgrad_chunks(N) * O * (D + 1) * sizeof(float) + 256; }

int head_forward(const char* who, bool l1, const float* x, const float* w, const float* b, const int64_t* cls, const float* tgt, int64_t N, int D,
                 int O, float* loss, float* saved, float* logits, void* workspace, size_t workspace_bytes, int32_t* status, hipStream_t s) {
  int rc;
  if ((rc = head_check(who, N, D, O))) return rc;
  if (N == 0) return fail(MANNER_HIP_E_INVALID, "%s: no row (the mean of nothing)", who);
  if (!x || !w || !b || !loss || !workspace || (l1 ? !tgt : !cls)) return fail(MANNER_HIP_E_INVALID, "%s: null pointer", who);
  if (workspace_bytes < head_fwd_ws(N)) return fail(MANNER_HIP_E_WORKSPACE, "%s: workspace too small", who);
  float* rowloss = static_cast<float*>(workspace);
  const dim3 grid(walk_grid(N)), block(256);
  if (l1) {
    hipLaunchKernelGGL(as_head_fwd_kernel<2>, grid, block, 0, s, x, w, b, cls, tgt, N, D, O, rowloss, saved, logits, status);
  } else if (staged(D, O)) {
    const size_t lds = (size_t)O * D * sizeof(float);
    if (lds > 64 * 1024)
      MANNER_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(as_head_fwd_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)AS_STAGE_BYTES));
    hipLaunchKernelGGL(as_head_fwd_kernel<0>, grid, block, lds, s, x, w, b, cls, tgt, N, D, O, rowloss, saved, logits, status);
  } else {
    hipLaunchKernelGGL(as_head_fwd_kernel<1>, grid, block, 0, s, x, w, b, cls, tgt, N, D, O, rowloss, saved, logits, status);
  }
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(as_mean_kernel<float>, dim3(1), dim3(256), 0, s, rowloss, N, (double)N, loss);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

template <int OC>
void launch_wgrad(const float* x, const float* saved, int64_t N, int D, int O, int64_t chunks, int64_t chunk_rows, float* part, hipStream_t s) {
  hipLaunchKernelGGL(as_head_wgrad_kernel<OC>, dim3((unsigned)((D + 1 + 63) / 64), (unsigned)chunks), dim3(64), 0, s, x, saved, N, D, O, chunk_rows, part);
}

int head_backward(const char* who, const float* g, const float* x, const float* w, const float* saved, int64_t N, int D, int O, float* dx, float* dw,
                  float* db, void* workspace, size_t workspace_bytes, hipStream_t s) {
  int rc;
  if ((rc = head_check(who, N, D, O))) return rc;
  if (N == 0) return fail(MANNER_HIP_E_INVALID, "%s: no row (the mean of nothing)", who);
  if (!g || !x || !w || !saved) return fail(MANNER_HIP_E_INVALID, "%s: null pointer", who);
  if (dx) {
    const dim3 grid(walk_grid(N)), block(256);
    if (staged(D, O)) {
      const size_t lds = (size_t)O * D * sizeof(float);
      if (lds > 64 * 1024)
        MANNER_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(as_head_dx_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)AS_STAGE_BYTES));
      hipLaunchKernelGGL(as_head_dx_kernel<true>, grid, block, lds, s, g, w, saved, N, D, O, dx);
    } else {
      hipLaunchKernelGGL(as_head_dx_kernel<false>, grid, block, 0, s, g, w, saved, N, D, O, dx);
    }
    MANNER_LAUNCH_CHECK();
  }
  if (dw || db) {
    if (!workspace) return fail(MANNER_HIP_E_INVALID, "%s: null pointer", who);
    if (workspace_bytes < head_bwd_ws(N, D, O)) return fail(MANNER_HIP_E_WORKSPACE, "%s: workspace too small", who);
    float* part = static_cast<float*>(workspace);
    const int64_t chunks = wgrad_chunks(N), chunk_rows = (N + chunks - 1) / chunks;
    if (O == 1) launch_wgrad<1>(x, saved, N, D, O, chunks, chunk_rows, part, s);
    else if (O <= 8) launch_wgrad<8>(x, saved, N, D, O, chunks, chunk_rows, part, s);
    else if (O <= 32) launch_wgrad<32>(x, saved, N, D, O, chunks, chunk_rows, part, s);
    else launch_wgrad<64>(x, saved, N, D, O, chunks, chunk_rows, part, s);
    MANNER_LAUNCH_CHECK();
    hipLaunchKernelGGL(as_head_wreduce_kernel, dim3((unsigned)((O * (D + 1) + 255) / 256)), dim3(256), 0, s, g, part, N, D, O, (int)chunks, dw, db);
    MANNER_LAUNCH_CHECK();
  }
  return MANNER_HIP_OK;
}

int senti_check(const char* who, int64_t T, int64_t NH, int64_t B, int64_t c_max) {
  if (T < 0 || NH < 0 || B < 0) return fail(MANNER_HIP_E_INVALID, "%s: bad shape T=%lld N_hist=%lld B=%lld", who, (long long)T, (long long)NH, (long long)B);
  if (B > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "%s: B exceeds the grid", who);
  if (c_max < 1 || (B > 0 && (T + B - 1) / B > c_max))
    return fail(MANNER_HIP_E_INVALID, "%s: c_max=%lld below the largest candidate count (T=%lld over B=%lld)", who, (long long)c_max, (long long)T, (long long)B);
  return MANNER_HIP_OK;
}

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" {

size_t manner_hip_head_workspace_bytes(int64_t N) { return head_fwd_ws(N); }
size_t manner_hip_head_backward_workspace_bytes(int64_t N, int32_t D, int32_t O) {
  return (D < 1 || O < 1 || D > AS_MAX_D || O > AS_MAX_O) ? 0 : head_bwd_ws(N, D, O);
}

int manner_hip_head_ce(const float* x, const float* w, const float* b, const int64_t* target, int64_t N, int32_t D, int32_t O, float* loss,
                       float* saved, float* logits, void* workspace, size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream) {
  return head_forward("head_ce", false, x, w, b, target, nullptr, N, D, O, loss, saved, logits, workspace, workspace_bytes, status, (hipStream_t)stream);
}

int manner_hip_head_ce_backward(const float* grad_loss, const float* x, const float* w, const float* saved, int64_t N, int32_t D, int32_t O,
                                float* grad_x, float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream) {
  return head_backward("head_ce_backward", grad_loss, x, w, saved, N, D, O, grad_x, grad_w, grad_b, workspace, workspace_bytes, (hipStream_t)stream);
}

int manner_hip_head_l1(const float* x, const float* w, const float* b, const float* target, int64_t N, int32_t D, float* loss, float* saved,
                       void* workspace, size_t workspace_bytes, manner_hip_stream_t stream) {
  return head_forward("head_l1", true, x, w, b, nullptr, target, N, D, 1, loss, saved, nullptr, workspace, workspace_bytes, nullptr, (hipStream_t)stream);
}

int manner_hip_head_l1_backward(const float* grad_loss, const float* x, const float* w, const float* saved, int64_t N, int32_t D, float* grad_x,
                                float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream) {
  return head_backward("head_l1_backward", grad_loss, x, w, saved, N, D, 1, grad_x, grad_w, grad_b, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t manner_hip_senti_div_workspace_bytes(int64_t B) { return B <= 0 ? 0 : (size_t)B * sizeof(double) + 256; }

int manner_hip_senti_div(const float* scores, const float* cand_score, const float* hist_score, const int64_t* hist_off, const int64_t* cand_off,
                         int64_t T, int64_t n_hist, int64_t B, int64_t c_max, float* loss, void* workspace, size_t workspace_bytes, int32_t* status,
                         manner_hip_stream_t stream) {
  int rc;
  if ((rc = senti_check("senti_div", T, n_hist, B, c_max))) return rc;
  if (B == 0) return fail(MANNER_HIP_E_INVALID, "senti_div: no impression (the mean of nothing)");
  if (!hist_off || !cand_off || !loss || !workspace || (T > 0 && (!scores || !cand_score)) || (n_hist > 0 && !hist_score))
    return fail(MANNER_HIP_E_INVALID, "senti_div: null pointer");
  if (workspace_bytes < manner_hip_senti_div_workspace_bytes(B)) return fail(MANNER_HIP_E_WORKSPACE, "senti_div: workspace too small");
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return fail(MANNER_HIP_E_INVALID, "senti_div: workspace not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(as_senti_div_fwd_kernel, dim3((unsigned)B), dim3(64), 0, s, scores, cand_score, hist_score, hist_off, cand_off, T, n_hist, c_max, part,
                     status);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(as_mean_kernel<double>, dim3(1), dim3(256), 0, s, part, B, (double)B * (double)c_max, loss);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_senti_div_backward(const float* grad_loss, const float* scores, const float* cand_score, const float* hist_score,
                                  const int64_t* hist_off, const int64_t* cand_off, int64_t T, int64_t n_hist, int64_t B, int64_t c_max,
                                  float* grad_scores, manner_hip_stream_t stream) {
  int rc;
  if ((rc = senti_check("senti_div_backward", T, n_hist, B, c_max))) return rc;
  if (B == 0 || T == 0) return MANNER_HIP_OK;
  if (!grad_loss || !scores || !cand_score || !hist_off || !cand_off || !grad_scores || (n_hist > 0 && !hist_score))
    return fail(MANNER_HIP_E_INVALID, "senti_div_backward: null pointer");
  hipLaunchKernelGGL(as_senti_div_bwd_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, grad_loss, scores, cand_score, hist_score, hist_off,
                     cand_off, T, n_hist, (double)B * (double)c_max, grad_scores);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // extern "C"
