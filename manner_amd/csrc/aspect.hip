// The auxiliary heads and losses of the aspect-aware baselines TANR-PLM and SentiRec-PLM (reference manner/models/baselines/
// tanr_plm_module.py:122-177, sentirec_plm_module.py:124-193), f32, forward and backward:
//   head_ce    nn.Linear(D, O) over every news row of the batch + nn.CrossEntropyLoss against its class: the mean of -log softmax(row)[t]
//   head_l1    nn.Linear(D, 1) + nn.L1Loss: the mean of |x . w + b - t|
//   senti_div  SentiRec's diversity regulariser relu(u_b s_bc score_bc).mean() over the dense [B, Cmax] block, on the ragged scores
// The two heads share one row walk (row_head.h, shared with debias.hip): a workgroup stages the weight ONCE (LDS, when it fits) and its four waves walk a grid-stride loop of
// rows under it, one row per wave at a time, the row in registers.  No [N, O] logits reach HBM unless asked for; what the backward needs
// ([N, O] p - y, or [N] sign) is saved.  Every reduction across rows has a fixed order (no floating-point atomics) and every grid comes
// from the shape alone: two runs give the same bits on any CU count.
#include <math.h>

#include <algorithm>

#include "row_head.h"

namespace manner {
namespace {

// ---------------------------------------------------------------- the row heads (row_head.h)
// The forward's policy: the target column is the class itself and a row's p - y is saved as it is (the backward applies g / N); `logits`
// (may be NULL) [N, O] receives the logits.  MODE 2 is the L1 head, O == 1: rowloss = |x . w + b - tgt|, saved [N] = sign(residual).
struct AsHead {
  const float* tgt;
  float* logits;
  __device__ __forceinline__ int column(int64_t t, int) const { return (int)t; }
  __device__ __forceinline__ float scaled(float v, int64_t, int64_t) const { return v; }
  __device__ __forceinline__ void keep_logit(float v, size_t at) const {
    if (logits) logits[at] = v;
  }
  __device__ __forceinline__ void single_row(const float (&xr)[RH_J], const float (&wr)[RH_J], const float* __restrict__ bias, int64_t r, int lane,
                                             float* __restrict__ rowloss, float* __restrict__ saved) const {
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < RH_J; ++j) a = fmaf(xr[j], wr[j], a);
    const float res = (wsum(a) + bias[0]) - tgt[r];
    if (lane == 0) {
      rowloss[r] = fabsf(res);
      if (saved) saved[r] = res > 0.f ? 1.f : (res < 0.f ? -1.f : res);      // sign(0) = 0, a NaN stays a NaN
    }
  }
};
// d x[r, d] = (g / N) sum_o saved[r, o] W[o, d].  O == 1 is the L1 head.
struct AsDx {
  __device__ __forceinline__ float coef(float g, int64_t N) const { return g / (float)N; }
  __device__ __forceinline__ float operator()(float v, size_t) const { return v; }
};

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
  if (O > RH_MAX_O) return fail(MANNER_HIP_E_INVALID, "%s: O=%d unsupported (O <= %d)", who, O, RH_MAX_O);
  if (D > RH_MAX_D) return fail(MANNER_HIP_E_INVALID, "%s: D=%d unsupported (D <= %d)", who, D, RH_MAX_D);
  return MANNER_HIP_OK;
}
bool staged(int D, int O) { return O > 1 && (size_t)O * D * sizeof(float) <= RH_STAGE_BYTES; }
size_t head_fwd_ws(int64_t N) { return N <= 0 ? 0 : (size_t)N * sizeof(float) + 256; }
size_t head_bwd_ws(int64_t N, int D, int O) { return N <= 0 ? 0 : (size_t)rh_chunks(N) * O * (D + 1) * sizeof(float) + 256; }

int head_forward(const char* who, bool l1, const float* x, const float* w, const float* b, const int64_t* cls, const float* tgt, int64_t N, int D,
                 int O, float* loss, float* saved, float* logits, void* workspace, size_t workspace_bytes, int32_t* status, hipStream_t s) {
  int rc;
  if ((rc = head_check(who, N, D, O))) return rc;
  if (N == 0) return fail(MANNER_HIP_E_INVALID, "%s: no row (the mean of nothing)", who);
  if (!x || !w || !b || !loss || !workspace || (l1 ? !tgt : !cls)) return fail(MANNER_HIP_E_INVALID, "%s: null pointer", who);
  if (workspace_bytes < head_fwd_ws(N)) return fail(MANNER_HIP_E_WORKSPACE, "%s: workspace too small", who);
  float* rowloss = static_cast<float*>(workspace);
  const AsHead head{tgt, logits};
  if (l1) rc = rh_launch_walk(rh_head_fwd_kernel<2, AsHead>, false, N, D, O, s, x, w, b, cls, head, N, D, O, rowloss, saved, status);
  else if (staged(D, O)) rc = rh_launch_walk(rh_head_fwd_kernel<0, AsHead>, true, N, D, O, s, x, w, b, cls, head, N, D, O, rowloss, saved, status);
  else rc = rh_launch_walk(rh_head_fwd_kernel<1, AsHead>, false, N, D, O, s, x, w, b, cls, head, N, D, O, rowloss, saved, status);
  if (rc) return rc;
  hipLaunchKernelGGL(as_mean_kernel<float>, dim3(1), dim3(256), 0, s, rowloss, N, (double)N, loss);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int head_backward(const char* who, const float* g, const float* x, const float* w, const float* saved, int64_t N, int D, int O, float* dx, float* dw,
                  float* db, void* workspace, size_t workspace_bytes, hipStream_t s) {
  int rc;
  if ((rc = head_check(who, N, D, O))) return rc;
  if (N == 0) return fail(MANNER_HIP_E_INVALID, "%s: no row (the mean of nothing)", who);
  if (!g || !x || !w || !saved) return fail(MANNER_HIP_E_INVALID, "%s: null pointer", who);
  if (dx) {
    if (staged(D, O)) rc = rh_launch_walk(rh_head_dx_kernel<true, AsDx>, true, N, D, O, s, g, w, saved, AsDx{}, N, D, O, dx);
    else rc = rh_launch_walk(rh_head_dx_kernel<false, AsDx>, false, N, D, O, s, g, w, saved, AsDx{}, N, D, O, dx);
    if (rc) return rc;
  }
  if (dw || db) {
    if (!workspace) return fail(MANNER_HIP_E_INVALID, "%s: null pointer", who);
    if (workspace_bytes < head_bwd_ws(N, D, O)) return fail(MANNER_HIP_E_WORKSPACE, "%s: workspace too small", who);
    if ((rc = rh_head_wgrad(g, (float)N, x, saved, N, D, O, static_cast<float*>(workspace), dw, db, s))) return rc;
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
  return (D < 1 || O < 1 || D > RH_MAX_D || O > RH_MAX_O) ? 0 : head_bwd_ws(N, D, O);
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
