// A one-layer GRU that returns every row's hidden state after its own `len[b]` steps (nn.GRU on pack_padded_sequence(enforce_sorted=
// False), `last_hidden`), f32, forward and backward — the short-term user model of the LSTUR baseline (reference
// manner/models/components/user_encoder.py:45-89) — and the gather of the long-term user rows with their per-user mask.
//   gi = x W_ih^T + b_ih for all (b, t) in one pass (it does not depend on h), x read in place by a batch and a slot stride;
//   then ONE PLAIN LAUNCH PER TIME STEP, t a kernel argument: a wave owns one hidden unit j, takes the three W_hh rows of j over K = H
//   for a tile of batch rows (the h rows of the tile in LDS, the lanes along K, a butterfly sum), and applies the gates and the update:
//     r = sigma(gi_r + gh_r), z = sigma(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h      (gh = h W_hh^T + b_hh)
//   Nothing is exchanged between workgroups inside a launch: no cooperative launch, no grid barrier, no counter.  W_hh (9 MB at
//   H = 868) is re-read from L2 / Infinity Cache at every step.  A row with t >= len[b] keeps h BY SELECTION, so a padded slot may
//   hold anything (its gi is never read; x there is staged as 0).
// Backward: S plain launches in reverse.  The launch of step t rebuilds the pre-activation gradients of its batch tile from dh_t and
// the saved gates (every workgroup for itself: they are elementwise), writes those of its own hidden units, and computes
// dh_{t-1} = dh_t z + dgh W_hh for them from a transposed copy of W_hh (the same wave-per-unit product).  The weight, bias and input
// gradients are taken after the loop over the stacked rows by manner_hip_linear_backward.  Every reduction has a fixed order.
#include <math.h>

#include <algorithm>

#include "train_common.h"

namespace manner {
namespace {

constexpr int GR_MAX_S = 256, GR_MAX_W = 1024;
constexpr int GR_BLOCK = 256, GR_WAVE = 64, GR_WAVES = GR_BLOCK / GR_WAVE;
constexpr int GR_ROWS = 8;           // batch rows per workgroup of the step kernels
constexpr int GR_UNITS = GR_WAVES;   // hidden units per workgroup of the step kernels: one per wave
static_assert(GR_ROWS <= GR_WAVE, "lane rr of a wave finishes batch row rr");
static_assert(GR_WAVE == 64, "common.h's wsum reduces 64 lanes");

// ---------------------------------------------------------------- one time step
// grid (ceil(H / GR_UNITS), ceil(B / GR_ROWS)).  hin [B, H] rows ldin apart (NULL: zeros), hout rows ldout apart (another buffer).
// gates (training) [B, 4, H] of this step: r, z, n, W_hn h + b_hn — written for the rows that take the step.
template <bool TRAIN>
__global__ __launch_bounds__(GR_BLOCK) void step_kernel(const float* __restrict__ gi, const float* __restrict__ W, const float* __restrict__ bh,
                                                   const int64_t* __restrict__ len, const float* __restrict__ hin, int64_t ldin,
                                                   float* __restrict__ hout, int64_t ldout, int t, int64_t B, int S, int H,
                                                   float* __restrict__ gates, int32_t* __restrict__ status) {
  __shared__ float hs[GR_ROWS][GR_MAX_W];
  const int64_t b0 = (int64_t)blockIdx.y * GR_ROWS;
  const int nr = (int)min((int64_t)GR_ROWS, B - b0);
  for (int i = threadIdx.x; i < GR_ROWS * H; i += GR_BLOCK) {
    const int rr = i / H, k = i - rr * H;
    hs[rr][k] = (hin && rr < nr) ? hin[(b0 + rr) * ldin + k] : 0.f;
  }
  if (t == 0 && blockIdx.x == 0 && (int)threadIdx.x < nr && status) {
    const int64_t l = len[b0 + threadIdx.x];
    if (l < 1 || l > S) atomicOr(status, MANNER_HIP_STATUS_LENGTHS);
  }
  __syncthreads();
  const int lane = threadIdx.x % GR_WAVE, j = blockIdx.x * GR_UNITS + threadIdx.x / GR_WAVE;
  if (j >= H) return;                                  // wave-uniform, after the only barrier
  const float* wr = W + (size_t)j * H;
  const float* wz = W + (size_t)(H + j) * H;
  const float* wn = W + (size_t)(2 * H + j) * H;
  float ar[GR_ROWS], az[GR_ROWS], an[GR_ROWS];
#pragma unroll
  for (int rr = 0; rr < GR_ROWS; ++rr) ar[rr] = az[rr] = an[rr] = 0.f;
  for (int k = lane; k < H; k += GR_WAVE) {
    const float vr = wr[k], vz = wz[k], vn = wn[k];
#pragma unroll
    for (int rr = 0; rr < GR_ROWS; ++rr) {
      const float hv = hs[rr][k];
      ar[rr] = fmaf(hv, vr, ar[rr]);
      az[rr] = fmaf(hv, vz, az[rr]);
      an[rr] = fmaf(hv, vn, an[rr]);
    }
  }
  const float br = bh[j], bz = bh[H + j], bn = bh[2 * H + j];
#pragma unroll
  for (int rr = 0; rr < GR_ROWS; ++rr) {
    const float sr = wsum(ar[rr]), sz = wsum(az[rr]), sn = wsum(an[rr]);      // every lane holds the sums
    if (lane == rr && rr < nr) {
      const int64_t b = b0 + rr;
      const float hp = hs[rr][j];
      float hv = hp;
      if (t < len[b]) {
        const float* g = gi + (size_t)(b * S + t) * 3 * H;
        const float hn = sn + bn;
        const float r = sigmoidf(g[j] + (sr + br)), z = sigmoidf(g[H + j] + (sz + bz)), n = tanhf(fmaf(r, hn, g[2 * H + j]));
        hv = fmaf(z, hp - n, n);                       // (1 - z) n + z h
        if (TRAIN) {
          float* gs = gates + (size_t)b * 4 * H;
          gs[j] = r; gs[H + j] = z; gs[2 * H + j] = n; gs[3 * H + j] = hn;
        }
      }
      hout[b * ldout + j] = hv;
    }
  }
}

// ---------------------------------------------------------------- one time step, backward
// grid as step_kernel.  din [B, H] rows ldin apart = dh_t, dout rows ldout apart = dh_{t-1}; hp [B, H] = h_{t-1}, gates [B, 4, H] of
// step t; wt [H, 3H] = W_hh^T.  A workgroup rebuilds, gate by gate, the hidden-path pre-activation gradients of all H units of its
// batch tile in LDS (rows that did not take the step: zeros), writes dgi [B S, 3H] (row b S + t) and dgh [B, 3H] of this step for its own
// units, and its waves take dgh . W_hh[:, k] for their units k.
__global__ __launch_bounds__(GR_BLOCK) void bstep_kernel(const float* __restrict__ wt, const int64_t* __restrict__ len, const float* __restrict__ din,
                                                    int64_t ldin, float* __restrict__ dout, int64_t ldout, const float* __restrict__ hp,
                                                    const float* __restrict__ gates, float* __restrict__ dgi, float* __restrict__ dgh, int t,
                                                    int64_t B, int S, int H) {
  __shared__ float ds[GR_ROWS][GR_MAX_W];
  const int64_t b0 = (int64_t)blockIdx.y * GR_ROWS;
  const int nr = (int)min((int64_t)GR_ROWS, B - b0);
  const int lane = threadIdx.x % GR_WAVE, k = blockIdx.x * GR_UNITS + threadIdx.x / GR_WAVE;
  float acc[GR_ROWS];
#pragma unroll
  for (int rr = 0; rr < GR_ROWS; ++rr) acc[rr] = 0.f;
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    __syncthreads();
    for (int i = threadIdx.x; i < GR_ROWS * H; i += GR_BLOCK) {
      const int rr = i / H, j = i - rr * H;
      float vi = 0.f, vh = 0.f;                        // d gi, d gh of gate g at (row rr, unit j)
      const int64_t b = b0 + rr;
      const bool on = rr < nr && t < len[b];
      if (on) {
        const float* gs = gates + (size_t)b * 4 * H;
        const float d = din[b * ldin + j], z = gs[H + j], n = gs[2 * H + j];
        if (g == 1) {
          vi = vh = d * (hp[b * H + j] - n) * (z * (1.0f - z));
        } else {
          const float dn = d * (1.0f - z) * (1.0f - n * n), r = gs[j];
          if (g == 2) { vi = dn; vh = dn * r; }
          else vi = vh = dn * gs[3 * H + j] * (r * (1.0f - r));
        }
      }
      ds[rr][j] = vh;
      if (rr < nr && j / GR_UNITS == (int)blockIdx.x) {
        dgi[(size_t)(b * S + t) * 3 * H + g * H + j] = vi;
        dgh[(size_t)b * 3 * H + g * H + j] = vh;
      }
    }
    __syncthreads();
    if (k < H) {
      const float* wk = wt + (size_t)k * 3 * H + g * H;
      for (int o = lane; o < H; o += GR_WAVE) {
        const float wv = wk[o];
#pragma unroll
        for (int rr = 0; rr < GR_ROWS; ++rr) acc[rr] = fmaf(ds[rr][o], wv, acc[rr]);
      }
    }
  }
  if (k >= H) return;
#pragma unroll
  for (int rr = 0; rr < GR_ROWS; ++rr) {
    const float s = wsum(acc[rr]);
    if (lane == rr && rr < nr) {
      const int64_t b = b0 + rr;
      const float d = din[b * ldin + k];
      dout[b * ldout + k] = t < len[b] ? fmaf(d, gates[(size_t)b * 4 * H + H + k], s) : d;
    }
  }
}

// ---------------------------------------------------------------- user rows
// out[b, :E] = m(b) src[row(b), :E], row(b) = ids[b] (ids given: a gather from the table, n_rows rows) or b; m(b) = 0 or 1 / (1 - p) by
// the counter-based generator at index b — nn.Dropout2d on [1, B, E]: a WHOLE USER ROW is dropped.  src rows lds apart, out rows ldo.
// An id outside [0, n_rows) raises MANNER_HIP_STATUS_INDEX and writes zeros.  grid (B)
__global__ __launch_bounds__(GR_BLOCK) void user_rows_kernel(const int64_t* __restrict__ ids, const float* __restrict__ src, int64_t n_rows, int64_t lds,
                                                        int E, Drop drop, float* __restrict__ out, int64_t ldo, int32_t* __restrict__ status) {
  const int64_t b = blockIdx.x;
  int64_t row = ids ? ids[b] : b;
  const bool bad = ids && (row < 0 || row >= n_rows);
  if (bad && threadIdx.x == 0 && status) atomicOr(status, MANNER_HIP_STATUS_INDEX);
  const float m = bad ? 0.f : drop.apply(1.0f, (uint64_t)b);
  if (bad) row = 0;
  for (int c = threadIdx.x; c < E; c += GR_BLOCK) out[b * ldo + c] = m == 0.f ? 0.f : src[row * lds + c] * m;
}

struct Saved { float *xs, *hs, *gates; };            // x rows [B S, I]; h_{t-1} [S, B, H]; r, z, n, W_hn h + b_hn [S, B, 4, H]
void plan_saved(FloatBump& b, Saved& s, size_t B, size_t S, size_t I, size_t H) {
  s.xs = b.take(B * S * I);
  s.hs = b.take(S * B * H);
  s.gates = b.take(S * B * 4 * H);
}
// forward: gi, two h buffers; backward: W_hh^T, dgi [B S, 3H], dgh [S, B, 3H], two dh buffers — one size serves both
struct Work { float *gi, *h[2], *wt, *dgh; };
void plan_work(FloatBump& b, Work& w, size_t B, size_t S, size_t H) {
  w.gi = b.take(B * S * 3 * H);
  w.h[0] = b.take(B * H);
  w.h[1] = b.take(B * H);
  w.wt = b.take(3 * H * H);
  w.dgh = b.take(S * B * 3 * H);
}

int gru_check(const char* who, int64_t B, int64_t S, int I, int H) {
  if (B < 0 || S < 1 || I < 1 || H < 1) return fail(MANNER_HIP_E_INVALID, "%s: bad shape B=%lld S=%lld I=%d H=%d", who, (long long)B, (long long)S, I, H);
  if (S > GR_MAX_S) return fail(MANNER_HIP_E_INVALID, "%s: S=%lld unsupported (S <= %d)", who, (long long)S, GR_MAX_S);
  if (I > GR_MAX_W) return fail(MANNER_HIP_E_INVALID, "%s: I=%d unsupported (I <= %d)", who, I, GR_MAX_W);
  if (H > GR_MAX_W) return fail(MANNER_HIP_E_INVALID, "%s: H=%d unsupported (H <= %d)", who, H, GR_MAX_W);
  if (B * S > 0x7fffffffll || (B + GR_ROWS - 1) / GR_ROWS > 65535) return fail(MANNER_HIP_E_INVALID, "%s: B=%lld exceeds the grid", who, (long long)B);
  return MANNER_HIP_OK;
}

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" {

size_t manner_hip_gru_saved_bytes(int64_t B, int64_t S, int32_t I, int32_t H) {
  if (B <= 0 || S <= 0 || I <= 0 || H <= 0) return 0;
  FloatBump b(nullptr);
  Saved s;
  plan_saved(b, s, (size_t)B, (size_t)S, (size_t)I, (size_t)H);
  return b.off * sizeof(float) + 256;
}

size_t manner_hip_gru_workspace_bytes(int64_t B, int64_t S, int32_t I, int32_t H) {
  if (B <= 0 || S <= 0 || I <= 0 || H <= 0) return 0;
  FloatBump b(nullptr);
  Work w;
  plan_work(b, w, (size_t)B, (size_t)S, (size_t)H);
  return b.off * sizeof(float) + 256;
}

int manner_hip_gru_forward(const float* x, int64_t x_stride_b, int64_t x_stride_s, const int64_t* lengths, const float* w_ih, const float* w_hh,
                           const float* b_ih, const float* b_hh, const float* h0, int64_t B, int64_t S, int32_t I, int32_t H, float* out,
                           int64_t ldo, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, int32_t* status,
                           manner_hip_stream_t stream) {
  int rc;
  if ((rc = gru_check("gru", B, S, I, H))) return rc;
  if (B == 0) return MANNER_HIP_OK;
  if (!x || !lengths || !w_ih || !w_hh || !b_ih || !b_hh || !out || !workspace) return fail(MANNER_HIP_E_INVALID, "gru: null pointer");
  if (ldo < H || x_stride_s < 0 || x_stride_b < 0) return fail(MANNER_HIP_E_INVALID, "gru: bad stride");
  if (workspace_bytes < manner_hip_gru_workspace_bytes(B, S, I, H)) return fail(MANNER_HIP_E_WORKSPACE, "gru: workspace too small");
  if (saved && saved_bytes < manner_hip_gru_saved_bytes(B, S, I, H)) return fail(MANNER_HIP_E_WORKSPACE, "gru: saved buffer too small");
  hipStream_t s = (hipStream_t)stream;
  FloatBump bw(workspace), bs(saved);
  Work w;
  Saved sv;
  plan_work(bw, w, (size_t)B, (size_t)S, (size_t)H);
  plan_saved(bs, sv, (size_t)B, (size_t)S, (size_t)I, (size_t)H);
  const int64_t R = B * S;
  const int Si = (int)S;
  if ((rc = launch_proj_rows(x, x_stride_b, x_stride_s, lengths, w_ih, b_ih, Si, 1, R, I, 3 * H, w.gi, saved ? sv.xs : nullptr, s))) return rc;
  const size_t BH = (size_t)B * H;
  if (saved) {                                       // hs[0] = h_0: the weight gradient reads it
    if (h0) MANNER_HIP_TRY(hipMemcpyAsync(sv.hs, h0, BH * sizeof(float), hipMemcpyDeviceToDevice, s));
    else MANNER_HIP_TRY(hipMemsetAsync(sv.hs, 0, BH * sizeof(float), s));
  }
  const dim3 grid((unsigned)((H + GR_UNITS - 1) / GR_UNITS), (unsigned)((B + GR_ROWS - 1) / GR_ROWS));
  const float* cur = saved ? sv.hs : h0;
  for (int t = 0; t < Si; ++t) {
    const bool last = t == Si - 1;
    float* dst = last ? out : (saved ? sv.hs + (size_t)(t + 1) * BH : w.h[t & 1]);
    const int64_t ldin = H, ldout = last ? ldo : H;
    if (saved)
      hipLaunchKernelGGL(step_kernel<true>, grid, dim3(GR_BLOCK), 0, s, w.gi, w_hh, b_hh, lengths, cur, ldin, dst, ldout, t, B, Si, (int)H,
                         sv.gates + (size_t)t * 4 * BH, status);
    else
      hipLaunchKernelGGL(step_kernel<false>, grid, dim3(GR_BLOCK), 0, s, w.gi, w_hh, b_hh, lengths, cur, ldin, dst, ldout, t, B, Si, (int)H,
                         (float*)nullptr, status);
    MANNER_LAUNCH_CHECK();
    cur = dst;
  }
  return MANNER_HIP_OK;
}

int manner_hip_gru_backward(const float* w_ih, const float* w_hh, const int64_t* lengths, const float* grad_out, int64_t ldg, int64_t B, int64_t S,
                            int32_t I, int32_t H, void* saved, size_t saved_bytes, float* grad_x, float* grad_h0, float* grad_w_ih,
                            float* grad_w_hh, float* grad_b_ih, float* grad_b_hh, void* workspace, size_t workspace_bytes,
                            manner_hip_stream_t stream) {
  int rc;
  if ((rc = gru_check("gru_backward", B, S, I, H))) return rc;
  if (!grad_w_ih || !grad_w_hh || !grad_b_ih || !grad_b_hh) return fail(MANNER_HIP_E_INVALID, "gru_backward: null gradient");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {                                      // no row: the parameter gradients are sums over nothing
    MANNER_HIP_TRY(hipMemsetAsync(grad_w_ih, 0, (size_t)3 * H * I * sizeof(float), s));
    MANNER_HIP_TRY(hipMemsetAsync(grad_w_hh, 0, (size_t)3 * H * H * sizeof(float), s));
    MANNER_HIP_TRY(hipMemsetAsync(grad_b_ih, 0, (size_t)3 * H * sizeof(float), s));
    MANNER_HIP_TRY(hipMemsetAsync(grad_b_hh, 0, (size_t)3 * H * sizeof(float), s));
    return MANNER_HIP_OK;
  }
  if (!w_ih || !w_hh || !lengths || !grad_out || !saved || !grad_x || !workspace) return fail(MANNER_HIP_E_INVALID, "gru_backward: null pointer");
  if (ldg < H) return fail(MANNER_HIP_E_INVALID, "gru_backward: bad stride");
  if (saved_bytes < manner_hip_gru_saved_bytes(B, S, I, H)) return fail(MANNER_HIP_E_WORKSPACE, "gru_backward: saved buffer too small");
  if (workspace_bytes < manner_hip_gru_workspace_bytes(B, S, I, H)) return fail(MANNER_HIP_E_WORKSPACE, "gru_backward: workspace too small");
  FloatBump bw(workspace), bs(saved);
  Work w;
  Saved sv;
  plan_work(bw, w, (size_t)B, (size_t)S, (size_t)H);
  plan_saved(bs, sv, (size_t)B, (size_t)S, (size_t)I, (size_t)H);
  const int Si = (int)S;
  const size_t BH = (size_t)B * H;
  float* dgi = w.gi;                                 // the forward's gi is dead: its place holds d gi [B S, 3H]
  if ((rc = launch_transpose_tile(w_hh, H, 3 * H, H, w.wt, s))) return rc;
  const dim3 grid((unsigned)((H + GR_UNITS - 1) / GR_UNITS), (unsigned)((B + GR_ROWS - 1) / GR_ROWS));
  const float* cur = grad_out;
  int64_t ldin = ldg;
  for (int t = Si - 1; t >= 0; --t) {
    float* dst = (t == 0 && grad_h0) ? grad_h0 : w.h[t & 1];
    hipLaunchKernelGGL(bstep_kernel, grid, dim3(GR_BLOCK), 0, s, w.wt, lengths, cur, ldin, dst, (int64_t)H, sv.hs + (size_t)t * BH,
                       sv.gates + (size_t)t * 4 * BH, dgi, w.dgh + (size_t)t * 3 * BH, t, B, Si, (int)H);
    MANNER_LAUNCH_CHECK();
    cur = dst;
    ldin = H;
  }
  const int64_t R = B * S;
  if ((rc = manner_hip_linear_backward(sv.hs, nullptr, w.dgh, R, H, 3 * H, nullptr, nullptr, grad_w_hh, grad_b_hh, stream))) return rc;
  return manner_hip_linear_backward(sv.xs, w_ih, dgi, R, I, 3 * H, nullptr, grad_x, grad_w_ih, grad_b_ih, stream);
}

int manner_hip_user_rows(const int64_t* ids, const float* src, int64_t n_rows, int64_t ld_src, int64_t B, int32_t E, float p, uint64_t seed,
                         uint32_t site, float* out, int64_t ld_out, int32_t* status, manner_hip_stream_t stream) {
  if (B < 0 || E <= 0 || B > 0x7fffffffll || ld_src < E || ld_out < E || (ids && n_rows <= 0))
    return fail(MANNER_HIP_E_INVALID, "user_rows: bad shape B=%lld E=%d", (long long)B, E);
  if (!(p >= 0.f && p < 1.f)) return fail(MANNER_HIP_E_INVALID, "user_rows: p=%f outside [0, 1)", p);
  if (B == 0) return MANNER_HIP_OK;
  if (!src || !out) return fail(MANNER_HIP_E_INVALID, "user_rows: null pointer");
  hipLaunchKernelGGL(user_rows_kernel, dim3((unsigned)B), dim3(GR_BLOCK), 0, (hipStream_t)stream, ids, src, n_rows, ld_src, (int)E, make_drop(seed, site, p), out,
                     ld_out, status);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // extern "C"
