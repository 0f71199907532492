// The module lines of the MINER baseline (reference manner/models/baselines/miner_module.py:153-242) between the leaf operators of
// poly.hip, f32, forward and backward:
//   category bias      (miner_module.py:162-181 + attention.py:75)  mean over ALL candidates of the batch of the category cosine, the
//                                                                   user's own candidates zeroed — as a [B, S, 1] bias for poly attention
//   code scores        (miner_module.py:195-202)                    max / mean over the K context codes of cand . user_k, ragged
//   disagreement loss  (miner_module.py:237-241, utils.py:4-31)     mean of the off-diagonal cosines among a user's K vectors
// Small, launch-bound wave-reduction kernels (wave64) on whole coalesced rows; nothing here needs the matrix pipe.  Every reduction
// across rows runs in a fixed order (no floating-point atomics): two runs give the same bits.
#include <math.h>

#include <algorithm>

#include "train_common.h"

namespace manner {
namespace {

constexpr int MN_MAX_DC = 1024, MN_MAX_S = 256, MN_MAX_K = 64, MN_MAX_D = 1024;
constexpr int MN_J = MN_MAX_D / 64;            // row elements per lane
static_assert(MN_MAX_DC == MN_MAX_D, "one row holder for both widths");


// ---------------------------------------------------------------- category bias
// Unit rows, one wave per row r of [candidates (T rows) | history (NH rows)]: unit[r, :] = e / ||e||, e = dropout(table[cat[r], :]).
// torchmetrics' pairwise_cosine_similarity divides by the norm itself — no epsilon: an all-zero row becomes 0 / 0 = NaN.  Dropout
// element index: (row within its side) * Dc + d, one site and one seed per side.  A category id outside [0, V) is never read: it raises
// MANNER_HIP_STATUS_INDEX and the row counts as zeros.
__global__ __launch_bounds__(256) void mn_unit_rows_kernel(const int64_t* __restrict__ cand_cat, const int64_t* __restrict__ hist_cat,
                                                           const float* __restrict__ table, int64_t V, int Dc, int64_t T, int64_t NH, Drop dh,
                                                           Drop dc, float* __restrict__ unit, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= T + NH) return;                                    // wave-uniform
  const bool is_cand = r < T;
  const int64_t side_row = is_cand ? r : r - T;
  const int64_t id = is_cand ? cand_cat[side_row] : hist_cat[side_row];
  const bool bad = id < 0 || id >= V;
  if (bad && lane == 0 && status) atomicOr(status, MANNER_HIP_STATUS_INDEX);
  const Drop drop = is_cand ? dc : dh;
  const float* row = table + (size_t)(bad ? 0 : id) * Dc;
  float e[MN_J], sq = 0.f;
#pragma unroll
  for (int j = 0; j < MN_J; ++j) {
    const int d = lane + 64 * j;
    e[j] = (d < Dc && !bad) ? drop.apply(row[d], (uint64_t)side_row * (uint64_t)Dc + (uint64_t)d) : 0.f;
    sq = fmaf(e[j], e[j], sq);
  }
  const float norm = sqrtf(wsum(sq));
#pragma unroll
  for (int j = 0; j < MN_J; ++j) {
    const int d = lane + 64 * j;
    if (d < Dc) unit[(size_t)r * Dc + d] = e[j] / norm;
  }
}

// grid (B, ceil(Dc / 64)): Y[b, d] = sum of the unit candidate rows t NOT among user b's own [c0, c1), summed directly (never
// Y_all - Y_own: that would lose the exact zeros and move the NaNs).  Wave w takes the columns t = w, w + 4, ... in ascending order on
// one chain; the four chains add as (0 + 1) + (2 + 3).
__global__ __launch_bounds__(256) void mn_exclusion_sum_kernel(const float* __restrict__ unit, const int64_t* __restrict__ cand_off, int64_t T,
                                                               int Dc, float* __restrict__ Y) {
  __shared__ float part[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = blockIdx.x;
  const int d = blockIdx.y * 64 + lane;
  const int64_t c0 = clampi(cand_off[b], 0, T), c1 = clampi(cand_off[b + 1], c0, T);
  float acc = 0.f;
  if (d < Dc) {
    for (int64_t t = wave; t < T; t += 4)
      if (t < c0 || t >= c1) acc += unit[(size_t)t * Dc + d];
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && d < Dc) Y[(size_t)b * Dc + d] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// One wave per dense slot (b, s): bias[b, s] = unit_hist[h0 + s, :] . Y[b, :] / T for a real slot, exactly 0 for a padded slot and for
// an empty exclusion set (every candidate of the batch is the user's own: the reference zeroes all columns, NaN rows included).
__global__ __launch_bounds__(256) void mn_bias_kernel(const float* __restrict__ unit_hist, const float* __restrict__ Y,
                                                      const int64_t* __restrict__ hist_off, const int64_t* __restrict__ cand_off, int64_t NH,
                                                      int64_t T, int64_t B, int S, int Dc, float* __restrict__ bias) {
  const int lane = threadIdx.x & 63;
  const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= B * S) return;                                  // wave-uniform
  const int64_t b = slot / S;
  const int s = (int)(slot - b * S);
  const int64_t h0 = clampi(hist_off[b], 0, NH), h1 = clampi(hist_off[b + 1], h0, NH);
  const int64_t c0 = clampi(cand_off[b], 0, T), c1 = clampi(cand_off[b + 1], c0, T);
  float v = 0.f;
  if (h0 + s < h1 && T - (c1 - c0) > 0) {
    const float* x = unit_hist + (size_t)(h0 + s) * Dc;
    const float* y = Y + (size_t)b * Dc;
    float a0 = 0.f, a1 = 0.f;
    int d = lane;
    for (; d + 64 < Dc; d += 128) { a0 = fmaf(x[d], y[d], a0); a1 = fmaf(x[d + 64], y[d + 64], a1); }
    if (d < Dc) a0 = fmaf(x[d], y[d], a0);
    v = wsum(a0 + a1) / (float)T;
  }
  if (lane == 0) bias[slot] = v;
}

// ---------------------------------------------------------------- scores over the context codes
__device__ __forceinline__ int64_t segment_of(const int64_t* __restrict__ off, int64_t B, int64_t t) {
  int64_t lo = 0, hi = B;                                      // the last b with off[b] <= t
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// One wave per candidate t of user b: v_k = cand[t, :] . user[b, k, :] for k = 0 .. K - 1, then max_k (MEAN false; ties keep the LOWEST
// k, as torch's max(dim) on the CPU does; `arg` receives it when given) or (sum_k v_k) / K (MEAN true).
template <bool MEAN>
__global__ __launch_bounds__(256) void mn_code_scores_kernel(const float* __restrict__ cand, const int64_t* __restrict__ cand_off,
                                                             const float* __restrict__ user, int64_t N, int64_t B, int K, int D,
                                                             float* __restrict__ out, int32_t* __restrict__ arg) {
  const int lane = threadIdx.x & 63;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < N; t += (int64_t)gridDim.x * 4) {
    const int64_t b = segment_of(cand_off, B, t);
    float c[MN_J];
#pragma unroll
    for (int j = 0; j < MN_J; ++j) {
      const int d = lane + 64 * j;
      c[j] = d < D ? cand[(size_t)t * D + d] : 0.f;
    }
    const float* ub = user + (size_t)b * K * D;
    float best = 0.f, total = 0.f;
    int best_k = 0;
    for (int k = 0; k < K; ++k) {
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < MN_J; ++j) {
        const int d = lane + 64 * j;
        if (d < D) a = fmaf(c[j], ub[(size_t)k * D + d], a);
      }
      a = wsum(a);
      if (MEAN) {
        total += a;
      } else if (k == 0 || a > best) {
        best = a;
        best_k = k;
      }
    }
    if (lane == 0) {
      out[t] = MEAN ? total / (float)K : best;
      if (!MEAN && arg) arg[t] = best_k;
    }
  }
}

// d cand[t, :] = g[t] user[b, arg[t], :] (max) or (g[t] / K) sum_k user[b, k, :] (mean, ascending k).  One wave per candidate.
template <bool MEAN>
__global__ __launch_bounds__(256) void mn_code_scores_dcand_kernel(const float* __restrict__ g, const int64_t* __restrict__ cand_off,
                                                                   const float* __restrict__ user, const int32_t* __restrict__ arg, int64_t N,
                                                                   int64_t B, int K, int D, float* __restrict__ dcand) {
  const int lane = threadIdx.x & 63;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < N; t += (int64_t)gridDim.x * 4) {
    const int64_t b = segment_of(cand_off, B, t);
    const float* ub = user + (size_t)b * K * D;
    const float gt = g[t];
    if (MEAN) {
      const float w = gt / (float)K;
      for (int d = lane; d < D; d += 64) {
        float a = 0.f;
        for (int k = 0; k < K; ++k) a += ub[(size_t)k * D + d];
        dcand[(size_t)t * D + d] = w * a;
      }
    } else {
      const float* ur = ub + (size_t)min(max(arg[t], 0), K - 1) * D;
      for (int d = lane; d < D; d += 64) dcand[(size_t)t * D + d] = gt * ur[d];
    }
  }
}

// grid (B, K) (max) or (B, 1) (mean): d user[b, k, d] = sum over the user's candidates t in ascending order of g[t] cand[t, d] — those
// with arg[t] == k (max), or all of them, divided by K and written to every k (mean).
template <bool MEAN>
__global__ __launch_bounds__(256) void mn_code_scores_duser_kernel(const float* __restrict__ g, const float* __restrict__ cand,
                                                                   const int64_t* __restrict__ cand_off, const int32_t* __restrict__ arg, int64_t N,
                                                                   int K, int D, float* __restrict__ duser) {
  const int64_t b = blockIdx.x;
  const int k = blockIdx.y;
  const int64_t c0 = clampi(cand_off[b], 0, N), c1 = clampi(cand_off[b + 1], c0, N);
  for (int d = threadIdx.x; d < D; d += 256) {
    float a = 0.f;
    for (int64_t t = c0; t < c1; ++t)
      if (MEAN || arg[t] == k) a = fmaf(g[t], cand[(size_t)t * D + d], a);
    if (MEAN) {
      a = a / (float)K;
      for (int kk = 0; kk < K; ++kk) duser[((size_t)b * K + kk) * D + d] = a;
    } else {
      duser[((size_t)b * K + k) * D + d] = a;
    }
  }
}

// ---------------------------------------------------------------- disagreement loss
// utils.py:4-31 with zero_diagonal=True, then .mean(): unit rows u_i = x_i / (1e-8 + ||x_i||) (the two `x_norm[torch.where(x_norm)
// == 0.0] = 1` lines of the reference index with a tuple compared to a float, i.e. with False: they change nothing), the sum over
// i != j of u_i . u_j, divided by B K K.  No K x K matrix: with s = sum_j u_j and r_i = s - u_i the sum is sum_i u_i . r_i.
// The first two phases, shared by forward and backward: den[i] = 1e-8 + ||x_i|| and s[d] = sum_i x[i, d] / den[i] (ascending i).
// All 256 threads call it; it ends with a barrier.
__device__ __forceinline__ void unit_sum(const float* __restrict__ xb, int K, int D, float* nrm, float* den, float* s) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < K; i += 4) {
    float sq = 0.f;
    for (int d = lane; d < D; d += 64) { const float v = xb[(size_t)i * D + d]; sq = fmaf(v, v, sq); }
    const float n = sqrtf(wsum(sq));
    if (lane == 0) { nrm[i] = n; den[i] = 1e-8f + n; }
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += 256) {
    float a = 0.f;
    for (int i = 0; i < K; ++i) a += xb[(size_t)i * D + d] / den[i];
    s[d] = a;
  }
  __syncthreads();
}

// grid (B): part[b] = sum_i u_i . (s - u_i), the products of a row summed per lane in f32, across the lanes and the rows in f64
__global__ __launch_bounds__(256) void mn_disagreement_fwd_kernel(const float* __restrict__ x, int K, int D, double* __restrict__ part) {
  __shared__ float nrm[MN_MAX_K], den[MN_MAX_K], s[MN_MAX_D];
  __shared__ double rowdot[MN_MAX_K];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* xb = x + (size_t)blockIdx.x * K * D;
  unit_sum(xb, K, D, nrm, den, s);
  for (int i = wave; i < K; i += 4) {
    float a = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float u = xb[(size_t)i * D + d] / den[i];
      a = fmaf(u, s[d] - u, a);
    }
    const double tot = wsum((double)a);
    if (lane == 0) rowdot[i] = tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < K; ++i) tot += rowdot[i];
    part[blockIdx.x] = tot;
  }
}
// one wave: lane l adds the users l, l + 64, ... in ascending order, the 64 sums meet in the butterfly; loss = total / (B K K)
__global__ __launch_bounds__(64) void mn_disagreement_reduce_kernel(const double* __restrict__ part, int64_t B, int K, float* __restrict__ loss) {
  double a = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += 64) a += part[b];
  a = wsum(a);
  if (threadIdx.x == 0) loss[0] = (float)(a / ((double)B * (double)K * (double)K));
}

// grid (B): with c_i = (2 g / (B K K)) (s - u_i) = d L / d u_i, through the normalisation
//   d x_i = c_i / den_i - (c_i . u_i) u_i / ||x_i||     and, for a zero row (torch's norm has the subgradient 0 there), d x_i = c_i / 1e-8.
__global__ __launch_bounds__(256) void mn_disagreement_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, int64_t B, int K, int D,
                                                                  float* __restrict__ dx) {
  __shared__ float nrm[MN_MAX_K], den[MN_MAX_K], s[MN_MAX_D];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* xb = x + (size_t)blockIdx.x * K * D;
  float* dxb = dx + (size_t)blockIdx.x * K * D;
  unit_sum(xb, K, D, nrm, den, s);
  const float coef = (float)(2.0 * (double)g[0] / ((double)B * (double)K * (double)K));
  for (int i = wave; i < K; i += 4) {
    float u[MN_J], c[MN_J], a = 0.f;
#pragma unroll
    for (int j = 0; j < MN_J; ++j) {
      const int d = lane + 64 * j;
      u[j] = d < D ? xb[(size_t)i * D + d] / den[i] : 0.f;
      c[j] = d < D ? coef * (s[d] - u[j]) : 0.f;
      a = fmaf(c[j], u[j], a);
    }
    const float dot = (float)wsum((double)a);
    const float n = nrm[i];
#pragma unroll
    for (int j = 0; j < MN_J; ++j) {
      const int d = lane + 64 * j;
      if (d < D) dxb[(size_t)i * D + d] = n > 0.f ? c[j] / den[i] - dot * u[j] / n : c[j] / den[i];
    }
  }
}

int scores_check(const char* who, int64_t N, int64_t B, int K, int D, int mode) {
  if (N < 0 || B < 0 || K < 1 || D < 1) return fail(MANNER_HIP_E_INVALID, "%s: bad shape N=%lld B=%lld K=%d D=%d", who, (long long)N, (long long)B, K, D);
  if (K > MN_MAX_K) return fail(MANNER_HIP_E_INVALID, "%s: K=%d unsupported (K <= %d)", who, K, MN_MAX_K);
  if (D > MN_MAX_D) return fail(MANNER_HIP_E_INVALID, "%s: D=%d unsupported (D <= %d)", who, D, MN_MAX_D);
  if (mode != 0 && mode != 1) return fail(MANNER_HIP_E_INVALID, "%s: mode=%d (0 = max, 1 = mean)", who, mode);
  if (B > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "%s: B exceeds the grid", who);
  return MANNER_HIP_OK;
}
int disagreement_check(const char* who, int64_t B, int K, int D) {
  if (B < 0 || K < 1 || D < 1) return fail(MANNER_HIP_E_INVALID, "%s: bad shape B=%lld K=%d D=%d", who, (long long)B, K, D);
  if (K > MN_MAX_K) return fail(MANNER_HIP_E_INVALID, "%s: K=%d unsupported (K <= %d)", who, K, MN_MAX_K);
  if (D > MN_MAX_D) return fail(MANNER_HIP_E_INVALID, "%s: D=%d unsupported (D <= %d)", who, D, MN_MAX_D);
  if (B > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "%s: B exceeds the grid", who);
  return MANNER_HIP_OK;
}
unsigned wave_grid(int64_t waves) {
  const int64_t blocks = (waves + 3) / 4;
  return (unsigned)(blocks < 65536 ? blocks : 65536);
}

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" {

size_t manner_hip_miner_category_bias_workspace_bytes(int64_t n_hist, int64_t T, int64_t B, int32_t Dc) {
  if (n_hist < 0 || T < 0 || B <= 0 || Dc <= 0) return 0;
  return (size_t)(n_hist + T + B) * (size_t)Dc * sizeof(float) + 256;
}

int manner_hip_miner_category_bias(const int64_t* hist_cat, const int64_t* cand_cat, const float* table, int64_t V, int32_t Dc,
                                   const int64_t* hist_off, const int64_t* cand_off, int64_t n_hist, int64_t T, int64_t B, int64_t S, float p,
                                   uint64_t seed_hist, uint64_t seed_cand, uint32_t site_hist, uint32_t site_cand, float* bias, void* workspace,
                                   size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream) {
  if (B < 0 || S < 1 || Dc < 1 || V < 1 || n_hist < 0 || T < 0)
    return fail(MANNER_HIP_E_INVALID, "miner_category_bias: bad shape B=%lld S=%lld Dc=%d V=%lld N_hist=%lld T=%lld", (long long)B, (long long)S, Dc,
                (long long)V, (long long)n_hist, (long long)T);
  if (Dc > MN_MAX_DC) return fail(MANNER_HIP_E_INVALID, "miner_category_bias: Dc=%d unsupported (Dc <= %d)", Dc, MN_MAX_DC);
  if (S > MN_MAX_S) return fail(MANNER_HIP_E_INVALID, "miner_category_bias: S=%lld unsupported (S <= %d)", (long long)S, MN_MAX_S);
  if (!(p >= 0.f && p < 1.f)) return fail(MANNER_HIP_E_INVALID, "miner_category_bias: p=%g outside [0, 1)", (double)p);
  if (B > 0x7fffffffll || (n_hist + T + 3) / 4 > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "miner_category_bias: B or the rows exceed the grid");
  if (B == 0) return MANNER_HIP_OK;
  if (!table || !hist_off || !cand_off || !bias || !workspace || (n_hist > 0 && !hist_cat) || (T > 0 && !cand_cat))
    return fail(MANNER_HIP_E_INVALID, "miner_category_bias: null pointer");
  if (workspace_bytes < manner_hip_miner_category_bias_workspace_bytes(n_hist, T, B, Dc))
    return fail(MANNER_HIP_E_WORKSPACE, "miner_category_bias: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* unit = static_cast<float*>(workspace);         // [T + N_hist, Dc]: unit candidate rows, then unit history rows
  float* Y = unit + (size_t)(T + n_hist) * Dc;          // [B, Dc]
  if (T + n_hist > 0) {
    hipLaunchKernelGGL(mn_unit_rows_kernel, dim3((unsigned)((T + n_hist + 3) / 4)), dim3(256), 0, s, cand_cat, hist_cat, table, V, (int)Dc, T, n_hist,
                       make_drop(seed_hist, site_hist, p), make_drop(seed_cand, site_cand, p), unit, status);
    MANNER_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mn_exclusion_sum_kernel, dim3((unsigned)B, (unsigned)((Dc + 63) / 64)), dim3(256), 0, s, unit, cand_off, T, (int)Dc, Y);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(mn_bias_kernel, dim3((unsigned)((B * S + 3) / 4)), dim3(256), 0, s, unit + (size_t)T * Dc, Y, hist_off, cand_off, n_hist, T, B,
                     (int)S, (int)Dc, bias);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_miner_code_scores(const float* cand, const int64_t* cand_off, const float* user, int64_t N, int64_t B, int32_t K, int32_t D,
                                 int32_t mode, float* out, int32_t* argmax, manner_hip_stream_t stream) {
  int rc;
  if ((rc = scores_check("miner_code_scores", N, B, K, D, mode))) return rc;
  if (N == 0 || B == 0) return MANNER_HIP_OK;
  if (!cand || !cand_off || !user || !out) return fail(MANNER_HIP_E_INVALID, "miner_code_scores: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (mode == 1)
    hipLaunchKernelGGL(mn_code_scores_kernel<true>, dim3(wave_grid(N)), dim3(256), 0, s, cand, cand_off, user, N, B, (int)K, (int)D, out, argmax);
  else
    hipLaunchKernelGGL(mn_code_scores_kernel<false>, dim3(wave_grid(N)), dim3(256), 0, s, cand, cand_off, user, N, B, (int)K, (int)D, out, argmax);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_miner_code_scores_backward(const float* grad_out, const float* cand, const int64_t* cand_off, const float* user,
                                          const int32_t* argmax, int64_t N, int64_t B, int32_t K, int32_t D, int32_t mode, float* grad_cand,
                                          float* grad_user, manner_hip_stream_t stream) {
  int rc;
  if ((rc = scores_check("miner_code_scores_backward", N, B, K, D, mode))) return rc;
  if (B == 0) return MANNER_HIP_OK;
  if (!cand_off || !grad_user) return fail(MANNER_HIP_E_INVALID, "miner_code_scores_backward: null pointer");
  if (N > 0 && (!grad_out || !cand || !user || !grad_cand || (mode == 0 && !argmax)))
    return fail(MANNER_HIP_E_INVALID, "miner_code_scores_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (mode == 1) {
    if (N > 0) hipLaunchKernelGGL(mn_code_scores_dcand_kernel<true>, dim3(wave_grid(N)), dim3(256), 0, s, grad_out, cand_off, user, argmax, N, B, (int)K, (int)D, grad_cand);
    hipLaunchKernelGGL(mn_code_scores_duser_kernel<true>, dim3((unsigned)B, 1), dim3(256), 0, s, grad_out, cand, cand_off, argmax, N, (int)K, (int)D, grad_user);
  } else {
    if (N > 0) hipLaunchKernelGGL(mn_code_scores_dcand_kernel<false>, dim3(wave_grid(N)), dim3(256), 0, s, grad_out, cand_off, user, argmax, N, B, (int)K, (int)D, grad_cand);
    hipLaunchKernelGGL(mn_code_scores_duser_kernel<false>, dim3((unsigned)B, (unsigned)K), dim3(256), 0, s, grad_out, cand, cand_off, argmax, N, (int)K, (int)D, grad_user);
  }
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

size_t manner_hip_disagreement_loss_workspace_bytes(int64_t B) { return B <= 0 ? 0 : (size_t)B * sizeof(double) + 256; }

int manner_hip_disagreement_loss(const float* user, int64_t B, int32_t K, int32_t D, float* loss, void* workspace, size_t workspace_bytes,
                                 manner_hip_stream_t stream) {
  int rc;
  if ((rc = disagreement_check("disagreement_loss", B, K, D))) return rc;
  if (B == 0) return fail(MANNER_HIP_E_INVALID, "disagreement_loss: no user (the mean of nothing)");
  if (!user || !loss || !workspace) return fail(MANNER_HIP_E_INVALID, "disagreement_loss: null pointer");
  if (workspace_bytes < manner_hip_disagreement_loss_workspace_bytes(B)) return fail(MANNER_HIP_E_WORKSPACE, "disagreement_loss: workspace too small");
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return fail(MANNER_HIP_E_INVALID, "disagreement_loss: workspace not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(mn_disagreement_fwd_kernel, dim3((unsigned)B), dim3(256), 0, s, user, (int)K, (int)D, part);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(mn_disagreement_reduce_kernel, dim3(1), dim3(64), 0, s, part, B, (int)K, loss);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_disagreement_loss_backward(const float* user, const float* grad_loss, int64_t B, int32_t K, int32_t D, float* grad_user,
                                          manner_hip_stream_t stream) {
  int rc;
  if ((rc = disagreement_check("disagreement_loss_backward", B, K, D))) return rc;
  if (B == 0) return MANNER_HIP_OK;
  if (!user || !grad_loss || !grad_user) return fail(MANNER_HIP_E_INVALID, "disagreement_loss_backward: null pointer");
  hipLaunchKernelGGL(mn_disagreement_bwd_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, user, grad_loss, B, (int)K, (int)D, grad_user);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // extern "C"
