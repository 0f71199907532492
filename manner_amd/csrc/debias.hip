// What makes SentiDebias-PLM itself (reference manner/models/baselines/senti_debias_plm_module.py:94-148, 163-167, 275-280), f32, forward
// and backward.  The sentiment encoder has only C = num_sent_classes distinct outputs, the CLASS TABLE T [C, D] (formed by the caller with
// linear_tanh on the C embedding rows); everything here reads T through a row's class and never writes the [N, D] sentiment rows:
//   orth_loss     |mean_hist cos(row, T[cls])| + |mean_cand cos(row, T[cls])| + mean_b |cos(user_free_b, user_aware_b)|,
//                 cos(a, b) = a . b / (1e-8 + |a| |b|)
//   class_dense   to_dense_batch of the sentiment rows: [B, width, D], zero padding
//   class_scores  user_aware_b . T[cls_t] on the ragged candidates, from the [B, C] products
//   adv_loss      Discriminator.forward + adversarial_loss on both row sets: mean_hist CE + mean_cand CE against class (cls - 1) mod O;
//                 layer 1 on the f32 matrix cores (wlin_kernel of caum.hip), layer 2 with the softmax as a row walk under a staged W2
// A row kernel gives a wave one row at a time, the row in registers, under a grid-stride loop.  Every reduction across rows has a fixed
// order (no floating-point atomics) and every grid comes from the shape alone: two runs give the same bits on any CU count.  A class
// outside its table is never used as an index: it raises MANNER_HIP_STATUS_INDEX and its row counts as 0 with gradient 0.
#include <math.h>

#include <algorithm>

#include "row_head.h"

namespace manner {
namespace {

// the row kernels here walk as row_head.h's do and bin as its weight gradient does
constexpr int DB_MAX_D = RH_MAX_D;                       // a row (news vector, or hidden activation) in registers: 16 floats per lane
constexpr int DB_MAX_C = 64, DB_MAX_O = RH_MAX_O;        // classes of the table; outputs of the discriminator (one per lane)
constexpr int DB_J = RH_J;
constexpr int DB_WG_ROWS = RH_WG_ROWS;                   // rows a workgroup takes per trip of its grid-stride loop
constexpr int DB_CHUNK_ROWS = RH_CHUNK_ROWS, DB_MAX_CHUNKS = RH_MAX_CHUNKS;      // binned sums: rows per partial sum at least; partial sums at most
constexpr float DB_EPS = 1e-8f;

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }      // torch's sign: 0 at 0 and at NaN


// all 256 threads: the sum of the threads' `a` in a fixed tree
__device__ __forceinline__ double block_sum(double a, double* sm) {
  __syncthreads();
  sm[threadIdx.x] = a;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  return sm[0];
}

// ---------------------------------------------------------------- cosines of row pairs
// one wave: a . b, |a|, |b| of two rows held as lane + 64 j (zeros past D)
struct Cos { float dot, na, nb; };
__device__ __forceinline__ Cos row_cos(const float (&a)[DB_J], const float (&b)[DB_J]) {
  float d = 0.f, sa = 0.f, sb = 0.f;
#pragma unroll
  for (int j = 0; j < DB_J; ++j) {
    d = fmaf(a[j], b[j], d);
    sa = fmaf(a[j], a[j], sa);
    sb = fmaf(b[j], b[j], sb);
  }
  return Cos{wsum(d), sqrtf(wsum(sa)), sqrtf(wsum(sb))};
}
__device__ __forceinline__ void load_row(const float* __restrict__ p, int D, int lane, float (&v)[DB_J]) {
#pragma unroll
  for (int j = 0; j < DB_J; ++j) v[j] = (p && lane + 64 * j < D) ? p[lane + 64 * j] : 0.f;
}
// the partner of row r: T[cls[r]] with a class table (NULL for a class outside it), other[r] without
__device__ __forceinline__ const float* partner(const float* __restrict__ other, const int64_t* __restrict__ cls, int64_t r, int D, int C) {
  if (!cls) return other + (size_t)r * D;
  const int64_t t = cls[r];
  return (t < 0 || t >= C) ? nullptr : other + (size_t)t * D;
}

// cosv[r] = cos(x[r], partner(r)).  Wave w of workgroup g takes the rows 8 (g + k G) + w + 4 i.
__global__ __launch_bounds__(256) void db_cos_fwd_kernel(const float* __restrict__ x, const float* __restrict__ other, const int64_t* __restrict__ cls,
                                                         int64_t N, int D, int C, float* __restrict__ cosv, int32_t* __restrict__ status) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * DB_WG_ROWS; base < N; base += (int64_t)gridDim.x * DB_WG_ROWS) {
    const int64_t end = base + DB_WG_ROWS < N ? base + DB_WG_ROWS : N;
    for (int64_t r = base + wave; r < end; r += 4) {
      float a[DB_J], b[DB_J];
      const float* o = partner(other, cls, r, D, C);
      load_row(x + (size_t)r * D, D, lane, a);
      load_row(o, D, lane, b);
      const Cos c = row_cos(a, b);
      if (lane == 0) {
        cosv[r] = o ? c.dot / (DB_EPS + c.na * c.nb) : 0.f;
        if (!o && status) atomicOr(status, MANNER_HIP_STATUS_INDEX);
      }
    }
  }
}

// One workgroup: out[0] = f(mean of v[0, n0)) + f(mean of v[n0, n)) + (u ? mean of |u[0, B)| : 0), f = |.| with ABS; means[0 .. 1] (may
// be NULL) receive the two means.  Thread i adds the entries i, i + 256, ... of a segment in ascending order in f64, the 256 sums meet in
// a fixed tree.  An empty segment is 0 / 0 = NaN, as torch.mean of nothing.
template <bool ABS>
__global__ __launch_bounds__(256) void db_segment_means_kernel(const float* __restrict__ v, int64_t n0, int64_t n, const float* __restrict__ u, int64_t B,
                                                               float* __restrict__ out, float* __restrict__ means) {
  __shared__ double sm[256];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n0; i += 256) a += (double)v[i];
  const double m0 = block_sum(a, sm) / (double)n0;
  a = 0.0;
  for (int64_t i = n0 + threadIdx.x; i < n; i += 256) a += (double)v[i];
  const double m1 = block_sum(a, sm) / (double)(n - n0);
  double m2 = 0.0;
  if (u) {
    a = 0.0;
    for (int64_t i = threadIdx.x; i < B; i += 256) a += (double)fabsf(u[i]);
    m2 = block_sum(a, sm) / (double)B;
  }
  if (threadIdx.x == 0) {
    out[0] = (float)((ABS ? fabs(m0) : m0) + (ABS ? fabs(m1) : m1) + m2);
    if (means) { means[0] = (float)m0; means[1] = (float)m1; }
  }
}

// The backward of a cosine, d cos / d a = b / den - (a . b) |b| (a / |a|) / den^2 with den = 1e-8 + |a| |b| and torch's zero gradient
// through the norm of a zero vector, times the row's coefficient:
//   with a class table: coef = g sign(means[segment]) / (rows of the segment); da -> dx (may be NULL); pq [N, 2] (may be NULL) receives
//     p = coef / den and q = coef (a . b) |a| / (den^2 |b|): d T[c] = sum over the rows of class c of p x - q T[c] (db_bin_kernel)
//   without: coef = g sign(cos_r) / N; da -> dx, db -> dother (each may be NULL)
__global__ __launch_bounds__(256) void db_cos_bwd_kernel(const float* __restrict__ g, const float* __restrict__ means, const float* __restrict__ x,
                                                         const float* __restrict__ other, const int64_t* __restrict__ cls, int64_t n0, int64_t N, int D,
                                                         int C, float* __restrict__ dx, float* __restrict__ dother, float* __restrict__ pq) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * DB_WG_ROWS; base < N; base += (int64_t)gridDim.x * DB_WG_ROWS) {
    const int64_t end = base + DB_WG_ROWS < N ? base + DB_WG_ROWS : N;
    for (int64_t r = base + wave; r < end; r += 4) {
      float a[DB_J], b[DB_J];
      const float* o = partner(other, cls, r, D, C);
      load_row(x + (size_t)r * D, D, lane, a);
      load_row(o, D, lane, b);
      const Cos c = row_cos(a, b);
      const float den = DB_EPS + c.na * c.nb;
      float coef;
      if (cls) coef = r < n0 ? g[0] * sgn(means[0]) / (float)n0 : g[0] * sgn(means[1]) / (float)(N - n0);
      else coef = g[0] * sgn(c.dot / den) / (float)N;
      if (!o) coef = 0.f;
      const float p = coef / den;
      const float ka = c.na > 0.f ? coef * c.dot * c.nb / (den * den * c.na) : 0.f;
      const float kb = c.nb > 0.f ? coef * c.dot * c.na / (den * den * c.nb) : 0.f;
#pragma unroll
      for (int j = 0; j < DB_J; ++j) {
        const int d = lane + 64 * j;
        if (d < D) {
          if (dx) dx[(size_t)r * D + d] = p * b[j] - ka * a[j];
          if (dother) dother[(size_t)r * D + d] = p * a[j] - kb * b[j];
        }
      }
      if (pq && lane == 0) {
        pq[2 * r] = p;
        pq[2 * r + 1] = kb;
      }
    }
  }
}

// ---------------------------------------------------------------- binned per-class sums: the gradient of the class table
// part[chunk][c][dd] = the sum over the chunk's rows of class c, ascending, of (dd < D ? p_r x[m, dd] : q_r); p = 1, q = 0 without pq.
// One wave per (64 columns, chunk): lane = column, the C accumulators of a lane in LDS (acc[c][lane], touched by that lane alone).
// DENSE: the rows are the slots m = b width + j of a dense [B, width, D] block, slot j of user b holding row off[b] + j when it has one —
// ascending m is ascending r.
template <bool DENSE>
__global__ __launch_bounds__(64) void db_bin_kernel(const float* __restrict__ x, const float* __restrict__ pq, const int64_t* __restrict__ cls,
                                                    const int64_t* __restrict__ off, int64_t width, int64_t M, int64_t N, int D, int C,
                                                    int64_t chunk_rows, float* __restrict__ part) {
  __shared__ float acc[DB_MAX_C * 64];
  const int lane = threadIdx.x;
  const int dd = blockIdx.x * 64 + lane;
  for (int c = 0; c < C; ++c) acc[c * 64 + lane] = 0.f;
  const int64_t m0 = (int64_t)blockIdx.y * chunk_rows, m1 = m0 + chunk_rows < M ? m0 + chunk_rows : M;
  for (int64_t m = m0; m < m1; ++m) {
    int64_t r = m;
    if (DENSE) {
      const int64_t b = m / width, j = m - b * width;
      const int64_t o0 = clampi(off[b], 0, N), o1 = clampi(off[b + 1], o0, N);
      if (j >= o1 - o0) continue;
      r = o0 + j;
    }
    const int64_t t = cls[r];
    if (t < 0 || t >= C) continue;
    float* slot = acc + (int)t * 64 + lane;
    if (dd < D) *slot = fmaf(pq ? pq[2 * r] : 1.f, x[(size_t)m * D + dd], *slot);
    else if (dd == D && pq) *slot += pq[2 * r + 1];
  }
  if (dd <= D)
    for (int c = 0; c < C; ++c) part[((size_t)blockIdx.y * C + c) * (D + 1) + dd] = acc[c * 64 + lane];
}
// one thread per (c, d): the chunks in ascending order; minus T[c, d] times the q column with T
__global__ __launch_bounds__(256) void db_bin_reduce_kernel(const float* __restrict__ part, const float* __restrict__ T, int D, int C, int chunks,
                                                            float* __restrict__ dT) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * D) return;
  const int c = i / D, d = i - c * D;
  float a = 0.f, q = 0.f;
  for (int k = 0; k < chunks; ++k) a += part[((size_t)k * C + c) * (D + 1) + d];
  if (T) {
    for (int k = 0; k < chunks; ++k) q += part[((size_t)k * C + c) * (D + 1) + D];
    a = fmaf(-T[i], q, a);
  }
  dT[i] = a;
}

// ---------------------------------------------------------------- class_dense / class_scores
// out[b, j] = T[cls[off[b] + j]] for j < c_b, zeros past it: one wave per dense row.  A user with more rows than `width` raises
// MANNER_HIP_STATUS_LENGTHS (the rows past it are dropped).
__global__ __launch_bounds__(256) void db_class_dense_kernel(const float* __restrict__ T, const int64_t* __restrict__ cls, const int64_t* __restrict__ off,
                                                             int64_t width, int64_t M, int64_t N, int D, int C, float* __restrict__ out,
                                                             int32_t* __restrict__ status) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t m = (int64_t)blockIdx.x * 4 + wave; m < M; m += (int64_t)gridDim.x * 4) {
    const int64_t b = m / width, j = m - b * width;
    const int64_t o0 = clampi(off[b], 0, N), o1 = clampi(off[b + 1], o0, N);
    if (lane == 0 && j == 0 && o1 - o0 > width && status) atomicOr(status, MANNER_HIP_STATUS_LENGTHS);
    const float* src = nullptr;
    if (j < o1 - o0) {
      const int64_t t = cls[o0 + j];
      if (t >= 0 && t < C) src = T + (size_t)t * D;
      else if (lane == 0 && status) atomicOr(status, MANNER_HIP_STATUS_INDEX);
    }
    for (int d = lane; d < D; d += 64) out[(size_t)m * D + d] = src ? src[d] : 0.f;
  }
}

// P[b, c] = u[b] . T[c]: one wave per pair, a per-lane fma chain over d = lane + 64 j and a butterfly
__global__ __launch_bounds__(256) void db_pairs_kernel(const float* __restrict__ u, const float* __restrict__ T, int64_t pairs, int D, int C,
                                                       float* __restrict__ P) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t pair = (int64_t)blockIdx.x * 4 + wave;
  if (pair >= pairs) return;
  const int64_t b = pair / C;
  const int c = (int)(pair - b * C);
  float a = 0.f;
  for (int d = lane; d < D; d += 64) a = fmaf(u[(size_t)b * D + d], T[(size_t)c * D + d], a);
  a = wsum(a);
  if (lane == 0) P[pair] = a;
}
// out[t] = P[b, cls[t]] for the candidates t of user b: one wave per user
__global__ __launch_bounds__(64) void db_gather_scores_kernel(const float* __restrict__ P, const int64_t* __restrict__ cls, const int64_t* __restrict__ off,
                                                              int64_t N, int C, float* __restrict__ out, int32_t* __restrict__ status) {
  const int64_t b = blockIdx.x;
  const int64_t o0 = clampi(off[b], 0, N), o1 = clampi(off[b + 1], o0, N);
  for (int64_t t = o0 + threadIdx.x; t < o1; t += 64) {
    const int64_t c = cls[t];
    const bool bad = c < 0 || c >= C;
    out[t] = bad ? 0.f : P[b * C + c];
    if (bad && status) atomicOr(status, MANNER_HIP_STATUS_INDEX);
  }
}
// G[b, c] = the sum of g[t] over user b's candidates of class c, ascending t: one thread per (b, c)
__global__ __launch_bounds__(256) void db_score_bins_kernel(const float* __restrict__ g, const int64_t* __restrict__ cls, const int64_t* __restrict__ off,
                                                            int64_t pairs, int64_t N, int C, float* __restrict__ G) {
  const int64_t pair = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pair >= pairs) return;
  const int64_t b = pair / C, c = pair - b * C;
  const int64_t o0 = clampi(off[b], 0, N), o1 = clampi(off[b + 1], o0, N);
  float a = 0.f;
  for (int64_t t = o0; t < o1; ++t)
    if (cls[t] == c) a += g[t];
  G[pair] = a;
}
// out[i, d] = sum_k G(i, k) src[k, d], k ascending: one thread per (i, d).  TRANSPOSED: G(i, k) = G[k, i] (d T[c] over the users),
// else G[i, k] (d user_aware[b] over the classes)
template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void db_score_grad_kernel(const float* __restrict__ G, const float* __restrict__ src, int64_t I, int64_t K, int D,
                                                            float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= I * D) return;
  const int64_t i = e / D;
  const int d = (int)(e - i * D);
  float a = 0.f;
  for (int64_t k = 0; k < K; ++k) a = fmaf(TRANSPOSED ? G[k * I + i] : G[i * K + k], src[(size_t)k * D + d], a);
  out[e] = a;
}

// ---------------------------------------------------------------- the adversarial head, layer 2 (row_head.h)
// Over the hidden rows h [N, H]: the row's cross-entropy against class (cls - 1) mod O — the module writes y_true[i, t - 1] = 1, so class 0
// lands on the last column; `saved` [N, O] = (p - y) / (rows of the row's segment: n0 history rows, then N - n0 candidate rows).
struct DbHead {
  int64_t n0;
  __device__ __forceinline__ int column(int64_t t, int O) const { return t == 0 ? O - 1 : (int)t - 1; }
  __device__ __forceinline__ float scaled(float v, int64_t r, int64_t N) const { return v * (1.0f / (float)(r < n0 ? n0 : N - n0)); }
  __device__ __forceinline__ void keep_logit(float, size_t) const {}
};
// dpre[r, k] = (g sum_o saved[r, o] W2[o, k], ascending o) (1 - h[r, k]^2): the gradient at layer 1's pre-activation
struct DbDpre {
  const float* h;
  __device__ __forceinline__ float coef(float g, int64_t) const { return g; }
  __device__ __forceinline__ float operator()(float v, size_t at) const {
    const float hv = h[at];
    return v * (1.0f - hv * hv);
  }
};
// d b1: part[chunk][k] = the sum of dpre[r, k] over the chunk's rows, ascending; then the chunks in ascending order
__global__ __launch_bounds__(64) void db_colsum_kernel(const float* __restrict__ v, int64_t N, int H, int64_t chunk_rows, float* __restrict__ part) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= H) return;
  const int64_t r0 = (int64_t)blockIdx.y * chunk_rows, r1 = r0 + chunk_rows < N ? r0 + chunk_rows : N;
  float a = 0.f;
  for (int64_t r = r0; r < r1; ++r) a += v[(size_t)r * H + k];
  part[(size_t)blockIdx.y * H + k] = a;
}
__global__ __launch_bounds__(256) void db_colsum_reduce_kernel(const float* __restrict__ part, int H, int chunks, float* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= H) return;
  float a = 0.f;
  for (int c = 0; c < chunks; ++c) a += part[(size_t)c * H + k];
  out[k] = a;
}

// ---------------------------------------------------------------- host side
int64_t bin_chunks(int64_t M) {
  const int64_t c = (M + DB_CHUNK_ROWS - 1) / DB_CHUNK_ROWS;
  return std::max<int64_t>(1, c < DB_MAX_CHUNKS ? c : DB_MAX_CHUNKS);
}
size_t aligned(size_t bytes) { return (bytes + 255) / 256 * 256; }
bool staged(int H, int O) { return (size_t)O * H * sizeof(float) <= RH_STAGE_BYTES; }

int table_check(const char* who, int64_t N, int D, int C) {
  if (N < 0 || D < 1 || C < 1) return fail(MANNER_HIP_E_INVALID, "%s: bad shape N=%lld D=%d C=%d", who, (long long)N, D, C);
  if (N > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "%s: N=%lld unsupported (N < 2^31)", who, (long long)N);
  if (C > DB_MAX_C) return fail(MANNER_HIP_E_INVALID, "%s: C=%d unsupported (C <= %d)", who, C, DB_MAX_C);
  return MANNER_HIP_OK;
}
int row_check(const char* who, int64_t N, int D, int C) {
  int rc;
  if ((rc = table_check(who, N, D, C))) return rc;
  if (D > DB_MAX_D) return fail(MANNER_HIP_E_INVALID, "%s: D=%d unsupported (D <= %d)", who, D, DB_MAX_D);
  return MANNER_HIP_OK;
}
int dense_check(const char* who, int64_t N, int64_t B, int64_t width, int D, int C) {
  int rc;
  if ((rc = table_check(who, N, D, C))) return rc;
  if (B < 0 || width < 0 || B > 0x7fffffffll || width > 0x7fffffffll || B * width > 0x7fffffffll)
    return fail(MANNER_HIP_E_INVALID, "%s: bad shape B=%lld width=%lld (B width < 2^31)", who, (long long)B, (long long)width);
  if (B * width < N) return fail(MANNER_HIP_E_INVALID, "%s: width=%lld below the largest row count (N=%lld over B=%lld)", who, (long long)width, (long long)N, (long long)B);
  return MANNER_HIP_OK;
}
int adv_check(const char* who, int64_t N, int64_t n_hist, int D, int H, int O) {
  if (N < 0 || n_hist < 0 || n_hist > N || D < 1 || H < 1 || O < 1)
    return fail(MANNER_HIP_E_INVALID, "%s: bad shape N=%lld n_hist=%lld D=%d H=%d O=%d", who, (long long)N, (long long)n_hist, D, H, O);
  if (N > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "%s: N=%lld unsupported (N < 2^31)", who, (long long)N);
  if (O > DB_MAX_O) return fail(MANNER_HIP_E_INVALID, "%s: O=%d unsupported (O <= %d)", who, O, DB_MAX_O);
  if (H > DB_MAX_D) return fail(MANNER_HIP_E_INVALID, "%s: H=%d unsupported (H <= %d)", who, H, DB_MAX_D);
  if (D > DB_MAX_D) return fail(MANNER_HIP_E_INVALID, "%s: D=%d unsupported (D <= %d)", who, D, DB_MAX_D);
  return MANNER_HIP_OK;
}

size_t bin_part_bytes(int64_t M, int D, int C) { return aligned((size_t)bin_chunks(M) * C * (D + 1) * sizeof(float)); }
// part = the workspace of bin_part_bytes(M, D, C)
int launch_bins(bool dense, const float* x, const float* pq, const int64_t* cls, const int64_t* off, int64_t width, int64_t M, int64_t N, int D, int C,
                const float* T, float* part, float* dT, hipStream_t s) {
  const int64_t chunks = bin_chunks(M), chunk_rows = std::max<int64_t>(1, (M + chunks - 1) / chunks);
  const dim3 grid((unsigned)((D + 1 + 63) / 64), (unsigned)chunks);
  if (dense) hipLaunchKernelGGL(db_bin_kernel<true>, grid, dim3(64), 0, s, x, pq, cls, off, width, M, N, D, C, chunk_rows, part);
  else hipLaunchKernelGGL(db_bin_kernel<false>, grid, dim3(64), 0, s, x, pq, cls, off, width, M, N, D, C, chunk_rows, part);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(db_bin_reduce_kernel, dim3((unsigned)((C * D + 255) / 256)), dim3(256), 0, s, part, T, D, C, (int)chunks, dT);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

size_t orth_fwd_ws(int64_t N, int64_t B) { return aligned((size_t)(N + B) * sizeof(float)); }
size_t orth_bwd_ws(int64_t N, int D, int C) { return aligned((size_t)2 * N * sizeof(float)) + bin_part_bytes(N, D, C); }

struct AdvBwd { size_t dpre, wt, w1part, w2part, b1part, total; };
AdvBwd adv_bwd_plan(int64_t N, int D, int H, int O) {
  AdvBwd p;
  const int64_t n = std::max<int64_t>(N, 1);
  size_t at = 0;
  p.dpre = at; at += aligned((size_t)n * H * sizeof(float));
  p.wt = at; at += aligned((size_t)D * H * sizeof(float));
  p.w1part = at; at += aligned(manner_hip_wgrad_rows_f32_workspace_bytes(n, D, H));
  p.w2part = at; at += aligned((size_t)bin_chunks(n) * O * (H + 1) * sizeof(float));
  p.b1part = at; at += aligned((size_t)bin_chunks(n) * H * sizeof(float));
  p.total = at;
  return p;
}

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" {

size_t manner_hip_orth_loss_workspace_bytes(int64_t N, int64_t B) { return (N < 0 || B < 0) ? 0 : orth_fwd_ws(N, B); }
size_t manner_hip_orth_loss_backward_workspace_bytes(int64_t N, int32_t D, int32_t C) {
  return (N < 0 || D < 1 || C < 1 || C > DB_MAX_C) ? 0 : orth_bwd_ws(N, D, C);
}

int manner_hip_orth_loss(const float* rows, int64_t N, int64_t n_hist, const float* table, const int64_t* cls, const float* user_free,
                         const float* user_aware, int64_t B, int32_t D, int32_t C, float* loss, float* means, void* workspace, size_t workspace_bytes,
                         int32_t* status, manner_hip_stream_t stream) {
  int rc;
  if ((rc = row_check("orth_loss", N, D, C))) return rc;
  if (B < 0 || B > 0x7fffffffll || n_hist < 0 || n_hist > N)
    return fail(MANNER_HIP_E_INVALID, "orth_loss: bad shape B=%lld n_hist=%lld N=%lld", (long long)B, (long long)n_hist, (long long)N);
  if (!table || !loss || !workspace || (N > 0 && (!rows || !cls)) || (B > 0 && (!user_free || !user_aware)))
    return fail(MANNER_HIP_E_INVALID, "orth_loss: null pointer");
  if (workspace_bytes < orth_fwd_ws(N, B)) return fail(MANNER_HIP_E_WORKSPACE, "orth_loss: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* cosv = static_cast<float*>(workspace);
  float* ucos = cosv + N;
  if (N > 0) {
    hipLaunchKernelGGL(db_cos_fwd_kernel, dim3(rh_walk_grid(N)), dim3(256), 0, s, rows, table, cls, N, D, C, cosv, status);
    MANNER_LAUNCH_CHECK();
  }
  if (B > 0) {
    hipLaunchKernelGGL(db_cos_fwd_kernel, dim3(rh_walk_grid(B)), dim3(256), 0, s, user_free, user_aware, (const int64_t*)nullptr, B, D, C, ucos,
                       (int32_t*)nullptr);
    MANNER_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(db_segment_means_kernel<true>, dim3(1), dim3(256), 0, s, cosv, n_hist, N, ucos, B, loss, means);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_orth_loss_backward(const float* grad_loss, const float* means, const float* rows, int64_t N, int64_t n_hist, const float* table,
                                  const int64_t* cls, const float* user_free, const float* user_aware, int64_t B, int32_t D, int32_t C,
                                  float* grad_rows, float* grad_table, float* grad_user_free, float* grad_user_aware, void* workspace,
                                  size_t workspace_bytes, manner_hip_stream_t stream) {
  int rc;
  if ((rc = row_check("orth_loss_backward", N, D, C))) return rc;
  if (B < 0 || B > 0x7fffffffll || n_hist < 0 || n_hist > N)
    return fail(MANNER_HIP_E_INVALID, "orth_loss_backward: bad shape B=%lld n_hist=%lld N=%lld", (long long)B, (long long)n_hist, (long long)N);
  if (!grad_loss || !means || !table || (N > 0 && (!rows || !cls)) || (B > 0 && (!user_free || !user_aware)))
    return fail(MANNER_HIP_E_INVALID, "orth_loss_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  float* pq = nullptr;
  float* part = nullptr;
  if (grad_table) {
    if (!workspace) return fail(MANNER_HIP_E_INVALID, "orth_loss_backward: null pointer");
    if (workspace_bytes < orth_bwd_ws(N, D, C)) return fail(MANNER_HIP_E_WORKSPACE, "orth_loss_backward: workspace too small");
    pq = static_cast<float*>(workspace);
    part = reinterpret_cast<float*>(static_cast<char*>(workspace) + aligned((size_t)2 * N * sizeof(float)));
  }
  if (N > 0 && (grad_rows || grad_table)) {
    hipLaunchKernelGGL(db_cos_bwd_kernel, dim3(rh_walk_grid(N)), dim3(256), 0, s, grad_loss, means, rows, table, cls, n_hist, N, D, C, grad_rows,
                       (float*)nullptr, pq);
    MANNER_LAUNCH_CHECK();
  }
  if (grad_table && (rc = launch_bins(false, rows, pq, cls, nullptr, 1, N, N, D, C, table, part, grad_table, s))) return rc;
  if (B > 0 && (grad_user_free || grad_user_aware)) {
    hipLaunchKernelGGL(db_cos_bwd_kernel, dim3(rh_walk_grid(B)), dim3(256), 0, s, grad_loss, means, user_free, user_aware, (const int64_t*)nullptr,
                       (int64_t)0, B, D, C, grad_user_free, grad_user_aware, (float*)nullptr);
    MANNER_LAUNCH_CHECK();
  }
  return MANNER_HIP_OK;
}

size_t manner_hip_class_dense_backward_workspace_bytes(int64_t B, int64_t width, int32_t D, int32_t C) {
  return (B < 0 || width < 0 || D < 1 || C < 1 || C > DB_MAX_C) ? 0 : bin_part_bytes(B * width, D, C);
}

int manner_hip_class_dense(const float* table, const int64_t* cls, const int64_t* off, int64_t N, int64_t B, int64_t width, int32_t D, int32_t C,
                           float* out, int32_t* status, manner_hip_stream_t stream) {
  int rc;
  if ((rc = dense_check("class_dense", N, B, width, D, C))) return rc;
  const int64_t M = B * width;
  if (M == 0) return MANNER_HIP_OK;
  if (!table || !off || !out || (N > 0 && !cls)) return fail(MANNER_HIP_E_INVALID, "class_dense: null pointer");
  const int64_t g = (M + 3) / 4;
  hipLaunchKernelGGL(db_class_dense_kernel, dim3((unsigned)std::min<int64_t>(g, RH_MAX_WG)), dim3(256), 0, (hipStream_t)stream, table, cls, off, width, M, N, D,
                     C, out, status);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_class_dense_backward(const float* grad_out, const int64_t* cls, const int64_t* off, int64_t N, int64_t B, int64_t width, int32_t D,
                                    int32_t C, float* grad_table, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream) {
  int rc;
  if ((rc = dense_check("class_dense_backward", N, B, width, D, C))) return rc;
  if (!grad_table) return MANNER_HIP_OK;
  const int64_t M = B * width;
  if (!workspace || !off || (M > 0 && !grad_out) || (N > 0 && !cls)) return fail(MANNER_HIP_E_INVALID, "class_dense_backward: null pointer");
  if (workspace_bytes < bin_part_bytes(M, D, C)) return fail(MANNER_HIP_E_WORKSPACE, "class_dense_backward: workspace too small");
  return launch_bins(true, grad_out, nullptr, cls, off, std::max<int64_t>(width, 1), M, N, D, C, nullptr, static_cast<float*>(workspace), grad_table,
                     (hipStream_t)stream);
}

size_t manner_hip_class_scores_workspace_bytes(int64_t B, int32_t C) { return (B < 0 || C < 1) ? 0 : aligned((size_t)B * C * sizeof(float)); }

int manner_hip_class_scores(const float* user, const float* table, const int64_t* cls, const int64_t* off, int64_t N, int64_t B, int32_t D, int32_t C,
                            float* out, void* workspace, size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream) {
  int rc;
  if ((rc = table_check("class_scores", N, D, C))) return rc;
  if (B < 0 || B * C > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "class_scores: bad shape B=%lld (B C < 2^31)", (long long)B);
  if (B == 0 || N == 0) return MANNER_HIP_OK;
  if (!user || !table || !cls || !off || !out || !workspace) return fail(MANNER_HIP_E_INVALID, "class_scores: null pointer");
  if (workspace_bytes < manner_hip_class_scores_workspace_bytes(B, C)) return fail(MANNER_HIP_E_WORKSPACE, "class_scores: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* P = static_cast<float*>(workspace);
  hipLaunchKernelGGL(db_pairs_kernel, dim3((unsigned)((B * C + 3) / 4)), dim3(256), 0, s, user, table, B * C, D, C, P);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(db_gather_scores_kernel, dim3((unsigned)B), dim3(64), 0, s, P, cls, off, N, C, out, status);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_class_scores_backward(const float* grad_out, const float* user, const float* table, const int64_t* cls, const int64_t* off, int64_t N,
                                     int64_t B, int32_t D, int32_t C, float* grad_user, float* grad_table, void* workspace, size_t workspace_bytes,
                                     manner_hip_stream_t stream) {
  int rc;
  if ((rc = table_check("class_scores_backward", N, D, C))) return rc;
  if (B < 0 || B * C > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "class_scores_backward: bad shape B=%lld (B C < 2^31)", (long long)B);
  if (!grad_user && !grad_table) return MANNER_HIP_OK;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {                                    // a sum over nothing
    if (grad_table) MANNER_HIP_TRY(hipMemsetAsync(grad_table, 0, (size_t)C * D * sizeof(float), s));
    return MANNER_HIP_OK;
  }
  if (!user || !table || !off || !workspace || (N > 0 && (!grad_out || !cls))) return fail(MANNER_HIP_E_INVALID, "class_scores_backward: null pointer");
  if (workspace_bytes < manner_hip_class_scores_workspace_bytes(B, C)) return fail(MANNER_HIP_E_WORKSPACE, "class_scores_backward: workspace too small");
  float* G = static_cast<float*>(workspace);
  hipLaunchKernelGGL(db_score_bins_kernel, dim3((unsigned)((B * C + 255) / 256)), dim3(256), 0, s, grad_out, cls, off, B * C, N, C, G);
  MANNER_LAUNCH_CHECK();
  if (grad_user) {
    hipLaunchKernelGGL(db_score_grad_kernel<false>, dim3((unsigned)((B * D + 255) / 256)), dim3(256), 0, s, G, table, B, (int64_t)C, D, grad_user);
    MANNER_LAUNCH_CHECK();
  }
  if (grad_table) {
    hipLaunchKernelGGL(db_score_grad_kernel<true>, dim3((unsigned)(((int64_t)C * D + 255) / 256)), dim3(256), 0, s, G, user, (int64_t)C, B, D, grad_table);
    MANNER_LAUNCH_CHECK();
  }
  return MANNER_HIP_OK;
}

size_t manner_hip_adv_loss_workspace_bytes(int64_t N) { return N < 0 ? 0 : aligned((size_t)N * sizeof(float)); }
size_t manner_hip_adv_loss_backward_workspace_bytes(int64_t N, int32_t D, int32_t H, int32_t O) {
  return (N < 0 || D < 1 || H < 1 || O < 1 || D > DB_MAX_D || H > DB_MAX_D || O > DB_MAX_O) ? 0 : adv_bwd_plan(N, D, H, O).total;
}

int manner_hip_adv_loss(const float* rows, int64_t N, int64_t n_hist, const float* w1, const float* b1, const float* w2, const float* b2,
                        const int64_t* cls, int32_t D, int32_t H, int32_t O, float* loss, float* hidden, float* saved, void* workspace,
                        size_t workspace_bytes, int32_t* status, manner_hip_stream_t stream) {
  int rc;
  if ((rc = adv_check("adv_loss", N, n_hist, D, H, O))) return rc;
  if (!w1 || !b1 || !w2 || !b2 || !loss || !workspace || (N > 0 && (!rows || !cls || !hidden))) return fail(MANNER_HIP_E_INVALID, "adv_loss: null pointer");
  if (workspace_bytes < manner_hip_adv_loss_workspace_bytes(N)) return fail(MANNER_HIP_E_WORKSPACE, "adv_loss: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* rowloss = static_cast<float*>(workspace);
  if (N > 0) {
    if ((rc = wlin_f32(true, rows, D, w1, D, b1, N, D, H, hidden, H, s))) return rc;
    const DbHead head{n_hist};
    if (staged(H, O)) rc = rh_launch_walk(rh_head_fwd_kernel<0, DbHead>, true, N, H, O, s, hidden, w2, b2, cls, head, N, H, O, rowloss, saved, status);
    else rc = rh_launch_walk(rh_head_fwd_kernel<1, DbHead>, false, N, H, O, s, hidden, w2, b2, cls, head, N, H, O, rowloss, saved, status);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(db_segment_means_kernel<false>, dim3(1), dim3(256), 0, s, rowloss, n_hist, N, (const float*)nullptr, (int64_t)0, loss, (float*)nullptr);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_adv_loss_backward(const float* grad_loss, const float* rows, int64_t N, const float* w1, const float* w2, const float* hidden,
                                 const float* saved, int32_t D, int32_t H, int32_t O, float* grad_rows, float* grad_w1, float* grad_b1, float* grad_w2,
                                 float* grad_b2, void* workspace, size_t workspace_bytes, manner_hip_stream_t stream) {
  int rc;
  if ((rc = adv_check("adv_loss_backward", N, 0, D, H, O))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {                                    // sums over nothing
    if (grad_w1) MANNER_HIP_TRY(hipMemsetAsync(grad_w1, 0, (size_t)H * D * sizeof(float), s));
    if (grad_b1) MANNER_HIP_TRY(hipMemsetAsync(grad_b1, 0, (size_t)H * sizeof(float), s));
    if (grad_w2) MANNER_HIP_TRY(hipMemsetAsync(grad_w2, 0, (size_t)O * H * sizeof(float), s));
    if (grad_b2) MANNER_HIP_TRY(hipMemsetAsync(grad_b2, 0, (size_t)O * sizeof(float), s));
    return MANNER_HIP_OK;
  }
  if (!grad_loss || !rows || !w1 || !w2 || !hidden || !saved || !workspace) return fail(MANNER_HIP_E_INVALID, "adv_loss_backward: null pointer");
  const AdvBwd p = adv_bwd_plan(N, D, H, O);
  if (workspace_bytes < p.total) return fail(MANNER_HIP_E_WORKSPACE, "adv_loss_backward: workspace too small");
  char* base = static_cast<char*>(workspace);
  float* dpre = reinterpret_cast<float*>(base + p.dpre);
  const int64_t chunks = bin_chunks(N), chunk_rows = (N + chunks - 1) / chunks;
  if (grad_rows || grad_w1 || grad_b1) {
    const DbDpre last{hidden};
    if (staged(H, O)) rc = rh_launch_walk(rh_head_dx_kernel<true, DbDpre>, true, N, H, O, s, grad_loss, w2, saved, last, N, H, O, dpre);
    else rc = rh_launch_walk(rh_head_dx_kernel<false, DbDpre>, false, N, H, O, s, grad_loss, w2, saved, last, N, H, O, dpre);
    if (rc) return rc;
  }
  if (grad_rows && (rc = wlin_dx_f32(dpre, H, w1, D, N, D, H, grad_rows, reinterpret_cast<float*>(base + p.wt), s))) return rc;
  if (grad_w1 && (rc = manner_hip_wgrad_rows_f32(dpre, H, rows, D, N, D, H, grad_w1, D, base + p.w1part, p.w2part - p.w1part, stream))) return rc;
  if (grad_b1) {
    float* part = reinterpret_cast<float*>(base + p.b1part);
    hipLaunchKernelGGL(db_colsum_kernel, dim3((unsigned)((H + 63) / 64), (unsigned)chunks), dim3(64), 0, s, dpre, N, H, chunk_rows, part);
    MANNER_LAUNCH_CHECK();
    hipLaunchKernelGGL(db_colsum_reduce_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, s, part, H, (int)chunks, grad_b1);
    MANNER_LAUNCH_CHECK();
  }
  if (grad_w2 || grad_b2) {
    if ((rc = rh_head_wgrad(grad_loss, 1.0f, hidden, saved, N, H, O, reinterpret_cast<float*>(base + p.w2part), grad_w2, grad_b2, s))) return rc;
  }
  return MANNER_HIP_OK;
}

}  // extern "C"
