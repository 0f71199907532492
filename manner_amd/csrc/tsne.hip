// t-SNE for the A-Module's embedding plots (reference manner/models/a_module.py:150-173, 191-212 call MulticoreTSNE.fit_transform on the
// CPU), restated from the published method (van der Maaten's implementation: kNN affinities, gains, momentum, early exaggeration) with
// EXACT repulsive forces, f32, f64 only in final fixed-order sums:
//   knn_rows_f32      exact k nearest neighbours of every row by squared Euclidean distance, ascending by (d2, index), the row itself left out
//   tsne_affinities   per row the beta whose conditional distribution over the k neighbours has the asked perplexity, and that distribution
//   tsne_repulsion    per row sum_j q^2 (y_i - y_j) and sum_j q over ALL j, q = 1 / (1 + |y_i - y_j|^2): the N-body loop, the hot kernel
//   tsne_step         Z, the attraction over a row's outgoing and incoming edges, dY, gains, u, Y and the centring
//   tsne_kl           sum P log(P / Q) over the non-zero entries of the symmetrised P
// No floating-point atomic, no grid-wide barrier, no counter: every sum has a fixed order and every grid comes from the shape alone, so
// two runs give the same bits.  Every loop is bounded by N (and an edge's index is checked against N before it is followed).
#include <float.h>
#include <math.h>

#include "common.h"

namespace manner {
namespace {

// ---------------------------------------------------------------- neighbours
// A workgroup of 8 waves owns KNN_TILE_Q = 32 query rows, four per wave, and walks tiles of KNN_TILE_C = 64 candidate rows, one per lane;
// both are staged in LDS KNN_DC features at a time (the candidate rows KNN_DC + 1 apart: lane l reads bank (l + d) % 32).  A distance is
// one fmaf chain of squared differences over the features in ascending order — not the Gram form, which cancels where neighbours are
// closest.  Each query keeps its best list in registers, position p = slot * 64 + lane, sorted by (d2, index); a tile's lanes that beat
// the k-th entry are balloted and inserted one by one in ascending candidate order (a shift by one lane).  Nothing [N, N] is written.
constexpr int KNN_TILE_Q = 32, KNN_TILE_C = 64, KNN_DC = 128, KNN_LDC = KNN_DC + 1, KNN_QPW = 4, KNN_THREADS = 512, KNN_SLOTS = 4;
constexpr int KNN_MAX_K = 255, KNN_MAX_D = 1024;
constexpr int64_t TSNE_MAX_N = 1 << 20;

__device__ __forceinline__ bool knn_before(float d, int i, float td, int ti) { return d < td || (d == td && i < ti); }

// (dv, ci) into the sorted list: an entry before it stays, the first entry not before it gives way to it, every later one takes its
// predecessor.  Slots in descending order, so that slot s - 1 is still the old one when lane 0 of slot s reads its last lane.
__device__ __forceinline__ void knn_insert(float (&ld)[KNN_SLOTS], int (&li)[KNN_SLOTS], float dv, int ci, int lane) {
#pragma unroll
  for (int s = KNN_SLOTS - 1; s >= 0; --s) {
    float pd = __shfl_up(ld[s], 1, 64);
    int pi = __shfl_up(li[s], 1, 64);
    if (s > 0) {
      const float cd = __shfl(ld[s - 1], 63, 64);
      const int cx = __shfl(li[s - 1], 63, 64);
      if (lane == 0) { pd = cd; pi = cx; }
    }
    const bool first = s == 0 && lane == 0;
    const bool keep = knn_before(ld[s], li[s], dv, ci);
    const bool prev_keep = first || knn_before(pd, pi, dv, ci);
    if (!keep) {
      ld[s] = prev_keep ? dv : pd;
      li[s] = prev_keep ? ci : pi;
    }
  }
}

// the entry at position k - 1 (slot ks, lane kl): what a candidate has to beat
__device__ __forceinline__ void knn_threshold(const float (&ld)[KNN_SLOTS], const int (&li)[KNN_SLOTS], int ks, int kl, float& td, int& ti) {
  float d = ld[0];
  int i = li[0];
#pragma unroll
  for (int s = 1; s < KNN_SLOTS; ++s)
    if (ks == s) { d = ld[s]; i = li[s]; }
  td = __shfl(d, kl, 64);
  ti = __shfl(i, kl, 64);
}

__global__ __launch_bounds__(KNN_THREADS) void ts_knn_kernel(const float* __restrict__ X, int N, int D, int k, int32_t* __restrict__ idx,
                                                          float* __restrict__ d2) {
  __shared__ __attribute__((aligned(16))) float qs[KNN_TILE_Q * KNN_DC];
  __shared__ float cs[KNN_TILE_C * KNN_LDC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * KNN_TILE_Q;
  const int ks = (k - 1) >> 6, kl = (k - 1) & 63;
  float ld[KNN_QPW][KNN_SLOTS];
  int li[KNN_QPW][KNN_SLOTS];
#pragma unroll
  for (int qi = 0; qi < KNN_QPW; ++qi)
#pragma unroll
    for (int s = 0; s < KNN_SLOTS; ++s) { ld[qi][s] = INFINITY; li[qi][s] = 0x7fffffff; }

  for (int c0 = 0; c0 < N; c0 += KNN_TILE_C) {
    float acc[KNN_QPW] = {0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < D; d0 += KNN_DC) {
      const int dc = min(KNN_DC, D - d0);
      __syncthreads();                                            // the previous chunk has been read
      for (int e = tid; e < KNN_TILE_Q * KNN_DC; e += KNN_THREADS) {
        const int r = e / KNN_DC, d = e % KNN_DC, q = q0 + r;
        qs[e] = (q < N && d < dc) ? X[(size_t)q * D + d0 + d] : 0.f;
      }
      for (int e = tid; e < KNN_TILE_C * KNN_DC; e += KNN_THREADS) {
        const int r = e / KNN_DC, d = e % KNN_DC, c = c0 + r;
        cs[r * KNN_LDC + d] = (c < N && d < dc) ? X[(size_t)c * D + d0 + d] : 0.f;
      }
      __syncthreads();
      const float* cr = cs + lane * KNN_LDC;
      const float* qr = qs + wave * KNN_QPW * KNN_DC;
      const int dc4 = (dc + 3) & ~3;                              // the padding is zeros on both sides: fmaf(0, 0, acc) = acc
      for (int d = 0; d < dc4; d += 4) {
        const float c0v = cr[d], c1v = cr[d + 1], c2v = cr[d + 2], c3v = cr[d + 3];
#pragma unroll
        for (int qi = 0; qi < KNN_QPW; ++qi) {
          const float4 qv = *reinterpret_cast<const float4*>(qr + qi * KNN_DC + d);
          float df = qv.x - c0v;
          acc[qi] = fmaf(df, df, acc[qi]);
          df = qv.y - c1v;
          acc[qi] = fmaf(df, df, acc[qi]);
          df = qv.z - c2v;
          acc[qi] = fmaf(df, df, acc[qi]);
          df = qv.w - c3v;
          acc[qi] = fmaf(df, df, acc[qi]);
        }
      }
    }
    const int c = c0 + lane;
#pragma unroll
    for (int qi = 0; qi < KNN_QPW; ++qi) {
      const int q = q0 + wave * KNN_QPW + qi;                     // the same in every lane
      if (q >= N) continue;
      float td;
      int ti;
      knn_threshold(ld[qi], li[qi], ks, kl, td, ti);
      unsigned long long mask = __ballot(c < N && c != q && knn_before(acc[qi], c, td, ti));
      while (mask) {
        const int b = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const float dv = __shfl(acc[qi], b, 64);
        knn_threshold(ld[qi], li[qi], ks, kl, td, ti);            // it tightens with every insertion
        if (knn_before(dv, c0 + b, td, ti)) knn_insert(ld[qi], li[qi], dv, c0 + b, lane);
      }
    }
  }
#pragma unroll
  for (int qi = 0; qi < KNN_QPW; ++qi) {
    const int q = q0 + wave * KNN_QPW + qi;
    if (q >= N) continue;
#pragma unroll
    for (int s = 0; s < KNN_SLOTS; ++s) {
      const int p = s * 64 + lane;
      if (p < k) {
        const bool filled = li[qi][s] != 0x7fffffff;               // a list stays short only where distances are NaN
        idx[(size_t)q * k + p] = filled ? li[qi][s] : -1;
        d2[(size_t)q * k + p] = ld[qi][s];
      }
    }
  }
}

// ---------------------------------------------------------------- conditional affinities
__device__ __forceinline__ float wmin(float v) { return -wmax(-v); }

// One wave per row, neighbour m = slot * 64 + lane.  The search of the published implementation (start at beta = 1, double or halve while
// the far bound is open, bisect afterwards, at most 200 trips, |H - log perplexity| < 1e-5) on distances taken relative to the row's
// smallest: p and H do not change under that shift, the exponentials then never all underflow, and a row of equal (or zero) distances
// is uniform at every beta.  beta stays finite: doubling saturates at FLT_MAX.
__global__ __launch_bounds__(256) void ts_aff_kernel(const float* __restrict__ d2, int64_t N, int k, float log_perp, float* __restrict__ p,
                                                  float* __restrict__ beta_out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  float dv[KNN_SLOTS], pv[KNN_SLOTS];
  float dmin = INFINITY;
#pragma unroll
  for (int s = 0; s < KNN_SLOTS; ++s) {
    const int m = s * 64 + lane;
    dv[s] = m < k ? d2[row * k + m] : INFINITY;
    dmin = fminf(dmin, dv[s]);
    pv[s] = 0.f;
  }
  dmin = wmin(dmin);
#pragma unroll
  for (int s = 0; s < KNN_SLOTS; ++s) dv[s] = s * 64 + lane < k ? dv[s] - dmin : 0.f;
  float beta = 1.f, used = 1.f, lo = 0.f, hi = 0.f, s0 = 1.f;
  bool has_lo = false, has_hi = false;
  for (int trip = 0; trip < 200; ++trip) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int s = 0; s < KNN_SLOTS; ++s)
      if (s * 64 + lane < k) {
        pv[s] = expf(-beta * dv[s]);
        a0 += pv[s];
        a1 = fmaf(dv[s], pv[s], a1);
      }
    s0 = wsum(a0);
    const float s1 = wsum(a1);
    used = beta;
    const float diff = (beta * s1 / s0 + logf(s0)) - log_perp;    // the same in every lane
    if (fabsf(diff) < 1e-5f) break;
    if (diff > 0.f) {
      lo = beta;
      has_lo = true;
      beta = has_hi ? 0.5f * beta + 0.5f * hi : fminf(beta * 2.f, FLT_MAX);
    } else {
      hi = beta;
      has_hi = true;
      beta = has_lo ? 0.5f * beta + 0.5f * lo : beta * 0.5f;
    }
  }
#pragma unroll
  for (int s = 0; s < KNN_SLOTS; ++s) {
    const int m = s * 64 + lane;
    if (m < k) p[row * k + m] = pv[s] / s0;
  }
  if (lane == 0) beta_out[row] = used;
}

// ---------------------------------------------------------------- repulsion
// A workgroup of two waves owns TSNE_TILE_I = 512 rows i, four per thread in registers, and walks its share of the tiles of TSNE_TILE_J =
// 512 rows j staged in LDS as float2; every lane reads the same j (a broadcast).  The self pair is not branched on: its q is exactly 1 and
// its force exactly 0, so a row's sum of q carries one 1 too many and Z subtracts N.  gridDim.y = the j split (tsne_split(N)): slice s walks
// the tiles [s jt / S, (s + 1) jt / S) and writes its own partial part[s][i] = (sum q^2 dx, sum q^2 dy, sum q, 0); the consumer adds a row's
// partials in ascending s.  zpart[s nb + b]: the workgroup's sum of q over its valid rows, f64, in a fixed tree.
constexpr int TSNE_TILE_I = 512, TSNE_TILE_J = 512, TSNE_THREADS = 128, TSNE_R = 4, TSNE_TARGET_WG = 1024, TSNE_CHUNK = 32;

int64_t tsne_blocks(int64_t N) { return (N + TSNE_TILE_I - 1) / TSNE_TILE_I; }
int tsne_split(int64_t N) {
  if (N <= 0) return 1;
  const int64_t nb = tsne_blocks(N), jt = (N + TSNE_TILE_J - 1) / TSNE_TILE_J;
  const int64_t s = std::min<int64_t>((TSNE_TARGET_WG + nb - 1) / nb, jt);
  return (int)std::max<int64_t>(s, 1);
}

__global__ __launch_bounds__(TSNE_THREADS) void ts_rep_kernel(const float2* __restrict__ Y, int N, int S, int jt, float4* __restrict__ part,
                                                           double* __restrict__ zpart) {
  __shared__ float2 ys[TSNE_TILE_J];
  __shared__ double red[TSNE_THREADS / 64];
  const int tid = threadIdx.x, b = blockIdx.x, s = blockIdx.y;
  const int i0 = b * TSNE_TILE_I;
  float2 yi[TSNE_R];
  float sx[TSNE_R], sy[TSNE_R], sq[TSNE_R];
#pragma unroll
  for (int r = 0; r < TSNE_R; ++r) {
    const int i = i0 + r * TSNE_THREADS + tid;
    yi[r] = i < N ? Y[i] : float2{0.f, 0.f};
    sx[r] = sy[r] = sq[r] = 0.f;
  }
  const int t0 = (int)((int64_t)s * jt / S), t1 = (int)((int64_t)(s + 1) * jt / S);
  for (int t = t0; t < t1; ++t) {
    const int j0 = t * TSNE_TILE_J;
    const int jn = min(TSNE_TILE_J, N - j0);
    __syncthreads();
    for (int e = tid; e < jn; e += TSNE_THREADS) ys[e] = Y[j0 + e];
    __syncthreads();
    // three levels of sums — TSNE_CHUNK pairs, the tile, the slice — so that a row's rounding error grows with the square root of the
    // chunk, not with N: one running sum over 512 terms alone stands 16 ulp from float64
    float tx[TSNE_R], ty[TSNE_R], tq[TSNE_R];
#pragma unroll
    for (int r = 0; r < TSNE_R; ++r) tx[r] = ty[r] = tq[r] = 0.f;
    for (int jc = 0; jc < jn; jc += TSNE_CHUNK) {
      const int je = min(jc + TSNE_CHUNK, jn);
      float cx[TSNE_R], cy[TSNE_R], cq[TSNE_R];
#pragma unroll
      for (int r = 0; r < TSNE_R; ++r) cx[r] = cy[r] = cq[r] = 0.f;
#pragma unroll 4
      for (int jj = jc; jj < je; ++jj) {
        const float2 yj = ys[jj];
#pragma unroll
        for (int r = 0; r < TSNE_R; ++r) {
          const float dx = yi[r].x - yj.x, dy = yi[r].y - yj.y;
          const float q = __builtin_amdgcn_rcpf(fmaf(dx, dx, fmaf(dy, dy, 1.f)));
          const float q2 = q * q;
          cx[r] = fmaf(q2, dx, cx[r]);
          cy[r] = fmaf(q2, dy, cy[r]);
          cq[r] += q;
        }
      }
#pragma unroll
      for (int r = 0; r < TSNE_R; ++r) { tx[r] += cx[r]; ty[r] += cy[r]; tq[r] += cq[r]; }
    }
#pragma unroll
    for (int r = 0; r < TSNE_R; ++r) { sx[r] += tx[r]; sy[r] += ty[r]; sq[r] += tq[r]; }
  }
  double z = 0.0;
#pragma unroll
  for (int r = 0; r < TSNE_R; ++r) {
    const int i = i0 + r * TSNE_THREADS + tid;
    if (i < N) {
      part[(size_t)s * N + i] = float4{sx[r], sy[r], sq[r], 0.f};
      z += (double)sq[r];
    }
  }
  z = wsum(z);
  if ((tid & 63) == 0) red[tid >> 6] = z;
  __syncthreads();
  if (tid == 0) zpart[(size_t)s * gridDim.x + b] = red[0] + red[1];
}

// all 256 threads: the sum of v[0 .. n) in f64 — thread t adds the entries t, t + 256, ... in ascending order, the 256 sums meet in a
// fixed tree; every thread returns it
__device__ __forceinline__ double block_sum256(const double* __restrict__ v, int n, int stride, double* sm) {
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += v[(size_t)i * stride];
  sm[threadIdx.x] = a;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();
  return r;
}

// ---------------------------------------------------------------- one iteration
// A workgroup of four waves owns STEP_ROWS = 64 rows, a wave 16 of them one after the other, the row's edges spread over the lanes: its k
// outgoing edges (i -> out_idx[i][m], p[i][m]) and its incoming ones in_src[in_off[i] .. in_off[i + 1]) — a ragged list, thousands for a
// hub, so a loop.  Edge (i -> j, p) adds p / (2 N) to P_ij and to P_ji.  Z = (sum of zpart) - N, summed by every workgroup in the same
// order.  Y is read from `y` and written to `y_out` (other rows' old coordinates are gathered while new ones are written), u and gains
// in place; ypart[b] = the workgroup's column sums of the new rows, f64, for the centring launch.
constexpr int STEP_ROWS = 64, STEP_RPW = 16;

__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }

__device__ __forceinline__ void attract(const float2* __restrict__ Y, int N, float2 yi, int j, float p, float& ax, float& ay) {
  if ((unsigned)j >= (unsigned)N) return;
  const float2 yj = Y[j];
  const float dx = yi.x - yj.x, dy = yi.y - yj.y;
  const float w = p / fmaf(dx, dx, fmaf(dy, dy, 1.f));
  ax = fmaf(w, dx, ax);
  ay = fmaf(w, dy, ay);
}

__global__ __launch_bounds__(256) void ts_step_kernel(const float2* __restrict__ Y, const float4* __restrict__ part, const double* __restrict__ zpart,
                                                   int nz, int S, const int32_t* __restrict__ out_idx, const float* __restrict__ out_p, int k,
                                                   const int64_t* __restrict__ in_off, const int32_t* __restrict__ in_src,
                                                   const float* __restrict__ in_p, int64_t E, int N, float exaggeration, float momentum, float lr,
                                                   float2* __restrict__ u, float2* __restrict__ gains, float2* __restrict__ y_out,
                                                   double* __restrict__ ypart) {
  __shared__ double sm[256];
  __shared__ double wx[4], wy[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double Z = block_sum256(zpart, nz, 1, sm) - (double)N;
  const float inv_z = Z > 0.0 ? (float)(1.0 / Z) : 0.f;
  const float scale = (float)((double)exaggeration / (2.0 * (double)N));
  double cx = 0.0, cy = 0.0;
  for (int rr = 0; rr < STEP_RPW; ++rr) {
    const int i = blockIdx.x * STEP_ROWS + wave * STEP_RPW + rr;
    if (i >= N) break;
    const float2 yi = Y[i];
    float ax = 0.f, ay = 0.f;
    for (int m = lane; m < k; m += 64) attract(Y, N, yi, out_idx[(size_t)i * k + m], out_p[(size_t)i * k + m], ax, ay);
    const int64_t e0 = clampi(in_off[i], 0, E), e1 = clampi(in_off[i + 1], e0, E);
    for (int64_t e = e0 + lane; e < e1; e += 64) attract(Y, N, yi, in_src[e], in_p[e], ax, ay);
    ax = wsum(ax);
    ay = wsum(ay);
    float rx = 0.f, ry = 0.f;
    for (int s = 0; s < S; ++s) {
      const float4 v = part[(size_t)s * N + i];
      rx += v.x;
      ry += v.y;
    }
    const float gx = scale * ax - inv_z * rx, gy = scale * ay - inv_z * ry;
    float2 uu = u[i], g = gains[i];
    g.x = fmaxf(sgn(gx) != sgn(uu.x) ? g.x + 0.2f : g.x * 0.8f, 0.01f);
    g.y = fmaxf(sgn(gy) != sgn(uu.y) ? g.y + 0.2f : g.y * 0.8f, 0.01f);
    uu.x = momentum * uu.x - lr * g.x * gx;
    uu.y = momentum * uu.y - lr * g.y * gy;
    const float2 yn{yi.x + uu.x, yi.y + uu.y};
    if (lane == 0) {
      u[i] = uu;
      gains[i] = g;
      y_out[i] = yn;
    }
    cx += (double)yn.x;
    cy += (double)yn.y;
  }
  if (lane == 0) { wx[wave] = cx; wy[wave] = cy; }
  __syncthreads();
  if (threadIdx.x == 0) {
    ypart[2 * (size_t)blockIdx.x] = ((wx[0] + wx[1]) + wx[2]) + wx[3];
    ypart[2 * (size_t)blockIdx.x + 1] = ((wy[0] + wy[1]) + wy[2]) + wy[3];
  }
}

// Y -= its column means: every workgroup sums the nbs partial column sums in the same order, then centres its 1024 rows
__global__ __launch_bounds__(256) void ts_centre_kernel(float2* __restrict__ Y, int N, const double* __restrict__ ypart, int nbs) {
  __shared__ double sm[256];
  const double mx = block_sum256(ypart, nbs, 2, sm) / (double)N;
  const double my = block_sum256(ypart + 1, nbs, 2, sm) / (double)N;
  const float fx = (float)mx, fy = (float)my;
  for (int r = 0; r < 4; ++r) {
    const int i = blockIdx.x * 1024 + r * 256 + threadIdx.x;
    if (i < N) {
      float2 v = Y[i];
      v.x -= fx;
      v.y -= fy;
      Y[i] = v;
    }
  }
}

// ---------------------------------------------------------------- KL
// Over the outgoing edges alone: P_ij = (p_j|i + p_i|j) / (2 N), the second term found by looking for i among j's k neighbours.  A mutual
// pair is met from both ends, once each; a one-way edge stands for the ordered pairs (i, j) and (j, i) and counts twice.
__global__ __launch_bounds__(256) void ts_kl_kernel(const float2* __restrict__ Y, const double* __restrict__ zpart, int nz,
                                                 const int32_t* __restrict__ out_idx, const float* __restrict__ out_p, int k, int N,
                                                 double* __restrict__ klpart) {
  __shared__ double sm[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double Z = block_sum256(zpart, nz, 1, sm) - (double)N;
  const float zf = (float)Z, inv2n = (float)(1.0 / (2.0 * (double)N));
  double acc = 0.0;
  for (int rr = 0; rr < STEP_RPW; ++rr) {
    const int i = blockIdx.x * STEP_ROWS + wave * STEP_RPW + rr;
    if (i >= N) break;
    const float2 yi = Y[i];
    for (int m = lane; m < k; m += 64) {
      const int j = out_idx[(size_t)i * k + m];
      if ((unsigned)j >= (unsigned)N || j == i) continue;
      float back = 0.f;
      bool mutual = false;
      for (int t = 0; t < k; ++t)
        if (out_idx[(size_t)j * k + t] == i) { back = out_p[(size_t)j * k + t]; mutual = true; }
      const float P = (out_p[(size_t)i * k + m] + back) * inv2n;
      if (P > 0.f) {
        const float2 yj = Y[j];
        const float dx = yi.x - yj.x, dy = yi.y - yj.y;
        const float term = P * logf(P * (zf * fmaf(dx, dx, fmaf(dy, dy, 1.f))));
        acc += (double)(mutual ? term : 2.f * term);
      }
    }
  }
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) klpart[blockIdx.x] = sm[0];
}

__global__ __launch_bounds__(256) void ts_sum_kernel(const double* __restrict__ v, int n, double* __restrict__ out) {
  __shared__ double sm[256];
  const double r = block_sum256(v, n, 1, sm);
  if (threadIdx.x == 0) out[0] = r;
}

// rows_are_points: the k entries of a row name other rows of the same N
int shape_check(const char* who, int64_t N, int k, bool rows_are_points = true) {
  if (k < 1 || k > KNN_MAX_K) return fail(MANNER_HIP_E_INVALID, "%s: k=%d unsupported (1 <= k <= %d)", who, k, KNN_MAX_K);
  if (N < 0 || N > TSNE_MAX_N) return fail(MANNER_HIP_E_INVALID, "%s: N=%lld outside [0, 2^20]", who, (long long)N);
  if (rows_are_points && N > 0 && N - 1 < k) return fail(MANNER_HIP_E_INVALID, "%s: N=%lld rows have fewer than k=%d other rows", who, (long long)N, k);
  return MANNER_HIP_OK;
}
int split_check(const char* who, int64_t N, int split) {
  if (split != tsne_split(N)) return fail(MANNER_HIP_E_INVALID, "%s: split=%d is not the split of N=%lld (%d)", who, split, (long long)N, tsne_split(N));
  return MANNER_HIP_OK;
}
unsigned step_blocks(int64_t N) { return (unsigned)((N + STEP_ROWS - 1) / STEP_ROWS); }

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" {

int manner_hip_knn_rows_f32(const float* x, int64_t N, int32_t D, int32_t k, int32_t* idx, float* d2, manner_hip_stream_t stream) {
  if (D < 1 || D > KNN_MAX_D) return fail(MANNER_HIP_E_INVALID, "knn_rows_f32: D=%d unsupported (1 <= D <= %d)", (int)D, KNN_MAX_D);
  int rc;
  if ((rc = shape_check("knn_rows_f32", N, k))) return rc;
  if (N == 0) return MANNER_HIP_OK;
  if (!x || !idx || !d2) return fail(MANNER_HIP_E_INVALID, "knn_rows_f32: null pointer");
  hipLaunchKernelGGL(ts_knn_kernel, dim3((unsigned)((N + KNN_TILE_Q - 1) / KNN_TILE_Q)), dim3(KNN_THREADS), 0, (hipStream_t)stream, x, (int)N, (int)D,
                     (int)k, idx, d2);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_tsne_affinities(const float* d2, int64_t N, int32_t k, float perplexity, float* p, float* beta, manner_hip_stream_t stream) {
  int rc;
  if ((rc = shape_check("tsne_affinities", N, k, false))) return rc;      // any [N, k] block of distances: its rows are searched one by one
  if (!(perplexity > 0.f) || !(perplexity < INFINITY))
    return fail(MANNER_HIP_E_INVALID, "tsne_affinities: perplexity=%g is not a positive number", (double)perplexity);
  if (N == 0) return MANNER_HIP_OK;
  if (!d2 || !p || !beta) return fail(MANNER_HIP_E_INVALID, "tsne_affinities: null pointer");
  hipLaunchKernelGGL(ts_aff_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d2, N, (int)k, logf(perplexity), p, beta);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_tsne_repulsion(const float* y, int64_t N, int32_t split, float* part, double* zpart, manner_hip_stream_t stream) {
  if (N < 0 || N > TSNE_MAX_N) return fail(MANNER_HIP_E_INVALID, "tsne_repulsion: N=%lld outside [0, 2^20]", (long long)N);
  int rc;
  if ((rc = split_check("tsne_repulsion", N, split))) return rc;
  if (N == 0) return MANNER_HIP_OK;
  if (!y || !part || !zpart) return fail(MANNER_HIP_E_INVALID, "tsne_repulsion: null pointer");
  if ((reinterpret_cast<uintptr_t>(y) & 7u) || (reinterpret_cast<uintptr_t>(part) & 15u) || (reinterpret_cast<uintptr_t>(zpart) & 7u))
    return fail(MANNER_HIP_E_INVALID, "tsne_repulsion: y / part / zpart not aligned to 8 / 16 / 8 bytes");
  const int64_t jt = (N + TSNE_TILE_J - 1) / TSNE_TILE_J;
  hipLaunchKernelGGL(ts_rep_kernel, dim3((unsigned)tsne_blocks(N), (unsigned)split), dim3(TSNE_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const float2*>(y), (int)N, (int)split, (int)jt, reinterpret_cast<float4*>(part), zpart);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_tsne_step(const float* y, const float* part, const double* zpart, int32_t split, const int32_t* out_idx, const float* out_p, int32_t k,
                         const int64_t* in_off, const int32_t* in_src, const float* in_p, int64_t n_in, int64_t N, float exaggeration,
                         float momentum, float learning_rate, float* u, float* gains, float* y_out, double* ypart, manner_hip_stream_t stream) {
  int rc;
  if ((rc = shape_check("tsne_step", N, k))) return rc;
  if ((rc = split_check("tsne_step", N, split))) return rc;
  if (n_in < 0 || n_in > N * (int64_t)k) return fail(MANNER_HIP_E_INVALID, "tsne_step: n_in=%lld outside [0, N k]", (long long)n_in);
  if (N == 0) return MANNER_HIP_OK;
  if (!y || !part || !zpart || !out_idx || !out_p || !in_off || !u || !gains || !y_out || !ypart || (n_in > 0 && (!in_src || !in_p)))
    return fail(MANNER_HIP_E_INVALID, "tsne_step: null pointer");
  if (y == y_out) return fail(MANNER_HIP_E_INVALID, "tsne_step: y_out must not be y (other rows' old coordinates are read while new ones are written)");
  if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(gains) | reinterpret_cast<uintptr_t>(y_out) |
        reinterpret_cast<uintptr_t>(zpart) | reinterpret_cast<uintptr_t>(ypart) | reinterpret_cast<uintptr_t>(in_off)) & 7u) ||
      (reinterpret_cast<uintptr_t>(part) & 15u))
    return fail(MANNER_HIP_E_INVALID, "tsne_step: a buffer is not aligned to its element");
  hipStream_t s = (hipStream_t)stream;
  const int nz = (int)(split * tsne_blocks(N));
  const unsigned nbs = step_blocks(N);
  hipLaunchKernelGGL(ts_step_kernel, dim3(nbs), dim3(256), 0, s, reinterpret_cast<const float2*>(y), reinterpret_cast<const float4*>(part), zpart, nz,
                     (int)split, out_idx, out_p, (int)k, in_off, in_src, in_p, n_in, (int)N, exaggeration, momentum, learning_rate,
                     reinterpret_cast<float2*>(u), reinterpret_cast<float2*>(gains), reinterpret_cast<float2*>(y_out), ypart);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_centre_kernel, dim3((unsigned)((N + 1023) / 1024)), dim3(256), 0, s, reinterpret_cast<float2*>(y_out), (int)N, ypart, (int)nbs);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_tsne_kl(const float* y, const double* zpart, int32_t split, const int32_t* out_idx, const float* out_p, int32_t k, int64_t N,
                       double* klpart, double* kl, manner_hip_stream_t stream) {
  int rc;
  if ((rc = shape_check("tsne_kl", N, k))) return rc;
  if ((rc = split_check("tsne_kl", N, split))) return rc;
  if (N == 0) return MANNER_HIP_OK;
  if (!y || !zpart || !out_idx || !out_p || !klpart || !kl) return fail(MANNER_HIP_E_INVALID, "tsne_kl: null pointer");
  if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(zpart) | reinterpret_cast<uintptr_t>(klpart) | reinterpret_cast<uintptr_t>(kl)) & 7u))
    return fail(MANNER_HIP_E_INVALID, "tsne_kl: a buffer is not aligned to its element");
  hipStream_t s = (hipStream_t)stream;
  const unsigned nbs = step_blocks(N);
  hipLaunchKernelGGL(ts_kl_kernel, dim3(nbs), dim3(256), 0, s, reinterpret_cast<const float2*>(y), zpart, (int)(split * tsne_blocks(N)), out_idx, out_p,
                     (int)k, (int)N, klpart);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_sum_kernel, dim3(1), dim3(256), 0, s, klpart, (int)nbs, kl);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // extern "C"
