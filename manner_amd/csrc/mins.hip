// The MINS baseline's operators (reference manner/models/components/user_encoder.py:181-243), f32, forward and backward.
//
// Channel GRU: a one-layer GRU over R = B C independent sequences (row r = b C + c reads the channel c of user b: the columns
// [c I, (c + 1) I) of x[b, t, :]) that all share one set of weights, every row returning its state after its own len[b] steps.
//   gi = x W_ih^T + b_ih for all (b, t, c) rows in one launch (rows_f32.hip's projection, the channel in the row address), then the
//   WHOLE RECURRENCE IN ONE LAUNCH: at H <= 128 the W_hh row of a (gate, unit) fits the registers of one thread, so a workgroup of
//   3 x 128 threads — thread = (gate g, unit j), row j of W_g in 128 registers, zero past H — owns a tile of CG_ROWS rows for all S
//   steps.  Per step: gh = h W_hh^T + b_hh into LDS (the tile's h rows are read from LDS as broadcasts), a workgroup barrier, the gates
//     r = sigma(gi_r + gh_r), z = sigma(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h
//   for the rows with t < len (the others keep h BY SELECTION: a padded slot may hold anything), a barrier.  Nothing is exchanged
//   between workgroups: no cooperative launch, no grid barrier, no counter.  The loop runs to the tile's largest length.
// Backward: one launch walking t = S - 1 .. 0; thread (g, k) holds COLUMN k of W_g.  Each step rebuilds the tile's gate gradients
// from dh_t and the saved gates, writes that step's d gi and d gh rows, forms the three products sum_j dgh_g[., j] W_g[j, k] and adds
// them through LDS in the order r, z, n: dh_{t-1} = dh_t z + that sum.  The saved and gradient rows are stacked in (b, t, c) order,
// so manner_hip_linear_backward over them gives the shared weights' gradients as one fixed-order row sum and grad_x as [B, S, C I].
//
// Axis-0 attention at head dims 65 .. 128: the layouts, statistics and arithmetic of caum.hip's a0any kernels (q scaled first, online
// softmax over the keys in ascending order) with the LANES ALONG THE HEAD DIM: a wave owns one query row (backward-kv: one key row)
// of a (slot, head) pair, each lane two of the up to 128 components, a score is a wave butterfly sum, the other side's rows are
// staged in LDS in tiles of AW_KT.  No floating-point atomics anywhere: the same inputs give the same bits.
#include <math.h>

#include <algorithm>

#include "train_common.h"

namespace manner {
namespace {

constexpr int CG_MAX_S = 256, CG_MAX_I = 1024;
constexpr int CG_HP = 128;               // register width of the recurrence: H <= CG_HP
constexpr int CG_BLOCK = 3 * CG_HP;      // thread = (gate, unit)
constexpr int CG_ROWS = 8;               // sequences per workgroup of the recurrence kernels
static_assert(CG_HP % 4 == 0, "the h rows are read as float4");

// the tile's rows: steps taken (the length clamped to [0, S]) and the stacked row (b S + 0) C + c of step 0 (step t: + t C)
struct Tile {
  int steps[CG_ROWS];
  int64_t row0[CG_ROWS];
  int64_t b[CG_ROWS];
  int c[CG_ROWS];
};
__device__ __forceinline__ void tile_rows(Tile& tl, const int64_t* __restrict__ len, int64_t r0, int nr, int S, int C, int32_t* status) {
  if (threadIdx.x < CG_ROWS) {
    const int rr = threadIdx.x;
    int steps = 0;
    int64_t bb = 0;
    int c = 0;
    if (rr < nr) {
      bb = (r0 + rr) / C;
      c = (int)((r0 + rr) - bb * C);
      const int64_t l = len[bb];
      if ((l < 1 || l > S) && status) atomicOr(status, MANNER_HIP_STATUS_LENGTHS);
      steps = (int)min(max(l, (int64_t)0), (int64_t)S);
    }
    tl.steps[rr] = steps;
    tl.b[rr] = bb;
    tl.c[rr] = c;
    tl.row0[rr] = bb * S * C + c;
  }
}
__device__ __forceinline__ int tile_steps(const Tile& tl) {
  int m = 0;
#pragma unroll
  for (int rr = 0; rr < CG_ROWS; ++rr) m = max(m, tl.steps[rr]);
  return m;
}

// ---------------------------------------------------------------- the recurrence, forward
// grid (ceil(R / CG_ROWS)), R = B C.  gi [B S C, 3H] in (b, t, c) order.  Training: hp [B S C, H] receives the state every row enters
// step t with (all S steps: the weight gradient reads every row), gates [B S C, 4, H] r, z, n, W_hn h + b_hn of the steps taken.
template <bool TRAIN>
__global__ __launch_bounds__(CG_BLOCK) void cg_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ W, const float* __restrict__ bh,
                                                     const int64_t* __restrict__ len, int64_t R, int S, int C, int H, float* __restrict__ out,
                                                     int64_t ldo, float* __restrict__ hp, float* __restrict__ gates, int32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) float hs[CG_ROWS][CG_HP];
  __shared__ float gh[3][CG_ROWS][CG_HP];
  __shared__ Tile tl;
  const int g = threadIdx.x / CG_HP, j = threadIdx.x - g * CG_HP;
  const int64_t r0 = (int64_t)blockIdx.x * CG_ROWS;
  const int nr = (int)min((int64_t)CG_ROWS, R - r0);
  tile_rows(tl, len, r0, nr, S, C, status);
  float w[CG_HP];
  {
    const float* wr = W + (size_t)(g * H + (j < H ? j : 0)) * H;
#pragma unroll
    for (int k = 0; k < CG_HP; ++k) w[k] = (j < H && k < H) ? wr[k] : 0.f;
  }
  const float bias = j < H ? bh[g * H + j] : 0.f;
  for (int i = threadIdx.x; i < CG_ROWS * CG_HP; i += CG_BLOCK) (&hs[0][0])[i] = 0.f;
  __syncthreads();
  const int tmax = tile_steps(tl);
  for (int t = 0; t < tmax; ++t) {
    float acc[CG_ROWS];
#pragma unroll
    for (int rr = 0; rr < CG_ROWS; ++rr) acc[rr] = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < CG_HP / 4; ++k4) {
#pragma unroll
      for (int rr = 0; rr < CG_ROWS; ++rr) {
        const float4 hv = reinterpret_cast<const float4*>(&hs[rr][0])[k4];       // the same address in every lane: a broadcast
        acc[rr] = fmaf(hv.x, w[4 * k4], acc[rr]);
        acc[rr] = fmaf(hv.y, w[4 * k4 + 1], acc[rr]);
        acc[rr] = fmaf(hv.z, w[4 * k4 + 2], acc[rr]);
        acc[rr] = fmaf(hv.w, w[4 * k4 + 3], acc[rr]);
      }
    }
#pragma unroll
    for (int rr = 0; rr < CG_ROWS; ++rr) gh[g][rr][j] = acc[rr] + bias;
    __syncthreads();
    for (int i = threadIdx.x; i < CG_ROWS * CG_HP; i += CG_BLOCK) {
      const int rr = i / CG_HP, u = i - rr * CG_HP;
      if (rr >= nr || u >= H) continue;
      const size_t row = (size_t)(tl.row0[rr] + (int64_t)t * C);
      const float hv = hs[rr][u];
      if (TRAIN) hp[row * H + u] = hv;
      if (t < tl.steps[rr]) {
        const float* gp = gi + row * 3 * H;
        const float hn = gh[2][rr][u];
        const float r = sigmoidf(gp[u] + gh[0][rr][u]), z = sigmoidf(gp[H + u] + gh[1][rr][u]), n = tanhf(fmaf(r, hn, gp[2 * H + u]));
        hs[rr][u] = fmaf(z, hv - n, n);                // (1 - z) n + z h
        if (TRAIN) {
          float* gs = gates + row * 4 * H;
          gs[u] = r; gs[H + u] = z; gs[2 * H + u] = n; gs[3 * H + u] = hn;
        }
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < CG_ROWS * CG_HP; i += CG_BLOCK) {
    const int rr = i / CG_HP, u = i - rr * CG_HP;
    if (rr >= nr || u >= H) continue;
    const float hv = hs[rr][u];
    if (TRAIN)
      for (int t = tmax; t < S; ++t) hp[(size_t)(tl.row0[rr] + (int64_t)t * C) * H + u] = hv;      // no row steps here: the state it keeps
    out[tl.b[rr] * ldo + (int64_t)tl.c[rr] * H + u] = hv;
  }
}

// ---------------------------------------------------------------- the recurrence, backward
// grid as cg_fwd_kernel.  gout [B, C H] rows ldg apart = d out.  Writes dgi, dgh [B S C, 3H] (every row of every step: zeros where the
// row did not take the step).
__global__ __launch_bounds__(CG_BLOCK) void cg_bwd_kernel(const float* __restrict__ W, const int64_t* __restrict__ len, const float* __restrict__ gout,
                                                     int64_t ldg, int64_t R, int S, int C, int H, const float* __restrict__ hp,
                                                     const float* __restrict__ gates, float* __restrict__ dgi, float* __restrict__ dgh) {
  __shared__ float dh[CG_ROWS][CG_HP];                 // dh_t; between the phases of a step: the part of dh_{t-1} that does not pass W_hh
  __shared__ __attribute__((aligned(16))) float dg[3][CG_ROWS][CG_HP];
  __shared__ float part[3][CG_ROWS][CG_HP];
  __shared__ Tile tl;
  const int g = threadIdx.x / CG_HP, k = threadIdx.x - g * CG_HP;
  const int64_t r0 = (int64_t)blockIdx.x * CG_ROWS;
  const int nr = (int)min((int64_t)CG_ROWS, R - r0);
  tile_rows(tl, len, r0, nr, S, C, nullptr);
  float w[CG_HP];                                      // column k of W_g
#pragma unroll
  for (int u = 0; u < CG_HP; ++u) w[u] = (k < H && u < H) ? W[(size_t)(g * H + u) * H + k] : 0.f;
  __syncthreads();
  const int tmax = tile_steps(tl);
  for (int i = threadIdx.x; i < CG_ROWS * CG_HP; i += CG_BLOCK) {
    const int rr = i / CG_HP, u = i - rr * CG_HP;
    const bool in = rr < nr && u < H;
    dh[rr][u] = in ? gout[tl.b[rr] * ldg + (int64_t)tl.c[rr] * H + u] : 0.f;
    if (!in) { dg[0][rr][u] = dg[1][rr][u] = dg[2][rr][u] = 0.f; }          // never written again: the products read them as zeros
    if (in)
      for (int t = tmax; t < S; ++t) {
        const size_t at = (size_t)(tl.row0[rr] + (int64_t)t * C) * 3 * H + u;
#pragma unroll
        for (int q = 0; q < 3; ++q) dgi[at + q * H] = dgh[at + q * H] = 0.f;
      }
  }
  for (int t = tmax - 1; t >= 0; --t) {
    // the same thread owns (rr, u) here and in the update below, so no barrier separates a step's update from the next step's rebuild
    for (int i = threadIdx.x; i < CG_ROWS * CG_HP; i += CG_BLOCK) {
      const int rr = i / CG_HP, u = i - rr * CG_HP;
      if (rr >= nr || u >= H) continue;
      const size_t row = (size_t)(tl.row0[rr] + (int64_t)t * C);
      float ir = 0.f, iz = 0.f, in = 0.f, hn = 0.f;    // d gi of r, z, n; d gh of n (d gh of r and z are d gi's)
      if (t < tl.steps[rr]) {
        const float* gs = gates + row * 4 * H;
        const float d = dh[rr][u], r = gs[u], z = gs[H + u], n = gs[2 * H + u];
        iz = d * (hp[row * H + u] - n) * (z * (1.0f - z));
        in = d * (1.0f - z) * (1.0f - n * n);
        hn = in * r;
        ir = in * gs[3 * H + u] * (r * (1.0f - r));
        dh[rr][u] = d * z;
      }
      dg[0][rr][u] = ir; dg[1][rr][u] = iz; dg[2][rr][u] = hn;
      float* pi = dgi + row * 3 * H + u;
      float* ph = dgh + row * 3 * H + u;
      pi[0] = ir; pi[H] = iz; pi[2 * H] = in;
      ph[0] = ir; ph[H] = iz; ph[2 * H] = hn;
    }
    __syncthreads();
    float acc[CG_ROWS];
#pragma unroll
    for (int rr = 0; rr < CG_ROWS; ++rr) acc[rr] = 0.f;
#pragma unroll
    for (int u4 = 0; u4 < CG_HP / 4; ++u4) {
#pragma unroll
      for (int rr = 0; rr < CG_ROWS; ++rr) {
        const float4 dv = reinterpret_cast<const float4*>(&dg[g][rr][0])[u4];
        acc[rr] = fmaf(dv.x, w[4 * u4], acc[rr]);
        acc[rr] = fmaf(dv.y, w[4 * u4 + 1], acc[rr]);
        acc[rr] = fmaf(dv.z, w[4 * u4 + 2], acc[rr]);
        acc[rr] = fmaf(dv.w, w[4 * u4 + 3], acc[rr]);
      }
    }
#pragma unroll
    for (int rr = 0; rr < CG_ROWS; ++rr) part[g][rr][k] = acc[rr];
    __syncthreads();
    for (int i = threadIdx.x; i < CG_ROWS * CG_HP; i += CG_BLOCK) {
      const int rr = i / CG_HP, u = i - rr * CG_HP;
      if (rr >= nr || u >= H || t >= tl.steps[rr]) continue;                   // a row that did not take the step passes dh through
      dh[rr][u] += (part[0][rr][u] + part[1][rr][u]) + part[2][rr][u];
    }
  }
}

// ---------------------------------------------------------------- axis-0 attention, 65 <= head dim <= 128 (the fixed-dim family: axis0.hip)
constexpr int AW_BLOCK = 256, AW_WAVES = 4;      // a wave per own row: AW_WAVES rows of one (slot, head) pair per workgroup
constexpr int AW_KT = 32;                        // rows of the other side per LDS tile (2 x 16 KiB)
constexpr int AW_DH = 128, AW_MIN_DH = 65;

// stages rows [t0, t0 + cnt) of one pair: a[j][d] = fa(j, d), b likewise; columns d >= dh are zeros
template <typename FA, typename FB>
__device__ __forceinline__ void aw_stage(int cnt, int dh, float (*a)[AW_DH], float (*b)[AW_DH], FA fa, FB fb) {
  for (int i = threadIdx.x; i < cnt * AW_DH; i += AW_BLOCK) {
    const int j = i / AW_DH, d = i - j * AW_DH;
    a[j][d] = d < dh ? fa(j, d) : 0.f;
    b[j][d] = d < dh ? fb(j, d) : 0.f;
  }
}

// grid (E heads, ceil(N / AW_WAVES)); qkv [N, E, 3D], out [N, E, D], stats [N E heads 3]
__global__ __launch_bounds__(AW_BLOCK) void aw_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ stats, int64_t N,
                                                     int E, int D, int heads, int dh) {
  __shared__ float ks[AW_KT][AW_DH], vs[AW_KT][AW_DH];
  const int lane = threadIdx.x % 64, wv = threadIdx.x / 64;
  const int pair = blockIdx.x, e = pair / heads, hh = pair - e * heads;
  const int64_t n = (int64_t)blockIdx.y * AW_WAVES + wv;
  const bool act = n < N;                               // wave-uniform
  const float scale = 1.0f / sqrtf((float)dh);
  const size_t ld = (size_t)E * 3 * D;
  const float* base = qkv + (size_t)e * 3 * D + hh * dh;
  const int d0 = lane, d1 = lane + 64;
  const bool on0 = act && d0 < dh, on1 = act && d1 < dh;
  const float q0 = on0 ? base[n * ld + d0] * scale : 0.f, q1 = on1 ? base[n * ld + d1] * scale : 0.f;
  float o0 = 0.f, o1 = 0.f, mx = -INFINITY, sum = 0.f;
  for (int64_t t0 = 0; t0 < N; t0 += AW_KT) {
    const int cnt = (int)min((int64_t)AW_KT, N - t0);
    __syncthreads();
    aw_stage(cnt, dh, ks, vs, [&](int j, int d) { return base[(t0 + j) * ld + D + d]; }, [&](int j, int d) { return base[(t0 + j) * ld + 2 * D + d]; });
    __syncthreads();
    if (act)
      for (int j = 0; j < cnt; ++j) {
        const float s = wsum(fmaf(q1, ks[j][d1], q0 * ks[j][d0]));
        if (s > mx) {
          const float f = expf(mx - s);
          sum *= f; o0 *= f; o1 *= f;
          mx = s;
        }
        const float p = expf(s - mx);
        sum += p;
        o0 = fmaf(p, vs[j][d0], o0);
        o1 = fmaf(p, vs[j][d1], o1);
      }
  }
  if (act) {
    const float inv = 1.0f / sum;
    float* dst = out + (size_t)n * E * D + (size_t)e * D + hh * dh;
    if (on0) dst[d0] = o0 * inv;
    if (on1) dst[d1] = o1 * inv;
    if (stats && lane == 0) {
      float* st = stats + ((size_t)n * E * heads + pair) * 3;
      st[0] = mx; st[1] = sum;
    }
  }
}
// wave = query row: D_i = d out_i . out_i, dq_i = sum_j P_ij (dP_ij - D_i) k_j / sqrt(dh); stats gets D_i
__global__ __launch_bounds__(AW_BLOCK) void aw_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ att, const float* __restrict__ datt,
                                                       float* __restrict__ dqkv, float* __restrict__ stats, int64_t N, int E, int D, int heads, int dh) {
  __shared__ float ks[AW_KT][AW_DH], vs[AW_KT][AW_DH];
  const int lane = threadIdx.x % 64, wv = threadIdx.x / 64;
  const int pair = blockIdx.x, e = pair / heads, hh = pair - e * heads;
  const int64_t n = (int64_t)blockIdx.y * AW_WAVES + wv;
  const bool act = n < N;
  const float scale = 1.0f / sqrtf((float)dh);
  const size_t ld = (size_t)E * 3 * D;
  const float* base = qkv + (size_t)e * 3 * D + hh * dh;
  const size_t oat = (size_t)(act ? n : 0) * E * D + (size_t)e * D + hh * dh;
  const int d0 = lane, d1 = lane + 64;
  const bool on0 = act && d0 < dh, on1 = act && d1 < dh;
  const float q0 = on0 ? base[n * ld + d0] * scale : 0.f, q1 = on1 ? base[n * ld + d1] * scale : 0.f;
  const float g0 = on0 ? datt[oat + d0] : 0.f, g1 = on1 ? datt[oat + d1] : 0.f;
  const float Dn = wsum(fmaf(g1, on1 ? att[oat + d1] : 0.f, g0 * (on0 ? att[oat + d0] : 0.f)));
  float* st = stats + ((size_t)(act ? n : 0) * E * heads + pair) * 3;
  const float mx = act ? st[0] : 0.f, inv = act ? 1.0f / st[1] : 0.f;
  float dq0 = 0.f, dq1 = 0.f;
  for (int64_t t0 = 0; t0 < N; t0 += AW_KT) {
    const int cnt = (int)min((int64_t)AW_KT, N - t0);
    __syncthreads();
    aw_stage(cnt, dh, ks, vs, [&](int j, int d) { return base[(t0 + j) * ld + D + d]; }, [&](int j, int d) { return base[(t0 + j) * ld + 2 * D + d]; });
    __syncthreads();
    if (act)
      for (int j = 0; j < cnt; ++j) {
        const float k0 = ks[j][d0], k1 = ks[j][d1];
        const float s = wsum(fmaf(q1, k1, q0 * k0)), gv = wsum(fmaf(g1, vs[j][d1], g0 * vs[j][d0]));
        const float dsc = expf(s - mx) * inv * (gv - Dn) * scale;
        dq0 = fmaf(dsc, k0, dq0);
        dq1 = fmaf(dsc, k1, dq1);
      }
  }
  if (act) {
    float* dst = dqkv + n * ld + (size_t)e * 3 * D + hh * dh;
    if (on0) dst[d0] = dq0;
    if (on1) dst[d1] = dq1;
    if (lane == 0) st[2] = Dn;
  }
}
// wave = key row: dk_j = sum_i dS_ij q_i (scaled), dv_j = sum_i P_ij d out_i, queries in ascending order
__global__ __launch_bounds__(AW_BLOCK) void aw_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ datt, const float* __restrict__ stats,
                                                        float* __restrict__ dqkv, int64_t N, int E, int D, int heads, int dh) {
  __shared__ float qs[AW_KT][AW_DH], gs[AW_KT][AW_DH];
  __shared__ float sm[AW_KT], sl[AW_KT], sd[AW_KT];
  const int lane = threadIdx.x % 64, wv = threadIdx.x / 64;
  const int pair = blockIdx.x, e = pair / heads, hh = pair - e * heads;
  const int64_t n = (int64_t)blockIdx.y * AW_WAVES + wv;
  const bool act = n < N;
  const float scale = 1.0f / sqrtf((float)dh);
  const size_t ld = (size_t)E * 3 * D;
  const float* base = qkv + (size_t)e * 3 * D + hh * dh;
  const int d0 = lane, d1 = lane + 64;
  const bool on0 = act && d0 < dh, on1 = act && d1 < dh;
  const float k0 = on0 ? base[n * ld + D + d0] : 0.f, k1 = on1 ? base[n * ld + D + d1] : 0.f;
  const float v0 = on0 ? base[n * ld + 2 * D + d0] : 0.f, v1 = on1 ? base[n * ld + 2 * D + d1] : 0.f;
  float dk0 = 0.f, dk1 = 0.f, dv0 = 0.f, dv1 = 0.f;
  for (int64_t t0 = 0; t0 < N; t0 += AW_KT) {
    const int cnt = (int)min((int64_t)AW_KT, N - t0);
    __syncthreads();
    aw_stage(cnt, dh, qs, gs, [&](int j, int d) { return base[(t0 + j) * ld + d] * scale; },
             [&](int j, int d) { return datt[(size_t)(t0 + j) * E * D + (size_t)e * D + hh * dh + d]; });
    if ((int)threadIdx.x < cnt) {
      const float* st = stats + ((size_t)(t0 + threadIdx.x) * E * heads + pair) * 3;
      sm[threadIdx.x] = st[0]; sl[threadIdx.x] = 1.f / st[1]; sd[threadIdx.x] = st[2];
    }
    __syncthreads();
    if (act)
      for (int i = 0; i < cnt; ++i) {
        const float a0 = qs[i][d0], a1 = qs[i][d1], b0 = gs[i][d0], b1 = gs[i][d1];
        const float s = wsum(fmaf(a1, k1, a0 * k0)), gv = wsum(fmaf(b1, v1, b0 * v0));
        const float p = expf(s - sm[i]) * sl[i];
        const float dsc = p * (gv - sd[i]);               // qs carries the 1 / sqrt(dh)
        dk0 = fmaf(dsc, a0, dk0); dk1 = fmaf(dsc, a1, dk1);
        dv0 = fmaf(p, b0, dv0); dv1 = fmaf(p, b1, dv1);
      }
  }
  if (act) {
    float* dst = dqkv + n * ld + (size_t)e * 3 * D + hh * dh;
    if (on0) { dst[D + d0] = dk0; dst[2 * D + d0] = dv0; }
    if (on1) { dst[D + d1] = dk1; dst[2 * D + d1] = dv1; }
  }
}

int aw_check(const char* who, int64_t L0, int64_t B1, int E, int heads) {
  if (L0 < 0 || B1 < 0 || E <= 0 || heads <= 0 || E % heads)
    return fail(MANNER_HIP_E_INVALID, "%s: bad shape L0=%lld B1=%lld E=%d heads=%d", who, (long long)L0, (long long)B1, E, heads);
  if (E / heads < AW_MIN_DH || E / heads > AW_DH)
    return fail(MANNER_HIP_E_INVALID, "%s: head_dim %d unsupported (%d <= head_dim <= %d)", who, E / heads, AW_MIN_DH, AW_DH);
  if (B1 * heads > 0x7fffffffll || (L0 + AW_WAVES - 1) / AW_WAVES > 65535) return fail(MANNER_HIP_E_INVALID, "%s: L0 or B1 exceeds the grid", who);
  return MANNER_HIP_OK;
}
dim3 aw_grid(int64_t L0, int64_t B1, int heads) { return dim3((unsigned)(B1 * heads), (unsigned)((L0 + AW_WAVES - 1) / AW_WAVES)); }

// all in (b, t, c) row order, N = B S C rows: x rows as read [N, I]; the state entering each step [N, H]; r, z, n, W_hn h + b_hn [N, 4, H]
struct Saved { float *xs, *hp, *gates; };
void plan_saved(FloatBump& b, Saved& s, size_t N, size_t I, size_t H) {
  s.xs = b.take(N * I);
  s.hp = b.take(N * H);
  s.gates = b.take(N * 4 * H);
}
// forward: gi [N, 3H]; backward: d gi in its place and d gh [N, 3H] — one size serves both
struct Work { float *gi, *dgh; };
void plan_work(FloatBump& b, Work& w, size_t N, size_t H) {
  w.gi = b.take(N * 3 * H);
  w.dgh = b.take(N * 3 * H);
}

int cg_check(const char* who, int64_t B, int64_t S, int C, int I, int H) {
  if (B < 0 || S < 1 || C < 1 || I < 1 || H < 1)
    return fail(MANNER_HIP_E_INVALID, "%s: bad shape B=%lld S=%lld C=%d I=%d H=%d", who, (long long)B, (long long)S, C, I, H);
  if (S > CG_MAX_S) return fail(MANNER_HIP_E_INVALID, "%s: S=%lld unsupported (S <= %d)", who, (long long)S, CG_MAX_S);
  if (I > CG_MAX_I) return fail(MANNER_HIP_E_INVALID, "%s: I=%d unsupported (I <= %d)", who, I, CG_MAX_I);
  if (H > CG_HP) return fail(MANNER_HIP_E_INVALID, "%s: H=%d unsupported (H <= %d)", who, H, CG_HP);
  if (B > 0x7fffffffll || B * C > 0x7fffffffll || B * C * S > 0x7fffffffll)
    return fail(MANNER_HIP_E_INVALID, "%s: B=%lld C=%d S=%lld exceeds the grid", who, (long long)B, C, (long long)S);
  return MANNER_HIP_OK;
}

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" {

size_t manner_hip_channel_gru_saved_bytes(int64_t B, int64_t S, int32_t C, int32_t I, int32_t H) {
  if (B <= 0 || S <= 0 || C <= 0 || I <= 0 || H <= 0) return 0;
  FloatBump b(nullptr);
  Saved s;
  plan_saved(b, s, (size_t)B * S * C, (size_t)I, (size_t)H);
  return b.off * sizeof(float) + 256;
}

size_t manner_hip_channel_gru_workspace_bytes(int64_t B, int64_t S, int32_t C, int32_t I, int32_t H) {
  if (B <= 0 || S <= 0 || C <= 0 || I <= 0 || H <= 0) return 0;
  FloatBump b(nullptr);
  Work w;
  plan_work(b, w, (size_t)B * S * C, (size_t)H);
  return b.off * sizeof(float) + 256;
}

int manner_hip_channel_gru_forward(const float* x, int64_t x_stride_b, int64_t x_stride_s, const int64_t* lengths, const float* w_ih,
                                   const float* w_hh, const float* b_ih, const float* b_hh, int64_t B, int64_t S, int32_t C, int32_t I, int32_t H,
                                   float* out, int64_t ldo, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                                   int32_t* status, manner_hip_stream_t stream) {
  int rc;
  if ((rc = cg_check("channel_gru", B, S, C, I, H))) return rc;
  if (B == 0) return MANNER_HIP_OK;
  if (!x || !lengths || !w_ih || !w_hh || !b_ih || !b_hh || !out || !workspace) return fail(MANNER_HIP_E_INVALID, "channel_gru: null pointer");
  if (ldo < (int64_t)C * H || x_stride_s < 0 || x_stride_b < 0) return fail(MANNER_HIP_E_INVALID, "channel_gru: bad stride");
  if (workspace_bytes < manner_hip_channel_gru_workspace_bytes(B, S, C, I, H)) return fail(MANNER_HIP_E_WORKSPACE, "channel_gru: workspace too small");
  if (saved && saved_bytes < manner_hip_channel_gru_saved_bytes(B, S, C, I, H)) return fail(MANNER_HIP_E_WORKSPACE, "channel_gru: saved buffer too small");
  hipStream_t s = (hipStream_t)stream;
  FloatBump bw(workspace), bs(saved);
  Work w;
  Saved sv;
  const int64_t N = B * S * C, R = B * C;
  plan_work(bw, w, (size_t)N, (size_t)H);
  plan_saved(bs, sv, (size_t)N, (size_t)I, (size_t)H);
  if ((rc = launch_proj_rows(x, x_stride_b, x_stride_s, lengths, w_ih, b_ih, (int)S, (int)C, N, (int)I, 3 * H, w.gi, saved ? sv.xs : nullptr, s))) return rc;
  const dim3 grid((unsigned)((R + CG_ROWS - 1) / CG_ROWS));
  if (saved)
    hipLaunchKernelGGL(cg_fwd_kernel<true>, grid, dim3(CG_BLOCK), 0, s, w.gi, w_hh, b_hh, lengths, R, (int)S, (int)C, (int)H, out, ldo, sv.hp, sv.gates,
                       status);
  else
    hipLaunchKernelGGL(cg_fwd_kernel<false>, grid, dim3(CG_BLOCK), 0, s, w.gi, w_hh, b_hh, lengths, R, (int)S, (int)C, (int)H, out, ldo, (float*)nullptr,
                       (float*)nullptr, status);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_channel_gru_backward(const float* w_ih, const float* w_hh, const int64_t* lengths, const float* grad_out, int64_t ldg, int64_t B,
                                    int64_t S, int32_t C, int32_t I, int32_t H, void* saved, size_t saved_bytes, float* grad_x, float* grad_w_ih,
                                    float* grad_w_hh, float* grad_b_ih, float* grad_b_hh, void* workspace, size_t workspace_bytes,
                                    manner_hip_stream_t stream) {
  int rc;
  if ((rc = cg_check("channel_gru_backward", B, S, C, I, H))) return rc;
  if (!grad_w_ih || !grad_w_hh || !grad_b_ih || !grad_b_hh) return fail(MANNER_HIP_E_INVALID, "channel_gru_backward: null gradient");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {                                      // no row: the parameter gradients are sums over nothing
    MANNER_HIP_TRY(hipMemsetAsync(grad_w_ih, 0, (size_t)3 * H * I * sizeof(float), s));
    MANNER_HIP_TRY(hipMemsetAsync(grad_w_hh, 0, (size_t)3 * H * H * sizeof(float), s));
    MANNER_HIP_TRY(hipMemsetAsync(grad_b_ih, 0, (size_t)3 * H * sizeof(float), s));
    MANNER_HIP_TRY(hipMemsetAsync(grad_b_hh, 0, (size_t)3 * H * sizeof(float), s));
    return MANNER_HIP_OK;
  }
  if (!w_ih || !w_hh || !lengths || !grad_out || !saved || !grad_x || !workspace) return fail(MANNER_HIP_E_INVALID, "channel_gru_backward: null pointer");
  if (ldg < (int64_t)C * H) return fail(MANNER_HIP_E_INVALID, "channel_gru_backward: bad stride");
  if (saved_bytes < manner_hip_channel_gru_saved_bytes(B, S, C, I, H)) return fail(MANNER_HIP_E_WORKSPACE, "channel_gru_backward: saved buffer too small");
  if (workspace_bytes < manner_hip_channel_gru_workspace_bytes(B, S, C, I, H))
    return fail(MANNER_HIP_E_WORKSPACE, "channel_gru_backward: workspace too small");
  FloatBump bw(workspace), bs(saved);
  Work w;
  Saved sv;
  const int64_t N = B * S * C, R = B * C;
  plan_work(bw, w, (size_t)N, (size_t)H);
  plan_saved(bs, sv, (size_t)N, (size_t)I, (size_t)H);
  float* dgi = w.gi;                                 // the forward's gi is dead: its place holds d gi
  hipLaunchKernelGGL(cg_bwd_kernel, dim3((unsigned)((R + CG_ROWS - 1) / CG_ROWS)), dim3(CG_BLOCK), 0, s, w_hh, lengths, grad_out, ldg, R, (int)S, (int)C,
                     (int)H, sv.hp, sv.gates, dgi, w.dgh);
  MANNER_LAUNCH_CHECK();
  if ((rc = manner_hip_linear_backward(sv.hp, nullptr, w.dgh, N, H, 3 * H, nullptr, nullptr, grad_w_hh, grad_b_hh, stream))) return rc;
  return manner_hip_linear_backward(sv.xs, w_ih, dgi, N, I, 3 * H, nullptr, grad_x, grad_w_ih, grad_b_ih, stream);
}

int manner_hip_axis0_attention_wide(const float* qkv, int64_t L0, int64_t B1, int32_t E, int32_t heads, float* out, float* stats,
                                    manner_hip_stream_t stream) {
  int rc;
  if ((rc = aw_check("axis0_attention_wide", L0, B1, E, heads))) return rc;
  if (L0 == 0 || B1 == 0) return MANNER_HIP_OK;
  if (!qkv || !out) return fail(MANNER_HIP_E_INVALID, "axis0_attention_wide: null pointer");
  hipLaunchKernelGGL(aw_fwd_kernel, aw_grid(L0, B1, heads), dim3(AW_BLOCK), 0, (hipStream_t)stream, qkv, out, stats, L0, (int)B1, (int)E, (int)heads,
                     E / heads);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_axis0_attention_wide_backward_q(const float* qkv, const float* out, const float* grad_out, int64_t L0, int64_t B1, int32_t E,
                                               int32_t heads, float* grad_qkv, float* stats, manner_hip_stream_t stream) {
  int rc;
  if ((rc = aw_check("axis0_attention_wide_backward_q", L0, B1, E, heads))) return rc;
  if (L0 == 0 || B1 == 0) return MANNER_HIP_OK;
  if (!qkv || !out || !grad_out || !grad_qkv || !stats) return fail(MANNER_HIP_E_INVALID, "axis0_attention_wide_backward_q: null pointer");
  hipLaunchKernelGGL(aw_bwd_q_kernel, aw_grid(L0, B1, heads), dim3(AW_BLOCK), 0, (hipStream_t)stream, qkv, out, grad_out, grad_qkv, stats, L0, (int)B1,
                     (int)E, (int)heads, E / heads);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_axis0_attention_wide_backward_kv(const float* qkv, const float* grad_out, const float* stats, int64_t L0, int64_t B1, int32_t E,
                                                int32_t heads, float* grad_qkv, manner_hip_stream_t stream) {
  int rc;
  if ((rc = aw_check("axis0_attention_wide_backward_kv", L0, B1, E, heads))) return rc;
  if (L0 == 0 || B1 == 0) return MANNER_HIP_OK;
  if (!qkv || !grad_out || !grad_qkv || !stats) return fail(MANNER_HIP_E_INVALID, "axis0_attention_wide_backward_kv: null pointer");
  hipLaunchKernelGGL(aw_bwd_kv_kernel, aw_grid(L0, B1, heads), dim3(AW_BLOCK), 0, (hipStream_t)stream, qkv, grad_out, stats, grad_qkv, L0, (int)B1,
                     (int)E, (int)heads, E / heads);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // extern "C"
