// The operators of the CAUM baseline (reference manner/models/baselines/caum_plm_module.py), f32, forward and backward:
//   CAUMUserEncoder.forward (manner/models/components/user_encoder.py:121-178) with its DenseAttention (attention.py:119-141)
//   axis-0 multi-head attention at ANY head dim 1..64 (CAUM ships 25 in the user encoder and 5 in the entity encoder)
//   ReLU (CAUMCategoryEncoder, news_encoder.py:350-355)
// One call scores ONE candidate per user: x [B, S, D] clicked news, c [B, D] candidate -> out [B].  The concatenated operands of the
// reference are never built by torch: a pack kernel writes the window operand [x[s-1], x[s], x[s+1], c] and [c, x[s]] once, the
// producers of cat[cnn, self] write into the two column ranges of one buffer, and the candidate half of the dense attention's first
// Linear is computed once per user.  nn.MultiheadAttention is batch_first=False but fed [B, S, U]: attention runs ACROSS THE B USERS
// of the call at each history slot (as in the reference's other batch_first=False calls), so B is the key axis.
// manner_hip_caum_scores_all (the last section) scores ALL candidate columns of a dense [B, C, D] tensor in one call, eval() only, on
// shared history products and an f32 MFMA linear.  manner_hip_caum_train_all_forward / _backward (after it) are the same loop in train():
// all columns as B C S rows of one call, column c under its own dropout seed, forward and backward, every product on the matrix cores
// (wlin_kernel; mwgrad_kernel for the weight gradients, exported alone as manner_hip_wgrad_rows_f32).
// The per-column workload is small (B = 8, S = 50, widths 400) and latency-bound: plain f32 VALU kernels — its nn.Linear, forward and
// all three gradients, is the row kernels of rows_f32.hip (launch_lin_rows, launch_dx_rows, launch_wgrad_rows, launch_colsum_rows).  Every
// reduction across rows runs in a fixed order (no floating-point atomics): two runs give the same bits.
#include <math.h>

#include <algorithm>

#include "train_common.h"

namespace manner {
namespace {

constexpr int CA_MAX_S = 256, CA_MAX_W = 1024, CA_MAX_DH = 64;
constexpr int CA_BLOCK = 256, CA_WAVE = 64, CA_WAVES = CA_BLOCK / CA_WAVE;      // threads per workgroup, lanes per wave, waves per workgroup
constexpr int CA_FLAT_GRID = 8192;   // most workgroups of a grid-stride elementwise launch
constexpr int CA_ROWS = 8;       // rows per workgroup of the score and row kernels
constexpr int CA_LDS = 7168;     // floats of each of the two staged attention operands (2 x 28 KiB)
constexpr int CA_KT = 64;        // rows of the other side per tile when a (slot, head) pair does not fit CA_LDS or B > 256
static_assert(CA_KT * CA_MAX_DH <= CA_LDS, "a tile of the largest head fits");
static_assert(CA_MAX_S % CA_WAVE == 0, "one wave holds a user's scores, CA_MAX_S / CA_WAVE per lane");
static_assert(CA_KT <= CA_BLOCK, "the statistics of a tile fit one entry per thread");
static_assert(CA_WAVE == 64, "common.h's wsum / wmax reduce 64 lanes");

// ---------------------------------------------------------------- window / candidate operands
// grid (B S): a1[r] = [xd[b, s-1], xd[b, s], xd[b, s+1], cd[b]] (circular shift, user_encoder.py:128-144), a2[r] = [cd[b], xd[b, s]]
// (:149-151), cd[b] = dropout1(c[b]) (:122), xd = dropout2(x) (:123).  c is read by its row stride (the cand[:, i, :] view).
__global__ __launch_bounds__(CA_BLOCK) void pack_kernel(const float* __restrict__ x, const float* __restrict__ c, int64_t c_stride, int S, int D,
                                                   Drop d1, Drop d2, float* __restrict__ a1, float* __restrict__ a2, float* __restrict__ cd) {
  const int64_t r = blockIdx.x, b = r / S;
  const int s = (int)(r - b * S);
  const int sl = s == 0 ? S - 1 : s - 1, sr = s == S - 1 ? 0 : s + 1;
  const size_t xb = (size_t)b * S * D;
  for (int d = threadIdx.x; d < D; d += CA_BLOCK) {
    const size_t il = xb + (size_t)sl * D + d, im = xb + (size_t)s * D + d, ir = xb + (size_t)sr * D + d;
    const float vl = d2.apply(x[il], il), vm = d2.apply(x[im], im), vr = d2.apply(x[ir], ir);
    const float cv = d1.apply(c[b * c_stride + d], (uint64_t)b * D + d);
    float* p1 = a1 + (size_t)r * 4 * D;
    p1[d] = vl; p1[D + d] = vm; p1[2 * D + d] = vr; p1[3 * D + d] = cv;
    float* p2 = a2 + (size_t)r * 2 * D;
    p2[d] = cv; p2[D + d] = vm;
    if (s == 0) cd[(size_t)b * D + d] = cv;
  }
}

// ---------------------------------------------------------------- axis-0 attention at any head dim (the fixed-dim family: axis0.hip)
// qkv [N, E, 3D] (q | k | v), attention along the N axis for each (slot e, head) pair; dh = D / heads is a run-time value under the
// compile-time register width DHP.  The arithmetic is that of axis0.hip's axis0_fwd_kernel / axis0_bwd_*: q scaled first, online
// softmax over the keys in ascending order.  Threads are filled at small N: a workgroup takes P pairs, thread = (pair, row), and the
// K / V rows (backward-kv: the Q / d out rows) of all its pairs sit in LDS (A0Plan: P * N * dh <= CA_LDS floats per operand).  A pair
// that does not fit, or N > 256, runs alone in its workgroups with the other side streamed in tiles of CA_KT rows.
struct A0Plan { int P, KT, RQ; };          // pairs per workgroup, other-side rows per tile, own rows per workgroup
A0Plan a0_plan(int64_t N, int dh) {
  if (N <= CA_BLOCK && N * dh <= CA_LDS) {
    const int n = (int)N;
    return A0Plan{std::min(CA_BLOCK / n, CA_LDS / (n * dh)), n, n};
  }
  return A0Plan{1, CA_KT, CA_BLOCK};
}
struct A0Thread {
  bool act;
  int pl, pair, e, hh;
  int64_t n;
};
__device__ __forceinline__ A0Thread a0_thread(const A0Plan& pl, int64_t N, int E, int heads) {
  A0Thread t;
  t.pl = threadIdx.x / pl.RQ;
  t.n = (int64_t)blockIdx.y * pl.RQ + (threadIdx.x - t.pl * pl.RQ);
  t.pair = blockIdx.x * pl.P + t.pl;
  t.act = t.pl < pl.P && t.pair < E * heads && t.n < N;
  if (!t.act) { t.pair = 0; t.n = 0; }
  t.e = t.pair / heads;
  t.hh = t.pair - t.e * heads;
  return t;
}
// stages the rows [t0, t0 + cnt) of the workgroup's pairs: a[(pp * KT + j) * dh + d] = src_a[...], likewise b
template <typename FA, typename FB>
__device__ __forceinline__ void a0_stage(const A0Plan& pl, int cnt, int dh, int E, int heads, float* a, float* b, FA fa, FB fb) {
  const int per = cnt * dh;
  for (int i = threadIdx.x; i < pl.P * per; i += CA_BLOCK) {
    const int pp = i / per, rem = i - pp * per, j = rem / dh, d = rem - j * dh;
    const int gp = blockIdx.x * pl.P + pp;
    const bool ok = gp < E * heads;
    const int e = ok ? gp / heads : 0, hh = ok ? gp - e * heads : 0;
    a[(pp * pl.KT + j) * dh + d] = ok ? fa(j, e, hh, d) : 0.f;
    b[(pp * pl.KT + j) * dh + d] = ok ? fb(j, e, hh, d) : 0.f;
  }
}

template <int DHP>
__global__ __launch_bounds__(CA_BLOCK) void a0any_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ stats, int64_t N,
                                                        int E, int D, int heads, int dh, A0Plan pl) {
  __shared__ float ks[CA_LDS], vs[CA_LDS];
  const A0Thread t = a0_thread(pl, N, E, heads);
  const float scale = 1.0f / sqrtf((float)dh);
  const size_t ld = (size_t)E * 3 * D;
  const float* base = qkv + (size_t)t.e * 3 * D + t.hh * dh;
  float q[DHP], o[DHP];
#pragma unroll
  for (int d = 0; d < DHP; ++d) { q[d] = (t.act && d < dh) ? base[t.n * ld + d] * scale : 0.f; o[d] = 0.f; }
  float mx = -INFINITY, sum = 0.f;
  for (int64_t t0 = 0; t0 < N; t0 += pl.KT) {
    const int cnt = (int)min((int64_t)pl.KT, N - t0);
    __syncthreads();
    a0_stage(pl, cnt, dh, E, heads, ks, vs,
             [&](int j, int e, int hh, int d) { return qkv[(t0 + j) * ld + (size_t)e * 3 * D + D + hh * dh + d]; },
             [&](int j, int e, int hh, int d) { return qkv[(t0 + j) * ld + (size_t)e * 3 * D + 2 * D + hh * dh + d]; });
    __syncthreads();
    if (t.act)
      for (int j = 0; j < cnt; ++j) {
        const float* kp = ks + (t.pl * pl.KT + j) * dh;
        const float* vp = vs + (t.pl * pl.KT + j) * dh;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < DHP; ++d)
          if (d < dh) s = fmaf(q[d], kp[d], s);
        if (s > mx) {
          const float f = expf(mx - s);
          sum *= f;
#pragma unroll
          for (int d = 0; d < DHP; ++d) o[d] *= f;
          mx = s;
        }
        const float p = expf(s - mx);
        sum += p;
#pragma unroll
        for (int d = 0; d < DHP; ++d)
          if (d < dh) o[d] = fmaf(p, vp[d], o[d]);
      }
  }
  if (t.act) {
    const float inv = 1.0f / sum;
    float* dst = out + (size_t)t.n * E * D + (size_t)t.e * D + t.hh * dh;
#pragma unroll
    for (int d = 0; d < DHP; ++d)
      if (d < dh) dst[d] = o[d] * inv;
    if (stats) {
      float* st = stats + ((size_t)t.n * E * heads + t.pair) * 3;
      st[0] = mx; st[1] = sum;
    }
  }
}
// thread = query row: D_i = d out_i . out_i (= sum_j dP_ij P_ij), dq_i = sum_j P_ij (dP_ij - D_i) k_j / sqrt(dh); stats gets D_i
template <int DHP>
__global__ __launch_bounds__(CA_BLOCK) void a0any_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ att, const float* __restrict__ datt,
                                                          float* __restrict__ dqkv, float* __restrict__ stats, int64_t N, int E, int D, int heads,
                                                          int dh, A0Plan pl) {
  __shared__ float ks[CA_LDS], vs[CA_LDS];
  const A0Thread t = a0_thread(pl, N, E, heads);
  const float scale = 1.0f / sqrtf((float)dh);
  const size_t ld = (size_t)E * 3 * D;
  const float* base = qkv + (size_t)t.e * 3 * D + t.hh * dh;
  const size_t oat = (size_t)t.n * E * D + (size_t)t.e * D + t.hh * dh;
  float q[DHP], go[DHP], dq[DHP];
  float Dn = 0.f;
#pragma unroll
  for (int d = 0; d < DHP; ++d) {
    const bool on = t.act && d < dh;
    q[d] = on ? base[t.n * ld + d] * scale : 0.f;
    go[d] = on ? datt[oat + d] : 0.f;
    if (on) Dn = fmaf(go[d], att[oat + d], Dn);
    dq[d] = 0.f;
  }
  float* st = stats + ((size_t)t.n * E * heads + t.pair) * 3;
  const float mx = t.act ? st[0] : 0.f, inv = t.act ? 1.0f / st[1] : 0.f;
  for (int64_t t0 = 0; t0 < N; t0 += pl.KT) {
    const int cnt = (int)min((int64_t)pl.KT, N - t0);
    __syncthreads();
    a0_stage(pl, cnt, dh, E, heads, ks, vs,
             [&](int j, int e, int hh, int d) { return qkv[(t0 + j) * ld + (size_t)e * 3 * D + D + hh * dh + d]; },
             [&](int j, int e, int hh, int d) { return qkv[(t0 + j) * ld + (size_t)e * 3 * D + 2 * D + hh * dh + d]; });
    __syncthreads();
    if (t.act)
      for (int j = 0; j < cnt; ++j) {
        const float* kp = ks + (t.pl * pl.KT + j) * dh;
        const float* vp = vs + (t.pl * pl.KT + j) * dh;
        float s = 0.f, gv = 0.f;
#pragma unroll
        for (int d = 0; d < DHP; ++d)
          if (d < dh) { s = fmaf(q[d], kp[d], s); gv = fmaf(go[d], vp[d], gv); }
        const float dsc = expf(s - mx) * inv * (gv - Dn) * scale;
#pragma unroll
        for (int d = 0; d < DHP; ++d)
          if (d < dh) dq[d] = fmaf(dsc, kp[d], dq[d]);
      }
  }
  if (t.act) {
    float* dst = dqkv + t.n * ld + (size_t)t.e * 3 * D + t.hh * dh;
#pragma unroll
    for (int d = 0; d < DHP; ++d)
      if (d < dh) dst[d] = dq[d];
    st[2] = Dn;
  }
}
// thread = key row: dk_j = sum_i dS_ij q_i (scaled), dv_j = sum_i P_ij d out_i, queries in ascending order
template <int DHP>
__global__ __launch_bounds__(CA_BLOCK) void a0any_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ datt, const float* __restrict__ stats,
                                                           float* __restrict__ dqkv, int64_t N, int E, int D, int heads, int dh, A0Plan pl) {
  __shared__ float qs[CA_LDS], gs[CA_LDS];
  __shared__ float sm[CA_BLOCK], sl[CA_BLOCK], sd[CA_BLOCK];
  const A0Thread t = a0_thread(pl, N, E, heads);
  const float scale = 1.0f / sqrtf((float)dh);
  const size_t ld = (size_t)E * 3 * D;
  const float* base = qkv + (size_t)t.e * 3 * D + t.hh * dh;
  float k[DHP], v[DHP], dk[DHP], dv[DHP];
#pragma unroll
  for (int d = 0; d < DHP; ++d) {
    const bool on = t.act && d < dh;
    k[d] = on ? base[t.n * ld + D + d] : 0.f;
    v[d] = on ? base[t.n * ld + 2 * D + d] : 0.f;
    dk[d] = dv[d] = 0.f;
  }
  for (int64_t t0 = 0; t0 < N; t0 += pl.KT) {
    const int cnt = (int)min((int64_t)pl.KT, N - t0);
    __syncthreads();
    a0_stage(pl, cnt, dh, E, heads, qs, gs,
             [&](int j, int e, int hh, int d) { return qkv[(t0 + j) * ld + (size_t)e * 3 * D + hh * dh + d] * scale; },
             [&](int j, int e, int hh, int d) { return datt[(size_t)(t0 + j) * E * D + (size_t)e * D + hh * dh + d]; });
    for (int i = threadIdx.x; i < pl.P * cnt; i += CA_BLOCK) {      // P * cnt <= 256 (resident: P * N <= 256; tiled: CA_KT)
      const int pp = i / cnt, j = i - pp * cnt;
      const int gp = blockIdx.x * pl.P + pp;
      const float* st = stats + ((size_t)(t0 + j) * E * heads + (gp < E * heads ? gp : 0)) * 3;
      sm[pp * pl.KT + j] = st[0]; sl[pp * pl.KT + j] = 1.f / st[1]; sd[pp * pl.KT + j] = st[2];
    }
    __syncthreads();
    if (t.act)
      for (int i = 0; i < cnt; ++i) {
        const int at = t.pl * pl.KT + i;
        const float* qp = qs + at * dh;
        const float* gp = gs + at * dh;
        float s = 0.f, gv = 0.f;
#pragma unroll
        for (int d = 0; d < DHP; ++d)
          if (d < dh) { s = fmaf(qp[d], k[d], s); gv = fmaf(gp[d], v[d], gv); }
        const float p = expf(s - sm[at]) * sl[at];
        const float dsc = p * (gv - sd[at]);               // qs carries the 1/sqrt(dh)
#pragma unroll
        for (int d = 0; d < DHP; ++d)
          if (d < dh) { dk[d] = fmaf(dsc, qp[d], dk[d]); dv[d] = fmaf(p, gp[d], dv[d]); }
      }
  }
  if (t.act) {
    float* dst = dqkv + t.n * ld + (size_t)t.e * 3 * D + t.hh * dh;
#pragma unroll
    for (int d = 0; d < DHP; ++d)
      if (d < dh) { dst[D + d] = dk[d]; dst[2 * D + d] = dv[d]; }
  }
}

int a0any_check(const char* who, int64_t L0, int64_t B1, int E, int heads) {
  if (L0 < 0 || B1 < 0 || E <= 0 || heads <= 0 || E % heads)
    return fail(MANNER_HIP_E_INVALID, "%s: bad shape L0=%lld B1=%lld E=%d heads=%d", who, (long long)L0, (long long)B1, E, heads);
  if (E / heads > CA_MAX_DH) return fail(MANNER_HIP_E_INVALID, "%s: head_dim %d unsupported (1 <= head_dim <= %d)", who, E / heads, CA_MAX_DH);
  if (B1 * heads > 0x7fffffffll || (L0 + CA_BLOCK - 1) / CA_BLOCK > 65535) return fail(MANNER_HIP_E_INVALID, "%s: L0 or B1 exceeds the grid", who);
  return MANNER_HIP_OK;
}
#define MANNER_A0ANY_DISPATCH(DH_, CALL) \
  do {                                   \
    if (DH_ <= 8) CALL(8);               \
    else if (DH_ <= 16) CALL(16);        \
    else if (DH_ <= 32) CALL(32);        \
    else CALL(64);                       \
  } while (0)

// what every launch of the family starts from: the head dim, the plan and the grid (pair tiles, row tiles) over E slots
struct A0Launch { int dh; A0Plan pl; dim3 g; };
A0Launch a0_launch(int64_t N, int64_t E, int D, int heads) {
  const int dh = D / heads;
  const A0Plan pl = a0_plan(N, dh);
  return A0Launch{dh, pl, dim3((unsigned)((E * heads + pl.P - 1) / pl.P), (unsigned)((N + pl.RQ - 1) / pl.RQ))};
}
int launch_a0any_fwd(const float* qkv, float* out, float* stats, int64_t N, int64_t E, int D, int heads, hipStream_t s) {
  const A0Launch l = a0_launch(N, E, D, heads);
#define MANNER_A0(DHP_) hipLaunchKernelGGL((a0any_fwd_kernel<DHP_>), l.g, dim3(CA_BLOCK), 0, s, qkv, out, stats, N, (int)E, D, heads, l.dh, l.pl)
  MANNER_A0ANY_DISPATCH(l.dh, MANNER_A0);
#undef MANNER_A0
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}
int launch_a0any_bwd_q(const float* qkv, const float* att, const float* datt, float* dqkv, float* stats, int64_t N, int64_t E, int D, int heads,
                       hipStream_t s) {
  const A0Launch l = a0_launch(N, E, D, heads);
#define MANNER_A0(DHP_) hipLaunchKernelGGL((a0any_bwd_q_kernel<DHP_>), l.g, dim3(CA_BLOCK), 0, s, qkv, att, datt, dqkv, stats, N, (int)E, D, heads, l.dh, l.pl)
  MANNER_A0ANY_DISPATCH(l.dh, MANNER_A0);
#undef MANNER_A0
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}
int launch_a0any_bwd_kv(const float* qkv, const float* datt, const float* stats, float* dqkv, int64_t N, int64_t E, int D, int heads, hipStream_t s) {
  const A0Launch l = a0_launch(N, E, D, heads);
#define MANNER_A0(DHP_) hipLaunchKernelGGL((a0any_bwd_kv_kernel<DHP_>), l.g, dim3(CA_BLOCK), 0, s, qkv, datt, stats, dqkv, N, (int)E, D, heads, l.dh, l.pl)
  MANNER_A0ANY_DISPATCH(l.dh, MANNER_A0);
#undef MANNER_A0
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

// ---------------------------------------------------------------- dense-attention tail
// grid (ceil(R / CA_ROWS)), one wave per row, two rows each: score[r] = t2[r, :] . wc + bc (attention.py:139) and
// g[r] = cd[b, :] . all[r, :] — the final dot product (user_encoder.py:174-176) taken inside the sum: out[b] = sum_s p[s] g[b, s].
__global__ __launch_bounds__(CA_BLOCK) void score_kernel(const float* __restrict__ t2, const float* __restrict__ wc, const float* __restrict__ bc,
                                                    const float* __restrict__ all, const float* __restrict__ cd, int64_t R, int S, int H2, int U,
                                                    float* __restrict__ score, float* __restrict__ g) {
  const int wave = threadIdx.x / CA_WAVE, lane = threadIdx.x % CA_WAVE;
  for (int rr = wave; rr < CA_ROWS; rr += CA_WAVES) {
    const int64_t r = (int64_t)blockIdx.x * CA_ROWS + rr;
    if (r >= R) break;                               // wave-uniform
    const float* cb = cd + (size_t)(r / S) * U;
    float a = 0.f, d = 0.f;
    for (int j = lane; j < H2; j += CA_WAVE) a = fmaf(t2[r * H2 + j], wc[j], a);
    for (int j = lane; j < U; j += CA_WAVE) d = fmaf(cb[j], all[r * U + j], d);
    a = wsum(a); d = wsum(d);
    if (lane == 0) { score[r] = a + bc[0]; g[r] = d; }
  }
}
// grid (ceil(B / 4)), one wave per user: p = softmax over ALL S slots (user_encoder.py:172, no mask), out[b] = sum_s p[s] g[b, s].
// With dout: ds[r] = p (dout g - sum p dout g) (the score's gradient), wq[r] = dout p (the weight of cd[b] in d all[r]); the backward
// rebuilds p from the saved scores (S exps per user) instead of reading it back.  This is the one kernel with fewer than B x row-tiles
// workgroups: what is left per user after score_kernel are S <= 256 scalars, CA_MAX_S / CA_WAVE per lane of one wave.
__global__ __launch_bounds__(CA_BLOCK) void user_kernel(const float* __restrict__ score, const float* __restrict__ g, int64_t B, int S,
                                                   float* __restrict__ out, const float* __restrict__ dout,
                                                   float* __restrict__ ds, float* __restrict__ wq) {
  const int lane = threadIdx.x % CA_WAVE;
  const int64_t b = (int64_t)blockIdx.x * CA_WAVES + (threadIdx.x / CA_WAVE);
  if (b >= B) return;
  float l[CA_MAX_S / CA_WAVE], gv[CA_MAX_S / CA_WAVE], m = -INFINITY;
#pragma unroll
  for (int j = 0; j < CA_MAX_S / CA_WAVE; ++j) {
    const int s = lane + CA_WAVE * j;
    l[j] = s < S ? score[b * S + s] : -INFINITY;
    gv[j] = s < S ? g[b * S + s] : 0.f;
    m = fmaxf(m, l[j]);
  }
  m = wmax(m);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < CA_MAX_S / CA_WAVE; ++j) {
    l[j] = lane + CA_WAVE * j < S ? expf(l[j] - m) : 0.f;
    sum += l[j];
  }
  sum = wsum(sum);
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < CA_MAX_S / CA_WAVE; ++j) {
    l[j] /= sum;
    acc = fmaf(l[j], gv[j], acc);
  }
  acc = wsum(acc);
  if (!dout) {
    if (lane == 0) out[b] = acc;
    return;
  }
  const float go = dout[b];
#pragma unroll
  for (int j = 0; j < CA_MAX_S / CA_WAVE; ++j) {
    const int s = lane + CA_WAVE * j;
    if (s < S) {
      ds[b * S + s] = l[j] * (go * (gv[j] - acc));            // the difference first: exactly zero at S = 1, as in torch
      wq[b * S + s] = go * l[j];
    }
  }
}
// grid (ceil(R / CA_ROWS)): dt2[r, j] = ds[r] wc[j] tanh'[r, j] (d2, saved by the forward), dall[r, d] = wq[r] cd[b, d]
__global__ __launch_bounds__(CA_BLOCK) void tail_rows_kernel(const float* __restrict__ ds, const float* __restrict__ wq, const float* __restrict__ wc,
                                                        const float* __restrict__ d2, const float* __restrict__ cd, int64_t R, int S, int H2, int U,
                                                        float* __restrict__ dt2, float* __restrict__ dall) {
  for (int rr = 0; rr < CA_ROWS; ++rr) {
    const int64_t r = (int64_t)blockIdx.x * CA_ROWS + rr;
    if (r >= R) break;
    const float dsr = ds[r], wr = wq[r];
    const float* cb = cd + (size_t)(r / S) * U;
    for (int j = threadIdx.x; j < H2; j += CA_BLOCK) dt2[r * H2 + j] = dsr * wc[j] * d2[r * H2 + j];
    for (int d = threadIdx.x; d < U; d += CA_BLOCK) dall[r * U + d] = wr * cb[d];
  }
}
// out[b, j] = add[b, j] + sum_s w[b, s] x[b, s, off + j] (w == NULL: 1), s ascending on two chains; x rows ldx apart.
// grid (B, ceil(cols / 256)).  With `drop`: out = dropout-mask(out) by element index b * cols + j (the candidate's gradient).
__global__ __launch_bounds__(CA_BLOCK) void segsum_kernel(const float* __restrict__ w, const float* __restrict__ x, int ldx, int off, const float* __restrict__ x2,
                                                     int ldx2, const float* __restrict__ add, int S, int cols, Drop drop, bool dropped,
                                                     float* __restrict__ out) {
  const int64_t b = blockIdx.x;
  const int j = blockIdx.y * CA_BLOCK + threadIdx.x;
  if (j >= cols) return;
  float a0 = 0.f, a1 = 0.f;
  for (int s = 0; s < S; ++s) {
    const size_t r = (size_t)b * S + s;
    float v = x[r * ldx + off + j];
    if (x2) v += x2[r * ldx2 + j];
    if (w) v *= w[r];
    if (s & 1) a1 += v; else a0 += v;
  }
  float v = (a0 + a1) + (add ? add[(size_t)b * cols + j] : 0.f);
  if (dropped) v = drop.apply(v, (uint64_t)b * cols + j);
  out[(size_t)b * cols + j] = v;
}
// grid (B S): d x[b, s] = mask2 (dA1[b, s+1][0:D] + dA1[b, s][D:2D] + dA1[b, s-1][2D:3D] + dA2[b, s][D:2D]) — a gather of the three
// windows that read x[b, s] (circular), not a scatter
__global__ __launch_bounds__(CA_BLOCK) void window_dx_kernel(const float* __restrict__ da1, const float* __restrict__ da2, int S, int D, Drop d2,
                                                        float* __restrict__ dx) {
  const int64_t r = blockIdx.x, b = r / S;
  const int s = (int)(r - b * S);
  const int sl = s == 0 ? S - 1 : s - 1, sr = s == S - 1 ? 0 : s + 1;
  const size_t rb = (size_t)b * S;
  for (int d = threadIdx.x; d < D; d += CA_BLOCK) {
    const float v = ((da1[(rb + sr) * 4 * D + d] + da1[(rb + s) * 4 * D + D + d]) + da1[(rb + sl) * 4 * D + 2 * D + d]) + da2[(rb + s) * 2 * D + D + d];
    const size_t at = (rb + s) * D + d;
    dx[at] = d2.apply(v, at);
  }
}
__global__ __launch_bounds__(CA_BLOCK) void drop_inplace_kernel(float* x, int64_t n, Drop d) {
  for (int64_t i = (int64_t)blockIdx.x * CA_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CA_BLOCK) x[i] = d.apply(x[i], (uint64_t)i);
}
__global__ __launch_bounds__(CA_BLOCK) void relu_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * CA_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CA_BLOCK)
    out[i] = g ? (x[i] > 0.f ? g[i] : 0.f) : fmaxf(x[i], 0.f);
}
__global__ __launch_bounds__(CA_BLOCK) void tanh_bwd_kernel(const float* __restrict__ y, const float* __restrict__ g, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * CA_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CA_BLOCK) out[i] = g[i] * (1.0f - y[i] * y[i]);
}
unsigned flat_grid(int64_t n) {
  const int64_t blocks = (n + CA_BLOCK - 1) / CA_BLOCK;
  return (unsigned)(blocks < CA_FLAT_GRID ? blocks : CA_FLAT_GRID);
}

// ---------------------------------------------------------------- CAUMUserEncoder
struct Dims { int64_t B, S, R; int D, F, U, H1, H2, heads; };
enum { P_W1, P_B1, P_W2, P_B2, P_WIN, P_BIN, P_WOUT, P_BOUT, P_W3, P_B3, P_WA, P_BA, P_WB, P_BB, P_WC, P_BC, P_COUNT };
int caum_check(const char* who, int64_t B, int64_t S, int D, int F, int U, int H1, int H2, int heads, Dims& m) {
  if (B < 0 || S < 1 || D < 1 || F < 1 || U < 1 || H1 < 1 || H2 < 1 || heads < 1 || U % heads)
    return fail(MANNER_HIP_E_INVALID, "%s: bad shape B=%lld S=%lld D=%d F=%d U=%d H1=%d H2=%d heads=%d", who, (long long)B, (long long)S, D, F, U, H1,
                H2, heads);
  if (S > CA_MAX_S) return fail(MANNER_HIP_E_INVALID, "%s: S=%lld unsupported (S <= %d)", who, (long long)S, CA_MAX_S);
  if (D > CA_MAX_W) return fail(MANNER_HIP_E_INVALID, "%s: D=%d unsupported (D <= %d)", who, D, CA_MAX_W);
  if (F > CA_MAX_W) return fail(MANNER_HIP_E_INVALID, "%s: F=%d unsupported (F <= %d)", who, F, CA_MAX_W);
  if (U > CA_MAX_W) return fail(MANNER_HIP_E_INVALID, "%s: U=%d unsupported (U <= %d)", who, U, CA_MAX_W);
  if (H1 > CA_MAX_W) return fail(MANNER_HIP_E_INVALID, "%s: H1=%d unsupported (H1 <= %d)", who, H1, CA_MAX_W);
  if (H2 > CA_MAX_W) return fail(MANNER_HIP_E_INVALID, "%s: H2=%d unsupported (H2 <= %d)", who, H2, CA_MAX_W);
  if (D != U) return fail(MANNER_HIP_E_INVALID, "%s: news_vector_dim %d != user_vector_dim %d (the dense attention reads cat[all, candidate] as 2 x user_vector_dim)", who, D, U);
  if (U / heads > CA_MAX_DH) return fail(MANNER_HIP_E_INVALID, "%s: head_dim %d unsupported (head_dim <= %d)", who, U / heads, CA_MAX_DH);
  if (B * S > 0x7fffffffll || (B + CA_BLOCK - 1) / CA_BLOCK > 65535) return fail(MANNER_HIP_E_INVALID, "%s: B*S exceeds the grid", who);
  m = Dims{B, S, B * S, D, F, U, H1, H2, heads};
  return MANNER_HIP_OK;
}
struct Saved { float *a1, *a2, *cd, *cat, *h2, *qkv, *att, *stats, *all, *ct, *t1, *t2, *d1, *d2, *score, *g; };
void plan_saved(FloatBump& b, Saved& s, const Dims& m) {
  const size_t R = (size_t)m.R, B = (size_t)m.B;
  s.a1 = b.take(R * 4 * m.D);
  s.a2 = b.take(R * 2 * m.D);
  s.cd = b.take(B * m.D);
  s.cat = b.take(R * (m.F + m.U));
  s.h2 = b.take(R * m.U);
  s.qkv = b.take(R * 3 * m.U);
  s.att = b.take(R * m.U);
  s.stats = b.take(R * m.heads * 3);
  s.all = b.take(R * m.U);
  s.ct = b.take(B * m.H1);
  s.t1 = b.take(R * m.H1);
  s.t2 = b.take(R * m.H2);
  s.d1 = b.take(R * m.H1);                      // tanh' of the two dense-attention layers
  s.d2 = b.take(R * m.H2);
  s.score = b.take(R);
  s.g = b.take(R);
}
struct Work { float *ds, *wq, *dt2, *dt1, *dall, *dct, *dcd, *dcat, *datt, *dqkv, *dh2, *da2, *da1, *part; };
// everything but the partial sums of the weight gradients
void plan_work_rows(FloatBump& b, Work& w, const Dims& m) {
  const size_t R = (size_t)m.R, B = (size_t)m.B;
  w.ds = b.take(R);
  w.wq = b.take(R);
  w.dt2 = b.take(R * m.H2);
  w.dt1 = b.take(R * m.H1);
  w.dall = b.take(R * m.U);
  w.dct = b.take(B * m.H1);
  w.dcd = b.take(B * m.D);
  w.dcat = b.take(R * (m.F + m.U));
  w.datt = b.take(R * m.U);
  w.dqkv = b.take(R * 3 * m.U);
  w.dh2 = b.take(R * m.U);
  w.da2 = b.take(R * 2 * m.D);
  w.da1 = b.take(R * 4 * m.D);
}
void plan_work(FloatBump& b, Work& w, const Dims& m) {
  plan_work_rows(b, w, m);
  const size_t ok = std::max({(size_t)m.F * 4 * m.D, (size_t)m.U * 2 * m.D, (size_t)3 * m.U * m.U, (size_t)m.U * (m.F + m.U), (size_t)m.H1 * m.U,
                              (size_t)m.H2 * m.H1, (size_t)m.H2});
  w.part = b.take((size_t)wgrad_rows_groups(m.R) * ok);
}

// ---------------------------------------------------------------- all candidates of a call on shared history products
// Every nn.Linear of CAUMUserEncoder.forward in front of a nonlinearity acts on a history-only operand plus a candidate-only operand
// (eval(): no dropout between them), so with b the user, s the slot, c the candidate column
//   q|k|v[b, c, s] = QH[b, s] + QC[b, c],  all[b, c, s] = M att[b, c, s] + A[b, s] + Bc[b, c],  pre[b, c, s] = Wa[:, :U] all[b, c, s] + CT[b, c]
// (M = W3[:, F:] Wout folded once per call; manner_hip_caum_scores_all below lists the terms).  Only att -> all -> t1 -> t2 run over the
// B C S wide rows, in (b, c, s) order so that score_kernel / user_kernel take (b, c) as B C pseudo-users.
constexpr int WL_BK = 32;                            // input features per staging of the row-tiled linear
constexpr int WL_LD = WL_BK + 1;                     // LDS row pitch in floats: odd, so that the rows of an MFMA operand read distinct banks
constexpr int WL_SMALL_ROWS = 1024;                  // fewer rows than this: the 32 x 32 tile (more workgroups), else 128 x 64
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// where row r of a pass sits: r = (b * cp + cl) * S + s with cl the column within the pass, c = c0 + cl the column of the call
struct RowMap { int S, cp, C, c0; };

// y[r, o] = act(bias[o] + add_bs[b S + s, o] + add_bc[b C + c, o] + sum_k x[r, k] W[o, k]) — each of the three terms may be NULL; x rows
// ldx apart, W rows ldw apart, y rows ldy apart.  True f32 on the matrix cores, in two tiles:
//   128 rows x 64 output features, grid (ceil(R / 128), ceil(O / 64)): each wave takes 32 rows x 64 features on v_mfma_f32_32x32x2_f32;
//   SMALL, 32 x 32, grid (ceil(R / 32), ceil(O / 32)): each wave takes a 16 x 16 quarter on v_mfma_f32_16x16x4_f32 — for the launches of a
//     few hundred rows (the history side and the candidate side at B = 8), which the large tile leaves on a few dozen workgroups.
// `deriv` [R, O] (TANH only, may be NULL): tanh' = 4 e / (1 + e)^2 from the pre-activation; add_el / mul_el [R, O] (may be NULL): the
// elementwise terms of a data gradient, y = (add_el + sum) * mul_el.
// Either way a workgroup stages its rows and weight rows per 32 input features (the next step's floats wait in registers while this
// one multiplies), and an output is one k-ascending fmaf chain whatever its place in a tile and whichever tile: a row's bits do not
// depend on the tile, the pass or the row count of the launch.
template <bool TANH, bool SMALL>
__global__ __launch_bounds__(CA_BLOCK) void wlin_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ W, int ldw,
                                                   const float* __restrict__ bias, const float* __restrict__ add_bs,
                                                   const float* __restrict__ add_bc, RowMap m, int64_t R, int K, int O, float* __restrict__ y, int ldy,
                                                   float* __restrict__ deriv, const float* __restrict__ add_el, const float* __restrict__ mul_el) {
  constexpr int BM = SMALL ? 32 : 128, BN = SMALL ? 32 : 64;
  constexpr int SROWS = CA_BLOCK / WL_BK, XV = BM / SROWS, WV = BN / SROWS;        // staging: 8 rows per sweep; floats per thread of x, of W
  __shared__ float xs[BM][WL_LD];
  __shared__ float ws[BN][WL_LD];
  const int tid = threadIdx.x, wave = tid / CA_WAVE, lane = tid % CA_WAVE;
  const int64_t r0 = (int64_t)blockIdx.x * BM;
  const int nr = (int)min((int64_t)BM, R - r0);
  const int o0 = blockIdx.y * BN;
  const int sk = tid % WL_BK, sr = tid / WL_BK;          // staging: thread = (input feature, row)
  float xv[XV], wv[WV];
  auto fetch = [&](int k0) {
    const bool kin = k0 + sk < K;
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int rr = sr + i * SROWS;
      xv[i] = (kin && rr < nr) ? x[(size_t)(r0 + rr) * ldx + k0 + sk] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < WV; ++i) {
      const int oo = sr + i * SROWS;
      wv[i] = (kin && o0 + oo < O) ? W[(size_t)(o0 + oo) * ldw + k0 + sk] : 0.f;          // past O or K: zeros, no branch below
    }
  };
  // one output: the epilogue terms in a fixed order
  auto emit = [&](int rr, int oo, float v) {
    const int o = o0 + oo;
    if (rr >= nr || o >= O) return;
    const int64_t r = r0 + rr;
    if (bias) v += bias[o];
    if (add_bs || add_bc) {                              // r < 2^31 (caum_all_check)
      const uint32_t pu = (uint32_t)r / (uint32_t)m.S, s = (uint32_t)r - pu * (uint32_t)m.S;
      const uint32_t b = pu / (uint32_t)m.cp, cl = pu - b * (uint32_t)m.cp;
      if (add_bs) v += add_bs[((size_t)b * m.S + s) * O + o];
      if (add_bc) v += add_bc[((size_t)b * m.C + m.c0 + cl) * O + o];
    }
    if (add_el) v += add_el[(size_t)r * O + o];          // the data gradients: (add + sum) * mul, as dx_rows_kernel
    if (mul_el) v *= mul_el[(size_t)r * O + o];
    y[(size_t)r * ldy + o] = TANH ? tanhf(v) : v;
    if (TANH && deriv) {                                 // tanh' from the pre-activation, as lin_rows_kernel
      const float e = expf(-2.0f * fabsf(v)), den = 1.0f + e;
      deriv[(size_t)r * O + o] = 4.0f * e / (den * den);
    }
  };
  f32x16 acc0, acc1;
  f32x4 accs;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
#pragma unroll
  for (int i = 0; i < 4; ++i) accs[i] = 0.f;
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += WL_BK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < XV; ++i) xs[sr + i * SROWS][sk] = xv[i];
#pragma unroll
    for (int i = 0; i < WV; ++i) ws[sr + i * SROWS][sk] = wv[i];
    __syncthreads();
    if (k0 + WL_BK < K) fetch(k0 + WL_BK);
    if constexpr (SMALL) {                               // operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
      const int ar = (wave >> 1) * 16 + (lane & 15), br = (wave & 1) * 16 + (lane & 15), kq = lane >> 4;
#pragma unroll
      for (int kk = 0; kk < WL_BK; kk += 4) accs = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[ar][kk + kq], ws[br][kk + kq], accs, 0, 0, 0);
    } else {                                             // A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
      const int ar = wave * 32 + (lane & 31), kh = lane >> 5;
#pragma unroll
      for (int kk = 0; kk < WL_BK; kk += 2) {
        const float a = xs[ar][kk + kh];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ws[lane & 31][kk + kh], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ws[32 + (lane & 31)][kk + kh], acc1, 0, 0, 0);
      }
    }
  }
  if constexpr (SMALL) {                                 // C / D map: column = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) emit((wave >> 1) * 16 + 4 * (lane >> 4) + reg, (wave & 1) * 16 + (lane & 15), accs[reg]);
  } else {                                               // C / D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int rr = wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      emit(rr, lane & 31, acc0[reg]);
      emit(rr, 32 + (lane & 31), acc1[reg]);
    }
  }
}
int launch_wlin(bool tanh_act, const float* x, int ldx, const float* W, int ldw, const float* bias, const float* add_bs, const float* add_bc, RowMap m,
                int64_t R, int K, int O, float* y, int ldy, hipStream_t s, float* deriv = nullptr, const float* add_el = nullptr,
                const float* mul_el = nullptr) {
  const bool small = R < WL_SMALL_ROWS;
  const int bm = small ? 32 : 128, bn = small ? 32 : 64;
  const dim3 g((unsigned)((R + bm - 1) / bm), (unsigned)((O + bn - 1) / bn));
#define MANNER_WLIN(T_, S_) hipLaunchKernelGGL((wlin_kernel<T_, S_>), g, dim3(CA_BLOCK), 0, s, x, ldx, W, ldw, bias, add_bs, add_bc, m, R, K, O, y, ldy, deriv, add_el, mul_el)
  if (tanh_act && small) MANNER_WLIN(true, true);
  else if (tanh_act) MANNER_WLIN(true, false);
  else if (small) MANNER_WLIN(false, true);
  else MANNER_WLIN(false, false);
#undef MANNER_WLIN
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

// a0any_fwd_kernel with q, k, v of the pair (e = cl S + s, head) formed on the way into registers and LDS: row n is
// QH[n, s] + QC[n, c0 + cl] (qh [N, S, 3D], qc [N, C, 3D]); out [(n cp + cl) S + s, D], no statistics.  The [N, C, S, 3D] tensor is never
// written.  A copy of a0any_fwd_kernel's walk, not an instantiation of it: as one body over an operand policy the all-columns forward
// measured 1.5 - 1.9 % slower than with this copy, twice (profiles/side_kernels/ab_parent_linear.json).
template <int DHP>
__global__ __launch_bounds__(CA_BLOCK) void a0sum_fwd_kernel(const float* __restrict__ qh, const float* __restrict__ qc, float* __restrict__ out, int64_t N,
                                                        RowMap m, int D, int heads, int dh, A0Plan pl) {
  __shared__ float ks[CA_LDS], vs[CA_LDS];
  const int E = m.cp * m.S;
  const A0Thread t = a0_thread(pl, N, E, heads);
  const float scale = 1.0f / sqrtf((float)dh);
  const size_t ldh = (size_t)m.S * 3 * D, ldc = (size_t)m.C * 3 * D;
  const int cl = t.e / m.S, sl = t.e - cl * m.S;
  const float* hb = qh + (size_t)t.n * ldh + (size_t)sl * 3 * D + t.hh * dh;
  const float* cb = qc + (size_t)t.n * ldc + (size_t)(m.c0 + cl) * 3 * D + t.hh * dh;
  float q[DHP], o[DHP];
#pragma unroll
  for (int d = 0; d < DHP; ++d) { q[d] = (t.act && d < dh) ? (hb[d] + cb[d]) * scale : 0.f; o[d] = 0.f; }
  float mx = -INFINITY, sum = 0.f;
  for (int64_t t0 = 0; t0 < N; t0 += pl.KT) {
    const int cnt = (int)min((int64_t)pl.KT, N - t0);
    auto row = [&](int third, int j, int e, int hh, int d) {
      const int c = e / m.S, s = e - c * m.S;
      const size_t at = (size_t)third * D + hh * dh + d;
      return qh[(t0 + j) * ldh + (size_t)s * 3 * D + at] + qc[(t0 + j) * ldc + (size_t)(m.c0 + c) * 3 * D + at];
    };
    __syncthreads();
    a0_stage(pl, cnt, dh, E, heads, ks, vs, [&](int j, int e, int hh, int d) { return row(1, j, e, hh, d); },
             [&](int j, int e, int hh, int d) { return row(2, j, e, hh, d); });
    __syncthreads();
    if (t.act)
      for (int j = 0; j < cnt; ++j) {
        const float* kp = ks + (t.pl * pl.KT + j) * dh;
        const float* vp = vs + (t.pl * pl.KT + j) * dh;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < DHP; ++d)
          if (d < dh) s = fmaf(q[d], kp[d], s);
        if (s > mx) {
          const float f = expf(mx - s);
          sum *= f;
#pragma unroll
          for (int d = 0; d < DHP; ++d) o[d] *= f;
          mx = s;
        }
        const float p = expf(s - mx);
        sum += p;
#pragma unroll
        for (int d = 0; d < DHP; ++d)
          if (d < dh) o[d] = fmaf(p, vp[d], o[d]);
      }
  }
  if (t.act) {
    const float inv = 1.0f / sum;
    float* dst = out + (((size_t)t.n * m.cp + cl) * m.S + sl) * D + t.hh * dh;
#pragma unroll
    for (int d = 0; d < DHP; ++d)
      if (d < dh) dst[d] = o[d] * inv;
  }
}
int launch_a0sum_fwd(const float* qh, const float* qc, float* out, int64_t N, RowMap m, int D, int heads, hipStream_t s) {
  const A0Launch l = a0_launch(N, (int64_t)m.cp * m.S, D, heads);
#define MANNER_A0(DHP_) hipLaunchKernelGGL((a0sum_fwd_kernel<DHP_>), l.g, dim3(CA_BLOCK), 0, s, qh, qc, out, N, m, D, heads, l.dh, l.pl)
  MANNER_A0ANY_DISPATCH(l.dh, MANNER_A0);
#undef MANNER_A0
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

// grid (B S): win[r] = [x[b, s-1], x[b, s], x[b, s+1]] (circular, user_encoder.py:128-144) — the history three quarters of linear1's operand
__global__ __launch_bounds__(CA_BLOCK) void window_kernel(const float* __restrict__ x, int S, int D, float* __restrict__ win) {
  const int64_t r = blockIdx.x, b = r / S;
  const int s = (int)(r - b * S);
  const int sl = s == 0 ? S - 1 : s - 1, sr = s == S - 1 ? 0 : s + 1;
  const float* xb = x + (size_t)b * S * D;
  float* p = win + (size_t)r * 3 * D;
  for (int d = threadIdx.x; d < D; d += CA_BLOCK) {
    p[d] = xb[(size_t)sl * D + d]; p[D + d] = xb[(size_t)s * D + d]; p[2 * D + d] = xb[(size_t)sr * D + d];
  }
}
// out[k, j] = in[j, k], in [n, n] (out_proj.weight, for the fold W3[:, F:] Wout as a row-times-row product)
__global__ __launch_bounds__(CA_BLOCK) void transpose_square_kernel(const float* __restrict__ in, int n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * CA_BLOCK + threadIdx.x;
  if (i >= (int64_t)n * n) return;
  const int k = (int)(i / n), j = (int)(i - (int64_t)k * n);
  out[i] = in[(size_t)j * n + k];
}

// dst[h, j] = src[h, j], j < width, rows dpitch / spitch floats apart: the candidate rows of a pass out of [B, C, D], its scores into [B, C]
__global__ __launch_bounds__(CA_BLOCK) void rows_copy_kernel(const float* __restrict__ src, int64_t spitch, float* __restrict__ dst, int64_t dpitch,
                                                        int64_t width, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * CA_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CA_BLOCK) {
    const int64_t h = i / width, j = i - h * width;
    dst[h * dpitch + j] = src[h * spitch + j];
  }
}

// the buffers of one call: what depends on (b, s) alone, on (b, c) alone, on the weights alone — taken once — and the wide rows of a pass
struct AllBufs {
  float *win, *wx, *hx, *qh, *a, *cx1, *cx2, *qc, *bcand, *ct, *owt, *fold, *ba;      // once per call
  float *att, *all, *t1, *t2, *score, *g, *cd, *outp;                                    // per pass of cp columns
};
void plan_all(FloatBump& b, AllBufs& w, const Dims& m, int64_t C, int64_t cp) {
  const size_t R = (size_t)m.R, N = (size_t)m.B * C, P = (size_t)m.B * cp, W = P * m.S;
  w.win = b.take(R * 3 * m.D);
  w.wx = b.take(R * m.F);
  w.hx = b.take(R * m.U);
  w.qh = b.take(R * 3 * m.U);
  w.a = b.take(R * m.U);
  w.cx1 = b.take(N * m.F);
  w.cx2 = b.take(N * m.U);
  w.qc = b.take(N * 3 * m.U);
  w.bcand = b.take(N * m.U);
  w.ct = b.take(N * m.H1);
  w.owt = b.take((size_t)m.U * m.U);
  w.fold = b.take((size_t)m.U * m.U);
  w.ba = b.take(m.U);
  w.att = b.take(W * m.U);
  w.all = b.take(W * m.U);
  w.t1 = b.take(W * m.H1);
  w.t2 = b.take(W * m.H2);
  w.score = b.take(W);
  w.g = b.take(W);
  w.cd = b.take(P * m.D);
  w.outp = b.take(P);
}
size_t all_bytes(const Dims& m, int64_t C, int64_t cp) {
  FloatBump b(nullptr);
  AllBufs w;
  plan_all(b, w, m, C, cp);
  return b.off * sizeof(float) + 256;
}
// most columns a pass may take: its rows and its (column, slot, head) pairs stay below 2^31
int64_t all_max_cols(const Dims& m, int64_t C) {
  const int64_t lim = 0x7fffffffll / (std::max<int64_t>(m.B, m.heads) * m.S);
  return std::max<int64_t>(1, std::min(C, lim));
}
int caum_all_check(const char* who, int64_t B, int64_t S, int64_t C, int D, int F, int U, int H1, int H2, int heads, Dims& m) {
  int rc;
  if ((rc = caum_check(who, B, S, D, F, U, H1, H2, heads, m))) return rc;
  if (C < 0) return fail(MANNER_HIP_E_INVALID, "%s: bad shape C=%lld", who, (long long)C);
  if (B * std::max<int64_t>(C, 1) > 0x7fffffffll || std::max<int64_t>(B, heads) * S > 0x7fffffffll)
    return fail(MANNER_HIP_E_INVALID, "%s: B*C or one column's rows exceed the grid", who);
  return MANNER_HIP_OK;
}

// ---------------------------------------------------------------- training over all candidate columns
// The per-column training entry with the C columns as rows: R' = B C S rows in (b, c, s) order, (b, c) a pseudo-user of S slots, so
// that score_kernel, user_kernel, tail_rows_kernel, segsum_kernel and colsum_rows_kernel run as they are and the attention sees
// qkv [B, C S, 3U].  Nothing is shared between the columns — the reference draws a fresh dropout2 mask of the clicked news per column —
// but every product runs once over C times the rows, on the matrix cores: wlin_kernel forward and for the data gradients (over a weight
// transposed once per call), mwgrad_kernel for the weight gradients.  Column c draws with seeds[c] at the element indices of the
// per-column call, so its masks are those of manner_hip_caum_user_forward with that seed.
__device__ __forceinline__ Drop col_drop(Drop d, const uint64_t* __restrict__ seeds, int c) {
  if (seeds) d.seed = seeds[c];
  return d;
}
// grid (B C S): pack_kernel for row (b, c, s) — x[b, s +- 1] circular inside the S slots, cand[b, c], the column's seed
__global__ __launch_bounds__(CA_BLOCK) void pack_cols_kernel(const float* __restrict__ x, const float* __restrict__ cand, int S, int C, int D, Drop d1,
                                                        Drop d2, const uint64_t* __restrict__ seeds, float* __restrict__ a1, float* __restrict__ a2,
                                                        float* __restrict__ cd) {
  const int64_t r = blockIdx.x, pu = r / S, b = pu / C;
  const int s = (int)(r - pu * S), c = (int)(pu - b * C);
  const int sl = s == 0 ? S - 1 : s - 1, sr = s == S - 1 ? 0 : s + 1;
  d1 = col_drop(d1, seeds, c);
  d2 = col_drop(d2, seeds, c);
  const size_t xb = (size_t)b * S * D;
  for (int d = threadIdx.x; d < D; d += CA_BLOCK) {
    const size_t il = xb + (size_t)sl * D + d, im = xb + (size_t)s * D + d, ir = xb + (size_t)sr * D + d;
    const float vl = d2.apply(x[il], il), vm = d2.apply(x[im], im), vr = d2.apply(x[ir], ir);
    const float cv = d1.apply(cand[(size_t)pu * D + d], (uint64_t)b * D + d);
    float* p1 = a1 + (size_t)r * 4 * D;
    p1[d] = vl; p1[D + d] = vm; p1[2 * D + d] = vr; p1[3 * D + d] = cv;
    float* p2 = a2 + (size_t)r * 2 * D;
    p2[d] = cv; p2[D + d] = vm;
    if (s == 0) cd[(size_t)pu * D + d] = cv;
  }
}
// dropout3 (and its backward) on [B C S, W] rows: element j of row (b, c, s) draws at (b S + s) W + j with the column's seed
__global__ __launch_bounds__(CA_BLOCK) void drop_cols_kernel(float* x, int64_t n, int S, int C, int W, Drop d3, const uint64_t* __restrict__ seeds) {
  for (int64_t i = (int64_t)blockIdx.x * CA_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CA_BLOCK) {
    const int64_t r = i / W, pu = r / S, b = pu / C;
    const int j = (int)(i - r * W), s = (int)(r - pu * S), c = (int)(pu - b * C);
    x[i] = col_drop(d3, seeds, c).apply(x[i], (uint64_t)(b * S + s) * W + j);
  }
}
// grid (B S): window_dx_kernel's gather for each column, masked by the column's dropout2, the C columns added in ascending c on one chain
__global__ __launch_bounds__(CA_BLOCK) void window_dx_cols_kernel(const float* __restrict__ da1, const float* __restrict__ da2, int S, int C, int D, Drop d2,
                                                             const uint64_t* __restrict__ seeds, float* __restrict__ dx) {
  const int64_t r = blockIdx.x, b = r / S;
  const int s = (int)(r - b * S);
  const int sl = s == 0 ? S - 1 : s - 1, sr = s == S - 1 ? 0 : s + 1;
  for (int d = threadIdx.x; d < D; d += CA_BLOCK) {
    const size_t at = (size_t)r * D + d;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
      const size_t rb = ((size_t)b * C + c) * S;
      const float v = ((da1[(rb + sr) * 4 * D + d] + da1[(rb + s) * 4 * D + D + d]) + da1[(rb + sl) * 4 * D + 2 * D + d]) + da2[(rb + s) * 2 * D + D + d];
      const float m = col_drop(d2, seeds, c).apply(v, at);
      acc = c == 0 ? m : acc + m;
    }
    dx[at] = acc;
  }
}
// grid (B C, ceil(D / 256)): d cand[b, c] = dropout1-mask(dcd[b, c] + sum_s (da1[b, c, s][3D:] + da2[b, c, s][:D])) — segsum_kernel's sum on two
// chains, the mask by the column's seed at b D + d
__global__ __launch_bounds__(CA_BLOCK) void cand_dx_cols_kernel(const float* __restrict__ da1, const float* __restrict__ da2, const float* __restrict__ dcd, int S,
                                                           int C, int D, Drop d1, const uint64_t* __restrict__ seeds, float* __restrict__ out) {
  const int64_t pu = blockIdx.x, b = pu / C;
  const int c = (int)(pu - b * C), j = blockIdx.y * CA_BLOCK + threadIdx.x;
  if (j >= D) return;
  float a0 = 0.f, a1 = 0.f;
  for (int s = 0; s < S; ++s) {
    const size_t r = (size_t)pu * S + s;
    const float v = da1[r * 4 * D + 3 * D + j] + da2[r * 2 * D + j];
    if (s & 1) a1 += v; else a0 += v;
  }
  out[(size_t)pu * D + j] = col_drop(d1, seeds, c).apply((a0 + a1) + dcd[(size_t)pu * D + j], (uint64_t)b * D + j);
}

// dW[o, k] = sum_r dy[r, o] x[r, k] on the matrix cores, true f32: the product dy^T x with the ROWS as the contraction axis.  dy rows
// ldy apart, x rows ldx apart.  grid (ceil(K / BK), ceil(O / BO), G) in two tiles, as wlin_kernel:
//   64 output x 128 input features: wave = (o half, k half), 32 x 64 as two accumulators of v_mfma_f32_32x32x2_f32;
//   SMALL (O or K below 64), 32 x 32: each wave a 16 x 16 quarter on v_mfma_f32_16x16x4_f32.
// Group g walks its rows [g chunk, (g + 1) chunk) in stagings of MW_RB rows: the dy and x rows go to LDS as they lie in memory (row-major,
// coalesced; the next staging's floats wait in registers while this one multiplies) and are the MFMA operands as they lie there:
// A[i = o][k = r] = dys[r][o], B[k = r][j = k] = xs[r][k].  Large tile: the 32 lanes of a ds_read_b32 group read consecutive floats of
// one row, conflict-free at any pitch.  Small tile: a group is 16 columns of two consecutive rows, which a pitch of 32 floats would put
// on the same 16 banks (2-way); the rows are MW_SMALL_PAD floats longer, so the second row starts 16 banks on.
// An output is one r-ascending fmaf chain per group (rows past the group's end are zeros); the G partial sums part[g][o][k] are added in ascending g by wgrad_reduce_kernel (G == 1 writes dW itself).  No atomics: the same bits
// every run.
constexpr int MW_RB = 32;            // rows per staging
constexpr int MW_MAX_GROUPS = 64;    // most row groups
constexpr int MW_FILL = 512;         // workgroups a launch aims at (2 per CU)
constexpr int MW_SMALL_PAD = 16;     // small tile: LDS rows 48 floats apart, so that the two rows of a 32-lane read group sit 16 banks apart
template <bool SMALL>
__global__ __launch_bounds__(CA_BLOCK) void mwgrad_kernel(const float* __restrict__ dy, int ldy, const float* __restrict__ x, int ldx, int64_t R, int K, int O,
                                                     int64_t chunk, float* __restrict__ out, int ldo, int64_t gstride) {
  constexpr int BO = SMALL ? 32 : 64, BK = SMALL ? 32 : 128;
  constexpr int DV = MW_RB * BO / CA_BLOCK, XV = MW_RB * BK / CA_BLOCK;      // floats per thread of a staging
  constexpr int DROWS = CA_BLOCK / BO, XROWS = CA_BLOCK / BK;                  // rows per sweep of the staging threads
  constexpr int PAD = SMALL ? MW_SMALL_PAD : 0;
  __shared__ float dys[MW_RB][BO + PAD];
  __shared__ float xs[MW_RB][BK + PAD];
  const int tid = threadIdx.x, wave = tid / CA_WAVE, lane = tid % CA_WAVE;
  const int k0 = blockIdx.x * BK, o0 = blockIdx.y * BO;
  const int64_t r0 = (int64_t)blockIdx.z * chunk, r1 = min(R, r0 + chunk);
  const int dc = tid % BO, dr = tid / BO, xc = tid % BK, xr = tid / BK;
  float dv[DV], xv[XV];
  auto fetch = [&](int64_t rb) {
#pragma unroll
    for (int i = 0; i < DV; ++i) {
      const int64_t r = rb + dr + i * DROWS;
      dv[i] = (r < r1 && o0 + dc < O) ? dy[(size_t)r * ldy + o0 + dc] : 0.f;           // past the group, O or K: zeros, no branch below
    }
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int64_t r = rb + xr + i * XROWS;
      xv[i] = (r < r1 && k0 + xc < K) ? x[(size_t)r * ldx + k0 + xc] : 0.f;
    }
  };
  f32x16 acc0, acc1;
  f32x4 accs;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
#pragma unroll
  for (int i = 0; i < 4; ++i) accs[i] = 0.f;
  fetch(r0);
  for (int64_t rb = r0; rb < r1; rb += MW_RB) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < DV; ++i) dys[dr + i * DROWS][dc] = dv[i];
#pragma unroll
    for (int i = 0; i < XV; ++i) xs[xr + i * XROWS][xc] = xv[i];
    __syncthreads();
    if (rb + MW_RB < r1) fetch(rb + MW_RB);
    if constexpr (SMALL) {                               // operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
      const int ao = (wave >> 1) * 16 + (lane & 15), bk = (wave & 1) * 16 + (lane & 15), rq = lane >> 4;
#pragma unroll
      for (int rr = 0; rr < MW_RB; rr += 4) accs = __builtin_amdgcn_mfma_f32_16x16x4f32(dys[rr + rq][ao], xs[rr + rq][bk], accs, 0, 0, 0);
    } else {                                             // A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
      const int ao = (wave & 1) * 32 + (lane & 31), bk = (wave >> 1) * 64 + (lane & 31), rh = lane >> 5;
#pragma unroll
      for (int rr = 0; rr < MW_RB; rr += 2) {
        const float a = dys[rr + rh][ao];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xs[rr + rh][bk], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xs[rr + rh][bk + 32], acc1, 0, 0, 0);
      }
    }
  }
  float* dst = out + (size_t)blockIdx.z * gstride;
  auto emit = [&](int oo, int kk, float v) {
    if (o0 + oo < O && k0 + kk < K) dst[(size_t)(o0 + oo) * ldo + k0 + kk] = v;
  };
  if constexpr (SMALL) {                                 // C / D map: column = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) emit((wave >> 1) * 16 + 4 * (lane >> 4) + reg, (wave & 1) * 16 + (lane & 15), accs[reg]);
  } else {                                               // C / D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int oo = (wave & 1) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      emit(oo, (wave >> 1) * 64 + (lane & 31), acc0[reg]);
      emit(oo, (wave >> 1) * 64 + 32 + (lane & 31), acc1[reg]);
    }
  }
}
// the split of a launch: a function of (R, O, K) alone.  Enough row groups for MW_FILL workgroups — the H2 x H1 and 1 x H2 products have a
// handful of (o, k) tiles — of at least one staging each, in whole stagings.
struct MwPlan { bool small; int G; int64_t chunk; };
MwPlan mw_plan(int64_t R, int K, int O) {
  MwPlan p;
  p.small = O < 64 || K < 64;
  const int64_t tiles = p.small ? (int64_t)((O + 31) / 32) * ((K + 31) / 32) : (int64_t)((O + 63) / 64) * ((K + 127) / 128);
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>({(int64_t)MW_MAX_GROUPS, (MW_FILL + tiles - 1) / tiles, R / MW_RB}));
  p.chunk = ((R + want - 1) / want + MW_RB - 1) / MW_RB * MW_RB;
  p.G = (int)((R + p.chunk - 1) / p.chunk);
  return p;
}
size_t mw_part_floats(int64_t R, int K, int O) {
  const MwPlan p = mw_plan(R, K, O);
  return p.G > 1 ? (size_t)p.G * O * K : 0;
}
// R >= 1; part holds mw_part_floats(R, K, O) floats
int launch_mwgrad(const float* dy, int ldy, const float* x, int ldx, int64_t R, int K, int O, float* part, float* dW, int ldo, hipStream_t s) {
  const MwPlan p = mw_plan(R, K, O);
  const int bo = p.small ? 32 : 64, bk = p.small ? 32 : 128;
  const dim3 g((unsigned)((K + bk - 1) / bk), (unsigned)((O + bo - 1) / bo), (unsigned)p.G);
  float* out = p.G == 1 ? dW : part;
  const int ld = p.G == 1 ? ldo : K;
  const int64_t gs = p.G == 1 ? 0 : (int64_t)O * K;
  if (p.small) hipLaunchKernelGGL(mwgrad_kernel<true>, g, dim3(CA_BLOCK), 0, s, dy, ldy, x, ldx, R, K, O, p.chunk, out, ld, gs);
  else hipLaunchKernelGGL(mwgrad_kernel<false>, g, dim3(CA_BLOCK), 0, s, dy, ldy, x, ldx, R, K, O, p.chunk, out, ld, gs);
  MANNER_LAUNCH_CHECK();
  return p.G > 1 ? launch_wgrad_reduce(part, K, O, p.G, dW, ldo, s) : MANNER_HIP_OK;
}
// the weight gradients of the all-columns backward, selected per launch by the row count alone: at equal (R, K, O) of the shipped widths
// (profiles/caum/kernel_trace.json, weight_gradient_equal_shapes) mwgrad_kernel is 2.1 - 7.7 x wgrad_rows_kernel from 320 rows on and
// slower only at the 40 rows of the B C pairs at B = 8 (7.3 against 5.6 us: one staging, 28 workgroups) — below MW_MIN_ROWS rows the
// one-thread-per-(o, k) kernel runs, in one group (wgrad_groups: no partial sums).  x [R, K] contiguous.
constexpr int MW_MIN_ROWS = 64;
static_assert(MW_MIN_ROWS <= WGRAD_GROUP_ROWS, "below MW_MIN_ROWS rows wgrad_rows_kernel writes dW itself");
int launch_wgrad_all(const float* dy, int ldy, const float* x, int64_t R, int K, int O, float* part, float* dW, int ldo, hipStream_t s) {
  if (R < MW_MIN_ROWS) return launch_wgrad_rows(dy, ldy, x, R, K, O, nullptr, dW, ldo, s);
  return launch_mwgrad(dy, ldy, x, K, R, K, O, part, dW, ldo, s);
}
// dx [R, K] = (add + dy W) * mul on wlin_kernel: W [O, K] (rows ldw apart) transposed into wt [K, O] first
int launch_mdx(const float* dy, int ldy, const float* W, int ldw, int64_t R, int K, int O, const float* add, const float* mul, float* dx, float* wt,
               hipStream_t s) {
  const int rc = launch_transpose_tile(W, ldw, O, K, wt, s);
  if (rc) return rc;
  return launch_wlin(false, dy, ldy, wt, O, nullptr, nullptr, nullptr, RowMap{1, 1, 1, 0}, R, O, K, dx, K, s, nullptr, add, mul);
}

// the wide view of a call: P = B C pseudo-users, R = B C S rows
int caum_train_all_check(const char* who, int64_t B, int64_t S, int64_t C, int D, int F, int U, int H1, int H2, int heads, Dims& m) {
  int rc;
  if ((rc = caum_check(who, B, S, D, F, U, H1, H2, heads, m))) return rc;
  if (C < 0) return fail(MANNER_HIP_E_INVALID, "%s: bad shape C=%lld", who, (long long)C);
  if (B * std::max<int64_t>(C, 1) > 0x7fffffffll || B * std::max<int64_t>(C, 1) * S > 0x7fffffffll || C * S * heads > 0x7fffffffll)
    return fail(MANNER_HIP_E_INVALID, "%s: B*C*S or C*S*heads exceeds the grid (below 2^31)", who);
  m = Dims{B * C, S, B * C * S, D, F, U, H1, H2, heads};
  return MANNER_HIP_OK;
}
struct WorkAll { Work w; float *dall2, *dcd2, *wt, *mpart; };
void plan_work_all(FloatBump& b, WorkAll& a, const Dims& m) {
  const size_t R = (size_t)m.R, P = (size_t)m.B;
  plan_work_rows(b, a.w, m);
  a.w.part = nullptr;
  a.dall2 = b.take(R * m.U);
  a.dcd2 = b.take(P * m.D);
  a.wt = b.take(std::max({(size_t)m.F * 4 * m.D, (size_t)m.U * 2 * m.D, (size_t)3 * m.U * m.U, (size_t)m.U * (m.F + m.U), (size_t)m.H1 * m.U,
                          (size_t)m.H1 * m.D, (size_t)m.H2 * m.H1}));
  const int FU = m.F + m.U;
  a.mpart = b.take(std::max({mw_part_floats(m.R, m.H2, 1), mw_part_floats(m.R, m.H1, m.H2), mw_part_floats(m.R, m.U, m.H1),
                             mw_part_floats(m.B, m.D, m.H1), mw_part_floats(m.R, FU, m.U), mw_part_floats(m.R, m.U, m.U),
                             mw_part_floats(m.R, m.U, 3 * m.U), mw_part_floats(m.R, 2 * m.D, m.U), mw_part_floats(m.R, 4 * m.D, m.F)}));
}

}  // namespace

// launch_wlin and launch_mdx for the other translation units (declared in common.h): flat rows, no per-(user, column) terms
int wlin_f32(bool tanh_act, const float* x, int ldx, const float* W, int ldw, const float* bias, int64_t R, int K, int O, float* y, int ldy,
             hipStream_t s) {
  return launch_wlin(tanh_act, x, ldx, W, ldw, bias, nullptr, nullptr, RowMap{1, 1, 1, 0}, R, K, O, y, ldy, s);
}
int wlin_dx_f32(const float* dy, int ldy, const float* W, int ldw, int64_t R, int K, int O, float* dx, float* wt, hipStream_t s) {
  return launch_mdx(dy, ldy, W, ldw, R, K, O, nullptr, nullptr, dx, wt, s);
}
}  // namespace manner

using namespace manner;

extern "C" {

int manner_hip_relu(const float* x, float* out, int64_t n, manner_hip_stream_t stream) {
  if (n == 0) return MANNER_HIP_OK;
  if (n < 0 || !x || !out) return fail(MANNER_HIP_E_INVALID, "relu: bad argument");
  hipLaunchKernelGGL(relu_kernel, dim3(flat_grid(n)), dim3(CA_BLOCK), 0, (hipStream_t)stream, x, (const float*)nullptr, out, n);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_relu_backward(const float* x, const float* grad_out, float* grad_x, int64_t n, manner_hip_stream_t stream) {
  if (n == 0) return MANNER_HIP_OK;
  if (n < 0 || !x || !grad_out || !grad_x) return fail(MANNER_HIP_E_INVALID, "relu_backward: bad argument");
  hipLaunchKernelGGL(relu_kernel, dim3(flat_grid(n)), dim3(CA_BLOCK), 0, (hipStream_t)stream, x, grad_out, grad_x, n);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_linear_tanh(const float* x, const float* weight, const float* bias, int64_t R, int32_t K, int32_t O, float* y,
                           manner_hip_stream_t stream) {
  if (R < 0 || K <= 0 || O <= 0 || R > 0x7fffffffll || O > 65535 * LIN_ROWS_OT) return fail(MANNER_HIP_E_INVALID, "linear_tanh: bad shape");
  if (R == 0) return MANNER_HIP_OK;
  if (!x || !weight || !y) return fail(MANNER_HIP_E_INVALID, "linear_tanh: null pointer");
  return launch_lin_rows(true, x, weight, K, bias, nullptr, 1, R, K, O, y, O, nullptr, (hipStream_t)stream);
}

int manner_hip_tanh_backward(const float* y, const float* grad_out, float* grad_pre, int64_t n, manner_hip_stream_t stream) {
  if (n == 0) return MANNER_HIP_OK;
  if (n < 0 || !y || !grad_out || !grad_pre) return fail(MANNER_HIP_E_INVALID, "tanh_backward: bad argument");
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(flat_grid(n)), dim3(CA_BLOCK), 0, (hipStream_t)stream, y, grad_out, grad_pre, n);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_axis0_attention_any(const float* qkv, int64_t L0, int64_t B1, int32_t E, int32_t heads, float* out, float* stats,
                                   manner_hip_stream_t stream) {
  int rc;
  if ((rc = a0any_check("axis0_attention_any", L0, B1, E, heads))) return rc;
  if (L0 == 0 || B1 == 0) return MANNER_HIP_OK;
  if (!qkv || !out) return fail(MANNER_HIP_E_INVALID, "axis0_attention_any: null pointer");
  return launch_a0any_fwd(qkv, out, stats, L0, B1, E, heads, (hipStream_t)stream);
}

int manner_hip_axis0_attention_any_backward_q(const float* qkv, const float* out, const float* grad_out, int64_t L0, int64_t B1, int32_t E,
                                              int32_t heads, float* grad_qkv, float* stats, manner_hip_stream_t stream) {
  int rc;
  if ((rc = a0any_check("axis0_attention_any_backward_q", L0, B1, E, heads))) return rc;
  if (L0 == 0 || B1 == 0) return MANNER_HIP_OK;
  if (!qkv || !out || !grad_out || !grad_qkv || !stats) return fail(MANNER_HIP_E_INVALID, "axis0_attention_any_backward_q: null pointer");
  return launch_a0any_bwd_q(qkv, out, grad_out, grad_qkv, stats, L0, B1, E, heads, (hipStream_t)stream);
}

int manner_hip_axis0_attention_any_backward_kv(const float* qkv, const float* grad_out, const float* stats, int64_t L0, int64_t B1, int32_t E,
                                               int32_t heads, float* grad_qkv, manner_hip_stream_t stream) {
  int rc;
  if ((rc = a0any_check("axis0_attention_any_backward_kv", L0, B1, E, heads))) return rc;
  if (L0 == 0 || B1 == 0) return MANNER_HIP_OK;
  if (!qkv || !grad_out || !grad_qkv || !stats) return fail(MANNER_HIP_E_INVALID, "axis0_attention_any_backward_kv: null pointer");
  return launch_a0any_bwd_kv(qkv, grad_out, stats, grad_qkv, L0, B1, E, heads, (hipStream_t)stream);
}

size_t manner_hip_caum_user_saved_bytes(int64_t B, int64_t S, int32_t D, int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads) {
  if (B <= 0 || S <= 0 || D <= 0 || F <= 0 || U <= 0 || H1 <= 0 || H2 <= 0 || heads <= 0) return 0;
  const Dims m{B, S, B * S, D, F, U, H1, H2, heads};
  FloatBump b(nullptr);
  Saved s;
  plan_saved(b, s, m);
  return b.off * sizeof(float) + 256;
}

int manner_hip_caum_user_forward(const float* x, const float* c, int64_t c_stride, const float* const* params, int64_t B, int64_t S, int32_t D,
                                 int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads, float p, uint64_t seed, uint32_t site0, float* out,
                                 void* saved, size_t saved_bytes, manner_hip_stream_t stream) {
  int rc;
  Dims m;
  if ((rc = caum_check("caum_user", B, S, D, F, U, H1, H2, heads, m))) return rc;
  if (!(p >= 0.f && p < 1.f)) return fail(MANNER_HIP_E_INVALID, "caum_user: p=%f outside [0, 1)", p);
  if (B == 0) return MANNER_HIP_OK;
  if (!x || !c || !params || !out || !saved) return fail(MANNER_HIP_E_INVALID, "caum_user: null pointer");
  for (int i = 0; i < P_COUNT; ++i)
    if (!params[i]) return fail(MANNER_HIP_E_INVALID, "caum_user: null parameter %d", i);
  if (c_stride < D) return fail(MANNER_HIP_E_INVALID, "caum_user: candidate row stride %lld < D=%d", (long long)c_stride, D);
  if (saved_bytes < manner_hip_caum_user_saved_bytes(B, S, D, F, U, H1, H2, heads)) return fail(MANNER_HIP_E_WORKSPACE, "caum_user: saved buffer too small");
  hipStream_t s = (hipStream_t)stream;
  FloatBump bump(saved);
  Saved sv;
  plan_saved(bump, sv, m);
  const int64_t R = m.R;
  const int FU = F + U, Si = (int)S;
  const Drop d1 = make_drop(seed, site0, p), d2 = make_drop(seed, site0 + 1, p), d3 = make_drop(seed, site0 + 2, p);
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)R), dim3(CA_BLOCK), 0, s, x, c, c_stride, Si, D, d1, d2, sv.a1, sv.a2, sv.cd);
  MANNER_LAUNCH_CHECK();
  // candi-cnn into cat[:, :F]; candi-selfatt: Linear, in-projection, attention along B, out-projection into cat[:, F:]
  if ((rc = launch_lin_rows(false, sv.a1, params[P_W1], 4 * D, params[P_B1], nullptr, 1, R, 4 * D, F, sv.cat, FU, nullptr, s))) return rc;
  if ((rc = launch_lin_rows(false, sv.a2, params[P_W2], 2 * D, params[P_B2], nullptr, 1, R, 2 * D, U, sv.h2, U, nullptr, s))) return rc;
  if ((rc = launch_lin_rows(false, sv.h2, params[P_WIN], U, params[P_BIN], nullptr, 1, R, U, 3 * U, sv.qkv, 3 * U, nullptr, s))) return rc;
  if ((rc = launch_a0any_fwd(sv.qkv, sv.att, sv.stats, B, S, U, heads, s))) return rc;
  if ((rc = launch_lin_rows(false, sv.att, params[P_WOUT], U, params[P_BOUT], nullptr, 1, R, U, U, sv.cat + F, FU, nullptr, s))) return rc;
  if (p > 0.f) {
    hipLaunchKernelGGL(drop_inplace_kernel, dim3(flat_grid(R * FU)), dim3(CA_BLOCK), 0, s, sv.cat, R * FU, d3);
    MANNER_LAUNCH_CHECK();
  }
  if ((rc = launch_lin_rows(false, sv.cat, params[P_W3], FU, params[P_B3], nullptr, 1, R, FU, U, sv.all, U, nullptr, s))) return rc;
  // candi-att: the candidate half of dense_att.linear once per user, then the two tanh layers over the rows
  if ((rc = launch_lin_rows(false, sv.cd, params[P_WA] + U, 2 * U, params[P_BA], nullptr, 1, B, D, H1, sv.ct, H1, nullptr, s))) return rc;
  if ((rc = launch_lin_rows(true, sv.all, params[P_WA], 2 * U, nullptr, sv.ct, Si, R, U, H1, sv.t1, H1, sv.d1, s))) return rc;
  if ((rc = launch_lin_rows(true, sv.t1, params[P_WB], H1, params[P_BB], nullptr, 1, R, H1, H2, sv.t2, H2, sv.d2, s))) return rc;
  hipLaunchKernelGGL(score_kernel, dim3((unsigned)((R + CA_ROWS - 1) / CA_ROWS)), dim3(CA_BLOCK), 0, s, sv.t2, params[P_WC], params[P_BC], sv.all, sv.cd, R,
                     Si, H2, U, sv.score, sv.g);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(user_kernel, dim3((unsigned)((B + CA_WAVES - 1) / CA_WAVES)), dim3(CA_BLOCK), 0, s, sv.score, sv.g, B, Si, out, (const float*)nullptr,
                     (float*)nullptr, (float*)nullptr);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

size_t manner_hip_caum_user_backward_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads) {
  if (B <= 0 || S <= 0 || D <= 0 || F <= 0 || U <= 0 || H1 <= 0 || H2 <= 0 || heads <= 0) return 0;
  const Dims m{B, S, B * S, D, F, U, H1, H2, heads};
  FloatBump b(nullptr);
  Work w;
  plan_work(b, w, m);
  return b.off * sizeof(float) + 256;
}

int manner_hip_caum_user_backward(const float* const* params, const float* grad_out, int64_t B, int64_t S, int32_t D, int32_t F, int32_t U,
                                  int32_t H1, int32_t H2, int32_t heads, float p, uint64_t seed, uint32_t site0, void* saved, size_t saved_bytes,
                                  float* grad_x, float* grad_c, float* const* grads, void* workspace, size_t workspace_bytes,
                                  manner_hip_stream_t stream) {
  int rc;
  Dims m;
  if ((rc = caum_check("caum_user_backward", B, S, D, F, U, H1, H2, heads, m))) return rc;
  if (!(p >= 0.f && p < 1.f)) return fail(MANNER_HIP_E_INVALID, "caum_user_backward: p=%f outside [0, 1)", p);
  if (!params || !grads) return fail(MANNER_HIP_E_INVALID, "caum_user_backward: null pointer");
  for (int i = 0; i < P_COUNT; ++i)
    if (!params[i] || !grads[i]) return fail(MANNER_HIP_E_INVALID, "caum_user_backward: null parameter or gradient %d", i);
  hipStream_t s = (hipStream_t)stream;
  const int FU = F + U, Si = (int)S;
  const size_t sizes[P_COUNT] = {(size_t)F * 4 * D, (size_t)F, (size_t)U * 2 * D, (size_t)U, (size_t)3 * U * U, (size_t)3 * U, (size_t)U * U, (size_t)U,
                                 (size_t)U * FU, (size_t)U, (size_t)H1 * 2 * U, (size_t)H1, (size_t)H2 * H1, (size_t)H2, (size_t)H2, 1};
  if (B == 0) {                                    // no user: the parameter gradients are sums over nothing
    for (int i = 0; i < P_COUNT; ++i) MANNER_HIP_TRY(hipMemsetAsync(grads[i], 0, sizes[i] * sizeof(float), s));
    return MANNER_HIP_OK;
  }
  if (!grad_out || !saved || !grad_x || !grad_c || !workspace) return fail(MANNER_HIP_E_INVALID, "caum_user_backward: null pointer");
  if (saved_bytes < manner_hip_caum_user_saved_bytes(B, S, D, F, U, H1, H2, heads)) return fail(MANNER_HIP_E_WORKSPACE, "caum_user_backward: saved buffer too small");
  if (workspace_bytes < manner_hip_caum_user_backward_workspace_bytes(B, S, D, F, U, H1, H2, heads))
    return fail(MANNER_HIP_E_WORKSPACE, "caum_user_backward: workspace too small");
  FloatBump bs(saved), bw(workspace);
  Saved sv;
  Work w;
  plan_saved(bs, sv, m);
  plan_work(bw, w, m);
  const int64_t R = m.R;
  const Drop d1 = make_drop(seed, site0, p), d2 = make_drop(seed, site0 + 1, p), d3 = make_drop(seed, site0 + 2, p);
  const unsigned row_tiles = (unsigned)((R + CA_ROWS - 1) / CA_ROWS);
  // the final dot, the weighted sum and the softmax: ds (d score), wq (the weight of cd[b] in d all)
  hipLaunchKernelGGL(user_kernel, dim3((unsigned)((B + CA_WAVES - 1) / CA_WAVES)), dim3(CA_BLOCK), 0, s, sv.score, sv.g, B, Si, (float*)nullptr, grad_out,
                     w.ds, w.wq);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(tail_rows_kernel, dim3(row_tiles), dim3(CA_BLOCK), 0, s, w.ds, w.wq, params[P_WC], sv.d2, sv.cd, R, Si, H2, U, w.dt2, w.dall);
  MANNER_LAUNCH_CHECK();
  // dense_att.linear3: d wc = sum_r ds[r] t2[r]; d bc is zero in exact arithmetic (the softmax is shift-invariant)
  if ((rc = launch_wgrad_rows(w.ds, 1, sv.t2, R, H2, 1, w.part, grads[P_WC], H2, s))) return rc;
  MANNER_HIP_TRY(hipMemsetAsync(grads[P_BC], 0, sizeof(float), s));
  // dense_att.linear2
  if ((rc = launch_wgrad_rows(w.dt2, H2, sv.t1, R, H1, H2, w.part, grads[P_WB], H1, s))) return rc;
  if ((rc = launch_colsum_rows(w.dt2, H2, R, H2, grads[P_BB], s))) return rc;
  if ((rc = launch_dx_rows(w.dt2, H2, params[P_WB], H1, R, H1, H2, nullptr, sv.d1, w.dt1, s))) return rc;
  // dense_att.linear: the history half over the rows, the candidate half over the users (d ct[b] = sum_s d t1[b, s])
  if ((rc = launch_wgrad_rows(w.dt1, H1, sv.all, R, U, H1, w.part, grads[P_WA], 2 * U, s))) return rc;
  if ((rc = launch_colsum_rows(w.dt1, H1, R, H1, grads[P_BA], s))) return rc;
  if ((rc = launch_dx_rows(w.dt1, H1, params[P_WA], 2 * U, R, U, H1, w.dall, nullptr, w.dall, s))) return rc;
  hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)B, (unsigned)((H1 + CA_BLOCK - 1) / CA_BLOCK)), dim3(CA_BLOCK), 0, s, (const float*)nullptr, w.dt1, H1, 0,
                     (const float*)nullptr, 0, (const float*)nullptr, Si, H1, d1, false, w.dct);
  MANNER_LAUNCH_CHECK();
  if ((rc = launch_wgrad_rows(w.dct, H1, sv.cd, B, D, H1, w.part, grads[P_WA] + U, 2 * U, s))) return rc;
  // d cd[b] = dout[b] user[b] + d ct[b] Wa[:, U:] (the window and self-attention routes are added at the end)
  hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)B, (unsigned)((U + CA_BLOCK - 1) / CA_BLOCK)), dim3(CA_BLOCK), 0, s, w.wq, sv.all, U, 0, (const float*)nullptr, 0,
                     (const float*)nullptr, Si, U, d1, false, w.dcd);
  MANNER_LAUNCH_CHECK();
  if ((rc = launch_dx_rows(w.dct, H1, params[P_WA] + U, 2 * U, B, D, H1, w.dcd, nullptr, w.dcd, s))) return rc;
  // linear3 and dropout3
  if ((rc = launch_wgrad_rows(w.dall, U, sv.cat, R, FU, U, w.part, grads[P_W3], FU, s))) return rc;
  if ((rc = launch_colsum_rows(w.dall, U, R, U, grads[P_B3], s))) return rc;
  if ((rc = launch_dx_rows(w.dall, U, params[P_W3], FU, R, FU, U, nullptr, nullptr, w.dcat, s))) return rc;
  if (p > 0.f) {
    hipLaunchKernelGGL(drop_inplace_kernel, dim3(flat_grid(R * FU)), dim3(CA_BLOCK), 0, s, w.dcat, R * FU, d3);
    MANNER_LAUNCH_CHECK();
  }
  // candi-selfatt: out-projection, attention, in-projection, linear2
  if ((rc = launch_wgrad_rows(w.dcat + F, FU, sv.att, R, U, U, w.part, grads[P_WOUT], U, s))) return rc;
  if ((rc = launch_colsum_rows(w.dcat + F, FU, R, U, grads[P_BOUT], s))) return rc;
  if ((rc = launch_dx_rows(w.dcat + F, FU, params[P_WOUT], U, R, U, U, nullptr, nullptr, w.datt, s))) return rc;
  if ((rc = launch_a0any_bwd_q(sv.qkv, sv.att, w.datt, w.dqkv, sv.stats, B, S, U, heads, s))) return rc;
  if ((rc = launch_a0any_bwd_kv(sv.qkv, w.datt, sv.stats, w.dqkv, B, S, U, heads, s))) return rc;
  if ((rc = launch_wgrad_rows(w.dqkv, 3 * U, sv.h2, R, U, 3 * U, w.part, grads[P_WIN], U, s))) return rc;
  if ((rc = launch_colsum_rows(w.dqkv, 3 * U, R, 3 * U, grads[P_BIN], s))) return rc;
  // the K third of d in_proj_bias is zero in exact arithmetic (a shift of every key moves every logit of a row alike)
  MANNER_HIP_TRY(hipMemsetAsync(grads[P_BIN] + U, 0, (size_t)U * sizeof(float), s));
  if ((rc = launch_dx_rows(w.dqkv, 3 * U, params[P_WIN], U, R, U, 3 * U, nullptr, nullptr, w.dh2, s))) return rc;
  if ((rc = launch_wgrad_rows(w.dh2, U, sv.a2, R, 2 * D, U, w.part, grads[P_W2], 2 * D, s))) return rc;
  if ((rc = launch_colsum_rows(w.dh2, U, R, U, grads[P_B2], s))) return rc;
  if ((rc = launch_dx_rows(w.dh2, U, params[P_W2], 2 * D, R, 2 * D, U, nullptr, nullptr, w.da2, s))) return rc;
  // candi-cnn: linear1 from cat[:, :F]
  if ((rc = launch_wgrad_rows(w.dcat, FU, sv.a1, R, 4 * D, F, w.part, grads[P_W1], 4 * D, s))) return rc;
  if ((rc = launch_colsum_rows(w.dcat, FU, R, F, grads[P_B1], s))) return rc;
  if ((rc = launch_dx_rows(w.dcat, FU, params[P_W1], 4 * D, R, 4 * D, F, nullptr, nullptr, w.da1, s))) return rc;
  // d x: the three windows and the self-attention operand; d c: the sums over the slots, through dropout1
  hipLaunchKernelGGL(window_dx_kernel, dim3((unsigned)R), dim3(CA_BLOCK), 0, s, w.da1, w.da2, Si, D, d2, grad_x);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)B, (unsigned)((D + CA_BLOCK - 1) / CA_BLOCK)), dim3(CA_BLOCK), 0, s, (const float*)nullptr, w.da1, 4 * D, 3 * D, w.da2,
                     2 * D, w.dcd, Si, D, d1, true, grad_c);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

size_t manner_hip_caum_scores_all_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D, int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads,
                                                  int64_t cols_per_pass) {
  if (B <= 0 || S <= 0 || C <= 0 || D <= 0 || F <= 0 || U <= 0 || H1 <= 0 || H2 <= 0 || heads <= 0 || cols_per_pass <= 0) return 0;
  const Dims m{B, S, B * S, D, F, U, H1, H2, heads};
  return all_bytes(m, C, std::min(cols_per_pass, all_max_cols(m, C)));
}

// CAUMPLMModule.forward's candidate loop in one call, eval(): out[b, c] = CAUMUserEncoder.forward(x, cand[:, c, :])[b].
//   once over the B S rows:  WX = W1[:, :3D] window + b1, HX = W2[:, D:] x + b2, QH = Win HX + bin, A = W3[:, :F] WX + (W3[:, F:] bout + b3)
//   once over the B C rows:  CX1 = W1[:, 3D:] c, CX2 = W2[:, :D] c, QC = Win CX2, Bc = W3[:, :F] CX1, CT = Wa[:, U:] c + ba
//   once per call:           M = W3[:, F:] Wout
//   per pass of columns, over its B cp S rows: att (q | k | v = QH + QC), all = M att + A + Bc, t1 = tanh(Wa[:, :U] all + CT),
//   t2 = tanh(Wb t1 + bb), then score_kernel / user_kernel with (b, c) as pseudo-users.
// The columns per pass follow from workspace_bytes; a column's bits do not depend on it.
int manner_hip_caum_scores_all(const float* x, const float* cand, const float* const* params, int64_t B, int64_t S, int64_t C, int32_t D, int32_t F,
                               int32_t U, int32_t H1, int32_t H2, int32_t heads, float* out, void* workspace, size_t workspace_bytes,
                               manner_hip_stream_t stream) {
  int rc;
  Dims m;
  if ((rc = caum_all_check("caum_scores_all", B, S, C, D, F, U, H1, H2, heads, m))) return rc;
  if (B == 0 || C == 0) return MANNER_HIP_OK;
  if (!x || !cand || !params || !out || !workspace) return fail(MANNER_HIP_E_INVALID, "caum_scores_all: null pointer");
  for (int i = 0; i < P_COUNT; ++i)
    if (!params[i]) return fail(MANNER_HIP_E_INVALID, "caum_scores_all: null parameter %d", i);
  if (workspace_bytes < all_bytes(m, C, 1))
    return fail(MANNER_HIP_E_WORKSPACE, "caum_scores_all: workspace too small (%zu bytes hold one column)", all_bytes(m, C, 1));
  int64_t cp = 1, hi = all_max_cols(m, C);                 // the most columns whose wide rows fit
  while (cp < hi) {
    const int64_t mid = (cp + hi + 1) / 2;
    if (all_bytes(m, C, mid) <= workspace_bytes) cp = mid; else hi = mid - 1;
  }
  const int64_t passes = (C + cp - 1) / cp;
  cp = (C + passes - 1) / passes;                          // as many passes, of even width (no last pass of one column)
  hipStream_t s = (hipStream_t)stream;
  FloatBump bump(workspace);
  AllBufs w;
  plan_all(bump, w, m, C, cp);
  const int64_t R = m.R, N = B * C;
  const int FU = F + U, Si = (int)S;
  const RowMap flat{1, 1, 1, 0};
  const float* const none = nullptr;
  hipLaunchKernelGGL(window_kernel, dim3((unsigned)R), dim3(CA_BLOCK), 0, s, x, Si, D, w.win);
  MANNER_LAUNCH_CHECK();
  if ((rc = launch_wlin(false, w.win, 3 * D, params[P_W1], 4 * D, params[P_B1], none, none, flat, R, 3 * D, F, w.wx, F, s))) return rc;
  if ((rc = launch_wlin(false, x, D, params[P_W2] + D, 2 * D, params[P_B2], none, none, flat, R, D, U, w.hx, U, s))) return rc;
  if ((rc = launch_wlin(false, w.hx, U, params[P_WIN], U, params[P_BIN], none, none, flat, R, U, 3 * U, w.qh, 3 * U, s))) return rc;
  hipLaunchKernelGGL(transpose_square_kernel, dim3((unsigned)(((int64_t)U * U + CA_BLOCK - 1) / CA_BLOCK)), dim3(CA_BLOCK), 0, s, params[P_WOUT], U, w.owt);
  MANNER_LAUNCH_CHECK();
  if ((rc = launch_wlin(false, params[P_W3] + F, FU, w.owt, U, none, none, none, flat, U, U, U, w.fold, U, s))) return rc;
  if ((rc = launch_wlin(false, params[P_BOUT], U, params[P_W3] + F, FU, params[P_B3], none, none, flat, 1, U, U, w.ba, U, s))) return rc;
  if ((rc = launch_wlin(false, w.wx, F, params[P_W3], FU, w.ba, none, none, flat, R, F, U, w.a, U, s))) return rc;
  if ((rc = launch_wlin(false, cand, D, params[P_W1] + 3 * D, 4 * D, none, none, none, flat, N, D, F, w.cx1, F, s))) return rc;
  if ((rc = launch_wlin(false, cand, D, params[P_W2], 2 * D, none, none, none, flat, N, D, U, w.cx2, U, s))) return rc;
  if ((rc = launch_wlin(false, w.cx2, U, params[P_WIN], U, none, none, none, flat, N, U, 3 * U, w.qc, 3 * U, s))) return rc;
  if ((rc = launch_wlin(false, w.cx1, F, params[P_W3], FU, none, none, none, flat, N, F, U, w.bcand, U, s))) return rc;
  if ((rc = launch_wlin(false, cand, D, params[P_WA] + U, 2 * U, params[P_BA], none, none, flat, N, D, H1, w.ct, H1, s))) return rc;
  for (int64_t c0 = 0; c0 < C; c0 += cp) {
    const int64_t n = std::min(cp, C - c0), P = B * n, rows = P * S;
    const RowMap rm{Si, (int)n, (int)C, (int)c0};
    if ((rc = launch_a0sum_fwd(w.qh, w.qc, w.att, B, rm, U, heads, s))) return rc;
    if ((rc = launch_wlin(false, w.att, U, w.fold, U, none, w.a, w.bcand, rm, rows, U, U, w.all, U, s))) return rc;
    if ((rc = launch_wlin(true, w.all, U, params[P_WA], 2 * U, none, none, w.ct, rm, rows, U, H1, w.t1, H1, s))) return rc;
    if ((rc = launch_wlin(true, w.t1, H1, params[P_WB], H1, params[P_BB], none, none, rm, rows, H1, H2, w.t2, H2, s))) return rc;
    const bool whole = n == C;
    if (!whole) {
      hipLaunchKernelGGL(rows_copy_kernel, dim3(flat_grid(P * D)), dim3(CA_BLOCK), 0, s, cand + c0 * D, C * D, w.cd, n * D, n * D, P * D);
      MANNER_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)((rows + CA_ROWS - 1) / CA_ROWS)), dim3(CA_BLOCK), 0, s, w.t2, params[P_WC], params[P_BC], w.all,
                       whole ? cand : w.cd, rows, Si, H2, U, w.score, w.g);
    MANNER_LAUNCH_CHECK();
    hipLaunchKernelGGL(user_kernel, dim3((unsigned)((P + CA_WAVES - 1) / CA_WAVES)), dim3(CA_BLOCK), 0, s, w.score, w.g, P, Si, whole ? out : w.outp,
                       (const float*)nullptr, (float*)nullptr, (float*)nullptr);
    MANNER_LAUNCH_CHECK();
    if (!whole) {
      hipLaunchKernelGGL(rows_copy_kernel, dim3(flat_grid(P)), dim3(CA_BLOCK), 0, s, w.outp, n, out + c0, C, n, P);
      MANNER_LAUNCH_CHECK();
    }
  }
  return MANNER_HIP_OK;
}

size_t manner_hip_wgrad_rows_f32_workspace_bytes(int64_t R, int32_t K, int32_t O) {
  if (R <= 0 || K <= 0 || O <= 0) return 0;
  return mw_part_floats(R, K, O) * sizeof(float);
}

int manner_hip_wgrad_rows_f32(const float* dy, int32_t ldy, const float* x, int32_t ldx, int64_t R, int32_t K, int32_t O, float* dW, int32_t ldo,
                              void* workspace, size_t workspace_bytes, manner_hip_stream_t stream) {
  if (R < 0 || K <= 0 || O <= 0 || ldy < O || ldx < K || ldo < K || R > 0x7fffffffll || O > 65535 * 32)
    return fail(MANNER_HIP_E_INVALID, "wgrad_rows_f32: bad shape R=%lld K=%d O=%d ldy=%d ldx=%d ldo=%d", (long long)R, K, O, ldy, ldx, ldo);
  if (!dW) return fail(MANNER_HIP_E_INVALID, "wgrad_rows_f32: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (R == 0) {                                    // a sum over nothing
    MANNER_HIP_TRY(hipMemset2DAsync(dW, (size_t)ldo * sizeof(float), 0, (size_t)K * sizeof(float), (size_t)O, s));
    return MANNER_HIP_OK;
  }
  if (!dy || !x) return fail(MANNER_HIP_E_INVALID, "wgrad_rows_f32: null pointer");
  const size_t need = mw_part_floats(R, K, O) * sizeof(float);
  if (need && (!workspace || workspace_bytes < need)) return fail(MANNER_HIP_E_WORKSPACE, "wgrad_rows_f32: workspace too small (%zu bytes)", need);
  return launch_mwgrad(dy, ldy, x, ldx, R, K, O, static_cast<float*>(workspace), dW, ldo, s);
}

size_t manner_hip_caum_train_all_saved_bytes(int64_t B, int64_t S, int64_t C, int32_t D, int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads) {
  if (B <= 0 || S <= 0 || C <= 0 || D <= 0 || F <= 0 || U <= 0 || H1 <= 0 || H2 <= 0 || heads <= 0) return 0;
  const Dims m{B * C, S, B * C * S, D, F, U, H1, H2, heads};
  FloatBump b(nullptr);
  Saved s;
  plan_saved(b, s, m);
  return b.off * sizeof(float) + 256;
}

int manner_hip_caum_train_all_forward(const float* x, const float* cand, const float* const* params, int64_t B, int64_t S, int64_t C, int32_t D,
                                      int32_t F, int32_t U, int32_t H1, int32_t H2, int32_t heads, float p, const uint64_t* seeds, uint32_t site0,
                                      float* scores, void* saved, size_t saved_bytes, manner_hip_stream_t stream) {
  int rc;
  Dims m;
  if ((rc = caum_train_all_check("caum_train_all", B, S, C, D, F, U, H1, H2, heads, m))) return rc;
  if (!(p >= 0.f && p < 1.f)) return fail(MANNER_HIP_E_INVALID, "caum_train_all: p=%f outside [0, 1)", p);
  if (B == 0 || C == 0) return MANNER_HIP_OK;
  if (!x || !cand || !params || !scores || !saved || (p > 0.f && !seeds)) return fail(MANNER_HIP_E_INVALID, "caum_train_all: null pointer");
  for (int i = 0; i < P_COUNT; ++i)
    if (!params[i]) return fail(MANNER_HIP_E_INVALID, "caum_train_all: null parameter %d", i);
  if (saved_bytes < manner_hip_caum_train_all_saved_bytes(B, S, C, D, F, U, H1, H2, heads)) return fail(MANNER_HIP_E_WORKSPACE, "caum_train_all: saved buffer too small");
  hipStream_t s = (hipStream_t)stream;
  FloatBump bump(saved);
  Saved sv;
  plan_saved(bump, sv, m);
  const int64_t R = m.R, P = m.B;
  const int FU = F + U, Si = (int)S, Ci = (int)C;
  const Drop d1 = make_drop(0, site0, p), d2 = make_drop(0, site0 + 1, p), d3 = make_drop(0, site0 + 2, p);      // the seed is the column's
  const RowMap flat{1, 1, 1, 0}, wide{Si, Ci, Ci, 0};
  const float* const none = nullptr;
  hipLaunchKernelGGL(pack_cols_kernel, dim3((unsigned)R), dim3(CA_BLOCK), 0, s, x, cand, Si, Ci, D, d1, d2, seeds, sv.a1, sv.a2, sv.cd);
  MANNER_LAUNCH_CHECK();
  // candi-cnn into cat[:, :F]; candi-selfatt: Linear, in-projection, attention along B per (column, slot, head), out-projection into cat[:, F:]
  if ((rc = launch_wlin(false, sv.a1, 4 * D, params[P_W1], 4 * D, params[P_B1], none, none, flat, R, 4 * D, F, sv.cat, FU, s))) return rc;
  if ((rc = launch_wlin(false, sv.a2, 2 * D, params[P_W2], 2 * D, params[P_B2], none, none, flat, R, 2 * D, U, sv.h2, U, s))) return rc;
  if ((rc = launch_wlin(false, sv.h2, U, params[P_WIN], U, params[P_BIN], none, none, flat, R, U, 3 * U, sv.qkv, 3 * U, s))) return rc;
  if ((rc = launch_a0any_fwd(sv.qkv, sv.att, sv.stats, B, C * S, U, heads, s))) return rc;
  if ((rc = launch_wlin(false, sv.att, U, params[P_WOUT], U, params[P_BOUT], none, none, flat, R, U, U, sv.cat + F, FU, s))) return rc;
  if (p > 0.f) {
    hipLaunchKernelGGL(drop_cols_kernel, dim3(flat_grid(R * FU)), dim3(CA_BLOCK), 0, s, sv.cat, R * FU, Si, Ci, FU, d3, seeds);
    MANNER_LAUNCH_CHECK();
  }
  if ((rc = launch_wlin(false, sv.cat, FU, params[P_W3], FU, params[P_B3], none, none, flat, R, FU, U, sv.all, U, s))) return rc;
  // candi-att: the candidate half of dense_att.linear once per (user, column), then the two tanh layers over the rows
  if ((rc = launch_wlin(false, sv.cd, D, params[P_WA] + U, 2 * U, params[P_BA], none, none, flat, P, D, H1, sv.ct, H1, s))) return rc;
  if ((rc = launch_wlin(true, sv.all, U, params[P_WA], 2 * U, none, none, sv.ct, wide, R, U, H1, sv.t1, H1, s, sv.d1))) return rc;
  if ((rc = launch_wlin(true, sv.t1, H1, params[P_WB], H1, params[P_BB], none, none, flat, R, H1, H2, sv.t2, H2, s, sv.d2))) return rc;
  hipLaunchKernelGGL(score_kernel, dim3((unsigned)((R + CA_ROWS - 1) / CA_ROWS)), dim3(CA_BLOCK), 0, s, sv.t2, params[P_WC], params[P_BC], sv.all, sv.cd, R,
                     Si, H2, U, sv.score, sv.g);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(user_kernel, dim3((unsigned)((P + CA_WAVES - 1) / CA_WAVES)), dim3(CA_BLOCK), 0, s, sv.score, sv.g, P, Si, scores, (const float*)nullptr,
                     (float*)nullptr, (float*)nullptr);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

size_t manner_hip_caum_train_all_backward_workspace_bytes(int64_t B, int64_t S, int64_t C, int32_t D, int32_t F, int32_t U, int32_t H1, int32_t H2,
                                                          int32_t heads) {
  if (B <= 0 || S <= 0 || C <= 0 || D <= 0 || F <= 0 || U <= 0 || H1 <= 0 || H2 <= 0 || heads <= 0) return 0;
  const Dims m{B * C, S, B * C * S, D, F, U, H1, H2, heads};
  FloatBump b(nullptr);
  WorkAll w;
  plan_work_all(b, w, m);
  return b.off * sizeof(float) + 256;
}

int manner_hip_caum_train_all_backward(const float* const* params, const float* grad_scores, int64_t B, int64_t S, int64_t C, int32_t D, int32_t F,
                                       int32_t U, int32_t H1, int32_t H2, int32_t heads, float p, const uint64_t* seeds, uint32_t site0, void* saved,
                                       size_t saved_bytes, float* grad_x, float* grad_cand, float* const* grads, void* workspace,
                                       size_t workspace_bytes, manner_hip_stream_t stream) {
  int rc;
  Dims m;
  if ((rc = caum_train_all_check("caum_train_all_backward", B, S, C, D, F, U, H1, H2, heads, m))) return rc;
  if (!(p >= 0.f && p < 1.f)) return fail(MANNER_HIP_E_INVALID, "caum_train_all_backward: p=%f outside [0, 1)", p);
  if (!params || !grads) return fail(MANNER_HIP_E_INVALID, "caum_train_all_backward: null pointer");
  for (int i = 0; i < P_COUNT; ++i)
    if (!params[i] || !grads[i]) return fail(MANNER_HIP_E_INVALID, "caum_train_all_backward: null parameter or gradient %d", i);
  hipStream_t s = (hipStream_t)stream;
  const int FU = F + U, Si = (int)S, Ci = (int)C;
  const size_t sizes[P_COUNT] = {(size_t)F * 4 * D, (size_t)F, (size_t)U * 2 * D, (size_t)U, (size_t)3 * U * U, (size_t)3 * U, (size_t)U * U, (size_t)U,
                                 (size_t)U * FU, (size_t)U, (size_t)H1 * 2 * U, (size_t)H1, (size_t)H2 * H1, (size_t)H2, (size_t)H2, 1};
  if (B == 0 || C == 0) {                          // no user or no column: the gradients are sums over nothing
    for (int i = 0; i < P_COUNT; ++i) MANNER_HIP_TRY(hipMemsetAsync(grads[i], 0, sizes[i] * sizeof(float), s));
    if (B > 0) {
      if (!grad_x) return fail(MANNER_HIP_E_INVALID, "caum_train_all_backward: null pointer");
      MANNER_HIP_TRY(hipMemsetAsync(grad_x, 0, (size_t)B * S * D * sizeof(float), s));
    }
    return MANNER_HIP_OK;
  }
  if (!grad_scores || !saved || !grad_x || !grad_cand || !workspace || (p > 0.f && !seeds))
    return fail(MANNER_HIP_E_INVALID, "caum_train_all_backward: null pointer");
  if (saved_bytes < manner_hip_caum_train_all_saved_bytes(B, S, C, D, F, U, H1, H2, heads))
    return fail(MANNER_HIP_E_WORKSPACE, "caum_train_all_backward: saved buffer too small");
  if (workspace_bytes < manner_hip_caum_train_all_backward_workspace_bytes(B, S, C, D, F, U, H1, H2, heads))
    return fail(MANNER_HIP_E_WORKSPACE, "caum_train_all_backward: workspace too small");
  FloatBump bs(saved), bw(workspace);
  Saved sv;
  WorkAll wa;
  plan_saved(bs, sv, m);
  plan_work_all(bw, wa, m);
  Work& w = wa.w;
  float* const part = wa.mpart;
  float* const wt = wa.wt;
  const int64_t R = m.R, P = m.B;
  const Drop d1 = make_drop(0, site0, p), d2 = make_drop(0, site0 + 1, p), d3 = make_drop(0, site0 + 2, p);
  const unsigned row_tiles = (unsigned)((R + CA_ROWS - 1) / CA_ROWS);
  // the final dot, the weighted sum and the softmax per (user, column): ds (d score), wq (the weight of cd[b, c] in d all)
  hipLaunchKernelGGL(user_kernel, dim3((unsigned)((P + CA_WAVES - 1) / CA_WAVES)), dim3(CA_BLOCK), 0, s, sv.score, sv.g, P, Si, (float*)nullptr, grad_scores,
                     w.ds, w.wq);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(tail_rows_kernel, dim3(row_tiles), dim3(CA_BLOCK), 0, s, w.ds, w.wq, params[P_WC], sv.d2, sv.cd, R, Si, H2, U, w.dt2, w.dall);
  MANNER_LAUNCH_CHECK();
  // dense_att.linear3: d wc = sum_r ds[r] t2[r]; d bc is zero in exact arithmetic (the softmax is shift-invariant)
  if ((rc = launch_wgrad_all(w.ds, 1, sv.t2, R, H2, 1, part, grads[P_WC], H2, s))) return rc;
  MANNER_HIP_TRY(hipMemsetAsync(grads[P_BC], 0, sizeof(float), s));
  // dense_att.linear2
  if ((rc = launch_wgrad_all(w.dt2, H2, sv.t1, R, H1, H2, part, grads[P_WB], H1, s))) return rc;
  if ((rc = launch_colsum_rows(w.dt2, H2, R, H2, grads[P_BB], s))) return rc;
  if ((rc = launch_mdx(w.dt2, H2, params[P_WB], H1, R, H1, H2, nullptr, sv.d1, w.dt1, wt, s))) return rc;
  // dense_att.linear: the history half over the rows, the candidate half over the (user, column) pairs (d ct[b, c] = sum_s d t1[b, c, s])
  if ((rc = launch_wgrad_all(w.dt1, H1, sv.all, R, U, H1, part, grads[P_WA], 2 * U, s))) return rc;
  if ((rc = launch_colsum_rows(w.dt1, H1, R, H1, grads[P_BA], s))) return rc;
  if ((rc = launch_mdx(w.dt1, H1, params[P_WA], 2 * U, R, U, H1, w.dall, nullptr, wa.dall2, wt, s))) return rc;
  hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)P, (unsigned)((H1 + CA_BLOCK - 1) / CA_BLOCK)), dim3(CA_BLOCK), 0, s, (const float*)nullptr, w.dt1, H1, 0,
                     (const float*)nullptr, 0, (const float*)nullptr, Si, H1, d1, false, w.dct);
  MANNER_LAUNCH_CHECK();
  if ((rc = launch_wgrad_all(w.dct, H1, sv.cd, P, D, H1, part, grads[P_WA] + U, 2 * U, s))) return rc;
  // d cd[b, c] = dout[b, c] user[b, c] + d ct[b, c] Wa[:, U:] (the window and self-attention routes are added at the end)
  hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)P, (unsigned)((U + CA_BLOCK - 1) / CA_BLOCK)), dim3(CA_BLOCK), 0, s, w.wq, sv.all, U, 0, (const float*)nullptr, 0,
                     (const float*)nullptr, Si, U, d1, false, w.dcd);
  MANNER_LAUNCH_CHECK();
  if ((rc = launch_mdx(w.dct, H1, params[P_WA] + U, 2 * U, P, D, H1, w.dcd, nullptr, wa.dcd2, wt, s))) return rc;
  // linear3 and dropout3
  if ((rc = launch_wgrad_all(wa.dall2, U, sv.cat, R, FU, U, part, grads[P_W3], FU, s))) return rc;
  if ((rc = launch_colsum_rows(wa.dall2, U, R, U, grads[P_B3], s))) return rc;
  if ((rc = launch_mdx(wa.dall2, U, params[P_W3], FU, R, FU, U, nullptr, nullptr, w.dcat, wt, s))) return rc;
  if (p > 0.f) {
    hipLaunchKernelGGL(drop_cols_kernel, dim3(flat_grid(R * FU)), dim3(CA_BLOCK), 0, s, w.dcat, R * FU, Si, Ci, FU, d3, seeds);
    MANNER_LAUNCH_CHECK();
  }
  // candi-selfatt: out-projection, attention, in-projection, linear2
  if ((rc = launch_wgrad_all(w.dcat + F, FU, sv.att, R, U, U, part, grads[P_WOUT], U, s))) return rc;
  if ((rc = launch_colsum_rows(w.dcat + F, FU, R, U, grads[P_BOUT], s))) return rc;
  if ((rc = launch_mdx(w.dcat + F, FU, params[P_WOUT], U, R, U, U, nullptr, nullptr, w.datt, wt, s))) return rc;
  if ((rc = launch_a0any_bwd_q(sv.qkv, sv.att, w.datt, w.dqkv, sv.stats, B, C * S, U, heads, s))) return rc;
  if ((rc = launch_a0any_bwd_kv(sv.qkv, w.datt, sv.stats, w.dqkv, B, C * S, U, heads, s))) return rc;
  if ((rc = launch_wgrad_all(w.dqkv, 3 * U, sv.h2, R, U, 3 * U, part, grads[P_WIN], U, s))) return rc;
  if ((rc = launch_colsum_rows(w.dqkv, 3 * U, R, 3 * U, grads[P_BIN], s))) return rc;
  // the K third of d in_proj_bias is zero in exact arithmetic (a shift of every key moves every logit of a row alike)
  MANNER_HIP_TRY(hipMemsetAsync(grads[P_BIN] + U, 0, (size_t)U * sizeof(float), s));
  if ((rc = launch_mdx(w.dqkv, 3 * U, params[P_WIN], U, R, U, 3 * U, nullptr, nullptr, w.dh2, wt, s))) return rc;
  if ((rc = launch_wgrad_all(w.dh2, U, sv.a2, R, 2 * D, U, part, grads[P_W2], 2 * D, s))) return rc;
  if ((rc = launch_colsum_rows(w.dh2, U, R, U, grads[P_B2], s))) return rc;
  if ((rc = launch_mdx(w.dh2, U, params[P_W2], 2 * D, R, 2 * D, U, nullptr, nullptr, w.da2, wt, s))) return rc;
  // candi-cnn: linear1 from cat[:, :F]
  if ((rc = launch_wgrad_all(w.dcat, FU, sv.a1, R, 4 * D, F, part, grads[P_W1], 4 * D, s))) return rc;
  if ((rc = launch_colsum_rows(w.dcat, FU, R, F, grads[P_B1], s))) return rc;
  if ((rc = launch_mdx(w.dcat, FU, params[P_W1], 4 * D, R, 4 * D, F, nullptr, nullptr, w.da1, wt, s))) return rc;
  // d x: per column the three windows and the self-attention operand through the column's dropout2, the columns added in ascending c;
  // d cand: the sums over the slots, through the column's dropout1
  hipLaunchKernelGGL(window_dx_cols_kernel, dim3((unsigned)(B * S)), dim3(CA_BLOCK), 0, s, w.da1, w.da2, Si, Ci, D, d2, seeds, grad_x);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(cand_dx_cols_kernel, dim3((unsigned)P, (unsigned)((D + CA_BLOCK - 1) / CA_BLOCK)), dim3(CA_BLOCK), 0, s, w.da1, w.da2, wa.dcd2, Si, Ci, D, d1,
                     seeds, grad_cand);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // extern "C"
