// The small f32 row kernels that the baselines' operator files share (declared in common.h), each with leading dimensions so that a
// dense caller passes its width and a caller that owns a column range of a wider buffer passes that buffer's:
//   launch_lin_rows      y = act(x W^T + b + rowadd) over dense rows — caum.hip (the per-column user encoder, manner_hip_linear_tanh)
//   launch_proj_rows     gi = x W^T + b over strided, length-masked (b, t[, c]) rows, the same kernel — the input projection of gru.hip and mins.hip
//   launch_dx_rows       dx = (add + dy W) * mul — train_small.hip (manner_hip_linear_backward), caum.hip
//   launch_wgrad_rows    dW = dy^T x over many rows, in row groups summed in a fixed order — poly.hip, caum.hip
//   launch_colsum_rows   db = the column sums of dy — train_small.hip (manner_hip_linear_backward), caum.hip
//   launch_transpose_tile  W^T through a 32 x 32 LDS tile — gru.hip, caum.hip
// Plain VALU kernels for latency-bound shapes.  Every reduction across rows runs in a fixed order (no floating-point atomics).
#include <algorithm>

#include "common.h"

namespace manner {
namespace {

constexpr int RF_BLOCK = 256, RF_WAVES = 4;
constexpr int PJ_ROWS = 8;       // rows per workgroup of the linear and of its data gradient
constexpr int PJ_OT = LIN_ROWS_OT;                   // output features per workgroup
constexpr int PJ_KS = 128;       // input features per step (x rows 4 KiB, weight tile PJ_OT x (PJ_KS + 1) floats = 32 KiB)
constexpr int DX_OC = 1024;      // output features staged per pass of the data gradient (32 KiB)
constexpr int CS_COLS = 64, CS_GROUPS = 16;          // column sum: columns per workgroup, row groups
constexpr int TT = 32;           // tile edge of the transpose
static_assert(PJ_OT * RF_WAVES == RF_BLOCK && PJ_KS % RF_WAVES == 0, "lin_rows_kernel: thread = (output feature, K quarter)");

// ---------------------------------------------------------------- nn.Linear over dense or strided rows
// Where row r of the product lies in x, NULL for a padded slot (t >= len[b]).  RowsDense: x + r K.  RowsBT: r = b S + t, x[b, t, :] at
// x + b xsb + t xss.  RowsBTC: r = (b S + t) C + c, the K columns [c K, (c + 1) K) of x[b, t, :].  Built in the kernel from its own scalar
// arguments (none, `S`, or `S, C`): scalars of the argument block, no struct to unpack, and no form carries another form's row arguments.
// The rest of the argument block is one list for all forms, so each form also receives what only the others read (the dense rows `xsb`,
// `xss`, `len`, `xs`; the projections `rowadd`, `SA`, `deriv`): 120 / 128 bytes of arguments against the 88 of a kernel written for one form.
// DENSE settles at compile time what a form does with them: the dense rows take their address x + r K straight from the row index, add
// `rowadd` and write no `xs`; the projections keep the table of row pointers in LDS, write `xs` and add no `rowadd`.
struct RowsDense {
  static constexpr bool DENSE = true;
  __device__ __forceinline__ const float* at(const float*, int64_t, int64_t, const int64_t*, int64_t, int) const { return nullptr; }      // never called
};
struct RowsBT {
  static constexpr bool DENSE = false;
  int S;
  __device__ __forceinline__ const float* at(const float* x, int64_t xsb, int64_t xss, const int64_t* len, int64_t r, int) const {
    const int64_t bb = r / S, t = r - bb * S;
    return t < len[bb] ? x + bb * xsb + t * xss : nullptr;
  }
};
struct RowsBTC {
  static constexpr bool DENSE = false;
  int S, C;
  __device__ __forceinline__ const float* at(const float* x, int64_t xsb, int64_t xss, const int64_t* len, int64_t r, int K) const {
    const int64_t bt = r / C, c = r - bt * C, bb = bt / S, t = bt - bb * S;
    return t < len[bb] ? x + bb * xsb + t * xss + c * K : nullptr;
  }
};
// y[r, o] = act(b[o] + rowadd[r / SA, o] + sum_k x_r[k] W[o, k]); the row is read as zeros at a padded slot, W rows ldw apart, y rows ldy
// apart (a column range of a wider buffer), b and rowadd may be NULL.  grid (ceil(R / PJ_ROWS), ceil(O / PJ_OT)): a workgroup owns
// PJ_ROWS rows x PJ_OT output features and walks K in steps of PJ_KS, the x rows and the weight tile staged in LDS by whole coalesced
// rows (the tile padded by one float against bank conflicts); thread = (output feature, wave): each wave takes a quarter of every K
// step on its own chain, and the four partial sums meet in LDS and are added pairwise, in a fixed order; then the bias, then rowadd,
// then tanh.
// TANH with `deriv` [R, O]: also tanh' = 4 e / (1 + e)^2, e = exp(-2 |pre|), taken from the pre-activation while it is in a register.
// 1 - y^2 from the rounded y loses 2 y^2 / (1 - y^2) of y's relative error — 18 x at y = 0.95 — and the bias gradients of the dense
// attention sum hundreds of such terms that cancel.
// `xs` [R, K] (training): the rows as they were read (zeros at the padded slots), for the weight gradient; written by the workgroups of
// the first output tile.
template <typename Rows, bool TANH, typename... RowArgs>
__global__ __launch_bounds__(RF_BLOCK) void lin_rows_kernel(const float* __restrict__ x, int64_t xsb, int64_t xss, const int64_t* __restrict__ len,
                                                       const float* __restrict__ W, int ldw, const float* __restrict__ b,
                                                       const float* __restrict__ rowadd, int SA, RowArgs... row_args, int64_t R, int K, int O,
                                                       float* __restrict__ y, int ldy, float* __restrict__ deriv, float* __restrict__ xs) {
  const Rows rows{row_args...};
  __shared__ float xt[PJ_ROWS][PJ_KS];
  __shared__ float ws[PJ_OT][PJ_KS + 1];
  __shared__ float red[RF_WAVES][PJ_ROWS][PJ_OT];
  __shared__ const float* rowp[PJ_ROWS];
  const int64_t r0 = (int64_t)blockIdx.x * PJ_ROWS;
  const int nr = (int)min((int64_t)PJ_ROWS, R - r0);
  if (!Rows::DENSE && threadIdx.x < PJ_ROWS) rowp[threadIdx.x] = (int)threadIdx.x < nr ? rows.at(x, xsb, xss, len, r0 + threadIdx.x, K) : nullptr;
  const int o0 = blockIdx.y * PJ_OT, oc = threadIdx.x % PJ_OT, kq = threadIdx.x / PJ_OT;
  float acc[PJ_ROWS];
#pragma unroll
  for (int rr = 0; rr < PJ_ROWS; ++rr) acc[rr] = 0.f;
  for (int k0 = 0; k0 < K; k0 += PJ_KS) {
    const int kc = min(PJ_KS, K - k0);
    __syncthreads();
    for (int i = threadIdx.x; i < PJ_ROWS * PJ_KS; i += RF_BLOCK) {
      const int rr = i / PJ_KS, k = i - rr * PJ_KS;
      const float* rp = Rows::DENSE ? (rr < nr ? x + (size_t)(r0 + rr) * K : nullptr) : rowp[rr];      // dense rows need no table
      const float v = (rp && k < kc) ? rp[k0 + k] : 0.f;
      xt[rr][k] = v;
      if (!Rows::DENSE && xs && blockIdx.y == 0 && rr < nr && k < kc) xs[(size_t)(r0 + rr) * K + k0 + k] = v;
    }
    for (int i = threadIdx.x; i < PJ_OT * PJ_KS; i += RF_BLOCK) {
      const int oo = i / PJ_KS, k = i - oo * PJ_KS;
      ws[oo][k] = (o0 + oo < O && k < kc) ? W[(size_t)(o0 + oo) * ldw + k0 + k] : 0.f;      // past O or K: zeros, no branch below
    }
    __syncthreads();
#pragma unroll 8
    for (int k = kq * (PJ_KS / RF_WAVES); k < (kq + 1) * (PJ_KS / RF_WAVES); ++k) {
      const float wv = ws[oc][k];
#pragma unroll
      for (int rr = 0; rr < PJ_ROWS; ++rr) acc[rr] = fmaf(xt[rr][k], wv, acc[rr]);
    }
  }
#pragma unroll
  for (int rr = 0; rr < PJ_ROWS; ++rr) red[kq][rr][oc] = acc[rr];
  __syncthreads();
  const int o = o0 + oc;
  if (kq == 0 && o < O) {
    const float bv = b ? b[o] : 0.f;
#pragma unroll
    for (int rr = 0; rr < PJ_ROWS; ++rr)
      if (rr < nr) {
        float v = ((red[0][rr][oc] + red[1][rr][oc]) + (red[2][rr][oc] + red[3][rr][oc])) + bv;
        if (Rows::DENSE && rowadd) v += rowadd[(size_t)((r0 + rr) / SA) * O + o];
        y[(size_t)(r0 + rr) * ldy + o] = TANH ? tanhf(v) : v;
        if (TANH && deriv) {
          const float e = expf(-2.0f * fabsf(v)), den = 1.0f + e;
          deriv[(size_t)(r0 + rr) * O + o] = 4.0f * e / (den * den);
        }
      }
  }
}

// ---------------------------------------------------------------- data gradient
// dx[r, k] = (add[r, k] + sum_o dy[r, o] W[o, k]) * mul[r, k]: dy rows ldy apart, W rows ldw apart, dx / add / mul [R, K]
// contiguous (add, mul may be NULL); `add` may be dx itself (each element is read and written by one thread).
// grid (ceil(R / PJ_ROWS), ceil(K / RF_BLOCK)): thread = input feature (the weight rows are read coalesced), o ascending on one chain
// that stays in registers across the passes of DX_OC staged output features.
__global__ __launch_bounds__(RF_BLOCK) void dx_rows_kernel(const float* __restrict__ dy, int ldy, const float* __restrict__ W, int ldw, int64_t R, int K,
                                                      int O, const float* add, const float* __restrict__ mul, float* dx) {
  __shared__ float ds[PJ_ROWS][DX_OC];
  const int64_t r0 = (int64_t)blockIdx.x * PJ_ROWS;
  const int nr = (int)min((int64_t)PJ_ROWS, R - r0);
  const int k = blockIdx.y * RF_BLOCK + threadIdx.x;
  float acc[PJ_ROWS];
#pragma unroll
  for (int rr = 0; rr < PJ_ROWS; ++rr) acc[rr] = 0.f;
  for (int o0 = 0; o0 < O; o0 += DX_OC) {
    const int no = min(DX_OC, O - o0);
    __syncthreads();
    for (int i = threadIdx.x; i < PJ_ROWS * no; i += RF_BLOCK) {
      const int rr = i / no, o = i - rr * no;
      ds[rr][o] = rr < nr ? dy[(size_t)(r0 + rr) * ldy + o0 + o] : 0.f;
    }
    __syncthreads();
    if (k < K)
      for (int o = 0; o < no; ++o) {
        const float w = W[(size_t)(o0 + o) * ldw + k];
#pragma unroll
        for (int rr = 0; rr < PJ_ROWS; ++rr) acc[rr] = fmaf(ds[rr][o], w, acc[rr]);
      }
  }
  if (k < K) {
#pragma unroll
    for (int rr = 0; rr < PJ_ROWS; ++rr)
      if (rr < nr) {
        const size_t at = (size_t)(r0 + rr) * K + k;
        float v = acc[rr] + (add ? add[at] : 0.f);
        if (mul) v *= mul[at];
        dx[at] = v;
      }
  }
}

// ---------------------------------------------------------------- weight gradient over many rows
// dW[o, k] = sum_r dy[r, o] x[r, k], dy rows ldy apart, x [R, K] contiguous, dW rows ldo apart.  grid (ceil(K / 256), O, G): group g sums
// its rows [g chunk, (g + 1) chunk) on four chains into part[g][o][k] (straight into dW when G == 1); wgrad_reduce_kernel adds the G
// partial sums in ascending g.
__global__ __launch_bounds__(RF_BLOCK) void wgrad_rows_kernel(const float* __restrict__ dy, int ldy, const float* __restrict__ x, int64_t R, int K, int O,
                                                             int64_t chunk, float* __restrict__ out, int ldo, int64_t gstride) {
  const int k = blockIdx.x * RF_BLOCK + threadIdx.x, o = blockIdx.y;
  if (k >= K) return;
  const int64_t r0 = (int64_t)blockIdx.z * chunk, r1 = min(R, r0 + chunk);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  int64_t r = r0;
  for (; r + 3 < r1; r += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = fmaf(dy[(r + u) * ldy + o], x[(r + u) * K + k], a[u]);
  }
  for (; r < r1; ++r) a[0] = fmaf(dy[r * ldy + o], x[r * K + k], a[0]);
  out[(size_t)blockIdx.z * gstride + (size_t)o * ldo + k] = (a[0] + a[1]) + (a[2] + a[3]);
}
__global__ __launch_bounds__(RF_BLOCK) void wgrad_reduce_kernel(const float* __restrict__ part, int K, int O, int G, float* __restrict__ dW, int ldo) {
  const int64_t i = (int64_t)blockIdx.x * RF_BLOCK + threadIdx.x, n = (int64_t)O * K;
  if (i >= n) return;
  float s = part[i];
  for (int g = 1; g < G; ++g) s += part[(size_t)g * n + i];
  const int64_t o = i / K;
  dW[o * ldo + (i - o * K)] = s;
}

// ---------------------------------------------------------------- column sum
// db[o] = sum_r dy[r, o], dy rows ldy apart.  A workgroup owns 64 columns and splits the rows over 16 groups of four accumulators each;
// the 64 partial sums of a column meet in LDS and are added pairwise, in a fixed order.  (One thread used to walk all R rows of its
// column with a single f32 accumulator: over the 771 .. 900 rows of the axis-0 attention tests that bias gradient sat 11 - 13 x further
// from float64 than a float32 CPU sum, past the 8 x bar of tests/test_gpu_side_ops.py, and every thread waited on R dependent loads.)
__global__ __launch_bounds__(CS_COLS * CS_GROUPS) void colsum_rows_kernel(const float* __restrict__ dy, int ldy, int64_t R, int O, float* __restrict__ db) {
  __shared__ float red[CS_GROUPS][CS_COLS];
  const int col = threadIdx.x % CS_COLS, g = threadIdx.x / CS_COLS;
  const int o = blockIdx.x * CS_COLS + col;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (o < O) {
    int64_t r = g;
    for (; r + 3 * CS_GROUPS < R; r += 4 * CS_GROUPS) {
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] += dy[(r + u * CS_GROUPS) * ldy + o];
    }
    for (; r < R; r += CS_GROUPS) s[0] += dy[r * ldy + o];
  }
  red[g][col] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  if (g == 0 && o < O) {
    float t[CS_GROUPS];
#pragma unroll
    for (int i = 0; i < CS_GROUPS; ++i) t[i] = red[i][col];
#pragma unroll
    for (int w = CS_GROUPS / 2; w > 0; w >>= 1) {
#pragma unroll
      for (int i = 0; i < w; ++i) t[i] += t[i + w];
    }
    db[o] = t[0];
  }
}

// ---------------------------------------------------------------- transpose
// out[k, o] = in[o, k]: in [O, K] rows ldw apart (a column range of a weight), out [K, O] contiguous.  grid (ceil(K / 32), ceil(O / 32)),
// a 32 x 32 tile through LDS, both sides coalesced.
__global__ __launch_bounds__(RF_BLOCK) void transpose_tile_kernel(const float* __restrict__ in, int ldw, int O, int K, float* __restrict__ out) {
  __shared__ float t[TT][TT + 1];
  const int k0 = blockIdx.x * TT, o0 = blockIdx.y * TT, tx = threadIdx.x % TT, ty = threadIdx.x / TT;
  for (int i = ty; i < TT; i += RF_BLOCK / TT)
    t[i][tx] = (o0 + i < O && k0 + tx < K) ? in[(size_t)(o0 + i) * ldw + k0 + tx] : 0.f;
  __syncthreads();
  for (int i = ty; i < TT; i += RF_BLOCK / TT)
    if (k0 + i < K && o0 + tx < O) out[(size_t)(k0 + i) * O + o0 + tx] = t[tx][i];
}

}  // namespace

// the four forms of lin_rows_kernel: dense rows with or without tanh (no strides, no copy-out), the two projections (dense W and y, bias only)
int launch_lin_rows(bool tanh_act, const float* x, const float* W, int ldw, const float* b, const float* rowadd, int S, int64_t R, int K, int O, float* y,
                    int ldy, float* deriv, hipStream_t s) {
  const dim3 g((unsigned)((R + PJ_ROWS - 1) / PJ_ROWS), (unsigned)((O + PJ_OT - 1) / PJ_OT));
  const int64_t* len = nullptr;
  float* xs = nullptr;
  if (tanh_act) hipLaunchKernelGGL((lin_rows_kernel<RowsDense, true>), g, dim3(RF_BLOCK), 0, s, x, (int64_t)0, (int64_t)0, len, W, ldw, b, rowadd, S, R, K, O, y, ldy, deriv, xs);
  else hipLaunchKernelGGL((lin_rows_kernel<RowsDense, false>), g, dim3(RF_BLOCK), 0, s, x, (int64_t)0, (int64_t)0, len, W, ldw, b, rowadd, S, R, K, O, y, ldy, deriv, xs);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}
int launch_proj_rows(const float* x, int64_t xsb, int64_t xss, const int64_t* len, const float* W, const float* b, int S, int C, int64_t R, int K, int O,
                     float* gi, float* xs, hipStream_t s) {
  const dim3 g((unsigned)((R + PJ_ROWS - 1) / PJ_ROWS), (unsigned)((O + PJ_OT - 1) / PJ_OT));
  const float* rowadd = nullptr;
  float* deriv = nullptr;
  if (C == 1) hipLaunchKernelGGL((lin_rows_kernel<RowsBT, false, int>), g, dim3(RF_BLOCK), 0, s, x, xsb, xss, len, W, K, b, rowadd, 1, S, R, K, O, gi, O, deriv, xs);
  else hipLaunchKernelGGL((lin_rows_kernel<RowsBTC, false, int, int>), g, dim3(RF_BLOCK), 0, s, x, xsb, xss, len, W, K, b, rowadd, 1, S, C, R, K, O, gi, O, deriv, xs);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}
int launch_dx_rows(const float* dy, int ldy, const float* W, int ldw, int64_t R, int K, int O, const float* add, const float* mul, float* dx, hipStream_t s) {
  hipLaunchKernelGGL(dx_rows_kernel, dim3((unsigned)((R + PJ_ROWS - 1) / PJ_ROWS), (unsigned)((K + RF_BLOCK - 1) / RF_BLOCK)), dim3(RF_BLOCK), 0, s, dy, ldy, W, ldw, R, K, O, add, mul, dx);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int wgrad_rows_groups(int64_t R) { return (int)std::max<int64_t>(1, std::min<int64_t>(WGRAD_MAX_GROUPS, R / WGRAD_GROUP_ROWS)); }
size_t wgrad_rows_part_floats(int64_t R, int K, int O) { return (size_t)wgrad_rows_groups(R) * (size_t)O * (size_t)K; }
int launch_wgrad_reduce(const float* part, int K, int O, int G, float* dW, int ldo, hipStream_t s) {
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(((int64_t)O * K + RF_BLOCK - 1) / RF_BLOCK)), dim3(RF_BLOCK), 0, s, part, K, O, G, dW, ldo);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}
int launch_wgrad_rows(const float* dy, int ldy, const float* x, int64_t R, int K, int O, float* part, float* dW, int ldo, hipStream_t s) {
  const int G = wgrad_rows_groups(R);
  const int64_t chunk = (R + G - 1) / G;
  const dim3 g((unsigned)((K + RF_BLOCK - 1) / RF_BLOCK), (unsigned)O, (unsigned)G);
  if (G == 1) hipLaunchKernelGGL(wgrad_rows_kernel, g, dim3(RF_BLOCK), 0, s, dy, ldy, x, R, K, O, chunk, dW, ldo, (int64_t)0);
  else hipLaunchKernelGGL(wgrad_rows_kernel, g, dim3(RF_BLOCK), 0, s, dy, ldy, x, R, K, O, chunk, part, K, (int64_t)O * K);
  MANNER_LAUNCH_CHECK();
  return G > 1 ? launch_wgrad_reduce(part, K, O, G, dW, ldo, s) : MANNER_HIP_OK;
}
int launch_colsum_rows(const float* dy, int ldy, int64_t R, int O, float* db, hipStream_t s) {
  hipLaunchKernelGGL(colsum_rows_kernel, dim3((unsigned)((O + CS_COLS - 1) / CS_COLS)), dim3(CS_COLS * CS_GROUPS), 0, s, dy, ldy, R, O, db);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}
int launch_transpose_tile(const float* in, int ldw, int O, int K, float* out, hipStream_t s) {
  hipLaunchKernelGGL(transpose_tile_kernel, dim3((unsigned)((K + TT - 1) / TT), (unsigned)((O + TT - 1) / TT)), dim3(RF_BLOCK), 0, s, in, ldw, O, K, out);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // namespace manner
