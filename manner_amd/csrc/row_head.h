// The row head of <= 64 classes that aspect.hip (head_ce, head_l1) and debias.hip (adv_loss, layer 2) share: nn.Linear(D, O) over every
// row + a cross-entropy, forward and backward.  A workgroup stages the weight ONCE (LDS, when it fits) and its four waves walk a
// grid-stride loop of rows under it, one row per wave at a time, the row in registers.  What differs between the callers is a policy
// struct passed by value (the target column and the row factor of the forward, the last line of the data gradient).  Every reduction
// across rows has a fixed order (no floating-point atomics) and every grid comes from the shape alone.
// The kernels are templates instantiated per caller: internal linkage, one copy per including file.
#pragma once
#include <math.h>

#include "common.h"

namespace manner {
namespace {

constexpr int RH_MAX_O = 64, RH_MAX_D = 1024;            // classes (one per lane); row width
constexpr int RH_J = RH_MAX_D / 64;                      // row elements per lane
constexpr int RH_WG_ROWS = 8, RH_MAX_WG = 512;           // rows a workgroup takes per trip of its grid-stride loop (two per wave: N is small and
                                                         // the chip wide); the grid's cap (two staged workgroups fit a CU)
constexpr int RH_CHUNK_ROWS = 32, RH_MAX_CHUNKS = 128;   // weight gradient: rows per partial sum at least; partial sums at most
constexpr size_t RH_STAGE_BYTES = 128 * 1024;            // a weight up to here is staged in LDS (160 KB per CU), a larger one is read through L2

// ---------------------------------------------------------------- forward
// MODE 0: cross-entropy, the weight staged in LDS; 1: cross-entropy, the weight read where it lies; 2: the head's own single-output row
// (head.single_row: O == 1, the weight row in registers).  Wave w of workgroup g takes the rows 8 (g + k G) + w + 4 i.  Per row: the row
// into registers, one dot product per class (four classes in flight, each a per-lane fma chain over d = lane + 64 j and a butterfly),
// class o's logit kept in lane o, then the softmax across the lanes and the cross-entropy against column head.column(class).
// rowloss [N] receives the row's loss, `saved` (may be NULL) [N, O] = (p - y) head.row_factor(r).
// A class outside [0, O) is never used as an index: it raises MANNER_HIP_STATUS_INDEX and its row counts as loss 0, gradient 0.
template <int MODE, typename Head>
__global__ __launch_bounds__(256) void rh_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                          const int64_t* __restrict__ cls, Head head, int64_t N, int D, int O,
                                                          float* __restrict__ rowloss, float* __restrict__ saved, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (MODE == 0) stage_weight(W, O * D, wl);
  float wr[RH_J];
  if (MODE == 2) {
#pragma unroll
    for (int j = 0; j < RH_J; ++j) wr[j] = lane + 64 * j < D ? W[lane + 64 * j] : 0.f;
  }
  const float bl = lane < O ? bias[lane] : 0.f;
  for (int64_t base = (int64_t)blockIdx.x * RH_WG_ROWS; base < N; base += (int64_t)gridDim.x * RH_WG_ROWS) {
    const int64_t end = base + RH_WG_ROWS < N ? base + RH_WG_ROWS : N;
    for (int64_t r = base + wave; r < end; r += 4) {
      float xr[RH_J];
#pragma unroll
      for (int j = 0; j < RH_J; ++j) xr[j] = lane + 64 * j < D ? x[(size_t)r * D + lane + 64 * j] : 0.f;
      if constexpr (MODE == 2) {
        head.single_row(xr, wr, bias, r, lane, rowloss, saved);
      } else {
        const float* w = MODE == 0 ? wl : W;
        float mine = -INFINITY;                                   // the logit of class `lane`
        for (int o0 = 0; o0 < O; o0 += 4) {
          float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < RH_J; ++j) {
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
        const int tt = bad ? 0 : head.column(t, O);
        const float m = wmax(mine);
        const float e = lane < O ? expf(mine - m) : 0.f;
        const float s = wsum(e);
        const float lt = __shfl(mine, tt, 64);
        if (lane < O) {
          if (saved) saved[(size_t)r * O + lane] = bad ? 0.f : head.scaled(e / s - (lane == tt ? 1.f : 0.f), r, N);
          head.keep_logit(mine, (size_t)r * O + lane);
        }
        if (lane == 0) {
          rowloss[r] = bad ? 0.f : (logf(s) + m) - lt;
          if (bad && status) atomicOr(status, MANNER_HIP_STATUS_INDEX);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- backward
// out[r, d] = last(last.coef(g, N) sum_o saved[r, o] W[o, d], r D + d), the sum in ascending o: the forward's row walk, lane o holding
// saved[r, o].
template <bool STAGED, typename Last>
__global__ __launch_bounds__(256) void rh_head_dx_kernel(const float* __restrict__ g, const float* __restrict__ W, const float* __restrict__ saved,
                                                         Last last, int64_t N, int D, int O, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (STAGED) stage_weight(W, O * D, wl);
  const float* w = STAGED ? wl : W;
  const float coef = last.coef(g[0], N);
  for (int64_t base = (int64_t)blockIdx.x * RH_WG_ROWS; base < N; base += (int64_t)gridDim.x * RH_WG_ROWS) {
    const int64_t end = base + RH_WG_ROWS < N ? base + RH_WG_ROWS : N;
    for (int64_t r = base + wave; r < end; r += 4) {
      const float mine = lane < O ? saved[(size_t)r * O + lane] : 0.f;
      float a[RH_J];
#pragma unroll
      for (int j = 0; j < RH_J; ++j) a[j] = 0.f;
      for (int o = 0; o < O; ++o) {
        const float t = __shfl(mine, o, 64);
#pragma unroll
        for (int j = 0; j < RH_J; ++j)
          if (64 * j < D) a[j] = fmaf(t, w[o * D + min(lane + 64 * j, D - 1)], a[j]);      // wave-uniform guard, clamped column
      }
#pragma unroll
      for (int j = 0; j < RH_J; ++j) {
        const int d = lane + 64 * j;
        if (d < D) out[(size_t)r * D + d] = last(coef * a[j], (size_t)r * D + d);
      }
    }
  }
}

// part[chunk][o][dd] = the sum over the chunk's rows, ascending, of saved[r, o] (dd < D ? x[r, dd] : 1): d W and, as column D of the same
// contraction with x = 1, d b.  One wave per (64 columns, chunk of rows): lane = column, the O classes in registers.
template <int OC>
__global__ __launch_bounds__(64) void rh_head_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ saved, int64_t N, int D, int O,
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

// one thread per (o, column): the chunks in ascending order, times g / div
__global__ __launch_bounds__(256) void rh_head_wreduce_kernel(const float* __restrict__ g, const float* __restrict__ part, float div, int D, int O,
                                                              int chunks, float* __restrict__ dW, float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= O * (D + 1)) return;
  const int o = i / (D + 1), dd = i - o * (D + 1);
  float a = 0.f;
  for (int c = 0; c < chunks; ++c) a += part[(size_t)c * O * (D + 1) + i];
  a *= g[0] / div;
  if (dd < D) {
    if (dW) dW[(size_t)o * D + dd] = a;
  } else if (db) {
    db[o] = a;
  }
}

// ---------------------------------------------------------------- host side
unsigned rh_walk_grid(int64_t N) {
  const int64_t g = (N + RH_WG_ROWS - 1) / RH_WG_ROWS;
  return (unsigned)(g < RH_MAX_WG ? g : RH_MAX_WG);
}
// partial sums of the weight gradient over N >= 1 rows
int64_t rh_chunks(int64_t N) {
  const int64_t c = (N + RH_CHUNK_ROWS - 1) / RH_CHUNK_ROWS;
  return c < RH_MAX_CHUNKS ? c : RH_MAX_CHUNKS;
}
// launches kernel<..>(args...) on the row walk, the weight [O, D] as dynamic LDS when STAGED
template <typename K, typename... Args>
int rh_launch_walk(K kernel, bool staged, int64_t N, int D, int O, hipStream_t s, Args... args) {
  const size_t lds = staged ? (size_t)O * D * sizeof(float) : 0;
  if (lds > 64 * 1024)
    MANNER_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RH_STAGE_BYTES));
  hipLaunchKernelGGL(kernel, dim3(rh_walk_grid(N)), dim3(256), lds, s, args...);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}
// dW [O, D], db [O] (either may be NULL) = (g / div) saved^T [x | 1] over N >= 1 rows; part holds rh_chunks(N) * O * (D + 1) floats
int rh_head_wgrad(const float* g, float div, const float* x, const float* saved, int64_t N, int D, int O, float* part, float* dW, float* db,
                  hipStream_t s) {
  const int64_t chunks = rh_chunks(N), chunk_rows = (N + chunks - 1) / chunks;
  const dim3 grid((unsigned)((D + 1 + 63) / 64), (unsigned)chunks);
  if (O == 1) hipLaunchKernelGGL(rh_head_wgrad_kernel<1>, grid, dim3(64), 0, s, x, saved, N, D, O, chunk_rows, part);
  else if (O <= 8) hipLaunchKernelGGL(rh_head_wgrad_kernel<8>, grid, dim3(64), 0, s, x, saved, N, D, O, chunk_rows, part);
  else if (O <= 32) hipLaunchKernelGGL(rh_head_wgrad_kernel<32>, grid, dim3(64), 0, s, x, saved, N, D, O, chunk_rows, part);
  else hipLaunchKernelGGL(rh_head_wgrad_kernel<64>, grid, dim3(64), 0, s, x, saved, N, D, O, chunk_rows, part);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(rh_head_wreduce_kernel, dim3((unsigned)((O * (D + 1) + 255) / 256)), dim3(256), 0, s, g, part, div, D, O, (int)chunks, dW, db);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // namespace
}  // namespace manner
