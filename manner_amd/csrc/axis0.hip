// The fixed-head-dim family of the axis-0 multi-head attention: nn.MultiheadAttention(batch_first=False) fed [batch, seq, E] (quirk
// Q1, reference news_encoder.py:60-72), so attention runs along axis 0, unmasked.  One forward kernel serves inference
// (manner_hip_entity_encode and manner_hip_mha_axis0 in entity.hip, through launch_axis0_attention) and training
// (manner_hip_axis0_attention), the two backward kernels serve manner_hip_axis0_attention_backward; one table holds the seven head
// dims.  The other two families live with the kernels they share helpers with: any head dim 1 .. 64 is caum.hip's a0any_*, head
// dims 65 .. 128 are mins.hip's aw_*.
#include <math.h>

#include "common.h"

namespace manner {
namespace {

// ---------------------------------------------------------------- forward
// attention over axis 0 for one (slot e, head): qkv [N, E, 3D] = [q | k | v], out [N, E, D].
// One thread per query row, keys streamed through LDS tiles of KT keys, online softmax.
template <int DH, int KT>
__global__ __launch_bounds__(256) void axis0_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, int64_t N, int E, int D,
                                                        int heads) {
  __shared__ float ks[KT * DH], vs[KT * DH];
  const int eh = blockIdx.x, e = eh / heads, hh = eh - e * heads;
  const int64_t n = (int64_t)blockIdx.y * 256 + threadIdx.x;
  const float scale = 1.0f / sqrtf((float)DH);
  const size_t ld = (size_t)E * 3 * D;
  const float* base = qkv + (size_t)e * 3 * D + hh * DH;
  float q[DH], o[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) { q[d] = n < N ? base[n * ld + d] * scale : 0.f; o[d] = 0.f; }   // q is scaled first, as torch does
  float mx = -INFINITY, sum = 0.f;
  for (int64_t t0 = 0; t0 < N; t0 += KT) {
    __syncthreads();
    for (int i = threadIdx.x; i < KT * DH; i += 256) {
      const int j = i / DH, d = i - j * DH;
      const int64_t kn = t0 + j;
      ks[i] = kn < N ? base[kn * ld + D + d] : 0.f;
      vs[i] = kn < N ? base[kn * ld + 2 * D + d] : 0.f;
    }
    __syncthreads();
    const int cnt = (int)min((int64_t)KT, N - t0);
    for (int j = 0; j < cnt; ++j) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) s = fmaf(q[d], ks[j * DH + d], s);
      if (s > mx) {
        const float f = expf(mx - s);
        sum *= f;
#pragma unroll
        for (int d = 0; d < DH; ++d) o[d] *= f;
        mx = s;
      }
      const float p = expf(s - mx);
      sum += p;
#pragma unroll
      for (int d = 0; d < DH; ++d) o[d] = fmaf(p, vs[j * DH + d], o[d]);
    }
  }
  if (n < N) {
    const float inv = 1.0f / sum;
    float* dst = out + (size_t)n * E * D + (size_t)e * D + hh * DH;
#pragma unroll
    for (int d = 0; d < DH; ++d) dst[d] = o[d] * inv;
  }
}

// ---------------------------------------------------------------- backward
// qkv [N, E, 3D] (q | k | v), d_att [N, E, D] -> d_qkv [N, E, 3D]; attention along the N axis for each (slot e, head).
// Kernel 1 (thread = query row): softmax statistics {max, sum}, D_i = sum_j dP_ij P_ij, dq_i.  Kernel 2 (thread = key row):
// dk_j = sum_i dS_ij q_i (scaled), dv_j = sum_i P_ij dO_i.
template <int DH, int KT>
__global__ __launch_bounds__(256) void axis0_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ datt,
                                                          float* __restrict__ dqkv, float* __restrict__ stats /*[N, E*heads, 3]*/,
                                                          int64_t N, int E, int D, int heads) {
  __shared__ float ks[KT * DH], vs[KT * DH];
  const int eh = blockIdx.x, e = eh / heads, hh = eh - e * heads;
  const int64_t n = (int64_t)blockIdx.y * 256 + threadIdx.x;
  const float scale = 1.0f / sqrtf((float)DH);
  const size_t ld = (size_t)E * 3 * D;
  const float* base = qkv + (size_t)e * 3 * D + hh * DH;
  float q[DH], go[DH], dq[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    q[d] = n < N ? base[n * ld + d] * scale : 0.f;
    go[d] = n < N ? datt[(size_t)n * E * D + (size_t)e * D + hh * DH + d] : 0.f;
    dq[d] = 0.f;
  }
  float mx = -INFINITY, sum = 0.f, Dn = 0.f;
  for (int pass = 0; pass < 3; ++pass) {
    for (int64_t t0 = 0; t0 < N; t0 += KT) {
      __syncthreads();
      for (int i = threadIdx.x; i < KT * DH; i += 256) {
        const int j = i / DH, d = i - j * DH;
        const int64_t kn = t0 + j;
        ks[i] = kn < N ? base[kn * ld + D + d] : 0.f;
        vs[i] = kn < N ? base[kn * ld + 2 * D + d] : 0.f;
      }
      __syncthreads();
      const int cnt = (int)min((int64_t)KT, N - t0);
      for (int j = 0; j < cnt; ++j) {
        float s = 0.f, gv = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) { s = fmaf(q[d], ks[j * DH + d], s); gv = fmaf(go[d], vs[j * DH + d], gv); }
        if (pass == 0) {
          if (s > mx) { sum *= expf(mx - s); mx = s; }
          sum += expf(s - mx);
        } else {
          const float p = expf(s - mx) / sum;
          if (pass == 1) Dn = fmaf(gv, p, Dn);
          else {
            const float ds = p * (gv - Dn) * scale;
#pragma unroll
            for (int d = 0; d < DH; ++d) dq[d] = fmaf(ds, ks[j * DH + d], dq[d]);
          }
        }
      }
    }
  }
  if (n < N) {
    float* dst = dqkv + n * ld + (size_t)e * 3 * D + hh * DH;
#pragma unroll
    for (int d = 0; d < DH; ++d) dst[d] = dq[d];
    float* st = stats + ((size_t)n * E * heads + eh) * 3;
    st[0] = mx; st[1] = sum; st[2] = Dn;
  }
}
template <int DH, int KT>
__global__ __launch_bounds__(256) void axis0_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ datt,
                                                           const float* __restrict__ stats, float* __restrict__ dqkv, int64_t N,
                                                           int E, int D, int heads) {
  __shared__ float qs[KT * DH], gs[KT * DH];
  __shared__ float sm[KT], sl[KT], sd[KT];
  const int eh = blockIdx.x, e = eh / heads, hh = eh - e * heads;
  const int64_t n = (int64_t)blockIdx.y * 256 + threadIdx.x;
  const float scale = 1.0f / sqrtf((float)DH);
  const size_t ld = (size_t)E * 3 * D;
  const float* base = qkv + (size_t)e * 3 * D + hh * DH;
  float k[DH], v[DH], dk[DH], dv[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    k[d] = n < N ? base[n * ld + D + d] : 0.f;
    v[d] = n < N ? base[n * ld + 2 * D + d] : 0.f;
    dk[d] = dv[d] = 0.f;
  }
  for (int64_t t0 = 0; t0 < N; t0 += KT) {
    __syncthreads();
    for (int i = threadIdx.x; i < KT * DH; i += 256) {
      const int j = i / DH, d = i - j * DH;
      const int64_t qn = t0 + j;
      qs[i] = qn < N ? base[qn * ld + d] * scale : 0.f;
      gs[i] = qn < N ? datt[(size_t)qn * E * D + (size_t)e * D + hh * DH + d] : 0.f;
    }
    for (int j = threadIdx.x; j < KT; j += 256) {
      const int64_t qn = t0 + j;
      const float* st = stats + ((size_t)(qn < N ? qn : 0) * E * heads + eh) * 3;
      sm[j] = st[0]; sl[j] = 1.f / st[1]; sd[j] = st[2];
    }
    __syncthreads();
    const int cnt = (int)min((int64_t)KT, N - t0);
    for (int i = 0; i < cnt; ++i) {
      float s = 0.f, gv = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) { s = fmaf(qs[i * DH + d], k[d], s); gv = fmaf(gs[i * DH + d], v[d], gv); }
      const float p = expf(s - sm[i]) * sl[i];
      const float ds = p * (gv - sd[i]);                  // qs carries the 1/sqrt(dh)
#pragma unroll
      for (int d = 0; d < DH; ++d) { dk[d] = fmaf(ds, qs[i * DH + d], dk[d]); dv[d] = fmaf(p, gs[i * DH + d], dv[d]); }
    }
  }
  if (n < N) {
    float* dst = dqkv + n * ld + (size_t)e * 3 * D + hh * DH;
#pragma unroll
    for (int d = 0; d < DH; ++d) { dst[D + d] = dk[d]; dst[2 * D + d] = dv[d]; }
  }
}

// One row per supported head dim: CALL(head dim, inference key tile, training key tile).  The columns were chosen separately (inference
// stages up to 32 KiB of keys and values per workgroup; the training column, which the two backward kernels with their wider per-thread
// state share, up to 20 KiB) and have not been measured against each other, so every launch keeps the tile it had.
#define MANNER_AXIS0_TILES(DH_, CALL)                                                                       \
  switch (DH_) {                                                                                            \
    case 4: CALL(4, 256, 256); break;                                                                       \
    case 8: CALL(8, 256, 256); break;                                                                       \
    case 10: CALL(10, 256, 256); break;                                                                     \
    case 16: CALL(16, 256, 128); break;                                                                     \
    case 32: CALL(32, 64, 64); break;                                                                       \
    case 48: CALL(48, 64, 32); break;                                                                       \
    case 64: CALL(64, 64, 32); break;                                                                       \
    default: return fail(MANNER_HIP_E_INVALID, "axis-0 attention: head_dim %d unsupported (4, 8, 10, 16, 32, 48, 64)", DH_); \
  }

}  // namespace

int launch_axis0_attention(const float* qkv, float* att, int64_t N, int64_t E, int D, int heads, bool train_tiles, hipStream_t s) {
  const dim3 g((unsigned)(E * heads), (unsigned)((N + 255) / 256)), b(256);
#define MANNER_A0F(DH_, KI_, KT_)                                                                                \
  do {                                                                                                           \
    if (train_tiles) hipLaunchKernelGGL((axis0_fwd_kernel<DH_, KT_>), g, b, 0, s, qkv, att, N, (int)E, D, heads); \
    else hipLaunchKernelGGL((axis0_fwd_kernel<DH_, KI_>), g, b, 0, s, qkv, att, N, (int)E, D, heads);            \
  } while (0)
  MANNER_AXIS0_TILES(D / heads, MANNER_A0F)
#undef MANNER_A0F
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // namespace manner

using namespace manner;

extern "C" {

// forward core only (the projections are separate Linear ops in the training graph)
int manner_hip_axis0_attention(const float* qkv, int64_t L0, int64_t B1, int32_t E, int32_t heads, float* out, manner_hip_stream_t stream) {
  if (L0 == 0 || B1 == 0) return MANNER_HIP_OK;
  if (!qkv || !out || L0 < 0 || B1 < 0 || E <= 0 || heads <= 0 || E % heads) return fail(MANNER_HIP_E_INVALID, "axis0_attention: bad argument");
  return launch_axis0_attention(qkv, out, L0, B1, E, heads, true, (hipStream_t)stream);
}

int manner_hip_axis0_attention_backward(const float* qkv, const float* grad_out, int64_t L0, int64_t B1, int32_t E, int32_t heads,
                                        float* grad_qkv, float* stats /*[L0 * B1 * heads * 3]*/, manner_hip_stream_t stream) {
  if (L0 == 0 || B1 == 0) return MANNER_HIP_OK;
  if (!qkv || !grad_out || !grad_qkv || !stats || L0 < 0 || B1 < 0 || E <= 0 || heads <= 0 || E % heads)
    return fail(MANNER_HIP_E_INVALID, "axis0_attention_backward: bad argument");
  const dim3 g((unsigned)(B1 * heads), (unsigned)((L0 + 255) / 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
#define MANNER_A0B(DH_, KI_, KT_)                                                                                                \
  do {                                                                                                                           \
    hipLaunchKernelGGL((axis0_bwd_q_kernel<DH_, KT_>), g, b, 0, s, qkv, grad_out, grad_qkv, stats, L0, (int)B1, E, heads);       \
    hipLaunchKernelGGL((axis0_bwd_kv_kernel<DH_, KT_>), g, b, 0, s, qkv, grad_out, stats, grad_qkv, L0, (int)B1, E, heads);      \
  } while (0)
  MANNER_AXIS0_TILES(E / heads, MANNER_A0B)
#undef MANNER_A0B
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // extern "C"
