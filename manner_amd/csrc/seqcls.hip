// The sequence-classification head of the sentiment annotator (reference manner/data/components/sentiment_annotator.py:25-38 over
// HF's RobertaClassificationHead / BERT's pooler + classifier, eval mode): per [CLS] row x, in f32,
//   h = tanh(Wd x + bd),  z = Wo h + bo,  p = softmax(z),  a = argmax p,  score by the reference's rule
// in ONE launch.  A workgroup owns a row panel and walks every column tile of the dense layer for it, so the [N, H] hidden activation
// never reaches memory and softmax, argmax and the rule finish where the logits were summed: no fan-in across workgroups, no atomics.
#include "common.h"

namespace manner {
namespace {

constexpr int SC_BLOCK = 256, SC_WAVE = 64;
constexpr int SC_BK = 32;                            // input features per staging, as wlin_kernel
constexpr int SC_LD = SC_BK + 1;                     // odd LDS pitch: the rows of an MFMA operand read distinct banks
constexpr int SC_MAX_L = 64, SC_MAX_H = 1024;
constexpr int SC_SMALL_ROWS = 8192;                  // fewer rows than this: the 32-row panel (up to one workgroup per CU), else 128 rows

// Summation order of every output, whichever panel: a hidden feature is one k-ascending fmaf chain from 0 (the f32 MFMA's own order,
// 32x32x2 or 16x16x4), then + bd, tanhf; a logit is ONE chain z = fmaf(h[o], Wo[l, o], z) over o = 0 .. H - 1 ascending that starts at
// bo[l] — the column tiles of the dense layer are visited in ascending order and each appends its columns to the chain.  The chain of
// (row, l) lives in one register of one thread from the first tile to the last.  So a row's bits depend on nothing but the row.
template <bool SMALL>
__global__ __launch_bounds__(SC_BLOCK) void seqcls_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ Wd,
                                                           const float* __restrict__ bd, const float* __restrict__ Wo,
                                                           const float* __restrict__ bo, int pos_idx, int neg_idx, int64_t N, int H, int L,
                                                           float* __restrict__ probs, int32_t* __restrict__ label, float* __restrict__ score) {
  constexpr int BM = SMALL ? 32 : 128, BN = SMALL ? 32 : 64;
  constexpr int SROWS = SC_BLOCK / SC_BK, XV = BM / SROWS, WV = BN / SROWS;
  constexpr int HLD = BN + 1;                          // pitch of the tanh tile
  constexpr int ZLD = SC_MAX_L + 1;                    // pitch of the logit rows
  constexpr int ZV = BM * SC_MAX_L / SC_BLOCK;         // logit chains per thread at L = 64
  __shared__ float xs[BM][SC_LD];
  __shared__ float ws[BN][SC_LD];
  __shared__ float hz[BM * (ZLD > HLD ? ZLD : HLD)];   // the tanh tile [BM][HLD] while the tiles run, the logits [BM][ZLD] after them
  const int tid = threadIdx.x, wave = tid / SC_WAVE, lane = tid % SC_WAVE;
  const int64_t r0 = (int64_t)blockIdx.x * BM;
  const int nr = (int)min((int64_t)BM, N - r0);
  const int sk = tid % SC_BK, sr = tid / SC_BK;
  const int npair = BM * L;                            // chain p = l * BM + row; thread tid holds p = tid + i * SC_BLOCK
  float z[ZV];
#pragma unroll
  for (int i = 0; i < ZV; ++i) {
    const int p = tid + i * SC_BLOCK;
    z[i] = p < npair ? bo[p / BM] : 0.f;
  }
  float xv[XV], wv[WV];
  for (int o0 = 0; o0 < H; o0 += BN) {
    auto fetch = [&](int k0) {
      const bool kin = k0 + sk < H;
#pragma unroll
      for (int i = 0; i < XV; ++i) {
        const int rr = sr + i * SROWS;
        xv[i] = (kin && rr < nr) ? x[(size_t)(r0 + rr) * ldx + k0 + sk] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < WV; ++i) {
        const int oo = sr + i * SROWS;
        wv[i] = (kin && o0 + oo < H) ? Wd[(size_t)(o0 + oo) * H + k0 + sk] : 0.f;
      }
    };
    f32x16 acc0, acc1;
    f32x4 accs;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
#pragma unroll
    for (int i = 0; i < 4; ++i) accs[i] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < H; k0 += SC_BK) {
      __syncthreads();                                   // the previous step's operands, and the previous tile's tanh tile, are read
#pragma unroll
      for (int i = 0; i < XV; ++i) xs[sr + i * SROWS][sk] = xv[i];
#pragma unroll
      for (int i = 0; i < WV; ++i) ws[sr + i * SROWS][sk] = wv[i];
      __syncthreads();
      if (k0 + SC_BK < H) fetch(k0 + SC_BK);
      if constexpr (SMALL) {                             // A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
        const int ar = (wave >> 1) * 16 + (lane & 15), br = (wave & 1) * 16 + (lane & 15), kq = lane >> 4;
#pragma unroll
        for (int kk = 0; kk < SC_BK; kk += 4) accs = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[ar][kk + kq], ws[br][kk + kq], accs, 0, 0, 0);
      } else {                                           // A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
        const int ar = wave * 32 + (lane & 31), kh = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < SC_BK; kk += 2) {
          const float a = xs[ar][kk + kh];
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ws[lane & 31][kk + kh], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ws[32 + (lane & 31)][kk + kh], acc1, 0, 0, 0);
        }
      }
    }
    // the tile's epilogue: tanh into LDS, then every chain takes the tile's columns in ascending order
    auto put = [&](int rr, int oo, float v) {
      const int o = o0 + oo;
      hz[rr * HLD + oo] = o < H ? tanhf(v + bd[o]) : 0.f;
    };
    if constexpr (SMALL) {                               // C / D map: column = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) put((wave >> 1) * 16 + 4 * (lane >> 4) + reg, (wave & 1) * 16 + (lane & 15), accs[reg]);
    } else {                                             // C / D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int rr = wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        put(rr, lane & 31, acc0[reg]);
        put(rr, 32 + (lane & 31), acc1[reg]);
      }
    }
    __syncthreads();
    const int cols = min(BN, H - o0);
#pragma unroll
    for (int i = 0; i < ZV; ++i) {
      const int p = tid + i * SC_BLOCK;
      if (p < npair) {
        const int l = p / BM, rr = p % BM;
        const float* wo = Wo + (size_t)l * H + o0;       // one or two l per wave: the loads are broadcasts, Wo stays in L2
        float v = z[i];
#pragma unroll 8
        for (int oo = 0; oo < cols; ++oo) v = fmaf(hz[rr * HLD + oo], wo[oo], v);
        z[i] = v;
      }
    }
  }
  __syncthreads();                                       // every chain has read the last tanh tile
#pragma unroll
  for (int i = 0; i < ZV; ++i) {
    const int p = tid + i * SC_BLOCK;
    if (p < npair) hz[(p % BM) * ZLD + p / BM] = z[i];
  }
  __syncthreads();
  if (tid < nr) {                                        // one thread per row: L <= 64 logits
    float* zr = hz + tid * ZLD;
    const int64_t r = r0 + tid;
    float mx = zr[0];
    bool finite = true;
    for (int l = 0; l < L; ++l) {
      const float v = zr[l];
      finite = finite && (fabsf(v) <= 3.402823466e38f);  // false for NaN and for an infinity
      mx = fmaxf(mx, v);
    }
    if (!finite) {                                       // a non-finite logit: no class, and nothing to rank by
      const float q = __builtin_nanf("");
      label[r] = -1;
      score[r] = q;
      if (probs) for (int l = 0; l < L; ++l) probs[(size_t)r * L + l] = q;
      return;
    }
    float sum = 0.f;
    for (int l = 0; l < L; ++l) {                        // the exponentials replace the logits of this row, summed in ascending order
      const float e = expf(zr[l] - mx);
      zr[l] = e;
      sum += e;
    }
    int a = 0;
    float pa = zr[0] / sum;
    const float p0 = pa;
    float pl = pa;
    for (int l = 0; l < L; ++l) {
      pl = zr[l] / sum;
      if (probs) probs[(size_t)r * L + l] = pl;
      if (pl > pa) { pa = pl; a = l; }                   // strict, on the probabilities: the lowest index at a tie, as numpy.argmax
    }
    label[r] = a;
    // the reference's rule; its third branch reads positions L - 1 and 0 whatever those labels are named
    score[r] = a == pos_idx ? pa : (a == neg_idx ? -pa : (1.0f - pa) * (pl - p0));
  }
}

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" int manner_hip_seqcls_head(const float* x, int64_t ldx, const float* dense_w, const float* dense_b, const float* out_w,
                                      const float* out_b, int64_t N, int32_t H, int32_t L, int32_t pos_idx, int32_t neg_idx, float* probs,
                                      int32_t* label, float* score, manner_hip_stream_t stream) {
  if (L < 1 || L > SC_MAX_L) return fail(MANNER_HIP_E_INVALID, "seqcls_head: L=%d unsupported (1 <= L <= %d)", (int)L, SC_MAX_L);
  if (H < 4 || H > SC_MAX_H || H % 4) return fail(MANNER_HIP_E_INVALID, "seqcls_head: H=%d unsupported (a multiple of 4, H <= %d)", (int)H, SC_MAX_H);
  if (N < 0 || N > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "seqcls_head: N=%lld outside [0, 2^31)", (long long)N);
  if (ldx < H) return fail(MANNER_HIP_E_INVALID, "seqcls_head: ldx=%lld below H=%d", (long long)ldx, (int)H);
  if (pos_idx < -1 || pos_idx >= L || neg_idx < -1 || neg_idx >= L)
    return fail(MANNER_HIP_E_INVALID, "seqcls_head: pos_idx=%d / neg_idx=%d outside [-1, L)", (int)pos_idx, (int)neg_idx);
  if (!dense_w || !dense_b || !out_w || !out_b || (N > 0 && (!x || !label || !score))) return fail(MANNER_HIP_E_INVALID, "seqcls_head: null pointer");
  if (N == 0) return MANNER_HIP_OK;
  hipStream_t s = (hipStream_t)stream;
  if (N < SC_SMALL_ROWS)
    hipLaunchKernelGGL((seqcls_kernel<true>), dim3((unsigned)((N + 31) / 32)), dim3(SC_BLOCK), 0, s, x, ldx, dense_w, dense_b, out_w, out_b,
                       (int)pos_idx, (int)neg_idx, N, (int)H, (int)L, probs, label, score);
  else
    hipLaunchKernelGGL((seqcls_kernel<false>), dim3((unsigned)((N + 127) / 128)), dim3(SC_BLOCK), 0, s, x, ldx, dense_w, dense_b, out_w, out_b,
                       (int)pos_idx, (int)neg_idx, N, (int)H, (int)L, probs, label, score);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}
