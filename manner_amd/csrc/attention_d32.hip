// K3 at head_dim 32 (the MiniLM family: hidden 384, 12 heads): the kernels of attention.hip restated for a head whose row is 64 bytes
// (16-bit) / 128 bytes (f32).  H % 128 == 0 with H = 32 heads means heads % 4 == 0, so the unit of work is a (news, head PAIR): two
// adjacent heads are one 128-byte (256-byte) segment of Q, K and V per token, and every global access, the LDS-DMA of V, the slab
// swizzles and the transposed V reads keep the shape they have at head_dim 64.  What changes is the arithmetic per head:
//   S^T = K Q^T   depth 32: head a of the pair takes k-steps 2a, 2a+1 of the four the 64-wide segment holds (16-bit), or 16 of the 32
//                 f32 steps — lane half h then holds features 32a + 16h .. + 15 of its row;
//   O^T = V^T P^T one 32-row block per head: block a of the two, fed with head a's softmax numerators;
//   softmax       each head keeps its own running max / sum; the scale is 32^-0.5.
// The dispatch (attention_varlen / attention_cls in attention.hip) sends H / heads == 32 here; head_dim 64 never reaches this file.
// Inference only: no split-operand (x3) output, no training kernels.
#include <math.h>

#include "common.h"

namespace manner {
namespace {

constexpr float SCALE32 = 0.17677669529663687f;                       // 32^-0.5
constexpr float C32 = 0.17677669529663687f * 1.44269504088896340736f;  // 32^-0.5 * log2(e)

// ---- short rows, 16-bit: one wave per (news, head pair); memory traffic exactly as attn_wave_bf16 moves it
template <typename TE, int NKT>
__device__ __forceinline__ void attn32_wave16(const TE* __restrict__ qkv, TE* __restrict__ ctx, int tok0, int L, int H, int hp,
                                              char* vl) {
  typedef typename E16<TE>::v8 e16x8;
  typedef typename E16<TE>::v4 e16x4;
  const int lane = threadIdx.x & 63, rr = lane & 31, h = lane >> 5;
  char* ol = vl + NKT * 32 * 128;                 // output slab behind the V image
  const size_t ld = 3 * (size_t)H;
  const TE* Qb = qkv + (size_t)tok0 * ld + hp * 64;
  const TE* Kb = Qb + H;
  const TE* Vb = Qb + 2 * H;
  const int r8 = lane >> 3, c8 = lane & 7;        // 16-byte piece c8 of the 128-byte segment of row r8 of an 8-row group
  f32x4 kt_[NKT][4], qt_[4];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = min(32 * kt + 8 * i + r8, L - 1);      // rows >= L replicate row L-1 (finite; masked / weighted by 0)
      kt_[kt][i] = *reinterpret_cast<const f32x4*>(Kb + (size_t)row * ld + 8 * (c8 ^ (((8 * i + r8) >> 1) & 7)));
    }
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = min(32 * kt + 8 * i + r8, L - 1);
      __builtin_amdgcn_global_load_lds(GLOBAL_PTR(Vb + (size_t)row * ld + 8 * c8), LDS_PTR(vl + (32 * kt + 8 * i) * 128), 16, 0, 0);
    }
  auto load_q = [&](int qb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = min(32 * qb + 8 * i + r8, L - 1);
      qt_[i] = *reinterpret_cast<const f32x4*>(Qb + (size_t)row * ld + 8 * (c8 ^ (((8 * i + r8) >> 1) & 7)));
    }
  };
  load_q(0);
  // K through the slab: lane (rr, h) holds K[key 32kt + rr][d = 16ks + 8h .. +7] of the PAIR's 64 columns — k-steps 0, 1 are head 0
  // of the pair, k-steps 2, 3 head 1
  e16x8 kf[NKT][4];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(ol + (8 * i + r8) * 128 + (c8 << 4)) = kt_[kt][i];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      kf[kt][ks] = *reinterpret_cast<const e16x8*>(ol + rr * 128 + (((2 * ks + h) ^ ((rr >> 1) & 7)) << 4));
    __builtin_amdgcn_wave_barrier();
  }
  const int gi = lane & 15;
  const int tr_base = ((gi >> 2) * 64 + 16 * ((lane >> 4) & 1) + 4 * (gi & 3)) * 2 + (4 * h) * 128;

#pragma unroll
  for (int qb = 0; qb < NKT; ++qb) {
    if (32 * qb >= L) break;
    e16x8 qfb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(ol + (8 * i + r8) * 128 + (c8 << 4)) = qt_[i];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      qfb[ks] = *reinterpret_cast<const e16x8*>(ol + rr * 128 + (((2 * ks + h) ^ ((rr >> 1) & 7)) << 4));
    __builtin_amdgcn_wave_barrier();
    if (qb == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the V image (LDS-DMA is not tracked by the compiler)
    if (qb + 1 < NKT && 32 * (qb + 1) < L) load_q(qb + 1);
    // head by head (one O^T block and one softmax state live at a time; both heads at once spill): online softmax over the 32-key
    // tiles, then O^T of the head -> its half of the output slab (chunks 4a .. 4a+3 of the 128-byte row; the slab is free once
    // the Q fragments of BOTH heads have been read, above)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float m = -INFINITY, l = 0.f;
      f32x16 o;
#pragma unroll
      for (int e = 0; e < 16; ++e) o[e] = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        f32x16 st;
#pragma unroll
        for (int e = 0; e < 16; ++e) st[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) st = E16<TE>::mfma32(kf[kt][2 * a + ks], qfb[2 * a + ks], st);
        if (kt == NKT - 1) {                           // L > 32 (NKT - 1): earlier tiles hold real keys only
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int key = 32 * kt + (e & 3) + 8 * (e >> 2) + 4 * h;
            st[e] = key < L ? st[e] : -INFINITY;
          }
        }
        float tmx = fmaxf(fmaxf(fmaxf(st[0], st[1]), fmaxf(st[2], st[3])), fmaxf(fmaxf(st[4], st[5]), fmaxf(st[6], st[7])));
        tmx = fmaxf(tmx, fmaxf(fmaxf(fmaxf(st[8], st[9]), fmaxf(st[10], st[11])), fmaxf(fmaxf(st[12], st[13]), fmaxf(st[14], st[15]))));
        tmx = fmaxf(tmx, __shfl_xor(tmx, 32, 64));
        const float mn = fmaxf(m, tmx);                // finite: tile 0 always holds key 0 < L
        const float nmc = -mn * C32;
        float rs = 0.f;
        e16x8 pf[2];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float p = __builtin_amdgcn_exp2f(fmaf(st[e], C32, nmc));   // exp((s - max) / sqrt(32)); 0 for masked keys
          pf[e >> 3][e & 7] = (TE)p;
          rs += p;
        }
        rs += __shfl_xor(rs, 32, 64);
        if (kt == 0) {
          l = rs;
        } else {
          const float alpha = __builtin_amdgcn_exp2f((m - mn) * C32);
          l = l * alpha + rs;
          if (__any(mn > m)) {                         // wave-uniform: some query's running max moved
#pragma unroll
            for (int e = 0; e < 16; ++e) o[e] *= alpha;
          }
        }
        m = mn;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const char* a0 = vl + tr_base + (32 * kt + 16 * s2) * 128 + (32 * a) * 2;
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 8 * 128));
          typedef short s16x8 __attribute__((ext_vector_type(8)));
          const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o = E16<TE>::mfma32(__builtin_bit_cast(e16x8, both), pf[s2], o);
        }
      }
      const float inv = 1.0f / l;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 4 * a + g;
        *reinterpret_cast<e16x4*>(ol + rr * 128 + ((c ^ ((rr >> 1) & 7)) << 4) + 8 * h) =
            e16x4{(TE)(o[4 * g] * inv), (TE)(o[4 * g + 1] * inv), (TE)(o[4 * g + 2] * inv), (TE)(o[4 * g + 3] * inv)};
      }
    }
    // the slab -> ctx rows as whole 128-byte row segments (attn_wave_bf16)
    {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 8 * i + r8;
        const int q = 32 * qb + row;
        const f32x4 v = *reinterpret_cast<const f32x4*>(ol + row * 128 + (c8 << 4));
        if (q < L) *reinterpret_cast<f32x4*>(ctx + (size_t)(tok0 + q) * H + hp * 64 + 8 * (c8 ^ ((row >> 1) & 7))) = v;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

template <typename TE>
__global__ __launch_bounds__(256, 2) void attn32_16_kernel(const TE* __restrict__ qkv, TE* __restrict__ ctx,
                                                           const int32_t* __restrict__ cu, int64_t n_units, int hpairs, int H,
                                                           int lds_per_wave) {
  extern __shared__ __attribute__((aligned(16))) char vlds[];
  const int wave = threadIdx.x >> 6;
  const int64_t unit = (int64_t)blockIdx.x * 4 + wave;
  if (unit >= n_units) return;
  const int n = (int)(unit / hpairs), hp = (int)(unit - (int64_t)n * hpairs);
  const int tok0 = __builtin_amdgcn_readfirstlane(cu[n]);
  const int L = __builtin_amdgcn_readfirstlane(cu[n + 1]) - tok0;
  if (L <= 0 || L > MANNER_HIP_MAX_LEN) return;      // wave-uniform: a long row (attn32_long16_kernel)
  char* vl = vlds + wave * lds_per_wave;
  if (L <= 32) attn32_wave16<TE, 1>(qkv, ctx, tok0, L, H, hp, vl);
  else if (L <= 64) attn32_wave16<TE, 2>(qkv, ctx, tok0, L, H, hp, vl);
  else if (L <= 96) attn32_wave16<TE, 3>(qkv, ctx, tok0, L, H, hp, vl);
  else attn32_wave16<TE, 4>(qkv, ctx, tok0, L, H, hp, vl);
}

// ---- short rows, exact f32 on the f32 matrix pipe: attn_wave_f32 per head pair.  Lane (row rr, half h) holds, for head a of the
// pair, the 16 features 32a + 16h .. + 15 of its K / Q row: MFMA step s pairs feature s with feature 16 + s of the head, for Q and
// K alike.
template <int NKT>
__device__ __forceinline__ void attn32_wave_f32(const float* __restrict__ qkv, float* __restrict__ ctx, int tok0, int L, int H,
                                                int hp, char* vl) {
  const int lane = threadIdx.x & 63, rr = lane & 31, h = lane >> 5;
  char* ol = vl + NKT * 32 * 256;                 // 8 KiB slab (32 rows x 256 B) behind the V image
  const size_t ld = 3 * (size_t)H;
  const float* Qb = qkv + (size_t)tok0 * ld + hp * 64;
  const float* Kb = Qb + H;
  const float* Vb = Qb + 2 * H;
  const int r4 = lane >> 4, c16 = lane & 15;      // coalesced piece: row r4 of a 4-row group, 16-byte chunk c16 of 16
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = min(32 * kt + 4 * i + r4, L - 1);
      __builtin_amdgcn_global_load_lds(GLOBAL_PTR(Vb + (size_t)row * ld + 4 * c16), LDS_PTR(vl + (32 * kt + 4 * i) * 256), 16, 0, 0);
    }
  // a 32-row tile of K or Q: coalesced rows -> slab (16-byte chunks XOR-swizzled with row & 15) -> frag[a][4j .. 4j+3] = chunk
  // 8a + 4h + j of row rr
  auto tile_to_frag = [&](const float* base, int row0, float (&frag)[2][16]) {
    f32x4 t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = min(row0 + 4 * i + r4, L - 1);
      t[i] = *reinterpret_cast<const f32x4*>(base + (size_t)row * ld + 4 * (c16 ^ ((4 * i + r4) & 15)));
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(ol + (4 * i + r4) * 256 + (c16 << 4)) = t[i];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(ol + rr * 256 + (((8 * a + 4 * h + j) ^ (rr & 15)) << 4));
        frag[a][4 * j] = v[0]; frag[a][4 * j + 1] = v[1]; frag[a][4 * j + 2] = v[2]; frag[a][4 * j + 3] = v[3];
      }
    __builtin_amdgcn_wave_barrier();
  };
  float kf[NKT][2][16];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) tile_to_frag(Kb, 32 * kt, kf[kt]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the V image has landed (LDS-DMA is not tracked by the compiler)
#pragma unroll
  for (int qb = 0; qb < NKT; ++qb) {
    if (32 * qb >= L) break;
    float qf[2][16];
    tile_to_frag(Qb, 32 * qb, qf);
    // head by head, as attn32_wave16: one O^T block and one softmax state live at a time; lane (query rr, half h) then owns features
    // 32a + 8g + 4h .. +3 of the pair's 64 and writes them into the slab (free once both heads' Q fragments are read)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float m = -INFINITY, l = 0.f;
      f32x16 o;
#pragma unroll
      for (int e = 0; e < 16; ++e) o[e] = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        f32x16 st;
#pragma unroll
        for (int e = 0; e < 16; ++e) st[e] = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[kt][a][s2], qf[a][s2], st, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = 32 * kt + (e & 3) + 8 * (e >> 2) + 4 * h;
          st[e] = key < L ? st[e] * SCALE32 : -INFINITY;           // scores * 32^-0.5, as the reference scales them
        }
        float tmx = st[0];
#pragma unroll
        for (int e = 1; e < 16; ++e) tmx = fmaxf(tmx, st[e]);
        tmx = fmaxf(tmx, __shfl_xor(tmx, 32, 64));
        const float mn = fmaxf(m, tmx);
        float rs = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) { st[e] = expf(st[e] - mn); rs += st[e]; }
        rs += __shfl_xor(rs, 32, 64);
        const float alpha = kt == 0 ? 0.f : expf(m - mn);
        l = l * alpha + rs;
        if (kt > 0) {
#pragma unroll
          for (int e = 0; e < 16; ++e) o[e] *= alpha;
        }
        m = mn;
        // O^T += V^T P^T: MFMA step t pairs key 8(t>>2) + (t&3) (k-slot 0) with key + 4 (k-slot 1); lane rr supplies feature 32a + rr
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const float vv = *reinterpret_cast<const float*>(vl + (32 * kt + 8 * (t >> 2) + (t & 3) + 4 * h) * 256 + 128 * a + rr * 4);
          o = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, st[t], o, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);             // one score tile live at a time: key tiles interleaved by the scheduler spill
      }
      const float inv = 1.0f / l;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = (32 * a + 8 * g + 4 * h) >> 2;             // 16-byte chunk 0..15 of the 256-byte row
        *reinterpret_cast<f32x4*>(ol + rr * 256 + ((c ^ (rr & 15)) << 4)) =
            f32x4{o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv};
      }
    }
    // the slab -> ctx rows as whole 256-byte row segments
    {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int row = 4 * i + r4;
        const int q = 32 * qb + row;
        const f32x4 v = *reinterpret_cast<const f32x4*>(ol + row * 256 + (c16 << 4));
        if (q < L) *reinterpret_cast<f32x4*>(ctx + (size_t)(tok0 + q) * H + hp * 64 + 4 * (c16 ^ (row & 15))) = v;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

__global__ __launch_bounds__(128, 1) void attn32_f32_kernel(const float* __restrict__ qkv, float* __restrict__ ctx,
                                                            const int32_t* __restrict__ cu, int64_t n_units, int hpairs, int H,
                                                            int lds_per_wave) {
  extern __shared__ __attribute__((aligned(16))) char vlds[];
  const int wave = threadIdx.x >> 6;
  const int64_t unit = (int64_t)blockIdx.x * 2 + wave;
  if (unit >= n_units) return;
  const int n = (int)(unit / hpairs), hp = (int)(unit - (int64_t)n * hpairs);
  const int tok0 = __builtin_amdgcn_readfirstlane(cu[n]);
  const int L = __builtin_amdgcn_readfirstlane(cu[n + 1]) - tok0;
  if (L <= 0 || L > MANNER_HIP_MAX_LEN) return;      // a long row: attn32_long_f32_kernel
  char* vl = vlds + wave * lds_per_wave;
  if (L <= 32) attn32_wave_f32<1>(qkv, ctx, tok0, L, H, hp, vl);
  else if (L <= 64) attn32_wave_f32<2>(qkv, ctx, tok0, L, H, hp, vl);
  else if (L <= 96) attn32_wave_f32<3>(qkv, ctx, tok0, L, H, hp, vl);
  else attn32_wave_f32<4>(qkv, ctx, tok0, L, H, hp, vl);
}

// ---- long rows (MANNER_HIP_MAX_LEN < L <= MANNER_HIP_MAX_LEN_INFER), 16-bit: attn_long16_kernel per head pair — one workgroup of
// LONG_WAVES waves per (news, head pair, block of 32 LONG_WAVES queries), the whole K and V segment of the pair staged once by
// LDS-DMA (rows_cap x 256 B), one 4 KiB output slab per wave.
constexpr int LONG_WAVES = 8;

template <typename TE>
__global__ __launch_bounds__(64 * LONG_WAVES, 1) void attn32_long16_kernel(const TE* __restrict__ qkv, TE* __restrict__ ctx,
                                                                           const int32_t* __restrict__ cu, int64_t n_units, int n_qb,
                                                                           int hpairs, int H, int rows_cap) {
  typedef typename E16<TE>::v8 e16x8;
  typedef typename E16<TE>::v4 e16x4;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int64_t unit = (int64_t)blockIdx.x / n_qb;
  const int qb = (int)((int64_t)blockIdx.x - unit * n_qb);
  if (unit >= n_units) return;
  const int n = (int)(unit / hpairs), hp = (int)(unit - (int64_t)n * hpairs);
  const int tok0 = __builtin_amdgcn_readfirstlane(cu[n]);
  const int L = __builtin_amdgcn_readfirstlane(cu[n + 1]) - tok0;
  if (L <= MANNER_HIP_MAX_LEN || L > rows_cap || 32 * LONG_WAVES * qb >= L) return;   // workgroup-uniform: a short row / past the row
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, rr = lane & 31, h = lane >> 5;
  const int r8 = lane >> 3, c8 = lane & 7;
  char* kimg = lds;
  char* vimg = lds + (size_t)rows_cap * 128;
  char* ol = lds + (size_t)rows_cap * 256 + wave * 4096;
  const size_t ld = 3 * (size_t)H;
  const TE* Qb = qkv + (size_t)tok0 * ld + hp * 64;
  const TE* Kb = Qb + H;
  const TE* Vb = Qb + 2 * H;
  const int nrows = (L + 31) & ~31;                   // <= rows_cap (a multiple of 32 that is >= L)
  const int q0 = 32 * LONG_WAVES * qb + 32 * wave;
  f32x4 qt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = min(q0 + 8 * i + r8, L - 1);
    qt[i] = *reinterpret_cast<const f32x4*>(Qb + (size_t)row * ld + 8 * (c8 ^ (((8 * i + r8) >> 1) & 7)));
  }
  for (int r0 = 8 * wave; r0 < nrows; r0 += 8 * LONG_WAVES) {
    const int row = min(r0 + r8, L - 1);
    __builtin_amdgcn_global_load_lds(GLOBAL_PTR(Kb + (size_t)row * ld + 8 * (c8 ^ (((r0 + r8) >> 1) & 7))), LDS_PTR(kimg + r0 * 128), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(GLOBAL_PTR(Vb + (size_t)row * ld + 8 * c8), LDS_PTR(vimg + r0 * 128), 16, 0, 0);
  }
  e16x8 qf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(ol + (8 * i + r8) * 128 + (c8 << 4)) = qt[i];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    qf[ks] = *reinterpret_cast<const e16x8*>(ol + rr * 128 + (((2 * ks + h) ^ ((rr >> 1) & 7)) << 4));
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's share of the K / V images (LDS-DMA is not tracked by the compiler)
  __syncthreads();                                      // ... and every other wave's
  if (q0 >= L) return;                                  // wave-uniform: no query of this wave is real (no barrier follows)

  const int gi = lane & 15;
  const int tr_base = ((gi >> 2) * 64 + 16 * ((lane >> 4) & 1) + 4 * (gi & 3)) * 2 + (4 * h) * 128;
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
  f32x16 o[2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[a][e] = 0.f;
  const int nkt = nrows >> 5;
  for (int kt = 0; kt < nkt; ++kt) {
    e16x8 kf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      kf[ks] = *reinterpret_cast<const e16x8*>(kimg + (32 * kt + rr) * 128 + (((2 * ks + h) ^ ((rr >> 1) & 7)) << 4));
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      f32x16 st;
#pragma unroll
      for (int e = 0; e < 16; ++e) st[e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) st = E16<TE>::mfma32(kf[2 * a + ks], qf[2 * a + ks], st);
      if (32 * kt + 32 > L) {                             // wave-uniform: the last tile holds keys >= L
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = 32 * kt + (e & 3) + 8 * (e >> 2) + 4 * h;
          st[e] = key < L ? st[e] : -INFINITY;
        }
      }
      float tmx = fmaxf(fmaxf(fmaxf(st[0], st[1]), fmaxf(st[2], st[3])), fmaxf(fmaxf(st[4], st[5]), fmaxf(st[6], st[7])));
      tmx = fmaxf(tmx, fmaxf(fmaxf(fmaxf(st[8], st[9]), fmaxf(st[10], st[11])), fmaxf(fmaxf(st[12], st[13]), fmaxf(st[14], st[15]))));
      tmx = fmaxf(tmx, __shfl_xor(tmx, 32, 64));
      const float mn = fmaxf(m[a], tmx);                  // finite: tile 0 always holds key 0 < L
      const float nmc = -mn * C32;
      float rs = 0.f;
      e16x8 pf[2];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float p = __builtin_amdgcn_exp2f(fmaf(st[e], C32, nmc));
        pf[e >> 3][e & 7] = (TE)p;
        rs += p;
      }
      rs += __shfl_xor(rs, 32, 64);
      if (kt == 0) {
        l[a] = rs;
      } else {
        const float alpha = __builtin_amdgcn_exp2f((m[a] - mn) * C32);
        l[a] = l[a] * alpha + rs;
        if (__any(mn > m[a])) {
#pragma unroll
          for (int e = 0; e < 16; ++e) o[a][e] *= alpha;
        }
      }
      m[a] = mn;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const char* a0 = vimg + tr_base + (32 * kt + 16 * s2) * 128 + (32 * a) * 2;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 8 * 128));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[a] = E16<TE>::mfma32(__builtin_bit_cast(e16x8, both), pf[s2], o[a]);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const float inv = 1.0f / l[a];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 4 * a + g;
      *reinterpret_cast<e16x4*>(ol + rr * 128 + ((c ^ ((rr >> 1) & 7)) << 4) + 8 * h) =
          e16x4{(TE)(o[a][4 * g] * inv), (TE)(o[a][4 * g + 1] * inv), (TE)(o[a][4 * g + 2] * inv), (TE)(o[a][4 * g + 3] * inv)};
    }
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 8 * i + r8;
    const int q = q0 + row;
    const f32x4 v = *reinterpret_cast<const f32x4*>(ol + row * 128 + (c8 << 4));
    if (q < L) *reinterpret_cast<f32x4*>(ctx + (size_t)(tok0 + q) * H + hp * 64 + 8 * (c8 ^ ((row >> 1) & 7))) = v;
  }
}

// ---- long rows, exact f32: attn_long_f32_kernel per head pair (K and V streamed through the LDS in chunks of LONGF_KC keys)
constexpr int LONGF_WAVES = 4, LONGF_KC = 128;
constexpr int LONGF_LDS = 2 * LONGF_KC * 256 + LONGF_WAVES * 8192;

__global__ __launch_bounds__(64 * LONGF_WAVES, 1) void attn32_long_f32_kernel(const float* __restrict__ qkv, float* __restrict__ ctx,
                                                                              const int32_t* __restrict__ cu, int64_t n_units, int n_qb,
                                                                              int hpairs, int H) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int64_t unit = (int64_t)blockIdx.x / n_qb;
  const int qb = (int)((int64_t)blockIdx.x - unit * n_qb);
  if (unit >= n_units) return;
  const int n = (int)(unit / hpairs), hp = (int)(unit - (int64_t)n * hpairs);
  const int tok0 = __builtin_amdgcn_readfirstlane(cu[n]);
  const int L = __builtin_amdgcn_readfirstlane(cu[n + 1]) - tok0;
  if (L <= MANNER_HIP_MAX_LEN || 32 * LONGF_WAVES * qb >= L) return;     // workgroup-uniform
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, rr = lane & 31, h = lane >> 5;
  const int r4 = lane >> 4, c16 = lane & 15;
  char* kimg = lds;
  char* vimg = lds + LONGF_KC * 256;
  char* ol = lds + 2 * LONGF_KC * 256 + wave * 8192;
  const size_t ld = 3 * (size_t)H;
  const float* Qb = qkv + (size_t)tok0 * ld + hp * 64;
  const float* Kb = Qb + H;
  const float* Vb = Qb + 2 * H;
  const int q0 = 32 * LONGF_WAVES * qb + 32 * wave;
  const bool active = q0 < L;                           // wave-uniform; an idle wave still takes part in the chunk loads and barriers
  float qf[2][16];
  {
    f32x4 t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = min(q0 + 4 * i + r4, L - 1);
      t[i] = *reinterpret_cast<const f32x4*>(Qb + (size_t)row * ld + 4 * (c16 ^ ((4 * i + r4) & 15)));
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(ol + (4 * i + r4) * 256 + (c16 << 4)) = t[i];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(ol + rr * 256 + (((8 * a + 4 * h + j) ^ (rr & 15)) << 4));
        qf[a][4 * j] = v[0]; qf[a][4 * j + 1] = v[1]; qf[a][4 * j + 2] = v[2]; qf[a][4 * j + 3] = v[3];
      }
    __builtin_amdgcn_wave_barrier();
  }
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
  f32x16 o[2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[a][e] = 0.f;
  for (int c0 = 0; c0 < L; c0 += LONGF_KC) {
    const int rows = min(LONGF_KC, (L - c0 + 31) & ~31);
    __syncthreads();                                    // every wave is done with the previous chunk
    for (int r0 = 4 * wave; r0 < rows; r0 += 4 * LONGF_WAVES) {   // 4 rows x 256 B per instruction
      const int row = min(c0 + r0 + r4, L - 1);
      __builtin_amdgcn_global_load_lds(GLOBAL_PTR(Kb + (size_t)row * ld + 4 * (c16 ^ ((r0 + r4) & 15))), LDS_PTR(kimg + r0 * 256), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(GLOBAL_PTR(Vb + (size_t)row * ld + 4 * c16), LDS_PTR(vimg + r0 * 256), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) continue;
    for (int kt = 0; kt < (rows >> 5); ++kt) {
      const int kbase = c0 + 32 * kt;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        float kf[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(kimg + (32 * kt + rr) * 256 + (((8 * a + 4 * h + j) ^ (rr & 15)) << 4));
          kf[4 * j] = v[0]; kf[4 * j + 1] = v[1]; kf[4 * j + 2] = v[2]; kf[4 * j + 3] = v[3];
        }
        f32x16 st;
#pragma unroll
        for (int e = 0; e < 16; ++e) st[e] = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[s2], qf[a][s2], st, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = kbase + (e & 3) + 8 * (e >> 2) + 4 * h;
          st[e] = key < L ? st[e] * SCALE32 : -INFINITY;
        }
        float tmx = st[0];
#pragma unroll
        for (int e = 1; e < 16; ++e) tmx = fmaxf(tmx, st[e]);
        tmx = fmaxf(tmx, __shfl_xor(tmx, 32, 64));
        const float mn = fmaxf(m[a], tmx);
        float rs = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) { st[e] = expf(st[e] - mn); rs += st[e]; }
        rs += __shfl_xor(rs, 32, 64);
        const float alpha = kbase == 0 ? 0.f : expf(m[a] - mn);
        l[a] = l[a] * alpha + rs;
        if (kbase > 0) {
#pragma unroll
          for (int e = 0; e < 16; ++e) o[a][e] *= alpha;
        }
        m[a] = mn;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const float vv = *reinterpret_cast<const float*>(vimg + (32 * kt + 8 * (t >> 2) + (t & 3) + 4 * h) * 256 + 128 * a + rr * 4);
          o[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, st[t], o[a], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const float inv = 1.0f / l[a];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = (32 * a + 8 * g + 4 * h) >> 2;
      *reinterpret_cast<f32x4*>(ol + rr * 256 + ((c ^ (rr & 15)) << 4)) =
          f32x4{o[a][4 * g] * inv, o[a][4 * g + 1] * inv, o[a][4 * g + 2] * inv, o[a][4 * g + 3] * inv};
    }
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = 4 * i + r4;
    const int q = q0 + row;
    const f32x4 v = *reinterpret_cast<const f32x4*>(ol + row * 256 + (c16 << 4));
    if (q < L) *reinterpret_cast<f32x4*>(ctx + (size_t)(tok0 + q) * H + hp * 64 + 4 * (c16 ^ (row & 15))) = v;
  }
}

// ---- last layer: one query ([CLS]) per news.  One wave per (news, head pair); lane (g = lane>>3, c = lane&7) walks key rows g, g+8,
// ... and owns the 8 columns 8c .. 8c+7 of the pair's 64, i.e. a quarter of head c>>2: a score is the sum over the FOUR lanes of a
// head (xor 1, 2), and the softmax state of a lane is that of its head.  Rows of any length up to MANNER_HIP_MAX_LEN_INFER: the
// softmax runs online over 128-key blocks.  f32 arithmetic in all three element types.
template <typename T> struct Row8;
template <> struct Row8<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float v[8]) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float v[8]) {
    bf16x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (bf16_t)v[e];
    *reinterpret_cast<bf16x8*>(p) = t;
  }
};
template <> struct Row8<f16_t> {
  static __device__ __forceinline__ void load(const f16_t* p, float v[8]) {
    const f16x8 t = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
  }
  static __device__ __forceinline__ void store(f16_t* p, const float v[8]) {
    f16x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (f16_t)v[e];
    *reinterpret_cast<f16x8*>(p) = t;
  }
};
template <> struct Row8<float> {
  static __device__ __forceinline__ void load(const float* p, float v[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
  }
  static __device__ __forceinline__ void store(float* p, const float v[8]) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
  }
};

template <typename T>
__global__ __launch_bounds__(256) void attn32_cls_kernel(const T* __restrict__ qcls, const T* __restrict__ kv, T* __restrict__ ctx,
                                                         const int32_t* __restrict__ cu, int64_t n_units, int hpairs, int H) {
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= n_units) return;
  const int lane = threadIdx.x & 63, g = lane >> 3, c = lane & 7;
  const int n = (int)(unit / hpairs), hp = (int)(unit - (int64_t)n * hpairs);
  const int tok0 = cu[n], L = cu[n + 1] - tok0;
  if (L <= 0) return;
  const size_t ld = 2 * (size_t)H;
  const T* Kb = kv + (size_t)tok0 * ld + hp * 64 + 8 * c;
  const T* Vb = Kb + H;
  float q[8];
  Row8<T>::load(qcls + (size_t)n * H + hp * 64 + 8 * c, q);
  constexpr int MAXR = MANNER_HIP_MAX_LEN / 8;       // 16 key rows per lane group and block
  float m = -INFINITY, sum = 0.f, o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < L; b0 += MANNER_HIP_MAX_LEN) {
    float sc[MAXR];
    float bm = -INFINITY;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
      const int key = b0 + 8 * r + g;
      float s = -INFINITY;
      if (b0 + 8 * r < L) {                           // wave-uniform
        float kr[8];
        Row8<T>::load(Kb + (size_t)min(key, L - 1) * ld, kr);
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(q[e], kr[e], d);
        d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64);      // the four lanes of this lane's head
        s = key < L ? d * SCALE32 : -INFINITY;
      }
      sc[r] = s;
      bm = fmaxf(bm, s);
    }
    bm = fmaxf(bm, __shfl_xor(bm, 8, 64)); bm = fmaxf(bm, __shfl_xor(bm, 16, 64)); bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float mn = fmaxf(m, bm);                    // finite: every block holds key b0 < L
    const float alpha = b0 == 0 ? 0.f : expf(m - mn);
    sum *= alpha;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] *= alpha;
    m = mn;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
      if (b0 + 8 * r < L) {
        const int key = b0 + 8 * r + g;
        const float p = expf(sc[r] - mn);             // 0 for masked keys
        sum += p;
        float vr[8];
        Row8<T>::load(Vb + (size_t)min(key, L - 1) * ld, vr);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = fmaf(p, vr[e], o[e]);
      }
    }
  }
  // over the eight row groups (xor 8, 16, 32 keeps the column piece c, hence the head)
  sum += __shfl_xor(sum, 8, 64); sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    o[e] += __shfl_xor(o[e], 8, 64); o[e] += __shfl_xor(o[e], 16, 64); o[e] += __shfl_xor(o[e], 32, 64);
  }
  if (g == 0) {
    const float inv = 1.0f / sum;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] *= inv;
    Row8<T>::store(ctx + (size_t)n * H + hp * 64 + 8 * c, o);
  }
}

}  // namespace

int attention_cls_d32(DType dt, const void* qcls, const void* kv, void* ctx_cls, const int32_t* cu, int64_t n_news, int heads, int H,
                      hipStream_t stream) {
  if (H != heads * 32 || heads % 2) return fail(MANNER_HIP_E_INVALID, "attention_cls_d32: H=%d heads=%d", H, heads);
  const int hpairs = heads / 2;
  const int64_t units = n_news * hpairs;
  if (units <= 0) return MANNER_HIP_OK;
  dim3 g((unsigned)((units + 3) / 4)), b(256);
  if (dt == DT_BF16)
    hipLaunchKernelGGL(attn32_cls_kernel<bf16_t>, g, b, 0, stream, static_cast<const bf16_t*>(qcls), static_cast<const bf16_t*>(kv),
                       static_cast<bf16_t*>(ctx_cls), cu, units, hpairs, H);
  else if (dt == DT_F16)
    hipLaunchKernelGGL(attn32_cls_kernel<f16_t>, g, b, 0, stream, static_cast<const f16_t*>(qcls), static_cast<const f16_t*>(kv),
                       static_cast<f16_t*>(ctx_cls), cu, units, hpairs, H);
  else
    hipLaunchKernelGGL(attn32_cls_kernel<float>, g, b, 0, stream, static_cast<const float*>(qcls), static_cast<const float*>(kv),
                       static_cast<float*>(ctx_cls), cu, units, hpairs, H);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int attention_varlen_d32(DType dt, const void* qkv, void* ctx, const int32_t* cu, int64_t n_news, int heads, int H, int max_len,
                         hipStream_t stream) {
  if (H != heads * 32 || heads % 2) return fail(MANNER_HIP_E_INVALID, "attention_varlen_d32: H=%d heads=%d", H, heads);
  if (max_len < 1 || max_len > MANNER_HIP_MAX_LEN_INFER)
    return fail(MANNER_HIP_E_INVALID, "padded length %d outside [1, %d]", max_len, MANNER_HIP_MAX_LEN_INFER);
  const int hpairs = heads / 2;
  const int64_t units = n_news * hpairs;
  if (units <= 0) return MANNER_HIP_OK;
  const bool long_rows = max_len > MANNER_HIP_MAX_LEN;
  const int short_len = long_rows ? MANNER_HIP_MAX_LEN : max_len;
  const int nkt = (short_len + 31) / 32;
  static bool lds_raised_dev[MAX_DEVICES] = {};
  bool& lds_raised = lds_raised_dev[current_device_slot()];   // the attribute is per device
  if (!lds_raised) {
    const int cap16 = 4 * (4 * 32 * 128 + 4096), capf = 2 * (4 * 32 * 256 + 8192);
    const int capl = MANNER_HIP_MAX_LEN_INFER * 256 + LONG_WAVES * 4096;   // 160 KiB
    MANNER_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(attn32_16_kernel<bf16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, cap16));
    MANNER_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(attn32_16_kernel<f16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, cap16));
    MANNER_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(attn32_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, capf));
    MANNER_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(attn32_long16_kernel<bf16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, capl));
    MANNER_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(attn32_long16_kernel<f16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, capl));
    MANNER_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(attn32_long_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LONGF_LDS));
    lds_raised = true;
  }
  if (is_16bit(dt)) {
    const int lds_per_wave = nkt * 32 * 128 + 4096;   // V image + the 32-query output slab
    const dim3 grid((unsigned)((units + 3) / 4)), block(256);
    if (dt == DT_F16)
      hipLaunchKernelGGL(attn32_16_kernel<f16_t>, grid, block, 4 * lds_per_wave, stream, static_cast<const f16_t*>(qkv),
                         static_cast<f16_t*>(ctx), cu, units, hpairs, H, lds_per_wave);
    else
      hipLaunchKernelGGL(attn32_16_kernel<bf16_t>, grid, block, 4 * lds_per_wave, stream, static_cast<const bf16_t*>(qkv),
                         static_cast<bf16_t*>(ctx), cu, units, hpairs, H, lds_per_wave);
  } else {
    const int lds_per_wave = nkt * 32 * 256 + 8192;   // f32 V image + the 32-row slab
    hipLaunchKernelGGL(attn32_f32_kernel, dim3((unsigned)((units + 1) / 2)), dim3(128), 2 * lds_per_wave, stream,
                       static_cast<const float*>(qkv), static_cast<float*>(ctx), cu, units, hpairs, H, lds_per_wave);
  }
  MANNER_LAUNCH_CHECK();
  if (!long_rows) return MANNER_HIP_OK;
  // rows of 129 .. max_len tokens: one workgroup per (news, head pair, query block); short rows return at once there
  if (is_16bit(dt)) {
    const int n_qb = (max_len + 32 * LONG_WAVES - 1) / (32 * LONG_WAVES);
    const int rows_cap = (max_len + 31) / 32 * 32;
    const int lds = rows_cap * 256 + LONG_WAVES * 4096;   // K + V images of the pair's whole row + one output slab per wave
    const dim3 grid((unsigned)(units * n_qb)), block(64 * LONG_WAVES);
    if (dt == DT_F16)
      hipLaunchKernelGGL(attn32_long16_kernel<f16_t>, grid, block, lds, stream, static_cast<const f16_t*>(qkv), static_cast<f16_t*>(ctx),
                         cu, units, n_qb, hpairs, H, rows_cap);
    else
      hipLaunchKernelGGL(attn32_long16_kernel<bf16_t>, grid, block, lds, stream, static_cast<const bf16_t*>(qkv),
                         static_cast<bf16_t*>(ctx), cu, units, n_qb, hpairs, H, rows_cap);
  } else {
    const int n_qb = (max_len + 32 * LONGF_WAVES - 1) / (32 * LONGF_WAVES);
    hipLaunchKernelGGL(attn32_long_f32_kernel, dim3((unsigned)(units * n_qb)), dim3(64 * LONGF_WAVES), LONGF_LDS, stream,
                       static_cast<const float*>(qkv), static_cast<float*>(ctx), cu, units, n_qb, hpairs, H);
  }
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // namespace manner
