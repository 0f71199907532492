// Development lab (round 6): the one work-removing GEMM design DESIGN.md named and never built — FOUR waves per
// CU, one per SIMD, each owning a 128 x 128 wave tile of the 256 x 256 workgroup tile (256 accumulator registers per lane), against
// the production main loop (8 waves, 128 x 64 wave tiles) on the same box in the same process.  Per k32 step a wave reads 8 + 8
// operand fragments for 64 v_mfma_f32_16x16x32 (0.25 ds_read_b128 per MFMA) where the production loop reads 4 + 8 for 32 (0.375):
// -33 % LDS fragment traffic, and a 4-wave barrier per K-step instead of an 8-wave one.  MAIN LOOPS ONLY, equal pipeline depth
// (cross-tile prefetch, persistent grid, the production tile order and LDS image).  Not shipped, not part of libmanner_hip.so.
//
//   VAR 0  register staging: global_load_dwordx4 -> VGPR -> ds_write_b128, two 64 KiB stages, loads one K-step ahead of their
//          ds_write (two ahead of their use); with one wave per SIMD an LDS-DMA piece's 60-100 issue cycles come straight out of
//          the matrix pipe's issue time, a global_load + ds_write_b128 pair costs ~20.
//   VAR 1  LDS-DMA (global_load_lds_dwordx4), the production pipeline (2 weight + 3 activation stages, activations two K-steps
//          ahead) with every wave issuing 8 weight + 8 activation pieces per K-step.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Imanner_amd/csrc tools/gemm4w_lab.hip -o tools/bin/gemm4w_lab
//   tools/bin/gemm4w_lab [M=65536] [check]      (check: both variants against a float64 host reference on sampled outputs)
#include <stdio.h>
#include <string.h>
#include <vector>
#include <random>
#define MANNER_W8_STAMPS 1
#include "../manner_amd/csrc/gemm.hip"
namespace manner { int fail(int code, const char* fmt, ...) { fprintf(stderr, "fail %d: %s\n", code, fmt); return code; } }
using namespace manner;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

namespace lab4 {
constexpr int BK = 64, ROWB = 128, OPB = 256 * ROWB;      // one operand tile of a K-step: 256 rows x 64 elements = 32 KiB
constexpr int NPOST = 2;                                  // clusters of a K-step behind its barrier (they compute from registers)

// cluster (0..15) in which piece p (0..15) of the next K-step is written to LDS / requested: spread over the clusters in front of the barrier
__host__ __device__ constexpr int piece_cluster(int p) { return (p * (16 - NPOST - 1)) / 16; }

template <typename TE, int VAR, bool STORE>
__global__ __launch_bounds__(256, 1) void gemm4w_kernel(const TE* __restrict__ X, const TE* __restrict__ W, float* __restrict__ Y,
                                                        int N, int K, int M, int n_tiles) {
  typedef typename E16<TE>::v8 e16x8;
  __shared__ __attribute__((aligned(1024))) char lds[(VAR == 0 ? 4 : 5) * OPB];      // 128 KiB / 160 KiB
  // ---- the production tile walk: persistent grid, XCD-remapped slot, row-panel-major tile order
  const int G = gridDim.x, blk = blockIdx.x;
  const int q8 = G >> 3, r8 = G & 7, xcd = blk & 7;
  const int slot = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blk >> 3);
  const int valid = (M / 256) * n_tiles;
  if (slot >= valid) return;
  const int my_tiles = (valid - slot + G - 1) / G;
  const int nk = K / BK;
  const int total = my_tiles * nk;                         // K-steps of this workgroup, across its tiles

  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wn = wave & 1, wm = wave >> 1;                 // wave tile: columns 128 wn .., rows 128 wm ..
  const int l15 = lane & 15, lq = lane >> 4, lrow = lane >> 3, lc = lane & 7;

  // ---- fragment addresses (the production LDS image: 128-byte rows, 16-byte chunks XOR-swizzled by (row >> 1) & 7)
  const int swz = (l15 >> 1) & 7;
  const int wfrag = (128 * wn + l15) * ROWB, xfrag = (128 * wm + l15) * ROWB;
  auto coff = [&](int s2) { return ((4 * s2 + lq) ^ swz) << 4; };
  // stage bases: VAR 0: stage s = [W | X] at s * 2 OPB;  VAR 1: W stage s at s * OPB, X stage x at 2 OPB + x * OPB
  auto wbase = [&](int cur, int xs) -> const char* { return lds + (VAR == 0 ? cur * 2 * OPB : cur * OPB); };
  auto xbase = [&](int cur, int xs) -> const char* { return lds + (VAR == 0 ? cur * 2 * OPB + OPB : 2 * OPB + xs * OPB); };

  // ---- the load stream: runs ahead of the compute stream, across tiles
  // VAR 0: wave (op = wave >> 1, hf = wave & 1) stages rows 128 hf .. + 127 of operand op: 16 pieces of 8 rows;
  // VAR 1: every wave brings rows 64 wave .. + 63 of BOTH operands: 8 + 8 pieces
  const int op = wave >> 1, hf = wave & 1;
  int ld_step = 0;                                         // the K-step the load stream requests next
  int ld_tile = slot, ld_kt = 0;
  auto tile_ptr = [&](int tile, int which /*0 W, 1 X*/, int row0) -> const TE* {
    const int mt = tile / n_tiles, nt = tile - mt * n_tiles;
    return (which == 0 ? W + (size_t)(nt * 256 + row0) * K : X + (size_t)(mt * 256 + row0) * K);
  };
  const TE* ld_w = nullptr;                                // VAR 0: this wave's operand;  VAR 1: the weight tile
  const TE* ld_x = nullptr;                                // VAR 1: the activation tile
  auto ld_point = [&]() {
    if (VAR == 0) ld_w = tile_ptr(ld_tile, op, 128 * hf + lrow) + lc * 8;
    else { ld_w = tile_ptr(ld_tile, 0, 64 * wave + lrow) ; ld_x = tile_ptr(ld_tile, 1, 64 * wave + lrow); }
  };
  ld_point();
  auto ld_advance = [&]() {                                // after a whole K-step has been requested
    ++ld_step;
    if (++ld_kt == nk) { ld_kt = 0; ld_tile += G; if (ld_step < total) ld_point(); }
  };

  // VAR 0 staging registers and LDS destinations
  e16x8 S[16];
  const int sdst = op * OPB + (128 * hf + lrow) * ROWB;    // + i * 1024 + swizzled chunk
  auto sdst_of = [&](int i) { return sdst + i * 1024 + ((lc ^ ((4 * (i & 1) + (lrow >> 1)) & 7)) << 4); };
  auto gload = [&](int i) { S[i] = *reinterpret_cast<const e16x8*>(ld_w + (size_t)(8 * i) * K + ld_kt * BK); };
  auto swrite = [&](int i, int stage) { *reinterpret_cast<e16x8*>(lds + stage * 2 * OPB + sdst_of(i)) = S[i]; };
  // VAR 1 LDS-DMA: lane -> (row lrow, source chunk lc ^ f(row)), linear 1 KiB destination per piece
  auto dma = [&](const TE* src, char* dst, int i) {
    const int voff = lrow * 0 + ((lc ^ ((4 * (i & 1) + (lane >> 4)) & 7)) * 8);
    __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + (size_t)(8 * i) * K + ld_kt * BK + voff), LDS_PTR(dst + i * 1024), 16, 0, 0);
  };

  f32x4 acc[8][8];
  e16x8 wf[2][8], xf[4];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: K-step 0 in LDS, K-step 1 requested (VAR 0: in the staging registers; VAR 1: in flight), first fragments in registers
  int xs = 0;                                              // VAR 1: activation stage of the current K-step (ring of 3)
  if (VAR == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) gload(i);
    ld_advance();
#pragma unroll
    for (int i = 0; i < 16; ++i) swrite(i, 0);
    if (ld_step < total) {
#pragma unroll
      for (int i = 0; i < 16; ++i) gload(i);
      ld_advance();
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) dma(ld_w, lds + 0 * OPB + 64 * wave * ROWB, i);
#pragma unroll
    for (int i = 0; i < 8; ++i) dma(ld_x, lds + 2 * OPB + 0 * OPB + 64 * wave * ROWB, i);
    ld_advance();
    if (ld_step < total) {
#pragma unroll
      for (int i = 0; i < 8; ++i) dma(ld_w, lds + 1 * OPB + 64 * wave * ROWB, i);
#pragma unroll
      for (int i = 0; i < 8; ++i) dma(ld_x, lds + 2 * OPB + 1 * OPB + 64 * wave * ROWB, i);
      // (ld_advance for step 1 happens when its successor's activations are issued: see the loop — VAR 1 keeps W and X streams apart)
    }
    if (ld_step < total) asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int a = 0; a < 8; ++a) wf[0][a] = *reinterpret_cast<const e16x8*>(wbase(0, 0) + wfrag + a * 16 * ROWB + coff(0));
  xf[0] = *reinterpret_cast<const e16x8*>(xbase(0, 0) + xfrag + coff(0));

  // VAR 1 bookkeeping of its two request streams: weights of step s+2 are issued behind the barrier of step s, activations of step
  // s+2 in front of it; both walk (tile, kt) on their own
  int w_tile = slot, w_kt = 2, x_tile = slot, x_kt = 2;
  if (VAR == 1) {
    auto norm = [&](int& tile, int& kt) { while (kt >= nk) { kt -= nk; tile += G; } };
    norm(w_tile, w_kt); norm(x_tile, x_kt);
  }

  // one K-step; MODE 0: steady state (two more steps follow), 1: second-to-last step of the workgroup, 2: its last step — compile-time,
  // so that the sixteen clusters of a step are ONE basic block
  auto kstep = [&](int s, auto mode_tag) {
    constexpr int MODE = decltype(mode_tag)::value;
    constexpr bool more1 = MODE <= 1, more2 = MODE == 0;
    const int cur = s & 1, nxt = cur ^ 1;
    const int xs1 = xs == 2 ? 0 : xs + 1, xs2 = xs1 == 2 ? 0 : xs1 + 1;
    const char* wb = wbase(cur, xs);
    const char* xb = xbase(cur, xs);
    const char* wb1 = wbase(nxt, xs1);
    const char* xb1 = xbase(nxt, xs1);
    const TE* xsrc = VAR == 1 && more2 ? tile_ptr(x_tile, 1, 64 * wave + lrow) : nullptr;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int s2 = c >> 3, b = c & 7;
      const int slot_c = c < 14 ? (c & 1) : c - 12;        // x-fragment slots: 0 / 1 alternate, clusters 14, 15 own slots 2, 3
      __builtin_amdgcn_sched_barrier(0);
      // -- the next K-step's operands
      if (VAR == 0) {
#pragma unroll
        for (int p = 0; p < 16; ++p)
          if (piece_cluster(p) == c) {
            if (more1) swrite(p, nxt);                     // S[p] was requested one K-step ago
            if (more2) gload(p);                           // ... and is requested again for the step after
          }
        if (c == 16 - NPOST - 1 && more2) ld_advance();
      } else {
        if (c < 4 && more2) {                              // activations two steps ahead: 2 pieces per cluster
#pragma unroll
          for (int i = 2 * c; i < 2 * c + 2; ++i) {
            const int voff = (lc ^ ((4 * (i & 1) + (lane >> 4)) & 7)) * 8;
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(xsrc + (size_t)(8 * i) * K + x_kt * BK + voff),
                                             LDS_PTR(lds + 2 * OPB + xs2 * OPB + 64 * wave * ROWB + i * 1024), 16, 0, 0);
          }
        }
        if (c == 3 && more2) { if (++x_kt == nk) { x_kt = 0; x_tile += G; } }
      }
      // -- fragments of the coming clusters
      if (c < 8) wf[1][c] = *reinterpret_cast<const e16x8*>(wb + wfrag + c * 16 * ROWB + coff(1));          // s2 = 1's weights
      if (c < 12) {                                        // cluster c + 1's activation fragment
        const int cn = c + 1;
        xf[cn & 1] = *reinterpret_cast<const e16x8*>(xb + xfrag + (cn & 7) * 16 * ROWB + coff(cn >> 3));
      } else if (c < 14) {                                 // clusters 14 and 15 (slots 2, 3): in registers before the barrier
        const int cn = c + 2;
        xf[cn - 12] = *reinterpret_cast<const e16x8*>(xb + xfrag + (cn & 7) * 16 * ROWB + coff(1));
      }
      if (c == 12) xf[1] = *reinterpret_cast<const e16x8*>(xb + xfrag + 5 * 16 * ROWB + coff(1));            // cluster 13 (slot 1)
      if (c >= 14 && more1) {                              // behind the barrier: the next K-step's first fragments from the other stage
#pragma unroll
        for (int a = 4 * (c - 14); a < 4 * (c - 14) + 4; ++a)
          wf[0][a] = *reinterpret_cast<const e16x8*>(wb1 + wfrag + a * 16 * ROWB + coff(0));
        if (c == 15) xf[0] = *reinterpret_cast<const e16x8*>(xb1 + xfrag + coff(0));
      }
      __builtin_amdgcn_sched_barrier(0);
      // -- 8 matrix instructions: one activation fragment against the wave's 8 weight fragments
#pragma unroll
      for (int a = 0; a < 8; ++a) acc[a][b] = E16<TE>::mfma16(wf[s2][a], xf[slot_c], acc[a][b]);
      __builtin_amdgcn_sched_barrier(0);
      if (c == 16 - NPOST - 1) {
        // every read of this step's stage is complete (its last two clusters compute from registers), the next step's operands are in LDS
        if (VAR == 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        else if (more2) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (VAR == 1 && more2) {                           // weights two steps ahead into the stage this step has finished with
          const TE* src = tile_ptr(w_tile, 0, 64 * wave + lrow);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int voff = (lc ^ ((4 * (i & 1) + (lane >> 4)) & 7)) * 8;
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + (size_t)(8 * i) * K + w_kt * BK + voff),
                                             LDS_PTR(lds + cur * OPB + 64 * wave * ROWB + i * 1024), 16, 0, 0);
          }
          if (++w_kt == nk) { w_kt = 0; w_tile += G; }
        }
      }
    }
    xs = xs1;
  };
  typedef std::integral_constant<int, 0> Mode0;
  typedef std::integral_constant<int, 1> Mode1;
  typedef std::integral_constant<int, 2> Mode2;

  int kt = 0, tile = slot;
  for (int s = 0; s < total; ++s) {
    if (s + 2 < total) kstep(s, Mode0{});
    else if (s + 1 < total) kstep(s, Mode1{});
    else kstep(s, Mode2{});
    if (++kt == nk) {                                      // tile done: the lab's "epilogue"
      if (STORE) {
        const int mt = tile / n_tiles, nt = tile - mt * n_tiles;
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 8; ++b) {
            const int n = nt * 256 + 128 * wn + 16 * a + 4 * lq, m = mt * 256 + 128 * wm + 16 * b + l15;
            *reinterpret_cast<f32x4*>(Y + (size_t)m * N + n) = acc[a][b];
          }
      } else {
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 8; ++b) asm volatile("" ::"a"(acc[a][b]));
      }
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      kt = 0;
      tile += G;
    }
  }
}
}  // namespace lab4

template <typename F>
static double time_us(F f, int iters) {
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  f(); f();
  CK(hipEventRecord(a, 0));
  for (int i = 0; i < iters; ++i) f();
  CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b));
  float ms; CK(hipEventElapsedTime(&ms, a, b));
  CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
  return 1e3 * ms / iters;
}

// ---- the hand-scheduled kernel (tools/gen_gemm4w_asm.py -> tools/bin/gemm4w.co): loaded as a code object, tiles from a host-built table
struct AsmKernel {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  int* table = nullptr;
  int stride = 0, grid = 0, threads = 256;
  bool load(const char* path, const char* name, int nthreads) {
    threads = nthreads;
    if (hipModuleLoad(&mod, path) != hipSuccess) { fprintf(stderr, "cannot load %s (build it: see tools/gen_gemm4w_asm.py)\n", path); return false; }
    CK(hipModuleGetFunction(&fn, mod, name));
    return true;
  }
  // the production walk: persistent grid of G workgroups, XCD-remapped slot, tile = slot + r G, row-panel-major (mt = tile / n_tiles)
  void plan(int M, int n_tiles) {
    const int valid = (M / 256) * n_tiles, G = valid < 256 ? valid : 256;
    const int maxt = (valid + G - 1) / G;
    stride = 2 + 2 * (maxt + 1);
    std::vector<int> h((size_t)G * stride, -1);
    const int q8 = G >> 3, r8 = G & 7;
    for (int blk = 0; blk < G; ++blk) {
      const int xcd = blk & 7;
      const int slot = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blk >> 3);
      int n = 0;
      for (int t = slot; t < valid; t += G, ++n) { h[(size_t)blk * stride + 2 + 2 * n] = t / n_tiles; h[(size_t)blk * stride + 3 + 2 * n] = t % n_tiles; }
      h[(size_t)blk * stride] = n;
      h[(size_t)blk * stride + 1] = 0;
    }
    if (table) CK(hipFree(table));
    CK(hipMalloc(&table, h.size() * 4));
    CK(hipMemcpy(table, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    grid = G;
  }
  void launch(const bf16_t* X, const bf16_t* W, float* Y, int K, int N, int store) {
    struct { const void* x; const void* w; void* y; const void* t; int k, n, stride, store; } args{X, W, Y, table, K, N, stride, store};
    size_t sz = sizeof(args);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    CK(hipModuleLaunchKernel(fn, grid, 1, 1, threads, 1, 1, 0, 0, nullptr, cfg));
  }
};

// 'stamps': in-kernel shader-clock split of the integrated kernels, per tile and wave: the K-loop, the whole epilogue and its OPEN (up
// to the point where bias, dln.vec and the rows' {mean, rstd} are in registers).  w8 rows: every epilogue class of the encoder layer
// with the constants fetched by the epilogue (pre 0) and staged in the slab under the K-loop (pre 1), bf16 and f16; NRES (in place,
// no fan-in) on the N = 768 shapes it runs at.  x16 rows: the compiler-scheduled kernel, bf16, as before.
template <typename TE, int EPI, bool PRE>
static void stamps_w8(const char* shape, const char* dt, const char* epi, dim3 g, const TE* X, const TE* W, const float* bias, TE* Y, int N, int K,
                      const int* mtot, int n_tiles, const DlnAux& ax, uint64_t* st) {
  CK(hipMemset(st, 0, 256 * 8 * 4 * 8));
  if (EPI == EPI_NRES) CK(hipMemset(Y, 0, (size_t)ax.part_stride * N * 2));   // (in place: Y is its own residual; part_stride = M here)
  hipLaunchKernelGGL((gemm_tn_w8_kernel<TE, TE, EPI, 0, PRE>), g, dim3(512), 0, 0, X, W, bias, EPI == EPI_NRES ? (const TE*)Y : (const TE*)nullptr, Y, N, K, mtot, n_tiles, ax);
  CK(hipDeviceSynchronize());
  std::vector<uint64_t> h(256 * 8 * 4);
  CK(hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
  double sk = 0, se = 0, sn = 0, so = 0;
  for (size_t i = 0; i < h.size(); i += 4) { sk += h[i]; se += h[i + 1]; sn += h[i + 2]; so += h[i + 3]; }
  printf("stamps %-4s w8  %-4s %-9s pre %d: per tile and wave: K-loop %.0f cycles, epilogue %.0f cycles, of which open %.0f (shader clock), %.0f tiles x waves\n",
         shape, dt, epi, (int)PRE, sk / sn, se / sn, so / sn, sn);
}

template <typename TE>
static void stamps_dtype(const char* shape, const char* dt, dim3 g, const TE* X, const TE* W, const float* bias, TE* Y, int N, int K, const int* mtot,
                         int n_tiles, const DlnAux& ax, uint64_t* st) {
  stamps_w8<TE, EPI_BIAS, false>(shape, dt, "BIAS", g, X, W, bias, Y, N, K, mtot, n_tiles, ax, st);
  stamps_w8<TE, EPI_BIAS, true>(shape, dt, "BIAS", g, X, W, bias, Y, N, K, mtot, n_tiles, ax, st);
  stamps_w8<TE, EPI_NORM, false>(shape, dt, "NORM", g, X, W, bias, Y, N, K, mtot, n_tiles, ax, st);
  stamps_w8<TE, EPI_NORM, true>(shape, dt, "NORM", g, X, W, bias, Y, N, K, mtot, n_tiles, ax, st);
  stamps_w8<TE, EPI_NORM_GELU, false>(shape, dt, "NORM_GELU", g, X, W, bias, Y, N, K, mtot, n_tiles, ax, st);
  stamps_w8<TE, EPI_NORM_GELU, true>(shape, dt, "NORM_GELU", g, X, W, bias, Y, N, K, mtot, n_tiles, ax, st);
  if (N == 768) {
    stamps_w8<TE, EPI_NRES, false>(shape, dt, "NRES", g, X, W, bias, Y, N, K, mtot, n_tiles, ax, st);
    stamps_w8<TE, EPI_NRES, true>(shape, dt, "NRES", g, X, W, bias, Y, N, K, mtot, n_tiles, ax, st);
  }
}

static void stamps_rows(const char* shape, int N, int K, int M, const bf16_t* X, const bf16_t* W, const std::vector<bf16_t>& hx,
                        const std::vector<bf16_t>& hw, const float* bias, bf16_t* Y16, const int* mtot, const DlnAux& aux) {
  const int n_tiles = N / 256, tiles = (M / 256) * n_tiles;
  dim3 g(tiles < 256 ? tiles : 256);
  uint64_t* st; CK(hipMalloc(&st, 256 * 8 * 4 * 8));
  DlnAux ax = aux; ax.aux32 = reinterpret_cast<const float*>(st);
  std::vector<float2> hm(M, float2{0.01f, 1.0f});
  float2 *mr, *part; float* vec;
  CK(hipMalloc(&mr, (size_t)M * 8)); CK(hipMalloc(&vec, 3072 * 4)); CK(hipMalloc(&part, (size_t)M * 8 * 12));
  CK(hipMemcpy(mr, hm.data(), (size_t)M * 8, hipMemcpyHostToDevice));
  std::vector<float> hv(3072, 1.0f); CK(hipMemcpy(vec, hv.data(), 3072 * 4, hipMemcpyHostToDevice));
  ax.vec = vec; ax.mr = mr; ax.part = part; ax.part_stride = M;
  stamps_dtype<bf16_t>(shape, "bf16", g, X, W, bias, Y16, N, K, mtot, n_tiles, ax, st);
  {                                                      // the same values as f16 operands
    static f16_t *Xh = nullptr, *Wh = nullptr;
    if (!Xh) {
      std::vector<f16_t> t(hx.size());
      for (size_t i = 0; i < hx.size(); ++i) t[i] = (f16_t)(float)hx[i];
      CK(hipMalloc(&Xh, t.size() * 2)); CK(hipMemcpy(Xh, t.data(), t.size() * 2, hipMemcpyHostToDevice));
      t.resize(hw.size());
      for (size_t i = 0; i < hw.size(); ++i) t[i] = (f16_t)(float)hw[i];
      CK(hipMalloc(&Wh, t.size() * 2)); CK(hipMemcpy(Wh, t.data(), t.size() * 2, hipMemcpyHostToDevice));
    }
    stamps_dtype<f16_t>(shape, "f16", g, Xh, Wh, bias, reinterpret_cast<f16_t*>(Y16), N, K, mtot, n_tiles, ax, st);
  }
  for (int e = 0; e < 3; ++e) {
    CK(hipMemset(st, 0, 256 * 8 * 3 * 8));
    if (e == 0) hipLaunchKernelGGL((gemm_tn_x16_kernel<bf16_t, bf16_t, EPI_BIAS, 0, false>), g, dim3(512), 0, 0, X, W, bias, (const bf16_t*)nullptr, Y16, N, K, mtot, n_tiles, ax);
    else if (e == 1) hipLaunchKernelGGL((gemm_tn_x16_kernel<bf16_t, bf16_t, EPI_NORM, 0, false>), g, dim3(512), 0, 0, X, W, bias, (const bf16_t*)nullptr, Y16, N, K, mtot, n_tiles, ax);
    else hipLaunchKernelGGL((gemm_tn_x16_kernel<bf16_t, bf16_t, EPI_NORM_GELU, 0, false>), g, dim3(512), 0, 0, X, W, bias, (const bf16_t*)nullptr, Y16, N, K, mtot, n_tiles, ax);
    CK(hipDeviceSynchronize());
    std::vector<uint64_t> h(256 * 8 * 3);
    CK(hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
    double sk = 0, se = 0, sn = 0;
    for (size_t i = 0; i < h.size(); i += 3) { sk += h[i]; se += h[i + 1]; sn += h[i + 2]; }
    printf("stamps %-4s x16 bf16 %-9s      : per tile and wave: K-loop %.0f cycles, epilogue %.0f cycles (shader clock), %.0f tiles x waves\n", shape,
           e == 0 ? "BIAS" : e == 1 ? "NORM" : "NORM_GELU", sk / sn, se / sn, sn);
  }
  CK(hipFree(st)); CK(hipFree(mr)); CK(hipFree(vec)); CK(hipFree(part));
}

int main(int argc, char** argv) {
  const int M = argc > 1 ? atoi(argv[1]) : 65536;
  const bool check = argc > 2 && !strcmp(argv[2], "check");
  const char* only = argc > 3 ? argv[3] : "";             // "prod" | "asm" | "v0" | "v1": one arm only (counter passes); "all": hipcc arms too
  const bool hipcc_vars = !strcmp(only, "all") || !strcmp(only, "v0") || !strcmp(only, "v1");
  struct Shape { const char* name; int N, K; };
  const Shape shapes[] = {{"qkv", 2304, 768}, {"out", 768, 768}, {"ffn1", 3072, 768}, {"ffn2", 768, 3072}};
  std::mt19937 rng(1);
  std::normal_distribution<float> nd(0.f, 1.f);
  const size_t xe = (size_t)M * 3072, we = (size_t)3072 * 3072;
  std::vector<bf16_t> hx(xe), hw(we);
  for (auto& v : hx) v = (bf16_t)nd(rng);
  for (auto& v : hw) v = (bf16_t)(0.05f * nd(rng));
  bf16_t *X, *W; float* bias; float* Y; bf16_t* Y16; int* mtot;
  CK(hipMalloc(&X, xe * 2)); CK(hipMalloc(&W, we * 2)); CK(hipMalloc(&bias, 3072 * 4)); CK(hipMalloc(&mtot, 4));
  CK(hipMalloc(&Y, (size_t)M * 3072 * 4)); CK(hipMalloc(&Y16, (size_t)M * 3072 * 2));
  CK(hipMemcpy(X, hx.data(), xe * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(W, hw.data(), we * 2, hipMemcpyHostToDevice));
  CK(hipMemset(bias, 0, 3072 * 4));
  CK(hipMemcpy(mtot, &M, 4, hipMemcpyHostToDevice));
  AsmKernel ak, ak8;
  const char* co = getenv("GEMM4W_CO") ? getenv("GEMM4W_CO") : "tools/bin/gemm4w.co";
  const bool have_asm = ak.load(co, "gemm4w_asm", 256);
  const bool have_asm8 = ak8.load(getenv("GEMM8W_CO") ? getenv("GEMM8W_CO") : "tools/bin/gemm8w.co", "gemm8w_asm", 512);

  if (argc > 2 && !strcmp(argv[2], "debug") && have_asm) {   // register dump of the epilogue's address path (see the generator): first tile of every workgroup
    const Shape& s = shapes[0];
    AsmKernel& dk = (argc > 3 && !strcmp(argv[3], "asm8") && have_asm8) ? ak8 : ak;
    dk.plan(M, s.N / 256);
    CK(hipMemset(Y, 0, 256 * 512 * 64));
    dk.launch(X, W, Y, s.K, s.N, (int)(0x80000000u | (unsigned)M));
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> d(256 * 512 * 16);
    CK(hipMemcpy(d.data(), Y, d.size() * 4, hipMemcpyDeviceToHost));
    unsigned long long y = (unsigned long long)Y;
    printf("Y = 0x%llx  N = %d\n", y, s.N);
    for (int wg : {0, 1, 9, 143})
      for (int t : {0, 1, 63, 64, 128, 192, 255, 256, 320, 511}) {
        if (t >= dk.threads) continue;
        const uint32_t* r = &d[((size_t)wg * 512 + t) * 16];
        printf("wg %3d tid %3d: v176 %10u  s40:41 (Y + %lld)  N %u | at start: s26 %u s27 %u s28 %u v0 0x%x | at end: s26 %u s27 %u s28 %u mt %d\n", wg, t, r[0],
               (long long)(((unsigned long long)r[2] << 32 | r[1]) - y), r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], (int)r[11]);
      }
    return 0;
  }
  if (check) {
    int bad = 0;
    std::vector<int> vars;
    if (have_asm) vars.push_back(2);
    if (have_asm8) vars.push_back(3);
    if (hipcc_vars) { vars.push_back(0); vars.push_back(1); }
    for (const auto& s : shapes)
      for (int var : vars) {
        const int n_tiles = s.N / 256, tiles = (M / 256) * n_tiles;
        dim3 g(tiles < 256 ? tiles : 256), b(256);
        CK(hipMemset(Y, 0xff, (size_t)M * s.N * 4));
        if (var == 0) hipLaunchKernelGGL((lab4::gemm4w_kernel<bf16_t, 0, true>), g, b, 0, 0, X, W, Y, s.N, s.K, M, n_tiles);
        else if (var == 1) hipLaunchKernelGGL((lab4::gemm4w_kernel<bf16_t, 1, true>), g, b, 0, 0, X, W, Y, s.N, s.K, M, n_tiles);
        else if (var == 2) { ak.plan(M, n_tiles); ak.launch(X, W, Y, s.K, s.N, M); }     // store = rows of Y: the epilogue's address guard
        else { ak8.plan(M, n_tiles); ak8.launch(X, W, Y, s.K, s.N, M); }
        CK(hipDeviceSynchronize());
        std::vector<float> hy((size_t)M * s.N);
        CK(hipMemcpy(hy.data(), Y, hy.size() * 4, hipMemcpyDeviceToHost));
        double worst = 0.0; size_t nan = 0;
        std::mt19937 pick(7 + var);
        for (int q = 0; q < 20000; ++q) {
          // rows / columns drawn over the whole problem (every wave, fragment and tile position gets hit), plus the four corners
          const int m = q < 4 ? (q & 1 ? M - 1 : 0) : (int)(pick() % (unsigned)M), n = q < 4 ? (q & 2 ? s.N - 1 : 0) : (int)(pick() % (unsigned)s.N);
          double ref = 0.0;
          for (int k = 0; k < s.K; ++k) ref += (double)(float)hx[(size_t)m * s.K + k] * (double)(float)hw[(size_t)n * s.K + k];
          const float got = hy[(size_t)m * s.N + n];
          if (got != got) ++nan;
          const double err = fabs((double)got - ref) / (1.0 + fabs(ref));
          if (err > worst) worst = err;
        }
        size_t unwritten = 0;
        for (size_t i = 0; i < hy.size(); i += 97) { uint32_t u; memcpy(&u, &hy[i], 4); if (u == 0xffffffffu) ++unwritten; }
        const bool ok = worst < 2e-3 && !nan && !unwritten;
        printf("check %-4s %s: worst rel err %.3e over 20000 sampled outputs, NaN %zu, unwritten (sampled) %zu  %s\n", s.name,
               var == 2 ? "asm 4-wave" : var == 3 ? "asm 8-wave" : var == 0 ? "hipcc VAR 0" : "hipcc VAR 1", worst, nan, unwritten, ok ? "ok" : "WRONG");
        if (!ok) bad = 1;
      }
    return bad;
  }

  printf("M = %d, bf16, N(0,1) activations, main loops only (no epilogue); production = gemm_tn_x16_kernel<ABL=1> (8 waves, 128x64 wave tiles)\n", M);
  auto want = [&](const char* arm) { return !*only || !strcmp(only, "all") || !strcmp(only, arm); };
  const int iters = getenv("LAB_ITERS") ? atoi(getenv("LAB_ITERS")) : 20, reps = getenv("LAB_REPS") ? atoi(getenv("LAB_REPS")) : 3;
  for (int rep = 0; rep < reps; ++rep)                        // alternate the arms: same box, same minute
    for (const auto& s : shapes) {
      const int n_tiles = s.N / 256, tiles = (M / 256) * n_tiles;
      const double fl = 2.0 * M * s.N * s.K;
      dim3 g(tiles < 256 ? tiles : 256);
      DlnAux aux{};
      aux.panel_mode = 1; aux.x_rows = M;
      double tp = 0, ta = 0, ta8 = 0, t0 = 0, t1 = 0;
      if (want("prod"))
        tp = time_us([&] { hipLaunchKernelGGL((gemm_tn_x16_kernel<bf16_t, bf16_t, EPI_BIAS, 1>), g, dim3(512), 0, 0, X, W, bias, (const bf16_t*)nullptr, Y16, s.N, s.K, mtot, n_tiles, aux); }, iters);
      if (have_asm && want("asm")) {
        ak.plan(M, n_tiles);
        ta = time_us([&] { ak.launch(X, W, Y, s.K, s.N, 0); }, iters);
      }
      if (have_asm8 && want("asm8")) {
        ak8.plan(M, n_tiles);
        ta8 = time_us([&] { ak8.launch(X, W, Y, s.K, s.N, 0); }, iters);
      }
      double tw8 = 0, tw8f = 0, tpf = 0;
      if (want("w8abl"))
        tw8 = time_us([&] { hipLaunchKernelGGL((gemm_tn_w8_kernel<bf16_t, bf16_t, EPI_BIAS, 1>), g, dim3(512), 0, 0, X, W, bias, (const bf16_t*)nullptr, Y16, s.N, s.K, mtot, n_tiles, aux); }, iters);
      if (want("w8full"))
        tw8f = time_us([&] { hipLaunchKernelGGL((gemm_tn_w8_kernel<bf16_t, bf16_t, EPI_BIAS, 0>), g, dim3(512), 0, 0, X, W, bias, (const bf16_t*)nullptr, Y16, s.N, s.K, mtot, n_tiles, aux); }, iters);
      if (want("prodfull"))
        tpf = time_us([&] { hipLaunchKernelGGL((gemm_tn_x16_kernel<bf16_t, bf16_t, EPI_BIAS, 0, false>), g, dim3(512), 0, 0, X, W, bias, (const bf16_t*)nullptr, Y16, s.N, s.K, mtot, n_tiles, aux); }, iters);
      if (want("stamps")) stamps_rows(s.name, s.N, s.K, M, X, W, hx, hw, bias, Y16, mtot, aux);
      if (hipcc_vars && want("v0"))
        t0 = time_us([&] { hipLaunchKernelGGL((lab4::gemm4w_kernel<bf16_t, 0, false>), g, dim3(256), 0, 0, X, W, Y, s.N, s.K, M, n_tiles); }, 20);
      if (hipcc_vars && want("v1"))
        t1 = time_us([&] { hipLaunchKernelGGL((lab4::gemm4w_kernel<bf16_t, 1, false>), g, dim3(256), 0, 0, X, W, Y, s.N, s.K, M, n_tiles); }, 20);
      printf("rep %d %-4s N=%4d K=%4d  production %7.1f us %6.0f TF | 4-wave asm %7.1f us %6.0f TF (%+5.1f %%)", rep, s.name, s.N, s.K, tp,
             tp ? fl / tp / 1e6 : 0, ta, ta ? fl / ta / 1e6 : 0, tp && ta ? 100 * (ta / tp - 1) : 0);
      printf(" | 8-wave asm %7.1f us %6.0f TF (%+5.1f %%)", ta8, ta8 ? fl / ta8 / 1e6 : 0, tp && ta8 ? 100 * (ta8 / tp - 1) : 0);
      printf(" | integrated W8: K-loops only %7.1f us, with the bias epilogue %7.1f us; production with the bias epilogue %7.1f us", tw8, tw8f, tpf);
      if (hipcc_vars) printf(" | hipcc VAR 0 %7.1f us (%+5.1f %%) | hipcc VAR 1 %7.1f us (%+5.1f %%)", t0, tp && t0 ? 100 * (t0 / tp - 1) : 0, t1, tp && t1 ? 100 * (t1 / tp - 1) : 0);
      printf("\n");
    }
  return 0;
}
