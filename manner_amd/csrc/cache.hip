// Content-addressed news-embedding cache (round 4): SURVEY.md §8(d) "mode T" — each unique news encoded once — behind the UNCHANGED
// drop-in call pattern.  The reference encodes every history and candidate occurrence of every impression again
// (manner/models/cr_module.py:107,113 -> news_encoder.py:29-37); a MIND dev set lists its 65 k news 4.2 M times.  In eval() under
// no_grad the text encoder is a pure function of (weights, real tokens of the row), row by row, so `MannerTextEncoder.forward` may look
// a row up by its tokens and encode only the rows it has not seen under the current weights.  Opt-in (MANNER_EMBED_CACHE_ROWS /
// MannerTextEncoder.embedding_cache_rows); bench.py's headline (mode R) and its `B8_eval` drop-in figure never use it.
//
//   manner_hip_news_key128        128-bit key of every row's REAL tokens (mask == 1 positions, any padded width)
//   manner_hip_news_cache_lookup  open-addressing table in caller-owned device memory: row -> {table row, state}
//   manner_hip_prefix_resolve / _store / _gather   token-packed payload of the frozen-prefix cache (below)
//
// HBM-trivial integer work (a batch is a few thousand rows of <= 512 tokens): one wave per row for the keys — coalesced 8-byte loads,
// a position-keyed 64-bit mix per token, two independent sums reduced over the wave — and one thread per row for the table, in three
// launches so that nobody reads a slot another thread of the same call is still filling.
#include "common.h"

namespace manner {
namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {          // splitmix64 finaliser: a bijection with full avalanche
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// key = (sum_j f0(j, id_j), sum_j f1(j, id_j)) over the real positions j, + a term of the token count: a sum of per-position random
// functions is a universal hash of the sequence (two rows collide only if the 64-bit sums do), position-keyed so that order matters,
// padding-width independent because padded positions add nothing.
__global__ __launch_bounds__(256) void news_key_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ mask, int64_t n_news,
                                                       int64_t padded_len, uint64_t* __restrict__ keys) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + wave;
  if (n >= n_news) return;
  const int64_t* ir = ids + n * padded_len;
  const int64_t* mr = mask + n * padded_len;
  uint64_t a = 0, b = 0, cnt = 0;
  for (int64_t j = lane; j < padded_len; j += 64) {
    if (mr[j] != 0) {
      const uint64_t t = (uint64_t)ir[j];
      a += mix64(t * 0x9e3779b97f4a7c15ull + (uint64_t)(j + 1) * 0xd1b54a32d192ed03ull);
      b += mix64((t + 0x632be59bd9b4e019ull) * 0xe7037ed1a0b428dbull ^ (uint64_t)(j + 1) * 0x8ebc6af09c88c6e3ull);
      ++cnt;
    }
  }
  a = wave_sum_u64(a); b = wave_sum_u64(b); cnt = wave_sum_u64(cnt);
  if (lane == 0) {
    a = mix64(a + cnt * 0xa0761d6478bd642full);
    b = mix64(b ^ (cnt + 1) * 0xe7037ed1a0b428dbull);
    keys[2 * n] = a ? a : 1;                         // 0 marks an empty slot
    keys[2 * n + 1] = b;
  }
}

// pass 1: find the slot holding k0 or claim an empty one.  scratch[n] = slot (-1: table full), scratch[n_news + n] = 1 when this
// thread's compare-and-swap put the key there (exactly one thread per new key, however often the key occurs in the call).
__global__ __launch_bounds__(256) void cache_claim_kernel(const uint64_t* __restrict__ keys, int64_t n_news, unsigned long long* slot_k0,
                                                          int64_t n_slots, int32_t* __restrict__ scratch) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= n_news) return;
  const unsigned long long k0 = keys[2 * n];
  const uint64_t maskb = (uint64_t)n_slots - 1;
  uint64_t i = mix64(k0) & maskb;
  int32_t slot = -1, won = 0;
  // bounded probing: insertion and search give up at the same distance, so a key is either within it or not in the table; a table
  // that has seen far more distinct keys than it has slots degrades to "encode, do not store" instead of to a long walk
  const int64_t max_probe = n_slots < 1024 ? n_slots : 1024;
  for (int64_t probe = 0; probe < max_probe; ++probe, i = (i + 1) & maskb) {
    unsigned long long cur = __hip_atomic_load(&slot_k0[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) {
      cur = atomicCAS(&slot_k0[i], 0ull, k0);
      if (cur == 0) { slot = (int32_t)i; won = 1; break; }
    }
    if (cur == k0) { slot = (int32_t)i; break; }
  }
  scratch[n] = slot;
  scratch[n_news + n] = won;
}

// pass 2: the claimants complete their slots: second key word and a table row (-1 when the table is full: the key stays known and
// its rows are encoded on every call, never stored)
__global__ __launch_bounds__(256) void cache_fill_kernel(const uint64_t* __restrict__ keys, int64_t n_news, uint64_t* __restrict__ slot_k1,
                                                         int32_t* __restrict__ slot_row, int32_t* row_count, int32_t capacity_rows,
                                                         const int32_t* __restrict__ scratch) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= n_news || !scratch[n_news + n]) return;
  const int32_t slot = scratch[n];
  slot_k1[slot] = keys[2 * n + 1];
  const int32_t r = atomicAdd(row_count, 1);
  slot_row[slot] = r < capacity_rows ? r : -1;
}

// pass 3: state 0 = the row's embedding is (or, for a duplicate of a key new in this call, will be) in the table; 1 = new: encode and
// store at rows_out; 2 = encode, do not store (table or slots full, or — 2^-64 — another key with the same first word owns the slot)
__global__ __launch_bounds__(256) void cache_resolve_kernel(const uint64_t* __restrict__ keys, int64_t n_news, const uint64_t* __restrict__ slot_k1,
                                                            const int32_t* __restrict__ slot_row, const int32_t* __restrict__ scratch,
                                                            int32_t* __restrict__ rows_out, int32_t* __restrict__ state_out) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= n_news) return;
  const int32_t slot = scratch[n];
  int32_t row = -1, state = 2;
  if (slot >= 0 && slot_k1[slot] == keys[2 * n + 1]) {
    row = slot_row[slot];
    state = row < 0 ? 2 : (scratch[n_news + n] ? 1 : 0);
    if (row < 0) row = -1;
  }
  rows_out[n] = row;
  state_out[n] = state;
}

// ---- token-packed payload of the frozen-prefix cache ---------------------------------------------------------------------------
// A table row (the index the lookup hands out) owns `row_len` tokens of a pool f32 [pool_tokens, H] at token `row_off`: a news costs
// its REAL tokens x H x 4 bytes whatever the padded width of the call that stored it.  row_len: -1 = nothing attempted yet (the state
// every row starts in, so a state-0 occurrence that meets it is a repeat of a key new in THIS call), -2 = the pool had no room (key
// known, no payload: encoded at every later call, never read), >= 1 = payload.  tok_count = tokens handed out; an add that would pass
// pool_tokens marks its row -2 and the counter may stay past the pool — no reader trusts it, every reader checks off + len itself.
// A row's tokens are contiguous in the padded source, the pool and the padded output, so store and gather are flat 16-byte copies,
// 32 KB per workgroup (8 loads in flight per lane, then 8 stores), indexed in 64 bits.
constexpr int PFX_CHUNK = 256 * 8;          // float4 per workgroup

__global__ __launch_bounds__(256) void prefix_resolve_kernel(int64_t n_news, const int32_t* __restrict__ row_len, int32_t capacity_rows,
                                                             int32_t* __restrict__ rows, int32_t* __restrict__ state) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= n_news || state[n] != 0) return;
  const int32_t r = rows[n];
  if (r < 0 || r >= capacity_rows || row_len[r] == -2) { rows[n] = -1; state[n] = 2; }
}

// one thread per freshly encoded row: where it sits in `fresh` (for the gather of this call) and, for state 1, its reservation
__global__ __launch_bounds__(256) void prefix_reserve_kernel(int64_t n_new, const int64_t* __restrict__ index, int64_t n_news,
                                                             const int32_t* __restrict__ rows, const int32_t* __restrict__ state,
                                                             const int32_t* __restrict__ lens, int32_t padded_len, int32_t capacity_rows,
                                                             unsigned long long pool_tokens, unsigned long long* tok_count,
                                                             int64_t* __restrict__ row_off, int32_t* __restrict__ row_len,
                                                             int32_t* __restrict__ row_src, int32_t* __restrict__ src_of) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_new) return;
  const int64_t n = index ? index[j] : j;
  if (n < 0 || n >= n_news) return;
  src_of[n] = (int32_t)j;
  if (state[n] != 1) return;
  const int32_t r = rows[n];
  if (r < 0 || r >= capacity_rows) return;
  row_src[r] = (int32_t)j;
  const int32_t len = lens[n];
  int64_t off = 0;
  int32_t got = -2;
  if (len >= 1 && len <= padded_len &&
      __hip_atomic_load(tok_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (unsigned long long)len <= pool_tokens) {
    const unsigned long long o = atomicAdd(tok_count, (unsigned long long)len);        // device scope: any interleaving of workgroups
    if (o + (unsigned long long)len <= pool_tokens) { off = (int64_t)o; got = len; }
  }
  row_off[r] = off;
  row_len[r] = got;
}

__global__ __launch_bounds__(256) void prefix_store_kernel(const float4* __restrict__ fresh, const int64_t* __restrict__ index, int64_t n_news,
                                                           const int32_t* __restrict__ rows, const int32_t* __restrict__ state,
                                                           int64_t row_f4 /* padded_len * H / 4 */, int32_t h4, int32_t chunks,
                                                           int32_t capacity_rows, int64_t pool_tokens, const int64_t* __restrict__ row_off,
                                                           const int32_t* __restrict__ row_len, float4* __restrict__ pool) {
  const int64_t j = blockIdx.x / chunks;
  const int64_t base = (int64_t)(blockIdx.x % chunks) * PFX_CHUNK + threadIdx.x;
  const int64_t n = index ? index[j] : j;
  if (n < 0 || n >= n_news || state[n] != 1) return;
  const int32_t r = rows[n];
  if (r < 0 || r >= capacity_rows) return;
  const int64_t len = row_len[r], off = row_off[r];
  if (len < 1 || off < 0 || off + len > pool_tokens) return;
  const int64_t live = (len * h4 < row_f4 ? len * h4 : row_f4);
  const float4* src = fresh + j * row_f4;
  float4* dst = pool + off * h4;
  float4 v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t i = base + k * 256;
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < live) v[k] = src[i];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) { const int64_t i = base + k * 256; if (i < live) dst[i] = v[k]; }
}

// out[n] = the row's tokens from the pool + zeros, or (no payload, `fresh` given) its freshly encoded row; otherwise left alone
__global__ __launch_bounds__(256) void prefix_gather_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ state,
                                                            int64_t row_f4, int32_t padded_len, int32_t h4, int32_t chunks,
                                                            int32_t capacity_rows, int64_t pool_tokens, const int64_t* __restrict__ row_off,
                                                            const int32_t* __restrict__ row_len, const int32_t* __restrict__ row_src,
                                                            const float4* __restrict__ pool, const float4* __restrict__ fresh,
                                                            int64_t n_fresh, const int32_t* __restrict__ src_of, float4* __restrict__ out) {
  const int64_t n = blockIdx.x / chunks;
  const int64_t base = (int64_t)(blockIdx.x % chunks) * PFX_CHUNK + threadIdx.x;
  const int32_t r = rows[n];
  const bool row_ok = r >= 0 && r < capacity_rows;
  const float4* src = nullptr;
  int64_t live = 0;
  if (row_ok) {
    const int64_t len = row_len[r], off = row_off[r];
    if (len >= 1 && off >= 0 && off + len <= pool_tokens) {
      src = pool + off * h4;
      live = (len < padded_len ? len : padded_len) * h4;
    }
  }
  if (!src && fresh) {
    const int64_t j = state[n] != 0 ? src_of[n] : (row_ok ? row_src[r] : -1);
    if (j >= 0 && j < n_fresh) { src = fresh + j * row_f4; live = row_f4; }
  }
  if (!src) return;
  float4* dst = out + n * row_f4;
  float4 v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t i = base + k * 256;
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < live) v[k] = src[i];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) { const int64_t i = base + k * 256; if (i < row_f4) dst[i] = v[k]; }
}

// shared argument checks of store and gather; *chunks = workgroups per row
int prefix_shape(const char* who, int64_t n, int64_t padded_len, int32_t hidden, int32_t capacity_rows, int64_t pool_tokens, int64_t* chunks) {
  if (n < 0 || padded_len < 1 || padded_len > MANNER_HIP_MAX_LEN_INFER || hidden < 4 || (hidden & 3) || capacity_rows < 0 || pool_tokens < 0)
    return fail(MANNER_HIP_E_INVALID, "%s: rows=%lld padded_len=%lld (1..%d) hidden=%d (a multiple of 4) capacity=%d pool_tokens=%lld", who,
                (long long)n, (long long)padded_len, MANNER_HIP_MAX_LEN_INFER, hidden, capacity_rows, (long long)pool_tokens);
  *chunks = (padded_len * (hidden / 4) + PFX_CHUNK - 1) / PFX_CHUNK;
  if (n * *chunks > 0x7fffffffll) return fail(MANNER_HIP_E_INVALID, "%s: %lld rows of %lld workgroups exceed one grid", who, (long long)n, (long long)*chunks);
  return MANNER_HIP_OK;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" int manner_hip_news_key128(const int64_t* ids, const int64_t* mask, int64_t n_news, int64_t padded_len, uint64_t* keys,
                                      manner_hip_stream_t stream) {
  if (n_news < 0 || padded_len < 0) return fail(MANNER_HIP_E_INVALID, "news_key128: n_news=%lld padded_len=%lld", (long long)n_news, (long long)padded_len);
  if (n_news == 0) return MANNER_HIP_OK;
  if (!ids || !mask || !keys) return fail(MANNER_HIP_E_INVALID, "news_key128: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(news_key_kernel, dim3((unsigned)((n_news + 3) / 4)), dim3(256), 0, s, ids, mask, n_news, padded_len, keys);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

extern "C" int manner_hip_news_cache_lookup(const uint64_t* keys, int64_t n_news, uint64_t* slot_keys, int32_t* slot_rows, int64_t n_slots,
                                            int32_t* row_count, int32_t capacity_rows, int32_t* rows_out, int32_t* state_out,
                                            int32_t* scratch, manner_hip_stream_t stream) {
  if (n_news < 0 || n_slots < 2 || (n_slots & (n_slots - 1)) || n_slots > 0x40000000 || capacity_rows < 0)
    return fail(MANNER_HIP_E_INVALID, "news_cache_lookup: n_news=%lld n_slots=%lld (a power of two <= 2^30) capacity=%d", (long long)n_news,
                (long long)n_slots, capacity_rows);
  if (n_news == 0) return MANNER_HIP_OK;
  if (!keys || !slot_keys || !slot_rows || !row_count || !rows_out || !state_out || !scratch)
    return fail(MANNER_HIP_E_INVALID, "news_cache_lookup: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 g((unsigned)((n_news + 255) / 256)), b(256);
  unsigned long long* k0 = reinterpret_cast<unsigned long long*>(slot_keys);
  uint64_t* k1 = slot_keys + n_slots;
  hipLaunchKernelGGL(cache_claim_kernel, g, b, 0, s, keys, n_news, k0, n_slots, scratch);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(cache_fill_kernel, g, b, 0, s, keys, n_news, k1, slot_rows, row_count, capacity_rows, scratch);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(cache_resolve_kernel, g, b, 0, s, keys, n_news, k1, slot_rows, scratch, rows_out, state_out);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

extern "C" int manner_hip_prefix_resolve(int32_t* rows, int32_t* state, int64_t n_news, const int32_t* row_len, int32_t capacity_rows,
                                         manner_hip_stream_t stream) {
  if (n_news < 0 || capacity_rows < 0) return fail(MANNER_HIP_E_INVALID, "prefix_resolve: n_news=%lld capacity=%d", (long long)n_news, capacity_rows);
  if (n_news == 0) return MANNER_HIP_OK;
  if (!rows || !state || !row_len) return fail(MANNER_HIP_E_INVALID, "prefix_resolve: null pointer");
  hipLaunchKernelGGL(prefix_resolve_kernel, dim3((unsigned)((n_news + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), n_news,
                     row_len, capacity_rows, rows, state);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

extern "C" int manner_hip_prefix_store(const float* fresh, int64_t n_new, const int64_t* index, int64_t n_news, const int32_t* rows,
                                       const int32_t* state, const int32_t* lens, int64_t padded_len, int32_t hidden, float* pool,
                                       int64_t pool_tokens, int32_t capacity_rows, int64_t* row_off, int32_t* row_len, int32_t* row_src,
                                       uint64_t* tok_count, int32_t* src_of, manner_hip_stream_t stream) {
  int64_t chunks = 0;
  if (int rc = prefix_shape("prefix_store", n_new, padded_len, hidden, capacity_rows, pool_tokens, &chunks)) return rc;
  if (n_news < n_new) return fail(MANNER_HIP_E_INVALID, "prefix_store: %lld fresh rows of a call of %lld", (long long)n_new, (long long)n_news);
  if (n_new == 0) return MANNER_HIP_OK;
  if (!fresh || !rows || !state || !lens || !pool || !row_off || !row_len || !row_src || !tok_count || !src_of)
    return fail(MANNER_HIP_E_INVALID, "prefix_store: null pointer");
  if (!aligned16(fresh) || !aligned16(pool)) return fail(MANNER_HIP_E_INVALID, "prefix_store: fresh and pool must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(prefix_reserve_kernel, dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, s, n_new, index, n_news, rows, state, lens,
                     (int32_t)padded_len, capacity_rows, (unsigned long long)pool_tokens, reinterpret_cast<unsigned long long*>(tok_count),
                     row_off, row_len, row_src, src_of);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(prefix_store_kernel, dim3((unsigned)(n_new * chunks)), dim3(256), 0, s, reinterpret_cast<const float4*>(fresh), index,
                     n_news, rows, state, padded_len * (hidden / 4), hidden / 4, (int32_t)chunks, capacity_rows, pool_tokens, row_off, row_len,
                     reinterpret_cast<float4*>(pool));
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

extern "C" int manner_hip_prefix_gather(const int32_t* rows, const int32_t* state, int64_t n_news, int64_t padded_len, int32_t hidden,
                                        const float* pool, int64_t pool_tokens, int32_t capacity_rows, const int64_t* row_off,
                                        const int32_t* row_len, const int32_t* row_src, const float* fresh, int64_t n_fresh,
                                        const int32_t* src_of, float* out, manner_hip_stream_t stream) {
  int64_t chunks = 0;
  if (int rc = prefix_shape("prefix_gather", n_news, padded_len, hidden, capacity_rows, pool_tokens, &chunks)) return rc;
  if (n_fresh < 0) return fail(MANNER_HIP_E_INVALID, "prefix_gather: n_fresh=%lld", (long long)n_fresh);
  if (n_news == 0) return MANNER_HIP_OK;
  if (!rows || !state || !pool || !row_off || !row_len || !row_src || !out || (fresh && !src_of))
    return fail(MANNER_HIP_E_INVALID, "prefix_gather: null pointer");
  if (!aligned16(pool) || !aligned16(out) || !aligned16(fresh)) return fail(MANNER_HIP_E_INVALID, "prefix_gather: pool, fresh and out must be 16-byte aligned");
  hipLaunchKernelGGL(prefix_gather_kernel, dim3((unsigned)(n_news * chunks)), dim3(256), 0, static_cast<hipStream_t>(stream), rows, state,
                     padded_len * (hidden / 4), (int32_t)padded_len, hidden / 4, (int32_t)chunks, capacity_rows, pool_tokens, row_off, row_len,
                     row_src, reinterpret_cast<const float4*>(pool), reinterpret_cast<const float4*>(fresh), n_fresh, src_of,
                     reinterpret_cast<float4*>(out));
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}
