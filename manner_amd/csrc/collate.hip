// Device-side collate: builds the tensors of a MINDRecBatch from a device-resident,
// pre-tokenised news store and the row indices of the batch's history / candidate news — what
// MINDCollate.__call__ (manner/data/components/mind_rec_dataset.py:114-137) assembles on the host with
// pd.concat + the tokenizer on every step.  Pure byte/index movement, HBM-bound: coalesced 16-byte stores of
// the int64 outputs, one wave per output row.
#include "common.h"

namespace manner {
namespace {

// _make_batch_assignees (mind_rec_dataset.py:171-174): seg[j] = i for off[i] <= j < off[i+1]
__global__ __launch_bounds__(256) void segments_kernel(const int64_t* __restrict__ off, int64_t B, int64_t total,
                                                      int64_t* __restrict__ seg) {
  for (int64_t j = blockIdx.x * 256ll + threadIdx.x; j < total; j += 256ll * gridDim.x) {
    int64_t lo = 0, hi = B;                       // largest i with off[i] <= j (empty segments are skipped)
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (off[mid] <= j) lo = mid; else hi = mid;
    }
    seg[j] = lo;
  }
}

typedef long long i64x2 __attribute__((ext_vector_type(2)));

// tokenizer(..., padding=True) restated on stored token rows (mind_rec_dataset.py:134-137): row r of the
// batch = the first min(len, Lp) stored ids of news rows[r], then pad_id; mask 1 / 0.
__global__ __launch_bounds__(256) void text_kernel(const int32_t* __restrict__ store_ids, const int32_t* __restrict__ store_len,
                                                  int64_t n_news, int Ls, const int32_t* __restrict__ rows, int64_t M,
                                                  int Lp, int pad_id, int64_t* __restrict__ ids, int64_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const int64_t r = blockIdx.x * 4ll + (threadIdx.x >> 6);
  if (r >= M) return;
  int64_t src = rows[r];
  src = src < 0 ? 0 : (src >= n_news ? n_news - 1 : src);
  int len = store_len[src];
  len = len < 0 ? 0 : (len > Ls ? Ls : len);
  const int32_t* in = store_ids + src * Ls;
  int64_t* oi = ids + r * Lp;
  int64_t* om = mask + r * Lp;
  if ((Lp & 1) == 0) {                            // rows are 16-byte aligned: two int64 per lane per store
    for (int c = 2 * lane; c < Lp; c += 128) {
      i64x2 v, m;
      v[0] = c < len ? in[c] : pad_id;         m[0] = c < len;
      v[1] = c + 1 < len ? in[c + 1] : pad_id; m[1] = c + 1 < len;
      *reinterpret_cast<i64x2*>(oi + c) = v;
      *reinterpret_cast<i64x2*>(om + c) = m;
    }
  } else {
    for (int c = lane; c < Lp; c += 64) {
      oi[c] = c < len ? in[c] : pad_id;
      om[c] = c < len;
    }
  }
}

// _tokenize_entities (mind_rec_dataset.py:139-144): entity index lists right-padded with 0 to the batch max
__global__ __launch_bounds__(256) void entities_kernel(const int32_t* __restrict__ store_ent, const int32_t* __restrict__ store_cnt,
                                                      int64_t n_news, int Es, const int32_t* __restrict__ rows, int64_t M, int E,
                                                      int64_t* __restrict__ out) {
  const int64_t total = M * (int64_t)E;
  for (int64_t j = blockIdx.x * 256ll + threadIdx.x; j < total; j += 256ll * gridDim.x) {
    const int64_t r = j / E;
    const int c = (int)(j - r * E);
    int64_t src = rows[r];
    src = src < 0 ? 0 : (src >= n_news ? n_news - 1 : src);
    int cnt = store_cnt[src];
    cnt = cnt > Es ? Es : cnt;
    out[j] = c < cnt ? store_ent[src * Es + c] : 0;
  }
}

// category / sentiment labels and the sentiment score of every batch row (mind_rec_dataset.py:164-168)
__global__ __launch_bounds__(256) void aspects_kernel(const int32_t* __restrict__ cat, const int32_t* __restrict__ sent,
                                                     const float* __restrict__ score, int64_t n_news,
                                                     const int32_t* __restrict__ rows, int64_t M, int64_t* __restrict__ ocat,
                                                     int64_t* __restrict__ osent, float* __restrict__ oscore) {
  for (int64_t r = blockIdx.x * 256ll + threadIdx.x; r < M; r += 256ll * gridDim.x) {
    int64_t src = rows[r];
    src = src < 0 ? 0 : (src >= n_news ? n_news - 1 : src);
    if (ocat) ocat[r] = cat[src];
    if (osent) osent[r] = sent[src];
    if (oscore) oscore[r] = score[src];
  }
}

// ------------------------------------------------------------------------------------------ training batches
// MINDRecDatasetTrain._sample_candidates (manner/data/components/mind_rec_dataset.py:13-77) as a counter-based rule (stated in
// include/manner_hip.h): every key is a pure function of (seed, epoch, impression, stream, slot) and every rank a count, so
// the result depends on nothing but the impression — no atomics, no execution order, no stored keys (LDS holds one tile of
// 256 recomputed keys at a time, whatever the impression's length).
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t slot_key(uint64_t base, uint32_t stream, int slot) {
  return mix64(base ^ ((uint64_t)stream << 32 | (uint32_t)slot));
}
__device__ __forceinline__ int select_bit(unsigned long long m, int k) {   // index of the k-th (0-based) set bit
  for (int i = 0; i < k; ++i) m &= m - 1;
  return __builtin_ctzll(m);
}

// Place of element s of the list [P, S] (T elements) in the output: the number of elements with a smaller (key(2, .), .).
// Called by the whole workgroup (barriers inside); `has` = this thread holds an element.
__device__ __forceinline__ int final_rank(uint64_t base, int T, int s, bool has, uint64_t* s_key) {
  const int tid = threadIdx.x;
  const uint64_t ks = slot_key(base, 2, s);
  int r = 0;
  for (int t0 = 0; t0 < T; t0 += 256) {
    s_key[tid] = slot_key(base, 2, t0 + tid);
    __syncthreads();
    if (has) {
      const int lim = T - t0 < 256 ? T - t0 : 256;
      for (int i = 0; i < lim; ++i) {
        const uint64_t k = s_key[i];
        r += (k < ks) || (k == ks && t0 + i < s);
      }
    }
    __syncthreads();
  }
  return r;
}

__global__ __launch_bounds__(256) void sample_kernel(const int32_t* __restrict__ cand_rows, const float* __restrict__ labels,
                                                    const int64_t* __restrict__ cand_off, int64_t n_imp, int64_t total,
                                                    const int64_t* __restrict__ users, const int64_t* __restrict__ imp_idx,
                                                    const int64_t* __restrict__ out_off, int64_t out_total, int ratio,
                                                    uint64_t seed_epoch, int32_t* __restrict__ out_rows, float* __restrict__ out_labels,
                                                    int32_t* __restrict__ out_pos, int64_t* __restrict__ out_users,
                                                    int32_t* __restrict__ status) {
  __shared__ uint64_t s_key[256];
  __shared__ unsigned long long s_mask[4];
  __shared__ int s_cnt[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  // every early return below depends on values the whole workgroup shares
  const int64_t imp = imp_idx[b];
  if (imp < 0 || imp >= n_imp) {
    if (tid == 0) { if (status) atomicOr(status, MANNER_HIP_STATUS_INDEX); if (out_users) out_users[b] = 0; }
    return;
  }
  if (out_users && tid == 0) out_users[b] = users[imp];
  const int64_t beg = cand_off[imp], end = cand_off[imp + 1];
  if (beg < 0 || end < beg || end > total || end - beg > 0x7fffffff) {
    if (tid == 0 && status) atomicOr(status, MANNER_HIP_STATUS_INDEX);
    return;
  }
  const int n = (int)(end - beg);
  const float* lab = labels + beg;
  const int32_t* rows = cand_rows + beg;

  int p = 0, q = 0;
  for (int j = tid; j < n; j += 256) {
    const float l = lab[j];
    p += l == 1.f;
    q += l == 0.f;
  }
  for (int o = 32; o > 0; o >>= 1) { p += __shfl_xor(p, o, 64); q += __shfl_xor(q, o, 64); }
  if (lane == 0) { s_cnt[wave] = p; s_cnt[4 + wave] = q; }
  __syncthreads();
  p = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  q = s_cnt[4] + s_cnt[5] + s_cnt[6] + s_cnt[7];
  __syncthreads();

  const int64_t T64 = (int64_t)p * (1 + (int64_t)ratio), m64 = (int64_t)p * ratio;
  const int64_t o0 = out_off[b], o1 = out_off[b + 1];
  if (o0 < 0 || o1 > out_total || o1 - o0 != T64 || T64 > 0x7fffffff || (m64 > 0 && q == 0)) {
    if (tid == 0 && status) atomicOr(status, MANNER_HIP_STATUS_LENGTHS);
    return;
  }
  if (p == 0) return;
  const int T = (int)T64, m = (int)m64;
  const bool replace = m > q;
  const uint64_t base = mix64(seed_epoch ^ (uint64_t)imp);

  // positives (element s = ordinal among the positives) and, without replacement, the m negatives of smallest (key(0, j), j)
  // (element p + rank), one chunk of 256 positions at a time
  int p_before = 0;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int j = c0 + tid;
    const float l = j < n ? lab[j] : -1.f;
    const bool is_pos = l == 1.f, is_neg = l == 0.f;
    const unsigned long long mp = __ballot(is_pos);
    if (lane == 0) s_cnt[wave] = __popcll(mp);
    __syncthreads();
    int before = p_before, all = 0;
    for (int w = 0; w < 4; ++w) { const int c = s_cnt[w]; before += w < wave ? c : 0; all += c; }
    int s = is_pos ? before + __popcll(mp & ((1ull << lane) - 1)) : -1;
    p_before += all;
    __syncthreads();
    if (!replace && m > 0) {
      const uint64_t kj = slot_key(base, 0, j);
      int r = 0;
      for (int t0 = 0; t0 < n; t0 += 256) {
        const int jp = t0 + tid;
        s_key[tid] = slot_key(base, 0, jp);
        const unsigned long long mk = __ballot(jp < n && lab[jp] == 0.f);
        if (lane == 0) s_mask[wave] = mk;
        __syncthreads();
        if (is_neg) {
          for (int w = 0; w < 4; ++w) {
            unsigned long long mm = s_mask[w];
            while (mm) {
              const int i = w * 64 + __builtin_ctzll(mm);
              mm &= mm - 1;
              const uint64_t k = s_key[i];
              r += (k < kj) || (k == kj && t0 + i < j);
            }
          }
        }
        __syncthreads();
      }
      if (is_neg && r < m) s = p + r;
    }
    const int d = final_rank(base, T, s, s >= 0, s_key);
    if (s >= 0) {
      out_rows[o0 + d] = rows[j];
      out_labels[o0 + d] = l;
      if (out_pos) out_pos[o0 + d] = j;
    }
  }
  if (!replace) return;

  // with replacement: draw t is the r-th negative in position order, found by a prefix count over chunks of the impression
  for (int c0 = 0; c0 < m; c0 += 256) {
    const int t = c0 + tid;
    const bool has = t < m;
    const int r = has ? (int)(((slot_key(base, 1, t) >> 32) * (uint64_t)q) >> 32) : -1;
    int pos = -1, seen = 0;
    for (int t0 = 0; t0 < n; t0 += 256) {
      const int jp = t0 + tid;
      const unsigned long long mk = __ballot(jp < n && lab[jp] == 0.f);
      if (lane == 0) s_mask[wave] = mk;
      __syncthreads();
      for (int w = 0; w < 4; ++w) {
        const unsigned long long mm = s_mask[w];
        const int c = __popcll(mm);
        if (has && pos < 0 && r >= seen && r < seen + c) pos = t0 + w * 64 + select_bit(mm, r - seen);
        seen += c;
      }
      __syncthreads();
    }
    const int d = final_rank(base, T, p + t, has, s_key);
    if (has && pos >= 0) {
      out_rows[o0 + d] = rows[pos];
      out_labels[o0 + d] = lab[pos];
      if (out_pos) out_pos[o0 + d] = pos;
    }
  }
}

// The ragged gather a shuffled batch needs for its history side: flat over the output, segment by binary search.
__global__ __launch_bounds__(256) void gather_segments_kernel(const int32_t* __restrict__ src, const float* __restrict__ src_f,
                                                             const int64_t* __restrict__ src_off, int64_t n_seg, int64_t src_total,
                                                             const int64_t* __restrict__ imp_idx, int64_t B,
                                                             const int64_t* __restrict__ out_off, int64_t out_total,
                                                             int32_t* __restrict__ out, float* __restrict__ out_f,
                                                             int32_t* __restrict__ status) {
  const int64_t g = blockIdx.x * 256ll + threadIdx.x, stride = 256ll * gridDim.x;
  for (int64_t b = g; b < B; b += stride) {                        // a segment without output elements is checked too
    const int64_t imp = imp_idx[b];
    int flag = 0;
    if (imp < 0 || imp >= n_seg) flag = MANNER_HIP_STATUS_INDEX;
    else if (src_off[imp + 1] - src_off[imp] != out_off[b + 1] - out_off[b]) flag = MANNER_HIP_STATUS_LENGTHS;
    if (flag && status) atomicOr(status, flag);
  }
  for (int64_t j = g; j < out_total; j += stride) {
    int64_t lo = 0, hi = B;                                        // largest b with out_off[b] <= j
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (out_off[mid] <= j) lo = mid; else hi = mid;
    }
    const int64_t k = j - out_off[lo], imp = imp_idx[lo];
    int32_t v = 0;
    float f = 0.f;
    if (imp >= 0 && imp < n_seg) {
      const int64_t s0 = src_off[imp], len = src_off[imp + 1] - s0;
      if (k >= 0 && k < len && len == out_off[lo + 1] - out_off[lo] && s0 >= 0 && s0 + k < src_total) {
        v = src[s0 + k];
        if (src_f) f = src_f[s0 + k];
      } else if (status) {
        atomicOr(status, MANNER_HIP_STATUS_LENGTHS);
      }
    }
    out[j] = v;
    if (out_f) out_f[j] = f;
  }
}

// Longest stored news / entity list among the rows of a (sampled) batch: one workgroup, no atomics.
__global__ __launch_bounds__(256) void rows_max_len_kernel(const int32_t* __restrict__ store_len, const int32_t* __restrict__ store_cnt,
                                                          int64_t n_news, const int32_t* __restrict__ rows, int64_t M,
                                                          int32_t* __restrict__ out_max) {
  __shared__ int s_max[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ml = 0, mc = 0;
  for (int64_t r = tid; r < M; r += 256) {
    int64_t src = rows[r];
    src = src < 0 ? 0 : (src >= n_news ? n_news - 1 : src);
    ml = max(ml, store_len[src]);
    if (store_cnt) mc = max(mc, store_cnt[src]);
  }
  for (int o = 32; o > 0; o >>= 1) { ml = max(ml, __shfl_xor(ml, o, 64)); mc = max(mc, __shfl_xor(mc, o, 64)); }
  if (lane == 0) { s_max[wave] = ml; s_max[4 + wave] = mc; }
  __syncthreads();
  if (tid == 0) {
    out_max[0] = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    out_max[1] = max(max(s_max[4], s_max[5]), max(s_max[6], s_max[7]));
  }
}

// ------------------------------------------------------------------------------------------ A-Module batches
// MPerClassSampler as MINDNewsDataModule uses it (manner/data/mind_news_datamodule.py:175-217) as a counter-based rule (stated in
// include/manner_hip.h, "A-Module batches"): a whole epoch in one launch, one wave per block (b, j) of m slots.  The class choice is
// a rank count over the L keys of batch b (each wave of the batch recounts it: L <= 1024 keys in LDS); Floyd's subset algorithm keeps
// the drawn set spread over the lanes, draw t in lane t & 63, register t >> 6, and its membership test is one wave-wide compare a step.
constexpr int MPC_MAX_M = 256, MPC_MAX_L = 1024;

__global__ __launch_bounds__(256) void m_per_class_kernel(const int64_t* __restrict__ class_off, const int32_t* __restrict__ class_members,
                                                         const int64_t* __restrict__ class_label, int L, int64_t N,
                                                         const int32_t* __restrict__ rows, int64_t n_news, int m, int k, int64_t units,
                                                         uint64_t seed_epoch, int32_t* __restrict__ out_idx, int32_t* __restrict__ out_rows,
                                                         int64_t* __restrict__ out_labels, int32_t* __restrict__ status) {
  __shared__ uint64_t s_key[4][MPC_MAX_L];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t unit_raw = blockIdx.x * 4ll + wave;
  const bool active = unit_raw < units;
  const int64_t unit = active ? unit_raw : units - 1;     // an idle wave of the last workgroup recounts the last unit and writes nothing
  const int64_t b = unit / k;
  const int j = (int)(unit - b * k);

  uint64_t* keys = s_key[wave];
  const uint64_t base_b = mix64(seed_epoch ^ (uint64_t)b);
  for (int l = lane; l < L; l += 64) keys[l] = slot_key(base_b, 16, l);
  __syncthreads();
  int cls = -1;                                           // the class of rank j by (key, l): the ranks are a permutation, so one lane hits
  for (int c0 = 0; c0 < L; c0 += 64) {
    const int l = c0 + lane;
    int r = -1;
    if (l < L) {
      const uint64_t kl = keys[l];
      r = 0;
      for (int i = 0; i < L; ++i) {
        const uint64_t ki = keys[i];
        r += (ki < kl) || (ki == kl && i < l);
      }
    }
    const unsigned long long hit = __ballot(r == j);
    if (hit) cls = c0 + __builtin_ctzll(hit);
  }
  if (!active || cls < 0) return;                         // (no barrier below)

  const int64_t o0 = class_off[cls], o1 = class_off[cls + 1];
  const int64_t label = class_label[cls];
  const int64_t out0 = unit * m;
  if (o0 < 0 || o1 > N || o1 <= o0) {                     // a class without members, or offsets that leave class_members
    for (int t = lane; t < m; t += 64) { out_idx[out0 + t] = 0; out_rows[out0 + t] = 0; out_labels[out0 + t] = label; }
    if (lane == 0 && status) atomicOr(status, MANNER_HIP_STATUS_INDEX);
    return;
  }
  const int n = (int)(o1 - o0);                           // N < 2^31

  const uint64_t base_u = mix64(seed_epoch ^ (uint64_t)unit);
  uint32_t h[4];
  int d[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    h[s] = (uint32_t)(slot_key(base_u, 17, s * 64 + lane) >> 32);
    d[s] = -1;
  }
  if (n >= m) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int lim = m - s * 64 < 64 ? m - s * 64 : 64;
      for (int i = 0; i < lim; ++i) {
        const uint32_t ht = (uint32_t)__shfl((int)h[s], i, 64);
        const int J = n - m + s * 64 + i;
        const int r = (int)(((uint64_t)ht * (uint64_t)(J + 1)) >> 32);
        const bool seen = d[0] == r || d[1] == r || d[2] == r || d[3] == r;
        const int v = __ballot(seen) ? J : r;
        if (lane == i) d[s] = v;
      }
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) d[s] = (int)(((uint64_t)h[s] * (uint64_t)n) >> 32);
  }

  int flag = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int t = s * 64 + lane;
    if (t < m) {                                          // 0 <= d[s] < n, so the read of class_members is inside [o0, o1)
      int64_t idx = class_members[o0 + d[s]];
      if (idx < 0 || idx >= N) { flag = MANNER_HIP_STATUS_INDEX; idx = idx < 0 ? 0 : N - 1; }
      int64_t row = rows[idx];
      if (row < 0 || row >= n_news) { flag = MANNER_HIP_STATUS_INDEX; row = row < 0 ? 0 : n_news - 1; }
      out_idx[out0 + t] = (int32_t)idx;
      out_rows[out0 + t] = (int32_t)row;
      out_labels[out0 + t] = label;
    }
  }
  if (flag && status) atomicOr(status, flag);
}

// The padding=True widths of every batch of the epoch: one wave per batch over the store rows the launch above wrote.
__global__ __launch_bounds__(256) void batch_width_kernel(const int32_t* __restrict__ store_len, const int32_t* __restrict__ store_cnt,
                                                         int64_t n_news, const int32_t* __restrict__ batch_rows, int64_t B, int64_t nb,
                                                         int32_t* __restrict__ out_width) {
  const int lane = threadIdx.x & 63;
  const int64_t b = blockIdx.x * 4ll + (threadIdx.x >> 6);
  if (b >= nb) return;
  const int32_t* r = batch_rows + b * B;
  int ml = 0, mc = 0;
  for (int64_t i = lane; i < B; i += 64) {
    int64_t src = r[i];
    src = src < 0 ? 0 : (src >= n_news ? n_news - 1 : src);
    ml = max(ml, store_len[src]);
    if (store_cnt) mc = max(mc, store_cnt[src]);
  }
  for (int o = 32; o > 0; o >>= 1) { ml = max(ml, __shfl_xor(ml, o, 64)); mc = max(mc, __shfl_xor(mc, o, 64)); }
  if (lane == 0) { out_width[2 * b] = ml; out_width[2 * b + 1] = mc; }
}

unsigned grid_for(int64_t n) { return (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

}  // namespace
}  // namespace manner

using namespace manner;

extern "C" {

int manner_hip_collate_segments(const int64_t* off, int64_t B, int64_t total, int64_t* seg, manner_hip_stream_t stream) {
  if (B < 0 || total < 0 || (total && (!off || !seg || B == 0))) return fail(MANNER_HIP_E_INVALID, "collate_segments: bad argument");
  if (total == 0) return MANNER_HIP_OK;
  hipLaunchKernelGGL(segments_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, off, B, total, seg);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_collate_text(const int32_t* store_ids, const int32_t* store_len, int64_t n_news, int32_t Ls,
                            const int32_t* rows, int64_t M, int32_t Lp, int32_t pad_id, int64_t* ids, int64_t* mask,
                            manner_hip_stream_t stream) {
  if (M == 0 || Lp == 0) return MANNER_HIP_OK;
  if (!store_ids || !store_len || !rows || !ids || !mask || n_news <= 0 || Ls <= 0 || Lp < 0 || M < 0)
    return fail(MANNER_HIP_E_INVALID, "collate_text: bad argument");
  hipLaunchKernelGGL(text_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, store_ids, store_len, n_news,
                     (int)Ls, rows, M, (int)Lp, (int)pad_id, ids, mask);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_collate_entities(const int32_t* store_ent, const int32_t* store_cnt, int64_t n_news, int32_t Es,
                                const int32_t* rows, int64_t M, int32_t E, int64_t* out, manner_hip_stream_t stream) {
  if (M == 0 || E == 0) return MANNER_HIP_OK;
  if (!store_ent || !store_cnt || !rows || !out || n_news <= 0 || Es <= 0 || E < 0 || M < 0)
    return fail(MANNER_HIP_E_INVALID, "collate_entities: bad argument");
  hipLaunchKernelGGL(entities_kernel, dim3(grid_for(M * (int64_t)E)), dim3(256), 0, (hipStream_t)stream, store_ent, store_cnt,
                     n_news, (int)Es, rows, M, (int)E, out);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_collate_aspects(const int32_t* category, const int32_t* sentiment, const float* sentiment_score, int64_t n_news,
                               const int32_t* rows, int64_t M, int64_t* out_category, int64_t* out_sentiment,
                               float* out_score, manner_hip_stream_t stream) {
  if (M == 0) return MANNER_HIP_OK;
  if (!rows || n_news <= 0 || M < 0 || (out_category && !category) || (out_sentiment && !sentiment) ||
      (out_score && !sentiment_score))
    return fail(MANNER_HIP_E_INVALID, "collate_aspects: bad argument");
  hipLaunchKernelGGL(aspects_kernel, dim3(grid_for(M)), dim3(256), 0, (hipStream_t)stream, category, sentiment, sentiment_score,
                     n_news, rows, M, out_category, out_sentiment, out_score);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_sample_candidates(const int32_t* cand_rows, const float* labels, const int64_t* cand_off, int64_t n_imp,
                                 int64_t total, const int64_t* users, const int64_t* imp_idx, int64_t B, const int64_t* out_off,
                                 int64_t out_total, int32_t ratio, uint64_t seed, uint64_t epoch, int32_t* out_rows,
                                 float* out_labels, int32_t* out_pos, int64_t* out_users, int32_t* status,
                                 manner_hip_stream_t stream) {
  if (B < 0 || n_imp < 0 || total < 0 || out_total < 0 || ratio < 0 || B > 0x7fffffff || (B && (!users != !out_users)))
    return fail(MANNER_HIP_E_INVALID, "sample_candidates: bad argument");
  if (B == 0) return MANNER_HIP_OK;
  if (!cand_off || !imp_idx || !out_off || (total && (!cand_rows || !labels)) || (out_total && (!out_rows || !out_labels)))
    return fail(MANNER_HIP_E_INVALID, "sample_candidates: null argument");
  const uint64_t seed_epoch = mix64(seed + 0x9E3779B97F4A7C15ull * (epoch + 1));
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, cand_rows, labels, cand_off, n_imp, total,
                     users, imp_idx, out_off, out_total, (int)ratio, seed_epoch, out_rows, out_labels, out_pos, out_users, status);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_gather_segments(const int32_t* src, const float* src_f, const int64_t* src_off, int64_t n_seg, int64_t src_total,
                               const int64_t* imp_idx, int64_t B, const int64_t* out_off, int64_t out_total, int32_t* out,
                               float* out_f, int32_t* status, manner_hip_stream_t stream) {
  if (B < 0 || n_seg < 0 || src_total < 0 || out_total < 0 || (out_total && (!src_f != !out_f)) || (out_total && B == 0))
    return fail(MANNER_HIP_E_INVALID, "gather_segments: bad argument");
  if (B == 0) return MANNER_HIP_OK;
  if (!src_off || !imp_idx || !out_off || (out_total && (!src || !out)))
    return fail(MANNER_HIP_E_INVALID, "gather_segments: null argument");
  hipLaunchKernelGGL(gather_segments_kernel, dim3(grid_for(out_total > B ? out_total : B)), dim3(256), 0, (hipStream_t)stream, src,
                     src_f, src_off, n_seg, src_total, imp_idx, B, out_off, out_total, out, out_f, status);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_rows_max_len(const int32_t* store_len, const int32_t* store_cnt, int64_t n_news, const int32_t* rows, int64_t M,
                            int32_t* out_max, manner_hip_stream_t stream) {
  if (!out_max || M < 0 || (M && (!store_len || !rows || n_news <= 0)))
    return fail(MANNER_HIP_E_INVALID, "rows_max_len: bad argument");
  hipLaunchKernelGGL(rows_max_len_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, store_len, store_cnt, n_news, rows, M, out_max);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

int manner_hip_sample_m_per_class(const int64_t* class_off, const int32_t* class_members, const int64_t* class_label, int32_t L,
                                  int64_t N, const int32_t* rows, const int32_t* store_len, const int32_t* store_cnt, int64_t n_news,
                                  int32_t m, int32_t k, int64_t nb, uint64_t seed, uint64_t epoch, int32_t* out_idx,
                                  int32_t* out_rows, int64_t* out_labels, int32_t* out_width, int32_t* status,
                                  manner_hip_stream_t stream) {
  if (m < 1 || m > MPC_MAX_M) return fail(MANNER_HIP_E_INVALID, "sample_m_per_class: m = %d outside [1, %d]", (int)m, MPC_MAX_M);
  if (L < 1 || L > MPC_MAX_L) return fail(MANNER_HIP_E_INVALID, "sample_m_per_class: L = %d outside [1, %d]", (int)L, MPC_MAX_L);
  if (k < 1 || k > L) return fail(MANNER_HIP_E_INVALID, "sample_m_per_class: k = %d outside [1, L = %d]", (int)k, (int)L);
  if (N < 1 || N > 0x7fffffff || n_news < 1 || nb < 0) return fail(MANNER_HIP_E_INVALID, "sample_m_per_class: bad argument");
  const int64_t B = (int64_t)k * m;                       // <= 2^18 after the checks above
  if (nb > 0x7fffffff / B) return fail(MANNER_HIP_E_INVALID, "sample_m_per_class: nb * k * m overflows 2^31");
  if (nb == 0) return MANNER_HIP_OK;
  if (!class_off || !class_members || !class_label || !rows || !store_len || !out_idx || !out_rows || !out_labels || !out_width)
    return fail(MANNER_HIP_E_INVALID, "sample_m_per_class: null argument");
  const int64_t units = nb * k;
  const uint64_t seed_epoch = mix64(seed + 0x9E3779B97F4A7C15ull * (epoch + 1));
  hipLaunchKernelGGL(m_per_class_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, (hipStream_t)stream, class_off, class_members,
                     class_label, (int)L, N, rows, n_news, (int)m, (int)k, units, seed_epoch, out_idx, out_rows, out_labels, status);
  MANNER_LAUNCH_CHECK();
  hipLaunchKernelGGL(batch_width_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, (hipStream_t)stream, store_len, store_cnt, n_news,
                     out_rows, B, nb, out_width);
  MANNER_LAUNCH_CHECK();
  return MANNER_HIP_OK;
}

}  // extern "C"
