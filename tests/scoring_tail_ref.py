"""Plain float64 references, derived error bounds, float32 emulations and shared case builders for the tail of the inference hot
path: the fused gather-mean-dot scorers (five kernel forms), the half-table copy, the additive pooler and ``dot``
(csrc/scoring.hip, csrc/pool.hip).  numpy only; nothing here imports manner_amd.hip.  The host test (test_scoring_tail_host.py)
and the GPU test (test_gpu_scoring_tail.py) build their inputs here, so both see the same bytes.

References (the literal formula of cr_module.py:116-131 as manner_oracle.cr_scores restates it):

    score[j] = < sum_h table[hist[h]] / H , table[cand[j]] >                      late_fusion
    score[j] = < user[b] , table[cand[j]] >                                       late_fusion_user
    score[j] = < mu + sum_h T'[hist[h]] / H , mu + T'[cand[j]] >                  late_fusion_half (T' = stored halves, mu optional)

Each returns, next to the float64 scores, the ERROR SCALE A_j of every candidate: the sum of the magnitudes of everything
the kernel adds up for it,

    A_j = sum_c |x_c| (sum_h |t_hc|) / H                     history forms (x = the candidate row, t = the history rows)
    A_j = sum_c |x_c u_c|                                    given user
    A_j = sum_c W_c (|x'_c| + |mu_c|),  W_c = |mu_c| + (sum_h |t'_hc|) / H       centred half table

DERIVED BOUNDS.  With u = 2^-24 (float32 round to nearest), every float32 addition, product, division or fused multiply-add
of the kernel contributes at most u times the magnitude of its result, and that magnitude is at most A_j once it is carried
through to the score.  So |kernel - float64| <= n u A_j (1 + small), where n counts the roundings on the longest path from
a table entry to the score and the second-order terms (n u < 1e-5 here) are covered by the factor 1.01.  Adding an exact
zero, the first addition into a zero accumulator and the float16 -> float32 conversions are exact and still counted where
that keeps a formula simple: the counts are upper bounds.  No measured number enters them.

  f32, column-block kernel (score_late_fusion_kernel) and whole-row kernel (score_rows_body), same order of operations:
    user vector: a wave adds its ceil(H/4) rows (<= ceil(H/4) additions), the four waves' partial sums meet in two
                 additions, one division by H                                                   ceil(H/4) + 3
    dot:         one product, two additions inside the 4-wide piece, one addition per 256-column trip (ceil(D/256)),
                 six shuffle steps over the 64 lanes                                           ceil(D/256) + 9
    n = ceil(H/4) + ceil(D/256) + 12
  given user (score_user, both kernels): the dot alone                                   n = ceil(D/256) + 9
  f16 table, column-block kernel (score_late_fusion_f16_kernel):
    user vector as above (the halves convert exactly)                                          ceil(H/4) + 3
    dot:         one product, three additions inside the 8-wide piece, one per 512-column trip, six shuffle steps
                                                                                               ceil(D/512) + 10
    n = ceil(H/4) + ceil(D/512) + 13
  f16 table, whole-row kernel (score_late_fusion_f16_rows_kernel, D = 256 NCB):
    user vector: a half-wave adds its ceil(H/8) rows, one addition joins the wave's two halves, two additions join the
                 waves, one division                                                           ceil(H/8) + 4
    dot:         one product, three in-piece additions, one addition per 256-column piece (NCB), five shuffle steps over
                 the 32 lanes of the row                                                       D/256 + 9
    n = ceil(H/8) + D/256 + 13
  centred table (either f16 kernel): w = u + mu is one more rounding of the user vector; the constant <w, mu> is a chain
    of ceil(D/256) fused multiply-adds per thread, six shuffle steps and two additions over the waves (ceil(D/256) + 8,
    its inputs carrying the user vector's roundings); one last addition joins the dot and the constant.  Dot and
    constant are disjoint sums, so the longer of the two chains bounds both:
    n = [user] + 1 + max([dot], ceil(D/256) + 8) + 1
  column mean (col_partial_kernel + col_mean_kernel): a block adds every 256th row into two accumulators,
    M = ceil(n_rows/256) rows per block -> <= ceil(M/2) additions and one joining them; the 256 partial sums and the
    division are double precision (256 2^-53, counted as 2^-44 relative); one rounding to float32:
    |mean - ref| <= 1.01 (ceil(M/2) + 2) u (sum_r |t_rc|) / n_rows
  dot (manner_hip_dot), A = sum_c |x_c u_c|:
    vector rows form: as the scorer's dot                                                n = ceil(D/256) + 9
    scalar rows form: one product and one addition per 64-column trip, six shuffle steps n = 2 ceil(D/64) + 6
    strided form:     a chain of D fused multiply-adds                                   n = D
  (the compiler may fuse a product into the addition that follows it in the two rows forms: fewer roundings, same bound).

EMULATIONS.  ``emulate_*`` redo each scorer form in float32 numpy in the kernel's order of operations (row -> wave
assignment, the j + 4 q slot rule, in-piece association, trip order, xor butterfly).  The host test holds them under the
bounds, and plants one defect at a time (DEFECTS) to show that the bounds are tight enough to notice each.
"""
import math
import zlib

import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.01

H_LIST = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 50)
C_LIST = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33)
F32_WIDTHS = (4, 100, 252, 256, 260, 512, 768, 1024, 3072)
F16_WIDTHS = (8, 264, 504, 512, 520, 768, 1024, 3072)
SCORER_REGIMES = ("randn", "collinear", "scale_down", "scale_up", "outlier")
EXACT_H = (1, 2, 4, 8, 16)


# ------------------------------------------------------------------------------------------------ references

def _segments(off):
    off = np.asarray(off, np.int64)
    return [(int(off[i]), int(off[i + 1])) for i in range(len(off) - 1)]


def hist_sizes_per_candidate(hist_off, cand_off):
    """H of the impression each candidate belongs to, int64 [sum c_i]."""
    h = np.diff(np.asarray(hist_off, np.int64))
    return np.repeat(h, np.diff(np.asarray(cand_off, np.int64)))


def late_fusion(table, hist_idx, hist_off, cand_idx, cand_off):
    """(scores, A): float64 ragged scores <mean(table[hist]), table[cand]> and their error scales."""
    t = np.asarray(table, np.float64)
    scores, scale = [], []
    for (h0, h1), (c0, c1) in zip(_segments(hist_off), _segments(cand_off)):
        rows = t[np.asarray(hist_idx[h0:h1], np.int64)]
        user = rows.sum(0) / float(h1 - h0)
        mag = np.abs(rows).sum(0) / float(h1 - h0)
        cand = t[np.asarray(cand_idx[c0:c1], np.int64)]
        scores.append(cand @ user)
        scale.append(np.abs(cand) @ mag)
    return np.concatenate(scores) if scores else np.zeros(0), np.concatenate(scale) if scale else np.zeros(0)


def late_fusion_user(table, user, cand_idx, cand_off):
    """(scores, A) for given user vectors [B, D]."""
    t, u = np.asarray(table, np.float64), np.asarray(user, np.float64)
    scores, scale = [], []
    for b, (c0, c1) in enumerate(_segments(cand_off)):
        cand = t[np.asarray(cand_idx[c0:c1], np.int64)]
        scores.append(cand @ u[b])
        scale.append(np.abs(cand) @ np.abs(u[b]))
    return np.concatenate(scores), np.concatenate(scale)


def late_fusion_half(rows16, mean, hist_idx, hist_off, cand_idx, cand_off):
    """(scores, A) over a stored half table ``rows16`` (the values read back from the device) and its optional mean [D]:
    <mu + mean(T'[hist]), mu + T'[cand]>.  Only the accumulation is judged, not the rounding of the stored rows."""
    t = np.asarray(rows16, np.float64)
    mu = np.zeros(t.shape[1]) if mean is None else np.asarray(mean, np.float64)
    scores, scale = [], []
    for (h0, h1), (c0, c1) in zip(_segments(hist_off), _segments(cand_off)):
        rows = t[np.asarray(hist_idx[h0:h1], np.int64)]
        w = mu + rows.sum(0) / float(h1 - h0)
        wmag = np.abs(mu) + np.abs(rows).sum(0) / float(h1 - h0)
        cand = t[np.asarray(cand_idx[c0:c1], np.int64)]
        scores.append((cand + mu) @ w)
        scale.append((np.abs(cand) + np.abs(mu)) @ wmag)
    return np.concatenate(scores), np.concatenate(scale)


def column_mean(table):
    """(mean, scale): float64 column mean [D] and sum_r |t_rc| / n_rows."""
    t = np.asarray(table, np.float64)
    return t.mean(0), np.abs(t).mean(0)


def additive_pool(x, lin_w, lin_b, query):
    """AdditiveAttention.forward (attention.py:21-27) in float64: softmax_s(tanh(x W^T + b) q) weighted sum of x; [B, D]."""
    x, w, b, q = (np.asarray(a, np.float64) for a in (x, lin_w, lin_b, query))
    logits = np.tanh(x @ w.T + b) @ q                                    # [B, S]
    e = np.exp(logits - logits.max(1, keepdims=True))
    wts = e / e.sum(1, keepdims=True)
    return np.einsum("bs,bsd->bd", wts, x)


def dot(user, cand):
    """(scores, A): DotProduct contract, user [B, 1, D], cand [B, D, C] -> [B, C] in float64."""
    u, c = np.asarray(user, np.float64), np.asarray(cand, np.float64)
    return np.einsum("bod,bdc->bc", u, c), np.einsum("bod,bdc->bc", np.abs(u), np.abs(c))


# ------------------------------------------------------------------------------------------------ derived bounds

def _ceil(a, b):
    return -(-np.asarray(a, np.int64) // b)


def ops_f32(H, D):
    return _ceil(H, 4) + math.ceil(D / 256) + 12


def ops_user(D):
    return math.ceil(D / 256) + 9


def ops_f16_block(H, D, centred=False):
    user, dotn = _ceil(H, 4) + 3, math.ceil(D / 512) + 10
    return user + 1 + max(dotn, math.ceil(D / 256) + 8) + 1 if centred else user + dotn


def ops_f16_rows(H, D, centred=False):
    user, dotn = _ceil(H, 8) + 4, D // 256 + 9
    return user + 1 + max(dotn, D // 256 + 8) + 1 if centred else user + dotn


def ops_col_mean(n_rows):
    return math.ceil(math.ceil(n_rows / 256) / 2) + 2


def ops_dot(form, D):
    return {"vector": math.ceil(D / 256) + 9, "scalar": 2 * math.ceil(D / 64) + 6, "strided": D}[form]


def bound(ops, scale):
    """|kernel - float64| <= 1.01 ops u A."""
    return SECOND_ORDER * np.asarray(ops, np.float64) * U * np.asarray(scale, np.float64)


def ratio_to_bound(err, bnd):
    """error / bound per entry; where the bound is zero (every term of the sum is zero) the kernel must return exactly zero"""
    err, bnd = np.asarray(err, np.float64), np.asarray(bnd, np.float64)
    return np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err == 0, 0.0, np.inf))


def scorer_ops(form, H, D, centred=False):
    """``form``: f32_block | f32_rows | user | f16_block | f16_rows."""
    if form in ("f32_block", "f32_rows"):
        return ops_f32(H, D)
    if form == "user":
        return ops_user(D) + 0 * np.asarray(H, np.int64)
    return ops_f16_block(H, D, centred) if form == "f16_block" else ops_f16_rows(H, D, centred)


def f32_form(D, generic=False):
    return "f32_rows" if D in (768, 1024) and not generic else "f32_block"


def f16_form(D, generic=False):
    return "f16_rows" if D in (768, 1024) and not generic else "f16_block"


# ------------------------------------------------------------------------------------------------ float32 emulations

DEFECTS = ("drop_last_hist_when_h_mod_8_is_1", "slot_plus_4_scored_for_slot", "divide_by_h_plus_1", "tail_column_block_skipped",
           "upper_half_wave_reads_ja", "centring_constant_left_out")
f32 = np.float32


def _butterfly(v, lanes):
    """xor butterfly over the last axis (``lanes`` wide): every lane ends with the sum; lane 0 is returned."""
    idx = np.arange(lanes)
    o = lanes // 2
    while o:
        v = v + v[..., idx ^ o]
        o //= 2
    return v[..., 0]


def _wave_sums(t32, idx, n_streams, defect):
    """partial sums of the history rows: stream s adds rows s, s + n_streams, ... in order, starting from +0"""
    if defect == "drop_last_hist_when_h_mod_8_is_1" and len(idx) % 8 == 1:
        idx = idx[:-1]
    parts = np.zeros((n_streams, t32.shape[1]), f32)
    for s in range(n_streams):
        for j in range(s, len(idx), n_streams):
            parts[s] = parts[s] + t32[idx[j]]
    return parts


def _quad_dot(rows, user, piece, trip, lanes):
    """rows [C, D] . user [D]: in-piece tree of ``piece`` products, one addition per ``trip`` columns, xor butterfly"""
    C, D = rows.shape
    Dp = -(-D // trip) * trip
    p = np.zeros((C, Dp), f32)
    p[:, :D] = rows * user[None, :]                                     # float32 products; columns past D add exact zeros
    p = p.reshape(C, Dp // trip, lanes, piece)
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    p = p[..., 0]
    a = np.zeros((C, lanes), f32)
    for k in range(p.shape[1]):
        a = a + p[:, k]
    return _butterfly(a, lanes)


def emulate_f32(table, hist_idx, hist_off, cand_idx, cand_off, user=None, defect=None):
    """score_late_fusion_kernel / score_rows_body (one order of operations for both) and, with ``user``, score_user."""
    t = np.asarray(table, f32)
    D = t.shape[1]
    out = np.zeros(int(np.asarray(cand_off)[-1]), f32)
    hist = _segments(hist_off) if user is None else [None] * (len(cand_off) - 1)
    for b, (hs, (c0, c1)) in enumerate(zip(hist, _segments(cand_off))):
        if user is None:
            idx = np.asarray(hist_idx[hs[0]:hs[1]], np.int64)
            p = _wave_sums(t, idx, 4, defect)
            hn = f32(len(idx) + (1 if defect == "divide_by_h_plus_1" else 0))
            u = ((p[0] + p[1]) + (p[2] + p[3])) / hn
        else:
            u = np.asarray(user[b], f32)
        ci = np.asarray(cand_idx[c0:c1], np.int64)
        if defect == "slot_plus_4_scored_for_slot":
            ci = np.array([ci[j + 4] if j + 4 < len(ci) else ci[j] for j in range(len(ci))], np.int64)
        uu = u.copy()
        if defect == "tail_column_block_skipped":
            uu[256 * (D // 256):] = 0
        if len(ci):
            out[c0:c1] = _quad_dot(t[ci], uu, 4, 256, 64)
    return out


def _centre(u, mean, D):
    """w = u + mu and <w, mu>: thread t runs a fused multiply-add chain over columns t, t + 256, ...; butterfly; 4 waves"""
    m = np.asarray(mean, f32)
    w = u + m
    Dp = -(-D // 256) * 256
    w64, m64 = np.zeros(Dp), np.zeros(Dp)
    w64[:D], m64[:D] = w, m
    cp = np.zeros(256, f32)
    for k in range(Dp // 256):                                          # fmaf: product exact in float64, one rounding
        cp = (w64[256 * k:256 * k + 256] * m64[256 * k:256 * k + 256] + cp.astype(np.float64)).astype(f32)
    cw = _butterfly(cp.reshape(4, 64), 64)
    return w, (cw[0] + cw[1]) + (cw[2] + cw[3])


def emulate_f16_block(rows16, mean, hist_idx, hist_off, cand_idx, cand_off, defect=None):
    """score_late_fusion_f16_kernel: 8-wide pieces, 512-column trips, optional centring constant."""
    t = np.asarray(rows16, np.float16).astype(f32)
    D = t.shape[1]
    out = np.zeros(int(np.asarray(cand_off)[-1]), f32)
    for (h0, h1), (c0, c1) in zip(_segments(hist_off), _segments(cand_off)):
        idx = np.asarray(hist_idx[h0:h1], np.int64)
        p = _wave_sums(t, idx, 4, defect)
        u = ((p[0] + p[1]) + (p[2] + p[3])) / f32(len(idx) + (1 if defect == "divide_by_h_plus_1" else 0))
        konst = f32(0)
        if mean is not None:
            u, konst = _centre(u, mean, D)
            if defect == "centring_constant_left_out":
                konst = f32(0)
        ci = np.asarray(cand_idx[c0:c1], np.int64)
        if len(ci):
            out[c0:c1] = _quad_dot(t[ci], u, 8, 512, 64) + konst
    return out


def emulate_f16_rows(rows16, mean, hist_idx, hist_off, cand_idx, cand_off, defect=None):
    """score_late_fusion_f16_rows_kernel (D = 256 NCB): list position p goes to wave (p % 8) // 2, half-wave p % 2; a half-wave
    of 32 lanes holds a whole row in NCB 8-wide pieces."""
    t = np.asarray(rows16, np.float16).astype(f32)
    D = t.shape[1]
    assert D % 256 == 0
    out = np.zeros(int(np.asarray(cand_off)[-1]), f32)
    for (h0, h1), (c0, c1) in zip(_segments(hist_off), _segments(cand_off)):
        idx = np.asarray(hist_idx[h0:h1], np.int64)
        p = _wave_sums(t, idx, 8, defect)                               # stream 2 wave + half
        p = p[0::2] + p[1::2]                                           # the wave's two halves
        u = ((p[0] + p[1]) + (p[2] + p[3])) / f32(len(idx) + (1 if defect == "divide_by_h_plus_1" else 0))
        konst = f32(0)
        if mean is not None:
            u, konst = _centre(u, mean, D)
            if defect == "centring_constant_left_out":
                konst = f32(0)
        ci = np.asarray(cand_idx[c0:c1], np.int64)
        if defect == "upper_half_wave_reads_ja":
            ci = np.array([ci[j - 1] if j % 2 else ci[j] for j in range(len(ci))], np.int64)
        if len(ci):
            out[c0:c1] = _quad_dot(t[ci], u, 8, 256, 32) + konst
    return out


# ------------------------------------------------------------------------------------------------ case builders

def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def make_table(regime, n_rows, D, rng):
    t = rng.standard_normal((n_rows, D))
    if regime == "collinear":                                           # one encoder's [CLS] rows: |score| in the hundreds
        t = rng.standard_normal(D)[None, :] + 0.05 * t
    elif regime == "scale_down":
        t = t * 2.0 ** -10
    elif regime == "scale_up":
        t = t * 2.0 ** 10
    elif regime == "outlier":
        cols = rng.choice(D, size=min(2, D), replace=False)
        t[:, cols] *= 30.0
    elif regime == "integer":
        t = rng.integers(-8, 9, size=(n_rows, D)).astype(np.float64)
    else:
        assert regime == "randn", regime
    return t.astype(np.float32)


def _lists(rng, n_rows, hs, cs):
    hist_idx = rng.integers(0, n_rows, size=int(np.sum(hs))).astype(np.int32)
    cand_idx = rng.integers(0, n_rows, size=int(np.sum(cs))).astype(np.int32)
    return {"hist_idx": hist_idx, "hist_off": _offsets(hs), "cand_idx": cand_idx, "cand_off": _offsets(cs)}


def width_case(D, regime="randn", n_rows=300, n_imp=48):
    """48 ragged impressions (1 .. 50 history rows, 0 .. 33 candidates) over an [n_rows, D] table."""
    rng = _rng("width", D, regime, n_rows)
    cs = rng.integers(0, 34, size=n_imp)
    cs[-1] = max(cs[-1], 1)                                              # (to_dense_batch counts impressions up to the last candidate's)
    case = _lists(rng, n_rows, rng.integers(1, 51, size=n_imp), cs)
    case["table"] = make_table(regime, n_rows, D, rng)
    case["user"] = rng.standard_normal((n_imp, D)).astype(np.float32)
    case["name"] = f"{regime}-D{D}-n{n_rows}"
    return case


def lengths_case(D, n_rows=300):
    """one impression per (H, C) pair of H_LIST x C_LIST: every batch size of every form is crossed."""
    rng = _rng("lengths", D)
    pairs = [(h, c) for h in H_LIST for c in C_LIST]
    case = _lists(rng, n_rows, [h for h, _ in pairs], [c for _, c in pairs])
    case["table"] = make_table("randn", n_rows, D, rng)
    case["user"] = rng.standard_normal((len(pairs), D)).astype(np.float32)
    case["name"] = f"lengths-D{D}"
    return case


def exact_case(D, n_rows=300):
    """integer entries in [-8, 8], H in {1, 2, 4, 8, 16}, integer users: every float32 operation of every form is exact."""
    rng = _rng("exact", D)
    hs = [EXACT_H[i % len(EXACT_H)] for i in range(40)]
    cs = rng.integers(0, 34, size=len(hs))
    cs[-1] = max(cs[-1], 1)
    case = _lists(rng, n_rows, hs, cs)
    case["table"] = make_table("integer", n_rows, D, rng)
    case["user"] = rng.integers(-8, 9, size=(len(hs), D)).astype(np.float32)
    case["name"] = f"exact-D{D}"
    return case


# every scorer case of the two tests as a spec (kind, D, regime, n_rows): the widths, the list lengths at one width per kernel, the
# value regimes; for the half table also two tables with fewer rows than the mean's 256 partial-sum blocks
F32_SPECS = [("width", D, "randn", 300) for D in F32_WIDTHS] + [("lengths", 260, "randn", 300), ("lengths", 768, "randn", 300)] + \
    [("width", D, regime, 300) for D in (768, 260) for regime in SCORER_REGIMES[1:]]
F16_SPECS = [("width", D, "randn", 300) for D in F16_WIDTHS] + [("lengths", 520, "randn", 300), ("lengths", 768, "randn", 300)] + \
    [("width", D, regime, 300) for D in (768, 520) for regime in SCORER_REGIMES[1:]] + \
    [("width", 768, "collinear", 100), ("width", 520, "randn", 37)]


def spec_id(spec):
    return "-".join(str(s) for s in spec)


def build_case(spec):
    kind, D, regime, n_rows = spec
    return lengths_case(D, n_rows) if kind == "lengths" else width_case(D, regime, n_rows)


def f32_cases():
    return [build_case(s) for s in F32_SPECS]


def f16_cases():
    return [build_case(s) for s in F16_SPECS]


def half_rows(table32, mean=None):
    """the stored half table the copy must produce: half(float32(T) - mean) (mean read back from the device), or half(T)"""
    t = np.asarray(table32, np.float32)
    return (t if mean is None else t - np.asarray(mean, np.float32)[None, :]).astype(np.float16)


POOL_REGIMES = ("base", "peaked", "near_tie", "outlier", "row_scale", "zero_tail", "zero_element", "tiny_w", "big_w", "collinear")


def pool_case(regime, B, S, D, Q, soft=False):
    """(x [B, S, D], W [Q, D], bias [Q], query [Q]) float32: ``randn`` rows, ``0.05 randn`` weights, a ``randn`` query (x 8 in
    the peaked regimes: max softmax weight 0.7 in base, 0.99 peaked), then the regime.
    ``soft``: the query is ``randn / (2 sqrt(Q))``.  A logit is a sum of Q terms tanh(.) q_j, so ANY float32 evaluation carries
    an absolute logit error of a few u |q|_1 (more where a BLAS adds the 768 products of a unit one after the other), which the
    softmax turns into the same RELATIVE error of every weight: with |q|_1 = 0.8 Q = 160 .. 260 float32 itself reaches
    2e-6 .. 6e-6 max|x| on some cases, over a tenth of the two-pass cap, where a bar cannot tell a wrong kernel from rounding.
    Only the two-pass cases named in POOL_SOFT take the soft query; every one-pass case keeps ``randn``."""
    rng = _rng("pool", regime, B, S, D, Q)
    x = rng.standard_normal((B, S, D))
    w = 0.05 * rng.standard_normal((Q, D))
    bias = 0.05 * rng.standard_normal(Q)
    q = rng.standard_normal(Q) * (0.5 / math.sqrt(Q) if soft else 1.0)
    if regime in ("peaked", "near_tie"):
        q = q * 8.0
    if regime == "near_tie" and S > 1:
        # two near-tied top logits: the top row and a twin 1e-2 away (weights near 0.5 / 0.5).  Of 4 B drawn elements the B with the
        # widest gap from the top to the runner-up are kept, so the pair holds nearly all the weight: a near-tie between two
        # UNRELATED rows under q x 8 is ill-conditioned for float32 itself (a relative weight error of u |q|_1 times the rows' distance)
        x = rng.standard_normal((4 * B, S, D))
        lg = np.sort(np.tanh(x @ w.T + bias) @ q, axis=1)
        x = x[np.sort(np.argsort(lg[:, -2] - lg[:, -1])[:B])]
        lg = np.tanh(x @ w.T + bias) @ q
        for b in range(B):
            top = int(np.argmax(lg[b]))
            x[b, (top + 1) % S] = x[b, top] + 1e-2 * rng.standard_normal(D)
    elif regime == "outlier":
        c0, c1 = rng.choice(D, size=2, replace=False)
        x[:, :, c0] *= 30.0
        x[:, :, c1] *= -20.0
    elif regime == "row_scale":                                          # 10^-3 .. 10^3 inside one batch element
        x = x * (10.0 ** np.linspace(-3.0, 3.0, S))[None, :, None]
    elif regime == "zero_tail":
        x[1::2, S // 2:] = 0.0
        if B == 1:
            x[0, S // 2:] = 0.0
    elif regime == "zero_element":
        x[B // 2] = 0.0
    elif regime == "tiny_w":
        w = w * 1e-3
    elif regime == "big_w":
        w = w * 50.0
    elif regime == "collinear":
        x = rng.standard_normal(D)[None, None, :] + 0.05 * x
    else:
        assert regime in ("base", "peaked", "near_tie"), regime
    return tuple(a.astype(np.float32) for a in (x, w, bias, q))


def pool_error(out, ref, x):
    """max over batch elements of max|out - ref| / max(1, max|x| of the element)"""
    out, ref, x = np.asarray(out, np.float64), np.asarray(ref, np.float64), np.asarray(x, np.float64)
    scale = np.maximum(1.0, np.abs(x).reshape(x.shape[0], -1).max(1))
    return float((np.abs(out - ref).max(1) / scale).max())


# the pooler's case groups and the shapes each runs at, (B, S, D, Q): the three routes hip.additive_pool chooses by shape, and
# "strict" = strict=True at every one-pass shape (f32 MFMA logits for Q <= 256, VALU logits for Q = 320)
_ONE_PASS = [(b, s, 768, q) for q in (17, 200, 320) for b, s in [(1, 1), (3, 16), (7, 17), (7, 50), (3, 64), (7, 65), (3, 128)]]
POOL_ROUTE_SHAPES = {
    "one_pass": _ONE_PASS,
    "two_pass_mfma": [(b, s, d, q) for q in (200, 256) for b, s, d in [(3, 50, 32), (7, 50, 64), (3, 50, 800), (7, 20, 1024), (3, 50, 1056)]] +
                     [(1, 129, 768, 200), (3, 255, 768, 200), (3, 256, 768, 256), (3, 257, 768, 200), (7, 300, 768, 200)],
    "strict": _ONE_PASS,
    "valu": [(7, 50, 100, 200), (3, 50, 64, 257), (3, 17, 768, 321), (1, 50, 100, 257)],
}
# every regime runs at one shape per group
POOL_REGIME_SHAPE = {"one_pass": (7, 50, 768, 200), "two_pass_mfma": (3, 129, 768, 200), "strict": (7, 50, 768, 200),
                     "valu": (3, 50, 100, 257)}
POOL_CAPS = {"one_pass": 1e-4, "two_pass_mfma": 2e-5, "strict": 2e-5, "valu": 2e-5}
# the two-pass cases that take the soft query (pool_case): with q = randn, float32 torch is above 3e-7 on them — cap / 10 = 2e-6 less
# a factor of six for another machine's BLAS.  (group, regime) for the regime shape; (group, "sweep") for the group's shape list on
# ``randn`` inputs.  No one-pass case is softened.
POOL_SOFT = {("two_pass_mfma", r) for r in ("sweep", "base", "zero_tail", "zero_element", "big_w")} | \
    {("strict", r) for r in ("sweep", "base", "peaked", "outlier", "row_scale", "zero_tail", "big_w")} | \
    {("valu", r) for r in ("sweep", "base", "row_scale", "zero_tail", "big_w")}


def pool_soft(group, regime, sweep=False):
    return (group, "sweep" if sweep else regime) in POOL_SOFT


def pool_route(B, S, D, Q, strict=False):
    """the route manner_hip_additive_pool_fused takes for a shape: one_pass | mfma (f32 MFMA logits + apply) | valu"""
    if not strict and D == 768 and S <= 128 and Q <= 320:
        return "one_pass"
    return "mfma" if D % 32 == 0 and Q <= 256 else "valu"


def pool_group_route(group, shape):
    """the route a group's shape is meant to reach"""
    if group == "strict":
        return "mfma" if shape[3] <= 256 else "valu"
    return {"one_pass": "one_pass", "two_pass_mfma": "mfma", "valu": "valu"}[group]


def dot_case(B, C, D, integer=False):
    rng = _rng("dot", B, C, D, integer)
    if integer:
        return rng.integers(-8, 9, size=(B, 1, D)).astype(np.float32), rng.integers(-8, 9, size=(B, C, D)).astype(np.float32)
    return rng.standard_normal((B, 1, D)).astype(np.float32), rng.standard_normal((B, C, D)).astype(np.float32)
