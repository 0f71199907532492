"""Inputs and references of the evaluation metrics (csrc/metrics.hip and the K13-K15 / aspect kernels of csrc/scoring.hip): AUC, MRR,
nDCG@k, aspect diversity / personalization, the val/test loss and the z-score fusion, at ties, special values and tile edges.
No GPU in this file: tests/test_metrics_host.py checks it on the CPU, tests/test_gpu_metrics.py runs the kernels against it.

The arbiter is oracle/manner_oracle.py (``topk_indices``, ``ndcg_at_k``, ``mrr``, ``binary_auroc``, ``diversity_at_k``,
``personalization_at_k``, ``model_step_loss``, ``zscore``).  This file adds the two things it lacks — the integer Mann-Whitney count
by sort + searchsorted (``mann_whitney``: the oracle's trapezoid is too slow for the 16.8 M-pair carry case) and an explicit ``c_max``
in the cross-entropy loss (``loss_rows``) — dtype-generic restatements of the float quantities (evaluated in float32 on the CPU they
are the yardstick of the MEASURED bar, as in tests/side_ops_ref.py), and one defective variant per defect the inputs were chosen for.

Bars.  Integers (top-k lists, (2U, P, N)) are exact.  Floats on inputs the older tests cover in kind keep the project's bars (the
``*_BAR`` constants).  The regimes new here (``NEW`` in a case's name: graded labels, k = 100, c = 1000, losses at scale 700 and at -50
with padding, z-scores at 777 +- 0.2) are held to ``measured_bar``: 8 x the error of the float32 CPU evaluation of the same restatement
against float64, that error floored at 2^-25 (a float32 result sits up to a quarter to half an ulp from float64 whatever computed it).
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

import manner_oracle as O
from side_ops_ref import MEASURED_FACTOR, QUARTER_ULP

NDCG_BAR, MRR_BAR, DIV_BAR, PERS_BAR, LOSS_RTOL, ZSCORE_REL = 1e-6, 1e-7, 1e-5, 1e-6, 2e-5, 2e-4
FLT_MAX, FLT_MIN, DENORM = np.float32(3.4028235e38), np.float32(1.1754944e-38), np.float32(1e-45)
NAN, INF = np.float32("nan"), np.float32("inf")
RS_TILE = 4096                                               # keys per workgroup of the AUC's split / radix kernels


def measured_bar(cpu_f32: float) -> float:
    return MEASURED_FACTOR * max(float(cpu_f32), QUARTER_ULP)


def offsets(counts: Sequence[int]) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ ranking: inputs
RANK_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1000)
RANK_FLAVOURS = ("continuous", "constant", "tie_runs", "nan_mixed", "specials", "all_nan")
RANK_LABELS = ("binary", "zeros", "ones", "graded")
RANK_K = (1, 5, 10, 64, 65, 100)
FUSED_COUNTS, FUSED_K = (1, 2, 64, 255, 256, 257, 319, 320, 321, 513), (10, 65)
SPECIALS = np.array([INF, -INF, 0.0, -0.0, DENORM, -DENORM, FLT_MAX, -FLT_MAX, 1.0, -1.0], np.float32)
PROBE = np.array([FLT_MAX, NAN, 0.0, INF, -0.0, NAN, -INF, 1.0, DENORM, -DENORM], np.float32)
PROBE_ORDER = [1, 5, 3, 0, 7, 8, 2, 4, 9, 6]


def rank_scores(flavour: str, c: int, rng) -> np.ndarray:
    j = np.arange(c)
    if flavour == "continuous":
        s = rng.standard_normal(c)
    elif flavour == "constant":
        s = np.full(c, 0.25)
    elif flavour == "tie_runs":                                 # runs of 70 equal values from position 17 on: none starts or ends on a
        s = np.array([0.5, -1.0, 0.5, 2.0])[((j + 53) // 70) % 4]   # multiple of the 64-lane stride, and 0.5 comes back in a later run
    elif flavour == "nan_mixed":
        s = rng.standard_normal(c)
        s[j % 64 == 0] = np.nan
        s[-1:] = np.nan
    elif flavour == "specials":
        s = SPECIALS[rng.integers(0, SPECIALS.size, c)]
    else:
        s = np.full(c, np.nan)
    return s.astype(np.float32)


def rank_labels(kind: str, c: int, rng) -> np.ndarray:
    if kind == "binary":
        y = (rng.random(c) < 0.2).astype(np.float32)
        if c > 1:
            y[rng.integers(0, c)] = 1.0
    elif kind == "graded":
        y = rng.integers(0, 4, c).astype(np.float32)
    else:
        y = np.full(c, 1.0 if kind == "ones" else 0.0, np.float32)
    return y


def _rank_batch(counts, seed) -> Dict[str, object]:
    rng = np.random.default_rng(seed)
    rows, s, y = [], [], []
    for ci, c in enumerate(counts):
        for fi, fl in enumerate(RANK_FLAVOURS):
            kind = RANK_LABELS[(ci + fi) % 4]
            rows.append((c, fl, kind))
            s.append(rank_scores(fl, c, rng))
            y.append(rank_labels(kind, c, rng))
    return {"scores": np.concatenate(s), "labels": np.concatenate(y), "off": offsets([r[0] for r in rows]), "rows": rows}


@functools.lru_cache(maxsize=None)
def rank_cases() -> Dict[str, Dict[str, object]]:
    """{"ragged": every count x every score flavour (78 impressions: no multiple of 4, the impressions of one workgroup), label kinds
    cycled so that every flavour and every count meets all four; "single": B = 1, the nan_mixed row of 129 with graded labels;
    "fused": the same flavours at the counts around score_fuse_rank_kernel's 256-thread stride and its 320-candidate LDS bound — the
    values tests/test_gpu_metrics.py injects into that kernel}."""
    rng = np.random.default_rng(41)
    single = {"scores": rank_scores("nan_mixed", 129, rng), "labels": rank_labels("graded", 129, rng), "off": offsets([129]),
              "rows": [(129, "nan_mixed", "graded")]}
    return {"ragged": _rank_batch(RANK_COUNTS, 40), "single": single, "fused": _rank_batch(FUSED_COUNTS, 90)}


def rank_row_is_new(row, k: int) -> bool:
    return row[2] == "graded" or row[0] == 1000 or k == 100


# ------------------------------------------------------------------------------------------------ ranking: the kernel's rule, restated
def ranks_before(a, ia, b, ib, tie_high=False, nan_last=False, ge=False):
    """scoring.hip's ranks_before on arrays: descending, NaN first, ties to the lower index.  The keywords plant a defect each."""
    na, nb = np.isnan(a), np.isnan(b)
    first = (ia > ib) if tie_high else (ia < ib)
    with np.errstate(invalid="ignore"):
        plain = (a >= b) if ge else ((a > b) | ((a == b) & first))
    nans = (nb & (~na | first)) if nan_last else (na & (~nb | first))
    return np.where(na | nb, nans, plain)


def kernel_ranks(s: np.ndarray, **defect) -> np.ndarray:
    """rank[a] = #{j : s[j] ranks before s[a]}: what each lane of rank_ndcg_kernel counts"""
    j = np.arange(s.size)
    return ranks_before(s[:, None], j[:, None], s[None, :], j[None, :], **defect).sum(0).astype(np.int64)


def rank_metrics(scores, labels, off, ks, dtype=np.float64, cut_short=False, idcg_in_score_order=False, mrr_last=False, **defect):
    """{k: (top-k lists [B, k] with -1 fill, nDCG [B], MRR [B])} the way the kernel forms them: every candidate finds its own rank and
    writes itself there; DCG / IDCG are sums of label / log2(rank + 2) over the ranks below k, in ``dtype``.  Without a keyword this is
    O.topk_indices / O.ndcg_at_k / O.mrr (tests/test_metrics_host.py); ``cut_short`` (top-k cut at k - 1), ``idcg_in_score_order``,
    ``mrr_last`` and the keywords of ``ranks_before`` plant a defect each."""
    b = len(off) - 1
    out = {k: (np.full((b, k), -1, np.int64), np.zeros(b, dtype), np.zeros(b, dtype)) for k in ks}
    disc = lambda r: (dtype(1) / np.log2(r.astype(dtype) + dtype(2))).astype(dtype)
    for i in range(b):
        s, y = scores[off[i]:off[i + 1]], labels[off[i]:off[i + 1]].astype(dtype)
        if s.size == 0:
            continue
        rank = kernel_ranks(s, **defect)
        lrank = rank if idcg_in_score_order else kernel_ranks(y)
        pos = rank[y > 0]
        for k in ks:
            top, ndcg, mrr = out[k]
            kk = k - 1 if cut_short else k
            inside, linside = rank < kk, lrank < kk
            top[i, rank[inside]] = np.nonzero(inside)[0]
            dcg = (y[inside] * disc(rank[inside]))[np.argsort(rank[inside], kind="stable")].sum(dtype=dtype)
            idcg = (y[linside] * disc(lrank[linside]))[np.argsort(lrank[linside], kind="stable")].sum(dtype=dtype)
            with np.errstate(invalid="ignore", divide="ignore"):
                ndcg[i] = dcg / idcg if y.sum() != 0 else 0
            if pos.size:
                mrr[i] = dtype(1) / dtype((pos.max() if mrr_last else pos.min()) + 1)
    return out


def oracle_rank(scores: np.ndarray, labels: np.ndarray, off: np.ndarray, k: int):
    """the oracle's (top-k lists with the -1 fill, nDCG [B], MRR [B]) in float64"""
    s, y, o = torch.from_numpy(scores), torch.from_numpy(labels), off.tolist()
    top = np.array([t + [-1] * (k - len(t)) for t in O.topk_indices(s, o, k)], np.int64).reshape(len(o) - 1, k)
    return top, O.ndcg_at_k(s, y, o, k)[1].numpy(), O.mrr(s, y, o)[1].numpy()


RANK_DEFECTS = {"ties_to_higher_index": dict(tie_high=True), "nan_last": dict(nan_last=True), "ge_for_gt": dict(ge=True),
                "cut_at_k_minus_1": dict(cut_short=True), "idcg_in_score_order": dict(idcg_in_score_order=True), "mrr_of_last_positive": dict(mrr_last=True)}


def rank_defect(name: str, scores, labels, off, ks):
    return rank_metrics(scores, labels, off, ks, **RANK_DEFECTS[name])


# ------------------------------------------------------------------------------------------------ AUC
def float_key(v: np.ndarray, flip=True) -> np.ndarray:
    """auc_split_kernel's ascending order-preserving u32 key of a float32 (``flip=False``: the defect without the flip of negatives)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg & flip, ~u, u ^ np.uint32(0x80000000)) if flip else (u ^ np.uint32(0x80000000))


def key_float(key: np.ndarray) -> np.ndarray:
    key = np.asarray(key, np.uint32)
    u = np.where((key & np.uint32(0x80000000)) != 0, key ^ np.uint32(0x80000000), ~key)
    return u.astype(np.uint32).view(np.float32)


def squashed(scores: np.ndarray, sigmoid_rule: bool, blind_to_one=False) -> np.ndarray:
    """torchmetrics' binary format step: any score outside [0, 1] (or NaN) sends all of them through the logistic function"""
    p = np.asarray(scores, np.float32)
    outside = int((~((p >= 0) & (p <= 1))).sum())
    if sigmoid_rule and outside > (1 if blind_to_one else 0):
        p = torch.from_numpy(p).sigmoid().numpy()
    return p


def mann_whitney(scores, labels, sigmoid_rule=True) -> Tuple[int, int, int]:
    """(2U, P, N), U = #(pos > neg) + #(pos == neg) / 2, in integers: the negatives sorted, every positive searched left and right"""
    v = squashed(scores, sigmoid_rule) + np.float32(0.0)
    is_pos = np.asarray(labels, np.float32) > 0.5
    pos, neg = v[is_pos], np.sort(v[~is_pos])
    return int(np.searchsorted(neg, pos, "left").sum() + np.searchsorted(neg, pos, "right").sum()), int(pos.size), int(neg.size)


def _lsd_sort(keys: np.ndarray, reverse_pass: Optional[int] = None) -> np.ndarray:
    for p in range(4):
        d = (keys >> np.uint32(8 * p)) & np.uint32(255)
        if p == reverse_pass:                                   # the scatter ranking its keys back to front inside a digit
            keys = keys[keys.size - 1 - np.argsort(d[::-1], kind="stable")]
        else:
            keys = keys[np.argsort(d, kind="stable")]
    return keys


def _bisect_count(neg: np.ndarray, pos: np.ndarray) -> int:
    """auc_count_kernel: lower and upper bound by bisection over ``neg`` as it is (sorted or not)"""
    total = 0
    for upper in (False, True):
        lo, hi = np.zeros(pos.size, np.int64), np.full(pos.size, neg.size, np.int64)
        while bool((lo < hi).any()):
            live = lo < hi
            mid = np.where(live, lo + ((hi - lo) >> 1), 0)
            probe = neg[np.minimum(mid, max(neg.size - 1, 0))] if neg.size else np.zeros(pos.size, np.uint32)
            right = (probe <= pos) if upper else (probe < pos)
            lo = np.where(live & right, mid + 1, lo)
            hi = np.where(live & ~right, mid, hi)
        total += int(lo.sum())
    return total


AUC_DEFECTS = ("ties_as_wins", "minus_zero_below_zero", "denormals_flushed", "format_rule_blind_to_one", "no_sign_flip", "third_pass_reversed",
               "last_tile_dropped")


def auc_defect(name: str, scores, labels, sigmoid_rule=True) -> Tuple[int, int, int]:
    p = squashed(scores, sigmoid_rule, blind_to_one=name == "format_rule_blind_to_one")
    v = p if name == "minus_zero_below_zero" else p + np.float32(0.0)
    if name == "denormals_flushed":                             # what a flush-to-zero build would make of `v += 0.0f`
        v = np.where(np.abs(v) < FLT_MIN, np.float32(0.0), v)
    is_pos = np.asarray(labels, np.float32) > 0.5
    key = float_key(v, flip=name != "no_sign_flip")
    pos, neg = key[is_pos], key[~is_pos]
    if name == "last_tile_dropped":
        neg = neg[:neg.size // RS_TILE * RS_TILE]
    neg = _lsd_sort(neg, reverse_pass=2 if name == "third_pass_reversed" else None)
    if name == "ties_as_wins":
        return 2 * int(np.searchsorted(neg, pos, "right").sum()), int(pos.size), int(neg.size)
    return _bisect_count(neg, pos), int(pos.size), int(neg.size)


class AucCase:
    """``exact``: the counts are the reference's integers; otherwise (continuous scores through the logistic function, where the device's
    expf and torch.sigmoid may split a tie differently) the project's |dAUC| < 1e-6 holds."""

    def __init__(self, name, scores, labels, sigmoid_rule, exact=True):
        self.name, self.sigmoid_rule, self.exact = name, sigmoid_rule, exact
        self.scores, self.labels = np.ascontiguousarray(scores, np.float32), np.ascontiguousarray(labels, np.float32)

    def __repr__(self):
        return self.name


def _mixed(rng, n_neg, n_pos, levels=97):
    y = np.zeros(n_neg + n_pos, np.float32)
    y[rng.permutation(n_neg + n_pos)[:n_pos]] = 1.0
    return (np.floor(rng.random(y.size) * levels) / levels).astype(np.float32), y


def auc_carry_case(n: int = 4096 * RS_TILE + RS_TILE + 1) -> AucCase:
    """(g) 4098 tiles: 256 * 4098 histogram entries are 257 scan segments, one more than rs_scan_segs_kernel scans in one trip"""
    rng = np.random.default_rng(77)
    return AucCase(f"g-carry-n{n}", rng.random(n, dtype=np.float32), (rng.random(n, dtype=np.float32) < 0.1).astype(np.float32), True)


@functools.lru_cache(maxsize=None)
def auc_cases() -> List[AucCase]:
    rng = np.random.default_rng(50)
    cases = []
    for big in (1, 4095, 4096, 4097, 8192, 8193):                                       # (a) class counts on the 4096-key tile edges
        for small in (1, 37):
            cases.append(AucCase(f"a-N{big}-P{small}", *_mixed(rng, big, small), True))
            if big != small:
                cases.append(AucCase(f"a-N{small}-P{big}", *_mixed(rng, small, big), True))
    n, p = 3 * RS_TILE + 5, RS_TILE + 3                                                  # (b) whole tiles own no key of one class
    s, _ = _mixed(rng, n - p, p)
    first = np.concatenate([np.ones(p, np.float32), np.zeros(n - p, np.float32)])
    cases += [AucCase("b-positives-first", s, first, True), AucCase("b-negatives-first", s, first[::-1].copy(), True)]
    n = 70001                                                                            # (c) raw: every byte of the key is live
    s = np.clip(rng.standard_normal(n) * 10.0 ** rng.uniform(-44, 38, n), -3e38, 3e38).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.float32)
    s[:10] = [INF, -INF, 0.0, -0.0, DENORM, -DENORM, FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN]
    y[:10] = [1, 0, 1, 0, 0, 1, 0, 1, 1, 0]
    s[10:20] = s[:10]
    s[10:12] = [1.0, -1.0]                          # one infinity of each sign only: the oracle subtracts neighbours, inf - inf is NaN
    y[10:20] = 1 - y[:10]
    s[100:400] = s[100]
    cases.append(AucCase("c-raw-wide", s, y, False))
    y = (rng.random(5000) < 0.4).astype(np.float32)                                      # (d) digit isolation, raw
    cases.append(AucCase("d-all-equal", np.full(5000, -3.25, np.float32), y, False))
    top = key_float((np.arange(256, dtype=np.uint32) << np.uint32(24)) | np.uint32(0x00345678))
    top = np.repeat(top[np.isfinite(top)], 20)
    cases.append(AucCase("d-top-byte", rng.permutation(top), (rng.random(top.size) < 0.4).astype(np.float32), False))
    two = key_float(np.array([0xC0123480, 0xC0123481], np.uint32))
    cases.append(AucCase("d-two-neighbours", two[rng.integers(0, 2, 5000)], y, False))
    low = np.repeat(key_float(np.uint32(0xC0123400) | np.arange(256, dtype=np.uint32)), 20)
    cases.append(AucCase("d-low-byte-256", rng.permutation(low), (rng.random(low.size) < 0.4).astype(np.float32), False))
    neg_low = np.repeat(key_float(np.uint32(0x3F123400) | np.arange(256, dtype=np.uint32)), 20)   # the same among negative floats
    cases.append(AucCase("d-low-byte-256-negative", rng.permutation(neg_low), (rng.random(neg_low.size) < 0.4).astype(np.float32), False))
    # (e) the format rule at its boundary.  Values at or under 1e-10 all become exactly 0.5 once squashed (exp(-x) rounds to 1), the
    # rest stay apart by more than any expf error and carry one class per value, every entry at 1.0 and above a positive: the squashed counts do not depend on
    # the logistic function's last bit, and they differ from the unsquashed ones
    tiny = np.array([0.0, -0.0, DENORM, 1e-40, FLT_MIN, 1e-30, 1e-20, 1e-10], np.float32)
    base = np.concatenate([np.tile(tiny, 40), np.tile(np.array([0.25, 0.5, 0.75], np.float32), 30), np.full(30, 1.0, np.float32)])
    y = (rng.random(base.size) < 0.5).astype(np.float32)
    y[base >= 1.0] = 1.0
    y[base == 0.5], y[(base == 0.25) | (base == 0.75)] = 1.0, 0.0      # one class per value: see the squashed grid below
    order = rng.permutation(base.size)
    base, y = base[order], y[order]
    spot = int(np.nonzero(base >= 1.0)[0][0])
    cases.append(AucCase("e-inside", base, y, True))
    for name, v in (("e-one-above-1", np.nextafter(np.float32(1), np.float32(2))), ("e-one-negative-denormal", -DENORM)):
        s = base.copy()
        s[spot] = v
        cases.append(AucCase(name, s, y, True))
    s, _ = _mixed(rng, 3000, 1000, levels=13)                                            # (f) label values around the 0.5 threshold
    lab = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1)), 2.0, -1.0, NAN, 0.0, 1.0], np.float32)[rng.integers(0, 7, 4000)]
    cases.append(AucCase("f-label-values", s, lab, True))
    # squashed and still exact: two infinities of each sign and +-FLT_MAX become exact 0 / 1 ties of both classes.  torch.sigmoid is
    # not a function of the value alone (an infinity in a SIMD group sends its neighbours down another path, one ulp apart), so every
    # finite value here carries one class — a split tie inside it changes nothing — and the grid stops at +-12, far from saturation
    s = rng.integers(-12, 13, 6000).astype(np.float32)
    y = ((s * 7) % 5 < 2).astype(np.float32)
    s[:600] = np.array([INF, -INF, FLT_MAX, -FLT_MAX], np.float32)[rng.integers(0, 4, 600)]
    y[:600] = (rng.random(600) < 0.4).astype(np.float32)
    order = rng.permutation(6000)
    cases.append(AucCase("h-squashed-grid-infinities", s[order], y[order], True))
    s = (4 * rng.standard_normal(50_000)).astype(np.float32)
    cases.append(AucCase("h-squashed-continuous", s, (rng.random(50_000) < 0.2).astype(np.float32), True, exact=False))
    return cases


# ------------------------------------------------------------------------------------------------ aspect metrics
ASPECT_CLASSES, ASPECT_K = (2, 4, 19, 63, 64), (1, 5, 10, 70)
ASPECT_C = (1, 2, 4, 5, 6, 9, 10, 11, 64, 69, 70, 71, 130, 33)
ASPECT_H = (1, 200, 3, 0, 17, 64, 65, 1, 200, 5, 2, 9, 30, 12)      # impression 3 has an empty history; impression 13 only class 0


@functools.lru_cache(maxsize=None)
def aspect_case(num_classes: int) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(60 + num_classes)
    co, ho = offsets(ASPECT_C), offsets(ASPECT_H)
    ca, ha = rng.integers(0, num_classes, co[-1]).astype(np.int32), rng.integers(0, num_classes, ho[-1]).astype(np.int32)
    for i, c in enumerate(ASPECT_C):                            # the highest class id in every row that has room, first in rank where k = 1
        if c >= 2:
            ca[co[i]] = ca[co[i] + c // 2] = num_classes - 1
    ha[ho[1]:ho[1] + 7] = num_classes - 1
    ca[co[13]:co[14]] = 0
    scores = rng.standard_normal(co[-1]).astype(np.float32)
    scores[co[:-1]] = 9.0                                       # the row's first candidate ranks first
    return {"scores": scores, "cand_aspect": ca, "hist_aspect": ha, "cand_off": co, "hist_off": ho}


def aspect_rows(top: np.ndarray, case, num_classes: int, divide_by_k=False, class_limit: Optional[int] = None):
    """(diversity [B], personalization [B]) from top-k lists with the -1 fill, in float64: entropy of the class distribution of the valid
    top entries over ln(num_classes), generalised Jaccard of the top-k and history class counts; 0 where the candidates' aspects sum to 0.
    ``divide_by_k`` and ``class_limit`` (classes >= the limit ignored) plant a defect each."""
    co, ho, ca, ha = case["cand_off"], case["hist_off"], case["cand_aspect"], case["hist_aspect"]
    b, k = top.shape
    div, pers = np.zeros(b), np.zeros(b)
    for i in range(b):
        a = ca[co[i]:co[i + 1]]
        if a.sum() == 0:
            continue
        idx = top[i][top[i] >= 0]
        pc = np.bincount(a[idx], minlength=num_classes).astype(np.float64)
        tc = np.bincount(ha[ho[i]:ho[i + 1]], minlength=num_classes).astype(np.float64)
        if class_limit is not None:
            pc[class_limit:], tc[class_limit:] = 0, 0
        p = pc / (k if divide_by_k else idx.size)
        nz = p > 0
        div[i] = -(p[nz] * np.log(p[nz])).sum() / np.log(num_classes)
        with np.errstate(invalid="ignore"):
            pers[i] = np.minimum(pc, tc).sum() / np.maximum(pc, tc).sum()
    return div, pers


def oracle_aspect(case, num_classes: int, k: int):
    s, ca = torch.from_numpy(case["scores"]), torch.from_numpy(case["cand_aspect"])
    co, ho = case["cand_off"].tolist(), case["hist_off"].tolist()
    return (O.diversity_at_k(s, ca, co, num_classes, k).numpy(),
            O.personalization_at_k(s, ca, torch.from_numpy(case["hist_aspect"]), co, ho, num_classes, k).numpy())


# ------------------------------------------------------------------------------------------------ evaluation loss
LOSS_SIZES = (1, 2, 63, 64, 65, 129, 300)
LOSS_SCALES = {"3": (0.0, 3.0), "700": (700.0, 0.2), "-50": (-50.0, 1.0)}
LOSS_TEMPERATURES = (0.36, 0.05)


def loss_rows(scores, labels, off, supcon: bool, temperature: float = 1.0, c_max: Optional[int] = None, dtype=torch.float64,
              pad_in_softmax=True) -> torch.Tensor:
    """Per-impression loss of CRModule.model_step in ``dtype``.  SupCon on the scores: -(1 / (n_pos + tiny)) sum_pos (v_j - logsumexp v),
    v = s / T over the real candidates.  Cross-entropy with probability targets over the dense row, zero-padded to ``c_max`` columns
    (default: the batch maximum — what the oracle does); ``pad_in_softmax=False`` plants the defect that leaves the padding out."""
    s, y = torch.as_tensor(scores).to(dtype), torch.as_tensor(labels).to(dtype)
    sizes = np.diff(off)
    width = int(sizes.max()) if c_max is None else int(c_max)
    out = []
    for i in range(len(off) - 1):
        si, yi = s[off[i]:off[i + 1]], y[off[i]:off[i + 1]]
        if supcon:
            v = si / temperature
            v = v - v.max()
            pos = (yi > 0.5).to(dtype)
            out.append(-((pos * (v - torch.logsumexp(v, 0))).sum() / (pos.sum() + torch.finfo(dtype).tiny)))
        else:
            row = torch.cat([si, si.new_zeros(width - si.numel())]) if pad_in_softmax else si
            out.append(-(yi * (si - torch.logsumexp(row, 0))).sum())
    return torch.stack(out)


def loss_reduce(per: torch.Tensor, labels, supcon: bool) -> torch.Tensor:
    """the batch value: mean (cross-entropy); mean of the per-impression losses > 0, 0 without a positive or a negative pair (SupCon)"""
    if not supcon:
        return per.mean()
    y = torch.as_tensor(labels)
    if not bool((y > 0.5).any()) or not bool((y <= 0.5).any()) or not bool((per > 0).any()):
        return per.sum() * 0
    return per[per > 0].mean()


class LossCase:
    def __init__(self, name, scores, labels, off, supcon, temperature, c_max, new):
        self.name, self.scores, self.labels, self.off = name, scores, labels, off
        self.supcon, self.temperature, self.c_max, self.new = supcon, temperature, c_max, new
        self._ref = {}

    def ref(self, dtype=torch.float64) -> Dict[str, torch.Tensor]:
        if dtype not in self._ref:
            per = loss_rows(self.scores, self.labels, self.off, self.supcon, self.temperature, self.c_max, dtype)
            self._ref[dtype] = {"per": per, "loss": loss_reduce(per, self.labels, self.supcon)}
        return self._ref[dtype]

    def bars(self) -> Dict[str, Dict[str, float]]:
        """{"per" / "loss": {"cpu_f32", "bar"}} relative to the largest entry: measured for the new regimes, 2e-5 (relative to
        max(1, largest entry): the project's rtol + atol) otherwise"""
        r64, r32 = self.ref(torch.float64), self.ref(torch.float32)
        out = {}
        for key in ("per", "loss"):
            cpu = loss_error(r32[key], r64[key])
            out[key] = {"cpu_f32": cpu, "bar": measured_bar(cpu) if self.new else LOSS_RTOL}
        return out

    def __repr__(self):
        return self.name


def loss_error(got, ref64) -> float:
    ref64 = torch.as_tensor(ref64).double().reshape(-1)
    err = float((torch.as_tensor(got).double().reshape(-1) - ref64).abs().max())
    return err / max(1.0, float(ref64.abs().max()))


def _loss_inputs(scale: str):
    """three groups of LOSS_SIZES: rows with one or two positives, rows without a positive, rows without a negative.  Drawn with the first
    salt at which every SupCon row loss is exactly 0 or at least 1e-3 at both temperatures: membership in the non-zero reducer is then no
    rounding matter (a condition on the reference side alone)."""
    centre, spread = LOSS_SCALES[scale]
    sizes = [c for _ in range(3) for c in LOSS_SIZES]
    off = offsets(sizes)
    for salt in range(64):
        rng = np.random.default_rng(7000 + 100 * salt + len(scale) + int(abs(float(scale))))
        scores = (centre + spread * rng.standard_normal(off[-1])).astype(np.float32)
        labels = np.zeros(off[-1], np.float32)
        for i, c in enumerate(sizes):
            row = labels[off[i]:off[i + 1]]
            if i // len(LOSS_SIZES) == 2:
                row[:] = 1.0
            elif i // len(LOSS_SIZES) == 0:
                row[rng.integers(0, c)] = 1.0
                if c >= 63:
                    row[rng.integers(0, c)] = 1.0
        per = torch.cat([loss_rows(scores, labels, off, True, t) for t in LOSS_TEMPERATURES]).abs()
        if bool(((per == 0) | (per >= 1e-3)).all()):
            return scores, labels, off
    raise AssertionError("no salt in 64 settles the loss inputs")


@functools.lru_cache(maxsize=None)
def loss_cases() -> List[LossCase]:
    cases = []
    for scale in LOSS_SCALES:
        scores, labels, off = _loss_inputs(scale)
        for t in LOSS_TEMPERATURES:
            new = scale == "700"                                 # mode 0 has no padding: -50 is a new regime in mode 1 only
            cases.append(LossCase(f"supcon-scale{scale}-T{t}" + ("-NEW" if new else ""), scores, labels, off, True, t, None, new))
        big = max(LOSS_SIZES)
        for c_max in (big, big + 1, 2 * big):
            new = scale != "3"                                   # at -50 every row shorter than c_max is padded, at every c_max
            cases.append(LossCase(f"ce-scale{scale}-cmax{c_max}" + ("-NEW" if new else ""), scores, labels, off, False, 1.0, c_max, new))
    return cases


# ------------------------------------------------------------------------------------------------ z-score fusion
ZSCORE_SIZES = (2, 3, 63, 64, 65, 128, 255, 256, 257, 300, 511, 513, 37, 40, 300, 2, 2)
ZSCORE_CONSTANT_ROWS = (13, 14)                                  # c = 40 (register path) and c = 300 (loop path): plane 0 constant
ZSCORE_WEIGHTS = ((-0.3, 0.2), (0.0, 0.7), (0.5, 0.0))
ZSCORE_PLANES = {"700+-40": ((700.0, 40.0), (-20.0, 3.0), (0.0, 0.5)), "777+-0.2-NEW": ((777.0, 0.2), (-20.0, 3.0), (0.0, 0.5))}


@functools.lru_cache(maxsize=None)
def zscore_case(name: str) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(80 + len(name))
    off = offsets(ZSCORE_SIZES)
    planes = np.stack([(m + sd * rng.standard_normal(off[-1])) for m, sd in ZSCORE_PLANES[name]]).astype(np.float32)
    for i in ZSCORE_CONSTANT_ROWS:                              # 777.125 * 300 and every partial sum of it are exact in float32: the mean
        planes[0, off[i]:off[i + 1]] = 777.125                  # is the value itself, the deviations are 0 and 0 / 0 is NaN in any order
    return {"planes": planes, "off": off}


def zscore_ref(case, weights, dtype=torch.float64) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fused ragged scores, the value of a padded slot per impression) by O.zscore on the dense zero-padded planes (one column wider than
    the longest row, so that every row has a padded slot), fused as EnsembleModule.forward does: z_0, then += w_k z_k, zero weights skipped"""
    off, planes = case["off"], torch.from_numpy(case["planes"]).to(dtype)
    sizes = np.diff(off)
    b, width = sizes.size, int(sizes.max()) + 1
    mask = torch.arange(width)[None, :] < torch.from_numpy(sizes)[:, None]
    fused = None
    for k, wk in enumerate((1.0,) + tuple(weights)):
        if k > 0 and wk == 0:
            continue
        dense = torch.zeros((b, width), dtype=dtype)
        dense[mask] = planes[k]
        z = O.zscore(dense, mask)
        fused = z if fused is None else fused + wk * z
    return fused[mask], fused[torch.arange(b), torch.from_numpy(sizes)]


def zscore_error(got, ref64, off) -> float:
    """largest |got - ref| over max(1, the row's largest finite |ref|), finite reference entries only; where the reference is not finite
    ``got`` must be the same NaN / infinity (inf returned otherwise).  ``off`` None: one value per row (the padded slot)."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    fin = np.isfinite(ref64)
    same = np.where(np.isnan(ref64), np.isnan(got), got == ref64)
    if not bool(same[~fin].all()) or not bool(np.isfinite(got[fin]).all()):
        return float("inf")
    worst = 0.0
    rows = [(i, i + 1) for i in range(ref64.size)] if off is None else list(zip(off[:-1], off[1:]))
    for a, b in rows:
        r, g, f = ref64[a:b], got[a:b], fin[a:b]
        if f.any():
            worst = max(worst, float(np.abs(g[f] - r[f]).max()) / max(1.0, float(np.abs(r[f]).max())))
    return worst
