"""The evaluation metrics on the device against tests/metrics_ref.py and the oracle: ranking / nDCG@k / MRR (rank_ndcg_kernel and the
one-launch score_fuse_rank_kernel, both of its branches), the global AUC (metrics.hip: split, four radix passes, the two-level scan
with its carry loop, the bisection count), aspect diversity / personalization, the val/test loss and the z-score fusion — at ties, NaN,
infinities, signed zeros, denormals, the 64-lane stride, k > 64, the 512- and 320-candidate thresholds and the 4096-key tile edges.

Top-k lists and the AUC's integers (2U, P, N) are exact.  Floats keep the project's bars where older tests cover the inputs in kind
and the MEASURED bar (8 x the float32 CPU evaluation's error against float64, floored at 2^-25) in the regimes new here; every float
test prints its error next to the CPU figure and the bar and records them with ``measured``
(profiles/metrics/measured_tolerances.json is that record from an MI355X).  What each input is for, and that the bars see the defects
they were chosen for: tests/test_metrics_host.py."""
import time

import numpy as np
import pytest
import torch

import manner_oracle as O
import metrics_ref as M
from manner_amd import hip, hotpath

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t.to(dtype) if dtype is not None else t).to(DEV)


_RANK_REF = {}


def _rank_ref(name, k):
    """the oracle's (top-k, nDCG, MRR) of a rank case and the float32 CPU nDCG of the restatement: computed once, shared, never modified"""
    if (name, k) not in _RANK_REF:
        case = M.rank_cases()[name]
        r32 = M.rank_metrics(case["scores"], case["labels"], case["off"], M.RANK_K, dtype=np.float32)
        for kk in M.RANK_K:
            _RANK_REF[(name, kk)] = M.oracle_rank(case["scores"], case["labels"], case["off"], kk) + (r32[kk][1],)
    return _RANK_REF[(name, k)]


def _hold_rank(tag, rows, k, got, ref, measured):
    """top-k exact; nDCG 1e-6 on the rows older tests cover in kind, the measured bar on the new regimes; MRR 1e-7"""
    top, ndcg, mrr = (t.cpu().numpy() for t in got)
    rtop, rndcg, rmrr, ndcg32 = ref
    assert np.array_equal(top.astype(np.int64), rtop), (tag, k, np.nonzero((top != rtop).any(1))[0][:8])
    new = np.array([M.rank_row_is_new(row, k) for row in rows])
    err = np.abs(ndcg.astype(np.float64) - rndcg)
    cpu = float(np.abs(ndcg32 - rndcg)[new].max()) if new.any() else 0.0
    e_new, e_old, e_mrr = (float(err[new].max()) if new.any() else 0.0), (float(err[~new].max()) if (~new).any() else 0.0), float(np.abs(mrr - rmrr).max())
    print(f"{tag} k={k}: nDCG error {e_old:.3e} (bar {M.NDCG_BAR}); new regimes {e_new:.3e}  cpu f32 {cpu:.3e}  bar {M.measured_bar(cpu):.3e}; "
          f"MRR error {e_mrr:.3e} (bar {M.MRR_BAR})")
    measured(**{f"{tag}_k{k}_ndcg_err": e_old, f"{tag}_k{k}_ndcg_bar": M.NDCG_BAR, f"{tag}_k{k}_ndcg_new_err": e_new, f"{tag}_k{k}_ndcg_new_cpu_f32": cpu,
                f"{tag}_k{k}_ndcg_new_bar": M.measured_bar(cpu), f"{tag}_k{k}_mrr_err": e_mrr, f"{tag}_k{k}_mrr_bar": M.MRR_BAR})
    assert np.isfinite(ndcg).all() and e_old < M.NDCG_BAR and e_new <= M.measured_bar(cpu) and e_mrr < M.MRR_BAR, (tag, k)


# ------------------------------------------------------------------------------------------------ ranking
@pytest.mark.parametrize("k", M.RANK_K)
@pytest.mark.parametrize("name", ["ragged", "single"])
def test_rank_ndcg_at_ties_special_values_and_both_staging_branches(name, k, measured):
    case = M.rank_cases()[name]
    got = hip.rank_ndcg(_cuda(case["scores"]), _cuda(case["labels"]), _cuda(case["off"]), k, with_mrr=True)
    _hold_rank(name, case["rows"], k, got, _rank_ref(name, k), measured)
    only_top, none = hip.rank_ndcg(_cuda(case["scores"]), None, _cuda(case["off"]), k)
    assert none is None and torch.equal(only_top, got[0])


@pytest.mark.parametrize("d", [768, 1024])
def test_fused_ranking_on_injected_scores(d, measured):
    """score_fuse_rank_kernel's in-LDS ranking (c <= 320) and its scratch branch on chosen score values: table row r = [v_r, 0, ...], every
    history the single row [1, 0, ...], K = 1 — the score of candidate r is v_r bit for bit (-0 becomes +0)"""
    fused_case = M.rank_cases()["fused"]
    v, off, rows = fused_case["scores"], fused_case["off"], fused_case["rows"]
    n, b = v.size, len(rows)
    table = torch.zeros((n + 1, d), device=DEV)
    table[:n, 0] = _cuda(v)
    table[n, 0] = 1.0
    hist_idx, hist_off = torch.full((b,), n, dtype=torch.int32, device=DEV), torch.arange(b + 1, dtype=torch.int64, device=DEV)
    cand_idx, cand_off, labels = torch.arange(n, dtype=torch.int32, device=DEV), _cuda(off), _cuda(fused_case["labels"])
    injected = hip.score_late_fusion(table, hist_idx, hist_off, cand_idx, cand_off)
    hip.check_status(DEV)
    want = torch.from_numpy(v + np.float32(0.0))                 # the precondition of everything below
    inj = injected.cpu()
    assert torch.equal(torch.isnan(inj), torch.isnan(want))
    assert torch.equal(inj[~torch.isnan(want)].view(torch.int32), want[~torch.isnan(want)].view(torch.int32))
    s_np = inj.numpy()
    for k in M.FUSED_K:
        res = hip.score_fuse_rank([table], [], hist_idx, hist_off, cand_idx, cand_off, labels=labels, k=k)
        hip.check_status(DEV)
        top, ndcg, mrr = hip.rank_ndcg(injected, labels, cand_off, k, with_mrr=True)
        assert torch.equal(res["scores"].view(torch.int32), injected.view(torch.int32))
        assert torch.equal(res["topk"], top) and torch.equal(res["mrr"], mrr)
        assert torch.equal(res["ndcg"].view(torch.int32), ndcg.view(torch.int32))
        r32 = M.rank_metrics(s_np, fused_case["labels"], off, (k,), dtype=np.float32)[k][1]
        ref = M.oracle_rank(s_np, fused_case["labels"], off, k) + (r32,)
        _hold_rank(f"fused_D{d}", rows, k, (res["topk"], res["ndcg"], res["mrr"]), ref, measured)


# ------------------------------------------------------------------------------------------------ AUC
AUC_CASES = M.auc_cases()


def _auc(scores, labels, rule):
    got, counts = hip.auc(_cuda(scores), _cuda(labels), sigmoid_rule=rule, return_counts=True)
    return float(got), tuple(int(v) for v in counts.tolist())


@pytest.mark.parametrize("case", AUC_CASES, ids=[c.name for c in AUC_CASES])
def test_auc_counts_are_the_reference_integers(case):
    want = M.mann_whitney(case.scores, case.labels, case.sigmoid_rule)
    got, counts = _auc(case.scores, case.labels, case.sigmoid_rule)
    perm = np.random.default_rng(5).permutation(case.scores.size)
    got_p, counts_p = _auc(case.scores[perm], case.labels[perm], case.sigmoid_rule)
    print(f"{case}: (2U, P, N) = {counts}, reference {want}")
    assert counts_p == counts and got_p == got                   # the order of the pairs changes nothing
    assert got == counts[0] / (2.0 * counts[1] * counts[2])
    if case.exact:
        assert counts == want
    else:                                                        # device expf against torch.sigmoid may split a tie
        assert counts[1:] == want[1:] and abs(got - want[0] / (2.0 * want[1] * want[2])) < 1e-6
    if case.name == "e-one-negative-denormal":                   # -1e-45 is outside [0, 1]: the counts are the squashed ones
        assert counts != M.mann_whitney(case.scores, case.labels, False)


def test_auc_past_one_trip_of_the_segment_scan(measured):
    """n = 16 777 216 + 4096 + 1: 4098 tiles, 257 scan segments — rs_scan_segs_kernel's carry loop runs a second trip"""
    t0 = time.time()
    case = M.auc_carry_case()
    want = M.mann_whitney(case.scores, case.labels)
    t1 = time.time()
    got, counts = _auc(case.scores, case.labels, True)
    t2 = time.time()
    print(f"{case}: inputs and reference {t1 - t0:.1f} s, device (upload included) {t2 - t1:.1f} s; (2U, P, N) = {counts}")
    measured(reference_seconds=t1 - t0, device_seconds=t2 - t1, wall_seconds=t2 - t0)
    assert counts == want and got == want[0] / (2.0 * want[1] * want[2])


# ------------------------------------------------------------------------------------------------ aspect metrics
@pytest.mark.parametrize("k", M.ASPECT_K)
@pytest.mark.parametrize("num_classes", M.ASPECT_CLASSES)
def test_aspect_metrics_from_the_top_k_of_rank_ndcg(num_classes, k, measured):
    case = M.aspect_case(num_classes)
    co, ho = _cuda(case["cand_off"]), _cuda(case["hist_off"])
    topk, _ = hip.rank_ndcg(_cuda(case["scores"]), None, co, k)
    want_top = np.array([t + [-1] * (k - len(t)) for t in O.topk_indices(torch.from_numpy(case["scores"]), case["cand_off"].tolist(), k)])
    assert np.array_equal(topk.cpu().numpy(), want_top)
    div, pers = hip.aspect_metrics(topk, _cuda(case["cand_aspect"]), co, num_classes, _cuda(case["hist_aspect"]), ho)
    rdiv, rpers = M.oracle_aspect(case, num_classes, k)
    e_div, e_pers = float(np.abs(div.cpu().numpy() - rdiv).max()), float(np.abs(pers.cpu().numpy() - rpers).max())
    print(f"classes {num_classes} k={k}: diversity error {e_div:.3e} (bar {M.DIV_BAR}), personalization error {e_pers:.3e} (bar {M.PERS_BAR})")
    measured(div_err=e_div, div_bar=M.DIV_BAR, pers_err=e_pers, pers_bar=M.PERS_BAR)
    assert e_div < M.DIV_BAR and e_pers < M.PERS_BAR
    assert div[13].item() == 0.0 and pers[13].item() == 0.0 and pers[3].item() == 0.0     # aspects all 0; an empty history
    only_div, none = hip.aspect_metrics(topk, _cuda(case["cand_aspect"]), co, num_classes)
    assert none is None and torch.equal(only_div, div)


# ------------------------------------------------------------------------------------------------ evaluation loss
LOSS_CASES = M.loss_cases()


@pytest.mark.parametrize("case", LOSS_CASES, ids=[c.name for c in LOSS_CASES])
def test_eval_loss_both_modes(case, measured):
    ref, bars = case.ref(torch.float64), case.bars()
    kw = dict(supcon=case.supcon, temperature=case.temperature, c_max=case.c_max)
    s, y, off = _cuda(case.scores), _cuda(case.labels), _cuda(case.off)
    got = {"per": hip.eval_loss(s, y, off, reduce=False, **kw).cpu(), "loss": hip.eval_loss(s, y, off, reduce=True, **kw).cpu()}
    rec, bad = {}, {}
    for key in ("per", "loss"):
        assert torch.isfinite(got[key]).all()
        err = M.loss_error(got[key], ref[key])
        print(f"{case} {key}: error {err:.3e}  cpu f32 {bars[key]['cpu_f32']:.3e}  bar {bars[key]['bar']:.3e}")
        rec.update({f"{key}_err": err, f"{key}_cpu_f32": bars[key]["cpu_f32"], f"{key}_bar": bars[key]["bar"]})
        if not err <= bars[key]["bar"]:
            bad[key] = (err, bars[key]["bar"])
    measured(**rec)
    assert not bad, (case, bad)
    if case.supcon:                                              # the non-zero reducer's members are the reference's
        assert torch.equal(got["per"] > 0, ref["per"] > 0)


# ------------------------------------------------------------------------------------------------ z-score fusion
@pytest.mark.parametrize("weights", M.ZSCORE_WEIGHTS, ids=str)
@pytest.mark.parametrize("name", sorted(M.ZSCORE_PLANES))
def test_zscore_fuse_near_tied_constant_and_two_candidate_rows(name, weights, measured):
    case = M.zscore_case(name)
    off = case["off"]
    fused, pad = hip.zscore_fuse(_cuda(case["planes"]), list(weights), _cuda(off), with_pad_value=True)
    only = hip.zscore_fuse(_cuda(case["planes"]), list(weights), _cuda(off))
    assert torch.equal(only.view(torch.int32), fused.view(torch.int32))
    f64, p64 = M.zscore_ref(case, weights)
    f32, p32 = M.zscore_ref(case, weights, torch.float32)
    new = "NEW" in name
    rec, bad = {}, {}
    for key, got, r64, r32, o in (("fused", fused, f64, f32, off), ("pad", pad, p64, p32, None)):
        err, cpu = M.zscore_error(got.cpu().numpy(), r64.numpy(), o), M.zscore_error(r32.numpy(), r64.numpy(), o)
        bar = M.measured_bar(cpu) if new else M.ZSCORE_REL
        print(f"{name} w={weights} {key}: error {err:.3e}  cpu f32 {cpu:.3e}  bar {bar:.3e}")
        rec.update({f"{key}_err": err, f"{key}_cpu_f32": cpu, f"{key}_bar": bar})
        if not err <= bar:                                       # inf: a NaN or an infinity where the reference has none, or the reverse
            bad[key] = (err, bar)
    measured(**rec)
    assert not bad, (name, weights, bad)
    z = fused.cpu()
    for i in M.ZSCORE_CONSTANT_ROWS:                             # std 0: NaN exactly where O.zscore gives NaN ...
        assert torch.isnan(z[off[i]:off[i + 1]]).all() and torch.isnan(f64[off[i]:off[i + 1]]).all()
    assert torch.equal(torch.isnan(z), torch.isnan(f64))
    topk, _ = hip.rank_ndcg(fused, None, _cuda(off), 10)         # ... and an all-NaN row ranks in index order
    want = np.array([t + [-1] * (10 - len(t)) for t in O.topk_indices(z, off.tolist(), 10)])
    assert np.array_equal(topk.cpu().numpy(), want)
    for i in M.ZSCORE_CONSTANT_ROWS:
        assert topk[i].tolist() == list(range(10))


# ------------------------------------------------------------------------------------------------ both paths through hotpath
def _epoch_want(scores, labels, co, ho, ccat, csen, hcat, hsen, with_auc):
    ts, tl = torch.from_numpy(scores), torch.from_numpy(labels)
    want = {"test/mrr": O.mrr(ts, tl, co.tolist())[0]}
    if with_auc:
        want["test/auc"] = O.binary_auroc(ts, tl)[0]
    for k in (5, 10):
        want[f"test/ndcg@{k}"] = O.ndcg_at_k(ts, tl, co.tolist(), k)[0]
        for name, cc, hh, ncls in (("categ", ccat, hcat, 64), ("sent", csen, hsen, 4)):
            want[f"test/{name}_div@{k}"] = float(O.diversity_at_k(ts, torch.from_numpy(cc), co.tolist(), ncls, k).mean())
            want[f"test/{name}_pers@{k}"] = float(O.personalization_at_k(ts, torch.from_numpy(cc), torch.from_numpy(hh), co.tolist(), ho.tolist(),
                                                                         ncls, k).mean())
    return want


def test_epoch_end_metrics_over_the_rank_cases(measured):
    """one pass of hotpath.epoch_end_metrics over the ragged rank case with 64 category classes, against the oracle calls of
    test_epoch_metrics_match_oracle.  NaN scores in the AUC are the one documented divergence (hip.auc): its key is held on the
    impressions without a NaN, every other key on all of them."""
    case = M.rank_cases()["ragged"]
    rng = np.random.default_rng(95)
    scores, labels, co = case["scores"], case["labels"], case["off"]
    h = rng.integers(1, 50, len(co) - 1)
    ho = M.offsets(h)
    ccat, csen = rng.integers(1, 64, co[-1]), rng.integers(0, 4, co[-1])
    hcat, hsen = rng.integers(1, 64, ho[-1]), rng.integers(0, 4, ho[-1])
    ccat[rng.integers(0, co[-1], 200)] = 63
    keep = np.array([not np.isnan(scores[a:b]).any() for a, b in zip(co[:-1], co[1:])])
    cmask, hmask = np.repeat(keep, np.diff(co)), np.repeat(keep, h)
    for tag, rows, cm, hm in (("all", np.ones_like(keep), np.ones_like(cmask), np.ones_like(hmask)), ("nan_free", keep, cmask, hmask)):
        s, y, c_off, h_off = scores[cm], labels[cm], M.offsets(np.diff(co)[rows]), M.offsets(h[rows])
        got = hotpath.epoch_end_metrics(_cuda(s), _cuda(y), _cuda(c_off), cand_categories=_cuda(ccat[cm]), cand_sentiments=_cuda(csen[cm]),
                                        hist_categories=_cuda(hcat[hm]), hist_sentiments=_cuda(hsen[hm]), hist_off=_cuda(h_off), num_categ_classes=64)
        want = _epoch_want(s, y, c_off, h_off, ccat[cm], csen[cm], hcat[hm], hsen[hm], with_auc=tag == "nan_free")
        assert set(got) == set(want) | {"test/auc"}
        for key, v in want.items():
            print(f"{tag} {key}: {float(got[key]):.7f} oracle {v:.7f}")
            measured(**{f"{tag}_{key}_err": abs(float(got[key]) - v)})
            assert abs(float(got[key]) - v) < 2e-5, (tag, key, float(got[key]), v)
