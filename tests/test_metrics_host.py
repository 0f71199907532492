"""CPU checks of tests/metrics_ref.py: its references agree with the oracle, its inputs hold what the GPU cases rely on, and every
planted defect changes a quantity that tests/test_gpu_metrics.py asserts, on that test's own inputs — any difference for the exact
quantities (top-k lists, (2U, P, N)), at least 10 x the bar for the floats.  If a defect hides, the inputs are too weak.
Run with ``-s`` to see what each defect moved."""
import numpy as np
import pytest
import torch

import manner_oracle as O
import metrics_ref as M

CLEAR = 10.0


# ------------------------------------------------------------------------------------------------ ranking
def _ks(name):
    return M.FUSED_K if name == "fused" else M.RANK_K


def _rank_ref(name):
    case = M.rank_cases()[name]
    return case, {k: M.oracle_rank(case["scores"], case["labels"], case["off"], k) for k in _ks(name)}


RANK_REF = {}


def rank_ref(name):
    if name not in RANK_REF:                                     # computed once, shared, never modified
        RANK_REF[name] = _rank_ref(name)
    return RANK_REF[name]


def test_the_kernels_ranking_rule_orders_as_stable_descending_argsort():
    order = torch.argsort(torch.from_numpy(M.PROBE), descending=True, stable=True).tolist()
    assert order == M.PROBE_ORDER and np.argsort(M.kernel_ranks(M.PROBE)).tolist() == M.PROBE_ORDER
    for name in ("ragged", "single", "fused"):
        case = M.rank_cases()[name]
        off, s = case["off"], case["scores"]
        for i in range(len(off) - 1):
            row = s[off[i]:off[i + 1]]
            rank = M.kernel_ranks(row)
            want = torch.argsort(torch.from_numpy(row), descending=True, stable=True).numpy()
            assert sorted(rank.tolist()) == list(range(row.size)) and np.array_equal(np.argsort(rank), want), case["rows"][i]


@pytest.mark.parametrize("name", ["ragged", "single", "fused"])
def test_rank_restatement_is_the_oracle_and_float32_sits_under_its_bar(name):
    case, ref = rank_ref(name)
    r64 = M.rank_metrics(case["scores"], case["labels"], case["off"], _ks(name))
    r32 = M.rank_metrics(case["scores"], case["labels"], case["off"], _ks(name), dtype=np.float32)
    for k in _ks(name):
        top, ndcg, mrr = ref[k]
        assert np.array_equal(r64[k][0], top) and np.array_equal(r32[k][0], top)
        assert np.abs(r64[k][1] - ndcg).max() < 1e-14 and np.array_equal(r64[k][2], mrr)
        assert r32[k][1].dtype == np.float32
        new = np.array([M.rank_row_is_new(row, k) for row in case["rows"]])
        cpu = float(np.abs(r32[k][1] - ndcg)[new].max()) if new.any() else 0.0
        print(f"{name} k={k}: float32 CPU nDCG error, new regimes {cpu:.3e} (bar {M.measured_bar(cpu):.3e}), others "
              f"{float(np.abs(r32[k][1] - ndcg)[~new].max()) if (~new).any() else 0.0:.3e} (bar {M.NDCG_BAR})")
        assert cpu < 1e-5                                        # float32 arithmetic, not a different function
        assert np.abs(r32[k][2] - mrr).max() < M.MRR_BAR


def test_rank_inputs_hold_what_they_were_chosen_for():
    case = M.rank_cases()["ragged"]
    rows, off, s, y = case["rows"], case["off"], case["scores"], case["labels"]
    assert len(rows) % 4 != 0 and len(M.rank_cases()["single"]["rows"]) == 1
    assert {r[0] for r in M.rank_cases()["fused"]["rows"]} == set(M.FUSED_COUNTS) and len(M.rank_cases()["fused"]["rows"]) == 60
    assert {r[0] for r in rows} == set(M.RANK_COUNTS) and max(M.RANK_K) > 64 and 64 in M.RANK_K and 65 in M.RANK_K
    for fl in M.RANK_FLAVOURS:                                   # every flavour meets every label kind, every count too
        assert {r[2] for r in rows if r[1] == fl} == set(M.RANK_LABELS)
    for c in M.RANK_COUNTS:
        assert {r[2] for r in rows if r[0] == c} == set(M.RANK_LABELS)
    for i, (c, fl, kind) in enumerate(rows):
        row = s[off[i]:off[i + 1]]
        if fl == "tie_runs" and c >= 127:                        # a run of equal values longer than 64 that crosses a multiple of 64
            change = np.nonzero(np.diff(row))[0] + 1
            runs = np.diff(np.concatenate([[0], change, [c]]))
            assert runs.max() > 64 and all(p % 64 for p in change)
        if fl == "nan_mixed" and c:
            assert np.isnan(row[0]) and np.isnan(row[-1]) and (c < 3 or np.isfinite(row).any()) and np.isnan(row[::64]).all()
        if fl == "specials" and c >= 127:
            assert {v.tobytes() for v in row} == {v.tobytes() for v in M.SPECIALS}
        if kind == "graded" and c >= 63:
            assert set(y[off[i]:off[i + 1]]) == {0.0, 1.0, 2.0, 3.0}


@pytest.mark.parametrize("defect", sorted(M.RANK_DEFECTS))
def test_planted_ranking_defect_is_seen(defect):
    seen = {}
    for name in ("ragged", "single", "fused"):
        case, ref = rank_ref(name)
        bad = M.rank_defect(defect, case["scores"], case["labels"], case["off"], _ks(name))
        for k in _ks(name):
            top, ndcg, mrr = ref[k]
            seen[(name, k)] = {"topk_rows": int((bad[k][0] != top).any(1).sum()), "ndcg": float(np.abs(bad[k][1] - ndcg).max()) / M.NDCG_BAR,
                               "mrr": float(np.abs(bad[k][2] - mrr).max()) / M.MRR_BAR}
    print(defect, {k: v for k, v in seen.items() if k[0] == "ragged"})
    for name in ("ragged", "single", "fused"):                   # seen in every batch, at some k
        assert any(v["topk_rows"] > 0 or v["ndcg"] >= CLEAR * 100 or v["mrr"] >= CLEAR for kk, v in seen.items() if kk[0] == name), defect
    if defect not in ("idcg_in_score_order", "mrr_of_last_positive"):
        assert all(v["topk_rows"] > 0 for (name, k), v in seen.items() if name != "single" and k > 1), defect


# ------------------------------------------------------------------------------------------------ AUC
AUC_CASES = M.auc_cases()


@pytest.mark.parametrize("case", AUC_CASES, ids=[c.name for c in AUC_CASES])
def test_mann_whitney_count_is_the_oracles_integers(case):
    with np.errstate(all="ignore"):
        want, cnt = O.binary_auroc(torch.from_numpy(case.scores), torch.from_numpy(case.labels), sigmoid_rule=case.sigmoid_rule)
    got = M.mann_whitney(case.scores, case.labels, case.sigmoid_rule)
    assert got == cnt and cnt[1] > 0 and cnt[2] > 0
    assert got[0] / (2.0 * got[1] * got[2]) == want
    perm = np.random.default_rng(3).permutation(case.scores.size)
    assert M.mann_whitney(case.scores[perm], case.labels[perm], case.sigmoid_rule) == got
    assert M.auc_defect("none", case.scores, case.labels, case.sigmoid_rule) == got      # the radix-sort emulation without a defect


def test_mann_whitney_count_on_a_small_carry_case():
    case = M.auc_carry_case(200_000)
    _, cnt = O.binary_auroc(torch.from_numpy(case.scores), torch.from_numpy(case.labels))
    assert M.mann_whitney(case.scores, case.labels) == cnt
    n = 4096 * M.RS_TILE + M.RS_TILE + 1                         # the full case: 4098 tiles, 257 scan segments of 4096 entries
    tiles = -(-n // M.RS_TILE)
    assert tiles == 4098 and -(-256 * tiles // 4096) == 257 and n == 16_777_216 + 4096 + 1


def test_auc_inputs_hold_what_they_were_chosen_for():
    by = {c.name: c for c in AUC_CASES}
    for big in (1, 4095, 4096, 4097, 8192, 8193):
        for small in (1, 37):
            assert M.mann_whitney(by[f"a-N{big}-P{small}"].scores, by[f"a-N{big}-P{small}"].labels)[1:] == (small, big)
            assert M.mann_whitney(by[f"a-N{small}-P{big}"].scores, by[f"a-N{small}-P{big}"].labels)[1:] == (big, small)
    for name in ("b-positives-first", "b-negatives-first"):      # a tile of positives only and two tiles of negatives only
        pos = by[name].labels > 0.5
        tiles = [pos[i:i + M.RS_TILE] for i in range(0, pos.size, M.RS_TILE)]
        assert any(t.all() for t in tiles) and sum(1 for t in tiles if not t.any()) >= 2 and pos.size == 3 * 4096 + 5
    c = by["c-raw-wide"]
    keys = M.float_key(c.scores[c.labels <= 0.5] + np.float32(0))
    for p in range(4):                                           # every pass of the sort over the negatives sees all 256 digits
        assert np.unique((keys >> np.uint32(8 * p)) & np.uint32(255)).size == 256, p
    assert np.isinf(c.scores).sum() == 2 and (c.scores < 0).sum() > 30000 and not np.isnan(c.scores).any()
    denormal = (np.abs(c.scores) < M.FLT_MIN) & (c.scores != 0)
    assert denormal.sum() > 500 and np.unique(c.scores, return_counts=True)[1].max() >= 300
    for name, byte in (("d-top-byte", 3), ("d-low-byte-256", 0), ("d-low-byte-256-negative", 0), ("d-two-neighbours", 0)):
        keys = np.unique(M.float_key(by[name].scores))
        diff = np.bitwise_or.reduce(keys ^ keys[0])
        assert diff & ~np.uint32(255 << (8 * byte)) == 0 and keys.size >= {"d-top-byte": 250, "d-two-neighbours": 2}.get(name, 256), name
    assert (by["d-low-byte-256-negative"].scores < 0).all() and np.isfinite(by["d-top-byte"].scores).all()
    u, p, n = M.mann_whitney(by["d-all-equal"].scores, by["d-all-equal"].labels, False)
    assert u == p * n
    inside, above, below = by["e-inside"], by["e-one-above-1"], by["e-one-negative-denormal"]
    for v in (np.float32(0.0), np.float32(-0.0), np.float32(1.0)):
        assert any(x.tobytes() == v.tobytes() for x in inside.scores)
    assert ((inside.scores >= 0) & (inside.scores <= 1)).all()
    assert (above.scores > 1).sum() == 1 and (below.scores < 0).sum() == 1 and below.scores.min() == -M.DENORM
    raw = M.mann_whitney(inside.scores, inside.labels, False)
    assert M.mann_whitney(inside.scores, inside.labels, True) == raw
    for case in (above, below):                                  # the squashed counts differ from the unsquashed: the branch shows in them
        assert M.mann_whitney(case.scores, case.labels, True) != M.mann_whitney(case.scores, case.labels, False)
    # and they do not hang on the last bit of the logistic function: a float64 sigmoid rounded to float32 gives the same counts
    for case in (above, below, by["h-squashed-grid-infinities"]):
        with np.errstate(over="ignore"):
            alt = (1.0 / (1.0 + np.exp(-case.scores.astype(np.float64)))).astype(np.float32)
        assert M.mann_whitney(alt, case.labels, False) == M.mann_whitney(case.scores, case.labels, True), case
    assert np.isinf(by["h-squashed-grid-infinities"].scores).sum() > 200
    lab = by["f-label-values"].labels
    for v in (0.5, np.nextafter(np.float32(0.5), np.float32(1)), 2.0, -1.0):
        assert (lab == np.float32(v)).any()
    assert np.isnan(lab).any()


@pytest.mark.parametrize("defect", M.AUC_DEFECTS)
def test_planted_auc_defect_is_seen(defect):
    seen = [c.name for c in AUC_CASES if c.exact and M.auc_defect(defect, c.scores, c.labels, c.sigmoid_rule) != M.mann_whitney(c.scores, c.labels, c.sigmoid_rule)]
    print(defect, "changes the counts of", seen)
    assert seen, defect
    expect = {"minus_zero_below_zero": "e-inside", "denormals_flushed": "e-inside", "format_rule_blind_to_one": "e-one-negative-denormal", "no_sign_flip": "c-raw-wide",
              "third_pass_reversed": "c-raw-wide", "last_tile_dropped": "a-N4097-P37", "ties_as_wins": "d-all-equal"}[defect]
    assert expect in seen, (defect, expect)


# ------------------------------------------------------------------------------------------------ aspect metrics
def _aspect_tops(case, k):
    s, off = torch.from_numpy(case["scores"]), case["cand_off"].tolist()
    return np.array([t + [-1] * (k - len(t)) for t in O.topk_indices(s, off, k)], np.int64)


@pytest.mark.parametrize("num_classes", M.ASPECT_CLASSES)
def test_aspect_restatement_is_the_oracle_and_defects_are_seen(num_classes):
    case = M.aspect_case(num_classes)
    ca, co, ho = case["cand_aspect"], case["cand_off"], case["hist_off"]
    assert ca.max() == num_classes - 1 and case["hist_aspect"].max() == num_classes - 1
    assert 0 in np.diff(ho) and {1, 200} <= set(np.diff(ho)) and ca[co[13]:co[14]].sum() == 0
    assert np.diff(co).min() == 1 and np.diff(co).max() == 130
    worst = {"divide_by_k": 0.0, "class_limit": 0.0}
    for k in M.ASPECT_K:
        top = _aspect_tops(case, k)
        assert k != 70 or ((top == -1).any(1).sum() >= 10 and (top >= 0).all(1).sum() >= 3)       # c < k occurs, c >= k too
        div, pers = M.aspect_rows(top, case, num_classes)
        odiv, opers = M.oracle_aspect(case, num_classes, k)
        assert np.abs(div - odiv).max() < M.DIV_BAR / CLEAR and np.abs(pers - opers).max() < M.PERS_BAR / CLEAR
        assert div[13] == 0 and pers[13] == 0 and pers[3] == 0 and div[3] > 0 or k == 1
        bad = M.aspect_rows(top, case, num_classes, divide_by_k=True)
        worst["divide_by_k"] = max(worst["divide_by_k"], np.abs(bad[0] - div).max() / M.DIV_BAR)
        if num_classes == 64:
            bad = M.aspect_rows(top, case, num_classes, class_limit=63)
            worst["class_limit"] = max(worst["class_limit"], min(np.nanmax(np.abs(bad[0] - div)) / M.DIV_BAR, np.nanmax(np.abs(bad[1] - pers)) / M.PERS_BAR))
    print(num_classes, worst)
    assert worst["divide_by_k"] >= CLEAR and (num_classes != 64 or worst["class_limit"] >= CLEAR)


# ------------------------------------------------------------------------------------------------ loss
LOSS_CASES = M.loss_cases()


@pytest.mark.parametrize("case", LOSS_CASES, ids=[c.name for c in LOSS_CASES])
def test_loss_restatement_is_the_oracle_and_float32_sits_under_its_bar(case):
    r64, r32, bars = case.ref(torch.float64), case.ref(torch.float32), case.bars()
    sizes = np.diff(case.off)
    assert set(sizes) == set(M.LOSS_SIZES) and len(sizes) % 4 != 0
    rows = [case.labels[a:b] for a, b in zip(case.off[:-1], case.off[1:])]
    assert any(r.sum() == 0 for r in rows) and any(r.size > 1 and r.min() == 1 for r in rows)
    if case.supcon or case.c_max == int(sizes.max()):            # the oracle pads to the batch maximum only
        loss, per = O.model_step_loss(torch.from_numpy(case.scores).double(), torch.from_numpy(case.labels).double(), case.off.tolist(),
                                      case.supcon, temperature=case.temperature)
        assert M.loss_error(r64["per"], per) < 1e-12 and M.loss_error(r64["loss"], loss) < 1e-12
    for key in ("per", "loss"):
        assert torch.isfinite(r64[key]).all() and r32[key].dtype == torch.float32
        err = M.loss_error(r32[key], r64[key])
        print(f"{case} {key}: cpu f32 {err:.3e}  bar {bars[key]['bar']:.3e}")
        assert err <= bars[key]["bar"] and err < 1e-3
    if not case.supcon:                                          # the planted defect: padded zeros left out of the softmax
        bad = M.loss_rows(case.scores, case.labels, case.off, False, c_max=case.c_max, pad_in_softmax=False)
        excess = M.loss_error(bad, r64["per"]) / bars["per"]["bar"]
        print(f"{case}: padding left out / bar = {excess:.3e}")
        assert excess >= CLEAR or "scale700" in case.name        # next to scores of 700 a padded zero weighs e^-700: only 3 and -50 see it
        assert excess >= CLEAR or excess == 0


def test_loss_cases_cover_the_listed_regimes():
    names = {c.name for c in LOSS_CASES}
    assert len(LOSS_CASES) == 3 * (2 + 3)
    for scale in ("3", "700", "-50"):
        for c_max in (300, 301, 600):
            assert any(n.startswith(f"ce-scale{scale}-cmax{c_max}") for n in names)
        for t in (0.36, 0.05):
            assert any(n.startswith(f"supcon-scale{scale}-T{t}") for n in names)
    far = next(c for c in LOSS_CASES if c.name.startswith("ce-scale-50-cmax600"))
    assert far.scores.max() < -40                               # every real score far below the padded zeros: the row maximum is the padding's 0


# ------------------------------------------------------------------------------------------------ z-score
@pytest.mark.parametrize("name", sorted(M.ZSCORE_PLANES))
def test_zscore_reference_and_its_float32_evaluation(name):
    case = M.zscore_case(name)
    off, planes = case["off"], case["planes"]
    sizes = np.diff(off)
    assert [int(sizes[i]) for i in M.ZSCORE_CONSTANT_ROWS] == [40, 300] and (sizes == 2).sum() >= 3
    for w in M.ZSCORE_WEIGHTS:
        f64, p64 = M.zscore_ref(case, w)
        f32, p32 = M.zscore_ref(case, w, torch.float32)
        assert f32.dtype == torch.float32
        for i in range(sizes.size):                              # the float64 evaluation of the older test, row by row
            a, b = off[i], off[i + 1]
            want, wpad = np.zeros(b - a), 0.0
            for k, wk in enumerate([1.0] + list(w)):
                if k > 0 and wk == 0.0:
                    continue
                x = planes[k, a:b].astype(np.float64)
                with np.errstate(invalid="ignore", divide="ignore"):
                    want += wk * (x - x.mean()) / x.std(ddof=1)
                    wpad += wk * (0.0 - x.mean()) / x.std(ddof=1)
            const = i in M.ZSCORE_CONSTANT_ROWS
            assert torch.isnan(f64[a:b]).all() == const and torch.isnan(f32[a:b]).all() == const
            if const:
                assert float(p64[i]) == -np.inf and float(p32[i]) == -np.inf
            else:
                assert np.abs(f64[a:b].numpy() - want).max() < 1e-9 * max(1.0, np.abs(want).max()) and abs(float(p64[i]) - wpad) < 1e-9 * abs(wpad)
        e, ep = M.zscore_error(f32, f64, off), M.zscore_error(p32, p64, None)
        print(f"{name} w={w}: cpu f32 fused {e:.3e} pad {ep:.3e}")
        assert e < (1e-2 if "NEW" in name else M.ZSCORE_REL) and np.isfinite(ep)
