"""CPU checks of tests/side_ops_ref.py: the restatements, the two bars, and that each bar sees the defect its shapes were chosen
for.  One planted defect per kernel loop (a dropped second trip, a dropped tail, a stale restage, a neighbouring dispatch case);
each must exceed its bar at least 10-fold on the inputs tests/test_gpu_side_ops.py uses — if one hides, the inputs are too weak.
Run with ``-s`` to see the ratios."""
import numpy as np
import pytest
import torch

import side_ops_ref as R

CLEAR = 10.0


def _ids(cases):
    return [c.name for c in cases]


MEASURED, DERIVED = R.all_measured_cases(), R.all_derived_cases()


@pytest.mark.parametrize("case", MEASURED, ids=_ids(MEASURED))
def test_float32_cpu_evaluation_sits_under_its_own_bar(case):
    """Trivially true (the bar is 8 x this error) unless the restatement is broken: a float32 evaluation that is far from float64, an
    output that is not finite, or two evaluations that do not name the same tensors."""
    r64, r32, bars = case.ref(torch.float64), case.ref(torch.float32), case.bars()
    assert set(r64) == set(r32) == set(bars)
    for k in sorted(r64):
        assert torch.isfinite(r64[k]).all() and torch.isfinite(r32[k]).all(), (case, k)
        assert r64[k].dtype == torch.float64 and r32[k].dtype == torch.float32, (case, k)
        err = R.rel_to_max(r32[k], r64[k])
        print(f"{case} {k}: cpu f32 {err:.3e}  bar {bars[k]['bar']:.3e}")
        assert err <= bars[k]["cpu_f32"] <= bars[k]["bar"] / R.MEASURED_FACTOR * (1 + 1e-12)
        assert err < 1e-4, (case, k, err)                          # float32 arithmetic, not a different function
        assert err == 0 or err >= R.QUARTER_ULP, (case, k, err)    # no bar rests on one lucky rounding (side_ops_ref's docstring)


@pytest.mark.parametrize("case", DERIVED, ids=_ids(DERIVED))
def test_derived_bound_holds_for_a_float32_numpy_evaluation(case):
    ref, absolute, f32 = case.terms(), case.terms(absolute=True), case.terms(dtype=np.float32)
    auto = case.ref(torch.float64)
    for k in sorted(ref):
        value, n = ref[k]
        assert f32[k][0].dtype == np.float32
        # the sums of products are the operator: they agree with autograd over the restatement to float64 rounding
        assert R.derived_ratio(auto[k].numpy(), value, absolute[k][0], n) < 1e-6, (case, k)
        ratio = R.derived_ratio(f32[k][0], value, absolute[k][0], n)
        print(f"{case} {k}: numpy f32 error / derived bound = {ratio:.3f}")
        assert ratio <= 1.0, (case, k, ratio)
        assert ((absolute[k][0] == 0) <= (value == 0)).all()       # the abs-sum is zero only where the result is exactly zero


def _measured_excess(case, defect, keys):
    """error of the defective restatement (float64) over the case's bar, per tensor"""
    ref, bars = case.ref(torch.float64), case.bars()
    out = {}
    for k in keys:
        assert bars[k]["bar"] > 0, (case, k)
        out[k] = R.rel_to_max(defect[k], ref[k]) / bars[k]["bar"]
        print(f"{case} {k}: planted defect / bar = {out[k]:.3e}")
    return out


def test_defect_columns_past_256_dropped():
    """the `c += 256` column loops of lf_train_fwd / lf_train_bwd / dot_bwd making one trip only"""
    case = R.scorer_case(260)
    ref, absolute = case.terms(), case.terms(absolute=True)
    hist, cand = case.leaves["hist"].numpy().copy(), case.leaves["cand"].numpy().copy()
    hist[:, 256:], cand[:, 256:] = 0, 0
    bad = R.late_fusion_terms(hist, cand, case.consts["hist_off"].tolist(), case.consts["cand_off"].tolist(), case.upstream["scores"].numpy())
    for k in ("user", "scores", "d_cand", "d_hist"):
        ratio = R.derived_ratio(bad[k][0], ref[k][0], absolute[k][0], ref[k][1])
        print(f"{case} {k}: planted defect / derived bound = {ratio:.3e}")
        assert ratio >= CLEAR, (k, ratio)
    case = R.dot_case(260, 5, True)
    ref, absolute = case.terms(), case.terms(absolute=True)
    user, rows = case.leaves["user"].numpy().copy(), case.leaves["cand"].numpy().copy()
    user[:, :, 256:], rows[:, :, 256:] = 0, 0
    bad = R.dot_terms(user, rows, True, case.upstream["out"].numpy())
    for k in ("out", "d_user", "d_cand"):
        ratio = R.derived_ratio(bad[k][0], ref[k][0], absolute[k][0], ref[k][1])
        print(f"{case} {k}: planted defect / derived bound = {ratio:.3e}")
        assert ratio >= CLEAR, (k, ratio)
    case = R.embedding_case(260, 0)
    ref, absolute = case.terms(), case.terms(absolute=True)
    bad = ref["d_table"][0].copy()
    bad[:, 256:] = 0
    assert R.derived_ratio(bad, ref["d_table"][0], absolute["d_table"][0], ref["d_table"][1]) >= CLEAR


@pytest.mark.parametrize("supcon", [True, False])
def test_defect_candidates_past_64_dropped_from_the_softmax(supcon):
    """the per-row lane loops `j += 64` of train_loss_kernel making one trip only"""
    case = R.loss_case(5, supcon)
    bad = R.evaluate(R.model_step_loss, case.leaves, dict(case.consts, softmax_limit=64), case.upstream, torch.float64)
    assert min(_measured_excess(case, bad, ("loss", "per", "d_scores")).values()) >= CLEAR


@pytest.mark.parametrize("supcon", [True, False])
def test_defect_impressions_past_256_dropped_from_the_reducer(supcon):
    """loss_reduce_kernel's `i += 256` stride making one trip only"""
    case = R.loss_case(257, supcon)
    bad = R.evaluate(R.model_step_loss, case.leaves, dict(case.consts, reduce_limit=256), case.upstream, torch.float64)
    assert min(_measured_excess(case, bad, ("loss", "d_scores")).values()) >= CLEAR


@pytest.mark.parametrize("n,d", [(65, 64), (130, 260)])
def test_defect_anchors_past_64_dropped_in_supcon_embeddings(n, d):
    """a_loss_kernel's `j += 64` (columns of the similarity row) and a_sim_kernel's `c += 64` making one trip only"""
    case = R.supcon_case(n, d, "class_of_one")
    ref, bars = case.ref(torch.float64), case.bars()
    emb = case.leaves["emb"].clone()
    emb[:, 64:] = 0                                              # the similarity from the first 64 columns only
    bad = R.evaluate(case.fn, {"emb": emb}, case.consts, case.upstream, torch.float64)
    if d > 64:
        assert R.rel_to_max(bad["loss"], ref["loss"]) / bars["loss"]["bar"] >= CLEAR
    short = R.evaluate(case.fn, {"emb": case.leaves["emb"][:64]}, dict(case.consts, labels=case.consts["labels"][:64]), case.upstream, torch.float64)
    excess = R.rel_to_max(short["per"], ref["per"][:64]) / bars["per"]["bar"]     # every anchor's row cut to its first 64 entries
    print(f"{case} per: planted defect / bar = {excess:.3e}")
    assert excess >= CLEAR


def _last_full_tile(l0, kt):
    return (l0 - 1) // kt * kt


@pytest.mark.parametrize("tiles", [R.AXIS0_KEY_TILE_TRAIN, R.AXIS0_KEY_TILE_ENTITY], ids=["train_small", "entity"])
@pytest.mark.parametrize("dh", R.AXIS0_DH)
def test_defect_last_partial_key_tile_dropped(dh, tiles):
    kt = tiles[dh]
    l0 = min(l for l in R.AXIS0_L0 if l > kt)                    # the smallest row count with a partial last tile
    assert 0 < l0 - _last_full_tile(l0, kt) < kt
    case = R.axis0_case(l0, 3, 2 * dh, 2)
    bad = R.evaluate(R.mha_axis0, case.leaves, dict(case.consts, key_limit=_last_full_tile(l0, kt)), case.upstream, torch.float64)
    assert min(_measured_excess(case, bad, ("out", "d_x", "d_in_w")).values()) >= CLEAR


@pytest.mark.parametrize("dh", R.AXIS0_DH)
@pytest.mark.parametrize("l0", [33, 300])
def test_defect_neighbouring_head_dim_case_applied(dh, l0):
    i = R.AXIS0_DH.index(dh)
    for other in {R.AXIS0_DH[max(i - 1, 0)], R.AXIS0_DH[min(i + 1, len(R.AXIS0_DH) - 1)]} - {dh}:
        case = R.axis0_case(l0, 3, 2 * dh, 2)
        bad = R.evaluate(R.mha_axis0, case.leaves, dict(case.consts, scale_dh=other), case.upstream, torch.float64)
        assert min(_measured_excess(case, bad, ("out", "d_x")).values()) >= CLEAR


DX_OC = 1024                    # rows_f32.hip: output features dx_rows_kernel stages per pass


@pytest.mark.parametrize("r,k,o", [(9, 8, 2049), (9, 8, 4100), (9, 300, 1030)])
@pytest.mark.parametrize("defect", ["second_pass_dropped", "stale_dy"])
def test_defect_in_the_passes_over_O_of_dx(r, k, o, defect):
    """dx_rows_kernel (rows_f32.hip) stages dy in passes of DX_OC = 1024 output features with the accumulators live across the passes"""
    assert (r, k, o) in R.LINEAR_SHAPES and o > DX_OC
    case = R.linear_case(r, k, o, True)
    ref, absolute = case.terms(), case.terms(absolute=True)
    dy, w = case.upstream["y"].double().numpy(), case.leaves["weight"].double().numpy()
    bad = dy[:, :DX_OC] @ w[:DX_OC]
    if defect == "stale_dy":                                     # every later pass multiplies what the first pass staged
        for o0 in range(DX_OC, o, DX_OC):
            no = min(DX_OC, o - o0)
            bad = bad + dy[:, :no] @ w[o0:o0 + no]
    ratio = R.derived_ratio(bad, ref["d_x"][0], absolute["d_x"][0], ref["d_x"][1])
    print(f"{case} d_x, {defect}: planted defect / derived bound = {ratio:.3e}")
    assert ratio >= CLEAR


def test_conditions_the_gpu_cases_rely_on():
    for b in R.LOSS_B:
        case = R.loss_case(b, True)
        scores, labels, off = case.leaves["scores"], case.consts["labels"], case.consts["cand_off"].tolist()
        per = case.ref(torch.float64)["per"]
        live = per[per != 0]
        assert (live >= 1e-3).all(), (b, float(live.min()))       # membership in the non-zero reducer is no rounding matter
        counts = np.diff(off)
        assert set(counts) <= set(R.LOSS_COUNTS) and (b < 6 or set(counts) == set(R.LOSS_COUNTS))
        assert int(counts.max()) < R.LOSS_C_MAX
        v = scores / np.float32(R.LOSS_TEMPERATURE)               # as the kernel forms it, in float32
        for i in range(b):
            row = torch.sort(v[off[i]:off[i + 1]], descending=True)[0]
            assert row.numel() == 1 or row[0] > row[1], (b, i)    # no exact tie in a row maximum
        if b >= 4:
            rows = [labels[off[i]:off[i + 1]] for i in range(b)]
            assert any(r.sum() == 0 for r in rows) and any(r.numel() > 1 and r.min() == 1 for r in rows)
            assert any(0 < r.sum() < r.numel() for r in rows)
    assert R.loss_case(257, True).ref()["per"][256] > 0 and R.loss_case(513, True).ref()["per"][512] > 0
    for n in R.SUPCON_N:
        for d in R.SUPCON_D:
            for kind in R.SUPCON_LABELS:
                case = R.supcon_case(n, d, kind)
                per = case.ref(torch.float64)["per"]
                assert (per[per != 0] >= 1e-3).all(), case
                e = case.leaves["emb"]
                top = torch.sort((e @ e.T) / np.float32(R.SUPCON_TEMPERATURE), dim=1, descending=True)[0]
                assert (top[:, 0] > top[:, 1]).all(), case
                if kind == "class_of_one" and n > 2:
                    assert per[-1] == 0 and float(case.ref()["loss"]) > 0
                if kind != "class_of_one" or n == 2:
                    assert float(case.ref()["loss"]) == 0         # no positive pair or no negative pair: the documented zero
    for dh in R.AXIS0_DH:                                         # every key tile of both columns is crossed, and the 256-row block
        for tiles in (R.AXIS0_KEY_TILE_TRAIN, R.AXIS0_KEY_TILE_ENTITY):
            assert any(l > tiles[dh] and l % tiles[dh] for l in R.AXIS0_L0)
    assert max(R.AXIS0_L0) > 256 and R.DROPOUT_N > 8192 * 256
    for case in (R.embedding_case(d, 0) for d in R.EMBEDDING_D):
        ids = case.consts["ids"].reshape(-1)
        assert ids.unique().numel() < ids.numel() and (ids == 0).sum() >= 3
