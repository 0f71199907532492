"""CPU checks of what test_gpu_scoring_tail.py stands on (scoring_tail_ref.py): the float64 references agree with manner_oracle,
the float32 emulation of every scorer form stays under its DERIVED bound on every case the GPU test runs, each planted defect
is pushed over the bound by the case built for it, the exactness cases are exact, and on the pooler cases float32 arithmetic
itself stays a decade under the caps the GPU bars must respect.  Run with -s to see the figures."""
import numpy as np
import pytest
import torch

import manner_oracle as O
import scoring_tail_ref as R


def _batch(off):
    return torch.from_numpy(np.repeat(np.arange(len(off) - 1), np.diff(off)))


def _oracle_scores(table64, case, user=None):
    hist = torch.from_numpy(table64[case["hist_idx"].astype(np.int64)])
    cand = torch.from_numpy(table64[case["cand_idx"].astype(np.int64)])
    bh, bc = _batch(case["hist_off"]), _batch(case["cand_off"])
    if user is None:
        dense = O.cr_scores(hist, bh, cand, bc, late_fusion=True)
    else:
        cand_agg, _ = O.to_dense_batch(cand, bc)
        dense = O.dot_product(torch.from_numpy(user).unsqueeze(1), cand_agg.permute(0, 2, 1))
    return O.ragged(dense, bc).numpy()


def _lists(case):
    return case["hist_idx"], case["hist_off"], case["cand_idx"], case["cand_off"]


def _mean32(table):
    return R.column_mean(table)[0].astype(np.float32)


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if len(b) else 0.0


def test_references_agree_with_the_oracle_in_float64():
    worst = 0.0
    for case in R.f32_cases():
        t64 = case["table"].astype(np.float64)
        worst = max(worst, _rel(R.late_fusion(case["table"], *_lists(case))[0], _oracle_scores(t64, case)))
        u64 = case["user"].astype(np.float64)
        worst = max(worst, _rel(R.late_fusion_user(case["table"], case["user"], case["cand_idx"], case["cand_off"])[0],
                                _oracle_scores(t64, case, u64)))
    for case in R.f16_cases():
        for mean in (None, _mean32(case["table"])):
            rows = R.half_rows(case["table"], mean)
            full = rows.astype(np.float64) + (0.0 if mean is None else mean.astype(np.float64)[None, :])
            worst = max(worst, _rel(R.late_fusion_half(rows, mean, *_lists(case))[0], _oracle_scores(full, case)))
    for route, shape in R.POOL_REGIME_SHAPE.items():
        for regime in R.POOL_REGIMES:
            x, w, b, q = R.pool_case(regime, *shape, soft=R.pool_soft(route, regime))
            ref = O.additive_attention(*(torch.from_numpy(a.astype(np.float64)) for a in (x, w, b, q))).numpy()
            worst = max(worst, _rel(R.additive_pool(x, w, b, q), ref))
    for D in (1, 3, 4, 252, 260, 768):
        u, c = R.dot_case(5, 7, D)
        ref = O.dot_product(torch.from_numpy(u.astype(np.float64)), torch.from_numpy(c.astype(np.float64)).permute(0, 2, 1)).numpy()
        worst = max(worst, _rel(R.dot(u, c.transpose(0, 2, 1))[0], ref))
    dense, mask = O.to_dense_batch(torch.arange(7.0), torch.tensor([0, 0, 2, 2, 2, 3, 3]))
    assert dense.tolist() == [[0, 1, 0], [0, 0, 0], [2, 3, 4], [5, 6, 0]] and mask.sum(1).tolist() == [2, 0, 3, 2]
    t = R.width_case(260)["table"]
    assert _rel(R.column_mean(t)[0], torch.from_numpy(t.astype(np.float64)).mean(0).numpy()) < 1e-12
    print(f"references vs manner_oracle in float64: worst relative difference {worst:.2e}")
    assert worst < 1e-12


def _emulations(defect=None):
    """(form, case name, emulated float32 scores, float64 scores, bound) for every case and form the GPU test runs"""
    for case in R.f32_cases():
        D = case["table"].shape[1]
        H = R.hist_sizes_per_candidate(case["hist_off"], case["cand_off"])
        ref, A = R.late_fusion(case["table"], *_lists(case))
        forms = ["f32_block"] + (["f32_rows"] if D in (768, 1024) else [])
        for form in forms:                                              # one order of operations for both f32 kernels
            yield form, case["name"], R.emulate_f32(case["table"], *_lists(case), defect=defect), ref, R.bound(R.scorer_ops(form, H, D), A)
        ref, A = R.late_fusion_user(case["table"], case["user"], case["cand_idx"], case["cand_off"])
        yield "user", case["name"], R.emulate_f32(case["table"], *_lists(case), user=case["user"], defect=defect), ref, \
            R.bound(R.scorer_ops("user", H, D), A)
    for case in R.f16_cases():
        D = case["table"].shape[1]
        H = R.hist_sizes_per_candidate(case["hist_off"], case["cand_off"])
        for mean in (None, _mean32(case["table"])):
            rows = R.half_rows(case["table"], mean)
            ref, A = R.late_fusion_half(rows, mean, *_lists(case))
            tag = "_centred" if mean is not None else ""
            yield "f16_block" + tag, case["name"], R.emulate_f16_block(rows, mean, *_lists(case), defect=defect), ref, \
                R.bound(R.scorer_ops("f16_block", H, D, mean is not None), A)
            if D in (768, 1024):
                yield "f16_rows" + tag, case["name"], R.emulate_f16_rows(rows, mean, *_lists(case), defect=defect), ref, \
                    R.bound(R.scorer_ops("f16_rows", H, D, mean is not None), A)


def test_float32_emulations_stay_under_the_derived_bounds(measured):
    worst = {}
    for form, name, emu, ref, bnd in _emulations():
        if not len(ref):
            continue
        ratio = R.ratio_to_bound(np.abs(emu.astype(np.float64) - ref), bnd)
        j = int(np.argmax(ratio))
        if ratio[j] > worst.get(form, (0.0, ""))[0]:
            worst[form] = (float(ratio[j]), f"{name} candidate {j}")
        assert ratio[j] <= 1.0, f"{form} on {name}: candidate {j} at {ratio[j]:.3f} of its derived bound"
    for form, (ratio, where) in sorted(worst.items()):
        print(f"{form:18s} largest emulation error / derived bound {ratio:.3f}  ({where})")
        measured(**{f"{form}_emulation_over_bound": ratio})
    assert set(worst) == {"f32_block", "f32_rows", "user", "f16_block", "f16_rows", "f16_block_centred", "f16_rows_centred"}


# defect -> (emulated form, case): the case built to catch it
PLANTED = {
    "drop_last_hist_when_h_mod_8_is_1": ("f16_rows", lambda: R.lengths_case(768)),
    "slot_plus_4_scored_for_slot": ("f32", lambda: R.lengths_case(260)),
    "divide_by_h_plus_1": ("f32", lambda: R.width_case(768)),
    "tail_column_block_skipped": ("f32", lambda: R.width_case(260)),
    "upper_half_wave_reads_ja": ("f16_rows", lambda: R.width_case(768)),
    "centring_constant_left_out": ("f16_block_centred", lambda: R.width_case(520, "collinear")),
}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_goes_over_the_bound(defect):
    form, build = PLANTED[defect]
    case = build()
    D = case["table"].shape[1]
    H = R.hist_sizes_per_candidate(case["hist_off"], case["cand_off"])
    over = {}
    for planted in (None, defect):
        if form == "f32":
            ref, A = R.late_fusion(case["table"], *_lists(case))
            emu, ops = R.emulate_f32(case["table"], *_lists(case), defect=planted), R.scorer_ops("f32_block", H, D)
        else:
            mean = _mean32(case["table"]) if form.endswith("centred") else None
            rows = R.half_rows(case["table"], mean)
            ref, A = R.late_fusion_half(rows, mean, *_lists(case))
            fn = R.emulate_f16_rows if form.startswith("f16_rows") else R.emulate_f16_block
            emu, ops = fn(rows, mean, *_lists(case), defect=planted), R.scorer_ops(form[:9].rstrip("_"), H, D, mean is not None)
        over[planted] = R.ratio_to_bound(np.abs(emu.astype(np.float64) - ref), R.bound(ops, A))
    assert over[None].max() <= 1.0                                      # the clean emulation passes on this very case
    j = int(np.argmax(over[defect]))
    print(f"{defect}: caught by {case['name']} ({form}), candidate {j} at {over[defect][j]:.3g} of its bound, "
          f"{int((over[defect] > 1.0).sum())} of {len(ref)} candidates over")
    assert over[defect][j] > 1.0


@pytest.mark.parametrize("D", [4, 260, 768, 1024])
def test_exactness_cases_are_exact(D):
    """integer tables, H a power of two: the float32 emulation EQUALS the float64 reference, in every form"""
    case = R.exact_case(D)
    ref, _ = R.late_fusion(case["table"], *_lists(case))
    assert np.array_equal(R.emulate_f32(case["table"], *_lists(case)).astype(np.float64), ref)
    refu, _ = R.late_fusion_user(case["table"], case["user"], case["cand_idx"], case["cand_off"])
    assert np.array_equal(R.emulate_f32(case["table"], *_lists(case), user=case["user"]).astype(np.float64), refu)
    if D % 8 == 0:
        rows = R.half_rows(case["table"])
        assert np.array_equal(rows.astype(np.float32), case["table"])
        assert np.array_equal(R.emulate_f16_block(rows, None, *_lists(case)).astype(np.float64), ref)
        if D % 256 == 0:
            assert np.array_equal(R.emulate_f16_rows(rows, None, *_lists(case)).astype(np.float64), ref)


def _pool_cases():
    for group, shapes in R.POOL_ROUTE_SHAPES.items():
        for shape in shapes:
            yield group, "base", shape, R.pool_soft(group, "base", sweep=True)
    for group, shape in R.POOL_REGIME_SHAPE.items():
        for regime in R.POOL_REGIMES:
            yield group, regime, shape, R.pool_soft(group, regime)


def test_pooler_cases_leave_float32_a_decade_under_the_caps(measured):
    """the float32 torch evaluation of every pooler case the GPU test ships, against float64: under a tenth of the cap of its
    group (1e-4 one-pass, 2e-5 two-pass) in units of max(1, max|x| of the batch element) — so a kernel that misses a cap is wrong,
    not unlucky with its input.  Every one-pass case runs the ``randn`` query; the two-pass cases named in POOL_SOFT run the soft one."""
    worst, failures = {}, []
    assert not any(g == "one_pass" for g, _ in R.POOL_SOFT)
    for group, regime, shape, soft in _pool_cases():
        assert R.pool_route(*shape, strict=group == "strict") == R.pool_group_route(group, shape), (group, shape)
        x, w, b, q = R.pool_case(regime, *shape, soft=soft)
        out = O.additive_attention(*(torch.from_numpy(a) for a in (x, w, b, q))).numpy()
        err = R.pool_error(out, R.additive_pool(x, w, b, q), x)
        key = (group, regime, "soft" if soft else "randn")
        worst[key] = max(worst.get(key, 0.0), err)
        assert np.isfinite(out).all()
        if not err < R.POOL_CAPS[group] / 10:
            failures.append(f"{group} {regime} {shape}: float32 itself is at {err:.2e}")
    for (group, regime, query), err in sorted(worst.items()):
        print(f"{group:14s} {regime:13s} q {query:5s} float32 CPU error {err:.2e}  (cap / 10 = {R.POOL_CAPS[group] / 10:.0e})")
        measured(**{f"{group}_{regime}_{query}_cpu_f32": err})
    assert not failures, failures


def test_a_zero_bound_demands_exactly_zero():
    """a candidate whose every term is zero (A_j = 0) must score exactly zero: no NaN ratio that compares as a pass"""
    assert R.ratio_to_bound([0.0, 1e-30, 1.0, 2.0], [0.0, 0.0, 2.0, 1.0]).tolist() == [0.0, np.inf, 0.5, 2.0]
