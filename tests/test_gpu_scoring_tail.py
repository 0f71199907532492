"""The tail of the inference hot path against plain float64 references (scoring_tail_ref.py), EVERY candidate, row and column:

A. the fused gather-mean-dot scorers in their five kernel forms (f32 column-block / whole-row, f16 column-block / whole-row,
   given user) under the DERIVED per-candidate bound n u A_j — widths at the edges of the 256- and 512-column trips, list
   lengths across every batch size, value regimes, exactness on integer tables, the status word;
B. the half-table copy: column mean under its derived bound, stored rows bit for bit;
C. the additive pooler on its three routes and the strict switch, ten value regimes, under bars MEASURED on an MI355X against
   float64 (x 1.5, rounded up: POOL_BARS, profiles/scoring_tail/measured_tolerances.json), none above the stated 1e-4 / 2e-5;
D. ``dot`` in its three kernel forms under its derived bound.

The kernel-against-kernel bit-equalities and the spot checks of test_gpu_parity.py stay where they are."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import manner_oracle as O  # noqa: E402
import scoring_tail_ref as R  # noqa: E402
from manner_amd import hip, hotpath  # noqa: E402

DEV = "cuda:0"
SWITCH = "MANNER_HIP_SCORER_GENERIC"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_lists(case):
    return tuple(_cuda(case[k]) for k in ("hist_idx", "hist_off", "cand_idx", "cand_off"))


def _lists(case):
    return case["hist_idx"], case["hist_off"], case["cand_idx"], case["cand_off"]


def _under(what, got, ref, bnd, ratios, failures):
    """every candidate under its bound; the largest error / bound is kept for the record"""
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    if not len(ref):
        return
    ratio = R.ratio_to_bound(np.abs(got - ref), bnd)                     # a zero bound demands exactly zero
    ratio[~np.isfinite(got)] = np.inf
    j = int(np.argmax(ratio))
    ratios[what] = max(ratios.get(what, 0.0), float(ratio[j]))
    print(f"  {what:28s} largest error / derived bound {ratio[j]:.3f} (candidate {j} of {len(ref)})")
    if ratio[j] > 1.0:
        failures.append(f"{what}: candidate {j} at {ratio[j]:.3g} of its bound, {int((ratio > 1).sum())} of {len(ref)} over")


# ================================================================================================ A. scorers

@pytest.mark.parametrize("spec", R.F32_SPECS, ids=R.spec_id)
def test_f32_scorers_under_the_derived_bound(spec, monkeypatch, measured):
    case = R.build_case(spec)
    D = case["table"].shape[1]
    table, user, lists = _cuda(case["table"]), _cuda(case["user"]), _dev_lists(case)
    H = R.hist_sizes_per_candidate(case["hist_off"], case["cand_off"])
    ref, A = R.late_fusion(case["table"], *_lists(case))
    refu, Au = R.late_fusion_user(case["table"], case["user"], case["cand_idx"], case["cand_off"])
    ratios, failures = {}, []
    for generic in ([False, True] if D in (768, 1024) else [False]):
        if generic:
            monkeypatch.setenv(SWITCH, "1")
        form = R.f32_form(D, generic)
        _under(form, hip.score_late_fusion(table, *lists), ref, R.bound(R.scorer_ops(form, H, D), A), ratios, failures)
        _under("user_" + form, hip.score_user(table, user, lists[2], lists[3]), refu, R.bound(R.scorer_ops("user", H, D), Au), ratios, failures)
    monkeypatch.delenv(SWITCH, raising=False)
    if D in (768, 1024):
        imp = dict(zip(("hist_idx", "hist_off", "cand_idx", "cand_off"), lists))
        fused = hotpath.score_impressions([table], imp, fused=True)["scores"]
        _under("fuse_rank", fused, ref, R.bound(R.scorer_ops("f32_rows", H, D), A), ratios, failures)
    hip.check_status(DEV)
    measured(**ratios)
    assert not failures, failures


@pytest.mark.parametrize("spec", R.F16_SPECS, ids=R.spec_id)
def test_f16_scorers_under_the_derived_bound(spec, monkeypatch, measured):
    """the references take the half values and the mean READ BACK from the device: only the accumulation is judged"""
    case = R.build_case(spec)
    D = case["table"].shape[1]
    table, lists = _cuda(case["table"]), _dev_lists(case)
    H = R.hist_sizes_per_candidate(case["hist_off"], case["cand_off"])
    plain, centred = hip.table_to_f16(table), hip.table_to_f16(table, centre=True)
    ratios, failures = {}, []
    for tag, half, mean in (("", plain, None), ("_centred", centred, centred.mean.cpu().numpy())):
        rows = (half if mean is None else half.rows).cpu().numpy()
        ref, A = R.late_fusion_half(rows, mean, *_lists(case))
        for generic in ([False, True] if D in (768, 1024) else [False]):
            if generic:
                monkeypatch.setenv(SWITCH, "1")
            form = R.f16_form(D, generic)
            _under(form + tag, hip.score_late_fusion(half, *lists), ref, R.bound(R.scorer_ops(form, H, D, mean is not None), A), ratios, failures)
        monkeypatch.delenv(SWITCH, raising=False)
    hip.check_status(DEV)
    measured(**ratios)
    assert not failures, failures


def test_unsupported_widths_are_refused_not_launched():
    case = R.width_case(8)
    lists = _dev_lists(case)
    wide = torch.zeros((300, 3076), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4, <= 3072"):
        hip.score_late_fusion(wide, *lists)
    with pytest.raises(RuntimeError, match="multiple of 4, <= 3072"):
        hip.score_user(wide, torch.zeros((len(case["cand_off"]) - 1, 3076), device=DEV), lists[2], lists[3])
    with pytest.raises(RuntimeError, match="multiple of 8, <= 3072"):
        hip.score_late_fusion(torch.zeros((300, 4), dtype=torch.float16, device=DEV), *lists)
    with pytest.raises(RuntimeError, match="multiple of 8, <= 3072"):
        hip.score_late_fusion(torch.zeros((300, 3080), dtype=torch.float16, device=DEV), *lists)
    hip.check_status(DEV)


@pytest.mark.parametrize("D", [4, 260, 520, 768, 1024])
def test_integer_tables_come_out_exact(D, monkeypatch):
    """entries in [-8, 8], H a power of two: every sum, the division and every product are exact in float32 (|sum| < 2^20 in units of
    1/16), so the five forms must EQUAL the float64 reference — no tolerance"""
    case = R.exact_case(D)
    table, user, lists = _cuda(case["table"]), _cuda(case["user"]), _dev_lists(case)
    ref, _ = R.late_fusion(case["table"], *_lists(case))
    refu, _ = R.late_fusion_user(case["table"], case["user"], case["cand_idx"], case["cand_off"])
    ran = []
    for generic in ([False, True] if D in (768, 1024) else [False]):
        if generic:
            monkeypatch.setenv(SWITCH, "1")
        got = {R.f32_form(D, generic): (hip.score_late_fusion(table, *lists), ref),
               "user_" + R.f32_form(D, generic): (hip.score_user(table, user, lists[2], lists[3]), refu)}
        if D % 8 == 0:
            half = hip.table_to_f16(table)
            assert torch.equal(half.float(), table)
            got[R.f16_form(D, generic)] = (hip.score_late_fusion(half, *lists), ref)
        for form, (out, want) in got.items():
            assert np.array_equal(out.cpu().numpy().astype(np.float64), want), form
            ran.append(form)
    monkeypatch.delenv(SWITCH, raising=False)
    hip.check_status(DEV)
    print(f"D={D}: exact in {ran}")


@pytest.mark.parametrize("half,D", [(False, 768), (False, 260), (True, 768), (True, 520)])
def test_one_bad_index_raises_and_leaves_the_other_impressions_alone(half, D):
    """one out-of-range index at a history position past the first batch, at a candidate position in the second in-flight slot (j + 4),
    and at an odd candidate position (the upper half-wave of the f16 whole-row form)"""
    case = R.width_case(D)
    ho, co = case["hist_off"], case["cand_off"]
    b = next(i for i in range(len(ho) - 1) if ho[i + 1] - ho[i] >= 20 and co[i + 1] - co[i] >= 12)
    table = _cuda(case["table"])
    if half:
        table = hip.table_to_f16(table)
    hip.check_status(DEV)
    clean = hip.score_late_fusion(table, *_dev_lists(case)).cpu()
    hip.check_status(DEV)
    keep = np.ones(int(co[-1]), bool)
    keep[co[b]:co[b + 1]] = False
    for key, pos, bad in (("hist_idx", ho[b] + 18, 300), ("cand_idx", co[b] + 5, -1), ("cand_idx", co[b] + 11, 2 ** 31 - 1)):
        dirty = dict(case)
        dirty[key] = case[key].copy()
        dirty[key][pos] = bad
        out = hip.score_late_fusion(table, *_dev_lists(dirty)).cpu()
        with pytest.raises(RuntimeError, match="index outside the table"):
            hip.check_status(DEV)
        hip.check_status(DEV)                                            # cleared by the check
        assert torch.equal(out[keep], clean[keep]), (key, int(pos))


# ================================================================================================ B. the half-table copy

@pytest.mark.parametrize("D", [4, 260, 768])
def test_half_table_copy_mean_and_stored_rows(D, measured):
    worst = 0.0
    for n_rows in (1, 2, 255, 256, 257, 511, 512, 513, 1000):
        t = R.make_table("collinear", n_rows, D, R._rng("copy", n_rows, D))
        dev = _cuda(t)
        ht = hip.table_to_f16(dev, centre=True)
        mean = ht.mean.cpu().numpy()
        ref, scale = R.column_mean(t)
        ratio = float(R.ratio_to_bound(np.abs(mean.astype(np.float64) - ref), R.bound(R.ops_col_mean(n_rows), scale)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (n_rows, ratio)
        assert np.array_equal(ht.rows.cpu().numpy().view(np.uint16), R.half_rows(t, mean).view(np.uint16)), n_rows
        assert torch.equal(hip.table_to_f16(dev).cpu(), torch.from_numpy(t).half()), n_rows
    hip.check_status(DEV)
    print(f"D={D}: column mean at most {worst:.3f} of its derived bound")
    measured(col_mean_over_bound=worst)


# ================================================================================================ C. the pooler

# max|out - float64| / max(1, max|x| of the batch element), measured on an MI355X (profiles/scoring_tail/measured_tolerances.json) x 1.5
# and rounded up to two digits — the margin of TILE_BARS, for run-to-run order effects of the LDS meeting points.  "base" covers the
# group's whole shape list.  Every one-pass case runs the ``randn`` query (x 8 peaked); its largest figure is big_w at 8e-6.
POOL_BARS = {
    "one_pass": {"base": 3.1e-06, "peaked": 9.2e-07, "near_tie": 1.3e-07, "outlier": 6.9e-07, "row_scale": 7.1e-07,
                 "zero_tail": 1.6e-06, "zero_element": 2.6e-07, "tiny_w": 1.5e-07, "big_w": 1.2e-05, "collinear": 2.0e-07},
    "two_pass_mfma": {"base": 1.2e-07, "peaked": 1.2e-08, "near_tie": 8.2e-08, "outlier": 4.7e-07, "row_scale": 3.3e-08,
                      "zero_tail": 4.4e-08, "zero_element": 4.0e-08, "tiny_w": 9.8e-08, "big_w": 9.6e-08, "collinear": 8.3e-07},
    "strict": {"base": 9.0e-08, "peaked": 1.1e-06, "near_tie": 2.2e-07, "outlier": 3.8e-08, "row_scale": 3.6e-07,
               "zero_tail": 5.6e-08, "zero_element": 3.5e-07, "tiny_w": 1.4e-07, "big_w": 2.1e-07, "collinear": 5.1e-07},
    "valu": {"base": 5.9e-08, "peaked": 1.0e-07, "near_tie": 9.9e-08, "outlier": 2.4e-07, "row_scale": 9.7e-09,
             "zero_tail": 3.8e-08, "zero_element": 3.1e-07, "tiny_w": 2.8e-08, "big_w": 5.4e-08, "collinear": 3.1e-07},
}


def _pool(group, regime, shape, sweep=False):
    """(error of the kernel, error of float32 torch on the CPU), both against float64 in units of the batch element's scale"""
    strict = group == "strict"
    assert R.pool_route(*shape, strict=strict) == R.pool_group_route(group, shape)
    x, w, b, q = R.pool_case(regime, *shape, soft=R.pool_soft(group, regime, sweep))
    ref = R.additive_pool(x, w, b, q)
    dev = [_cuda(a) for a in (x, w, b, q)]
    out = hip.additive_pool(*dev, strict=strict)
    again = hip.additive_pool(*dev, strict=strict)
    hip.check_status(DEV)
    assert torch.isfinite(out).all(), (group, regime, shape)
    assert torch.equal(out, again), (group, regime, shape)               # same bits on a second call
    if group == "one_pass":
        # the route is OBSERVED, not only inferred from the shape: the one-pass kernel (split products, hardware exp / rcp) cannot
        # give the bits of the two-pass path, which a fallback (misaligned x, out or workspace) would
        assert not torch.equal(out, hip.additive_pool(*dev, strict=True)), (regime, shape)
    cpu = O.additive_attention(*(torch.from_numpy(a) for a in (x, w, b, q))).numpy()
    return R.pool_error(out.cpu().numpy(), ref, x), R.pool_error(cpu, ref, x)


@pytest.mark.parametrize("group", list(R.POOL_ROUTE_SHAPES))
def test_pooler_shapes_against_float64(group, measured):
    """the shapes that change a route's geometry (strips per batch element, passes over the units, a last workgroup with missing
    batch elements, partial and full 16-unit tiles at every k-step count, 256-row chunks and 1024-column blocks of the apply
    kernel) on ``randn`` inputs; "strict" = strict=True at every one-pass shape"""
    bar, worst, worst_cpu, failures = POOL_BARS[group]["base"], 0.0, 0.0, []
    for shape in R.POOL_ROUTE_SHAPES[group]:
        err, cpu = _pool(group, "base", shape, sweep=True)
        print(f"  {group} B,S,D,Q={shape}: error {err:.3e} (float32 on the CPU {cpu:.3e}), bar {bar:.1e}")
        worst, worst_cpu = max(worst, err), max(worst_cpu, cpu)
        if not err <= bar:
            failures.append((shape, err))
    measured(err=worst, cpu_f32=worst_cpu, bar=bar)
    assert not failures, failures


@pytest.mark.parametrize("regime", R.POOL_REGIMES)
@pytest.mark.parametrize("group", list(R.POOL_REGIME_SHAPE))
def test_pooler_regimes_against_float64(group, regime, measured):
    shape, bar = R.POOL_REGIME_SHAPE[group], POOL_BARS[group][regime]
    err, cpu = _pool(group, regime, shape)
    print(f"  {group} {regime} B,S,D,Q={shape}: error {err:.3e} (float32 on the CPU {cpu:.3e}), bar {bar:.1e}")
    measured(err=err, cpu_f32=cpu, bar=bar)
    assert err <= bar


def test_bars_stay_under_the_conditions():
    """no one-pass bar above 1e-4, no two-pass bar above 2e-5: the bars hip.additive_pool and test_gpu_parity.py state; and the
    committed record holds the measurement every bar was taken from"""
    for route, bars in POOL_BARS.items():
        assert set(bars) == set(R.POOL_REGIMES)
        for regime, bar in bars.items():
            assert 0 < bar <= R.POOL_CAPS[route], (route, regime, bar)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scoring_tail", "measured_tolerances.json")
    with open(path) as f:
        rec = json.load(f)
    for route, bars in POOL_BARS.items():
        for regime, bar in bars.items():
            got = rec[f"test_pooler_regimes_against_float64[{route}-{regime}]"]
            err = got["err"] if regime != "base" else max(got["err"], rec[f"test_pooler_shapes_against_float64[{route}]"]["err"])
            assert got["bar"] == bar and 1.5 * err <= bar, (route, regime, err, bar)


# ================================================================================================ D. dot

def _dot_form(u, cand):
    """the kernel form manner_hip_dot picks for a [B, D, C] view"""
    sb, sd, sc = cand.stride()
    if sd != 1:
        return "strided"
    ok = cand.shape[1] % 4 == 0 and sb % 4 == 0 and sc % 4 == 0 and cand.data_ptr() % 16 == 0 and u.data_ptr() % 16 == 0
    return "vector" if ok else "scalar"


def _dot_views(cand):
    """[B, C, D] values as the [B, D, C] views that reach each form: permuted rows, rows with a stride that is no multiple of 4,
    rows 4 bytes off the alignment, a materialised [B, D, C] tensor"""
    B, C, D = cand.shape
    yield "rows", cand.permute(0, 2, 1)
    padded = torch.zeros((B, C, D + 1), dtype=cand.dtype, device=cand.device)
    padded[:, :, :D] = cand
    yield "odd_stride", padded[:, :, :D].permute(0, 2, 1)
    flat = torch.zeros(B * C * D + 1, dtype=cand.dtype, device=cand.device)
    flat[1:] = cand.reshape(-1)
    yield "unaligned", flat[1:].view(B, C, D).permute(0, 2, 1)
    yield "materialised", cand.permute(0, 2, 1).contiguous()


@pytest.mark.parametrize("B,C", [(1, 1), (1, 5), (3, 341)])
def test_dot_three_forms_under_the_derived_bound(B, C, measured):
    seen, ratios, failures = set(), {}, []
    for D in (1, 3, 4, 252, 260, 768):
        for integer in (False, True):
            u, c = R.dot_case(B, C, D, integer)
            ref, A = R.dot(u, c.transpose(0, 2, 1))
            ud, cd = _cuda(u), _cuda(c)
            for how, view in _dot_views(cd):
                form = _dot_form(ud, view)
                seen.add((how, form))
                out = hip.dot(ud, view).cpu().numpy().astype(np.float64)
                if integer:
                    assert np.array_equal(out, ref), (D, how, form)
                    continue
                ratio = float(R.ratio_to_bound(np.abs(out - ref), R.bound(R.ops_dot(form, D), A)).max())
                ratios[form] = max(ratios.get(form, 0.0), ratio)
                if not ratio <= 1.0:
                    failures.append((D, how, form, ratio))
    hip.check_status(DEV)
    print(f"  B={B} C={C}: largest error / derived bound {ratios}; forms reached {sorted(seen)}")
    measured(**ratios)
    assert {f for _, f in seen} == ({"vector", "scalar", "strided"} if C > 1 else {"vector", "scalar"})
    assert ("odd_stride", "scalar") in seen and ("unaligned", "scalar") in seen and ("rows", "vector") in seen
    assert not failures, failures
