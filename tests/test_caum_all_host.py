"""The shared-product form of CAUM's candidate loop (tests/caum_all_ref.py) without a GPU: it equals the float64 loop over the columns
(``caum_ref.caum_module_forward``) to 1e-12 of the largest score at every shape tests/test_gpu_caum_all.py runs, its float32
evaluation stays within the case's MEASURED bar (8 x the float32 CPU error of the loop), with ``w3b out_w`` folded and without, and
every planted defect exceeds that bar at least 10-fold on the shapes it is shown at."""
import pytest
import torch

import caum_all_ref as CA
import side_ops_ref as R


def _ids(shape):
    return "B{}-S{}-D{}-F{}-H{}-{}-h{}-C{}".format(*shape)


def _form(case, dtype, **kw):
    return R.evaluate(CA.caum_scores_all, case.leaves, dict(case.consts, **kw), None, dtype)["scores"]


@pytest.mark.parametrize("shape", CA.SHAPES, ids=_ids)
def test_the_shared_product_form_is_the_loop_over_the_columns(shape):
    case = CA.all_case(*shape)
    ref, bar = case.ref()["scores"], case.bars()["scores"]
    assert tuple(ref.shape) == (shape[0], shape[7]) and float(ref.abs().max()) > 0
    for fold in (True, False):
        exact = R.rel_to_max(_form(case, torch.float64, fold=fold), ref)
        single = R.rel_to_max(_form(case, torch.float32, fold=fold), ref)
        print(f"{case} fold={fold}: float64 {exact:.2e}; float32 {single:.2e} = {single / bar['cpu_f32']:.2f} x the loop's {bar['cpu_f32']:.2e} (bar 8 x)")
        assert exact <= 1e-12, (case, fold, exact)
        assert single <= bar["bar"], (case, fold, single, bar)


def test_the_cases_settle_and_carry_the_padded_rows():
    for shape in CA.SHAPES:
        case = CA.all_case(*shape)
        assert all(v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP for v in case.bars().values()), case
        hist, cand = case.leaves["hist"], case.leaves["cand"]
        if shape[0] > 1:
            assert not cand[1, -1].any() and not hist[1, -1].any() and hist[0, -1].any() and cand[0, -1].any(), case
            assert float(case.ref()["scores"][1, -1]) == 0.0                       # a zero candidate row scores an exact zero


def _partial(case):
    c = case.leaves["cand"].shape[1]
    return next(n for n in (2, 3, 4) if c % n)


# (planted defect, keyword arguments of the restatement as a function of the case)
_PLANTED = [
    ("QC added to q but not to k", lambda c: dict(candidate_in_keys=False)),
    ("every column attends with column 0's QC", lambda c: dict(own_column=False)),
    ("the (b, c) terms read at the transposed row c B + b", lambda c: dict(transposed_rows=True)),
    ("w3b out_b left out of A", lambda c: dict(out_bias_term=False)),
    ("CT left out", lambda c: dict(candidate_tanh_term=False)),
    ("slots past a row tile left out of the softmax over S", lambda c: dict(slot_limit=8 if c.leaves["hist"].shape[1] > 8 else c.leaves["hist"].shape[1] - 1)),
    ("the columns of a last partial pass left at zero", lambda c: dict(zero_partial_pass=_partial(c))),
]


@pytest.mark.parametrize("shape", CA.DEFECT_SHAPES, ids=_ids)
@pytest.mark.parametrize("what,kwargs", _PLANTED, ids=[p[0] for p in _PLANTED])
def test_a_planted_defect_exceeds_the_bar_tenfold(what, kwargs, shape):
    case = CA.all_case(*shape)
    b, s, c = shape[0], shape[1], shape[7]
    assert b != c and c >= 3 and s >= 5
    ratio = R.rel_to_max(_form(case, torch.float64, **kwargs(case)), case.ref()["scores"]) / case.bars()["scores"]["bar"]
    print(what, case, f"{ratio:.3g} x the bar")
    assert ratio >= 10.0, (what, ratio)
