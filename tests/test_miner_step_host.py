"""CPU checks of tests/miner_step_ref.py: the disagreement restatement against the reference's own function (tests/golden/
miner_step.npz), the measured cases settled, the NaN placement of the zero-row bias cases, and every planted defect past its bar at
one listed shape at least — so the bars tests/test_gpu_miner_step.py holds the kernels to would catch a wrong quirk."""
import os

import numpy as np
import pytest
import torch

import miner_ref as M
import miner_step_ref as S
import side_ops_ref as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "miner_step.npz"))


def test_disagreement_restatement_is_the_reference_function(golden):
    user = torch.from_numpy(golden["user"]).requires_grad_(True)
    for key, zero in (("distance", False), ("distance_zero_diagonal", True)):
        got = S.pairwise_cosine_similarity_3d(user, user, zero_diagonal=zero).detach().numpy()
        assert np.abs(got - golden[key]).max() <= 2e-7, key       # float32 both: a matmul's summation order apart
    loss = S.disagreement(user)["loss"]
    loss.backward()
    assert abs(float(loss.detach()) - float(golden["loss"])) <= 2e-7 * abs(float(golden["loss"])) + 1e-9
    g, ref = user.grad.numpy(), golden["d_user"]
    zr = S.DISAGREEMENT_ZERO_ROW
    assert np.isfinite(ref).all() and np.abs(ref[zr]).max() > 1e5                    # the zero row: finite, through 1 / 1e-8
    assert np.abs(g[zr] - ref[zr]).max() <= 1e-5 * np.abs(ref[zr]).max()
    rest = np.ones(ref.shape[:2], bool)
    rest[zr] = False
    assert np.abs(g[rest] - ref[rest]).max() <= 1e-5 * np.abs(ref[rest]).max()


def test_every_measured_case_is_settled():
    for case in S.all_measured_cases():
        for k, v in case.bars().items():
            assert v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP, (case, k, v)
    for k, v in S.zero_row_bars(S.disagreement_case(3, 5, 64, True)).items():
        assert v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP, (k, v)


def test_one_vector_per_user_has_no_disagreement():
    ref = S.disagreement_case(1, 1, 4).ref()
    assert float(ref["loss"]) == 0.0 and float(ref["d_user"].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ NaN placement of the bias
def test_zero_candidate_row_poisons_the_other_users_only():
    case = S.BIAS_ZERO_ROW_CASES["zero-cand-row"]                  # the zero row is among the candidates of impression 1
    bias = case.ref()[0][:, :, 0]
    ho = case.hist_off.tolist()
    for b in range(3):
        h = ho[b + 1] - ho[b]
        assert bool(torch.isnan(bias[b, :h]).all()) == (b != 1) and bool(torch.isfinite(bias[b, :h]).all()) == (b == 1)
        assert float(bias[b, h:].abs().sum()) == 0.0               # padded slots: exactly 0, never NaN


def test_zero_history_row_is_nan_unless_every_column_is_its_users_own():
    bias = S.BIAS_ZERO_ROW_CASES["zero-hist-row"].ref()[0][:, :, 0]
    nan = torch.isnan(bias)
    assert bool(nan[0, 1]) and int(nan.sum()) == 1
    alone = S.BIAS_ZERO_ROW_CASES["zero-hist-row-one-user"].ref()[0]
    assert float(alone.abs().max()) == 0.0 and not bool(torch.isnan(alone).any())
    assert float(S.BIAS_CASES["one-user"].ref()[0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ planted defects
def _bias_ratio(case, **defect):
    ref, absolute = case.ref()
    got = S.category_bias(**case.args(), **defect)["bias"]
    if not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return float("inf")                                      # a NaN moved: compared by position, no bar to meet
    ok = ~torch.isnan(ref)
    return R.derived_ratio(got[ok].numpy(), ref[ok].numpy(), absolute[ok.numpy()], case.n)


@pytest.mark.parametrize("defect", [dict(zero_own=False), dict(count_non_own=True), dict(eps=1e-8)], ids=["own-kept", "non-own-count", "epsilon"])
def test_bias_bar_sees_a_wrong_quirk(defect):
    cases = [c for c in list(S.BIAS_CASES.values()) + list(S.BIAS_ZERO_ROW_CASES.values()) if not (defect.get("count_non_own") and len(c.hist_off) == 2)]
    assert all(_bias_ratio(c) == 0.0 for c in cases)
    worst = {c.name: _bias_ratio(c, **defect) for c in cases}
    assert max(worst.values()) > 1.0, worst


def test_bias_bar_sees_a_dropout_mask_indexed_by_the_column_alone():
    case = S.BIAS_CASES["shipped-Dc300"]
    p, seeds = S.BIAS_DROPOUT_P, S.BIAS_DROPOUT_SEEDS
    ref, absolute = case.ref(seeds, p)
    keeps = S.dropout_keeps(seeds, p, case.hist_cat.numel(), case.cand_cat.numel(), case.dc, by_column=True)
    got = S.category_bias(**case.args(), keeps=keeps, p=p)["bias"]
    assert R.derived_ratio(got.numpy(), ref.numpy(), absolute, case.n) > 1.0
    assert not torch.equal(ref, case.ref()[0])                   # and the masks do something


def test_scores_bar_sees_ties_going_to_the_last_code():
    case = S.scores_case(3, 5, 64, (6, 4, 1), "max", True)
    ref, absolute = case.terms(), case.terms(absolute=True)
    auto = case.ref()
    for k in ("out", "d_cand", "d_user"):                        # the plain-sum form and the autograd form of the restatement agree
        assert R.derived_ratio(auto[k].numpy(), ref[k][0], absolute[k][0], ref[k][1]) <= 1.0, k
    assert float(auto["d_user"][:, 2].abs().max()) == 0.0 and float(auto["d_user"][:, 0].abs().max()) > 0.0
    bad = R.evaluate(S.code_scores, case.leaves, dict(case.consts, tie_last=True), case.upstream, torch.float64)
    assert torch.equal(bad["out"], auto["out"])                  # a tie: the value cannot tell, the gradient does
    assert R.derived_ratio(bad["d_user"].numpy(), ref["d_user"][0], absolute["d_user"][0], ref["d_user"][1]) > 1.0


@pytest.mark.parametrize("score_type", S.SCORE_TYPES)
@pytest.mark.parametrize("shape", S.SCORE_SHAPES, ids=lambda s: "B{}-K{}-D{}".format(*s[:3]))
def test_scores_terms_are_the_restatement(shape, score_type):
    case = S.scores_case(*shape, score_type)
    ref, absolute, auto = case.terms(), case.terms(absolute=True), case.ref()
    for k in ("out", "d_cand", "d_user"):
        assert R.derived_ratio(auto[k].numpy(), ref[k][0], absolute[k][0], ref[k][1]) <= 1.0, k


@pytest.mark.parametrize("defect", [dict(keep_diagonal=True), dict(k_minus_one=True), dict(one_plus_norm=True)],
                         ids=["diagonal-kept", "K-minus-one", "one-plus-norm"])
def test_disagreement_bar_sees_a_wrong_quirk(defect):
    worst = {}
    for shape in S.DISAGREEMENT_SHAPES[:4]:
        case = S.disagreement_case(*shape)
        bad = R.evaluate(S.disagreement, case.leaves, defect, case.upstream, torch.float64)
        worst[shape] = max(R.rel_to_max(bad[k], case.ref()[k]) / case.bars()[k]["bar"] for k in ("loss", "d_user"))
    assert max(worst.values()) > 1.0, worst


@pytest.mark.parametrize("score_type", M.SCORE_TYPES)
def test_step_bar_sees_padded_zeros_left_out_of_the_softmax(score_type):
    case = S.step_case(score_type)
    bad = R.evaluate(S.miner_step, case.leaves, dict(case.consts, pad_in_softmax=False), case.upstream, torch.float64)
    assert R.rel_to_max(bad["loss"], case.ref()["loss"]) > case.bars()["loss"]["bar"]
    assert R.rel_to_max(bad["d_cand"], case.ref()["d_cand"]) > case.bars()["d_cand"]["bar"]
