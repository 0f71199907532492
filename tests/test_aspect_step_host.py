"""The restatements of tests/aspect_step_ref.py against torch's own calls — the ones TANRPLMModule / SentiRecPLMModule make — in float64
on the CPU, the conditions its cases promise (settled figures, no residual or product near a kink), and the library's new exports."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import aspect_step_ref as A
import side_ops_ref as R
from miner_step_ref import to_dense


def _f64(case):
    return {k: v.double() for k, v in case.leaves.items()}


@pytest.mark.parametrize("shape", A.HEAD_SHAPES, ids=lambda s: "N{}-D{}-O{}".format(*s))
def test_head_ce_is_cross_entropy_with_one_hot_probability_targets(shape):
    case = A.ce_case(*shape)
    lv, target = _f64(case), case.consts["target"]
    logits = F.linear(lv["x"], lv["weight"], lv["bias"])
    want = nn.CrossEntropyLoss()(logits, F.one_hot(target, num_classes=shape[2]).type_as(logits))
    got = A.head_ce(**lv, target=target)["loss"]
    assert abs(float(got) - float(want)) <= 1e-13 * abs(float(want))
    value, n = A.ce_logits_terms(case)
    assert n == shape[1] + 1 and np.abs(value - logits.numpy()).max() <= 1e-12
    with pytest.raises(RuntimeError):
        F.one_hot(torch.tensor([shape[2]]), num_classes=shape[2])      # the reference raises on a topic outside the table


@pytest.mark.parametrize("shape", A.HEAD_SHAPES, ids=lambda s: "N{}-D{}".format(*s[:2]))
def test_head_l1_is_l1_loss_of_the_flattened_head(shape):
    n, d, _ = shape
    case = A.l1_case(n, d)
    lv, target = _f64(case), case.consts["target"].double()
    want = nn.L1Loss()(F.linear(lv["x"], lv["weight"], lv["bias"]).flatten(), target)
    assert abs(float(A.head_l1(**lv, target=target)["loss"]) - float(want)) <= 1e-13 * abs(float(want))
    clearance, zeros = A.l1_kink_clearance(case)
    assert clearance > 8.0, (case, clearance)                          # every residual is clear of the kink ...
    assert zeros == ([A.ZERO_ROW] if n > A.ZERO_ROW else [])            # ... or exactly zero by construction: the all-zero row
    if zeros:
        ref = case.ref()
        assert float(ref["d_x"][A.ZERO_ROW].abs().max()) == 0.0 and float(case.ref(torch.float32)["d_x"][A.ZERO_ROW].abs().max()) == 0.0


def _dense_senti(case, dtype=torch.float64):
    """sentirec_plm_module.py:180-192 on zero-padded dense blocks"""
    cs = case.consts
    ho, co = cs["hist_off"], cs["cand_off"]
    scores = case.leaves["scores"].to(dtype).requires_grad_(True)
    s_hist = to_dense(cs["hist_score"].to(dtype), ho, max(int((ho[1:] - ho[:-1]).max()), 1))
    s_cand, dense = to_dense(cs["cand_score"].to(dtype), co, cs["c_max"]), to_dense(scores, co, cs["c_max"])
    u = torch.div(s_hist.sum(dim=1), (ho[1:] - ho[:-1]))
    loss = F.relu(u.unsqueeze(dim=-1) * s_cand * dense).mean()
    loss.backward()
    return loss.detach(), scores.grad


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("b", A.SENTI_B)
def test_senti_div_is_relu_mean_over_the_dense_blocks(b, padded):
    case = A.senti_case(b, padded)
    want, want_grad = _dense_senti(case)
    ref = case.ref()
    assert tuple(ref["loss"].shape) == () and abs(float(ref["loss"]) - float(want)) <= 1e-13 * abs(float(want))
    assert float((ref["d_scores"] - 0.75 * want_grad).abs().max()) <= 1e-15
    clearance, zeros = A.senti_kink_clearance(case)
    assert clearance > 8.0 and zeros >= 1, (case, clearance, zeros)     # clear of the kink, or exactly 0 (a neutral news)
    neutral = case.consts["cand_score"] == 0
    assert float(ref["d_scores"][neutral].abs().max()) == 0.0 and float(ref["d_scores"].abs().max()) > 0
    assert case.consts["c_max"] - max(R.LOSS_COUNTS[:b]) == (A.SENTI_PAD if padded else 0)


def test_senti_div_empty_history_is_nan_where_torch_puts_it():
    case = A.senti_empty_case()
    want, want_grad = _dense_senti(case)
    ref = case.ref()
    co = case.consts["cand_off"].tolist()
    own = torch.zeros(co[-1], dtype=torch.bool)
    own[co[1]:co[2]] = True
    assert torch.isnan(want) and torch.isnan(ref["loss"])
    assert torch.equal(torch.isnan(ref["d_scores"]), own) and torch.equal(torch.isnan(want_grad), own)
    assert float((ref["d_scores"][~own] - 0.75 * want_grad[~own]).abs().max()) <= 1e-15


def test_every_measured_case_is_settled():
    for case in A.all_measured_cases():
        for k, v in case.bars().items():
            assert v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP, (case, k, v)
        assert set(case.ref()) >= {"loss", "d_" + next(iter(case.leaves))}


def test_loss_lines_are_the_sums_the_modules_form():
    cs = A.step_consts()
    nh, t, d = int(cs["hist_off"][-1]), int(cs["cand_off"][-1]), 16
    hist, cand, scores = R.randn(1, nh, d).double(), R.randn(2, t, d).double(), R.randn(3, t).double()
    w, b = R.randn(4, A.STEP_TOPICS, d).double(), R.randn(5, A.STEP_TOPICS).double()
    y_true, dense = to_dense(cs["labels"].double(), cs["cand_off"], cs["c_max"]), to_dense(scores, cs["cand_off"], cs["c_max"])
    ce = nn.CrossEntropyLoss()(dense, y_true)
    topics = torch.cat((cs["cand_topic"], cs["hist_topic"]))
    logits = F.linear(torch.cat((cand, hist)), w, b)
    want = ce + A.TOPIC_COEF * nn.CrossEntropyLoss()(logits, F.one_hot(topics, num_classes=A.STEP_TOPICS).type_as(logits))
    got = A.tanr_loss_lines(scores, hist, cand, w, b, cs["hist_topic"], cs["cand_topic"], cs["labels"], cs["cand_off"], cs["c_max"])["loss"]
    assert abs(float(got) - float(want)) <= 1e-13 * abs(float(want))
    w1, b1 = R.randn(6, 1, d).double(), R.randn(7, 1).double()
    senti = torch.cat((cs["cand_score"], cs["hist_score"])).double()
    pred = nn.L1Loss()(F.linear(torch.cat((cand, hist)), w1, b1).flatten(), senti)
    s_hist = to_dense(cs["hist_score"].double(), cs["hist_off"], max(A.STEP_HIST))
    u = s_hist.sum(dim=1) / torch.tensor(A.STEP_HIST)
    div = F.relu(u.unsqueeze(-1) * to_dense(cs["cand_score"].double(), cs["cand_off"], cs["c_max"]) * dense).mean()
    want = ce + A.SENTI_PRED_COEF * pred + A.SENTI_DIV_COEF * div
    got = A.sentirec_loss_lines(scores, hist, cand, w1, b1, cs["hist_score"], cs["cand_score"], cs["labels"], cs["hist_off"], cs["cand_off"],
                                cs["c_max"])["loss"]
    assert abs(float(got) - float(want)) <= 1e-13 * abs(float(want))


def test_library_exports_the_aspect_entries_under_abi_8():
    from manner_amd import _lib
    lib = _lib.load()
    assert lib.manner_hip_abi_version() == 8
    for name in ("manner_hip_head_ce", "manner_hip_head_ce_backward", "manner_hip_head_l1", "manner_hip_head_l1_backward", "manner_hip_senti_div",
                 "manner_hip_senti_div_backward", "manner_hip_head_workspace_bytes", "manner_hip_head_backward_workspace_bytes",
                 "manner_hip_senti_div_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.manner_hip_head_workspace_bytes(0) == 0 and lib.manner_hip_head_workspace_bytes(10) >= 40
    assert lib.manner_hip_head_backward_workspace_bytes(100, 768, 19) >= 4 * 19 * 769 * 4
    assert lib.manner_hip_head_backward_workspace_bytes(100, 1028, 19) == 0 and lib.manner_hip_senti_div_workspace_bytes(5) >= 40
