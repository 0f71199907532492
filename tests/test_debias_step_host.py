"""The float64 restatements of tests/debias_step_ref.py against a second formulation in torch's own calls, as
SentiDebiasPLMModule makes them (reference manner/models/baselines/senti_debias_plm_module.py): ``nn.Embedding(padding_idx=0)`` +
``nn.Linear`` + ``tanh`` for the [N, D] sentiment rows, dense ``pad_sequence`` blocks with ``bmm`` for the scores,
``nn.CrossEntropyLoss`` against the explicit one-hot matrix that the module's own loop fills.  No GPU."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import pad_sequence

import debias_step_ref as D
import side_ops_ref as R
from miner_step_ref import to_dense


def _f64(case):
    return {k: v.double() for k, v in case.leaves.items()}


def _split(rows, off):
    o = off.tolist()
    return [rows[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def _module_adversarial_loss(preds, targets):
    """SentiDebiasPLMModule.adversarial_loss, line for line"""
    y_true = torch.zeros(preds.shape, dtype=preds.dtype)
    for i in range(targets.shape[0]):
        y_true[i, targets[i] - 1] = 1.0
    return nn.CrossEntropyLoss()(preds, y_true)


@pytest.mark.parametrize("shape", D.ORTH_SHAPES[:3], ids=str)
def test_orth_loss_is_the_modules_three_terms(shape):
    case = D.orth_case(*shape)
    lv, cls, nh = _f64(case), case.consts["cls"], case.consts["n_hist"]
    senti = lv["table"][cls]
    news, s_news = (lv["rows"][:nh], lv["rows"][nh:]), (senti[:nh], senti[nh:])
    terms = [torch.mean(torch.div(torch.sum(v * s, dim=-1), 1e-8 + torch.linalg.norm(v, dim=1, ord=2) * torch.linalg.norm(s, dim=1, ord=2)), dim=-1)
             for v, s in zip(news, s_news)]
    uf, ua = lv["user_free"], lv["user_aware"]
    user = torch.div(torch.bmm(uf.unsqueeze(dim=1), ua.unsqueeze(dim=-1)).squeeze(dim=1),
                     (1e-8 + torch.linalg.norm(uf, dim=1, ord=2) * torch.linalg.norm(ua, dim=1, ord=2)).unsqueeze(dim=1))
    loss_orth = torch.abs(terms[0]) + torch.abs(terms[1]) + torch.abs(user)
    assert terms[0].dim() == 0 and tuple(user.shape) == (shape[4], 1) and tuple(loss_orth.shape) == (shape[4], 1)
    want, got = torch.mean(loss_orth), D.orth_loss(**lv, cls=cls, n_hist=nh)["loss"]
    assert abs(float(got) - float(want)) <= 1e-13 * abs(float(want))
    assert D.orth_kink_clearance(case) >= 1e-2                     # the rounding of a cosine is near 1e-7


def test_orth_loss_of_an_empty_history_is_nan_and_a_zero_row_sends_nothing_through_its_norm():
    case = D.orth_case(5, 4, 260, 4, 4)
    lv, cls = _f64(case), case.consts["cls"]
    assert torch.isnan(D.orth_loss(**lv, cls=cls, n_hist=0)["loss"]) and torch.isnan(D.orth_loss(**lv, cls=cls, n_hist=9)["loss"])
    zero = D.orth_zero_case()
    ref = zero.ref()
    z, t = D.ZERO_ROW, zero.leaves["table"].double()[zero.consts["cls"][D.ZERO_ROW]]
    want = 0.75 * t / 1e-8 / 5                                     # sign(mean) = +1 for the history; no term through |0|
    assert torch.isfinite(ref["d_rows"]).all() and float((ref["d_rows"][z] - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_class_table_reads_row_zero_as_it_lies_and_sends_it_no_gradient():
    c, e, d = 4, 12, 20
    emb, lin = nn.Embedding(c, e, padding_idx=0).double(), nn.Linear(e, d).double()
    with torch.no_grad():
        emb.weight.copy_(R.randn(1, c, e).double())                # row 0 too
    cls = torch.tensor([0, 3, 1, 0, 2, 2])
    w = emb.weight.detach().clone().requires_grad_(True)
    lw, lb = lin.weight.detach().clone().requires_grad_(True), lin.bias.detach().clone().requires_grad_(True)
    g = R.randn(2, cls.numel(), d).double()
    (torch.tanh(lin(emb(cls))) * g).sum().backward()
    (D.class_table(w, lw, lb)[cls] * g).sum().backward()
    assert torch.equal(torch.tanh(lin(emb(cls))), D.class_table(w, lw, lb)[cls]) and float(emb.weight[0].detach().abs().max()) > 0
    assert float(w.grad[0].abs().max()) == 0.0 and float(w.grad[1:].abs().max()) > 0.0
    for a, b in ((w.grad, emb.weight.grad), (lw.grad, lin.weight.grad), (lb.grad, lin.bias.grad)):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    alone = D.class_table(w, lw, lb)[:1]                           # tanh(W e_0 + b) still reaches the linear
    assert float(torch.autograd.grad(alone.sum(), lb)[0].abs().max()) > 0.0


@pytest.mark.parametrize("shape", D.RAGGED_SHAPES, ids=str)
def test_class_dense_and_class_scores_are_the_dense_blocks_of_the_module(shape):
    dense, scores = D.dense_case(*shape), D.scores_case(*shape)
    table, cs = dense.leaves["table"].double(), dense.consts
    block = pad_sequence(_split(table[cs["cls"]], cs["off"]), batch_first=True)
    got = D.class_dense(table, **cs)["out"]
    assert torch.equal(got[:, :block.shape[1]], block) and float(got[:, block.shape[1]:].abs().sum()) == 0.0 and got.shape[1] == cs["width"]
    lv, cs = _f64(scores), scores.consts
    cand = pad_sequence(_split(lv["table"][cs["cls"]], cs["off"]), batch_first=True)
    want = torch.bmm(lv["user"].unsqueeze(dim=1), cand.permute(0, 2, 1)).squeeze(dim=1)         # DotProduct
    got = to_dense(D.class_scores(**lv, **cs)["scores"], cs["off"], cand.shape[1])
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    counts = cs["off"][1:] - cs["off"][:-1]
    assert float(want[torch.arange(cand.shape[1])[None, :] >= counts[:, None]].abs().sum()) == 0.0     # a zero-padded row scores exactly 0


@pytest.mark.parametrize("shape", D.ADV_SHAPES[:6], ids=str)
def test_adv_loss_is_the_discriminator_and_the_modules_one_hot_loop(shape):
    case = D.adv_case(*shape)
    lv, cls, nh = _f64(case), case.consts["cls"], case.consts["n_hist"]

    def disc(x):
        return F.linear(torch.tanh(F.linear(x, lv["w1"], lv["b1"])), lv["w2"], lv["b2"])
    want = _module_adversarial_loss(disc(lv["rows"][:nh]), cls[:nh]) + _module_adversarial_loss(disc(lv["rows"][nh:]), cls[nh:])
    got = D.adv_loss(**lv, cls=cls, n_hist=nh)["loss"]
    assert abs(float(got) - float(want)) <= 1e-13 * abs(float(want))
    assert int((cls == 0).sum()) > 0                               # the wrap is exercised


def test_class_zero_wraps_onto_the_last_column():
    preds = R.randn(3, 5, 4).double()
    zeros, last = torch.zeros(5, dtype=torch.int64), torch.full((5,), 4)
    want = -torch.log_softmax(preds, dim=1)[:, 3].mean()
    assert abs(float(_module_adversarial_loss(preds, zeros)) - float(want)) <= 1e-14
    case = D.adv_case(5, 4, 260, 33, 4)
    lv = _f64(case)
    a, b = D.adv_loss(**lv, cls=torch.zeros(9, dtype=torch.int64), n_hist=5)["loss"], D.adv_loss(**lv, cls=torch.full((9,), 4), n_hist=5)["loss"]
    assert torch.equal(a, b) and torch.equal(_module_adversarial_loss(preds, zeros), _module_adversarial_loss(preds, last))


def test_generator_lines_are_the_modules_sum():
    cs = D.step_consts()
    nh, t, d, b = int(cs["hist_off"][-1]), int(cs["cand_off"][-1]), 16, len(D.STEP_HIST)
    table = torch.tanh(R.randn(1, D.STEP_CLASSES, d).double())
    rows = D.step_rows(d, cs, table).double()
    hist, cand = rows[:nh], rows[nh:]
    uf, ua = R.randn(2, b, d).double(), R.randn(3, b, d).double()
    disc = [R.randn(4, D.STEP_H, d).double(), R.randn(5, D.STEP_H).double(), R.randn(6, D.STEP_CLASSES, D.STEP_H).double(), R.randn(7, D.STEP_CLASSES).double()]
    sh, sc = table[cs["cls_hist"]], table[cs["cls_cand"]]
    got = D.generator_lines(hist, cand, uf, ua, sh, sc, *disc, cs["cls_hist"], cs["cls_cand"], cs["labels"], cs["cand_off"], cs["c_max"])
    cand_dense, senti_dense = to_dense(cand, cs["cand_off"], cs["c_max"]), to_dense(sc, cs["cand_off"], cs["c_max"])
    free = torch.bmm(uf.unsqueeze(dim=1), cand_dense.permute(0, 2, 1)).squeeze(dim=1)
    combined = free + torch.bmm(ua.unsqueeze(dim=1), senti_dense.permute(0, 2, 1)).squeeze(dim=1)
    orth = D.orth_loss(rows, table, uf, ua, torch.cat((cs["cls_hist"], cs["cls_cand"])), nh)["loss"]

    def pred(x):
        return F.linear(torch.tanh(F.linear(x, disc[0], disc[1])), disc[2], disc[3])
    adv = _module_adversarial_loss(pred(hist), cs["cls_hist"]) + _module_adversarial_loss(pred(cand), cs["cls_cand"])
    y_true = to_dense(cs["labels"].double(), cs["cand_off"], cs["c_max"])
    want = nn.CrossEntropyLoss()(combined, y_true) + D.BETA * orth - D.ALPHA * adv
    assert abs(float(got["loss"]) - float(want)) <= 1e-12 * abs(float(want)) and abs(float(got["orth"]) - float(orth)) <= 1e-13
    assert float((got["combined"] - combined).abs().max()) <= 1e-12 and float((got["free"] - free).abs().max()) <= 1e-12
    d_loss = D.adv_loss(rows, *disc, torch.cat((cs["cls_hist"], cs["cls_cand"])), nh)["loss"]
    assert abs(float(d_loss) - float(adv)) <= 1e-13 * abs(float(adv))


def test_every_measured_case_is_settled():
    for case in D.all_measured_cases() + [D.orth_zero_case()]:
        for k, v in case.bars().items():
            assert v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP, (case, k, v)
        assert set(case.ref()) >= {"d_" + n for n in case.leaves}


def test_library_exports_the_debias_entries_under_abi_8():
    from manner_amd import _lib
    lib = _lib.load()
    assert lib.manner_hip_abi_version() == 8
    for name in ("manner_hip_orth_loss", "manner_hip_orth_loss_backward", "manner_hip_class_dense", "manner_hip_class_dense_backward",
                 "manner_hip_class_scores", "manner_hip_class_scores_backward", "manner_hip_adv_loss", "manner_hip_adv_loss_backward",
                 "manner_hip_orth_loss_workspace_bytes", "manner_hip_orth_loss_backward_workspace_bytes",
                 "manner_hip_class_dense_backward_workspace_bytes", "manner_hip_class_scores_workspace_bytes", "manner_hip_adv_loss_workspace_bytes",
                 "manner_hip_adv_loss_backward_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name in _lib.header_symbols(), name
    assert lib.manner_hip_orth_loss_workspace_bytes(10, 3) >= 52 and lib.manner_hip_orth_loss_backward_workspace_bytes(100, 768, 4) >= 4 * 4 * 769 * 4
    assert lib.manner_hip_orth_loss_backward_workspace_bytes(100, 768, 65) == 0
    assert lib.manner_hip_adv_loss_backward_workspace_bytes(100, 768, 400, 4) >= 100 * 400 * 4 + 768 * 400 * 4
    assert lib.manner_hip_adv_loss_backward_workspace_bytes(100, 768, 1028, 4) == 0 and lib.manner_hip_adv_loss_backward_workspace_bytes(100, 768, 400, 65) == 0
    from manner_amd import hip, hotpath, train
    for mod, names in ((hip, ("orth_loss", "class_dense", "class_scores", "adv_loss")), (train, ("orth_loss", "class_dense", "class_scores", "adv_loss", "class_table")),
                       (hotpath, ("senti_debias_forward", "senti_debias_generator_step", "senti_debias_discriminator_step"))):
        assert all(callable(getattr(mod, n, None)) for n in names), mod
