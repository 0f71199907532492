"""The kernels of csrc/miner.hip — MINERModule's category bias, the max / mean aggregation over the context codes, the disagreement
loss — and ``hotpath.miner_forward`` / ``miner_train_step`` against the float64 restatements of tests/miner_step_ref.py, at the
smallest shapes that take every loop twice and fire every guard.

Bars (tests/side_ops_ref.py, used as they are): DERIVED for the bias (n = 2 Dc + T, the absolute-value sum over the non-own columns;
an entry whose sum is empty must be exactly 0) and for the code scores (n = D for 'max', D + K for 'mean'); MEASURED for the
disagreement loss and the step.  Every test prints its errors next to the bars and records them with ``measured``
(profiles/miner/measured_tolerances_step.json is that record from an MI355X)."""
import pytest
import torch
from torch import nn

import miner_ref as M
import miner_step_ref as S
import side_ops_ref as R
from manner_amd import hip, hotpath, train
from manner_amd.models.components.attention import PolyAttention, TargetAwareAttention
from test_gpu_miner import _encoder, miner_golden  # noqa: F401  (the tiny-preset encoder of the leaf tests and its fixture)
from test_gpu_side_ops import _hold_derived, _hold_measured, _run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ category bias
def _bias(case, p=0.0, seeds=(0, 0)):
    a = case.args(DEV, torch.float32)
    return hip.miner_category_bias(a["hist_cat"], a["cand_cat"], a["table"], a["hist_off"], a["cand_off"], a["width"], p=p, seeds=seeds)


def _hold_bias(case, got, ref, absolute, measured, tag=""):
    got = got.cpu()
    assert tuple(got.shape) == tuple(ref.shape) == (len(case.hist_off) - 1, case.width, 1)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), case   # a NaN is compared by position
    ok = ~torch.isnan(ref)
    ratio = R.derived_ratio(got[ok].numpy(), ref[ok].numpy(), absolute[ok.numpy()], case.n)
    print(f"bias {case}{tag}: error / derived bound = {ratio:.3f} (bar 1, n = {case.n})")
    measured(**{f"bias{tag}_over_bound": ratio}, bar=1.0)
    assert ratio <= 1.0, (case, ratio)


@pytest.mark.parametrize("name", list(S.BIAS_CASES))
def test_category_bias(name, measured):
    case = S.BIAS_CASES[name]
    got = _bias(case)
    _hold_bias(case, got, *case.ref(), measured)
    assert torch.equal(got, _bias(case))                           # fixed-order sums: the same bits
    if name == "one-user":
        assert float(got.abs().max()) == 0.0                       # every column is the user's own
    hip.check_status(DEV)


@pytest.mark.parametrize("name", list(S.BIAS_ZERO_ROW_CASES))
def test_category_bias_zero_rows_put_their_nans_where_the_reference_does(name, measured):
    case = S.BIAS_ZERO_ROW_CASES[name]
    _hold_bias(case, _bias(case), *case.ref(), measured)


def test_category_bias_dropout_follows_the_counter_rule(measured):
    case = S.BIAS_CASES["shipped-Dc300"]
    p, seeds = S.BIAS_DROPOUT_P, S.BIAS_DROPOUT_SEEDS
    got = _bias(case, p, seeds)
    _hold_bias(case, got, *case.ref(seeds, p), measured, tag="_dropout")
    assert torch.equal(got, _bias(case, p, seeds)) and not torch.equal(got, _bias(case))
    keep = S.dropout_keeps(seeds, p, case.hist_cat.numel(), case.cand_cat.numel(), case.dc)[1]
    assert torch.equal(train.dropout_mask(seeds[1], S.SITE_CAND, p, keep.numel(), DEV).cpu().bool(), keep.reshape(-1))


def test_category_bias_raises_a_category_outside_the_table_through_the_status_word():
    case = S.BIAS_CASES["Dc5"]
    a = case.args(DEV, torch.float32)
    hip.check_status(DEV)
    bad = a["cand_cat"].clone()
    bad[3] = case.v
    hip.miner_category_bias(a["hist_cat"], bad, a["table"], a["hist_off"], a["cand_off"], a["width"])
    with pytest.raises(RuntimeError, match="index outside the table"):
        hip.check_status(DEV)
    bad = a["hist_cat"].clone()
    bad[0] = -1
    hip.miner_category_bias(bad, a["cand_cat"], a["table"], a["hist_off"], a["cand_off"], a["width"])
    with pytest.raises(RuntimeError, match="index outside the table"):
        hip.check_status(DEV)
    hip.check_status(DEV)


def test_category_bias_refuses_widths_past_its_bounds(measured):
    case = S.BIAS_CASES["Dc5"]
    a = case.args(DEV, torch.float32)
    wide = torch.zeros(case.v, 1028, device=DEV)
    with pytest.raises(RuntimeError, match=r"miner_category_bias: Dc=1028 unsupported \(Dc <= 1024\)"):
        hip.miner_category_bias(a["hist_cat"], a["cand_cat"], wide, a["hist_off"], a["cand_off"], a["width"])
    with pytest.raises(RuntimeError, match=r"miner_category_bias: S=257 unsupported \(S <= 256\)"):
        hip.miner_category_bias(a["hist_cat"], a["cand_cat"], a["table"], a["hist_off"], a["cand_off"], 257)
    _hold_bias(case, _bias(case), *case.ref(), measured)           # the library is still usable


def _poly_with_full_bias(x, lin_w, codes, mask, bias):
    return M.poly_attention(x, lin_w, codes, mask, bias)


def test_poly_attention_takes_the_one_column_bias_for_the_whole_matrix(measured):
    """PolyAttention(bias = the [B, S, 1] kernel output) against the restated PolyAttention fed the reference's [B, S, T] bias"""
    bc = S.BIAS_CASES["shipped-Dc300"]
    b, s, d, q, k = 3, bc.width, 64, 24, 5
    ho = bc.hist_off
    mask = torch.arange(s)[None, :] < (ho[1:] - ho[:-1])[:, None]
    full = S.category_bias_full(**bc.args(dtype=torch.float32))

    def build(salt):
        leaves, _, _ = M.poly_inputs(b, s, d, q, k, 0, salt + 11)
        return R.Case("poly-with-category-bias", _poly_with_full_bias, leaves, {"mask": mask, "bias": full}, None)
    case = R.settled(build)
    module = PolyAttention(input_embed_dim=d, num_context_codes=k, context_code_dim=q).to(DEV)
    with torch.no_grad():
        module.linear.weight.copy_(case.leaves["lin_w"])
        module.context_codes.copy_(case.leaves["codes"])
        out = module(clicked_news_vector=case.leaves["x"].to(DEV), attn_mask=mask.to(DEV), bias=_bias(bc))
    _hold_measured(case, {"out": out.cpu()}, measured)


# ------------------------------------------------------------------------------------------------ scores over the context codes
def _scores(cand, user, cand_off, score_type):
    return {"out": train.miner_code_scores(cand, cand_off, user, score_type)}


@pytest.mark.parametrize("score_type", S.SCORE_TYPES)
@pytest.mark.parametrize("shape", S.SCORE_SHAPES, ids=lambda s: "B{}-K{}-D{}".format(*s[:3]))
def test_code_scores_forward_and_backward(shape, score_type, measured):
    case = S.scores_case(*shape, score_type)
    got = _run(case, _scores)
    _hold_derived(case, got, measured)
    again = hip.miner_code_scores(case.leaves["cand"].to(DEV), case.consts["cand_off"].to(DEV), case.leaves["user"].to(DEV), score_type)
    assert torch.equal(again.cpu(), got["out"])                    # the inference wrapper: the same kernel
    assert all(torch.equal(v, got[k]) for k, v in _run(case, _scores).items())


def test_code_scores_tie_goes_to_the_lowest_code(measured):
    case = S.scores_case(3, 5, 64, (6, 4, 1), "max", True)
    got = _run(case, _scores)
    _hold_derived(case, got, measured)
    assert float(got["d_user"][:, 2].abs().max()) == 0.0 and float(got["d_user"][:, 0].abs().max()) > 0.0


@pytest.mark.parametrize("shape,limit", [((1, 65, 8), r"K=65 unsupported \(K <= 64\)"), ((1, 4, 1028), r"D=1028 unsupported \(D <= 1024\)")],
                         ids=["K65", "D1028"])
def test_code_scores_and_disagreement_refuse_shapes_past_their_bounds(shape, limit):
    b, k, d = shape
    cand, user, off = R.randn(1, 3, d).to(DEV), R.randn(2, b, k, d).to(DEV), torch.tensor([0, 3], device=DEV)
    for score_type in S.SCORE_TYPES:
        with pytest.raises(RuntimeError, match="miner_code_scores: " + limit):
            hip.miner_code_scores(cand, off, user, score_type)
    with pytest.raises(RuntimeError, match="disagreement_loss: " + limit):
        hip.disagreement_loss(user)
    with pytest.raises(ValueError, match="score_type"):
        hip.miner_code_scores(cand, off, user, "weighted")
    ok = S.scores_case(*S.SCORE_SHAPES[0], "mean")
    assert torch.isfinite(_run(ok, _scores)["out"]).all()          # the library is still usable


# ------------------------------------------------------------------------------------------------ disagreement loss
def _disagreement(user):
    return {"loss": train.disagreement_loss(user)}


@pytest.mark.parametrize("shape", S.DISAGREEMENT_SHAPES, ids=lambda s: "B{}-K{}-D{}".format(*s))
def test_disagreement_loss_forward_and_backward(shape, measured):
    case = S.disagreement_case(*shape)
    got = _run(case, _disagreement)
    _hold_measured(case, got, measured)
    assert torch.equal(hip.disagreement_loss(case.leaves["user"].to(DEV)).cpu(), got["loss"])
    assert all(torch.equal(v, got[k]) for k, v in _run(case, _disagreement).items())
    if shape[1] == 1:
        assert float(got["loss"]) == 0.0 and float(got["d_user"].abs().max()) == 0.0


def test_disagreement_loss_zero_row_gets_the_gradient_through_the_epsilon(measured):
    case = S.disagreement_case(3, 5, 64, True)
    got = _run(case, _disagreement)
    _hold_measured(case, got, measured, keys=["loss"])
    bars, parts, ref = S.zero_row_bars(case), S.zero_row_parts(got["d_user"]), S.zero_row_parts(case.ref()["d_user"])
    assert torch.isfinite(got["d_user"]).all() and float(ref["d_user_zero_row"].abs().max()) > 1e5
    rec, bad = {}, {}
    for k in sorted(parts):
        err = R.rel_to_max(parts[k], ref[k])
        print(f"{case} {k}: error {err:.3e}  cpu f32 {bars[k]['cpu_f32']:.3e}  bar {bars[k]['bar']:.3e}")
        rec.update({f"{k}_err": err, f"{k}_cpu_f32": bars[k]["cpu_f32"], f"{k}_bar": bars[k]["bar"]})
        if not err <= bars[k]["bar"]:
            bad[k] = (err, bars[k]["bar"])
    measured(**rec)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ forward and the training step
class _StubEncoder(nn.Module):
    """an embedding lookup on the first token id: the news vectors are the leaves"""

    def __init__(self, rows):
        super().__init__()
        self.weight = nn.Parameter(rows.clone())

    def forward(self, tokens):
        return nn.functional.embedding(tokens["input_ids"][:, 0], self.weight)


def _tokens(ids):
    ids = ids.reshape(-1, 1).to(DEV)
    return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}


def _segments(off):
    counts = (off[1:] - off[:-1])
    return torch.repeat_interleave(torch.arange(len(counts)), counts).to(DEV)


def _step_setup(case, with_max=True, p=0.0):
    lv, cs = case.leaves, case.consts
    _, _, d, q, k, _, _ = M.MINER_SHAPE
    n_hist, n_cand = lv["hist"].shape[0], lv["cand"].shape[0]
    enc = _StubEncoder(torch.cat([lv["hist"], lv["cand"]])).to(DEV)
    user_encoder, target = PolyAttention(input_embed_dim=d, num_context_codes=k, context_code_dim=q).to(DEV), TargetAwareAttention(input_embed_dim=d).to(DEV)
    with torch.no_grad():
        user_encoder.linear.weight.copy_(lv["poly_w"])
        user_encoder.context_codes.copy_(lv["codes"])
        target.linear.weight.copy_(lv["target_w"])
    emb = nn.Embedding.from_pretrained(cs["table"].clone(), freeze=True).to(DEV)
    batch = {"users": torch.arange(len(cs["hist_off"]) - 1, device=DEV), "batch_hist": _segments(cs["hist_off"]), "batch_cand": _segments(cs["cand_off"]),
             "x_hist": {"text": _tokens(torch.arange(n_hist)), "category": cs["hist_cat"].to(DEV)},
             "x_cand": {"text": _tokens(torch.arange(n_hist, n_hist + n_cand)), "category": cs["cand_cat"].to(DEV)},
             "labels": cs["labels"].to(DEV)}
    if with_max:
        batch.update(hist_max=max(S.STEP_HIST), cand_max=max(S.STEP_CAND))
    kw = dict(score_type=cs["score_type"], target_aware_attn=target, category_embedding=emb, category_dropout=nn.Dropout(p))
    return enc, user_encoder, target, batch, kw


@pytest.mark.parametrize("score_type", M.SCORE_TYPES)
def test_miner_train_step_matches_the_restated_step(score_type, measured):
    case = S.step_case(score_type)
    enc, user_encoder, target, batch, kw = _step_setup(case, with_max=False)
    loss, ragged, cand_off = hotpath.miner_train_step(enc, user_encoder, batch, **kw)
    (loss * case.upstream["loss"].to(DEV)).backward()
    hip.check_status(DEV)
    n_hist = case.leaves["hist"].shape[0]
    assert torch.equal(cand_off.cpu(), case.consts["cand_off"]) and not ragged.requires_grad
    grads = {"hist": enc.weight.grad[:n_hist], "cand": enc.weight.grad[n_hist:], "poly_w": user_encoder.linear.weight.grad,
             "codes": user_encoder.context_codes.grad, "target_w": target.linear.weight.grad}
    got = {"loss": loss.detach().cpu(), "scores": ragged.cpu()}
    got.update({"d_" + n: (torch.zeros_like(case.leaves[n]) if g is None else g.detach().cpu()) for n, g in grads.items()})
    assert (grads["target_w"] is not None) == (score_type == "weighted")
    _hold_measured(case, got, measured)


@pytest.mark.parametrize("score_type", M.SCORE_TYPES)
def test_miner_forward_dense_pads_with_exact_zeros(score_type):
    case = S.step_case(score_type)
    enc, user_encoder, _, batch, kw = _step_setup(case)
    with torch.no_grad():
        user_d, dense = hotpath.miner_forward(enc, user_encoder, batch, dense=True, **kw)
        user_r, ragged = hotpath.miner_forward(enc, user_encoder, batch, dense=False, **kw)
    real = torch.arange(max(S.STEP_CAND))[None, :] < torch.tensor(S.STEP_CAND)[:, None]
    assert dense.shape == real.shape and tuple(user_d.shape) == (M.MINER_SHAPE[0], M.MINER_SHAPE[4], M.MINER_SHAPE[2])
    assert torch.equal(user_d, user_r) and torch.equal(dense.cpu()[real], ragged.cpu()) and float(dense.cpu()[~real].abs().sum()) == 0.0
    assert torch.equal(ragged.cpu(), hotpath.miner_train_step(enc, user_encoder, batch, **kw)[1].cpu())       # forward of the step: the same bits
    with pytest.raises(ValueError, match="Invalid method of aggregating scores."):
        hotpath.miner_forward(enc, user_encoder, batch, **dict(kw, score_type="sum"))


def test_category_dropout_draws_two_seeds_in_train_and_none_otherwise():
    case = S.step_case("max")
    enc, user_encoder, _, batch, kw = _step_setup(case, p=S.BIAS_DROPOUT_P)
    drop = kw["category_dropout"]
    cs = case.consts

    def run():
        with torch.no_grad():
            return hotpath.miner_forward(enc, user_encoder, batch, dense=False, **kw)[0]

    torch.manual_seed(5)
    seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2)]
    end = torch.get_rng_state()
    torch.manual_seed(5)
    drop.train()
    got = run()
    assert torch.equal(torch.get_rng_state(), end)                 # history first, then candidates: two draws
    torch.manual_seed(5)
    assert torch.equal(got, run())
    s = max(S.STEP_HIST)
    ho, co = cs["hist_off"].to(DEV), cs["cand_off"].to(DEV)
    bias = hip.miner_category_bias(cs["hist_cat"].to(DEV), cs["cand_cat"].to(DEV), cs["table"].to(DEV), ho, co, s, p=drop.p, seeds=seeds)
    with torch.no_grad():
        hist = hip.to_dense(enc.weight[:int(ho[-1])].detach().contiguous(), ho, s)
        want = user_encoder(clicked_news_vector=hist, attn_mask=(torch.arange(s, device=DEV)[None, :] < (ho[1:] - ho[:-1])[:, None]), bias=bias)
    assert torch.equal(got, want)
    drop.eval()
    before = torch.get_rng_state()
    plain = run()
    assert torch.equal(torch.get_rng_state(), before) and not torch.equal(plain, got)
    drop.train()
    drop.p = 0.0
    assert torch.equal(run(), plain) and torch.equal(torch.get_rng_state(), before)      # train() at p = 0: the bits of eval(), no draw


def test_miner_train_step_over_the_news_encoder(miner_golden):  # noqa: F811
    z, meta = miner_golden
    d, q, k = meta["news_embedding_dim"], 24, 5
    enc, _ = _encoder(z, meta, apply_reduce_dim=True, text_embedding_dim=128, news_embedding_dim=d)
    enc.train_precision = "fp32"
    enc.train()
    ids, mask = torch.from_numpy(z["enc_ids"]).to(DEV), torch.from_numpy(z["enc_mask"]).to(DEV)
    case = S.step_case("mean")
    cs = case.consts
    n_hist, n_cand = int(cs["hist_off"][-1]), int(cs["cand_off"][-1])
    pick_h, pick_c = torch.arange(n_hist, device=DEV) % ids.shape[0], (torch.arange(n_cand, device=DEV) * 2 + 1) % ids.shape[0]
    user_encoder = PolyAttention(input_embed_dim=d, num_context_codes=k, context_code_dim=q).to(DEV)
    emb = nn.Embedding.from_pretrained(cs["table"].clone(), freeze=True).to(DEV)
    batch = {"users": torch.arange(len(S.STEP_HIST), device=DEV), "batch_hist": _segments(cs["hist_off"]), "batch_cand": _segments(cs["cand_off"]),
             "x_hist": {"text": {"input_ids": ids[pick_h], "attention_mask": mask[pick_h]}, "category": cs["hist_cat"].to(DEV)},
             "x_cand": {"text": {"input_ids": ids[pick_c], "attention_mask": mask[pick_c]}, "category": cs["cand_cat"].to(DEV)},
             "labels": cs["labels"].to(DEV), "hist_max": max(S.STEP_HIST), "cand_max": max(S.STEP_CAND)}
    loss, ragged, _ = hotpath.miner_train_step(enc, user_encoder, batch, score_type="mean", category_embedding=emb, category_dropout=nn.Dropout(0.2))
    loss.backward()
    hip.check_status(DEV)
    assert torch.isfinite(loss) and torch.isfinite(ragged).all() and ragged.shape == (n_cand,)
    trained = [p for n, p in enc.plm_model.named_parameters() if p.requires_grad and p.grad is not None]
    assert float(enc.reduce_dim.weight.grad.abs().max()) > 0 and trained and any(float(p.grad.abs().max()) > 0 for p in trained)
    assert float(user_encoder.context_codes.grad.abs().max()) > 0


def test_miner_train_step_reads_nothing_back_from_the_device():
    case = S.step_case("weighted")
    enc, user_encoder, _, batch, kw = _step_setup(case)
    loss, _, _ = hotpath.miner_train_step(enc, user_encoder, batch, **kw)                 # warm-up: first-use allocations and module loads
    loss.backward()
    torch.cuda.synchronize()
    want = loss.detach().clone()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for st in M.SCORE_TYPES:
            loss, _, _ = hotpath.miner_train_step(enc, user_encoder, batch, **dict(kw, score_type=st))
            loss.backward()
            if st == "weighted":
                again = loss.detach()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(again, want)
    hip.check_status(DEV)
