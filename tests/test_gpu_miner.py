"""The MINER baseline's kernels (csrc/poly.hip) and mirror classes against the float64 restatements of tests/miner_ref.py, at the
smallest shapes that take every loop twice and fire every guard: poly attention forward and backward (64-slot trips of the softmax,
16-code workgroups, 64-wide trips over Q and D, the row groups of the weight gradients, S at its bound), the target-aware mixture
(8-candidate tiles, K past half a wave, zero-padded rows), the batched dot product on the permuted view, MINERNewsEncoder on the
tiny preset, and the operator lines of MINERModule.forward over the mirror classes.

Everything with tanh / exp / erf inside is held to the MEASURED bar, the dot product to the DERIVED bar (tests/side_ops_ref.py);
every test prints its errors next to the bars and records them with ``measured`` (profiles/miner/measured_tolerances.json is that
record from an MI355X)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import miner_ref as M
import side_ops_ref as R
from manner_amd import hip, train
from manner_amd.config import PRESETS
from manner_amd.models.components.attention import PolyAttention, TargetAwareAttention
from manner_amd.models.components.click_predictors import DotProduct
from manner_amd.models.components.news_encoder import MannerTextEncoder, MINERNewsEncoder
from manner_amd.weights import make_plm_weights
from test_gpu_side_ops import _hold_derived, _hold_measured, _run
from test_oracle_golden import compare_train_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ poly attention
def _poly(x, lin_w, codes, mask, bias=None):
    return {"out": train.poly_attention(x, mask, lin_w, codes, bias)}


@pytest.mark.parametrize("shape", M.POLY_SHAPES, ids=lambda s: "B{}-S{}-D{}-Q{}-K{}-T{}".format(*s))
def test_poly_attention_forward_and_backward(shape, measured):
    case = M.poly_case(*shape)
    got = _run(case, _poly)
    _hold_measured(case, got, measured)
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    cs = {k: v.to(DEV) for k, v in case.consts.items()}
    again = hip.poly_attention(lv["x"], cs["mask"], lv["lin_w"], lv["codes"], cs.get("bias"))     # the inference wrapper: the same kernels
    assert torch.equal(again.cpu(), got["out"])
    assert all(torch.equal(v, got[k]) for k, v in _run(case, _poly).items())                       # fixed-order reductions: the same bits


def test_poly_attention_user_without_history(measured):
    """an all-false mask: every logit is 1e-30, the weights are uniform and finite, no logit receives a gradient"""
    case = M.poly_case(2, 9, 64, 24, 5, 0, empty_user=0)
    got = _run(case, _poly)
    _hold_measured(case, got, measured)
    x = case.leaves["x"]
    assert torch.allclose(got["out"][0], x[0].mean(0).expand(5, 64), atol=1e-6)


def test_poly_attention_takes_a_byte_mask_and_refuses_a_bias_that_needs_a_gradient():
    case = M.poly_case(*M.POLY_SHAPES[1])
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    mask, bias = case.consts["mask"].to(DEV), case.consts["bias"].to(DEV)
    a = hip.poly_attention(lv["x"], mask, lv["lin_w"], lv["codes"], bias)
    assert torch.equal(a, hip.poly_attention(lv["x"], mask.to(torch.uint8), lv["lin_w"], lv["codes"], bias))
    with pytest.raises(RuntimeError, match="no gradient is built for `bias`"):
        train.poly_attention(lv["x"], mask, lv["lin_w"], lv["codes"], bias.clone().requires_grad_(True))


@pytest.mark.parametrize("shape,limit", [((1, 257, 8, 4, 2), r"S=257 unsupported \(S <= 256\)"), ((1, 4, 8, 4, 65), r"K=65 unsupported \(K <= 64\)"),
                                         ((1, 4, 8, 513, 2), r"Q=513 unsupported \(Q <= 512\)"), ((1, 4, 1028, 4, 2), r"D=1028 unsupported \(D <= 1024\)")],
                         ids=["S257", "K65", "Q513", "D1028"])
def test_poly_attention_refuses_shapes_past_its_bounds(shape, limit):
    b, s, d, q, k = shape
    x, w, codes = R.randn(1, b, s, d).to(DEV), R.randn(2, q, d).to(DEV), R.randn(3, k, q).to(DEV)
    mask = torch.ones(b, s, dtype=torch.bool, device=DEV)
    with pytest.raises(RuntimeError, match="poly_attention: " + limit):
        hip.poly_attention(x, mask, w, codes)
    with pytest.raises(RuntimeError, match="poly_attention: " + limit):
        train.poly_attention(x.requires_grad_(True), mask, w, codes)
    lib = hip._lib.load()
    g, dx, dw, dc = torch.zeros(b, k, d, device=DEV), torch.empty_like(x), torch.empty_like(w), torch.empty_like(codes)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="poly_attention_backward: " + limit):
        hip._lib.check(lib.manner_hip_poly_attention_backward(hip._ptr(x), hip._ptr(mask), hip._ptr(w), hip._ptr(codes), hip._ptr(None), 0, hip._ptr(g),
                                                              b, s, d, q, k, hip._ptr(dx), hip._ptr(dw), hip._ptr(dc), hip._ptr(ws), ws.numel(),
                                                              hip._stream()))
    # the library is still usable
    case = M.poly_case(*M.POLY_SHAPES[4])
    assert torch.isfinite(_run(case, _poly)["out"]).all()


# ------------------------------------------------------------------------------------------------ target-aware mixture
def _target(query, key, value, lin_w):
    return {"out": train.target_attention(query, key, value, lin_w)}


@pytest.mark.parametrize("shape", M.TARGET_SHAPES, ids=lambda s: "B{}-K{}-C{}-D{}-pad{}".format(*s))
def test_target_attention_forward_and_backward(shape, measured):
    case = M.target_case(*shape)
    got = _run(case, _target)
    _hold_measured(case, got, measured)
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    assert torch.equal(hip.target_attention(lv["query"], lv["key"], lv["value"], lv["lin_w"]).cpu(), got["out"])
    assert all(torch.equal(v, got[k]) for k, v in _run(case, _target).items())
    if shape[4]:                                                 # zero-padded candidate rows: uniform weights times zero values
        assert float(got["out"][1:, -shape[4]:].abs().max()) == 0.0


@pytest.mark.parametrize("shape,limit", [((1, 65, 3, 8), r"K=65 unsupported \(K <= 64\)"), ((1, 4, 3, 1028), r"D=1028 unsupported \(D <= 1024\)")],
                         ids=["K65", "D1028"])
def test_target_attention_refuses_shapes_past_its_bounds(shape, limit):
    b, k, c, d = shape
    q, key, v, w = R.randn(1, b, k, d).to(DEV), R.randn(2, b, c, d).to(DEV), R.randn(3, b, c, k).to(DEV), R.randn(4, d, d).to(DEV)
    with pytest.raises(RuntimeError, match="target_attention: " + limit):
        hip.target_attention(q, key, v, w)


# ------------------------------------------------------------------------------------------------ batched dot product
@pytest.mark.parametrize("shape", M.BMM_SHAPES, ids=lambda s: "B{}-M{}-D{}-N{}".format(*s))
def test_batched_dot_product_on_the_permuted_view(shape, measured):
    """DotProduct as MINERModule.forward calls it: [B, C, D] times the permuted view of [B, K, D], read in place, through the module"""
    case = M.bmm_case(*shape)
    module = DotProduct()
    got = _run(case, lambda a, rows: {"out": module(a, rows.permute(0, 2, 1))})
    _hold_derived(case, got, measured)
    a, rows = case.leaves["a"].to(DEV), case.leaves["rows"].to(DEV)
    with torch.no_grad():
        assert torch.equal(module(a, rows.permute(0, 2, 1)).cpu(), got["out"])                     # the inference route
        dense = module(a, rows.permute(0, 2, 1).contiguous())                                      # a contiguous [B, D, N] operand
    assert R.derived_ratio(dense.cpu().numpy(), case.terms()["out"][0], case.terms(absolute=True)["out"][0], shape[2]) <= 1.0


def test_dot_product_with_one_row_keeps_its_kernel_and_its_shape():
    user, rows = R.randn(21, 5, 1, 96).to(DEV), R.randn(22, 5, 7, 96).to(DEV)
    out = DotProduct()(user, rows.permute(0, 2, 1))
    assert out.shape == (5, 7) and torch.equal(out, hip.dot(user, rows.permute(0, 2, 1)))
    ur = user.clone().requires_grad_(True)
    assert torch.equal(DotProduct()(ur, rows.permute(0, 2, 1)).detach(), out)
    with pytest.raises(AssertionError):                          # the one-row wrapper itself still takes one row only: M > 1 is routed past it
        hip.dot(R.randn(23, 5, 3, 96).to(DEV), rows.permute(0, 2, 1))


# ------------------------------------------------------------------------------------------------ MINERNewsEncoder
@pytest.fixture(scope="module")
def miner_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "miner.npz"))
    return z, json.loads(str(z["meta"]))["encoder"]


def _encoder(z, meta, cls=MINERNewsEncoder, **kw):
    cfg = PRESETS[meta["preset"]]
    w = make_plm_weights(cfg, seed=meta["seed"], std=meta["std"], with_pooler=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = cls(plm_model=meta["preset"], frozen_layers=meta["frozen_layers"], dropout_probability=0.0, **kw)
    missing, unexpected = enc.plm_model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not unexpected and all(k.startswith("pooler.") for k in missing)
    enc.plm_model.hidden_dropout_prob = enc.plm_model.attention_probs_dropout_prob = 0.0           # the golden's HF config
    if getattr(enc, "apply_reduce_dim", False):
        enc.reduce_dim.load_state_dict({"weight": torch.from_numpy(z["enc_reduce_w"]), "bias": torch.from_numpy(z["enc_reduce_b"])})
    return enc.to(DEV), cfg


def _batch(z):
    return {"input_ids": torch.from_numpy(z["enc_ids"]).to(DEV), "attention_mask": torch.from_numpy(z["enc_mask"]).to(DEV)}


def test_miner_news_encoder_eval_is_the_cls_vector_then_the_linear(miner_golden, measured):
    z, meta = miner_golden
    kw = dict(apply_reduce_dim=True, text_embedding_dim=128, news_embedding_dim=meta["news_embedding_dim"])
    enc, _ = _encoder(z, meta, **kw)
    plain, _ = _encoder(z, meta, **dict(kw, apply_reduce_dim=False))
    text, _ = _encoder(z, meta, cls=MannerTextEncoder)
    with torch.no_grad():
        out, cls, cls_text = enc.eval()(_batch(z)), plain.eval()(_batch(z)), text.eval()(_batch(z))
    assert torch.equal(cls, cls_text)                                                # apply_reduce_dim=False: the [CLS] vector itself
    assert np.abs(cls.cpu().numpy() - z["enc_cls_eval"]).max() < 1e-4 and np.abs(out.cpu().numpy() - z["enc_out_eval"]).max() < 1e-4
    c, w, b = cls.double().cpu().numpy(), z["enc_reduce_w"].astype(np.float64), z["enc_reduce_b"].astype(np.float64)
    ratio = R.derived_ratio(out.cpu().numpy(), c @ w.T + b, np.abs(c) @ np.abs(w).T + np.abs(b), c.shape[1] + 1)
    print(f"MINERNewsEncoder eval: error / derived bound = {ratio:.3f} (bar 1)")
    measured(out_over_bound=ratio, bar=1.0)
    assert ratio <= 1.0
    assert sorted({k.split(".")[0] for k in enc.state_dict()}) == ["plm_model", "reduce_dim"]


def test_miner_news_encoder_training_matches_reference(miner_golden):
    """train() with every dropout probability 0: outputs within 1e-4 and every gradient within 1e-3 of its tensor's largest entry —
    the tolerances of test_gpu_train.py::test_train_gradients_match_reference — incl. reduce_dim's and the frozen layer's None"""
    z, meta = miner_golden
    enc, _ = _encoder(z, meta, apply_reduce_dim=True, text_embedding_dim=128, news_embedding_dim=meta["news_embedding_dim"])
    enc.train_precision = "fp32"
    out = enc.train()(_batch(z))
    assert np.abs(out.detach().cpu().numpy() - z["enc_out"]).max() < 1e-4
    (out * torch.from_numpy(z["enc_R"]).to(DEV)).sum().backward()
    hip.check_status(DEV)
    zenc = {k[4:]: z[k] for k in z.files if k.startswith("enc_")}
    expect = {k[len("grad:"):]: v for k, v in zenc.items() if k.startswith("grad:")}
    grads = {k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in enc.plm_model.named_parameters()}
    compare_train_grads(grads, zenc, meta, expect, rel=1e-3)
    for name, p in (("w", enc.reduce_dim.weight), ("b", enc.reduce_dim.bias)):
        ref = z["enc_d_reduce_" + name]
        assert np.abs(p.grad.cpu().numpy() - ref).max() <= 1e-3 * np.abs(ref).max(), name


# ------------------------------------------------------------------------------------------------ MINERModule.forward, restated
@pytest.mark.parametrize("score_type", M.SCORE_TYPES)
def test_miner_forward_over_the_mirror_classes(score_type, measured):
    """the operator lines of MINERModule.forward (baselines/miner_module.py:183-212) over PolyAttention, DotProduct and
    TargetAwareAttention of this package against the same lines over the float64 restatements"""
    case = M.miner_case(score_type)
    _, _, d, q, k, _, _ = M.MINER_SHAPE
    user_encoder, click_predictor = PolyAttention(input_embed_dim=d, num_context_codes=k, context_code_dim=q).to(DEV), DotProduct()
    target = TargetAwareAttention(input_embed_dim=d).to(DEV)
    with torch.no_grad():
        user_encoder.linear.weight.copy_(case.leaves["poly_w"])
        user_encoder.context_codes.copy_(case.leaves["codes"])
        target.linear.weight.copy_(case.leaves["target_w"])
    hist, cand = (case.leaves[n].to(DEV).requires_grad_(True) for n in ("hist", "cand"))
    user_vector = user_encoder(clicked_news_vector=hist, attn_mask=case.consts["mask"].to(DEV), bias=case.consts["bias"].to(DEV))
    scores = click_predictor(cand, user_vector.permute(0, 2, 1))
    if score_type == "max":
        scores = scores.max(dim=2)[0]
    elif score_type == "mean":
        scores = scores.mean(dim=2)
    else:
        scores = target(query=user_vector, key=cand, value=scores)
    ((scores * case.upstream["scores"].to(DEV)).sum() + (user_vector * case.upstream["user"].to(DEV)).sum()).backward()
    params = {"poly_w": user_encoder.linear.weight, "codes": user_encoder.context_codes, "target_w": target.linear.weight, "hist": hist, "cand": cand}
    got = {"user": user_vector.detach().cpu(), "scores": scores.detach().cpu()}
    got.update({"d_" + n: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu() for n, p in params.items()})
    _hold_measured(case, got, measured)
