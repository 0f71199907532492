"""The f32 side operators against the float64 restatements of tests/side_ops_ref.py, at the smallest shapes that take every
kernel loop a second time and fire every guard: the training scorer and loss (train.hip), nn.Linear forward and backward with its
passes over O and its 128 KiB of LDS, the pooler backward up to its S bound, every head dim of the axis-0 attention dispatch in
both columns of its key tiles and the 256-row block, the embedding and the flat dropout past its grid cap.

Pure sums of products are held to the DERIVED bar, everything with exp / tanh / log inside to the MEASURED bar (8 x the error of
the float32 CPU evaluation of the same restatement); both come from the reference side only.  Every test prints its errors next
to the bars and records them with ``measured`` (profiles/side_ops/measured_tolerances.json is that record from an MI355X)."""
import ctypes as C

import numpy as np
import pytest
import torch

import side_ops_ref as R
from manner_amd import _lib, hip, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(case, fn):
    return R.evaluate(fn, case.leaves, case.consts, case.upstream, torch.float32, DEV)


def _hold_derived(case, got, measured, keys=None):
    ref, absolute = case.terms(), case.terms(absolute=True)
    worst = {}
    for k in keys or sorted(ref):
        assert tuple(got[k].shape) == tuple(ref[k][0].shape), (case, k)
        worst[k] = R.derived_ratio(got[k].numpy(), ref[k][0], absolute[k][0], ref[k][1])
        print(f"{case} {k}: error / derived bound = {worst[k]:.3f} (bar 1)")
    measured(**{f"{k}_over_bound": v for k, v in worst.items()}, bar=1.0)
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (case, bad)


def _hold_measured(case, got, measured, keys=None):
    ref, bars = case.ref(torch.float64), case.bars()
    rec, bad = {}, {}
    for k in keys or sorted(ref):
        assert tuple(got[k].shape) == tuple(ref[k].shape) and torch.isfinite(got[k]).all(), (case, k)
        err = R.rel_to_max(got[k], ref[k])
        print(f"{case} {k}: error {err:.3e}  cpu f32 {bars[k]['cpu_f32']:.3e}  bar {bars[k]['bar']:.3e}")
        rec.update({f"{k}_err": err, f"{k}_cpu_f32": bars[k]["cpu_f32"], f"{k}_bar": bars[k]["bar"]})
        if not err <= bars[k]["bar"]:
            bad[k] = (err, bars[k]["bar"])
    measured(**rec)
    assert not bad, (case, bad)


# ------------------------------------------------------------------------------------------------ scorer
def _late_fusion(hist, cand, hist_off, cand_off):
    scores = train.late_fusion_scores(hist, hist_off, cand, cand_off)
    b, d = hist_off.numel() - 1, hist.shape[1]
    user, again = torch.empty((b, d), device=DEV), torch.empty(cand.shape[0], device=DEV)      # `user` is what the backward reads
    _lib.check(_lib.load().manner_hip_late_fusion_train_forward(hip._ptr(hist.detach()), hip._ptr(hist_off), hip._ptr(cand.detach()),
                                                                hip._ptr(cand_off), b, d, hip._ptr(user), hip._ptr(again), hip._stream()))
    assert torch.equal(again, scores.detach())
    return {"user": user, "scores": scores}


@pytest.mark.parametrize("d", R.SCORER_D)
def test_late_fusion_scorer_forward_and_backward(d, measured):
    case = R.scorer_case(d)
    _hold_derived(case, _run(case, _late_fusion), measured)


@pytest.mark.parametrize("permuted", [False, True], ids=["contiguous", "rows"])
@pytest.mark.parametrize("c", R.DOT_C)
@pytest.mark.parametrize("d", R.DOT_D)
def test_dot_product_forward_and_backward(d, c, permuted, measured):
    case = R.dot_case(d, c, permuted)
    got = _run(case, lambda user, cand, permuted: {"out": train.dot(user, cand.permute(0, 2, 1) if permuted else cand)})
    _hold_derived(case, got, measured)


# ------------------------------------------------------------------------------------------------ losses
def _model_step_loss(scores, labels, cand_off, supcon, temperature, c_max):
    loss, per = train.model_step_loss(scores, labels, cand_off, supcon=supcon, temperature=temperature, c_max=c_max)
    return {"loss": loss, "per": per}


@pytest.mark.parametrize("supcon", [True, False], ids=["supcon", "ce"])
@pytest.mark.parametrize("b", R.LOSS_B)
def test_model_step_loss_and_gradient(b, supcon, measured):
    case = R.loss_case(b, supcon)
    got = _run(case, _model_step_loss)
    if supcon:                                                   # the non-zero reducer's members are the reference's
        assert torch.equal(got["per"] > 0, case.ref()["per"] > 0)
    _hold_measured(case, got, measured)


def _supcon_embeddings(emb, labels, temperature):
    loss, per = train.supcon_embedding_loss(emb, labels, temperature)
    return {"loss": loss, "per": per}


@pytest.mark.parametrize("kind", R.SUPCON_LABELS)
@pytest.mark.parametrize("d", R.SUPCON_D)
@pytest.mark.parametrize("n", R.SUPCON_N)
def test_supcon_embedding_loss_and_gradient(n, d, kind, measured):
    case = R.supcon_case(n, d, kind)
    _hold_measured(case, _run(case, _supcon_embeddings), measured)


# ------------------------------------------------------------------------------------------------ nn.Linear, pooler
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("r,k,o", R.LINEAR_SHAPES)
def test_linear_forward_and_backward(r, k, o, with_bias, measured):
    case = R.linear_case(r, k, o, with_bias)
    _hold_derived(case, _run(case, lambda x, weight, bias=None: {"y": train.linear(x, weight, bias)}), measured)


@pytest.mark.parametrize("b,s,d,q", R.POOL_SHAPES)
def test_additive_pool_strict_forward_and_backward(b, s, d, q, measured):
    case = R.pool_case(b, s, d, q)
    _hold_measured(case, _run(case, lambda x, lin_w, lin_b, query: {"out": train.additive_pool(x, lin_w, lin_b, query)}), measured)


def test_additive_pool_backward_refuses_rows_past_its_bound():
    case = R.pool_case(2, 1024, 64, 16)
    lv = {k: v.to(DEV).requires_grad_(True) for k, v in case.leaves.items()}
    lv["x"] = R.randn(7, 2, 1025, 64).to(DEV).requires_grad_(True)
    out = train.additive_pool(lv["x"], lv["lin_w"], lv["lin_b"], lv["query"])          # the forward has no such bound
    with pytest.raises(RuntimeError, match=r"additive_pool_backward: bad argument \(S <= 1024\)"):
        out.sum().backward()


# ------------------------------------------------------------------------------------------------ axis-0 attention
def _train_mha(x, in_w, in_b, out_w, out_b, heads):
    return {"out": train.mha_axis0(x, in_w, in_b, out_w, out_b, heads)}


def _hip_mha(case):
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    return {"out": hip.mha_axis0(lv["x"], lv["in_w"], lv["in_b"], lv["out_w"], lv["out_b"], case.consts["heads"]).cpu()}


@pytest.mark.parametrize("l0", R.AXIS0_L0)
@pytest.mark.parametrize("dh", R.AXIS0_DH)
def test_axis0_attention_every_head_dim_forward_and_backward(dh, l0, measured):
    """axis0.hip's axis0_fwd / bwd_q / bwd_kv at every case of the dispatch: rows below, at and past each key tile and past
    the 256-row block, with the two Linear projections around them"""
    case = R.axis0_case(l0, 3, 2 * dh, 2)
    _hold_measured(case, _run(case, _train_mha), measured)


@pytest.mark.parametrize("l0", R.AXIS0_L0)
@pytest.mark.parametrize("dh", R.AXIS0_DH)
def test_axis0_attention_every_head_dim_inference_kernel(dh, l0, measured):
    """axis0.hip's axis0_fwd_kernel on the inference key tiles (other than the training ones at head dims 16, 48, 64) through hip.mha_axis0"""
    case = R.axis0_case(l0, 3, 2 * dh, 2)
    _hold_measured(case, _hip_mha(case), measured, keys=("out",))


@pytest.mark.parametrize("l0,b1", R.AXIS0_GEMM_ROUTE)
def test_axis0_attention_on_the_padded_panel_gemm_route(l0, b1, measured):
    """E = 128: both projections of hip.mha_axis0 go through the f32 GEMM on a zero-padded copy of the rows (36 rows: one partial
    panel; 387 rows: three full panels and a partial one); the training path at the same shape keeps the VALU Linear"""
    case = R.axis0_case(l0, b1, 128, 2)
    _hold_measured(case, _hip_mha(case), measured, keys=("out",))
    _hold_measured(case, _run(case, _train_mha), measured)


@pytest.mark.parametrize("d,heads", R.ENTITY_DIMS)
@pytest.mark.parametrize("n", R.ENTITY_N)
def test_entity_encode(n, d, heads, measured):
    case = R.entity_case(n, d, heads)
    w = [case.leaves[k.replace(".", "__")].to(DEV) for k in R.ENTITY_KEYS]
    out = hip.entity_encode(case.consts["ids"].to(DEV), *w, heads)
    hip.check_status(DEV)
    _hold_measured(case, {"out": out.cpu()}, measured)


def test_axis0_attention_refuses_an_unsupported_head_dim():
    case = R.axis0_case(33, 3, 16, 2)
    x = R.randn(5, 9, 3, 24).to(DEV)
    w = [R.randn(6, 72, 24).to(DEV), R.randn(7, 72).to(DEV), R.randn(8, 24, 24).to(DEV), R.randn(9, 24).to(DEV)]
    msg = r"axis-0 attention: head_dim 12 unsupported \(4, 8, 10, 16, 32, 48, 64\)"
    with pytest.raises(RuntimeError, match=msg):
        hip.mha_axis0(x, *w, 2)
    with pytest.raises(RuntimeError, match=msg):
        train.mha_axis0(x, *w, 2)
    with pytest.raises(RuntimeError, match=msg):                 # the backward entry point has the same dispatch
        qkv, g = R.randn(10, 9, 3, 72).to(DEV), R.randn(11, 9, 3, 24).to(DEV)
        dqkv, stats = torch.empty_like(qkv), torch.empty(9 * 3 * 2 * 3, device=DEV)
        _lib.check(_lib.load().manner_hip_axis0_attention_backward(hip._ptr(qkv), hip._ptr(g), 9, 3, 24, 2, hip._ptr(dqkv), hip._ptr(stats),
                                                                   hip._stream()))
    # the library is still usable
    assert torch.isfinite(_hip_mha(case)["out"]).all()


# ------------------------------------------------------------------------------------------------ embedding, dropout
@pytest.mark.parametrize("padding_idx", [0, None])
@pytest.mark.parametrize("d", R.EMBEDDING_D)
def test_embedding_forward_and_table_gradient(d, padding_idx, measured):
    case = R.embedding_case(d, padding_idx)
    got = _run(case, lambda table, ids, padding_idx: {"out": train.embedding(ids, table, padding_idx)})
    hip.check_status(DEV)
    assert torch.equal(got["out"], case.leaves["table"][case.consts["ids"]])            # a gather: every bit
    _hold_derived(case, got, measured, keys=("d_table",))
    assert (float(got["d_table"][0].abs().max()) == 0.0) == (padding_idx == 0)


def test_dropout_past_the_grid_cap(measured):
    """n = 8192 * 256 + 1000: the 8192-block grid strides, and the last stride is a partial one"""
    n, p, seed, site = R.DROPOUT_N, R.DROPOUT_P, 11, 3
    x = R.randn(12, n).to(DEV).requires_grad_(True)
    y = train.dropout(x, p, seed=seed, site=site)
    keep = train.dropout_mask(seed, site, p, n, DEV).float()
    dropped = float((keep == 0).float().mean())
    print(f"dropout n={n}: dropped fraction {dropped:.5f} (p = {p})")
    measured(dropped_fraction=dropped, p=p)
    assert torch.equal(y.detach(), x.detach() * keep / 0.8)
    g = R.randn(13, n).to(DEV)
    (y * g).sum().backward()
    assert torch.equal(x.grad, g * keep / 0.8)
    assert abs(dropped - p) < 5 * (p * (1 - p) / n) ** 0.5       # five standard deviations of a fair draw of n bits
