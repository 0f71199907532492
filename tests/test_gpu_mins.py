"""The MINS baseline's kernels (csrc/mins.hip) and mirror classes against the float64 restatement of tests/mins_ref.py, at the smallest
shapes that take every loop twice and fire every guard (mins_ref.CGRU_SHAPES / wide_shapes / USER_SHAPES): the channel GRU at the golden
shape, the shipped width 128, the zero-padded widths 127 and 65, H = 1 and 5, C = 1, B = 1, 9 rows (one past the 8-row tile, which spans
users of different lengths), S = 1, all lengths 1, all lengths S, S = 256, 3285 stacked rows and I != H; the wide attention at head dims
65, 96, 127, 128 over 1, 2, 9, 65 and 257 rows; the user encoder at head dims 4 (narrow attention), 65, 66 and 128.

Every output has sigma / tanh / exp inside: the MEASURED bar of tests/side_ops_ref.py — 8 x the error of the float32 CPU evaluation of the
same restatement.  Tensors the reference makes exactly zero are held to ``not t.any()``.  Every test prints its errors next to the bars
and records them with ``measured`` (profiles/mins/measured_tolerances.json is that record from an MI355X)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import mins_ref as MR
import side_ops_ref as R
from manner_amd import hip, train
from manner_amd.config import PRESETS
from manner_amd.models.components.news_encoder import NAMLCategoryEncoder, NAMLNewsEncoder
from manner_amd.models.components.user_encoder import MINSUserEncoder
from manner_amd.weights import make_mha_pool_weights, make_plm_weights
from test_gpu_caum import _close
from test_gpu_side_ops import _hold_measured, _run
from test_mins_host import golden_case, golden_params, golden_want, rows_of
from test_oracle_golden import compare_train_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
USER_ORDER = MR.MHA_PARAMS + MR.GRU_PARAMS


def _cgru(x, w_ih, w_hh, b_ih, b_hh, *, lengths, channels):
    return {"out": train.channel_gru_last_hidden(x, lengths, w_ih, w_hh, b_ih, b_hh, channels)}


def _wide(x, in_w, in_b, out_w, out_b, heads):
    return {"out": train.mha_axis0_wide(x, in_w, in_b, out_w, out_b, heads)}


def _user(x, in_w, in_b, out_w, out_b, w_ih, w_hh, b_ih, b_hh, pool_w, pool_b, query, *, lengths, channels):
    hidden = train.mins_user(x, lengths, [in_w, in_b, out_w, out_b, w_ih, w_hh, b_ih, b_hh], channels)
    return {"out": train._UnitPool.apply(hidden, query, pool_w, pool_b), "hidden": hidden}


def _on_device(case):
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    cs = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in case.consts.items()}
    return lv, cs


def _same_bits(a, b):
    return all(torch.equal(v, b[k]) for k, v in a.items())


# ------------------------------------------------------------------------------------------------ the channel GRU
@pytest.mark.parametrize("shape", MR.CGRU_SHAPES, ids=lambda s: "B{}-S{}-C{}-I{}-H{}-{}".format(*s))
def test_channel_gru_forward_and_backward(shape, measured):
    case = MR.cgru_case(*shape)
    got = _run(case, _cgru)
    _hold_measured(case, got, measured)
    lv, cs = _on_device(case)
    again = hip.channel_gru_last_hidden(lv["x"], cs["lengths"], *[lv[n] for n in MR.GRU_PARAMS], cs["channels"])      # the inference wrapper
    assert torch.equal(again.cpu(), got["out"])
    assert _same_bits(_run(case, _cgru), got)                                                                        # fixed-order reductions
    lens = case.consts["lengths"]
    for b in range(min(shape[0], 16)):
        assert not got["d_x"][b, int(lens[b]):].any()                                                                # exactly 0 past the length
    # x past the lengths filled with NaN or 1e30 changes no bit
    for fill in (float("nan"), 1e30):
        x = case.leaves["x"].clone()
        for b in range(x.shape[0]):
            x[b, int(lens[b]):] = fill
        filled = R.evaluate(_cgru, dict(case.leaves, x=x), case.consts, case.upstream, torch.float32, DEV)
        assert _same_bits(filled, got), fill
        assert torch.equal(hip.channel_gru_last_hidden(x.to(DEV), cs["lengths"], *[lv[n] for n in MR.GRU_PARAMS], cs["channels"]).cpu(), got["out"])
    hip.check_status(DEV)


def test_channel_gru_agrees_with_the_per_channel_entry(measured):
    """``gru_last_hidden`` on every channel view — autograd adds its per-channel weight gradients — against the single-launch entry:
    outputs and gradients are held to agree within the MEASURED bar of the case"""
    c, i = MR.PER_CHANNEL_SHAPE[2:4]
    case = MR.cgru_case(*MR.PER_CHANNEL_SHAPE)
    got = _run(case, _cgru)
    _hold_measured(case, got, measured)

    def per_channel(x, w_ih, w_hh, b_ih, b_hh, *, lengths, channels):
        return {"out": torch.cat([train.gru_last_hidden(x[:, :, ch * i:(ch + 1) * i], lengths, w_ih, w_hh, b_ih, b_hh) for ch in range(channels)], dim=1)}
    old = _run(case, per_channel)
    bars, ref = case.bars(), case.ref()
    rec = {}
    for k in sorted(ref):
        err = R.rel_to_max(old[k], got[k].double())
        print(f"{case} {k}: per-channel entry vs single launch {err:.3e}  bar {bars[k]['bar']:.3e}")
        rec[f"{k}_per_channel_err"], rec[f"{k}_bar"] = err, bars[k]["bar"]
        assert err <= bars[k]["bar"], (k, err, bars[k]["bar"])
    measured(**rec)
    lv, cs = _on_device(case)
    params = [lv[n] for n in MR.GRU_PARAMS]
    views = torch.cat([hip.gru_last_hidden(lv["x"][:, :, ch * i:(ch + 1) * i], cs["lengths"], *params) for ch in range(c)], dim=1)
    assert R.rel_to_max(views.cpu(), got["out"].double()) <= bars["out"]["bar"]


# ------------------------------------------------------------------------------------------------ the wide attention
@pytest.mark.parametrize("shape", MR.wide_shapes(), ids=lambda s: "L{}-B{}-h{}-dh{}".format(*s))
def test_wide_attention_forward_and_backward(shape, measured):
    case = MR.wide_case(*shape)
    got = _run(case, _wide)
    _hold_measured(case, got, measured)
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    heads = case.consts["heads"]
    assert torch.equal(hip.mha_axis0_wide(lv["x"], lv["in_w"], lv["in_b"], lv["out_w"], lv["out_b"], heads).cpu(), got["out"])
    assert _same_bits(_run(case, _wide), got)


# ------------------------------------------------------------------------------------------------ refusals and input errors
def _shaped(b, s, c, i, h):
    x, lengths = R.randn(1, b, s, c * i).to(DEV), torch.full((b,), s, dtype=torch.int64, device=DEV)
    return x, lengths, [R.randn(2, 3 * h, i, scale=0.1).to(DEV), R.randn(3, 3 * h, h, scale=0.1).to(DEV), R.randn(4, 3 * h, scale=0.1).to(DEV),
                        R.randn(5, 3 * h, scale=0.1).to(DEV)]


@pytest.mark.parametrize("shape,limit", [((1, 2, 2, 4, 129), r"H=129 unsupported \(H <= 128\)"), ((1, 257, 2, 4, 4), r"S=257 unsupported \(S <= 256\)"),
                                         ((1, 2, 1, 1028, 4), r"I=1028 unsupported \(I <= 1024\)")], ids=["H129", "S257", "I1028"])
def test_channel_gru_refuses_shapes_past_its_bounds(shape, limit):
    x, lengths, params = _shaped(*shape)
    b, s, c, i, h = shape
    with pytest.raises(RuntimeError, match="channel_gru: " + limit):
        hip.channel_gru_last_hidden(x, lengths, *params, c)
    with pytest.raises(RuntimeError, match="channel_gru: " + limit):
        train.channel_gru_last_hidden(x.requires_grad_(True), lengths, *params, c)
    lib = hip._lib.load()
    buf = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    p = hip._ptr(buf)
    with pytest.raises(RuntimeError, match="channel_gru_backward: " + limit):
        hip._lib.check(lib.manner_hip_channel_gru_backward(p, p, hip._ptr(lengths), p, c * h, b, s, c, i, h, p, buf.numel(), p, p, p, p, p, p, buf.numel(),
                                                           hip._stream()))
    case = MR.cgru_case(*MR.CGRU_SHAPES[0])                      # the library is still usable
    assert torch.isfinite(_run(case, _cgru)["out"]).all()


@pytest.mark.parametrize("dh,entry,limit", [(129, "wide", r"axis0_attention_wide: head_dim 129 unsupported \(65 <= head_dim <= 128\)"),
                                            (64, "wide", r"axis0_attention_wide: head_dim 64 unsupported \(65 <= head_dim <= 128\)"),
                                            (65, "any", r"axis0_attention_any: head_dim 65 unsupported \(1 <= head_dim <= 64\)")],
                         ids=["wide-129", "wide-64", "any-65"])
def test_the_two_attentions_refuse_each_other_s_head_dims(dh, entry, limit):
    e = 2 * dh
    x = R.randn(1, 2, 3, e).to(DEV)
    w = [R.randn(2, 3 * e, e, scale=e ** -0.5).to(DEV), R.randn(3, 3 * e).to(DEV), R.randn(4, e, e, scale=e ** -0.5).to(DEV), R.randn(5, e).to(DEV)]
    fns = (hip.mha_axis0_wide, train.mha_axis0_wide) if entry == "wide" else (hip.mha_axis0_any, train.mha_axis0_any)
    for fn in fns:
        with pytest.raises(RuntimeError, match=limit):
            fn(x, *w, 2)
    if entry == "wide":
        lib = hip._lib.load()
        buf = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
        p = hip._ptr(buf)
        for name, call in (("_backward_q", lambda: lib.manner_hip_axis0_attention_wide_backward_q(p, p, p, 2, 3, e, 2, p, p, hip._stream())),
                           ("_backward_kv", lambda: lib.manner_hip_axis0_attention_wide_backward_kv(p, p, p, 2, 3, e, 2, p, hip._stream()))):
            with pytest.raises(RuntimeError, match=limit.replace("wide:", "wide" + name + ":")):
                hip._lib.check(call())
    case = MR.wide_case(2, 1, 1, 65)                             # the library is still usable
    assert torch.isfinite(_run(case, _wide)["out"]).all()


@pytest.mark.parametrize("what", ["length-0", "length-S+1"])
def test_bad_lengths_raise_at_the_status_check(what):
    """a length 0 and a length S + 1 set a bit in the device status word: ``check_status`` raises, nothing faults, the other rows'
    outputs are untouched and the next call is clean"""
    case = MR.cgru_case(*MR.CGRU_SHAPES[0])
    lv, cs = _on_device(case)
    params = [lv[n] for n in MR.GRU_PARAMS]
    c = cs["channels"]
    hip.check_status(DEV)
    lengths = cs["lengths"].clone()
    lengths[2] = 0 if what == "length-0" else lv["x"].shape[1] + 1
    out = hip.channel_gru_last_hidden(lv["x"], lengths, *params, c)
    with pytest.raises(RuntimeError, match="manner_hip input error"):
        hip.check_status(DEV)
    assert torch.isfinite(out).all()
    good = hip.channel_gru_last_hidden(lv["x"], cs["lengths"], *params, c)
    hip.check_status(DEV)
    rows = [0, 1, 3]
    assert torch.equal(out[rows], good[rows])                   # the other rows are untouched by the bad one
    x = lv["x"].clone().requires_grad_(True)
    train.channel_gru_last_hidden(x, lengths, *params, c).sum().backward()
    with pytest.raises(RuntimeError, match="manner_hip input error"):
        hip.check_status(DEV)
    assert torch.isfinite(x.grad).all()
    hip.check_status(DEV)


# ------------------------------------------------------------------------------------------------ the user encoder
@pytest.mark.parametrize("shape", MR.USER_SHAPES, ids=lambda s: "B{}-S{}-D{}-C{}".format(*s))
def test_user_encoder_forward_and_backward(shape, measured):
    case = MR.user_case(*shape)
    got = _run(case, _user)
    _hold_measured(case, got, measured)
    assert torch.equal(got["out"], got["hidden"])                                                # the pooler over one slot: the identity
    assert not got["d_pool_w"].any() and not got["d_pool_b"].any() and not got["d_query"].any()   # exact zeros
    assert got["d_x"][-1, 1:].any()                              # NOT zero past a length: the attention reads those slots for the other users
    lv, cs = _on_device(case)
    again = hip.mins_user(lv["x"], cs["lengths"], [lv[n] for n in USER_ORDER], cs["channels"])
    assert torch.equal(again.cpu(), got["out"])
    assert _same_bits(_run(case, _user), got)
    hip.check_status(DEV)


@pytest.fixture(scope="module")
def mins_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "mins.npz"))
    return z, json.loads(str(z["meta"]))


@pytest.mark.parametrize("tag", ["user", "wide"])
def test_user_encoder_mirror_matches_the_reference(mins_golden, tag, measured):
    """the mirror class, loaded through load_state_dict(strict=True), against the reference's own float32 outputs and gradients at the
    MEASURED bar of the golden's values (no tighter than 8 half-ulps, as the host test holds the restatement to them)"""
    z, meta = mins_golden
    v = meta["variants"][tag]
    case = R.Case("golden-" + tag, MR.mins_user, *golden_case(z, meta, tag))
    ref64, ref32 = case.ref(torch.float64), case.ref(torch.float32)
    enc = MINSUserEncoder(news_embedding_dim=v["D"], query_vector_dim=v["Q"], num_filters=v["D"], num_gru_channels=v["C"])
    sd = {MR.STATE_KEYS[name]: t for name, t in golden_params(z, meta, tag).items()}
    sd.update({f"multi_channel_gru.{c}.{k[len('gru.'):]}": t for c in range(v["C"]) for k, t in list(sd.items()) if k.startswith("gru.")})
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(DEV).train()
    lengths = torch.from_numpy(z["lengths"]).to(DEV)
    x = torch.from_numpy(z[tag + "_x"]).to(DEV).requires_grad_(True)
    out = enc(x, lengths)
    (out * torch.from_numpy(z[tag + "_up"]).to(DEV)).sum().backward()
    named = dict(enc.named_parameters())
    assert len(named) == 11
    got = {"out": out.detach().cpu(), "d_x": x.grad.cpu()}
    got.update({"d_" + name: named[key].grad.cpu() for name, key in MR.STATE_KEYS.items()})
    rec, bad = {}, {}
    for k, w in golden_want(z, tag, tag).items():
        bar = R.MEASURED_FACTOR * max(R.rel_to_max(rows_of(ref32[k], w), rows_of(ref64[k], w)), R.U32)
        err = R.rel_to_max(rows_of(got[k], w), torch.from_numpy(np.asarray(w)))
        print(f"golden-{tag} {k}: vs the reference's float32 {err:.3e}  bar {bar:.3e}")
        rec.update({f"{k}_err": err, f"{k}_bar": bar})
        if not err <= bar:
            bad[k] = (err, bar)
    measured(**rec)
    assert not bad, bad
    for name in MR.POOL_PARAMS:                                  # zero tensors, not None
        assert named[MR.STATE_KEYS[name]].grad is not None and not got["d_" + name].any(), name
    params = [t.detach() for t in enc._params()]
    mha = getattr(hip, "mha_axis0_" + hip.axis0_family(v["D"] // v["C"]))
    hidden = hip.channel_gru_last_hidden(mha(x.detach(), *params[:4], v["C"]), lengths, *params[4:], v["C"])
    assert torch.equal(out.detach(), hidden)                    # the output IS the concatenated hidden states
    with torch.no_grad():
        assert torch.equal(enc.eval()(x.detach(), lengths), out.detach())                        # the inference route
    with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
        assert enc(x.detach(), lengths).dtype == torch.float32 and torch.equal(enc(x.detach(), lengths), out.detach())
    enc.multihead_attention.dropout = 0.1
    with pytest.raises(RuntimeError, match="attention-probability dropout inside nn.MultiheadAttention is not built"):
        enc(x.detach(), lengths)
    hip.check_status(DEV)


# ------------------------------------------------------------------------------------------------ the news side
def test_category_encoder_mirror_matches_the_reference(mins_golden, measured):
    z, meta = mins_golden
    n = meta["news"]
    ce = NAMLCategoryEncoder(num_categories=n["num_categories"], category_embedding_dim=n["category_dim"], category_output_dim=n["category_out"])
    ce.load_state_dict({k[len("categ_sd:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("categ_sd:")}, strict=True)
    ce = ce.to(DEV)
    ids = torch.from_numpy(z["categ_ids"]).to(DEV)
    out = ce(ids)
    (out * torch.from_numpy(z["categ_up"]).to(DEV)).sum().backward()
    rec = {}
    _close(out, z["categ_out"], 1e-4, "out", rec)
    for k, p in ce.named_parameters():
        _close(p.grad, z["categ_grad:" + k], 1e-3, k, rec)
    assert not ce.category_embedding.weight.grad[0].any()        # the padding row
    with torch.no_grad():
        assert torch.equal(ce(ids), out.detach())
    measured(**rec)
    hip.check_status(DEV)


def test_news_encoder_mirror_matches_the_reference(mins_golden, measured):
    """train() with every dropout probability 0: outputs within 1e-4 and every gradient within 1e-3 of its tensor's largest entry — the
    tolerances the PLMTextEncoder mirror is held to in test_gpu_lstur.py; the padding row's gradient is exactly 0"""
    z, meta = mins_golden
    rec = {}
    n = meta["news"]
    cfg = PRESETS[n["preset"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = NAMLNewsEncoder(plm_model=n["preset"], frozen_layers=n["frozen_layers"], text_embedding_dim=cfg.hidden, num_attention_heads=n["text_heads"],
                              query_vector_dim=n["query_dim"], dropout_probability=0.0, num_categories=n["num_categories"],
                              category_embedding_dim=n["category_dim"])
    sd = {"text_encoder.plm_model." + k: torch.from_numpy(v) for k, v in make_plm_weights(cfg, seed=n["seed"], std=n["std"]).items()}
    sd.update({k: torch.from_numpy(v) for k, v in make_mha_pool_weights(cfg.hidden, n["query_dim"], seed=n["seed"], prefix="text_encoder.").items()})
    sd.update({k[len("news_sd:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("news_sd:")})
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(DEV)
    plm = enc.text_encoder.plm_model
    plm.hidden_dropout_prob = plm.attention_probs_dropout_prob = 0.0                                  # the golden's HF config
    enc.text_encoder.train_precision = enc.text_encoder.precision = "fp32"
    news = {"text": {"input_ids": torch.from_numpy(z["news_ids"]).to(DEV), "attention_mask": torch.from_numpy(z["news_mask"]).to(DEV)},
            "category": torch.from_numpy(z["news_categ"]).to(DEV)}
    with torch.no_grad():
        ev = enc.eval()(news)
    _close(ev, z["news_out_eval"], 1e-4, "eval out", rec)
    out = enc.train()(news)
    assert tuple(out.shape) == tuple(z["news_out"].shape) == (len(z["news_categ"]), cfg.hidden)
    _close(out, z["news_out"], 1e-4, "out", rec)
    (out * torch.from_numpy(z["news_R"]).to(DEV)).sum().backward()
    hip.check_status(DEV)
    zt = {k[len("news_"):]: z[k] for k in z.files if k.startswith("news_")}
    expect = {k[len("grad:"):]: v for k, v in zt.items() if k.startswith("grad:")}
    grads = {k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in plm.named_parameters()}
    compare_train_grads(grads, zt, n, expect, rel=1e-3)
    rest = {k: p for k, p in enc.named_parameters() if not k.startswith("text_encoder.plm_model.")}
    assert set(rest) == {k[len("pgrad:"):] for k in zt if k.startswith("pgrad:")}
    for k, p in rest.items():
        want = zt["pgrad:" + k]
        g = p.grad.cpu().numpy()
        _close(g[:want.shape[0]] if g.shape != want.shape else g, want, 1e-3, k, rec)
    assert not enc.category_encoder.category_embedding.weight.grad[0].any()
    measured(**rec)
