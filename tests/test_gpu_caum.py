"""The CAUM baseline's kernels (csrc/caum.hip) and mirror classes against the float64 restatement of tests/caum_ref.py, at the
smallest shapes that take every loop twice and fire every guard (caum_ref.USER_SHAPES): the golden and the shipped sizes, odd widths
at head dim 25, S = 1 and 2 (the circular window folds onto itself), B = 1, S past one and two 8-row tiles, B past what one workgroup
holds of several (slot, head) pairs (65) and past the 256-row block with its 64-key tiles (257), width 1024 (32 128-feature
steps of linear1's input, three 1024-feature chunks of the in-projection's data gradient), S at its bound, and — a shape of this
file's own — B = 365: 1095 rows, past the 16 row groups of the weight gradients (WG_MAX_GROUPS x WG_ROWS = 1024 rows; the other
shapes stop at 771).  ``mha_axis0_any`` alone adds head dim 12 (the 16-wide register width, which none of the listed head dims
takes) and 129 rows of head dim 64 (the tiled path below the 256-row block: 8256 floats > CA_LDS).

Every output has tanh / exp inside: the MEASURED bar of tests/side_ops_ref.py.  The two gradients that are zero in exact arithmetic
(d dense_att.linear3.bias, the K third of d in_proj_bias) are held to the absolute bound of caum_ref.zero_gradient_bounds.  Every test
prints its errors next to the bars and records them with ``measured`` (profiles/caum/measured_tolerances.json is that record from an
MI355X)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import caum_ref as CR
import side_ops_ref as R
from manner_amd import hip, train
from manner_amd.config import PRESETS
from manner_amd.models.components.attention import DenseAttention
from manner_amd.models.components.news_encoder import CAUMCategoryEncoder, CAUMNewsEncoder
from manner_amd.models.components.user_encoder import CAUMUserEncoder
from manner_amd.weights import make_mha_pool_weights, make_plm_weights
from test_gpu_side_ops import _hold_measured, _run
from test_oracle_golden import compare_train_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _user(x, c, heads, p=0.0, seed=0, **w):
    return {"out": train.caum_user_scores(x, c, [w[n] for n in CR.PARAMS], heads, p=p, seed=seed)}


def _hold_user(case, got, measured):
    """the MEASURED bar on everything but d_bc (zero in exact arithmetic, its relative error means nothing), then the two absolute bounds"""
    _hold_measured(case, got, measured, keys=[k for k in sorted(case.ref()) if k != "d_bc"])
    bounds, u = CR.zero_gradient_bounds(case), case.leaves["w2"].shape[0]
    dbc, dk = float(got["d_bc"].abs().max()), got["d_in_b"][u:2 * u].abs().numpy()
    print(f"{case} d_bc: |{dbc:.3e}| bound {bounds['d_bc'][0]:.3e}; K third of d_in_b: max |{dk.max():.3e}| least bound {bounds['d_in_b_k'].min():.3e}")
    measured(d_bc_abs=dbc, d_bc_bound=bounds["d_bc"][0], d_in_b_k_abs=dk.max(), d_in_b_k_least_bound=bounds["d_in_b_k"].min())
    assert dbc <= bounds["d_bc"][0] and (dk <= bounds["d_in_b_k"]).all(), case


# ------------------------------------------------------------------------------------------------ the user encoder
@pytest.mark.parametrize("shape", CR.USER_SHAPES, ids=lambda s: "B{}-S{}-D{}-F{}-H{}-{}-h{}".format(*s))
def test_user_encoder_forward_and_backward(shape, measured):
    case = CR.user_case(*shape)
    got = _run(case, _user)
    _hold_user(case, got, measured)
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    again = hip.caum_user_scores(lv["x"], lv["c"], [lv[n] for n in CR.PARAMS], shape[6])                  # the inference wrapper: the same kernels
    assert torch.equal(again.cpu(), got["out"])
    assert all(torch.equal(v, got[k]) for k, v in _run(case, _user).items())                               # fixed-order reductions: the same bits


def test_user_encoder_reads_the_strided_candidate_view():
    case = CR.user_case(*CR.GOLDEN_SHAPE)
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    params = [lv[n] for n in CR.PARAMS]
    cand = torch.randn(3, 5, 20, device=DEV)
    cand[:, 2, :] = lv["c"]
    view = cand[:, 2, :]
    assert not view.is_contiguous()
    assert torch.equal(hip.caum_user_scores(lv["x"], view, params, 4), hip.caum_user_scores(lv["x"], lv["c"], params, 4))
    leaf = cand.clone().requires_grad_(True)
    train.caum_user_scores(lv["x"], leaf[:, 2, :], params, 4).sum().backward()
    assert float(leaf.grad[:, 2].abs().max()) > 0 and float(leaf.grad[:, [0, 1, 3, 4]].abs().max()) == 0.0


def _shaped(b, s, d, f, h1, h2):
    x, c = R.randn(1, b, s, d).to(DEV), R.randn(2, b, d).to(DEV)
    return x, c, [R.randn(3 + i, *shp, scale=0.1).to(DEV) for i, shp in enumerate(CR.param_shapes(d, f, d, h1, h2).values())]


@pytest.mark.parametrize("shape,heads,limit", [((1, 257, 8, 8, 8, 8), 2, r"S=257 unsupported \(S <= 256\)"),
                                               ((1, 3, 1028, 8, 8, 8), 4, r"D=1028 unsupported \(D <= 1024\)"),
                                               ((1, 3, 8, 1028, 8, 8), 2, r"F=1028 unsupported \(F <= 1024\)"),
                                               ((1, 3, 8, 8, 1028, 8), 2, r"H1=1028 unsupported \(H1 <= 1024\)"),
                                               ((1, 3, 8, 8, 8, 1028), 2, r"H2=1028 unsupported \(H2 <= 1024\)"),
                                               ((1, 3, 130, 8, 8, 8), 2, r"head_dim 65 unsupported \(head_dim <= 64\)")],
                         ids=["S257", "D1028", "F1028", "H1-1028", "H2-1028", "dh65"])
def test_user_encoder_refuses_shapes_past_its_bounds(shape, heads, limit):
    x, c, params = _shaped(*shape)
    with pytest.raises(RuntimeError, match="caum_user: " + limit):
        hip.caum_user_scores(x, c, params, heads)
    with pytest.raises(RuntimeError, match="caum_user: " + limit):
        train.caum_user_scores(x.requires_grad_(True), c, params, heads)
    b, s, d, f, h1, h2 = shape
    lib = hip._lib.load()
    tab = (hip.C.c_void_p * 16)(*[t.data_ptr() for t in params])
    buf = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="caum_user_backward: " + limit):
        hip._lib.check(lib.manner_hip_caum_user_backward(tab, hip._ptr(c), b, s, d, f, d, h1, h2, heads, hip.C.c_float(0.0), hip.C.c_uint64(0),
                                                         hip.C.c_uint32(7), hip._ptr(buf), buf.numel(), hip._ptr(buf), hip._ptr(buf), tab,
                                                         hip._ptr(buf), buf.numel(), hip._stream()))
    case = CR.user_case(*CR.GOLDEN_SHAPE)                       # the library is still usable
    assert torch.isfinite(_run(case, _user)["out"]).all()


def test_user_encoder_refuses_a_news_width_that_is_not_the_user_width_and_attention_dropout():
    """DenseAttention(input_dim=2 U) is fed cat[all (U), candidate (D)]: the reference raises a matmul shape error unless D == U; the
    mirror names both numbers at forward, construction stays legal"""
    enc = CAUMUserEncoder(news_vector_dim=24, num_filters=8, dense_att_hidden_dim1=8, dense_att_hidden_dim2=8, user_vector_dim=20,
                          num_attention_heads=4, dropout_probability=0.0).to(DEV)
    x, c = R.randn(1, 2, 3, 24).to(DEV), R.randn(2, 2, 24).to(DEV)
    for mode in (enc.train(), enc.eval()):
        with pytest.raises(RuntimeError, match=r"news_vector_dim 24 != user_vector_dim 20"):
            mode(x, c)
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"news_vector_dim 24 != user_vector_dim 20"):
        enc(x, c)
    ok = CAUMUserEncoder(news_vector_dim=20, num_filters=8, dense_att_hidden_dim1=8, dense_att_hidden_dim2=8, user_vector_dim=20,
                         num_attention_heads=4, dropout_probability=0.0).to(DEV)
    ok.multihead_attention.dropout = 0.1
    with pytest.raises(RuntimeError, match="attention-probability dropout inside nn.MultiheadAttention is not built"):
        ok(R.randn(1, 2, 3, 20).to(DEV), R.randn(2, 2, 20).to(DEV))
    ok.multihead_attention.dropout = 0.0
    assert torch.isfinite(ok(R.randn(1, 2, 3, 20).to(DEV), R.randn(2, 2, 20).to(DEV))).all()


# ------------------------------------------------------------------------------------------------ mha_axis0_any alone
def _any(x, in_w, in_b, out_w, out_b, heads):
    return {"out": train.mha_axis0_any(x, in_w, in_b, out_w, out_b, heads)}


def _seven(x, in_w, in_b, out_w, out_b, heads):
    return {"out": train.mha_axis0(x, in_w, in_b, out_w, out_b, heads)}


@pytest.mark.parametrize("case", CR.any_cases(), ids=str)
def test_mha_axis0_any_forward_and_backward(case, measured):
    got = _run(case, _any)
    _hold_measured(case, got, measured)
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    heads = case.consts["heads"]
    assert torch.equal(hip.mha_axis0_any(lv["x"], lv["in_w"], lv["in_b"], lv["out_w"], lv["out_b"], heads).cpu(), got["out"])
    assert all(torch.equal(v, got[k]) for k, v in _run(case, _any).items())
    if case.leaves["x"].shape[2] // heads in (48, 64):          # a head dim of the seven-case dispatch: the same bar holds it too
        _hold_measured(case, _run(case, _seven), lambda **kw: measured(**{"seven_" + k: v for k, v in kw.items()}), keys=["out", "d_x"])


def test_mha_axis0_any_refuses_a_head_past_64_and_the_seven_case_dispatch_keeps_its_message():
    x = R.randn(1, 2, 3, 130).to(DEV)
    w = [R.randn(2, 390, 130).to(DEV), R.randn(3, 390).to(DEV), R.randn(4, 130, 130).to(DEV), R.randn(5, 130).to(DEV)]
    with pytest.raises(RuntimeError, match=r"axis0_attention_any: head_dim 65 unsupported \(1 <= head_dim <= 64\)"):
        hip.mha_axis0_any(x, *w, 2)
    x5 = R.randn(1, 2, 3, 10).to(DEV)
    w5 = [R.randn(2, 30, 10).to(DEV), R.randn(3, 30).to(DEV), R.randn(4, 10, 10).to(DEV), R.randn(5, 10).to(DEV)]
    with pytest.raises(RuntimeError, match=r"axis-0 attention: head_dim 5 unsupported \(4, 8, 10, 16, 32, 48, 64\)"):
        hip.mha_axis0(x5, *w5, 2)
    assert torch.isfinite(hip.mha_axis0_any(x5, *w5, 2)).all()


# ------------------------------------------------------------------------------------------------ ReLU and linear + tanh alone
def test_relu_pair_is_exact_past_one_grid_of_the_elementwise_launch():
    """out = max(x, 0) and grad_x = grad_out where x > 0 — bit for bit, with exact zeros and negative zeros among the inputs (no
    gradient AT zero, as torch) and more elements than one pass of the grid-stride launch covers (8192 workgroups x 256 threads)"""
    n = R.DROPOUT_N
    x, g = R.randn(41, n), R.randn(42, n)
    x[::7], x[3::11] = 0.0, -0.0
    xd = x.to(DEV).requires_grad_(True)
    out = train.relu(xd)
    out.backward(g.to(DEV))
    assert torch.equal(out.detach().cpu(), x.clamp(min=0.0)) and torch.equal(hip.relu(x.to(DEV)).cpu(), x.clamp(min=0.0))
    assert torch.equal(xd.grad.cpu(), torch.where(x > 0, g, torch.zeros_like(g)))
    assert float(xd.grad.cpu()[::7].abs().max()) == 0.0 and float(xd.grad.cpu()[3::11].abs().max()) == 0.0


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", CR.LINEAR_TANH_SHAPES, ids=lambda s: "R{}-K{}-O{}".format(*s))
def test_linear_tanh_forward_and_backward(shape, with_bias, measured):
    """tanh(nn.Linear) in one kernel and its backward (tanh_backward, then linear_backward) alone — tanh inside, so the MEASURED bar"""
    case = CR.linear_tanh_case(*shape, with_bias)
    got = _run(case, lambda x, weight, bias=None: {"y": train.linear_tanh(x, weight, bias)})
    _hold_measured(case, got, measured)
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    assert torch.equal(hip.linear_tanh(lv["x"], lv["weight"], lv.get("bias")).cpu(), got["y"])


# ------------------------------------------------------------------------------------------------ dropout
def _mirror(case, p, shape):
    _, _, d, f, h1, h2, heads = shape
    enc = CAUMUserEncoder(news_vector_dim=d, num_filters=f, dense_att_hidden_dim1=h1, dense_att_hidden_dim2=h2, user_vector_dim=d,
                          num_attention_heads=heads, dropout_probability=p)
    enc.load_state_dict({CR.STATE_KEYS[n]: case.leaves[n] for n in CR.PARAMS}, strict=True)
    return enc.to(DEV)


def _mirror_run(enc, case):
    x, c = (case.leaves[n].to(DEV).requires_grad_(True) for n in ("x", "c"))
    out = enc(x, c)
    (out * case.upstream["out"].to(DEV)).sum().backward()
    got = {"out": out.detach().cpu(), "d_x": x.grad.cpu(), "d_c": c.grad.cpu()}
    got.update({"d_" + n: p.grad.detach().cpu() for n, p in zip(CR.PARAMS, enc._params())})
    return got


@pytest.mark.parametrize("shape", [CR.GOLDEN_SHAPE, (9, 5, 50, 12, 10, 6, 2)], ids=["golden", "odd"])
def test_user_encoder_dropout_follows_the_keep_masks(shape, measured):
    """train() at p = 0.2: the seed draw is replayed under torch.manual_seed, the three keep-masks come from train.dropout_mask (sites
    7, 8, 9), and outputs and gradients are held to the restatement with those masks; eval() is the p = 0 case bit for bit"""
    p, (b, s, d, f, _, _, _) = 0.2, shape
    base = CR.user_case(*shape)
    for manual in range(1234, 1266):                             # the first seed whose masks settle every float32 CPU figure (side_ops_ref)
        torch.manual_seed(manual)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        keep = [train.dropout_mask(seed, hip.CAUM_DROPOUT_SITE + i, p, n, DEV).cpu() for i, n in enumerate((b * d, b * s * d, b * s * (f + d)))]
        case = R.Case(str(base) + "-dropout", base.fn, base.leaves, dict(base.consts, p=p, keep1=keep[0].reshape(b, d), keep2=keep[1].reshape(b, s, d),
                                                                          keep3=keep[2].reshape(b, s, f + d)), base.upstream)
        if all(v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP for k, v in case.bars().items() if k != "d_bc"):
            break
    else:
        raise AssertionError("no seed in 32 settles the dropout case")
    assert all(0.6 < float(k.float().mean()) < 0.95 for k in keep[1:])
    enc = _mirror(base, p, shape).train()
    torch.manual_seed(manual)
    got = _mirror_run(enc, base)
    assert R.rel_to_max(got["out"], base.ref()["out"]) > 1e-3                                      # the dropouts are on
    _hold_user(case, got, measured)
    enc.eval()
    enc.zero_grad()
    plain = _mirror_run(_mirror(base, 0.0, shape).train(), base)
    assert all(torch.equal(v, plain[k]) for k, v in _mirror_run(enc, base).items())


# ------------------------------------------------------------------------------------------------ the mirrors on the goldens
@pytest.fixture(scope="module")
def caum_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "caum.npz"))
    return z, json.loads(str(z["meta"]))


def _close(got, want, rel, what, rec=None):
    """within ``rel`` of the tensor's largest golden entry; ``rec`` (a dict) receives the figure for ``measured``"""
    got, want = np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got), np.asarray(want)
    assert got.shape == want.shape, what
    err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-3)
    if rec is not None:
        rec[what.replace(" ", "_") + "_rel"] = err
    assert err <= rel, (what, err, float(np.abs(want).max()))


def test_user_encoder_mirror_matches_the_reference(caum_golden, measured):
    z, _ = caum_golden
    rec = {}
    _, _, d, f, h1, h2, heads = CR.GOLDEN_SHAPE
    enc = CAUMUserEncoder(news_vector_dim=d, num_filters=f, dense_att_hidden_dim1=h1, dense_att_hidden_dim2=h2, user_vector_dim=d,
                          num_attention_heads=heads, dropout_probability=0.0)
    enc.load_state_dict({k[len("user_sd:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("user_sd:")}, strict=True)
    enc = enc.to(DEV).train()
    x, c = (torch.from_numpy(z[k]).to(DEV).requires_grad_(True) for k in ("user_x", "user_c"))
    out = enc(x, c)
    (out * torch.from_numpy(z["user_up"]).to(DEV)).sum().backward()
    _close(out, z["user_out"], 1e-4, "out", rec)
    _close(x.grad, z["user_d_x"], 1e-3, "d_x", rec)
    _close(c.grad, z["user_d_c"], 1e-3, "d_c", rec)
    for k, p in enc.named_parameters():
        _close(p.grad, z["user_grad:" + k], 1e-3, k, rec)
    measured(**rec)
    with torch.no_grad():
        assert torch.equal(enc.eval()(x.detach(), c.detach()), out.detach())                        # the inference route: the same kernels


def test_dense_attention_mirror_alone_matches_the_reference(caum_golden, measured):
    z, _ = caum_golden
    rec = {}
    _, _, d, _, h1, h2, _ = CR.GOLDEN_SHAPE
    da = DenseAttention(input_dim=2 * d, hidden_dim1=h1, hidden_dim2=h2)
    da.load_state_dict({k[len("dense_sd:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("dense_sd:")}, strict=True)
    da = da.to(DEV)
    v = torch.from_numpy(z["dense_x"]).to(DEV).requires_grad_(True)
    out = da(v)
    assert tuple(out.shape) == tuple(z["dense_out"].shape) and out.shape[-1] == 1
    (out * torch.from_numpy(z["dense_up"]).to(DEV)).sum().backward()
    _close(out, z["dense_out"], 1e-4, "out", rec)
    _close(v.grad, z["dense_d_x"], 1e-3, "d_x", rec)
    for k, p in da.named_parameters():
        _close(p.grad, z["dense_grad:" + k], 1e-3, k, rec)
    with torch.no_grad():
        _close(da(v.detach()), z["dense_out"], 1e-4, "out under no_grad", rec)
    measured(**rec)


def test_category_encoder_mirror_matches_the_reference(caum_golden, measured):
    z, meta = caum_golden
    rec = {}
    n = meta["news"]
    ce = CAUMCategoryEncoder(num_categories=n["num_categories"], category_embedding_dim=n["category_dim"], category_output_dim=n["category_dim"],
                             dropout_probability=0.0)
    ce.load_state_dict({k[len("categ_sd:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("categ_sd:")}, strict=True)
    ce = ce.to(DEV).train()
    out = ce(torch.from_numpy(z["categ_ids"]).to(DEV))
    (out * torch.from_numpy(z["categ_up"]).to(DEV)).sum().backward()
    _close(out, z["categ_out"], 1e-5, "out", rec)
    assert float(out.detach().min()) == 0.0 and float((out.detach() == 0).float().mean()) > 0.1                        # the ReLU cuts
    for k, p in ce.named_parameters():
        _close(p.grad, z["categ_grad:" + k], 1e-4, k, rec)
    measured(**rec)
    assert float(ce.category_embedding.weight.grad[0].abs().max()) == 0.0                             # the padding row
    with torch.no_grad():
        assert torch.equal(ce.eval()(torch.from_numpy(z["categ_ids"]).to(DEV)), out.detach())


@pytest.mark.parametrize("tag", ["ent", "noent"])
def test_news_encoder_mirror_matches_the_reference(caum_golden, tag, measured):
    """train() with every dropout probability 0: outputs within 1e-4 and every gradient within 1e-3 of its tensor's largest entry — the
    tolerances of test_gpu_train.py::test_train_gradients_match_reference; the entity encoder runs at head dim 5"""
    z, meta = caum_golden
    rec = {}
    n = meta["news"]
    cfg = PRESETS[n["preset"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = CAUMNewsEncoder(plm_model=n["preset"], frozen_layers=n["frozen_layers"], text_embedding_dim=cfg.hidden,
                              text_num_attention_heads=n["text_heads"], query_vector_dim=n["query_dim"], dropout_probability=0.0,
                              num_categories=n["num_categories"], category_embedding_dim=n["category_dim"], use_entities=tag == "ent",
                              entity_embeddings=torch.from_numpy(z["news_entity_table"]), entity_embedding_dim=n["entity_dim"],
                              entity_num_attention_heads=n["entity_heads"], news_out_embedding_dim=n["news_out"])
    sd = {"text_encoder.plm_model." + k: torch.from_numpy(v) for k, v in make_plm_weights(cfg, seed=n["seed"], std=n["std"]).items()}
    sd.update({k: torch.from_numpy(v) for k, v in make_mha_pool_weights(cfg.hidden, n["query_dim"], seed=n["seed"], prefix="text_encoder.").items()})
    sd.update({k[len(f"news_{tag}_sd:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"news_{tag}_sd:")})
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(DEV)
    plm = enc.text_encoder.plm_model
    plm.hidden_dropout_prob = plm.attention_probs_dropout_prob = 0.0                                  # the golden's HF config
    enc.text_encoder.train_precision = enc.text_encoder.precision = "fp32"
    news = {"text": {"input_ids": torch.from_numpy(z["news_ids"]).to(DEV), "attention_mask": torch.from_numpy(z["news_mask"]).to(DEV)},
            "category": torch.from_numpy(z["news_categ"]).to(DEV), "entities": torch.from_numpy(z["news_entities"]).to(DEV)}
    with torch.no_grad():
        _close(enc.eval()(news), z[f"news_{tag}_out_eval"], 1e-4, "eval", rec)
    out = enc.train()(news)
    _close(out, z[f"news_{tag}_out"], 1e-4, "out", rec)
    (out * torch.from_numpy(z["news_R"]).to(DEV)).sum().backward()
    hip.check_status(DEV)
    zt = {k[len(f"news_{tag}_"):]: z[k] for k in z.files if k.startswith(f"news_{tag}_")}
    expect = {k[len("grad:"):]: v for k, v in zt.items() if k.startswith("grad:")}
    grads = {k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in plm.named_parameters()}
    compare_train_grads(grads, zt, n, expect, rel=1e-3)      # the golden keeps the PLM's gradients once, with entities: frozen / not frozen only without
    rest = {k: p for k, p in enc.named_parameters() if not k.startswith("text_encoder.plm_model.")}
    assert set(rest) == {k[len("pgrad:"):] for k in zt if k.startswith("pgrad:")}
    for k, p in rest.items():
        want = zt["pgrad:" + k]
        g = p.grad.cpu().numpy()
        _close(g[:want.shape[0]] if g.shape != want.shape else g, want, 1e-3, k, rec)
    measured(**rec)


# ------------------------------------------------------------------------------------------------ CAUMPLMModule.forward, restated
def test_caum_forward_over_the_mirror_classes(measured):
    """the operator lines of CAUMPLMModule.forward (baselines/caum_plm_module.py:155-165) over the CAUMUserEncoder of this package —
    the candidate loop on cand[:, i, :] views, the row assignment into the transposed scores — against the float64 restatement
    looped the same way: C = 5, one zero-padded candidate row and one zero-padded history row"""
    case = CR.module_case()
    b, s, d, f, h1, h2, heads, c_n = CR.MODULE_SHAPE
    enc = CAUMUserEncoder(news_vector_dim=d, num_filters=f, dense_att_hidden_dim1=h1, dense_att_hidden_dim2=h2, user_vector_dim=d,
                          num_attention_heads=heads, dropout_probability=0.0)
    enc.load_state_dict({CR.STATE_KEYS[n]: case.leaves[n] for n in CR.PARAMS}, strict=True)
    enc = enc.to(DEV).train()
    hist, cand = (case.leaves[n].to(DEV).requires_grad_(True) for n in ("hist", "cand"))
    scores = torch.zeros(cand.shape[0], cand.shape[1], device=DEV)
    scores = scores.transpose(1, 0)
    for i in range(cand.shape[1]):
        cand_score = enc(hist, cand[:, i, :])
        scores[i, :] = cand_score
    scores = scores.transpose(1, 0)
    (scores * case.upstream["scores"].to(DEV)).sum().backward()
    got = {"scores": scores.detach().cpu(), "d_hist": hist.grad.cpu(), "d_cand": cand.grad.cpu()}
    got.update({"d_" + n: p.grad.detach().cpu() for n, p in zip(CR.PARAMS, enc._params())})
    _hold_measured(case, got, measured, keys=[k for k in sorted(case.ref()) if k != "d_bc"])
    assert float(got["d_bc"].abs().max()) == 0.0                                                    # written as an exact zero
    with torch.no_grad():
        again = torch.stack([enc.eval()(hist.detach(), cand.detach()[:, i, :]) for i in range(c_n)], dim=1)
    assert torch.equal(again.cpu(), got["scores"])
