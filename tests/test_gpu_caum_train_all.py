"""``manner_hip_caum_train_all_forward`` / ``_backward`` (csrc/caum.hip) — CAUM's candidate loop in train(), every column in one call,
column c under its own seed — with ``train.caum_scores_all``, ``CAUMUserEncoder.train_all_columns`` and ``hotpath.caum_train_step``
above them, against the float64 loop over the columns with the same keep-masks (tests/caum_train_all_ref.py; tests/
test_caum_train_all_host.py holds that restatement and its planted defects on the CPU).  Forward and every gradient sit under the
MEASURED bar of tests/side_ops_ref.py (8 x the float32 CPU error of that loop, relative to the tensor's largest entry); the two
gradients that are zero in exact arithmetic must be exact zeros.  ``manner_hip_wgrad_rows_f32`` alone — the matrix-core weight
gradient — is a pure sum of products: the DERIVED bar (n + 4) 2^-24 sum |a b| with n = R.  Every test prints its errors next to the
bars and records them with ``measured`` (profiles/caum/measured_tolerances.json is that record from an MI355X)."""
import os

import numpy as np
import pytest
import torch

import caum_ref as CR
import caum_train_all_ref as T
import side_ops_ref as R
from manner_amd import hip, hotpath, train
from manner_amd.models.components.user_encoder import CAUMUserEncoder
from test_gpu_side_ops import _hold_measured

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(shape):
    return "B{}-S{}-D{}-F{}-H{}-{}-h{}-C{}".format(*shape)


def device_mask(seed, site, p, n):
    """the masks as the device generator gives them (``train.dropout_mask``), on the CPU"""
    return train.dropout_mask(seed, site, p, n, DEV).cpu()


def _scores_all(hist, cand, heads, p=0.0, seeds=None, **w):
    return {"scores": train.caum_scores_all(hist, cand, [w[n] for n in CR.PARAMS], heads, p=p, seeds=seeds)}


def _run(case):
    return R.evaluate(_scores_all, case.leaves, {"heads": case.consts["heads"], "p": case.p, "seeds": case.seeds}, case.upstream, torch.float32, DEV)


def _hold(case, got, measured):
    """the MEASURED bar on everything but d_bc; d_bc and the K third of d_in_b are written as exact zeros"""
    _hold_measured(case, got, measured, keys=[k for k in sorted(case.ref()) if k != "d_bc"])
    u = case.leaves["w2"].shape[0]
    assert float(got["d_bc"].abs().max()) == 0.0 and float(got["d_in_b"][u:2 * u].abs().max()) == 0.0, case


# ------------------------------------------------------------------------------------------------ 1. forward and every gradient
_CASES = [(s, 0.0) for s in T.DROPOUT_SHAPES + T.PLAIN_ONLY_SHAPES] + [(s, T.P) for s in T.DROPOUT_SHAPES]


@pytest.mark.parametrize("shape,p", _CASES, ids=[_ids(s) + f"-p{p}" for s, p in _CASES])
def test_scores_all_forward_and_every_gradient(shape, p, measured):
    case = T.train_case(shape, p, device_mask)
    got = _run(case)
    _hold(case, got, measured)
    if shape[0] > 1:
        assert float(got["scores"][1, -1]) == 0.0                              # the zero candidate row, with or without dropout
    if p > 0:
        assert R.rel_to_max(got["scores"], T.train_case(shape, 0.0, device_mask).ref()["scores"]) > 1e-3          # the dropouts are on
    again = _run(case)
    assert all(torch.equal(v, got[k]) for k, v in again.items()), [k for k, v in again.items() if not torch.equal(v, got[k])]


# ------------------------------------------------------------------------------------------------ 2. the keep rule
@pytest.mark.parametrize("seed", [0x0123456789ABCDEF, 2 ** 62 - 5])
def test_dropout_mask_is_the_numpy_keep_rule(seed):
    n = R.DROPOUT_N
    for site in range(T.SITE0, T.SITE0 + 3):
        assert torch.equal(device_mask(seed, site, T.P, n), T.numpy_mask(seed, site, T.P, n)), (seed, site)


# ------------------------------------------------------------------------------------------------ 3. C = 1 against the golden
def _encoder(leaves, shape, p, all_columns):
    _, _, d, f, h1, h2, heads = shape[:7]
    enc = CAUMUserEncoder(news_vector_dim=d, num_filters=f, dense_att_hidden_dim1=h1, dense_att_hidden_dim2=h2, user_vector_dim=d,
                          num_attention_heads=heads, dropout_probability=p)
    enc.load_state_dict(leaves, strict=True)
    enc.train_all_columns = all_columns
    return enc.to(DEV)


def test_one_column_meets_the_golden_of_the_reference_class(golden_dir, measured):
    """train(), p = 0, ``train_all_columns``: the reference's own CAUMUserEncoder on (user_x, user_c) — out within 1e-4 and every
    gradient within 1e-3 of its tensor's largest entry, the tolerances of test_gpu_caum.py::test_user_encoder_mirror_matches_the_reference"""
    z = np.load(os.path.join(golden_dir, "caum.npz"))
    enc = _encoder({k[len("user_sd:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("user_sd:")}, CR.GOLDEN_SHAPE, 0.0, True).train()
    x, c = (torch.from_numpy(z[k]).to(DEV).requires_grad_(True) for k in ("user_x", "user_c"))
    out = enc.forward_all(x, c[:, None, :])[:, 0]
    (out * torch.from_numpy(z["user_up"]).to(DEV)).sum().backward()
    rec = {}

    def close(got, want, rel, what):
        got, want = got.detach().cpu().numpy(), np.asarray(want)
        assert got.shape == want.shape, what
        rec[what + "_rel"] = err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-3)
        print(f"{what}: {err:.3e} (bar {rel:g})")
        assert err <= rel, (what, err)

    close(out, z["user_out"], 1e-4, "out")
    close(x.grad, z["user_d_x"], 1e-3, "d_x")
    close(c.grad, z["user_d_c"], 1e-3, "d_c")
    for k, p in enc.named_parameters():
        close(p.grad, z["user_grad:" + k], 1e-3, k)
    measured(**rec)


# ------------------------------------------------------------------------------------------------ 4. the mirror route
def _loop_by_hand(enc, hist, cand):
    """CAUMPLMModule.forward's own lines (baselines/caum_plm_module.py:156-163)"""
    scores = torch.zeros(cand.shape[0], cand.shape[1], device=DEV)
    scores = scores.transpose(1, 0)
    for i in range(cand.shape[1]):
        scores[i, :] = enc(hist, cand[:, i, :])
    return scores.transpose(1, 0)


def _with_gradients(enc, run, case):
    hist, cand = (case.leaves[n].to(DEV).requires_grad_(True) for n in ("hist", "cand"))
    enc.zero_grad()
    torch.manual_seed(case.manual)
    scores = run(enc, hist, cand)
    (scores * case.upstream["scores"].to(DEV)).sum().backward()
    drawn = int(torch.randint(0, 2 ** 62, (1,)).item())                                        # where the CPU generator stands afterwards
    got = {"scores": scores.detach().cpu(), "d_hist": hist.grad.cpu(), "d_cand": cand.grad.cpu()}
    got.update({"d_" + n: p.grad.detach().cpu() for n, p in zip(CR.PARAMS, enc._params())})
    return got, drawn


def test_forward_all_over_all_columns_and_the_loop_hold_to_one_restatement(measured, monkeypatch):
    """under one torch.manual_seed, ``forward_all`` with ``train_all_columns`` and the loop by hand draw the same seeds, apply the
    same masks and leave the CPU generator in the same state; the attribute on never enters the per-column entry, the attribute off
    is the loop bit for bit"""
    shape = T.MODULE_SHAPE
    case = T.train_case(shape, T.P, device_mask)
    state = {CR.STATE_KEYS[n]: case.leaves[n] for n in CR.PARAMS}
    calls = []
    per_column = train.caum_user_scores
    monkeypatch.setattr(train, "caum_user_scores", lambda *a, **k: (calls.append(1), per_column(*a, **k))[1])
    on = _encoder(state, shape, T.P, True).train()
    got, drawn = _with_gradients(on, lambda e, h, c: e.forward_all(h, c), case)
    assert not calls                                                                           # one call over all columns
    _hold(case, got, lambda **kw: measured(**{"all_columns_" + k: v for k, v in kw.items()}))
    off = _encoder(state, shape, T.P, False).train()
    assert CAUMUserEncoder.train_all_columns is False                                          # the default stays the loop
    hand, drawn_hand = _with_gradients(off, _loop_by_hand, case)
    assert len(calls) == shape[7]
    _hold(case, hand, lambda **kw: measured(**{"loop_" + k: v for k, v in kw.items()}))
    assert drawn == drawn_hand
    loop, drawn_loop = _with_gradients(off, lambda e, h, c: e.forward_all(h, c), case)
    assert drawn_loop == drawn_hand and all(torch.equal(loop[k], hand[k]) for k in hand)
    plain = _encoder(state, shape, 0.0, True).eval()                                           # a recorded graph without dropout: no draw
    torch.manual_seed(case.manual)
    before = torch.get_rng_state()
    hist, cand = (case.leaves[n].to(DEV).requires_grad_(True) for n in ("hist", "cand"))
    scores = plain.forward_all(hist, cand)
    assert scores.requires_grad and torch.equal(torch.get_rng_state(), before) and len(calls) == 2 * shape[7]
    assert R.rel_to_max(scores.detach().cpu(), T.train_case(shape, 0.0, device_mask).ref()["scores"]) <= 1e-4


# ------------------------------------------------------------------------------------------------ 5. refusals
def _shaped(b, s, d, f, h1, h2, c=2):
    x, cand = R.randn(1, b, s, d).to(DEV), R.randn(2, b, c, d).to(DEV)
    return x, cand, [R.randn(3 + i, *shp, scale=0.1).to(DEV) for i, shp in enumerate(CR.param_shapes(d, f, d, h1, h2).values())]


@pytest.mark.parametrize("shape,heads,limit", [((1, 257, 8, 8, 8, 8), 2, r"S=257 unsupported \(S <= 256\)"),
                                               ((1, 3, 1028, 8, 8, 8), 4, r"D=1028 unsupported \(D <= 1024\)"),
                                               ((1, 3, 8, 1028, 8, 8), 2, r"F=1028 unsupported \(F <= 1024\)"),
                                               ((1, 3, 8, 8, 1028, 8), 2, r"H1=1028 unsupported \(H1 <= 1024\)"),
                                               ((1, 3, 8, 8, 8, 1028), 2, r"H2=1028 unsupported \(H2 <= 1024\)"),
                                               ((1, 3, 130, 8, 8, 8), 2, r"head_dim 65 unsupported \(head_dim <= 64\)")],
                         ids=["S257", "D1028", "F1028", "H1-1028", "H2-1028", "dh65"])
def test_scores_all_refuses_shapes_past_the_bounds(shape, heads, limit):
    x, cand, params = _shaped(*shape)
    with pytest.raises(RuntimeError, match="caum_train_all: " + limit):
        train.caum_scores_all(x.requires_grad_(True), cand, params, heads)
    b, s, d, f, h1, h2 = shape
    lib = hip._lib.load()
    tab = (hip.C.c_void_p * 16)(*[t.data_ptr() for t in params])
    buf = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="caum_train_all_backward: " + limit):
        hip._lib.check(lib.manner_hip_caum_train_all_backward(tab, hip._ptr(buf), b, s, 2, d, f, d, h1, h2, heads, hip.C.c_float(0.0), None,
                                                              hip.C.c_uint32(7), hip._ptr(buf), buf.numel(), hip._ptr(buf), hip._ptr(buf), tab,
                                                              hip._ptr(buf), buf.numel(), hip._stream()))


def test_scores_all_without_columns_or_users_and_a_negative_count():
    x, cand, params = _shaped(3, 4, 8, 8, 8, 8, c=0)
    leaves = [x.requires_grad_(True), cand.requires_grad_(True)] + [t.requires_grad_(True) for t in params]
    out = train.caum_scores_all(leaves[0], leaves[1], leaves[2:], 2)
    assert tuple(out.shape) == (3, 0) and out.dtype == torch.float32
    out.sum().backward()                                                                        # C == 0: every gradient an exact zero
    assert all(t.grad is not None and tuple(t.grad.shape) == tuple(t.shape) and float(t.grad.abs().sum()) == 0.0 for t in leaves)
    x0, cand0, _ = _shaped(0, 4, 8, 8, 8, 8, c=3)
    fresh = [t.detach().clone().requires_grad_(True) for t in params]
    out0 = train.caum_scores_all(x0, cand0, fresh, 2)
    assert tuple(out0.shape) == (0, 3)
    out0.sum().backward()                                                                       # B == 0: the parameter gradients are zeros
    assert all(t.grad is not None and float(t.grad.abs().sum()) == 0.0 for t in fresh)
    tab = (hip.C.c_void_p * 16)(*[t.data_ptr() for t in params])
    buf = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r"caum_train_all: bad shape C=-1"):
        hip._lib.check(hip._lib.load().manner_hip_caum_train_all_forward(hip._ptr(x), hip._ptr(buf), tab, 3, 4, -1, 8, 8, 8, 8, 8, 2, hip.C.c_float(0.0),
                                                                         None, hip.C.c_uint32(7), hip._ptr(buf), hip._ptr(buf), buf.numel(),
                                                                         hip._stream()))
    with pytest.raises(ValueError, match="one seed per candidate column"):
        train.caum_scores_all(*_shaped(3, 4, 8, 8, 8, 8)[:2], params, 2, p=0.2, seeds=[1])
    case = T.train_case(T.MODULE_SHAPE, 0.0, device_mask)                                       # the library is still usable
    assert torch.isfinite(_run(case)["scores"]).all()


# ------------------------------------------------------------------------------------------------ 6. the weight-gradient kernel alone
def _wgrad(dy, x):
    r, o = dy.shape
    k = x.shape[1]
    lib = hip._lib.load()
    dw = torch.full((o, k), float("nan"), dtype=torch.float32, device=DEV)
    need = int(lib.manner_hip_wgrad_rows_f32_workspace_bytes(r, k, o))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    hip._lib.check(lib.manner_hip_wgrad_rows_f32(hip._ptr(dy), o, hip._ptr(x), k, r, k, o, hip._ptr(dw), k, hip._ptr(ws), need, hip._stream()))
    return dw.cpu()


@pytest.mark.parametrize("shape", T.WGRAD_SHAPES, ids=lambda s: "R{}-K{}-O{}".format(*s))
def test_wgrad_rows_f32_alone_under_the_derived_bar(shape, measured):
    r, k, o = shape
    dy, x = T.wgrad_inputs(r, k, o)
    got = _wgrad(dy.to(DEV), x.to(DEV))
    ref = dy.double().T @ x.double()
    ratio = R.derived_ratio(got.numpy(), ref.numpy(), (dy.double().abs().T @ x.double().abs()).numpy(), r)
    print(f"wgrad_rows_f32 R{r}-K{k}-O{o}: error / derived bound = {ratio:.3f} (bar 1)")
    measured(d_weight_over_bound=ratio, bar=1.0)
    assert ratio <= 1.0
    assert torch.equal(_wgrad(dy.to(DEV), x.to(DEV)), got)                                      # fixed-order sums: the same bits


# ------------------------------------------------------------------------------------------------ 7. hotpath.caum_train_step
def test_caum_train_step_on_a_ragged_batch(measured):
    """three impressions with 3 / 1 / 2 clicked news and 5 / 3 / 5 candidates, a stub news encoder that returns the rows it is given,
    train() at p = 0.2 with ``train_all_columns``: the loss and its gradient into the news rows against
    ``side_ops_ref.model_step_loss(supcon=False)`` over the float64 restatement on the zero-padded dense tensors with the same masks"""
    _, _, d, f, h1, h2, heads, _ = T.MODULE_SHAPE
    n_hist, n_cand, s, c = (3, 1, 2), (5, 3, 5), 3, 5
    hist_off, cand_off = (torch.tensor(np.concatenate([[0], np.cumsum(n)]), dtype=torch.int64) for n in (n_hist, n_cand))
    labels = torch.zeros(sum(n_cand))
    labels[[0, 6, 10]] = 1.0
    hist_at = torch.tensor([i * s + j for i, n in enumerate(n_hist) for j in range(n)])
    cand_at = torch.tensor([i * c + j for i, n in enumerate(n_cand) for j in range(n)])

    def step(x_hist, x_cand, heads, p=0.0, keeps=None, **w):
        hist = x_hist.new_zeros(3 * s, d).index_put((hist_at,), x_hist).reshape(3, s, d)
        cand = x_cand.new_zeros(3 * c, d).index_put((cand_at,), x_cand).reshape(3, c, d)
        scores = T.caum_train_all(hist, cand, heads, p, keeps, **w)["scores"]
        return {"loss": R.model_step_loss(scores.reshape(-1)[cand_at], labels, cand_off, False, 1.0, c_max=c)["loss"]}

    def build(trial):
        leaves, _, _ = CR.caum_inputs(3, s, d, f, h1, h2, heads, 41)
        leaves = dict({k: v for k, v in leaves.items() if k not in ("x", "c")}, x_hist=R.randn(3700, sum(n_hist), d), x_cand=R.randn(3701, sum(n_cand), d))
        seeds = T.draw_seeds(1234 + trial, c)
        case = R.Case("caum-train-step-ragged", step, leaves, {"heads": heads, "p": T.P, "keeps": T.column_keeps(seeds, T.P, 3, s, d, f, device_mask)},
                      {"loss": torch.tensor(1.0)})
        case.manual = 1234 + trial
        return case
    case = T.settle(build)
    enc = _encoder({CR.STATE_KEYS[n]: case.leaves[n] for n in CR.PARAMS}, T.MODULE_SHAPE, T.P, True).train()
    rows = {k: case.leaves[k].to(DEV).requires_grad_(True) for k in ("x_hist", "x_cand")}
    batch = {"x_hist": rows["x_hist"], "x_cand": rows["x_cand"], "labels": labels.to(DEV), "users": torch.arange(3, device=DEV),
             "batch_hist": torch.repeat_interleave(torch.arange(3), torch.tensor(n_hist)).to(DEV),
             "batch_cand": torch.repeat_interleave(torch.arange(3), torch.tensor(n_cand)).to(DEV), "hist_max": s, "cand_max": c}
    torch.manual_seed(case.manual)
    loss, ragged, off = hotpath.caum_train_step(lambda r: r, enc, batch)
    loss.backward()
    assert tuple(ragged.shape) == (sum(n_cand),) and not ragged.requires_grad and torch.equal(off.cpu(), cand_off)
    got = {"loss": loss.detach().cpu(), "d_x_hist": rows["x_hist"].grad.cpu(), "d_x_cand": rows["x_cand"].grad.cpu()}
    got.update({"d_" + n: p.grad.detach().cpu() for n, p in zip(CR.PARAMS, enc._params())})
    _hold_measured(case, got, measured, keys=["loss", "d_x_hist", "d_x_cand"])
