"""The LSTUR baseline's kernels (csrc/gru.hip) and mirror classes against the float64 restatement of tests/lstur_ref.py, at the smallest
shapes that take every loop twice and fire every guard (lstur_ref.GRU_SHAPES / USER_SHAPES / STRIDED_SHAPE): the golden shape with and
without an initial state, the shipped widths 868 -> 868 and 868 -> 434 (no multiple of 64: every K loop ends in a partial trip), S = 1,
all lengths 1 (every later step fully masked), all lengths S, B = 1, B = 9 (one past the 8-row tile), H = 1 and 5 (one past a
workgroup's four units), the bounds I = H = 1024 and S = 256, 1095 stacked rows, I != H both ways, and the channel view of a wider
tensor read in place.

Every output has sigma / tanh inside: the MEASURED bar of tests/side_ops_ref.py — 8 x the error of the float32 CPU evaluation of the same
restatement, which runs the same S steps.  Every test prints its errors next to the bars and records them with ``measured``
(profiles/lstur/measured_tolerances.json is that record from an MI355X)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import lstur_ref as LR
import side_ops_ref as R
from manner_amd import hip, train
from manner_amd.config import PRESETS
from manner_amd.models.components.news_encoder import LSTURCategoryEncoder, LSTURNewsEncoder
from manner_amd.models.components.user_encoder import LSTURUserEncoder
from manner_amd.weights import make_mha_pool_weights, make_plm_weights
from test_gpu_caum import _close
from test_gpu_side_ops import _hold_measured, _run
from test_lstur_host import golden_case, golden_want
from test_oracle_golden import compare_train_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
USER_PARAMS = ("table",) + LR.GRU_PARAMS


def _gru(x, w_ih, w_hh, b_ih, b_hh, h0=None, *, lengths, channels=None):
    if channels is not None:
        x = x[:, :, channels[0]:channels[1]]
    return {"out": train.gru_last_hidden(x, lengths, w_ih, w_hh, b_ih, b_hh, h0)}


def _user(x, table, w_ih, w_hh, b_ih, b_hh, *, user, lengths, method, p=0.0, seed=0):
    return {"out": train.lstur_user(user, x, lengths, [table, w_ih, w_hh, b_ih, b_hh], method, p=p, seed=seed)}


def _on_device(case):
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    cs = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in case.consts.items()}
    return lv, cs


def _same_bits(a, b):
    return all(torch.equal(v, b[k]) for k, v in a.items())


# ------------------------------------------------------------------------------------------------ the GRU
@pytest.mark.parametrize("shape", LR.GRU_SHAPES, ids=lambda s: "B{}-S{}-I{}-H{}-{}-{}".format(*s[:5], "h0" if s[5] else "zero"))
def test_gru_forward_and_backward(shape, measured):
    case = LR.gru_case(*shape)
    got = _run(case, _gru)
    _hold_measured(case, got, measured)
    lv, cs = _on_device(case)
    again = hip.gru_last_hidden(lv["x"], cs["lengths"], *[lv[n] for n in LR.GRU_PARAMS], lv.get("h0"))          # the inference wrapper
    assert torch.equal(again.cpu(), got["out"])
    assert _same_bits(_run(case, _gru), got)                                                                    # fixed-order reductions
    lens = case.consts["lengths"]
    for b in range(min(shape[0], 16)):
        assert not got["d_x"][b, int(lens[b]):].any()                                                            # exactly 0 past the length
    hip.check_status(DEV)


def test_gru_reads_a_strided_channel_view(measured):
    """the MINS form: I = H = 8, channels 8 .. 15 of a 24-wide tensor, no initial state — read in place, same bits as a contiguous copy"""
    case = LR.strided_case()
    got = _run(case, _gru)
    _hold_measured(case, got, measured)
    lv, cs = _on_device(case)
    lo, hi = cs["channels"]
    view = lv["x"][:, :, lo:hi]
    assert not view.is_contiguous()
    params = [lv[n] for n in LR.GRU_PARAMS]
    assert torch.equal(hip.gru_last_hidden(view, cs["lengths"], *params), hip.gru_last_hidden(view.contiguous(), cs["lengths"], *params))
    assert torch.equal(hip.gru_last_hidden(view, cs["lengths"], *params).cpu(), got["out"])
    assert not got["d_x"][:, :, :lo].any() and not got["d_x"][:, :, hi:].any() and got["d_x"][:, 0, lo:hi].any()


@pytest.mark.parametrize("fill", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("which", ["gru", "ini", "con"])
def test_padded_slots_are_never_read(which, fill):
    """x[b, len[b]:] filled with NaN or 1e30 changes no bit of the output or of any gradient, and d x there is exactly 0"""
    case, fn = (LR.gru_case(*LR.GRU_SHAPES[0]), _gru) if which == "gru" else (LR.user_case(4, 5, 6, which), _user)
    base = _run(case, fn)
    x = case.leaves["x"].clone()
    lens = case.consts["lengths"]
    for b in range(x.shape[0]):
        x[b, int(lens[b]):] = fill
    assert torch.isnan(x).any() or float(x.abs().max()) > 9e29
    filled = R.evaluate(fn, dict(case.leaves, x=x), case.consts, case.upstream, torch.float32, DEV)
    assert _same_bits(filled, base)
    for b in range(x.shape[0]):
        assert not filled["d_x"][b, int(lens[b]):].any()
    lv, cs = _on_device(case)
    params = [lv[n] for n in LR.GRU_PARAMS]
    if which == "gru":
        out = hip.gru_last_hidden(x.to(DEV), cs["lengths"], *params, lv["h0"])
    else:
        out = hip.lstur_user(cs["user"], x.to(DEV), cs["lengths"], [lv["table"]] + params, which)
    assert torch.equal(out.cpu(), base["out"])


# ------------------------------------------------------------------------------------------------ the user encoder
@pytest.mark.parametrize("shape", LR.USER_SHAPES, ids=lambda s: "B{}-S{}-I{}-{}".format(*s))
def test_user_encoder_forward_and_backward(shape, measured):
    case = LR.user_case(*shape)
    got = _run(case, _user)
    _hold_measured(case, got, measured)
    lv, cs = _on_device(case)
    again = hip.lstur_user(cs["user"], lv["x"], cs["lengths"], [lv[n] for n in USER_PARAMS], shape[3])
    assert torch.equal(again.cpu(), got["out"])
    assert _same_bits(_run(case, _user), got)                   # a user repeats twice at the most: the table's two-term sums have one order
    used = set(case.consts["user"].tolist()) - {0}
    for row in range(case.leaves["table"].shape[0]):
        assert bool(got["d_table"][row].any()) == (row in used), row        # the padding row and the unused users: exactly 0
    hip.check_status(DEV)


@pytest.mark.parametrize("method", ["ini", "con"])
def test_a_repeated_user_gets_the_sum_of_its_rows(method):
    """users [1, 0, 3, 3] against [1, 0, 3, 4] with row 4 a copy of row 3: the two rows' gradients add up to the repeated user's, bit for bit"""
    case = LR.user_case(4, 5, 6, method)
    assert case.consts["user"].tolist() == [1, 0, 3, 3]
    got = _run(case, _user)
    table = case.leaves["table"].clone()
    table[4] = table[3]
    apart = R.evaluate(_user, dict(case.leaves, table=table), dict(case.consts, user=torch.tensor([1, 0, 3, 4])), case.upstream, torch.float32, DEV)
    assert torch.equal(apart["out"], got["out"])
    assert apart["d_table"][3].any() and apart["d_table"][4].any() and not torch.equal(apart["d_table"][3], apart["d_table"][4])
    assert torch.equal(apart["d_table"][3] + apart["d_table"][4], got["d_table"][3]) and not got["d_table"][4].any()


def _mask_seed(p, rows=4):
    """the first seed whose per-row mask keeps row 0 and drops another of the first ``rows`` (a function of (seed, row) alone)"""
    for seed in range(1, 64):
        keep = train.dropout_mask(seed, hip.LSTUR_DROPOUT_SITE, p, rows, DEV).cpu().bool()
        if keep[0] and not keep.all():
            return seed, keep
    raise AssertionError("no seed in 63 keeps one user and drops another")


@pytest.mark.parametrize("method", ["ini", "con"])
def test_masking_drops_whole_users_by_seed_and_row(method, measured):
    p = 0.5
    case = LR.user_case(4, 5, 6, method)
    lv, cs = _on_device(case)
    table, params = lv["table"], [lv[n] for n in USER_PARAMS]
    h = table.shape[1]
    user = torch.tensor([1, 2, 3, 4], device=DEV)               # distinct users: a dropped one's row shows in the table's gradient
    seed, keep = _mask_seed(p)
    # the rows the GRU starts from (ini) / that are appended (con): exactly 0 or exactly 2 x the embedding row
    rows = hip.user_rows(user, table, torch.empty((4, h), device=DEV), p, seed)
    want = torch.where(keep[:, None].to(DEV), 2.0 * table[user], torch.zeros_like(table[user]))
    assert torch.equal(rows, want)
    leaf = table.clone().requires_grad_(True)
    out = train.lstur_user(user, lv["x"], cs["lengths"], [leaf] + params[1:], method, p=p, seed=seed)
    if method == "con":
        assert torch.equal(out.detach()[:, h:], want)
    else:                                                        # ini: the same call as the p = 0 call started from the masked rows
        direct = hip.gru_last_hidden(lv["x"], cs["lengths"], *params[1:], want)
        assert torch.equal(out.detach(), direct)
    # the mask depends on (seed, row) only: the first two rows of the batch alone get the same rows
    two = train.lstur_user(user[:2], lv["x"][:2], cs["lengths"][:2], params, method, p=p, seed=seed)
    assert torch.equal(two, out.detach()[:2])
    (out * case.upstream["out"].to(DEV)).sum().backward()
    for b in range(4):
        assert bool(leaf.grad[int(user[b])].any()) == bool(keep[b]), b        # a dropped user's row gets zero gradient
    # the kept rows' gradient carries the 1 / (1 - p): held to the restatement with this keep-mask
    masked = R.Case(str(case) + "-masked", case.fn, case.leaves, dict(case.consts, user=user.cpu(), p=p, keep=keep.to(torch.uint8)), case.upstream)
    got = R.evaluate(_user, case.leaves, dict(case.consts, user=user.cpu(), p=p, seed=seed), case.upstream, torch.float32, DEV)
    _hold_measured(masked, got, measured, keys=["out", "d_x", "d_table", "d_w_hh"])


def _mirror(z, method, p=0.0):
    shape = json.loads(str(z["meta"]))["shape"]
    enc = LSTURUserEncoder(num_users=shape["num_users"], input_dim=shape["I"], user_masking_probability=p, long_short_term_method=method)
    enc.load_state_dict({k[len(f"user_{method}_sd:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"user_{method}_sd:")}, strict=True)
    return enc.to(DEV)


@pytest.fixture(scope="module")
def lstur_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "lstur.npz"))
    return z, json.loads(str(z["meta"]))


@pytest.mark.parametrize("method", ["ini", "con"])
def test_user_encoder_mirror_matches_the_reference(lstur_golden, method, measured):
    """the mirror class, loaded through load_state_dict, against the reference's own float32 outputs and gradients at the MEASURED bar of
    the golden's values (no tighter than 8 half-ulps, as the host test holds the restatement to them)"""
    z, _ = lstur_golden
    case = R.Case("golden-" + method, LR.lstur_user, *golden_case(z, method))
    ref64, ref32 = case.ref(torch.float64), case.ref(torch.float32)
    enc = _mirror(z, method).train()
    user, lengths = torch.from_numpy(z["user"]).to(DEV), torch.from_numpy(z["lengths"]).to(DEV)
    x = torch.from_numpy(z["user_x"]).to(DEV).requires_grad_(True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = enc(user, x, lengths)
    assert not [w for w in caught if "dropout2d" in str(w.message).lower()]                                      # torch's 3-D input warning
    (out * torch.from_numpy(z[f"user_{method}_up"]).to(DEV)).sum().backward()
    got = {"out": out.detach().cpu(), "d_x": x.grad.cpu()}
    got.update({"d_" + name: dict(enc.named_parameters())[key].grad.cpu() for name, key in LR.STATE_KEYS.items()})
    rec, bad = {}, {}
    for k, w in golden_want(z, method, "user").items():
        bar = R.MEASURED_FACTOR * max(R.rel_to_max(ref32[k], ref64[k]), R.U32)
        err = R.rel_to_max(got[k], torch.from_numpy(np.asarray(w)))
        print(f"golden-{method} {k}: vs the reference's float32 {err:.3e}  bar {bar:.3e}")
        rec.update({f"{k}_err": err, f"{k}_bar": bar})
        if not err <= bar:
            bad[k] = (err, bar)
    measured(**rec)
    assert not bad, bad
    assert not got["d_table"][0].any()                           # padding_idx
    with torch.no_grad():
        assert torch.equal(enc.eval()(user, x.detach(), lengths), out.detach())                                  # the inference route
    hip.check_status(DEV)


@pytest.mark.parametrize("method", ["ini", "con"])
def test_mirror_masks_in_train_only(lstur_golden, method):
    """train() at p = 0.5 draws one seed per call off torch's CPU generator and masks whole users; eval() applies no mask (grad or not)"""
    z, _ = lstur_golden
    plain, masked = _mirror(z, method, 0.0), _mirror(z, method, 0.5)
    user = torch.tensor([1, 2, 3, 4], device=DEV)
    lengths, x = torch.from_numpy(z["lengths"]).to(DEV), torch.from_numpy(z["user_x"]).to(DEV)
    want = plain.eval()(user, x, lengths)
    assert torch.equal(masked.eval()(user, x, lengths), want)
    with torch.no_grad():
        assert torch.equal(masked.eval()(user, x, lengths), want.detach())
    for manual in range(40):
        torch.manual_seed(manual)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        keep = train.dropout_mask(seed, hip.LSTUR_DROPOUT_SITE, 0.5, 4, DEV).cpu().bool()
        if keep.any() and not keep.all():
            break
    torch.manual_seed(manual)
    out = masked.train()(user, x, lengths)
    h = plain.gru.hidden_size
    rows = torch.where(keep[:, None].to(DEV), 2.0 * plain.long_term_user_embedding.weight.detach()[user], torch.zeros(4, h, device=DEV))
    if method == "con":
        assert torch.equal(out.detach()[:, h:], rows) and torch.equal(out.detach()[:, :h], want.detach()[:, :h])
    else:
        g = plain.gru
        assert torch.equal(out.detach(), hip.gru_last_hidden(x, lengths, g.weight_ih_l0.detach(), g.weight_hh_l0.detach(), g.bias_ih_l0.detach(),
                                                             g.bias_hh_l0.detach(), rows))


# ------------------------------------------------------------------------------------------------ the news encoder
def test_category_encoder_mirror_matches_the_reference(lstur_golden):
    z, meta = lstur_golden
    n = meta["news"]
    ce = LSTURCategoryEncoder(num_categories=n["num_categories"], category_embedding_dim=n["category_dim"])
    ce.load_state_dict({k[len("categ_sd:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("categ_sd:")}, strict=True)
    ce = ce.to(DEV)
    out = ce(torch.from_numpy(z["categ_ids"]).to(DEV))
    (out * torch.from_numpy(z["categ_up"]).to(DEV)).sum().backward()
    assert torch.equal(out.detach().cpu(), torch.from_numpy(z["categ_out"]))                                     # a lookup: to the bit
    grad = ce.category_embedding.weight.grad.cpu()
    _close(grad, z["categ_grad:category_embedding.weight"], 1e-6, "category_embedding.weight")
    assert not grad[0].any()                                     # the padding row
    hip.check_status(DEV)


def test_news_encoder_mirror_matches_the_reference(lstur_golden, measured):
    """train() with every dropout probability 0: the text half within 1e-4 and every gradient within 1e-3 of its tensor's largest entry —
    the tolerances the PLMTextEncoder mirror is held to elsewhere (test_gpu_caum.py, test_gpu_train.py); the category half equals the
    table's rows to the bit"""
    z, meta = lstur_golden
    rec = {}
    n = meta["news"]
    cfg = PRESETS[n["preset"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = LSTURNewsEncoder(plm_model=n["preset"], frozen_layers=n["frozen_layers"], text_embedding_dim=cfg.hidden, num_attention_heads=n["text_heads"],
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
    t = cfg.hidden
    table = enc.category_encoder.category_embedding.weight.detach()
    with torch.no_grad():
        ev = enc.eval()(news)
    _close(ev[:, :t], z["news_out_eval"][:, :t], 1e-4, "eval text", rec)
    assert torch.equal(ev[:, t:], table[news["category"]])
    out = enc.train()(news)
    assert tuple(out.shape) == tuple(z["news_out"].shape) == (len(z["news_categ"]), t + n["category_dim"])
    _close(out[:, :t], z["news_out"][:, :t], 1e-4, "text", rec)
    assert torch.equal(out.detach()[:, t:], table[news["category"]]) and torch.equal(out.detach()[:, t:].cpu(), torch.from_numpy(z["news_out"][:, t:]))
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


# ------------------------------------------------------------------------------------------------ refusals and input errors
def _shaped(b, s, i, h):
    x, lengths = R.randn(1, b, s, i).to(DEV), torch.full((b,), s, dtype=torch.int64, device=DEV)
    return x, lengths, [R.randn(2, 3 * h, i, scale=0.1).to(DEV), R.randn(3, 3 * h, h, scale=0.1).to(DEV), R.randn(4, 3 * h, scale=0.1).to(DEV),
                        R.randn(5, 3 * h, scale=0.1).to(DEV)]


@pytest.mark.parametrize("shape,limit", [((1, 257, 4, 4), r"S=257 unsupported \(S <= 256\)"), ((1, 2, 1028, 4), r"I=1028 unsupported \(I <= 1024\)"),
                                         ((1, 2, 4, 1028), r"H=1028 unsupported \(H <= 1024\)")], ids=["S257", "I1028", "H1028"])
def test_gru_refuses_shapes_past_its_bounds(shape, limit):
    x, lengths, params = _shaped(*shape)
    b, s, i, h = shape
    with pytest.raises(RuntimeError, match="gru: " + limit):
        hip.gru_last_hidden(x, lengths, *params)
    with pytest.raises(RuntimeError, match="gru: " + limit):
        train.gru_last_hidden(x.requires_grad_(True), lengths, *params)
    if i == h:                                                   # the user encoder's wrappers reach the same entry
        table, user = R.randn(6, 3, h).to(DEV), torch.ones(b, dtype=torch.int64, device=DEV)
        for wrapper in (hip.lstur_user, train.lstur_user):
            with pytest.raises(RuntimeError, match="gru: " + limit):
                wrapper(user, x.detach(), lengths, [table] + params, "ini")
    lib = hip._lib.load()
    buf = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    p = hip._ptr(buf)
    with pytest.raises(RuntimeError, match="gru_backward: " + limit):
        hip._lib.check(lib.manner_hip_gru_backward(p, p, hip._ptr(lengths), p, h, b, s, i, h, p, buf.numel(), p, p, p, p, p, p, p, buf.numel(), hip._stream()))
    case = LR.gru_case(*LR.GRU_SHAPES[0])                        # the library is still usable
    assert torch.isfinite(_run(case, _gru)["out"]).all()


@pytest.mark.parametrize("what", ["length-0", "length-S+1", "user-id"])
def test_bad_lengths_and_user_ids_raise_at_the_status_check(what):
    """a length 0, a length S + 1 and a user id = num_users set a bit in the device status word: ``check_status`` raises, nothing faults, and
    the next call is clean"""
    case = LR.user_case(4, 5, 6, "ini")
    lv, cs = _on_device(case)
    params = [lv[n] for n in USER_PARAMS]
    hip.check_status(DEV)
    user, lengths = cs["user"].clone(), cs["lengths"].clone()
    if what == "length-0":
        lengths[2] = 0
    elif what == "length-S+1":
        lengths[2] = 6
    else:
        user[2] = lv["table"].shape[0]
    out = hip.lstur_user(user, lv["x"], lengths, params, "ini")
    with pytest.raises(RuntimeError, match="manner_hip input error"):
        hip.check_status(DEV)
    assert torch.isfinite(out).all()
    good = hip.lstur_user(cs["user"], lv["x"], cs["lengths"], params, "ini")
    hip.check_status(DEV)
    rows = [0, 1, 3]
    assert torch.equal(out[rows], good[rows])                   # the other rows are untouched by the bad one
    x = lv["x"].clone().requires_grad_(True)
    train.lstur_user(user, x, lengths, params, "ini").sum().backward()
    with pytest.raises(RuntimeError, match="manner_hip input error"):
        hip.check_status(DEV)
    assert torch.isfinite(x.grad).all()
