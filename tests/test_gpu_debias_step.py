"""The kernels of csrc/debias.hip — SentiDebias's orthogonality loss, the sentiment side of its scores (``class_dense``,
``class_scores``) and its adversarial head — and ``hotpath.senti_debias_forward`` / ``senti_debias_generator_step`` /
``senti_debias_discriminator_step`` against the float64 restatements of tests/debias_step_ref.py.

Shapes: ``debias_step_ref.ORTH_SHAPES`` / ``RAGGED_SHAPES`` / ``ADV_SHAPES`` say next to each shape which loop of the kernels it is the
smallest shape for (a segment of one row, a wave's second row, the D and H tails, the second workgroup, the chunks of the binned sums and
their cap, the grid-stride trips, the two tiles of the matrix-core linear, W2 staged below and above 64 KB and unstaged, each class-count
instance of the W2 gradient).

Bars: MEASURED of tests/side_ops_ref.py, used as it is, for every output and every gradient.  Every test prints its errors next to the
bars and records them with ``measured`` (profiles/debias/measured_tolerances.json is that record from an MI355X).  No entry is left out
of a comparison; the kinks of |.| are kept away from by the inputs (debias_step_ref's docstring)."""
import pytest
import torch
from torch import nn

import debias_step_ref as D
import side_ops_ref as R
from manner_amd import hip, hotpath, train
from manner_amd.models.components.user_encoder import NRMSUserEncoder
from test_gpu_miner_step import _segments, _StubEncoder, _tokens
from test_gpu_side_ops import _hold_measured, _run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(shapes):
    return ["-".join(str(v) for v in s) for s in shapes]


def _orth(rows, table, user_free, user_aware, cls, n_hist):
    return {"loss": train.orth_loss(rows, n_hist, table, cls, user_free, user_aware)}


def _dense(table, cls, off, width):
    return {"out": train.class_dense(table, cls, off, width)}


def _scores(user, table, cls, off):
    return {"scores": train.class_scores(user, table, cls, off)}


def _adv(rows, w1, b1, w2, b2, cls, n_hist):
    return {"loss": train.adv_loss(rows, n_hist, w1, b1, w2, b2, cls)}


def _on_dev(case):
    return {k: v.to(DEV) for k, v in case.leaves.items()}, {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in case.consts.items()}


def _same_bits(case, fn, got):
    again = _run(case, fn)
    assert all(torch.equal(v, got[k]) for k, v in again.items()), case                 # fixed-order sums: the same bits


def _subset(case, fn, names):
    """the gradients of ``names`` alone (every other leaf without requires_grad: its pointer is NULL in the backward)"""
    lv, cs = _on_dev(case)
    for n in names:
        lv[n] = lv[n].clone().requires_grad_(True)
    out = fn(**lv, **cs)
    sum((out[k] * g.to(DEV)).sum() for k, g in case.upstream.items()).backward()
    return {"d_" + n: lv[n].grad.cpu() for n in names}


# ------------------------------------------------------------------------------------------------ the orthogonality loss
@pytest.mark.parametrize("shape", D.ORTH_SHAPES, ids=_ids(D.ORTH_SHAPES))
def test_orth_loss_forward_and_backward(shape, measured):
    case = D.orth_case(*shape)
    got = _run(case, _orth)
    _hold_measured(case, got, measured)
    _same_bits(case, _orth, got)
    lv, cs = _on_dev(case)
    plain = hip.orth_loss(lv["rows"], cs["n_hist"], lv["table"], cs["cls"], lv["user_free"], lv["user_aware"])
    assert torch.equal(plain.cpu(), got["loss"])                   # the no-graph wrapper: the same kernels
    hip.check_status(DEV)


def test_orth_loss_honours_null_gradient_pointers():
    case = D.orth_case(5, 4, 260, 4, 4)
    full = _run(case, _orth)
    for names in (("rows",), ("table",), ("user_free",), ("user_aware",), ("rows", "user_aware"), ("table", "user_free")):
        for k, v in _subset(case, _orth, names).items():
            assert torch.equal(v, full[k]), (names, k)


def test_orth_loss_empty_history_is_nan():
    case = D.orth_case(5, 4, 260, 4, 4)
    lv, cs = _on_dev(case)
    assert torch.isnan(hip.orth_loss(lv["rows"], 0, lv["table"], cs["cls"], lv["user_free"], lv["user_aware"]))
    assert torch.isnan(hip.orth_loss(lv["rows"], 9, lv["table"], cs["cls"], lv["user_free"], lv["user_aware"]))
    hip.check_status(DEV)


def test_orth_loss_zero_row_gets_torchs_zero_through_its_norm(measured):
    """news row 2 is all zero: its cosine is 0, its gradient T[cls] / 1e-8 with nothing through the norm; that row and the others are
    held apart, each to 8 x the float32 CPU error of its own part"""
    case = D.orth_zero_case()
    got, ref64, ref32 = _run(case, _orth), case.ref(torch.float64), case.ref(torch.float32)
    z = D.ZERO_ROW

    def parts(r):
        rest = torch.cat((r["d_rows"][:z], r["d_rows"][z + 1:]))
        return dict({k: v for k, v in r.items() if k != "d_rows"}, d_rows_zero=r["d_rows"][z], d_rows_rest=rest)
    got, ref64, ref32 = parts(got), parts(ref64), parts(ref32)
    bars, bad = R.measured_bars(ref64, ref32), {}
    assert float(ref64["d_rows_zero"].abs().max()) > 1e6
    for k in sorted(ref64):
        assert torch.isfinite(got[k]).all(), k
        err = R.rel_to_max(got[k], ref64[k])
        print(f"{case} {k}: error {err:.3e}  cpu f32 {bars[k]['cpu_f32']:.3e}  bar {bars[k]['bar']:.3e}")
        measured(**{f"{k}_err": err, f"{k}_bar": bars[k]["bar"]})
        if not err <= bars[k]["bar"]:
            bad[k] = (err, bars[k]["bar"])
    assert not bad, bad


def test_a_class_outside_the_table_raises_through_the_status_word(measured):
    case = D.orth_case(5, 4, 260, 4, 4)
    lv, cs = _on_dev(case)
    off = torch.tensor([0, 5, 9], device=DEV)
    adv = D.adv_case(5, 4, 260, 33, 4)
    al, ac = _on_dev(adv)
    hip.check_status(DEV)
    for value in (4, -1):
        bad = cs["cls"].clone()
        bad[4] = value
        calls = (lambda: hip.orth_loss(lv["rows"], cs["n_hist"], lv["table"], bad, lv["user_free"], lv["user_aware"]),
                 lambda: hip.class_dense(lv["table"], bad, off, 6),
                 lambda: hip.class_scores(lv["user_free"][:2], lv["table"], bad, off),
                 lambda: hip.adv_loss(al["rows"], ac["n_hist"], al["w1"], al["b1"], al["w2"], al["b2"], bad))
        for call in calls:
            out = call()
            with pytest.raises(RuntimeError, match="index outside the table"):
                hip.check_status(DEV)
            assert torch.isfinite(out).all()                       # the class was never used as an index
    hip.check_status(DEV)
    _hold_measured(case, _run(case, _orth), measured)              # the library is still usable


def test_shapes_past_the_bounds_are_refused(measured):
    t = torch.zeros(3, dtype=torch.int64, device=DEV)
    off = torch.tensor([0, 3], device=DEV)

    def z(*shape):
        return torch.zeros(*shape, device=DEV)
    with pytest.raises(RuntimeError, match=r"orth_loss: D=1028 unsupported \(D <= 1024\)"):
        hip.orth_loss(z(3, 1028), 1, z(4, 1028), t, z(2, 1028), z(2, 1028))
    with pytest.raises(RuntimeError, match=r"orth_loss: C=65 unsupported \(C <= 64\)"):
        hip.orth_loss(z(3, 8), 1, z(65, 8), t, z(2, 8), z(2, 8))
    with pytest.raises(RuntimeError, match=r"class_dense: C=65 unsupported \(C <= 64\)"):
        hip.class_dense(z(65, 8), t, off, 3)
    with pytest.raises(RuntimeError, match=r"class_dense: width=2 below the largest row count"):
        hip.class_dense(z(4, 8), t, off, 2)
    with pytest.raises(RuntimeError, match=r"class_scores: C=65 unsupported \(C <= 64\)"):
        hip.class_scores(z(1, 8), z(65, 8), t, off)
    with pytest.raises(RuntimeError, match=r"adv_loss: O=65 unsupported \(O <= 64\)"):
        hip.adv_loss(z(3, 8), 1, z(5, 8), z(5), z(65, 5), z(65), t)
    with pytest.raises(RuntimeError, match=r"adv_loss: H=1028 unsupported \(H <= 1024\)"):
        hip.adv_loss(z(3, 8), 1, z(1028, 8), z(1028), z(4, 1028), z(4), t)
    with pytest.raises(RuntimeError, match=r"adv_loss: D=1028 unsupported \(D <= 1024\)"):
        hip.adv_loss(z(3, 1028), 1, z(5, 1028), z(5), z(4, 5), z(4), t)
    with pytest.raises(ValueError, match="0 <= n_hist <= N"):
        hip.adv_loss(z(3, 8), 4, z(5, 8), z(5), z(4, 5), z(4), t)
    hip.class_dense(z(4, 8), torch.zeros(5, dtype=torch.int64, device=DEV), torch.tensor([0, 4, 5], device=DEV), 3)    # 2 x 3 >= 5, but user 0 has 4
    with pytest.raises(RuntimeError, match="manner_hip input error"):
        hip.check_status(DEV)
    hip.check_status(DEV)
    case = D.orth_case(1, 1, 4, 2, 1)
    _hold_measured(case, _run(case, _orth), measured)              # the library is still usable


# ------------------------------------------------------------------------------------------------ the sentiment side of the scores
@pytest.mark.parametrize("shape", D.RAGGED_SHAPES, ids=_ids(D.RAGGED_SHAPES))
def test_class_dense_forward_and_backward(shape, measured):
    case = D.dense_case(*shape)
    got = _run(case, _dense)
    _hold_measured(case, got, measured)
    _same_bits(case, _dense, got)
    lv, cs = _on_dev(case)
    assert torch.equal(hip.class_dense(lv["table"], **cs).cpu(), got["out"])
    assert torch.equal(got["out"], case.ref()["out"].float())      # a copy: the table's bits, and exact zeros in the padded slots
    hip.check_status(DEV)


@pytest.mark.parametrize("shape", D.RAGGED_SHAPES, ids=_ids(D.RAGGED_SHAPES))
def test_class_scores_forward_and_backward(shape, measured):
    case = D.scores_case(*shape)
    got = _run(case, _scores)
    _hold_measured(case, got, measured)
    _same_bits(case, _scores, got)
    lv, cs = _on_dev(case)
    assert torch.equal(hip.class_scores(lv["user"], lv["table"], **cs).cpu(), got["scores"])
    for names in (("user",), ("table",)):
        for k, v in _subset(case, _scores, names).items():
            assert torch.equal(v, got[k]), (names, k)
    hip.check_status(DEV)


# ------------------------------------------------------------------------------------------------ the adversarial head
@pytest.mark.parametrize("shape", D.ADV_SHAPES, ids=_ids(D.ADV_SHAPES))
def test_adv_loss_forward_and_backward(shape, measured):
    case = D.adv_case(*shape)
    got = _run(case, _adv)
    _hold_measured(case, got, measured)
    _same_bits(case, _adv, got)
    lv, cs = _on_dev(case)
    assert torch.equal(hip.adv_loss(lv["rows"], cs["n_hist"], lv["w1"], lv["b1"], lv["w2"], lv["b2"], cs["cls"]).cpu(), got["loss"])
    hip.check_status(DEV)


@pytest.mark.parametrize("shape", [(5, 4, 260, 33, 4), (515, 515, 4, 3, 2)], ids=["9-rows", "1030-rows"])
def test_adv_loss_honours_null_gradient_pointers(shape):
    """the generator step asks for d rows alone, the discriminator step for the four parameter gradients alone: the bits of the full
    backward"""
    case = D.adv_case(*shape)
    full = _run(case, _adv)
    for names in (("rows",), ("w1", "b1", "w2", "b2"), ("b1",), ("w2",), ("w1", "b2")):
        for k, v in _subset(case, _adv, names).items():
            assert torch.equal(v, full[k]), (names, k)


def test_adv_loss_wraps_class_zero_onto_the_last_column():
    """every row of class 0: the loss is that of column O - 1.  Which column was read is decided against the float64 losses of all O
    columns: the kernel's figure lies within a hundredth of the gap to the nearest other column (the gaps are tenths, float32 rounding
    of the loss is near 1e-7)"""
    case = D.adv_case(5, 4, 260, 33, 4)
    lv, cs = _on_dev(case)
    got = float(hip.adv_loss(lv["rows"], cs["n_hist"], lv["w1"], lv["b1"], lv["w2"], lv["b2"], torch.zeros_like(cs["cls"])))
    l64 = {k: v.double() for k, v in case.leaves.items()}
    column = [float(D.adv_loss(**l64, cls=torch.full_like(case.consts["cls"], (k + 1) % 4), n_hist=5)["loss"]) for k in range(4)]
    gap = min(abs(column[k] - column[3]) for k in range(3))
    print(f"{case} all rows of class 0: got {got:.7f}, columns {column}, gap {gap:.3e}")
    assert gap > 1e-3 and abs(got - column[3]) <= 1e-2 * gap
    hip.check_status(DEV)


# ------------------------------------------------------------------------------------------------ the two steps and the forward
class _SentimentEncoder(nn.Module):
    """the reference's SentimentEncoder, by its parameter names; its forward is never called"""

    def __init__(self, classes, e, d):
        super().__init__()
        self.embedding_layer = nn.Embedding(classes, e, padding_idx=0)
        self.linear = nn.Linear(e, d)


class _Discriminator(nn.Module):
    def __init__(self, d, h, o):
        super().__init__()
        self.linear1, self.linear2 = nn.Linear(d, h), nn.Linear(h, o)


STEP_D = 64


def _params(*modules):
    return [(f"{i}.{n}", p) for i, m in enumerate(modules) for n, p in m.named_parameters()]


def _zero(*modules):
    for _, p in _params(*modules):
        p.grad = None


def _step_modules(salt=0):
    torch.manual_seed(21 + salt)
    user_encoder = NRMSUserEncoder(news_embedding_dim=STEP_D, num_attention_heads=4, query_vector_dim=24).to(DEV)
    senti = _SentimentEncoder(D.STEP_CLASSES, D.STEP_E, STEP_D).to(DEV)
    disc = _Discriminator(STEP_D, D.STEP_H, D.STEP_CLASSES).to(DEV)
    with torch.no_grad():
        senti.embedding_layer.weight.copy_(R.randn(5700 + salt, D.STEP_CLASSES, D.STEP_E))        # row 0 too: it is read as it lies
    cs = D.step_consts(salt)
    table = D.class_table(senti.embedding_layer.weight.detach().cpu().double(), senti.linear.weight.detach().cpu().double(),
                          senti.linear.bias.detach().cpu().double())
    enc = _StubEncoder(D.step_rows(STEP_D, cs, table, salt)).to(DEV)
    return enc, user_encoder, senti, disc, cs


def _step_batch(cs, with_max=True):
    nh, t = int(cs["hist_off"][-1]), int(cs["cand_off"][-1])
    batch = {"users": torch.arange(len(D.STEP_HIST), device=DEV), "batch_hist": _segments(cs["hist_off"]), "batch_cand": _segments(cs["cand_off"]),
             "x_hist": {"text": _tokens(torch.arange(nh)), "sentiment": cs["cls_hist"].to(DEV)},
             "x_cand": {"text": _tokens(torch.arange(nh, nh + t)), "sentiment": cs["cls_cand"].to(DEV)}, "labels": cs["labels"].to(DEV)}
    if with_max:
        batch.update(hist_max=max(D.STEP_HIST), cand_max=max(D.STEP_CAND))
    return batch


def _composed(enc, user_encoder, senti, disc, cs, dtype):
    """the generator step with the user encoder's two calls on the device (the mirror, from train.* pieces) and every line of the module
    around them restated on the CPU in ``dtype``, the [N, D] sentiment rows formed as the module forms them; the sentiment encoder's and
    the discriminator's parameters are CPU leaves in ``dtype``, so that their float64 gradients are not rounded to the parameters' float32
    -> {loss, orth, combined, free, d_<every parameter>, d_rows}"""
    nh, s = int(cs["hist_off"][-1]), max(D.STEP_HIST)
    ho = cs["hist_off"].to(DEV)
    leaf = enc.weight.detach().clone().requires_grad_(True)
    own = {n: p.detach().cpu().to(dtype).requires_grad_(True) for n, p in _params(user_encoder, senti, disc) if not n.startswith("0.")}

    def cpu(v):
        return v.cpu().to(dtype)
    senti_rows = [torch.tanh(nn.functional.embedding(c, own["1.embedding_layer.weight"], padding_idx=0) @ own["1.linear.weight"].T + own["1.linear.bias"])
                  for c in (cs["cls_hist"], cs["cls_cand"])]
    user_free = user_encoder(train.to_dense(leaf[:nh], ho, s))
    user_aware = user_encoder(train.to_dense(senti_rows[0].to(DEV).float(), ho, s))
    out = D.generator_lines(cpu(leaf[:nh]), cpu(leaf[nh:]), cpu(user_free), cpu(user_aware), senti_rows[0], senti_rows[1], own["2.linear1.weight"],
                            own["2.linear1.bias"], own["2.linear2.weight"], own["2.linear2.bias"], cs["cls_hist"], cs["cls_cand"], cs["labels"],
                            cs["cand_off"], cs["c_max"])
    _zero(user_encoder)
    (out["loss"] * 0.75).backward()
    res = {k: v.detach().cpu() for k, v in out.items()}
    res["d_rows"] = leaf.grad.detach().cpu()
    res.update({"d_" + n: p.grad.detach().cpu().clone() for n, p in _params(user_encoder)})
    res.update({"d_" + n: v.grad.detach().clone() for n, v in own.items()})
    return res


def _hold(kind, got, ref64, ref32, measured, rec):
    bars, bad = R.measured_bars(ref64, ref32), {}
    for k in sorted(ref64):
        assert tuple(got[k].shape) == tuple(ref64[k].shape) and torch.isfinite(got[k]).all(), k
        err = R.rel_to_max(got[k], ref64[k])
        print(f"{kind} {k}: error {err:.3e}  cpu f32 {bars[k]['cpu_f32']:.3e}  bar {bars[k]['bar']:.3e}")
        rec.update({f"{k}_err": err, f"{k}_cpu_f32": bars[k]["cpu_f32"], f"{k}_bar": bars[k]["bar"]})
        if not err <= bars[k]["bar"]:
            bad[k] = (err, bars[k]["bar"])
    measured(**rec)
    assert not bad, bad


def test_generator_step_and_forward_match_the_restated_module_lines(measured):
    """``senti_debias_generator_step`` over the stub encoder and the mirror NRMSUserEncoder, B = 3: g_loss and the gradients of the news
    rows, the user encoder, the sentiment encoder (embedding row 0: exactly zero) and the discriminator, and ``senti_debias_forward``'s
    loss_orth and dense scores (padded slots exactly 0), against the module's lines restated in float64 on the CPU; MEASURED bar: 8 x
    the error of the same composition with those lines in float32 on the CPU, at the first salt at which those figures are settled."""
    for salt in range(32):
        enc, user_encoder, senti, disc, cs = _step_modules(salt)
        batch = _step_batch(cs)
        _zero(enc, user_encoder, senti, disc)
        loss, ragged, cand_off = hotpath.senti_debias_generator_step(enc, user_encoder, senti, disc, batch, D.ALPHA, D.BETA)
        (loss * 0.75).backward()
        hip.check_status(DEV)
        got = {"loss": loss.detach().cpu(), "d_rows": enc.weight.grad.detach().cpu().clone()}
        got.update({"d_" + n: p.grad.detach().cpu().clone() for n, p in _params(user_encoder, senti, disc)})
        with torch.no_grad():
            combined, free, orth, hist_rows, cand_rows = hotpath.senti_debias_forward(enc, user_encoder, senti, batch)
            combined_r, free_r, orth_r, _, _ = hotpath.senti_debias_forward(enc, user_encoder, senti, batch, dense=False)
            quiet = hotpath.senti_debias_generator_step(enc, user_encoder, senti, disc, batch, D.ALPHA, D.BETA)
        got.update(orth=orth.cpu(), combined=combined.cpu(), free=free.cpu())
        ref64, ref32 = (_composed(enc, user_encoder, senti, disc, cs, dt) for dt in (torch.float64, torch.float32))
        bars = R.measured_bars(ref64, ref32)
        if all(v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP for v in bars.values()):
            break
    else:
        raise AssertionError("no salt in 32 settles the step")
    nh, t = int(cs["hist_off"][-1]), int(cs["cand_off"][-1])
    assert torch.equal(cand_off.cpu(), cs["cand_off"]) and not ragged.requires_grad and ragged.shape == (t,)
    assert float(got["d_1.embedding_layer.weight"][0].abs().max()) == 0.0 and float(got["d_1.embedding_layer.weight"][1:].abs().max()) > 0.0
    assert float(got["d_1.linear.bias"].abs().max()) > 0.0
    _hold("generator step", got, ref64, ref32, measured, {"salt": salt})
    real = torch.arange(max(D.STEP_CAND))[None, :] < torch.tensor(D.STEP_CAND)[:, None]
    for dense, rag in ((combined, combined_r), (free, free_r)):
        assert dense.shape == real.shape and torch.equal(dense.cpu()[real], rag.cpu()) and float(dense.cpu()[~real].abs().sum()) == 0.0
    assert torch.equal(free_r, ragged) and torch.equal(orth, orth_r)
    assert torch.equal(hist_rows, enc.weight[:nh]) and torch.equal(cand_rows, enc.weight[nh:])
    assert torch.equal(quiet[0], loss.detach()) and torch.equal(quiet[1], ragged)      # under no_grad: the same kernels, the same bits
    with torch.no_grad():                                          # without hist_max / cand_max: one device read, the same bits
        assert torch.equal(hotpath.senti_debias_generator_step(enc, user_encoder, senti, disc, _step_batch(cs, False), D.ALPHA, D.BETA)[0], quiet[0])


def test_generator_step_with_a_frozen_discriminator_forms_the_rows_gradient_alone():
    enc, user_encoder, senti, disc, cs = _step_modules()
    batch = _step_batch(cs)
    hotpath.senti_debias_generator_step(enc, user_encoder, senti, disc, batch, D.ALPHA, D.BETA)[0].backward()
    want = enc.weight.grad.clone()
    assert disc.linear1.weight.grad is not None
    _zero(enc, user_encoder, senti, disc)
    for p in disc.parameters():
        p.requires_grad_(False)                                    # toggle_optimizer(optimizer_g)
    hotpath.senti_debias_generator_step(enc, user_encoder, senti, disc, batch, D.ALPHA, D.BETA)[0].backward()
    assert torch.equal(enc.weight.grad, want) and all(p.grad is None for p in disc.parameters())


def test_discriminator_step_matches_the_restated_loss(measured):
    for salt in range(32):
        enc, _, _, disc, cs = _step_modules(salt)
        batch = _step_batch(cs)
        _zero(enc, disc)
        loss = hotpath.senti_debias_discriminator_step(enc, disc, batch)
        (loss * 0.75).backward()
        hip.check_status(DEV)
        assert enc.weight.grad is None                             # the rows are detached
        got = {"loss": loss.detach().cpu()}
        got.update({"d_" + n: p.grad.detach().cpu().clone() for n, p in _params(disc)})
        nh = int(cs["hist_off"][-1])
        refs = []
        for dt in (torch.float64, torch.float32):
            leaves = {n: p.detach().cpu().to(dt).requires_grad_(True) for n, p in _params(disc)}
            out = D.adv_loss(enc.weight.detach().cpu().to(dt), leaves["0.linear1.weight"], leaves["0.linear1.bias"], leaves["0.linear2.weight"],
                             leaves["0.linear2.bias"], torch.cat((cs["cls_hist"], cs["cls_cand"])), nh)["loss"]
            (out * 0.75).backward()
            refs.append(dict({"loss": out.detach()}, **{"d_" + n: v.grad for n, v in leaves.items()}))
        bars = R.measured_bars(*refs)
        if all(v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP for v in bars.values()):
            break
    else:
        raise AssertionError("no salt in 32 settles the step")
    _hold("discriminator step", got, refs[0], refs[1], measured, {"salt": salt})
    with torch.no_grad():
        assert torch.equal(hotpath.senti_debias_discriminator_step(enc, disc, batch), loss.detach())


def test_steps_read_nothing_back_from_the_device():
    enc, user_encoder, senti, disc, cs = _step_modules()
    batch = _step_batch(cs)

    def both():
        g = hotpath.senti_debias_generator_step(enc, user_encoder, senti, disc, batch, D.ALPHA, D.BETA)[0]
        g.backward()
        d = hotpath.senti_debias_discriminator_step(enc, disc, batch)
        d.backward()
        return g.detach(), d.detach()

    want = both()                                                  # warm-up: first-use allocations and module loads
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = both()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
    hip.check_status(DEV)
