"""The kernels of csrc/aspect.hip — TANR's topic head with its cross-entropy, SentiRec's sentiment head with its L1 loss and its
diversity regulariser — and ``hotpath.tanr_train_step`` / ``sentirec_train_step`` against the float64 restatements of
tests/aspect_step_ref.py.

Shapes: ``aspect_step_ref.HEAD_SHAPES`` says next to each (N, D, O) which loop of the kernels it is the smallest shape for (the second
row of a wave, the D tail, the second workgroup, the LDS staging below and above 64 KB and the unstaged weight, the trips of the mean
kernel, the chunks of the weight gradient and their cap, the grid-stride trip, each class-count instance of the weight-gradient kernel);
the L1 head runs at the same (N, D).  The regulariser runs at B = 1 / 4 / 5 with candidate counts cycled from (65, 130, 63, 2, 64, 1) — a
lane's second and third candidate, a wave with one live lane — history lengths from (1, 2, 50), and ``c_max`` equal to and larger than
the largest count.

Bars (tests/side_ops_ref.py, used as they are): DERIVED for the optional logits output (n = D) and for the finite gradients beside an
empty history; MEASURED for the three losses, all their gradients and the two steps.  Every test prints its errors next to the bars and
records them with ``measured`` (profiles/aspect/measured_tolerances.json is that record from an MI355X).  No entry is left out of a
comparison; the kinks of |.| and relu are kept away from by the inputs (aspect_step_ref's docstring)."""
import pytest
import torch
from torch import nn

import aspect_step_ref as A
import side_ops_ref as R
from manner_amd import hip, hotpath, train
from manner_amd.models.components.user_encoder import NAMLUserEncoder, NRMSUserEncoder
from test_gpu_miner import _encoder, miner_golden  # noqa: F401  (the tiny-preset encoder of the leaf tests and its fixture)
from test_gpu_miner_step import _segments, _StubEncoder, _tokens
from test_gpu_side_ops import _hold_measured, _run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEAD_IDS = ["N{}-D{}-O{}".format(*s) for s in A.HEAD_SHAPES]


def _ce(x, weight, bias, target):
    return {"loss": train.head_ce_loss(x, weight, bias, target)}


def _l1(x, weight, bias, target):
    return {"loss": train.head_l1_loss(x, weight, bias, target)}


def _div(scores, cand_score, hist_score, hist_off, cand_off, c_max):
    return {"loss": train.senti_div_loss(scores, cand_score, hist_score, hist_off, cand_off, c_max)}


def _on_dev(case):
    return {k: v.to(DEV) for k, v in case.leaves.items()}, {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in case.consts.items()}


# ------------------------------------------------------------------------------------------------ the topic head
@pytest.mark.parametrize("shape", A.HEAD_SHAPES, ids=HEAD_IDS)
def test_head_ce_forward_and_backward(shape, measured):
    case = A.ce_case(*shape)
    got = _run(case, _ce)
    _hold_measured(case, got, measured)
    assert all(torch.equal(v, got[k]) for k, v in _run(case, _ce).items())             # fixed-order sums: the same bits
    lv, cs = _on_dev(case)
    plain = hip.head_ce_loss(lv["x"], lv["weight"], lv["bias"], cs["target"])
    loss, logits = hip.head_ce_loss(lv["x"], lv["weight"], lv["bias"], cs["target"], return_logits=True)
    assert torch.equal(plain.cpu(), got["loss"]) and torch.equal(loss.cpu(), got["loss"])    # the inference wrapper: the same kernel
    (value, n), (absolute, _) = A.ce_logits_terms(case), A.ce_logits_terms(case, absolute=True)
    ratio = R.derived_ratio(logits.cpu().numpy(), value, absolute, n)
    print(f"{case} logits: error / derived bound = {ratio:.3f} (bar 1, n = {n})")
    measured(logits_over_bound=ratio, bar=1.0)
    assert tuple(logits.shape) == (shape[0], shape[2]) and ratio <= 1.0, (case, ratio)
    hip.check_status(DEV)


def test_head_ce_honours_null_gradient_pointers():
    """a frozen head asks for d x alone, detached rows for d W and d b alone: the same bits as the full backward"""
    case = A.ce_case(9, 260, 19)
    full = _run(case, _ce)
    lv, cs = _on_dev(case)
    x = lv["x"].clone().requires_grad_(True)
    train.head_ce_loss(x, lv["weight"], lv["bias"], cs["target"]).mul(case.upstream["loss"].to(DEV)).backward()
    assert torch.equal(x.grad.cpu(), full["d_x"])
    w, b = lv["weight"].clone().requires_grad_(True), lv["bias"].clone().requires_grad_(True)
    train.head_ce_loss(lv["x"], w, b, cs["target"]).mul(case.upstream["loss"].to(DEV)).backward()
    assert torch.equal(w.grad.cpu(), full["d_weight"]) and torch.equal(b.grad.cpu(), full["d_bias"])
    b_only = lv["bias"].clone().requires_grad_(True)
    train.head_ce_loss(lv["x"], lv["weight"], b_only, cs["target"]).mul(case.upstream["loss"].to(DEV)).backward()
    assert torch.equal(b_only.grad.cpu(), full["d_bias"])


def test_head_ce_raises_a_topic_outside_the_table_through_the_status_word(measured):
    case = A.ce_case(9, 260, 19)
    lv, cs = _on_dev(case)
    hip.check_status(DEV)
    for value in (19, -1):
        bad = cs["target"].clone()
        bad[4] = value
        loss = hip.head_ce_loss(lv["x"], lv["weight"], lv["bias"], bad)
        with pytest.raises(RuntimeError, match="index outside the table"):
            hip.check_status(DEV)
        assert torch.isfinite(loss)                                # the class was never used as an index
    hip.check_status(DEV)
    _hold_measured(case, _run(case, _ce), measured)                # the library is still usable


def test_heads_refuse_shapes_past_their_bounds(measured):
    x, t = R.randn(1, 3, 8).to(DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r"head_ce: O=65 unsupported \(O <= 64\)"):
        hip.head_ce_loss(x, torch.zeros(65, 8, device=DEV), torch.zeros(65, device=DEV), t)
    wide = torch.zeros(3, 1028, device=DEV)
    with pytest.raises(RuntimeError, match=r"head_ce: D=1028 unsupported \(D <= 1024\)"):
        hip.head_ce_loss(wide, torch.zeros(19, 1028, device=DEV), torch.zeros(19, device=DEV), t)
    with pytest.raises(RuntimeError, match=r"head_l1: D=1028 unsupported \(D <= 1024\)"):
        hip.head_l1_loss(wide, torch.zeros(1, 1028, device=DEV), torch.zeros(1, device=DEV), t.float())
    with pytest.raises(ValueError, match="weight \\[1, D\\] expected"):
        hip.head_l1_loss(x, torch.zeros(2, 8, device=DEV), torch.zeros(2, device=DEV), t.float())
    case = A.ce_case(1, 4, 2)
    _hold_measured(case, _run(case, _ce), measured)                # the library is still usable


# ------------------------------------------------------------------------------------------------ the sentiment head
@pytest.mark.parametrize("shape", A.HEAD_SHAPES, ids=["N{}-D{}".format(*s[:2]) for s in A.HEAD_SHAPES])
def test_head_l1_forward_and_backward(shape, measured):
    n, d, _ = shape
    case = A.l1_case(n, d)
    got = _run(case, _l1)
    _hold_measured(case, got, measured)
    assert all(torch.equal(v, got[k]) for k, v in _run(case, _l1).items())
    lv, cs = _on_dev(case)
    assert torch.equal(hip.head_l1_loss(lv["x"], lv["weight"], lv["bias"], cs["target"]).cpu(), got["loss"])
    if n > A.ZERO_ROW:                                             # residual exactly 0: sign(0) = 0, no gradient for the row
        assert float(got["d_x"][A.ZERO_ROW].abs().max()) == 0.0 and float(got["d_x"][A.ZERO_ROW + 1].abs().max()) > 0.0


def test_head_l1_honours_null_gradient_pointers():
    case = A.l1_case(9, 260)
    full = _run(case, _l1)
    lv, cs = _on_dev(case)
    x = lv["x"].clone().requires_grad_(True)
    train.head_l1_loss(x, lv["weight"], lv["bias"], cs["target"]).mul(case.upstream["loss"].to(DEV)).backward()
    assert torch.equal(x.grad.cpu(), full["d_x"])
    w = lv["weight"].clone().requires_grad_(True)
    train.head_l1_loss(lv["x"], w, lv["bias"], cs["target"]).mul(case.upstream["loss"].to(DEV)).backward()
    assert torch.equal(w.grad.cpu(), full["d_weight"])


# ------------------------------------------------------------------------------------------------ the diversity regulariser
@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("b", A.SENTI_B)
def test_senti_div_forward_and_backward(b, padded, measured):
    case = A.senti_case(b, padded)
    got = _run(case, _div)
    _hold_measured(case, got, measured)
    assert all(torch.equal(v, got[k]) for k, v in _run(case, _div).items())
    lv, cs = _on_dev(case)
    assert torch.equal(hip.senti_div_loss(lv["scores"], **cs).cpu(), got["loss"])
    neutral = case.consts["cand_score"] == 0
    blocked = case.ref()["d_scores"] == 0
    assert bool(neutral.any()) and torch.equal(got["d_scores"] == 0, blocked)          # exactly 0 where the product is <= 0
    hip.check_status(DEV)


def test_senti_div_empty_history_is_nan_by_position(measured):
    """the loss is NaN, and so are the gradients of the candidates of the user without history; every other gradient is finite and held
    to the DERIVED bar of a product behind an h-term mean: |got - ref| <= (h + 4) 2^-24 |ref| (u: h - 1 additions and a division; u s;
    g / (B c_max); their product)"""
    case = A.senti_empty_case()
    got, ref = _run(case, _div), case.ref()
    assert torch.isnan(got["loss"]) and torch.isnan(ref["loss"])
    nan = torch.isnan(ref["d_scores"])
    assert bool(nan.any()) and torch.equal(torch.isnan(got["d_scores"]), nan)
    ho, co = case.consts["hist_off"], case.consts["cand_off"]
    h = torch.repeat_interleave(ho[1:] - ho[:-1], co[1:] - co[:-1])
    ok = ~nan
    ratio = R.derived_ratio(got["d_scores"][ok].numpy(), ref["d_scores"][ok].numpy(), ref["d_scores"][ok].abs().numpy(), h[ok].numpy())
    print(f"{case} finite d_scores: error / derived bound = {ratio:.3f} (bar 1)")
    measured(d_scores_over_bound=ratio, bar=1.0)
    assert ratio <= 1.0
    lv, cs = _on_dev(case)
    assert torch.isnan(hip.senti_div_loss(lv["scores"], **cs))


def test_senti_div_refuses_a_c_max_below_the_largest_count(measured):
    case = A.senti_case(4, False)                                  # counts 65, 130, 63, 2
    lv, cs = _on_dev(case)
    with pytest.raises(RuntimeError, match=r"senti_div: c_max=64 below the largest candidate count"):
        hip.senti_div_loss(lv["scores"], **dict(cs, c_max=64))    # 4 x 64 < 260: known on the host
    with pytest.raises(RuntimeError, match=r"senti_div: c_max=0 below"):
        hip.senti_div_loss(lv["scores"], **dict(cs, c_max=0))
    hip.check_status(DEV)
    hip.senti_div_loss(lv["scores"], **dict(cs, c_max=100))       # 4 x 100 >= 260, but impression 1 has 130: known on the device only
    with pytest.raises(RuntimeError, match="manner_hip input error"):
        hip.check_status(DEV)
    hip.check_status(DEV)
    _hold_measured(case, _run(case, _div), measured)               # the library is still usable


# ------------------------------------------------------------------------------------------------ the two training steps
def _params(*modules):
    return [(f"{i}.{n}", p) for i, m in enumerate(modules) for n, p in m.named_parameters()]


def _zero(*modules):
    for _, p in _params(*modules):
        p.grad = None


def _step_batch(cs, ids, mask, with_max=True):
    nh, t = int(cs["hist_off"][-1]), int(cs["cand_off"][-1])
    pick_h, pick_c = torch.arange(nh, device=DEV) % ids.shape[0], (torch.arange(t, device=DEV) * 2 + 1) % ids.shape[0]
    batch = {"users": torch.arange(len(A.STEP_HIST), device=DEV), "batch_hist": _segments(cs["hist_off"]), "batch_cand": _segments(cs["cand_off"]),
             "x_hist": {"text": {"input_ids": ids[pick_h], "attention_mask": mask[pick_h]}, "category": cs["hist_topic"].to(DEV),
                        "sentiment_score": cs["hist_score"].to(DEV)},
             "x_cand": {"text": {"input_ids": ids[pick_c], "attention_mask": mask[pick_c]}, "category": cs["cand_topic"].to(DEV),
                        "sentiment_score": cs["cand_score"].to(DEV)},
             "labels": cs["labels"].to(DEV)}
    if with_max:
        batch.update(hist_max=max(A.STEP_HIST), cand_max=max(A.STEP_CAND))
    return batch


def _composed(kind, rows, user_encoder, head, cs, dtype):
    """the same step from train.* pieces, its loss lines restated on the CPU in ``dtype`` -> {loss, d_<every trainable>, d_rows}"""
    nh, t, s, c_max = int(cs["hist_off"][-1]), int(cs["cand_off"][-1]), max(A.STEP_HIST), cs["c_max"]
    ho, co = cs["hist_off"].to(DEV), cs["cand_off"].to(DEV)
    leaf = rows.detach().clone().requires_grad_(True)
    hist, cand = leaf[:nh], leaf[nh:]
    user = user_encoder(train.to_dense(hist, ho, s))
    dense = train.dot(user.unsqueeze(1), train.to_dense(cand, co, c_max).permute(0, 2, 1))
    ragged = dense.reshape(-1).index_select(0, train.dense_slots(co, t, c_max))

    def cpu(v):
        return v.cpu().to(dtype)
    if kind == "tanr":
        loss = A.tanr_loss_lines(cpu(ragged), cpu(hist), cpu(cand), cpu(head.weight), cpu(head.bias), cs["hist_topic"], cs["cand_topic"], cs["labels"],
                                 cs["cand_off"], c_max)["loss"]
    else:
        loss = A.sentirec_loss_lines(cpu(ragged), cpu(hist), cpu(cand), cpu(head.weight), cpu(head.bias), cs["hist_score"], cs["cand_score"],
                                     cs["labels"], cs["hist_off"], cs["cand_off"], c_max)["loss"]
    _zero(user_encoder, head)
    (loss * 0.75).backward()
    out = {"loss": loss.detach().cpu(), "d_rows": leaf.grad.detach().cpu()}
    out.update({"d_" + n: p.grad.detach().cpu().clone() for n, p in _params(user_encoder, head)})
    return out


@pytest.mark.parametrize("kind", ["tanr", "sentirec"])
def test_train_step_matches_the_step_composed_with_the_restated_losses(kind, miner_golden, measured):  # noqa: F811
    """``tanr_train_step`` / ``sentirec_train_step`` over the tiny-preset encoder, B = 3: the loss and the gradients of the head, of the
    user encoder and of the news rows against the same step composed from ``train.*`` pieces with the loss lines restated in float64 on
    the CPU; MEASURED bar: 8 x the error of that composition with the loss lines in float32 on the CPU.  The head's initialisation and the
    batch's aspects are drawn with the first salt at which those float32 figures are settled (side_ops_ref's docstring).  Under
    ``torch.no_grad()`` the step gives the bits of the grad-mode forward."""
    z, meta = miner_golden
    d, q = meta["news_embedding_dim"], 24
    enc, _ = _encoder(z, meta, apply_reduce_dim=True, text_embedding_dim=128, news_embedding_dim=d)
    enc.train_precision = "fp32"
    enc.train()
    seen = []
    enc.register_forward_hook(lambda _m, _i, out: (out.retain_grad() if out.requires_grad else None, seen.append(out))[1])
    ids, mask = torch.from_numpy(z["enc_ids"]).to(DEV), torch.from_numpy(z["enc_mask"]).to(DEV)
    torch.manual_seed(11)
    if kind == "tanr":
        user_encoder, o = NAMLUserEncoder(news_embedding_dim=d, query_vector_dim=q).to(DEV), A.STEP_TOPICS
    else:
        user_encoder, o = NRMSUserEncoder(news_embedding_dim=d, num_attention_heads=d // 8, query_vector_dim=q).to(DEV), 1
    head = nn.Linear(d, o).to(DEV)

    def step(batch):
        if kind == "tanr":
            return hotpath.tanr_train_step(enc, user_encoder, head, batch, A.TOPIC_COEF)
        return hotpath.sentirec_train_step(enc, user_encoder, head, batch, A.SENTI_PRED_COEF, A.SENTI_DIV_COEF)

    for salt in range(32):
        cs = A.step_consts(salt)
        with torch.no_grad():
            head.weight.copy_(R.randn(4400 + salt, o, d, scale=d ** -0.5))
            head.bias.copy_(R.randn(4401 + salt, o, scale=0.1))
        batch = _step_batch(cs, ids, mask)
        _zero(enc, user_encoder, head)
        del seen[:]
        loss, ragged, cand_off = step(batch)
        (loss * 0.75).backward()
        hip.check_status(DEV)
        rows = seen[0]
        assert len(seen) == 1 and rows.shape[0] == int(cs["hist_off"][-1]) + int(cs["cand_off"][-1])      # ONE encoder call, history first
        assert torch.equal(cand_off.cpu(), cs["cand_off"]) and not ragged.requires_grad and ragged.shape == (int(cs["cand_off"][-1]),)
        got = {"loss": loss.detach().cpu(), "d_rows": rows.grad.detach().cpu()}
        got.update({"d_" + n: p.grad.detach().cpu().clone() for n, p in _params(user_encoder, head)})
        assert float(enc.reduce_dim.weight.grad.abs().max()) > 0   # the rows' gradient went on into the news encoder
        ref64, ref32 = (_composed(kind, rows, user_encoder, head, cs, dt) for dt in (torch.float64, torch.float32))
        bars = R.measured_bars(ref64, ref32)
        if all(v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP for v in bars.values()):
            break
    else:
        raise AssertionError("no salt in 32 settles the step")
    rec, bad = {"salt": salt}, {}
    for k in sorted(ref64):
        assert tuple(got[k].shape) == tuple(ref64[k].shape) and torch.isfinite(got[k]).all(), k
        err = R.rel_to_max(got[k], ref64[k])
        print(f"{kind} step {k}: error {err:.3e}  cpu f32 {bars[k]['cpu_f32']:.3e}  bar {bars[k]['bar']:.3e}")
        rec.update({f"{k}_err": err, f"{k}_cpu_f32": bars[k]["cpu_f32"], f"{k}_bar": bars[k]["bar"]})
        if not err <= bars[k]["bar"]:
            bad[k] = (err, bars[k]["bar"])
    measured(**rec)
    assert not bad, bad
    with torch.no_grad():
        quiet, ragged_q, _ = step(batch)
    assert torch.equal(quiet, loss.detach()) and torch.equal(ragged_q, ragged)
    with torch.no_grad():                                          # without hist_max / cand_max: one device read, the same bits
        assert torch.equal(step(_step_batch(cs, ids, mask, with_max=False))[0], quiet)


@pytest.mark.parametrize("kind", ["tanr", "sentirec"])
def test_forward_returns_the_references_pair(kind):
    """``tanr_forward`` / ``sentirec_forward``: scores [B, Cmax] with exact zeros in the padded slots — the bits of the step's ragged
    scores — and the head's output over the candidate rows, then the history rows"""
    cs = A.step_consts()
    nh, t, d, o = int(cs["hist_off"][-1]), int(cs["cand_off"][-1]), 64, (A.STEP_TOPICS if kind == "tanr" else 1)
    rows = R.randn(4500, nh + t, d)
    enc = _StubEncoder(rows).to(DEV)
    torch.manual_seed(12)
    user_encoder = (NAMLUserEncoder(news_embedding_dim=d, query_vector_dim=24) if kind == "tanr" else
                    NRMSUserEncoder(news_embedding_dim=d, num_attention_heads=4, query_vector_dim=24)).to(DEV)
    head = nn.Linear(d, o).to(DEV)
    batch = _step_batch(cs, torch.zeros(1, 1, dtype=torch.int64, device=DEV), torch.ones(1, 1, dtype=torch.int64, device=DEV))
    batch["x_hist"]["text"], batch["x_cand"]["text"] = _tokens(torch.arange(nh)), _tokens(torch.arange(nh, nh + t))
    fwd = hotpath.tanr_forward if kind == "tanr" else hotpath.sentirec_forward
    with torch.no_grad():
        dense, aux = fwd(enc, user_encoder, head, batch)
        ragged, aux_r = fwd(enc, user_encoder, head, batch, dense=False)
        if kind == "tanr":
            step = hotpath.tanr_train_step(enc, user_encoder, head, batch, A.TOPIC_COEF)
        else:
            step = hotpath.sentirec_train_step(enc, user_encoder, head, batch, A.SENTI_PRED_COEF, A.SENTI_DIV_COEF)
        want = torch.cat((hip.linear(rows[nh:].to(DEV), head.weight, head.bias), hip.linear(rows[:nh].to(DEV), head.weight, head.bias)))
    real = torch.arange(max(A.STEP_CAND))[None, :] < torch.tensor(A.STEP_CAND)[:, None]
    assert dense.shape == real.shape and torch.equal(dense.cpu()[real], ragged.cpu()) and float(dense.cpu()[~real].abs().sum()) == 0.0
    assert torch.equal(ragged, step[1]) and tuple(aux.shape) == (nh + t, o) and torch.equal(aux, aux_r) and torch.equal(aux, want)
    hip.check_status(DEV)


def test_train_steps_read_nothing_back_from_the_device():
    cs = A.step_consts()
    nh, t, d = int(cs["hist_off"][-1]), int(cs["cand_off"][-1]), 64
    enc = _StubEncoder(R.randn(4600, nh + t, d)).to(DEV)
    torch.manual_seed(13)
    naml, nrms = NAMLUserEncoder(news_embedding_dim=d, query_vector_dim=24).to(DEV), NRMSUserEncoder(d, 4, 24).to(DEV)
    topic, senti = nn.Linear(d, A.STEP_TOPICS).to(DEV), nn.Linear(d, 1).to(DEV)
    batch = _step_batch(cs, torch.zeros(1, 1, dtype=torch.int64, device=DEV), torch.ones(1, 1, dtype=torch.int64, device=DEV))
    batch["x_hist"]["text"], batch["x_cand"]["text"] = _tokens(torch.arange(nh)), _tokens(torch.arange(nh, nh + t))

    def both():
        a = hotpath.tanr_train_step(enc, naml, topic, batch, A.TOPIC_COEF)[0]
        a.backward()
        b = hotpath.sentirec_train_step(enc, nrms, senti, batch, A.SENTI_PRED_COEF, A.SENTI_DIV_COEF)[0]
        b.backward()
        return a.detach(), b.detach()

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
