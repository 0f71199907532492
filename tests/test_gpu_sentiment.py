"""The sentiment annotator on the MI355X: manner_hip_seqcls_head alone against the float64 restatement of tests/sentiment_ref.py at
the row counts around both panel heights and at hidden sizes that are and are not multiples of the K staging; a row's bits whatever
the call around it; the rule's branches, a tie and non-finite rows by construction; and the annotator end to end against the golden
written from the reference's own class (tests/golden/make_golden_sentiment.py).

probs and score are held to the MEASURED bar (8 x the float32 CPU evaluation's error against float64, relative to the tensor's
largest entry, floored at 2^-25); labels on every row whose float64 top-2 gap is at least 10 x that bar.  The one-row call runs row 0
of the 300-row case and is held to that case's bars (sentiment_ref.single_row_case says why).  The figures are recorded with
``measured`` (profiles/sentiment/measured_tolerances.json is that record from an MI355X)."""
import numpy as np
import pytest
import torch

import sentiment_ref as SR
from manner_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _head(inp, pos, neg, with_probs=True, x=None):
    label, score, probs = hip.seqcls_head(_dev(inp["x"]) if x is None else x, _dev(inp["dense_w"]), _dev(inp["dense_b"]), _dev(inp["out_w"]),
                                          _dev(inp["out_b"]), pos, neg, with_probs=with_probs)
    return label.cpu().numpy(), score.cpu().numpy(), None if probs is None else probs.cpu().numpy()


def _hold(tag, case, label, score, probs, rec, bad):
    ref, bars = case["ref"], case["bars"]
    got = {"score": score} if probs is None else {"probs": probs, "score": score}
    for k, v in got.items():
        assert v.shape == ref[k].shape and np.isfinite(v).all(), (tag, k)
        err = SR.rel_to_max(v, ref[k], case["scale"][k])
        print(f"{tag} {k}: error {err:.3e}  cpu f32 {bars[k]['cpu_f32']:.3e}  bar {bars[k]['bar']:.3e}")
        for name, val in ((f"{k}_err", err), (f"{k}_cpu_f32", bars[k]["cpu_f32"]), (f"{k}_bar", bars[k]["bar"])):
            rec[name] = max(rec.get(name, 0.0), val)
        if not err <= bars[k]["bar"]:
            bad[(tag, k)] = (err, bars[k]["bar"])
    held = case["held"]
    assert len(held) == 1 or (~held).mean() <= SR.LOW_GAP_SHARE, tag
    wrong = int((label[held] != ref["label"][held]).sum())
    rec["rows_not_held"] = rec.get("rows_not_held", 0) + int((~held).sum())
    if wrong:
        bad[(tag, "label")] = wrong


@pytest.mark.parametrize("nl", SR.HEAD_L)
@pytest.mark.parametrize("h", SR.HEAD_H)
def test_head_against_float64(h, nl, measured):
    pos, neg = (nl - 1, 0) if nl >= 2 else (-1, -1)
    rec, bad = {}, {}
    for n in SR.HEAD_N:
        case = SR.head_case(n, h, nl, pos, neg)
        label, score, probs = _head(case["inputs"], pos, neg)
        assert label.dtype == np.int32 and probs.shape == (n, nl)
        _hold(f"N={n} H={h} L={nl}", case, label, score, probs, rec, bad)
    measured(**rec)
    assert not bad, bad


@pytest.mark.parametrize("n", [65, 8321])
def test_head_strided_rows_without_probs_or_named_classes(n, measured):
    h, nl = 128, 3
    case = SR.head_case(n, h, nl, -1, -1, seed0=7)
    wide = torch.full((n, h + 12), float("nan"), device=DEV)                 # ldx = H + 12: the pad is never read
    wide[:, :h] = _dev(case["inputs"]["x"])
    x = wide[:, :h]
    assert x.stride(0) == h + 12
    label, score, probs = _head(case["inputs"], -1, -1, with_probs=False, x=x)
    assert probs is None
    rec, bad = {}, {}
    _hold(f"N={n} ldx=H+12", case, label, score, None, rec, bad)
    measured(**rec)
    assert not bad, bad
    ref = case["ref"]
    a = ref["label"]
    third = (1 - ref["probs"][np.arange(n), a]) * (ref["probs"][:, -1] - ref["probs"][:, 0])
    assert np.allclose(ref["score"], third, rtol=0, atol=1e-15)              # no class is named: every row takes the third branch


def test_a_rows_bits_do_not_depend_on_the_call():
    h, nl = 768, 3
    for n, places in ((300, (0, 299)), (8400, (0, 4100, 8399))):              # the 32-row panel, then the 128-row one
        inp = SR.head_inputs(n, h, nl, seed=11)
        dw, db, ow, ob = (_dev(inp[k]) for k in ("dense_w", "dense_b", "out_w", "out_b"))
        row = _dev(inp["x"][17:18])
        alone = hip.seqcls_head(row, dw, db, ow, ob, 2, 0)
        for place in places:
            x = _dev(inp["x"]).clone()
            x[place] = row[0]
            full = hip.seqcls_head(x, dw, db, ow, ob, 2, 0)
            for a, f in zip(alone, full):
                assert torch.equal(a[0], f[place]), (n, place)
        base = hip.seqcls_head(_dev(inp["x"])[:300], dw, db, ow, ob, 2, 0)   # the same 300 rows through either panel
        both = hip.seqcls_head(_dev(inp["x"]), dw, db, ow, ob, 2, 0)
        for a, f in zip(base, both):
            assert torch.equal(a, f[:300]), n


def _constant_logits(bo, pos, neg, x=None, n=3, h=36):
    """Wd = 0, bd = 0: h = tanh(0) = 0 and every row's logits are bo"""
    nl = len(bo)
    inp = {"x": np.ones((n, h), np.float32) if x is None else x, "dense_w": np.zeros((h, h), np.float32), "dense_b": np.zeros(h, np.float32),
           "out_w": np.ones((nl, h), np.float32), "out_b": np.asarray(bo, np.float32)}
    return _head(inp, pos, neg)


@pytest.mark.parametrize("bo,pos,neg,want", [
    ([0.1, 0.2, 3.0], 2, 0, 2), ([3.0, 0.2, 0.1], 2, 0, 0), ([0.5, 3.0, 1.5], 2, 0, 1),       # positive, negative, the third branch
    ([0.1, 0.2, 3.0], 0, 1, 2), ([0.1, 0.2, 3.0], -1, -1, 2), ([3.0, 0.2, 0.1], -1, -1, 0),   # by id2label's ids, not by position
    ([1.0, 2.0, 2.0], 2, 0, 1), ([2.0, 1.0, 2.0], 2, 0, 0), ([2.0, 2.0, 2.0], 1, 2, 0),       # ties: the lowest index
    ([91.0, 88.0, 90.0], 0, 2, 0), ([-200.0, -100.0, -101.0], 2, 0, 1)])                      # the row maximum is subtracted
def test_rule_branches_by_construction(bo, pos, neg, want):
    label, score, probs = _constant_logits(bo, pos, neg)
    ref = SR.from_logits(np.tile(np.asarray(bo, np.float32).astype(np.float64), (3, 1)), pos, neg)
    assert (ref["label"] == want).all()
    assert (label == want).all()
    assert np.abs(probs - ref["probs"]).max() < 1e-6 and np.abs(score - ref["score"]).max() < 1e-6
    assert np.abs(probs.sum(axis=1) - 1).max() < 1e-6


def test_non_finite_rows():
    x = np.ones((5, 36), np.float32)
    x[1, 7], x[3, 0] = np.nan, np.inf                                        # 0 * nan and 0 * inf: rows 1 and 3 alone lose their logits
    label, score, probs = _constant_logits([0.5, 3.0, 1.5], 2, 0, x=x, n=5)
    assert list(label) == [1, -1, 1, -1, 1]
    assert np.isnan(score[[1, 3]]).all() and np.isfinite(score[[0, 2, 4]]).all() and np.isnan(probs[[1, 3]]).all()
    assert score[0] == score[2] == score[4]
    for bad in (np.inf, -np.inf, np.nan):
        label, score, _ = _constant_logits([0.5, bad, 1.5], 2, 0)
        assert (label == -1).all() and np.isnan(score).all()


def test_no_rows():
    inp = SR.head_inputs(1, 36, 3, seed=0)
    label, score, probs = _head(dict(inp, x=np.zeros((0, 36), np.float32)), 2, 0)
    assert label.shape == (0,) and score.shape == (0,) and probs.shape == (0, 3)


# ---------------------------------------------------------------- the annotator end to end against the reference's own class
class StubTokenizer:
    """title key -> its prepared rows, with the HF tokenizer's call signature"""

    def __init__(self, g, pad_id):
        self.g, self.pad_id = g, pad_id

    def __call__(self, text, return_tensors=None, padding=None, truncation=None, max_length=None):
        one = isinstance(text, str)
        idx = [int(t.split("-")[1]) for t in ([text] if one else text)]
        lens = self.g["mask"][idx].sum(axis=1)
        lp = int(lens.max())
        return {"input_ids": torch.from_numpy(self.g["ids"][idx][:, :lp]), "attention_mask": torch.from_numpy(self.g["mask"][idx][:, :lp])}


@pytest.fixture(scope="module")
def sets(golden_dir):
    return SR.golden_sets(golden_dir)


def _annotator(g, precision):
    from manner_amd.data.components.sentiment_annotator import SentimentAnnotator
    cfg, sd = SR.golden_state_dict(g)
    return SentimentAnnotator(tokenizer=StubTokenizer(g, cfg.pad_id), config=SR.hf_config_dict(cfg, g["id2label"]), state_dict=sd, device=DEV,
                              precision=precision)


@pytest.mark.parametrize("st,precision", [("a", "fp32"), ("b", "fp32"), ("w", "fp32"), ("w", "f16x3"), ("a", None), ("w", None)])
def test_annotator_against_the_golden(sets, st, precision, measured):
    g = sets[st]
    ann = _annotator(g, precision)
    assert ann.precision == (precision or ("f16x3" if st == "w" else "fp32"))          # 128-wide backbones cannot tile the split GEMMs
    assert (ann.pos_idx, ann.neg_idx) == SR.pos_neg(g["id2label"])
    out = ann.annotate_tokens(_dev(g["ids"]), _dev(g["mask"]))
    assert out["label_id"].dtype == torch.int32 and out["score"].dtype == torch.float32 and out["probs"].shape == (96, 3)
    assert all(t.is_cuda for t in out.values())
    p_ref = SR.softmax(g["logits"].astype(np.float64))
    e_probs = float(np.abs(out["probs"].cpu().numpy() - p_ref).max())
    e_score = float(np.abs(out["score"].cpu().numpy() - g["score"]).max())
    print(f"set {st} {ann.precision}: probs error {e_probs:.3e}, score error {e_score:.3e} (bar 1e-4)")
    measured(probs_err=e_probs, score_err=e_score, bar=1e-4)
    assert e_probs < 1e-4 and e_score < 1e-4
    held = SR.top2_gap(p_ref) >= 1e-3
    assert np.array_equal(out["label_id"].cpu().numpy()[held], g["label"][held])
    # the reference's call, one title per rule branch, and the batched call
    for cls in range(3):
        i = int(np.argmax(g["label"] == cls))
        name, score = ann(f"title-{i}")
        assert isinstance(name, str) and isinstance(score, float)
        assert name == g["label_name"][i] and abs(score - float(g["score"][i])) < 1e-4
    classes, scores = ann.annotate([f"title-{i}" for i in range(96)], batch_size=40)
    assert [c for c, h in zip(classes, held) if h] == [c for c, h in zip(g["label_name"], held) if h]
    assert scores.dtype == np.float32 and np.abs(scores - g["score"]).max() < 1e-4
    s2i = ann.sentiment2index(classes)
    assert sorted(s2i.values()) == [1, 2, 3] and s2i[classes[0]] == 1


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_annotator_in_16_bit_modes(sets, precision, measured):
    g = sets["w"]
    out = _annotator(g, precision).annotate_tokens(_dev(g["ids"]), _dev(g["mask"]))
    probs, label = out["probs"].cpu().numpy(), out["label_id"].cpu().numpy()
    assert np.abs(probs.sum(axis=1) - 1).max() < 1e-5
    assert ((label >= 0) & (label < 3)).all() and np.isfinite(out["score"].cpu().numpy()).all()
    p_ref = SR.softmax(g["logits"].astype(np.float64))
    measured(probs_err=float(np.abs(probs - p_ref).max()), score_err=float(np.abs(out["score"].cpu().numpy() - g["score"]).max()),
             label_agreement=float((label == g["label"]).mean()))          # recorded, not asserted
