"""The sentiment annotator without a GPU: the float64 restatement (tests/sentiment_ref.py) against the golden written from the
reference's own class, each planted defect caught on the golden's inputs, the checkpoint splitter, the first-appearance class map, the
reference's signatures, the install keyword, and the argument checks of manner_hip_seqcls_head (made before any launch)."""
import ctypes as C
import inspect
import sys
import types

import numpy as np
import pytest
import torch

import sentiment_ref as SR


@pytest.fixture(scope="module")
def sets(golden_dir):
    return SR.golden_sets(golden_dir)


@pytest.fixture(scope="module")
def restated(sets):
    """set -> the restatement over the oracle's float64 encoder path (no HF)"""
    import manner_oracle as O
    from manner_amd.weights import split_sequence_classifier
    out, cache = {}, {}
    for st in ("a", "b", "w"):
        g = sets[st]
        cfg, sd = SR.golden_state_dict(g)
        key = "t" if st in ("a", "b") else st
        if key not in cache:
            plm, head = split_sequence_classifier(sd)
            cls = O.encode_cls(g["ids"], g["mask"], {k: torch.from_numpy(np.asarray(v)).double() for k, v in plm.items()}, cfg).numpy()
            cache[key] = (cls, head)
        cls, head = cache[key]
        pos, neg = SR.pos_neg(g["id2label"])
        out[st] = dict(SR.head(cls, head["dense.weight"], head["dense.bias"], head["out.weight"], head["out.bias"], pos, neg), cls=cls, pos=pos,
                       neg=neg)
    return out


@pytest.mark.parametrize("st", ["a", "b", "w"])
def test_restatement_reproduces_the_golden(sets, restated, st):
    g, r = sets[st], restated[st]
    assert np.array_equal(r["label"], g["label"])
    assert [g["id2label"][int(a)] for a in r["label"]] == g["label_name"]
    err64 = np.abs(r["score"] - g["score64"]).max()
    err32 = np.abs(r["score"] - g["score"].astype(np.float64)).max()
    print(f"set {st}: score error vs the reference in float64 {err64:.3e}, vs the reference as it runs (float32) {err32:.3e}")
    assert np.abs(r["logits"] - g["logits64"]).max() < 1e-9
    assert err64 < 1e-6
    # the reference as it runs carries its own float32 rounding: it is held to what the golden itself shows between its two runs
    own32 = np.abs(g["score"].astype(np.float64) - g["score64"]).max()
    assert err32 <= own32 + 1e-6, (err32, own32)


def test_golden_covers_the_rule(sets):
    for st in ("a", "b", "w"):
        g = sets[st]
        share = np.bincount(g["label"], minlength=3) / len(g["label"])
        assert share.min() >= 0.10, (st, share)
        p = SR.softmax(g["logits64"])
        gap = SR.top2_gap(p)
        assert (gap < 1e-3).mean() <= 0.05 and gap.min() >= 1e-5
        pos, neg = SR.pos_neg(g["id2label"])
        assert {pos, neg} < set(range(3)) and len({pos, neg}) == 2          # with >= 10 % per class: all three branches occur
    assert SR.pos_neg(sets["b"]["id2label"]) == (0, 1)                       # the third branch of set b is class 2: it reads p[2] - p[0]


@pytest.mark.parametrize("defect,st", [("neutral_by_name", "b"), ("negative_sign", "a"), ("drop_one_minus", "a"),
                                       ("posneg_by_position", "b")])
def test_planted_rule_defects_change_the_scores(sets, restated, defect, st):
    g, r = sets[st], restated[st]
    bad = SR.from_logits(r["logits"], r["pos"], r["neg"], defect=defect)
    assert np.abs(r["score"] - g["score64"]).max() < 1e-6
    assert np.abs(bad["score"] - g["score64"]).max() > 1e-2, defect


def test_planted_softmax_defect_on_logits_near_90(sets, restated):
    z = (restated["a"]["logits"] + 90.0).astype(np.float32)                  # softmax is shift invariant; exp(90) overflows float32
    good = SR.from_logits(z, 2, 0)
    assert np.array_equal(good["label"], sets["a"]["label"]) and np.abs(good["score"] - sets["a"]["score64"]).max() < 1e-4
    bad = SR.from_logits(z, 2, 0, defect="softmax_no_max")
    over = z.max(axis=1) > 88.73                                              # float32 exp overflows above 88.72
    assert over.mean() > 0.5
    assert not np.isfinite(bad["score"][over]).any() and (bad["label"][over] == -1).all()


def test_planted_argmax_defect_at_a_tie(restated):
    z = restated["a"]["logits"].copy()
    top = z.max(axis=1)
    z[:, 0], z[:, 2] = top, top                                              # an exact tie of the first and the last class
    good, bad = SR.from_logits(z, 2, 0), SR.from_logits(z, 2, 0, defect="argmax_last")
    assert (good["label"] == 0).all() and (bad["label"] == 2).all()
    assert (good["score"] < 0).all() and (bad["score"] > 0).all()


def test_split_sequence_classifier_layouts():
    from manner_amd.weights import split_sequence_classifier
    t = lambda *s: np.zeros(s, np.float32) + len(s)
    rob = {"roberta.embeddings.word_embeddings.weight": t(5, 4), "roberta.embeddings.position_ids": np.arange(3),
           "roberta.encoder.layer.0.output.dense.bias": t(4), "classifier.dense.weight": t(4, 4), "classifier.dense.bias": t(4),
           "classifier.out_proj.weight": t(3, 4), "classifier.out_proj.bias": t(3)}
    plm, head = split_sequence_classifier(rob)
    assert sorted(plm) == ["embeddings.word_embeddings.weight", "encoder.layer.0.output.dense.bias"]      # no pooler: accepted
    assert head["dense.weight"] is rob["classifier.dense.weight"] and head["out.bias"] is rob["classifier.out_proj.bias"]
    assert head["dense.bias"] is rob["classifier.dense.bias"] and head["out.weight"] is rob["classifier.out_proj.weight"]
    bert = {"bert.embeddings.word_embeddings.weight": t(5, 4), "bert.pooler.dense.weight": t(4, 4), "bert.pooler.dense.bias": t(4),
            "classifier.weight": t(2, 4), "classifier.bias": t(2)}
    plm, head = split_sequence_classifier(bert)
    assert "embeddings.word_embeddings.weight" in plm
    assert head["dense.weight"] is bert["bert.pooler.dense.weight"] and head["dense.bias"] is bert["bert.pooler.dense.bias"]
    assert head["out.weight"] is bert["classifier.weight"] and head["out.bias"] is bert["classifier.bias"]
    distil = {"distilbert.embeddings.word_embeddings.weight": t(5, 4), "pre_classifier.weight": t(4, 4), "pre_classifier.bias": t(4),
              "classifier.weight": t(2, 4), "classifier.bias": t(2)}
    with pytest.raises(ValueError, match="pre_classifier"):
        split_sequence_classifier(distil)
    with pytest.raises(ValueError):
        split_sequence_classifier({"roberta.embeddings.word_embeddings.weight": t(5, 4)})


def test_xlm_roberta_preset():
    from manner_amd.config import ARCH_ROBERTA, PRESETS
    c = PRESETS["xlm-roberta-base"]
    assert (c.arch, c.vocab, c.max_pos, c.type_vocab, c.ln_eps, c.pad_id) == (ARCH_ROBERTA, 250002, 514, 1, 1e-5, 1)
    assert (c.hidden, c.layers, c.heads, c.intermediate) == (768, 12, 12, 3072)


def test_sentiment2index_is_the_reference_expression():
    pd = pytest.importorskip("pandas")
    from manner_amd.data.components.sentiment_annotator import SentimentAnnotator
    rng = np.random.default_rng(5)
    classes = list(rng.permutation(["neutral"] * 7 + ["positive"] * 5 + ["negative"] * 9 + ["mixed"] * 2))
    news = pd.DataFrame({"sentiment_class": classes})
    news_sentiment = news["sentiment_class"].drop_duplicates().reset_index(drop=True)          # mind_dataframe.py:210-211
    expected = {v: k + 1 for k, v in news_sentiment.to_dict().items()}
    assert SentimentAnnotator.sentiment2index(classes) == expected
    assert SentimentAnnotator.sentiment2index([]) == {}


def test_signatures_equal_the_reference(sets):
    """against the reference's own signatures as the golden's generator recorded them"""
    from manner_amd.data.components.sentiment_annotator import SentimentAnnotator as Own

    def positional(fn):
        return [[p.name, None if p.default is p.empty else p.default, p.kind.name] for p in inspect.signature(fn).parameters.values()
                if p.kind != p.KEYWORD_ONLY]

    assert positional(Own.__init__) == sets["signatures"]["__init__"]
    assert positional(Own.forward) == sets["signatures"]["forward"]
    assert [row[:2] for row in sets["signatures"]["__init__"][1:]] == [["sentiment_model", "cardiffnlp/twitter-xlm-roberta-base-sentiment"],
                                                                      ["tokenizer_max_length", 96]]
    extra = [p.name for p in inspect.signature(Own.__init__).parameters.values() if p.kind == p.KEYWORD_ONLY]
    assert extra == ["tokenizer", "config", "state_dict", "device", "precision"]


def test_a_hub_name_alone_is_refused():
    from manner_amd.data.components.sentiment_annotator import SentimentAnnotator
    with pytest.raises(ValueError, match="no hub access"):
        SentimentAnnotator()
    with pytest.raises(ValueError, match="precision"):
        SentimentAnnotator(config={}, state_dict={}, precision="int8")


@pytest.fixture
def fake_reference(monkeypatch):
    """a stand-in for the reference's packages, as far as install() looks: the four operator modules and the three annotator holders"""
    from manner_amd import binding
    made = {}

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__file__ = "/nowhere/" + name.replace(".", "/") + ".py"
        for k, v in attrs.items():
            setattr(m, k, v)
        monkeypatch.setitem(sys.modules, name, m)
        made[name] = m
        return m

    for pkg in ("manner", "manner.models", "manner.models.components", "manner.data", "manner.data.components"):
        module(pkg).__path__ = []
    for leaf, names in binding.TARGETS.items():
        module("manner.models.components." + leaf, **{n: type(n, (), {}) for n in names})
    original = type("SentimentAnnotator", (), {})
    for name in binding.ANNOTATOR_MODULES:
        module(name, SentimentAnnotator=original)
    yield made, original
    binding.uninstall()


def test_install_rebinds_the_annotator_only_on_request(fake_reference):
    import manner_amd
    from manner_amd import binding
    from manner_amd.data.components.sentiment_annotator import SentimentAnnotator as Own
    made, original = fake_reference
    report = manner_amd.install()
    assert not any(m in report for m in binding.ANNOTATOR_MODULES)
    assert all(made[m].SentimentAnnotator is original for m in binding.ANNOTATOR_MODULES)
    plain = {k: sorted(v) for k, v in report.items()}
    assert sorted(plain) == sorted("manner.models.components." + leaf for leaf in binding.TARGETS)
    report = manner_amd.install(annotator=True)
    assert {m: report[m] for m in binding.ANNOTATOR_MODULES} == {m: ["SentimentAnnotator"] for m in binding.ANNOTATOR_MODULES}
    assert all(made[m].SentimentAnnotator is Own for m in binding.ANNOTATOR_MODULES)
    manner_amd.uninstall()
    assert all(made[m].SentimentAnnotator is original for m in binding.ANNOTATOR_MODULES)


# ---------------------------------------------------------------- the entry's argument checks: before any launch, no device needed
_OK = dict(ldx=128, N=4, H=128, L=3, pos=2, neg=0)


def _call(null=(), **over):
    from manner_amd import _lib
    lib = _lib.load()
    a = dict(_OK, **over)
    buf = (C.c_float * 16)()                                                # never dereferenced: every case below fails a check first
    p = {k: C.c_void_p(0 if k in null else C.addressof(buf)) for k in ("x", "wd", "bd", "wo", "bo", "probs", "label", "score")}
    rc = lib.manner_hip_seqcls_head(p["x"], a["ldx"], p["wd"], p["bd"], p["wo"], p["bo"], a["N"], a["H"], a["L"], a["pos"], a["neg"], p["probs"],
                                    p["label"], p["score"], C.c_void_p(0))
    return rc, lib.manner_hip_last_error().decode()


@pytest.mark.parametrize("over,word", [(dict(L=0, pos=-1, neg=-1), "L=0"), (dict(L=65), "L=65"), (dict(H=1028, ldx=1028), "H=1028"),
                                       (dict(H=130, ldx=130), "H=130"), (dict(ldx=127), "ldx=127"), (dict(N=-1), "N=-1"),
                                       (dict(N=2 ** 31), "N=2147483648"), (dict(pos=3), "pos_idx=3"), (dict(neg=-2), "neg_idx=-2")])
def test_entry_refuses_bad_shapes(over, word):
    rc, msg = _call(**over)
    assert rc == 1 and "seqcls_head" in msg and word in msg, (rc, msg)


@pytest.mark.parametrize("null", ["x", "wd", "bd", "wo", "bo", "label", "score"])
def test_entry_refuses_null_pointers(null):
    rc, msg = _call(null=(null,))
    assert rc == 1 and "seqcls_head" in msg and "null" in msg, (rc, msg)


def test_entry_with_no_rows_launches_nothing():
    rc, _ = _call(N=0, null=("x", "probs"))
    assert rc == 0


def test_export_is_declared_and_bound_under_abi_8():
    from manner_amd import _lib
    assert "manner_hip_seqcls_head" in _lib.header_symbols() and "manner_hip_seqcls_head" in _lib.SIGNATURES
    assert _lib.load().manner_hip_abi_version() == 8 == _lib.ABI_VERSION
