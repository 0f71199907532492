"""News of 129..512 tokens through the inference engine (encode_cls / encode_hidden and the module mirror in eval()): the long-row
attention kernels against the reference's goldens and the oracle, and rows of <= 128 tokens bit-identical to what they give in a
short batch.  Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import manner_oracle as O  # noqa: E402  (tests/conftest.py puts oracle/ on sys.path)
from manner_amd import hip  # noqa: E402
from manner_amd.config import PRESETS, EncoderConfig  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from manner_amd.weights import make_plm_weights  # noqa: E402

DEV = "cuda:0"
FP32_TOL = 1e-4
MODES = ("fp32", "f16x3", "bf16x3", "f16", "bf16")
GOLDEN_LONG = ["enc_long_bert_base", "enc_long_roberta"]


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return z, json.loads(str(z["meta"]))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_ENC = {}


def _encoder(preset, seed, std):
    key = (preset, seed, std)
    if key not in _ENC:
        for k in list(_ENC):                             # one bert-base-sized handle at a time
            _ENC.pop(k)[0].close()
        cfg = PRESETS[preset]
        _ENC[key] = (hip.HipEncoder(cfg, make_plm_weights(cfg, seed=seed, std=std), precisions=MODES, device=DEV), cfg)
    return _ENC[key]


def _cos(a, b):
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


@pytest.mark.parametrize("prec", ["fp32", "f16x3", "bf16x3"])
@pytest.mark.parametrize("name", GOLDEN_LONG)
def test_long_rows_parity_modes_meet_the_fp32_bar(golden_dir, name, prec, measured):
    z, meta = _load(golden_dir, name)
    enc, _ = _encoder(meta["preset"], meta["seed"], meta["std"])
    ids, mask = _cuda(z["ids"]), _cuda(z["mask"])
    out = enc.encode_cls(ids, mask, precision=prec, host_lengths=z["mask"].sum(1)).cpu().numpy()
    enc.status()
    err = np.abs(out - z["out"]).max()
    long_err = np.abs(out - z["out"])[z["mask"].sum(1) > 128].max()
    measured(bound=FP32_TOL, max_abs_err=err, long_rows_max_abs_err=long_err)
    print(f"{name} {prec}: max-abs err vs reference {err:.3e} (rows > 128 tokens: {long_err:.3e})")
    assert err < FP32_TOL
    out2 = enc.encode_cls(ids, mask, precision=prec).cpu().numpy()        # device-side lengths: the same bits
    assert np.array_equal(out, out2)


@pytest.mark.parametrize("prec,tol,cos_min", [("f16", 2e-2, 0.99999), ("bf16", 0.1, 0.999)])
@pytest.mark.parametrize("name", GOLDEN_LONG)
def test_long_rows_16bit_modes_close_to_reference(golden_dir, name, prec, tol, cos_min, measured):
    z, meta = _load(golden_dir, name)
    enc, _ = _encoder(meta["preset"], meta["seed"], meta["std"])
    out = enc.encode_cls(_cuda(z["ids"]), _cuda(z["mask"]), precision=prec).cpu().numpy()
    enc.status()
    ref = z["out"]
    err = np.abs(out - ref).max()
    cos = _cos(out, ref).min()
    measured(bound=tol, max_abs_err=err, cosine_bound=cos_min, min_cosine=cos)
    print(f"{name} {prec}: max-abs err {err:.3e}, min cosine {cos:.7f}")
    assert err < tol and cos > cos_min


def _short_and_long(cfg, seed):
    g = np.random.default_rng(seed)
    short_len = g.integers(2, 97, 40)
    short_len[:3] = [2, 96, 33]
    s_ids, s_mask = synth_news_tokens(40, cfg, seed=seed, lengths=short_len)
    l_ids, l_mask = synth_news_tokens(6, cfg, seed=seed + 1, lengths=np.array([129, 512, 300, 161, 2, 128]), pad_to=512)
    # the short news interleaved with the long ones, in a batch padded to 512
    order = np.concatenate([np.arange(0, 40, 2), [40, 41], np.arange(1, 40, 2), [42, 43, 44, 45]])
    pad = lambda a, v: np.pad(a, ((0, 0), (0, 512 - a.shape[1])), constant_values=v)   # noqa: E731
    b_ids = np.concatenate([pad(s_ids, cfg.pad_id), l_ids])[order]
    b_mask = np.concatenate([pad(s_mask, 0), l_mask])[order]
    where = np.argsort(order)[:40]                       # batch row of short news i
    return s_ids, s_mask, b_ids, b_mask, where


@pytest.mark.parametrize("prec", MODES)
def test_short_rows_give_the_same_bits_next_to_long_rows(golden_dir, prec):
    """The invariant that makes long rows a pure addition: a row of <= 128 tokens runs the same kernels whatever the padded length and
    its neighbours — encode_cls and encode_hidden, with and without host lengths.  f16x3 is compared with the short batch padded to 128:
    its short-row attention kernel is instantiated per padded length (at most 1..4 key tiles), and the four-tile instance gives rows of
    <= 96 tokens bits that differ from the three-tile one in the last place (so it was before long rows existed); a call that may carry
    long rows runs the four-tile instance, i.e. gives every short row the bits of a 128-padded call."""
    _, meta = _load(golden_dir, "enc_long_bert_base")
    enc, cfg = _encoder(meta["preset"], meta["seed"], meta["std"])
    s_ids, s_mask, b_ids, b_mask, where = _short_and_long(cfg, 70)
    assert s_ids.shape[1] <= 96
    if prec == "f16x3":
        s_ids = np.pad(s_ids, ((0, 0), (0, 128 - s_ids.shape[1])), constant_values=cfg.pad_id)
        s_mask = np.pad(s_mask, ((0, 0), (0, 128 - s_mask.shape[1])))
    lp = s_ids.shape[1]
    for hl in (False, True):
        alone = enc.encode_cls(_cuda(s_ids), _cuda(s_mask), precision=prec, host_lengths=s_mask.sum(1) if hl else None)
        mixed = enc.encode_cls(_cuda(b_ids), _cuda(b_mask), precision=prec, host_lengths=b_mask.sum(1) if hl else None)
        enc.status()
        assert torch.equal(alone, mixed[torch.from_numpy(where).to(DEV)]), (prec, hl)
    for hl in (False, True):
        alone = enc.encode_hidden(_cuda(s_ids), _cuda(s_mask), 6, precision=prec, host_lengths=s_mask.sum(1) if hl else None)
        mixed = enc.encode_hidden(_cuda(b_ids), _cuda(b_mask), 6, precision=prec, host_lengths=b_mask.sum(1) if hl else None)
        enc.status()
        rows = mixed[torch.from_numpy(where).to(DEV)]
        assert torch.equal(alone, rows[:, :lp]), (prec, hl)
        assert float(rows[:, lp:].abs().max()) == 0.0


# ---- long-kernel stress against the oracle (fp32 mode): a small two-layer model whose layer 0 runs the long flash kernel and whose
# last layer the long [CLS] branch
STRESS_CFG = EncoderConfig(hidden=256, layers=2, heads=4, intermediate=1024, vocab=2048, max_pos=512)


def _stress_weights(kind, seed=80):
    cfg = STRESS_CFG
    w = make_plm_weights(cfg, seed=seed, std=0.05)
    H = cfg.hidden
    w["embeddings.position_embeddings.weight"][:] = 0.0
    w["embeddings.token_type_embeddings.weight"][:] = 0.0
    g = np.random.default_rng(seed)
    for layer in range(cfg.layers):
        p = f"encoder.layer.{layer}.attention.self."
        if kind == "equal":                              # q = 0: every score 0, the softmax uniform over the row
            w[p + "query.weight"][:] = 0.0
            w[p + "query.bias"][:] = 0.0
        elif kind == "peaked":
            # rank-one scores: per head, q = a (u.x + b) u and k = a u u^T x, so every query ranks the keys by u.x — largest at the
            # marker token, whose (normalised) embedding is u — and the softmax is close to one-hot there
            u = g.standard_normal(H).astype(np.float32)
            u -= u.mean()
            u /= np.linalg.norm(u)
            a = 6.0
            wq = np.zeros((H, H), np.float32)
            wk = np.zeros((H, H), np.float32)
            for h in range(cfg.heads):
                wq[64 * h] = a * u
                wk[64 * h] = a * u
            w[p + "query.weight"][:] = wq
            w[p + "key.weight"][:] = wk
            w[p + "query.bias"][:] = 0.0
            w[p + "query.bias"][0::64] = a * 4.0
            w[p + "key.bias"][:] = 0.0
            if layer == 0:
                w["embeddings.word_embeddings.weight"][7] = u * 40.0
    return cfg, w


def _stress_case(cfg, lengths, seed, marker=None):
    ids, mask = synth_news_tokens(len(lengths), cfg, seed=seed, lengths=np.asarray(lengths))
    if marker is not None:
        for n, ln in enumerate(lengths):
            ids[n, marker(ln)] = 7
    return ids, mask


def _check_against_oracle(enc, cfg, w, ids, mask, measured, tag, **kw):
    out = enc.encode_cls(_cuda(ids), _cuda(mask), precision="fp32", **kw).cpu().numpy()
    h1 = enc.encode_hidden(_cuda(ids), _cuda(mask), 1, precision="fp32", **kw).cpu()
    enc.status()
    ref = O.encode_cls(ids, mask, w, cfg).numpy()
    cfg1 = dataclasses.replace(cfg, layers=1)
    ref1 = O.encode_tokens(ids, mask, {k: v for k, v in w.items() if "layer.1." not in k}, cfg1)
    keep = torch.from_numpy(mask).bool()
    err = np.abs(out - ref).max()
    err1 = float((h1[keep] - ref1[keep]).abs().max())
    measured(**{f"{tag}_cls_err": err, f"{tag}_layer0_err": err1})
    print(f"{tag}: CLS err {err:.3e}, hidden_states[1] err {err1:.3e}")
    assert err < FP32_TOL and err1 < FP32_TOL, (tag, err, err1)
    return out


@pytest.mark.parametrize("kind", ["random", "peaked_last", "peaked_first", "equal"])
def test_long_kernels_match_the_oracle_under_stress(kind, measured):
    cfg, w = _stress_weights("peaked" if kind.startswith("peaked") else kind)
    enc = hip.HipEncoder(cfg, w, precisions=("fp32",), device=DEV)
    try:
        lengths = [129, 160, 161, 512, 2, 128]
        marker = {"peaked_last": lambda ln: ln - 1, "peaked_first": lambda ln: 1}.get(kind)
        ids, mask = _stress_case(cfg, lengths, seed=81, marker=marker)
        _check_against_oracle(enc, cfg, w, ids, mask, measured, kind, host_lengths=mask.sum(1))
    finally:
        enc.close()


def test_many_short_long_rows_across_chunk_boundaries(measured):
    """Many 129-token rows between 2-token rows, with a workspace of 256-token chunks: every chunk boundary falls somewhere else in the
    pattern; the result is the single-chunk result bit for bit and the oracle's."""
    cfg, w = _stress_weights("random")
    enc = hip.HipEncoder(cfg, w, precisions=("fp32",), device=DEV)
    try:
        lengths = np.array([129, 2, 2, 129, 129, 2] * 8)
        ids, mask = _stress_case(cfg, lengths, seed=82)
        whole = _check_against_oracle(enc, cfg, w, ids, mask, measured, "mix", host_lengths=mask.sum(1))
        small = enc.encode_cls(_cuda(ids), _cuda(mask), precision="fp32", host_lengths=mask.sum(1), max_chunk_tokens=256).cpu().numpy()
        enc.status()
        assert np.array_equal(whole, small)
    finally:
        enc.close()


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_encode_hidden_of_long_rows_matches_reference(golden_dir, prec, measured):
    z, meta = _load(golden_dir, "hidden_long_bert_base")
    enc, _ = _encoder(meta["preset"], meta["seed"], meta["std"])
    keep = torch.from_numpy(z["mask"]).bool()
    rows = torch.from_numpy(z["rows"])
    for k in meta["layers"]:
        h = enc.encode_hidden(_cuda(z["ids"]), _cuda(z["mask"]), k, precision=prec).cpu()
        enc.status()
        assert float(h[~keep].abs().max()) == 0.0
        err = np.abs(h[keep][rows].numpy() - z[f"h{k}"]).max()
        measured(**{f"h{k}_err": err, "bound": FP32_TOL})
        print(f"hidden_states[{k}] {prec}: max-abs err {err:.3e}")
        assert err < FP32_TOL, (k, err)


def _mirror(golden_dir, name="enc_long_bert_base", frozen=(0,)):
    from manner_amd.models.components.news_encoder import MannerNewsEncoder
    z, meta = _load(golden_dir, name)
    cfg = PRESETS[meta["preset"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = MannerNewsEncoder(plm_model=meta["preset"], frozen_layers=list(frozen), dropout_probability=0.2, use_entities=False,
                                entity_embeddings=None, entity_embedding_dim=100, num_attention_heads=10, query_vector_dim=200,
                                text_embedding_dim=cfg.hidden)
    w = make_plm_weights(cfg, seed=meta["seed"], std=meta["std"])
    enc.load_state_dict({"text_encoder.plm_model." + k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    # the rows of the golden that fit 300 tokens, padded to 300 (the reference's output does not depend on the padding)
    sel = z["mask"].sum(1) <= 300
    news = {"text": {"input_ids": _cuda(z["ids"][sel, :300]), "attention_mask": _cuda(z["mask"][sel, :300])}}
    return enc.to(DEV), news, z["out"][sel]


@pytest.mark.parametrize("autocast,tol,cos_min", [(None, FP32_TOL, None), (torch.float16, 2e-2, 0.99999), (torch.bfloat16, 0.1, 0.999)])
def test_module_mirror_eval_on_a_300_token_batch(golden_dir, autocast, tol, cos_min, measured):
    enc, news, ref = _mirror(golden_dir)
    enc.eval()
    assert news["text"]["input_ids"].shape[1] == 300 and int(news["text"]["attention_mask"].sum(1).max()) > 128
    with torch.no_grad():
        if autocast is None:
            out = enc(news)
        else:
            with torch.autocast("cuda", dtype=autocast):
                out = enc(news)
    out = out.float().cpu().numpy()
    err = np.abs(out - ref).max()
    cos = _cos(out, ref).min()
    measured(bound=tol, max_abs_err=err, min_cosine=cos)
    print(f"mirror eval autocast={autocast}: max-abs err {err:.3e}, min cosine {cos:.7f}")
    assert err < tol and (cos_min is None or cos > cos_min)


def test_module_mirror_cache_returns_the_bits_of_a_fresh_encode(golden_dir):
    enc, news, _ = _mirror(golden_dir)
    enc.eval()
    enc.text_encoder.precision = "f16"
    with torch.no_grad():
        fresh = enc(news).clone()
        enc.text_encoder.embedding_cache_rows = 64
        miss = enc(news).clone()                         # rows encoded and stored
        hit = enc(news).clone()                          # every row from the table
    assert torch.equal(fresh, miss) and torch.equal(fresh, hit)


def test_module_mirror_training_keeps_the_128_token_limit(golden_dir):
    enc, news, _ = _mirror(golden_dir)
    enc.train()
    enc.text_encoder.train_precision = "fp32"
    with pytest.raises(RuntimeError, match="padded_len"):
        enc(news)


def test_padded_len_beyond_512_is_invalid():
    enc, cfg = _encoder("bert-base-uncased", 60, 0.02)
    ids, mask = synth_news_tokens(2, cfg, seed=3, lengths=np.array([5, 40]), pad_to=513)
    with pytest.raises(RuntimeError, match="512"):
        enc.encode_cls(_cuda(ids), _cuda(mask), precision="fp32")
    enc.status()


def test_bad_mask_in_a_long_row_raises():
    enc, cfg = _encoder("bert-base-uncased", 60, 0.02)
    ids, mask = synth_news_tokens(3, cfg, seed=4, lengths=np.array([5, 300, 200]), pad_to=320)
    mask[1, 250] = 0                                     # a hole: not a prefix mask
    enc.encode_cls(_cuda(ids), _cuda(mask), precision="bf16")
    with pytest.raises(RuntimeError, match="prefix mask"):
        enc.status()
    enc.status()


def test_rows_beyond_the_position_table_raise():
    # tiny-roberta: 130 positions from pad_id + 1 = 2, i.e. 128 tokens; a 129-token row now passes the padded-length check and
    # raises the reference's IndexError instead
    cfg = PRESETS["tiny-roberta"]
    enc = hip.HipEncoder(cfg, make_plm_weights(cfg, seed=5, std=0.05), precisions=("fp32", "bf16"), device=DEV)
    try:
        ids, mask = synth_news_tokens(2, cfg, seed=5, lengths=np.array([7, 129]))
        enc.encode_cls(_cuda(ids), _cuda(mask), precision="fp32")
        with pytest.raises(RuntimeError, match="position"):
            enc.status()
        enc.status()
    finally:
        enc.close()
    # roberta-base: 514 positions = 512 tokens, the inference limit; a 513-token row is refused by its padded length
    enc, cfg = _encoder("roberta-base", 61, 0.02)
    ids, mask = synth_news_tokens(1, cfg, seed=6, lengths=np.array([513]))
    with pytest.raises(RuntimeError, match="512"):
        enc.encode_cls(_cuda(ids), _cuda(mask), precision="fp32")
