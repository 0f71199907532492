"""The 16-bit attention (attention.hip's attn_long16_kernel and short MFMA kernel, the pruned last layer; train_attn.hip's
attn_train_mfma_*_kernel and *_long_kernel passes, and the VALU form) held to a float64 reference (tests/slice_ref.py) per slice:
per (news, 32-token block, head) cell, per head of the layer-0 Q / K / V gradients, per 32-position block of the position table,
per (news, 32-token block) of the word-embedding rows and per news for [CLS].  Each map has two bars, on its maximum and on its
outlier ratio (maximum / median): a defect confined to one head, tile or row block moves the ratio long before it moves a
whole-tensor maximum.  Bars: the measured values of profiles/attention_slices/measured_tolerances.json with headroom (BARS).

Two-layer configs at bert-base width (768, 12 heads, 512 positions) and roberta-large width (1024, 16 heads, RoBERTa, 514
positions), a vocabulary of 8192 with one id per (news, position) outside [CLS] / [SEP] / padding (each word-embedding gradient
row is one token's input gradient), HF-init weights and a structured set whose attention out-projection is the identity (head h
stays in features 64h .. 64h+63 up to the LayerNorm).  Two batches, padded to 512 and to 385, cover the 32-row tile, 128-key
block and 256-query block edges.  Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import slice_ref as S  # noqa: E402
from manner_amd import _lib, hip, train  # noqa: E402
from manner_amd.config import ARCH_BERT, PRESETS  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from manner_amd.weights import make_plm_weights  # noqa: E402
from test_gpu_long_train import _replay_keep  # noqa: E402

DEV = "cuda:0"
VOCAB = 8192
WIDTHS = {"bert-base": dataclasses.replace(PRESETS["bert-base-uncased"], layers=2, vocab=VOCAB),
          "roberta-large": dataclasses.replace(PRESETS["roberta-large"], layers=2, vocab=VOCAB)}
BATCHES = {512: [31, 33, 128, 159, 161, 192, 255, 257, 384, 447, 511, 512],
           385: [2, 32, 127, 129, 160, 191, 193, 256, 383, 385]}
# storage points the reference rounds at (slice_ref.STORE_POINTS): all four make the inference maps tightest; in training the
# backward's own 16-bit points are not restated, so the forward's points alone are rounded there too
STORE = S.STORE_POINTS
DROP = dict(p_hidden=0.1, p_attn=0.1, p_out=0.1)
SEED = 20261016
# (map maximum, outlier ratio) per quantity and mode: the largest value measured on an MI355X over every case and subject of the
# quantity (profiles/attention_slices/measured_tolerances.json), the maximum x ~1.5 and the ratio x ~1.25, rounded up.  The Q / K
# gradients run through dS = P (dP - D), a difference of nearly equal terms at HF-init weights: their rounding noise differs from
# head to head by up to 4.3x in both the MFMA and the VALU kernels alike (the same heads), hence the wider ratio bar there.
BARS = {
    ("hidden", "f16"): (1e-3, 1.6), ("hidden", "bf16"): (8e-3, 1.6),           # measured 5.9e-4 / 4.8e-3, ratios <= 1.29
    ("cls", "f16"): (1e-3, 1.6), ("cls", "bf16"): (8.5e-3, 1.6),              # 6.8e-4 / 5.6e-3, <= 1.21
    ("train_cls", "f16"): (7.5e-4, 1.8), ("train_cls", "bf16"): (6e-3, 1.8),  # 4.9e-4 / 3.9e-3, <= 1.44
    ("qk_grad", "f16"): (5e-3, 5.5), ("qk_grad", "bf16"): (4.5e-2, 5.5),      # 3.1e-3 / 2.9e-2, <= 4.33
    ("v_grad", "f16"): (1e-3, 1.9), ("v_grad", "bf16"): (7.5e-3, 1.9),        # 6.2e-4 / 4.9e-3, <= 1.49
    ("pos_grad", "f16"): (1.2e-3, 1.5), ("pos_grad", "bf16"): (8.5e-3, 1.5),  # 7.4e-4 / 5.5e-3, <= 1.20
    ("word_grad", "f16"): (1e-3, 1.4), ("word_grad", "bf16"): (8e-3, 1.4),    # 6.6e-4 / 5.3e-3, <= 1.10
}
PARITY_BARS = {"fp32": (1e-5, 1.6), "f16x3": (1e-5, 1.6)}      # measured <= 1.3e-6, ratios <= 1.21 (and FP32_TOL on the largest error)
QKV = [f"encoder.layer.0.attention.self.{m}.{p}" for m in ("query", "key", "value") for p in ("weight", "bias")]
WORD, POS = "embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_CASES = {}


def _case(width, weights, pad):
    """cfg, float32 weights, ids, mask: one id of its own per (news, position) between [CLS] and [SEP]."""
    key = (width, weights, pad)
    if key not in _CASES:
        cfg = WIDTHS[width]
        w = make_plm_weights(cfg, seed=SEED % 1000, std=0.02, with_pooler=False)
        if weights == "ident":
            for l in range(cfg.layers):
                w[f"encoder.layer.{l}.attention.output.dense.weight"] = np.eye(cfg.hidden, dtype=np.float32)
                w[f"encoder.layer.{l}.attention.output.dense.bias"] = np.zeros(cfg.hidden, dtype=np.float32)
        lens = np.array(BATCHES[pad])
        ids, mask = synth_news_tokens(len(lens), cfg, seed=pad, lengths=lens, pad_to=pad)
        inner = (mask != 0) & (np.arange(pad)[None, :] > 0) & (np.arange(pad)[None, :] < lens[:, None] - 1)
        ids[inner] = 200 + np.random.default_rng(pad).permutation(VOCAB - 200)[:int(inner.sum())]
        _CASES[key] = cfg, w, ids, mask
    return _CASES[key]


_REFS = {}


def _ref(width, weights, pad, mode, train_mode=False):
    """The float64 reference, cached per (config, weights, lengths, mode rounding, inference / train); computed on the GPU in
    float64 (torch), kept on the host."""
    key = (width, weights, pad, mode, train_mode)
    if key not in _REFS:
        cfg, w, ids, mask = _case(width, weights, pad)
        store = STORE if mode in S.DT16 else ()
        m16 = mode if mode in S.DT16 else None
        if not train_mode:
            r = S.reference(cfg, w, ids, mask, mode=m16, store=store, device=DEV)
            _REFS[key] = {"hidden1": r["hidden"][1].cpu().numpy(), "cls": r["cls"].cpu().numpy()}
        else:
            keep = _replay_keep(SEED, DROP["p_hidden"], DROP["p_out"], cfg, mask)
            keep.p_attn = DROP["p_attn"]
            r = S.reference(cfg, w, ids, mask, mode=m16, store=store, train=True, R=_R(cfg, len(mask)), keep=keep, device=DEV,
                            grad_keys=QKV + [WORD, POS], **DROP)
            _REFS[key] = {"cls": r["cls"].cpu().numpy(), "grads": {k: g.cpu().numpy() for k, g in r["grads"].items()}}
        torch.cuda.empty_cache()
    return _REFS[key]


def _R(cfg, n):
    return torch.from_numpy(np.random.default_rng(SEED).standard_normal((n, cfg.hidden)))


_ENC = {}


def _engine(width, weights):
    key = (width, weights)
    if key not in _ENC:
        for k in list(_ENC):                             # one handle at a time
            _ENC.pop(k).close()
        cfg, w, _, _ = _case(width, weights, 512)
        _ENC[key] = hip.HipEncoder(cfg, w, precisions=("f16", "bf16", "fp32", "f16x3"), device=DEV)
    return _ENC[key]


def _check(tag, m, bars, record, failures):
    """Record the map next to its bars, then compare (every map of a case is measured before the first bar fails)."""
    record(**{f"{tag}_max": m["max"], f"{tag}_ratio": m["ratio"], f"{tag}_worst_label": m["worst"], f"{tag}_bar_max": bars[0],
              f"{tag}_bar_ratio": bars[1]})
    if not (m["max"] < bars[0] and m["ratio"] < bars[1]):
        failures.append(f"{tag}: {m!r} vs bars {bars}")


# ------------------------------------------------------------------------------------------------ inference
@pytest.mark.parametrize("pad", [512, 385])
@pytest.mark.parametrize("weights", ["hf", "ident"])
@pytest.mark.parametrize("width", list(WIDTHS))
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_inference_16bit_per_slice(mode, width, weights, pad, measured):
    """encode_hidden(n_layers=1) per (news, 32-token block, head) and encode_cls over both layers (the pruned last layer) per news,
    with host lengths and with device lengths."""
    cfg, w, ids, mask = _case(width, weights, pad)
    ref = _ref(width, weights, pad, mode)
    enc = _engine(width, weights)
    lab = S.token_block_head_labels(mask, cfg.hidden, cfg.heads)
    failures = []
    for how, hl in (("host", mask.sum(1)), ("device", None)):
        h1 = enc.encode_hidden(_cuda(ids), _cuda(mask), 1, precision=mode, host_lengths=hl)
        cls = enc.encode_cls(_cuda(ids), _cuda(mask), precision=mode, host_lengths=hl)
        hip.check_status(DEV)
        _check(f"{how}_hidden", S.error_map(h1.cpu().numpy(), ref["hidden1"], lab), BARS[("hidden", mode)], measured, failures)
        _check(f"{how}_cls", S.error_map(cls.cpu().numpy(), ref["cls"], S.news_labels(len(mask), cfg.hidden)), BARS[("cls", mode)],
               measured, failures)
    assert not failures, failures


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_inference_parity_modes_keep_the_maps_quiet(mode, measured):
    """The exact-f32 long kernel through the same maps against the unrounded reference: a correct kernel gives a quiet map."""
    cfg, w, ids, mask = _case("roberta-large", "hf", 385)
    ref = _ref("roberta-large", "hf", 385, None)
    enc = _engine("roberta-large", "hf")
    h1 = enc.encode_hidden(_cuda(ids), _cuda(mask), 1, precision=mode, host_lengths=mask.sum(1)).cpu().numpy()
    cls = enc.encode_cls(_cuda(ids), _cuda(mask), precision=mode).cpu().numpy()
    hip.check_status(DEV)
    failures = []
    _check("hidden", S.error_map(h1, ref["hidden1"], S.token_block_head_labels(mask, cfg.hidden, cfg.heads)), PARITY_BARS[mode],
           measured, failures)
    _check("cls", S.error_map(cls, ref["cls"], S.news_labels(len(mask), cfg.hidden)), PARITY_BARS[mode], measured, failures)
    err = max(float(np.abs(h1 - ref["hidden1"])[mask != 0].max()), float(np.abs(cls - ref["cls"]).max()))
    measured(max_abs_err=err)
    assert err < 1e-4 and not failures, (err, failures)


# ------------------------------------------------------------------------------------------------ training
def _grad_labels(cfg, ids, mask):
    """Word-embedding rows per (news, 32-token block) of the token that owns the row, -1 for [CLS] / [SEP] / pad and unused rows;
    position rows per 32-position block of the rows in use."""
    n, lp = mask.shape
    nb = (lp + 31) // 32
    word = np.full(cfg.vocab, -1, dtype=np.int64)
    lens = mask.sum(1)
    for i in range(n):
        for t in range(1, lens[i] - 1):
            word[ids[i, t]] = i * nb + t // 32
    first = 0 if cfg.arch == ARCH_BERT else cfg.pad_id + 1
    pos = np.full(cfg.max_pos, -1, dtype=np.int64)
    pos[first:first + int(lens.max())] = np.arange(int(lens.max())) // 32
    return word[:, None], pos[:, None]


@pytest.mark.parametrize("pad", [512, 385])
@pytest.mark.parametrize("weights", ["hf", "ident"])
@pytest.mark.parametrize("width", list(WIDTHS))
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_train_16bit_per_slice(mode, width, weights, pad, monkeypatch, measured):
    """encode_train(max_len=512), nothing frozen (layer 0 runs the full attention backward), dropout on at all five sites with the
    masks replayed into the reference; both saved layouts (MANNER_HIP_TRAIN_SAVE16) and the VALU form (MANNER_HIP_TRAIN_ATTN_VALU)
    as subjects of the same maps: layer-0 Q / K / V weight and bias gradients per head, position-embedding gradient per 32-position
    block, word-embedding rows per (news, 32-token block), [CLS] per news."""
    cfg, w, ids, mask = _case(width, weights, pad)
    ref = _ref(width, weights, pad, mode, train_mode=True)
    word_lab, pos_lab = _grad_labels(cfg, ids, mask)
    R = _R(cfg, len(mask)).float().to(DEV)
    monkeypatch.setenv("MANNER_HIP_GEMM_SMALL_TILES", "0")                  # the lean layout's fused-GeLU GEMMs at this batch size
    failures = []
    for save16, valu in (("1", "0"), ("0", "0"), ("0", "1")):          # the VALU form has one layout (the lean one needs MFMA)
        monkeypatch.setenv("MANNER_HIP_TRAIN_SAVE16", save16)
        monkeypatch.setenv("MANNER_HIP_TRAIN_ATTN_VALU", valu)
        params = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in w.items()}
        out = train.encode_train(cfg, params, _cuda(ids), _cuda(mask), precision=mode, seed=SEED, max_len=_lib.MAX_LEN_TRAIN, **DROP)
        (out * R).sum().backward()
        hip.check_status(DEV)
        assert _lib.load().manner_hip_train_layout_last() == (3 if save16 == "1" else 1 if valu == "0" else 0)   # the subject really ran
        tag = "valu" if valu == "1" else f"mfma_save16_{save16}"
        g = {k: params[k].grad.cpu().numpy() for k in QKV + [WORD, POS]}
        _check(f"{tag}_cls", S.error_map(out.detach().cpu().numpy(), ref["cls"], S.news_labels(len(mask), cfg.hidden)),
               BARS[("train_cls", mode)], measured, failures)
        for k in QKV:
            if k.endswith("key.bias"):           # zero in exact arithmetic: no scale to hold it to (test_gpu_long_train bounds it)
                continue
            _check(f"{tag}_{k.split('.')[-2]}_{k.split('.')[-1]}", S.error_map(g[k], ref["grads"][k], S.head_row_labels(g[k].shape, cfg.heads),
                                                                                min_count=cfg.head_dim, per_slice=True),
                   BARS[("v_grad" if ".value." in k else "qk_grad", mode)], measured, failures)
        _check(f"{tag}_pos", S.error_map(g[POS], ref["grads"][POS], pos_lab, per_slice=True), BARS[("pos_grad", mode)], measured, failures)
        _check(f"{tag}_word", S.error_map(g[WORD], ref["grads"][WORD], word_lab, per_slice=True), BARS[("word_grad", mode)], measured, failures)
    assert not failures, failures
