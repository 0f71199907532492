"""The persistent 16-bit GEMMs (gemm.hip's gemm_tn_w8_kernel / gemm_tn_x16_kernel with 256- and 192-row panels, the in-launch
LayerNorm fan-in, the deferred and the classic LayerNorm algebra) and the weight-gradient kernels (wgrad.hip's wgrad_tr_kernel and the
transposing path, the bias / LayerNorm reductions) held to the float64 reference of tests/slice_ref.py per tile: hidden states per
64 x 64 block of packed token rows (packed_tile_labels), every encoder weight gradient per 128 x 64 wave tile (weight_tile_labels),
every bias and LayerNorm gradient per 64 elements (vector_block_labels), [CLS] per news.  The kernel-vs-kernel equality tests tie
these kernels to each other; a defect in a part they share (tile_walk, the epilogues, reduce_partials, the zero-page rule) passes
all of them and the whole-tensor cosine bars — test_gemm_tiles_host.py plants such defects and shows these maps flag them.

A. inference at the cases of test_gpu_attention_slices with MANNER_HIP_GEMM_SMALL_TILES=0, so every launch runs a persistent kernel;
B. inference on 22 450 tokens in one chunk: more 256 x 256 tiles than CUs in every launch by the default rule, so workgroups walk on
   to a second tile (the cross-tile operand pipeline of the w8 kernel);
C. training, dropout on, every parameter gradient of both layers.

Bars: TILE_BARS, by the rule above BARS of test_gpu_attention_slices, from profiles/gemm_tiles/measured_tolerances.json; no ratio bar
above FLAG / 2 of the host test, no maximum above the whole-tensor bars of the 16-bit modes.  Run on the MI355X box: ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import slice_ref as S  # noqa: E402
from manner_amd import _lib, hip, train  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from test_gemm_tiles_host import FLAG  # noqa: E402
from test_gpu_attention_slices import (BARS, DEV, DROP, PARITY_BARS, SEED, STORE, _ENC, _R, _case, _check, _cuda, _engine,  # noqa: E402
                                       _replay_keep)

ABS_CAP = {"f16": 2e-2, "bf16": 0.1, "f16x3": 1e-4}       # the whole-tensor bars these modes already have
# (map maximum, outlier ratio) per quantity and mode: the largest value measured on an MI355X over every case and subject of the
# quantity (profiles/gemm_tiles/measured_tolerances.json, the figures behind each line: f16 / bf16 / f16x3), the maximum x 1.5 and the
# ratio x 1.25, rounded up.  hidden1 / hidden2: encode_hidden(1) / (2) of part A; big_*: part B; the rest: part C, per tensor kind over
# both layers.  The Q / K weight tiles keep the ratio bar the head-to-head rounding noise of those gradients already has (see BARS;
# measured here <= 2.09 per tile); no other tensor does — the Q bias, whose 64-element blocks are heads, has its measured bar.
QK_RATIO = BARS[("qk_grad", "f16")][1]
TILE_BARS = {
    ("hidden1_tiles", "f16"): (8.2e-4, 1.45), ("hidden1_tiles", "bf16"): (6.5e-3, 1.55),   # 5.41e-4 1.15 / 4.30e-3 1.20
    ("hidden2_tiles", "f16"): (1.2e-3, 1.7), ("hidden2_tiles", "bf16"): (8.1e-3, 1.55),   # 7.42e-4 1.33 / 5.36e-3 1.20
    ("hidden2_heads", "f16"): (1.1e-3, 1.65), ("hidden2_heads", "bf16"): (8.9e-3, 1.55),   # 7.13e-4 1.28 / 5.87e-3 1.23
    ("big_hidden1_tiles", "f16"): (7.5e-4, 1.4), ("big_hidden1_tiles", "bf16"): (5.9e-3, 1.4),   # 4.94e-4 1.11 / 3.93e-3 1.10
    ("big_hidden1_tiles", "f16x3"): (1.0e-6, 1.45), ("big_cls", "f16x3"): (1.4e-6, 1.4),       # 6.66e-7 1.14, 9.31e-7 1.11
    ("big_cls", "f16"): (9.4e-4, 1.4), ("big_cls", "bf16"): (7.5e-3, 1.4),   # 6.22e-4 1.11 / 4.98e-3 1.09
    ("train_cls", "f16"): (6.5e-4, 1.55), ("train_cls", "bf16"): (4.9e-3, 1.5),   # 4.29e-4 1.23 / 3.24e-3 1.17
    ("q_weight", "f16"): (3.2e-3, QK_RATIO), ("q_weight", "bf16"): (3.2e-2, QK_RATIO),   # 2.11e-3 1.94 / 2.11e-2 2.02
    ("k_weight", "f16"): (3.5e-3, QK_RATIO), ("k_weight", "bf16"): (3.5e-2, QK_RATIO),   # 2.33e-3 2.08 / 2.32e-2 2.09
    ("v_weight", "f16"): (8.6e-4, 1.55), ("v_weight", "bf16"): (7.6e-3, 1.65),   # 5.70e-4 1.22 / 5.05e-3 1.30
    ("ao_weight", "f16"): (1.1e-3, 1.7), ("ao_weight", "bf16"): (8.3e-3, 1.6),   # 6.97e-4 1.33 / 5.49e-3 1.27
    ("f1_weight", "f16"): (1.1e-3, 1.6), ("f1_weight", "bf16"): (9.3e-3, 1.65),   # 7.23e-4 1.27 / 6.19e-3 1.29
    ("f2_weight", "f16"): (1.1e-3, 1.7), ("f2_weight", "bf16"): (9.0e-3, 1.65),   # 7.11e-4 1.34 / 5.96e-3 1.28
    ("q_bias", "f16"): (4.1e-3, 3.4), ("q_bias", "bf16"): (4.8e-2, 3.85),   # 2.68e-3 2.69 / 3.13e-2 3.06
    ("v_bias", "f16"): (8.1e-4, 1.65), ("v_bias", "bf16"): (6.9e-3, 1.85),   # 5.37e-4 1.31 / 4.60e-3 1.46
    ("ao_bias", "f16"): (8.4e-4, 1.95), ("ao_bias", "bf16"): (5.6e-3, 1.9),   # 5.57e-4 1.52 / 3.68e-3 1.49
    ("f1_bias", "f16"): (1.1e-3, 1.9), ("f1_bias", "bf16"): (8.5e-3, 1.95),   # 6.86e-4 1.50 / 5.65e-3 1.54
    ("f2_bias", "f16"): (6.0e-4, 1.65), ("f2_bias", "bf16"): (5.2e-3, 1.75),   # 3.99e-4 1.29 / 3.44e-3 1.38
    ("ln1_weight", "f16"): (7.5e-4, 1.7), ("ln1_weight", "bf16"): (6.5e-3, 1.85),   # 4.99e-4 1.33 / 4.28e-3 1.48
    ("ln1_bias", "f16"): (8.1e-4, 2.05), ("ln1_bias", "bf16"): (5.0e-3, 1.7),   # 5.37e-4 1.62 / 3.29e-3 1.33
    ("ln2_weight", "f16"): (7.7e-4, 1.9), ("ln2_weight", "bf16"): (6.7e-3, 2.15),   # 5.11e-4 1.50 / 4.42e-3 1.68
    ("ln2_bias", "f16"): (5.6e-4, 1.85), ("ln2_bias", "bf16"): (4.3e-3, 1.65),   # 3.71e-4 1.48 / 2.80e-3 1.28
    ("eln_weight", "f16"): (7.5e-4, 1.7), ("eln_weight", "bf16"): (5.9e-3, 1.65),   # 4.96e-4 1.34 / 3.90e-3 1.31
    ("eln_bias", "f16"): (7.3e-4, 1.8), ("eln_bias", "bf16"): (5.3e-3, 1.7),   # 4.85e-4 1.44 / 3.51e-3 1.33
}
SWITCHES = ("MANNER_HIP_GEMM_SMALL_TILES", "MANNER_HIP_GEMM_ASM", "MANNER_HIP_GEMM_PANEL", "MANNER_HIP_DLN_FANIN", "MANNER_HIP_DEFER_LN",
            "MANNER_HIP_WGRAD_TR", "MANNER_HIP_TRAIN_SAVE16", "MANNER_HIP_TRAIN_ATTN_VALU", "MANNER_HIP_TRAIN_GELU_FUSED")


def test_bars_stay_under_the_conditions():
    """No ratio bar above FLAG / 2 (the host test's planted defects clear FLAG), no maximum above the whole-tensor bar of its mode."""
    for (quantity, mode), (bar_max, bar_ratio) in TILE_BARS.items():
        assert bar_ratio <= FLAG / 2 and bar_max <= ABS_CAP[mode], (quantity, mode)
    assert QK_RATIO == BARS[("qk_grad", "bf16")][1] and QK_RATIO <= FLAG / 2 and max(b[1] for b in PARITY_BARS.values()) <= FLAG / 2


def _env(monkeypatch, **switches):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv("MANNER_HIP_" + k, v)


# ------------------------------------------------------------------------------------------------ A. inference, persistent kernels forced
_LABELS = {}


def _labels(width, pad):
    """Over the real tokens only ([tokens, H]): 64 x 64 tiles of packed rows, (news, 32-token block, head) cells, and the selector."""
    if (width, pad) not in _LABELS:
        cfg, _, _, mask = _case(width, "hf", pad)
        sel = mask != 0
        _LABELS[(width, pad)] = (S.packed_tile_labels(mask, cfg.hidden)[sel], S.token_block_head_labels(mask, cfg.hidden, cfg.heads)[sel],
                                 torch.from_numpy(sel).to(DEV))
    return _LABELS[(width, pad)]


_REFS = {}


def _ref(width, pad, mode):
    """hidden_states[1], [2] over the real tokens and [CLS], float64, computed on the GPU once per (case, mode rounding)."""
    key = (width, pad, mode)
    if key not in _REFS:
        cfg, w, ids, mask = _case(width, "hf", pad)
        r = S.reference(cfg, w, ids, mask, mode=mode, store=STORE, device=DEV)
        sel = torch.from_numpy(mask != 0).to(DEV)
        _REFS[key] = {"h1": r["hidden"][1][sel].cpu().numpy(), "h2": r["hidden"][2][sel].cpu().numpy(), "cls": r["cls"].cpu().numpy()}
        del r
        torch.cuda.empty_cache()
    return _REFS[key]


def _inference_maps(enc, width, pad, mode, measured):
    cfg, w, ids, mask = _case(width, "hf", pad)
    ref = _ref(width, pad, mode)
    tiles, heads, sel = _labels(width, pad)
    news = S.news_labels(len(mask), cfg.hidden)
    failures, first = [], None
    for how, hl in (("host", mask.sum(1)), ("device", None)):
        out = [enc.encode_hidden(_cuda(ids), _cuda(mask), 1, precision=mode, host_lengths=hl)[sel],
               enc.encode_hidden(_cuda(ids), _cuda(mask), 2, precision=mode, host_lengths=hl)[sel],
               enc.encode_cls(_cuda(ids), _cuda(mask), precision=mode, host_lengths=hl)]
        hip.check_status(DEV)
        if first is not None and all(torch.equal(a, b) for a, b in zip(out, first[0])):
            maps = first[1]                                          # the same bits: the same maps
        else:
            h1, h2, cls = (t.cpu().numpy() for t in out)
            maps = (S.error_map(h1, ref["h1"], tiles), S.error_map(h1, ref["h1"], heads), S.error_map(h2, ref["h2"], tiles),
                    S.error_map(h2, ref["h2"], heads), S.error_map(cls, ref["cls"], news))
        if first is None:
            first = (out, maps)
        _check(f"{how}_h1_tiles", maps[0], TILE_BARS[("hidden1_tiles", mode)], measured, failures)
        _check(f"{how}_h1_heads", maps[1], BARS[("hidden", mode)], measured, failures)
        _check(f"{how}_h2_tiles", maps[2], TILE_BARS[("hidden2_tiles", mode)], measured, failures)
        _check(f"{how}_h2_heads", maps[3], TILE_BARS[("hidden2_heads", mode)], measured, failures)
        _check(f"{how}_cls", maps[4], BARS[("cls", mode)], measured, failures)
    return failures


SUBJECTS_A = {"default": {}, "asm8_panel256": {"GEMM_ASM": "8", "GEMM_PANEL": "256"}, "asm0_panel192": {"GEMM_ASM": "0", "GEMM_PANEL": "192"},
              "no_fanin": {"DLN_FANIN": "0"}}


@pytest.mark.parametrize("subject", list(SUBJECTS_A))
@pytest.mark.parametrize("pad", [512, 385])
@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("width", ["bert-base", "roberta-large"])
def test_inference_persistent_gemms_per_tile(width, mode, pad, subject, monkeypatch, measured):
    """encode_hidden(1), encode_hidden(2) per 64 x 64 tile of packed rows and per (news, 32-token block, head) cell, encode_cls per news,
    with host and with device lengths, every launch on a persistent kernel: library defaults, the hand-scheduled kernel on 256-row
    panels, the compiler-scheduled kernel on 192-row panels, the row statistics finished by a launch of their own."""
    _env(monkeypatch, GEMM_SMALL_TILES="0", **SUBJECTS_A[subject])
    failures = _inference_maps(_engine(width, "hf"), width, pad, mode, measured)
    assert not failures, failures


@pytest.mark.parametrize("pad", [512, 385])
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_inference_classic_layernorm_per_tile(mode, pad, monkeypatch, measured):
    """The same maps from a handle created under MANNER_HIP_DEFER_LN=0: LayerNorm as kernels of its own, not the deferred algebra."""
    _env(monkeypatch, GEMM_SMALL_TILES="0", DEFER_LN="0")
    key = ("bert-base", "hf", "classic_ln")
    if key not in _ENC:
        for k in list(_ENC):                             # one handle at a time
            _ENC.pop(k).close()
        cfg, w, _, _ = _case("bert-base", "hf", 512)
        _ENC[key] = hip.HipEncoder(cfg, w, precisions=("f16", "bf16"), device=DEV)       # the switch is read here
    failures = _inference_maps(_ENC[key], "bert-base", pad, mode, measured)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ B. more tiles than CUs
BIG_NEWS, BIG_PAD = 400, 96
BIG_LENS = np.resize([2, 31, 33, 63, 64, 65, 95, 96], BIG_NEWS)
_BIG = {}


def _big_case():
    if "case" not in _BIG:
        cfg, w, _, _ = _case("bert-base", "hf", 512)
        ids, mask = synth_news_tokens(BIG_NEWS, cfg, seed=BIG_PAD, lengths=BIG_LENS, pad_to=BIG_PAD)
        _BIG["case"] = cfg, w, ids, mask, S.packed_tile_labels(mask, cfg.hidden)[mask != 0], torch.from_numpy(mask != 0).to(DEV)
    return _BIG["case"]


def _big_ref(mode):
    m16 = mode if mode in S.DT16 else None                      # f16x3: the unrounded reference
    if m16 not in _BIG:
        cfg, w, ids, mask, _, sel = _big_case()
        r = S.reference(cfg, w, ids, mask, mode=m16, store=STORE if m16 else (), device=DEV)
        _BIG[m16] = {"h1": r["hidden"][1][sel].cpu().numpy(), "cls": r["cls"].cpu().numpy()}
        del r
        torch.cuda.empty_cache()
    return _BIG[m16]


@pytest.mark.parametrize("subject", ["default", "asm0"])
@pytest.mark.parametrize("mode", ["f16", "bf16", "f16x3"])
def test_inference_more_tiles_than_cus_per_tile(mode, subject, monkeypatch, measured):
    """22 450 tokens in one chunk, bert-base width: 88 row panels x 3 column tiles at N = 768, more than the device has CUs, so by the
    default launch rule workgroups take a second tile; neither 192 nor 256 divides the token count (a partial last panel)."""
    _env(monkeypatch, **({"GEMM_ASM": "0"} if subject == "asm0" else {}))
    cfg, w, ids, mask, tiles, sel = _big_case()
    tokens = int(mask.sum())
    assert tokens > 22016 and tokens % 192 and tokens % 256 and tokens <= 65536
    assert -(-tokens // 256) * (cfg.hidden // 256) > torch.cuda.get_device_properties(0).multi_processor_count
    ref = _big_ref(mode)
    enc = _engine("bert-base", "hf")
    h1 = enc.encode_hidden(_cuda(ids), _cuda(mask), 1, precision=mode, host_lengths=mask.sum(1))[sel].cpu().numpy()
    cls = enc.encode_cls(_cuda(ids), _cuda(mask), precision=mode, host_lengths=mask.sum(1)).cpu().numpy()
    hip.check_status(DEV)
    failures = []
    _check("h1_tiles", S.error_map(h1, ref["h1"], tiles), TILE_BARS[("big_hidden1_tiles", mode)], measured, failures)
    _check("cls", S.error_map(cls, ref["cls"], S.news_labels(len(mask), cfg.hidden)), TILE_BARS[("big_cls", mode)], measured, failures)
    if mode == "f16x3":
        err = max(float(np.abs(h1 - ref["h1"]).max()), float(np.abs(cls - ref["cls"]).max()))
        measured(max_abs_err=err)
        assert err < 1e-4, err
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ C. training, every gradient
CASES_C = [("bert-base", 512), ("roberta-large", 385)]
SUBJECTS_C = {"small_tiles": ({}, 1), "persistent": ({"GEMM_SMALL_TILES": "0"}, 3),
              "persistent_transposing_wgrad": ({"GEMM_SMALL_TILES": "0", "WGRAD_TR": "0"}, 3)}      # switches, the saved layout they give
SHORT = {"attention.self.query": "q", "attention.self.key": "k", "attention.self.value": "v", "attention.output.dense": "ao",
         "attention.output.LayerNorm": "ln1", "intermediate.dense": "f1", "output.dense": "f2", "output.LayerNorm": "ln2",
         "embeddings.LayerNorm": "eln"}


def _quantity(name):
    """encoder.layer.1.attention.self.query.weight -> (layer tag "l1", quantity "q_weight")."""
    stem, leaf = name.rsplit(".", 1)
    layer = ""
    if stem.startswith("encoder.layer."):
        layer, stem = "l" + stem.split(".")[2], stem.split(".", 3)[3]
    return layer, f"{SHORT[stem]}_{leaf}"


def _held(w):
    """Every 2-D encoder weight, every bias and LayerNorm parameter; not the embedding tables (test_gpu_attention_slices maps those),
    not the key bias (zero in exact arithmetic: no scale to hold it to; test_gpu_long_train bounds it)."""
    return [k for k in w if (k.startswith("encoder.layer.") or k.startswith("embeddings.LayerNorm.")) and not k.endswith("key.bias")]


_TRAIN_REFS = {}


def _train_ref(width, pad, mode):
    key = (width, pad, mode)
    if key not in _TRAIN_REFS:
        cfg, w, ids, mask = _case(width, "hf", pad)
        keep = _replay_keep(SEED, DROP["p_hidden"], DROP["p_out"], cfg, mask)
        keep.p_attn = DROP["p_attn"]
        r = S.reference(cfg, w, ids, mask, mode=mode, store=STORE, train=True, R=_R(cfg, len(mask)), keep=keep, device=DEV,
                        grad_keys=None, **DROP)
        _TRAIN_REFS[key] = {"cls": r["cls"].cpu().numpy(), "grads": {k: r["grads"][k].cpu().numpy() for k in _held(w)}}
        del r
        torch.cuda.empty_cache()
    return _TRAIN_REFS[key]


@pytest.mark.parametrize("subject", list(SUBJECTS_C))
@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("width,pad", CASES_C)
def test_train_every_gradient_per_tile(width, pad, mode, subject, monkeypatch, measured):
    """encode_train(max_len=512), nothing frozen, dropout on at all five sites with the masks replayed into the reference: the Q, K, V,
    attention-output, FFN1 and FFN2 weight gradients of both layers per 128 x 64 tile, every bias and LayerNorm gamma / beta gradient
    (the embedding LayerNorm included) per 64 elements, [CLS] per news — from the 128 x 128 kernels (environment unset), the
    persistent kernels with wgrad_tr_kernel, and the persistent kernels with the transposing weight-gradient path."""
    switches, layout = SUBJECTS_C[subject]
    _env(monkeypatch, **switches)
    cfg, w, ids, mask = _case(width, "hf", pad)
    ref = _train_ref(width, pad, mode)
    params = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in w.items()}
    out = train.encode_train(cfg, params, _cuda(ids), _cuda(mask), precision=mode, seed=SEED, max_len=_lib.MAX_LEN_TRAIN, **DROP)
    (out * _R(cfg, len(mask)).float().to(DEV)).sum().backward()
    hip.check_status(DEV)
    assert _lib.load().manner_hip_train_layout_last() == layout                      # the subject really ran
    failures = []
    _check("cls", S.error_map(out.detach().cpu().numpy(), ref["cls"], S.news_labels(len(mask), cfg.hidden)),
           TILE_BARS[("train_cls", mode)], measured, failures)
    for k in _held(w):
        g, r = params[k].grad.cpu().numpy(), ref["grads"][k]
        layer, quantity = _quantity(k)
        if g.ndim == 2:
            m = S.error_map(g, r, S.weight_tile_labels(g.shape), per_slice=True)
        else:
            m = S.error_map(g, r, S.vector_block_labels(len(g)), min_count=64, per_slice=True)
        _check(f"{layer}_{quantity}".lstrip("_"), m, TILE_BARS[(quantity, mode)], measured, failures)
    assert not failures, failures
