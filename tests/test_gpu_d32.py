"""Head dimension 32 (the MiniLM family) through the inference engine: encode_cls / encode_hidden and the module mirror in eval()
against the reference's goldens and the oracle, the bits of a row independent of its neighbours, padding and chunking, and the
refusals (split modes, other head dimensions, training, full rows).  Run on the MI355X box: ``pytest -m gpu``.

The 16-bit bars are MEASURED in the session, not chosen: the head_dim-64 kernels on the twin shape (half the heads, everything else
equal: "tiny-bert-512" for "tiny-bert-d32"), the same seed, std and tokens, against the oracle; head_dim 32 may err 2 x that against
the reference (half the products per score, an accumulation order no better, other weights per head).  Both sides are recorded.

The planted scale defect (tests/d32_common.py) is held 4 x clear of each bar, measured as the bar's error is: max-abs over the
fixture's output.  Per ROW the defect is at least 8.7e-2 (tiny shape) / 2.3e-1 (H = 384) at the 16-bit fixtures' std 0.1, which is
4 x clear of the f16 bars (2 x 2.9e-3, 2 x 4.1e-3) but not of the bf16 bars (2 x 2.6e-2, 2 x 3.0e-2: bf16's own rounding), at no
std between 0.05 and 0.2; the per-row minimum is recorded next to the maximum."""
import dataclasses
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import manner_oracle as O  # noqa: E402  (tests/conftest.py puts oracle/ on sys.path)
from manner_amd import hip, train  # noqa: E402
from manner_amd.config import PRESETS, EncoderConfig  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from manner_amd.weights import make_plm_weights  # noqa: E402

import d32_common as D  # noqa: E402

DEV = "cuda:0"
MODES = ("fp32", "f16", "bf16")
REFUSAL = "head_dim 32: training and full rows support head_dim 64 only"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_ENC = {}


def _encoder(cfg, seed, std):
    key = (cfg, seed, std)
    if key not in _ENC:
        w = make_plm_weights(cfg, seed=seed, std=std)
        _ENC[key] = (hip.HipEncoder(cfg, w, precisions=MODES, device=DEV), w)
    return _ENC[key]


def _fixture_encoder(meta):
    return _encoder(PRESETS[meta["preset"]], meta["seed"], meta["std"])[0]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for k in list(_ENC):
        _ENC.pop(k)[0].close()


# ---------------------------------------------------------------- fp32 mode
@pytest.mark.parametrize("name", D.GOLDEN_ENC)
def test_fp32_meets_the_fp32_bar_on_the_goldens(golden_dir, name, measured):
    z, meta = D.load(golden_dir, name)
    enc = _fixture_encoder(meta)                 # on the parent commit encoder_create raises here
    ids, mask = _cuda(z["ids"]), _cuda(z["mask"])
    out = enc.encode_cls(ids, mask, precision="fp32", host_lengths=z["mask"].sum(1))
    enc.status()
    err = np.abs(out.cpu().numpy() - z["out"]).max(1)
    measured(bound=D.FP32_TOL, max_abs_err=err.max(), rows_over_128_max_abs_err=err[z["mask"].sum(1) > 128].max())
    print(f"{name} fp32: max-abs err vs reference {err.max():.3e} (per row {np.array2string(err, precision=1)})")
    assert err.max() < D.FP32_TOL
    assert torch.equal(out, enc.encode_cls(ids, mask, precision="fp32"))                                       # device-side lengths
    assert torch.equal(out, enc.encode_cls(ids, mask, precision="fp32", host_lengths=z["mask"].sum(1)))      # two calls


def test_fp32_encode_hidden_of_long_rows_matches_reference(golden_dir, measured):
    z, meta = D.load(golden_dir, "hidden_mini_minilm")
    enc = _fixture_encoder(meta)
    keep = torch.from_numpy(z["mask"]).bool()
    rows = torch.from_numpy(z["rows"])
    for k in meta["layers"]:
        h = enc.encode_hidden(_cuda(z["ids"]), _cuda(z["mask"]), k, precision="fp32").cpu()
        enc.status()
        assert float(h[~keep].abs().max()) == 0.0
        err = np.abs(h[keep][rows].numpy() - z[f"h{k}"]).max()
        measured(**{f"h{k}_err": err, "bound": D.FP32_TOL})
        print(f"hidden_states[{k}] fp32: max-abs err {err:.3e}")
        assert err < D.FP32_TOL, (k, err)


# the stress cases of tests/test_gpu_long_rows.py with stride 32 (d32_common.stress_weights, shared with test_gpu_d32_slices.py)
STRESS_CFG = D.STRESS_CFG
_stress_weights = D.stress_weights


@pytest.mark.parametrize("kind", ["equal", "peaked_last", "peaked_first"])
def test_fp32_long_kernels_match_the_oracle_under_stress(kind, measured):
    cfg, w = _stress_weights(kind)
    lengths = [129, 160, 161, 512, 2, 128]
    ids, mask = synth_news_tokens(len(lengths), cfg, seed=81, lengths=np.asarray(lengths))
    if kind in D.MARKER_AT:
        D.place_marker(ids, lengths, kind)
    enc = hip.HipEncoder(cfg, w, precisions=("fp32",), device=DEV)
    try:
        out = enc.encode_cls(_cuda(ids), _cuda(mask), precision="fp32", host_lengths=mask.sum(1)).cpu().numpy()
        h1 = enc.encode_hidden(_cuda(ids), _cuda(mask), 1, precision="fp32", host_lengths=mask.sum(1)).cpu()
        enc.status()
    finally:
        enc.close()
    ref = O.encode_cls(ids, mask, w, cfg).numpy()
    ref1 = O.encode_tokens(ids, mask, {k: v for k, v in w.items() if "layer.1." not in k}, dataclasses.replace(cfg, layers=1))
    keep = torch.from_numpy(mask).bool()
    err = np.abs(out - ref).max()
    err1 = float((h1[keep] - ref1[keep]).abs().max())
    measured(cls_err=err, layer0_err=err1, bound=D.FP32_TOL)
    print(f"{kind}: CLS err {err:.3e}, hidden_states[1] err {err1:.3e}")
    assert err < D.FP32_TOL and err1 < D.FP32_TOL


# ---------------------------------------------------------------- f16 / bf16: bars measured on the head_dim-64 twin
_TWIN = {}


def _twin_measure(golden_dir, name, prec):
    """(max-abs error, cosine deficit) of the head_dim-64 kernels on the twin shape against the oracle: same seed, std and tokens."""
    key = (name, prec)
    if key not in _TWIN:
        z, meta = D.load(golden_dir, name)
        tcfg = D.twin_config(PRESETS[meta["preset"]])
        assert tcfg.head_dim == 64
        enc, tw = _encoder(tcfg, meta["seed"], meta["std"])
        if ("ref", name) not in _TWIN:
            _TWIN[("ref", name)] = O.encode_cls(z["ids"], z["mask"], tw, tcfg).numpy()
        ref = _TWIN[("ref", name)]
        out = enc.encode_cls(_cuda(z["ids"]), _cuda(z["mask"]), precision=prec).cpu().numpy()
        enc.status()
        _TWIN[key] = (float(np.abs(out - ref).max()), float(1.0 - D.cosine(out.astype(np.float64), ref.astype(np.float64)).min()))
    return _TWIN[key]


def _scale_defect(golden_dir, name):
    key = ("defect", name)
    if key not in _TWIN:
        z, meta = D.load(golden_dir, name)
        cfg, w = D.fixture_weights(meta)
        _TWIN[key] = np.abs(O.encode_cls(z["ids"], z["mask"], D.defect_scale(cfg, w), cfg).numpy() - z["out"]).max(1)
    return _TWIN[key]


def _check_16bit(golden_dir, name, prec, out, ref, measured, tag=""):
    twin_err, twin_cosdef = _twin_measure(golden_dir, name, prec)
    bar, cos_bar = 2.0 * twin_err, 2.0 * twin_cosdef
    err = np.abs(out - ref).max()
    cosdef = 1.0 - D.cosine(out.astype(np.float64), ref.astype(np.float64)).min()
    defect = _scale_defect(golden_dir, name)
    measured(**{tag + "twin_max_abs_err": twin_err, tag + "twin_cosine_deficit": twin_cosdef, tag + "bound": bar, tag + "cosine_deficit_bound": cos_bar,
                tag + "max_abs_err": err, tag + "cosine_deficit": cosdef, tag + "scale_defect_max_abs": defect.max(),
                tag + "scale_defect_min_over_rows": defect.min()})
    print(f"{name} {prec}{' ' + tag if tag else ''}: max-abs err {err:.3e} (bar 2 x {twin_err:.3e}), cosine deficit {cosdef:.3e} (bar 2 x {twin_cosdef:.3e}); "
          f"scale defect {defect.max():.3e} (per row at least {defect.min():.3e})")
    assert defect.max() > 4.0 * bar, "the fixture cannot see the head_dim-64 constant at this bar"
    assert err < bar and cosdef <= cos_bar


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name", D.GOLDEN_ENC_16BIT)
def test_16bit_modes_within_twice_the_head_dim_64_twin(golden_dir, name, prec, measured):
    z, meta = D.load(golden_dir, name)
    assert meta["std"] == 0.1
    enc = _fixture_encoder(meta)
    out = enc.encode_cls(_cuda(z["ids"]), _cuda(z["mask"]), precision=prec).cpu().numpy()
    enc.status()
    _check_16bit(golden_dir, name, prec, out, z["out"], measured)


# ---------------------------------------------------------------- bits
def _short_and_long(cfg, seed):
    g = np.random.default_rng(seed)
    short_len = g.integers(2, 97, 24)
    short_len[:5] = [2, 96, 33, 32, 64]
    s_ids, s_mask = synth_news_tokens(24, cfg, seed=seed, lengths=short_len)
    l_ids, l_mask = synth_news_tokens(6, cfg, seed=seed + 1, lengths=np.array([129, 512, 300, 161, 2, 128]), pad_to=512)
    order = np.concatenate([np.arange(0, 24, 2), [24, 25], np.arange(1, 24, 2), [26, 27, 28, 29]])     # short news between the long ones
    pad = lambda a, v: np.pad(a, ((0, 0), (0, 512 - a.shape[1])), constant_values=v)   # noqa: E731
    b_ids = np.concatenate([pad(s_ids, cfg.pad_id), l_ids])[order]
    b_mask = np.concatenate([pad(s_mask, 0), l_mask])[order]
    return s_ids, s_mask, b_ids, b_mask, np.argsort(order)[:24]


@pytest.mark.parametrize("prec", MODES)
@pytest.mark.parametrize("name", D.GOLDEN_ENC)
def test_short_rows_give_the_same_bits_next_to_long_rows(golden_dir, name, prec):
    """A row of <= 128 tokens runs the same kernel body whatever the padded length and its neighbours: encode_cls and encode_hidden,
    with and without host lengths."""
    _, meta = D.load(golden_dir, name)
    enc = _fixture_encoder(meta)
    s_ids, s_mask, b_ids, b_mask, where = _short_and_long(enc.cfg, 70)
    assert s_ids.shape[1] <= 96
    lp = s_ids.shape[1]
    where = torch.from_numpy(where).to(DEV)
    for hl in (False, True):
        alone = enc.encode_cls(_cuda(s_ids), _cuda(s_mask), precision=prec, host_lengths=s_mask.sum(1) if hl else None)
        mixed = enc.encode_cls(_cuda(b_ids), _cuda(b_mask), precision=prec, host_lengths=b_mask.sum(1) if hl else None)
        enc.status()
        assert torch.equal(alone, mixed[where]), (prec, hl)
    alone = enc.encode_hidden(_cuda(s_ids), _cuda(s_mask), 1, precision=prec)
    rows = enc.encode_hidden(_cuda(b_ids), _cuda(b_mask), 1, precision=prec, host_lengths=b_mask.sum(1))[where]
    enc.status()
    assert torch.equal(alone, rows[:, :lp]) and float(rows[:, lp:].abs().max()) == 0.0


@pytest.mark.parametrize("prec", MODES)
def test_chunking_does_not_change_the_bits(golden_dir, prec, measured):
    """Many 129-token rows between 2-token rows with a workspace of 256-token chunks: every chunk boundary falls somewhere else in the
    pattern; the result is the single-chunk result bit for bit (and, in fp32, the oracle's)."""
    _, meta = D.load(golden_dir, "enc_tiny_bert_d32")
    enc = _fixture_encoder(meta)
    cfg, w = D.fixture_weights(meta)
    lengths = np.array([129, 2, 2, 129, 129, 2] * 6)
    ids, mask = synth_news_tokens(len(lengths), cfg, seed=82, lengths=lengths)
    whole = enc.encode_cls(_cuda(ids), _cuda(mask), precision=prec, host_lengths=mask.sum(1))
    small = enc.encode_cls(_cuda(ids), _cuda(mask), precision=prec, host_lengths=mask.sum(1), max_chunk_tokens=256)
    dev_lengths = enc.encode_cls(_cuda(ids), _cuda(mask), precision=prec, max_chunk_tokens=256)
    enc.status()
    assert torch.equal(whole, small) and torch.equal(whole, dev_lengths)
    if prec == "fp32":
        err = np.abs(whole.cpu().numpy() - O.encode_cls(ids, mask, w, cfg).numpy()).max()
        measured(max_abs_err=err, bound=D.FP32_TOL)
        assert err < D.FP32_TOL


# ---------------------------------------------------------------- edges
@pytest.mark.parametrize("prec", MODES)
@pytest.mark.parametrize("name", D.GOLDEN_ENC)
def test_calls_of_one_and_three_news(golden_dir, name, prec):
    """One news is 2 (tiny shape) or 6 (H = 384) head pairs, three news 6 or 18: not a multiple of the four waves of a 16-bit or [CLS]
    workgroup.  (A head_dim-32 model has an even number of pairs, so the two-wave f32 workgroups are always full.)  Every row gives the
    bits it has in the 16-news batch; L = 2 alone as well."""
    z, meta = D.load(golden_dir, name)
    enc = _fixture_encoder(meta)
    lens = z["mask"].sum(1)
    full = enc.encode_cls(_cuda(z["ids"]), _cuda(z["mask"]), precision=prec)
    full_h = enc.encode_hidden(_cuda(z["ids"]), _cuda(z["mask"]), 1, precision=prec)
    for pick in ([0], [15], [10], [0, 9, 12], [4, 13, 1]):
        lp = int(lens[pick].max())
        ids, mask = _cuda(z["ids"][pick, :lp]), _cuda(z["mask"][pick, :lp])
        out = enc.encode_cls(ids, mask, precision=prec)
        h = enc.encode_hidden(ids, mask, 1, precision=prec)
        enc.status()
        idx = torch.tensor(pick, device=DEV)
        assert torch.equal(out, full[idx]), (pick, prec)
        assert torch.equal(h, full_h[idx][:, :lp]), (pick, prec)
    assert lens[0] == 2


# ---------------------------------------------------------------- refusals
def test_split_modes_are_refused_at_head_dim_32():
    cfg = PRESETS["tiny-bert-d32"]
    w = make_plm_weights(cfg, seed=1, std=0.05)
    for mode in ("f16x3", "bf16x3"):
        with pytest.raises(RuntimeError, match=r'BF16X3 / F16X3 have no head_dim 32 attention .*"fp32" is the parity-grade mode'):
            hip.HipEncoder(cfg, w, precisions=("fp32", mode), device=DEV)
    # at a width the split modes tile, too
    cfg = EncoderConfig(hidden=256, heads=8, layers=1, intermediate=1024, vocab=512, max_pos=64)
    with pytest.raises(RuntimeError, match='"fp32" is the parity-grade mode'):
        hip.HipEncoder(cfg, make_plm_weights(cfg, seed=1, std=0.05), precisions=("f16x3",), device=DEV)


@pytest.mark.parametrize("hidden,heads", [(128, 8), (384, 8)])        # head_dim 16, 48
def test_other_head_dims_are_refused(hidden, heads):
    cfg = EncoderConfig(hidden=hidden, heads=heads, layers=1, intermediate=512, vocab=512, max_pos=64)
    with pytest.raises(RuntimeError, match=rf"hidden={hidden} heads={heads} .*head_dim 32 or 64"):
        hip.HipEncoder(cfg, make_plm_weights(cfg, seed=1, std=0.05), precisions=("fp32",), device=DEV)


def _d32_params(requires_grad):
    cfg = PRESETS["tiny-bert-d32"]
    w = make_plm_weights(cfg, seed=2, std=0.05)
    params = {k: torch.from_numpy(v).to(DEV).requires_grad_(requires_grad) for k, v in w.items() if not k.startswith("pooler.")}
    ids, mask = synth_news_tokens(3, cfg, seed=2, lengths=np.array([5, 17, 9]))
    return cfg, params, _cuda(ids), _cuda(mask)


@pytest.mark.parametrize("prec", MODES)
def test_training_and_full_rows_refuse_head_dim_32(prec):
    """manner_hip_train_forward and manner_hip_encode_full return the error from their configuration check, which precedes every plan and
    launch; the device status word stays clear."""
    cfg, params, ids, mask = _d32_params(True)
    with pytest.raises(RuntimeError, match=REFUSAL):
        train.encode_train(cfg, params, ids, mask, precision=prec, seed=1)
    with pytest.raises(RuntimeError, match=REFUSAL):
        train.encode_full_train(cfg, params, ids, mask, precision=prec, seed=1)
    with pytest.raises(RuntimeError, match=REFUSAL):
        hip.encode_full(cfg, {k: v.detach() for k, v in params.items()}, ids, mask, precision=prec)
    hip.check_status(ids.device)


def _mirror(meta, cls="MannerTextEncoder"):
    from manner_amd.models.components import news_encoder as NE
    cfg = PRESETS[meta["preset"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if cls == "MannerTextEncoder":
            enc, prefix = NE.MannerTextEncoder(plm_model=meta["preset"], frozen_layers=[0], dropout_probability=0.2), "plm_model."
        elif cls == "MannerNewsEncoder":
            enc = NE.MannerNewsEncoder(plm_model=meta["preset"], frozen_layers=[0], dropout_probability=0.2, use_entities=False, entity_embeddings=None,
                                       entity_embedding_dim=100, num_attention_heads=10, query_vector_dim=200, text_embedding_dim=cfg.hidden)
            prefix = "text_encoder.plm_model."
        else:
            enc = NE.PLMTextEncoder(plm_model=meta["preset"], frozen_layers=[0], text_embedding_dim=cfg.hidden, num_attention_heads=4,
                                    query_vector_dim=32, dropout_probability=0.2)
            prefix = "plm_model."
    w = make_plm_weights(cfg, seed=meta["seed"], std=meta["std"])
    enc.load_state_dict({prefix + k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    return enc.to(DEV)


def test_module_mirror_raises_in_train_mode(golden_dir):
    z, meta = D.load(golden_dir, "enc_tiny_bert_d32")
    text = {"input_ids": _cuda(z["ids"][:4, :64]), "attention_mask": _cuda(z["mask"][:4, :64])}
    enc = _mirror(meta).train()
    with pytest.raises(ValueError, match="head_dim 32 .*supports head_dim 64 only"):
        enc(text)
    news = _mirror(meta, "MannerNewsEncoder").train()
    with pytest.raises(ValueError, match="head_dim 32 .*supports head_dim 64 only"):
        news({"text": text})
    plm = _mirror(meta, "PLMTextEncoder")
    for mode in (plm.train(), plm.eval()):
        with pytest.raises(ValueError, match="head_dim 32 .*full rows.* head_dim 64 only"), torch.no_grad():
            mode(text)


# ---------------------------------------------------------------- the module mirror in eval()
@pytest.mark.parametrize("autocast,mode", [(None, "fp32"), (torch.float16, "f16"), (torch.bfloat16, "bf16")])
def test_module_mirror_eval_follows_the_callers_autocast(golden_dir, autocast, mode, measured):
    name = "enc_tiny_bert_d32" if mode == "fp32" else "enc_tiny_bert_d32_s10"
    z, meta = D.load(golden_dir, name)
    enc = _mirror(meta).eval()
    text = {"input_ids": _cuda(z["ids"]), "attention_mask": _cuda(z["mask"])}
    with torch.no_grad():
        if autocast is None:
            assert enc.resolved_precision() == "fp32"
            out = enc(text)
        else:
            with torch.autocast("cuda", dtype=autocast):
                assert enc.resolved_precision() == mode
                out = enc(text)
    enc.check_inputs()
    out = out.float().cpu().numpy()
    if mode == "fp32":
        err = np.abs(out - z["out"]).max()
        measured(bound=D.FP32_TOL, max_abs_err=err)
        print(f"mirror eval, no autocast: max-abs err {err:.3e}")
        assert err < D.FP32_TOL
    else:
        _check_16bit(golden_dir, name, mode, out, z["out"], measured)


@pytest.mark.parametrize("mode", MODES)
def test_module_mirror_cache_returns_the_bits_of_a_fresh_encode(golden_dir, mode):
    z, meta = D.load(golden_dir, "enc_tiny_bert_d32")
    enc = _mirror(meta, "MannerNewsEncoder").eval()
    news = {"text": {"input_ids": _cuda(z["ids"]), "attention_mask": _cuda(z["mask"])}}
    enc.text_encoder.precision = mode
    with torch.no_grad():
        fresh = enc(news).clone()
        enc.text_encoder.embedding_cache_rows = 64
        miss = enc(news).clone()                         # rows encoded and stored
        hit = enc(news).clone()                          # every row from the table
    assert torch.equal(fresh, miss) and torch.equal(fresh, hit)
