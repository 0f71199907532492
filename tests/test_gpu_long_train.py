"""Training on news of 129..512 tokens (MANNER_HIP_MAX_LEN_TRAIN): the long-row training attention (train_attn.hip's
*_long_kernel passes in the 16-bit modes, the row-block grid of train.hip's VALU kernels in fp32 mode) against the reference's own
gradients (tests/golden/train_long_*.npz), the oracle with replayed dropout masks, the VALU kernels and the fp32 mode — and the
rows of <= 128 tokens keeping their bits.  Run on the MI355X box: ``pytest -m gpu``."""
import ctypes as C
import dataclasses
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import manner_oracle as O  # noqa: E402
from manner_amd import _lib, hip, train  # noqa: E402
from manner_amd.config import PRESETS  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from manner_amd.weights import make_plm_weights  # noqa: E402
from test_long_train_host import KEY_BIAS_ABS, split_key_bias  # noqa: E402
from test_oracle_golden import compare_train_grads, golden_train_case  # noqa: E402

DEV = "cuda:0"
LONG = _lib.MAX_LEN_TRAIN


def _params(w, frozen=()):
    return {k: torch.from_numpy(v).to(DEV).requires_grad_(k not in frozen) for k, v in w.items()}


def _grads(params):
    return {k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in params.items()}


def _rel(a, b, floor=1e-3):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


def _cos(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


def _cuda(a):
    return torch.from_numpy(a).to(DEV)


def _run(cfg, params, ids, mask, R, **kw):
    kw.setdefault("max_len", LONG)
    out = train.encode_train(cfg, params, ids, mask, **kw)
    (out * R).sum().backward()
    return out.detach().cpu().numpy(), _grads(params)


# ------------------------------------------------------------------------------------------------ 1. reference parity
@pytest.mark.parametrize("name", ["train_long_tiny_bert", "train_long_tiny_roberta"])
def test_long_rows_train_gradients_match_reference(golden_dir, name):
    """fp32, all dropout off, rows of 2..512 tokens: the [CLS] outputs and every parameter gradient of the reference (the bars of
    test_train_gradients_match_reference), incl. the gradient through the frozen layer 0 into the embedding tables."""
    cfg, w, z, meta, expect = golden_train_case(golden_dir, name)
    params = _params(w, frozen=set(meta["frozen"]))
    out = train.encode_train(cfg, params, _cuda(z["ids"]), _cuda(z["mask"]), precision="fp32", p_hidden=0.0, p_attn=0.0, p_out=0.0,
                             max_len=LONG)
    assert np.abs(out.detach().cpu().numpy() - z["out"]).max() < 1e-4
    (out * _cuda(z["R"])).sum().backward()
    hip.check_status(DEV)
    rest, kb = split_key_bias(expect)
    g = _grads(params)
    compare_train_grads(g, z, meta, rest, rel=1e-3)
    for k in kb:
        assert np.abs(g[k]).max() < KEY_BIAS_ABS, (k, np.abs(g[k]).max())


# ------------------------------------------------------------------------------------------------ 2. dropout against the oracle
def _replay_keep(seed, p_hidden, p_out, cfg, mask_np):
    """The implementation's keep-bits (manner_hip_dropout_mask) in the oracle's padded layout; the attention bits of a news of more
    than 128 tokens come from its own stream (site | 0x80000000, index ((m * heads + head) << 9) + key)."""
    lens = mask_np.sum(1)
    cu = np.concatenate([[0], np.cumsum(lens)])
    n, lp = mask_np.shape
    m, h, a = int(cu[-1]), cfg.hidden, cfg.heads

    def keep(site, kind):
        if kind == "cls":
            return train.dropout_mask(seed, site, p_out, n * h, DEV).cpu().view(n, h).float()
        if kind == "rows":
            bits = train.dropout_mask(seed, site, p_hidden, m * h, DEV).cpu().view(m, h).float()
            out = torch.ones(n, lp, h)
            for i in range(n):
                out[i, :lens[i]] = bits[cu[i]:cu[i + 1]]
            return out
        short = train.dropout_mask(seed, site, keep.p_attn, m * a * 256, DEV).cpu().view(m, a, 256).float()
        long_ = train.dropout_mask(seed, site | 0x80000000, keep.p_attn, m * a * 512, DEV).cpu().view(m, a, 512).float()
        out = torch.ones(n, a, lp, lp)
        for i in range(n):
            src = long_ if lens[i] > _lib.MAX_LEN else short
            k = min(lp, src.shape[2])
            out[i, :, :lens[i], :k] = src[cu[i]:cu[i + 1], :, :k].permute(1, 0, 2)
        return out

    return keep


def test_long_rows_dropout_matches_oracle_on_replayed_masks():
    """All five sites on (0.1 / 0.1 / 0.2), short and long rows in one batch (the long rows' attention bits from their own stream):
    forward and backward against autograd over the oracle fed the very masks the kernels drew; a second seed, another network."""
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=81, std=0.05, with_pooler=False)
    frozen = {k for k in w if "layer.0." in k}
    lens = np.array([2, 40, 128, 129, 257, 300])
    ids_np, mask_np = synth_news_tokens(len(lens), cfg, seed=81, lengths=lens)
    R = torch.from_numpy(np.random.default_rng(3).standard_normal((len(lens), cfg.hidden)).astype(np.float32))
    seed, ph, pa, po = 7654321, 0.1, 0.1, 0.2
    params = _params(w, frozen)
    out = train.encode_train(cfg, params, _cuda(ids_np), _cuda(mask_np), precision="fp32", p_hidden=ph, p_attn=pa, p_out=po, seed=seed,
                             max_len=LONG)
    (out * R.to(DEV)).sum().backward()
    keep = _replay_keep(seed, ph, po, cfg, mask_np)
    keep.p_attn = pa
    wt = {k: torch.from_numpy(v).requires_grad_(k not in frozen) for k, v in w.items()}
    ref = O.encode_cls_train(ids_np, mask_np, wt, cfg, p_hidden=ph, p_attn=pa, p_out=po, keep=keep)
    (ref * R).sum().backward()
    assert (out.detach().cpu() - ref.detach()).abs().max() < 2e-4
    g = _grads(params)
    for k, v in wt.items():
        if v.grad is None:
            assert g[k] is None, k
        elif k.endswith("attention.self.key.bias"):
            assert np.abs(g[k]).max() < KEY_BIAS_ABS and np.abs(v.grad.numpy()).max() < KEY_BIAS_ABS, k
        else:
            assert _rel(g[k], v.grad.numpy()) < 2e-3, (k, _rel(g[k], v.grad.numpy()))
    out2 = train.encode_train(cfg, params, _cuda(ids_np), _cuda(mask_np), precision="fp32", p_hidden=ph, p_attn=pa, p_out=po,
                              seed=seed + 1, max_len=LONG)
    assert (out2 - out).abs().max() > 1e-2


# ------------------------------------------------------------------------------------------------ 3. matrix pipe against VALU
@pytest.mark.parametrize("precision,rel,cos_min", [("f16", 2e-2, 0.9999), ("bf16", 8e-2, 0.999)])
def test_long_matrix_pipe_attention_tracks_the_valu_kernels(precision, rel, cos_min, monkeypatch, measured):
    """The *_long_kernel passes against the VALU kernels' row-block form (MANNER_HIP_TRAIN_ATTN_VALU=1), one process, same weights,
    inputs and dropout bits; the bars of test_matrix_pipe_training_attention_tracks_the_valu_kernels.  bert-base width, 2 layers,
    rows that end inside a key tile, short rows beside them."""
    cfg = dataclasses.replace(PRESETS["bert-base-uncased"], layers=2)
    w = make_plm_weights(cfg, seed=82, std=0.02, with_pooler=False)
    lens = np.array([17, 128, 129, 200, 333, 480, 512])
    ids_np, mask_np = synth_news_tokens(len(lens), cfg, seed=82, lengths=lens)
    ids, mask = _cuda(ids_np), _cuda(mask_np)
    R = torch.from_numpy(np.random.default_rng(8).standard_normal((len(lens), cfg.hidden)).astype(np.float32)).to(DEV)
    res = {}
    for valu in ("1", None):
        if valu is None:
            monkeypatch.delenv("MANNER_HIP_TRAIN_ATTN_VALU", raising=False)
        else:
            monkeypatch.setenv("MANNER_HIP_TRAIN_ATTN_VALU", valu)
        params = _params(w)
        out = train.encode_train(cfg, params, ids, mask, precision=precision, p_hidden=0.1, p_attn=0.1, p_out=0.2, seed=11, max_len=LONG)
        (out * R).sum().backward()
        res[valu] = (out.detach().cpu().numpy(), _grads(params))
    monkeypatch.delenv("MANNER_HIP_TRAIN_ATTN_VALU", raising=False)
    a, b = res[None][0].astype(np.float64), res["1"][0].astype(np.float64)
    assert np.abs(a - b).max() <= rel * np.abs(b).max()
    worst = (0.0, 1.0, None)
    for k, g in res["1"][1].items():
        x, y = res[None][1][k].astype(np.float64).ravel(), g.astype(np.float64).ravel()
        assert np.isfinite(x).all(), k
        if k.endswith("attention.self.key.bias"):
            qs = np.abs(res["1"][1][k.replace("key.bias", "query.bias")]).max()
            assert np.abs(x).max() <= 2e-2 * qs and np.abs(y).max() <= 2e-2 * qs, (k, np.abs(x).max(), np.abs(y).max(), qs)
            continue
        e = np.abs(x - y).max() / max(np.abs(y).max(), 1e-12)
        c = _cos(x, y)
        if e > worst[0]:
            worst = (e, c, k)
        assert e <= rel and c >= cos_min, (k, e, c)
    measured(bound_rel=rel, bound_cos=cos_min, worst_rel_to_max=worst[0], cosine_of_that_tensor=worst[1], tensor=str(worst[2]),
             output_max_abs_diff=float(np.abs(a - b).max()), output_scale=float(np.abs(b).max()))


# ------------------------------------------------------------------------------------------------ 4. 16-bit modes against fp32
@pytest.mark.parametrize("save16", ["1", "0"])
@pytest.mark.parametrize("precision,tol,cos_min", [("f16", 2e-2, 0.999), ("bf16", 1e-1, 0.99)])
def test_long_rows_16bit_modes_track_fp32(precision, tol, cos_min, save16, monkeypatch, measured):
    """Both saved layouts: the lean one (16-bit-only activations) needs the fused-GeLU GEMMs, which this batch (1.8 k tokens) reaches
    with the small-problem GEMM tiles off (MANNER_HIP_GEMM_SMALL_TILES=0: same bits, other tiles)."""
    monkeypatch.setenv("MANNER_HIP_TRAIN_SAVE16", save16)
    monkeypatch.setenv("MANNER_HIP_GEMM_SMALL_TILES", "0")
    cfg = dataclasses.replace(PRESETS["bert-base-uncased"], layers=2)
    w = make_plm_weights(cfg, seed=83, std=0.02, with_pooler=False)
    lens = np.array([2, 96, 129, 256, 257, 400, 512])
    ids_np, mask_np = synth_news_tokens(len(lens), cfg, seed=83, lengths=lens)
    ids, mask = _cuda(ids_np), _cuda(mask_np)
    R = torch.from_numpy(np.random.default_rng(9).standard_normal((len(lens), cfg.hidden)).astype(np.float32)).to(DEV)
    res = {p: _run(cfg, _params(w), ids, mask, R, precision=p, p_hidden=0.0, p_attn=0.0, p_out=0.0) for p in ("fp32", precision)}
    assert bool(_lib.load().manner_hip_train_layout_last() & 2) == (save16 == "1")     # the layout under test really ran
    err = float(np.abs(res[precision][0] - res["fp32"][0]).max())
    assert err < tol
    worst = 1.0
    for k, g in res["fp32"][1].items():
        if np.abs(g).max() < 1e-6 or k.endswith("attention.self.key.bias"):
            continue
        c = _cos(res[precision][1][k], g)
        worst = min(worst, c)
        assert c > cos_min, (k, c)
    measured(output_max_abs_diff=err, worst_gradient_cosine=worst)


# ------------------------------------------------------------------------------------------------ 5. short rows keep their bits
@pytest.mark.parametrize("precision", ["fp32", "f16", "bf16"])
def test_short_rows_keep_their_bits_under_a_long_padded_length(precision):
    """The same rows of <= 128 tokens padded to 128 and to 300 (same token_bound, dropout on): equal outputs and gradients."""
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=84, std=0.05, with_pooler=False)
    lens = np.array([2, 17, 64, 100, 128])
    R = torch.from_numpy(np.random.default_rng(4).standard_normal((len(lens), cfg.hidden)).astype(np.float32)).to(DEV)
    ids128, mask128 = synth_news_tokens(len(lens), cfg, seed=84, lengths=lens, pad_to=128)
    res = []
    for pad in (128, 300):
        ids_np = np.pad(ids128, ((0, 0), (0, pad - 128)), constant_values=cfg.pad_id)
        mask_np = np.pad(mask128, ((0, 0), (0, pad - 128)))
        res.append(_run(cfg, _params(w, {k for k in w if "layer.0." in k}), _cuda(ids_np), _cuda(mask_np), R, precision=precision,
                        p_hidden=0.1, p_attn=0.1, p_out=0.2, seed=21, token_bound=int(lens.sum())))
    assert np.array_equal(res[0][0], res[1][0])
    for k, g in res[0][1].items():
        if g is None:
            assert res[1][1][k] is None
        elif k in ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight"):
            assert _rel(res[1][1][k], g) < 1e-5, k                       # f32 atomics: summation order
        else:
            assert np.array_equal(res[1][1][k], g), k


@pytest.mark.parametrize("precision", ["fp32", "f16", "bf16"])
def test_short_rows_beside_long_rows_give_their_short_batch_outputs(precision, measured):
    """Dropout off: rows of <= 128 tokens in a batch that also holds long rows give their outputs of a short-only batch."""
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=85, std=0.05, with_pooler=False)
    ids_s, mask_s = synth_news_tokens(3, cfg, seed=85, lengths=np.array([3, 50, 128]), pad_to=128)
    ids_l, mask_l = synth_news_tokens(2, cfg, seed=86, lengths=np.array([300, 512]), pad_to=512)
    ids_m = np.concatenate([np.pad(ids_s, ((0, 0), (0, 384)), constant_values=cfg.pad_id), ids_l])
    mask_m = np.concatenate([np.pad(mask_s, ((0, 0), (0, 384))), mask_l])
    outs = []
    for ids_np, mask_np in ((ids_s, mask_s), (ids_m, mask_m)):
        with torch.no_grad():
            out = train.encode_train(cfg, _params(w), _cuda(ids_np), _cuda(mask_np), precision=precision, p_hidden=0.0, p_attn=0.0,
                                     p_out=0.0, max_len=LONG)
        outs.append(out.cpu().numpy()[:3])
    diff = float(np.abs(outs[0] - outs[1]).max())
    measured(short_rows_max_abs_diff=diff)
    assert diff == 0.0, diff


# ------------------------------------------------------------------------------------------------ 6. frozen prefix
def test_long_rows_train_from_cached_frozen_prefix():
    """Embeddings and layer 0 frozen, rows up to 512: the prefix from the inference engine's encode_hidden (long rows there too), same
    outputs and gradients as the full path (the bar of test_train_from_cached_frozen_prefix)."""
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=87, std=0.05, with_pooler=False)
    frozen = {k for k in w if k.startswith("embeddings.") or "layer.0." in k}
    ids_np, mask_np = synth_news_tokens(4, cfg, seed=87, lengths=np.array([20, 129, 300, 512]))
    ids, mask = _cuda(ids_np), _cuda(mask_np)
    R = torch.from_numpy(np.random.default_rng(2).standard_normal((4, cfg.hidden)).astype(np.float32)).to(DEV)
    full = _params(w, frozen)
    out_full, g_full = _run(cfg, full, ids, mask, R, precision="fp32", p_hidden=0.0, p_attn=0.0, p_out=0.0)
    engine = hip.HipEncoder(cfg, w, precisions=("fp32",), device=DEV)
    cached = _params(w, frozen)
    out_c, g_c = _run(cfg, cached, ids, mask, R, precision="fp32", p_hidden=0.0, p_attn=0.0, p_out=0.0, prefix_engine=engine)
    engine.close()
    assert np.abs(out_c - out_full).max() < 5e-5
    for k in w:
        if k in frozen:
            assert g_full[k] is None and g_c[k] is None
        elif not k.endswith("attention.self.key.bias"):
            assert _rel(g_c[k], g_full[k]) < 1e-3, k


# ------------------------------------------------------------------------------------------------ 7. buffers
@pytest.mark.parametrize("token_bound", [False, True])
@pytest.mark.parametrize("prec", ["f16", "bf16", "fp32"])
def test_long_rows_stay_inside_the_declared_buffers(prec, token_bound):
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=88, std=0.05, with_pooler=False)
    lens = np.array([5, 129, 250, 301, 512])
    n = len(lens)
    ids_np, mask_np = synth_news_tokens(n, cfg, seed=88, lengths=lens)
    tokens = int(mask_np.sum())
    assert tokens % 256 != 0
    ids, mask = _cuda(ids_np), _cuda(mask_np)
    lp = ids.shape[1]
    m_bound = ((tokens if token_bound else n * lp) + 255) // 256 * 256
    lib = _lib.load()
    cc = train._cfg_c(cfg)
    names = hip.weight_table_order(cfg)
    weights = [torch.from_numpy(w[k]).to(DEV).contiguous() for k in names]
    grads = [torch.zeros_like(t) if "layer.0." not in k else None for k, t in zip(names, weights)]
    G = 1 << 20
    need_s = int(lib.manner_hip_train_saved_bytes(C.byref(cc), n, m_bound, 0))
    need_w = int(lib.manner_hip_train_workspace_bytes(C.byref(cc), m_bound))
    saved = torch.full((need_s + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.full((need_w + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.empty((n, cfg.hidden), dtype=torch.float32, device=DEV)
    gout = torch.randn((n, cfg.hidden), device=DEV)
    status = hip.device_status(DEV)
    p_s, p_w = C.c_void_p(saved.data_ptr() + G), C.c_void_p(ws.data_ptr() + G)
    precision = _lib.PRECISIONS[prec]
    _lib.check(lib.manner_hip_train_forward(C.byref(cc), train._table(weights), len(weights), hip._ptr(ids), hip._ptr(mask), n, lp, m_bound,
                                            precision, 0, None, C.c_float(0.1), C.c_float(0.1), C.c_float(0.2), C.c_uint64(5), hip._ptr(out),
                                            p_s, need_s, p_w, need_w, hip._ptr(status.word), hip._stream()))
    _lib.check(lib.manner_hip_train_backward(C.byref(cc), train._table(weights), len(weights), hip._ptr(ids), n, lp, m_bound, precision, 0,
                                             C.c_float(0.1), C.c_float(0.1), C.c_float(0.2), C.c_uint64(5), hip._ptr(gout), p_s, need_s,
                                             train._table(grads), None, p_w, need_w, hip._stream()))
    torch.cuda.synchronize()
    hip.check_status(DEV)
    for name, buf in (("saved", saved), ("workspace", ws)):
        assert bool((buf[:G] == 0xA5).all()), f"{name}: bytes in FRONT of the buffer were written"
        assert bool((buf[-G:] == 0xA5).all()), f"{name}: bytes BEHIND the buffer were written"
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(g).all()) for g in grads if g is not None)


# ------------------------------------------------------------------------------------------------ 8. the module mirror's opt-in
def _mirror_enc():
    from manner_amd.models.components.news_encoder import MannerNewsEncoder
    cfg = PRESETS["tiny-bert-512"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = MannerNewsEncoder(plm_model="tiny-bert-512", frozen_layers=[0], dropout_probability=0.2, use_entities=False,
                                entity_embeddings=None, entity_embedding_dim=100, num_attention_heads=10, query_vector_dim=200,
                                text_embedding_dim=cfg.hidden)
    w = make_plm_weights(cfg, seed=89, std=0.05)
    enc.load_state_dict({"text_encoder.plm_model." + k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return enc.to(DEV), cfg


@pytest.mark.parametrize("autocast", [None, torch.float16])
def test_module_mirror_trains_on_long_news_when_opted_in(autocast, monkeypatch):
    from manner_amd.models.components.news_encoder import MannerTextEncoder
    monkeypatch.setattr(MannerTextEncoder, "train_max_length", LONG)
    enc, cfg = _mirror_enc()
    enc.train()
    ids, mask = synth_news_tokens(4, cfg, seed=90, lengths=np.array([10, 129, 250, 300]), pad_to=300)
    news = {"text": {"input_ids": _cuda(ids), "attention_mask": _cuda(mask)}}
    if autocast is None:
        out = enc(news)
    else:
        with torch.autocast("cuda", dtype=autocast):
            out = enc(news)
    out.float().square().sum().backward()
    hip.check_status(DEV)
    named = dict(enc.text_encoder.plm_model.named_parameters())
    for k in ("embeddings.word_embeddings.weight", "encoder.layer.1.attention.self.query.weight", "encoder.layer.1.output.dense.weight"):
        g = named[k].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    assert named["encoder.layer.0.attention.self.query.weight"].grad is None
    # a padded batch beyond the training limit still raises with the opt-in, and a row beyond the position table raises its error
    ids5, mask5 = synth_news_tokens(2, cfg, seed=91, lengths=np.array([5, 40]), pad_to=513)
    with pytest.raises(RuntimeError, match="padded_len"):
        enc({"text": {"input_ids": _cuda(ids5), "attention_mask": _cuda(mask5)}})


def test_long_row_beyond_the_position_table_raises():
    cfg = PRESETS["tiny-roberta"]                        # 130 positions, starting at pad_id + 1 = 2: at most 128 tokens
    w = make_plm_weights(cfg, seed=92, std=0.05, with_pooler=False)
    ids, mask = synth_news_tokens(2, cfg, seed=92, lengths=np.array([10, 200]))
    train.encode_train(cfg, _params(w), _cuda(ids), _cuda(mask), precision="fp32", p_hidden=0.0, p_attn=0.0, p_out=0.0, max_len=LONG)
    with pytest.raises(RuntimeError, match="position|token"):
        hip.check_status(DEV)
