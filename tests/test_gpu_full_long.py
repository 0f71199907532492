"""PLMTextEncoder's "full rows" (every padded position a row of the PLM, the real tokens its attention keys) on padded batches of
129..512 positions (MANNER_HIP_MAX_LEN_FULL): hip.encode_full, train.encode_full_train and the module mirror against the
reference's own PLMTextEncoder (tests/golden/train_plm_long.npz), the long-row matrix-pipe attention with a key count per news
(train_attn.hip, KEYS) against the VALU kernels' row-block form and against fp32, the zeros it owes the rows that are no keys, the
declared buffers, and batches of <= 128 positions keeping their bits.  Run on the MI355X box: ``pytest -m gpu``."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from manner_amd import _lib, hip, train  # noqa: E402
from manner_amd.config import PRESETS  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from manner_amd.weights import make_mha_pool_weights, make_plm_weights  # noqa: E402
from test_long_train_host import KEY_BIAS_ABS  # noqa: E402

DEV = "cuda:0"
FULL = _lib.MAX_LEN_FULL
# the bars of test_long_matrix_pipe_attention_tracks_the_valu_kernels (matrix pipe against VALU: relative error, cosine) and of
# test_long_rows_16bit_modes_track_fp32 (a 16-bit mode against fp32: LayerNorm outputs max-abs, gradient cosine)
PIPE_BAR = {"f16": (2e-2, 0.9999), "bf16": (8e-2, 0.999)}
FP32_BAR = {"f16": (2e-2, 0.999), "bf16": (1e-1, 0.99)}


def _cuda(a):
    return torch.from_numpy(a).to(DEV)


def _rel(a, b, floor=1e-3):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


def _cos(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


def _params(w):
    return {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in w.items()}


def _grads(params):
    return {k: p.grad.cpu().numpy() for k, p in params.items()}


def _tokens(cfg, lens, lp, seed):
    """ids / mask [n, lp] with `lens` real tokens a news (1 allowed: the [CLS] alone)."""
    lens = np.asarray(lens)
    ids, mask = synth_news_tokens(len(lens), cfg, seed=seed, lengths=np.maximum(lens, 2), pad_to=lp)
    one = lens == 1
    ids[one, 1], mask[one, 1] = cfg.pad_id, 0
    return ids, mask


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "train_plm_long.npz"))
    return z, json.loads(str(z["meta"]))


def _mirror(preset, heads, query_dim, w, mw, frozen_layers, p=0.0):
    from manner_amd.models.components.news_encoder import PLMTextEncoder
    cfg = PRESETS[preset]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = PLMTextEncoder(plm_model=preset, frozen_layers=frozen_layers, text_embedding_dim=cfg.hidden, num_attention_heads=heads,
                             query_vector_dim=query_dim, dropout_probability=p)
    sd = {"plm_model." + k: torch.from_numpy(v) for k, v in w.items()}
    sd.update({k: torch.from_numpy(v) for k, v in mw.items()})
    enc.load_state_dict(sd, strict=True)
    return enc.to(DEV)


# ------------------------------------------------------------------------------------------------ 1. reference parity, fp32
@pytest.mark.parametrize("case", ["p300", "p512"])
@pytest.mark.parametrize("tag", ["bert", "roberta"])
def test_plm_text_encoder_trains_on_long_news_like_the_reference(golden, tag, case, monkeypatch):
    """train() on padded batches of 300 (1 .. 300 real tokens) and 512 positions: the pooled output within 1e-4 and every gradient
    within the relative 2e-3 of test_plm_text_encoder_training_matches_reference; the key bias analytically zero; the pad token's
    embedding row without gradient."""
    from manner_amd.models.components.news_encoder import PLMTextEncoder
    z, meta = golden
    monkeypatch.setattr(PLMTextEncoder, "train_max_length", FULL)
    preset, heads = meta["plm"][tag]
    cfg = PRESETS[preset]
    w = make_plm_weights(cfg, seed=meta["seed"], std=meta["std"])
    mw = make_mha_pool_weights(cfg.hidden, meta["query_dim"], seed=meta["seed"])
    enc = _mirror(preset, heads, meta["query_dim"], w, mw, meta["frozen_layers"]).train()
    enc.plm_model.hidden_dropout_prob = enc.plm_model.attention_probs_dropout_prob = 0.0
    key = f"{tag}_{case}"
    assert z[f"{key}_ids"].shape[1] == meta["cases"][case]["padded_len"] > _lib.MAX_LEN
    out = enc({"input_ids": _cuda(z[f"{key}_ids"]), "attention_mask": _cuda(z[f"{key}_mask"])})
    (out * _cuda(z[f"{key}_R"])).sum().backward()
    hip.check_status(DEV)
    err = float((out.detach().cpu() - torch.from_numpy(z[f"{key}_out"])).abs().max())
    print(f"{key}: output max-abs error {err:.3e}")
    assert err < 1e-4
    frozen = set(z[f"{key}_frozen"].tolist())
    checked = 0
    for k, p in enc.named_parameters():
        if k.startswith("plm_model.pooler."):
            continue
        if k in frozen:
            assert p.grad is None, k
            continue
        want = z[f"{key}_grad:{k}"]
        got = p.grad.cpu().numpy()
        if got.shape != want.shape:
            got = got[np.r_[0:8, 8:got.shape[0]:37]]
        if k.endswith("attention.self.key.bias"):           # analytically zero (softmax is shift-invariant)
            print(f"{key}: {k} max-abs {np.abs(got).max():.3e} (reference {np.abs(want).max():.3e})")
            assert np.abs(got).max() < KEY_BIAS_ABS and np.abs(want).max() < KEY_BIAS_ABS
            continue
        r = _rel(got, want)
        print(f"{key}: d {k}: relative max error {r:.3e}")
        assert r < 2e-3, (key, k, r)
        checked += 1
    assert checked >= 25
    pad_row = enc.plm_model.embeddings.word_embeddings.weight.grad[cfg.pad_id]
    assert float(pad_row.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. inference
@pytest.mark.parametrize("lp", [129, 300, 512])
@pytest.mark.parametrize("tag", ["bert", "roberta"])
def test_encode_full_gives_the_reference_hidden_states_beyond_128_positions(golden, tag, lp, measured):
    """hip.encode_full in fp32 against HF's last_hidden_state as the reference's PLMTextEncoder saw it (a sample of positions, padded
    ones included) within 1e-4; f16 / bf16 (the long-row matrix-pipe forward) against the fp32 result.  129 positions: the news of
    <= 129 real tokens of the 300-wide batch cut to 129 columns — a position's state depends on itself and on the real tokens only."""
    z, meta = golden
    cfg = PRESETS[meta["plm"][tag][0]]
    w = {k: _cuda(v) for k, v in make_plm_weights(cfg, seed=meta["seed"], std=meta["std"]).items() if not k.startswith("pooler.")}
    key = f"{tag}_{'p512' if lp == 512 else 'p300'}"
    ids, mask = z[f"{key}_ids"], z[f"{key}_mask"]
    hs_n, hs_t, hs = z[f"{key}_hs_news"], z[f"{key}_hs_pos"], z[f"{key}_hs"]
    if lp < ids.shape[1]:
        rows = np.nonzero(mask.sum(1) <= lp)[0]
        assert len(rows) == 5 and mask[rows].sum(1).max() == lp
        ids, mask = np.ascontiguousarray(ids[rows, :lp]), np.ascontiguousarray(mask[rows, :lp])
        sel = np.isin(hs_n, rows) & (hs_t < lp)
        hs_n, hs_t, hs = np.searchsorted(rows, hs_n[sel]), hs_t[sel], hs[sel]
    assert ids.shape[1] == lp and (hs_t >= mask.sum(1)[hs_n]).any()          # padded positions are among the sample
    out = {p: hip.encode_full(cfg, w, _cuda(ids), _cuda(mask), precision=p).cpu().numpy() for p in ("fp32", "f16", "bf16")}
    hip.check_status(DEV)
    err = float(np.abs(out["fp32"][hs_n, hs_t] - hs).max())
    errs = {p: float(np.abs(out[p] - out["fp32"]).max()) for p in ("f16", "bf16")}
    print(f"{key} lp={lp}: fp32 vs reference {err:.3e}, f16 vs fp32 {errs['f16']:.3e}, bf16 vs fp32 {errs['bf16']:.3e}")
    measured(fp32_vs_reference=err, f16_vs_fp32=errs["f16"], bf16_vs_fp32=errs["bf16"], bound_f16=FP32_BAR["f16"][0],
             bound_bf16=FP32_BAR["bf16"][0])
    assert err < 1e-4
    for p in ("f16", "bf16"):
        assert np.isfinite(out[p]).all() and errs[p] < FP32_BAR[p][0], (p, errs[p])


# ------------------------------------------------------------------------------------------------ 3. matrix pipe against VALU
def _full_train(cfg, w, ids, mask, R, monkeypatch, valu, **kw):
    if valu:
        monkeypatch.setenv("MANNER_HIP_TRAIN_ATTN_VALU", "1")
    else:
        monkeypatch.delenv("MANNER_HIP_TRAIN_ATTN_VALU", raising=False)
    params = _params(w)
    out = train.encode_full_train(cfg, params, ids, mask, max_len=FULL, **kw)
    layout = int(_lib.load().manner_hip_train_layout_last())
    (out * R).sum().backward()
    monkeypatch.delenv("MANNER_HIP_TRAIN_ATTN_VALU", raising=False)
    return out.detach().cpu().numpy(), _grads(params), layout


def _hold_grads(ga, gb, rel, cos_min, tag):
    """Every gradient of run a against run b: relative to the tensor's largest entry, and by cosine; the (analytically zero) key bias
    against the query bias' scale, as test_long_matrix_pipe_attention_tracks_the_valu_kernels does."""
    worst = (0.0, 1.0, None)
    for k, g in gb.items():
        x, y = ga[k].astype(np.float64).ravel(), g.astype(np.float64).ravel()
        assert np.isfinite(x).all() and np.isfinite(y).all(), (tag, k)
        if k.endswith("attention.self.key.bias"):
            qs = np.abs(gb[k.replace("key.bias", "query.bias")]).max()
            assert np.abs(x).max() <= 2e-2 * qs and np.abs(y).max() <= 2e-2 * qs, (tag, k, np.abs(x).max(), np.abs(y).max(), qs)
            continue
        e = np.abs(x - y).max() / max(np.abs(y).max(), 1e-12)
        c = _cos(x, y)
        if e > worst[0]:
            worst = (e, c, k)
        print(f"{tag}: d {k}: relative-to-max {e:.3e}, cosine {c:.6f}")
        assert e <= rel and c >= cos_min, (tag, k, e, c)
    return worst


@pytest.mark.parametrize("p_attn", [0.0, 0.1])
@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_full_rows_matrix_pipe_attention_tracks_the_valu_kernels(precision, p_attn, monkeypatch, measured):
    """encode_full_train at 300 positions, forward and backward, as shipped (the long-row kernels with key counts) and under
    MANNER_HIP_TRAIN_ATTN_VALU=1 (the f32 kernels' row-block grid): same weights, inputs and seed, so with p_attn = 0.1 the same
    keep-bits.  Key counts on both sides of a 32-key tile, of 128, and the whole row."""
    rel, cos_min = PIPE_BAR[precision]
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=93, std=0.05, with_pooler=False)
    ids_np, mask_np = _tokens(cfg, [3, 31, 33, 128, 129, 300], 300, seed=93)
    ids, mask = _cuda(ids_np), _cuda(mask_np)
    R = torch.from_numpy(np.random.default_rng(93).standard_normal((6, 300, cfg.hidden)).astype(np.float32)).to(DEV)
    kw = dict(precision=precision, p_hidden=0.0, p_attn=p_attn, seed=17)
    out_v, g_v, lay_v = _full_train(cfg, w, ids, mask, R, monkeypatch, True, **kw)
    out_m, g_m, lay_m = _full_train(cfg, w, ids, mask, R, monkeypatch, False, **kw)
    hip.check_status(DEV)
    assert lay_m & 1 and not lay_v & 1                       # the layout word follows the path that ran
    a, b = out_m.astype(np.float64), out_v.astype(np.float64)
    oerr = float(np.abs(a - b).max())
    print(f"{precision} p_attn={p_attn}: output max-abs diff {oerr:.3e} at scale {np.abs(b).max():.3e}")
    assert np.isfinite(a).all() and oerr <= rel * np.abs(b).max()
    worst = _hold_grads(g_m, g_v, rel, cos_min, f"{precision} p_attn={p_attn}")
    measured(bound_rel=rel, bound_cos=cos_min, worst_rel_to_max=worst[0], cosine_of_that_tensor=worst[1], tensor=str(worst[2]),
             output_max_abs_diff=oerr, output_scale=float(np.abs(b).max()))


# ------------------------------------------------------------------------------------------------ 4. zeros past the key count
def _c_full_step(cfg, weights, ids, mask, prec, monkeypatch, valu, fill, margin=0, p_attn=0.0, gout=None):
    """manner_hip_train_full_forward + _backward on buffers filled with `fill` bytes (+ `margin` canary bytes on either side)."""
    if valu:
        monkeypatch.setenv("MANNER_HIP_TRAIN_ATTN_VALU", "1")
    else:
        monkeypatch.delenv("MANNER_HIP_TRAIN_ATTN_VALU", raising=False)
    lib = _lib.load()
    cc = train._cfg_c(cfg)
    n, lp = ids.shape
    m_bound = (n * lp + 255) // 256 * 256
    need_s = int(lib.manner_hip_train_saved_bytes(C.byref(cc), n, m_bound, 0))
    need_w = int(lib.manner_hip_train_workspace_bytes(C.byref(cc), m_bound))
    saved = torch.full((need_s + 2 * margin,), fill, dtype=torch.uint8, device=DEV)
    ws = torch.full((need_w + 2 * margin,), fill, dtype=torch.uint8, device=DEV)
    hid_bytes = n * lp * cfg.hidden * 4
    hidden = torch.full((hid_bytes + 2 * margin,), fill, dtype=torch.uint8, device=DEV)
    grads = [torch.zeros_like(t) for t in weights]
    if gout is None:
        gout = torch.randn((n, lp, cfg.hidden), device=DEV)
    status = hip.device_status(DEV)
    p_s, p_w, p_h = (C.c_void_p(t.data_ptr() + margin) for t in (saved, ws, hidden))
    precision = _lib.PRECISIONS[prec]
    _lib.check(lib.manner_hip_train_full_forward(C.byref(cc), train._table(weights), len(weights), hip._ptr(ids), hip._ptr(mask), n, lp,
                                                 precision, C.c_float(0.0), C.c_float(p_attn), C.c_uint64(5), p_h, p_s, need_s, p_w, need_w,
                                                 hip._ptr(status.word), hip._stream()))
    layout = int(lib.manner_hip_train_layout_last())
    _lib.check(lib.manner_hip_train_layout_next(layout))
    _lib.check(lib.manner_hip_train_full_backward(C.byref(cc), train._table(weights), len(weights), hip._ptr(ids), n, lp, precision,
                                                  C.c_float(0.0), C.c_float(p_attn), C.c_uint64(5), hip._ptr(gout), p_s, need_s,
                                                  train._table(grads), p_w, need_w, hip._stream()))
    torch.cuda.synchronize()
    monkeypatch.delenv("MANNER_HIP_TRAIN_ATTN_VALU", raising=False)
    hip.check_status(DEV)
    out = hidden[margin:margin + hid_bytes].view(torch.float32).view(n, lp, cfg.hidden)
    return out, grads, layout, (saved, ws, hidden)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_rows_past_the_key_count_get_zero_key_and_value_gradients(precision, monkeypatch, measured):
    """One news of 5 real tokens at 300 positions (its key blocks 1 and 2 lie wholly past the key count, inside the row) beside one of
    200: the C entry points on `saved` / `workspace` filled with NaN bytes.  d qkv is read whole by the data-gradient and
    weight-gradient GEMMs, so a key block whose d k / d v store is skipped leaves NaN in every parameter gradient below it."""
    rel, cos_min = PIPE_BAR[precision]
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=94, std=0.05, with_pooler=False)
    names = hip.weight_table_order(cfg)
    weights = [torch.from_numpy(w[k]).to(DEV).contiguous() for k in names]
    ids_np, mask_np = _tokens(cfg, [5, 200], 300, seed=94)
    ids, mask = _cuda(ids_np), _cuda(mask_np)
    gout = torch.from_numpy(np.random.default_rng(94).standard_normal((2, 300, cfg.hidden)).astype(np.float32)).to(DEV)
    out_v, g_v, lay_v, _ = _c_full_step(cfg, weights, ids, mask, precision, monkeypatch, True, 0xFF, p_attn=0.1, gout=gout)
    out_m, g_m, lay_m, _ = _c_full_step(cfg, weights, ids, mask, precision, monkeypatch, False, 0xFF, p_attn=0.1, gout=gout)
    assert lay_m & 1 and not lay_v & 1
    assert bool(torch.isfinite(out_m).all()) and all(bool(torch.isfinite(g).all()) for g in g_m)
    worst = _hold_grads({k: g.cpu().numpy() for k, g in zip(names, g_m)}, {k: g.cpu().numpy() for k, g in zip(names, g_v)}, rel, cos_min,
                        precision)
    measured(bound_rel=rel, bound_cos=cos_min, worst_rel_to_max=worst[0], cosine_of_that_tensor=worst[1], tensor=str(worst[2]))


# ------------------------------------------------------------------------------------------------ 5. tile edges in one batch
def test_key_counts_on_every_tile_edge_in_one_batch(monkeypatch, measured):
    """Key counts 31 .. 512 around every 32-key tile edge class, the 128-key short-row limit, the 256-key half and the row's end, at
    512 positions (H = 128, 2 heads, 2 layers): f16 on the matrix pipe held PER NEWS against the VALU kernels and against fp32."""
    keys = [31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512]
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=95, std=0.05, with_pooler=False)
    ids_np, mask_np = _tokens(cfg, keys, 512, seed=95)
    ids, mask = _cuda(ids_np), _cuda(mask_np)
    R = torch.from_numpy(np.random.default_rng(95).standard_normal((len(keys), 512, cfg.hidden)).astype(np.float32)).to(DEV)
    kw = dict(p_hidden=0.0, p_attn=0.0, seed=3)
    out_m, g_m, lay_m = _full_train(cfg, w, ids, mask, R, monkeypatch, False, precision="f16", **kw)
    out_v, g_v, lay_v = _full_train(cfg, w, ids, mask, R, monkeypatch, True, precision="f16", **kw)
    out_f, g_f, _ = _full_train(cfg, w, ids, mask, R, monkeypatch, False, precision="fp32", **kw)
    hip.check_status(DEV)
    assert lay_m & 1 and not lay_v & 1
    rel, cos_min = PIPE_BAR["f16"]
    tol, cos32 = FP32_BAR["f16"]
    rec = {}
    for i, k in enumerate(keys):
        a, b, f = out_m[i].astype(np.float64), out_v[i].astype(np.float64), out_f[i].astype(np.float64)
        ev, ef = float(np.abs(a - b).max() / np.abs(b).max()), float(np.abs(a - f).max())
        print(f"{k} keys: matrix pipe vs VALU {ev:.3e} of the largest entry, vs fp32 max-abs {ef:.3e}")
        rec[f"keys{k}_vs_valu"], rec[f"keys{k}_vs_fp32"] = ev, ef
        assert np.isfinite(a).all() and ev <= rel and ef < tol, (k, ev, ef)
    _hold_grads(g_m, g_v, rel, cos_min, "f16 vs VALU")
    for k, g in g_f.items():
        if np.abs(g).max() < 1e-6 or k.endswith("attention.self.key.bias"):
            continue
        c = _cos(g_m[k], g)
        assert c > cos32, (k, c)
    measured(bound_rel=rel, bound_fp32=tol, **rec)


# ------------------------------------------------------------------------------------------------ 6. buffers
@pytest.mark.parametrize("lp,lens", [(129, [5, 100, 129]), (512, [5, 257, 512])])
@pytest.mark.parametrize("prec", ["fp32", "f16", "bf16"])
def test_full_rows_stay_inside_the_declared_buffers(prec, lp, lens, monkeypatch):
    """`saved`, `workspace` and `hidden` with canary margins, training step and inference call: the margins stay untouched."""
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=96, std=0.05, with_pooler=False)
    weights = [torch.from_numpy(w[k]).to(DEV).contiguous() for k in hip.weight_table_order(cfg)]
    ids_np, mask_np = _tokens(cfg, lens, lp, seed=96)
    ids, mask = _cuda(ids_np), _cuda(mask_np)
    G = 1 << 20
    out, grads, _, bufs = _c_full_step(cfg, weights, ids, mask, prec, monkeypatch, False, 0xA5, margin=G, p_attn=0.1)
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(g).all()) for g in grads)
    lib = _lib.load()
    cc = train._cfg_c(cfg)
    n = len(lens)
    need = int(lib.manner_hip_encode_full_workspace_bytes(C.byref(cc), n, lp))
    ws = torch.full((need + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    hid_bytes = n * lp * cfg.hidden * 4
    hidden = torch.full((hid_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(lib.manner_hip_encode_full(C.byref(cc), train._table(weights), len(weights), hip._ptr(ids), hip._ptr(mask), n, lp,
                                          _lib.PRECISIONS[prec], C.c_void_p(hidden.data_ptr() + G), C.c_void_p(ws.data_ptr() + G), need,
                                          hip._ptr(hip.device_status(DEV).word), hip._stream()))
    torch.cuda.synchronize()
    hip.check_status(DEV)
    assert bool(torch.isfinite(hidden[G:G + hid_bytes].view(torch.float32)).all())
    for name, buf in (("saved", bufs[0]), ("workspace", bufs[1]), ("hidden", bufs[2]), ("inference workspace", ws), ("inference hidden", hidden)):
        assert bool((buf[:G] == 0xA5).all()), f"{name}: bytes in FRONT of the buffer were written"
        assert bool((buf[-G:] == 0xA5).all()), f"{name}: bytes BEHIND the buffer were written"


# ------------------------------------------------------------------------------------------------ 7. short batches keep their bits
@pytest.mark.parametrize("train_precision", ["fp32", "f16"])
def test_short_full_row_batches_keep_their_bits_under_the_opt_in(train_precision, monkeypatch):
    """96 positions, dropout on, one torch seed: equal outputs and gradients with and without train_max_length = 512 — the opt-in
    changes what is accepted, not what is computed."""
    from manner_amd.models.components.news_encoder import PLMTextEncoder
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=97, std=0.05)
    mw = make_mha_pool_weights(cfg.hidden, 200, seed=97)
    ids_np, mask_np = _tokens(cfg, [1, 20, 64, 96], 96, seed=97)
    batch = {"input_ids": _cuda(ids_np), "attention_mask": _cuda(mask_np)}
    res = []
    for limit in (_lib.MAX_LEN, FULL):
        monkeypatch.setattr(PLMTextEncoder, "train_max_length", limit)
        enc = _mirror("tiny-bert-512", 4, 200, w, mw, [0], p=0.2).train()
        enc.train_precision = train_precision
        torch.manual_seed(5)
        out = enc(batch)
        out.square().sum().backward()
        res.append((out.detach(), {k: p.grad for k, p in enc.named_parameters() if p.grad is not None}))
    hip.check_status(DEV)
    assert torch.equal(res[0][0], res[1][0]) and res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 20
    for k, g in res[0][1].items():
        if k.endswith(("word_embeddings.weight", "position_embeddings.weight", "additive_attention.query")):
            assert _rel(res[1][1][k].cpu().numpy(), g.cpu().numpy()) < 1e-5, k          # f32 atomics: summation order
        else:
            assert torch.equal(res[1][1][k], g), k


# ------------------------------------------------------------------------------------------------ 8. the module mirror
def test_module_mirror_takes_long_news_behind_the_opt_in(monkeypatch):
    from manner_amd.models.components.news_encoder import PLMTextEncoder
    cfg = PRESETS["tiny-bert-512"]
    w = make_plm_weights(cfg, seed=98, std=0.05)
    mw = make_mha_pool_weights(cfg.hidden, 200, seed=98)
    enc = _mirror("tiny-bert-512", 4, 200, w, mw, [0], p=0.2)
    ids_np, mask_np = _tokens(cfg, [1, 40, 129, 200], 200, seed=98)
    batch = {"input_ids": _cuda(ids_np), "attention_mask": _cuda(mask_np)}
    # without the opt-in train() refuses, naming the attribute
    monkeypatch.setattr(PLMTextEncoder, "train_max_length", _lib.MAX_LEN)
    enc.train()
    with pytest.raises(RuntimeError, match="train_max_length"):
        enc(batch)
    # with it, under fp16 autocast: finite loss and gradients, reproducible under one torch seed, different under another
    monkeypatch.setattr(PLMTextEncoder, "train_max_length", FULL)
    outs = []
    for seed in (3, 3, 4):
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(seed)
        with torch.autocast("cuda", dtype=torch.float16):
            out = enc(batch)
        loss = out.float().square().sum()
        loss.backward()
        assert bool(torch.isfinite(loss))
        named = dict(enc.plm_model.named_parameters())
        for k in ("embeddings.word_embeddings.weight", "encoder.layer.1.attention.self.query.weight", "encoder.layer.1.output.dense.weight"):
            g = named[k].grad
            assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
        assert named["encoder.layer.0.attention.self.query.weight"].grad is None
        assert bool(torch.isfinite(enc.multihead_attention.in_proj_weight.grad).all())
        outs.append(out.detach().float())
    assert int(_lib.load().manner_hip_train_layout_last()) & 1      # fp16 autocast at 200 positions: the matrix pipe ran
    assert torch.equal(outs[0], outs[1]) and float((outs[0] - outs[2]).abs().max()) > 1e-3
    # a batch beyond 512 positions raises, opt-in or not
    ids5, mask5 = _tokens(cfg, [5, 40], 513, seed=99)
    wide = {"input_ids": _cuda(ids5), "attention_mask": _cuda(mask5)}
    with pytest.raises(RuntimeError, match="padded_len"):
        enc(wide)
    # eval() under no_grad: 512 positions without the opt-in
    monkeypatch.setattr(PLMTextEncoder, "train_max_length", _lib.MAX_LEN)
    enc.eval()
    ids_e, mask_e = _tokens(cfg, [1, 300, 512], 512, seed=100)
    with torch.no_grad():
        out = enc({"input_ids": _cuda(ids_e), "attention_mask": _cuda(mask_e)})
        assert out.shape == (3, cfg.hidden) and bool(torch.isfinite(out).all())
        with pytest.raises(RuntimeError, match="padded_len"):
            enc(wide)
    hip.check_status(DEV)


def test_full_row_beyond_the_position_table_raises():
    """tiny-roberta has 130 positions starting at pad_id + 1 = 2: a news of 200 real tokens indexes past the table — the position-index
    error of the other entry points, through the status word."""
    cfg = PRESETS["tiny-roberta"]
    w = {k: _cuda(v) for k, v in make_plm_weights(cfg, seed=92, std=0.05, with_pooler=False).items()}
    ids, mask = synth_news_tokens(2, cfg, seed=92, lengths=np.array([10, 200]))
    hip.encode_full(cfg, w, _cuda(ids), _cuda(mask), precision="fp32")
    with pytest.raises(RuntimeError, match="position|token"):
        hip.check_status(DEV)
    train.encode_full_train(cfg, {k: v.requires_grad_(True) for k, v in w.items()}, _cuda(ids), _cuda(mask), precision="fp32", p_hidden=0.0,
                            p_attn=0.0, max_len=FULL)
    with pytest.raises(RuntimeError, match="position|token"):
        hip.check_status(DEV)
