"""The per-slice maps and bars of test_gpu_d32_slices.py (head_dim 32: attention_d32.hip's attn32_16_kernel, attn32_long16_kernel,
attn32_cls_kernel and their f32 forms), on the CPU: the batches, configs and weight sets of the GPU file, the conditions it relies on,
and the proof that its maps see one planted defect per loop, branch or lane group of those kernels.

The model of a kernel with a defect is the float64 restatement (slice_ref.reference) with the defect planted in its attention stage
(the ``attn`` hook; the crossed heads through the weights, d32_common.defect_crossed), rounded at the kernels' storage points; it is
mapped against the same restatement without storage rounding, so the defect stands in the rounding noise a 16-bit kernel has.  The
model of the GPU bar (2 x the same map of the head_dim-64 kernels on the twin config) is 2 x that map of the twin's rounded
restatement; for fp32 it is 8 x the map of the float32 evaluation against float64, as on the GPU.  A defect is SEEN when the map's
maximum is at least CLEAR x the modelled bar or its outlier ratio exceeds FLAG (the GPU bar on the ratio is FLAG / 2), and ``worst``
names a slice the defect was planted in.  DEFECTS lists, per defect, the (config, weight set, batch, map) that see it in every mode."""
import functools
import math

import numpy as np
import pytest
import torch

import d32_common as D
import slice_ref as S
from manner_amd.config import PRESETS
from manner_amd.synth import synth_news_tokens
from manner_amd.weights import make_plm_weights
from side_ops_ref import MEASURED_FACTOR, QUARTER_ULP
from test_gemm_tiles_host import FLAG, QUIET_RATIO

CLEAR = 10.0                         # a planted defect exceeds the modelled bar of its map at least this many times
SEED, STD = 32, 0.1                  # std 0.1 as the head_dim-32 16-bit goldens: at 0.02 the softmax is near uniform and hides score defects
MODES = ("f16", "bf16", "fp32")
SHORT, QBLOCK, CLS_BLOCK = 128, 256, 128      # MANNER_HIP_MAX_LEN; queries per workgroup of attn32_long16_kernel; keys per block of attn32_cls_kernel
CONFIGS = {"tiny-bert-d32": PRESETS["tiny-bert-d32"], "mini-minilm": PRESETS["mini-minilm"], "stress-d32": D.STRESS_CFG}
# odd news counts: N x head pairs is no multiple of the four waves of a 16-bit or [CLS] workgroup
BATCHES = {512: [31, 33, 64, 65, 96, 97, 128, 129, 255, 256, 257, 511, 512],
           385: [2, 7, 8, 9, 32, 127, 136, 137, 160, 383, 385],
           161: [129, 130, 160, 161, 2],
           70: [2, 3, 31, 32, 33, 64, 65, 69, 70]}
# per batch: the key-tile counts of the short kernels' instantiations it reaches, n_qb and rows_cap of the long 16-bit launch
REACHES = {512: dict(nkt={1, 2, 3, 4}, n_qb=2, rows_cap=512), 385: dict(nkt={1, 4}, n_qb=2, rows_cap=416),
           161: dict(nkt={1}, n_qb=1, rows_cap=192), 70: dict(nkt={1, 2, 3}, n_qb=0, rows_cap=0)}
PEAKED_WORDS = 1000 + 37 * np.arange(8)       # the word ids of the peaked batches (synth_news_tokens draws its words from 1000 up)
CASES = ([(c, ws, pad) for c in ("tiny-bert-d32", "mini-minilm") for ws in ("hf", "ident") for pad in BATCHES]
         + [("stress-d32", ws, pad) for ws in ("peaked_first", "peaked_last") for pad in (512, 385)])


# ------------------------------------------------------------------------------------------------ cases
def weights_of(cfg, kind):
    """hf: seeded weights at std 0.1; ident: the same with the attention out-projection the identity in both layers and the last
    layer's FFN output zero (up to LayerNorm's row-wise affine, head h stays in features 32h .. 32h+31 of hidden state 1 and of
    [CLS]); peaked_*: d32_common.stress_weights.  The same construction serves a config and its twin."""
    if kind in D.MARKER_AT:
        return D.stress_weights(kind, cfg=cfg, with_pooler=False)[1]
    w = make_plm_weights(cfg, seed=SEED, std=STD, with_pooler=False)
    if kind == "ident":
        for l in range(cfg.layers):
            w[f"encoder.layer.{l}.attention.output.dense.weight"] = np.eye(cfg.hidden, dtype=np.float32)
            w[f"encoder.layer.{l}.attention.output.dense.bias"] = np.zeros(cfg.hidden, dtype=np.float32)
        w[f"encoder.layer.{cfg.layers - 1}.output.dense.weight"][:] = 0.0
        w[f"encoder.layer.{cfg.layers - 1}.output.dense.bias"][:] = 0.0
    else:
        assert kind == "hf", kind
    return w


@functools.lru_cache(maxsize=None)
def case(config, weights, pad, twin=False):
    """cfg, float32 weights, ids, mask; ``twin``: the head_dim-64 twin on the same seed, std, tokens and construction."""
    cfg = CONFIGS[config]
    assert cfg.head_dim == 32 and cfg.layers == 2 and cfg.vocab == 2048 and cfg.max_pos == 512
    lens = np.array(BATCHES[pad])
    ids, mask = synth_news_tokens(len(lens), cfg, seed=pad, lengths=lens, pad_to=pad)
    if weights in D.MARKER_AT:
        # the last layer of the stress weights is a near one-hot softmax over u.x of the keys: among the ~400 distinct words of a long news
        # the two largest are near ties, and that news' [CLS] is ill-conditioned — the float32 evaluation of the restatement alone then has
        # outlier ratios of 3 .. 11 over the news, whatever the token seed.  Eight distinct words keep the keys apart (ratios <= 1.6 at
        # every seed tried), so the peaked batches draw their words from PEAKED_WORDS; the lengths are those of BATCHES.
        ids = np.where(ids >= 1000, PEAKED_WORDS[ids % len(PEAKED_WORDS)], ids)
        D.place_marker(ids, lens, weights)
    if twin:
        cfg = D.twin_config(cfg)
        assert cfg.head_dim == 64
    return cfg, weights_of(cfg, weights), ids, mask


def cls_head_labels(n, hidden):
    """[N, H]: one slice per head of 32 features over all news."""
    return np.repeat((np.arange(hidden, dtype=np.int64) // 32)[None, :], n, 0)


def numpy_result(r):
    return {"hidden1": r["hidden"][1].cpu().numpy(), "cls": r["cls"].cpu().numpy()}


def maps(cfg, mask, got, ref):
    """The three maps of a case; ``cfg`` is the head_dim-32 config, for the twin's outputs as well (the same labelling)."""
    n = len(mask)
    assert n * 32 >= S.MIN_SLICE and cfg.hidden >= S.MIN_SLICE
    return {"hidden": S.error_map(got["hidden1"], ref["hidden1"], S.token_block_head_labels(mask, cfg.hidden, cfg.heads)),
            "cls": S.error_map(got["cls"], ref["cls"], S.news_labels(n, cfg.hidden)),
            "cls_head": S.error_map(got["cls"], ref["cls"], cls_head_labels(n, cfg.hidden))}


def bar_16bit(twin_max, mode):
    """The bar on a 16-bit map's maximum: 2 x the twin's figure, never above the mode's whole-tensor bar."""
    return min(2.0 * twin_max, ABS_CAP[mode])


def bar_fp32(f32_max):
    """The bar on an fp32 map's maximum: MEASURED_FACTOR x the float32 evaluation's figure, that figure floored at 2^-25."""
    return MEASURED_FACTOR * max(f32_max, QUARTER_ULP)


ABS_CAP = {"f16": 2e-2, "bf16": 0.1}          # test_gpu_gemm_tiles.ABS_CAP (asserted equal in test_gpu_d32_slices.py)


# ------------------------------------------------------------------------------------------------ the attention stage, with defects
def attention(cfg, lens, rnd, defect=None):
    """An ``attn`` hook of slice_ref.reference: the stage as the reference has it, with one defect of DEFECTS planted.  Defects of the
    short and long kernels go into layer 0 (hidden state 1 sees them), those of attn32_cls_kernel into the last layer."""
    d, last = cfg.head_dim, cfg.layers - 1
    L = torch.as_tensor(np.asarray(lens), dtype=torch.long)

    def attn(layer, q, k, v, add_mask):
        n, a, s, _ = q.shape
        pos = torch.arange(s)
        scale = torch.full((a,), d ** -0.5, dtype=q.dtype)
        if defect == "scale":                                    # 1. head 1 of every pair keeps the head_dim-64 constant
            scale[1::2] = 64 ** -0.5
        raw = torch.matmul(q, k.transpose(2, 3))
        if defect == "cls_eight_lanes" and layer == last:        # 10. the dot product summed over the eight lanes of the pair
            raw = raw + raw[:, torch.arange(a) ^ 1]
        logits = raw * (d ** -0.5) + add_mask if defect != "scale" else raw * scale[None, :, None, None] + add_mask
        drop = torch.zeros((n, s), dtype=torch.bool)             # keys left out
        copies = torch.zeros(n, dtype=q.dtype)                   # further copies of key L - 1 that are counted
        if defect == "tile3" and layer == 0:                     # 3. key tile 3 dropped in the NKT = 4 instantiation
            drop = ((L > 96) & (L <= SHORT))[:, None] & (pos >= 96)[None, :]
        if defect == "pad_copies" and layer == 0:                # 4. long rows: keys L .. ceil32(L) - 1 hold key L - 1 and are not masked
            copies = torch.where(L > SHORT, (-L) % 32, 0).to(q.dtype)
        if defect == "cls_block2" and layer == last:             # 8. the second 128-key block is dropped
            drop = ((pos >= CLS_BLOCK) & (pos < 2 * CLS_BLOCK))[None, :].expand(n, s)
        if defect == "cls_group" and layer == last:              # 9. lanes g >= L mod 8 of the last eight-key group hold key L - 1 and count
            copies = ((-L) % 8).to(q.dtype)
        if drop.any():
            logits = logits.masked_fill(drop[:, None, None, :], torch.finfo(torch.float32).min)
        if copies.any():
            bump = torch.zeros((n, s), dtype=q.dtype)
            bump[torch.arange(n), L - 1] = torch.log1p(copies)
            logits = logits + bump[:, None, None, :]
        if defect == "no_rescale" and layer == 0:                # 7. the online softmax over 32-key tiles without o *= alpha
            ctx = _online_softmax(logits, v, rnd, rescale=False)
        else:
            ctx = torch.matmul(rnd(torch.softmax(logits, dim=-1), "probs"), v)
        if layer == 0 and defect in ("wave7_zero", "wave7_copy", "n_qb"):
            long_row = (L > SHORT)[:, None]
            if defect == "n_qb":                                 # 6. one query block only: queries from 256 up are never written
                hit, src = long_row & (pos >= QBLOCK)[None, :], None
            else:                                                # 5. wave 7 of a workgroup: its 32 queries zeroed / given wave 6's output
                hit = long_row & (pos % QBLOCK >= QBLOCK - 32)[None, :]
                src = None if defect == "wave7_zero" else ctx[:, :, torch.clamp(pos - 32, min=0)]
            hit = hit[:, None, :, None]
            ctx = torch.where(hit, torch.zeros_like(ctx) if src is None else src, ctx)
        return ctx
    return attn


def _online_softmax(logits, v, rnd, rescale=True):
    """attn32_wave16 / attn32_long16_kernel's loop over 32-key tiles: running maximum m, sum l and output o; the numerators are rounded
    at the "probs" point, as the kernels feed them to the PV product.  ``rescale=False`` leaves out o *= alpha."""
    n, a, s, _ = logits.shape
    m = torch.full((n, a, s), -math.inf, dtype=logits.dtype)
    l = torch.zeros_like(m)
    o = torch.zeros_like(v)
    for k0 in range(0, s, 32):
        st = logits[..., k0:k0 + 32]
        mn = torch.maximum(m, st.max(-1).values)
        p = torch.exp(st - mn[..., None])
        alpha = torch.exp(m - mn)
        l = l * alpha + p.sum(-1)
        if rescale:
            o = o * alpha[..., None]
        o = o + torch.matmul(rnd(p, "probs"), v[:, :, k0:k0 + 32])
        m = mn
    return o / l[..., None]


DEFECT_NAMES = ("scale", "crossed_layer0", "crossed_last", "tile3", "pad_copies", "wave7_zero", "wave7_copy", "n_qb", "no_rescale",
                "cls_block2", "cls_group", "cls_eight_lanes")


@functools.lru_cache(maxsize=None)
def restated(config, weights, pad, mode, store, twin=False, dtype="float64", defect=None):
    """slice_ref.reference of a case as numpy: ``mode`` None is the unrounded restatement (the fp32 kernels' reference), ``store`` rounds
    at every storage point, ``dtype`` "float32" is the yardstick of the fp32 bar, ``defect`` one of DEFECT_NAMES."""
    cfg, w, ids, mask = case(config, weights, pad, twin)
    points = S.STORE_POINTS if store else ()
    hook = None
    if defect in ("crossed_layer0", "crossed_last"):
        w = D.defect_crossed(cfg, w, layers=[0 if defect == "crossed_layer0" else cfg.layers - 1])
    elif defect is not None:
        hook = attention(cfg, mask.sum(1), S._rounder(mode, points), defect)
    return numpy_result(S.reference(cfg, w, ids, mask, mode=mode, store=points, dtype=getattr(torch, dtype), attn=hook))


def host_maps(config, weights, pad, mode, defect=None, twin=False):
    """The model of a kernel's maps: for a 16-bit mode the rounded restatement against the one without storage rounding, for fp32 the
    float32 evaluation against float64; with ``defect`` planted in the former."""
    cfg, _, _, mask = case(config, weights, pad)
    if mode == "fp32":
        got = restated(config, weights, pad, None, False, twin, "float32", defect)
        ref = restated(config, weights, pad, None, False, twin)
    else:
        got = restated(config, weights, pad, mode, True, twin, "float64", defect)
        ref = restated(config, weights, pad, mode, False, twin)
    return maps(cfg, mask, got, ref)


def host_bar(config, weights, pad, mode, which):
    """The host model of the GPU bar on a map's maximum."""
    if mode == "fp32":
        return bar_fp32(host_maps(config, weights, pad, "fp32")[which]["max"])
    return bar_16bit(host_maps(config, weights, pad, mode, twin=True)[which]["max"], mode)


# ------------------------------------------------------------------------------------------------ where a defect is planted
def planted(config, pad, defect, which):
    """The labels of the slices of map ``which`` that ``defect`` is planted in (before merging)."""
    cfg = CONFIGS[config]
    lens = np.array(BATCHES[pad])
    nb = (pad + 31) // 32
    news = {"tile3": (lens > 96) & (lens <= SHORT), "pad_copies": (lens > SHORT) & (lens % 32 != 0), "wave7_zero": lens > QBLOCK - 32,
            "wave7_copy": lens > QBLOCK - 32, "n_qb": lens > QBLOCK, "no_rescale": lens > 32, "cls_block2": lens > CLS_BLOCK,
            "cls_group": lens % 8 != 0}.get(defect, np.ones(len(lens), dtype=bool))
    heads = range(1, cfg.heads, 2) if defect == "scale" else range(cfg.heads)
    if which == "cls":
        return {int(i) for i in np.nonzero(news)[0]}
    if which == "cls_head":
        return set(heads)
    blocks = {"wave7_zero": lambda b: b % 8 == 7, "wave7_copy": lambda b: b % 8 == 7, "n_qb": lambda b: b >= 8}.get(defect, lambda b: True)
    return {(int(i) * cfg.heads + h) * nb + b for i in np.nonzero(news)[0] for h in heads for b in range((int(lens[i]) + 31) // 32) if blocks(b)}


def names_a_planted_slice(m, labels):
    """``worst`` is the (merged) slice of one of ``labels``."""
    groups = {int(m["labels"][np.searchsorted(m["labels"], lab, "right") - 1]) for lab in labels}
    return m["worst"] in groups


def seen(m, bar):
    """(by the maximum, by the ratio): the two ways a map shows a defect."""
    return m["max"] >= CLEAR * bar, m["ratio"] > FLAG


# per defect: the (config, weight set, batch, map) on which every mode sees it.  The scale and the eight-lane defect touch every
# (news, block) alike, so only the maximum can show them, and ``worst`` can name the head only where heads stay apart (ident).
TINY, MINI, STRESS = "tiny-bert-d32", "mini-minilm", "stress-d32"
DEFECTS = {
    "scale": [(MINI, "ident", 385, "hidden"), (TINY, "ident", 70, "hidden")],
    "crossed_layer0": [(TINY, "ident", 161, "hidden"), (MINI, "hf", 70, "hidden")],
    "crossed_last": [(TINY, "ident", 161, "cls"), (TINY, "ident", 161, "cls_head"), (MINI, "ident", 70, "cls_head")],
    "tile3": [(TINY, "hf", 512, "hidden"), (TINY, "hf", 385, "hidden")],
    "pad_copies": [(TINY, "hf", 385, "hidden")],
    "wave7_zero": [(TINY, "hf", 512, "hidden"), (TINY, "hf", 385, "hidden")],
    "wave7_copy": [(TINY, "hf", 512, "hidden"), (TINY, "hf", 385, "hidden")],
    "n_qb": [(TINY, "hf", 512, "hidden"), (TINY, "hf", 385, "hidden")],
    "no_rescale": [(STRESS, "peaked_last", 512, "hidden"), (STRESS, "peaked_last", 385, "hidden")],
    "cls_block2": [(TINY, "hf", 512, "cls"), (TINY, "hf", 385, "cls")],
    "cls_group": [(TINY, "hf", 385, "cls"), (TINY, "hf", 70, "cls")],
    "cls_eight_lanes": [(TINY, "ident", 161, "cls_head"), (MINI, "ident", 70, "cls_head"), (TINY, "hf", 70, "cls")],
}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    restated.cache_clear()
    case.cache_clear()


# ------------------------------------------------------------------------------------------------ conditions
def test_the_defect_list_is_whole():
    assert set(DEFECTS) == set(DEFECT_NAMES)
    assert all((c, ws, pad) in CASES for where in DEFECTS.values() for c, ws, pad, _ in where)
    assert CLEAR >= 10.0 and FLAG == 12.0 and QUIET_RATIO == 2.0 and MEASURED_FACTOR == 8.0 and QUARTER_ULP == 2.0 ** -25


@pytest.mark.parametrize("pad", list(BATCHES))
def test_batches_reach_what_the_gpu_file_relies_on(pad):
    """Units no multiple of a workgroup's four waves; the instantiations of the short kernels, n_qb and rows_cap of the long 16-bit
    launch (attention_varlen_d32); the edges each batch is there for."""
    lens = np.array(BATCHES[pad])
    assert lens.max() == pad <= 512 and lens.min() >= 2 and len(lens) % 2 == 1
    for name in (TINY, MINI):
        hpairs = CONFIGS[name].heads // 2
        assert (len(lens) * hpairs) % 4 != 0, (name, pad)
    assert CONFIGS[STRESS].heads // 2 == 4                   # the peaked sets: four pairs a news, whole workgroups
    want = REACHES[pad]
    assert {int(-(-min(l, SHORT) // 32)) for l in lens if l <= SHORT} == want["nkt"]
    n_qb = -(-pad // QBLOCK) if pad > SHORT else 0
    rows_cap = -(-pad // 32) * 32 if pad > SHORT else 0
    assert (n_qb, rows_cap) == (want["n_qb"], want["rows_cap"])
    stride_nkt = -(-min(pad, SHORT) // 32)                   # the LDS stride per wave of the short launch
    assert stride_nkt == (3 if pad == 70 else 4)
    if pad == 385:
        assert rows_cap - 385 == 31 and -(-(385 - QBLOCK) // 32) == 5 and -(-(383 - QBLOCK) // 32) == 4   # 31 masked keys; a part-filled second block
        assert {l % 8 for l in lens} >= {0, 1, 7} and {136, 137} <= set(lens)          # the eight-key and 128-key edges of [CLS]
    if pad == 161:
        assert 129 in lens and all(32 * w >= 129 for w in (5, 6, 7)) and 32 * 4 < 129   # waves 5 .. 7 idle at L = 129
    if pad == 512:
        assert {97, 128, 257} <= set(lens) and (lens > QBLOCK).sum() == 3                # 257: a second block of one wave, one query


def test_existing_callers_of_the_reference_keep_their_bits():
    """The hook without a defect is the reference's own stage, bit for bit, in both evaluations; the online form agrees with it."""
    cfg, w, ids, mask = case(TINY, "hf", 161)
    for mode, store, dtype in (("bf16", S.STORE_POINTS, torch.float64), (None, (), torch.float32)):
        plain = S.reference(cfg, w, ids, mask, mode=mode, store=store, dtype=dtype)
        hooked = S.reference(cfg, w, ids, mask, mode=mode, store=store, dtype=dtype,
                             attn=attention(cfg, mask.sum(1), S._rounder(mode, store)))
        assert all(torch.equal(a, b) for a, b in zip(plain["hidden"], hooked["hidden"])) and torch.equal(plain["cls"], hooked["cls"])
    q, k, v = (torch.from_numpy(np.random.default_rng(i).standard_normal((2, 4, 70, 32))) for i in range(3))
    logits = torch.matmul(q, k.transpose(2, 3))
    ident = lambda t, point: t   # noqa: E731
    assert torch.allclose(_online_softmax(logits, v, ident), torch.matmul(torch.softmax(logits, -1), v), rtol=1e-12, atol=1e-14)


# ------------------------------------------------------------------------------------------------ quiet maps
@pytest.mark.parametrize("config,weights,pad", CASES)
def test_maps_are_quiet_without_a_defect(config, weights, pad):
    """Every map of every case: the rounded restatement stays under QUIET_RATIO (the per-head [CLS] map included: on ident it is the
    map the GPU file asserts), and under the modelled bar; the float32 figure of every fp32 map is at least 2^-25."""
    for mode in ("f16", "bf16"):
        for which, m in host_maps(config, weights, pad, mode).items():
            assert m["ratio"] < QUIET_RATIO, (mode, which, m)
            assert m["max"] < host_bar(config, weights, pad, mode, which), (mode, which, m)
    for which, m in host_maps(config, weights, pad, "fp32").items():
        assert m["max"] >= QUARTER_ULP and m["ratio"] < QUIET_RATIO, (which, m)


# ------------------------------------------------------------------------------------------------ the defects
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("defect", DEFECT_NAMES)
def test_a_planted_defect_is_seen_and_named(defect, mode):
    """Map maximum / modelled bar in bf16, the mode that sees least (f16 about 8 x these, fp32 about 1000 x), first case of DEFECTS:
    scale 17 (hidden, ident), crossed 226 (hidden, layer 0) / 177 (cls) and 214 (cls per head, last layer), tile3 18 with ratio 43,
    pad_copies 42 with ratio 29, wave7 zeroed 208 / copied 34 with ratios 479 / 77, n_qb 207 with ratio 470, no_rescale 471,
    cls_block2 16 with ratio 29 (pad 385: 7.3, seen by its ratio of 14), cls_group 32 with ratio 62, cls_eight_lanes 27 (cls per head)."""
    for config, weights, pad, which in DEFECTS[defect]:
        m = host_maps(config, weights, pad, mode, defect)[which]
        bar = host_bar(config, weights, pad, mode, which)
        by_max, by_ratio = seen(m, bar)
        print(f"{defect} {mode} {config} {weights} pad {pad}, map {which}: max {m['max']:.3e} = {m['max'] / bar:.1f} x bar {bar:.3e}, "
              f"ratio {m['ratio']:.1f}, worst {m['worst']}: seen by {'max' if by_max else ''} {'ratio' if by_ratio else ''}")
        assert by_max or by_ratio, (config, weights, pad, which, m, bar)
        assert names_a_planted_slice(m, planted(config, pad, defect, which)), (config, weights, pad, which, m)
        hit = planted(config, pad, defect, which)
        if which == "hidden" and len(hit) < len(m["rms"]) // 2:          # confined to few slices: the ratio alone must show it
            assert by_ratio, (config, weights, pad, m)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pad", [512, 385])
def test_the_missing_rescale_is_harmless_where_the_maximum_never_moves(pad, mode):
    """peaked_first: the marker sits in key tile 0, alpha is 1 in every later tile and the defect changes nothing — that set forces the
    other outcome of the kernels' ``__any(mn > m)`` branch, and only peaked_last can see the rescale missing."""
    for which, m in host_maps(STRESS, "peaked_first", pad, mode, "no_rescale").items():
        bar = host_bar(STRESS, "peaked_first", pad, mode, which)
        assert m["max"] < bar and m["ratio"] < FLAG / 2, (which, m, bar)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("defect", ["crossed_last", "cls_eight_lanes"])
def test_the_per_head_cls_map_on_ident_flags_the_pair_defects(defect, mode):
    for config, pad in ((TINY, 161), (MINI, 70), (TINY, 512)):
        quiet = host_maps(config, "ident", pad, mode)["cls_head"]
        bar = host_bar(config, "ident", pad, mode, "cls_head")
        m = host_maps(config, "ident", pad, mode, defect)["cls_head"]
        assert quiet["max"] < bar and quiet["ratio"] < QUIET_RATIO, (quiet, bar)
        assert m["max"] >= CLEAR * bar, (config, pad, m, bar)


