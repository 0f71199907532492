"""The three batches of test_gpu_train_scale.py (the training step held to float64 past 4096 token rows and 8192 padded positions),
their conditions, their maps and the bar of the fp32 subjects, on the CPU at H = 128 (tiny-bert-512, tiny-roberta-514) with the row
counts of the GPU test:

  P  76 news padded to 128, 8 229 packed rows = 2 x 4096 + 37 (ln_bwd_kernel walks 1024 workgroups x 4 waves, one row a wave: two
     full trips of its row loop and a third that reaches ten workgroups and leaves the tenth with one wave), 9 728 padded positions
     (> EMBED_ORDERED_MAX = 8192: embed_bwd_kernel, the atomic scatter), one word id per (news, position);
  R  the same lengths with the word ids drawn from 300 values: every table row sums ~27 tokens;
  F  full rows, 85 news at 97 positions = 8 245 rows, 1 .. 97 real tokens: the padded positions are rows too.

The bar of an fp32 kernel is MEASURED_FACTOR (8) x the same map of the float32 evaluation of the restatement (slice_ref.reference with
dtype=torch.float32) against its float64 evaluation, the figure at least QUARTER_ULP (side_ops_ref: below it the figure is the luck of
one rounding; the objective's weights R are redrawn then).  This file shows that the figure is settled on every map, and that one
defect per loop or branch the new shapes reach, planted into the float64 restatement, exceeds the bar of the map that should see it
CLEAR-fold and is named by ``worst``.  For the 16-bit subjects (bars: ABS_CAP on the maximum, FLAG / 2 on the outlier ratio) it shows
the maps quiet on operand rounding at these slice counts, and late rows zeroed or shifted by one row over FLAG."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import manner_oracle as O
import slice_ref as S
from manner_amd.config import ARCH_BERT, PRESETS
from manner_amd.synth import synth_news_tokens
from manner_amd.weights import make_plm_weights
from side_ops_ref import MEASURED_FACTOR, QUARTER_ULP
from test_gemm_tiles_host import FLAG, QUIET_RATIO

SEED = 20261021
VOCAB = 16384                        # room for one id per (news, position) of batch P
FIRST_ID = 200                       # above [CLS] / [SEP] / pad of both architectures
TRIP = 4096                          # train.hip: LN_BWD_BLOCKS (1024) workgroups x 4 waves, one row a wave
ORDERED_MAX = 8192                   # train.hip: EMBED_ORDERED_MAX; more padded positions run the atomic embed_bwd_kernel
CYCLE_P, LP_P = (2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128), 128
R_VALUES = 300
CYCLE_F, N_F, LP_F = (1, 2, 31, 32, 33, 64, 65, 96, 97), 85, 97
CLEAR = 10.0                         # a planted defect exceeds the bar of its map at least this many times
ABS_CAP_MAX = 0.1                    # the widest bar on a map's maximum of the 16-bit subjects (ABS_CAP of test_gpu_gemm_tiles.py)
WORD, POS, TYPE = ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
                   "embeddings.token_type_embeddings.weight")
ELN_G, ELN_B = "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"
HOST = {"tiny-bert": dataclasses.replace(PRESETS["tiny-bert-512"], vocab=VOCAB),
        "tiny-roberta": dataclasses.replace(PRESETS["tiny-roberta-514"], vocab=VOCAB)}


# ------------------------------------------------------------------------------------------------ the batches
def lengths_p() -> np.ndarray:
    lens = np.array(CYCLE_P * 2 + (128,) * 51 + (35,))
    return lens[np.random.default_rng(SEED).permutation(len(lens))]


def batch_p(cfg, repeated: bool = False):
    """ids, mask [76, 128]: one id of its own per (news, position) between [CLS] and [SEP], or (``repeated``, batch R) one of 300."""
    lens = lengths_p()
    ids, mask = synth_news_tokens(len(lens), cfg, seed=SEED % 1000, lengths=lens, pad_to=LP_P)
    inner = inner_positions(mask)
    rng = np.random.default_rng(SEED + int(repeated))
    if repeated:
        ids[inner] = FIRST_ID + rng.integers(0, R_VALUES, int(inner.sum()))
    else:
        ids[inner] = FIRST_ID + rng.permutation(cfg.vocab - FIRST_ID)[:int(inner.sum())]
    return ids, mask


def batch_f(cfg):
    """ids, mask [85, 97] with 1 .. 97 real tokens a news (1: the [CLS] alone); the padded positions hold the pad token."""
    lens = np.resize(CYCLE_F, N_F)
    ids, mask = synth_news_tokens(N_F, cfg, seed=SEED % 1000 + 1, lengths=np.maximum(lens, 2), pad_to=LP_F)
    one = lens == 1
    ids[one, 1], mask[one, 1] = cfg.pad_id, 0
    return ids, mask


def inner_positions(mask) -> np.ndarray:
    lens = np.asarray(mask).sum(1)
    col = np.arange(mask.shape[1])[None, :]
    return (col > 0) & (col < lens[:, None] - 1)


def check_conditions_p(cfg, ids, mask, repeated: bool) -> None:
    n, lp = mask.shape
    lens, m = mask.sum(1), int(mask.sum())
    assert (n, lp) == (76, LP_P) and m == 8229 == 2 * TRIP + 37
    assert 2 * TRIP < m < 2 * TRIP + 256 and (m - 2 * TRIP) % 4 != 0          # a third trip of ten workgroups, the tenth with one wave
    assert -(-(m - 2 * TRIP) // 4) == 10 and (m - 2 * TRIP) % 4 == 1
    assert n * lp == 9728 > ORDERED_MAX                                       # the atomic scatter
    assert set(CYCLE_P) <= set(lens.tolist()) and 35 in lens and int((lens == 128).sum()) == 53
    inner = inner_positions(mask)
    vals, cnt = np.unique(ids[inner], return_counts=True)
    assert vals.min() >= FIRST_ID and vals.max() < cfg.vocab
    if repeated:
        assert len(vals) == R_VALUES and 10 <= cnt.min() and cnt.max() <= 60, (len(vals), cnt.min(), cnt.max())
    else:
        assert (cnt == 1).all() and len(vals) == m - 2 * n
    trips = S.trip_labels(mask)
    assert sorted(np.unique(trips[mask != 0]).tolist()) == [0, 1, 2] and int((trips == 2).sum()) == 37
    assert (mask[ids == cfg.pad_id] == 0).all() and (ids[mask == 0] == cfg.pad_id).all()


def check_conditions_f(cfg, ids, mask) -> None:
    n, lp = mask.shape
    lens = mask.sum(1)
    assert (n, lp) == (N_F, LP_F) and n * lp == 8245 == 2 * TRIP + 53 and n * lp > ORDERED_MAX and (n * lp - 2 * TRIP) % 4 != 0
    assert set(lens.tolist()) == set(CYCLE_F)
    assert (ids[mask == 0] == cfg.pad_id).all() and (ids[mask != 0] != cfg.pad_id).all()
    assert cfg.pad_id + 1 + lp <= cfg.max_pos


# ------------------------------------------------------------------------------------------------ the maps
def held(names):
    """Every 2-D encoder weight, every bias and LayerNorm parameter, the embedding LayerNorm included; not the key bias (zero in exact
    arithmetic: no scale to hold it to)."""
    return [k for k in names if (k.startswith("encoder.layer.") or k.startswith("embeddings.LayerNorm.")) and not k.endswith("key.bias")]


def word_block_labels(cfg, ids, mask) -> np.ndarray:
    """[vocab, 1]: (news, 32-token block) of the token that owns the row, -1 for [CLS] / [SEP] / pad and unused rows (unique ids)."""
    nb = (mask.shape[1] + 31) // 32
    word = np.full(cfg.vocab, -1, dtype=np.int64)
    news, t = np.nonzero(inner_positions(mask))
    word[ids[news, t]] = news * nb + t // 32
    return word[:, None]


def pos_block_labels(cfg, mask) -> np.ndarray:
    first = 0 if cfg.arch == ARCH_BERT else cfg.pad_id + 1
    longest = int(mask.sum(1).max())
    pos = np.full(cfg.max_pos, -1, dtype=np.int64)
    pos[first:first + longest] = np.arange(longest) // 32
    return pos[:, None]


def _type_labels(cfg) -> np.ndarray:
    lab = np.full((cfg.type_vocab, cfg.hidden), -1, dtype=np.int64)
    lab[0] = S.vector_block_labels(cfg.hidden)
    return lab


def parameter_maps(cfg, got, ref, names) -> dict:
    """The token-type row and every bias / LayerNorm gamma, beta per 64 elements, every 2-D weight gradient per 128 x 64 tile."""
    out = {"type_row": S.error_map(got[TYPE], ref[TYPE], _type_labels(cfg), min_count=64, per_slice=True)}
    for k in held(names):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if g.ndim == 2:
            out[k] = S.error_map(g, r, S.weight_tile_labels(g.shape), per_slice=True)
        else:
            out[k] = S.error_map(g, r, S.vector_block_labels(len(g)), min_count=64, per_slice=True)
    return out


def maps_p(cfg, ids, mask, got, ref) -> dict:
    """Batch P.  got / ref: {"cls": [N, H], "grads": {name: array}}."""
    g, r = got["grads"], ref["grads"]
    out = {"cls": S.error_map(got["cls"], ref["cls"], S.news_labels(len(mask), cfg.hidden))}
    used = np.unique(ids[inner_positions(mask)])                        # the map only reads these rows
    out["word"] = S.error_map(np.asarray(g[WORD])[used], np.asarray(r[WORD])[used], word_block_labels(cfg, ids, mask)[used], per_slice=True)
    out["pos"] = S.error_map(g[POS], r[POS], pos_block_labels(cfg, mask), per_slice=True)
    out.update(parameter_maps(cfg, g, r, r.keys()))
    return out


def table_rows(cfg, ids, mask, full: bool):
    """The rows of the word and of the position table a batch reaches; full rows: the pad token's row and RoBERTa's pad position too."""
    sel = np.ones(mask.shape, dtype=bool) if full else mask != 0
    pos = O.position_ids(torch.from_numpy(ids), cfg.arch, cfg.pad_id).numpy()
    return np.unique(ids[sel]), np.unique(pos[sel])


def maps_rows(cfg, ids, mask, got, ref, full: bool) -> dict:
    """The word and the position table per row (batches with repeated ids)."""
    g, r = got["grads"], ref["grads"]
    wr, pr = table_rows(cfg, ids, mask, full)
    return {"word_rows": S.error_map(np.asarray(g[WORD])[wr], np.asarray(r[WORD])[wr], S.table_row_labels(cfg.vocab, wr)[wr],
                                     min_count=cfg.hidden, per_slice=True),
            "pos_rows": S.error_map(g[POS], r[POS], S.table_row_labels(cfg.max_pos, pr), min_count=cfg.hidden, per_slice=True)}


def maps_f(cfg, ids, mask, got, ref) -> dict:
    """Batch F.  got / ref: {"out": [N, Lp, H], "grads": ...}; the output per (news, 32-position block), padded positions included."""
    every = np.ones(mask.shape, dtype=np.int64)
    out = {"out": S.error_map(got["out"], ref["out"], S.token_block_head_labels(every, cfg.hidden, 1))}
    out.update(maps_rows(cfg, ids, mask, got, ref, full=True))
    out.update(parameter_maps(cfg, got["grads"], ref["grads"], ref["grads"].keys()))
    return out


def slice_trips(m: S.SliceMap, mask, last: bool = False) -> np.ndarray:
    """The trip (packed row // 4096) of the first token, or of the ``last``, of every slice of a (news, 32-token block) map over the
    tokens between [CLS] and [SEP] (at H >= 128 a block of one token is a slice: none is merged)."""
    nb = (mask.shape[1] + 31) // 32
    trips = S.trip_labels(mask)
    news, blk = np.divmod(m["labels"], nb)
    t = np.minimum(32 * blk + 31, mask.sum(1)[news] - 2) if last else np.maximum(32 * blk, 1)
    return trips[news, t]


def trip_medians(m: S.SliceMap, mask) -> dict:
    t = slice_trips(m, mask)
    return {int(k): float(np.median(m["rms"][t == k])) for k in np.unique(t)}


def numpy_result(r: dict) -> dict:
    return {k: ({n: g.detach().cpu().numpy() for n, g in v.items() if g is not None} if k == "grads" else v.detach().cpu().numpy())
            for k, v in r.items()}


def fp32_bars(maps32: dict) -> dict:
    """{map: MEASURED_FACTOR x the maximum of the float32 evaluation's map}; every figure is above the floor."""
    low = {k: m["max"] for k, m in maps32.items() if not m["max"] >= QUARTER_ULP}
    assert not low, f"float32 figures below 2^-25: {low}"
    return {k: MEASURED_FACTOR * m["max"] for k, m in maps32.items()}


def settled(build, salts: int = 8):
    """build(salt) -> (anything, maps of the float32 evaluation) at the first salt whose figures are all at least QUARTER_ULP."""
    for salt in range(salts):
        made = build(salt)
        if all(m["max"] >= QUARTER_ULP for m in made[-1].values()):
            return (salt,) + tuple(made)
    raise AssertionError(f"no salt in {salts} settles the float32 figures")


def draw_R(shape, salt: int) -> torch.Tensor:
    """The objective's weights, float64 values that float32 holds exactly: the kernels read the same numbers as the reference."""
    return torch.from_numpy(np.random.default_rng(SEED + 7919 * salt).standard_normal(shape).astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------------------------------------ the host cases
BATCHES = ("P", "R", "F")


def _tokens(batch, cfg):
    return batch_f(cfg) if batch == "F" else batch_p(cfg, repeated=batch == "R")


def _maps(batch, cfg, ids, mask, got, ref):
    if batch == "P":
        return maps_p(cfg, ids, mask, got, ref)
    if batch == "R":
        return maps_rows(cfg, ids, mask, got, ref, full=False)
    return maps_f(cfg, ids, mask, got, ref)


def _evaluate(batch, cfg, w, ids, mask, R, dtype=torch.float64, embed=None):
    return numpy_result(S.reference(cfg, w, ids, mask, train=True, R=R, dtype=dtype, full=batch == "F", embed=embed))


@functools.lru_cache(maxsize=None)
def host_case(batch: str, name: str):
    """cfg, ids, mask, R, the float64 evaluation, the maps of the float32 evaluation and the salt that settled them."""
    cfg = HOST[name]
    w = make_plm_weights(cfg, seed=SEED % 1000, std=0.02, with_pooler=False)
    ids, mask = _tokens(batch, cfg)
    shape = mask.shape + (cfg.hidden,) if batch == "F" else (len(mask), cfg.hidden)

    def build(salt):
        R = draw_R(shape, salt)
        ref64 = _evaluate(batch, cfg, w, ids, mask, R)
        ref32 = _evaluate(batch, cfg, w, ids, mask, R, dtype=torch.float32)
        return R, ref64, _maps(batch, cfg, ids, mask, ref32, ref64)

    salt, R, ref64, maps32 = settled(build)
    return dict(cfg=cfg, w=w, ids=ids, mask=mask, R=R, ref=ref64, maps32=maps32, salt=salt)


@pytest.mark.parametrize("name", list(HOST))
def test_conditions_of_the_three_batches(name):
    cfg = HOST[name]
    for repeated in (False, True):
        ids, mask = batch_p(cfg, repeated)
        check_conditions_p(cfg, ids, mask, repeated)
    assert np.array_equal(batch_p(cfg)[1], batch_p(cfg, True)[1])           # batch R: the lengths of batch P
    ids, mask = batch_f(cfg)
    check_conditions_f(cfg, ids, mask)
    wr, pr = table_rows(cfg, ids, mask, full=True)
    assert cfg.pad_id in wr and (cfg.arch == ARCH_BERT or cfg.pad_id in pr)
    m = S.error_map(np.ones((cfg.vocab, 4)), np.ones((cfg.vocab, 4)), word_block_labels(cfg, *batch_p(cfg)), min_count=1)
    assert sorted(np.unique(slice_trips(m, batch_p(cfg)[1])).tolist()) == [0, 1, 2]       # every trip owns slices of the word-row map


def test_labellings():
    mask = np.array([[1, 1, 1, 0], [1, 1, 0, 0], [1, 1, 1, 1]])
    assert S.trip_labels(mask, rows_per_trip=4).tolist() == [[0, 0, 0, -1], [0, 1, -1, -1], [1, 1, 1, 2]]
    assert S.trip_labels(np.ones((2, 3)), rows_per_trip=4).tolist() == [[0, 0, 0], [0, 1, 1]]
    lab = S.table_row_labels(6, [4, 1, 4])
    assert lab.shape == (6, 1) and lab[:, 0].tolist() == [-1, 1, -1, -1, 4, -1]
    got, ref = np.zeros((6, 128)), np.zeros((6, 128))
    ref[1], ref[4], got[1], got[4] = 1.0, 10.0, 1.0, 11.0
    m = S.error_map(got, ref, lab, min_count=128, per_slice=True)             # one slice a row, each against its own scale
    assert m["labels"].tolist() == [1, 4] and m["worst"] == 4 and abs(m["max"] - 0.1) < 1e-12


@pytest.mark.parametrize("name", list(HOST))
@pytest.mark.parametrize("batch", BATCHES)
def test_the_float32_evaluation_is_settled_on_every_map(batch, name):
    case = host_case(batch, name)
    for k, m in case["maps32"].items():
        print(f"{batch} {name} {k}: float32 evaluation max {m['max']:.3e} ratio {m['ratio']:.2f} -> bar {MEASURED_FACTOR * m['max']:.3e}")
    bars = fp32_bars(case["maps32"])
    assert min(bars.values()) >= MEASURED_FACTOR * QUARTER_ULP and max(bars.values()) < 1e-4, (min(bars.values()), max(bars.values()))
    if batch == "P":
        print("per-trip medians of the word-row map:", trip_medians(case["maps32"]["word"], case["mask"]))


def test_full_rows_restate_the_padding_index():
    """The pad token's word row and RoBERTa's pad position take no gradient (HF's padding_idx); BERT's position table has none: the rows
    of its padded positions take theirs.  The [CLS] objective never reaches a padded position."""
    for name, cfg in HOST.items():
        g = host_case("F", name)["ref"]["grads"]
        assert not g[WORD][cfg.pad_id].any()
        if cfg.arch == ARCH_BERT:
            assert all(g[POS][t].any() for t in range(1, LP_F))
        else:
            assert not g[POS][cfg.pad_id].any() and all(g[POS][cfg.pad_id + 1 + t].any() for t in range(LP_F))
        g = host_case("P", name)["ref"]["grads"]
        assert not g[WORD][cfg.pad_id].any()


# ------------------------------------------------------------------------------------------------ planted defects
class _Rows(torch.autograd.Function):
    """table[idx]; the table gradient summed as a defective scatter would: ``limit`` (positions n * Lp + t >= limit left out), ``once``
    (a repeated row takes its first position only), ``padding_idx`` (that row takes nothing)."""

    @staticmethod
    def forward(ctx, table, idx, padding_idx, limit, once):
        ctx.idx, ctx.rows, ctx.opts = idx, table.shape[0], (padding_idx, limit, once)
        return table[idx]

    @staticmethod
    def backward(ctx, g):
        padding_idx, limit, once = ctx.opts
        idx = ctx.idx.reshape(-1)
        g = g.reshape(idx.numel(), -1)
        take = torch.ones_like(idx, dtype=torch.bool)
        if padding_idx is not None:
            take &= idx != padding_idx
        if limit is not None:
            take &= torch.arange(idx.numel()) < limit
        at = torch.nonzero(take)[:, 0]
        if once:
            at = at[torch.from_numpy(np.unique(idx[at].numpy(), return_index=True)[1])]
        return torch.zeros((ctx.rows, g.shape[1]), dtype=g.dtype).index_add_(0, idx[at], g[at]), None, None, None, None


class _LayerNormRows(torch.autograd.Function):
    """LayerNorm over the rows of ``rows`` ([N, L] bool, packed in news order as ln_bwd_kernel sees them) with the backward written out:
    ``stale`` computes packed row m >= 4096 from the operands of row m - 4096, ``trip_dropped`` leaves the rows >= 8192 out of d gamma
    and d beta."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, rows, defect):
        mean = x.mean(-1, keepdim=True)
        rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
        xhat = (x - mean) * rstd
        ctx.save_for_backward(xhat, rstd, gamma)
        ctx.rows, ctx.defect = rows, defect
        return xhat * gamma + beta

    @staticmethod
    def backward(ctx, dy):
        xhat, rstd, gamma = ctx.saved_tensors
        d, xh, rs = dy[ctx.rows], xhat[ctx.rows], rstd[ctx.rows]             # [M, H] packed
        g = d * gamma
        dx = rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
        cg, cb = d * xh, d
        if ctx.defect == "stale":
            src = torch.arange(len(d))
            src[TRIP:] -= TRIP
            dx, cg, cb = dx[src], cg[src], cb[src]
        if ctx.defect == "trip_dropped":
            cg, cb = cg[:2 * TRIP], cb[:2 * TRIP]
        full = torch.zeros_like(dy)
        full[ctx.rows] = dx
        return full, cg.sum(0), cb.sum(0), None, None, None


def planted(defect, mask, full: bool):
    """The embedding stage of slice_ref.reference (``embed``) with one defect, or with none (``defect=None``)."""
    rows = torch.ones(mask.shape, dtype=torch.bool) if full else torch.from_numpy(mask != 0)

    def embed(ids, p, cfg):
        pos = O.position_ids(ids, cfg.arch, cfg.pad_id)
        if defect == "pad_position":                                          # t + pad_id + 1: the rule of the real positions
            pos = torch.where(ids.ne(cfg.pad_id), pos, torch.arange(ids.shape[1])[None, :] + cfg.pad_id + 1)
        word_pad = cfg.pad_id if full and defect != "pad_row" else None
        pos_pad = cfg.pad_id if full and cfg.arch != ARCH_BERT else None
        limit, once = (ORDERED_MAX if defect == "late_positions" else None), defect == "once"
        x = _Rows.apply(p[WORD], ids, word_pad, limit, once) + p[TYPE][0] + _Rows.apply(p[POS], pos, pos_pad, limit, once)
        return _LayerNormRows.apply(x, p[ELN_G], p[ELN_B], cfg.ln_eps, rows, defect)
    return embed


def _planted_maps(batch, name, defect):
    case = host_case(batch, name)
    bad = _evaluate(batch, case["cfg"], case["w"], case["ids"], case["mask"], case["R"], embed=planted(defect, case["mask"], batch == "F"))
    return case, _maps(batch, case["cfg"], case["ids"], case["mask"], bad, case["ref"]), fp32_bars(case["maps32"])


def _excess(maps, bars, key, defect):
    x = maps[key]["max"] / bars[key]
    print(f"{defect}: {key} {maps[key]!r} / bar {bars[key]:.3e} = {x:.3e}")
    return x


@pytest.mark.parametrize("name", list(HOST))
@pytest.mark.parametrize("batch", BATCHES)
def test_the_written_out_embedding_stage_is_the_restatement(batch, name):
    """Without a defect the stage the defects are planted in gives the gradients of the restatement: every map far under its bar."""
    _, maps, bars = _planted_maps(batch, name, None)
    assert all(m["max"] < 1e-3 * bars[k] for k, m in maps.items()), {k: m["max"] for k, m in maps.items()}


@pytest.mark.parametrize("name", list(HOST))
def test_a_stale_prefetch_in_the_layernorm_backward_is_flagged(name):
    """Rows >= 4096 of the embedding LayerNorm's backward computed from the operands of the row 4096 earlier: with unique ids every
    word row is one such row."""
    case, maps, bars = _planted_maps("P", name, "stale")
    assert _excess(maps, bars, "word", "stale") >= CLEAR
    m = maps["word"]
    assert slice_trips(m, case["mask"])[int(np.argmax(m["rms"]))] >= 1, m      # worst names a slice of the rows >= 4096
    good = m["rms"][slice_trips(m, case["mask"], last=True) == 0]
    assert good.max() < bars["word"]                                           # the first trip is untouched
    assert min(_excess(maps, bars, k, "stale") for k in (ELN_G, ELN_B, "pos")) >= CLEAR


@pytest.mark.parametrize("name", list(HOST))
def test_gamma_and_beta_partials_without_the_third_trip_are_flagged(name):
    _, maps, bars = _planted_maps("P", name, "trip_dropped")
    assert min(_excess(maps, bars, k, "trip_dropped") for k in (ELN_G, ELN_B)) >= CLEAR
    assert maps["word"]["max"] < bars["word"] and maps["pos"]["max"] < bars["pos"]      # nothing else moves


@pytest.mark.parametrize("name", list(HOST))
def test_a_scatter_without_the_positions_past_8192_is_flagged(name):
    case, maps, bars = _planted_maps("P", name, "late_positions")
    assert min(_excess(maps, bars, k, "late_positions") for k in ("word", "pos")) >= CLEAR
    nb = (LP_P + 31) // 32
    assert maps["word"]["worst"] // nb >= ORDERED_MAX // LP_P, maps["word"]      # a news whose positions lie past 8192


@pytest.mark.parametrize("name", list(HOST))
def test_repeated_ids_counted_once_are_flagged(name):
    case, maps, bars = _planted_maps("R", name, "once")
    assert min(_excess(maps, bars, k, "once") for k in ("word_rows", "pos_rows")) >= CLEAR
    ids, mask = case["ids"], case["mask"]
    assert int((ids[mask != 0] == maps["word_rows"]["worst"]).sum()) > 1


def test_a_roberta_padded_position_embedded_as_a_real_one_is_flagged():
    case, maps, bars = _planted_maps("F", "tiny-roberta", "pad_position")
    assert min(_excess(maps, bars, k, "pad_position") for k in ("out", "pos_rows")) >= CLEAR
    nb = (LP_F + 31) // 32
    news, blk = divmod(maps["out"]["worst"], nb)
    assert (case["mask"][news, 32 * blk:32 * blk + 32] == 0).any(), maps["out"]      # a block with padded positions


@pytest.mark.parametrize("name", list(HOST))
def test_a_pad_row_that_takes_the_gradient_of_the_padded_positions_is_flagged(name):
    case, maps, bars = _planted_maps("F", name, "pad_row")
    assert _excess(maps, bars, "word_rows", "pad_row") >= CLEAR and maps["word_rows"]["worst"] == case["cfg"].pad_id


# ------------------------------------------------------------------------------------------------ the 16-bit conditions
@pytest.fixture(scope="module")
def rows16():
    """A [8229, 128] product over K = 512 in the padded layout of batch P: float64, and from operands rounded to the 16-bit types."""
    g = torch.Generator().manual_seed(21)
    mask = batch_p(HOST["tiny-bert"])[1]
    m = int(mask.sum())
    x, w = torch.randn((m, 512), generator=g, dtype=torch.float64), 0.05 * torch.randn((128, 512), generator=g, dtype=torch.float64)
    S.limit_threads()
    out = {"mask": mask, "ref": (x @ w.T).numpy(), "labels": S.token_block_head_labels(mask, 128, 1)}
    for mode, dt in S.DT16.items():
        out[mode] = (x.to(dt).float() @ w.to(dt).float().T).numpy()
    return out


def _padded(rows, mask):
    out = np.zeros(mask.shape + (rows.shape[1],), dtype=np.float64)
    out[mask != 0] = rows
    return out


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_16bit_rounding_is_quiet_at_the_slice_counts_of_batch_p(rows16, mode):
    mask = rows16["mask"]
    m = S.error_map(_padded(rows16[mode], mask), _padded(rows16["ref"], mask), rows16["labels"])
    print(mode, m)
    assert len(m["rms"]) >= 250 and m["ratio"] < QUIET_RATIO, m
    cls = S.error_map(rows16[mode][:76], rows16["ref"][:76], S.news_labels(76, 128))
    tile = S.error_map(rows16[mode][:256].T @ rows16["ref"][:256], rows16["ref"][:256].T @ rows16["ref"][:256],
                       S.weight_tile_labels((128, 128)), per_slice=True)
    print(mode, cls, tile)
    assert cls["ratio"] < QUIET_RATIO and tile["ratio"] < QUIET_RATIO, (cls, tile)


@pytest.mark.parametrize("first", [TRIP, 2 * TRIP])
@pytest.mark.parametrize("defect", ["zeroed", "shifted"])
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_late_rows_zeroed_or_shifted_by_one_are_flagged(rows16, mode, defect, first):
    """The 16-bit d16 / o16 stores of the rows a later trip visits, lost or written one row off: an error of order one in their slices.
    From the third trip on (37 rows) the outlier ratio names them; from the second trip on half the slices are wrong, the median with
    them, and the maximum is five times the widest bar it is held to."""
    mask = rows16["mask"]
    hip = rows16[mode].copy()
    hip[first:] = 0.0 if defect == "zeroed" else np.roll(rows16[mode], 1, axis=0)[first:]
    m = S.error_map(_padded(hip, mask), _padded(rows16["ref"], mask), rows16["labels"])
    print(mode, defect, first, m)
    assert m["max"] > 5 * ABS_CAP_MAX and (m["ratio"] > FLAG or first == TRIP), m
    nb = (LP_P + 31) // 32
    news, blk = divmod(m["worst"], nb)
    last_row = int(np.cumsum(mask.ravel()).reshape(mask.shape)[news, :min(32 * blk + 32, LP_P)].max()) - 1
    assert last_row >= first, (m, last_row)                                    # the worst slice holds late rows
