"""The training step held to the float64 reference of tests/slice_ref.py past 4096 token rows and 8192 padded positions, where
train.hip takes code that the smaller batches of test_gpu_attention_slices.py / test_gpu_gemm_tiles.py never reach:

  ln_bwd_kernel       1024 workgroups x 4 waves, one row a wave: past 4096 rows its row loop takes further trips and the prefetch of
                      the wave's next row (dy, x, {mean, rstd}; dy may alias dx) fires; <3> for H <= 768, <LN_V4> above
  embed_bwd_kernel    the atomic scatter-add, past EMBED_ORDERED_MAX = 8192 padded positions (below: embed_bwd_ordered_kernel); its
                      full-row branches: RoBERTa's pad position, the pad rows that take no gradient
  fp32 training mode  the f32 GEMMs over many row tiles, the token-split weight gradients, colsum / reduce_partials over 8 k rows

Two layers at bert-base width (BERT) and at roberta-large width (RoBERTa), a vocabulary of 16 384.  The batches, their conditions and
their maps are those of test_train_scale_host.py, which plants one defect per loop or branch reached here and shows that the maps see it:

  P  encode_train, 76 news padded to 128, M = 8 229 rows = 2 x 4096 + 37, N x Lp = 9 728: fp32, f16, bf16, dropout on at all five
     sites (the masks replayed into the reference), nothing frozen, one word id per (news, position)
  R  the same lengths, word ids drawn from 300 values: the atomics sum ~27 tokens a row (fp32, bert-base width)
  F  encode_full_train, 85 news x 97 positions = 8 245 rows, 1 .. 97 real tokens, R over all positions (fp32, both widths)

Bars, none of them measured from the kernels.  fp32 subjects: every map's maximum at most MEASURED_FACTOR (8) x the maximum of the same
map of the float32 evaluation of the restatement (on the GPU, without TF32) against its float64 evaluation, that figure at least
QUARTER_ULP (side_ops_ref).  f16 / bf16 subjects: ABS_CAP of test_gpu_gemm_tiles.py.  Every subject: outlier ratio at most FLAG / 2.
The figures of the MI355X run: profiles/train_scale/measured_tolerances.json.  Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import slice_ref as S  # noqa: E402
import test_train_scale_host as T  # noqa: E402
from manner_amd import hip, train  # noqa: E402
from manner_amd.config import ARCH_BERT  # noqa: E402
from manner_amd.weights import make_plm_weights  # noqa: E402
from side_ops_ref import MEASURED_FACTOR, QUARTER_ULP  # noqa: E402
from test_gemm_tiles_host import FLAG  # noqa: E402
from test_gpu_attention_slices import DEV, DROP, STORE, WIDTHS, _cuda, _replay_keep  # noqa: E402
from test_gpu_gemm_tiles import ABS_CAP, SWITCHES, _quantity  # noqa: E402

CONFIGS = {k: dataclasses.replace(c, vocab=T.VOCAB) for k, c in WIDTHS.items()}
RATIO_BAR = FLAG / 2
SEED = T.SEED
WORD, POS = T.WORD, T.POS


def test_bars_stay_under_the_conditions():
    """The ratio bar at FLAG / 2 (the host test's late-row defects clear FLAG), the 16-bit maxima under the widest bar the host test
    plants its order-one defects against, the fp32 factor the project's."""
    assert RATIO_BAR <= FLAG / 2 and MEASURED_FACTOR == 8.0 and QUARTER_ULP == 2.0 ** -25
    assert max(ABS_CAP[m] for m in ("f16", "bf16")) <= T.ABS_CAP_MAX and 5 * T.ABS_CAP_MAX < 1.0


# ------------------------------------------------------------------------------------------------ cases and references
_W = {}          # per width: weights, replayed dropout masks, references


def _width(width):
    if width not in _W:
        cfg = CONFIGS[width]
        _W[width] = {"cfg": cfg, "w": make_plm_weights(cfg, seed=SEED % 1000, std=0.02, with_pooler=False), "refs": {}}
    return _W[width]


@pytest.fixture(scope="module", autouse=True)
def _release():
    """The references (host) and the replayed masks (device) go when the file is done."""
    yield
    _W.clear()
    torch.cuda.empty_cache()


def _keep(width, mask):
    """The kernels' keep-bits for the lengths of batch P (and R), each site drawn once and kept on the device."""
    st = _width(width)
    if "keep" not in st:
        raw = _replay_keep(SEED, DROP["p_hidden"], DROP["p_out"], st["cfg"], mask)
        raw.p_attn = DROP["p_attn"]
        memo = {}

        def keep(site, kind):
            if (site, kind) not in memo:
                memo[(site, kind)] = raw(site, kind).to(DEV)
            return memo[(site, kind)]
        st["keep"] = keep
    return st["keep"]


def _tokens(width, batch):
    cfg = _width(width)["cfg"]
    return T.batch_f(cfg) if batch == "F" else T.batch_p(cfg, repeated=batch == "R")


def _shape(width, batch):
    cfg = CONFIGS[width]
    return (T.N_F, T.LP_F, cfg.hidden) if batch == "F" else (76, cfg.hidden)


def _reference(width, batch, mode, dtype, salt):
    """slice_ref.reference on the GPU, cached per (batch, mode rounding, type, draw of R), kept on the host."""
    st = _width(width)
    key = (batch, mode, dtype, salt)
    if key not in st["refs"]:
        cfg, w = st["cfg"], st["w"]
        ids, mask = _tokens(width, batch)
        R = T.draw_R(_shape(width, batch), salt)
        if batch == "F":
            r = S.reference(cfg, w, ids, mask, train=True, R=R, full=True, device=DEV, dtype=dtype)
        else:
            m16 = mode if mode in S.DT16 else None
            r = S.reference(cfg, w, ids, mask, mode=m16, store=STORE if m16 else (), train=True, R=R, keep=_keep(width, mask), device=DEV,
                            dtype=dtype, grad_keys=[WORD, POS] if batch == "R" else None, **DROP)
        st["refs"][key] = T.numpy_result(r)
        del r
        torch.cuda.empty_cache()
    return st["refs"][key]


def _maps(width, batch, got, ref):
    cfg = CONFIGS[width]
    ids, mask = _tokens(width, batch)
    if batch == "P":
        return T.maps_p(cfg, ids, mask, got, ref)
    if batch == "R":
        return T.maps_rows(cfg, ids, mask, got, ref, full=False)
    return T.maps_f(cfg, ids, mask, got, ref)


def _fp32_case(width, batch):
    """salt, R, the float64 reference and the maps of the float32 evaluation, at the first draw of R that settles every figure."""
    st = _width(width)
    if ("fp32", batch) not in st:
        def build(salt):
            ref64 = _reference(width, batch, None, torch.float64, salt)
            ref32 = _reference(width, batch, None, torch.float32, salt)
            return T.draw_R(_shape(width, batch), salt), ref64, _maps(width, batch, ref32, ref64)
        st[("fp32", batch)] = T.settled(build)
    return st[("fp32", batch)]


def _unset(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _tag(name):
    return "_".join(_quantity(name)).lstrip("_") if name.startswith(("encoder.layer.", "embeddings.LayerNorm.")) else name


def _hold(name, m, bar_max, f32_max, record, failures):
    """Print and record the map next to its bars, then compare (every map of a subject is measured before the first bar fails)."""
    tag = _tag(name)
    print(f"  {tag}: max {m['max']:.3e} (bar {bar_max:.3e})  ratio {m['ratio']:.2f} (bar {RATIO_BAR:.1f})  worst {m['worst']}  slices {len(m['rms'])}")
    record(**{f"{tag}_max": m["max"], f"{tag}_bar_max": bar_max, f"{tag}_ratio": m["ratio"], f"{tag}_bar_ratio": RATIO_BAR,
              f"{tag}_worst_label": m["worst"]})
    if f32_max is not None:
        record(**{f"{tag}_float32_evaluation_max": f32_max})
    if not (m["max"] <= bar_max and m["ratio"] <= RATIO_BAR):
        failures.append(f"{tag}: {m!r} vs bars ({bar_max:.3e}, {RATIO_BAR})")


def _hold_all(maps, bars, maps32, record):
    failures = []
    for k, m in maps.items():
        _hold(k, m, bars[k], None if maps32 is None else maps32[k]["max"], record, failures)
    return failures


def _params(w):
    return {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in w.items()}


def _untouched_rows_are_zero(grad, rows):
    rest = torch.ones(grad.shape[0], dtype=torch.bool, device=grad.device)
    rest[torch.from_numpy(np.asarray(rows)).to(grad.device)] = False
    return torch.equal(grad[rest], torch.zeros_like(grad[rest]))


def _paths(cfg, n, lp, record):
    record(ln_bwd_instantiation="<3>" if cfg.hidden <= 768 else "<LN_V4>",
           embedding_backward="embed_bwd_kernel (atomic)" if n * lp > T.ORDERED_MAX else "embed_bwd_ordered_kernel", positions=n * lp)
    assert n * lp > T.ORDERED_MAX


# ------------------------------------------------------------------------------------------------ P. packed rows, unique ids
@pytest.mark.parametrize("width,mode", [(w, m) for w in CONFIGS for m in ("fp32", "f16", "bf16")])
def test_packed_rows_past_two_trips_per_slice(width, mode, monkeypatch, measured):
    """encode_train on batch P: [CLS] per news, word rows per (news, 32-token block), position rows per 32-position block, the token-type
    row and every bias / LayerNorm gamma, beta per 64 elements, every 2-D weight gradient per 128 x 64 tile; the word-row medians per
    trip of ln_bwd_kernel."""
    _unset(monkeypatch)
    st = _width(width)
    cfg, w = st["cfg"], st["w"]
    ids, mask = _tokens(width, "P")
    T.check_conditions_p(cfg, ids, mask, repeated=False)
    m_rows, (n, lp) = int(mask.sum()), mask.shape
    assert 8192 < m_rows < 8448 and (m_rows - 8192) % 4 != 0 and n * lp == 9728 > 8192
    _paths(cfg, n, lp, measured)
    if mode == "fp32":
        salt, R, ref, maps32 = _fp32_case(width, "P")
        bars = T.fp32_bars(maps32)
    else:
        salt, R, maps32 = 0, T.draw_R(_shape(width, "P"), 0), None
        ref = _reference(width, "P", mode, torch.float64, 0)
    params = _params(w)
    out = train.encode_train(cfg, params, _cuda(ids), _cuda(mask), precision=mode, seed=SEED, **DROP)
    (out * R.float().to(DEV)).sum().backward()
    hip.check_status(DEV)
    got = {"cls": out.detach().cpu().numpy(), "grads": {k: p.grad.cpu().numpy() for k, p in params.items()}}
    maps = T.maps_p(cfg, ids, mask, got, ref)
    if mode != "fp32":
        bars = {k: ABS_CAP[mode] for k in maps}
    print(f"\nbatch P, {width}, {mode}: M = {m_rows}, N x Lp = {n * lp}, draw {salt}")
    failures = _hold_all(maps, bars, maps32, measured)
    medians = T.trip_medians(maps["word"], mask)
    print("  word-row medians per trip:", medians)
    assert sorted(medians) == [0, 1, 2]
    measured(rows=m_rows, draw=salt, **{f"word_median_trip{k}": v for k, v in medians.items()})
    assert _untouched_rows_are_zero(params[WORD].grad, np.unique(ids[mask != 0]))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ R. packed rows, repeated ids
def test_repeated_ids_through_the_atomic_scatter_per_table_row(monkeypatch, measured):
    """encode_train in fp32 on batch R, bert-base width: the word and the position table per row — each word row the sum of ~27 tokens,
    [CLS] / [SEP] of 76, a position row of up to 76; the rows of unused ids exactly zero."""
    _unset(monkeypatch)
    width = "bert-base"
    st = _width(width)
    cfg, w = st["cfg"], st["w"]
    ids, mask = _tokens(width, "R")
    T.check_conditions_p(cfg, ids, mask, repeated=True)
    _paths(cfg, *mask.shape, measured)
    salt, R, ref, maps32 = _fp32_case(width, "R")
    bars = T.fp32_bars(maps32)
    params = _params(w)
    out = train.encode_train(cfg, params, _cuda(ids), _cuda(mask), precision="fp32", seed=SEED, **DROP)
    (out * R.float().to(DEV)).sum().backward()
    hip.check_status(DEV)
    got = {"cls": out.detach().cpu().numpy(), "grads": {k: params[k].grad.cpu().numpy() for k in (WORD, POS)}}
    maps = T.maps_rows(cfg, ids, mask, got, ref, full=False)
    print(f"\nbatch R, {width}, fp32: M = {int(mask.sum())}, N x Lp = {mask.size}, draw {salt}")
    failures = _hold_all(maps, bars, maps32, measured)
    measured(draw=salt)
    wr, pr = T.table_rows(cfg, ids, mask, full=False)
    assert len(wr) == T.R_VALUES + 2 and len(maps["word_rows"]["rms"]) == len(wr) and len(maps["pos_rows"]["rms"]) == len(pr) == T.LP_P
    assert _untouched_rows_are_zero(params[WORD].grad, wr) and _untouched_rows_are_zero(params[POS].grad, pr)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ F. full rows
@pytest.mark.parametrize("width", list(CONFIGS))
def test_full_rows_past_two_trips_per_slice(width, monkeypatch, measured):
    """encode_full_train in fp32 on batch F, no dropout, the objective over all positions: the output per (news, 32-position block) with
    the padded positions, the gradient maps of batch P with the word and the position table per row; the pad token's word row and
    RoBERTa's pad position exactly zero, BERT's position rows of padded positions non-zero and inside the bar."""
    _unset(monkeypatch)
    st = _width(width)
    cfg, w = st["cfg"], st["w"]
    ids, mask = _tokens(width, "F")
    T.check_conditions_f(cfg, ids, mask)
    n, lp = mask.shape
    assert n * lp == 8245 == 2 * 4096 + 53 and n * lp > 8192
    _paths(cfg, n, lp, measured)
    salt, R, ref, maps32 = _fp32_case(width, "F")
    bars = T.fp32_bars(maps32)
    params = _params(w)
    out = train.encode_full_train(cfg, params, _cuda(ids), _cuda(mask), precision="fp32", p_hidden=0.0, p_attn=0.0, seed=SEED)
    (out * R.float().to(DEV)).sum().backward()
    hip.check_status(DEV)
    got = {"out": out.detach().cpu().numpy(), "grads": {k: p.grad.cpu().numpy() for k, p in params.items()}}
    maps = T.maps_f(cfg, ids, mask, got, ref)
    print(f"\nbatch F, {width}, fp32: M = N x Lp = {n * lp}, draw {salt}")
    failures = _hold_all(maps, bars, maps32, measured)
    measured(rows=n * lp, draw=salt)
    wr, pr = T.table_rows(cfg, ids, mask, full=True)
    gw, gp = params[WORD].grad, params[POS].grad
    assert cfg.pad_id in wr and not bool(gw[cfg.pad_id].any())                       # the pad token's word row
    assert _untouched_rows_are_zero(gw, wr) and _untouched_rows_are_zero(gp, pr)
    padded_at = np.nonzero((mask == 0).any(0))[0]
    assert len(padded_at) == lp - 1
    if cfg.arch == ARCH_BERT:                                                        # no padding index: the rows of padded positions take theirs
        assert all(bool(gp[int(t)].any()) for t in padded_at) and set(padded_at) <= set(maps["pos_rows"]["labels"].tolist())
    else:
        assert cfg.pad_id in pr and not bool(gp[cfg.pad_id].any())                   # RoBERTa's pad position
        assert not bool(gp[:cfg.pad_id].any())
    assert not failures, failures
