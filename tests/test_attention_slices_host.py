"""The float64 reference and the per-slice error map of tests/slice_ref.py, on the CPU: the reference restates the oracle's fp32 path
(inference and train-mode gradients under replayed dropout masks), the map stays quiet on pure 16-bit rounding noise and flags a
defect confined to one (head, 32-token block) cell that is a tenth of the absolute bar.  The GPU side is
test_gpu_attention_slices.py."""
import numpy as np
import pytest
import torch

import manner_oracle as O
import slice_ref as S
from manner_amd.config import PRESETS
from manner_amd.synth import synth_news_tokens
from manner_amd.weights import make_plm_weights

LENS = np.array([2, 31, 33, 128, 129, 161, 257, 385, 512])
# the whole-tensor bars of the existing 16-bit tests (test_long_rows_16bit_modes_close_to_reference): the planted defect is a tenth
ABS_BAR = {"f16": 2e-2, "bf16": 0.1}
# the map of the reference against itself at 16-bit rounding stays under QUIET_RATIO; a one-cell defect goes over FLAG_RATIO
QUIET_RATIO, FLAG_RATIO = 2.0, 3.0

_CASES = {}


def _case(name):
    if name not in _CASES:
        cfg = PRESETS[name]
        w = make_plm_weights(cfg, seed=101, std=0.05, with_pooler=False)
        ids, mask = synth_news_tokens(len(LENS), cfg, seed=101, lengths=LENS)
        _CASES[name] = cfg, w, ids, mask
    return _CASES[name]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", ["tiny-bert-512", "tiny-roberta-514"])
def test_reference_without_rounding_matches_the_oracle_inference(name):
    cfg, w, ids, mask = _case(name)
    ref = S.reference(cfg, w, ids, mask)
    with torch.no_grad():
        h1 = O.encode_tokens(ids, mask, w, cfg, layers=1).numpy()
        hl = O.encode_tokens(ids, mask, w, cfg).numpy()
    m = mask.astype(bool)
    assert _rel(ref["hidden"][1].numpy()[m], h1[m]) < 1e-5
    assert _rel(ref["hidden"][-1].numpy()[m], hl[m]) < 1e-5
    assert _rel(ref["cls"].numpy(), O.encode_cls(ids, mask, w, cfg).numpy()) < 1e-5


@pytest.mark.parametrize("name", ["tiny-bert-512", "tiny-roberta-514"])
def test_reference_without_rounding_matches_the_oracle_train_gradients(name):
    """Dropout on at all five sites, the same keep masks fed to both: [CLS] outputs and every parameter gradient."""
    cfg, w, ids, mask = _case(name)
    n, lp = mask.shape
    g = torch.Generator().manual_seed(7)
    shapes = {"rows": (n, lp, cfg.hidden), "attn": (n, cfg.heads, lp, lp), "cls": (n, cfg.hidden)}
    masks = {}

    def keep(site, kind):
        if site not in masks:
            masks[site] = (torch.rand(shapes[kind], generator=g) >= 0.1).float()
        return masks[site]

    R = torch.randn((n, cfg.hidden), generator=g)
    kw = dict(p_hidden=0.1, p_attn=0.1, p_out=0.1, keep=keep)
    ref = S.reference(cfg, w, ids, mask, train=True, R=R, **kw)
    wt = {k: torch.from_numpy(v).requires_grad_(True) for k, v in w.items()}
    out = O.encode_cls_train(ids, mask, wt, cfg, **kw)
    (out * R).sum().backward()
    assert _rel(ref["cls"].numpy(), out.detach().numpy()) < 1e-5
    for k, t in wt.items():
        if k.endswith("attention.self.key.bias"):             # zero in exact arithmetic (softmax shift invariance)
            assert np.abs(ref["grads"][k].numpy()).max() < 1e-12, k
            continue
        assert _rel(ref["grads"][k].numpy(), t.grad.numpy()) < 1e-5, k


@pytest.fixture(scope="module")
def noise_case():
    """hidden_states[1] and [CLS] of tiny-bert-512: unrounded reference and the fully rounded one per 16-bit mode."""
    cfg, w, ids, mask = _case("tiny-bert-512")
    exact = S.reference(cfg, w, ids, mask)
    rounded = {m: S.reference(cfg, w, ids, mask, mode=m, store=S.STORE_POINTS) for m in ("f16", "bf16")}
    return cfg, mask, exact, rounded


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_error_map_is_quiet_on_rounding_noise(noise_case, mode):
    cfg, mask, exact, rounded = noise_case
    lab = S.token_block_head_labels(mask, cfg.hidden, cfg.heads)
    m = S.error_map(rounded[mode]["hidden"][1], exact["hidden"][1], lab)
    assert len(m["rms"]) > 30
    assert m["max"] < ABS_BAR[mode] and m["ratio"] < QUIET_RATIO, m
    c = S.error_map(rounded[mode]["cls"], exact["cls"], S.news_labels(len(LENS), cfg.hidden))
    assert c["ratio"] < QUIET_RATIO, c


@pytest.mark.parametrize("where", [(5, 1, 4), (8, 0, 15), (0, 1, 0)])      # (news, head, block): a long row's last block, a 2-token row
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_error_map_flags_a_defect_in_one_cell(noise_case, mode, where):
    """A perturbation of a tenth of the absolute bar in one (news, head, block) cell of the rounded reference: the whole-tensor
    max error stays far under the bar, the map's outlier ratio flags it and names the cell."""
    cfg, mask, exact, rounded = noise_case
    lab = S.token_block_head_labels(mask, cfg.hidden, cfg.heads)
    hip = rounded[mode]["hidden"][1].numpy().copy()
    news, head, blk = where
    d = cfg.head_dim
    rows = slice(32 * blk, min(32 * (blk + 1), int(LENS[news])))
    sign = np.where(np.random.default_rng(1).random(hip[news, rows, head * d:(head + 1) * d].shape) < 0.5, -1.0, 1.0)
    hip[news, rows, head * d:(head + 1) * d] += 0.1 * ABS_BAR[mode] * sign
    ref = exact["hidden"][1].numpy()
    assert np.abs(hip - ref)[mask.astype(bool)].max() < 0.2 * ABS_BAR[mode]
    m = S.error_map(hip, ref, lab)
    assert m["ratio"] > FLAG_RATIO, m
    planted = (news * cfg.heads + head) * ((mask.shape[1] + 31) // 32) + blk
    assert m["worst"] == m["labels"][np.searchsorted(m["labels"], planted, "right") - 1], m


def test_error_map_merges_small_slices():
    ref = np.ones(100)
    lab = np.repeat([0, 1, 2, 3, 4], [5, 30, 5, 30, 30])           # 0 joins 1 (it comes first), 2 joins 1
    hip = ref.copy()
    hip[70:] += 0.5                                                 # label 4
    hip[:5] += 2.0
    m = S.error_map(hip, ref, lab, min_count=10)
    assert list(m["labels"]) == [0, 3, 4] and m["worst"] == 0
    assert np.allclose(m["rms"], [np.sqrt(20.0 / 40), 0.0, 0.5])
    lab[-30:] = -1                                                  # left out entirely, also from the scale
    m = S.error_map(hip, ref, lab, min_count=10)
    assert list(m["labels"]) == [0, 3] and np.isclose(m["ratio"], 2.0)                 # median of two slices: their mean
