"""Head-dimension-32 attention (attention_d32.hip: attn32_16_kernel, attn32_long16_kernel, attn32_cls_kernel and their f32 forms) held to
the float64 reference of tests/slice_ref.py per slice: hidden state 1 (encode_hidden with one layer: the short and long kernels over
every query) per (news, 32-token block, head of 32), [CLS] of two layers (the last layer's attn32_cls_kernel) per news and per head
over all news — in f16, bf16 and fp32, with host lengths and with device lengths, every call one chunk.

Configs, weight sets and batches are those of test_d32_slices_host.py, which shows that these maps see one planted defect per loop,
branch or lane group of the kernels and which asserts the conditions relied on here: tiny-bert-d32 (two head pairs) and mini-minilm
(six), HF-init weights at std 0.1 and the set whose out-projection is the identity (heads stay apart), padded to 512, 385 (rows_cap
416, 31 masked keys), 161 (n_qb = 1, idle waves) and 70 (short rows, another LDS stride); the peaked sets (both outcomes of the online
softmax's rescale branch) at H = 256 padded to 512 and 385.

Bars, none of them taken from the head_dim-32 kernels.  f16 / bf16: a map's maximum at most 2 x the same map of the head_dim-64
kernels on the twin config (half the heads, the same seed, std, tokens and construction), measured here against the twin's own
float64 reference, and never above ABS_CAP of test_gpu_gemm_tiles.py.  fp32: 8 x the same map of the float32 evaluation of the
restatement (on the GPU, without TF32) against float64, that figure floored at 2^-25.  Every outlier ratio below FLAG / 2.  The
per-head [CLS] map is recorded everywhere and asserted on the identity set, where it means something.  Padded positions of
encode_hidden are exactly zero; host and device lengths give the same bits.  The figures of the MI355X run:
profiles/d32_slices/measured_tolerances.json.  Run on the MI355X box: ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import slice_ref as S  # noqa: E402
import test_d32_slices_host as T  # noqa: E402
from manner_amd import hip  # noqa: E402
from side_ops_ref import MEASURED_FACTOR, QUARTER_ULP  # noqa: E402
from test_gemm_tiles_host import FLAG  # noqa: E402
from test_gpu_gemm_tiles import ABS_CAP  # noqa: E402

DEV = "cuda:0"
RATIO_BAR = FLAG / 2
STORE = S.STORE_POINTS
# one (config, weight set) after the other, so that one pair of handles (subject and twin) lives at a time
PARAMS = [(c, ws, pad, mode) for c, ws, pad in sorted(T.CASES, key=lambda k: (k[0], k[1], -k[2])) for mode in T.MODES]


def test_bars_are_the_projects():
    assert RATIO_BAR == 6.0 and MEASURED_FACTOR == 8.0 and QUARTER_ULP == 2.0 ** -25
    assert all(T.ABS_CAP[m] == ABS_CAP[m] for m in ("f16", "bf16")) and T.bar_16bit(1.0, "bf16") == ABS_CAP["bf16"]
    assert T.bar_16bit(1e-4, "f16") == 2e-4 and T.bar_fp32(0.0) == 8.0 * 2.0 ** -25 and T.bar_fp32(1e-6) == 8e-6


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_ENC, _REFS = {}, {}


def _engines(config, weights):
    """(subject, twin): the head_dim-32 engine and the head_dim-64 engine of the twin config."""
    key = (config, weights)
    if key not in _ENC:
        for k in list(_ENC):
            for e in _ENC.pop(k):
                e.close()
        _REFS.clear()
        made = []
        for twin in (False, True):
            cfg, w, _, _ = T.case(config, weights, 512, twin)
            assert cfg.head_dim == (64 if twin else 32)
            made.append(hip.HipEncoder(cfg, w, precisions=T.MODES, device=DEV))
        _ENC[key] = tuple(made)
    return _ENC[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for k in list(_ENC):
        for e in _ENC.pop(k):
            e.close()
    _REFS.clear()
    T.case.cache_clear()
    torch.cuda.empty_cache()


def _ref(config, weights, pad, mode, twin=False, dtype=torch.float64):
    """slice_ref.reference on the GPU, cached per case while its (config, weight set) is the live one, kept on the host."""
    key = (config, weights, pad, mode, twin, dtype)
    if key not in _REFS:
        cfg, w, ids, mask = T.case(config, weights, pad, twin)
        m16 = mode if mode in S.DT16 else None
        _REFS[key] = T.numpy_result(S.reference(cfg, w, ids, mask, mode=m16, store=STORE if m16 else (), device=DEV, dtype=dtype))
    return _REFS[key]


def _encode(enc, ids, mask, mode, host_lengths):
    h1 = enc.encode_hidden(_cuda(ids), _cuda(mask), 1, precision=mode, host_lengths=host_lengths)
    cls = enc.encode_cls(_cuda(ids), _cuda(mask), precision=mode, host_lengths=host_lengths)
    enc.status()
    hip.check_status(DEV)
    return h1, cls


@pytest.mark.parametrize("config,weights,pad,mode", PARAMS)
def test_head_dim_32_per_slice(config, weights, pad, mode, measured):
    cfg, w, ids, mask = T.case(config, weights, pad)
    assert mask.shape == (len(T.BATCHES[pad]), pad) and mask.sum(1).tolist() == T.BATCHES[pad]
    enc, twin_enc = _engines(config, weights)
    h1, cls = _encode(enc, ids, mask, mode, mask.sum(1))
    h1_dev, cls_dev = _encode(enc, ids, mask, mode, None)
    got = {"hidden1": h1.float().cpu().numpy(), "cls": cls.float().cpu().numpy()}
    maps = T.maps(cfg, mask, got, _ref(config, weights, pad, mode))
    if mode == "fp32":
        side = T.maps(cfg, mask, _ref(config, weights, pad, None, dtype=torch.float32), _ref(config, weights, pad, None))
        bars = {k: T.bar_fp32(m["max"]) for k, m in side.items()}
        side_name = "float32_evaluation"
    else:
        t1, tcls = _encode(twin_enc, ids, mask, mode, mask.sum(1))
        side = T.maps(cfg, mask, {"hidden1": t1.float().cpu().numpy(), "cls": tcls.float().cpu().numpy()},
                      _ref(config, weights, pad, mode, twin=True))
        bars = {k: T.bar_16bit(m["max"], mode) for k, m in side.items()}
        side_name = "twin"
    failures = []
    print(f"\n{config} {weights} pad {pad} {mode}")
    for k, m in maps.items():                              # every map is recorded before the first bar fails
        held = k != "cls_head" or weights == "ident"
        print(f"  {k}: max {m['max']:.3e} (bar {bars[k]:.3e}, {side_name} {side[k]['max']:.3e})  ratio {m['ratio']:.2f} "
              f"({side_name} {side[k]['ratio']:.2f}, bar {RATIO_BAR:.1f})  worst {m['worst']}  slices {len(m['rms'])}{'' if held else '  (recorded only)'}")
        measured(**{f"{k}_max": m["max"], f"{k}_bar_max": bars[k], f"{k}_ratio": m["ratio"], f"{k}_bar_ratio": RATIO_BAR, f"{k}_worst_label": m["worst"],
                    f"{k}_{side_name}_max": side[k]["max"], f"{k}_{side_name}_ratio": side[k]["ratio"], f"{k}_asserted": float(held)})
        if held and not (m["max"] <= bars[k] and m["ratio"] < RATIO_BAR):
            failures.append(f"{k}: {m!r} vs bars ({bars[k]:.3e}, {RATIO_BAR})")
    keep = torch.from_numpy(mask != 0).to(DEV)
    padding_zero = not bool(h1[~keep].any()) and not bool(h1_dev[~keep].any())
    same_bits = torch.equal(h1, h1_dev) and torch.equal(cls, cls_dev)
    measured(padding_exactly_zero=float(padding_zero), host_and_device_lengths_equal=float(same_bits))
    assert padding_zero, "padded positions of encode_hidden are not exactly zero"
    assert same_bits, "host lengths and device lengths give different bits"
    assert not failures, failures
