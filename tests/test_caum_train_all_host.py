"""CAUM's candidate loop in train() over all columns (tests/caum_train_all_ref.py) without a GPU: the loop restatement with masks
equals ``caum_ref.caum_module_forward`` at p = 0, the wide form — the rows in (b, c, s) order, as the kernels take them — equals the
loop with the same masks at p = 0 and p = 0.2, forward and every gradient; every planted defect of the wide layout and of the mask
indices moves an asserted quantity past its MEASURED bar at least 10-fold; the seed search settles within 32 seeds for every dropout
shape the GPU test runs; and header, binding and built library agree on the new exports under ABI 8."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import caum_ref as CR
import caum_train_all_ref as T
import side_ops_ref as R
from manner_amd import _lib


def _ids(shape):
    return "B{}-S{}-D{}-F{}-H{}-{}-h{}-C{}".format(*shape)


def _eval(case, fn, dtype=torch.float64, consts=None, **kw):
    return R.evaluate(fn, case.leaves, dict(case.consts if consts is None else consts, **kw), case.upstream, dtype)


# ------------------------------------------------------------------------------------------------ the restatements
def test_the_keep_rule_is_splitmix64_with_the_float32_threshold():
    assert T.threshold(0.0) == 0 and T.threshold(0.2) == 13421773 * 64 and T.threshold(0.5) == 2 ** 31          # 0.2f = 13421773 2^-26
    # splitmix64's first output for the state 0 (the published test vector 0xE220A8397B1DCDAF): seed ^ site-term = 0 at site 0
    assert int(T.drop_bits(0, 0, np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF >> 32
    keep = T.numpy_mask(99, 8, 0.2, 1 << 16)
    assert 0.79 < float(keep.float().mean()) < 0.81
    assert not torch.equal(keep, T.numpy_mask(99, 9, 0.2, 1 << 16)) and not torch.equal(keep, T.numpy_mask(98, 8, 0.2, 1 << 16))
    assert bool(T.numpy_mask(99, 8, 0.0, 64).all())


@pytest.mark.parametrize("shape", T.DEFECT_SHAPES, ids=_ids)
def test_the_loop_without_dropout_is_the_module_forward(shape):
    case = T.train_case(shape, 0.0)
    ref = case.ref()
    want = R.evaluate(CR.caum_module_forward, case.leaves, {"heads": shape[6]}, case.upstream, torch.float64)
    assert set(ref) == set(want) and all(torch.equal(ref[k], want[k]) for k in want)
    assert tuple(ref["scores"].shape) == (shape[0], shape[7])


@pytest.mark.parametrize("p", [0.0, T.P], ids=["p0", "p0.2"])
@pytest.mark.parametrize("shape", T.DEFECT_SHAPES + ((3, 1) + T.GW + (5,), (3, 2) + T.GW + (5,)), ids=_ids)
def test_the_wide_form_is_the_loop_with_the_same_masks(shape, p):
    case = T.train_case(shape, p)
    ref, bars = case.ref(), case.bars()
    exact, single = _eval(case, T.caum_train_all_wide), _eval(case, T.caum_train_all_wide, torch.float32)
    for k in sorted(ref):
        if k == "d_bc":                                                        # zero in exact arithmetic: rounding noise on both sides
            continue
        e64 = R.rel_to_max(exact[k], ref[k])
        assert e64 <= 1e-11, (case, k, e64)
        assert R.rel_to_max(single[k], ref[k]) <= bars[k]["bar"], (case, k)
    if p > 0:
        plain = T.train_case(shape, 0.0).ref()["scores"]
        assert R.rel_to_max(ref["scores"], plain) > 0.05                      # the dropouts move the scores
        assert all(0.6 < float(k.float().mean()) < 0.95 for col in case.consts["keeps"] for k in col[1:])
    if shape[0] > 1:
        assert float(ref["scores"][1, -1]) == 0.0                              # the zero candidate row scores an exact zero, masks or not


# ------------------------------------------------------------------------------------------------ planted defects
def _masks(case, shape, **kw):
    b, s, d, f = shape[:4]
    return dict(case.consts, keeps=T.column_keeps(case.seeds, case.p, b, s, d, f, **kw))


# (planted defect, the function evaluated, its constants as a function of (case, shape), the quantities it must move)
_PLANTED = [
    ("column c draws with column 0's seed", T.caum_train_all, lambda c, s: _masks(c, s, same_seed=True), ("scores",)),
    ("dropout3 indexed by the wide row", T.caum_train_all, lambda c, s: _masks(c, s, wide_dropout3=True), ("scores",)),
    ("d hist from the last column alone", T.caum_train_all_wide, lambda c, s: dict(c.consts, d_hist_last_only=True), ("d_hist",)),
    ("d hist summed before the per-column mask", T.caum_train_all_wide, lambda c, s: dict(c.consts, d_hist_one_mask=True), ("d_hist",)),
    ("pseudo-user terms read at c B + b", T.caum_train_all_wide, lambda c, s: dict(c.consts, transposed_rows=True), ("scores",)),
    ("the window wraps across the columns", T.caum_train_all_wide, lambda c, s: dict(c.consts, wrap_over_columns=True), ("scores",)),
]


@pytest.mark.parametrize("shape", T.DEFECT_SHAPES, ids=_ids)
@pytest.mark.parametrize("what,fn,consts,moved", _PLANTED, ids=[p[0] for p in _PLANTED])
def test_a_planted_defect_exceeds_the_bar_tenfold(what, fn, consts, moved, shape):
    case = T.train_case(shape, T.P)
    assert shape[0] != shape[7] and shape[7] >= 3 and shape[1] >= 5
    got, ref, bars = _eval(case, fn, consts=consts(case, shape)), case.ref(), case.bars()
    for k in moved:
        ratio = R.rel_to_max(got[k], ref[k]) / bars[k]["bar"]
        print(what, case, k, f"{ratio:.3g} x the bar")
        assert ratio >= 10.0, (what, k, ratio)
    if moved == ("d_hist",):
        assert torch.equal(got["scores"], _eval(case, T.caum_train_all_wide)["scores"])      # a defect of the backward alone


# ------------------------------------------------------------------------------------------------ the seed search
@pytest.mark.parametrize("shape", T.DROPOUT_SHAPES, ids=_ids)
def test_the_seed_search_settles_within_32_seeds(shape):
    case = T.train_case(shape, T.P)
    assert 1234 <= case.manual <= 1265 and len(case.seeds) == shape[7] and T.is_settled(case)
    assert case.seeds == T.draw_seeds(case.manual, shape[7])


# ------------------------------------------------------------------------------------------------ header, binding, library
EXPORTS = ["manner_hip_caum_train_all_saved_bytes", "manner_hip_caum_train_all_forward", "manner_hip_caum_train_all_backward_workspace_bytes",
           "manner_hip_caum_train_all_backward", "manner_hip_wgrad_rows_f32_workspace_bytes", "manner_hip_wgrad_rows_f32"]


@pytest.mark.parametrize("name", EXPORTS)
def test_header_declares_the_export_and_the_binding_matches_its_arguments(name):
    with open(_lib.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = re.findall(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", text)
    assert len(protos) == 1, name
    args = [a.strip() for a in protos[0][1].split(",")]
    res, bound = _lib.SIGNATURES[name]
    assert res is (C.c_int if protos[0][0] == "int" else _lib._SZ)
    assert len(args) == len(bound), (name, args)
    for a, b in zip(args, bound):
        if "*" in a or a.startswith("manner_hip_stream_t"):
            assert b in (_lib._P, C.POINTER(_lib._P)), (name, a)
        elif a.startswith("int64_t"):
            assert b is _lib._I64, (name, a)
        elif a.startswith("size_t"):
            assert b is _lib._SZ, (name, a)
        elif a.startswith("float"):
            assert b is C.c_float, (name, a)
        elif a.startswith("uint32_t"):
            assert b is C.c_uint32, (name, a)
        else:
            assert a.startswith("int32_t") and b is _lib._I32, (name, a)
    assert name in _lib.header_symbols()


def test_the_library_exports_the_entries_under_abi_8_and_checks_before_it_launches():
    lib = _lib.load()
    for name in EXPORTS:
        assert hasattr(lib, name)
    assert lib.manner_hip_abi_version() == 8 == _lib.ABI_VERSION
    p = 4096                                                        # a non-null address that is never dereferenced
    tab = (C.c_void_p * 16)(*([p] * 16))
    f0 = C.c_float(0.0)
    assert lib.manner_hip_caum_train_all_forward(p, p, tab, 3, 4, -1, 8, 8, 8, 8, 8, 2, f0, None, 7, p, p, 1 << 20, None) == 1
    assert b"caum_train_all: bad shape C=-1" in lib.manner_hip_last_error()
    assert lib.manner_hip_caum_train_all_forward(p, p, tab, 3, 257, 2, 8, 8, 8, 8, 8, 2, f0, None, 7, p, p, 1 << 20, None) == 1
    assert b"caum_train_all: S=257 unsupported (S <= 256)" in lib.manner_hip_last_error()
    assert lib.manner_hip_caum_train_all_forward(p, p, tab, 1 << 20, 256, 8, 8, 8, 8, 8, 8, 2, f0, None, 7, p, p, 1 << 20, None) == 1      # B C S = 2^31
    assert b"caum_train_all: B*C*S" in lib.manner_hip_last_error()
    assert lib.manner_hip_caum_train_all_backward(tab, p, 3, 4, -1, 8, 8, 8, 8, 8, 2, f0, None, 7, p, 1 << 20, p, p, tab, p, 1 << 20, None) == 1
    assert b"caum_train_all_backward: bad shape C=-1" in lib.manner_hip_last_error()
    assert lib.manner_hip_caum_train_all_forward(p, p, tab, 3, 4, 0, 8, 8, 8, 8, 8, 2, f0, None, 7, p, p, 0, None) == 0                     # no column: nothing to do
    assert lib.manner_hip_caum_train_all_forward(p, p, tab, 3, 4, 2, 8, 8, 8, 8, 8, 2, C.c_float(0.2), None, 7, p, p, 1 << 30, None) == 1   # p > 0 without seeds
    assert lib.manner_hip_caum_train_all_saved_bytes(3, 4, 0, 8, 8, 8, 8, 8, 2) == 0
    one, five = (lib.manner_hip_caum_train_all_saved_bytes(8, 50, c, 400, 400, 400, 400, 256, 16) for c in (1, 5))
    assert 0 < one < five <= 5 * one
    assert one >= lib.manner_hip_caum_user_saved_bytes(8, 50, 400, 400, 400, 400, 256, 16)
    # the row groups of the weight gradient depend on (R, K, O) alone: none for few rows, G O K floats of partial sums otherwise
    assert lib.manner_hip_wgrad_rows_f32_workspace_bytes(1, 4, 1) == 0 and lib.manner_hip_wgrad_rows_f32_workspace_bytes(33, 70, 33) == 0
    big = lib.manner_hip_wgrad_rows_f32_workspace_bytes(2100, 1600, 400)
    assert big > 0 and big % (1600 * 400 * 4) == 0 and 2 <= big // (1600 * 400 * 4) <= 64
    assert lib.manner_hip_wgrad_rows_f32(p, 1, p, 8, 5, 8, 2, p, 8, None, 0, None) == 1                                                   # ldy < O
    assert b"wgrad_rows_f32" in lib.manner_hip_last_error()
