"""A-Module batches, CPU side: the numpy restatement of the M-per-class rule (tests/news_sample_ref.py — the GPU test holds the
device to it bit for bit) has the properties of MPerClassSampler's documented behaviour, each of four planted defects breaks one
of the asserted quantities, and the header, the binding and the built library agree on the new entry point under ABI 8."""
import ctypes as C
import re

import numpy as np
import pytest

import news_sample_ref as ref
from manner_amd import _lib
from manner_amd.data.components import mind_news_dataset as mnd
from train_sample_ref import key as real_key

SEED = 42
EXPORT = "manner_hip_sample_m_per_class"
# (n, m, units, the 99.9 % point of chi-square with n - 1 degrees of freedom)
INCLUSION = ((25, 20, 4000, 51.2), (21, 20, 4000, 45.3), (300, 20, 4000, 380.3), (65, 64, 4000, 104.7), (7, 1, 4000, 22.5))


# ---------------------------------------------------------------------------------------------- the asserted quantities
def _chi2(counts, trials, m):
    """Inclusion counts of ``trials`` draws of m out of n, normalised to chi-square with n - 1 degrees of freedom.  Without
    replacement the indicator of a member has variance p (1 - p), p = m / n, and covariance -p (1 - p) / (n - 1) with another's:
    sum (c - E)^2 / (E (1 - p)) * (n - 1) / n.  With replacement (m > n) it is Pearson's statistic of trials * m multinomial draws."""
    n = counts.size
    exp = trials * m / n
    if m > n:
        return float((((counts - exp) ** 2) / exp).sum())
    return float((((counts - exp) ** 2) / (exp * (1 - m / n))).sum() * (n - 1) / n)


def check_blocks_are_distinct_and_in_range():
    for n, m in ((25, 20), (21, 20), (20, 20), (300, 20), (65, 64), (64, 64), (7, 1), (1, 1), (257, 256), (100000, 20)):
        for unit in range(100):
            d = ref.draw(n, m, SEED, 0, unit)
            assert d.shape == (m,) and d.min() >= 0 and d.max() < n, (n, m, unit)
            assert np.unique(d).size == m, (n, m, unit)
    for n, m in ((5, 20), (1, 3), (19, 20)):                         # fewer members than slots: in range, with repeats
        for unit in range(100):
            d = ref.draw(n, m, SEED, 0, unit)
            assert d.shape == (m,) and d.min() >= 0 and d.max() < n


def check_inclusion_is_uniform():
    stats = {}
    for n, m, units, bound in INCLUSION:
        counts = np.zeros(n)
        for unit in range(units):
            counts[ref.draw(n, m, SEED, 0, unit)] += 1
        stats[(n, m)] = (_chi2(counts, units, m), bound)
    counts = np.zeros(5)                                             # with replacement: n = 5, m = 20
    for unit in range(4000):
        np.add.at(counts, ref.draw(5, 20, SEED, 0, unit), 1)
    stats[(5, 20)] = (_chi2(counts, 4000, 20), 18.5)
    counts = np.zeros(18)                                            # class choice: L = 18, k = 3 over 6000 batches
    for b in range(6000):
        c = ref.choose_classes(18, 3, SEED, 0, b)
        assert np.unique(c).size == 3 and c.min() >= 0 and c.max() < 18
        counts[c] += 1
    stats["classes"] = (_chi2(counts, 6000, 3), 40.8)
    print("chi-square (bound): " + ", ".join(f"{k}: {v:.1f} ({b})" for k, (v, b) in stats.items()))
    for k, (v, b) in stats.items():
        assert v < b, (k, v, b)


def _equal_classes(n_classes, n):
    return ref.class_tables(np.repeat(np.arange(n_classes) * 3 + 1, n))      # labels 1, 4, 7, ...: a label is not its class number


def check_blocks_of_a_batch_draw_independently():
    """Four classes of 25 members, k = 3 blocks of m = 20: no two blocks of a batch hold the same positions of their classes (two
    independent draws coincide with probability 5! / 25!)."""
    tables = _equal_classes(4, 25)
    for b in range(200):
        idx, lab = ref.sample_batch(tables, 20, 3, SEED, 0, b)
        pos = (idx % 25).reshape(3, 20)
        assert np.unique(lab.reshape(3, 20)[:, 0]).size == 3
        for i in range(3):
            for j in range(i):
                assert not np.array_equal(pos[i], pos[j]), (b, i, j)


def check_draws_are_independent_of_the_class_choice():
    """k = 1, 18 classes of 5 members, m = 20 draws with replacement: the draw in the slot whose number is the chosen class is
    uniform over the 5 members (4 degrees of freedom, 6000 batches).  Keys shared between the two streams would make it the
    smallest of 18."""
    tables = _equal_classes(18, 5)
    counts = np.zeros(5)
    for b in range(6000):
        idx, lab = ref.sample_batch(tables, 20, 1, SEED, 0, b)
        c = int((lab[0] - 1) // 3)
        assert (idx // 5 == c).all()                                 # every drawn member has the block's label
        counts[idx[c] % 5] += 1
    stat = _chi2(counts, 6000 // 20, 20)                             # 6000 single draws
    print(f"slot-of-class draw: {stat:.1f} (18.5)")
    assert stat < 18.5, stat


# ---------------------------------------------------------------------------------------------- the restatement
def test_blocks_are_distinct_and_in_range():
    check_blocks_are_distinct_and_in_range()


def test_inclusion_and_class_choice_are_uniform():
    check_inclusion_is_uniform()


def test_blocks_of_a_batch_draw_independently():
    check_blocks_of_a_batch_draw_independently()


def test_draws_are_independent_of_the_class_choice():
    check_draws_are_independent_of_the_class_choice()


def test_epoch_shape_labels_and_the_three_value_errors():
    g = np.random.default_rng(3)
    labels = g.choice([2, 3, 5, 7, 11], 127, p=[0.5, 0.2, 0.2, 0.08, 0.02])
    idx, lab = ref.sample_epoch(labels, 4, 12, SEED, 1)
    assert idx.shape == lab.shape == (127 // 12, 12) and idx.min() >= 0 and idx.max() < 127
    assert np.array_equal(labels[idx], lab)                          # every drawn member has the block's label
    blocks = lab.reshape(-1, 3, 4)
    assert (blocks == blocks[:, :, :1]).all()                        # a block is one class ...
    assert all(np.unique(b[:, 0]).size == 3 for b in blocks)         # ... and a batch k distinct ones
    again = ref.sample_epoch(labels, 4, 12, SEED, 1)
    assert np.array_equal(idx, again[0]) and not np.array_equal(idx, ref.sample_epoch(labels, 4, 12, SEED, 2)[0])
    assert not np.array_equal(idx, ref.sample_epoch(labels, 4, 12, SEED + 1, 1)[0])
    assert ref.sample_epoch(labels[:12], 4, 12, SEED, 0)[0].shape == (1, 12)
    with pytest.raises(ValueError, match="fewer news"):
        ref.sample_epoch(labels[:11], 4, 12, SEED, 0)
    with pytest.raises(ValueError, match="multiple"):
        ref.sample_epoch(labels, 5, 12, SEED, 0)
    with pytest.raises(ValueError, match="too few classes"):
        ref.sample_epoch(labels, 2, 12, SEED, 0)                     # 2 * 5 classes < 12


class _FakeDataset:
    """What DeviceNewsTrainSampler looks at before it touches a device."""

    def __init__(self, labels):
        self.labels = np.asarray(labels, np.int64)
        self.class_label, self.class_off, self.class_members = mnd.class_tables(self.labels)

    def __len__(self):
        return self.labels.size


def test_the_sampler_raises_the_same_value_errors_on_the_host_and_counts_the_epoch():
    labels = np.random.default_rng(3).integers(0, 5, 127)
    s = mnd.DeviceNewsTrainSampler(None, _FakeDataset(labels), 4, 12, seed=1)
    assert len(s) == 10 and (s.m, s.k) == (4, 3)
    with pytest.raises(ValueError, match="fewer than one batch"):
        mnd.DeviceNewsTrainSampler(None, _FakeDataset(labels[:11]), 4, 12)
    with pytest.raises(ValueError, match="not a multiple"):
        mnd.DeviceNewsTrainSampler(None, _FakeDataset(labels), 5, 12)
    with pytest.raises(ValueError, match="cannot fill"):
        mnd.DeviceNewsTrainSampler(None, _FakeDataset(labels), 2, 12)
    with pytest.raises(ValueError, match="samples_per_class <= 256"):
        mnd.DeviceNewsTrainSampler(None, _FakeDataset(np.arange(600) % 2), 257, 514)
    with pytest.raises(RuntimeError, match="sample_epoch"):
        s.batch(0)
    with pytest.raises(ValueError, match="aspect"):
        mnd.NewsDataset(None, None, "topic")


def test_the_package_builds_the_class_tables_of_the_restatement():
    g = np.random.default_rng(9)
    for labels in (g.integers(-3, 40, 500), np.array([7]), np.array([5, 5, 5, 2])):
        a, b = mnd.class_tables(labels), ref.class_tables(labels)
        assert a[0].dtype == np.int64 and a[1].dtype == np.int64 and a[2].dtype == np.int32
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        for l in range(a[0].size):
            mem = a[2][a[1][l]:a[1][l + 1]]
            assert (np.diff(mem) > 0).all() and (np.asarray(labels)[mem] == a[0][l]).all()


# ---------------------------------------------------------------------------------------------- planted defects
def _draw_with(defect):
    def draw(n, m, seed, epoch, unit):
        h = real_key(seed, epoch, unit, 17, np.arange(m)) >> np.uint64(32)
        if n < m:
            return ((h * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
        out = []
        for t in range(m):
            J = n - m + t - (1 if defect == "J" else 0)
            r = int((h[t] * np.uint64(J + 1)) >> np.uint64(32))
            out.append(J if (r in out and defect != "membership") else r)
        return np.asarray(out, np.int64)
    return draw


def test_the_unplanted_copy_of_the_draw_is_the_restatement():
    for n, m in ((25, 20), (20, 20), (5, 20), (300, 64)):
        assert np.array_equal(_draw_with(None)(n, m, SEED, 3, 11), ref.draw(n, m, SEED, 3, 11))


@pytest.mark.parametrize("defect", ["J", "membership"])
def test_a_planted_defect_in_floyds_step_breaks_distinctness_and_uniformity(defect, monkeypatch):
    monkeypatch.setattr(ref, "draw", _draw_with(defect))
    with pytest.raises(AssertionError):
        check_blocks_are_distinct_and_in_range()
    with pytest.raises(AssertionError):
        check_inclusion_is_uniform()


def test_one_unit_per_batch_makes_the_blocks_of_a_batch_draw_alike(monkeypatch):
    monkeypatch.setattr(ref, "key", lambda seed, epoch, imp, stream, slot: real_key(seed, epoch, imp // 3 if stream == 17 else imp,
                                                                                     stream, slot))       # unit = b at k = 3
    check_blocks_are_distinct_and_in_range()                         # (a defect the per-block properties do not see)
    with pytest.raises(AssertionError):
        check_blocks_of_a_batch_draw_independently()


def test_stream_16_reused_for_the_draws_ties_them_to_the_class_choice(monkeypatch):
    monkeypatch.setattr(ref, "key", lambda seed, epoch, imp, stream, slot: real_key(seed, epoch, imp, 16, slot))
    check_blocks_are_distinct_and_in_range()
    with pytest.raises(AssertionError):
        check_draws_are_independent_of_the_class_choice()


# ---------------------------------------------------------------------------------------------- header, binding, library
def test_header_declares_the_entry_point_and_the_binding_matches_its_arguments():
    with open(_lib.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = re.findall(r"\bint\s+" + EXPORT + r"\s*\(([^;]*?)\)\s*;", text)
    assert len(protos) == 1
    args = [a.strip() for a in protos[0].split(",")]
    res, bound = _lib.SIGNATURES[EXPORT]
    assert res is C.c_int and len(args) == len(bound) == 20, args
    assert args[-1].startswith("manner_hip_stream_t")
    for a, b in zip(args, bound):
        if "*" in a or a.startswith("manner_hip_stream_t"):
            assert b is _lib._P, a
        elif a.startswith("int64_t"):
            assert b is _lib._I64, a
        elif a.startswith("uint64_t"):
            assert b is C.c_uint64, a
        else:
            assert a.startswith("int32_t") and b is _lib._I32, a
    assert EXPORT in _lib.header_symbols()


def test_the_library_exports_the_entry_point_under_abi_8_and_refuses_bad_arguments_before_launch():
    lib = _lib.load()
    assert hasattr(lib, EXPORT) and lib.manner_hip_abi_version() == 8 == _lib.ABI_VERSION
    p = 4096                                                         # a non-null address that is never dereferenced
    fn = lib.manner_hip_sample_m_per_class

    def call(L=18, N=1000, n_news=1000, m=20, k=3, nb=16, rows=p, out_width=p):
        return fn(p, p, p, L, N, rows, p, None, n_news, m, k, nb, 0, 0, p, p, p, out_width, None, None)

    # checked before anything is launched, so no device is needed
    for kw, text in ((dict(m=257, N=10 ** 6), b"m = 257"), (dict(m=0), b"m = 0"), (dict(L=1025, k=3), b"L = 1025"), (dict(L=0), b"L = 0"),
                     (dict(k=19), b"k = 19"), (dict(k=0), b"k = 0"), (dict(N=2 ** 31), b"bad argument"), (dict(N=0), b"bad argument"),
                     (dict(nb=-1), b"bad argument"), (dict(n_news=0), b"bad argument"),
                     (dict(k=2 ** 31 - 1, m=256), b"k = 2147483647"),                  # k * m overflows int32: refused as k > L
                     (dict(L=1024, k=1024, m=256, nb=2 ** 13), b"overflows"),          # nb * k * m = 2^31
                     (dict(nb=2 ** 62), b"overflows"),                                 # nb * k * m overflows int64
                     (dict(rows=None), b"null argument"), (dict(out_width=None), b"null argument")):
        assert call(**kw) == 1, kw
        assert text in lib.manner_hip_last_error(), (kw, lib.manner_hip_last_error())
    assert call(nb=0, rows=None, out_width=None) == 0                # an empty epoch is legal and touches nothing
