"""Training batches, CPU side: the numpy restatement of the sampling rule (tests/train_sample_ref.py — the GPU test holds the
device to it bit for bit) draws the distribution of the reference's MINDRecDatasetTrain, ``plan_train_batch`` sizes a batch as
the restatement does, and the header, the binding and the built library agree on the new entry points under ABI 8."""
import re

import numpy as np
import pytest

from manner_amd import _lib
from manner_amd.data.components.mind_rec_dataset import ParsedBehaviors, click_counts, plan_train_batch
from train_sample_ref import key, mix, sample

EXPORTS = ["manner_hip_sample_candidates", "manner_hip_gather_segments", "manner_hip_rows_max_len"]


def test_mix_and_key_are_the_stated_arithmetic_modulo_2_to_64():
    M = 1 << 64

    def mix_int(x):
        x ^= x >> 30
        x = x * 0xBF58476D1CE4E5B9 % M
        x ^= x >> 27
        x = x * 0x94D049BB133111EB % M
        return x ^ (x >> 31)

    for x in (0, 1, 0x9E3779B97F4A7C15, M - 1, 123456789012345678):
        assert int(mix(np.uint64(x))) == mix_int(x)
    for seed, epoch, imp, stream, slot in ((42, 0, 0, 0, 0), (0, 19999, 7, 2, 1499), (M - 1, 3, 123456, 1, 5)):
        want = mix_int(mix_int(mix_int((seed + 0x9E3779B97F4A7C15 * (epoch + 1)) % M) ^ imp) ^ (stream << 32 | slot))
        assert int(key(seed, epoch, imp, stream, np.array([slot]))[0]) == want
    # splitmix64's first output for state 0 (the published test vector of this finaliser: mix(0 + golden))
    assert int(mix(np.uint64(0x9E3779B97F4A7C15))) == 0xE220A8397B1DCDAF


def test_the_rule_draws_the_reference_distribution():
    """The three experiments of the issue at seed 42, 20 000 epochs each: every negative is included equally often, the first
    output slot holds each element of the list equally often (so each positive 1/6 and each negative 4/6 / 10 of the time), and
    draws with replacement are uniform.  Bounds: the p = 0.001 points of chi-square with 9, 11 and 2 degrees of freedom."""
    epochs = 20000
    lab = np.zeros(12, np.float32)
    lab[[1, 5]] = 1                                                  # p = 2, q = 10, ratio 2: 4 of 10 negatives, no replacement
    neg = np.flatnonzero(lab == 0)
    included, first = np.zeros(12), np.zeros(12)
    for e in range(epochs):
        s = sample(lab, 2, 42, e, 0)
        assert s.size == 6 and (s == 1).sum() == 1 and (s == 5).sum() == 1          # every positive in every output
        included[s] += 1
        first[s[0]] += 1
    exp = epochs * 4 / 10
    chi_incl = float((((included[neg] - exp) ** 2) / exp).sum())
    exp_first = np.where(lab == 1, epochs / 6, epochs * (4 / 6) / 10)
    chi_first = float((((first - exp_first) ** 2) / exp_first).sum())
    lab2 = np.array([0, 1, 0, 1, 0], np.float32)                    # p = 2, q = 3, ratio 4: 8 draws from 3 negatives
    drawn = np.zeros(5)
    for e in range(epochs):
        s = sample(lab2, 4, 42, e, 0)
        assert s.size == 10 and (s == 1).sum() == 1 and (s == 3).sum() == 1
        np.add.at(drawn, s, 1)
    exp2 = epochs * 8 / 3
    chi_repl = float((((drawn[[0, 2, 4]] - exp2) ** 2) / exp2).sum())
    print(f"chi-square: inclusion {chi_incl:.2f} (9 dof), first slot {chi_first:.2f} (11 dof), with replacement {chi_repl:.2f} (2 dof)")
    assert chi_incl < 27.88 and chi_first < 31.26 and chi_repl < 13.82


def _random_labels(g, n):
    lab = (g.random(n) < g.choice([0.05, 0.3, 0.7])).astype(np.float32)
    if n > 2 and g.random() < 0.3:
        lab[g.integers(0, n)] = 0.5                                  # neither clicked nor non-clicked
    return lab


def test_structure_of_a_sample_over_random_impressions():
    g = np.random.default_rng(5)
    seen_repl = seen_norepl = seen_empty = 0
    for imp in range(300):
        n = int(g.integers(1, 80))
        lab = _random_labels(g, n)
        ratio = int(g.choice([1, 2, 4]))
        pos, neg = np.flatnonzero(lab == 1), np.flatnonzero(lab == 0)
        p, q, m = pos.size, neg.size, ratio * pos.size
        if p > 0 and q == 0:
            with pytest.raises(ValueError):
                sample(lab, ratio, 9, 1, imp)
            continue
        s = sample(lab, ratio, 9, 1, imp)
        if p == 0:
            assert s.size == 0
            seen_empty += 1
            continue
        assert s.size == p + m and s.min() >= 0 and s.max() < n
        is_pos = lab[s] == 1
        assert np.array_equal(np.sort(s[is_pos]), pos)               # every positive exactly once
        chosen = s[~is_pos]
        assert chosen.size == m and (lab[chosen] == 0).all()         # m negatives, each a real non-clicked position
        if m <= q:
            assert np.unique(chosen).size == m
            seen_norepl += 1
        else:
            seen_repl += 1
        assert np.array_equal(s, sample(lab, ratio, 9, 1, imp))      # a pure function of its arguments
    assert seen_repl > 20 and seen_norepl > 20 and seen_empty > 5


def _behaviors(label_lists, g, n_news=50):
    cand_off = np.concatenate([[0], np.cumsum([len(l) for l in label_lists])]).astype(np.int64)
    hs = g.integers(0, 6, len(label_lists))
    hist_off = np.concatenate([[0], np.cumsum(hs)]).astype(np.int64)
    return ParsedBehaviors(users=np.arange(len(label_lists), dtype=np.int64),
                           hist_rows=g.integers(0, n_news, int(hist_off[-1])).astype(np.int32), hist_off=hist_off,
                           cand_rows=g.integers(0, n_news, int(cand_off[-1])).astype(np.int32), cand_off=cand_off,
                           labels=np.concatenate(label_lists).astype(np.float32) if label_lists else np.zeros(0, np.float32))


def test_plan_train_batch_sizes_a_batch_as_the_restatement_does():
    g = np.random.default_rng(11)
    labs = []
    while len(labs) < 60:
        lab = _random_labels(g, int(g.integers(1, 40)))
        if not ((lab == 1).any() and not (lab == 0).any()):
            labs.append(lab)
    labs[7] = np.zeros(0, np.float32)                                # an impression without candidates
    labs[8] = np.array([1, 0.5, 0, 0.5], np.float32)                 # 0.5 is in neither class
    bhv = _behaviors(labs, g)
    p_all, q_all = click_counts(bhv)
    assert p_all[8] == 1 and q_all[8] == 1 and p_all[7] == 0 and q_all[7] == 0
    assert np.array_equal(p_all, [int((l == 1).sum()) for l in labs]) and np.array_equal(q_all, [int((l == 0).sum()) for l in labs])
    for ratio, idx in ((1, range(0, 60)), (4, [8, 7, 8, 59, 0, 3]), (4, g.permutation(60)[:17]), (2, [])):
        plan = plan_train_batch(bhv, idx, ratio)
        idx = np.asarray(list(idx), np.int64)
        sizes = [sample(labs[i], ratio, 3, 0, int(i)).size for i in idx]
        assert np.array_equal(plan.out_off, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
        assert np.array_equal(plan.indices, idx) and np.array_equal(plan.m, ratio * plan.p)
        assert np.array_equal(plan.hist_off, np.concatenate([[0], np.cumsum(bhv.hist_off[idx + 1] - bhv.hist_off[idx])]))
        assert plan.cand_max == (max(sizes) if sizes else 0)
        assert plan.hist_max == (int(np.diff(plan.hist_off).max()) if idx.size else 0)
    with pytest.raises(IndexError):
        plan_train_batch(bhv, [0, 60], 4)


def test_plan_train_batch_refuses_clicks_without_negatives_before_any_launch():
    g = np.random.default_rng(12)
    bhv = _behaviors([np.array([1, 0, 0], np.float32), np.array([1, 1, 0.5], np.float32), np.array([0, 0], np.float32)], g)
    plan_train_batch(bhv, [0, 2], 4)
    with pytest.raises(ValueError, match="impression 1"):
        plan_train_batch(bhv, [0, 1], 4)


def test_width_bounds_cover_every_candidate_of_the_clicked_impressions():
    from manner_amd.data.components.mind_rec_dataset import impression_widths
    g = np.random.default_rng(13)
    labs = [np.array([1, 0, 0, 0], np.float32), np.array([0, 0, 0], np.float32), np.array([0, 1, 0], np.float32)]
    bhv = _behaviors(labs, g)
    lengths, ents = g.integers(2, 90, 50).astype(np.int32), g.integers(0, 6, 50).astype(np.int32)
    w = impression_widths(bhv, lengths, ents)
    for i in range(3):
        c = bhv.cand_rows[bhv.cand_off[i]:bhv.cand_off[i + 1]]
        h = bhv.hist_rows[bhv.hist_off[i]:bhv.hist_off[i + 1]]
        assert w["cand_text"][i] == lengths[c].max() and w["cand_ent"][i] == ents[c].max()
        assert w["hist_text"][i] == (lengths[h].max() if h.size else 0)
    plan = plan_train_batch(bhv, [2, 1, 0], 2, w)
    assert plan.cand_text_bound == max(w["cand_text"][0], w["cand_text"][2])      # impression 1 has no click: it contributes nothing
    assert plan.cand_ent_bound == max(w["cand_ent"][0], w["cand_ent"][2])
    assert plan.hist_text_width == w["hist_text"].max() and plan.hist_ent_width == w["hist_ent"].max()


@pytest.mark.parametrize("name", EXPORTS)
def test_header_declares_the_entry_point_and_the_binding_matches_its_arguments(name):
    with open(_lib.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = re.findall(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text)
    assert len(protos) == 1, name
    args = [a.strip() for a in protos[0].split(",")]
    res, bound = _lib.SIGNATURES[name]
    assert len(args) == len(bound), (name, args)
    assert args[-1].startswith("manner_hip_stream_t")
    import ctypes as C
    for a, b in zip(args, bound):
        if "*" in a or a.startswith("manner_hip_stream_t"):
            assert b is _lib._P, (name, a)
        elif a.startswith("int64_t"):
            assert b is _lib._I64, (name, a)
        elif a.startswith("uint64_t"):
            assert b is C.c_uint64, (name, a)
        else:
            assert a.startswith("int32_t") and b is _lib._I32, (name, a)
    assert name in _lib.header_symbols()


def test_the_library_exports_the_entry_points_under_abi_8_and_refuses_bad_arguments():
    lib = _lib.load()
    for name in EXPORTS:
        assert hasattr(lib, name)
    assert lib.manner_hip_abi_version() == 8 == _lib.ABI_VERSION
    p = 4096                                                        # a non-null address that is never dereferenced
    # checked before anything is launched, so no device is needed
    assert lib.manner_hip_sample_candidates(p, p, p, 4, 9, None, p, -1, p, 5, 4, 0, 0, p, p, None, None, None, None) == 1
    assert b"sample_candidates" in lib.manner_hip_last_error()
    assert lib.manner_hip_sample_candidates(p, p, None, 4, 9, None, p, 2, p, 5, 4, 0, 0, p, p, None, None, None, None) == 1
    assert lib.manner_hip_sample_candidates(p, p, p, 4, 9, p, p, 2, p, 5, 4, 0, 0, p, p, None, None, None, None) == 1   # users without out_users
    assert lib.manner_hip_sample_candidates(p, p, p, 4, 9, None, p, 2, p, 5, 4, 0, 0, None, p, None, None, None, None) == 1
    assert lib.manner_hip_gather_segments(p, None, p, 4, 9, p, -1, p, 5, p, None, None, None) == 1
    assert b"gather_segments" in lib.manner_hip_last_error()
    assert lib.manner_hip_gather_segments(p, p, p, 4, 9, p, 2, p, 5, p, None, None, None) == 1                          # src_f without out_f
    assert lib.manner_hip_gather_segments(None, None, p, 4, 9, p, 2, p, 5, p, None, None, None) == 1
    assert lib.manner_hip_rows_max_len(p, None, 4, p, 3, None, None) == 1 and b"rows_max_len" in lib.manner_hip_last_error()
    # empty batches are legal and touch nothing
    assert lib.manner_hip_sample_candidates(None, None, None, 0, 0, None, None, 0, None, 0, 4, 0, 0, None, None, None, None, None, None) == 0
    assert lib.manner_hip_gather_segments(None, None, None, 0, 0, None, 0, None, 0, None, None, None, None) == 0
