"""Token-packed frozen-prefix store, CPU side: the header and the binding agree on the new exports, the size function agrees with a
hand count, the numpy model of reserve / store / gather (tests/prefix_packed_model.py — the GPU test holds the device to the same
model) returns what a dictionary keyed by real tokens returns, and the new switch is documented."""
import os
import re

import numpy as np
import pytest

from manner_amd import _lib, hip
from prefix_packed_model import PackedStoreModel, check_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["manner_hip_prefix_resolve", "manner_hip_prefix_store", "manner_hip_prefix_gather"]


@pytest.mark.parametrize("name", EXPORTS)
def test_header_declares_the_export_and_the_binding_matches_its_arguments(name):
    with open(_lib.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = re.findall(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text)
    assert len(protos) == 1, name
    args = [a.strip() for a in protos[0].split(",")]
    res, bound = _lib.SIGNATURES[name]
    assert len(args) == len(bound), (name, args)
    assert args[-1].startswith("manner_hip_stream_t")
    for a, b in zip(args, bound):                                   # pointers bind as pointers, 64-bit sizes as 64-bit
        if "*" in a or a.startswith("manner_hip_stream_t"):
            assert b is _lib._P, (name, a)
        elif a.startswith("int64_t"):
            assert b is _lib._I64, (name, a)
        else:
            assert a.startswith("int32_t") and b is _lib._I32, (name, a)
    assert name in _lib.header_symbols()


def test_the_library_exports_the_new_entry_points_under_the_same_abi_version():
    lib = _lib.load()
    for name in EXPORTS:
        assert hasattr(lib, name)
    assert lib.manner_hip_abi_version() == _lib.ABI_VERSION


def test_size_function_agrees_with_a_hand_count():
    # 100 rows -> 256 hash slots of 20 bytes (two 8-byte key words and a 4-byte row) + the 4-byte row counter; 16 bytes of row
    # metadata (8-byte offset, 4-byte length, 4-byte scratch) + the 8-byte token counter; 1000 tokens of 32 f32
    b = hip.prefix_cache_bytes(32, 100, pool_tokens=1000)
    assert b == {"payload": 1000 * 32 * 4, "rows": 100 * 16 + 8, "slots": 256 * 20 + 4, "total": 128000 + 1608 + 5124}
    # the seeded 65 238-news pool at bert-base width: 2 x 65 238 rounds up to 131 072 slots
    b = hip.prefix_cache_bytes(768, 65238, pool_tokens=5863594)
    assert b["payload"] == 5863594 * 3072 and b["rows"] == 65238 * 16 + 8 and b["slots"] == 131072 * 20 + 4
    assert b["total"] == 18012960768 + 1043816 + 2621444
    # the fixed-width table the same function prices for the comparison
    p = hip.prefix_cache_bytes(768, 65238, max_len=512)
    assert p == {"payload": 65238 * 512 * 3072, "rows": 0, "slots": 131072 * 20 + 4, "total": 102610501632 + 2621444}
    with pytest.raises(ValueError):
        hip.prefix_cache_bytes(768, 10)
    with pytest.raises(ValueError):
        hip.prefix_cache_bytes(768, 10, pool_tokens=5, max_len=5)


def test_seeded_title_abstract_pool_costs_its_real_tokens():
    """The figure the issue asks for: the title+abstract profile capped at 512, 65 238 news, seed 42."""
    from manner_amd.synth import synth_lengths
    lens = synth_lengths(65238, 42, 512, "title_abstract")
    assert int(lens.sum()) == 5863594 and int(lens.max()) <= 512
    packed = hip.prefix_cache_bytes(768, 65238, pool_tokens=int(lens.sum()))["total"]
    padded = hip.prefix_cache_bytes(768, 65238, max_len=512)["total"]
    print(f"bytes per news: packed {packed / 65238:.0f}, padded to 512 {padded / 65238:.0f}, ratio {padded / packed:.3f}")
    assert (packed, padded) == (18016626028, 102613123076)          # 276 KB against 1.57 MB per news: 5.70x, recorded, not a bar


def _encode(hidden):
    """A stand-in encoder: a row's hidden states are a function of its own tokens (and positions) only."""
    def enc(rows):
        out = []
        for t in rows:
            g = np.random.default_rng([len(t)] + list(t))
            out.append(g.standard_normal((len(t), hidden)).astype(np.float32))
        return out
    return enc


def _draw(g, pool, n, width):
    pick = g.integers(0, len(pool), n)
    pick[::7] = pick[1]                                             # duplicates inside the call
    rows = [pool[i] for i in pick]
    return rows, max(width, max(len(r) for r in rows))


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_model_returns_what_a_dictionary_keyed_by_real_tokens_returns(order):
    hidden = 8
    g = np.random.default_rng(3)
    pool = [tuple(int(x) for x in g.integers(1, 50, int(ln))) for ln in g.integers(5, 301, 120)]
    pool += [pool[3][:-1], pool[3] + (7,)]                          # a prefix and an extension of a stored news are other news
    total = sum(len(t) for t in set(pool))
    model = PackedStoreModel(hidden, capacity_rows=110, pool_tokens=total // 2)          # the pool fills up; later so does the table
    enc = _encode(hidden)
    truth = {}
    reserve = {"ascending": None, "descending": lambda k: range(k - 1, -1, -1),
               "shuffled": lambda k: np.random.default_rng(k).permutation(k)}[order]
    filled_mid_batch = served = 0
    for step, (n, width) in enumerate(((30, 0), (30, 300), (17, 40), (64, 129), (64, 512), (40, 0), (64, 128), (64, 300), (64, 0))):
        rows, lp = _draw(g, pool, n, width)
        before = (model.row_len == -2).sum(), (model.row_len >= 1).sum()
        out, todo = model.hidden_states(rows, lp, enc, reserve)
        after = (model.row_len == -2).sum(), (model.row_len >= 1).sum()
        filled_mid_batch += int(after[0] > before[0] and after[1] > before[1])
        served += n - len(todo)
        for t, o in zip(rows, out):
            want = truth.setdefault(t, enc([t])[0])
            assert np.array_equal(o[:len(t)], want) and not o[len(t):].any(), step
        # only what has no payload was encoded: first occurrences of new keys, every occurrence of a key without payload
        assert len(set(todo.tolist())) == len(todo) and model.tok_count <= model.pool_tokens
        check_layout(model.row_off, model.row_len, model.tok_count, model.pool_tokens, model.row_count)
    assert filled_mid_batch >= 1 and served > 0 and model.row_count > model.capacity
    stored, none = check_layout(model.row_off, model.row_len, model.tok_count, model.pool_tokens, model.row_count)
    assert stored > 0 and none > 0
    # an all-hit call of stored news encodes nothing and reads the pool only
    kept = [t for t, r in model.row_of.items() if r >= 0 and model.row_len[r] >= 1][:20]
    out, todo = model.hidden_states(kept, 512, lambda rows: pytest.fail("encoded a stored news") if rows else [])
    assert len(todo) == 0 and all(np.array_equal(o[:len(t)], truth[t]) for t, o in zip(kept, out))


def test_new_switch_is_in_the_design_table_and_off_by_default():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    section = text[text.index("## 7. Switches"):text.index("## 7a.")]
    assert "MANNER_PREFIX_CACHE_TOKENS" in section
    from manner_amd.models.components.news_encoder import MannerTextEncoder
    assert MannerTextEncoder.prefix_cache_tokens == int(os.environ.get("MANNER_PREFIX_CACHE_TOKENS", "0"))
    assert hasattr(hip, "PackedPrefixCache") and issubclass(hip.PackedPrefixCache, hip.NewsEmbeddingCache)


def test_entry_points_refuse_bad_arguments_with_a_message():
    """Checked before anything is launched, so no device is needed: null pointers, padded_len outside [1, 512], hidden not a
    multiple of 4, negative sizes -> MANNER_HIP_E_INVALID and a message naming the entry point."""
    lib = _lib.load()
    p = 4096                                                        # any non-null, 16-byte aligned address: never dereferenced

    def store(fresh=p, n_new=1, n=1, lp=16, hidden=8, pool=p, pool_tokens=64, cap=4):
        return lib.manner_hip_prefix_store(fresh, n_new, None, n, p, p, p, lp, hidden, pool, pool_tokens, cap, p, p, p, p, p, None)

    def gather(rows=p, n=1, lp=16, hidden=8, pool=p, pool_tokens=64, cap=4, out=p, n_fresh=0):
        return lib.manner_hip_prefix_gather(rows, p, n, lp, hidden, pool, pool_tokens, cap, p, p, p, None, n_fresh, None, out, None)

    cases = [(store, dict(fresh=None)), (store, dict(pool=None)), (store, dict(lp=0)), (store, dict(lp=513)), (store, dict(hidden=6)),
             (store, dict(n_new=-1)), (store, dict(pool_tokens=-1)), (store, dict(cap=-1)), (store, dict(n_new=2, n=1)),
             (store, dict(pool=p + 4)),
             (gather, dict(rows=None)), (gather, dict(out=None)), (gather, dict(lp=0)), (gather, dict(lp=513)), (gather, dict(hidden=2)),
             (gather, dict(n=-1)), (gather, dict(n_fresh=-1)), (gather, dict(out=p + 8))]
    for fn, bad in cases:
        assert fn(**bad) == 1, (fn.__name__, bad)                   # MANNER_HIP_E_INVALID
        assert ("prefix_" + fn.__name__).encode() in lib.manner_hip_last_error(), bad
    assert lib.manner_hip_prefix_resolve(None, p, 3, p, 4, None) == 1 and b"prefix_resolve" in lib.manner_hip_last_error()
    assert lib.manner_hip_prefix_resolve(p, p, -1, p, 4, None) == 1
    # empty calls are legal and touch nothing
    assert store(n_new=0, n=0) == 0 and gather(n=0) == 0 and lib.manner_hip_prefix_resolve(None, None, 0, None, 4, None) == 0
