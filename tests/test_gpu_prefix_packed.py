"""Token-packed frozen-prefix store on the device (csrc/cache.hip manner_hip_prefix_*, hip.PackedPrefixCache,
MannerTextEncoder.prefix_cache_tokens).  Run on the MI355X box: ``pytest -m gpu``.

The store must never change a number: whatever it returns is compared with ``engine.encode_hidden`` on the same batch by
``torch.equal``; its bookkeeping is compared with the numpy model of tests/prefix_packed_model.py."""
import dataclasses
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from manner_amd import _lib, hip  # noqa: E402
from manner_amd.config import PRESETS  # noqa: E402
from manner_amd.models.components.news_encoder import MannerTextEncoder  # noqa: E402
from manner_amd.synth import synth_lengths, synth_news_tokens  # noqa: E402
from manner_amd.weights import make_plm_weights  # noqa: E402
from prefix_packed_model import PackedStoreModel, check_layout  # noqa: E402

DEV = "cuda:0"
WIDTHS = (40, 128, 129, 300, 512)
POOL_LENS = np.array([5, 9, 17, 23, 31, 40, 40, 12, 64, 100, 127, 128, 128, 77, 129, 130, 200, 256, 257, 300, 300, 299, 301, 400,
                      480, 511, 512, 512])


def _cfg(name):
    return dataclasses.replace(PRESETS["bert-base-uncased"], layers=2) if name == "bert-base-2-layers" else PRESETS[name]


def _engine(name, seed, precisions):
    cfg = _cfg(name)
    w = make_plm_weights(cfg, seed=seed, std=0.02 if cfg.hidden > 128 else 0.05, with_pooler=False)
    return cfg, hip.HipEncoder(cfg, w, precisions=precisions, device=DEV)


def _batch(ids, mask, pick, width):
    pick = np.asarray(pick)
    assert int(mask[pick].sum(1).max()) <= width
    return (torch.from_numpy(ids[pick][:, :width].copy()).to(DEV), torch.from_numpy(mask[pick][:, :width].copy()).to(DEV))


def _tokens(ids, mask, pick):
    return [tuple(int(t) for t in ids[i][mask[i] == 1]) for i in pick]


def _zeros(hidden):
    return lambda rows: [np.zeros((len(t), hidden), np.float32) for t in rows]


def _check(cache, engine, b, prec, model=None, tokens=None):
    """hidden_states == encode_hidden to the bit, zeros at padded positions; returns the rows this call encoded."""
    before = cache.encoded
    got = cache.hidden_states(engine, b[0], b[1], 1, prec)
    want = engine.encode_hidden(b[0], b[1], 1, precision=prec)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got, want)
    assert not bool((got * (b[1] == 0).unsqueeze(2)).count_nonzero())            # exactly zero (and no NaN) where the mask is 0
    assert not bool(torch.isnan(got).any())
    if model is not None:
        model.hidden_states(tokens, b[0].shape[1], _zeros(cache.hidden))
        assert (model.lookups, model.encoded) == (cache.lookups, cache.encoded)
    return cache.encoded - before


# ------------------------------------------------------------------------------------------------ 1. the same bits as the engine
@pytest.mark.parametrize("prec", ["fp32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["tiny-bert-512", "tiny-roberta-514", "bert-base-2-layers"])
def test_hidden_states_equal_the_engine_bit_for_bit(name, prec):
    cfg, engine = _engine(name, 31, (prec,))
    ids, mask = synth_news_tokens(len(POOL_LENS), cfg, seed=31, lengths=POOL_LENS, pad_to=512)
    short = [i for i, ln in enumerate(POOL_LENS) if ln <= 40]
    mid = [i for i, ln in enumerate(POOL_LENS) if 40 < ln <= 300]
    cache = hip.PackedPrefixCache(cfg.hidden, 64, int(POOL_LENS.sum()), DEV)
    model = PackedStoreModel(cfg.hidden, 64, int(POOL_LENS.sum()))

    def call(pick, width):
        return _check(cache, engine, _batch(ids, mask, pick, width), prec, model, _tokens(ids, mask, pick))

    first = short[:5]
    assert call(first, 40) == len(first)                                          # all miss
    assert call(first, 40) == 0                                                   # all hit
    assert call(first[::-1] + mid[:4], 300) == 4                                  # stored at 40, asked for at 300; mixed
    assert call(first, 40) == 0                                                   # ... and back
    assert call([mid[5], short[5], mid[5], mid[5], short[0], short[5]], 300) == 2        # duplicates of two new keys
    assert call([mid[5], short[5]], 300) == 0
    rng = np.random.default_rng(7)
    for width in WIDTHS + WIDTHS[::-1]:
        fits = [i for i, ln in enumerate(POOL_LENS) if ln <= width]
        call(rng.choice(fits, 12), width)
    call(np.arange(len(POOL_LENS)), 512)
    assert call(np.arange(len(POOL_LENS)), 512) == 0                              # every news is in the pool now
    assert int(cache.tok_count.item()) == int(POOL_LENS.sum())
    check_layout(cache.row_off.cpu().numpy(), cache.row_len.cpu().numpy(), int(cache.tok_count.item()), cache.pool_tokens,
                 int(cache.row_count.item()))
    engine.status()
    engine.close()


# ------------------------------------------------------------------------------------------------ 2. training through the mirror
def _text_encoder(seed, preset="tiny-bert-512"):
    cfg = PRESETS[preset]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = MannerTextEncoder(preset, frozen_layers=[0], dropout_probability=0.2)
    w = make_plm_weights(cfg, seed=seed, std=0.05, with_pooler=True)
    enc.plm_model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    for n, p in enc.plm_model.named_parameters():
        if n.startswith("embeddings."):
            p.requires_grad_(False)
    enc.train_max_length = 512
    return cfg, enc.to(DEV).train()


def _step(enc, b, R, seed):
    for p in enc.parameters():
        p.grad = None
    torch.manual_seed(seed)                                                       # the dropout seed comes from torch's CPU generator
    out = enc(b)
    (out * R[:out.shape[0]]).sum().backward()
    return out.detach().clone(), {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("precision", ["fp32", "f16"])
def test_training_with_the_packed_store_equals_recomputing_the_frozen_prefix(precision):
    cfg, enc = _text_encoder(41)
    enc.train_precision = precision
    lens = np.array([5, 40, 128, 129, 300, 512, 77])
    ids, mask = synth_news_tokens(len(lens), cfg, seed=41, lengths=lens, pad_to=512)
    b = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    R = torch.from_numpy(np.random.default_rng(8).standard_normal((len(lens), cfg.hidden)).astype(np.float32)).to(DEV)
    enc.prefix_cache_rows = 0
    plain = [_step(enc, b, R, 200 + k) for k in range(2)]
    assert getattr(enc, "_prefix_cache", None) is None
    enc.prefix_cache_rows, enc.prefix_cache_tokens = 16, int(lens.sum())
    packed = []
    for k in range(2):
        packed.append(_step(enc, b, R, 200 + k))
        pc = enc._prefix_cache
        assert isinstance(pc, hip.PackedPrefixCache)
        assert (pc.lookups, pc.encoded) == ((k + 1) * len(lens), len(lens))       # the second step encoded no prefix
    for (o1, g1), (o2, g2) in zip(plain, packed):
        assert torch.equal(o1, o2)
        assert g1.keys() == g2.keys() and len(g1) > 4
        for n in g1:
            assert torch.equal(g1[n], g2[n]), n


# ------------------------------------------------------------------------------------------------ 3. wide batches are cached
def test_a_batch_padded_to_300_is_cached_where_the_fixed_width_table_bypasses_it():
    cfg, engine = _engine("tiny-bert-512", 32, ("f16",))
    lens = np.array([20, 64, 128, 129, 200, 300, 5, 250])
    ids, mask = synth_news_tokens(len(lens), cfg, seed=32, lengths=lens, pad_to=300)
    b = _batch(ids, mask, np.arange(len(lens)), 300)
    packed = hip.PackedPrefixCache(cfg.hidden, 32, int(lens.sum()), DEV)
    assert _check(packed, engine, b, "f16") == len(lens)
    assert _check(packed, engine, b, "f16") == 0

    class Counting:
        rows = 0

        def encode_hidden(self, i, m, *a, **k):
            self.rows += i.shape[0]
            return engine.encode_hidden(i, m, *a, **k)

    padded, counting = hip.PrefixCache(cfg.hidden, 128, 32, DEV), Counting()
    for k in (1, 2):                                                              # wider than max_len: every pass encodes every row
        out = padded.hidden_states(counting, b[0], b[1], 1, "f16")
        assert counting.rows == k * len(lens) and int(padded.row_count.item()) == 0
        assert torch.equal(out, engine.encode_hidden(b[0], b[1], 1, precision="f16"))
    counting.rows = 0
    packed.hidden_states(counting, b[0], b[1], 1, "f16")
    assert counting.rows == 0
    engine.close()


# ------------------------------------------------------------------------------------------------ 4. pool exhaustion and bounds
def test_a_full_pool_serves_by_encoding_and_writes_nothing_outside_it():
    cfg, engine = _engine("tiny-bert-512", 33, ("fp32",))
    H = cfg.hidden
    ids, mask = synth_news_tokens(len(POOL_LENS), cfg, seed=33, lengths=POOL_LENS, pad_to=512)
    pool_tokens = int(POOL_LENS.sum()) // 3                                       # holds only some of the batch
    guard = 4096                                                                  # f32 words of 0xA5 on each side (16-byte multiples)
    raw = torch.full(((2 * guard + pool_tokens * H) * 4,), 0xA5, dtype=torch.uint8, device=DEV)
    words = raw.view(torch.float32)
    pool = words[guard:guard + pool_tokens * H].view(pool_tokens, H)
    cache = hip.PackedPrefixCache(H, 64, pool_tokens, DEV, pool=pool)
    everything = np.arange(len(POOL_LENS))
    n_first = _check(cache, engine, _batch(ids, mask, np.concatenate([everything, everything[:6]]), 512), "fp32")
    assert n_first == len(POOL_LENS)                                              # the repeats of a key that got no payload are served too
    row_len = cache.row_len.cpu().numpy()
    stored, none = check_layout(cache.row_off.cpu().numpy(), row_len, int(cache.tok_count.item()), pool_tokens, int(cache.row_count.item()))
    assert stored >= 1 and none >= 1 and stored + none == len(POOL_LENS)          # it filled up in the middle of the batch
    rows, state = cache.lookup(*_batch(ids, mask, everything, 512))
    assert not bool(state.ne(0).any())
    rows = rows.cpu().numpy()
    has_payload = row_len[rows] >= 1
    # later calls, other widths and orders: a key without payload is encoded again (every occurrence), never read from the pool
    rng = np.random.default_rng(9)
    for width in (512, 300, 512, 129):
        fits = np.array([i for i, ln in enumerate(POOL_LENS) if ln <= width])
        pick = np.concatenate([rng.permutation(fits), fits[:3]])
        n_enc = _check(cache, engine, _batch(ids, mask, pick, width), "fp32")
        assert n_enc == int((~has_payload[pick]).sum())
        assert np.array_equal(cache.row_len.cpu().numpy(), row_len)
    torch.cuda.synchronize()
    canary = torch.full((guard * 4,), 0xA5, dtype=torch.uint8, device=DEV)
    assert torch.equal(raw[:guard * 4], canary) and torch.equal(raw[-guard * 4:], canary)
    # every stored payload is the row's own hidden states (nothing partial, nothing stale)
    want = engine.encode_hidden(*_batch(ids, mask, everything, 512), 1, precision="fp32")
    off = cache.row_off.cpu().numpy()
    for i, r in enumerate(rows.tolist()):
        if row_len[r] >= 1:
            assert row_len[r] == POOL_LENS[i] and torch.equal(pool[off[r]:off[r] + row_len[r]], want[i, :row_len[r]])
    engine.status()
    engine.close()


# ------------------------------------------------------------------------------------------------ 5. invalidation
def test_frozen_weight_or_precision_change_empties_the_store_and_an_exception_leaves_no_key_behind():
    cfg, enc = _text_encoder(42)
    enc.train_precision = "fp32"
    lens = np.array([7, 130, 300, 64])
    ids, mask = synth_news_tokens(len(lens), cfg, seed=42, lengths=lens, pad_to=300)
    b = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    R = torch.ones((len(lens), cfg.hidden), device=DEV)
    enc.prefix_cache_rows, enc.prefix_cache_tokens = 16, int(lens.sum())
    o0, _ = _step(enc, b, R, 1)
    _step(enc, b, R, 1)
    pc = enc._prefix_cache
    assert (pc.lookups, pc.encoded, int(pc.tok_count.item())) == (8, 4, int(lens.sum()))
    with torch.no_grad():                                                         # an optimiser-visible write to a FROZEN tensor
        enc.plm_model.get_parameter("encoder.layer.0.output.dense.weight").mul_(1.3)
    o1, _ = _step(enc, b, R, 1)
    assert enc._prefix_cache is pc and (pc.lookups, pc.encoded) == (4, 4)         # emptied, every news encoded again
    assert not torch.equal(o0, o1)
    enc.prefix_cache_rows = 0
    o1_plain, _ = _step(enc, b, R, 1)
    assert torch.equal(o1, o1_plain)
    enc.prefix_cache_rows = 16
    _step(enc, b, R, 1)
    enc.train_precision = "bf16"                                                  # other arithmetic: other hidden states
    o2, _ = _step(enc, b, R, 1)
    assert enc._prefix_cache is pc and (pc.lookups, pc.encoded) == (4, 4)
    enc.prefix_cache_rows = 0
    assert torch.equal(o2, _step(enc, b, R, 1)[0])
    enc.invalidate()
    assert int(pc.row_count.item()) == 0 and int(pc.tok_count.item()) == 0

    class Boom(RuntimeError):
        pass

    class Failing:
        def encode_hidden(self, *a, **k):
            raise Boom()

    with pytest.raises(Boom):
        pc.hidden_states(Failing(), b["input_ids"], b["attention_mask"], 1, "fp32")
    assert int(pc.row_count.item()) == 0 and int(pc.tok_count.item()) == 0
    assert not bool(pc.slot_keys.count_nonzero()) and bool(pc.slot_rows.eq(-1).all()) and bool(pc.row_len.eq(-1).all())


# ------------------------------------------------------------------------------------------------ 6. defaults
def test_without_the_switch_the_mirror_keeps_the_fixed_width_table_and_its_bits():
    cfg, enc = _text_encoder(43)
    enc.train_precision = "f16"
    enc.prefix_cache_tokens = 0
    lens = np.array([9, 33, 40, 21, 40, 12])
    ids, mask = synth_news_tokens(len(lens), cfg, seed=43, lengths=lens, pad_to=40)
    b = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    wide_ids, wide_mask = synth_news_tokens(3, cfg, seed=44, lengths=np.array([200, 50, 129]), pad_to=200)
    wide = {"input_ids": torch.from_numpy(wide_ids).to(DEV), "attention_mask": torch.from_numpy(wide_mask).to(DEV)}
    R = torch.ones((len(lens), cfg.hidden), device=DEV)
    enc.prefix_cache_rows = 0
    plain = [_step(enc, x, R, 5) for x in (b, b, wide)]
    enc.prefix_cache_rows, enc.prefix_cache_len = 16, 40
    cached = [_step(enc, x, R, 5) for x in (b, b, wide)]
    pc = enc._prefix_cache
    assert type(pc) is hip.PrefixCache and pc.max_len == 40
    assert (pc.lookups, pc.encoded) == (12, 6)                                    # the wide batch bypassed the table, as before
    for (o1, g1), (o2, g2) in zip(plain, cached):
        assert torch.equal(o1, o2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    # the unchanged class, driven directly, returns what the mirror fed the training engine
    engine = enc._hip_prefix
    direct = hip.PrefixCache(cfg.hidden, 40, 16, DEV)
    for _ in range(2):
        assert torch.equal(direct.hidden_states(engine, b["input_ids"], b["attention_mask"], 1, "f16"),
                           engine.encode_hidden(b["input_ids"], b["attention_mask"], 1, precision="f16"))


# ------------------------------------------------------------------------------------------------ 7. the memory claim
def test_a_pool_of_exactly_the_real_tokens_stores_every_news_of_the_long_profile(measured):
    cfg, engine = _engine("tiny-bert-512", 34, ("f16",))
    n = 600
    lens = synth_lengths(n, 42, 512, "title_abstract")
    ids, mask = synth_news_tokens(n, cfg, seed=42, lengths=lens, pad_to=512)
    assert len({tuple(r[m == 1]) for r, m in zip(ids, mask)}) == n
    total = int(lens.sum())
    cache = hip.PackedPrefixCache(cfg.hidden, n, total, DEV)
    for lo in range(0, n, 100):
        pick = np.arange(lo, lo + 100)
        cache.hidden_states(engine, *_batch(ids, mask, pick, int(lens[pick].max())), 1, "f16")
    assert cache.encoded == n and int(cache.tok_count.item()) == total
    stored, none = check_layout(cache.row_off.cpu().numpy(), cache.row_len.cpu().numpy(), total, total, int(cache.row_count.item()))
    assert (stored, none) == (n, 0)
    pick = np.random.default_rng(1).permutation(n)[:64]
    assert _check(cache, engine, _batch(ids, mask, pick, 512), "f16") == 0
    packed = hip.prefix_cache_bytes(cfg.hidden, n, pool_tokens=total)
    padded = hip.prefix_cache_bytes(cfg.hidden, n, max_len=512)
    slots = 2048 * 20 + 4
    assert packed["total"] == total * cfg.hidden * 4 + n * 16 + 8 + slots and padded["total"] == n * 512 * cfg.hidden * 4 + slots
    assert cache.pool.numel() * 4 == packed["payload"]
    ratio = padded["total"] / packed["total"]
    print(f"title+abstract profile, {n} news: {total / n:.1f} real tokens per news, padded / packed bytes = {ratio:.3f}")
    measured(padded_over_packed_bytes=ratio, real_tokens_per_news=total / n)     # recorded, not barred
    engine.close()


# ------------------------------------------------------------------------------------------------ argument checks
def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    cache = hip.PackedPrefixCache(8, 4, 64, DEV)
    z32 = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.zeros((4, 16, 8), device=DEV)
    P = hip._ptr

    def gather(lp=16, hidden=8, pool=cache.pool, n=4, pool_tokens=64):
        return lib.manner_hip_prefix_gather(P(z32), P(z32), n, lp, hidden, P(pool), pool_tokens, 4, P(cache.row_off), P(cache.row_len),
                                            P(cache.row_src), None, 0, None, P(out), hip._stream())

    assert gather() == 0
    for bad in (dict(lp=0), dict(lp=513), dict(hidden=6), dict(pool=None), dict(n=-1), dict(pool_tokens=-1)):
        assert gather(**bad) != 0, bad
        assert lib.manner_hip_last_error()
    with pytest.raises(RuntimeError, match="prefix_store"):
        _lib.check(lib.manner_hip_prefix_store(None, 1, None, 1, P(z32), P(z32), P(z32), 16, 8, P(cache.pool), 64, 4, P(cache.row_off),
                                               P(cache.row_len), P(cache.row_src), P(cache.tok_count), P(z32), hip._stream()))
    with pytest.raises(RuntimeError, match="prefix_resolve"):
        _lib.check(lib.manner_hip_prefix_resolve(None, P(z32), 4, P(cache.row_len), 4, hip._stream()))
    with pytest.raises(ValueError):
        hip.PackedPrefixCache(6, 4, 64, DEV)
    torch.cuda.synchronize()
