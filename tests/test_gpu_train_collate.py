"""Training batches on the device: ``sample_candidates`` equals the numpy restatement of the sampling rule (tests/train_sample_ref.py)
bit for bit, whatever the batch; ``gather_segments`` equals numpy indexing; ``DeviceTrainCollate`` builds the batch that ``DeviceCollate``
builds from the restatement's sampled lists, without a device-to-host read in its default mode; and a training step runs on it."""
import warnings

import numpy as np
import pytest
import torch

from manner_amd import _lib, hip
from manner_amd.config import PRESETS
from manner_amd.data.components.mind_rec_dataset import (DeviceCollate, DeviceTrainCollate, NewsStore, ParsedBehaviors,
                                                        plan_train_batch)
from manner_amd.weights import make_plm_weights
from train_sample_ref import sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 42
SIZES = (2, 5, 63, 64, 65, 257, 1500)


# ---------------------------------------------------------------------------------------------- the sampler's data set
def _variants(n, g):
    """Label vectors of one impression length: p = 1 and p = 3 among negatives, a click-heavy one (q < p: replacement at every ratio),
    a sparse one (most labels are neither 0 nor 1: replacement at ratio 4, none at ratio 1) and one without a click."""
    out = []
    one = np.zeros(n, np.float32)
    one[g.integers(0, n)] = 1
    out.append(one)                                                  # n = 2: q = 1, so ratio 4 draws with replacement
    if n >= 5:
        three = np.zeros(n, np.float32)
        three[[0, n // 2, n - 1]] = 1                                # n = 5: q = 2 < 3 = m at ratio 1 already
        out.append(three)
        heavy = np.ones(n, np.float32)
        heavy[g.choice(n, max(1, n // 10), replace=False)] = 0       # n = 1500: 1350 clicks, 6750 elements at ratio 4
        out.append(heavy)
        sparse = np.full(n, 0.5, np.float32)
        where = g.choice(n, 3, replace=False)
        sparse[where[0]], sparse[where[1:]] = 1, 0                   # p = 1, q = 2
        out.append(sparse)
    out.append(np.zeros(n, np.float32))                              # p = 0: an empty segment
    return out


_DATA = {}


def _sampler_data():
    if not _DATA:
        g = np.random.default_rng(1)
        labs = [v for n in SIZES for v in _variants(n, g)]
        off = np.concatenate([[0], np.cumsum([l.size for l in labs])]).astype(np.int64)
        _DATA.update(labs=labs, off=off, labels=np.concatenate(labs), rows=g.integers(0, 100000, int(off[-1])).astype(np.int32),
                     users=g.integers(0, 1000, len(labs)).astype(np.int64), ref={})
        _DATA["dev"] = {k: torch.from_numpy(_DATA[k]).to(DEV) for k in ("off", "labels", "rows", "users")}
    return _DATA


def _ref(ratio, imp, seed=SEED, epoch=0):
    """The restatement's sample of one impression of the data set — computed once and shared."""
    d = _sampler_data()
    k = (ratio, imp, seed, epoch)
    if k not in d["ref"]:
        d["ref"][k] = sample(d["labs"][imp], ratio, seed, epoch, imp)
    return d["ref"][k]


def _run(idx, ratio, seed=SEED, epoch=0):
    d = _sampler_data()
    sizes = [_ref(ratio, int(i), seed, epoch).size for i in idx]
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    t = d["dev"]
    rows, lab, users, pos = hip.sample_candidates(t["rows"], t["labels"], t["off"], torch.as_tensor(np.asarray(idx, np.int64)).to(DEV),
                                                  torch.from_numpy(out_off).to(DEV), int(out_off[-1]), ratio, seed, epoch,
                                                  users=t["users"], return_pos=True)
    return rows.cpu().numpy(), lab.cpu().numpy(), users.cpu().numpy(), pos.cpu().numpy(), out_off


@pytest.mark.parametrize("ratio", [1, 4])
def test_sample_candidates_equals_the_restatement_bit_for_bit(ratio):
    d = _sampler_data()
    n_imp = len(d["labs"])
    g = np.random.default_rng(ratio)
    kinds = set()
    batches = [np.array([n_imp - 3]), g.permutation(n_imp)[:7], g.integers(0, n_imp, 64),
               np.concatenate([g.permutation(n_imp), g.permutation(n_imp)])[:64]]       # every impression at least once, most twice
    assert [b.size for b in batches] == [1, 7, 64, 64]
    for idx in batches:
        rows, lab, users, pos, out_off = _run(idx, ratio)
        assert np.array_equal(users, d["users"][idx])
        for b, imp in enumerate(idx):
            want = _ref(ratio, int(imp))
            beg = int(d["off"][imp])
            sl = slice(int(out_off[b]), int(out_off[b + 1]))
            assert np.array_equal(pos[sl], want), (ratio, int(imp), d["labs"][imp].size)
            assert np.array_equal(rows[sl], d["rows"][beg + want]) and np.array_equal(lab[sl], d["labels"][beg + want])
            l = d["labs"][imp]
            p, q = int((l == 1).sum()), int((l == 0).sum())
            kinds.add((l.size, "empty" if p == 0 else "replace" if ratio * p > q else "subset"))
    hip.check_status(DEV)
    for n in SIZES:                                                  # every length was seen empty, and sampled with and without replacement
        assert (n, "empty") in kinds and ((n, "replace") in kinds or ratio == 1 and n == 2) and ((n, "subset") in kinds or ratio == 4 and n == 2)


def test_a_sample_depends_on_seed_epoch_and_impression_only():
    d = _sampler_data()
    imp = next(i for i, l in enumerate(d["labs"]) if l.size == 257 and (l == 1).sum() == 3)          # q = 254 >= 20
    other = [i for i in range(len(d["labs"])) if i != imp]

    def of(idx, place, **kw):
        rows, lab, users, pos, out_off = _run(idx, 4, **kw)
        return pos[out_off[place]:out_off[place + 1]]

    a = of([imp] + other[:5], 0)
    b = of(other[5:20] + [imp, other[0], imp], 15)                   # another batch, another place
    c = of(other[5:20] + [imp, other[0], imp], 17)                   # and twice in one batch
    assert a.size == 15 and np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, _ref(4, imp))
    e1 = of([imp], 0, epoch=1)
    s1 = of([imp], 0, seed=SEED + 1)
    assert np.array_equal(e1, sample(d["labs"][imp], 4, SEED, 1, imp)) and np.array_equal(s1, sample(d["labs"][imp], 4, SEED + 1, 0, imp))
    assert not np.array_equal(e1, a) and not np.array_equal(s1, a) and not np.array_equal(s1, e1)
    hip.check_status(DEV)


@pytest.mark.parametrize("companion", [False, True])
def test_gather_segments_equals_numpy_indexing(companion):
    g = np.random.default_rng(3)
    sizes = np.array([0, 1, 1500, 3, 0, 7, 64])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    src = g.integers(-5, 10 ** 6, int(off[-1])).astype(np.int32)
    src_f = g.standard_normal(int(off[-1])).astype(np.float32)
    for idx in ([2], [0, 4], [4, 1, 0, 2, 2, 6, 3, 1, 5, 0], []):
        idx = np.asarray(idx, np.int64)
        out_off = np.concatenate([[0], np.cumsum(sizes[idx])]).astype(np.int64)
        take = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx]).astype(np.int64) if idx.size else np.zeros(0, np.int64)
        got = hip.gather_segments(torch.from_numpy(src).to(DEV), torch.from_numpy(off).to(DEV), torch.from_numpy(idx).to(DEV),
                                  torch.from_numpy(out_off).to(DEV), int(out_off[-1]),
                                  src_f=torch.from_numpy(src_f).to(DEV) if companion else None)
        if companion:
            assert np.array_equal(got[1].cpu().numpy(), src_f[take])
            got = got[0]
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), src[take])
    hip.check_status(DEV)


def test_rows_max_len_is_the_maximum_over_the_rows():
    g = np.random.default_rng(4)
    lens, cnts = g.integers(1, 97, 500).astype(np.int32), g.integers(0, 9, 500).astype(np.int32)
    for m in (0, 1, 255, 257, 1000):
        rows = g.integers(0, 500, m).astype(np.int32)
        got = hip.rows_max_len(torch.from_numpy(lens).to(DEV), torch.from_numpy(rows).to(DEV), torch.from_numpy(cnts).to(DEV)).tolist()
        assert got == ([int(lens[rows].max()), int(cnts[rows].max())] if m else [0, 0])
    assert hip.rows_max_len(torch.from_numpy(lens).to(DEV), torch.from_numpy(rows).to(DEV)).tolist() == [int(lens[rows].max()), 0]


# ---------------------------------------------------------------------------------------------- errors
def test_bad_indices_raise_at_the_next_status_check_and_write_nothing_outside_the_outputs():
    d = _sampler_data()
    t = d["dev"]
    n_imp = len(d["labs"])
    good = next(i for i, l in enumerate(d["labs"]) if l.size == 65 and (l == 1).sum() == 3)
    hip.check_status(DEV)
    lib, word = _lib.load(), hip.device_status(DEV).word
    G = 64                                                           # guard elements on either side of every output

    def launch(idx, out_off):
        total = int(out_off[-1])
        bufs = [torch.full((total + 2 * G,), -7, dtype=dt, device=DEV) for dt in (torch.int32, torch.float32, torch.int32)]
        users = torch.full((len(idx) + 2 * G,), -7, dtype=torch.int64, device=DEV)
        idx_d, off_d = torch.tensor(idx, dtype=torch.int64, device=DEV), torch.tensor(out_off, dtype=torch.int64, device=DEV)
        esz = {torch.int32: 4, torch.float32: 4, torch.int64: 8}
        ptr = lambda b: b.data_ptr() + G * esz[b.dtype]
        _lib.check(lib.manner_hip_sample_candidates(hip._ptr(t["rows"]), hip._ptr(t["labels"]), hip._ptr(t["off"]), n_imp, t["rows"].numel(),
                                                    hip._ptr(t["users"]), hip._ptr(idx_d), len(idx), hip._ptr(off_d), total, 4, SEED, 0,
                                                    ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(users), hip._ptr(word), hip._stream()))
        torch.cuda.synchronize()
        for b in bufs + [users]:
            assert bool((b[:G] == -7).all()) and bool((b[-G:] == -7).all())
        return bufs[2][G:-G].cpu().numpy()

    # an index outside the data set: its segment stays untouched, the good impression beside it is sampled as ever
    pos = launch([n_imp, good, -1], [0, 15, 30, 45])
    assert (pos[:15] == -7).all() and np.array_equal(pos[15:30], _ref(4, good)) and (pos[30:] == -7).all()
    with pytest.raises(RuntimeError, match="index outside the table"):
        hip.check_status(DEV)
    hip.check_status(DEV)                                            # raised once, then clear
    # offsets that disagree with the clicks the kernel counts, and a segment that leaves the outputs
    for out_off in ([0, 14], [0, 16], [-3, 12]):
        pos = launch([good], out_off)
        assert (pos == -7).all()
        with pytest.raises(RuntimeError, match="host_lengths disagree"):
            hip.check_status(DEV)
    # gather_segments: a bad index and a wrong length are flagged, the flagged elements are zeros
    off = torch.tensor([0, 3, 5], dtype=torch.int64, device=DEV)
    src = torch.arange(1, 6, dtype=torch.int32, device=DEV)
    got = hip.gather_segments(src, off, torch.tensor([1, 2], device=DEV), torch.tensor([0, 2, 4], device=DEV), 4)
    assert got.tolist() == [4, 5, 0, 0]
    with pytest.raises(RuntimeError, match="index outside the table"):
        hip.check_status(DEV)
    got = hip.gather_segments(src, off, torch.tensor([0], device=DEV), torch.tensor([0, 2], device=DEV), 2)
    assert got.tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="host_lengths disagree"):
        hip.check_status(DEV)
    hip.check_status(DEV)


# ---------------------------------------------------------------------------------------------- DeviceTrainCollate
_WORLD = {}


def _world():
    """A small store (tiny-bert ids, lengths 4..40, 0..5 entities) and 12 impressions of 10..30 candidates; news 0 is the longest and
    the richest in entities and a non-clicked candidate of every impression, so the default mode's bounds usually exceed the sample."""
    if not _WORLD:
        cfg = PRESETS["tiny-bert"]
        g = np.random.default_rng(21)
        n_news = 80
        lens = g.integers(4, 30, n_news)
        ents = g.integers(0, 4, n_news)
        lens[0], ents[0] = 40, 5
        tokens = [[101] + g.integers(1000, cfg.vocab, int(l) - 2).tolist() + [102] for l in lens]
        store = NewsStore([f"N{i}" for i in range(n_news)], tokens, cfg.pad_id, entities=[g.integers(1, 50, int(e)).tolist() for e in ents],
                          category=g.integers(0, 18, n_news).tolist(), sentiment=g.integers(0, 3, n_news).tolist(),
                          sentiment_score=g.standard_normal(n_news).astype(np.float32).tolist(), device=DEV)
        hist, cand, labs = [], [], []
        for i in range(12):
            hist.append(g.integers(1, n_news, int(g.integers(1, 8))))
            c = np.concatenate([[0], g.choice(np.arange(1, n_news), int(g.integers(9, 30)), replace=False)])
            l = np.zeros(c.size, np.float32)
            l[g.choice(np.arange(1, c.size), 1 + (i % 2), replace=False)] = 1
            cand.append(c)
            labs.append(l)
        labs[5][:] = 0                                               # an impression without a click
        off = lambda parts: np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
        bhv = ParsedBehaviors(users=g.integers(0, 500, 12).astype(np.int64), hist_rows=np.concatenate(hist).astype(np.int32), hist_off=off(hist),
                              cand_rows=np.concatenate(cand).astype(np.int32), cand_off=off(cand), labels=np.concatenate(labs))
        _WORLD.update(cfg=cfg, store=store, bhv=bhv)
    return _WORLD


def _sampled_behaviors(bhv, idx, ratio, seed, epoch):
    """The batch's impressions with the restatement's sampled candidate lists, as a data set of its own."""
    hist = [bhv.hist_rows[bhv.hist_off[i]:bhv.hist_off[i + 1]] for i in idx]
    cand, labs = [], []
    for i in idx:
        beg, end = int(bhv.cand_off[i]), int(bhv.cand_off[i + 1])
        s = beg + sample(bhv.labels[beg:end], ratio, seed, epoch, int(i))
        cand.append(bhv.cand_rows[s])
        labs.append(bhv.labels[s])
    off = lambda parts: np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return ParsedBehaviors(users=bhv.users[np.asarray(idx, np.int64)], hist_rows=cat(hist, np.int32), hist_off=off(hist),
                           cand_rows=cat(cand, np.int32), cand_off=off(cand), labels=cat(labs, np.float32))


def _flat(batch):
    out = {k: batch[k] for k in ("batch_hist", "batch_cand", "labels", "users", "hist_max", "cand_max")}
    for side in ("x_hist", "x_cand"):
        x = batch[side]
        out.update({f"{side}.ids": x["text"]["input_ids"], f"{side}.mask": x["text"]["attention_mask"]})
        out.update({f"{side}.{k}": x[k] for k in ("entities", "category", "sentiment", "sentiment_score")})
    return out


BATCHES = ([3, 0, 7, 11], range(4, 8), [5], [9, 9, 2, 10, 1, 6, 8], [])


@pytest.mark.parametrize("ratio", [1, 4])
def test_exact_width_batch_equals_device_collate_over_the_sampled_lists(ratio):
    w = _world()
    collate = DeviceTrainCollate(w["store"], w["bhv"], neg_sampling_ratio=ratio, seed=7, exact_width=True)
    for epoch in (0, 3):
        collate.set_epoch(epoch)
        for idx in BATCHES:
            got = _flat(collate(idx))
            sampled = _sampled_behaviors(w["bhv"], list(idx), ratio, 7, epoch)
            want = _flat(DeviceCollate(w["store"], sampled)(range(0, len(sampled))) if len(sampled)
                         else DeviceCollate(w["store"], sampled)([]))
            assert got.keys() == want.keys()
            for k in want:
                if isinstance(want[k], int):
                    assert got[k] == want[k], (k, list(idx))
                else:
                    assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (k, list(idx))
    hip.check_status(DEV)


def test_default_mode_pads_to_host_known_bounds_and_encodes_to_the_same_embeddings():
    from manner_amd.models.components.news_encoder import MannerTextEncoder
    w = _world()
    cfg, store = w["cfg"], w["store"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        te = MannerTextEncoder("tiny-bert", [], 0.0)
    te.plm_model.load_state_dict({k: torch.from_numpy(v) for k, v in make_plm_weights(cfg, seed=5, std=0.05, with_pooler=True).items()},
                                 strict=True)
    te = te.to(DEV).eval()
    te.precision = "fp32"
    loose = DeviceTrainCollate(store, w["bhv"], neg_sampling_ratio=1, seed=7)
    exact = DeviceTrainCollate(store, w["bhv"], neg_sampling_ratio=1, seed=7, exact_width=True)
    wider = 0
    for idx in BATCHES:
        a, b = _flat(loose(idx)), _flat(exact(idx))
        for k in ("batch_hist", "batch_cand", "labels", "users"):
            assert torch.equal(a[k], b[k]), k
        assert (a["hist_max"], a["cand_max"]) == (b["hist_max"], b["cand_max"])
        for k in a:
            if k.startswith("x_hist.") or k in ("x_cand.category", "x_cand.sentiment", "x_cand.sentiment_score"):
                assert torch.equal(a[k], b[k]), k
        plan = plan_train_batch(w["bhv"], idx, 1, loose.widths)
        for k, fill, bound in (("x_cand.ids", store.pad_id, plan.cand_text_bound), ("x_cand.mask", 0, plan.cand_text_bound),
                               ("x_cand.entities", 0, plan.cand_ent_bound)):
            lp = b[k].shape[1]
            assert a[k].shape == (b[k].shape[0], bound) and bound >= lp
            assert torch.equal(a[k][:, :lp], b[k]) and bool((a[k][:, lp:] == fill).all()), k
            wider += int(bound > lp and a[k].shape[0] > 0)
        if a["x_cand.ids"].shape[0]:
            with torch.no_grad():
                ea = te({"input_ids": a["x_cand.ids"], "attention_mask": a["x_cand.mask"]})
                eb = te({"input_ids": b["x_cand.ids"], "attention_mask": b["x_cand.mask"]})
            assert ea.shape == (a["x_cand.ids"].shape[0], cfg.hidden) and torch.equal(ea, eb)
    assert wider >= 3                                                # the bounds did exceed the sampled batches' widths
    hip.check_status(DEV)


def test_default_mode_reads_nothing_back_from_the_device():
    w = _world()
    collate = DeviceTrainCollate(w["store"], w["bhv"], neg_sampling_ratio=4, seed=7)
    order = np.random.default_rng(2).permutation(12)
    order_d = collate.upload_order(order)
    collate(order_d[0:4])                                            # warm-up: first-use allocations and module loads
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = collate(order_d[4:8])
        also = collate([int(i) for i in order[8:12]])                # a host sequence costs one host-to-device copy, no read either
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    want = collate([int(i) for i in order[4:8]])
    for k, v in _flat(want).items():
        assert v == _flat(got)[k] if isinstance(v, int) else torch.equal(v, _flat(got)[k]), k
    assert also["users"].tolist() == w["bhv"].users[order[8:12]].tolist()
    hip.check_status(DEV)


def test_clicks_without_negatives_raise_value_error_before_any_launch():
    w = _world()
    b = w["bhv"]
    labels = b.labels.copy()
    beg, end = int(b.cand_off[2]), int(b.cand_off[3])
    labels[beg:end] = np.where(labels[beg:end] == 1, 1, 0.5)         # impression 2: clicks, and nothing that counts as non-clicked
    bhv = ParsedBehaviors(b.users, b.hist_rows, b.hist_off, b.cand_rows, b.cand_off, labels)
    collate = DeviceTrainCollate(w["store"], bhv, neg_sampling_ratio=4)
    collate([0, 1])
    torch.cuda.synchronize()
    launched = []
    real = hip.sample_candidates
    hip.sample_candidates = lambda *a, **k: launched.append(1) or real(*a, **k)
    try:
        with pytest.raises(ValueError, match="impression 2"):
            collate([1, 2, 3])
    finally:
        hip.sample_candidates = real
    assert not launched
    with pytest.raises(IndexError):
        collate([0, 12])
    hip.check_status(DEV)


def test_cr_train_step_runs_on_a_sampled_batch():
    from manner_amd import hotpath
    from manner_amd.models.components.news_encoder import MannerNewsEncoder
    w = _world()
    cfg = w["cfg"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = MannerNewsEncoder(plm_model="tiny-bert", frozen_layers=[0], dropout_probability=0.0, use_entities=False,
                                entity_embeddings=None, entity_embedding_dim=100, num_attention_heads=10, query_vector_dim=200,
                                text_embedding_dim=cfg.hidden)
    enc.load_state_dict({"text_encoder.plm_model." + k: torch.from_numpy(v)
                         for k, v in make_plm_weights(cfg, seed=70, std=0.05, with_pooler=True).items()}, strict=True)
    enc = enc.to(DEV).train()
    enc.text_encoder.train_precision = "fp32"
    batch = DeviceTrainCollate(w["store"], w["bhv"], neg_sampling_ratio=4, seed=1)([0, 2, 3, 8])
    assert batch["labels"].numel() == int(batch["labels"].sum()) * 5
    loss, scores, cand_off = hotpath.cr_train_step(enc, batch, supcon=True, temperature=0.36)
    loss.backward()
    assert bool(torch.isfinite(loss)) and scores.numel() == batch["labels"].numel()
    seen = 0
    for k, p in enc.named_parameters():
        if p.requires_grad and "pooler." not in k:                   # (the [CLS] slice bypasses the pooler, as in the reference)
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            seen += int(p.grad.abs().sum() > 0)
        else:
            assert p.grad is None, k
    assert seen > 10
    hip.check_status(DEV)
