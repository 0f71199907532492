"""A-Module batches on the device: ``sample_m_per_class`` equals the numpy restatement of the rule (tests/news_sample_ref.py) bit for
bit over a whole epoch; ``DeviceNewsTrainSampler.batch`` and ``DeviceNewsCollate`` build the batch numpy builds from the same
indices, the former without any read-back or upload per batch; and an A-Module training step runs on a sampled batch."""
import warnings

import numpy as np
import pytest
import torch

import news_sample_ref as ref
from manner_amd import _lib, hip
from manner_amd.config import PRESETS
from manner_amd.data.components.mind_news_dataset import DeviceNewsCollate, DeviceNewsTrainSampler, NewsDataset
from manner_amd.data.components.mind_rec_dataset import NewsStore, ParsedBehaviors
from manner_amd.weights import make_entity_weights, make_plm_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 42
N_NEWS = 1000                                                       # rows of the sampler tests' store (lengths and entity counts only)


# ---------------------------------------------------------------------------------------------- the sampler's data sets
_SETS = {}


def _dataset(m, n_classes, big=False):
    """Labels of ``n_classes`` classes whose sizes cycle through {1, m - 1, m, m + 1, 300} (``big``: the last class has 100 000
    members, so that Floyd's J + 1 passes 2^16), in shuffled order, label values 3 c + 1; tables, store rows and lengths on both
    sides.  Built once per (m, L)."""
    k = (m, n_classes, big)
    if k not in _SETS:
        g = np.random.default_rng(m * 100 + n_classes)
        sizes = [s for s in (1, m - 1, m, m + 1, 300) if s > 0]
        sizes = [sizes[c % len(sizes)] for c in range(n_classes)]
        if big:
            sizes[-1] = 100000
        labels = g.permutation(np.repeat(np.arange(n_classes) * 3 + 1, sizes)).astype(np.int64)
        tables = ref.class_tables(labels)
        rows = g.integers(0, N_NEWS, labels.size).astype(np.int32)
        lens, cnts = g.integers(1, 97, N_NEWS).astype(np.int32), g.integers(0, 9, N_NEWS).astype(np.int32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        _SETS[k] = dict(labels=labels, tables=tables, sizes=sizes, rows=rows, lens=lens, cnts=cnts, ref={},
                        dev=dict(off=up(tables[1]), members=up(tables[2].astype(np.int32)), label=up(tables[0]), rows=up(rows),
                                 lens=up(lens), cnts=up(cnts)))
    return _SETS[k]


def _ref_epoch(d, m, k, nb, seed=SEED, epoch=0):
    """The restatement's epoch over a data set — computed once and shared."""
    key = (m, k, nb, seed, epoch)
    if key not in d["ref"]:
        got = [ref.sample_batch(d["tables"], m, k, seed, epoch, b) for b in range(nb)]
        idx, lab = np.concatenate([x[0] for x in got]), np.concatenate([x[1] for x in got])
        rows = d["rows"][idx]
        width = np.stack([d["lens"][rows].reshape(nb, -1).max(1), d["cnts"][rows].reshape(nb, -1).max(1)], 1)
        d["ref"][key] = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in
                              (idx.astype(np.int32), rows.astype(np.int32), lab.astype(np.int64), width.astype(np.int32)))
    return d["ref"][key]


def _run(d, m, k, nb, seed=SEED, epoch=0, cnts=True):
    t = d["dev"]
    return hip.sample_m_per_class(t["off"], t["members"], t["label"], t["rows"], t["lens"], t["cnts"] if cnts else None, m, k, nb, seed,
                                  epoch)


# (m, L, k, nb, big): every m of {1, 20, 64, 65} with k in {1, 3, L} and L in {3, 4, 19}, then m = 129 and 256 (the drawn set in three
# and four registers a lane); nb * k is not a multiple of the 4 waves of a workgroup in most, and nb runs from 1 to 37
CASES = [(1, 3, 1, 1, False), (1, 4, 4, 37, False), (1, 19, 19, 3, False), (20, 3, 3, 5, False), (20, 4, 1, 37, False),
         (20, 19, 19, 2, True), (20, 19, 3, 13, True), (64, 3, 1, 1, False), (64, 4, 4, 3, False), (64, 19, 3, 7, False),
         (64, 19, 19, 2, False), (65, 3, 3, 2, False), (65, 4, 1, 37, False), (65, 19, 19, 5, False), (129, 4, 4, 1, False),
         (256, 4, 4, 2, False)]


@pytest.mark.parametrize("m,n_classes,k,nb,big", CASES)
def test_sample_m_per_class_equals_the_restatement_bit_for_bit(m, n_classes, k, nb, big):
    d = _dataset(m, n_classes, big)
    want = _ref_epoch(d, m, k, nb)
    got = _run(d, m, k, nb)
    for name, g, w in zip(("idx", "rows", "labels", "width"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g.cpu(), w), (name, m, n_classes, k, nb)
    hip.check_status(DEV)
    if k == n_classes == 19:                                         # every class size was drawn from: with and without replacement
        assert {s for s in (1, m - 1, m, m + 1, 300) if s > 0} <= set(d["sizes"])
    if big and k == n_classes:                                       # and Floyd's r did pass 2^16 in the class of 100 000
        idx = want[0].numpy().reshape(nb, k, m)
        lab = want[2].numpy().reshape(nb, k, m)[:, :, 0]
        pos = np.searchsorted(np.flatnonzero(d["labels"] == 3 * (n_classes - 1) + 1), idx[lab == 3 * (n_classes - 1) + 1])
        assert pos.max() >= 1 << 16


def test_without_entity_counts_the_second_width_is_zero():
    d = _dataset(20, 4)
    got, want = _run(d, 20, 3, 5, cnts=False), _ref_epoch(d, 20, 3, 5)
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[3][:, 0].cpu(), want[3][:, 0]) and not bool(got[3][:, 1].any())


def test_a_sample_depends_on_seed_and_epoch_only():
    d = _dataset(20, 19, True)
    a = _run(d, 20, 3, 13)
    filler = torch.randn(1 << 20, device=DEV)                        # other work between the calls
    filler = (filler * 2).sum()
    b = _run(d, 20, 3, 13)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # another stream
        c = _run(d, 20, 3, 13)
    side.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    longer = _run(d, 20, 3, 37)                                      # another grid: batch b does not depend on the epoch's length
    assert torch.equal(longer[0][:13 * 60], a[0])
    e1, s1 = _run(d, 20, 3, 13, epoch=1), _run(d, 20, 3, 13, seed=SEED + 1)
    for got, want in ((e1, _ref_epoch(d, 20, 3, 13, epoch=1)), (s1, _ref_epoch(d, 20, 3, 13, seed=SEED + 1))):
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[2].cpu(), want[2])
    assert not torch.equal(e1[0], a[0]) and not torch.equal(s1[0], a[0]) and not torch.equal(s1[0], e1[0])
    assert bool(torch.isfinite(filler))
    hip.check_status(DEV)


# ---------------------------------------------------------------------------------------------- errors
def test_a_bad_rows_entry_raises_at_the_next_status_check_and_writes_nothing_outside_the_outputs():
    """Three classes of four members, m = 4 and k = 3: every member is drawn in every batch, the two bad rows among them."""
    labels = np.repeat([5, 6, 9], 4).astype(np.int64)
    label, off, members = ref.class_tables(labels)
    rows = np.arange(12, dtype=np.int32) * 3
    rows[2], rows[7] = 40, -1                                        # a store of 40 news: one past the end, and a negative row
    lens, cnts = np.arange(1, 41, dtype=np.int32), (np.arange(40, dtype=np.int32) % 7)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = [up(off), up(members.astype(np.int32)), up(label), up(rows), up(lens), up(cnts)]
    hip.check_status(DEV)
    lib, word = _lib.load(), hip.device_status(DEV).word
    G, nb = 64, 2                                                    # guard elements on either side of every output
    bufs = [torch.full((n + 2 * G,), -7, dtype=dt, device=DEV) for n, dt in ((nb * 12, torch.int32), (nb * 12, torch.int32),
                                                                           (nb * 12, torch.int64), (nb * 2, torch.int32))]
    ptr = lambda b: b.data_ptr() + G * b.element_size()
    _lib.check(lib.manner_hip_sample_m_per_class(hip._ptr(t[0]), hip._ptr(t[1]), hip._ptr(t[2]), 3, 12, hip._ptr(t[3]), hip._ptr(t[4]),
                                                 hip._ptr(t[5]), 40, 4, 3, nb, SEED, 0, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]),
                                                 ptr(bufs[3]), hip._ptr(word), hip._stream()))
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:G] == -7).all()) and bool((b[-G:] == -7).all())
    idx, out_rows, lab, width = (b[G:-G].cpu().numpy() for b in bufs)
    want_idx, want_lab = (np.concatenate(x) for x in zip(*[ref.sample_batch((label, off, members), 4, 3, SEED, 0, b) for b in range(nb)]))
    assert np.array_equal(idx, want_idx) and np.array_equal(lab, want_lab)
    assert np.array_equal(np.sort(idx.reshape(nb, 12), 1), np.tile(np.arange(12), (nb, 1)))
    assert np.array_equal(out_rows, np.clip(rows[idx], 0, 39))       # the bad entries are clamped into the store, the rest untouched
    assert np.array_equal(width.reshape(nb, 2), [[40, 6]] * nb)
    with pytest.raises(RuntimeError, match="index outside the table"):
        hip.check_status(DEV)
    hip.check_status(DEV)                                            # raised once, then clear
    # a class without members is flagged too, and its block is written as zeros
    off_bad = up(np.array([0, 4, 4, 12], np.int64))
    got = hip.sample_m_per_class(off_bad, t[1], t[2], up(np.arange(12, dtype=np.int32)), t[4], t[5], 4, 3, 1, SEED, 0)
    blocks = got[0].cpu().numpy().reshape(3, 4)
    assert (blocks[got[2].cpu().numpy().reshape(3, 4)[:, 0] == 6] == 0).all()
    with pytest.raises(RuntimeError, match="index outside the table"):
        hip.check_status(DEV)
    for kw in (dict(m=257), dict(k=4)):                              # refused before launch, with the library's message
        with pytest.raises(RuntimeError, match="sample_m_per_class"):
            hip.sample_m_per_class(t[0], t[1], t[2], t[3], t[4], t[5], kw.get("m", 4), kw.get("k", 3), 1, SEED, 0)
    hip.check_status(DEV)


# ---------------------------------------------------------------------------------------------- the classes around the kernel
_WORLD = {}


def _world():
    """A store of 200 news (tiny-bert ids, lengths 4..40, 0..5 entities, 4 categories, 3 sentiments) and behaviours that refer to
    about 150 of them, so that a data-set index is not a store row."""
    if not _WORLD:
        cfg = PRESETS["tiny-bert"]
        g = np.random.default_rng(31)
        n_news = 200
        lens, ents = g.integers(4, 30, n_news), g.integers(0, 4, n_news)
        lens[17], ents[23] = 40, 5
        tokens = [[101] + g.integers(1000, cfg.vocab, int(l) - 2).tolist() + [102] for l in lens]
        entities = [g.integers(1, 50, int(e)).tolist() for e in ents]
        cat, sent = g.choice([0, 1, 2, 3], n_news, p=[0.6, 0.2, 0.15, 0.05]), g.integers(0, 3, n_news)
        store = NewsStore([f"N{i}" for i in range(n_news)], tokens, cfg.pad_id, entities=entities, category=cat.tolist(),
                          sentiment=sent.tolist(), device=DEV)
        used = np.sort(g.choice(n_news, 150, replace=False))
        hist, cand = g.choice(used, 300), np.concatenate([used, g.choice(used, 100)])
        g.shuffle(cand)
        bhv = ParsedBehaviors(users=np.zeros(10, np.int64), hist_rows=hist.astype(np.int32), hist_off=np.arange(0, 301, 30, dtype=np.int64),
                              cand_rows=cand.astype(np.int32), cand_off=np.arange(0, 251, 25, dtype=np.int64),
                              labels=np.zeros(250, np.float32))
        _WORLD.update(cfg=cfg, store=store, bhv=bhv, used=used, tokens=tokens, entities=entities, cat=cat, sent=sent)
    return _WORLD


def _numpy_batch(w, rows, labels, entities=True):
    """What the news-side MINDCollate returns for the store rows ``rows``: ids padded with pad_id to the batch maximum, mask 1 / 0,
    entities right-padded with 0, everything int64."""
    tok = [w["tokens"][r] for r in rows]
    lp = max((len(t) for t in tok), default=0)
    ids = np.full((len(tok), lp), w["store"].pad_id, np.int64)
    mask = np.zeros((len(tok), lp), np.int64)
    for i, t in enumerate(tok):
        ids[i, :len(t)], mask[i, :len(t)] = t, 1
    news = {"text": {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask)}}
    if entities:
        lists = [w["entities"][r] for r in rows]
        width = max((len(e) for e in lists), default=0)
        ent = np.zeros((len(lists), width), np.int64)
        for i, e in enumerate(lists):
            ent[i, :len(e)] = e
        news["entities"] = torch.from_numpy(ent)
    return {"news": news, "labels": torch.from_numpy(np.asarray(labels, np.int64))}


def _same(got, want):
    assert got.keys() == want.keys() and got["news"].keys() == want["news"].keys()
    pairs = [(got["labels"], want["labels"]), (got["news"]["text"]["input_ids"], want["news"]["text"]["input_ids"]),
             (got["news"]["text"]["attention_mask"], want["news"]["text"]["attention_mask"])]
    if "entities" in want["news"]:
        pairs.append((got["news"]["entities"], want["news"]["entities"]))
    for g, x in pairs:
        assert g.is_cuda and g.dtype == torch.int64 == x.dtype and g.shape == x.shape and torch.equal(g.cpu(), x)


@pytest.mark.parametrize("aspect", ["category", "sentiment"])
def test_the_dataset_is_the_referenced_news_in_ascending_store_row(aspect):
    w = _world()
    ds = NewsDataset(w["store"], w["bhv"], aspect)
    assert len(ds) == 150 and np.array_equal(ds.rows, w["used"]) and ds.rows.dtype == np.int32
    assert np.array_equal(ds.labels, (w["cat"] if aspect == "category" else w["sent"])[w["used"]])
    for a, b in zip((ds.class_label, ds.class_off, ds.class_members), ref.class_tables(ds.labels)):
        assert np.array_equal(a, b)
    assert torch.equal(ds.rows_d.cpu(), torch.from_numpy(ds.rows)) and torch.equal(ds.class_members_d.cpu(), torch.from_numpy(ds.class_members))


@pytest.mark.parametrize("entities", [True, False])
def test_device_news_collate_equals_the_numpy_built_batch(entities):
    w = _world()
    ds = NewsDataset(w["store"], w["bhv"], "category")
    collate = DeviceNewsCollate(w["store"], ds, entities=entities)
    for idx in (range(0, 60), range(137, 150), range(5, 6), [149, 0, 3, 3, 77], [], torch.tensor([9, 8, 120], device=DEV)):
        got = collate(idx)
        idx_h = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else list(idx), np.int64)
        _same(got, _numpy_batch(w, ds.rows[idx_h], ds.labels[idx_h], entities))
        assert ("entities" in got["news"]) == entities
    with pytest.raises(IndexError):
        collate([0, 150])
    with pytest.raises(IndexError):
        collate(range(140, 151))
    hip.check_status(DEV)


@pytest.mark.parametrize("aspect,m,batch_size", [("category", 4, 12), ("sentiment", 5, 15), ("category", 1, 4)])
def test_sampled_batches_equal_the_numpy_built_batches_of_the_restatements_indices(aspect, m, batch_size):
    w = _world()
    ds = NewsDataset(w["store"], w["bhv"], aspect)
    sampler = DeviceNewsTrainSampler(w["store"], ds, m, batch_size, seed=7)
    assert len(sampler) == 150 // batch_size
    for epoch in (0, 2):
        sampler.set_epoch(epoch)
        sampler.sample_epoch()
        idx, lab = ref.sample_epoch(ds.labels, m, batch_size, 7, epoch)
        assert torch.equal(sampler.idx_d.cpu(), torch.from_numpy(idx.reshape(-1).astype(np.int32)))
        for i in range(0, len(sampler), 3):
            _same(sampler.batch(i), _numpy_batch(w, ds.rows[idx[i]], lab[i]))
    plain = DeviceNewsTrainSampler(w["store"], ds, m, batch_size, seed=7, entities=False)
    plain.set_epoch(2)
    plain.sample_epoch()
    _same(plain.batch(1), _numpy_batch(w, ds.rows[idx[1]], lab[1], entities=False))
    assert "entities" not in plain.batch(1)["news"]
    with pytest.raises(IndexError):
        sampler.batch(len(sampler))
    hip.check_status(DEV)


def test_batch_reads_nothing_back_and_copies_nothing_up(monkeypatch):
    w = _world()
    ds = NewsDataset(w["store"], w["bhv"], "category")
    sampler = DeviceNewsTrainSampler(w["store"], ds, 4, 12, seed=3)
    sampler.sample_epoch()                                           # allowed its one synchronising read
    sampler.batch(0)                                                 # warm-up: first-use allocations and module loads
    uploads = []
    real_from_numpy, real_tensor = torch.from_numpy, torch.tensor
    monkeypatch.setattr(torch, "from_numpy", lambda *a, **k: uploads.append("from_numpy") or real_from_numpy(*a, **k))
    monkeypatch.setattr(torch, "tensor", lambda *a, **k: uploads.append("tensor") or real_tensor(*a, **k))
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [sampler.batch(i) for i in (1, 5, 11)]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    monkeypatch.undo()
    assert not uploads                                               # no host array became a tensor: slices of the epoch's outputs only
    idx, lab = ref.sample_epoch(ds.labels, 4, 12, 3, 0)
    for i, b in zip((1, 5, 11), got):
        _same(b, _numpy_batch(w, ds.rows[idx[i]], lab[i]))
        assert b["labels"].untyped_storage().data_ptr() == sampler.labels_d.untyped_storage().data_ptr()
    torch.cuda.set_sync_debug_mode("error")                          # the epoch launch itself does read back: once
    try:
        with pytest.raises(RuntimeError):
            sampler.sample_epoch()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    hip.check_status(DEV)


_STEPS = {}


def _a_train_steps():
    """``hotpath.a_train_step`` + backward on a tiny fp32 encoder with the entity branch, three times from the same weights: on a
    sampled batch, on the numpy-built batch of the same indices, and on that batch once more.  Run once and shared."""
    if not _STEPS:
        from manner_amd import hotpath
        from manner_amd.models.components.news_encoder import MannerNewsEncoder
        w = _world()
        cfg = w["cfg"]
        ew = make_entity_weights(50, 100, 200, cfg.hidden, seed=8)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            enc = MannerNewsEncoder(plm_model="tiny-bert", frozen_layers=[0], dropout_probability=0.0, use_entities=True,
                                    entity_embeddings=ew["entity_encoder.pretrained_embedding.weight"], entity_embedding_dim=100,
                                    num_attention_heads=10, query_vector_dim=200, text_embedding_dim=cfg.hidden)
        sd = {"text_encoder.plm_model." + k: torch.from_numpy(v) for k, v in make_plm_weights(cfg, seed=70, std=0.05, with_pooler=True).items()}
        sd.update({k: torch.from_numpy(v) for k, v in ew.items()})
        enc.load_state_dict(sd, strict=True)
        enc = enc.to(DEV).train()
        te = enc.text_encoder
        te.train_precision = "fp32"
        te.plm_model.hidden_dropout_prob = te.plm_model.attention_probs_dropout_prob = 0.0
        ds = NewsDataset(w["store"], w["bhv"], "category")
        sampler = DeviceNewsTrainSampler(w["store"], ds, 4, 12, seed=5)
        sampler.sample_epoch()
        idx, lab = ref.sample_epoch(ds.labels, 4, 12, 5, 0)
        built = _numpy_batch(w, ds.rows[idx[2]], lab[2])
        _same(sampler.batch(2), built)
        to_dev = lambda x: {k: to_dev(v) for k, v in x.items()} if isinstance(x, dict) else x.to(DEV)
        results = []
        for batch in (sampler.batch(2), to_dev(built), to_dev(built)):
            enc.zero_grad(set_to_none=True)
            loss, emb = hotpath.a_train_step(enc, batch, temperature=0.1)
            loss.backward()
            results.append((loss.detach().clone(), emb.clone(), {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}))
        hip.check_status(DEV)
        _STEPS.update(results=results, labels=lab[2], hidden=cfg.hidden)
    return _STEPS


def test_a_train_step_runs_on_a_sampled_batch_to_the_loss_of_the_numpy_built_batch():
    s = _a_train_steps()
    (la, ea, ga), (lb, eb, gb), _ = s["results"]
    labels = s["labels"]
    assert (labels[:, None] == labels[None, :]).sum() > labels.size and (labels[:, None] != labels[None, :]).any()    # both kinds of pair
    assert bool(torch.isfinite(la)) and float(la) > 0 and ea.shape == (12, s["hidden"])
    assert torch.equal(la, lb) and torch.equal(ea, eb)
    assert ga.keys() == gb.keys() and len(ga) > 10 and "entity_encoder.pretrained_embedding.weight" in ga
    assert all(bool(torch.isfinite(g).all()) for g in ga.values()) and sum(int(g.abs().sum() > 0) for g in ga.values()) > 10


def test_a_train_step_gradients_equal_those_of_the_numpy_built_batch():
    """``.grad`` of every parameter after the step on the sampled batch is ``torch.equal`` to the step on the numpy-built batch.

    This holds the training kernels to sums in a fixed order at the size of an A-Module step: the word, position and entity
    embedding gradients (``embed_bwd_ordered_kernel``, csrc/train.hip; ``embedding_bwd_ordered_kernel``, csrc/train_small.hip) and
    the entity pooler's query (``pool_dq_kernel``) were f32 ``atomicAdd`` sums, which differed by 2e-7 to 7e-7 of the largest
    gradient from one run of the SAME batch to the next.  The third step (the built batch once more) is that control."""
    s = _a_train_steps()
    (_, _, ga), (_, _, gb), (_, _, gc) = s["results"]
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp(min=1e-30))
    differ = [k for k in ga if not torch.equal(ga[k], gb[k])]
    for k in ga:                                                     # the figures, before anything is asserted
        print(f"{k}: sampled vs built {rel(ga[k], gb[k]):.3g}, built vs built again {rel(gb[k], gc[k]):.3g}")
    assert not differ, differ
    assert all(torch.equal(gb[k], gc[k]) for k in gb)
