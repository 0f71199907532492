"""Device-side batches for the A-Module: the news-side counterpart of ``mind_rec_dataset.py``.

The reference trains an A-Module from a host loop: ``MINDNewsDataset.__getitem__`` does one ``DataFrame.iloc`` per news
(manner/data/components/mind_news_dataset.py:28-32), ``pytorch_metric_learning.samplers.MPerClassSampler`` orders the epoch over
the whole label array (manner/data/mind_news_datamodule.py:175-217) and the news-side ``MINDCollate`` concatenates 60 one-row
frames, calls the tokenizer and pads the entities on every step (mind_news_dataset.py:38-86).  Here the news live in the
device-resident ``NewsStore``; ``NewsDataset`` is the set of news a behaviours file refers to with one aspect label each,
``DeviceNewsCollate`` builds the ``MINDNewsBatch`` of any indices (the val / test path) and ``DeviceNewsTrainSampler`` draws a whole
epoch of M-per-class batches in one launch (the rule of include/manner_hip.h, "A-Module batches") and serves batch ``i`` from slices
of it: one synchronising read per EPOCH, none per batch.

Host code is numpy; everything on the GPU goes through ``manner_amd.hip`` (no CPU fallback).
"""
from __future__ import annotations

from typing import Sequence, Union

import numpy as np
import torch

from ... import hip
from .mind_batch import MINDNewsBatch
from .mind_rec_dataset import NewsStore, ParsedBehaviors

ASPECTS = ("category", "sentiment")
MAX_SAMPLES_PER_CLASS, MAX_CLASSES = 256, 1024        # the sampler kernel's bounds (include/manner_hip.h)


def class_tables(labels: np.ndarray):
    """-> (class_label int64 [L] ascending, class_off int64 [L + 1], class_members int32 [N]): the data-set indices grouped by
    label with a stable sort, so the members of a class are in ascending order."""
    labels = np.asarray(labels, np.int64).reshape(-1)
    members = np.argsort(labels, kind="stable").astype(np.int32)
    class_label, counts = np.unique(labels, return_counts=True)
    class_off = np.zeros(class_label.size + 1, np.int64)
    np.cumsum(counts, out=class_off[1:])
    return class_label.astype(np.int64), class_off, members


class NewsDataset:
    """``MINDNewsDataset`` over a ``NewsStore``: the news that any history or candidate list of ``behaviors`` refers to, each once,
    with its ``aspect`` label (``"category"`` or ``"sentiment"``: ``store.cat_d`` / ``store.sent_d``).

    Order: ASCENDING STORE ROW.  The reference's order is the iteration order of a Python ``set`` of news ids
    (mind_news_dataset.py:16-25), which is arbitrary (string hashing is salted per process); ascending store row is the order
    chosen here, and data-set index ``i`` means ``rows[i]`` everywhere below.  The class tables are built once, on the host."""

    def __init__(self, store: NewsStore, behaviors: ParsedBehaviors, aspect: str):
        if aspect not in ASPECTS:
            raise ValueError(f"aspect must be one of {ASPECTS}, got {aspect!r}")
        self.store, self.aspect = store, aspect
        rows = np.unique(np.concatenate([behaviors.hist_rows, behaviors.cand_rows])).astype(np.int32)
        if rows.size and (rows[0] < 0 or rows[-1] >= len(store)):
            raise IndexError(f"behaviours refer to a news row outside [0, {len(store)})")
        self.rows = rows
        column = store.cat_d if aspect == "category" else store.sent_d
        self.labels = column.cpu().numpy().astype(np.int64)[rows]                 # read once per data set
        self.class_label, self.class_off, self.class_members = class_tables(self.labels)
        dev = store.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.rows_d, self.labels_d = up(self.rows), up(self.labels)
        self.class_label_d, self.class_off_d, self.class_members_d = up(self.class_label), up(self.class_off), up(self.class_members)

    def __len__(self) -> int:
        return int(self.rows.shape[0])


def _news_batch(store: NewsStore, rows_d: torch.Tensor, labels_d: torch.Tensor, lp: int, width: int, entities: bool) -> MINDNewsBatch:
    ids, mask = hip.collate_text(store.ids_d, store.len_d, rows_d, lp, store.pad_id)
    news = {"text": {"input_ids": ids, "attention_mask": mask}}
    if entities:
        news["entities"] = hip.collate_entities(store.ent_d, store.cnt_d, rows_d, width)
    return MINDNewsBatch(news=news, labels=labels_d)


class DeviceNewsCollate:
    """The news-side ``MINDCollate`` with the store on the device: ``collate(indices) -> MINDNewsBatch`` =
    ``{"news": {"text": {"input_ids", "attention_mask"}, "entities"}, "labels"}``, all int64, text padded to the longest news of
    the batch and entities right-padded with 0 to the longest list (both exact, from the host's lengths).  ``entities=False``
    gives Adressa's batch, ``text`` only (adressa_news_dataset.py:58-61).

    ``indices``: data-set indices as a ``range``, a sequence or an int64 device tensor.  A contiguous ``range`` — the val / test
    path, ``shuffle=False`` — is served from device slices without any host-to-device copy; a sequence costs one upload of its
    rows and labels; a device tensor is read back first, which synchronises."""

    def __init__(self, store: NewsStore, dataset: NewsDataset, entities: bool = True):
        self.store, self.ds, self.entities = store, dataset, bool(entities)

    def __call__(self, indices: Union[range, Sequence[int], torch.Tensor]) -> MINDNewsBatch:
        ds, st = self.ds, self.store
        if isinstance(indices, range) and indices.step == 1 and len(indices) > 0:
            i0, i1 = indices.start, indices.stop
            if i0 < 0 or i1 > len(ds):
                raise IndexError(f"news index outside [0, {len(ds)})")
            rows_h, rows_d, labels_d = ds.rows[i0:i1], ds.rows_d[i0:i1], ds.labels_d[i0:i1]
        else:
            if isinstance(indices, torch.Tensor):
                if indices.dtype != torch.int64 or indices.dim() != 1:
                    raise TypeError("a tensor of news indices must be int64 and one-dimensional")
                indices = indices.cpu().numpy()                                   # the documented synchronising read
            idx = np.asarray(list(indices) if not isinstance(indices, np.ndarray) else indices, np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= len(ds)):
                raise IndexError(f"news index outside [0, {len(ds)})")
            rows_h = ds.rows[idx]
            rows_d = torch.from_numpy(rows_h).to(st.device, non_blocking=True)
            labels_d = torch.from_numpy(ds.labels[idx]).to(st.device, non_blocking=True)
        lp = int(st.lengths[rows_h].max()) if rows_h.size else 0                  # tokenizer padding=True: batch max
        width = int(st.ent_counts[rows_h].max()) if rows_h.size and self.entities else 0
        return _news_batch(st, rows_d, labels_d, lp, width, self.entities)


class DeviceNewsTrainSampler:
    """``MPerClassSampler(labels, samples_per_class, batch_size, length_before_new_iter=len(dataset))`` + ``MINDCollate`` on the
    device.  An epoch is ``len(self) = len(dataset) // batch_size`` batches of ``batch_size // samples_per_class`` distinct
    classes, each a block of ``samples_per_class`` consecutive slots holding distinct members of the class (draws with replacement
    where the class is smaller).  Inside a block the members stand in draw order, which is not a uniform permutation and need not
    be: SupCon, the batch-coupled entity attention and the iid dropouts are equivariant to the order inside a batch.

        sampler.set_epoch(e)
        sampler.sample_epoch()             # ONE launch for the whole epoch, then ONE synchronising read: the batches' widths
        for i in range(len(sampler)):
            batch = sampler.batch(i)       # slices + the collate kernels: no device-to-host read, no host-to-device copy

    A sample is a pure function of (``seed``, epoch) and the labels.  The widths are read back because they must be exact: the
    entity branch's additive pooler is unmasked, so entity columns beyond the batch maximum would change the
    embeddings.  As the original asserts, ``ValueError`` is raised on the host — before any launch — for ``len(dataset) <
    batch_size``, ``batch_size % samples_per_class != 0`` and ``samples_per_class * L < batch_size`` (L distinct labels)."""

    def __init__(self, store: NewsStore, dataset: NewsDataset, samples_per_class: int, batch_size: int, seed: int = 0,
                 entities: bool = True):
        m, bs = int(samples_per_class), int(batch_size)
        n_cls = int(dataset.class_label.shape[0])
        if m < 1 or bs < 1:
            raise ValueError("samples_per_class and batch_size must be at least 1")
        if len(dataset) < bs:
            raise ValueError(f"the data set has {len(dataset)} news, fewer than one batch of {bs}")
        if bs % m != 0:
            raise ValueError(f"batch_size {bs} is not a multiple of samples_per_class {m}")
        if m * n_cls < bs:
            raise ValueError(f"{n_cls} classes of {m} samples cannot fill a batch of {bs}")
        if m > MAX_SAMPLES_PER_CLASS or n_cls > MAX_CLASSES:
            raise ValueError(f"the sampler kernel takes samples_per_class <= {MAX_SAMPLES_PER_CLASS} and at most {MAX_CLASSES} classes")
        self.store, self.ds, self.entities = store, dataset, bool(entities)
        self.m, self.k, self.batch_size, self.nb = m, bs // m, bs, len(dataset) // bs
        self.seed, self.epoch = int(seed), 0
        self.idx_d = self.rows_d = self.labels_d = None
        self.widths = None                                                        # host [[text, entities]] * nb of the sampled epoch

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        return self.nb

    def sample_epoch(self) -> None:
        ds, st = self.ds, self.store
        self.idx_d, self.rows_d, self.labels_d, width = hip.sample_m_per_class(
            ds.class_off_d, ds.class_members_d, ds.class_label_d, ds.rows_d, st.len_d, st.cnt_d if self.entities else None,
            self.m, self.k, self.nb, self.seed, self.epoch)
        self.widths = width.tolist()                                              # the one synchronising read per epoch

    def batch(self, i: int) -> MINDNewsBatch:
        if self.widths is None:
            raise RuntimeError("call sample_epoch() before batch(i)")
        if not 0 <= i < self.nb:
            raise IndexError(f"batch {i} outside [0, {self.nb})")
        lo, hi = i * self.batch_size, (i + 1) * self.batch_size
        lp, width = self.widths[i]
        return _news_batch(self.store, self.rows_d[lo:hi], self.labels_d[lo:hi], lp, width, self.entities)
