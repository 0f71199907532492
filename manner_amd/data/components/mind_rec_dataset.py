"""Device-side collate for the evaluation path.

The reference assembles every batch on the host: ``MINDRecDatasetTest.__getitem__`` does two
``DataFrame.loc`` lookups per impression (manner/data/components/mind_rec_dataset.py:87-99) and
``MINDCollate.__call__`` concatenates the frames and re-tokenises every news of the batch
(:114-137, :146-168).  Here the news are tokenised once into a device-resident ``NewsStore``, the
behaviours are parsed once into CSR index arrays (``ParsedBehaviors``), and ``DeviceCollate`` builds the
same ``MINDRecBatch`` tensors with four HIP kernels (``csrc/collate.hip``) — the host only slices offsets.

Training batches: ``MINDRecDatasetTrain`` (manner/data/components/mind_rec_dataset.py:13-77) keeps every
clicked candidate of an impression, draws ``neg_sampling_ratio`` non-clicked ones per click (with replacement only when there
are too few, :59-63) and permutes the result, all with numpy's global stream on the host, before ``DataFrame.loc``,
``pd.concat`` and the tokenizer.  ``DeviceTrainCollate`` draws the same distribution on the device with a counter-based rule
(include/manner_hip.h, "training batches": a pure function of seed, epoch and impression) and collates the sampled batch with
the kernels above; ``plan_train_batch`` is its host half (sizes and offsets only).  No device-to-host read per batch.

Host code is numpy; everything on the GPU goes through ``manner_amd.hip`` (no CPU fallback).
"""
from __future__ import annotations

import io
import os
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Union

import numpy as np
import torch

from ... import hip
from .mind_batch import MINDRecBatch


# ---------------------------------------------------------------------------------------------- behaviours
@dataclass
class ParsedBehaviors:
    """CSR form of the behaviours frame (columns user / history / candidates / labels, mind_dataframe.py:359)."""
    users: np.ndarray        # int64 [B]
    hist_rows: np.ndarray    # int32 [sum h_i]  store rows, history already cut to max_history_length
    hist_off: np.ndarray     # int64 [B+1]
    cand_rows: np.ndarray    # int32 [sum c_i]
    cand_off: np.ndarray     # int64 [B+1]
    labels: np.ndarray       # float32 [sum c_i]

    def __len__(self) -> int:
        return int(self.users.shape[0])


def _ids_of_list_literal(field: str) -> List[str]:
    """The reference's converter for the cached frame (mind_dataframe.py:281-284):
    ``x.strip("[]").replace("'", "").split(", ")`` — note that "[]" yields [""]."""
    return field.strip("[]").replace("'", "").split(", ")


def parse_behaviors(source: Union[str, io.TextIOBase, Iterable[str]], nid2row: Dict[str, int], max_history_length: int,
                    uid2index: Optional[Dict[str, int]] = None) -> ParsedBehaviors:
    """Parse a behaviours file into CSR arrays.

    Accepts both wire formats of the reference: the cached ``parsed_behaviors.tsv`` (header
    ``user / history / candidates / labels``, lists serialised as ``['N1', 'N2']`` / ``[1, 0]`` —
    mind_dataframe.py:278-288) and the raw MIND ``behaviors.tsv`` (``impid uid time history impressions``,
    impressions ``N1-1 N2-0``; rows without history dropped, ``user = uid2index.get(uid, 0)`` — :291-357).
    History is cut to its first ``max_history_length`` items as MINDRecDatasetTest.__getitem__ does (:91).
    Unknown news ids raise KeyError, like ``news.loc``.
    """
    if isinstance(source, (str, os.PathLike)):
        with open(source, "r", encoding="utf-8") as f:
            return parse_behaviors(f, nid2row, max_history_length, uid2index)
    users: List[int] = []
    hist: List[int] = []
    cand: List[int] = []
    labels: List[float] = []
    hist_off = [0]
    cand_off = [0]
    parsed_format: Optional[bool] = None
    uid2index = uid2index or {}
    for line in source:
        line = line.rstrip("\n").rstrip("\r")
        if not line:
            continue
        cols = line.split("\t")
        if parsed_format is None:
            parsed_format = cols[:4] == ["user", "history", "candidates", "labels"]
            if parsed_format:
                continue
        if parsed_format:
            user = int(cols[0])
            h_ids = _ids_of_list_literal(cols[1])
            c_ids = _ids_of_list_literal(cols[2])
            lab = [int(x) for x in cols[3].strip("[]").split(", ")]
        else:
            if len(cols) < 5:
                raise ValueError(f"behaviors.tsv row with {len(cols)} columns")
            h_ids = cols[3].split()
            if not h_ids:                              # "drop interactions of users without history" (:311-314)
                continue
            user = int(uid2index.get(cols[1], 0))
            imps = cols[4].split()
            c_ids = [x.split("-")[0] for x in imps]
            lab = [int(x.split("-")[1]) for x in imps]
        h_ids = h_ids[:max_history_length]
        users.append(user)
        hist.extend(nid2row[n] for n in h_ids)
        cand.extend(nid2row[n] for n in c_ids)
        labels.extend(lab)
        hist_off.append(len(hist))
        cand_off.append(len(cand))
    if len(labels) != len(cand):
        raise ValueError("candidates and labels differ in length")
    return ParsedBehaviors(np.asarray(users, np.int64), np.asarray(hist, np.int32), np.asarray(hist_off, np.int64),
                           np.asarray(cand, np.int32), np.asarray(cand_off, np.int64), np.asarray(labels, np.float32))


# ---------------------------------------------------------------------------------------------- news store
class NewsStore:
    """Pre-tokenised news, resident in HBM.  Row order defines ``nid2row``.

    ``token_ids`` holds what ``tokenizer(text, truncation=True)`` returns for each news (special tokens
    included, cut to ``tokenizer_max_length`` = 96, configs/data/mind_rec.yaml:41); ``entities`` the filtered
    entity index lists (title + abstract concatenated when both aspects are used, mind_rec_dataset.py:147-158).
    """

    def __init__(self, nids: Sequence[str], token_ids: Sequence[Sequence[int]], pad_id: int,
                 entities: Optional[Sequence[Sequence[int]]] = None, category: Optional[Sequence[int]] = None,
                 sentiment: Optional[Sequence[int]] = None, sentiment_score: Optional[Sequence[float]] = None,
                 device: Union[str, torch.device] = "cuda"):
        n = len(nids)
        self.nid2row = {nid: i for i, nid in enumerate(nids)}
        if len(self.nid2row) != n:
            raise ValueError("duplicate news ids")
        self.pad_id = int(pad_id)
        self.lengths = np.fromiter((len(t) for t in token_ids), np.int32, n)
        width = max(int(self.lengths.max()) if n else 0, 1)
        ids = np.full((n, width), pad_id, np.int32)
        for i, t in enumerate(token_ids):
            ids[i, :len(t)] = t
        entities = entities if entities is not None else [[]] * n
        self.ent_counts = np.fromiter((len(e) for e in entities), np.int32, n)
        ent = np.zeros((n, max(int(self.ent_counts.max()) if n else 0, 1)), np.int32)
        for i, e in enumerate(entities):
            ent[i, :len(e)] = e
        zeros = np.zeros(n, np.int32)
        dev = torch.device(device)
        self.ids_d = torch.from_numpy(ids).to(dev)
        self.len_d = torch.from_numpy(self.lengths).to(dev)
        self.ent_d = torch.from_numpy(ent).to(dev)
        self.cnt_d = torch.from_numpy(self.ent_counts).to(dev)
        self.cat_d = torch.from_numpy(np.asarray(category if category is not None else zeros, np.int32)).to(dev)
        self.sent_d = torch.from_numpy(np.asarray(sentiment if sentiment is not None else zeros, np.int32)).to(dev)
        self.score_d = torch.from_numpy(np.asarray(sentiment_score if sentiment_score is not None else zeros, np.float32)).to(dev)
        self.device = dev

    @classmethod
    def from_arrays(cls, ids: np.ndarray, lengths: np.ndarray, pad_id: int, device: Union[str, torch.device] = "cuda"):
        """Store over an already padded token matrix int32 [N, L] (row i = news i; nids are the row numbers)."""
        self = cls.__new__(cls)
        n = ids.shape[0]
        dev = torch.device(device)
        self.nid2row = None
        self.pad_id = int(pad_id)
        self.lengths = np.ascontiguousarray(lengths, np.int32)
        self.ent_counts = np.zeros(n, np.int32)
        self.ids_d = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(dev)
        self.len_d = torch.from_numpy(self.lengths).to(dev)
        self.ent_d = torch.zeros((n, 1), dtype=torch.int32, device=dev)
        self.cnt_d = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.cat_d = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.sent_d = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.score_d = torch.zeros((n,), dtype=torch.float32, device=dev)
        self.device = dev
        return self

    def __len__(self) -> int:
        return int(self.lengths.shape[0])


# ---------------------------------------------------------------------------------------------- collate
def _collate_side(st: "NewsStore", rows_d: torch.Tensor, off_d: torch.Tensor, total: int, lp: int, width: int):
    """Segment ids and the news tensors of one side (history or candidates) of a batch: store rows ``rows_d`` [total], CSR offsets
    ``off_d``, text padded to ``lp`` and entities to ``width``."""
    seg = hip.collate_segments_sized(off_d, total)
    ids, mask = hip.collate_text(st.ids_d, st.len_d, rows_d, lp, st.pad_id)
    ent = hip.collate_entities(st.ent_d, st.cnt_d, rows_d, width)
    cat, sent, score = hip.collate_aspects(st.cat_d, st.sent_d, st.score_d, rows_d)
    x = {"text": {"input_ids": ids, "attention_mask": mask}, "entities": ent, "category": cat, "sentiment": sent,
         "sentiment_score": score}
    return seg, x


class DeviceCollate:
    """``MINDCollate`` with the store on the device: ``collate(indices) -> MINDRecBatch``.

    ``indices`` is the list of behaviour rows a DataLoader batch holds (any order); a contiguous ``range``
    is served from device-resident slices without any host-to-device copy.
    """

    def __init__(self, store: NewsStore, behaviors: ParsedBehaviors):
        self.store, self.bhv = store, behaviors
        dev = store.device
        self.hist_rows_d = torch.from_numpy(behaviors.hist_rows).to(dev)
        self.cand_rows_d = torch.from_numpy(behaviors.cand_rows).to(dev)
        self.labels_d = torch.from_numpy(behaviors.labels).to(dev)
        self.users_d = torch.from_numpy(behaviors.users).to(dev)

    def _side(self, rows_d: torch.Tensor, rows_h: np.ndarray, sizes: np.ndarray):
        st = self.store
        off = np.zeros(sizes.shape[0] + 1, np.int64)
        np.cumsum(sizes, out=off[1:])
        off_d = torch.from_numpy(off).to(st.device, non_blocking=True)
        lp = int(st.lengths[rows_h].max()) if rows_h.size else 0          # tokenizer padding=True: batch max
        width = int(st.ent_counts[rows_h].max()) if rows_h.size else 0    # _tokenize_entities: batch max
        return _collate_side(st, rows_d, off_d, int(off[-1]), lp, width)

    def __call__(self, indices: Union[range, Sequence[int]]) -> MINDRecBatch:
        b = self.bhv
        contiguous = isinstance(indices, range) and indices.step == 1 and len(indices) > 0
        if contiguous:
            i0, i1 = indices.start, indices.stop
            h0, h1, c0, c1 = int(b.hist_off[i0]), int(b.hist_off[i1]), int(b.cand_off[i0]), int(b.cand_off[i1])
            hist_h, cand_h = b.hist_rows[h0:h1], b.cand_rows[c0:c1]
            hist_d, cand_d = self.hist_rows_d[h0:h1], self.cand_rows_d[c0:c1]
            labels, users = self.labels_d[c0:c1], self.users_d[i0:i1]
            hs, cs = np.diff(b.hist_off[i0:i1 + 1]), np.diff(b.cand_off[i0:i1 + 1])
        else:
            idx = np.asarray(list(indices), np.int64)
            hs, cs = (b.hist_off[idx + 1] - b.hist_off[idx]), (b.cand_off[idx + 1] - b.cand_off[idx])
            take = lambda off, sizes: (np.concatenate([np.arange(off[i], off[i] + s) for i, s in zip(idx, sizes)])
                                       if idx.size else np.zeros(0, np.int64))
            hsel, csel = take(b.hist_off, hs), take(b.cand_off, cs)
            hist_h, cand_h = b.hist_rows[hsel], b.cand_rows[csel]
            dev = self.store.device
            hist_d, cand_d = torch.from_numpy(hist_h).to(dev), torch.from_numpy(cand_h).to(dev)
            labels, users = torch.from_numpy(b.labels[csel]).to(dev), torch.from_numpy(b.users[idx]).to(dev)
        batch_hist, x_hist = self._side(hist_d, hist_h, hs)
        batch_cand, x_cand = self._side(cand_d, cand_h, cs)
        batch = MINDRecBatch(batch_hist=batch_hist, batch_cand=batch_cand, x_hist=x_hist, x_cand=x_cand, labels=labels,
                             users=users)
        # host-known extras (not part of the reference's TypedDict; its consumers ignore them): the widths of the dense
        # [B, max, *] views, so that K9 needs no device read-back (to_dense_batch computes them with a sync)
        batch["hist_max"] = int(hs.max()) if hs.size else 0
        batch["cand_max"] = int(cs.max()) if cs.size else 0
        return batch


# ---------------------------------------------------------------------------------------------- training batches
def _segment_reduce(ufunc, values: np.ndarray, off: np.ndarray, dtype) -> np.ndarray:
    """``ufunc.reduceat`` over CSR segments, 0 for an empty one (reduceat alone returns the element at its start)."""
    sizes = np.diff(off)
    out = np.zeros(sizes.shape[0], dtype)
    full = sizes > 0
    if full.any():
        out[full] = ufunc.reduceat(values, off[:-1][full])
    return out


def click_counts(behaviors: ParsedBehaviors):
    """(p, q) int64 [n_imp]: clicked (label == 1) and non-clicked (label == 0) candidates per impression; any other label counts
    as neither, as in the reference's ``np.where(labels == 1)`` / ``== 0`` (:53-54).  Computed once per data set."""
    got = behaviors.__dict__.get("_click_counts")
    if got is None:
        lab = behaviors.labels
        got = (_segment_reduce(np.add, (lab == 1).astype(np.int64), behaviors.cand_off, np.int64),
               _segment_reduce(np.add, (lab == 0).astype(np.int64), behaviors.cand_off, np.int64))
        behaviors.__dict__["_click_counts"] = got
    return got


def impression_widths(behaviors: ParsedBehaviors, lengths: np.ndarray, ent_counts: np.ndarray) -> Dict[str, np.ndarray]:
    """Per impression, the longest token row and entity list among its history and among ALL its candidates (int64 [n_imp] each):
    what the padded widths of a batch are made of, once per data set."""
    b = behaviors
    return {"hist_text": _segment_reduce(np.maximum, lengths[b.hist_rows], b.hist_off, np.int64),
            "hist_ent": _segment_reduce(np.maximum, ent_counts[b.hist_rows], b.hist_off, np.int64),
            "cand_text": _segment_reduce(np.maximum, lengths[b.cand_rows], b.cand_off, np.int64),
            "cand_ent": _segment_reduce(np.maximum, ent_counts[b.cand_rows], b.cand_off, np.int64)}


@dataclass
class TrainBatchPlan:
    """What the host knows of a sampled batch before anything is drawn: every size, no content."""
    indices: np.ndarray       # int64 [B]  impressions of the batch
    hist_sizes: np.ndarray    # int64 [B]
    hist_off: np.ndarray      # int64 [B+1]
    p: np.ndarray             # int64 [B]  clicked candidates
    q: np.ndarray             # int64 [B]  non-clicked candidates
    m: np.ndarray             # int64 [B]  negatives drawn = ratio * p
    out_off: np.ndarray       # int64 [B+1] prefix sum of p + m: the sampled candidates' offsets
    hist_max: int
    cand_max: int             # max p * (1 + ratio)
    hist_text_width: int = 0  # exact (the history is not sampled); the four widths are 0 without ``widths``
    hist_ent_width: int = 0
    cand_text_bound: int = 0  # upper bounds: over all candidates of the batch's impressions that have a click
    cand_ent_bound: int = 0


def plan_train_batch(behaviors: ParsedBehaviors, indices: Union[range, Sequence[int], np.ndarray], ratio: int,
                     widths: Optional[Dict[str, np.ndarray]] = None) -> TrainBatchPlan:
    """Sizes and offsets of the training batch over the impressions ``indices`` (any order, repeats allowed) — pure numpy.
    An impression with clicks and no non-clicked candidate raises ``ValueError`` here, before any launch: it is the case in which
    the reference's ``np.random.choice`` raises (:59-63).  ``widths``: ``impression_widths`` of the data set."""
    if ratio < 1:
        raise ValueError("neg_sampling_ratio must be at least 1")
    idx = np.asarray(indices if not isinstance(indices, range) else np.arange(indices.start, indices.stop, indices.step), np.int64)
    idx = idx.reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= len(behaviors)):
        raise IndexError(f"impression index outside [0, {len(behaviors)})")
    p_all, q_all = click_counts(behaviors)
    p, q = p_all[idx], q_all[idx]
    bad = np.flatnonzero((p > 0) & (q == 0))
    if bad.size:
        raise ValueError(f"impression {int(idx[bad[0]])} has clicks and no non-clicked candidate to sample from")
    m = ratio * p
    hs = behaviors.hist_off[idx + 1] - behaviors.hist_off[idx]
    hist_off, out_off = np.zeros(idx.size + 1, np.int64), np.zeros(idx.size + 1, np.int64)
    np.cumsum(hs, out=hist_off[1:])
    np.cumsum(p + m, out=out_off[1:])
    plan = TrainBatchPlan(idx, hs, hist_off, p, q, m, out_off, int(hs.max()) if idx.size else 0, int((p + m).max()) if idx.size else 0)
    if widths is not None and idx.size:
        clicked = p > 0                               # an impression without a click contributes no candidate
        plan.hist_text_width, plan.hist_ent_width = int(widths["hist_text"][idx].max()), int(widths["hist_ent"][idx].max())
        if clicked.any():
            plan.cand_text_bound = int(widths["cand_text"][idx[clicked]].max())
            plan.cand_ent_bound = int(widths["cand_ent"][idx[clicked]].max())
    return plan


class DeviceTrainCollate:
    """``MINDRecDatasetTrain`` + ``MINDCollate`` with the data set on the device: ``collate(indices) -> MINDRecBatch`` of the
    impressions ``indices`` with their candidates sampled (every click, ``neg_sampling_ratio`` non-clicked per click, shuffled)
    by two launches in front of the ``collate_*`` kernels.  A sample is a pure function of (``seed``, epoch, impression): call
    ``set_epoch`` once per epoch, as with a ``DistributedSampler``.

    ``indices``: a ``range``, a sequence, or an int64 tensor on the device.  The host needs the indices to size the batch, so a
    device tensor should be a contiguous slice of what ``upload_order`` returned (a whole epoch's permutation, uploaded once; the
    host keeps its copy); any other device tensor is read back, which synchronises.

    Default mode: NO device-to-host read per call.  The sampled candidates' text / entity tensors are padded to host-known
    upper bounds (the longest among ALL candidates of the batch's impressions): pad id, mask 0, entity 0 beyond the sampled
    batch's real maximum — the encoders pack real tokens, so the extra columns cost nothing downstream.
    ``exact_width=True`` reads the sampled batch's two maxima back (ONE synchronising read of two integers per call) and trims
    the candidate tensors to the reference's ``padding=True`` widths.  The history side is exact in both modes.

    Bad input raises through the device status word like the scoring kernels' (at the next ``hotpath`` call's poll or
    ``hip.check_status``); an impression with clicks and nothing to sample raises ``ValueError`` on the host."""

    def __init__(self, store: NewsStore, behaviors: ParsedBehaviors, neg_sampling_ratio: int = 4, seed: int = 0,
                 exact_width: bool = False):
        if neg_sampling_ratio < 1:
            raise ValueError("neg_sampling_ratio must be at least 1")
        self.store, self.bhv = store, behaviors
        self.ratio, self.seed, self.exact_width, self.epoch = int(neg_sampling_ratio), int(seed), bool(exact_width), 0
        dev = store.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.hist_rows_d, self.hist_off_d = up(behaviors.hist_rows), up(behaviors.hist_off)
        self.cand_rows_d, self.cand_off_d = up(behaviors.cand_rows), up(behaviors.cand_off)
        self.labels_d, self.users_d = up(behaviors.labels), up(behaviors.users)
        self.widths = impression_widths(behaviors, store.lengths, store.ent_counts)
        click_counts(behaviors)
        self._order_h: Optional[np.ndarray] = None
        self._order_d: Optional[torch.Tensor] = None

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def upload_order(self, order: Union[Sequence[int], np.ndarray]) -> torch.Tensor:
        """Upload an epoch's impression order once; slices of the returned int64 device tensor are batches for ``__call__``."""
        order_h = np.ascontiguousarray(np.asarray(order, np.int64).reshape(-1)).copy()
        if order_h.size and (order_h.min() < 0 or order_h.max() >= len(self.bhv)):
            raise IndexError(f"impression index outside [0, {len(self.bhv)})")
        self._order_h, self._order_d = order_h, torch.from_numpy(order_h).to(self.store.device)
        return self._order_d

    def _indices(self, indices):
        """-> (host int64 array, the same on the device or None)."""
        if isinstance(indices, torch.Tensor):
            if indices.dtype != torch.int64 or indices.dim() != 1:
                raise TypeError("a tensor of impression indices must be int64 and one-dimensional")
            if not indices.is_cuda:
                return indices.numpy(), None
            o = self._order_d
            if (o is not None and indices.is_contiguous()
                    and indices.untyped_storage().data_ptr() == o.untyped_storage().data_ptr()):
                s = indices.storage_offset()
                return self._order_h[s:s + indices.numel()], indices
            return indices.cpu().numpy(), indices.contiguous()           # a foreign device tensor: one synchronising read
        return indices, None

    def __call__(self, indices) -> MINDRecBatch:
        idx_h, idx_d = self._indices(indices)
        plan = plan_train_batch(self.bhv, idx_h, self.ratio, self.widths)
        nb, dev = plan.indices.size, self.store.device
        # one host-to-device copy per batch: the two offset arrays (and the indices, unless they are on the device already)
        parts = [plan.hist_off, plan.out_off] + ([plan.indices] if idx_d is None else [])
        packed = torch.from_numpy(np.concatenate(parts)).to(dev, non_blocking=True)
        hist_off_d, out_off_d = packed[:nb + 1], packed[nb + 1:2 * nb + 2]
        if idx_d is None:
            idx_d = packed[2 * nb + 2:]
        n_hist, n_cand = int(plan.hist_off[-1]), int(plan.out_off[-1])
        cand_d, labels, users, _ = hip.sample_candidates(self.cand_rows_d, self.labels_d, self.cand_off_d, idx_d, out_off_d, n_cand,
                                                         self.ratio, self.seed, self.epoch, users=self.users_d)
        hist_d = hip.gather_segments(self.hist_rows_d, self.hist_off_d, idx_d, hist_off_d, n_hist)
        lp, width = plan.cand_text_bound, plan.cand_ent_bound
        if self.exact_width:
            lp, width = hip.rows_max_len(self.store.len_d, cand_d, self.store.cnt_d).tolist()     # the documented synchronising read
        batch_hist, x_hist = _collate_side(self.store, hist_d, hist_off_d, n_hist, plan.hist_text_width, plan.hist_ent_width)
        batch_cand, x_cand = _collate_side(self.store, cand_d, out_off_d, n_cand, lp, width)
        batch = MINDRecBatch(batch_hist=batch_hist, batch_cand=batch_cand, x_hist=x_hist, x_cand=x_cand, labels=labels, users=users)
        batch["hist_max"], batch["cand_max"] = plan.hist_max, plan.cand_max       # host-known, as in DeviceCollate
        return batch
