"""numpy restatement of the M-per-class sampling rule (include/manner_hip.h, "A-Module batches"): the device is held to this to
the bit.  ``key`` is the training sampler's (tests/train_sample_ref.py), its third argument the batch or the unit.

The distinct labels in ascending value are the classes 0..L-1; the members of a class are data-set indices in ascending order.
An epoch is nb = N // batch_size batches of k = batch_size // m blocks of m slots:
  class choice of batch b: the k classes with the smallest (key(stream 16, imp = b, slot = l), l), in that order;
  block j of batch b has unit = b * k + j and draws from its class of n members, h_t = key(stream 17, imp = unit, slot = t) >> 32:
    n >= m (Floyd's subset algorithm): for t = 0..m-1: J = n - m + t, r = (h_t * (J + 1)) >> 32; append J if r was appended before,
            else r;
    n <  m: draw t is (h_t * n) >> 32;
  the block lists the drawn members in draw order (not a uniform permutation of the subset, and it need not be: the consumers of a
  batch are equivariant to the order inside it).
"""
import numpy as np

from train_sample_ref import key

_U = np.uint64


def class_tables(labels):
    """-> (class_label int64 [L], class_off int64 [L + 1], class_members int64 [N] grouped by class, ascending inside a class)."""
    labels = np.asarray(labels, np.int64)
    class_label, counts = np.unique(labels, return_counts=True)
    members = np.concatenate([np.flatnonzero(labels == v) for v in class_label]) if labels.size else np.zeros(0, np.int64)
    return class_label, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), members.astype(np.int64)


def choose_classes(n_classes, k, seed, epoch, b):
    """-> int64 [k]: the classes of batch ``b`` in block order."""
    keys = key(seed, epoch, b, 16, np.arange(n_classes))
    return np.lexsort((np.arange(n_classes), keys))[:k].astype(np.int64)


def draw(n, m, seed, epoch, unit):
    """-> int64 [m]: positions in a class of ``n`` members, in draw order."""
    h = key(seed, epoch, unit, 17, np.arange(m)) >> _U(32)
    if n < m:
        return ((h * _U(n)) >> _U(32)).astype(np.int64)
    out = []
    for t in range(m):
        J = n - m + t
        r = int((h[t] * _U(J + 1)) >> _U(32))
        out.append(J if r in out else r)
    return np.asarray(out, np.int64)


def sample_batch(tables, m, k, seed, epoch, b):
    """-> (data-set indices int64 [k * m], labels int64 [k * m]) of batch ``b``."""
    class_label, class_off, members = tables
    idx, lab = [], []
    for j, c in enumerate(choose_classes(class_label.size, k, seed, epoch, b)):
        beg, n = int(class_off[c]), int(class_off[c + 1] - class_off[c])
        idx.append(members[beg + draw(n, m, seed, epoch, b * k + j)])
        lab.append(np.full(m, class_label[c], np.int64))
    return np.concatenate(idx), np.concatenate(lab)


def sample_epoch(labels, m, batch_size, seed, epoch):
    """-> (indices int64 [nb, batch_size], labels int64 [nb, batch_size]); ``ValueError`` where MPerClassSampler asserts."""
    labels = np.asarray(labels, np.int64)
    tables = class_tables(labels)
    if labels.size < batch_size:
        raise ValueError("fewer news than one batch")
    if batch_size % m != 0:
        raise ValueError("batch_size is not a multiple of m")
    if m * tables[0].size < batch_size:
        raise ValueError("too few classes to fill a batch")
    k, nb = batch_size // m, labels.size // batch_size
    got = [sample_batch(tables, m, k, seed, epoch, b) for b in range(nb)]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
