"""numpy restatement of the training sampler's rule (include/manner_hip.h, "training batches"): the device is held to this
to the bit.  Everything is arithmetic modulo 2^64 on uint64 arrays (which wrap silently in numpy).

For an impression with positions 0..n-1, P = positions with label == 1 (p of them), N = positions with label == 0 (q of them),
m = ratio * p:
  m <= q: S = the m negatives with the smallest (key(stream 0, slot = position), position), in that order;
  m >  q: draw t = 0..m-1 is the r-th negative in position order, r = ((key(stream 1, slot t) >> 32) * q) >> 32;
  the list [P in position order, then S] is returned in ascending order of (key(stream 2, slot s), s).
"""
import numpy as np

_U = np.uint64
GOLDEN = 0x9E3779B97F4A7C15


def mix(x):
    shape = np.shape(x)
    x = np.array(x, dtype=_U, ndmin=1)                 # (a copy; at least 1-d, so that the products wrap as array arithmetic does)
    x ^= x >> _U(30)
    x *= _U(0xBF58476D1CE4E5B9)
    x ^= x >> _U(27)
    x *= _U(0x94D049BB133111EB)
    x ^= x >> _U(31)
    return x.reshape(shape)


def key(seed, epoch, imp, stream, slot):
    """uint64 array of the shape of ``slot``."""
    s0 = (int(seed) + GOLDEN * (int(epoch) + 1)) % (1 << 64)
    base = mix(mix(_U(s0)) ^ _U(int(imp)))
    return mix(base ^ (_U(int(stream) << 32) | np.asarray(slot, dtype=_U)))


def _order(keys):
    """Indices in ascending (key, index) order."""
    return np.lexsort((np.arange(keys.shape[0]), keys))


def sample(labels, ratio, seed, epoch, imp):
    """-> int64 positions, p * (1 + ratio) of them."""
    labels = np.asarray(labels)
    pos = np.flatnonzero(labels == 1)
    neg = np.flatnonzero(labels == 0)
    p, q = pos.size, neg.size
    m = ratio * p
    if p == 0:
        return np.zeros(0, np.int64)
    if q == 0 and m > 0:
        raise ValueError("an impression with clicks and no negative cannot be sampled")
    if m <= q:
        chosen = neg[_order(key(seed, epoch, imp, 0, neg))[:m]]
    else:
        k = key(seed, epoch, imp, 1, np.arange(m))
        r = ((k >> _U(32)) * _U(q)) >> _U(32)
        chosen = neg[r.astype(np.int64)]
    listed = np.concatenate([pos, chosen]).astype(np.int64)
    return listed[_order(key(seed, epoch, imp, 2, np.arange(listed.size)))]
