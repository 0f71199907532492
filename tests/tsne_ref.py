"""A float64 restatement of manner_amd.manifold.TSNE (the published t-SNE with kNN affinities and exact forces), the inputs the GPU
tests run the kernels on, and the two bars they are held to.  No GPU in this file: tests/test_tsne_host.py checks the restatement, the
bars and the planted defects on the CPU, tests/test_gpu_tsne.py runs the kernels against it.

Everything is dense ([N, N] arrays: fine at test sizes) and dtype-generic: evaluated in float64 it is the reference, evaluated in float32
on the CPU it is the yardstick of the MEASURED bar.

DERIVED bar (the squared distances, pure sums of squares): |got - ref64| <= (D + 4) 2^-24 sum_d (x_id - x_jd)^2 — D roundings of the
fmaf chain, the rounding of each difference (twice its relative error in the square), and slack for the order.

MEASURED bar (everything with exp, log or a reciprocal inside): 8 x the error of this restatement in float32 on the CPU against float64,
relative to the tensor's largest entry, floored at 2^-25 (a float32 result sits up to half an ulp of itself from float64 whatever
computed it).  A CPU figure strictly between 0 and 2^-25 is the luck of one rounding: such inputs are redrawn (``settled``), a condition
on the reference side alone.

Planted defects: every function takes ``defect``, a string naming ONE deliberate error of the kind a kernel could make; the host tests
show that each moves an asserted quantity at least ten-fold past its bar on the GPU tests' own inputs.
"""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import numpy as np
import torch

U32 = 2.0 ** -24
FLOOR = 2.0 ** -25
MEASURED_FACTOR = 8.0
TILE_I = TILE_J = 512          # manner_amd.hip.TSNE_TILE_I / _J: asserted equal by the host test
KNN_TILE_Q, KNN_TILE_C = 32, 64
TARGET_WG = 1024


def j_split(n: int) -> int:
    if n <= 0:
        return 1
    nb, jt = -(-n // TILE_I), -(-n // TILE_J)
    return max(1, min(-(-TARGET_WG // nb), jt))


# ------------------------------------------------------------------------------------------------ bars
def rel_to_max(got, ref64) -> float:
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    if not ref64.size:
        return 0.0
    err, scale = float(np.abs(got - ref64).max()), float(np.abs(ref64).max())
    return err / scale if scale > 0 else err


def measured_bar(ref32, ref64) -> Dict[str, float]:
    cpu = rel_to_max(ref32, ref64)
    return {"cpu_f32": cpu, "bar": max(MEASURED_FACTOR * cpu, FLOOR)}


def lucky(bars: Dict[str, Dict[str, float]]) -> bool:
    return any(0 < b["cpu_f32"] < FLOOR for b in bars.values())


def settled(build):
    """build(salt) -> (anything, {name: measured_bar}) at the first salt without a lucky rounding"""
    for salt in range(32):
        out = build(salt * 100003)
        if not lucky(out[1]):
            return out
    raise AssertionError("no salt in 32 settles the case")


def d2_bound(d2_ref64, D: int):
    return (D + 4) * U32 * np.asarray(d2_ref64, np.float64)


# ------------------------------------------------------------------------------------------------ steps 1-3
def normalise(X, dt=np.float64):
    X = np.asarray(X).astype(dt)
    X = X - X.mean(0, keepdims=True)
    return X / np.abs(X).max()


def sqdist(X) -> np.ndarray:
    """[N, N] float64: direct sums of squared differences"""
    X = np.asarray(X, np.float64)
    out = np.zeros((len(X), len(X)))
    for d in range(X.shape[1]):
        out += np.subtract.outer(X[:, d], X[:, d]) ** 2
    return out


def knn(X, k: int, defect: Optional[str] = None, dist: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(idx int32 [N, k], d2 float64 [N, k]): exact, the row itself excluded, ascending by (d2, idx)"""
    D2 = sqdist(X) if dist is None else dist
    n = len(D2)
    if n - 1 < k:
        raise ValueError("N - 1 < k")
    key = D2.copy()
    np.fill_diagonal(key, np.inf)
    if defect == "ties_high":
        order = (n - 1 - np.argsort(key[:, ::-1], axis=1, kind="stable"))[:, :k]
    else:
        order = np.argsort(key, axis=1, kind="stable")[:, :k]
    if defect == "drop_kth":
        order = order.copy()
        order[:, k - 1] = order[:, max(k - 2, 0)]
    return order.astype(np.int32), np.take_along_axis(D2, order, 1)


def kth_gap(X, k: int) -> np.ndarray:
    """per row the float64 gap between its k-th and (k + 1)-th distance (inf where there is no (k + 1)-th)"""
    D2 = sqdist(X)
    np.fill_diagonal(D2, np.inf)
    s = np.sort(D2, axis=1)
    return s[:, k] - s[:, k - 1] if k < len(D2) - 1 else np.full(len(D2), np.inf)


def affinities(d2, perplexity: float, dt=np.float64, trips: Optional[list] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(p [N, k], beta [N]) in ``dt``: the binary search of the published implementation, on distances relative to the row's smallest
    (p and H do not change under the shift); beta saturates at the largest finite ``dt``.  ``trips``: a list that receives the number
    of trips each row took"""
    d = np.asarray(d2).astype(dt)
    d = d - d.min(1, keepdims=True)
    n, k = d.shape
    half, two, big = dt(0.5), dt(2), np.finfo(dt).max
    beta, lo, hi = np.ones(n, dt), np.zeros(n, dt), np.zeros(n, dt)
    has_lo, has_hi, done = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    P, S0, used, count = np.zeros((n, k), dt), np.ones(n, dt), np.ones(n, dt), np.zeros(n, np.int64)
    logp = np.log(dt(perplexity))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for _ in range(200):
            a = np.flatnonzero(~done)
            if not len(a):
                break
            b = beta[a]
            pv = np.exp(-b[:, None] * d[a])
            s0, s1 = pv.sum(1, dtype=dt), (d[a] * pv).sum(1, dtype=dt)
            diff = (b * s1 / s0 + np.log(s0)) - logp
            P[a], S0[a], used[a] = pv, s0, b
            count[a] += 1
            fin = np.abs(diff) < dt(1e-5)
            up, dn = (diff > 0) & ~fin, ~(diff > 0) & ~fin
            iu, idn = a[up], a[dn]
            lo[iu], has_lo[iu] = b[up], True
            beta[iu] = np.where(has_hi[iu], half * b[up] + half * hi[iu], np.minimum(b[up] * two, big))
            hi[idn], has_hi[idn] = b[dn], True
            beta[idn] = np.where(has_lo[idn], half * b[dn] + half * lo[idn], b[dn] * half)
            done[a[fin]] = True
    if trips is not None:
        trips.append(count)
    return P / S0[:, None], used


def perplexities(p) -> np.ndarray:
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.exp(-np.where(p > 0, p * np.log(p), 0.0).sum(1))


def joint(idx, p, defect: Optional[str] = None) -> np.ndarray:
    """[N, N] float64: P = (P_cond + P_cond^T) / (2 N) from the directed edge list — edge (i -> j, p) adds p / (2 N) to P_ij and P_ji"""
    idx, p = np.asarray(idx), np.asarray(p, np.float64)
    n, k = idx.shape
    Pc = np.zeros((n, n))
    np.add.at(Pc, (np.repeat(np.arange(n), k), idx.reshape(-1)), p.reshape(-1))
    if defect == "no_incoming":
        return Pc / (2.0 * n)
    if defect == "incoming_first_k":                                  # of every row's incoming edges (ascending source) only the first k
        keep = np.cumsum(Pc > 0, axis=0) <= k
        return (Pc + (Pc * keep).T) / (2.0 * n)
    return (Pc + Pc.T) / (2.0 * n)


# ------------------------------------------------------------------------------------------------ steps 5-6 (torch, batched over leading dims)
def repulsion(Y: torch.Tensor, defect: Optional[str] = None):
    """rows [.., N, 3] = (sum_j q^2 dx, sum_j q^2 dy, sum_j q) over ALL j — the self pair, q = 1 and force 0, included, as the kernel
    has it — and Z = (sum of the row sums) - N"""
    n = Y.shape[-2]
    dx = Y[..., :, None, 0] - Y[..., None, :, 0]
    dy = Y[..., :, None, 1] - Y[..., None, :, 1]
    q = 1.0 / (1.0 + dx * dx + dy * dy)
    if defect in ("drop_last_tile", "drop_second_partial"):
        jt = -(-n // TILE_J)
        s = j_split(n)
        gone = range((jt - 1) * TILE_J, n) if defect == "drop_last_tile" else range((1 * jt // s) * TILE_J, min(n, (2 * jt // s) * TILE_J))
        q = q.clone()
        q[..., :, list(gone)] = 0
    q2 = q * q
    rows = torch.stack([(q2 * dx).sum(-1), (q2 * dy).sum(-1), q.sum(-1)], -1)
    Z = rows[..., 2].sum(-1) - (0 if defect == "self_in_z" else n)
    return rows, Z


def gradient(P: torch.Tensor, Y: torch.Tensor, exaggeration: float = 1.0, defect: Optional[str] = None) -> torch.Tensor:
    """dY_i = exaggeration sum_j P_ij q_ij (y_i - y_j) - (1 / Z) sum_j q_ij^2 (y_i - y_j): no factor 4"""
    dx = Y[..., :, None, 0] - Y[..., None, :, 0]
    dy = Y[..., :, None, 1] - Y[..., None, :, 1]
    q = 1.0 / (1.0 + dx * dx + dy * dy)
    w = P * q
    att = torch.stack([(w * dx).sum(-1), (w * dy).sum(-1)], -1)
    if defect in ("drop_last_tile", "drop_second_partial", "self_in_z"):
        rows, Z = repulsion(Y, defect)
    else:                                                                # repulsion(Y), from the q at hand
        q2 = q * q
        rows = torch.stack([(q2 * dx).sum(-1), (q2 * dy).sum(-1), q.sum(-1)], -1)
        Z = rows[..., 2].sum(-1) - Y.shape[-2]
    return exaggeration * att - rows[..., :2] / Z[..., None, None]


def step(P, Y, u, gains, exaggeration, momentum, lr, defect: Optional[str] = None):
    dY = gradient(P, Y, exaggeration, defect)
    differ = torch.sign(dY) != torch.sign(u)
    if defect == "gains_eq":
        differ = ~differ
    gains = torch.where(differ, gains + 0.2, gains * 0.8).clamp(min=0.01)
    u = momentum * u - lr * gains * dY
    Y = Y + u
    if defect != "no_centring":
        Y = Y - Y.mean(-2, keepdim=True)
    return Y, u, gains, dY


def kl_divergence(P: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    dx = Y[..., :, None, 0] - Y[..., None, :, 0]
    dy = Y[..., :, None, 1] - Y[..., None, :, 1]
    q = 1.0 / (1.0 + dx * dx + dy * dy)
    n = Y.shape[-2]
    Z = (q.sum((-1, -2)) - n)[..., None, None]
    Pn = torch.where(P > 0, P, torch.ones_like(P))
    return torch.where(P > 0, P * torch.log(Pn * Z / q), torch.zeros_like(P)).sum((-1, -2))


def iterate(P, Y0, n_iter, early_exaggeration=12.0, learning_rate=200.0, n_iter_early_exag=250, defect: Optional[str] = None, watch=None):
    """n_iter iterations from Y0 ([.., N, 2]: leading dims are independent runs over one P).  ``watch``: a list that receives per
    iteration min |dY| / max |dY| over the non-zero entries."""
    Y, u, gains = Y0, torch.zeros_like(Y0), torch.ones_like(Y0)
    for it in range(n_iter):
        early = it < n_iter_early_exag
        ex = early_exaggeration if early or defect == "exaggeration_stays" else 1.0
        mom = 0.5 if early or defect == "momentum_stays" else 0.8
        Y, u, gains, dY = step(P, Y, u, gains, ex, mom, learning_rate, defect)
        if watch is not None:
            a = dY.abs()
            watch.append(float(a[a > 0].min() / a.max()))
    return Y


def fit(X, perplexity=30.0, n_iter=1000, random_state=None, dt=np.float64, Y0=None, **kw):
    """The whole of TSNE.fit_transform in ``dt`` -> (Y, KL, (idx, p)).  In float32 every stage runs in float32 from the float32 X."""
    tdt = torch.float64 if dt == np.float64 else torch.float32
    Xn = normalise(np.asarray(X, dt), dt)
    k = int(3 * perplexity)
    idx, d2 = knn(Xn, k)
    p, _ = affinities(d2.astype(dt), perplexity, dt)
    P = torch.from_numpy(joint(idx, p)).to(tdt)
    if Y0 is None:
        Y0 = 1e-4 * np.random.RandomState(random_state).randn(len(Xn), 2)
    Y = iterate(P, torch.from_numpy(np.asarray(Y0, np.float32)).to(tdt), n_iter, **kw)
    return Y, kl_divergence(P, Y), (idx, p)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def line_points(seed: int, n: int, d: int) -> np.ndarray:
    """float32 [n, d]: generic positions along one direction plus a little noise — neighbour ranks are well separated at every D"""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 1, n)) * n
    v = rng.standard_normal(d)
    v /= np.linalg.norm(v)
    return (np.outer(rng.permutation(t), v) + 0.01 * rng.standard_normal((n, d))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def knn_continuous(n: int, d: int, k: int):
    """(X, idx, d2, rows left out) at the first seed whose every row has a float64 gap between its k-th and (k + 1)-th distance above
    twice the derived bar"""
    for seed in range(64):
        X = line_points(1000 * seed + n + d + k, n, d)
        idx, d2 = knn(X, k)
        left_out = int((kth_gap(X, k) <= 2 * d2_bound(d2[:, k - 1], d)).sum())
        if left_out == 0:
            return X, idx, d2, left_out
    raise AssertionError("no seed in 64 separates the ranks")


@functools.lru_cache(maxsize=None)
def knn_integer(n: int, d: int, k: int, kind: str):
    """Integer-valued rows (distances exact in float32): 'dup' few distinct values, duplicate rows and many ties; 'same' every row equal
    (every distance 0: the order is the index order across every candidate-tile edge); 'runs' blocks of equal rows longer than a tile"""
    rng = np.random.default_rng(n * 7 + d * 3 + k)
    if kind == "same":
        X = np.full((n, d), 2.0, np.float32)
    elif kind == "runs":
        X = np.repeat(rng.integers(0, 3, (-(-n // 70), d)), 70, axis=0)[:n].astype(np.float32)
    else:
        X = rng.integers(0, 3 if d > 8 else 2, (n, d)).astype(np.float32)
    idx, d2 = knn(X, k)
    return X, idx, d2


KNN_SHAPES = [(2, 1, 1), (31, 1, 1), (31, 256, 30), (32, 3, 30), (33, 256, 30), (63, 768, 30), (64, 1024, 1), (65, 3, 30), (91, 256, 90),
              (129, 256, 90), (256, 3, 255), (257, 1024, 255), (300, 768, 90)]


def affinity_rows(kind: str, k: int, salt: int = 0) -> np.ndarray:
    """float32 [rows, k] squared distances, ascending per row"""
    rng = np.random.default_rng(17 + k + salt)
    rows = 261
    base = np.sort(rng.gamma(4.0, 2.0, (rows, k)), axis=1)
    if kind == "continuous":
        d = base
    elif kind == "constant":
        d = np.repeat(rng.uniform(0.1, 50.0, (rows, 1)), k, axis=1)
    elif kind == "zero":
        d = np.zeros((rows, k))
    elif kind == "doubling":                                            # beta ends above 2^30
        d = base * 10.0 ** -rng.uniform(10, 14, (rows, 1))
    elif kind == "halving":                                             # beta ends below 2^-30
        d = base * 10.0 ** rng.uniform(10, 14, (rows, 1))
    else:
        raise KeyError(kind)
    return d.astype(np.float32)


AFFINITY_KINDS = ("continuous", "constant", "zero", "doubling", "halving")


@functools.lru_cache(maxsize=None)
def affinity_case(kind: str, k: int):
    """(d2, p64, beta64, perplexity, bars) settled.  The search ends at the first trip with |H - log perplexity| < 1e-5, so p is defined
    only up to which trip that is: ANY float32 evaluation, the kernel included, ends some rows one trip away from float64, and that
    moves p by orders more than rounding does.  A draw in which the float32 CPU evaluation happens to end every row on float64's trip
    measures rounding alone and says nothing about a float32 search: it is redrawn like a lucky rounding.  Not so where there is
    nothing to search: constant and zero rows (and k = 1) are uniform at every beta, p = 1 / k whatever is drawn."""
    perp = max(k / 3.0, 1.0)
    searching = k > 1 and kind not in ("constant", "zero")

    def build(salt):
        d2 = affinity_rows(kind, k, salt)
        t64, t32 = [], []
        p64, b64 = affinities(d2, perp, np.float64, t64)
        p32, _ = affinities(d2, perp, np.float32, t32)
        if searching and (t64[0] == t32[0]).all():
            return None, {"redraw": {"cpu_f32": FLOOR / 2, "bar": 0.0}}
        return (d2, p64, b64, perp), {"p": measured_bar(p32, p64)}
    (d2, p64, b64, perp), bars = settled(build) if searching else build(0)
    return d2, p64, b64, perp, bars


def repulsion_sizes():
    sizes = [1, 2, TILE_I - 1, TILE_I, TILE_I + 1, 2 * TILE_I + 1]
    first_split = next(n for n in range(1, 4 * TILE_I) if j_split(n) > 1)
    return sorted(set(sizes + [first_split]))


@functools.lru_cache(maxsize=None)
def repulsion_case(n: int, scale: float):
    """(Y float32, rows64, Z64, bars) settled"""
    def build(salt):
        Y = (np.random.default_rng(n + salt).standard_normal((n, 2)) * scale).astype(np.float32)
        r64, z64 = repulsion(torch.from_numpy(Y).double())
        r32, z32 = repulsion(torch.from_numpy(Y))
        bars = {"fx": measured_bar(r32[:, 0], r64[:, 0]), "fy": measured_bar(r32[:, 1], r64[:, 1]), "q": measured_bar(r32[:, 2], r64[:, 2])}
        if n > 1:
            bars["Z"] = measured_bar(z32, z64)
        return (Y, r64.numpy(), float(z64)), bars
    (Y, r64, z64), bars = settled(build)
    return Y, r64, z64, bars


def star_edges(seed: int, n: int, k: int):
    """A directed edge list [n, k] that no neighbour search made: every row but 0 points at the hub 0 (n - 1 > 1024 incoming edges), its
    other targets lie among the rows 1 .. 100, so the rows above 100 have no incoming edge at all; p random, each row summing to 1"""
    rng = np.random.default_rng(seed)
    idx = np.zeros((n, k), np.int32)
    for i in range(n):
        pool = np.setdiff1d(np.arange(1, 101), [i])
        idx[i] = np.sort(rng.choice(pool, k, replace=False)) if i == 0 else np.concatenate([[0], np.sort(rng.choice(pool, k - 1, replace=False))])
    p = rng.uniform(0.1, 1.0, (n, k))
    return idx, (p / p.sum(1, keepdims=True)).astype(np.float32)


STEP_KINDS = ("star_early", "star_late", "flat")


@functools.lru_cache(maxsize=None)
def step_case(kind: str):
    """One iteration on identical inputs.  'star_early': exaggeration 12, momentum 0.5; 'star_late': 1 and 0.8; 'flat': every point on
    one horizontal line, so dY_y is exactly 0 everywhere, against u_y both zero and non-zero.  A quarter of the gains sit at 0.011 (times
    0.8 falls below the 0.01 floor), a quarter of u is exactly 0.  Redrawn while any non-zero |dY| is below 1e-6 of the largest (a sign
    that float32 could flip), or a float32 figure is a lucky rounding."""
    n, k = 1201, 3
    ex, mom = (12.0, 0.5) if kind == "star_early" else (1.0, 0.8)

    def build(salt):
        rng = np.random.default_rng(99 + salt + len(kind))
        idx, p = star_edges(5 + salt, n, k)
        Y = (rng.standard_normal((n, 2)) * 3.0).astype(np.float32)
        if kind == "flat":
            Y[:, 1] = 0.5
        u = (rng.standard_normal((n, 2)) * 0.05).astype(np.float32)
        u[rng.uniform(size=(n, 2)) < 0.25] = 0.0
        gains = rng.uniform(0.5, 2.0, (n, 2)).astype(np.float32)
        gains[rng.uniform(size=(n, 2)) < 0.25] = 0.011
        P = joint(idx, p)
        out = {}
        for name, tdt in (("64", torch.float64), ("32", torch.float32)):
            t = lambda a: torch.from_numpy(np.asarray(a)).to(tdt)
            out[name] = step(t(P), t(Y), t(u), t(gains), ex, mom, 200.0)
        dY = out["64"][3].abs()
        if float(dY[dY > 0].min()) < 1e-6 * float(dY.max()):
            return None, {"redraw": {"cpu_f32": FLOOR / 2, "bar": 0.0}}
        bars = {nm: measured_bar(out["32"][i], out["64"][i]) for i, nm in enumerate(("Y", "u", "gains"))}
        return dict(idx=idx, p=p, Y=Y, u=u, gains=gains, P=P, ex=ex, mom=mom, lr=200.0, ref=[o.numpy() for o in out["64"]]), bars
    case, bars = settled(build)
    return case, bars


def cluster_points(seed: int, clusters: int, per: int, d: int):
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.standard_normal((clusters, d))
    labels = np.repeat(np.arange(clusters), per)
    return (centres[labels] + rng.standard_normal((clusters * per, d))).astype(np.float32), labels


@functools.lru_cache(maxsize=None)
def fit_case(n: int, perplexity: float, n_iter: int, n_iter_early_exag: int):
    """TSNE(perplexity, n_iter, n_iter_early_exag, random_state=0) on n clustered points in 16 dimensions -> (X, Y64, KL64, bars);
    redrawn while any |dY| of the float64 run falls below 1e-6 of that step's largest (a sign that float32 could flip)"""
    def build(salt):
        X = cluster_points(11 + salt + n, 6, -(-n // 6), 16)[0][:n]
        watch = []
        Y64, kl64, _ = fit(X, perplexity, n_iter, 0, np.float64, n_iter_early_exag=n_iter_early_exag, watch=watch)
        if min(watch) < 1e-6:
            return None, {"redraw": {"cpu_f32": FLOOR / 2, "bar": 0.0}}
        Y32, kl32, _ = fit(X, perplexity, n_iter, 0, np.float32, n_iter_early_exag=n_iter_early_exag)
        return (X, Y64.numpy(), float(kl64)), {"Y": measured_bar(Y32, Y64), "kl": measured_bar(kl32, kl64)}
    (X, Y64, kl64), bars = settled(build)
    return X, Y64, kl64, bars


def ten_iterations_case(n_iter_early_exag: int):
    """TSNE(n_iter=10) at N = 300, perplexity 10, random_state 0 -> (X, Y64, bars)"""
    X, Y64, _, bars = fit_case(300, 10.0, 10, n_iter_early_exag)
    return X, Y64, bars


STEP_ROWS = 64                  # manner_amd.hip.TSNE_STEP_ROWS: rows per workgroup of the step and KL kernels
ROW_EDGE_SIZES = (STEP_ROWS - 1, STEP_ROWS, STEP_ROWS + 1, 2 * STEP_ROWS + 1)


def purity(Y, labels) -> float:
    """the share of points whose nearest neighbour in the plane carries their own label"""
    D2 = sqdist(np.asarray(Y, np.float64))
    np.fill_diagonal(D2, np.inf)
    return float((labels[D2.argmin(1)] == labels).mean())


@functools.lru_cache(maxsize=None)
def end_to_end_case():
    """Six Gaussian clusters of 50 points in 16 dimensions (centres 6 randn, unit noise, default_rng(0)), perplexity 10: the float64
    restatement from eight initialisations (random_state 0 .. 7), all in one batch -> (X, labels, P, KLs [8], purities [8])"""
    X, labels = cluster_points(0, 6, 50, 16)
    Xn = normalise(X)
    idx, d2 = knn(Xn, 30)
    p, _ = affinities(d2, 10.0)
    P = torch.from_numpy(joint(idx, p))
    Y0 = torch.from_numpy(np.stack([1e-4 * np.random.RandomState(s).randn(len(X), 2) for s in range(8)]).astype(np.float32)).double()
    Y = iterate(P, Y0, 1000)
    kls = kl_divergence(P, Y).numpy()
    return X, labels, P, kls, np.array([purity(y, labels) for y in Y.numpy()])
