"""Float64 restatements of the f32 side operators (training scorer and loss, nn.Linear, AdditiveAttention, axis-0 multi-head
attention, nn.Embedding), the shapes at which their kernels take every loop a second time, and the two bars they are held to.
No GPU in this file: tests/test_side_ops_host.py checks the restatements and the bars on the CPU, tests/test_gpu_side_ops.py
runs the kernels against them.

Every operator is written from its definition in plain torch, dtype-generic: evaluated in float64 it is the reference, evaluated
in float32 on the CPU it is the yardstick of the MEASURED bar.  Gradients come from torch autograd.

DERIVED bar (pure sums of products: linear forward / dx / dW / db, late-fusion user / scores / d cand / d hist, DotProduct and
its gradients, the embedding's table gradient): componentwise |got - ref64| <= (n + 4) * 2^-24 * sum |a_i * b_i|, n the
reduction length, the absolute-value sum evaluated in float64 from the same inputs (the ``*_terms`` functions with
``absolute=True``).  That is the textbook bound n * u * sum|a b| of a length-n f32 dot product in any summation order (u = 2^-24;
an fma chain rounds less often), with four more roundings allowed for what surrounds the sum: the bias add, the 1 / h of a mean
(rounded itself, then multiplied), a factor that is itself a rounded sum.  Where a factor is a rounded sum, n counts both sums
(scores: D + h, because user carries (h + 1) u already).  No floor, no excluded entries.

MEASURED bar (exp / tanh / log / softmax inside): the same restatement in float32 on the CPU, its error against float64 relative
to the tensor's largest entry, times 8 (the kernel's other summation order and the device's expf / tanhf, a few ulp from libm).
A float32 result sits up to half an ulp of itself from float64 — 2^-25 to 2^-24 of its value — whatever computed it.  A CPU
figure below 2^-25 is therefore the luck of that one rounding (typical of a scalar loss), not a measure of float32 arithmetic, and
8 x it is a bar that no float32 result is sure to meet.  Such inputs are too weak to judge a kernel by: every measured case draws
its inputs with the first salt (``settled``) at which each float32 CPU figure is exactly zero or at least 2^-25 — a condition on
the reference side alone, asserted by the host tests.
"""
from __future__ import annotations

import functools
from typing import Callable, Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

import manner_oracle as O

Tensor = torch.Tensor
U32 = 2.0 ** -24
MEASURED_FACTOR = 8.0


def randn(seed: int, *shape: int, scale: float = 1.0) -> Tensor:
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


# ------------------------------------------------------------------------------------------------ evaluation and bars
def evaluate(fn: Callable[..., Dict[str, Tensor]], leaves: Dict[str, Tensor], consts: dict, upstream: Optional[Dict[str, Tensor]],
             dtype: torch.dtype, device: str = "cpu") -> Dict[str, Tensor]:
    """fn(**leaves, **consts) -> {name: tensor} with the float leaves in ``dtype`` on ``device``; with ``upstream`` = {output name:
    d L / d output}, also {"d_<leaf>": gradient}.  Everything comes back on the CPU."""
    lv = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(upstream is not None) for k, v in leaves.items()}
    cs = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in consts.items()}
    outs = fn(**lv, **cs)
    res = {k: v.detach().cpu() for k, v in outs.items()}
    if upstream is not None:
        total = None
        for k, g in upstream.items():
            t = (outs[k] * g.to(device=device, dtype=dtype)).sum()
            total = t if total is None else total + t
        total.backward()
        for k, v in lv.items():
            res["d_" + k] = (v.grad if v.grad is not None else torch.zeros_like(v)).detach().cpu()
    return res


def rel_to_max(got: Tensor, ref64: Tensor) -> float:
    """max |got - ref| over the tensor's largest |ref| entry (an all-zero reference leaves the absolute error)."""
    ref64 = ref64.double()
    err = float((got.double() - ref64).abs().max()) if ref64.numel() else 0.0
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    return err / scale if scale > 0 else err


def measured_bars(ref64: Dict[str, Tensor], ref32: Dict[str, Tensor]) -> Dict[str, Dict[str, float]]:
    """{name: {"cpu_f32": error of the float32 CPU evaluation, "bar": 8 x that}}."""
    return {k: {"cpu_f32": rel_to_max(ref32[k], ref64[k]), "bar": MEASURED_FACTOR * rel_to_max(ref32[k], ref64[k])} for k in ref64}


def derived_ratio(got, ref64, abs64, n) -> float:
    """max over the entries of |got - ref64| / ((n + 4) 2^-24 sum|a b|); an entry whose absolute-value sum is zero is exactly zero
    in the reference and must be exactly zero in ``got`` (ratio inf otherwise)."""
    got, ref64, abs64 = (np.asarray(a, np.float64) for a in (got, ref64, abs64))
    bound = (np.asarray(n, np.float64) + 4.0) * U32 * abs64
    err = np.abs(got - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


QUARTER_ULP = 2.0 ** -25


def settled(build: Callable[[int], "Case"]) -> "Case":
    """build(salt) at the first salt whose float32 CPU figures are all exactly zero or at least 2^-25 (module docstring)"""
    for salt in range(32):
        case = build(salt * 100003)
        if all(v["cpu_f32"] == 0 or v["cpu_f32"] >= QUARTER_ULP for v in case.bars().values()):
            return case
    raise AssertionError("no salt in 32 settles the case")


class Case:
    """One operator at one shape: ``fn`` (the restatement), its float ``leaves``, ``consts``, the ``upstream`` gradients, and for
    the derived bar ``terms(absolute) -> {name: (values, n)}``."""

    def __init__(self, name, fn, leaves, consts, upstream, terms=None):
        self.name, self.fn, self.leaves, self.consts, self.upstream, self.terms = name, fn, leaves, consts, upstream, terms
        self._ref = {}

    def ref(self, dtype=torch.float64) -> Dict[str, Tensor]:
        if dtype not in self._ref:                              # computed once, shared by every test that needs it, never modified
            self._ref[dtype] = evaluate(self.fn, self.leaves, self.consts, self.upstream, dtype)
        return self._ref[dtype]

    def bars(self):
        return measured_bars(self.ref(torch.float64), self.ref(torch.float32))

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------ scorer
def late_fusion(hist: Tensor, cand: Tensor, hist_off: Tensor, cand_off: Tensor) -> Dict[str, Tensor]:
    """CRModule.forward with late fusion on ragged rows: user_i = mean of the history rows of impression i, s_j = <user_i, cand_j>."""
    ho, co = hist_off.tolist(), cand_off.tolist()
    users = [hist[ho[i]:ho[i + 1]].sum(0) / (ho[i + 1] - ho[i]) for i in range(len(ho) - 1)]
    scores = [cand[co[i]:co[i + 1]] @ users[i] for i in range(len(co) - 1)]
    return {"user": torch.stack(users), "scores": torch.cat(scores)}


def late_fusion_terms(hist, cand, hist_off, cand_off, g, absolute=False, dtype=np.float64):
    """{name: (value, n)} of the scorer and its gradients for d L / d scores = g, as plain sums of products; ``absolute``: every
    factor replaced by its absolute value (the sum |a b| of the derived bar)."""
    f = np.abs if absolute else (lambda a: a)
    hist, cand, g = (f(np.asarray(a, dtype)) for a in (hist, cand, g))
    d = hist.shape[1]
    user, scores, dhist, dcand = [], [], [], []
    n_user, n_scores, n_dhist, n_dcand = [], [], [], []
    for i in range(len(hist_off) - 1):
        h0, h1, c0, c1 = hist_off[i], hist_off[i + 1], cand_off[i], cand_off[i + 1]
        h, c = h1 - h0, c1 - c0
        u = hist[h0:h1].sum(0, dtype=dtype) / dtype(h)
        user.append(u)
        scores.append(cand[c0:c1] @ u)
        dcand.append(g[c0:c1, None] * u[None, :])
        dhist.append(np.tile((g[c0:c1] @ cand[c0:c1]) / dtype(h), (h, 1)))
        n_user.append(np.full(d, h))
        n_scores.append(np.full(c, d + h))                      # a D-term dot product whose one factor carries (h + 1) u
        n_dcand.append(np.full((c, d), h + 1))                  # one product with the rounded mean
        n_dhist.append(np.full((h, d), c + 1))                  # C-term sum, then the 1 / h
    return {"user": (np.stack(user), np.stack(n_user)), "scores": (np.concatenate(scores), np.concatenate(n_scores)),
            "d_cand": (np.concatenate(dcand), np.concatenate(n_dcand)), "d_hist": (np.concatenate(dhist), np.concatenate(n_dhist))}


SCORER_D = (4, 64, 256, 260, 768, 1024)
SCORER_HIST = (1, 2, 50, 1, 2, 50)
SCORER_CAND = (1, 3, 4, 5, 9, 130)


@functools.lru_cache(maxsize=None)
def scorer_case(d: int) -> Case:
    hoff = np.concatenate([[0], np.cumsum(SCORER_HIST)]).astype(np.int64)
    coff = np.concatenate([[0], np.cumsum(SCORER_CAND)]).astype(np.int64)
    hist, cand, g = randn(100 + d, int(hoff[-1]), d), randn(200 + d, int(coff[-1]), d), randn(300 + d, int(coff[-1]))
    terms = functools.partial(late_fusion_terms, hist.numpy(), cand.numpy(), hoff.tolist(), coff.tolist(), g.numpy())
    return Case(f"scorer-D{d}", late_fusion, {"hist": hist, "cand": cand},
                {"hist_off": torch.from_numpy(hoff), "cand_off": torch.from_numpy(coff)}, {"scores": g}, terms)


def dot_product(user: Tensor, cand: Tensor, permuted: bool) -> Dict[str, Tensor]:
    """DotProduct: bmm(user [B, 1, D], cand [B, D, C]); ``permuted``: ``cand`` arrives as rows [B, C, D] and is viewed as [B, D, C]."""
    return {"out": torch.bmm(user, cand.permute(0, 2, 1) if permuted else cand).squeeze(1)}


def dot_terms(user, cand, permuted, g, absolute=False, dtype=np.float64):
    f = np.abs if absolute else (lambda a: a)
    user, cand, g = (f(np.asarray(a, dtype)) for a in (user, cand, g))
    bdc = np.transpose(cand, (0, 2, 1)) if permuted else cand            # [B, D, C]
    b, d, c = bdc.shape
    dc = user[:, 0, :, None] * g[:, None, :]                             # [B, D, C]
    return {"out": (np.einsum("bd,bdc->bc", user[:, 0], bdc), np.full((b, c), d)),
            "d_user": (np.einsum("bc,bdc->bd", g, bdc)[:, None, :], np.full((b, 1, d), c)),
            "d_cand": (np.transpose(dc, (0, 2, 1)) if permuted else dc, 1)}


DOT_D, DOT_C, DOT_B = (96, 260, 768), (1, 5, 300), 5


@functools.lru_cache(maxsize=None)
def dot_case(d: int, c: int, permuted: bool) -> Case:
    user, g = randn(400 + d + c, DOT_B, 1, d), randn(500 + d + c, DOT_B, c)
    cand = randn(600 + d + c, DOT_B, c, d) if permuted else randn(600 + d + c, DOT_B, d, c)
    terms = functools.partial(dot_terms, user.numpy(), cand.numpy(), permuted, g.numpy())
    return Case(f"dot-D{d}-C{c}-{'rows' if permuted else 'contiguous'}", dot_product, {"user": user, "cand": cand},
                {"permuted": permuted}, {"out": g}, terms)


# ------------------------------------------------------------------------------------------------ model_step loss
def model_step_loss(scores: Tensor, labels: Tensor, cand_off: Tensor, supcon: bool, temperature: float, c_max: Optional[int] = None,
                    softmax_limit: Optional[int] = None, reduce_limit: Optional[int] = None) -> Dict[str, Tensor]:
    """The loss of CRModule.model_step on ragged scores.
    SupCon on the scores: l_i = -(1 / n_pos) sum_{j positive} (v_j - log sum_{k real} exp v_k), v = s / T; the batch value is the
    mean over the impressions with l_i > 0 (the non-zero mean reducer), 0 if there is none.
    Cross-entropy with probability targets over the dense row, zero-padded to ``c_max`` columns (the padding is in the softmax);
    the batch value is the mean over the batch.
    ``softmax_limit`` / ``reduce_limit`` plant a defect (columns >= the limit left out of the log-sum-exp, impressions >= the limit
    left out of the reducer): tests/test_side_ops_host.py shows that the bars see them."""
    off = cand_off.tolist()
    b = len(off) - 1
    sizes = torch.tensor([off[i + 1] - off[i] for i in range(b)])
    seg = torch.repeat_interleave(torch.arange(b), sizes)
    pos = torch.arange(off[-1]) - torch.tensor(off[:-1])[seg]
    width = int(sizes.max()) if supcon else int(c_max)
    seg, pos = seg.to(scores.device), pos.to(scores.device)
    dense = scores.new_zeros((b, width)).index_put((seg, pos), scores)
    y = scores.new_zeros((b, width)).index_put((seg, pos), labels.to(scores.dtype))
    valid = torch.zeros((b, width), dtype=torch.bool, device=scores.device).index_put((seg, pos), torch.ones_like(seg, dtype=torch.bool))
    cols = torch.arange(width, device=scores.device)[None, :] < (width if softmax_limit is None else softmax_limit)
    ninf = float("-inf")
    if supcon:
        v = dense / temperature
        v = v - v.masked_fill(~valid, ninf).max(dim=1, keepdim=True)[0].detach()
        lse = torch.logsumexp(v.masked_fill(~(valid & cols), ninf), dim=1, keepdim=True)
        posm = ((y > 0.5) & valid).to(scores.dtype)
        per = -((posm * (v - lse)).sum(1) / (posm.sum(1) + torch.finfo(scores.dtype).tiny))
        live = per > 0
        if reduce_limit is not None:
            live = live & (torch.arange(b, device=scores.device) < reduce_limit)
        loss = per[live].mean() if bool(live.any()) else per.sum() * 0
    else:
        lse = torch.logsumexp(dense.masked_fill(~cols, ninf), dim=1, keepdim=True)
        per = -(y * (dense - lse)).sum(1)
        loss = per.mean() if reduce_limit is None else per[:reduce_limit].mean()
    return {"loss": loss, "per": per}


LOSS_B = (1, 4, 5, 257, 513)
LOSS_COUNTS = (65, 130, 63, 2, 64, 1)          # cycled over the impressions: index 256 has 64 candidates, index 512 has 63
LOSS_TEMPERATURE, LOSS_C_MAX = 0.36, 137


def loss_inputs(b: int, salt: int = 0):
    rng = np.random.default_rng(700 + b + salt)
    counts = np.array([LOSS_COUNTS[i % len(LOSS_COUNTS)] for i in range(b)])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    scores = (rng.standard_normal(off[-1]) * 0.5).astype(np.float32)
    labels = np.zeros(off[-1], np.float32)
    for i in range(b):
        row = labels[off[i]:off[i + 1]]
        if i % 8 == 2:
            row[:] = 1.0                                         # no negative
        elif i % 8 == 3:
            continue                                             # no positive
        else:
            row[rng.integers(0, counts[i])] = 1.0                # a row of one candidate: that one, no negative, loss exactly 0
            if counts[i] >= 3 and i % 3 == 0:
                row[(int(np.argmax(row)) + 1 + rng.integers(0, counts[i] - 2)) % counts[i]] = 1.0
    return torch.from_numpy(scores), torch.from_numpy(labels), torch.from_numpy(off)


@functools.lru_cache(maxsize=None)
def loss_case(b: int, supcon: bool) -> Case:
    return settled(lambda salt: _loss_case(b, supcon, salt))


def _loss_case(b, supcon, salt):
    scores, labels, off = loss_inputs(b, salt)
    return Case(f"loss-{'supcon' if supcon else 'ce'}-B{b}", model_step_loss, {"scores": scores},
                {"labels": labels, "cand_off": off, "supcon": supcon, "temperature": LOSS_TEMPERATURE if supcon else 1.0, "c_max": LOSS_C_MAX},
                {"loss": torch.tensor(0.75)})


def supcon_embeddings(emb: Tensor, labels: Tensor, temperature: float) -> Dict[str, Tensor]:
    """SupCon on embeddings with the un-normalised dot-product similarity: m = E E^T / T; positives of anchor i = the other rows
    of its label, negatives = the rows of other labels; l_i = -(1 / n_pos) sum_pos (m_ij - log sum_{k != i} exp m_ik); the batch
    value is the mean over the anchors with l_i > 0, and 0 when the batch has no positive pair or no negative pair.
    (The oracle's function builds its masks in float32 whatever the input: in float64 its `n_pos + tiny` is 0 for a class of one.)"""
    n = emb.shape[0]
    same = labels[:, None] == labels[None, :]
    eye = torch.eye(n, dtype=torch.bool, device=emb.device)
    pos = (same & ~eye).to(emb.dtype)
    if not (bool(pos.any()) and bool((~same).any())):
        return {"loss": emb.sum() * 0, "per": emb.new_zeros(n)}
    m = (emb @ emb.T) / temperature
    m = m - m.max(dim=1, keepdim=True)[0].detach()
    lse = torch.logsumexp(m.masked_fill(eye, float("-inf")), dim=1, keepdim=True)
    per = -((pos * (m - lse)).sum(1) / (pos.sum(1) + torch.finfo(emb.dtype).tiny))
    live = per > 0
    return {"loss": per[live].mean() if bool(live.any()) else per.sum() * 0, "per": per}


SUPCON_N, SUPCON_D, SUPCON_LABELS, SUPCON_TEMPERATURE = (2, 63, 65, 130), (64, 260, 768), ("class_of_one", "one_class", "distinct"), 0.5


def supcon_labels(n: int, kind: str) -> Tensor:
    if kind == "one_class":
        return torch.full((n,), 4, dtype=torch.int64)
    if kind == "distinct":
        return torch.arange(n, dtype=torch.int64)
    lab = torch.arange(n, dtype=torch.int64) % 3
    lab[-1] = 99                                                 # a class of one: an anchor without a positive
    return lab


@functools.lru_cache(maxsize=None)
def supcon_case(n: int, d: int, kind: str) -> Case:
    return settled(lambda salt: _supcon_case(n, d, kind, salt))


def _supcon_case(n, d, kind, salt):
    emb = randn(800 + n + d + salt, n, d, scale=d ** -0.25)             # |E_i|^2 / T ~ 2 sqrt(D), E_i . E_j / T ~ N(0, 4): the diagonal dominates
    return Case(f"supcon-N{n}-D{d}-{kind}", supcon_embeddings, {"emb": emb}, {"labels": supcon_labels(n, kind), "temperature": SUPCON_TEMPERATURE},
                {"loss": torch.tensor(0.75)})


# ------------------------------------------------------------------------------------------------ nn.Linear
def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Dict[str, Tensor]:
    y = x @ weight.T
    return {"y": y if bias is None else y + bias}


def linear_terms(x, weight, bias, dy, absolute=False, dtype=np.float64):
    f = np.abs if absolute else (lambda a: a)
    x, weight, dy = (f(np.asarray(a, dtype)) for a in (x, weight, dy))
    r, k = x.shape
    o = weight.shape[0]
    out = {"y": (x @ weight.T, k), "d_x": (dy @ weight, o), "d_weight": (dy.T @ x, r)}
    if bias is not None:
        out["y"] = (out["y"][0] + f(np.asarray(bias, dtype)), k + 1)
        out["d_bias"] = (dy.sum(0, dtype=dtype), r)
    return out


# (9, 300, 1030): the data gradient's second tile of 256 input features (44 of them) and its second pass of 1024 staged output features
# (6 of them) in one launch, with a second row tile of one row
LINEAR_SHAPES = ((1, 4, 1), (9, 8, 2049), (9, 8, 4100), (17, 257, 300), (8, 512, 5), (7, 2049, 3), (9, 4096, 5), (65, 8, 70), (9, 300, 1030))


@functools.lru_cache(maxsize=None)
def linear_case(r: int, k: int, o: int, with_bias: bool) -> Case:
    s = 900 + r + k + o
    x, w, dy = randn(s, r, k), randn(s + 1, o, k), randn(s + 2, r, o)
    leaves = {"x": x, "weight": w}
    if with_bias:
        leaves["bias"] = randn(s + 3, o)
    terms = functools.partial(linear_terms, x.numpy(), w.numpy(), leaves["bias"].numpy() if with_bias else None, dy.numpy())
    return Case(f"linear-R{r}-K{k}-O{o}-{'bias' if with_bias else 'nobias'}", linear, leaves, {}, {"y": dy}, terms)


# ------------------------------------------------------------------------------------------------ AdditiveAttention
def additive_pool(x: Tensor, lin_w: Tensor, lin_b: Tensor, query: Tensor) -> Dict[str, Tensor]:
    return {"out": O.additive_attention(x, lin_w, lin_b, query)}       # dtype-preserving: softmax_s(tanh(x W^T + b) . q) weighted sum


POOL_SHAPES = ((3, 1, 64, 16), (2, 257, 100, 200), (2, 1024, 64, 16))


@functools.lru_cache(maxsize=None)
def pool_case(b: int, s: int, d: int, q: int) -> Case:
    return settled(lambda salt: _pool_case(b, s, d, q, salt))


def _pool_case(b, s, d, q, salt):
    sd = 1000 + s + d + salt
    leaves = {"x": randn(sd, b, s, d), "lin_w": randn(sd + 1, q, d, scale=d ** -0.5), "lin_b": randn(sd + 2, q, scale=0.1),
              "query": randn(sd + 3, q, scale=2.0 * q ** -0.5)}
    return Case(f"pool-B{b}-S{s}-D{d}-Q{q}", additive_pool, leaves, {}, {"out": randn(sd + 4, b, d)})


# ------------------------------------------------------------------------------------------------ axis-0 attention
def mha_axis0(x: Tensor, in_w: Tensor, in_b: Tensor, out_w: Tensor, out_b: Tensor, heads: int, key_limit: Optional[int] = None,
              scale_dh: Optional[int] = None) -> Dict[str, Tensor]:
    """nn.MultiheadAttention(E, heads, batch_first=False) on x [L0, B1, E] without masks: in-projection, per (b1, head) softmax
    attention ALONG AXIS 0 with the queries scaled by dh^-1/2, out-projection.
    ``key_limit`` (keys >= the limit dropped) and ``scale_dh`` (the scale of another head dim) plant defects for the host tests."""
    l0, b1, e = x.shape
    dh = e // heads
    q, k, v = (x @ in_w.T + in_b).split(e, dim=-1)

    def split_heads(t):                                       # [L0, B1, E] -> [B1 * heads, L0, dh]
        return t.reshape(l0, b1 * heads, dh).transpose(0, 1)

    q, k, v = split_heads(q) * float(scale_dh or dh) ** -0.5, split_heads(k), split_heads(v)
    if key_limit is not None:
        k, v = k[:, :key_limit], v[:, :key_limit]
    att = torch.softmax(q @ k.transpose(1, 2), dim=-1)
    o = (att @ v).transpose(0, 1).reshape(l0, b1, e)
    return {"out": o @ out_w.T + out_b}


AXIS0_DH = (4, 8, 10, 16, 32, 48, 64)
AXIS0_L0 = (1, 33, 65, 129, 257, 300)
AXIS0_KEY_TILE_TRAIN = {4: 256, 8: 256, 10: 256, 16: 128, 32: 64, 48: 32, 64: 32}        # axis0.hip, training column
AXIS0_KEY_TILE_ENTITY = {4: 256, 8: 256, 10: 256, 16: 256, 32: 64, 48: 64, 64: 64}       # axis0.hip, inference column
AXIS0_GEMM_ROUTE = ((12, 3), (129, 3))            # E = 128: L0 * B1 = 36 and 387 rows, below and above one 128-row panel


@functools.lru_cache(maxsize=None)
def axis0_case(l0: int, b1: int, e: int, heads: int) -> Case:
    return settled(lambda salt: _axis0_case(l0, b1, e, heads, salt))


def _axis0_case(l0, b1, e, heads, salt):
    s = 1100 + 7 * l0 + e + salt
    leaves = {"x": randn(s, l0, b1, e), "in_w": randn(s + 1, 3 * e, e, scale=e ** -0.5), "in_b": randn(s + 2, 3 * e, scale=0.1),
              "out_w": randn(s + 3, e, e, scale=e ** -0.5), "out_b": randn(s + 4, e, scale=0.1)}
    return Case(f"axis0-L{l0}-B{b1}-E{e}-h{heads}", mha_axis0, leaves, {"heads": heads}, {"out": randn(s + 5, l0, b1, e)})


ENTITY_N, ENTITY_SLOTS, ENTITY_DIMS, ENTITY_Q, ENTITY_ROWS = (1, 65, 257), 3, ((16, 2), (100, 10)), 20, 50
ENTITY_KEYS = ("pretrained_embedding.weight", "multihead_attention.in_proj_weight", "multihead_attention.in_proj_bias",
               "multihead_attention.out_proj.weight", "multihead_attention.out_proj.bias", "additive_attention.linear.weight",
               "additive_attention.linear.bias", "additive_attention.query")


def entity_encode(ids: Tensor, heads: int, **w: Tensor) -> Dict[str, Tensor]:
    return {"out": O.entity_encoder(ids, {k.replace("__", "."): v for k, v in w.items()}, heads)}      # dtype-preserving


@functools.lru_cache(maxsize=None)
def entity_case(n: int, d: int, heads: int) -> Case:
    return settled(lambda salt: _entity_case(n, d, heads, salt))


def _entity_case(n, d, heads, salt):
    s = 1200 + n + d + salt
    q = ENTITY_Q
    shapes = ((ENTITY_ROWS, d), (3 * d, d), (3 * d,), (d, d), (d,), (q, d), (q,), (q,))
    scales = (1.0, d ** -0.5, 0.1, d ** -0.5, 0.1, d ** -0.5, 0.1, 2.0 * q ** -0.5)
    leaves = {k.replace(".", "__"): randn(s + i, *shp, scale=sc) for i, (k, shp, sc) in enumerate(zip(ENTITY_KEYS, shapes, scales))}
    ids = torch.from_numpy(np.random.default_rng(s + 20).integers(0, ENTITY_ROWS, (n, ENTITY_SLOTS)))
    return Case(f"entity-N{n}-D{d}-h{heads}", entity_encode, leaves, {"ids": ids, "heads": heads}, None)


# ------------------------------------------------------------------------------------------------ nn.Embedding
def embedding(table: Tensor, ids: Tensor, padding_idx: Optional[int]) -> Dict[str, Tensor]:
    return {"out": F.embedding(ids, table, padding_idx=padding_idx)}


def embedding_terms(ids, padding_idx, n_rows, g, absolute=False, dtype=np.float64):
    """d table[r] = sum of the upstream rows whose id is r (none for r = padding_idx): a sum of products with 1."""
    f = np.abs if absolute else (lambda a: a)
    g = f(np.asarray(g, dtype)).reshape(-1, g.shape[-1])
    dt, cnt = np.zeros((n_rows, g.shape[1]), dtype), np.zeros(n_rows, np.int64)
    for r, i in enumerate(np.asarray(ids).reshape(-1)):
        if padding_idx is None or i != padding_idx:
            dt[i] += g[r]
            cnt[i] += 1
    return {"d_table": (dt, np.broadcast_to(cnt[:, None], dt.shape))}


EMBEDDING_D, EMBEDDING_ROWS = (100, 260, 768), 11


@functools.lru_cache(maxsize=None)
def embedding_case(d: int, padding_idx: Optional[int]) -> Case:
    s = 1300 + d
    ids = torch.from_numpy(np.random.default_rng(s).integers(0, EMBEDDING_ROWS, (6, 5)))      # 30 draws of 11 rows: ids repeat
    ids[0, :3] = 0                                                                              # row 0 (the padding row) three times
    g = randn(s + 1, 6, 5, d)
    terms = functools.partial(embedding_terms, ids.numpy(), padding_idx, EMBEDDING_ROWS, g.numpy())
    return Case(f"embedding-D{d}-pad{padding_idx}", embedding, {"table": randn(s + 2, EMBEDDING_ROWS, d)},
                {"ids": ids, "padding_idx": padding_idx}, {"out": g}, terms)


DROPOUT_N, DROPOUT_P = 8192 * 256 + 1000, 0.2


def all_measured_cases():
    cases = [loss_case(b, sc) for b in LOSS_B for sc in (True, False)]
    cases += [supcon_case(n, d, k) for n in SUPCON_N for d in SUPCON_D for k in SUPCON_LABELS]
    cases += [pool_case(*s) for s in POOL_SHAPES]
    cases += [axis0_case(l0, 3, 2 * dh, 2) for dh in AXIS0_DH for l0 in AXIS0_L0]
    cases += [axis0_case(l0, b1, 128, 2) for l0, b1 in AXIS0_GEMM_ROUTE]
    cases += [entity_case(n, d, h) for n in ENTITY_N for d, h in ENTITY_DIMS]
    return cases


def all_derived_cases():
    cases = [scorer_case(d) for d in SCORER_D]
    cases += [dot_case(d, c, p) for d in DOT_D for c in DOT_C for p in (False, True)]
    cases += [linear_case(r, k, o, wb) for r, k, o in LINEAR_SHAPES for wb in (True, False)]
    cases += [embedding_case(d, p) for d in EMBEDDING_D for p in (0, None)]
    return cases
