"""CAUMPLMModule.forward's candidate loop in train() — dropout on, gradients wanted — as ``manner_hip_caum_train_all_forward`` /
``_backward`` compute it: every column of the dense candidates in one call, column c under its own seed.  No GPU in this file:
tests/test_caum_train_all_host.py holds the restatements and their planted defects on the CPU, tests/test_gpu_caum_train_all.py
runs the kernels.

``caum_train_all`` is the reference: the loop over ``caum_ref.caum_user`` with the keep-masks (keep1, keep2, keep3) of each column,
dtype-generic (float64: the reference, float32 on the CPU: the yardstick of the MEASURED bar of tests/side_ops_ref.py).
``caum_train_all_wide`` is the same function in the form the kernels take — B C S rows in (b, c, s) order, (b, c) a pseudo-user of S
slots, attention along B per (column, slot, head) — and carries the planted defects of that layout.

``keep_rule`` restates the counter-based dropout generator of csrc/train_common.h in numpy: splitmix64 over (seed, site, index); an
element is kept when the top 32 bits are >= floor(p 2^32), p taken as the float32 the library receives.  ``column_keeps`` builds the
three masks of every column from it at the element indices of the per-column call:
  dropout1  b D + d            dropout2  (b S + s) D + d            dropout3  (b S + s)(F + U) + j.
The dropout cases search ``torch.manual_seed`` 1234 .. 1265 for the first seed whose masks leave every float32 CPU figure exactly
zero or at least 2^-25 (``side_ops_ref.QUARTER_ULP``; d_bc, zero in exact arithmetic, excepted) and raise if none does."""
from __future__ import annotations

import functools
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

import caum_all_ref as CA
import caum_ref as CR
from side_ops_ref import QUARTER_ULP, Case, randn

Tensor = torch.Tensor
SITE0 = 7                                                      # hip.CAUM_DROPOUT_SITE
Keeps = Sequence[Tuple[Tensor, Tensor, Tensor]]


# ------------------------------------------------------------------------------------------------ the keep rule
def drop_bits(seed: int, site: int, idx: np.ndarray) -> np.ndarray:
    """train_common.h drop_bits: the top 32 bits of splitmix64 over (seed, site, index)"""
    with np.errstate(over="ignore"):
        z = (np.uint64(seed & (2 ** 64 - 1)) ^ (np.uint64(site) * np.uint64(0xD6E8FEB86659FD93))) + (idx.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def threshold(p: float) -> int:
    """train_common.h make_drop: floor(p 2^32) of the float32 p, saturated"""
    t = float(np.float32(p)) * 4294967296.0
    return 0 if p <= 0 else 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def keep_rule(seed: int, site: int, p: float, idx: np.ndarray) -> np.ndarray:
    return drop_bits(seed, site, idx) >= np.uint32(threshold(p))


def numpy_mask(seed: int, site: int, p: float, n: int) -> Tensor:
    """the mask of the elements 0 .. n - 1 (what ``train.dropout_mask`` returns from the device)"""
    return torch.from_numpy(keep_rule(seed, site, p, np.arange(n, dtype=np.uint64)))


def column_keeps(seeds: Sequence[int], p: float, b: int, s: int, d: int, f: int, mask_fn: Callable = numpy_mask, *, same_seed: bool = False,
                 wide_dropout3: bool = False) -> List[Tuple[Tensor, Tensor, Tensor]]:
    """(keep1 [B, D], keep2 [B, S, D], keep3 [B, S, F + U]) of every column, U = D.  Planted defects: ``same_seed`` (every column draws
    with column 0's seed), ``wide_dropout3`` (dropout3 indexed by the wide row (b C + c) S + s where b S + s is meant)."""
    c_n, fu = len(seeds), f + d
    out = []
    for c, seed in enumerate(seeds):
        seed = seeds[0] if same_seed else seed
        k1 = mask_fn(seed, SITE0, p, b * d).reshape(b, d)
        k2 = mask_fn(seed, SITE0 + 1, p, b * s * d).reshape(b, s, d)
        if wide_dropout3:
            k3 = mask_fn(seed, SITE0 + 2, p, b * c_n * s * fu).reshape(b, c_n, s, fu)[:, c]
        else:
            k3 = mask_fn(seed, SITE0 + 2, p, b * s * fu).reshape(b, s, fu)
        out.append((k1, k2, k3))
    return out


# ------------------------------------------------------------------------------------------------ the loop (the reference)
def caum_train_all(hist: Tensor, cand: Tensor, heads: int, p: float = 0.0, keeps: Optional[Keeps] = None, **w: Tensor) -> Dict[str, Tensor]:
    """hist [B, S, D], cand [B, C, D], the 16 leaves of ``caum_ref.PARAMS`` -> scores [B, C]: one ``caum_ref.caum_user`` call per column
    on the cand[:, i, :] view with that column's masks"""
    rows = []
    for i in range(cand.shape[1]):
        k1, k2, k3 = keeps[i] if keeps is not None else (None, None, None)
        rows.append(CR.caum_user(hist, cand[:, i, :], heads=heads, p=p, keep1=k1, keep2=k2, keep3=k3, **w)["out"])
    return {"scores": torch.stack(rows, dim=1)}


# ------------------------------------------------------------------------------------------------ the wide form (what the kernels do)
def caum_train_all_wide(hist: Tensor, cand: Tensor, heads: int, p: float = 0.0, keeps: Optional[Keeps] = None, *, transposed_rows: bool = False,
                        wrap_over_columns: bool = False, d_hist_last_only: bool = False, d_hist_one_mask: bool = False,
                        **w: Tensor) -> Dict[str, Tensor]:
    """The same function on [B, C, S, *] rows.  Planted defects: ``transposed_rows`` (the pseudo-user term of the dense attention read
    at row c B + b of its flattened [B C] rows), ``wrap_over_columns`` (the circular window over the C S rows of a user where the S
    slots of a column are meant), ``d_hist_last_only`` (d hist from the last column alone), ``d_hist_one_mask`` (the columns'
    d hist summed first and masked once, by column 0's dropout2 mask)."""
    b, s, d = hist.shape
    c = cand.shape[1]
    f, u = w["w1"].shape[0], w["w2"].shape[0]
    dh = u // heads
    scale = 1.0 / (1.0 - p) if p > 0.0 else 1.0
    xw = hist[:, None].expand(b, c, s, d)
    if d_hist_last_only:
        xw = torch.cat([hist.detach()[:, None].expand(b, c - 1, s, d), hist[:, None]], dim=1)
    if keeps is None:
        cd, xd = cand, xw
    else:
        k1, k2 = (torch.stack([k[i] for k in keeps], dim=1).to(hist.dtype) for i in (0, 1))
        cd, xd = cand * k1 * scale, xw * k2 * scale
        if d_hist_one_mask:
            one = xw * k2[:, :1] * scale
            xd = one + (xd - one).detach()
    if wrap_over_columns:
        flat = xd.reshape(b, c * s, d)
        left, right = torch.roll(flat, 1, dims=1).reshape(b, c, s, d), torch.roll(flat, -1, dims=1).reshape(b, c, s, d)
    else:
        left, right = torch.roll(xd, 1, dims=2), torch.roll(xd, -1, dims=2)
    w1 = w["w1"]
    cnn = left @ w1[:, :d].T + xd @ w1[:, d:2 * d].T + right @ w1[:, 2 * d:3 * d].T + (cd @ w1[:, 3 * d:].T)[:, :, None, :] + w["b1"]
    h2 = (cd @ w["w2"][:, :d].T)[:, :, None, :] + xd @ w["w2"][:, d:].T + w["b2"]
    qkv = h2 @ w["in_w"].T + w["in_b"]

    def split_heads(t):                                                                  # [B, C, S, U] -> [C, S, heads, B, dh]
        return t.reshape(b, c, s, heads, dh).permute(1, 2, 3, 0, 4)

    q, k, v = (split_heads(t) for t in qkv.split(u, dim=-1))
    att = torch.softmax((q * float(dh) ** -0.5) @ k.transpose(-1, -2), dim=-1) @ v
    self_att = att.permute(3, 0, 1, 2, 4).reshape(b, c, s, u) @ w["out_w"].T + w["out_b"]
    cat = torch.cat([cnn, self_att], dim=-1)
    if keeps is not None:
        cat = cat * torch.stack([k[2] for k in keeps], dim=1).to(cat.dtype) * scale
    allv = cat @ w["w3"].T + w["b3"]
    ct = cd @ w["wa"][:, u:].T + w["ba"]
    if transposed_rows:
        ct = ct.reshape(b * c, -1).reshape(c, b, -1).transpose(0, 1)
    t2 = torch.tanh(torch.tanh(allv @ w["wa"][:, :u].T + ct[:, :, None, :]) @ w["wb"].T + w["bb"])
    score = (t2 @ w["wc"].T).squeeze(-1) + w["bc"]
    user = (torch.softmax(score, dim=-1)[..., None] * allv).sum(dim=2)
    return {"scores": (cd * user).sum(dim=-1)}


# ------------------------------------------------------------------------------------------------ shapes and cases
GW = CA.GOLDEN_WIDTHS
MODULE_SHAPE = (3, 7, 20, 24, 12, 8, 4, 5)
ODD_SHAPE = (9, 5, 50, 12, 10, 6, 2, 4)
SHIPPED_SHAPE = (8, 50, 400, 400, 400, 256, 16, 3)
#: (B, S, D = U, F, H1, H2, heads, C) with dropout: 105 rows on the small tiles; odd widths at head dim 25; 1200 rows at the shipped
#: widths (the 128-row tile of the linear, the large tile of the weight gradient); S = 1 and 2 (the window folds onto itself); B = 1;
#: C = 1; B = 65 and 257: past one workgroup's pairs and past the 256-row block of the attention
DROPOUT_SHAPES = (MODULE_SHAPE, ODD_SHAPE, SHIPPED_SHAPE, (3, 1) + GW + (5,), (3, 2) + GW + (5,), (1, 7) + GW + (5,), (3, 7) + GW + (1,),
                  (65, 3, 10, 6, 6, 4, 2, 2), (257, 3, 10, 6, 6, 4, 2, 2))
#: without dropout only: width 1024 (the widest K and O, partial last tiles) and S at its bound
PLAIN_ONLY_SHAPES = ((2, 3, 1024, 260, 1024, 260, 16, 2), (2, 256, 8, 8, 8, 8, 2, 2))
#: the shapes the planted defects are shown at
DEFECT_SHAPES = (MODULE_SHAPE, ODD_SHAPE)
P = 0.2


def draw_seeds(manual: int, c: int) -> List[int]:
    """the draws of the candidate loop under ``torch.manual_seed(manual)``: one per column, in column order"""
    torch.manual_seed(manual)
    return [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(c)]


def is_settled(case: Case) -> bool:
    return all(v["cpu_f32"] == 0 or v["cpu_f32"] >= QUARTER_ULP for k, v in case.bars().items() if k != "d_bc")


def settle(build: Callable[[int], Case]) -> Case:
    """build(trial) at the first of 32 trials that settles (trial t of a dropout case is torch.manual_seed(1234 + t))"""
    for trial in range(32):
        case = build(trial)
        if is_settled(case):
            return case
    raise AssertionError("no seed in 32 settles the case")


@functools.lru_cache(maxsize=None)
def train_case(shape: tuple, p: float, mask_fn: Callable = numpy_mask) -> Case:
    """``caum_all_ref.all_case``'s leaves (one zero history slot, one zero candidate row where B > 1), an upstream randn [B, C]; with
    p > 0 the masks of the first settling torch.manual_seed in 1234 .. 1265.  The case carries ``manual`` (that seed, None at p = 0),
    ``seeds`` and ``p``."""
    b, s, d, f, _, _, heads, c = shape
    base = CA.all_case(*shape)

    def build(trial):
        consts = {"heads": heads}
        manual, seeds = None, None
        if p > 0:
            manual = 1234 + trial
            seeds = draw_seeds(manual, c)
            consts.update(p=p, keeps=column_keeps(seeds, p, b, s, d, f, mask_fn))
        case = Case(f"{base}-train-p{p}", caum_train_all, base.leaves, consts, {"scores": randn(3500 + c + (0 if p > 0 else trial), b, c)})
        case.manual, case.seeds, case.p = manual, seeds, p
        return case
    return settle(build)


# ------------------------------------------------------------------------------------------------ the weight-gradient kernel alone
#: (R, K, O): the smallest; partial tiles on all three axes of the small tile; several row groups with a ragged last one; the shipped
#: linear1 on the large tile; the O = 1 product of dense_att.linear3
WGRAD_SHAPES = ((1, 4, 1), (33, 70, 33), (1100, 130, 70), (2100, 1600, 400), (105, 8, 1))


def wgrad_inputs(r: int, k: int, o: int):
    return randn(3600 + r + k, r, o), randn(3601 + r + o, r, k)
