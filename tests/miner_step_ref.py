"""Float64 restatements of MINERModule's own lines (reference manner/models/baselines/miner_module.py:153-242) — the category bias, the
max / mean aggregation over the context codes, the disagreement loss, and forward + model_step's loss over them — written from the
reference's lines in plain torch, dtype-generic, with autograd for the gradients; the cases the kernels of csrc/miner.hip are run at and
the planted defects that show the bars see every quirk.  No GPU in this file: tests/test_miner_step_host.py checks the restatements on
the CPU, tests/test_gpu_miner_step.py runs the kernels against them.

torchmetrics is not installed where these tests run, so the two lines of its ``pairwise_cosine_similarity`` that the bias goes through
are restated here (``torchmetrics_cosine``): ``x / torch.norm(x, p=2, dim=1)`` for both operands — no epsilon — then ``x @ y.T``.  The
bias restatement is the naive one of the reference: the whole [N_hist, T] matrix, to dense, the user's own columns zeroed, the mean over
all T columns.

Bars: those of tests/side_ops_ref.py, used as they are.  DERIVED for the bias (n = 2 Dc + T: two norms and the T-term sum around a
Dc-term dot product; the absolute-value sum runs over the non-own columns only) and for the code scores (n = D for 'max', D + K for
'mean', gradients likewise); MEASURED for the disagreement loss and the step."""
from __future__ import annotations

import functools
from typing import Dict, Optional, Sequence

import numpy as np
import torch

import miner_ref as M
from caum_train_all_ref import keep_rule
from side_ops_ref import QUARTER_ULP, Case, measured_bars, randn, settled

Tensor = torch.Tensor
SITE_HIST, SITE_CAND = 12, 13                                  # hip.MINER_DROPOUT_SITE, + 1


def offsets(counts: Sequence[int]) -> Tensor:
    return torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))


def to_dense(rows: Tensor, off: Tensor, width: int) -> Tensor:
    """``to_dense_batch``: ragged rows [N, *] -> [B, width, *], padded slots 0"""
    o = off.tolist()
    out = rows.new_zeros((len(o) - 1, width) + tuple(rows.shape[1:]))
    for b in range(len(o) - 1):
        out[b, :o[b + 1] - o[b]] = rows[o[b]:o[b + 1]]
    return out


# ------------------------------------------------------------------------------------------------ category bias
def torchmetrics_cosine(x: Tensor, y: Tensor, eps: float = 0.0) -> Tensor:
    """torchmetrics.functional.pairwise_cosine_similarity(x, y), its two lines restated: each operand divided by its row norm, no
    epsilon (``eps`` plants one), then the product."""
    x = x / (torch.norm(x, p=2, dim=1).unsqueeze(1) + eps)
    y = y / (torch.norm(y, p=2, dim=1).unsqueeze(1) + eps)
    return x @ y.T


def dropout_keeps(seeds: Sequence[int], p: float, n_hist: int, t: int, dc: int, by_column: bool = False):
    """(keep_hist [N_hist, Dc], keep_cand [T, Dc]) of the counter rule: element row * Dc + d, history at (seeds[0], SITE_HIST), candidates
    at (seeds[1], SITE_CAND).  ``by_column`` plants the mask indexed by d alone."""
    def keep(seed, site, rows):
        if by_column:
            return torch.from_numpy(np.broadcast_to(keep_rule(seed, site, p, np.arange(dc, dtype=np.uint64)), (rows, dc)).copy())
        return torch.from_numpy(keep_rule(seed, site, p, np.arange(rows * dc, dtype=np.uint64)).reshape(rows, dc))
    return keep(seeds[0], SITE_HIST, n_hist), keep(seeds[1], SITE_CAND, t)


def category_bias_full(table: Tensor, hist_cat: Tensor, cand_cat: Tensor, hist_off: Tensor, cand_off: Tensor, width: int, *,
                       keeps=None, p: float = 0.0, zero_own: bool = True, eps: float = 0.0) -> Tensor:
    """miner_module.py:162-181 -> the bias PolyAttention receives, [B, S, T]: embedding, dropout (``keeps`` = (keep_hist, keep_cand)),
    the cosine matrix, to dense by the history, the columns of each user's own candidates zeroed."""
    x, y = table[hist_cat], table[cand_cat]
    if keeps is not None:
        x, y = x * keeps[0].to(x.dtype) / (1.0 - p), y * keeps[1].to(y.dtype) / (1.0 - p)
    dense = to_dense(torchmetrics_cosine(x, y, eps), hist_off, width)
    co = cand_off.tolist()
    if zero_own:
        for b in range(len(co) - 1):                             # masked_fill_(mask, 0): a NaN in an own column goes too
            dense[b, :, co[b]:co[b + 1]] = 0.0
    return dense


def category_bias(table: Tensor, hist_cat: Tensor, cand_cat: Tensor, hist_off: Tensor, cand_off: Tensor, width: int, *, keeps=None,
                  p: float = 0.0, zero_own: bool = True, count_non_own: bool = False, eps: float = 0.0) -> Dict[str, Tensor]:
    """... and the mean over ALL T columns that attention.py:75 takes of it: bias [B, S, 1].  Planted defects: ``zero_own`` False,
    ``count_non_own`` (the mean over the non-own count), ``eps`` (an epsilon in the cosine)."""
    full = category_bias_full(table, hist_cat, cand_cat, hist_off, cand_off, width, keeps=keeps, p=p, zero_own=zero_own, eps=eps)
    if count_non_own:
        co = cand_off
        n = (full.shape[2] - (co[1:] - co[:-1])).to(full.dtype)
        return {"bias": (full.sum(dim=2) / n[:, None]).unsqueeze(2)}
    return {"bias": full.mean(dim=2, keepdim=True)}


def category_bias_abs(table, hist_cat, cand_cat, hist_off, cand_off, width, keeps=None, p=0.0) -> np.ndarray:
    """the absolute-value sum of the DERIVED bar, float64: (1 / T) sum over the NON-OWN columns t and over d of |x^_d y^_td|, [B, S, 1]; a
    NaN row counts as zeros here (its entries are compared by position, not by the bar)."""
    x, y = table.double()[hist_cat], table.double()[cand_cat]
    if keeps is not None:
        x, y = x * keeps[0].double() / (1.0 - p), y * keeps[1].double() / (1.0 - p)
    x = torch.nan_to_num(x / torch.norm(x, dim=1, keepdim=True)).abs()
    y = torch.nan_to_num(y / torch.norm(y, dim=1, keepdim=True)).abs()
    dense = to_dense(x @ y.T, hist_off, width)
    co = cand_off.tolist()
    for b in range(len(co) - 1):
        dense[b, :, co[b]:co[b + 1]] = 0.0
    return dense.mean(dim=2, keepdim=True).numpy()


class BiasCase:
    def __init__(self, name, hist_counts, cand_counts, dc, width=None, v=11, zero_row: Optional[str] = None):
        self.name, self.dc, self.v = name, dc, v
        self.hist_off, self.cand_off = offsets(hist_counts), offsets(cand_counts)
        self.width = max(hist_counts) if width is None else width
        n_hist, t = int(self.hist_off[-1]), int(self.cand_off[-1])
        rng = np.random.default_rng(3000 + dc + n_hist + t)
        self.table = randn(3100 + dc + n_hist, v, dc)
        self.hist_cat = torch.from_numpy(rng.integers(1, v, n_hist))
        self.cand_cat = torch.from_numpy(rng.integers(1, v, t))
        self.zero_row = zero_row
        if zero_row is not None:                                 # category 0 is an all-zero row (a padding category)
            self.table[0] = 0.0
            if zero_row == "cand":                               # among the candidates of impression 1
                self.cand_cat[int(self.cand_off[1])] = 0
            else:                                                # history row 1 of user 0
                self.hist_cat[1] = 0
        self.n = 2 * dc + t

    def args(self, device="cpu", dtype=torch.float64):
        return dict(table=self.table.to(device=device, dtype=dtype), hist_cat=self.hist_cat.to(device), cand_cat=self.cand_cat.to(device),
                    hist_off=self.hist_off.to(device), cand_off=self.cand_off.to(device), width=self.width)

    @functools.lru_cache(maxsize=None)
    def ref(self, seeds=None, p=0.0):
        keeps = None if seeds is None else dropout_keeps(seeds, p, self.hist_cat.numel(), self.cand_cat.numel(), self.dc)
        a = self.args()
        return category_bias(**a, keeps=keeps, p=p)["bias"], category_bias_abs(**self.args(dtype=torch.float32), keeps=keeps, p=p)

    def __repr__(self):
        return self.name


BIAS_RAGGED_HIST, BIAS_RAGGED_CAND = (9, 3, 6, 1, 8), (40, 7, 61, 2, 20)        # 130 candidates in total
#: the shipped width (four 64-lane trips and a tail), a width below one trip, one user (every entry exactly 0), T past one trip of the
#: exclusion sum, S at its bound
BIAS_CASES = {c.name: c for c in (
    BiasCase("shipped-Dc300", (7, 4, 1), (2, 5, 1), 300), BiasCase("Dc5", (7, 4, 1), (2, 5, 1), 5), BiasCase("one-user", (4,), (3,), 64),
    BiasCase("T130", BIAS_RAGGED_HIST, BIAS_RAGGED_CAND, 64), BiasCase("S256", (256, 3), (2, 3), 8))}
BIAS_ZERO_ROW_CASES = {c.name: c for c in (
    BiasCase("zero-cand-row", (7, 4, 1), (2, 5, 1), 64, zero_row="cand"), BiasCase("zero-hist-row", (7, 4, 1), (2, 5, 1), 64, zero_row="hist"),
    BiasCase("zero-hist-row-one-user", (4,), (3,), 64, zero_row="hist"))}
BIAS_DROPOUT_P, BIAS_DROPOUT_SEEDS = 0.2, (0x1234567890ABCDEF >> 2, 987654321987)


# ------------------------------------------------------------------------------------------------ scores over the context codes
def code_scores(cand: Tensor, user: Tensor, cand_off: Tensor, score_type: str, tie_last: bool = False) -> Dict[str, Tensor]:
    """miner_module.py:195-202 on the ragged rows: cand [N, D], user [B, K, D] -> [N].  A zero-padded row of the dense form scores 0
    and sends no gradient, so the ragged form is the same function.  ``tie_last`` plants ties going to the LAST code."""
    off = cand_off.tolist()
    out = []
    for b in range(len(off) - 1):
        m = cand[off[b]:off[b + 1]] @ user[b].T                  # [c, K]
        if score_type == "mean":
            out.append(m.mean(dim=1))
        elif tie_last:
            idx = m.shape[1] - 1 - m.flip(1).max(dim=1)[1]
            out.append(m.gather(1, idx[:, None])[:, 0])
        else:
            out.append(m.max(dim=1)[0])
    return {"out": torch.cat(out)}


def code_scores_terms(cand, user, cand_off, score_type, g, absolute=False, dtype=np.float64):
    """{name: (value, n)} as plain sums of products (the argmax taken from the signed float64 products in both forms)"""
    f = np.abs if absolute else (lambda a: a)
    cs, us, gs = (np.asarray(a, dtype) for a in (cand, user, g))
    c, u, g = f(cs), f(us), f(gs)
    b_n, k, d = u.shape
    out, dc, du = np.zeros(len(c), dtype), np.zeros_like(c), np.zeros_like(u)
    for b in range(b_n):
        sl = slice(cand_off[b], cand_off[b + 1])
        m = c[sl] @ u[b].T
        if score_type == "mean":
            out[sl] = m.mean(1)
            dc[sl] = (g[sl, None] / k) * u[b].sum(0)[None, :]
            du[b] = (g[sl] @ c[sl] / k)[None, :]
        else:
            arg = np.argmax(cs[sl] @ us[b].T, axis=1)            # the first maximum
            out[sl] = m[np.arange(len(arg)), arg]
            dc[sl] = g[sl, None] * u[b][arg]
            for j, a in enumerate(arg):
                du[b, a] += g[sl][j] * c[sl][j]
    n = d if score_type == "max" else d + k
    return {"out": (out, n), "d_cand": (dc, n), "d_user": (du, n)}


#: (B, K, D, candidate counts): the golden widths, K = 32 with a user past 32 four-candidate workgroups, K past half a wave with an odd
#: width, one code
SCORE_SHAPES = ((3, 5, 64, (6, 4, 1)), (2, 32, 256, (130, 1)), (2, 33, 100, (9, 2)), (2, 1, 64, (3, 3)))
SCORE_TYPES = ("max", "mean")


@functools.lru_cache(maxsize=None)
def scores_case(b, k, d, counts, score_type, tie=False) -> Case:
    sd = 3200 + k + d + sum(counts)
    off = offsets(counts)
    cand, user, g = randn(sd, int(off[-1]), d, scale=2.0 * d ** -0.5), randn(sd + 1, b, k, d), randn(sd + 2, int(off[-1]))
    if tie:
        user[:, 2] = user[:, 0]                                  # code 2 ties with code 0 bit for bit ...
        # ... and every product of a candidate with them is positive, so the pair is the maximum of every candidate
        cand = cand.abs() * torch.sign(user[torch.repeat_interleave(torch.arange(b), torch.tensor(counts)), 0])
    terms = functools.partial(code_scores_terms, cand.numpy(), user.numpy(), off.tolist(), score_type, g.numpy())
    return Case(f"scores-{score_type}-B{b}-K{k}-D{d}" + ("-tie" if tie else ""), code_scores, {"cand": cand, "user": user},
                {"cand_off": off, "score_type": score_type}, {"out": g}, terms)


# ------------------------------------------------------------------------------------------------ disagreement loss
def pairwise_cosine_similarity_3d(x: Tensor, y: Tensor, zero_diagonal: bool = False, one_plus_norm: bool = False) -> Tensor:
    """components/utils.py:4-31.  Its two lines ``x_norm[torch.where(x_norm)==0.0] = 1`` compare a TUPLE with a float — False, i.e.
    index 0 of a new leading axis of size 0 after broadcasting: they assign nothing — so they are left out; a zero row is
    0 / 1e-8 = 0.  ``one_plus_norm`` plants 1 + norm in place of 1e-8 + norm."""
    x_norm = torch.linalg.norm(x, dim=2, keepdim=True)
    y_norm = torch.linalg.norm(y, dim=2, keepdim=True)
    e = 1.0 if one_plus_norm else 1e-8
    x = torch.div(x, e + x_norm)
    y = torch.div(y, e + y_norm)
    distance = torch.matmul(x, y.permute(0, 2, 1))
    if zero_diagonal:
        mask = torch.eye(x.shape[1]).repeat(x.shape[0], 1, 1).bool()
        distance = distance.masked_fill(mask.to(distance.device), 0)
    return distance


def disagreement(user: Tensor, keep_diagonal: bool = False, k_minus_one: bool = False, one_plus_norm: bool = False) -> Dict[str, Tensor]:
    """miner_module.py:237-241: the off-diagonal cosines, ``.mean()`` = divided by B K K.  Planted: the diagonal kept, the divisor
    B K (K - 1), 1 + norm."""
    dist = pairwise_cosine_similarity_3d(user, user, zero_diagonal=not keep_diagonal, one_plus_norm=one_plus_norm)
    b, k, _ = user.shape
    return {"loss": dist.sum() / (b * k * (k - 1)) if k_minus_one else dist.mean()}


#: (B, K, D): the golden shape, the shipped widths, K past half a wave with an odd width, users past one 64-user reduction group, and
#: one vector per user (loss and gradient exactly 0)
DISAGREEMENT_SHAPES = ((3, 5, 64), (2, 32, 256), (2, 33, 100), (130, 2, 8), (1, 1, 4))
DISAGREEMENT_ZERO_ROW = (1, 3)


@functools.lru_cache(maxsize=None)
def disagreement_case(b, k, d, zero_row=False) -> Case:
    def build(salt):
        user = randn(3300 + b + k + d + salt, b, k, d)
        if zero_row:
            user[DISAGREEMENT_ZERO_ROW] = 0.0
        return Case(f"disagreement-B{b}-K{k}-D{d}" + ("-zero-row" if zero_row else ""), disagreement, {"user": user}, {}, {"loss": torch.tensor(0.75)})
    if not zero_row:
        return settled(build)
    for salt in range(32):                                       # `settled`, with the two parts of the gradient judged on their own
        case = build(salt * 100003)
        figures = [v["cpu_f32"] for v in case.bars().values()] + [v["cpu_f32"] for v in zero_row_bars(case).values()]
        if all(f == 0 or f >= QUARTER_ULP for f in figures):
            return case
    raise AssertionError("no salt in 32 settles the case")


def zero_row_parts(d_user: Tensor) -> Dict[str, Tensor]:
    """the gradient of the zero row (scaled by 1 / 1e-8) and of the remaining rows: compared separately, each relative to its own
    largest entry — otherwise the 1e8-scaled row sets the scale for all"""
    rest = torch.ones(d_user.shape[:2], dtype=torch.bool)
    rest[DISAGREEMENT_ZERO_ROW] = False
    return {"d_user_zero_row": d_user[DISAGREEMENT_ZERO_ROW], "d_user_rest": d_user[rest]}


def zero_row_bars(case: Case):
    return measured_bars(zero_row_parts(case.ref(torch.float64)["d_user"]), zero_row_parts(case.ref(torch.float32)["d_user"]))


# ------------------------------------------------------------------------------------------------ forward + model_step's loss
def cross_entropy_dense(ragged: Tensor, labels: Tensor, cand_off: Tensor, c_max: int, pad_in_softmax: bool = True) -> Tensor:
    """nn.CrossEntropyLoss(scores [B, Cmax], y_true [B, Cmax]) with probability targets on the zero-padded rows: the padded zeros ARE
    in the softmax (``pad_in_softmax`` False plants them left out); mean over the batch."""
    dense, y = to_dense(ragged, cand_off, c_max), to_dense(labels.to(ragged.dtype), cand_off, c_max)
    logits = dense
    if not pad_in_softmax:
        real = to_dense(torch.ones_like(ragged), cand_off, c_max) > 0
        logits = dense.masked_fill(~real, float("-inf"))
    lse = torch.logsumexp(logits, dim=1, keepdim=True)
    return -(y * (dense - lse)).sum(dim=1).mean()


def miner_step(hist: Tensor, cand: Tensor, poly_w: Tensor, codes: Tensor, target_w: Tensor, table: Tensor, hist_cat: Tensor, cand_cat: Tensor,
               hist_off: Tensor, cand_off: Tensor, labels: Tensor, score_type: str, pad_in_softmax: bool = True) -> Dict[str, Tensor]:
    """MINERModule.forward (miner_module.py:153-212) and the loss lines of model_step (:226-242) on ragged news vectors hist [N_hist, D],
    cand [N_cand, D], with the category bias (no dropout): ragged scores and the loss."""
    ho, co = hist_off, cand_off
    s, c_max = int((ho[1:] - ho[:-1]).max()), int((co[1:] - co[:-1]).max())
    hist_dense, cand_dense = to_dense(hist, ho, s), to_dense(cand, co, c_max)
    mask = torch.arange(s)[None, :] < (ho[1:] - ho[:-1])[:, None]
    bias = category_bias_full(table.to(hist.dtype), hist_cat, cand_cat, ho, co, s)
    out = M.miner_forward(hist_dense, cand_dense, poly_w, codes, target_w, mask, bias, score_type)
    real = torch.arange(c_max)[None, :] < (co[1:] - co[:-1])[:, None]
    ragged = out["scores"][real]
    loss = cross_entropy_dense(ragged, labels, co, c_max, pad_in_softmax) + disagreement(out["user"])["loss"]
    return {"loss": loss, "scores": ragged}


STEP_HIST, STEP_CAND, STEP_DC, STEP_V = (9, 5, 2), (6, 4, 1), 16, 7          # B, S, D, Q, K, C, T of miner_ref.MINER_SHAPE


@functools.lru_cache(maxsize=None)
def step_case(score_type: str) -> Case:
    b, s, d, q, k, c, t = M.MINER_SHAPE
    assert (b, s, c, t) == (len(STEP_HIST), max(STEP_HIST), max(STEP_CAND), sum(STEP_CAND))
    ho, co = offsets(STEP_HIST), offsets(STEP_CAND)

    def build(salt):
        sd = 3400 + salt
        rng = np.random.default_rng(sd)
        leaves = {"hist": randn(sd, int(ho[-1]), d), "cand": randn(sd + 1, t, d, scale=2.0 * d ** -0.5), "poly_w": randn(sd + 2, q, d, scale=d ** -0.5),
                  "codes": randn(sd + 3, k, q, scale=2.0 * q ** -0.5), "target_w": randn(sd + 4, d, d, scale=d ** -0.5)}
        labels = torch.zeros(t)
        labels[co[:-1]] = 1.0                                    # the clicked candidate comes first
        consts = {"table": randn(sd + 5, STEP_V, STEP_DC), "hist_cat": torch.from_numpy(rng.integers(0, STEP_V, int(ho[-1]))),
                  "cand_cat": torch.from_numpy(rng.integers(0, STEP_V, t)), "hist_off": ho, "cand_off": co, "labels": labels,
                  "score_type": score_type}
        return Case(f"miner-step-{score_type}", miner_step, leaves, consts, {"loss": torch.tensor(0.75)})
    return settled(build)


def all_measured_cases():
    return ([disagreement_case(*s) for s in DISAGREEMENT_SHAPES] + [disagreement_case(3, 5, 64, True)] + [step_case(t) for t in M.SCORE_TYPES])
