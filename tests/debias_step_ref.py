"""Float64 restatements of what makes SentiDebias-PLM itself (reference manner/models/baselines/senti_debias_plm_module.py): the sentiment
encoder (:41-42), the three orthogonality terms (:109-135), the bias-aware scores (:142-146), the discriminator with its wrapped one-hot
target (:163-167, 275-280) and the loss lines of the two optimiser steps (:339-355) — written from the module's lines in plain torch,
dtype-generic, with autograd for the gradients — and the cases the kernels of csrc/debias.hip are run at.  No GPU in this file:
tests/test_debias_step_host.py checks the restatements on the CPU, tests/test_gpu_debias_step.py runs the kernels against them.

There is NO golden of the LightningModule itself: lightning, torchmetrics and torch_geometric are not installed where these tests run, so
``SentiDebiasPLMModule`` cannot be imported.  What the host tests hold the restatements to instead is a second formulation in torch's own
calls: dense ``pad_sequence`` blocks with ``bmm``, ``nn.Embedding(padding_idx=0)``, and ``nn.CrossEntropyLoss`` against an explicit
one-hot matrix filled by the module's own loop ``y_true[i, targets[i] - 1] = 1``.

The shapes of the module's lines 109-135: ``loss_orth_clicked_news`` and ``loss_orth_candidate_news`` are SCALARS (a mean over all rows of
the set), ``loss_orth_user`` is [B, 1]; ``|s1| + |s2| + |[B, 1]|`` broadcasts to [B, 1] and its mean is
``|s1| + |s2| + mean_b |cos_b|``: the absolute value sits outside the mean for the two news terms and inside it for the user term.

Bars: MEASURED of tests/side_ops_ref.py for everything (8 x the float32 CPU error against float64), every case ``settled``.

Kinks of |.| are kept away from by the inputs, never by leaving entries out of a comparison: a news row is noise plus +-0.5 sqrt(D) times
the unit vector of its class's table row, + for the history and - for the candidates, so each set's mean cosine is near +-0.45; a
bias-aware user vector is noise plus +-0.5 times the bias-free one, the sign alternating over the users.
"""
from __future__ import annotations

import functools
from typing import Dict

import numpy as np
import torch

from miner_step_ref import cross_entropy_dense, offsets, to_dense
from side_ops_ref import LOSS_COUNTS, Case, randn, settled

Tensor = torch.Tensor
ALPHA, BETA = 0.15, 10.0                                        # configs/model/senti_debias_plm.yaml: alpha_coefficient, beta_coefficient


# ------------------------------------------------------------------------------------------------ the module's lines
def cos_eps(a: Tensor, b: Tensor) -> Tensor:
    """a . b / (1e-8 + |a| |b|) per row: the epsilon outside the product, as upstream"""
    return (a * b).sum(dim=-1) / (1e-8 + torch.linalg.norm(a, dim=-1, ord=2) * torch.linalg.norm(b, dim=-1, ord=2))


def class_table(embedding: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    """SentimentEncoder.forward of every class: row 0 is ``padding_idx``: read as it lies, no gradient into the embedding"""
    return torch.tanh(torch.cat((embedding[:1].detach(), embedding[1:])) @ weight.T + bias)


def orth_loss(rows: Tensor, table: Tensor, user_free: Tensor, user_aware: Tensor, cls: Tensor, n_hist: int) -> Dict[str, Tensor]:
    cos = cos_eps(rows, table[cls])
    return {"loss": cos[:n_hist].mean().abs() + cos[n_hist:].mean().abs() + cos_eps(user_free, user_aware).abs().mean()}


def segments(off: Tensor) -> Tensor:
    return torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1])


def class_dense(table: Tensor, cls: Tensor, off: Tensor, width: int) -> Dict[str, Tensor]:
    return {"out": to_dense(table[cls], off, width)}


def class_scores(user: Tensor, table: Tensor, cls: Tensor, off: Tensor) -> Dict[str, Tensor]:
    return {"scores": (user[segments(off)] * table[cls]).sum(dim=-1)}


def adv_rows(rows: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, cls: Tensor) -> Tensor:
    """-log softmax(W2 tanh(W1 x + b1) + b2)[(cls - 1) mod O] per row"""
    logits = torch.tanh(rows @ w1.T + b1) @ w2.T + b2
    logp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
    return -logp[torch.arange(rows.shape[0]), (cls - 1) % w2.shape[0]]


def adv_loss(rows: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, cls: Tensor, n_hist: int) -> Dict[str, Tensor]:
    """two means summed, not one mean over all rows"""
    ce = adv_rows(rows, w1, b1, w2, b2, cls)
    return {"loss": ce[:n_hist].mean() + ce[n_hist:].mean()}


def generator_lines(hist: Tensor, cand: Tensor, user_free: Tensor, user_aware: Tensor, senti_hist: Tensor, senti_cand: Tensor, w1: Tensor,
                    b1: Tensor, w2: Tensor, b2: Tensor, cls_hist: Tensor, cls_cand: Tensor, labels: Tensor, cand_off: Tensor, c_max: int,
                    alpha: float = ALPHA, beta: float = BETA) -> Dict[str, Tensor]:
    """senti_debias_plm_module.py:109-146 and 339-343 below the encoders, on the [N, D] sentiment rows as the module forms them ->
    g_loss, loss_orth, the dense combined and bias-free scores"""
    orth = cos_eps(hist, senti_hist).mean().abs() + cos_eps(cand, senti_cand).mean().abs() + cos_eps(user_free, user_aware).abs().mean()
    seg = segments(cand_off)
    free = (user_free[seg] * cand).sum(dim=-1)
    combined = free + (user_aware[seg] * senti_cand).sum(dim=-1)
    adv = adv_rows(hist, w1, b1, w2, b2, cls_hist).mean() + adv_rows(cand, w1, b1, w2, b2, cls_cand).mean()
    loss = cross_entropy_dense(combined, labels, cand_off, c_max) + beta * orth - alpha * adv
    return {"loss": loss, "orth": orth, "combined": to_dense(combined, cand_off, c_max), "free": to_dense(free, cand_off, c_max)}


# ------------------------------------------------------------------------------------------------ cases: the orthogonality loss
#: (n_hist, n_cand, D, C, B) and the loop of csrc/debias.hip each one is the smallest shape for:
#:   (1, 1, 4, 2, 1)         a segment of one row, twice; one 64-lane trip with 4 live lanes; one user
#:   (5, 4, 260, 4, 4)       9 rows: wave 0's second row (rows w + 4 i of a workgroup's 8) and a second workgroup with one row; D = 260: a
#:                           fifth 64-lane trip with 4 live lanes and five column blocks of the binned sums; the shipped C
#:   (20, 13, 768, 16, 5)    33 rows: the second chunk of the binned sums (32 rows each), one row in it; the shipped D; C = 16
#:   (4200, 4000, 4, 2, 5)   8200 rows: past 512 workgroups x 8 rows, the grid-stride loop's second and third trip; past 128 chunks x 32 rows,
#:                           chunks of 65 rows; the segment-mean kernel's 17th trip
ORTH_SHAPES = ((1, 1, 4, 2, 1), (5, 4, 260, 4, 4), (20, 13, 768, 16, 5), (4200, 4000, 4, 2, 5))


def classes(seed: int, n: int, c: int) -> Tensor:
    """classes in [0, c), every one of them present when n >= c, class 0 first"""
    t = torch.from_numpy(np.random.default_rng(seed).integers(0, c, n))
    if n >= c:
        t[:c] = torch.arange(c)
    else:
        t[0] = 0
    return t


def _orth_leaves(nh, nc, d, c, b, sd):
    n = nh + nc
    cls = classes(sd + 5, n, c)
    table = torch.tanh(randn(sd + 1, c, d))
    sign = torch.cat((torch.ones(nh), -torch.ones(nc)))[:, None]
    unit = table[cls] / table[cls].norm(dim=1, keepdim=True)
    rows = randn(sd, n, d) + sign * 0.5 * d ** 0.5 * unit
    user_free = randn(sd + 2, b, d)
    flip = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(b)])[:, None]
    user_aware = randn(sd + 3, b, d) + flip * 0.5 * user_free
    return {"rows": rows, "table": table, "user_free": user_free, "user_aware": user_aware}, cls


def _orth_case(nh, nc, d, c, b, salt) -> Case:
    leaves, cls = _orth_leaves(nh, nc, d, c, b, 5000 + nh + nc + d + c + b + salt)
    return Case(f"orth-Nh{nh}-Nc{nc}-D{d}-C{c}-B{b}", orth_loss, leaves, {"cls": cls, "n_hist": nh}, {"loss": torch.tensor(0.75)})


@functools.lru_cache(maxsize=None)
def orth_case(nh: int, nc: int, d: int, c: int, b: int) -> Case:
    return settled(lambda salt: _orth_case(nh, nc, d, c, b, salt))


ZERO_ROW = 2


@functools.lru_cache(maxsize=None)
def orth_zero_case() -> Case:
    """(5, 4, 260, 4, 4) with news row 2 all zero: its cosine is 0 / 1e-8 = 0 and its own gradient T[cls] / 1e-8 — held apart from the
    other rows', which it would dwarf — with torch's zero through the norm of the zero vector"""
    def build(salt):
        case = _orth_case(5, 4, 260, 4, 4, salt + 7)
        case.leaves["rows"][ZERO_ROW] = 0.0
        case.name += "-zero-row"
        return case
    return settled(build)


def orth_kink_clearance(case: Case):
    """-> the smallest of |mean_hist cos|, |mean_cand cos|, min_b |cos_b| in float64: how far the inputs keep from the kinks"""
    lv, cs = case.leaves, case.consts
    cos = cos_eps(lv["rows"].double(), lv["table"].double()[cs["cls"]])
    nh = cs["n_hist"]
    return min(float(cos[:nh].mean().abs()), float(cos[nh:].mean().abs()), float(cos_eps(lv["user_free"].double(), lv["user_aware"].double()).abs().min()))


# ------------------------------------------------------------------------------------------------ cases: class_dense / class_scores
#: (B, D, C) with the row counts cycled from side_ops_ref.LOSS_COUNTS = (65, 130, 63, 2, 64, 1), as tests/test_gpu_aspect_step.py:
#:   (1, 4, 2)      one user, 65 rows: a lane's second candidate in the gather; three chunks of the dense binned sums
#:   (4, 260, 4)    ragged counts 65 / 130 / 63 / 2: a lane's third candidate, padded slots; D = 260: the column tail
#:   (5, 768, 16)   the shipped D, a user of 64 rows; C = 16
#:   (17, 4, 2)     class_dense: 17 x 137 = 2329 dense rows, past 512 workgroups x 4 rows: the grid-stride loop's second trip
RAGGED_SHAPES = ((1, 4, 2), (4, 260, 4), (5, 768, 16), (17, 4, 2))
DENSE_PAD = 7


def ragged_counts(b: int):
    return [LOSS_COUNTS[i % len(LOSS_COUNTS)] for i in range(b)]


def _dense_case(b, d, c, salt) -> Case:
    sd = 5200 + b + d + c + salt
    counts = ragged_counts(b)
    off = offsets(counts)
    width = max(counts) + DENSE_PAD
    cls = classes(sd + 1, int(off[-1]), c)
    return Case(f"class-dense-B{b}-D{d}-C{c}", class_dense, {"table": torch.tanh(randn(sd, c, d))}, {"cls": cls, "off": off, "width": width},
                {"out": randn(sd + 2, b, width, d)})


@functools.lru_cache(maxsize=None)
def dense_case(b: int, d: int, c: int) -> Case:
    return settled(lambda salt: _dense_case(b, d, c, salt))


def _scores_case(b, d, c, salt) -> Case:
    sd = 5300 + b + d + c + salt
    off = offsets(ragged_counts(b))
    cls = classes(sd + 1, int(off[-1]), c)
    return Case(f"class-scores-B{b}-D{d}-C{c}", class_scores, {"user": randn(sd, b, d), "table": torch.tanh(randn(sd + 2, c, d))},
                {"cls": cls, "off": off}, {"scores": randn(sd + 3, int(off[-1]))})


@functools.lru_cache(maxsize=None)
def scores_case(b: int, d: int, c: int) -> Case:
    return settled(lambda salt: _scores_case(b, d, c, salt))


# ------------------------------------------------------------------------------------------------ cases: the adversarial head
#: (n_hist, n_cand, D, H, O):
#:   (1, 1, 4, 3, 2)          a segment of one row, twice; one staging of the matrix-core linear with 4 live features; one class block
#:   (5, 4, 260, 33, 4)       9 rows: a wave's second row and a second workgroup; D = 260: the linear's ninth staging with 4 live features;
#:                            H = 33: a second 32-feature tile with one live feature; the shipped O
#:   (20, 13, 768, 400, 4)    the shipped widths; 33 rows: a second 32-row tile and a second chunk of the fixed-order sums with one row
#:   (5, 4, 8, 33, 19)        five class blocks, the last with three live classes; the 32-class instance of the W2 gradient
#:   (5, 4, 8, 400, 64)       W2 of 100 KB: staged in LDS past the 64 KB a launch gets without asking; the 64-class instance
#:   (5, 4, 8, 1024, 64)      W2 of 256 KB: NOT staged, read through L2; the largest hidden row
#:   (515, 515, 4, 3, 2)      1030 rows: the linear's 128 x 64 tile (the switch is at 1024 rows), forward and for d x
#:   (4200, 4000, 4, 3, 2)    8200 rows: the row walks' second and third grid-stride trip; chunks of 65 rows
ADV_SHAPES = ((1, 1, 4, 3, 2), (5, 4, 260, 33, 4), (20, 13, 768, 400, 4), (5, 4, 8, 33, 19), (5, 4, 8, 400, 64), (5, 4, 8, 1024, 64),
              (515, 515, 4, 3, 2), (4200, 4000, 4, 3, 2))


def _adv_leaves(n, d, h, o, sd):
    return {"rows": randn(sd, n, d), "w1": randn(sd + 1, h, d, scale=d ** -0.5), "b1": randn(sd + 2, h, scale=0.1),
            "w2": randn(sd + 3, o, h, scale=h ** -0.5), "b2": randn(sd + 4, o, scale=0.1)}


def _adv_case(nh, nc, d, h, o, salt) -> Case:
    sd = 5400 + nh + nc + d + h + o + salt
    return Case(f"adv-Nh{nh}-Nc{nc}-D{d}-H{h}-O{o}", adv_loss, _adv_leaves(nh + nc, d, h, o, sd),
                {"cls": classes(sd + 5, nh + nc, o), "n_hist": nh}, {"loss": torch.tensor(0.75)})


@functools.lru_cache(maxsize=None)
def adv_case(nh: int, nc: int, d: int, h: int, o: int) -> Case:
    return settled(lambda salt: _adv_case(nh, nc, d, h, o, salt))


# ------------------------------------------------------------------------------------------------ the two steps
STEP_HIST, STEP_CAND, STEP_CLASSES, STEP_E, STEP_H = (9, 5, 2), (6, 4, 1), 4, 12, 33           # B = 3


def step_consts(salt: int = 0):
    """labels and sentiment classes of the B = 3 step batch (the news rows come from the encoder under test)"""
    ho, co = offsets(STEP_HIST), offsets(STEP_CAND)
    nh, t = int(ho[-1]), int(co[-1])
    labels = torch.zeros(t)
    labels[co[:-1]] = 1.0
    return {"hist_off": ho, "cand_off": co, "labels": labels, "c_max": max(STEP_CAND), "cls_hist": classes(5500 + salt, nh, STEP_CLASSES),
            "cls_cand": classes(5501 + salt, t, STEP_CLASSES)}


def step_rows(d: int, cs, table: Tensor, salt: int = 0) -> Tensor:
    """news rows [N_hist + N_cand, d] kept away from the kinks as the orth cases' rows are, for a given class table"""
    nh, t = int(cs["hist_off"][-1]), int(cs["cand_off"][-1])
    cls = torch.cat((cs["cls_hist"], cs["cls_cand"]))
    sign = torch.cat((torch.ones(nh), -torch.ones(t)))[:, None]
    unit = table[cls] / table[cls].norm(dim=1, keepdim=True)
    return randn(5600 + salt, nh + t, d) + sign * 0.5 * d ** 0.5 * unit.float()


def all_measured_cases():
    cases = [orth_case(*s) for s in ORTH_SHAPES] + [adv_case(*s) for s in ADV_SHAPES]
    return cases + [dense_case(*s) for s in RAGGED_SHAPES] + [scores_case(*s) for s in RAGGED_SHAPES]
