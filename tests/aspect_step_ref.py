"""Float64 restatements of what makes TANR-PLM and SentiRec-PLM themselves (reference manner/models/baselines/tanr_plm_module.py:139-141,
172-177 and sentirec_plm_module.py:141-143,174-193): the topic head with its cross-entropy, the sentiment head with its L1 loss, the
sentiment diversity regulariser, and the loss lines of the two ``model_step``s over them — written from their definitions in plain torch,
dtype-generic, with autograd for the gradients — and the cases the kernels of csrc/aspect.hip are run at.  No GPU in this file:
tests/test_aspect_step_host.py checks the restatements on the CPU, tests/test_gpu_aspect_step.py runs the kernels against them.

There is NO golden of the two LightningModules themselves: lightning, torchmetrics and torch_geometric are not installed where these tests
run, so ``TANRPLMModule`` / ``SentiRecPLMModule`` cannot be imported.  What the host tests hold the restatements to instead are torch's
own calls the modules make — ``nn.CrossEntropyLoss`` with one-hot probability targets, ``nn.L1Loss``, ``F.relu(...).mean()`` on dense
zero-padded blocks.

Bars: those of tests/side_ops_ref.py, used as they are.  DERIVED for the optional logits output (``linear_terms``, n = D) and for the
finite gradients of the empty-history case (a product of h + 4 roundings); MEASURED for the three losses and all their gradients.

Kinks are kept out by the choice of inputs, never by leaving entries out of a comparison:
* L1: every target is the float64 head output minus a residual drawn with 0.1 <= |r| <= 1.5, far above the rounding of the row's dot
  product, (D + 4) 2^-24 sum |x w|; or the row is all zero with target == bias, the residual exactly 0 in every arithmetic — it must send
  gradient 0 (torch's sign(0)).
* senti_div: history scores have one sign per user and 0.2 <= |s| <= 1, candidate scores 0.2 <= |s| <= 1 of either sign, scores
  0.1 <= |score| <= 2: every product u s score is at least 4e-3 in size, far above its rounding — or exactly 0: a neutral news with
  s = 0.0, and the padded slots.
"""
from __future__ import annotations

import functools
from typing import Dict, Sequence

import numpy as np
import torch

from miner_step_ref import cross_entropy_dense, offsets, to_dense
from side_ops_ref import LOSS_COUNTS, U32, Case, linear_terms, randn, settled

Tensor = torch.Tensor
TOPIC_COEF, SENTI_PRED_COEF, SENTI_DIV_COEF = 0.2, 0.4, 10.0           # configs/model/tanr_plm.yaml, sentirec_plm.yaml


# ------------------------------------------------------------------------------------------------ the three losses
def head_ce(x: Tensor, weight: Tensor, bias: Tensor, target: Tensor) -> Dict[str, Tensor]:
    """the mean over all rows of -log softmax(x W^T + b)[target]"""
    logits = x @ weight.T + bias
    logp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
    return {"loss": -logp[torch.arange(x.shape[0]), target].sum() / x.shape[0]}


def head_l1(x: Tensor, weight: Tensor, bias: Tensor, target: Tensor) -> Dict[str, Tensor]:
    """the mean of |x . w + b - target|; weight [1, D], bias [1]"""
    res = x @ weight[0] + bias[0] - target.to(x.dtype)
    return {"loss": res.abs().sum() / x.shape[0]}


def senti_div(scores: Tensor, cand_score: Tensor, hist_score: Tensor, hist_off: Tensor, cand_off: Tensor, c_max: int) -> Dict[str, Tensor]:
    """(1 / (B c_max)) sum over the impressions b and their candidates t of max(u_b s_t score_t, 0), u_b = the mean of user b's history
    sentiment scores; the padded slots of the dense block add 0 for a user with a history and count in the divisor.  A user without one has
    u = 0 / 0 = NaN, and NaN times the padded zeros is NaN too: its impression adds NaN whatever its candidate count.  ``v * (v > 0)``
    keeps a NaN where ``relu`` keeps it."""
    ho, co = hist_off.tolist(), cand_off.tolist()
    b = len(co) - 1
    total = scores.new_zeros(())
    for i in range(b):
        u = hist_score[ho[i]:ho[i + 1]].to(scores.dtype).sum() / (ho[i + 1] - ho[i])
        v = u * cand_score[co[i]:co[i + 1]].to(scores.dtype) * scores[co[i]:co[i + 1]]
        total = total + (v * (v > 0).to(v.dtype)).sum()
        if co[i + 1] - co[i] < c_max:
            total = total + u * 0.0                              # the padded slots: 0, or the NaN of an empty history
    return {"loss": total / (b * c_max)}


# ------------------------------------------------------------------------------------------------ cases of the two heads
#: (N, D, O) and the loop of csrc/aspect.hip each one is the smallest shape for:
#:   (1, 4, 2)        one row, one lane group, one block of four classes with two of them past O
#:   (9, 260, 19)     wave 0's second row (rows w + 4 i of a workgroup's 8) and the second workgroup; D = 260: a fifth 64-lane trip with 4
#:                    live lanes; O = 19: five class blocks, the last with one live class; the 32-class weight-gradient kernel
#:   (33, 1024, 19)   a weight of 76 KB: staged in LDS past the 64 KB a launch gets without asking; the second chunk of the weight
#:                    gradient (32 rows each)
#:   (257, 768, 19)   the shipped widths; the mean kernel's second trip (256 threads); 9 weight-gradient chunks
#:   (513, 1024, 64)  a weight of 256 KB: NOT staged, read through L2; the mean kernel's third trip; every lane a class; the 64-class
#:                    weight-gradient kernel; 17 chunks
#:   (8200, 4, 2)     past 512 workgroups x 8 rows: the grid-stride loop's second and third trip; past 128 chunks x 32 rows: chunks of
#:                    65 rows
HEAD_SHAPES = ((1, 4, 2), (9, 260, 19), (33, 1024, 19), (257, 768, 19), (513, 1024, 64), (8200, 4, 2))
ZERO_ROW = 3                                                    # L1, N >= 9: this row is all zero with target == bias


def _head_leaves(n, d, o, sd):
    return {"x": randn(sd, n, d), "weight": randn(sd + 1, o, d, scale=d ** -0.5), "bias": randn(sd + 2, o, scale=0.1)}


def _ce_case(n, d, o, salt) -> Case:
    sd = 4000 + n + d + o + salt
    target = torch.from_numpy(np.random.default_rng(sd + 3).integers(0, o, n))
    if n >= o:
        target[:o] = torch.arange(o)                             # every class occurs
    return Case(f"head-ce-N{n}-D{d}-O{o}", head_ce, _head_leaves(n, d, o, sd), {"target": target}, {"loss": torch.tensor(0.75)})


@functools.lru_cache(maxsize=None)
def ce_case(n: int, d: int, o: int) -> Case:
    return settled(lambda salt: _ce_case(n, d, o, salt))


def ce_logits_terms(case: Case, absolute: bool = False):
    """(value, n) of the logits as plain sums of products: side_ops_ref.linear_terms"""
    lv = case.leaves
    return linear_terms(lv["x"].numpy(), lv["weight"].numpy(), lv["bias"].numpy(), np.zeros((lv["x"].shape[0], lv["weight"].shape[0])),
                        absolute=absolute)["y"]


def l1_residuals(n: int, sd: int) -> Tensor:
    rng = np.random.default_rng(sd)
    return torch.from_numpy(rng.uniform(0.1, 1.5, n) * rng.choice([-1.0, 1.0], n))


def _l1_case(n, d, salt) -> Case:
    sd = 4100 + n + d + salt
    leaves = _head_leaves(n, d, 1, sd)
    if n > ZERO_ROW:
        leaves["x"][ZERO_ROW] = 0.0
    y64 = leaves["x"].double() @ leaves["weight"][0].double() + leaves["bias"][0].double()
    target = (y64 - l1_residuals(n, sd + 3)).float()
    if n > ZERO_ROW:
        target[ZERO_ROW] = leaves["bias"][0]
    return Case(f"head-l1-N{n}-D{d}", head_l1, leaves, {"target": target}, {"loss": torch.tensor(0.75)})


@functools.lru_cache(maxsize=None)
def l1_case(n: int, d: int) -> Case:
    return settled(lambda salt: _l1_case(n, d, salt))


def l1_kink_clearance(case: Case):
    """-> (the smallest ratio |residual| / ((D + 4) 2^-24 (sum |x w| + |b| + |t|)) over the rows whose float64 residual is not exactly
    zero, the indices of the rows where it is)"""
    lv, t = case.leaves, case.consts["target"].double()
    x, w, b = lv["x"].double(), lv["weight"][0].double(), lv["bias"][0].double()
    res = x @ w + b - t
    bound = (x.shape[1] + 4) * U32 * ((x.abs() @ w.abs()) + b.abs() + t.abs())
    live = res != 0
    return float((res.abs() / bound)[live].min()) if bool(live.any()) else float("inf"), torch.nonzero(~live).reshape(-1).tolist()


# ------------------------------------------------------------------------------------------------ cases of the regulariser
SENTI_B, SENTI_HIST, SENTI_PAD = (1, 4, 5), (1, 2, 50), 7       # candidate counts cycle through side_ops_ref.LOSS_COUNTS


def senti_inputs(b: int, salt: int = 0, empty: Sequence[int] = ()):
    rng = np.random.default_rng(4200 + b + salt)
    counts = [LOSS_COUNTS[i % len(LOSS_COUNTS)] for i in range(b)]
    hist = [0 if i in empty else SENTI_HIST[i % len(SENTI_HIST)] for i in range(b)]
    ho, co = offsets(hist), offsets(counts)
    t, nh = int(co[-1]), int(ho[-1])
    sign_user = np.repeat(rng.choice([-1.0, 1.0], b), hist)
    hist_score = torch.from_numpy((rng.uniform(0.2, 1.0, nh) * sign_user).astype(np.float32))
    cand_score = rng.uniform(0.2, 1.0, t) * rng.choice([-1.0, 1.0], t)
    cand_score[rng.random(t) < 0.15] = 0.0                       # neutral news
    cand_score[0] = 0.0
    scores = rng.uniform(0.1, 2.0, t) * rng.choice([-1.0, 1.0], t)
    return torch.from_numpy(scores.astype(np.float32)), torch.from_numpy(cand_score.astype(np.float32)), hist_score, ho, co, max(counts)


def _senti_case(b, padded, salt, empty=()) -> Case:
    scores, cand_score, hist_score, ho, co, widest = senti_inputs(b, salt, empty)
    consts = {"cand_score": cand_score, "hist_score": hist_score, "hist_off": ho, "cand_off": co, "c_max": widest + (SENTI_PAD if padded else 0)}
    name = f"senti-div-B{b}-{'padded' if padded else 'tight'}" + ("-empty-history" if empty else "")
    return Case(name, senti_div, {"scores": scores}, consts, {"loss": torch.tensor(0.75)})


@functools.lru_cache(maxsize=None)
def senti_case(b: int, padded: bool) -> Case:
    return settled(lambda salt: _senti_case(b, padded, salt))


@functools.lru_cache(maxsize=None)
def senti_empty_case() -> Case:
    """user 1 of 4 has no history: the loss is NaN, and so are the gradients of that user's candidates — and only those"""
    return _senti_case(4, True, 0, empty=(1,))


def senti_kink_clearance(case: Case):
    """-> (the smallest ratio |u s score| / ((h + 4) 2^-24 mean|hist| |s| |score|) over the real slots whose float64 product is not
    exactly zero, the number of slots where it is)"""
    cs = case.consts
    ho, co = cs["hist_off"].tolist(), cs["cand_off"].tolist()
    sc, s, hs = case.leaves["scores"].double(), cs["cand_score"].double(), cs["hist_score"].double()
    worst, zeros = float("inf"), 0
    for i in range(len(co) - 1):
        h = ho[i + 1] - ho[i]
        if h == 0:
            continue
        prod = hs[ho[i]:ho[i + 1]].sum() / h * s[co[i]:co[i + 1]] * sc[co[i]:co[i + 1]]
        bound = (h + 4) * U32 * hs[ho[i]:ho[i + 1]].abs().sum() / h * s[co[i]:co[i + 1]].abs() * sc[co[i]:co[i + 1]].abs()
        live = prod != 0
        zeros += int((~live).sum())
        if bool(live.any()):
            worst = min(worst, float((prod.abs() / bound)[live].min()))
    return worst, zeros


# ------------------------------------------------------------------------------------------------ the loss lines of the two model_steps
def tanr_loss_lines(scores: Tensor, hist: Tensor, cand: Tensor, weight: Tensor, bias: Tensor, hist_topic: Tensor, cand_topic: Tensor,
                    labels: Tensor, cand_off: Tensor, c_max: int, coef: float = TOPIC_COEF) -> Dict[str, Tensor]:
    """tanr_plm_module.py:168-177 on the ragged scores and news rows: CrossEntropyLoss(scores [B, Cmax], y_true) on the zero-padded
    rows + coef x the topic head's cross-entropy over cat(candidate rows, history rows), the reference's order."""
    head = head_ce(torch.cat((cand, hist)), weight, bias, torch.cat((cand_topic, hist_topic)))["loss"]
    return {"loss": cross_entropy_dense(scores, labels, cand_off, c_max) + coef * head}


def sentirec_loss_lines(scores: Tensor, hist: Tensor, cand: Tensor, weight: Tensor, bias: Tensor, hist_score: Tensor, cand_score: Tensor,
                        labels: Tensor, hist_off: Tensor, cand_off: Tensor, c_max: int, pred_coef: float = SENTI_PRED_COEF,
                        div_coef: float = SENTI_DIV_COEF) -> Dict[str, Tensor]:
    """sentirec_plm_module.py:170-193: the same CrossEntropyLoss + pred_coef x L1Loss of the sentiment head over cat(candidate rows,
    history rows) + div_coef x the diversity regulariser."""
    head = head_l1(torch.cat((cand, hist)), weight, bias, torch.cat((cand_score, hist_score)))["loss"]
    div = senti_div(scores, cand_score, hist_score, hist_off, cand_off, c_max)["loss"]
    return {"loss": cross_entropy_dense(scores, labels, cand_off, c_max) + pred_coef * head + div_coef * div}


STEP_HIST, STEP_CAND, STEP_TOPICS = (9, 5, 2), (6, 4, 1), 19    # B = 3


def step_consts(salt: int = 0):
    """labels, topics and sentiment scores of the B = 3 step batch (the news rows come from the encoder under test)"""
    rng = np.random.default_rng(4300 + salt)
    ho, co = offsets(STEP_HIST), offsets(STEP_CAND)
    nh, t = int(ho[-1]), int(co[-1])
    labels = torch.zeros(t)
    labels[co[:-1]] = 1.0
    sign_user = np.repeat(rng.choice([-1.0, 1.0], len(STEP_HIST)), STEP_HIST)
    cand_score = rng.uniform(0.2, 1.0, t) * rng.choice([-1.0, 1.0], t)
    cand_score[2] = 0.0
    return {"hist_off": ho, "cand_off": co, "labels": labels, "c_max": max(STEP_CAND),
            "hist_topic": torch.from_numpy(rng.integers(0, STEP_TOPICS, nh)), "cand_topic": torch.from_numpy(rng.integers(0, STEP_TOPICS, t)),
            "hist_score": torch.from_numpy((rng.uniform(0.2, 1.0, nh) * sign_user).astype(np.float32)),
            "cand_score": torch.from_numpy(cand_score.astype(np.float32))}


def all_measured_cases():
    cases = [ce_case(*s) for s in HEAD_SHAPES] + [l1_case(n, d) for n, d, _ in HEAD_SHAPES]
    return cases + [senti_case(b, p) for b in SENTI_B for p in (False, True)]
