"""Float64 restatements of the MINER baseline's operators — PolyAttention, TargetAwareAttention (reference
manner/models/components/attention.py:60-84, 102-116) and DotProduct as MINERModule.forward calls it (baselines/miner_module.py:
195-198) — written from their definitions in plain torch, dtype-generic, with autograd for the gradients; the shapes the kernels
are run at and the planted defects that show the bars see every loop and quirk.  No GPU in this file: tests/test_miner_host.py
checks the restatements on the CPU, tests/test_gpu_miner.py runs the kernels against them.

The two bars are those of tests/side_ops_ref.py, used as they are: the DERIVED bar (n + 4) 2^-24 sum|a b| for the pure sums of
products (the batched dot product and its gradients), the MEASURED bar — 8 x the error of the same restatement in float32 on the
CPU, relative to the tensor's largest entry, inputs drawn at the first ``settled`` salt — for everything with tanh / exp / erf."""
from __future__ import annotations

import functools
from typing import Dict, Optional

import numpy as np
import torch

from side_ops_ref import Case, randn, settled

Tensor = torch.Tensor


# ------------------------------------------------------------------------------------------------ PolyAttention
def poly_attention(x: Tensor, lin_w: Tensor, codes: Tensor, mask: Tensor, bias: Optional[Tensor] = None, *, masked_logit: float = 1e-30,
                   bias_count: Optional[Tensor] = None, slot_limit: Optional[int] = None, code_limit: Optional[int] = None,
                   tanh_grad: bool = True, projection_route: bool = True) -> Dict[str, Tensor]:
    """x [B, S, D], lin_w [Q, D], codes [K, Q], mask bool [B, S], bias [B, S, T] or None -> out [B, K, D]:
    logit[b, k, s] = tanh(x W^T)[b, s, :] . codes[k, :] + mean_t bias[b, s, t]; a masked slot's logit is REPLACED by 1e-30 (it stays
    in the softmax); softmax over s; out = sum_s p x.  The mean runs over all T columns.
    The keyword arguments plant defects for tests/test_miner_host.py: ``masked_logit`` (-inf: the usual masking), ``bias_count``
    ([B]: the bias sum divided by a per-user count), ``slot_limit`` / ``code_limit`` (history slots / context codes >= the limit
    dropped), ``tanh_grad`` False (the tanh derivative left out of the backward), ``projection_route`` False (no gradient into x
    through the projection)."""
    pre = (x if projection_route else x.detach()) @ lin_w.T
    proj = torch.tanh(pre) if tanh_grad else pre + (torch.tanh(pre) - pre).detach()
    logits = proj @ codes.T                                                        # [B, S, K]
    if bias is not None:
        b = bias.to(x.dtype)
        mean = b.mean(dim=2) if bias_count is None else b.sum(dim=2) / bias_count.to(x.dtype)[:, None]
        logits = logits + mean[:, :, None]
    logits = logits.permute(0, 2, 1)                                               # [B, K, S]
    logits = torch.where(mask[:, None, :], logits, torch.full_like(logits, masked_logit))
    xs = x
    if slot_limit is not None:
        logits, xs = logits[:, :, :slot_limit], x[:, :slot_limit]
    out = torch.softmax(logits, dim=2) @ xs
    if code_limit is not None:
        out = torch.cat([out[:, :code_limit], torch.zeros_like(out[:, code_limit:])], dim=1)
    return {"out": out}


def ragged_mask(b: int, s: int, empty_user: Optional[int] = None) -> Tensor:
    """User 0 keeps every slot, the others lose more and more of the tail (at least one slot stays); ``empty_user``: all false."""
    mask = torch.zeros(b, s, dtype=torch.bool)
    for i in range(b):
        mask[i, :max(1, s - (i * s) // max(b, 2))] = True
    if empty_user is not None:
        mask[empty_user] = False
    return mask


def poly_inputs(b, s, d, q, k, t, salt=0, empty_user=None):
    sd = 2000 + 3 * s + d + q + k + salt
    leaves = {"x": randn(sd, b, s, d), "lin_w": randn(sd + 1, q, d, scale=d ** -0.5), "codes": randn(sd + 2, k, q, scale=2.0 * q ** -0.5)}
    consts = {"mask": ragged_mask(b, s, empty_user)}
    if t:
        bias = randn(sd + 3, b, s, t, scale=0.5)
        own = max(1, t // (b + 1))
        for i in range(b):                                     # the caller zeroes the columns of the user's own candidates
            bias[i, :, (i * own) % t:(i * own) % t + own] = 0.0
        consts["bias"] = bias
    return leaves, consts, {"out": randn(sd + 4, b, k, d)}


POLY_GOLDEN = (3, 7, 64, 24, 5)
#: (B, S, D, Q, K, T): T = 0 is "no bias".  The golden shape with and without bias, the shipped config, S past one 64-slot trip with
#: K past two 16-code workgroups, the smallest shape, odd widths with several trips of every loop and a bias, a batch whose
#: reductions of d codes / d W go past one row group, and S at its bound.
POLY_SHAPES = ((3, 7, 64, 24, 5, 0), (3, 7, 64, 24, 5, 11), (2, 50, 256, 200, 32, 0), (2, 65, 768, 200, 33, 0), (1, 1, 4, 1, 1, 0),
               (5, 130, 100, 130, 64, 13), (300, 9, 64, 24, 5, 0), (1, 256, 8, 4, 2, 0))


@functools.lru_cache(maxsize=None)
def poly_case(b, s, d, q, k, t, empty_user=None) -> Case:
    def build(salt):
        leaves, consts, up = poly_inputs(b, s, d, q, k, t, salt, empty_user)
        return Case(f"poly-B{b}-S{s}-D{d}-Q{q}-K{k}-T{t}" + ("" if empty_user is None else f"-empty{empty_user}"), poly_attention, leaves, consts, up)
    return settled(build)


# ------------------------------------------------------------------------------------------------ TargetAwareAttention
def target_attention(query: Tensor, key: Tensor, value: Tensor, lin_w: Tensor, *, softmax_dim: int = 2) -> Dict[str, Tensor]:
    """query [B, K, D], key [B, C, D], value [B, C, K], lin_w [D, D] -> out [B, C] = sum_k softmax_k(key . gelu(query W^T)^T) value
    (erf GELU).  ``softmax_dim`` = 1 plants the softmax over the candidates."""
    pre = query @ lin_w.T
    proj = 0.5 * pre * (1.0 + torch.erf(pre * 2.0 ** -0.5))
    weights = torch.softmax(key @ proj.permute(0, 2, 1), dim=softmax_dim)          # [B, C, K]
    return {"out": (weights * value).sum(dim=2)}


#: (B, K, C, D, zero-padded candidate rows): the golden shape, K = 32 with candidates past sixteen 8-row tiles, one candidate,
#: K past half a wave with an odd width, and a batch whose last rows are to_dense_batch's zero padding
TARGET_SHAPES = ((3, 5, 6, 64, 0), (2, 32, 130, 256, 0), (2, 5, 1, 64, 0), (2, 33, 9, 100, 0), (3, 5, 6, 64, 2))


@functools.lru_cache(maxsize=None)
def target_case(b, k, c, d, padded) -> Case:
    def build(salt):
        sd = 2100 + k + c + d + padded + salt
        key, value = randn(sd + 1, b, c, d, scale=2.0 * d ** -0.5), randn(sd + 2, b, c, k)
        for i in range(1, b):                                  # users 1.. end in `padded` all-zero candidate rows
            if padded:
                key[i, c - padded:], value[i, c - padded:] = 0.0, 0.0
        leaves = {"query": randn(sd, b, k, d), "key": key, "value": value, "lin_w": randn(sd + 3, d, d, scale=d ** -0.5)}
        return Case(f"target-B{b}-K{k}-C{c}-D{d}-pad{padded}", target_attention, leaves, {}, {"out": randn(sd + 4, b, c)})
    return settled(build)


# ------------------------------------------------------------------------------------------------ batched dot product
def bmm_rows(a: Tensor, rows: Tensor) -> Dict[str, Tensor]:
    """DotProduct on a [B, M, D] and the permuted view of rows [B, N, D]: bmm(a, rows^T).squeeze(1) -> [B, M, N] ([B, N] at M = 1)"""
    return {"out": torch.bmm(a, rows.permute(0, 2, 1)).squeeze(dim=1)}


def bmm_terms(a, rows, g, absolute=False, dtype=np.float64):
    f = np.abs if absolute else (lambda v: v)
    a, rows, g = (f(np.asarray(v, dtype)) for v in (a, rows, g))
    _, m, d = a.shape
    n = rows.shape[1]
    return {"out": (np.einsum("bmd,bnd->bmn", a, rows), d), "d_a": (np.einsum("bmn,bnd->bmd", g, rows), n),
            "d_rows": (np.einsum("bmd,bmn->bnd", a, g), m)}


BMM_SHAPES = ((4, 37, 256, 32), (2, 37, 1024, 32))            # (B, M, D, N): MINER's [B, C, D] x [B, D, K]


@functools.lru_cache(maxsize=None)
def bmm_case(b, m, d, n) -> Case:
    sd = 2200 + m + d + n
    a, rows, g = randn(sd, b, m, d), randn(sd + 1, b, n, d), randn(sd + 2, b, m, n)
    return Case(f"bmm-B{b}-M{m}-D{d}-N{n}", bmm_rows, {"a": a, "rows": rows}, {}, {"out": g},
                functools.partial(bmm_terms, a.numpy(), rows.numpy(), g.numpy()))


# ------------------------------------------------------------------------------------------------ MINERModule.forward, restated
SCORE_TYPES = ("max", "mean", "weighted")


def miner_forward(hist: Tensor, cand: Tensor, poly_w: Tensor, codes: Tensor, target_w: Tensor, mask: Tensor, bias: Optional[Tensor],
                  score_type: str) -> Dict[str, Tensor]:
    """The operator lines of MINERModule.forward (baselines/miner_module.py:183-212) on dense inputs: hist [B, S, D], cand [B, C, D]"""
    user = poly_attention(hist, poly_w, codes, mask, bias)["out"]
    scores = bmm_rows(cand, user)["out"]
    if score_type == "max":
        scores = scores.max(dim=2)[0]
    elif score_type == "mean":
        scores = scores.mean(dim=2)
    else:
        scores = target_attention(user, cand, scores, target_w)["out"]
    return {"user": user, "scores": scores}


MINER_SHAPE = (3, 9, 64, 24, 5, 6, 11)                         # B, S, D, Q, K, C, T


@functools.lru_cache(maxsize=None)
def miner_case(score_type: str) -> Case:
    b, s, d, q, k, c, t = MINER_SHAPE

    def build(salt):
        leaves, consts, _ = poly_inputs(b, s, d, q, k, t, salt + 7)
        sd = 2300 + salt
        leaves = {"hist": leaves["x"], "cand": randn(sd, b, c, d, scale=2.0 * d ** -0.5), "poly_w": leaves["lin_w"], "codes": leaves["codes"],
                  "target_w": randn(sd + 1, d, d, scale=d ** -0.5)}
        up = {"scores": randn(sd + 2, b, c), "user": randn(sd + 3, b, k, d, scale=0.1)}
        return Case(f"miner-{score_type}", miner_forward, leaves, dict(consts, score_type=score_type), up)
    return settled(build)


def all_measured_cases():
    return ([poly_case(*s) for s in POLY_SHAPES] + [poly_case(2, 9, 64, 24, 5, 0, empty_user=0)] + [target_case(*s) for s in TARGET_SHAPES]
            + [miner_case(t) for t in SCORE_TYPES])
