"""Float64 restatement of the CAUM baseline's user encoder — CAUMUserEncoder.forward with its DenseAttention (reference
manner/models/components/user_encoder.py:121-178, attention.py:119-141) — written from its definition in plain torch, dtype-generic,
with autograd for the gradients, in the SPLIT form the kernels compute: the weights of the concatenated operands are split by column
range instead of concatenating the operands (tests/test_caum_host.py holds it to the reference's own class through the golden).
No GPU in this file: tests/test_caum_host.py checks the restatement and the planted defects on the CPU, tests/test_gpu_caum.py runs
the kernels against it.

The bars are those of tests/side_ops_ref.py, used as they are.  Every output here has exp / tanh inside: the MEASURED bar — 8 x the
error of this restatement in float32 on the CPU, relative to the tensor's largest entry, inputs drawn at the first ``settled`` salt.
Two gradients are zero in exact arithmetic (both softmaxes are shift-invariant): the K third of d in_proj_bias and
d dense_att.linear3.bias.  They cannot be held relative to themselves; ``zero_gradient_bounds`` gives their absolute bound
(n + 4) 2^-24 sum |terms| with the terms taken from this restatement (an exact zero passes)."""
from __future__ import annotations

import functools
from typing import Dict, Optional

import numpy as np
import torch

from side_ops_ref import U32, Case, mha_axis0, randn, settled

Tensor = torch.Tensor

PARAMS = ("w1", "b1", "w2", "b2", "in_w", "in_b", "out_w", "out_b", "w3", "b3", "wa", "ba", "wb", "bb", "wc", "bc")
#: the state-dict key of each restatement argument (CAUMUserEncoder)
STATE_KEYS = dict(zip(PARAMS, ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "multihead_attention.in_proj_weight",
                               "multihead_attention.in_proj_bias", "multihead_attention.out_proj.weight", "multihead_attention.out_proj.bias",
                               "linear3.weight", "linear3.bias", "dense_att.linear.weight", "dense_att.linear.bias", "dense_att.linear2.weight",
                               "dense_att.linear2.bias", "dense_att.linear3.weight", "dense_att.linear3.bias")))


def caum_user(x: Tensor, c: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, in_w: Tensor, in_b: Tensor, out_w: Tensor, out_b: Tensor,
              w3: Tensor, b3: Tensor, wa: Tensor, ba: Tensor, wb: Tensor, bb: Tensor, wc: Tensor, bc: Tensor, heads: int, p: float = 0.0,
              keep1: Optional[Tensor] = None, keep2: Optional[Tensor] = None, keep3: Optional[Tensor] = None, *, swap_shift: bool = False,
              attend_along_s: bool = False, key_limit: Optional[int] = None, candidate_term: bool = True, slot_limit: Optional[int] = None,
              scale_dh: Optional[int] = None, raw_candidate_in_dot: bool = False, probe: Optional[dict] = None) -> Dict[str, Tensor]:
    """x [B, S, D] clicked news, c [B, D] one candidate per user -> out [B].  ``keep1`` [B, D], ``keep2`` [B, S, D], ``keep3``
    [B, S, F + U]: the keep-masks of dropout1 / 2 / 3 at probability ``p`` (None: no dropout).
      cnn  = W1 . [xd[s-1], xd[s], xd[s+1], cd] + b1 (circular shift), h2 = W2 . [cd, xd[s]] + b2,
      self = MultiheadAttention(batch_first=False) on h2 [B, S, U]: attention ALONG B at each slot,
      all  = W3 . dropout3(cat[cnn, self]) + b3,
      score = wc . tanh(Wb tanh(Wa[:, :U] all + Wa[:, U:] cd + ba) + bb) + bc, softmax over ALL S slots,
      out  = cd . sum_s p[s] all[s].
    The keyword-only arguments plant defects for tests/test_caum_host.py: ``swap_shift`` (left and right neighbour exchanged),
    ``attend_along_s`` (attention along the history instead of along the batch), ``key_limit`` (keys >= the limit dropped),
    ``candidate_term`` False (the candidate half of the dense attention's first Linear left out), ``slot_limit`` (history slots >= the
    limit left out of the softmax and the weighted sum), ``scale_dh`` (the 1 / sqrt of another head width), ``raw_candidate_in_dot`` (c for
    the dropped-out candidate in the final dot).  ``probe``: a dict that receives the intermediates ``score`` and ``k`` (the key rows)."""
    d = x.shape[2]
    u = w2.shape[0]
    scale = 1.0 / (1.0 - p) if p > 0.0 else 1.0
    cd = c if keep1 is None else c * keep1.to(c.dtype) * scale
    xd = x if keep2 is None else x * keep2.to(x.dtype) * scale
    left, right = torch.roll(xd, 1, dims=1), torch.roll(xd, -1, dims=1)
    if swap_shift:
        left, right = right, left
    cnn = left @ w1[:, :d].T + xd @ w1[:, d:2 * d].T + right @ w1[:, 2 * d:3 * d].T + (cd @ w1[:, 3 * d:].T)[:, None, :] + b1
    h2 = (cd @ w2[:, :d].T)[:, None, :] + xd @ w2[:, d:].T + b2
    if probe is not None:
        k_rows = h2 @ in_w[u:2 * u].T + in_b[u:2 * u]
        if k_rows.requires_grad:
            k_rows.retain_grad()
        probe["k"] = k_rows
        in_parts = (h2 @ in_w[:u].T + in_b[:u], k_rows, h2 @ in_w[2 * u:].T + in_b[2 * u:])
        self_att = _attention_core(in_parts, out_w, out_b, heads)
    elif attend_along_s:
        self_att = mha_axis0(h2.transpose(0, 1), in_w, in_b, out_w, out_b, heads, key_limit, scale_dh)["out"].transpose(0, 1)
    else:
        self_att = mha_axis0(h2, in_w, in_b, out_w, out_b, heads, key_limit, scale_dh)["out"]
    cat = torch.cat([cnn, self_att], dim=-1)
    if keep3 is not None:
        cat = cat * keep3.to(cat.dtype) * scale
    allv = cat @ w3.T + b3
    pre = allv @ wa[:, :u].T + ba
    if candidate_term:
        pre = pre + (cd @ wa[:, u:].T)[:, None, :]
    t2 = torch.tanh(torch.tanh(pre) @ wb.T + bb)
    score = (t2 @ wc.T).squeeze(-1) + bc
    if probe is not None:
        if score.requires_grad:
            score.retain_grad()
        probe["score"] = score
    if slot_limit is not None:
        score, allv = score[:, :slot_limit], allv[:, :slot_limit]
    user = (torch.softmax(score, dim=-1)[:, :, None] * allv).sum(dim=1)
    return {"out": ((c if raw_candidate_in_dot else cd) * user).sum(dim=-1)}


def _attention_core(qkv, out_w, out_b, heads):
    """side_ops_ref.mha_axis0 after the in-projection, on separate q / k / v rows (so that the key rows can keep their gradient)"""
    q, k, v = qkv
    l0, b1, e = q.shape
    dh = e // heads

    def split_heads(t):
        return t.reshape(l0, b1 * heads, dh).transpose(0, 1)

    att = torch.softmax((split_heads(q) * float(dh) ** -0.5) @ split_heads(k).transpose(1, 2), dim=-1)
    return (att @ split_heads(v)).transpose(0, 1).reshape(l0, b1, e) @ out_w.T + out_b


def reference_form(x, c, heads, **w):
    """The CONCATENATED form, line by line as user_encoder.py:121-178 at dropout 0 (the host test holds the split form to it)"""
    rep = c[:, None, :].repeat(1, x.shape[1], 1)
    left = torch.cat([x[:, -1:, :], x[:, :-1, :]], dim=-2)
    right = torch.cat([x[:, 1:, :], x[:, :1, :]], dim=-2)
    cnn = torch.cat([left, x, right, rep], dim=-1) @ w["w1"].T + w["b1"]
    h2 = torch.cat([rep, x], dim=-1) @ w["w2"].T + w["b2"]
    self_att = mha_axis0(h2, w["in_w"], w["in_b"], w["out_w"], w["out_b"], heads)["out"]
    allv = torch.cat([cnn, self_att], dim=-1) @ w["w3"].T + w["b3"]
    att = torch.cat([allv, rep], dim=-1)
    score = (torch.tanh(torch.tanh(att @ w["wa"].T + w["ba"]) @ w["wb"].T + w["bb"]) @ w["wc"].T + w["bc"]).squeeze(-1)
    user = torch.bmm(torch.softmax(score, dim=-1)[:, None, :], allv).squeeze(1)
    return {"out": torch.bmm(c[:, None, :], user[:, :, None]).flatten()}


def param_shapes(d, f, u, h1, h2):
    return {"w1": (f, 4 * d), "b1": (f,), "w2": (u, 2 * d), "b2": (u,), "in_w": (3 * u, u), "in_b": (3 * u,), "out_w": (u, u), "out_b": (u,),
            "w3": (u, f + u), "b3": (u,), "wa": (h1, 2 * u), "ba": (h1,), "wb": (h2, h1), "bb": (h2,), "wc": (1, h2), "bc": (1,)}


def caum_inputs(b, s, d, f, h1, h2, heads, salt=0, pad_slots=0):
    """Leaves at scales that keep every tanh and both softmaxes in their curved range; ``pad_slots``: the last slots of user 1.. are
    zero rows (to_dense_batch)."""
    u = d
    sd = 3000 + 5 * s + d + f + h1 + salt
    leaves = {"x": randn(sd, b, s, d), "c": randn(sd + 1, b, d)}
    for i, (name, shape) in enumerate(param_shapes(d, f, u, h1, h2).items()):
        scale = 0.1 if len(shape) == 1 else 2.0 * shape[1] ** -0.5 if name in ("wc", "wb") else shape[1] ** -0.5
        leaves[name] = randn(sd + 2 + i, *shape, scale=scale)
    if pad_slots:
        leaves["x"][1:, s - pad_slots:] = 0.0
    return leaves, {"heads": heads}, {"out": randn(sd + 30, b)}


GOLDEN_SHAPE = (3, 7, 20, 24, 12, 8, 4)
#: (B, S, D = U, F, H1, H2, heads).  The golden shape; the shipped sizes (head dim 25); odd widths with head dim 25; S = 1 (left = right =
#: self) and S = 2 (left = right); B = 1; S = 9 and 17, past one and two 8-row tiles; B = 65 and 257, past the rows of one workgroup's
#: several pairs and past the 256-row block with 64-key tiles; width 1024 (32 128-feature steps of linear1's input, three 1024-feature chunks of the
#: in-projection's gradient); S = 256 at width 8; and B = 365: 1095 rows, past the 16 row groups of the weight gradients (1088 rows)
USER_SHAPES = (GOLDEN_SHAPE, (8, 50, 400, 400, 400, 256, 16), (9, 5, 50, 12, 10, 6, 2), (3, 1, 20, 24, 12, 8, 4), (3, 2, 20, 24, 12, 8, 4),
               (1, 7, 20, 24, 12, 8, 4), (3, 9, 20, 24, 12, 8, 4), (3, 17, 20, 24, 12, 8, 4), (65, 3, 10, 6, 6, 4, 2), (257, 3, 10, 6, 6, 4, 2),
               (2, 3, 1024, 260, 1024, 260, 16), (2, 256, 8, 8, 8, 8, 2), (365, 3, 10, 6, 6, 4, 2))
#: the shapes the planted defects are shown at: the golden's, the odd widths, the shipped sizes
DEFECT_SHAPES = (GOLDEN_SHAPE, (9, 5, 50, 12, 10, 6, 2), (8, 50, 400, 400, 400, 256, 16))


@functools.lru_cache(maxsize=None)
def user_case(b, s, d, f, h1, h2, heads, pad_slots=0) -> Case:
    def build(salt):
        leaves, consts, up = caum_inputs(b, s, d, f, h1, h2, heads, salt, pad_slots)
        return Case(f"caum-B{b}-S{s}-D{d}-F{f}-H{h1}-{h2}-h{heads}" + (f"-pad{pad_slots}" if pad_slots else ""), caum_user, leaves, consts, up)
    return settled(build)


def zero_gradient_bounds(case: Case) -> Dict[str, np.ndarray]:
    """The absolute bounds (n + 4) 2^-24 sum |terms| of the two analytically-zero gradients of ``case`` (float64, from the restatement):
    ``d_bc`` = sum_r d score[r] (n = B S) and ``d_in_b_k`` [U] = sum_r d k[r, :] (n = B S)."""
    lv = {k: v.detach().double().requires_grad_(True) for k, v in case.leaves.items()}
    probe: dict = {}
    out = caum_user(**lv, **case.consts, probe=probe)["out"]
    (out * case.upstream["out"].double()).sum().backward()
    n = float(probe["score"].numel())
    return {"d_bc": np.array([(n + 4.0) * U32 * float(probe["score"].grad.abs().sum())]),
            "d_in_b_k": (n + 4.0) * U32 * probe["k"].grad.abs().sum(dim=(0, 1)).numpy()}


# ------------------------------------------------------------------------------------------------ CAUMPLMModule.forward, restated
def caum_module_forward(hist: Tensor, cand: Tensor, heads: int, **w: Tensor) -> Dict[str, Tensor]:
    """The operator lines of CAUMPLMModule.forward (baselines/caum_plm_module.py:155-165) on dense inputs: hist [B, S, D],
    cand [B, C, D] -> scores [B, C], one user-encoder call per candidate column on the cand[:, i, :] view"""
    rows = [caum_user(hist, cand[:, i, :], heads=heads, **w)["out"] for i in range(cand.shape[1])]          # scores[i, :] = cand_score
    return {"scores": torch.stack(rows, dim=0).transpose(1, 0)}


MODULE_SHAPE = (3, 7, 20, 24, 12, 8, 4, 5)                     # B, S, D, F, H1, H2, heads, C


@functools.lru_cache(maxsize=None)
def module_case() -> Case:
    b, s, d, f, h1, h2, heads, c = MODULE_SHAPE

    def build(salt):
        leaves, consts, _ = caum_inputs(b, s, d, f, h1, h2, heads, salt + 11, pad_slots=1)
        cand = randn(3100 + salt, b, c, d)
        cand[1, c - 1] = 0.0                                   # a zero-padded candidate row (to_dense_batch)
        leaves = dict({k: v for k, v in leaves.items() if k not in ("x", "c")}, hist=leaves["x"], cand=cand)
        return Case("caum-module", caum_module_forward, leaves, consts, {"scores": randn(3101 + salt, b, c)})
    return settled(build)


# ------------------------------------------------------------------------------------------------ mha_axis0_any alone
ANY_DH = (1, 5, 12, 25, 48, 64)        # 12: the 16-wide register width, which none of the other head dims takes
ANY_L0 = (1, 33, 65, 257)
#: (L0, B1, E, heads) beyond the grid ANY_DH x ANY_L0: 129 rows of head dim 64 are more than one workgroup's LDS holds (8256 > 7168
#: floats) at L0 <= 256 — the tiled path below the 256-row block
ANY_EXTRA = ((129, 3, 128, 2),)


def any_cases():
    from side_ops_ref import axis0_case
    return [axis0_case(l0, 3, 2 * dh, 2) for dh in ANY_DH for l0 in ANY_L0] + [axis0_case(*s) for s in ANY_EXTRA]


# ------------------------------------------------------------------------------------------------ linear + tanh alone
def linear_tanh(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Dict[str, Tensor]:
    y = x @ weight.T
    return {"y": torch.tanh(y if bias is None else y + bias)}


#: (R, K, O): the smallest, and rows past two 8-row tiles with K past eight 128-feature steps (the last one partial) and O past four
#: 64-feature tiles (the last one partial)
LINEAR_TANH_SHAPES = ((1, 4, 1), (17, 1030, 300))


@functools.lru_cache(maxsize=None)
def linear_tanh_case(r: int, k: int, o: int, with_bias: bool) -> Case:
    def build(salt):
        s = 3200 + r + k + o + salt
        leaves = {"x": randn(s, r, k), "weight": randn(s + 1, o, k, scale=k ** -0.5)}
        if with_bias:
            leaves["bias"] = randn(s + 2, o, scale=0.5)
        return Case(f"linear_tanh-R{r}-K{k}-O{o}-{'bias' if with_bias else 'nobias'}", linear_tanh, leaves, {}, {"y": randn(s + 3, r, o)})
    return settled(build)
