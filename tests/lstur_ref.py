"""Float64 restatement of the LSTUR baseline's user encoder — LSTURUserEncoder.forward (reference
manner/models/components/user_encoder.py:70-89): ``nn.GRU`` on ``pack_padded_sequence(enforce_sorted=False)``, ``last_hidden``, the
user embedding and its ``nn.Dropout2d`` — written from its definition in plain torch, dtype-generic, with autograd for the gradients.
No GPU in this file: tests/test_lstur_host.py checks the restatement and the planted defects on the CPU, tests/test_gpu_lstur.py runs
the kernels (csrc/gru.hip) against it.

The recurrence, for t = 0 .. S - 1 and gate order r | z | n:
    r = sigma(W_ir x_t + b_ir + W_hr h + b_hr),  z = sigma(W_iz x_t + b_iz + W_hz h + b_hz),
    n = tanh(W_in x_t + b_in + r (W_hn h + b_hn)),  h <- (1 - z) n + z h   for the rows with t < len[b]; the others keep h.
Slots t >= len[b] are never read: the restatement replaces them by zeros before the projection, so their d x is exactly 0.

The bar is the MEASURED bar of tests/side_ops_ref.py, used as it is: 8 x the error of this restatement in float32 on the CPU, relative
to the tensor's largest entry, inputs drawn at the first ``settled`` salt.  The float32 evaluation runs the same S steps, so the bar
grows with the recurrence as the kernel's error does."""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import torch

from side_ops_ref import Case, randn, settled

Tensor = torch.Tensor

GRU_PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh")
#: the state-dict key of each restatement argument (LSTURUserEncoder)
STATE_KEYS = {"table": "long_term_user_embedding.weight", "w_ih": "gru.weight_ih_l0", "w_hh": "gru.weight_hh_l0", "b_ih": "gru.bias_ih_l0",
              "b_hh": "gru.bias_hh_l0"}


def gru_last_hidden(x: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, h0: Optional[Tensor] = None, *, lengths: Tensor,
                    channels: Optional[Tuple[int, int]] = None, gate_order: str = "rzn", reset_before_matmul: bool = False,
                    last_at_s: bool = False) -> Dict[str, Tensor]:
    """x [B, S, I] (``channels`` = (lo, hi): the view x[:, :, lo:hi] of a wider tensor), lengths int64 [B], h0 [B, H] or None ->
    out [B, H], row b after its own lengths[b] steps.  The keyword-only arguments after ``channels`` plant defects for
    tests/test_lstur_host.py: ``gate_order`` "zrn" (the first two thirds exchanged), ``reset_before_matmul`` (n from W_hn (r h) instead
    of r (W_hn h + b_hn)), ``last_at_s`` (every row takes all S steps)."""
    if channels is not None:
        x = x[:, :, channels[0]:channels[1]]
    b, s, _ = x.shape
    hd = w_hh.shape[1]
    live = torch.arange(s, device=x.device)[None, :] < lengths[:, None]                 # [B, S]
    if last_at_s:
        live = torch.ones_like(live)
    gi = torch.where(live[:, :, None], x, torch.zeros_like(x)) @ w_ih.T + b_ih
    h = x.new_zeros((b, hd)) if h0 is None else h0
    first, second = (0, 1) if gate_order == "rzn" else (1, 0)
    for t in range(s):
        gh = h @ w_hh.T + b_hh
        g = gi[:, t]
        r = torch.sigmoid(g[:, first * hd:(first + 1) * hd] + gh[:, first * hd:(first + 1) * hd])
        z = torch.sigmoid(g[:, second * hd:(second + 1) * hd] + gh[:, second * hd:(second + 1) * hd])
        hn = (r * h) @ w_hh[2 * hd:].T + b_hh[2 * hd:] if reset_before_matmul else r * gh[:, 2 * hd:]
        n = torch.tanh(g[:, 2 * hd:] + hn)
        h = torch.where(live[:, t, None], (1.0 - z) * n + z * h, h)
    return {"out": h}


def lstur_user(x: Tensor, table: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, *, user: Tensor, lengths: Tensor, method: str,
               p: float = 0.0, keep: Optional[Tensor] = None, **defects) -> Dict[str, Tensor]:
    """user int64 [B], x [B, S, I], table [num_users, E] (row 0 = padding_idx: it receives no gradient) -> ``ini``: [B, H], the GRU
    started from the user's row; ``con``: [B, 2 H] = cat(last hidden from zero, the user's row).  ``keep`` [B]: the keep-mask of
    nn.Dropout2d on [1, B, E] at probability ``p`` — one draw per USER.  A ``keep`` of shape [B, E] plants the per-element defect."""
    rows = table[user]
    rows = torch.where((user == 0)[:, None], rows.detach(), rows)
    if keep is not None:
        k = keep.to(rows.dtype)
        rows = rows * (k[:, None] if k.dim() == 1 else k) * (1.0 / (1.0 - p))
    if method == "ini":
        return gru_last_hidden(x, w_ih, w_hh, b_ih, b_hh, rows, lengths=lengths, **defects)
    return {"out": torch.cat([gru_last_hidden(x, w_ih, w_hh, b_ih, b_hh, None, lengths=lengths, **defects)["out"], rows], dim=1)}


# ------------------------------------------------------------------------------------------------ shapes
ROW_TILE, UNIT_SLICE = 8, 4              # batch rows and hidden units per workgroup of the step kernels (csrc/gru.hip GR_ROWS, GR_UNITS)
GOLDEN_SHAPE = (4, 5, 6, 6)
#: (B, S, I, H, lengths, h0).  The golden shape with and without an initial state; S = 1 (the only step writes the output); all lengths
#: 1 at S = 3 (every later step fully masked) and all lengths = S (nothing masked); B = 1; B = 9, one past the 8-row tile (a second
#: row tile with one row); H = 1 and H = 5, one past the four units of a workgroup; the bounds I = H = 1024 at B = 2, S = 2 (eight
#: full 128-feature steps of the projection, sixteen trips of a wave over K); S = 256 at width 4; B = 365 at S = 3: 1095
#: stacked rows, past the 16 x 64 rows one pass of the bias-gradient groups covers; I != H both ways (the projection's K against the
#: recurrence's)
GRU_SHAPES = ((4, 5, 6, 6, "mixed", True), (4, 5, 6, 6, "mixed", False), (3, 1, 6, 6, "mixed", True), (3, 3, 6, 6, "ones", True),
              (3, 3, 6, 6, "full", False), (1, 4, 6, 6, "mixed", True), (9, 3, 6, 6, "mixed", True), (3, 3, 6, 1, "mixed", True),
              (3, 3, 6, 5, "mixed", False), (2, 2, 1024, 1024, "mixed", True), (2, 256, 4, 4, "mixed", False), (365, 3, 6, 6, "mixed", True),
              (3, 4, 150, 70, "mixed", True), (3, 4, 1, 130, "mixed", False))
#: the MINS form: I = H = 8, the channels 8 .. 15 of a 24-wide tensor read in place, no initial state
STRIDED_SHAPE = (3, 4, 24, 8, (8, 16))
#: (B, S, I, method): the golden shape; the shipped widths (I = 868; H = 868 for ini, 434 for con: neither a multiple of 64, every
#: K loop ends in a partial trip) at B = 2, S = 3; and B = 9, past the row tile, where users repeat across tiles
USER_SHAPES = ((4, 5, 6, "ini"), (4, 5, 6, "con"), (2, 3, 868, "ini"), (2, 3, 868, "con"), (9, 3, 10, "ini"), (9, 3, 10, "con"))
DEFECT_SHAPES = ((4, 5, 6, "ini"), (4, 5, 6, "con"), (2, 3, 868, "ini"), (2, 3, 868, "con"))


def lengths_of(b: int, s: int, kind: str) -> Tensor:
    if kind == "ones":
        return torch.ones(b, dtype=torch.int64)
    if kind == "full":
        return torch.full((b,), s, dtype=torch.int64)
    lens = torch.tensor([1 + (7 * i + 3) % s for i in range(b)], dtype=torch.int64)
    lens[0] = s
    if b > 1:
        lens[-1] = 1
    return lens


def users_of(b: int) -> Tensor:
    """ids 1 .. B with the padding row at position 1 and a repeated user at positions 2, 3 (the golden's [1, 0, 3, 3]); the table has
    B + 3 rows, so the last two users are unused"""
    user = torch.arange(1, b + 1, dtype=torch.int64)
    if b > 1:
        user[1] = 0
    if b > 3:
        user[3] = user[2]
    return user


def gru_leaves(b, s, i, h, with_h0, salt, width=None):
    """weights at 2 / sqrt(fan-in): the gates' pre-activations reach the curved range of sigma and tanh"""
    sd = 4000 + 7 * s + i + 3 * h + b + salt
    leaves = {"x": randn(sd, b, s, width or i), "w_ih": randn(sd + 1, 3 * h, i, scale=2.0 * i ** -0.5),
              "w_hh": randn(sd + 2, 3 * h, h, scale=2.0 * h ** -0.5), "b_ih": randn(sd + 3, 3 * h, scale=0.3), "b_hh": randn(sd + 4, 3 * h, scale=0.3)}
    if with_h0:
        leaves["h0"] = randn(sd + 5, b, h, scale=0.7)
    return leaves, sd


@functools.lru_cache(maxsize=None)
def gru_case(b, s, i, h, kind, with_h0) -> Case:
    def build(salt):
        leaves, sd = gru_leaves(b, s, i, h, with_h0, salt)
        return Case(f"gru-B{b}-S{s}-I{i}-H{h}-{kind}-{'h0' if with_h0 else 'zero'}", gru_last_hidden, leaves, {"lengths": lengths_of(b, s, kind)},
                    {"out": randn(sd + 6, b, h)})
    return settled(build)


@functools.lru_cache(maxsize=None)
def strided_case() -> Case:
    b, s, width, h, channels = STRIDED_SHAPE

    def build(salt):
        leaves, sd = gru_leaves(b, s, h, h, False, salt, width=width)
        return Case("gru-strided", gru_last_hidden, leaves, {"lengths": lengths_of(b, s, "mixed"), "channels": channels}, {"out": randn(sd + 6, b, h)})
    return settled(build)


@functools.lru_cache(maxsize=None)
def user_case(b, s, i, method) -> Case:
    h = i if method == "ini" else i // 2

    def build(salt):
        leaves, sd = gru_leaves(b, s, i, h, False, salt + 17)
        table = randn(sd + 7, b + 3, h, scale=0.7)
        table[0] = 0.0                                           # padding_idx = 0
        leaves["table"] = table
        width = h if method == "ini" else 2 * h
        return Case(f"lstur-B{b}-S{s}-I{i}-{method}", lstur_user, leaves, {"user": users_of(b), "lengths": lengths_of(b, s, "mixed"), "method": method},
                    {"out": randn(sd + 8, b, width)})
    return settled(build)
