"""Float64 restatement of the MINS baseline's user encoder — MINSUserEncoder.forward (reference
manner/models/components/user_encoder.py:211-243): ``nn.MultiheadAttention(D, heads=C, batch_first=False)`` on [B, S, D] (attention
ALONG AXIS 0, across the users of the call, unmasked), ``torch.chunk`` into C channels, every channel through ONE ``nn.GRU`` on
``pack_padded_sequence(hist_size, enforce_sorted=False)``, ``last_hidden`` concatenated, ``AdditiveAttention`` over that one slot — and of
the channel GRU alone and the NAML news side (news_encoder.py:174-236), written from their definitions in plain torch on
lstur_ref.gru_last_hidden and side_ops_ref.mha_axis0, dtype-generic, with autograd for the gradients.  No GPU in this file:
tests/test_mins_host.py checks the restatement and the planted defects on the CPU, tests/test_gpu_mins.py runs the kernels
(csrc/mins.hip) against it.

The bar is the MEASURED bar of tests/side_ops_ref.py, used as it is: 8 x the error of this restatement in float32 on the CPU, relative
to the tensor's largest entry, inputs drawn at the first ``settled`` salt.  Tensors the reference makes exactly zero (the pooler's three
gradients, the GRU's d x past a length) have a float32 figure of exactly zero, so their bar is zero: they are held to ``not t.any()``."""
from __future__ import annotations

import functools
from typing import Dict

import torch
import torch.nn.functional as F

import manner_oracle as O
from lstur_ref import gru_last_hidden, gru_leaves, lengths_of
from side_ops_ref import Case, axis0_case, mha_axis0, randn, settled

Tensor = torch.Tensor

GRU_PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh")
MHA_PARAMS = ("in_w", "in_b", "out_w", "out_b")
POOL_PARAMS = ("pool_w", "pool_b", "query")
#: the state-dict key of each restatement argument (MINSUserEncoder); ``multi_channel_gru.{c}.*`` alias the four ``gru.*`` tensors
STATE_KEYS = {"in_w": "multihead_attention.in_proj_weight", "in_b": "multihead_attention.in_proj_bias",
              "out_w": "multihead_attention.out_proj.weight", "out_b": "multihead_attention.out_proj.bias", "w_ih": "gru.weight_ih_l0",
              "w_hh": "gru.weight_hh_l0", "b_ih": "gru.bias_ih_l0", "b_hh": "gru.bias_hh_l0", "pool_w": "additive_attention.linear.weight",
              "pool_b": "additive_attention.linear.bias", "query": "additive_attention.query"}


def channel_gru(x: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, *, lengths: Tensor, channels: int, interleaved: bool = False,
                reverse_cat: bool = False, last_at_s: bool = False, shift_lengths: bool = False) -> Dict[str, Tensor]:
    """x [B, S, C I] -> out [B, C H]: channel c = the columns [c I, (c + 1) I) (``torch.chunk``), every channel through the same GRU
    tensors, row b after its own lengths[b] steps, the channels' states concatenated in order.  The keyword-only arguments after
    ``channels`` plant defects for tests/test_mins_host.py: ``interleaved`` (channel c = x[..., c::C]), ``reverse_cat`` (the outputs
    concatenated in reverse), ``last_at_s`` (every row takes all S steps), ``shift_lengths`` (the B C rows' lengths shifted by one row:
    channel 0 of user b runs to the length of user b - 1)."""
    c = int(channels)
    width = x.shape[2] // c
    row_len = lengths.repeat_interleave(c)
    if shift_lengths:
        row_len = torch.roll(row_len, 1)
    row_len = row_len.reshape(-1, c)
    outs = []
    for ch in range(c):
        xc = x[:, :, ch::c] if interleaved else x[:, :, ch * width:(ch + 1) * width]
        outs.append(gru_last_hidden(xc, w_ih, w_hh, b_ih, b_hh, None, lengths=row_len[:, ch], last_at_s=last_at_s)["out"])
    return {"out": torch.cat(outs[::-1] if reverse_cat else outs, dim=1)}


def mins_user(x: Tensor, in_w: Tensor, in_b: Tensor, out_w: Tensor, out_b: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor,
              pool_w: Tensor, pool_b: Tensor, query: Tensor, *, lengths: Tensor, channels: int, attention_axis1: bool = False,
              **defects) -> Dict[str, Tensor]:
    """x [B, S, D] -> ``out`` [B, D] and ``hidden`` [B, D], the concatenated states before the final pooler (``out`` equals it bit for
    bit: a softmax over one slot is 1).  ``attention_axis1`` plants the defect of attending along the history instead of across the
    users; ``defects`` are ``channel_gru``'s."""
    if attention_axis1:
        mixed = mha_axis0(x.transpose(0, 1), in_w, in_b, out_w, out_b, channels)["out"].transpose(0, 1)
    else:
        mixed = mha_axis0(x, in_w, in_b, out_w, out_b, channels)["out"]
    hidden = channel_gru(mixed, w_ih, w_hh, b_ih, b_hh, lengths=lengths, channels=channels, **defects)["out"]
    return {"out": O.additive_attention(hidden[:, None, :], pool_w, pool_b, query), "hidden": hidden}


def naml_category(table: Tensor, lin_w: Tensor, lin_b: Tensor, *, ids: Tensor) -> Dict[str, Tensor]:
    """NAMLCategoryEncoder: embedding (padding_idx = 0: row 0 receives no gradient) -> Linear -> ReLU"""
    return {"out": torch.relu(F.embedding(ids, table, padding_idx=0) @ lin_w.T + lin_b)}


def naml_news(text: Tensor, table: Tensor, lin_w: Tensor, lin_b: Tensor, pool_w: Tensor, pool_b: Tensor, query: Tensor, *, ids: Tensor) -> Dict[str, Tensor]:
    """NAMLNewsEncoder after its text encoder: the text vector [N, D] and the category vector stacked to [N, 2, D] and pooled"""
    categ = naml_category(table, lin_w, lin_b, ids=ids)["out"]
    return {"out": O.additive_attention(torch.stack([text, categ], dim=1), pool_w, pool_b, query)}


# ------------------------------------------------------------------------------------------------ shapes
ROW_TILE, REG_WIDTH = 8, 128            # sequences per workgroup and register width of the recurrence kernels (csrc/mins.hip CG_ROWS, CG_HP)
WAVE_ROWS, KEY_TILE = 4, 32             # own rows per workgroup and other-side rows per LDS tile of the wide attention (AW_WAVES, AW_KT)
#: (B, S, C, I, H, lengths).  The golden; the shipped width 128 (every register of the row holds a weight); 127 and 65 (registers
#: zero-padded past H); H = 1 and 5; C = 1; B = 1; 9 rows (one past the 8-row tile; the first tile spans users of different lengths);
#: S = 1; all lengths 1 and all lengths S; the bound S = 256; 3285 stacked rows at B = 365 (past one pass of the weight- and
#: bias-gradient groups); I != H (the projection's K against the recurrence's)
CGRU_SHAPES = ((4, 5, 3, 4, 4, "mixed"), (2, 3, 6, 128, 128, "mixed"), (2, 3, 2, 127, 127, "mixed"), (2, 3, 2, 65, 65, "mixed"),
               (3, 3, 3, 1, 1, "mixed"), (3, 3, 3, 5, 5, "mixed"), (3, 3, 1, 6, 6, "mixed"), (1, 4, 3, 6, 6, "mixed"), (3, 3, 3, 6, 6, "mixed"),
               (3, 1, 3, 6, 6, "mixed"), (3, 3, 3, 6, 6, "ones"), (3, 3, 3, 6, 6, "full"), (2, 256, 2, 4, 4, "mixed"), (365, 3, 3, 6, 6, "mixed"),
               (3, 4, 2, 150, 70, "mixed"))
#: the shape at which the single-launch entry is compared with ``gru_last_hidden`` per channel view
PER_CHANNEL_SHAPE = (4, 5, 3, 6, 6, "mixed")
#: (B, S, D, C): the golden (head dim 4: the ``_any`` attention); the second golden, head dim 66 (the wide attention); the shipped
#: D = 768, C = 6 (head dim and channel width 128); B = 9 at head dim 65, the boundary
USER_SHAPES = ((4, 5, 12, 3), (4, 5, 132, 2), (2, 3, 768, 6), (9, 3, 130, 2))
DEFECT_SHAPES = ((4, 5, 12, 3), (4, 5, 132, 2))
WIDE_DH, WIDE_L0 = (65, 96, 127, 128), (1, 2, 9, 65, 257)
POOL_Q = 8


def wide_shapes():
    """(L0, B1, heads, dh): one row, one past a wave set, past a key tile, past a 256-row block; at 257 rows B1 = heads = 1"""
    shapes = []
    for dh in WIDE_DH:
        for l0 in WIDE_L0:
            for b1, heads in (((1, 1),) if l0 == 257 else ((1, 1), (1, 3), (5, 1), (5, 3))):
                shapes.append((l0, b1, heads, dh))
    return tuple(shapes)


def wide_case(l0, b1, heads, dh) -> Case:
    return axis0_case(l0, b1, heads * dh, heads)


@functools.lru_cache(maxsize=None)
def cgru_case(b, s, c, i, h, kind) -> Case:
    def build(salt):
        leaves, sd = gru_leaves(b, s, i, h, False, salt + 31 * c, width=c * i)
        return Case(f"cgru-B{b}-S{s}-C{c}-I{i}-H{h}-{kind}", channel_gru, leaves, {"lengths": lengths_of(b, s, kind), "channels": c},
                    {"out": randn(sd + 6, b, c * h)})
    return settled(build)


def seeded_user_params(sd: int, d: int, c: int, q: int = POOL_Q) -> Dict[str, Tensor]:
    """the eleven MINSUserEncoder tensors by restatement name (``STATE_KEYS``), GRU weights at 2 / sqrt(fan-in): the gates'
    pre-activations reach the curved range of sigma and tanh.  tests/golden/make_golden_mins.py seeds the reference's class with them."""
    w = d // c
    return {"in_w": randn(sd + 1, 3 * d, d, scale=d ** -0.5), "in_b": randn(sd + 2, 3 * d, scale=0.1),
            "out_w": randn(sd + 3, d, d, scale=d ** -0.5), "out_b": randn(sd + 4, d, scale=0.1),
            "w_ih": randn(sd + 5, 3 * w, w, scale=2.0 * w ** -0.5), "w_hh": randn(sd + 6, 3 * w, w, scale=2.0 * w ** -0.5),
            "b_ih": randn(sd + 7, 3 * w, scale=0.3), "b_hh": randn(sd + 8, 3 * w, scale=0.3), "pool_w": randn(sd + 9, q, d, scale=d ** -0.5),
            "pool_b": randn(sd + 10, q, scale=0.1), "query": randn(sd + 11, q, scale=2.0 * q ** -0.5)}


def user_leaves(b, s, d, c, salt):
    sd = 5000 + 11 * s + d + 5 * c + b + salt
    return dict(seeded_user_params(sd, d, c), x=randn(sd, b, s, d)), sd


@functools.lru_cache(maxsize=None)
def user_case(b, s, d, c) -> Case:
    def build(salt):
        leaves, sd = user_leaves(b, s, d, c, salt)
        return Case(f"mins-B{b}-S{s}-D{d}-C{c}", mins_user, leaves, {"lengths": lengths_of(b, s, "mixed"), "channels": c}, {"out": randn(sd + 12, b, d)})
    return settled(build)
