"""The SHARED-PRODUCT form of CAUMPLMModule.forward's candidate loop (reference baselines/caum_plm_module.py:155-165 over
CAUMUserEncoder.forward, user_encoder.py:121-178) — what ``manner_hip_caum_scores_all`` computes — written from its algebra in plain
torch, dtype-generic.  No GPU in this file: tests/test_caum_all_host.py holds it to ``caum_ref.caum_module_forward`` (the loop over the
columns) and shows the planted defects on the CPU, tests/test_gpu_caum_all.py runs the kernels.

In eval() no dropout sits between the operands, and every nn.Linear in front of a nonlinearity acts on a history-only operand plus a
candidate-only operand.  With b the user, s the history slot, c the candidate column, w3a = w3[:, :F], w3b = w3[:, F:]:
  cnn[b, c, s] = WX[b, s] + CX1[b, c]           WX = W1[:, :3D] window + b1,           CX1 = W1[:, 3D:] cand
  h2[b, c, s]  = HX[b, s] + CX2[b, c]           HX = W2[:, D:] x + b2,                 CX2 = W2[:, :D] cand
  qkv[b, c, s] = QH[b, s] + QC[b, c]            QH = in_w HX + in_b,                   QC  = in_w CX2
  all[b, c, s] = w3b out_w att[b, c, s] + A[b, s] + Bc[b, c]      A = w3a WX + w3b out_b + b3,   Bc = w3a CX1
  pre[b, c, s] = wa[:, :U] all[b, c, s] + CT[b, c]                CT = wa[:, U:] cand + ba
so three products run over the B C S rows (four with ``fold`` False: out_w, then w3b) and one attention across the B users per
(column, slot, head); everything else is taken once over B S rows or once over B C rows.

The references and the bars are those of tests/caum_ref.py and tests/side_ops_ref.py, used as they are: ``all_case`` is a
``side_ops_ref.Case`` whose function is ``caum_ref.caum_module_forward`` — the float64 loop is the reference, and the MEASURED bar is
8 x ITS float32 CPU error relative to the largest score."""
from __future__ import annotations

import functools
from typing import Dict, Optional

import torch

import caum_ref as CR
from side_ops_ref import Case, randn, settled

Tensor = torch.Tensor


def caum_scores_all(hist: Tensor, cand: Tensor, heads: int, *, fold: bool = True, candidate_in_keys: bool = True, own_column: bool = True,
                    transposed_rows: bool = False, out_bias_term: bool = True, candidate_tanh_term: bool = True,
                    slot_limit: Optional[int] = None, zero_partial_pass: Optional[int] = None, **w: Tensor) -> Dict[str, Tensor]:
    """hist [B, S, D], cand [B, C, D], the 16 leaves of ``caum_ref.PARAMS`` -> scores [B, C].  ``fold``: w3b out_w as one U x U matrix.
    The other keyword-only arguments plant defects for tests/test_caum_all_host.py: ``candidate_in_keys`` False (QC added to q and v
    but not to k), ``own_column`` False (every column attends with column 0's QC), ``transposed_rows`` (the (b, c) terms QC, Bc, CT
    read at row c B + b of their flattened [B C] rows where b C + c is meant), ``out_bias_term`` False (w3b out_b left out of A),
    ``candidate_tanh_term`` False (CT left out), ``slot_limit`` (slots >= the limit left out of the softmax over S and the weighted
    sum), ``zero_partial_pass`` = n (walking the columns n per pass, those of a last partial pass left at zero)."""
    b, s, d = hist.shape
    c = cand.shape[1]
    f, u = w["w1"].shape[0], w["w2"].shape[0]
    dh = u // heads
    w3a, w3b = w["w3"][:, :f], w["w3"][:, f:]
    # once over the B S rows
    window = torch.cat([torch.roll(hist, 1, dims=1), hist, torch.roll(hist, -1, dims=1)], dim=-1)
    wx = window @ w["w1"][:, :3 * d].T + w["b1"]
    hx = hist @ w["w2"][:, d:].T + w["b2"]
    qh = hx @ w["in_w"].T + w["in_b"]
    a = wx @ w3a.T + ((w3b @ w["out_b"] + w["b3"]) if out_bias_term else w["b3"])
    # once over the B C rows
    cx1 = cand @ w["w1"][:, 3 * d:].T
    cx2 = cand @ w["w2"][:, :d].T
    qc = cx2 @ w["in_w"].T
    bc_ = cx1 @ w3a.T
    ct = cand @ w["wa"][:, u:].T + w["ba"]
    if transposed_rows:
        qc, bc_, ct = (t.reshape(b * c, -1).reshape(c, b, -1).transpose(0, 1) for t in (qc, bc_, ct))
    qc_att = qc if own_column else qc[:, :1].expand_as(qc)
    # the attention across the B users at each (column, slot, head)
    qkv = qh[:, None, :, :] + qc_att[:, :, None, :]                                      # [B, C, S, 3U]
    q, k, v = qkv[..., :u], qkv[..., u:2 * u], qkv[..., 2 * u:]
    if not candidate_in_keys:
        k = qh[:, None, :, u:2 * u].expand_as(k)

    def split_heads(t):                                                                  # [B, C, S, U] -> [C, S, heads, B, dh]
        return t.reshape(b, c, s, heads, dh).permute(1, 2, 3, 0, 4)

    p = torch.softmax((split_heads(q) * float(dh) ** -0.5) @ split_heads(k).transpose(-1, -2), dim=-1)
    att = (p @ split_heads(v)).permute(3, 0, 1, 2, 4).reshape(b, c, s, u)
    # the three (four) products over the B C S rows
    mixed = att @ (w3b @ w["out_w"]).T if fold else (att @ w["out_w"].T) @ w3b.T
    allv = mixed + a[:, None, :, :] + bc_[:, :, None, :]
    pre = allv @ w["wa"][:, :u].T
    if candidate_tanh_term:
        pre = pre + ct[:, :, None, :]
    t2 = torch.tanh(torch.tanh(pre) @ w["wb"].T + w["bb"])
    score = (t2 @ w["wc"].T).squeeze(-1) + w["bc"]                                       # [B, C, S]
    if slot_limit is not None:
        score, allv = score[..., :slot_limit], allv[:, :, :slot_limit]
    user = (torch.softmax(score, dim=-1)[..., None] * allv).sum(dim=2)                   # [B, C, U]
    scores = (cand * user).sum(dim=-1)
    if zero_partial_pass is not None and c % zero_partial_pass:
        scores = torch.cat([scores[:, :c - c % zero_partial_pass], torch.zeros_like(scores[:, c - c % zero_partial_pass:])], dim=1)
    return {"scores": scores}


GOLDEN_WIDTHS = CR.GOLDEN_SHAPE[2:]                            # D = U, F, H1, H2, heads of tests/golden/caum.npz
#: (B, S, D = U, F, H1, H2, heads, C), the cases of tests/test_gpu_caum_all.py.  The row-tiled linear has two tiles — 32 rows x 32
#: output features for a launch of fewer than 1024 rows, 128 x 64 from 1024 rows on — so every launch over the B S, B C or B C S rows
#: of a case takes the one its row count selects; the score kernel takes 8 rows and the softmax kernel 4 pseudo-users (b, c) per workgroup:
#:   the module shape: B C S = 105 rows — three 32-row tiles and 9 rows, thirteen 8-row tiles and 1 row; B C = 15 pseudo-users, not a
#:     multiple of 4; every width below one 32-feature tile;
#:   the shipped widths at C = 3: 1200 wide rows, the 128-row tile (9 tiles and 48 rows), 400 history rows on the 32-row tile (12 and
#:     16 rows), widths of 12 and 8 steps of 32 input features and a last one of 16;
#:   odd widths at head dim 25 with B, S, C all different (180 rows on the 32-row tile: 5 tiles and 20 rows), and the same widths at
#:     C = 25: 1125 wide rows on the 128-row tile (8 tiles and 101 rows) with K = 50 (a last step of 18) and O = 50, 12, 10, 6 inside
#:     one 64-feature tile;
#:   C = 1, B = 1, S = 1 (the window folds onto itself) and S = 2 at the golden widths;
#:   B = 65 and 257: past the rows of one workgroup's several (column, slot, head) pairs and past the 256-row block of the attention;
#:   width 1024, the widest K and O of the linear (32 steps of 32 input features; F = H2 = 260: a last step of 4 and a last tile of
#:     4): 12 wide rows on the 32-row tile (32 tiles of 32 output features), and at S = 128, C = 4 exactly 1024 wide rows, the first
#:     row count of the 128-row tile (16 tiles of 64 output features);
#:   S = 256, the bound (1024 wide rows at width 8);
#:   C = 65 at widths of 10: the kernels tile no column axis (the columns are rows), so "one past the tile" is one past the 64 lanes of a
#:     wave, the only 64 in them; 585 rows.
SHAPES = ((3, 7, 20, 24, 12, 8, 4, 5), (8, 50, 400, 400, 400, 256, 16, 3), (9, 5, 50, 12, 10, 6, 2, 4), (9, 5, 50, 12, 10, 6, 2, 25),
          (3, 7) + GOLDEN_WIDTHS + (1,), (1, 7) + GOLDEN_WIDTHS + (5,), (3, 1) + GOLDEN_WIDTHS + (5,), (3, 2) + GOLDEN_WIDTHS + (5,),
          (65, 3, 10, 6, 6, 4, 2, 2), (257, 3, 10, 6, 6, 4, 2, 2), (2, 3, 1024, 260, 1024, 260, 16, 2), (2, 128, 1024, 260, 1024, 260, 16, 4),
          (2, 256, 8, 8, 8, 8, 2, 2), (3, 3, 10, 6, 6, 4, 2, 65))
#: the shapes the planted defects are shown at (B != C in each, C >= 3, S >= 5): the module's, the odd widths, the shipped widths
DEFECT_SHAPES = (SHAPES[0], SHAPES[2], SHAPES[1])


@functools.lru_cache(maxsize=None)
def all_case(b, s, d, f, h1, h2, heads, c) -> Case:
    """``caum_ref.module_case`` at any shape: the last history slot of the users 1.. and the last candidate row of user 1 are zero
    rows (to_dense_batch) wherever there is a user 1"""
    def build(salt):
        leaves, consts, _ = CR.caum_inputs(b, s, d, f, h1, h2, heads, salt + 17 + c, pad_slots=1 if b > 1 else 0)
        cand = randn(3300 + 7 * c + salt, b, c, d)
        if b > 1:
            cand[1, c - 1] = 0.0
        leaves = dict({k: v for k, v in leaves.items() if k not in ("x", "c")}, hist=leaves["x"], cand=cand)
        return Case(f"caum-all-B{b}-S{s}-D{d}-F{f}-H{h1}-{h2}-h{heads}-C{c}", CR.caum_module_forward, leaves, consts, None)
    return settled(build)
