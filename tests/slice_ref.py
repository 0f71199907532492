"""Float64 reference of the encoder and per-slice error maps for the 16-bit attention tests (test_attention_slices_host.py,
test_gpu_attention_slices.py), the GEMM tile tests (test_gemm_tiles_host.py, test_gpu_gemm_tiles.py) and the training step past 4096
rows and 8192 positions (test_train_scale_host.py, test_gpu_train_scale.py: the full-row objective, the float32 evaluation of the same
restatement as the yardstick of the fp32 kernels, labels per trip of a row loop and per table row).  A helper module, not a conftest.

``reference`` restates the oracle's encoder (manner_oracle.encode_tokens / encode_cls_train, whose embedding function it calls)
in float64, on the operands the 16-bit kernels consume: every weight matrix and embedding table rounded to the mode's 16-bit type
(biases and LayerNorm parameters stay f32, as the kernels read them), then widened.  Optionally it rounds at the kernels'
storage points as well (``store``; the inference path's points of tools/precision_sim.py):

  "qkv"    Q | K | V after the fused projection (the 16-bit qkv buffer the attention kernels read)
  "probs"  the probabilities fed to the PV product (after dropout and its 1 / (1 - p) scale)
  "ctx"    the attention output (the 16-bit ctx the out-projection GEMM reads)
  "inter"  the GeLU output (the 16-bit FFN intermediate)

In train mode a rounded point passes its gradient straight through: the backward's own 16-bit points (saved activations,
dctx16, dqkv16 of train.hip / train_attn.hip) are not restated.  The GPU tests use the points listed in their STORE tuple.

``error_map`` turns a kernel output and its reference into one RMS error per slice (a (news, 32-token block, head) cell, or any
labelling), relative to the RMS of the reference over the whole tensor, plus the map's maximum and its outlier ratio
(maximum / median): rounding noise spreads evenly over slices, a defect confined to one head or one block does not.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

import manner_oracle as O

DT16 = {"f16": torch.float16, "bf16": torch.bfloat16}
STORE_POINTS = ("qkv", "probs", "ctx", "inter")
MIN_SLICE = 128                      # elements below which a slice's RMS is too unstable to stand alone
MAX_THREADS = 16


def limit_threads() -> None:
    if torch.get_num_threads() > MAX_THREADS:
        torch.set_num_threads(MAX_THREADS)


def operands(w: Dict[str, object], mode: Optional[str], device="cpu", dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The weights as the kernels consume them, in ``dtype`` (float64): matrices and tables rounded to ``mode``'s 16-bit type first."""
    out = {}
    for k, v in w.items():
        t = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v.detach().cpu()).float()
        if mode is not None and t.dim() == 2:
            t = t.to(DT16[mode]).float()
        out[k] = t.to(dtype).to(device)
    return out


def _rounder(mode: Optional[str], store: Sequence[str]) -> Callable[[torch.Tensor, str], torch.Tensor]:
    unknown = set(store) - set(STORE_POINTS)
    assert not unknown, unknown
    assert mode is not None or not store, "storage rounding needs a 16-bit mode"
    pts = frozenset(store)

    def rnd(t, point):
        if point not in pts:
            return t
        return t + (t.to(DT16[mode]).to(t.dtype) - t).detach()          # straight-through in train mode
    return rnd


def embeddings(ids, p, cfg, full: bool = False):
    """The embedding stage of ``reference``: the oracle's; ``full``: the same sum with HF's padding_idx, which the padded positions
    of the full-row objective reach — nn.Embedding(padding_idx=pad_token_id) gives the pad token's word row no gradient, and RoBERTa
    builds its position table the same way (BERT's position table has no padding index)."""
    if not full:
        return O.embeddings(ids, p, cfg)
    pos = O.position_ids(ids, cfg.arch, cfg.pad_id).to(ids.device)
    x = F.embedding(ids, p["embeddings.word_embeddings.weight"], padding_idx=cfg.pad_id)
    x = x + p["embeddings.token_type_embeddings.weight"][0]
    x = x + F.embedding(pos, p["embeddings.position_embeddings.weight"], padding_idx=None if cfg.arch == O.ARCH_BERT else cfg.pad_id)
    return F.layer_norm(x, (cfg.hidden,), p["embeddings.LayerNorm.weight"], p["embeddings.LayerNorm.bias"], cfg.ln_eps)


def reference(cfg, w, ids, mask, mode: Optional[str] = None, store: Sequence[str] = (), train: bool = False, R=None,
              p_hidden: float = 0.0, p_attn: float = 0.0, p_out: float = 0.0, keep=None, device="cpu", grad_keys=None,
              dtype=torch.float64, full: bool = False, embed=None, attn=None) -> dict:
    """Float64 encoder over ``cfg.layers`` layers.

    Inference (``train=False``): {"hidden": [hidden_states[0..layers]] each [N, L, H], "cls": [N, H]}.
    Train (``train=True``): the reference of train.encode_train — the dropout sites of manner_oracle.encode_cls_train with
    ``keep(site, kind)`` replaying the kernels' masks — and autograd of (out * R).sum(): {"cls": [N, H], "grads": {name: grad}}
    over ``grad_keys`` (default: every tensor).  Results are float64 tensors on ``device``.

    ``full`` (train mode): the reference of train.encode_full_train — the objective is (hidden_states[-1] * R).sum() with ``R``
    [N, L, H] over all positions, the padded ones included (computed here as HF computes them: their own queries over the real
    keys), no [CLS] dropout, the embedding tables with HF's padding_idx (``embeddings``): {"out": [N, L, H], "grads": ...}.
    ``dtype``: the type the whole restatement is evaluated in — operands, additive mask, ``R`` and every result.  In float32 it is
    the yardstick of the measured bar of the fp32 kernels (side_ops_ref): run it on the CPU, or on a GPU without TF32.
    ``embed(ids, p, cfg)`` replaces the embedding stage: the host tests plant defects there.  ``attn(layer, q, k, v, add_mask)`` replaces
    the score, softmax and PV stage of a layer (q, k, v [N, heads, L, head_dim] after their storage point, add_mask [N, 1, 1, L]; it
    returns the context [N, heads, L, head_dim] before the "ctx" point and rounds the "probs" point itself): test_d32_slices_host.py
    plants one defect per loop of attention_d32.hip there."""
    limit_threads()
    if dtype != torch.float64 and torch.device(device).type == "cuda":
        assert not torch.backends.cuda.matmul.allow_tf32, "the float32 evaluation is a yardstick only without TF32"
    assert not full or train, "full rows: the training objective over all positions"
    ids, mask = O._t(ids).long().to(device), O._t(mask).to(device)
    p = O.bert_named(operands(w, mode, device, dtype), cfg)
    if train:
        for k in (p if grad_keys is None else grad_keys):
            p[k].requires_grad_(True)
    rnd = _rounder(mode, store)
    n, s = ids.shape
    h, a, d = cfg.hidden, cfg.heads, cfg.head_dim

    def drop(x, prob, site, kind):
        if not train or prob <= 0.0:
            return x
        return x * keep(site, kind).to(device=device, dtype=x.dtype) / (1.0 - prob)

    add_mask = torch.zeros(mask.shape, dtype=dtype, device=device)
    add_mask = add_mask.masked_fill(mask == 0, torch.finfo(torch.float32).min)[:, None, None, :]
    with torch.set_grad_enabled(train):
        x = drop(embeddings(ids, p, cfg, full) if embed is None else embed(ids, p, cfg), p_hidden, 0, "rows")
        hidden = [x]
        for l in range(cfg.layers):
            pre = f"encoder.layer.{l}."

            def lin(t, name):
                return F.linear(t, p[pre + name + ".weight"], p[pre + name + ".bias"])

            q, k, v = (rnd(lin(x, f"attention.self.{m}"), "qkv").view(n, s, a, d).transpose(1, 2) for m in ("query", "key", "value"))
            if attn is None:
                att = F.softmax(torch.matmul(q, k.transpose(2, 3)) * (d ** -0.5) + add_mask, dim=-1)
                att = rnd(drop(att, p_attn, 8 * (l + 1), "attn"), "probs")
                ctx = torch.matmul(att, v)
            else:
                assert not train, "the attention hook restates the inference kernels"
                ctx = attn(l, q, k, v, add_mask)
            ctx = rnd(ctx.transpose(1, 2).reshape(n, s, h), "ctx")
            x = F.layer_norm(drop(lin(ctx, "attention.output.dense"), p_hidden, 8 * (l + 1) + 1, "rows") + x, (h,),
                             p[pre + "attention.output.LayerNorm.weight"], p[pre + "attention.output.LayerNorm.bias"], cfg.ln_eps)
            inter = rnd(F.gelu(lin(x, "intermediate.dense")), "inter")
            x = F.layer_norm(drop(lin(inter, "output.dense"), p_hidden, 8 * (l + 1) + 2, "rows") + x, (h,),
                             p[pre + "output.LayerNorm.weight"], p[pre + "output.LayerNorm.bias"], cfg.ln_eps)
            hidden.append(x)
        cls = x if full else drop(x[:, 0, :], p_out, 1, "cls")
        if not train:
            return {"hidden": hidden, "cls": cls}
        (cls * O._t(R).to(device=device, dtype=dtype)).sum().backward()
    return {"out" if full else "cls": cls.detach(), "grads": {k: (None if t.grad is None else t.grad) for k, t in p.items() if t.requires_grad}}


# ------------------------------------------------------------------------------------------------ labellings
def token_block_head_labels(mask: np.ndarray, hidden: int, heads: int, block: int = 32) -> np.ndarray:
    """[N, L, H] int64: one label per (news, head, token block) over the real tokens, -1 on padding.  Labels run over blocks
    fastest, so a short last block merges with the block before it in the same news and head."""
    mask = np.asarray(mask)
    n, lp = mask.shape
    nb = (lp + block - 1) // block
    news = np.arange(n)[:, None, None]
    blk = (np.arange(lp) // block)[None, :, None]
    head = (np.arange(hidden) // (hidden // heads))[None, None, :]
    lab = (news * heads + head) * nb + blk
    return np.where(mask[:, :, None] != 0, lab, -1).astype(np.int64)


def news_labels(n: int, hidden: int) -> np.ndarray:
    """[N, H]: one slice per news (the [CLS] outputs)."""
    return np.repeat(np.arange(n, dtype=np.int64)[:, None], hidden, 1)


def head_row_labels(shape, heads: int) -> np.ndarray:
    """A [H_out, ...] projection weight or [H_out] bias: one slice per head (rows 64h .. 64h+63)."""
    rows = np.arange(shape[0]) // (shape[0] // heads)
    return np.broadcast_to(rows.reshape((-1,) + (1,) * (len(shape) - 1)), shape).astype(np.int64)


def packed_tile_labels(mask: np.ndarray, hidden: int, rows: int = 64, cols: int = 64) -> np.ndarray:
    """[N, L, H] int64: (packed_row // rows) * (hidden // cols) + col // cols over the real tokens, -1 on padding.  packed_row is
    the running count of real tokens in news order: the row the GEMMs see when the call is one chunk.  64 x 64 divides the 256- and
    192-row panels, the 256-column tile and the 128 x 64 wave tile of the persistent GEMMs."""
    mask = np.asarray(mask) != 0
    assert hidden % cols == 0, (hidden, cols)
    row = (np.cumsum(mask.ravel()) - 1).reshape(mask.shape)
    lab = (row // rows)[:, :, None] * (hidden // cols) + (np.arange(hidden) // cols)[None, None, :]
    return np.where(mask[:, :, None], lab, -1).astype(np.int64)


def weight_tile_labels(shape, tn: int = 128, tk: int = 64) -> np.ndarray:
    """An [N, K] weight gradient: one slice per tn x tk block, the wave tiles of the 256 x 256 wgrad_tr_kernel tile and of the
    data-gradient GEMMs.  Labels run over K blocks fastest."""
    n, k = shape
    return ((np.arange(n) // tn)[:, None] * ((k + tk - 1) // tk) + (np.arange(k) // tk)[None, :]).astype(np.int64)


def vector_block_labels(n: int, block: int = 64) -> np.ndarray:
    """A bias or LayerNorm gamma / beta gradient: one slice per ``block`` elements (use with min_count=block, per_slice=True)."""
    return (np.arange(n) // block).astype(np.int64)


def trip_labels(mask: np.ndarray, rows_per_trip: int = 4096) -> np.ndarray:
    """[N, L] int64: packed row // ``rows_per_trip`` over the real tokens, -1 on padding — the trip of a grid-stride row loop that
    visits the row (ln_bwd_kernel: 1024 workgroups of four waves, one row a wave); for full rows pass a mask of ones."""
    mask = np.asarray(mask) != 0
    row = (np.cumsum(mask.ravel()) - 1).reshape(mask.shape)
    return np.where(mask, row // rows_per_trip, -1).astype(np.int64)


def table_row_labels(n_rows: int, rows) -> np.ndarray:
    """[n_rows, 1] int64: an embedding-table gradient of a batch with repeated ids, one slice per table row in ``rows`` (the label is
    the row), -1 elsewhere (use with min_count=H, per_slice=True)."""
    lab = np.full(n_rows, -1, dtype=np.int64)
    rows = np.asarray(sorted(set(int(r) for r in rows)), dtype=np.int64)
    lab[rows] = rows
    return lab[:, None]


# ------------------------------------------------------------------------------------------------ the map
class SliceMap(dict):
    """rms: per-slice RMS error / RMS(reference); labels: the first label of each (merged) slice; max, median, ratio, worst."""

    def __repr__(self):
        return f"SliceMap(max={self['max']:.3e}, median={self['median']:.3e}, ratio={self['ratio']:.2f}, worst={self['worst']}, n={len(self['rms'])})"


def error_map(hip, ref, labels, min_count: int = MIN_SLICE, per_slice: bool = False, floor: float = 1e-2) -> SliceMap:
    """Per-slice RMS of (hip - ref) over the elements of each label (>= 0; -1 is left out), divided by the RMS of ``ref`` over all
    labelled elements.  Slices of fewer than ``min_count`` elements are merged into the slice of the next lower label (the first
    one into the next higher), so the labelling decides who a slice's neighbour is.

    ``per_slice``: divide each slice by the RMS of ``ref`` over that slice instead (at least ``floor`` x the whole tensor's RMS), for
    tensors whose slices differ in scale by construction — a gradient row of a token in a 31-token news is an order of magnitude
    larger than one in a 512-token news, and 16-bit rounding noise scales with it."""
    hip = np.asarray(hip.detach().cpu() if isinstance(hip, torch.Tensor) else hip, dtype=np.float64)
    ref = np.asarray(ref.detach().cpu() if isinstance(ref, torch.Tensor) else ref, dtype=np.float64)
    labels = np.broadcast_to(np.asarray(labels), ref.shape)
    assert hip.shape == ref.shape, (hip.shape, ref.shape)
    sel = labels >= 0
    lab, e, r = labels[sel], (hip - ref)[sel], ref[sel]
    assert np.isfinite(e).all(), "non-finite kernel output"
    scale = float(np.sqrt(np.mean(r * r)))
    assert scale > 0.0, "all-zero reference"
    uniq, inv = np.unique(lab, return_inverse=True)
    cnt = np.bincount(inv).astype(np.float64)
    sq = np.bincount(inv, weights=e * e)
    rq = np.bincount(inv, weights=r * r)
    groups = []                                            # [first label, count, error sum of squares, reference sum of squares]
    for u, c, s, q in zip(uniq, cnt, sq, rq):
        if groups and (groups[-1][1] < min_count or c < min_count):   # the slice before is still too small, or this one is: merge
            groups[-1][1] += c
            groups[-1][2] += s
            groups[-1][3] += q
        else:
            groups.append([int(u), c, s, q])
    rms = np.array([np.sqrt(s / c) / (max(np.sqrt(q / c), floor * scale) if per_slice else scale) for _, c, s, q in groups])
    med = float(np.median(rms))
    i = int(np.argmax(rms))
    return SliceMap(rms=rms, labels=np.array([g[0] for g in groups]), max=float(rms[i]), median=med,
                    ratio=float(rms[i] / med) if med > 0 else float("inf"), worst=int(groups[i][0]))
