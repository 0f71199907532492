"""Device-side composition of the hot path above the C ABI.

* ``cr_forward`` / ``ensemble_forward`` restate ``CRModule.forward`` (reference
  manner/models/cr_module.py:105-131) and ``EnsembleModule.forward`` / ``_submodel_forward``
  (reference manner/models/ensemble_module.py:95-151) on the fused HIP kernels, returning the same
  dense ``[B, Cmax]`` score matrix (padded slots: 0 for the CR-Module, the z-scored zero for the ensemble)
  — mode R of SURVEY.md §8d: every history and candidate occurrence is encoded.
* ``caum_forward`` / ``caum_train_step`` and ``miner_forward`` / ``miner_train_step`` do the same for ``CAUMPLMModule`` and
  ``MINERModule`` (reference manner/models/baselines/): the module's own lines between the mirrored leaf classes.
* ``tanr_forward`` / ``tanr_train_step`` and ``sentirec_forward`` / ``sentirec_train_step`` are ``TANRPLMModule`` and
  ``SentiRecPLMModule``: the auxiliary head over every news row, its loss and SentiRec's diversity regulariser (csrc/aspect.hip).
* ``senti_debias_forward`` / ``senti_debias_generator_step`` / ``senti_debias_discriminator_step`` are ``SentiDebiasPLMModule``'s
  generator and its two optimiser steps: the sentiment encoder as a class table, the orthogonality terms, the bias-aware scores and the
  adversarial discriminator (csrc/debias.hip).
* ``encode_table`` / ``score_impressions`` are the table architecture (mode T): each unique news is
  encoded once per module into ``[N_news, D]``, impressions are scored by index.  Valid for
  ``use_entities=False`` only.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import hip, train

Tensor = torch.Tensor


def segment_offsets(batch: Tensor, num_segments: int) -> Tensor:
    """Sorted segment ids (reference ``_make_batch_assignees``, mind_rec_dataset.py:171-174) -> CSR
    offsets int64 [B+1], on device, no host sync: off[i] = first position whose id is >= i (the ids are sorted ascending, as the
    reference's collate produces them).  Round 5: ``torch.bincount`` — used here before — reads its input's maximum back to the host
    to size its output, i.e. it WAITS for everything enqueued so far; in a training step that was the whole encoder forward
    (2.7 ms of host stall per call, after which the GPU idled through the backward's enqueue latency)."""
    marks = torch.arange(num_segments + 1, dtype=batch.dtype, device=batch.device)
    return torch.searchsorted(batch.contiguous(), marks, right=False).to(torch.int64)


def _width(batch: Dict, key: str, off: Tensor) -> int:
    """Width of a dense [B, max, *] view: the collate's host-known maximum when the batch carries it (``hist_max`` /
    ``cand_max``, set by DeviceCollate), else one device read — the same sync ``to_dense_batch`` performs."""
    w = batch.get(key) if hasattr(batch, "get") else None
    if w is not None:
        return int(w)
    return int((off[1:] - off[:-1]).max()) if off.numel() > 1 else 0


def ragged_to_dense(values: Tensor, off: Tensor, width: Optional[int] = None, fill: Optional[Tensor] = None) -> Tensor:
    """K9 for a ragged vector / row matrix: [sum c_i, *] -> [B, Cmax, *] (``to_dense_batch`` layout) through
    ``manner_hip_to_dense``; padded slots hold 0, or ``fill[b]``."""
    if width is None:
        width = int((off[1:] - off[:-1]).max()) if off.numel() > 1 else 0   # the same sync to_dense_batch performs
    return hip.to_dense(values, off, width, fill=fill)


def _late_fusion_ragged(hist_vec: Tensor, cand_vec: Tensor, hist_off: Tensor, cand_off: Tensor) -> Tensor:
    table = torch.cat([hist_vec, cand_vec], dim=0)
    nh, nc = hist_vec.shape[0], cand_vec.shape[0]
    hidx = torch.arange(nh, dtype=torch.int32, device=table.device)
    cidx = torch.arange(nh, nh + nc, dtype=torch.int32, device=table.device)
    return hip.score_late_fusion(table, hidx, hist_off, cidx, cand_off, total_cand=nc)


def cr_forward(news_encoder, batch: Dict, late_fusion: bool = True, user_encoder=None, click_predictor=None,
               dense: bool = True) -> Tensor:
    """CRModule.forward: scores [B, Cmax] (or the ragged [sum c_i] vector with ``dense=False``).  No torch indexing
    and — when the batch carries ``hist_max`` / ``cand_max`` — no host synchronisation.  Padded slots are exactly 0, as in the
    reference — but for an impression WITHOUT history rows (which the reference's loader drops, mind_dataframe.py:313): its real
    candidates score NaN here as there (0 / 0), its padded slots 0 here and NaN there (NaN user . zero vector)."""
    nb = batch["users"].numel() if "users" in batch and batch["users"] is not None else int(batch["batch_cand"].max()) + 1
    hip.status_poll(batch["batch_cand"].device)
    hist_vec = news_encoder(batch["x_hist"])
    cand_vec = news_encoder(batch["x_cand"])
    hist_off = segment_offsets(batch["batch_hist"], nb)
    cand_off = segment_offsets(batch["batch_cand"], nb)
    if late_fusion:
        ragged = _late_fusion_ragged(hist_vec, cand_vec, hist_off, cand_off)
    else:
        # early fusion: the unmasked additive pooler sees the ZERO-PADDED history
        hist_dense = hip.to_dense(hist_vec, hist_off, _width(batch, "hist_max", hist_off))
        user = user_encoder(hist_dense)
        if click_predictor is not None and dense:
            # the reference's own call shape: DotProduct(user [B,1,D], cand^T [B,D,Cmax]) on the dense candidates
            cand_dense = hip.to_dense(cand_vec, cand_off, _width(batch, "cand_max", cand_off))
            return click_predictor(user.unsqueeze(1), cand_dense.permute(0, 2, 1))
        cidx = torch.arange(cand_vec.shape[0], dtype=torch.int32, device=cand_vec.device)
        ragged = hip.score_user(cand_vec, user, cidx, cand_off)
    hip.status_arm(cand_vec.device)
    return hip.to_dense(ragged, cand_off, _width(batch, "cand_max", cand_off)) if dense else ragged


def caum_forward(news_encoder, user_encoder, batch: Dict, dense: bool = True) -> Tensor:
    """CAUMPLMModule.forward (reference baselines/caum_plm_module.py:146-165): the two news-encoder calls, ``to_dense_batch`` of both
    sides, and the candidate loop as ONE call of ``user_encoder.forward_all`` (the CAUMUserEncoder of this package) -> scores
    [B, Cmax] with the reference's value in every slot: a zero-padded candidate row scores 0, a zero-padded history row takes part
    in every user's softmax.  No host synchronisation when the batch carries ``hist_max`` / ``cand_max``.  ``dense=False`` returns
    the real slots of that matrix as the ragged [sum c_i] vector (the padded rows still take part in the attention across the
    users, as in the reference; the selection reads the count back to the host).  With grad enabled and news rows that require grad
    the dense tensors come from ``train.to_dense`` and the scores keep their graph into the rows (``dense=True`` only)."""
    nb =batch["users"].numel() if "users" in batch and batch["users"] is not None else int(batch["batch_cand"].max()) + 1
    hip.status_poll(batch["batch_cand"].device)
    hist_vec = news_encoder(batch["x_hist"])
    cand_vec = news_encoder(batch["x_cand"])
    hist_off = segment_offsets(batch["batch_hist"], nb)
    cand_off = segment_offsets(batch["batch_cand"], nb)
    if dense and torch.is_grad_enabled() and (hist_vec.requires_grad or cand_vec.requires_grad):      # training: the rows keep their graph
        hist_dense = train.to_dense(hist_vec, hist_off, _width(batch, "hist_max", hist_off))
        cand_dense = train.to_dense(cand_vec, cand_off, _width(batch, "cand_max", cand_off))
    else:
        hist_dense = hip.to_dense(hist_vec, hist_off, _width(batch, "hist_max", hist_off))
        cand_dense = hip.to_dense(cand_vec, cand_off, _width(batch, "cand_max", cand_off), with_mask=not dense)
    if not dense:
        cand_dense, real = cand_dense
    scores = user_encoder.forward_all(hist_dense, cand_dense)
    hip.status_arm(cand_vec.device)
    return scores if dense else scores[real]


def caum_train_step(news_encoder, user_encoder, batch: Dict):
    """CAUMPLMModule.model_step for training (reference baselines/caum_plm_module.py:174-189): ``forward`` through ``caum_forward`` —
    the candidate loop as one ``forward_all`` call; with ``CAUMUserEncoder.train_all_columns`` set, one library call forward and one
    backward for all columns — then ``nn.CrossEntropyLoss(scores, y_true)`` on the dense zero-padded rows, computed by
    ``train.model_step_loss(supcon=False, c_max=...)`` from the real slots: a zero-padded candidate row scores exactly 0 with or without
    dropout, the padded zero that loss mode puts into the softmax.  No host synchronisation when the batch carries ``hist_max`` /
    ``cand_max``.  Returns (loss, ragged scores [sum c_i] detached, cand_off) — call ``loss.backward()`` and step the optimiser."""
    nb = batch["users"].numel() if "users" in batch and batch["users"] is not None else int(batch["batch_cand"].max()) + 1
    cand_off = segment_offsets(batch["batch_cand"], nb)
    c_max = _width(batch, "cand_max", cand_off)
    dense = caum_forward(news_encoder, user_encoder, dict(batch, cand_max=c_max), dense=True)
    ragged = dense.reshape(-1).index_select(0, train.dense_slots(cand_off, int(batch["batch_cand"].numel()), c_max))
    loss, _ = train.model_step_loss(ragged, batch["labels"].to(torch.float32), cand_off, supcon=False, c_max=c_max)
    return loss, ragged.detach(), cand_off


def _cat_tokens(a: Dict, b: Dict, pad_id: int) -> Dict:
    """Two tokenised news sets as one call: rows of `a` then rows of `b`, right-padded to the longer padded length."""
    la, lb = a["input_ids"].shape[1], b["input_ids"].shape[1]
    lp = max(la, lb)

    def pad(t, l, value):
        return t if l == lp else torch.nn.functional.pad(t, (0, lp - l), value=value)

    return {"input_ids": torch.cat([pad(a["input_ids"], la, pad_id), pad(b["input_ids"], lb, pad_id)]),
            "attention_mask": torch.cat([pad(a["attention_mask"], la, 0), pad(b["attention_mask"], lb, 0)])}


def encode_hist_and_cand(news_encoder, x_hist: Dict, x_cand: Dict):
    """The two news_encoder calls of CRModule.forward (cr_module.py:107,113).  Without entities a news embedding does not
    depend on its batch, so both sets go through ONE call — one pass over the weights, GEMMs twice as tall —
    and are split afterwards; with use_entities=True the entity attention couples the news of a call (Q1) and the
    reference's two separate calls are kept."""
    keyed = isinstance(x_hist, dict) and "text" in x_hist
    if getattr(news_encoder, "use_entities", False):
        return news_encoder(x_hist), news_encoder(x_cand)
    th, tc = (x_hist["text"], x_cand["text"]) if keyed else (x_hist, x_cand)
    pad_id = getattr(getattr(getattr(news_encoder, "text_encoder", None), "plm_model", None), "cfg", None)
    merged = _cat_tokens(th, tc, pad_id.pad_id if pad_id is not None else 0)
    both = news_encoder({"text": merged} if keyed else merged)
    n_hist = th["input_ids"].shape[0]
    return both[:n_hist], both[n_hist:]


def cr_train_step(news_encoder, batch: Dict, supcon: bool = True, temperature: float = 0.1):
    """CRModule.model_step for training (cr_module.py:140-171 with late_fusion=True, the shipped MANNeR setting): the
    encoder in train() mode, the fused late-fusion scorer and the loss, all with autograd on the HIP engine.
    Returns (loss, ragged scores [sum c_i] detached, cand_off) — call ``loss.backward()`` and step the reference's optimiser."""
    nb = batch["users"].numel() if "users" in batch and batch["users"] is not None else int(batch["batch_cand"].max()) + 1
    hip.status_poll(batch["batch_cand"].device)       # (encode_train arms the word again after its own kernels)
    hist_off = segment_offsets(batch["batch_hist"], nb)
    cand_off = segment_offsets(batch["batch_cand"], nb)
    hist_vec, cand_vec = encode_hist_and_cand(news_encoder, batch["x_hist"], batch["x_cand"])
    scores = train.late_fusion_scores(hist_vec, hist_off, cand_vec, cand_off)
    c_max = None if supcon else _width(batch, "cand_max", cand_off)
    loss, _ = train.model_step_loss(scores, batch["labels"].to(torch.float32), cand_off, supcon=supcon, temperature=temperature,
                                    c_max=c_max)
    return loss, scores.detach(), cand_off


def _miner_scores(hist_vec: Tensor, cand_vec: Tensor, user_encoder, batch: Dict, nb: int, score_type: str, target_aware_attn,
                  category_embedding, category_dropout):
    """The lines of MINERModule.forward below its two encoder calls (reference baselines/miner_module.py:156-212) ->
    (user_vector [B, K, D], ragged scores [sum c_i], cand_off, Cmax or None when nothing needed it)."""
    if score_type not in ("max", "mean", "weighted"):
        raise ValueError("Invalid method of aggregating scores.")
    hist_off = segment_offsets(batch["batch_hist"], nb)
    cand_off = segment_offsets(batch["batch_cand"], nb)
    s = _width(batch, "hist_max", hist_off)
    graph = torch.is_grad_enabled() and (hist_vec.requires_grad or cand_vec.requires_grad)
    hist_dense = (train.to_dense if graph else hip.to_dense)(hist_vec, hist_off, s)
    mask_hist = torch.arange(s, device=hist_off.device)[None, :] < (hist_off[1:] - hist_off[:-1])[:, None]
    bias = None
    if category_embedding is not None:
        p = float(category_dropout.p) if category_dropout is not None and category_dropout.training else 0.0
        # the mirrors' seed draw on torch's CPU generator, history first; none at p = 0 or in eval()
        seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2)] if p > 0.0 else (0, 0)
        bias = hip.miner_category_bias(batch["x_hist"]["category"], batch["x_cand"]["category"], category_embedding.weight.detach(), hist_off,
                                       cand_off, s, p=p, seeds=seeds)
    user_vector = user_encoder(clicked_news_vector=hist_dense, attn_mask=mask_hist, bias=bias)
    c_max = None
    if score_type == "weighted":
        if target_aware_attn is None:
            raise ValueError("score_type 'weighted' needs target_aware_attn")
        c_max = _width(batch, "cand_max", cand_off)
        grad_on = torch.is_grad_enabled()
        cand_dense = (train.to_dense if grad_on and cand_vec.requires_grad else hip.to_dense)(cand_vec, cand_off, c_max)
        rows = user_vector.permute(0, 2, 1)
        value = train.bmm(cand_dense, rows) if grad_on and (cand_dense.requires_grad or user_vector.requires_grad) else hip.bmm(cand_dense, rows)
        dense = target_aware_attn(query=user_vector, key=cand_dense, value=value)
        ragged = dense.reshape(-1).index_select(0, train.dense_slots(cand_off, int(batch["batch_cand"].numel()), c_max))
    elif torch.is_grad_enabled() and (cand_vec.requires_grad or user_vector.requires_grad):
        ragged = train.miner_code_scores(cand_vec, cand_off, user_vector, score_type)
    else:
        ragged = hip.miner_code_scores(cand_vec, cand_off, user_vector, score_type)
    return user_vector, ragged, cand_off, c_max


def _miner_dense(ragged: Tensor, cand_off: Tensor, width: int) -> Tensor:
    return (train.to_dense if torch.is_grad_enabled() and ragged.requires_grad else hip.to_dense)(ragged, cand_off, width)


def miner_forward(news_encoder, user_encoder, batch: Dict, *, score_type: str, target_aware_attn=None, category_embedding=None,
                  category_dropout=None, dense: bool = True):
    """MINERModule.forward (reference baselines/miner_module.py:153-212) -> (user_vector [B, K, D], scores): the two news-encoder calls on
    ``batch["x_hist"]["text"]`` / ``batch["x_cand"]["text"]``, the history to dense with its mask, the category bias as ONE
    ``hip.miner_category_bias`` call when ``category_embedding`` (the frozen nn.Embedding) is given — ``category_dropout`` is the
    module's nn.Dropout, its ``.p`` and ``.training`` are read — ``user_encoder`` (the PolyAttention of this package), and the scores:
    'max' / 'mean' by ``miner_code_scores`` on the ragged rows, 'weighted' through to_dense -> bmm -> ``target_aware_attn``.
    ``dense=True`` returns [B, Cmax] with padded slots exactly 0 (a zero-padded candidate row scores 0 under all three types),
    ``dense=False`` the ragged [sum c_i] vector.  No host synchronisation when the batch carries ``hist_max`` / ``cand_max``."""
    nb = batch["users"].numel() if "users" in batch and batch["users"] is not None else int(batch["batch_cand"].max()) + 1
    hip.status_poll(batch["batch_cand"].device)
    hist_vec = news_encoder(batch["x_hist"]["text"])
    cand_vec = news_encoder(batch["x_cand"]["text"])
    user_vector, ragged, cand_off, c_max = _miner_scores(hist_vec, cand_vec, user_encoder, batch, nb, score_type, target_aware_attn,
                                                        category_embedding, category_dropout)
    hip.status_arm(cand_vec.device)
    if not dense:
        return user_vector, ragged
    return user_vector, _miner_dense(ragged, cand_off, c_max if c_max is not None else _width(batch, "cand_max", cand_off))


def miner_train_step(news_encoder, user_encoder, batch: Dict, *, score_type: str, target_aware_attn=None, category_embedding=None,
                     category_dropout=None):
    """The loss lines of MINERModule.model_step (reference baselines/miner_module.py:226-242): ``forward`` as ``miner_forward`` — with both
    news sets through ONE encoder call — then ``nn.CrossEntropyLoss(scores [B, Cmax], y_true)`` from the ragged scores
    (``train.model_step_loss(supcon=False, c_max=...)`` supplies the padded zeros) plus ``train.disagreement_loss(user_vector)``.
    Returns (loss, ragged scores [sum c_i] detached, cand_off) — call ``loss.backward()`` and step the optimiser.  The metrics
    bookkeeping of ``model_step`` (preds / targets / sizes per impression) is the caller's."""
    nb = batch["users"].numel() if "users" in batch and batch["users"] is not None else int(batch["batch_cand"].max()) + 1
    hip.status_poll(batch["batch_cand"].device)
    # one encoder call for both sets, as encode_hist_and_cand (MINERNewsEncoder takes the token dict itself and holds the PLM directly)
    th, tc = batch["x_hist"]["text"], batch["x_cand"]["text"]
    cfg = getattr(getattr(news_encoder, "plm_model", None), "cfg", None)
    both = news_encoder(_cat_tokens(th, tc, cfg.pad_id if cfg is not None else 0))
    hist_vec, cand_vec = both[:th["input_ids"].shape[0]], both[th["input_ids"].shape[0]:]
    user_vector, ragged, cand_off, c_max = _miner_scores(hist_vec, cand_vec, user_encoder, batch, nb, score_type, target_aware_attn,
                                                        category_embedding, category_dropout)
    hip.status_arm(cand_vec.device)
    if c_max is None:
        c_max = _width(batch, "cand_max", cand_off)
    ce, _ = train.model_step_loss(ragged, batch["labels"].to(torch.float32), cand_off, supcon=False, c_max=c_max)
    return ce + train.disagreement_loss(user_vector), ragged.detach(), cand_off


def _encode_joined(news_encoder, th: Dict, tc: Dict):
    """Both token sets through ONE call of a PLMTextEncoder, as ``encode_hist_and_cand`` -> (rows [N_hist + N_cand, D] as the encoder
    left them, history first; N_hist)."""
    cfg = getattr(getattr(news_encoder, "plm_model", None), "cfg", None)
    return news_encoder(_cat_tokens(th, tc, cfg.pad_id if cfg is not None else 0)), th["input_ids"].shape[0]


def _aspect_scores(hist_vec: Tensor, cand_vec: Tensor, user_encoder, batch: Dict, nb: int):
    """The lines TANRPLMModule.forward and SentiRecPLMModule.forward share below the encoder calls (tanr_plm_module.py:125-136): both
    sides to dense, the user encoder (NAMLUserEncoder / NRMSUserEncoder of this package), DotProduct -> (scores [B, Cmax], hist_off,
    cand_off, Cmax); a zero-padded candidate row scores exactly 0."""
    hist_off = segment_offsets(batch["batch_hist"], nb)
    cand_off = segment_offsets(batch["batch_cand"], nb)
    s, c_max = _width(batch, "hist_max", hist_off), _width(batch, "cand_max", cand_off)
    graph = torch.is_grad_enabled()
    dense_of = train.to_dense if graph and (hist_vec.requires_grad or cand_vec.requires_grad) else hip.to_dense
    user = user_encoder(dense_of(hist_vec, hist_off, s))
    cand_dense = dense_of(cand_vec, cand_off, c_max)
    dot = train.dot if graph and (user.requires_grad or cand_dense.requires_grad) else hip.dot
    return dot(user.unsqueeze(1), cand_dense.permute(0, 2, 1)), hist_off, cand_off, c_max


def _aspect_forward(news_encoder, user_encoder, predictor, batch: Dict, dense: bool):
    nb = batch["users"].numel() if "users" in batch and batch["users"] is not None else int(batch["batch_cand"].max()) + 1
    hip.status_poll(batch["batch_cand"].device)
    hist_vec = news_encoder(batch["x_hist"]["text"])
    cand_vec = news_encoder(batch["x_cand"]["text"])
    scores, _, cand_off, c_max = _aspect_scores(hist_vec, cand_vec, user_encoder, batch, nb)
    graph = torch.is_grad_enabled() and (cand_vec.requires_grad or predictor.weight.requires_grad)
    lin = train.linear if graph else hip.linear
    w, b = (predictor.weight, predictor.bias) if graph else (predictor.weight.detach(), predictor.bias.detach())
    head = torch.cat((lin(cand_vec, w, b), lin(hist_vec, w, b)), dim=0)      # the reference's order; O columns wide, not D
    hip.status_arm(cand_vec.device)
    if not dense:
        scores = scores.reshape(-1).index_select(0, train.dense_slots(cand_off, int(batch["batch_cand"].numel()), c_max))
    return scores, head


def tanr_forward(news_encoder, user_encoder, topic_predictor, batch: Dict, dense: bool = True):
    """TANRPLMModule.forward (reference baselines/tanr_plm_module.py:122-143) -> (scores [B, Cmax], topic_scores [N, num_topics]): the
    two news-encoder calls on ``batch["x_hist"]["text"]`` / ``batch["x_cand"]["text"]``, both sides to dense, ``user_encoder`` (the
    NAMLUserEncoder of this package), DotProduct, and ``topic_predictor`` (the module's own nn.Linear) over the candidate rows, then
    the history rows — this path materialises the logits; ``tanr_train_step`` does not.  Padded score slots are exactly 0;
    ``dense=False`` returns the ragged [sum c_i] scores.  No host synchronisation when the batch carries ``hist_max`` / ``cand_max``."""
    return _aspect_forward(news_encoder, user_encoder, topic_predictor, batch, dense)


def sentirec_forward(news_encoder, user_encoder, sentiment_predictor, batch: Dict, dense: bool = True):
    """SentiRecPLMModule.forward (reference baselines/sentirec_plm_module.py:124-145) -> (scores [B, Cmax], senti_scores [N, 1]):
    ``tanr_forward`` with the NRMSUserEncoder of this package and the module's ``nn.Linear(D, 1)``."""
    return _aspect_forward(news_encoder, user_encoder, sentiment_predictor, batch, dense)


def _aspect_step(news_encoder, user_encoder, batch: Dict):
    """forward for a step: ONE encoder call -> (rows [N_hist + N_cand, D] history first, ragged scores, hist_off, cand_off, Cmax, CE)"""
    nb = batch["users"].numel() if "users" in batch and batch["users"] is not None else int(batch["batch_cand"].max()) + 1
    hip.status_poll(batch["batch_cand"].device)
    rows, n_hist = _encode_joined(news_encoder, batch["x_hist"]["text"], batch["x_cand"]["text"])
    dense, hist_off, cand_off, c_max = _aspect_scores(rows[:n_hist], rows[n_hist:], user_encoder, batch, nb)
    ragged = dense.reshape(-1).index_select(0, train.dense_slots(cand_off, int(batch["batch_cand"].numel()), c_max))
    ce, _ = train.model_step_loss(ragged, batch["labels"].to(torch.float32), cand_off, supcon=False, c_max=c_max)
    return rows, ragged, hist_off, cand_off, c_max, ce


def _head_params(predictor):
    return (predictor.weight, predictor.bias) if torch.is_grad_enabled() else (predictor.weight.detach(), predictor.bias.detach())


def tanr_train_step(news_encoder, user_encoder, topic_predictor, batch: Dict, topic_pred_loss_coef: float):
    """The loss lines of TANRPLMModule.model_step (reference baselines/tanr_plm_module.py:157-177): ``forward`` with both news sets
    through ONE encoder call, ``nn.CrossEntropyLoss(scores [B, Cmax], y_true)`` from the ragged scores, plus ``topic_pred_loss_coef``
    times the topic head's cross-entropy over every news row — ``train.head_ce_loss`` on the encoder's output as it lies (history
    rows, then candidate rows, the categories in the same order: the mean does not depend on the order), no ``torch.cat`` of the rows,
    no one-hot matrix, no [N, num_topics] logits.  Under ``torch.no_grad()`` (val/loss, test/loss) the same kernels run without
    saving anything.  Returns (loss, ragged scores [sum c_i] detached, cand_off); the metrics bookkeeping of ``model_step`` is the
    caller's.  No host synchronisation when the batch carries ``hist_max`` / ``cand_max``."""
    rows, ragged, _, cand_off, _, ce = _aspect_step(news_encoder, user_encoder, batch)
    topics = torch.cat((batch["x_hist"]["category"].reshape(-1), batch["x_cand"]["category"].reshape(-1))).to(torch.int64)
    head = (train.head_ce_loss if torch.is_grad_enabled() else hip.head_ce_loss)(rows, *_head_params(topic_predictor), topics)
    hip.status_arm(rows.device)
    return ce + float(topic_pred_loss_coef) * head, ragged.detach(), cand_off


def sentirec_train_step(news_encoder, user_encoder, sentiment_predictor, batch: Dict, senti_pred_loss_coef: float, senti_div_loss_coef: float):
    """The loss lines of SentiRecPLMModule.model_step (reference baselines/sentirec_plm_module.py:159-193): as ``tanr_train_step`` with
    ``nn.L1Loss`` of the sentiment head over every news row (``train.head_l1_loss``) times ``senti_pred_loss_coef``, plus
    ``senti_div_loss_coef`` times the diversity regulariser ``relu(u * s_cand * scores).mean()`` over the dense [B, Cmax] block —
    ``train.senti_div_loss`` on the ragged scores, the user's mean history sentiment formed on the device: no dense blocks, no
    per-impression host loop, no host read.  Returns (loss, ragged scores [sum c_i] detached, cand_off)."""
    rows, ragged, hist_off, cand_off, c_max, ce = _aspect_step(news_encoder, user_encoder, batch)
    hs, cs = batch["x_hist"]["sentiment_score"].reshape(-1).to(torch.float32), batch["x_cand"]["sentiment_score"].reshape(-1).to(torch.float32)
    graph = torch.is_grad_enabled()
    head = (train.head_l1_loss if graph else hip.head_l1_loss)(rows, *_head_params(sentiment_predictor), torch.cat((hs, cs)))
    div = (train.senti_div_loss if graph else hip.senti_div_loss)(ragged, cs, hs, hist_off, cand_off, c_max)
    hip.status_arm(rows.device)
    return ce + float(senti_pred_loss_coef) * head + float(senti_div_loss_coef) * div, ragged.detach(), cand_off


def _debias_classes(batch: Dict):
    return batch["x_hist"]["sentiment"].reshape(-1).to(torch.int64), batch["x_cand"]["sentiment"].reshape(-1).to(torch.int64)


def _debias_lines(rows: Tensor, n_hist: int, user_encoder, sentiment_encoder, batch: Dict, nb: int):
    """The lines of SentiDebias's Generator.forward below its encoder calls (reference baselines/senti_debias_plm_module.py:94-146) on the
    joined rows [N_hist + N_cand, D], history first -> (bias-free ragged scores, combined ragged scores, loss_orth, cand_off, Cmax, the
    classes of all rows).  The sentiment encoder is its class table [C, D]; the [N, D] sentiment rows are never formed."""
    ops = train if torch.is_grad_enabled() else hip
    table = train.class_table(sentiment_encoder.embedding_layer.weight, sentiment_encoder.linear.weight, sentiment_encoder.linear.bias)
    hist_off = segment_offsets(batch["batch_hist"], nb)
    cand_off = segment_offsets(batch["batch_cand"], nb)
    s, c_max = _width(batch, "hist_max", hist_off), _width(batch, "cand_max", cand_off)
    hist_vec, cand_vec = rows[:n_hist], rows[n_hist:]
    cls_hist, cls_cand = _debias_classes(batch)
    cls = torch.cat((cls_hist, cls_cand))
    dense_of = train.to_dense if torch.is_grad_enabled() and rows.requires_grad else hip.to_dense
    user_free = user_encoder(dense_of(hist_vec, hist_off, s))
    user_aware = user_encoder(ops.class_dense(table, cls_hist, hist_off, s))
    cand_dense = dense_of(cand_vec, cand_off, c_max)
    dot = train.dot if torch.is_grad_enabled() and (user_free.requires_grad or cand_dense.requires_grad) else hip.dot
    free = dot(user_free.unsqueeze(1), cand_dense.permute(0, 2, 1)).reshape(-1).index_select(0, train.dense_slots(cand_off, cand_vec.shape[0], c_max))
    combined = free + ops.class_scores(user_aware, table, cls_cand, cand_off)
    orth = ops.orth_loss(rows, n_hist, table, cls, user_free, user_aware)
    return free, combined, orth, cand_off, c_max, cls


def _discriminator_params(discriminator):
    p = (discriminator.linear1.weight, discriminator.linear1.bias, discriminator.linear2.weight, discriminator.linear2.bias)
    return p if torch.is_grad_enabled() else tuple(t.detach() for t in p)


def senti_debias_forward(news_encoder, user_encoder, sentiment_encoder, batch: Dict, dense: bool = True):
    """SentiDebias's Generator.forward (reference baselines/senti_debias_plm_module.py:85-148) -> (combined_scores, bias_free_scores,
    loss_orth, clicked_news_vector, candidate_news_vector): the two news-encoder calls on ``batch["x_hist"]["text"]`` /
    ``batch["x_cand"]["text"]``, ``user_encoder`` (the NRMSUserEncoder of this package) once on the dense history and once on the dense
    sentiment rows (``class_dense`` of the class table), the three orthogonality terms (``orth_loss``), DotProduct, and the bias-aware
    scores from the [B, C] products (``class_scores``).  ``sentiment_encoder`` is the module's own SentimentEncoder (``embedding_layer``,
    ``linear``).  Scores are [B, Cmax] with padded slots exactly 0, or the ragged [sum c_i] vectors with ``dense=False``.  No host
    synchronisation when the batch carries ``hist_max`` / ``cand_max``."""
    nb = batch["users"].numel() if "users" in batch and batch["users"] is not None else int(batch["batch_cand"].max()) + 1
    hip.status_poll(batch["batch_cand"].device)
    hist_vec = news_encoder(batch["x_hist"]["text"])
    cand_vec = news_encoder(batch["x_cand"]["text"])
    n_hist = hist_vec.shape[0]
    rows = torch.cat((hist_vec, cand_vec))                        # the operators take the rows as one block, history first
    free, combined, orth, cand_off, c_max, _ = _debias_lines(rows, n_hist, user_encoder, sentiment_encoder, batch, nb)
    hip.status_arm(rows.device)
    if dense:
        free, combined = _miner_dense(free, cand_off, c_max), _miner_dense(combined, cand_off, c_max)
    return combined, free, orth, hist_vec, cand_vec


def senti_debias_generator_step(news_encoder, user_encoder, sentiment_encoder, discriminator, batch: Dict, alpha: float, beta: float):
    """The generator half of SentiDebiasPLMModule.training_step (reference baselines/senti_debias_plm_module.py:339-343):
    ``CrossEntropyLoss(combined_scores, y_true) + beta * loss_orth - alpha * (adversarial_loss(history) + adversarial_loss(candidates))``
    with both news sets through ONE encoder call, the cross-entropy from the ragged combined scores
    (``train.model_step_loss(supcon=False, c_max=...)``) and the discriminator with its loss as ``adv_loss`` on the rows as they lie.
    ``discriminator`` is the module's own (``linear1``, ``linear2``); frozen by ``toggle_optimizer`` it receives no gradient and only the
    rows' is formed.  Returns (g_loss, bias-free ragged scores [sum c_i] detached, cand_off) — ``manual_backward``, the two optimisers,
    the logging and the metrics stay the caller's.  Under ``torch.no_grad()`` the same kernels run without saving anything.  No host
    synchronisation when the batch carries ``hist_max`` / ``cand_max``."""
    nb = batch["users"].numel() if "users" in batch and batch["users"] is not None else int(batch["batch_cand"].max()) + 1
    hip.status_poll(batch["batch_cand"].device)
    rows, n_hist = _encode_joined(news_encoder, batch["x_hist"]["text"], batch["x_cand"]["text"])
    free, combined, orth, cand_off, c_max, cls = _debias_lines(rows, n_hist, user_encoder, sentiment_encoder, batch, nb)
    ce, _ = train.model_step_loss(combined, batch["labels"].to(torch.float32), cand_off, supcon=False, c_max=c_max)
    adv = (train.adv_loss if torch.is_grad_enabled() else hip.adv_loss)(rows, n_hist, *_discriminator_params(discriminator), cls)
    hip.status_arm(rows.device)
    return ce + float(beta) * orth - float(alpha) * adv, free.detach(), cand_off


def senti_debias_discriminator_step(news_encoder, discriminator, batch: Dict):
    """The discriminator half of SentiDebiasPLMModule.training_step (reference baselines/senti_debias_plm_module.py:353-355): the news
    rows re-encoded under the generator's updated weights — ONE encoder call, alone: the reference's second generator pass also runs the
    user encoders, the scores and the orthogonality terms, which nothing reads there — detached, and ``d_loss`` = ``adv_loss`` over
    them with gradients into the discriminator's four parameters only."""
    hip.status_poll(batch["batch_cand"].device)
    rows, n_hist = _encode_joined(news_encoder, batch["x_hist"]["text"], batch["x_cand"]["text"])
    cls = torch.cat(_debias_classes(batch))
    loss = (train.adv_loss if torch.is_grad_enabled() else hip.adv_loss)(rows.detach(), n_hist, *_discriminator_params(discriminator), cls)
    hip.status_arm(rows.device)
    return loss


def a_train_step(news_encoder, batch: Dict, temperature: float = 0.1):
    """AModule.model_step for training (a_module.py:102-108): news embeddings in train() mode and the supervised contrastive
    loss over their aspect labels, both with autograd on the HIP engine.  Returns (loss, embeddings detached)."""
    emb = news_encoder(batch["news"])
    loss, _ = train.supcon_embedding_loss(emb, batch["labels"], temperature=temperature)
    return loss, emb.detach()


def ensemble_forward(news_encoders: Sequence, batch: Dict, weights: Sequence[float], dense: bool = True) -> Tensor:
    """EnsembleModule.forward: CR scores + weighted A-module scores, each z-normalised per impression.
    ``news_encoders[0]`` is the CR-Module's encoder; a zero weight skips that module's encoder entirely
    (ensemble_module.py:100,105).  ``dense=True`` returns the reference's [B, Cmax] matrix slot for slot: its z-score
    runs over the whole zero-padded row (ensemble_module.py:145-149), so PADDED slots hold
    ``sum_k w_k (0 - mean_k) / std_k`` rather than 0 (the reference's consumers mask them away; they are reproduced
    here so that the output is identical, not merely equivalent)."""
    nb = batch["users"].numel()
    hip.status_poll(batch["users"].device)
    hist_off = segment_offsets(batch["batch_hist"], nb)
    cand_off = segment_offsets(batch["batch_cand"], nb)
    planes, used = [], []
    for k, enc in enumerate(news_encoders):
        if k > 0 and weights[k - 1] == 0:
            continue
        planes.append(_late_fusion_ragged(enc(batch["x_hist"]), enc(batch["x_cand"]), hist_off, cand_off))
        if k > 0:
            used.append(weights[k - 1])
    hip.status_arm(cand_off.device)
    if not dense:
        return hip.zscore_fuse(torch.stack(planes), used, cand_off)
    fused, pad = hip.zscore_fuse(torch.stack(planes), used, cand_off, with_pad_value=True)
    return hip.to_dense(fused, cand_off, _width(batch, "cand_max", cand_off), fill=pad)


# ------------------------------------------------------------------------------------- table mode

def encode_table(encoder: hip.HipEncoder, ids: Tensor, mask: Tensor, precision: str = "bf16",
                 host_lengths: Optional[np.ndarray] = None, max_chunk_tokens: int = 65536,
                 out: Optional[Tensor] = None) -> Tensor:
    """Encode a (shard of the) news pool once: [N, Lp] tokens -> [N, D] float32 table rows."""
    return encoder.encode_cls(ids, mask, precision=precision, host_lengths=host_lengths,
                              max_chunk_tokens=max_chunk_tokens, out=out)


def score_impressions(tables: Sequence[Tensor], imp: Dict[str, Tensor], weights: Sequence[float] = (),
                      labels: Optional[Tensor] = None, k: int = 10, fused: Optional[bool] = None) -> Dict[str, Tensor]:
    """Score impressions against per-module tables, fuse, rank.  ``imp``: hist_idx/cand_idx int32,
    hist_off/cand_off int64 (device).  With a single table and no weights the scores are the raw
    late-fusion dot products (CRModule.forward); otherwise the ensemble's z-scored fusion.
    ``fused``: SURVEY §8e phase C as ONE launch (``hip.score_fuse_rank``: float32 tables with D = 768 / 1024, the K score planes stay in
    LDS) or as K scorer launches -> ``zscore_fuse`` -> ``rank_ndcg``; the two give the same bits.  Default (MANNER_PHASE_C=auto): one
    launch for one or two tables or tables that fit the Infinity Cache together, separate launches otherwise; MANNER_PHASE_C=fused /
    separate force either."""
    import os
    hip.status_poll(tables[0].device)                 # an out-of-range news index of an earlier call raises here (IndexError in the reference)
    can_fuse = all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] in (768, 1024) for t in tables) \
        and 1 <= len(tables) <= 9
    if fused is None:
        # One launch wins for one or two tables (K = 1: 0.99 vs 1.13 ms MIND-small, 5.8 vs 7.0 ms on the 660 MB roberta-large table;
        # K = 2: 1.82 vs 1.91 ms) and for tables that stay cache-resident together; with three 495 MB tables it interleaves 1.5 GB of row
        # gathers per impression where the separate launches sweep ONE table at a time through the 256 MiB Infinity Cache: 15.0 vs 13.6 ms
        # for the MIND-large dev set (profiles/r4_final/bench_config3.json) — so the default follows the footprint.
        env = os.environ.get("MANNER_PHASE_C", "auto")
        small = len(tables) <= 2 or sum(t.numel() * 4 for t in tables) <= 256 * 2 ** 20
        fused = can_fuse and env != "separate" and (env == "fused" or small)
    if fused:
        if not can_fuse:
            raise ValueError("score_impressions(fused=True): float32 tables with D = 768 or 1024 only")
        res = hip.score_fuse_rank(tables, list(weights), imp["hist_idx"], imp["hist_off"], imp["cand_idx"], imp["cand_off"], labels=labels, k=k)
        hip.status_arm(tables[0].device)
        return res
    planes = []
    for j, t in enumerate(tables):
        if j > 0 and weights[j - 1] == 0:
            continue
        planes.append(hip.score_late_fusion(t, imp["hist_idx"], imp["hist_off"], imp["cand_idx"], imp["cand_off"]))
    hip.status_arm(tables[0].device)
    if len(tables) == 1 and len(weights) == 0:
        scores = planes[0]
    else:
        scores = hip.zscore_fuse(torch.stack(planes), [w for w in weights if w != 0], imp["cand_off"])
    topk, ndcg, mrr = hip.rank_ndcg(scores, labels, imp["cand_off"], k, with_mrr=True)
    return {"scores": scores, "topk": topk, "ndcg": ndcg, "mrr": mrr}


# ------------------------------------------------------------------------------------- epoch-end metrics

def epoch_end_metrics(scores: Tensor, labels: Tensor, cand_off: Tensor, *, cand_categories: Optional[Tensor] = None,
                       cand_sentiments: Optional[Tensor] = None, hist_categories: Optional[Tensor] = None,
                       hist_sentiments: Optional[Tensor] = None, hist_off: Optional[Tensor] = None,
                       num_categ_classes: int = 19, num_sent_classes: int = 4, with_auc_mrr: bool = True,
                       prefix: str = "test/") -> Dict[str, Tensor]:
    """What ``on_test_epoch_end`` logs, from the ragged epoch tensors and entirely on the device:

    * CRModule (cr_module.py:78-87, 264-273): ``auc``, ``mrr``, ``ndcg@5``, ``ndcg@10``;
    * EnsembleModule (ensemble_module.py:50-84, 214-252): ``ndcg@5/10`` plus, when the aspect tensors are given,
      ``categ_div@5/10``, ``sent_div@5/10`` (manner/metrics/functional.py:8-28) and ``categ_pers@5/10``,
      ``sent_pers@5/10`` (:31-62).
    Retrieval metrics are means over impressions; AUC is one curve over all pairs (hip.auc).  Keys carry ``prefix``.
    """
    out: Dict[str, Tensor] = {}
    tops = {}
    for k in (5, 10):
        topk, ndcg, mrr = hip.rank_ndcg(scores, labels, cand_off, k, with_mrr=True)
        tops[k] = topk
        out[f"{prefix}ndcg@{k}"] = ndcg.mean()
        if k == 10 and with_auc_mrr:
            out[f"{prefix}mrr"] = mrr.mean()
    if with_auc_mrr:
        out[f"{prefix}auc"] = hip.auc(scores, labels)
    for name, cand, hist, classes in (("categ", cand_categories, hist_categories, num_categ_classes),
                                      ("sent", cand_sentiments, hist_sentiments, num_sent_classes)):
        if cand is None:
            continue
        for k in (5, 10):
            div, pers = hip.aspect_metrics(tops[k], cand.to(torch.int32), cand_off, classes,
                                           None if hist is None else hist.to(torch.int32), hist_off)
            out[f"{prefix}{name}_div@{k}"] = div.mean()
            if pers is not None:
                out[f"{prefix}{name}_pers@{k}"] = pers.mean()
    return out
