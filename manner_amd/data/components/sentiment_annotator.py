"""``SentimentAnnotator`` — the reference's news-pool sentiment labelling (manner/data/components/sentiment_annotator.py:9-38) on the HIP
encoder: the XLM-R / RoBERTa / BERT backbone through ``hip.HipEncoder.encode_cls`` and the classifier, softmax, argmax and score rule
in one launch of ``hip.seqcls_head`` (csrc/seqcls.hip).

The reference fetches tokenizer, config and checkpoint from the hub by name.  There is no hub access here: ``sentiment_model`` is a local
HF directory, or the three are handed in (``tokenizer=``, ``config=``, ``state_dict=``).  ``forward(text)`` keeps the reference's
signature and return; ``annotate(titles)`` is the batched call that a whole news pool wants:

    annotator = SentimentAnnotator("/models/twitter-xlm-roberta-base-sentiment")
    classes, scores = annotator.annotate(news["title"].tolist())
    s2i = annotator.sentiment2index(classes)            # the reference's first-appearance map (mind_dataframe.py:210-211)
    sentiment = np.array([s2i[c] for c in classes])     # with `scores`: the sentiment / sentiment_score arrays of the news table
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from ... import hip
from ...config import EncoderConfig, from_hf_dict
from ...weights import split_sequence_classifier

PRECISIONS = ("f16x3", "fp32", "f16", "bf16")


def _encoder_config(config) -> EncoderConfig:
    if isinstance(config, EncoderConfig):
        return config
    return from_hf_dict(config if isinstance(config, dict) else config.to_dict())


def _id2label(config, num_labels: int) -> Dict[int, str]:
    raw = config.get("id2label") if isinstance(config, dict) else getattr(config, "id2label", None)
    if not raw:
        return {i: f"LABEL_{i}" for i in range(num_labels)}
    out = {int(k): str(v) for k, v in raw.items()}
    if sorted(out) != list(range(num_labels)):
        raise ValueError(f"SentimentAnnotator: id2label {out} does not name the {num_labels} classes of the checkpoint")
    return out


class SentimentAnnotator(nn.Module):
    """reference sentiment_annotator.py:9-38.  The two positional arguments are the reference's; the keyword-only ones hand in what the
    reference downloads: ``tokenizer`` (a callable with the HF tokenizer's call signature), ``config`` (an HF config object, or the dict of its
    ``config.json``, with ``id2label``), ``state_dict`` (a ``*ForSequenceClassification``
    state dict, see ``weights.split_sequence_classifier``).  ``precision``: the encoder's arithmetic — "f16x3" (the default: the parity
    grade a ``trainer.precision=32`` run gets; a backbone whose sizes are not multiples of 256 takes "fp32", as MannerTextEncoder does),
    "fp32", "f16" or "bf16".  The head always runs in f32."""

    def __init__(self, sentiment_model: str = "cardiffnlp/twitter-xlm-roberta-base-sentiment", tokenizer_max_length: int = 96, *,
                 tokenizer=None, config=None, state_dict=None, device=None, precision: Optional[str] = None) -> None:
        super().__init__()
        self.tokenizer_max_length = int(tokenizer_max_length)
        if precision is not None and precision not in PRECISIONS:
            raise ValueError(f"SentimentAnnotator: precision {precision!r} is not one of {PRECISIONS}")
        local = isinstance(sentiment_model, str) and os.path.isdir(sentiment_model)
        if not local and (config is None or state_dict is None):
            raise ValueError(
                f"sentiment model {sentiment_model!r} is not a local HF directory and no config= / state_dict= was handed in; "
                "there is no hub access in this build")
        if local:
            if config is None:
                with open(os.path.join(sentiment_model, "config.json")) as f:
                    config = json.load(f)
            if state_dict is None:
                state_dict = self._load_state_dict(sentiment_model)
            if tokenizer is None:
                from transformers import AutoTokenizer
                tokenizer = AutoTokenizer.from_pretrained(sentiment_model, model_max_length=self.tokenizer_max_length, local_files_only=True)
        self.tokenizer = tokenizer
        self.config = config
        self.encoder_config = _encoder_config(config)
        plm, head = split_sequence_classifier(state_dict)
        num_labels = int(head["out.weight"].shape[0])
        self.id2label = _id2label(config, num_labels)
        names = [self.id2label[i] for i in range(num_labels)]
        self.pos_idx = names.index("positive") if "positive" in names else -1
        self.neg_idx = names.index("negative") if "negative" in names else -1
        cfg = self.encoder_config
        tiles = cfg.hidden % 256 == 0 and cfg.intermediate % 256 == 0
        self.precision = precision if precision is not None else ("f16x3" if tiles else "fp32")
        self.device = torch.device(device if device is not None else "cuda")
        self._encoder = hip.HipEncoder(cfg, {k: torch.as_tensor(v) for k, v in plm.items() if not k.startswith("pooler.")},
                                       precisions=(self.precision,), device=self.device)
        for k, v in head.items():
            self.register_buffer("head_" + k.replace(".", "_"), torch.as_tensor(v).detach().to(device=self.device, dtype=torch.float32).contiguous())

    @staticmethod
    def _load_state_dict(path: str):
        st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
        if os.path.exists(st):
            from safetensors.torch import load_file
            return load_file(st)
        if os.path.exists(pt):
            return torch.load(pt, map_location="cpu", weights_only=True)
        raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {path}")

    # ------------------------------------------------------------------ device
    def annotate_tokens(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Device tensors in, device tensors out, no host read: ``label_id`` int32 [N], ``score`` f32 [N], ``probs`` f32 [N, L].  One
        ``encode_cls`` (which chunks the rows as ``hotpath.encode_table`` does) and one head launch over its [CLS] rows."""
        cls = self._encoder.encode_cls(input_ids, attention_mask, precision=self.precision)
        label, score, probs = hip.seqcls_head(cls, self.head_dense_weight, self.head_dense_bias, self.head_out_weight, self.head_out_bias,
                                              self.pos_idx, self.neg_idx, with_probs=True)
        return {"label_id": label, "score": score, "probs": probs}

    def _tokens(self, enc) -> Tuple[torch.Tensor, torch.Tensor]:
        ids, mask = enc["input_ids"], enc["attention_mask"]
        return (torch.as_tensor(ids).to(device=self.device, dtype=torch.int64), torch.as_tensor(mask).to(device=self.device, dtype=torch.int64))

    # ------------------------------------------------------------------ the reference's call
    def forward(self, text: str) -> Tuple[str, float]:
        encoded_input = self.tokenizer(text, return_tensors='pt', padding=True, truncation=True)
        out = self.annotate_tokens(*self._tokens(encoded_input))
        label_id = int(out["label_id"][0])
        if label_id < 0:
            raise FloatingPointError("SentimentAnnotator: non-finite logits")
        return (self.id2label[label_id], float(out["score"][0]))

    # ------------------------------------------------------------------ the batched call
    def annotate(self, titles: Sequence[str], batch_size: int = 4096) -> Tuple[List[str], np.ndarray]:
        """(classes, scores) of all titles: tokenized per chunk of ``batch_size`` with padding and truncation at ``tokenizer_max_length``,
        one ``annotate_tokens`` per chunk, one host read at the end."""
        titles = list(titles)
        labels, scores = [], []
        for i in range(0, len(titles), int(batch_size)):
            enc = self.tokenizer(titles[i:i + int(batch_size)], return_tensors='pt', padding=True, truncation=True,
                                 max_length=self.tokenizer_max_length)
            out = self.annotate_tokens(*self._tokens(enc))
            labels.append(out["label_id"])
            scores.append(out["score"])
        if not labels:
            return [], np.zeros((0,), np.float32)
        label_id = torch.cat(labels).cpu().numpy()
        if (label_id < 0).any():
            raise FloatingPointError(f"SentimentAnnotator: non-finite logits at title {int(np.argmax(label_id < 0))}")
        return [self.id2label[int(a)] for a in label_id], torch.cat(scores).cpu().numpy()

    @staticmethod
    def sentiment2index(classes: Sequence[str]) -> Dict[str, int]:
        """The reference's map (mind_dataframe.py:210-211: ``drop_duplicates().reset_index(drop=True)``, then ``{v: k + 1}``): classes
        numbered from 1 in order of first appearance."""
        out: Dict[str, int] = {}
        for c in classes:
            if c not in out:
                out[c] = len(out) + 1
        return out
