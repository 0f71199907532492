"""What labelling a MIND-small news pool with sentiment costs -> profiles/sentiment/probe.json.

The ``xlm-roberta-base`` shape with seeded weights, 65 238 synthetic titles of bench.py's title-length distribution
(``synth_news_tokens(profile="title")``), a 3-class head.  Everything is timed in one run, as the median of ``--rounds`` rounds in
which the variants alternate:

  annotate   ``SentimentAnnotator.annotate_tokens`` in f16x3 / f16 / bf16 beside ``encode_cls`` alone on the same tokens: what the head
             adds to the encoder
  head       ``hip.seqcls_head`` alone at N = 64 / 4096 / 65 238 beside the composition the library offered before csrc/seqcls.hip —
             ``hip.linear_tanh`` + ``hip.linear`` + torch softmax / argmax / where — with the achieved fraction of the 157 TF f32
             matrix peak (the dense layer's 2 N H^2 FLOP over the head's time)
  reference  the reference's way: the HF model on 16 CPU threads, one title per call, on 64 titles (random weights of the same shape)

    python tools/sentiment_probe.py [--rounds 9] [--news 65238] [--legs annotate,head,reference] [--out profiles/sentiment/probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]

from aspect_probe import measure  # noqa: E402
from manner_amd import hip  # noqa: E402
from manner_amd.config import PRESETS  # noqa: E402
from manner_amd.data.components.sentiment_annotator import SentimentAnnotator  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from manner_amd.weights import make_plm_weights  # noqa: E402
from sentiment_ref import head_inputs, hf_config_dict  # noqa: E402

DEV = "cuda:0"
ID2LABEL = {0: "negative", 1: "neutral", 2: "positive"}
F32_PEAK = 157e12
SEED = 7


def composed(x, dw, db, ow, ob, pos, neg):
    """the same outputs from the library's older kernels and torch"""
    p = torch.softmax(hip.linear(hip.linear_tanh(x, dw, db), ow, ob), dim=1)
    pa, a = p.max(dim=1)
    score = torch.where(a == pos, pa, torch.where(a == neg, -pa, (1 - pa) * (p[:, -1] - p[:, 0])))
    return a.to(torch.int32), score, p


def annotate_leg(args, cfg, ids, mask):
    w = make_plm_weights(cfg, seed=SEED, std=0.02, with_pooler=False)
    head = head_inputs(1, cfg.hidden, 3, seed=SEED)
    sd = {"roberta." + k: v for k, v in w.items()}
    sd.update({"classifier.dense.weight": head["dense_w"], "classifier.dense.bias": head["dense_b"], "classifier.out_proj.weight": head["out_w"],
               "classifier.out_proj.bias": head["out_b"]})
    out = {}
    for prec in ("f16x3", "f16", "bf16"):
        ann = SentimentAnnotator(config=hf_config_dict(cfg, ID2LABEL), state_dict=sd, device=DEV, precision=prec)
        rec = measure({"annotate_tokens": lambda: ann.annotate_tokens(ids, mask),
                       "encode_cls": lambda: ann._encoder.encode_cls(ids, mask, precision=prec)}, args.rounds, 1, warm=1)
        rec["head_share_of_call"] = round(1 - rec["encode_cls_us"] / rec["annotate_tokens_us"], 5)
        rec["titles_per_s"] = round(ids.shape[0] / rec["annotate_tokens_us"] * 1e6, 1)
        out[prec] = rec
        del ann
        torch.cuda.empty_cache()
    return out


def head_leg(args, cfg):
    h = cfg.hidden
    out = {}
    for n in (64, 4096, args.news):
        inp = {k: torch.from_numpy(v).to(DEV) for k, v in head_inputs(n, h, 3, seed=SEED).items()}
        a = (inp["x"], inp["dense_w"], inp["dense_b"], inp["out_w"], inp["out_b"], 2, 0)
        one, two = hip.seqcls_head(*a), composed(*a)
        agree = float((one[0] == two[0]).float().mean())
        rec = measure({"seqcls_head": lambda: hip.seqcls_head(*a), "composed": lambda: composed(*a)}, args.rounds, 200 if n < 10000 else 20)
        rec["labels_equal_share"] = agree
        rec["score_max_abs_diff"] = float((one[1] - two[1]).abs().max())
        rec["head_over_composed"] = round(rec["seqcls_head_us"] / rec["composed_us"], 3)
        rec["f32_matrix_peak_fraction"] = round(2.0 * n * h * h / (rec["seqcls_head_us"] * 1e-6) / F32_PEAK, 5)
        out[f"N={n}"] = rec
    return out


def reference_leg(cfg, ids, mask, titles=64):
    try:
        from transformers import XLMRobertaConfig, XLMRobertaForSequenceClassification
    except ImportError as e:
        return {"skipped": str(e)}
    torch.set_num_threads(16)
    conf = XLMRobertaConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                            intermediate_size=cfg.intermediate, max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab,
                            layer_norm_eps=cfg.ln_eps, pad_token_id=cfg.pad_id, num_labels=3)
    model = XLMRobertaForSequenceClassification(conf).eval()
    ids, mask = ids[:titles].cpu(), mask[:titles].cpu()
    per = []
    with torch.no_grad():
        for i in range(titles + 4):
            j = i % titles
            n = int(mask[j].sum())
            t0 = time.perf_counter()
            torch.softmax(model(input_ids=ids[j:j + 1, :n], attention_mask=mask[j:j + 1, :n]).logits[0], dim=0).numpy()
            if i >= 4:
                per.append(time.perf_counter() - t0)
    return {"titles": titles, "cpu_threads": 16, "ms_per_title_median": round(float(np.median(per)) * 1e3, 3),
            "titles_per_s": round(titles / float(np.sum(per)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--news", type=int, default=65238)
    ap.add_argument("--legs", default="annotate,head,reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sentiment", "probe.json"))
    args = ap.parse_args()
    cfg = PRESETS["xlm-roberta-base"]
    ids_np, mask_np = synth_news_tokens(args.news, cfg, seed=42, max_len=96, profile="title")
    ids, mask = torch.from_numpy(ids_np).to(DEV), torch.from_numpy(mask_np).to(DEV)
    legs = args.legs.split(",")
    out = {"device": torch.cuda.get_device_name(0), "preset": "xlm-roberta-base", "news": args.news, "tokens": int(mask_np.sum()),
           "padded_length": int(ids_np.shape[1]), "rounds": args.rounds, "labels": 3,
           "method": "median of alternating rounds in one process; wall time around a device synchronise"}
    if "head" in legs:
        out["head"] = head_leg(args, cfg)
    if "annotate" in legs:
        out["annotate"] = annotate_leg(args, cfg, ids, mask)
    if "reference" in legs:
        out["reference"] = reference_leg(cfg, ids, mask)
        if "annotate" in out and "titles_per_s" in out["reference"]:
            out["speedup_over_reference"] = {p: round(r["titles_per_s"] / out["reference"]["titles_per_s"], 1) for p, r in out["annotate"].items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
