#!/usr/bin/env python3
"""Cost of training on long news (up to 512 tokens): one training step of the text encoder (manner_amd.train.encode_train forward +
backward) at the bert-base shape with the reference's frozen_layers [0..7] and trainable embeddings (the gradient crosses every
layer), over uniform rows of 96 / 128 / 256 / 512 tokens at about 64 k tokens per step.  Run as a fresh process:

    python tools/long_train_probe.py [--precisions f16,bf16] [--lengths 96,128,256,512] [--out FILE]

Per (precision, row length): ms per step and µs per token (device events around `--iters` steps after two warm-up steps) and the
ratio of µs per token to the 96-token figure.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this
script (`--iters 1`); `--flops` prints the attention FLOPs per step that the achieved rates divide by: forward 4 L^2 H, backward-q
6 L^2 H, backward-kv 8 L^2 H per news and layer."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from manner_amd import _lib, hip, train  # noqa: E402
from manner_amd.config import PRESETS  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from manner_amd.weights import make_plm_weights  # noqa: E402


def attention_flops(L, n, cfg):
    """{pass: FLOPs of one step} over every layer (all layers run forward and backward: the embeddings train)."""
    per = {"forward": 4.0, "backward_q": 6.0, "backward_kv": 8.0}
    return {k: v * L * L * cfg.hidden * n * cfg.layers for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="f16,bf16")
    ap.add_argument("--lengths", default="96,128,256,512")
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--flops", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = PRESETS["bert-base-uncased"]
    lengths = [int(x) for x in a.lengths.split(",")]
    if a.flops:
        for L in lengths:
            print(json.dumps({"L": L, "news": a.tokens // L, **attention_flops(L, a.tokens // L, cfg)}))
        return
    dev = torch.device("cuda", 0)
    w = make_plm_weights(cfg, seed=1, std=0.02, with_pooler=False)
    frozen = {k for k in w for l in range(8) if f"layer.{l}." in k}
    params = {k: torch.from_numpy(v).to(dev).requires_grad_(k not in frozen) for k, v in w.items()}
    rows = []
    for L in lengths:
        n = a.tokens // L
        ids_np, mask_np = synth_news_tokens(n, cfg, seed=L, lengths=np.full(n, L))
        ids, mask = torch.from_numpy(ids_np).to(dev), torch.from_numpy(mask_np).to(dev)
        R = torch.randn((n, cfg.hidden), device=dev)
        for prec in a.precisions.split(","):
            def step():
                for p in params.values():
                    p.grad = None
                out = train.encode_train(cfg, params, ids, mask, precision=prec, seed=3, max_len=_lib.MAX_LEN_TRAIN,
                                         token_bound=n * L)
                (out * R).sum().backward()
            for _ in range(2):
                step()
            hip.check_status(dev)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                step()
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.iters
            row = {"precision": prec, "L": L, "news": n, "tokens": n * L, "step_ms": round(ms, 3), "us_per_token": round(1e3 * ms / (n * L), 5)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    for r in rows:
        base = [b for b in rows if b["precision"] == r["precision"] and b["L"] == 96]
        if base:
            r["us_per_token_vs_96"] = round(r["us_per_token"] / base[0]["us_per_token"], 3)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
