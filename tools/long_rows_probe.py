#!/usr/bin/env python3
"""Cost of long news (up to 512 tokens) in the inference engine: encode_cls at the bert-base shape over uniform rows of 96 / 128 / 256 /
384 / 512 tokens, about 65 k tokens per call.  Run as a fresh process:

    python tools/long_rows_probe.py [--precisions f16,bf16,fp32] [--lengths 96,128,256,384,512] [--out FILE]

Per (precision, row length): µs per token of the whole call (CUDA events around `--iters` calls, the default two-stream schedule) and,
from one call under the encoder's per-launch profiling (HIP events around each launch, streams serialised), the attention launches'
time — 11 full layers (short-row kernel + long-row kernel; rows > 128 tokens run only the latter) plus the last layer's [CLS] attention
— with the effective rate of the full layers, 4 L^2 H FLOPs per news per layer (QK^T and PV)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from manner_amd import hip  # noqa: E402
from manner_amd.config import PRESETS  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from manner_amd.weights import make_plm_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="f16,bf16")
    ap.add_argument("--lengths", default="96,128,256,384,512")
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = PRESETS["bert-base-uncased"]
    dev = torch.device("cuda", 0)
    precs = a.precisions.split(",")
    enc = hip.HipEncoder(cfg, make_plm_weights(cfg, seed=1, std=0.02), precisions=tuple(precs), device=dev)
    rows = []
    for L in [int(x) for x in a.lengths.split(",")]:
        n = a.tokens // L
        ids_np, mask_np = synth_news_tokens(n, cfg, seed=L, lengths=[L] * n)
        ids, mask = torch.from_numpy(ids_np).to(dev), torch.from_numpy(mask_np).to(dev)
        hl = mask_np.sum(1)
        for prec in precs:
            for _ in range(2):
                enc.encode_cls(ids, mask, precision=prec, host_lengths=hl, max_chunk_tokens=a.tokens)
            enc.status()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                enc.encode_cls(ids, mask, precision=prec, host_lengths=hl, max_chunk_tokens=a.tokens)
            t1.record()
            torch.cuda.synchronize()
            call_ms = t0.elapsed_time(t1) / a.iters
            enc.profile(True)
            enc.profile_read()
            enc.encode_cls(ids, mask, precision=prec, host_lengths=hl, max_chunk_tokens=a.tokens)
            prof = enc.profile_read()
            enc.profile(False)
            enc.status()
            attn_ms, attn_launches = prof["attention"]
            flops = 4.0 * L * L * cfg.hidden * n * (cfg.layers - 1)
            row = {"precision": prec, "L": L, "news": n, "tokens": n * L, "call_ms": round(call_ms, 3),
                   "us_per_token": round(1e3 * call_ms / (n * L), 5), "attention_ms": round(attn_ms, 3),
                   "attention_launches": attn_launches, "attention_pflops": round(flops / (attn_ms * 1e-3) / 1e15, 3),
                   "profiled_call_ms": round(sum(v[0] for v in prof.values()), 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    for prec in precs:
        base = [r for r in rows if r["precision"] == prec and r["L"] == 96]
        for r in rows:
            if base and r["precision"] == prec:
                r["us_per_token_vs_96"] = round(r["us_per_token"] / base[0]["us_per_token"], 3)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    enc.close()


if __name__ == "__main__":
    main()
