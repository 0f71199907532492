#!/usr/bin/env python3
"""Cost of the "full rows" path (PLMTextEncoder: every padded position a row of the PLM) on padded batches of up to 512 positions, at
the bert-base shape with about 64 k rows per call: `hip.encode_full` (inference) and one PLMTextEncoder training step (PLM with
autograd over full rows, axis-0 attention, additive pooler; forward + backward) at 96 / 128 / 256 / 512 positions in f16 and bf16,
and at 256 / 512 the same step under MANNER_HIP_TRAIN_ATTN_VALU=1 (the f32 attention kernels' row-block grid).  Run as a fresh process:

    python tools/full_rows_probe.py [--precisions f16,bf16] [--lengths 96,128,256,512] [--rows 65536] [--out profiles/full_rows_long/probe.json]

Every figure is the MEDIAN over `--iters` calls, each bracketed by its own pair of device events, after one warm-up call.  Real-token
counts are uniform in [padded_len / 4, padded_len] (a tokenizer_max_length batch of title + abstract).  The yardstick is the per-row
time at 128 positions, which the commit before this path existed runs with the same kernels: `vs_128` is the ratio to it.
The share of the three long attention kernels is not visible between device events outside the library: it comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/full_rows_probe.py --iters 1 ...` run.  What this script records beside the step
times is `valu_over_pipe`, the whole-step ratio of the VALU run to the matrix-pipe run at the same shape."""
import argparse
import json
import os
import statistics
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from manner_amd import _lib, hip  # noqa: E402
from manner_amd.config import PRESETS  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from manner_amd.weights import make_mha_pool_weights, make_plm_weights  # noqa: E402


def median_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="f16,bf16")
    ap.add_argument("--lengths", default="96,128,256,512")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="truncate the PLM (0 = all 12 layers)")
    ap.add_argument("--no-valu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "full_rows_long", "probe.json"))
    a = ap.parse_args()
    from manner_amd.models.components.news_encoder import PLMTextEncoder
    dev = torch.device("cuda", 0)
    cfg = PRESETS["bert-base-uncased"]
    if a.layers:
        import dataclasses
        cfg = dataclasses.replace(cfg, layers=a.layers)
    PLMTextEncoder.train_max_length = _lib.MAX_LEN_FULL
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = PLMTextEncoder(plm_model="bert-base-uncased", frozen_layers=[], text_embedding_dim=cfg.hidden, num_attention_heads=16,
                             query_vector_dim=200, dropout_probability=0.2)
    if a.layers:
        enc.plm_model = type(enc.plm_model)(cfg)
    sd = {"plm_model." + k: torch.from_numpy(v) for k, v in make_plm_weights(cfg, seed=1, std=0.02).items()}
    sd.update({k: torch.from_numpy(v) for k, v in make_mha_pool_weights(cfg.hidden, 200, seed=1).items()})
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev)
    weights = {k: v.detach() for k, v in enc.plm_model.named_parameters() if not k.startswith("pooler.")}
    rows = []
    for lp in [int(x) for x in a.lengths.split(",")]:
        n = max(1, a.rows // lp)
        lens = np.random.default_rng(lp).integers(max(2, lp // 4), lp + 1, size=n)
        ids_np, mask_np = synth_news_tokens(n, cfg, seed=lp, lengths=lens, pad_to=lp)
        ids, mask = torch.from_numpy(ids_np).to(dev), torch.from_numpy(mask_np).to(dev)
        batch = {"input_ids": ids, "attention_mask": mask}
        for prec in a.precisions.split(","):
            enc.train_precision = prec

            def infer():
                with torch.no_grad():
                    hip.encode_full(cfg, weights, ids, mask, precision=prec)

            def step():
                enc.zero_grad(set_to_none=True)
                enc(batch).square().sum().backward()

            enc.eval()
            row = {"precision": prec, "padded_len": lp, "news": n, "rows": n * lp, "layers": cfg.layers}
            row["encode_full_ms"] = round(median_ms(infer, a.iters), 3)
            enc.train()
            os.environ.pop("MANNER_HIP_TRAIN_ATTN_VALU", None)
            row["train_step_ms"] = round(median_ms(step, a.iters), 3)
            row["matrix_pipe"] = bool(int(_lib.load().manner_hip_train_layout_last()) & 1)
            if lp > _lib.MAX_LEN and not a.no_valu:
                os.environ["MANNER_HIP_TRAIN_ATTN_VALU"] = "1"
                row["train_step_valu_ms"] = round(median_ms(step, a.iters), 3)
                row["encode_full_valu_ms"] = round(median_ms(infer, a.iters), 3)
                os.environ.pop("MANNER_HIP_TRAIN_ATTN_VALU", None)
                row["valu_over_pipe"] = round(row["train_step_valu_ms"] / row["train_step_ms"], 3)
            hip.check_status(dev)
            for k in ("encode_full", "train_step"):
                row[k + "_us_per_row"] = round(1e3 * row[k + "_ms"] / (n * lp), 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
    for r in rows:
        base = [b for b in rows if b["precision"] == r["precision"] and b["padded_len"] == _lib.MAX_LEN]
        if base:
            for k in ("encode_full", "train_step"):
                r[k + "_vs_128"] = round(r[k + "_us_per_row"] / base[0][k + "_us_per_row"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
