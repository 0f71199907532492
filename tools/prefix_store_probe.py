#!/usr/bin/env python3
"""Frozen-prefix cache: the token-packed store (hip.PackedPrefixCache) beside the fixed-width table (hip.PrefixCache), same process,
same inputs, alternating.  Run as a fresh process on the GPU:

    python tools/prefix_store_probe.py [--out profiles/prefix_packed/probe.json] [--only calls,kernels,train] [--reps 5]

calls    time per ``hidden_states`` call once every news is stored (all hit): 128 news padded to 512 (title+abstract lengths of
         synth.synth_lengths, seed 42) and 700 news padded to 96 (title lengths).  The fixed-width table gets max_len = the batch
         width, so that it does cache.  Device events around ``--iters`` calls; ``--reps`` windows per form, alternating; the spread
         reported is (max - min) / median over the windows.
kernels  the gather and the store entry points alone (events around back-to-back launches), bytes = real tokens read + padded (gather)
         or real (store) tokens written, against the 8 TB/s HBM figure of DESIGN §4.
train    one training step (encode_train forward + backward) at bert-base, frozen_layers [0..7], embeddings frozen, f16: the prefix
         recomputed every step, from the fixed-width table, from the packed store.

Kernel times by name come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script (``--only calls --reps 1``)."""
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
from manner_amd.synth import synth_lengths, synth_news_tokens  # noqa: E402
from manner_amd.weights import make_plm_weights  # noqa: E402

HBM_TBS = 8.0
SHAPES = (("128_news_padded_512", 128, 512, "title_abstract"), ("700_news_padded_96", 700, 96, "title"))
FIRST = 8                                                    # frozen_layers [0..7]


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def alternate(forms, iters, reps):
    """{name: {median_ms, spread, windows_ms}} of callables timed in alternation."""
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    wins = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            wins[k].append(window(fn, iters))
    out = {}
    for k, w in wins.items():
        med = float(np.median(w))
        out[k] = {"median_ms": round(med, 4), "spread_over_median": round((max(w) - min(w)) / med, 4), "windows_ms": [round(x, 4) for x in w]}
    return out


def batch(cfg, n, width, profile, dev):
    lens = synth_lengths(n, 42, width, profile)
    ids, mask = synth_news_tokens(n, cfg, seed=42, lengths=lens, pad_to=width)
    return torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_packed", "probe.json"))
    ap.add_argument("--only", default="calls,kernels,train")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--train-iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    only = a.only.split(",")
    dev = torch.device("cuda", 0)
    cfg = PRESETS["bert-base-uncased"]
    w = make_plm_weights(cfg, seed=1, std=0.02, with_pooler=False)
    engine = hip.HipEncoder(cfg, w, precisions=("f16",), device=dev)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "one box", "hbm_TBs_assumed": HBM_TBS, "iters_per_window": a.iters,
           "windows_per_form": a.reps}
    lib = _lib.load()
    for name, n, width, profile in SHAPES:
        ids, mask, lens = batch(cfg, n, width, profile, dev)
        tokens = int(lens.sum())
        row = res[name] = {"news": n, "padded_len": width, "real_tokens": tokens,
                           "packed_bytes": hip.prefix_cache_bytes(cfg.hidden, n, pool_tokens=tokens)["total"],
                           "padded_bytes": hip.prefix_cache_bytes(cfg.hidden, n, max_len=width)["total"]}
        packed = hip.PackedPrefixCache(cfg.hidden, n, tokens, dev)
        padded = hip.PrefixCache(cfg.hidden, width, n, dev)
        ref = engine.encode_hidden(ids, mask, FIRST, precision="f16")
        for c in (packed, padded):
            c.hidden_states(engine, ids, mask, FIRST, "f16")
            assert torch.equal(c.hidden_states(engine, ids, mask, FIRST, "f16"), ref) and c.encoded == n      # all hit, same bits
        if "calls" in only:
            row["hidden_states_all_hit"] = alternate({"packed": lambda: packed.hidden_states(engine, ids, mask, FIRST, "f16"),
                                                      "padded": lambda: padded.hidden_states(engine, ids, mask, FIRST, "f16")}, a.iters, a.reps)
            assert packed.encoded == n and padded.encoded == n
        if "kernels" in only:
            rows, state = packed.lookup(ids, mask)
            out = torch.empty((n, width, cfg.hidden), dtype=torch.float32, device=dev)
            P = hip._ptr

            def gather():
                _lib.check(lib.manner_hip_prefix_gather(P(rows), P(state), n, width, cfg.hidden, P(packed.pool), packed.pool_tokens,
                                                        packed.capacity, P(packed.row_off), P(packed.row_len), P(packed.row_src), None, 0,
                                                        None, P(out), hip._stream()))
            calls = 3 + a.iters * a.reps
            big = hip.PackedPrefixCache(cfg.hidden, n, tokens * calls, dev)        # every store call reserves its tokens anew
            lens32 = mask.sum(1, dtype=torch.int32)
            ones = torch.ones(n, dtype=torch.int32, device=dev)
            rows_id = torch.arange(n, dtype=torch.int32, device=dev)
            src_of = torch.empty(n, dtype=torch.int32, device=dev)

            def store():
                _lib.check(lib.manner_hip_prefix_store(P(ref), n, None, n, P(rows_id), P(ones), P(lens32), width, cfg.hidden, P(big.pool),
                                                       big.pool_tokens, big.capacity, P(big.row_off), P(big.row_len), P(big.row_src),
                                                       P(big.tok_count), P(src_of), hip._stream()))
            k = alternate({"gather": gather, "store": store}, a.iters, a.reps)
            assert torch.equal(out, ref) and int(big.tok_count.item()) == tokens * calls
            real, pad = tokens * cfg.hidden * 4, n * width * cfg.hidden * 4
            for nm, moved in (("gather", real + pad), ("store", 2 * real)):
                k[nm]["bytes_moved"] = moved
                k[nm]["TBs"] = round(moved / (k[nm]["median_ms"] * 1e-3) / 1e12, 3)
                k[nm]["fraction_of_hbm"] = round(k[nm]["TBs"] / HBM_TBS, 3)
            row["kernels"] = k
            del big
        if "train" in only:
            frozen = {key for key in w if key.startswith("embeddings.") or any(f"layer.{l}." in key for l in range(FIRST))}
            params = {key: torch.from_numpy(v).to(dev).requires_grad_(key not in frozen) for key, v in w.items()}
            R = torch.randn((n, cfg.hidden), device=dev)

            def step(cache):
                def run():
                    for p in params.values():
                        p.grad = None
                    extra = {}
                    if cache is not None:
                        with torch.no_grad():
                            extra = dict(start_layer=FIRST, prefix_hidden=cache.hidden_states(engine, ids, mask, FIRST, "f16"))
                    o = train.encode_train(cfg, params, ids, mask, precision="f16", seed=3, prefix_engine=engine, max_len=_lib.MAX_LEN_TRAIN,
                                           token_bound=tokens, **extra)
                    (o * R).sum().backward()
                    return o
                return run
            forms = {"no_cache": step(None), "padded_cache": step(padded), "packed_store": step(packed)}
            outs = {key: fn().detach().clone() for key, fn in forms.items()}
            assert torch.equal(outs["no_cache"], outs["padded_cache"]) and torch.equal(outs["no_cache"], outs["packed_store"])
            row["train_step_f16_frozen_0_7"] = alternate(forms, a.train_iters, a.reps)
            del params
        del packed, padded
        torch.cuda.empty_cache()
        print(json.dumps({name: row}), flush=True)
    hip.check_status(dev)
    engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
