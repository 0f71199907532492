#!/usr/bin/env python3
"""Time the assembly of one training batch, negative sampling included ("train collate").

Three ways to turn B impressions into a sampled MINDRecBatch on the GPU, on MIND-shaped synthetic impressions
(manner_amd/synth.py: up to 50 history and 300 candidate news per impression, titles of up to 96 tokens):

  device        DeviceTrainCollate, default mode: sampling and collate on the device, no device-to-host read
  device_exact  DeviceTrainCollate(exact_width=True): one synchronising read of the sampled batch's widths per call
  host_sampled  what the repository offered before: the impressions are sampled on the host (the numpy restatement of the same
                rule, tests/train_sample_ref.py), uploaded as a data set of their own, and collated by DeviceCollate from a
                non-contiguous index list.  Its figure is the sum of three parts, reported separately: sampling, the per-epoch
                construction of the DeviceCollate (both divided by the batches of the epoch) and the collate call.

Every variant ends in a device synchronise inside its timed window; the variants alternate round by round, each round times
``--iters`` batches, and the median round is reported with the spread.  Writes one JSON file.

    python tools/train_collate_probe.py --out profiles/train_collate/probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from manner_amd import hip                                                                    # noqa: E402
from manner_amd.config import PRESETS                                                         # noqa: E402
from manner_amd.data.components.mind_rec_dataset import (DeviceCollate, DeviceTrainCollate, NewsStore,  # noqa: E402
                                                        ParsedBehaviors, click_counts)
from manner_amd.synth import synth_impressions, synth_news_tokens                             # noqa: E402
from train_sample_ref import sample                                                           # noqa: E402


def build_world(n_news, n_imp, seed, max_len, dev):
    cfg = PRESETS["bert-base"] if "bert-base" in PRESETS else PRESETS["tiny-bert"]
    ids, mask = synth_news_tokens(n_news, cfg, seed=seed, max_len=max_len)
    store = NewsStore.from_arrays(ids.astype(np.int32), mask.sum(1).astype(np.int32), cfg.pad_id, device=dev)
    imp = synth_impressions(n_imp, n_news, seed=seed, max_hist=50, max_cand=300)
    bhv = ParsedBehaviors(users=np.arange(n_imp, dtype=np.int64), hist_rows=imp["hist_idx"].astype(np.int32),
                          hist_off=imp["hist_off"].astype(np.int64), cand_rows=imp["cand_idx"].astype(np.int32),
                          cand_off=imp["cand_off"].astype(np.int64), labels=imp["labels"].astype(np.float32))
    p, q = click_counts(bhv)
    usable = np.flatnonzero((p > 0) & (q > 0))                     # an impression of clicks only cannot be sampled (the reference raises)
    return store, bhv, usable


def host_sampled_epoch(store, bhv, order, ratio, seed, epoch):
    """The epoch's impressions (in ``order``) with sampled candidate lists, as a data set of its own -> (ParsedBehaviors, seconds)."""
    t0 = time.perf_counter()
    hist, cand, labs = [], [], []
    for i in order:
        beg, end = int(bhv.cand_off[i]), int(bhv.cand_off[i + 1])
        s = beg + sample(bhv.labels[beg:end], ratio, seed, epoch, int(i))
        cand.append(bhv.cand_rows[s])
        labs.append(bhv.labels[s])
        hist.append(bhv.hist_rows[bhv.hist_off[i]:bhv.hist_off[i + 1]])
    off = lambda parts: np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    out = ParsedBehaviors(users=bhv.users[order], hist_rows=np.concatenate(hist), hist_off=off(hist), cand_rows=np.concatenate(cand),
                          cand_off=off(cand), labels=np.concatenate(labs))
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--news", type=int, default=20000)
    ap.add_argument("--impressions", type=int, default=2048)
    ap.add_argument("--max-len", type=int, default=96, help="tokenizer_max_length")
    ap.add_argument("--ratio", type=int, default=4)
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--iters", type=int, default=50, help="batches per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_collate", "probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_collate_probe: no GPU — this measurement has no CPU form")
    dev = "cuda:0"
    store, bhv, usable = build_world(args.news, args.impressions, args.seed, args.max_len, dev)
    result = {"device": torch.cuda.get_device_name(0), "news": args.news, "impressions": int(usable.size), "max_len": args.max_len,
              "ratio": args.ratio, "iters_per_round": args.iters, "rounds": args.rounds, "batch": {}}
    for nb in args.batch_sizes:
        n_batches = args.iters
        order = np.random.default_rng(args.seed).permutation(usable)[:nb * n_batches]
        assert order.size == nb * n_batches, "raise --impressions or lower --iters"
        loose = DeviceTrainCollate(store, bhv, neg_sampling_ratio=args.ratio, seed=args.seed)
        exact = DeviceTrainCollate(store, bhv, neg_sampling_ratio=args.ratio, seed=args.seed, exact_width=True)
        order_d = loose.upload_order(order)
        order_e = exact.upload_order(order)
        shuffled = np.random.default_rng(args.seed + 1).permutation(order.size)    # a DataLoader shuffles the pre-sampled epoch

        def run_device(c, od):
            for k in range(n_batches):
                c(od[k * nb:(k + 1) * nb])
            torch.cuda.synchronize()

        def run_host(epoch):
            sampled, t_sample = host_sampled_epoch(store, bhv, order, args.ratio, args.seed, epoch)
            t0 = time.perf_counter()
            c = DeviceCollate(store, sampled)
            torch.cuda.synchronize()
            t_build = time.perf_counter() - t0
            t0 = time.perf_counter()
            for k in range(n_batches):
                c(shuffled[k * nb:(k + 1) * nb].tolist())
            torch.cuda.synchronize()
            return t_sample, t_build, time.perf_counter() - t0

        # the three produce the same batch (checked once, outside the timed windows, for the first batch in the epoch's order)
        sampled, _ = host_sampled_epoch(store, bhv, order[:nb], args.ratio, args.seed, 0)
        want, got = DeviceCollate(store, sampled)(range(0, nb)), exact(order_e[:nb])
        assert torch.equal(want["x_cand"]["text"]["input_ids"], got["x_cand"]["text"]["input_ids"])
        assert torch.equal(want["labels"], got["labels"]) and torch.equal(want["batch_hist"], got["batch_hist"])
        run_device(loose, order_d), run_device(exact, order_e), run_host(0)                 # warm-up of every variant
        times = {"device": [], "device_exact": [], "host_sampled": [], "host_sampling": [], "host_build": [], "host_collate": []}
        for r in range(args.rounds):
            loose.set_epoch(r), exact.set_epoch(r)
            t0 = time.perf_counter()
            run_device(loose, order_d)
            times["device"].append((time.perf_counter() - t0) / n_batches * 1e3)
            t0 = time.perf_counter()
            run_device(exact, order_e)
            times["device_exact"].append((time.perf_counter() - t0) / n_batches * 1e3)
            ts, tb, tc = run_host(r)
            for k, v in (("host_sampling", ts), ("host_build", tb), ("host_collate", tc), ("host_sampled", ts + tb + tc)):
                times[k].append(v / n_batches * 1e3)
        hip.check_status(dev)
        result["batch"][str(nb)] = {k: {"ms_per_batch_median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                       "max": round(max(v), 4)} for k, v in times.items()}
        print(f"B = {nb}: " + ", ".join(f"{k} {statistics.median(v):.3f} ms" for k, v in times.items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
