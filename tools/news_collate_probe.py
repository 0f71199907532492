#!/usr/bin/env python3
"""Time the assembly of one A-Module training batch, M-per-class sampling included ("news collate").

The reference's A-Module configuration (configs/data/mind_news.yaml:49-50: batch_size 60, samples_per_class 20) over a synthetic
pool of 65 238 news (the size of MIND-small's news set) with titles of up to 96 tokens and up to 8 entities, for the category
aspect (18 classes, skewed) and the sentiment aspect (4 classes):

  device        DeviceNewsTrainSampler.batch(i): slices of the epoch's sample + the collate kernels, no read-back, no upload
  host_indices  the same batches from host-side indices: the numpy restatement of the same rule (tests/news_sample_ref.py), an
                upload of the batch's rows and labels, and the same collate kernels (DeviceNewsCollate over a sequence).  Its two
                parts are reported separately: sampling and collate.
  epoch_launch  sample_epoch(): the one launch pair for the whole epoch and its one synchronising read, per epoch and per batch

Every variant ends in a device synchronise inside its timed window; the variants alternate round by round, each round times
``--iters`` batches (the device variant ``--passes`` times over, the epoch launch ``--epoch-reps`` times, so that no window is
shorter than a tenth of a second or so), and the median of the rounds is reported with the spread.  Writes one JSON file.

    python tools/news_collate_probe.py --out profiles/news_collate/probe.json
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
from manner_amd.data.components.mind_news_dataset import DeviceNewsCollate, DeviceNewsTrainSampler, NewsDataset  # noqa: E402
from manner_amd.data.components.mind_rec_dataset import NewsStore, ParsedBehaviors            # noqa: E402
from manner_amd.synth import synth_news_tokens                                                # noqa: E402
import news_sample_ref as ref                                                                 # noqa: E402


def build_world(n_news, seed, max_len, dev):
    cfg = PRESETS["bert-base"] if "bert-base" in PRESETS else PRESETS["tiny-bert"]
    g = np.random.default_rng(seed)
    ids, mask = synth_news_tokens(n_news, cfg, seed=seed, max_len=max_len)
    store = NewsStore.from_arrays(ids.astype(np.int32), mask.sum(1).astype(np.int32), cfg.pad_id, device=dev)
    counts = g.integers(0, 9, n_news).astype(np.int32)
    ent = np.where(np.arange(8)[None, :] < counts[:, None], g.integers(1, 40000, (n_news, 8)), 0).astype(np.int32)
    p18 = 1.0 / np.arange(1, 19)                                   # a skewed category distribution, every class of 20 or more
    cat = g.choice(18, n_news, p=p18 / p18.sum()).astype(np.int32)
    sent = g.integers(0, 4, n_news).astype(np.int32)
    store.ent_counts = counts
    store.ent_d, store.cnt_d = torch.from_numpy(ent).to(dev), torch.from_numpy(counts).to(dev)
    store.cat_d, store.sent_d = torch.from_numpy(cat).to(dev), torch.from_numpy(sent).to(dev)
    bhv = ParsedBehaviors(users=np.zeros(1, np.int64), hist_rows=np.zeros(0, np.int32), hist_off=np.zeros(2, np.int64),
                          cand_rows=np.arange(n_news, dtype=np.int32), cand_off=np.array([0, n_news], np.int64),
                          labels=np.zeros(n_news, np.float32))
    return store, bhv


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--news", type=int, default=65238)
    ap.add_argument("--max-len", type=int, default=96, help="tokenizer_max_length")
    ap.add_argument("--batch-size", type=int, default=60)
    ap.add_argument("--samples-per-class", type=int, default=20)
    ap.add_argument("--iters", type=int, default=1000, help="batches per pass of a timed round")
    ap.add_argument("--passes", type=int, default=5, help="passes over those batches in a round of the device variant")
    ap.add_argument("--epoch-reps", type=int, default=50, help="epoch launches per timed round")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "news_collate", "probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("news_collate_probe: no GPU — this measurement has no CPU form")
    dev = "cuda:0"
    store, bhv = build_world(args.news, args.seed, args.max_len, dev)
    m, bs, n_it = args.samples_per_class, args.batch_size, args.iters
    result = {"device": torch.cuda.get_device_name(0), "news": args.news, "max_len": args.max_len, "batch_size": bs,
              "samples_per_class": m, "iters_per_round": n_it, "device_passes": args.passes,
              "epoch_launches_per_round": args.epoch_reps, "rounds": args.rounds, "aspect": {}}
    for aspect in ("category", "sentiment"):
        ds = NewsDataset(store, bhv, aspect)
        sampler = DeviceNewsTrainSampler(store, ds, m, bs, seed=args.seed)
        collate = DeviceNewsCollate(store, ds)
        tables = ref.class_tables(ds.labels)
        assert n_it <= len(sampler), "lower --iters"

        def run_device():
            for _ in range(args.passes):
                for i in range(n_it):
                    sampler.batch(i)
            torch.cuda.synchronize()

        def run_host(epoch):
            t0 = time.perf_counter()
            idx = [ref.sample_batch(tables, m, sampler.k, args.seed, epoch, b)[0] for b in range(n_it)]
            t_sample = time.perf_counter() - t0
            t0 = time.perf_counter()
            for b in range(n_it):
                collate(idx[b])
            torch.cuda.synchronize()
            return t_sample, time.perf_counter() - t0

        def run_epoch(epoch, reps=1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for r in range(reps):
                sampler.set_epoch(epoch * reps + r)
                sampler.sample_epoch()                               # ends in its own synchronising read
            return (time.perf_counter() - t0) / reps

        # the two produce the same batch (checked once, outside the timed windows)
        run_epoch(0)
        want, got = collate(ref.sample_batch(tables, m, sampler.k, args.seed, 0, 3)[0]), sampler.batch(3)
        assert torch.equal(want["news"]["text"]["input_ids"], got["news"]["text"]["input_ids"])
        assert torch.equal(want["news"]["entities"], got["news"]["entities"]) and torch.equal(want["labels"], got["labels"])
        run_device(), run_host(0)                                    # warm-up of every variant
        times = {"device": [], "host_indices": [], "host_sampling": [], "host_collate": [], "epoch_launch_per_epoch": [],
                 "epoch_launch": []}
        for r in range(args.rounds):
            te = run_epoch(r + 1, args.epoch_reps)
            times["epoch_launch_per_epoch"].append(te * 1e6)
            times["epoch_launch"].append(te / len(sampler) * 1e6)
            t0 = time.perf_counter()
            run_device()
            times["device"].append((time.perf_counter() - t0) / (n_it * args.passes) * 1e6)
            ts, tc = run_host(r)
            for k, v in (("host_sampling", ts), ("host_collate", tc), ("host_indices", ts + tc)):
                times[k].append(v / n_it * 1e6)
        hip.check_status(dev)
        result["aspect"][aspect] = {"classes": int(ds.class_label.size), "batches_per_epoch": len(sampler),
                                    **{k: {("us_per_epoch_median" if k.endswith("per_epoch") else "us_per_batch_median"):
                                           round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                       for k, v in times.items()}}
        print(f"{aspect}: " + ", ".join(f"{k} {statistics.median(v):.1f} us" for k, v in times.items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
