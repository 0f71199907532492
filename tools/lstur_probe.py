"""Time per call of the LSTUR baseline's user encoder (csrc/gru.hip through the ``LSTURUserEncoder`` mirror) beside the float32 torch
composition the reference runs — the embedding, ``hist_size.cpu()``, ``pack_padded_sequence(enforce_sorted=False)`` and ``nn.GRU``
(MIOpen) on the packed input — on the same device, forward (eval, no_grad) and forward + backward (train(), the user mask at the shipped
p = 0.5 on both sides), at the shipped widths (S = 50, I = 768 + 100 = 868;
``ini``: H = 868, ``con``: H = 434) for B = 8 and 64 users, histories of 1 .. 50 clicks.

Method: every variant is warmed up, then timed in alternating rounds (HIP, torch, HIP, torch, ...) of ``--calls`` calls each with one
device synchronise around the round; the figure is the median round over the calls.  A call is S dependent launches of a
[B, H] x [H, 3H] product (the weights, 9 MB at H = 868, re-read from L2 / Infinity Cache every step): the figures are launch latency
plus that stream, not a share of any peak.  The embedding table has 1000 rows here (the shipped 643 372 x 868 table is 2.2 GB and
its dense gradient another 2.2 GB on either side; the table's size does not enter the forward).

Each GPU step under a time limit of its own, the steps chained so that a failure ends the run:

    timeout -k 10 400 python tools/lstur_probe.py --out profiles/lstur/probe.json && \
    timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d /tmp/lstur_trace -- python tools/lstur_probe.py --trace-steps 20 && \
    python tools/lstur_probe.py --summarise /tmp/lstur_trace --out profiles/lstur/kernel_trace.json

(``--trace-steps``: a few forward + backward steps of B = 8 / ini, nothing timed; ``--summarise``: the per-kernel table of that trace.)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

DEV = "cuda:0"
S, I, USERS = 50, 868, 1000


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def rounds(ours, theirs, n_rounds, calls):
    for f in (ours, theirs):
        timed(f, 10)                                             # warm-up: code objects, allocator, MIOpen's find, autograd graph
    a, t = [], []
    for _ in range(n_rounds):
        a.append(timed(ours, calls))
        t.append(timed(theirs, calls))
    return {"hip_us": round(statistics.median(a), 2), "torch_f32_us": round(statistics.median(t), 2),
            "hip_min_max_us": [round(min(a), 2), round(max(a), 2)], "torch_min_max_us": [round(min(t), 2), round(max(t), 2)]}


class TorchComposition(torch.nn.Module):
    """the reference's forward in plain torch: embedding, Dropout2d, hist_size.cpu(), pack_padded_sequence, nn.GRU, last hidden"""

    def __init__(self, method, hidden):
        super().__init__()
        self.method = method
        self.long_term_user_embedding = torch.nn.Embedding(USERS, hidden, padding_idx=0)
        self.dropout = torch.nn.Dropout2d(p=0.5)
        self.gru = torch.nn.GRU(I, hidden)

    def forward(self, user, x, hist_size):
        rows = self.dropout(self.long_term_user_embedding(user).unsqueeze(0))
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, hist_size.cpu().int(), batch_first=True, enforce_sorted=False)
        if self.method == "ini":
            return self.gru(packed, rows)[1].squeeze(0)
        return torch.cat((self.gru(packed)[1].squeeze(0), rows.squeeze(0)), dim=1)


def build(method, b):
    from manner_amd.models.components.user_encoder import LSTURUserEncoder
    hidden = I if method == "ini" else I // 2
    g = torch.Generator().manual_seed(11 + b)
    theirs = TorchComposition(method, hidden)
    ours = LSTURUserEncoder(num_users=USERS, input_dim=I, user_masking_probability=0.5, long_short_term_method=method)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    x = torch.randn(b, S, I, generator=g).to(DEV)
    user = torch.randint(1, USERS, (b,), generator=g).to(DEV)
    hist = torch.randint(1, S + 1, (b,), generator=g)
    hist[0] = S
    up = torch.randn(b, hidden if method == "ini" else 2 * hidden, generator=g).to(DEV)
    return ours.to(DEV).eval(), theirs.to(DEV).eval(), user, x, hist.to(DEV), up


def steps(enc, user, x, hist, up):
    xg = x.clone().requires_grad_(True)

    def fwd():
        enc.eval()
        with torch.no_grad():
            enc(user, x, hist)

    def step():                                                  # train(): MIOpen's RNN backward needs it; the user mask (p = 0.5) is on on both sides
        enc.train()
        enc.zero_grad(set_to_none=True)
        xg.grad = None
        (enc(user, xg, hist) * up).sum().backward()
    return fwd, step


def summarise(trace_dir, out):
    """per (kernel, grid) of a rocprofv3 --kernel-trace csv: launches, mean, least and total microseconds"""
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"lstur_probe: no *kernel_trace.csv under {trace_dir}")
    table = {}
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                low = {k.lower(): v for k, v in row.items()}
                grid = tuple(int(low.get("grid_size_" + a, 0) or 0) // max(int(low.get("workgroup_size_" + a, 1) or 1), 1) for a in "xyz")
                us = (int(low["end_timestamp"]) - int(low["start_timestamp"])) / 1e3
                table.setdefault((low.get("kernel_name", ""), grid), []).append(us)
    kernels = [{"kernel": k, "workgroups": list(g), "launches": len(v), "mean_us": round(statistics.mean(v), 2), "min_us": round(min(v), 2),
                "total_us": round(sum(v), 1)} for (k, g), v in table.items()]
    kernels.sort(key=lambda r: -r["total_us"])
    with open(out, "w") as f:
        json.dump({"source": "rocprofv3 --kernel-trace over tools/lstur_probe.py --trace-steps (a run of its own; B = 8, S = 50, ini: I = H = 868; "
                             "forward + backward steps of the mirror only)", "unit": "microseconds per launch", "kernels": kernels}, f, indent=1)
    print("wrote", out, len(kernels), "kernel rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstur", "probe.json"))
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("lstur_probe: needs the GPU (a timing taken elsewhere says nothing)")
    warnings.simplefilter("ignore")                              # nn.Dropout2d on a 3-D input (the torch composition)
    if args.trace_steps:
        ours, _, user, x, hist, up = build("ini", 8)
        _, step = steps(ours, user, x, hist, up)
        for _ in range(args.trace_steps):
            step()
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "shape": {"S": S, "I": I, "H": {"ini": I, "con": I // 2}},
              "rounds": args.rounds, "calls_per_round": args.calls, "unit": "microseconds per call, median round", "cases": {}}
    for method in ("ini", "con"):
        for b in (8, 64):
            ours, theirs, user, x, hist, up = build(method, b)
            with torch.no_grad():
                rec = {"max_abs_difference_of_the_forwards": float((ours(user, x, hist) - theirs(user, x, hist)).abs().max())}
            fwd, step = steps(ours, user, x, hist, up)
            tfwd, tstep = steps(theirs, user, x, hist, up)
            rec["forward"] = rounds(fwd, tfwd, args.rounds, args.calls)
            rec["forward_backward"] = rounds(step, tstep, args.rounds, max(args.calls // 2, 5))
            print(f"{method} B={b}: {rec}", flush=True)
            result["cases"][f"{method}/B{b}"] = rec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
