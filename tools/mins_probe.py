"""Time per call of the MINS baseline's user encoder (csrc/mins.hip through the ``MINSUserEncoder`` mirror) at the shipped shape —
S = 50, D = F = 768, C = 6 channels (head dim and channel width 128) — for B = 8 and 64 users, histories of 1 .. 50 clicks, forward
(eval, no_grad) and forward + backward, on three paths alternated in one run:

    torch       the float32 torch composition of the reference's lines: nn.MultiheadAttention on [B, S, D], torch.chunk, per channel
                hist_size.cpu(), pack_padded_sequence(enforce_sorted=False) and the one nn.GRU (MIOpen), cat, the additive pooler
    hip         this mirror: the wide axis-0 attention, one input projection and ONE launch for the recurrence of all B C sequences
    per_channel the same attention, then what the library offered before: six ``gru_last_hidden`` calls on the channel views
                (6 x (1 + 50) launches forward) and ``torch.cat`` — what the single-launch recurrence is to be judged against

Method: every path is warmed up, then timed in alternating rounds (hip, per_channel, torch, hip, ...) of ``--calls`` calls each with one
device synchronise around the round; the figure is the median round, the spread its least and largest round.

Each GPU step under a time limit of its own, the steps chained so that a failure ends the run:

    timeout -k 10 400 python tools/mins_probe.py --out profiles/mins/probe.json && \
    timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/mins_trace -- python tools/mins_probe.py --trace-steps 20 && \
    python tools/mins_probe.py --summarise /tmp/mins_trace --out profiles/mins/kernel_trace.json

(``--trace-steps``: a few forward + backward steps of the mirror at B = 8, nothing timed; ``--summarise``: the per-kernel table of that trace.)
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
S, D, C, Q = 50, 768, 6, 200
PATHS = ("hip", "per_channel", "torch")


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def rounds(fns, n_rounds, calls):
    for f in fns.values():
        timed(f, 10)                                             # warm-up: code objects, allocator, MIOpen's find, autograd graph
    took = {k: [] for k in fns}
    for _ in range(n_rounds):
        for k, f in fns.items():
            took[k].append(timed(f, calls))
    out = {}
    for k, v in took.items():
        out[k + "_us"], out[k + "_min_max_us"] = round(statistics.median(v), 2), [round(min(v), 2), round(max(v), 2)]
    return out


def build(b):
    from manner_amd import hip, train
    from manner_amd.models.components.attention import _differentiable
    from manner_amd.models.components.user_encoder import MINSUserEncoder

    class TorchComposition(torch.nn.Module):
        """the reference's forward in plain torch"""

        def __init__(self):
            super().__init__()
            self.num_gru_channels = C
            self.multihead_attention = torch.nn.MultiheadAttention(embed_dim=D, num_heads=C)
            self.pool_linear = torch.nn.Linear(D, Q)
            self.pool_query = torch.nn.Parameter(torch.empty(Q).uniform_(-0.1, 0.1))
            self.gru = torch.nn.GRU(D // C, D // C)

        def forward(self, x, hist_size):
            mixed, _ = self.multihead_attention(x, x, x)
            channels = []
            for chunk in torch.chunk(mixed, C, dim=2):
                packed = torch.nn.utils.rnn.pack_padded_sequence(chunk, hist_size.cpu().int(), batch_first=True, enforce_sorted=False)
                channels.append(self.gru(packed)[1])
            v = torch.cat(channels, dim=2).transpose(0, 1)                                     # [B, 1, D]
            w = torch.softmax(torch.tanh(self.pool_linear(v)) @ self.pool_query, dim=1)
            return torch.bmm(w.unsqueeze(1), v).squeeze(1)

    class PerChannel(MINSUserEncoder):
        """the mirror's attention, then one ``gru_last_hidden`` call per channel view: the path the library offered before"""

        def forward(self, x, hist_size):
            p = self._params()
            if _differentiable(self, x):
                mixed = train.mha_axis0_wide(x, *p[:4], C)
                return torch.cat([train.gru_last_hidden(mixed[:, :, c * (D // C):(c + 1) * (D // C)], hist_size, *p[4:]) for c in range(C)], dim=1)
            p = [t.detach() for t in p]
            mixed = hip.mha_axis0_wide(x, *p[:4], C)
            return torch.cat([hip.gru_last_hidden(mixed[:, :, c * (D // C):(c + 1) * (D // C)], hist_size, *p[4:]) for c in range(C)], dim=1)

    g = torch.Generator().manual_seed(13 + b)
    theirs = TorchComposition()
    ours, old = MINSUserEncoder(D, Q, D, C), PerChannel(D, Q, D, C)
    sd = {k: v for k, v in theirs.state_dict().items() if not k.startswith("pool_")}
    sd.update({"additive_attention.linear.weight": theirs.pool_linear.weight.detach(), "additive_attention.linear.bias": theirs.pool_linear.bias.detach(),
               "additive_attention.query": theirs.pool_query.detach()})
    sd.update({f"multi_channel_gru.{c}.{k[len('gru.'):]}": v for c in range(C) for k, v in list(sd.items()) if k.startswith("gru.")})
    for m in (ours, old):
        m.load_state_dict(sd, strict=True)
    x = torch.randn(b, S, D, generator=g).to(DEV)
    hist = torch.randint(1, S + 1, (b,), generator=g)
    hist[0] = S
    up = torch.randn(b, D, generator=g).to(DEV)
    return {"hip": ours.to(DEV), "per_channel": old.to(DEV), "torch": theirs.to(DEV)}, x, hist.to(DEV), up


def steps(enc, x, hist, up):
    xg = x.clone().requires_grad_(True)

    def fwd():
        enc.eval()
        with torch.no_grad():
            enc(x, hist)

    def step():                                                  # train(): MIOpen's RNN backward needs it
        enc.train()
        enc.zero_grad(set_to_none=True)
        xg.grad = None
        (enc(xg, hist) * up).sum().backward()
    return fwd, step


def summarise(trace_dir, out):
    """per (kernel, grid) of a rocprofv3 --kernel-trace csv: launches, mean, least and total microseconds"""
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"mins_probe: no *kernel_trace.csv under {trace_dir}")
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
        json.dump({"source": "rocprofv3 --kernel-trace --stats over tools/mins_probe.py --trace-steps (a run of its own; B = 8, S = 50, D = 768, C = 6; "
                             "forward + backward steps of the mirror only)", "unit": "microseconds per launch", "kernels": kernels}, f, indent=1)
    print("wrote", out, len(kernels), "kernel rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mins", "probe.json"))
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("mins_probe: needs the GPU (a timing taken elsewhere says nothing)")
    warnings.simplefilter("ignore")
    if args.trace_steps:
        encs, x, hist, up = build(8)
        _, step = steps(encs["hip"], x, hist, up)
        for _ in range(args.trace_steps):
            step()
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "shape": {"S": S, "D": D, "C": C, "head_dim": D // C},
              "rounds": args.rounds, "calls_per_round": args.calls, "unit": "microseconds per call, median round", "paths": list(PATHS), "cases": {}}
    for b in (8, 64):
        encs, x, hist, up = build(b)
        with torch.no_grad():
            outs = {k: e.eval()(x, hist) for k, e in encs.items()}
        rec = {"max_abs_difference_of_the_forwards": {k: float((outs[k] - outs["torch"]).abs().max()) for k in ("hip", "per_channel")}}
        fns = {k: steps(encs[k], x, hist, up) for k in PATHS}
        rec["forward"] = rounds({k: f[0] for k, f in fns.items()}, args.rounds, args.calls)
        rec["forward_backward"] = rounds({k: f[1] for k, f in fns.items()}, args.rounds, max(args.calls // 2, 5))
        print(f"B={b}: {rec}", flush=True)
        result["cases"][f"B{b}"] = rec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
