"""Time per call of the CAUM baseline's user encoder (csrc/caum.hip through the ``CAUMUserEncoder`` mirror) beside the same restatement
run as plain float32 torch on the same device, forward and forward + backward, at the shipped widths (S = 50, D = U = F = H1 = 400,
H2 = 256, 16 heads: head dim 25) for B = 8 and 64 users; the candidate loop of ``CAUMPLMModule.forward`` at C = 5 and C = 40 three
ways — the loop over the per-column mirror, ``forward_all`` (one library call on shared history products) and the loop over the
float32 torch composition — with the achieved TFLOP/s of the row-tiled linear inside ``forward_all``; and the share of a call that does not depend on the candidate (the history-side products of the three windows, of linear2 and of nothing
else: everything past them mixes the candidate in), which is what an eval()-time memo across the loop could save.
The training leg: forward + backward of the C = 5 candidate loop in train() at p = 0.2, three ways alternated in one run — the loop
over the per-column mirror, ``CAUMUserEncoder.train_all_columns`` (one library call forward, one backward, for all columns) and the
loop over the float32 torch composition with keep-masks — with every round's figure kept, so that "below the loop in every round
pair" can be read off the file.

Method: every variant is warmed up, then timed in alternating rounds (HIP, torch, HIP, torch, ... — three variants alternate the same way) of ``--calls`` calls each with
one device synchronise around the round; the figure is the median round over the calls.  These shapes are launch-bound: the figures
are host-enqueue plus kernel time of a few dozen small launches, not a share of any peak.

    python tools/caum_probe.py [--rounds 9] [--calls 200] [--out profiles/caum/probe.json]
    python tools/caum_probe.py --train-only                      # the training leg alone, merged into the cases of --out
    rocprofv3 --kernel-trace -d /tmp/caum_trace -- python tools/caum_probe.py --trace-steps 20 --trace-batch 64
    python tools/caum_probe.py --summarise /tmp/caum_trace --section B64 --out profiles/caum/kernel_trace.json
    (sections B8, B64; with --trace-per-column at --trace-batch 40 / 320: per_column_B40, per_column_B320; with --trace-wgrad-alone at
    --trace-batch 8 / 64: wgrad_alone_B8, wgrad_alone_B64 — one traced run each)
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import caum_ref as CR  # noqa: E402
from manner_amd.models.components.user_encoder import CAUMUserEncoder  # noqa: E402

DEV = "cuda:0"
S, D, F, H1, H2, HEADS = 50, 400, 400, 400, 256, 16


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def rounds(ours, theirs, n_rounds, calls):
    for f in (ours, theirs):
        timed(f, 20)                                             # warm-up: code objects, allocator, autograd graph
    a, t = [], []
    for _ in range(n_rounds):
        a.append(timed(ours, calls))
        t.append(timed(theirs, calls))
    return {"hip_us": round(statistics.median(a), 2), "torch_f32_us": round(statistics.median(t), 2),
            "hip_min_max_us": [round(min(a), 2), round(max(a), 2)], "torch_min_max_us": [round(min(t), 2), round(max(t), 2)]}


def rounds3(variants, n_rounds, calls, keep_rounds=False):
    """``rounds`` for any number of named variants, alternating within each round: {name_us, name_min_max_us}; ``keep_rounds``:
    {name_rounds_us} with every round's figure instead of the extremes"""
    for f in variants.values():
        timed(f, 3)
    got = {k: [] for k in variants}
    for _ in range(n_rounds):
        for k, f in variants.items():
            got[k].append(timed(f, calls))
    out = {}
    for k, v in got.items():
        out[k + "_us"] = round(statistics.median(v), 2)
        if keep_rounds:
            out[k + "_rounds_us"] = [round(t, 2) for t in v]
        else:
            out[k + "_min_max_us"] = [round(min(v), 2), round(max(v), 2)]
    return out


def linear_rate(fn, flops):
    """device time of the launches of the row-tiled linear (wlin_kernel) inside one call of ``fn``, by torch's profiler, and the
    TFLOP/s that is over the multiply-adds of those launches (the 157.3 TFLOP/s f32 matrix peak is the yardstick)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    def device_us(e):
        return getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)

    def short(key):                                              # void manner::(anonymous namespace)::wlin_kernel<true, false>(...) -> wlin_kernel<true, false>
        hit = re.search(r"(\w+_kernel(?:<[^>]*>)?)", key)
        return hit.group(1) if hit else key[:60]
    rows = [e for e in prof.key_averages() if "wlin_kernel" in e.key]
    us, every = sum(device_us(e) for e in rows), sum(device_us(e) for e in prof.key_averages())
    by_kernel = {}
    for e in prof.key_averages():
        if device_us(e) > 0:
            by_kernel[short(e.key)] = round(by_kernel.get(short(e.key), 0.0) + device_us(e), 2)
    return {"wlin_launches": sum(e.count for e in rows), "wlin_device_us": round(us, 2), "all_kernels_device_us": round(every, 2),
            "device_us_by_kernel": dict(sorted(by_kernel.items(), key=lambda kv: -kv[1])),
            "wlin_gflop": round(flops / 1e9, 3), "wlin_tflops": round(flops / us / 1e6, 2) if us else None, "f32_matrix_peak_tflops": 157.3}


def history_side(x, w):
    """what of one call does not depend on the candidate: the three window products and the history half of linear2"""
    d = x.shape[2]
    left, right = torch.roll(x, 1, dims=1), torch.roll(x, -1, dims=1)
    return (left @ w["w1"][:, :d].T + x @ w["w1"][:, d:2 * d].T + right @ w["w1"][:, 2 * d:3 * d].T, x @ w["w2"][:, d:].T)


TRAIN_C, TRAIN_P = 5, 0.2


def train_steps(b):
    """forward + backward of the C = 5 candidate loop in train() at p = 0.2: {name: step} for the loop over the per-column mirror,
    ``train_all_columns`` and the loop over the float32 torch composition (keep-masks drawn once per column, applied in every step)"""
    leaves, _, _ = CR.caum_inputs(b, S, D, F, H1, H2, HEADS)
    encs = {}
    for name, on in (("loop", False), ("train_all", True)):
        enc = CAUMUserEncoder(news_vector_dim=D, num_filters=F, dense_att_hidden_dim1=H1, dense_att_hidden_dim2=H2, user_vector_dim=D,
                              num_attention_heads=HEADS, dropout_probability=TRAIN_P)
        enc.load_state_dict({CR.STATE_KEYS[n]: leaves[n] for n in CR.PARAMS}, strict=True)
        enc.train_all_columns = on
        encs[name] = enc.to(DEV).train()
    wg = {n: leaves[n].to(DEV).requires_grad_(True) for n in CR.PARAMS}
    xg = leaves["x"].to(DEV).requires_grad_(True)
    cg = CR.randn(75, b, TRAIN_C, D).to(DEV).requires_grad_(True)
    up = CR.randn(76, b, TRAIN_C).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    keeps = [[torch.rand(shape, device=DEV, generator=gen) >= TRAIN_P for shape in ((b, D), (b, S, D), (b, S, F + D))] for _ in range(TRAIN_C)]

    def mirror(enc):
        def step():
            enc.zero_grad()
            xg.grad = cg.grad = None
            (enc.forward_all(xg, cg) * up).sum().backward()
        return step

    def torch_step():
        for t in (xg, cg, *wg.values()):
            t.grad = None
        scores = torch.zeros(b, TRAIN_C, device=DEV).transpose(1, 0)
        for i in range(TRAIN_C):
            scores[i, :] = CR.caum_user(xg, cg[:, i, :], heads=HEADS, p=TRAIN_P, keep1=keeps[i][0], keep2=keeps[i][1], keep3=keeps[i][2], **wg)["out"]
        (scores.transpose(1, 0) * up).sum().backward()
    return {"loop": mirror(encs["loop"]), "train_all": mirror(encs["train_all"]), "torch_f32": torch_step}


def train_leg(result, n_rounds, calls):
    for b in (8, 64):
        rec = {"columns": TRAIN_C, "p": TRAIN_P, "what": "forward + backward of the candidate loop in train(), microseconds per step"}
        rec.update(rounds3(train_steps(b), n_rounds, calls, keep_rounds=True))
        rec["train_all_below_the_loop_in_every_round"] = all(a < l for a, l in zip(rec["train_all_rounds_us"], rec["loop_rounds_us"]))
        rec["loop_over_train_all"] = round(rec["loop_us"] / rec["train_all_us"], 2)
        result["cases"][f"B{b}/train_loop_C{TRAIN_C}"] = rec
        print(f"B={b} training loop C={TRAIN_C}: {rec}", flush=True)


def per_column_step(b):
    """forward + backward of ONE per-column call at batch ``b`` (p = 0.2): at b = 5 B its launches have the rows of the all-columns
    route at batch B and C = 5 — wgrad_rows_kernel at the (R, K, O) of mwgrad_kernel"""
    leaves, _, up = CR.caum_inputs(b, S, D, F, H1, H2, HEADS)
    enc = CAUMUserEncoder(news_vector_dim=D, num_filters=F, dense_att_hidden_dim1=H1, dense_att_hidden_dim2=H2, user_vector_dim=D,
                          num_attention_heads=HEADS, dropout_probability=TRAIN_P)
    enc.load_state_dict({CR.STATE_KEYS[n]: leaves[n] for n in CR.PARAMS}, strict=True)
    enc = enc.to(DEV).train()
    xg, cg, up = leaves["x"].to(DEV).requires_grad_(True), leaves["c"].to(DEV).requires_grad_(True), up["out"].to(DEV)

    def step():
        enc.zero_grad()
        xg.grad = cg.grad = None
        (enc(xg, cg) * up).sum().backward()
    return step


def wgrad_alone(b, steps):
    """manner_hip_wgrad_rows_f32 — mwgrad_kernel alone — at the (R, K, O) of every weight gradient of the all-columns route at batch
    ``b``, C = 5, whatever kernel the entry itself selects there"""
    from manner_amd import hip
    lib = hip._lib.load()
    for _, kind, k, o in WGRAD_PRODUCTS:
        r = b * TRAIN_C * S if kind == "rows" else b * TRAIN_C
        dy, x, dw = torch.randn(r, o, device=DEV), torch.randn(r, k, device=DEV), torch.empty(o, k, device=DEV)
        need = int(lib.manner_hip_wgrad_rows_f32_workspace_bytes(r, k, o))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
        for _ in range(steps):
            hip._lib.check(lib.manner_hip_wgrad_rows_f32(hip._ptr(dy), o, hip._ptr(x), k, r, k, o, hip._ptr(dw), k, hip._ptr(ws), need, hip._stream()))
    torch.cuda.synchronize()


# the nine weight gradients of a call at the shipped widths: (parameters, rows of the product, K, O)
WGRAD_PRODUCTS = (("dense_att.linear3.weight", "rows", H2, 1), ("dense_att.linear2.weight", "rows", H1, H2),
                  ("dense_att.linear.weight[:, :U], out_proj.weight", "rows", D, D), ("dense_att.linear.weight[:, U:]", "pairs", D, H1),
                  ("linear3.weight, linear2.weight", "rows", F + D, D), ("in_proj_weight", "rows", D, 3 * D), ("linear1.weight", "rows", 4 * D, F))


def wgrad_ab(doc):
    """wgrad_rows_kernel against mwgrad_kernel at equal (R, K, O), from the sections of the trace file: mwgrad_kernel alone at the
    shapes of the all-columns route at batch B, C = 5, beside one per-column call at batch 5 B.  A product's launches are found by the (k, o) extent of their grids; among those
    the product over the B C S rows has the most row groups and the one over the B C pairs the fewest."""
    def pick(section, kernel, xy, kind):
        rows = [k for k in doc[section]["kernels"] if k["kernel"].startswith(kernel) and tuple(k["workgroups"][:2]) == xy]
        if not rows:
            return None
        return (max if kind == "rows" else min)(rows, key=lambda k: k["workgroups"][2])
    table = []
    for b in (8, 64):
        for name, kind, k, o in WGRAD_PRODUCTS:
            small = o < 64 or k < 64
            new = pick(f"wgrad_alone_B{b}", "mwgrad_kernel", (-(-k // 32), -(-o // 32)) if small else (-(-k // 128), -(-o // 64)), kind)
            old = pick(f"per_column_B{5 * b}", "wgrad_rows_kernel", (-(-k // 256), o), kind)
            if new and old:
                table.append({"product": name, "R": (b * TRAIN_C * S) if kind == "rows" else b * TRAIN_C, "K": k, "O": o,
                              "wgrad_rows_kernel_us": old["mean_us"], "wgrad_rows_groups": old["workgroups"][2],
                              "mwgrad_kernel_us": new["mean_us"], "mwgrad_groups": new["workgroups"][2],
                              "old_over_new": round(old["mean_us"] / new["mean_us"], 2)})
    return table


def summarise(trace_dir, out, section):
    """per (kernel, grid) of a rocprofv3 --kernel-trace csv over ONE --trace-steps run (one route at one batch size, so that a grid
    names one launch shape): launches, mean, least and total microseconds, kept as ``section`` under "train_all_columns" of ``out``
    beside what the file already holds; with the per_column and wgrad_alone sections there, also the equal-shape table of the two weight-gradient kernels"""
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"caum_probe: no *kernel_trace.csv under {trace_dir}")
    table = {}
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                low = {k.lower(): v for k, v in row.items()}
                grid = tuple(int(low.get("grid_size_" + a, 0) or 0) // max(int(low.get("workgroup_size_" + a, 1) or 1), 1) for a in "xyz")
                raw = low.get("kernel_name", "")
                hit = re.search(r"(\w+_kernel(?:<[^>]*>)?)", raw)       # void manner::(anonymous namespace)::wlin_kernel<true, false>(...) -> wlin_kernel<true, false>
                table.setdefault((hit.group(1) if hit else raw, grid), []).append((int(low["end_timestamp"]) - int(low["start_timestamp"])) / 1e3)
    kernels = [{"kernel": k, "workgroups": list(g), "launches": len(v), "mean_us": round(statistics.mean(v), 2), "min_us": round(min(v), 2),
                "total_us": round(sum(v), 1)} for (k, g), v in table.items()]
    kernels.sort(key=lambda r: -r["total_us"])
    doc = {}
    if os.path.exists(out):
        with open(out) as f:
            doc = json.load(f)
    top = doc.setdefault("train_all_columns", {})
    top["source"] = ("rocprofv3 --kernel-trace over tools/caum_probe.py --trace-steps, one run per section: B8 / B64 = forward + backward steps of "
                     "CAUMUserEncoder.train_all_columns at C = 5, p = 0.2, the shipped widths; per_column_B40 / _B320 = forward + backward of one "
                     "per-column call at five times the batch, whose launches have the same rows; wgrad_alone_B8 / _B64 = manner_hip_wgrad_rows_f32 "
                     "at the (R, K, O) of every weight gradient of B8 / B64")
    top["unit"] = "microseconds per launch"
    top[section] = {"kernels": kernels}
    if all(k in top for k in ("wgrad_alone_B8", "wgrad_alone_B64", "per_column_B40", "per_column_B320")):
        top["weight_gradient_equal_shapes"] = wgrad_ab(top)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
    print("wrote", out, section, len(kernels), "kernel rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--train-only", action="store_true")
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--trace-batch", type=int, default=8)
    ap.add_argument("--trace-per-column", action="store_true")
    ap.add_argument("--trace-wgrad-alone", action="store_true")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--section", default="B8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caum", "probe.json"))
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.out, args.section)
    if not torch.cuda.is_available():
        raise SystemExit("caum_probe: needs the GPU (a timing taken elsewhere says nothing)")
    if args.trace_steps and args.trace_wgrad_alone:
        return wgrad_alone(args.trace_batch, args.trace_steps)
    if args.trace_steps:
        step = per_column_step(args.trace_batch) if args.trace_per_column else train_steps(args.trace_batch)["train_all"]
        for _ in range(args.trace_steps):
            step()
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "shape": {"S": S, "D": D, "F": F, "H1": H1, "H2": H2, "heads": HEADS}, "rounds": args.rounds, "calls_per_round": args.calls,
              "unit": "microseconds per call, median round", "cases": {}}
    if args.train_only:
        if os.path.exists(args.out):
            with open(args.out) as f:
                result = json.load(f)
        train_leg(result, args.rounds, max(args.calls // TRAIN_C, 5))
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
        print("wrote", args.out)
        return
    for b in (8, 64):
        leaves, consts, up = CR.caum_inputs(b, S, D, F, H1, H2, HEADS)
        enc = CAUMUserEncoder(news_vector_dim=D, num_filters=F, dense_att_hidden_dim1=H1, dense_att_hidden_dim2=H2, user_vector_dim=D,
                              num_attention_heads=HEADS, dropout_probability=0.0)
        enc.load_state_dict({CR.STATE_KEYS[n]: leaves[n] for n in CR.PARAMS}, strict=True)
        enc = enc.to(DEV).eval()
        w = {n: leaves[n].to(DEV) for n in CR.PARAMS}
        wg = {n: t.clone().requires_grad_(True) for n, t in w.items()}
        x, c, up = leaves["x"].to(DEV), leaves["c"].to(DEV), up["out"].to(DEV)
        xg, cg = x.clone().requires_grad_(True), c.clone().requires_grad_(True)

        def ref(xx, cc, ww):
            return CR.caum_user(xx, cc, heads=HEADS, **ww)["out"]

        def hip_fwd():
            with torch.no_grad():
                enc(x, c)

        def ref_fwd():
            with torch.no_grad():
                ref(x, c, w)

        def hip_step():
            enc.zero_grad()
            xg.grad = cg.grad = None
            (enc(xg, cg) * up).sum().backward()

        def ref_step():
            for t in (xg, cg, *wg.values()):
                t.grad = None
            (ref(xg, cg, wg) * up).sum().backward()

        def hist_only():
            with torch.no_grad():
                history_side(x, w)

        with torch.no_grad():
            rec = {"max_abs_difference_of_the_forwards": float((enc(x, c) - ref(x, c, w)).abs().max())}
        rec["forward"] = rounds(hip_fwd, ref_fwd, args.rounds, args.calls)
        rec["forward_backward"] = rounds(hip_step, ref_step, args.rounds, args.calls)
        print(f"B={b} user encoder: {rec}", flush=True)
        # the candidate-independent share, measured on the torch composition (the only form in which it exists as separate launches)
        timed(hist_only, 20)
        hist = statistics.median(timed(hist_only, args.calls) for _ in range(args.rounds))
        rec["history_side_torch_f32_us"] = round(hist, 2)
        rec["history_side_share_of_the_torch_forward"] = round(hist / rec["forward"]["torch_f32_us"], 3)
        fl_hist, fl_all = 2.0 * b * S * (3 * D * F + D * D), 2.0 * b * S * (4 * D * F + 2 * D * D + 3 * D * D + D * D + (F + D) * D + D * H1 + H1 * H2)
        rec["history_side_share_of_the_multiply_adds"] = round(fl_hist / fl_all, 3)
        result["cases"][f"B{b}/user_encoder"] = rec
        for c_n in (5, 40):                                      # the loop of CAUMPLMModule.forward (baselines/caum_plm_module.py:155-165)
            cand = CR.randn(70 + c_n, b, c_n, D).to(DEV)

            def loop(call):
                def run():
                    with torch.no_grad():
                        scores = torch.zeros(b, c_n, device=DEV).transpose(1, 0)
                        for i in range(c_n):
                            scores[i, :] = call(cand[:, i, :])
                return run
            def all_columns():
                with torch.no_grad():
                    enc.forward_all(x, cand)
            calls = max(args.calls // c_n, 5)
            rec = rounds3({"hip": loop(lambda cc: enc(x, cc)), "forward_all": all_columns, "torch_f32": loop(lambda cc: ref(x, cc, w))}, args.rounds, calls)
            with torch.no_grad():
                by_loop = torch.stack([enc(x, cand[:, i, :]) for i in range(c_n)], dim=1)
                rec["max_abs_difference_forward_all_to_the_loop"] = float((enc.forward_all(x, cand) - by_loop).abs().max())
            r, n, wide = b * S, b * c_n, b * c_n * S                    # rows of the history side, of the candidate side, wide rows
            flops = 2.0 * (r * (3 * D * F + D * D + 3 * D * D + F * D) + n * (D * F + D * D + 3 * D * D + F * D + D * H1) + D * D * D + D * D
                           + wide * (D * D + D * H1 + H1 * H2))
            rec["linear"] = linear_rate(all_columns, flops)
            rec["wide_rows_gflop"] = round(2.0 * wide * (D * D + D * H1 + H1 * H2) / 1e9, 3)
            result["cases"][f"B{b}/module_loop_C{c_n}"] = rec
            print(f"B={b} loop C={c_n}: {rec}", flush=True)
    train_leg(result, args.rounds, max(args.calls // TRAIN_C, 5))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
