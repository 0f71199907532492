"""Time per call of the CAUM baseline's user encoder (csrc/caum.hip through the ``CAUMUserEncoder`` mirror) beside the same restatement
run as plain float32 torch on the same device, forward and forward + backward, at the shipped widths (S = 50, D = U = F = H1 = 400,
H2 = 256, 16 heads: head dim 25) for B = 8 and 64 users; the candidate loop of ``CAUMPLMModule.forward`` at C = 5 and C = 40 three
ways — the loop over the per-column mirror, ``forward_all`` (one library call on shared history products) and the loop over the
float32 torch composition — with the achieved TFLOP/s of the row-tiled linear inside ``forward_all``; and the share of a call that does not depend on the candidate (the history-side products of the three windows, of linear2 and of nothing
else: everything past them mixes the candidate in), which is what an eval()-time memo across the loop could save.

Method: every variant is warmed up, then timed in alternating rounds (HIP, torch, HIP, torch, ... — three variants alternate the same way) of ``--calls`` calls each with
one device synchronise around the round; the figure is the median round over the calls.  These shapes are launch-bound: the figures
are host-enqueue plus kernel time of a few dozen small launches, not a share of any peak.

    python tools/caum_probe.py [--rounds 9] [--calls 200] [--out profiles/caum/probe.json]
"""
import argparse
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


def rounds3(variants, n_rounds, calls):
    """``rounds`` for any number of named variants, alternating within each round: {name_us, name_min_max_us}"""
    for f in variants.values():
        timed(f, 3)
    got = {k: [] for k in variants}
    for _ in range(n_rounds):
        for k, f in variants.items():
            got[k].append(timed(f, calls))
    out = {}
    for k, v in got.items():
        out[k + "_us"] = round(statistics.median(v), 2)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caum", "probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("caum_probe: needs the GPU (a timing taken elsewhere says nothing)")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "shape": {"S": S, "D": D, "F": F, "H1": H1, "H2": H2, "heads": HEADS}, "rounds": args.rounds, "calls_per_round": args.calls,
              "unit": "microseconds per call, median round", "cases": {}}
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
