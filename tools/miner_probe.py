"""Time per call of the MINER baseline's three operators (csrc/poly.hip through manner_amd.hip / manner_amd.train) beside the same
restatement run as plain float32 torch on the same device, forward and forward + backward, at the reference's shapes
(S = 50, D = 256, Q = 200, K = 32, C = 40) for B = 8 and 64 users.

Method: every variant is warmed up, then timed in alternating rounds (HIP, torch, HIP, torch, ...) of ``--calls`` calls each with
one device synchronise around the round; the figure is the median round over the calls.  These shapes are launch-bound: the figures
are host-enqueue plus kernel time of a handful of small launches, not a share of any peak.

    python tools/miner_probe.py [--rounds 9] [--calls 200] [--out profiles/miner/probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import miner_ref as M  # noqa: E402
from manner_amd import hip, train  # noqa: E402

DEV = "cuda:0"
S, D, Q, K, C = 50, 256, 200, 32, 40


def variants(b):
    """{operator: (hip forward, torch forward, leaves, upstream)}; the forwards take the leaves and return the output"""
    leaves, consts, up = M.poly_inputs(b, S, D, Q, K, b * C)
    mask, bias = consts["mask"].to(DEV), consts["bias"].to(DEV)
    tq, tk, tv, tw = (M.randn(i, *shp).to(DEV) for i, shp in enumerate(((b, K, D), (b, C, D), (b, C, K), (D, D)), 50))
    tw *= D ** -0.5
    cand, user = M.randn(60, b, C, D).to(DEV), M.randn(61, b, K, D).to(DEV)
    return {
        "poly_attention": (lambda x, w, c: train.poly_attention(x, mask, w, c, bias), lambda x, w, c: hip.poly_attention(x, mask, w, c, bias),
                           lambda x, w, c: M.poly_attention(x, w, c, mask, bias)["out"],
                           [leaves[n].to(DEV) for n in ("x", "lin_w", "codes")], up["out"].to(DEV)),
        "target_attention": (train.target_attention, hip.target_attention, lambda q, k, v, w: M.target_attention(q, k, v, w)["out"],
                             [tq, tk, tv, tw], M.randn(62, b, C).to(DEV)),
        "dot_product": (lambda a, r: train.bmm(a, r.permute(0, 2, 1)), lambda a, r: hip.bmm(a, r.permute(0, 2, 1)),
                        lambda a, r: M.bmm_rows(a, r)["out"], [cand, user], M.randn(63, b, C, K).to(DEV)),
    }


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "miner", "probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("miner_probe: needs the GPU (a timing taken elsewhere says nothing)")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "shape": {"S": S, "D": D, "Q": Q, "K": K, "C": C},
              "rounds": args.rounds, "calls_per_round": args.calls, "unit": "microseconds per call, median round", "cases": {}}
    for b in (8, 64):
        for name, (hip_train, hip_infer, ref, leaves, up) in variants(b).items():
            grad_leaves = [t.clone().requires_grad_(True) for t in leaves]

            def step(fn):
                def run():
                    for t in grad_leaves:
                        t.grad = None
                    (fn(*grad_leaves) * up).sum().backward()
                return run

            def fwd(fn):
                def run():
                    with torch.no_grad():
                        fn(*leaves)
                return run
            todo = {"forward": (fwd(hip_infer), fwd(ref)), "forward_backward": (step(hip_train), step(ref))}
            with torch.no_grad():
                err = float((hip_infer(*leaves) - ref(*leaves)).abs().max())
            rec = {"max_abs_difference_of_the_forwards": err}
            for what, (ours, theirs) in todo.items():
                for f in (ours, theirs):
                    timed(f, 20)                                         # warm-up: code objects, allocator, autograd graph
                a, t = [], []
                for _ in range(args.rounds):
                    a.append(timed(ours, args.calls))
                    t.append(timed(theirs, args.calls))
                rec[what] = {"hip_us": round(statistics.median(a), 2), "torch_f32_us": round(statistics.median(t), 2),
                             "hip_min_max_us": [round(min(a), 2), round(max(a), 2)], "torch_min_max_us": [round(min(t), 2), round(max(t), 2)]}
                print(f"B={b} {name} {what}: hip {rec[what]['hip_us']} us, torch f32 {rec[what]['torch_f32_us']} us", flush=True)
            result["cases"][f"B{b}/{name}"] = rec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
