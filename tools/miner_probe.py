"""Time per call of the MINER baseline's three operators (csrc/poly.hip through manner_amd.hip / manner_amd.train) beside the same
restatement run as plain float32 torch on the same device, forward and forward + backward, at the reference's shapes
(S = 50, D = 256, Q = 200, K = 32, C = 40) for B = 8 and 64 users.

Method: every variant is warmed up, then timed in alternating rounds (HIP, torch, HIP, torch, ...) of ``--calls`` calls each with
one device synchronise around the round; the figure is the median round over the calls.  These shapes are launch-bound: the figures
are host-enqueue plus kernel time of a handful of small launches, not a share of any peak.

The ``module_step`` leg times MINERModule's own lines: ``hotpath.miner_train_step`` (forward + backward, C = 5 candidates per user) and
``hotpath.miner_forward`` (forward only, C = 40) over encoder-free stub news vectors (an embedding lookup), category bias with Dc = 300,
all three score types, against the route a user has today — the module's lines (baselines/miner_module.py:153-242) restated in float32
torch over the mirror leaf classes of this package, the [N_hist, T] cosine matrix and the per-impression Python loop included.

    python tools/miner_probe.py [--rounds 9] [--calls 200] [--step-calls 20] [--legs operators,module_step] [--out profiles/miner/probe.json]
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
from manner_amd import hip, hotpath, train  # noqa: E402
from manner_amd.models.components.attention import PolyAttention, TargetAwareAttention  # noqa: E402
from manner_amd.models.components.click_predictors import DotProduct  # noqa: E402

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


DC, V = 300, 19                                                 # the shipped category embedding width; MIND's category count


def to_dense_batch(x, batch, nb):
    """torch_geometric's ``to_dense_batch`` restated in torch (its maximum is read back to the host, as there)"""
    num = torch.bincount(batch, minlength=nb)
    cum = torch.cat([num.new_zeros(1), num.cumsum(0)])
    width = int(num.max())
    idx = torch.arange(batch.numel(), device=x.device) - cum[batch] + batch * width
    out = x.new_zeros((nb * width,) + tuple(x.shape[1:]))
    out[idx] = x
    mask = torch.zeros(nb * width, dtype=torch.bool, device=x.device)
    mask[idx] = True
    return out.view((nb, width) + tuple(x.shape[1:])), mask.view(nb, width)


def module_lines_today(enc, user_encoder, click, target, table, batch, score_type, with_loss):
    """MINERModule.forward and the loss lines of model_step as the unchanged reference module runs them today over the mirror classes"""
    nb = batch["users"].numel()
    hist_dense, mask_hist = to_dense_batch(enc(batch["x_hist"]["text"]), batch["batch_hist"], nb)
    cand_dense, _ = to_dense_batch(enc(batch["x_cand"]["text"]), batch["batch_cand"], nb)
    x, y = table[batch["x_hist"]["category"]], table[batch["x_cand"]["category"]]
    x, y = x / torch.norm(x, p=2, dim=1).unsqueeze(1), y / torch.norm(y, p=2, dim=1).unsqueeze(1)     # torchmetrics' two lines
    bias, _ = to_dense_batch(x @ y.T, batch["batch_hist"], nb)
    mask_cand = batch["batch_cand"].unsqueeze(dim=0).repeat(bias.shape[0], 1)
    cand_idx = [torch.where(mask_cand[i] == i)[0] for i in range(mask_cand.shape[0])]
    mask = torch.zeros(mask_cand.shape, dtype=torch.bool, device=bias.device)
    for i in range(mask.shape[0]):
        mask[i, cand_idx[i]] = True
    bias = bias.masked_fill_(mask.unsqueeze(dim=1).repeat(1, bias.shape[1], 1), 0)
    user = user_encoder(clicked_news_vector=hist_dense, attn_mask=mask_hist, bias=bias)
    scores = click(cand_dense, user.permute(0, 2, 1))
    if score_type == "max":
        scores = scores.max(dim=2)[0]
    elif score_type == "mean":
        scores = scores.mean(dim=2)
    else:
        scores = target(query=user, key=cand_dense, value=scores)
    if not with_loss:
        return scores
    y_true, _ = to_dense_batch(batch["labels"], batch["batch_cand"], nb)
    un = user / (1e-8 + torch.linalg.norm(user, dim=2, keepdim=True))
    dist = torch.matmul(un, un.permute(0, 2, 1))
    dist = dist.masked_fill(torch.eye(user.shape[1], device=user.device).repeat(user.shape[0], 1, 1).bool(), 0)
    return torch.nn.functional.cross_entropy(scores, y_true) + dist.mean()


def module_step_leg(args):
    out = {"shape": {"S": S, "D": D, "Q": Q, "K": K, "Dc": DC, "C_forward_backward": 5, "C_forward": 40}, "calls_per_round": args.step_calls,
           "baseline": "the module's lines in float32 torch over the mirror leaf classes (N_hist x T cosine matrix, per-impression loop)",
           "cases": {}}
    for b in (8, 64):
        for what, c in (("forward_backward", 5), ("forward", 40)):
            hist_n = [S - (i % 5) * 7 for i in range(b)]
            n_hist, n_cand = sum(hist_n), b * c
            rows = torch.nn.Parameter(M.randn(70 + b + c, n_hist + n_cand, D).to(DEV))
            user_encoder, target, click = PolyAttention(D, K, Q).to(DEV), TargetAwareAttention(D).to(DEV), DotProduct()
            table = M.randn(71, V, DC).to(DEV)
            emb = torch.nn.Embedding.from_pretrained(table, freeze=True)
            gen = torch.Generator().manual_seed(b + c)

            def enc(tokens):
                return torch.nn.functional.embedding(tokens["input_ids"][:, 0], rows)

            def tok(lo, hi):
                ids = torch.arange(lo, hi, device=DEV).reshape(-1, 1)
                return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
            labels = torch.zeros(b, c)
            labels[:, 0] = 1.0
            batch = {"users": torch.arange(b, device=DEV), "batch_hist": torch.repeat_interleave(torch.arange(b), torch.tensor(hist_n)).to(DEV),
                     "batch_cand": torch.repeat_interleave(torch.arange(b), c).to(DEV), "labels": labels.reshape(-1).to(DEV),
                     "x_hist": {"text": tok(0, n_hist), "category": torch.randint(0, V, (n_hist,), generator=gen).to(DEV)},
                     "x_cand": {"text": tok(n_hist, n_hist + n_cand), "category": torch.randint(0, V, (n_cand,), generator=gen).to(DEV)},
                     "hist_max": max(hist_n), "cand_max": c}
            params = [rows] + list(user_encoder.parameters()) + list(target.parameters())
            for score_type in M.SCORE_TYPES:
                kw = dict(score_type=score_type, target_aware_attn=target, category_embedding=emb, category_dropout=None)

                def clear():
                    for t in params:
                        t.grad = None
                if what == "forward_backward":
                    def ours():
                        clear()
                        hotpath.miner_train_step(enc, user_encoder, batch, **kw)[0].backward()

                    def theirs():
                        clear()
                        module_lines_today(enc, user_encoder, click, target, table, batch, score_type, True).backward()
                    with torch.no_grad():
                        diff = float((hotpath.miner_train_step(enc, user_encoder, batch, **kw)[0]
                                      - module_lines_today(enc, user_encoder, click, target, table, batch, score_type, True)).abs())
                else:
                    def ours():
                        with torch.no_grad():
                            hotpath.miner_forward(enc, user_encoder, batch, **kw)

                    def theirs():
                        with torch.no_grad():
                            module_lines_today(enc, user_encoder, click, target, table, batch, score_type, False)
                    with torch.no_grad():
                        diff = float((hotpath.miner_forward(enc, user_encoder, batch, **kw)[1]
                                      - module_lines_today(enc, user_encoder, click, target, table, batch, score_type, False)).abs().max())
                for f in (ours, theirs):
                    timed(f, 5)
                a, t = [], []
                for _ in range(args.rounds):
                    a.append(timed(ours, args.step_calls))
                    t.append(timed(theirs, args.step_calls))
                rec = {"hip_us": round(statistics.median(a), 2), "torch_f32_us": round(statistics.median(t), 2),
                       "hip_min_max_us": [round(min(a), 2), round(max(a), 2)], "torch_min_max_us": [round(min(t), 2), round(max(t), 2)],
                       "max_abs_difference": diff}
                print(f"module_step B={b} C={c} {score_type} {what}: hip {rec['hip_us']} us, torch f32 {rec['torch_f32_us']} us", flush=True)
                out["cases"][f"B{b}/{score_type}/{what}"] = rec
    hip.check_status(DEV)
    return out


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
    ap.add_argument("--step-calls", type=int, default=20)
    ap.add_argument("--legs", default="operators,module_step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "miner", "probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("miner_probe: needs the GPU (a timing taken elsewhere says nothing)")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "shape": {"S": S, "D": D, "Q": Q, "K": K, "C": C},
              "rounds": args.rounds, "calls_per_round": args.calls, "unit": "microseconds per call, median round", "cases": {}}
    legs = args.legs.split(",")
    if "operators" not in legs and os.path.exists(args.out):       # a leg on its own keeps the other legs' record
        with open(args.out) as f:
            result = json.load(f)
    for b in (8, 64) if "operators" in legs else ():
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
    if "module_step" in legs:
        result["module_step"] = module_step_leg(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
