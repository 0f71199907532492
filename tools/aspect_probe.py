"""Time per call of the auxiliary heads and losses of TANR-PLM and SentiRec-PLM (csrc/aspect.hip through manner_amd.hip / manner_amd.train)
and of the two training steps built on them, at the reference's shapes: D = 768, S = 50 history rows per user, 19 topics; C = 5 candidates
per user forward + backward (training) and C = 40 forward only (validation: the ``no_grad`` path), for B = 8 and 64 users — N = B (S + C)
news rows: 440 / 3 520 and 720 / 5 760.

Each figure stands beside two baselines, alternated with it in one process:
  (a) ``torch_f32``  the same lines as float32 torch on the same device — what the unchanged module runs today over the mirror classes:
      ``torch.cat`` of the rows, ``F.one_hot``, ``nn.CrossEntropyLoss`` / ``nn.L1Loss``, the dense blocks and, in SentiRec, the
      per-impression Python loop with its host read;
  (b) ``composed``   what the library could already do without csrc/aspect.hip: ``train.linear`` (``hip.linear`` forward only) followed by
      the existing loss kernel ``train.model_step_loss(supcon=False)`` on N uniform segments of O logits (the L1 head has no such kernel:
      its (b) is ``train.linear`` + torch's ``abs().mean()``; the regulariser has no (b)).

Method: every variant is warmed up, then timed in alternating rounds of ``--calls`` calls each with one device synchronise around the
round; the figure is the median round over the calls.  These shapes are launch-bound: the figures are host-enqueue plus kernel time of a
handful of small launches, not a share of any peak.  The ``module_step`` leg times ``hotpath.tanr_train_step`` /
``hotpath.sentirec_train_step`` over encoder-free stub news vectors (an embedding lookup) beside (a).

    python tools/aspect_probe.py [--rounds 9] [--calls 100] [--step-calls 20] [--legs operators,module_step] [--out profiles/aspect/probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

from manner_amd import hip, hotpath, train  # noqa: E402
from manner_amd.models.components.click_predictors import DotProduct  # noqa: E402
from manner_amd.models.components.user_encoder import NAMLUserEncoder, NRMSUserEncoder  # noqa: E402
from miner_probe import timed, to_dense_batch  # noqa: E402
from side_ops_ref import randn  # noqa: E402

DEV = "cuda:0"
S, D, O, Q, HEADS = 50, 768, 19, 200, 16
TOPIC_COEF, SENTI_PRED_COEF, SENTI_DIV_COEF = 0.2, 0.4, 10.0
SHAPES = (("forward_backward", 5), ("forward", 40))


def measure(fns, rounds, calls, warm=5):
    """{name: fn} -> {name_us: median round, name_min_max_us: [min, max]}, the variants alternated round by round"""
    for f in fns.values():
        timed(f, warm)
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(timed(f, calls))
    rec = {}
    for k, v in got.items():
        rec[k + "_us"] = round(statistics.median(v), 2)
        rec[k + "_min_max_us"] = [round(min(v), 2), round(max(v), 2)]
    return rec


def make_batch(b, c, seed):
    hist_n = [S - (i % 5) * 7 for i in range(b)]
    n_hist, n_cand = sum(hist_n), b * c
    gen = torch.Generator().manual_seed(seed)

    def tok(lo, hi):
        ids = torch.arange(lo, hi, device=DEV).reshape(-1, 1)
        return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}

    def senti(n):
        return (torch.rand(n, generator=gen) * 2 - 1).to(DEV)
    labels = torch.zeros(b, c)
    labels[:, 0] = 1.0
    return {"users": torch.arange(b, device=DEV), "batch_hist": torch.repeat_interleave(torch.arange(b), torch.tensor(hist_n)).to(DEV),
            "batch_cand": torch.repeat_interleave(torch.arange(b), c).to(DEV), "labels": labels.reshape(-1).to(DEV),
            "x_hist": {"text": tok(0, n_hist), "category": torch.randint(0, O, (n_hist,), generator=gen).to(DEV), "sentiment_score": senti(n_hist)},
            "x_cand": {"text": tok(n_hist, n_hist + n_cand), "category": torch.randint(0, O, (n_cand,), generator=gen).to(DEV),
                       "sentiment_score": senti(n_cand)},
            "hist_max": max(hist_n), "cand_max": c}, n_hist, n_cand


def senti_div_today(scores_dense, batch, nb):
    """sentirec_plm_module.py:180-192 as the module runs it: dense blocks and the per-impression loop with its host read"""
    senti_hist, mask_hist = to_dense_batch(batch["x_hist"]["sentiment_score"], batch["batch_hist"], nb)
    senti_cand, _ = to_dense_batch(batch["x_cand"]["sentiment_score"], batch["batch_cand"], nb)
    hist_size = torch.tensor([torch.where(mask_hist[i])[0].shape[0] for i in range(mask_hist.shape[0])], device=scores_dense.device)
    user_mean = torch.div(senti_hist.sum(dim=1), hist_size)
    return F.relu(user_mean.unsqueeze(dim=-1) * senti_cand * scores_dense).mean()


def operators_leg(args):
    out = {}
    for b in (8, 64):
        for what, c in SHAPES:
            batch, n_hist, n_cand = make_batch(b, c, 100 + b + c)
            n = n_hist + n_cand
            grad = what == "forward_backward"
            x = randn(1, n, D).to(DEV).requires_grad_(grad)
            w, bias = (randn(2, O, D, scale=D ** -0.5).to(DEV).requires_grad_(grad), randn(3, O, scale=0.1).to(DEV).requires_grad_(grad))
            w1, b1 = (randn(4, 1, D, scale=D ** -0.5).to(DEV).requires_grad_(grad), randn(5, 1, scale=0.1).to(DEV).requires_grad_(grad))
            topics = torch.cat((batch["x_hist"]["category"], batch["x_cand"]["category"]))
            senti = torch.cat((batch["x_hist"]["sentiment_score"], batch["x_cand"]["sentiment_score"]))
            one_hot_flat = F.one_hot(topics, num_classes=O).float().reshape(-1)
            uniform = torch.arange(n + 1, device=DEV) * O
            hist_off = hotpath.segment_offsets(batch["batch_hist"], b)
            cand_off = hotpath.segment_offsets(batch["batch_cand"], b)
            scores = randn(6, n_cand).to(DEV).requires_grad_(grad)
            leaves = [x, w, bias, w1, b1, scores]

            def run(fn):
                def go():
                    if grad:
                        for t in leaves:
                            t.grad = None
                        fn().backward()
                    else:
                        with torch.no_grad():
                            fn()
                return go
            lin = train.linear if grad else hip.linear
            ops = {
                "head_ce": {"hip": lambda: (train.head_ce_loss if grad else hip.head_ce_loss)(x, w, bias, topics),
                            "torch_f32": lambda: F.cross_entropy(F.linear(x, w, bias), F.one_hot(topics, num_classes=O).type_as(x)),
                            "composed": lambda: train.model_step_loss(lin(x, w, bias).reshape(-1), one_hot_flat, uniform, supcon=False, c_max=O)[0]},
                "head_l1": {"hip": lambda: (train.head_l1_loss if grad else hip.head_l1_loss)(x, w1, b1, senti),
                            "torch_f32": lambda: F.l1_loss(F.linear(x, w1, b1).flatten(), senti),
                            "composed": lambda: (lin(x, w1, b1).flatten() - senti).abs().mean()},
                "senti_div": {"hip": lambda: (train.senti_div_loss if grad else hip.senti_div_loss)(scores, batch["x_cand"]["sentiment_score"],
                                                                                                     batch["x_hist"]["sentiment_score"], hist_off, cand_off, c),
                              "torch_f32": lambda: senti_div_today(to_dense_batch(scores, batch["batch_cand"], b)[0], batch, b)},
            }
            for name, fns in ops.items():
                with torch.no_grad():
                    values = {k: float(f()) for k, f in fns.items()}
                rec = measure({k: run(f) for k, f in fns.items()}, args.rounds, args.calls)
                rec.update(rows=n, values=values)
                print(f"B={b} C={c} {name} {what}: " + ", ".join(f"{k} {rec[k + '_us']} us" for k in fns), flush=True)
                out[f"B{b}/C{c}/{name}/{what}"] = rec
    hip.check_status(DEV)
    return out


def module_lines_today(kind, enc, user_encoder, click, head, batch):
    """TANRPLMModule / SentiRecPLMModule forward and the loss lines of model_step as the unchanged module runs them over the mirror classes"""
    nb = batch["users"].numel()
    hist_vec, cand_vec = enc(batch["x_hist"]["text"]), enc(batch["x_cand"]["text"])
    hist_dense, _ = to_dense_batch(hist_vec, batch["batch_hist"], nb)
    cand_dense, _ = to_dense_batch(cand_vec, batch["batch_cand"], nb)
    scores = click(user_encoder(hist_dense).unsqueeze(dim=1), cand_dense.permute(0, 2, 1))
    aux = head(torch.cat((cand_vec, hist_vec), dim=0))
    y_true, _ = to_dense_batch(batch["labels"], batch["batch_cand"], nb)
    loss = F.cross_entropy(scores, y_true)
    if kind == "tanr":
        topics = torch.cat((batch["x_cand"]["category"], batch["x_hist"]["category"]))
        return loss + TOPIC_COEF * F.cross_entropy(aux, F.one_hot(topics, num_classes=O).type_as(aux))
    senti = torch.cat((batch["x_cand"]["sentiment_score"], batch["x_hist"]["sentiment_score"]))
    return loss + SENTI_PRED_COEF * F.l1_loss(aux.flatten(), senti) + SENTI_DIV_COEF * senti_div_today(scores, batch, nb)


def module_step_leg(args):
    out = {}
    for kind in ("tanr", "sentirec"):
        for b in (8, 64):
            for what, c in SHAPES:
                batch, n_hist, n_cand = make_batch(b, c, 200 + b + c)
                rows = torch.nn.Parameter(randn(7, n_hist + n_cand, D).to(DEV))
                torch.manual_seed(b + c)
                user_encoder = (NAMLUserEncoder(D, Q) if kind == "tanr" else NRMSUserEncoder(D, HEADS, Q)).to(DEV)
                head, click = torch.nn.Linear(D, O if kind == "tanr" else 1).to(DEV), DotProduct()
                params = [rows] + list(user_encoder.parameters()) + list(head.parameters())
                grad = what == "forward_backward"

                def enc(tokens):
                    return F.embedding(tokens["input_ids"][:, 0], rows)

                def ours_loss():
                    if kind == "tanr":
                        return hotpath.tanr_train_step(enc, user_encoder, head, batch, TOPIC_COEF)[0]
                    return hotpath.sentirec_train_step(enc, user_encoder, head, batch, SENTI_PRED_COEF, SENTI_DIV_COEF)[0]

                def theirs_loss():
                    return module_lines_today(kind, enc, user_encoder, click, head, batch)

                def run(fn):
                    def go():
                        if grad:
                            for t in params:
                                t.grad = None
                            fn().backward()
                        else:
                            with torch.no_grad():
                                fn()
                    return go
                with torch.no_grad():
                    diff = float((ours_loss() - theirs_loss()).abs())
                rec = measure({"hip": run(ours_loss), "torch_f32": run(theirs_loss)}, args.rounds, args.step_calls)
                rec.update(rows=n_hist + n_cand, abs_difference_of_the_losses=diff)
                print(f"module_step {kind} B={b} C={c} {what}: hip {rec['hip_us']} us, torch f32 {rec['torch_f32_us']} us", flush=True)
                out[f"{kind}/B{b}/C{c}/{what}"] = rec
    hip.check_status(DEV)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--step-calls", type=int, default=20)
    ap.add_argument("--legs", default="operators,module_step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aspect", "probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aspect_probe: needs the GPU (a timing taken elsewhere says nothing)")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "shape": {"S": S, "D": D, "O": O, "Q": Q, "heads": HEADS, "C_forward_backward": 5, "C_forward": 40},
              "rounds": args.rounds, "calls_per_round": args.calls, "step_calls_per_round": args.step_calls,
              "unit": "microseconds per call, median round",
              "baselines": {"torch_f32": "the same lines in float32 torch over the mirror classes",
                            "composed": "train.linear (hip.linear forward only) + train.model_step_loss(supcon=False) on N uniform segments "
                                        "of O logits; for the L1 head train.linear + torch abs().mean()"}}
    legs = args.legs.split(",")
    if os.path.exists(args.out):                                   # a leg on its own keeps the other leg's record
        with open(args.out) as f:
            old = json.load(f)
        result.update({k: old[k] for k in ("operators", "module_step") if k in old})
    if "operators" in legs:
        result["operators"] = operators_leg(args)
    if "module_step" in legs:
        result["module_step"] = module_step_leg(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
