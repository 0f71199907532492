"""Time per call of SentiDebias-PLM's generator and discriminator lines (csrc/debias.hip through manner_amd.hip / manner_amd.train) and of
the two optimiser steps built on them, at the reference's shapes: D = 768, discriminator hidden H = 400, sentiment embedding E = 256,
C = O = 4 sentiment classes, S = 50 history rows per user; C_cand = 5 candidates per user forward + backward (training) and C_cand = 40
forward only (validation: the ``no_grad`` path), for B = 8 and 64 users — N = B (S + C_cand) news rows.

Each figure stands beside two baselines, alternated with it in one process:
  (a) ``torch_f32``  the module's lines as float32 torch on the same device: ``nn.Embedding`` + ``nn.Linear`` + ``tanh`` over all N
      sentiment rows, ``to_dense_batch``, ``bmm``, the cosine lines, the discriminator's two ``nn.Linear`` and ``nn.CrossEntropyLoss``
      against a one-hot matrix.  The module fills that matrix with a Python loop over the rows (one device write and one index read per
      row); here it is ONE ``scatter_``, which favours the baseline by the whole loop;
  (b) ``composed``   what the library offered before csrc/debias.hip: ``train.embedding`` + ``train.linear_tanh`` for the N sentiment
      rows, ``train.to_dense``, ``train.dot``, ``train.linear_tanh`` + ``train.head_ce_loss`` per row set for the discriminator (the
      wrapped target formed by torch); the cosine lines have no earlier kernel and stay torch's.

The ``orth`` and ``senti_scores`` figures include forming the class table (``train.class_table``: ``linear_tanh`` on C rows), since both
baselines pay for the sentiment encoder inside them.

Method: every variant is warmed up, then timed in alternating rounds of ``--calls`` calls each with one device synchronise around the
round; the figure is the median round over the calls.  These shapes are launch-bound: the figures are host-enqueue plus kernel time of a
handful of small launches, not a share of any peak.  The ``module_step`` leg times ``hotpath.senti_debias_generator_step`` and
``senti_debias_discriminator_step`` over encoder-free stub news vectors (an embedding lookup) beside (a).

    python tools/debias_probe.py [--rounds 9] [--calls 100] [--step-calls 20] [--legs operators,module_step] [--out profiles/debias/probe.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]

from aspect_probe import measure  # noqa: E402
from manner_amd import hip, hotpath, train  # noqa: E402
from manner_amd.models.components.click_predictors import DotProduct  # noqa: E402
from manner_amd.models.components.user_encoder import NRMSUserEncoder  # noqa: E402
from miner_probe import to_dense_batch  # noqa: E402
from side_ops_ref import randn  # noqa: E402

DEV = "cuda:0"
S, D, H, E, C, Q, HEADS = 50, 768, 400, 256, 4, 200, 16
ALPHA, BETA = 0.15, 10.0
SHAPES = (("forward_backward", 5), ("forward", 40))


def make_batch(b, c, seed):
    hist_n = [S - (i % 5) * 7 for i in range(b)]
    n_hist, n_cand = sum(hist_n), b * c
    gen = torch.Generator().manual_seed(seed)

    def tok(lo, hi):
        ids = torch.arange(lo, hi, device=DEV).reshape(-1, 1)
        return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
    labels = torch.zeros(b, c)
    labels[:, 0] = 1.0
    return {"users": torch.arange(b, device=DEV), "batch_hist": torch.repeat_interleave(torch.arange(b), torch.tensor(hist_n)).to(DEV),
            "batch_cand": torch.repeat_interleave(torch.arange(b), c).to(DEV), "labels": labels.reshape(-1).to(DEV),
            "x_hist": {"text": tok(0, n_hist), "sentiment": torch.randint(0, C, (n_hist,), generator=gen).to(DEV)},
            "x_cand": {"text": tok(n_hist, n_hist + n_cand), "sentiment": torch.randint(0, C, (n_cand,), generator=gen).to(DEV)},
            "hist_max": max(hist_n), "cand_max": c}, n_hist, n_cand


def cos_eps(a, b):
    return torch.div(torch.sum(a * b, dim=-1), 1e-8 + torch.linalg.norm(a, dim=1, ord=2) * torch.linalg.norm(b, dim=1, ord=2))


def orth_lines(hist, cand, senti_hist, senti_cand, uf, ua):
    return (torch.abs(torch.mean(cos_eps(hist, senti_hist))) + torch.abs(torch.mean(cos_eps(cand, senti_cand))) + torch.abs(cos_eps(uf, ua))).mean()


def adversarial_loss(preds, targets):
    """the module's adversarial_loss with its row loop as one scatter_ (module docstring)"""
    y_true = torch.zeros_like(preds).scatter_(1, ((targets - 1) % preds.shape[1]).unsqueeze(1), 1.0)
    return F.cross_entropy(preds, y_true)


class SentimentEncoder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.embedding_layer = torch.nn.Embedding(C, E, padding_idx=0)
        self.linear = torch.nn.Linear(E, D)

    def forward(self, sentiment):
        return torch.tanh(self.linear(self.embedding_layer(sentiment)))


class Discriminator(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.linear1, self.linear2 = torch.nn.Linear(D, H), torch.nn.Linear(H, C)

    def forward(self, x):
        return self.linear2(torch.tanh(self.linear1(x)))


def runner(grad, leaves):
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
    return run


def operators_leg(args):
    out = {}
    for b in (8, 64):
        for what, c in SHAPES:
            batch, n_hist, n_cand = make_batch(b, c, 100 + b + c)
            n, grad = n_hist + n_cand, what == "forward_backward"
            torch.manual_seed(b + c)
            senti, disc = SentimentEncoder().to(DEV), Discriminator().to(DEV)
            rows = randn(1, n, D).to(DEV).requires_grad_(grad)
            uf, ua = randn(2, b, D).to(DEV).requires_grad_(grad), randn(3, b, D).to(DEV).requires_grad_(grad)
            cls_h, cls_c = batch["x_hist"]["sentiment"], batch["x_cand"]["sentiment"]
            cls = torch.cat((cls_h, cls_c))
            hist_off, cand_off = hotpath.segment_offsets(batch["batch_hist"], b), hotpath.segment_offsets(batch["batch_cand"], b)
            s_max = batch["hist_max"]
            emb, lin = senti.embedding_layer, senti.linear
            dw = [disc.linear1.weight, disc.linear1.bias, disc.linear2.weight, disc.linear2.bias]
            for p in list(senti.parameters()) + dw:
                p.requires_grad_(grad)
            leaves = [rows, uf, ua] + list(senti.parameters()) + dw
            run = runner(grad, leaves)
            T = train if grad else hip

            def table():
                return train.class_table(emb.weight, lin.weight, lin.bias)

            def rows_composed(ids):
                e = train.embedding(ids, emb.weight, 0)              # under no_grad the same kernel, nothing saved
                return (train.linear_tanh if grad else hip.linear_tanh)(e, lin.weight, lin.bias)

            def scores_ours():
                t = table()
                return T.class_dense(t, cls_h, hist_off, s_max).sum() + T.class_scores(ua, t, cls_c, cand_off).sum()

            def scores_torch():
                hd, _ = to_dense_batch(senti(cls_h), batch["batch_hist"], b)
                cd, _ = to_dense_batch(senti(cls_c), batch["batch_cand"], b)
                return hd.sum() + torch.bmm(ua.unsqueeze(dim=1), cd.permute(0, 2, 1)).squeeze(dim=1).sum()

            def scores_composed():
                dense_of, dot = (train.to_dense, train.dot) if grad else (hip.to_dense, hip.dot)
                hd, cd = dense_of(rows_composed(cls_h), hist_off, s_max), dense_of(rows_composed(cls_c), cand_off, c)
                return hd.sum() + dot(ua.unsqueeze(1), cd.permute(0, 2, 1)).sum()

            def adv_composed():
                lt = train.linear_tanh if grad else hip.linear_tanh
                ce = train.head_ce_loss if grad else hip.head_ce_loss
                return sum(ce(lt(r, dw[0], dw[1]), dw[2], dw[3], (t - 1) % C) for r, t in ((rows[:n_hist], cls_h), (rows[n_hist:], cls_c)))

            ops = {
                "orth": {"hip": lambda: T.orth_loss(rows, n_hist, table(), cls, uf, ua),
                         "torch_f32": lambda: orth_lines(rows[:n_hist], rows[n_hist:], senti(cls_h), senti(cls_c), uf, ua),
                         "composed": lambda: orth_lines(rows[:n_hist], rows[n_hist:], rows_composed(cls_h), rows_composed(cls_c), uf, ua)},
                "senti_scores": {"hip": scores_ours, "torch_f32": scores_torch, "composed": scores_composed},
                "adv": {"hip": lambda: T.adv_loss(rows, n_hist, *dw, cls),
                        "torch_f32": lambda: adversarial_loss(disc(rows[:n_hist]), cls_h) + adversarial_loss(disc(rows[n_hist:]), cls_c),
                        "composed": adv_composed},
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


def generator_today(enc, user_encoder, senti, click, disc, batch):
    """Generator.forward and the generator half of training_step as the unchanged module runs them over the mirror classes"""
    nb = batch["users"].numel()
    hist_vec, cand_vec = enc(batch["x_hist"]["text"]), enc(batch["x_cand"]["text"])
    hist_dense, _ = to_dense_batch(hist_vec, batch["batch_hist"], nb)
    cand_dense, _ = to_dense_batch(cand_vec, batch["batch_cand"], nb)
    senti_hist, senti_cand = senti(batch["x_hist"]["sentiment"]), senti(batch["x_cand"]["sentiment"])
    senti_hist_dense, _ = to_dense_batch(senti_hist, batch["batch_hist"], nb)
    senti_cand_dense, _ = to_dense_batch(senti_cand, batch["batch_cand"], nb)
    uf, ua = user_encoder(hist_dense), user_encoder(senti_hist_dense)
    orth = orth_lines(hist_vec, cand_vec, senti_hist, senti_cand, uf, ua)
    combined = click(uf.unsqueeze(dim=1), cand_dense.permute(0, 2, 1)) + click(ua.unsqueeze(dim=1), senti_cand_dense.permute(0, 2, 1))
    y_true, _ = to_dense_batch(batch["labels"], batch["batch_cand"], nb)
    adv = adversarial_loss(disc(hist_vec), batch["x_hist"]["sentiment"]) + adversarial_loss(disc(cand_vec), batch["x_cand"]["sentiment"])
    return F.cross_entropy(combined, y_true) + BETA * orth - ALPHA * adv


def module_step_leg(args):
    out = {}
    for b in (8, 64):
        for what, c in SHAPES:
            batch, n_hist, n_cand = make_batch(b, c, 200 + b + c)
            rows = torch.nn.Parameter(randn(7, n_hist + n_cand, D).to(DEV))
            torch.manual_seed(b + c)
            user_encoder, senti, disc, click = NRMSUserEncoder(D, HEADS, Q).to(DEV), SentimentEncoder().to(DEV), Discriminator().to(DEV), DotProduct()
            params = [rows] + list(user_encoder.parameters()) + list(senti.parameters()) + list(disc.parameters())
            grad = what == "forward_backward"
            run = runner(grad, params)

            def enc(tokens):
                return F.embedding(tokens["input_ids"][:, 0], rows)

            def disc_today():
                hist_vec, cand_vec = enc(batch["x_hist"]["text"]).detach(), enc(batch["x_cand"]["text"]).detach()
                return adversarial_loss(disc(hist_vec), batch["x_hist"]["sentiment"]) + adversarial_loss(disc(cand_vec), batch["x_cand"]["sentiment"])
            steps = {"generator": (lambda: hotpath.senti_debias_generator_step(enc, user_encoder, senti, disc, batch, ALPHA, BETA)[0],
                                   lambda: generator_today(enc, user_encoder, senti, click, disc, batch)),
                     "discriminator": (lambda: hotpath.senti_debias_discriminator_step(enc, disc, batch), disc_today)}
            for name, (ours, theirs) in steps.items():
                with torch.no_grad():
                    diff = float((ours() - theirs()).abs())
                rec = measure({"hip": run(ours), "torch_f32": run(theirs)}, args.rounds, args.step_calls)
                rec.update(rows=n_hist + n_cand, abs_difference_of_the_losses=diff)
                print(f"module_step {name} B={b} C={c} {what}: hip {rec['hip_us']} us, torch f32 {rec['torch_f32_us']} us", flush=True)
                out[f"{name}/B{b}/C{c}/{what}"] = rec
    hip.check_status(DEV)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--step-calls", type=int, default=20)
    ap.add_argument("--legs", default="operators,module_step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "debias", "probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("debias_probe: needs the GPU (a timing taken elsewhere says nothing)")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "shape": {"S": S, "D": D, "H": H, "E": E, "C": C, "O": C, "Q": Q, "heads": HEADS, "C_cand_forward_backward": 5, "C_cand_forward": 40},
              "rounds": args.rounds, "calls_per_round": args.calls, "step_calls_per_round": args.step_calls,
              "unit": "microseconds per call, median round",
              "baselines": {"torch_f32": "the module's lines in float32 torch over the mirror classes; the one-hot row loop of adversarial_loss as one "
                                         "scatter_, which favours this baseline",
                            "composed": "train.embedding + train.linear_tanh for the N sentiment rows, train.to_dense, train.dot, train.linear_tanh + "
                                        "train.head_ce_loss per row set; the cosine lines stay torch's"}}
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
