"""Golden vectors of the MINER baseline's leaf classes -> tests/golden/miner.npz, tests/golden/miner_state_dict_keys.json.

Run in the build container only, like make_golden.py (it needs the reference checkout that make_golden.py puts on sys.path, and
transformers):

    python tests/golden/make_golden_miner.py

It imports the REFERENCE's own ``PolyAttention``, ``TargetAwareAttention`` (manner/models/components/attention.py:32-116),
``DotProduct`` (click_predictors.py:5-12) and ``MINERNewsEncoder`` (news_encoder.py:297-328, over a tiny seeded HF BertModel
built from a config), runs them on seeded inputs a few units wide and stores inputs, parameters, outputs and the autograd
gradients of loss = sum(out * R) at dropout probability 0.  Only data goes into the fixtures; no test reads the reference.
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import PRESETS, hf_model_dir, make_plm_weights, synth_news_tokens  # noqa: E402  (puts the reference on sys.path)

from manner.models.components.attention import PolyAttention, TargetAwareAttention  # noqa: E402
from manner.models.components.click_predictors import DotProduct  # noqa: E402
from manner.models.components.news_encoder import MINERNewsEncoder  # noqa: E402

B, S, D, Q, K, C, T = 3, 7, 64, 24, 5, 6, 11
HIST = (7, 4, 1)                       # ragged histories: the mask of to_dense_batch
ENC_N, ENC_LP, ENC_LENGTHS, ENC_OUT, ENC_ROWS = 5, 12, (2, 5, 9, 12, 7), 24, 4
SEED = 61


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def grads_of(out, upstream, leaves):
    (out * upstream).sum().backward()
    res = {k: v.grad.detach().numpy().copy() for k, v in leaves.items()}
    for v in leaves.values():
        v.grad = None
    return res


def main():
    torch.manual_seed(SEED)
    rng = np.random.default_rng(SEED)
    out, keys = {}, {}
    with torch.enable_grad():
        # ---- PolyAttention: ragged mask, x non-zero at masked slots too (the kernel may not assume to_dense_batch's zeros)
        poly = PolyAttention(input_embed_dim=D, num_context_codes=K, context_code_dim=Q)
        keys["PolyAttention"] = {k: list(v.shape) for k, v in poly.state_dict().items()}
        x = rnd(rng, B, S, D).requires_grad_(True)
        mask = torch.zeros(B, S, dtype=torch.bool)
        for b, h in enumerate(HIST):
            mask[b, :h] = True
        bias = rnd(rng, B, S, T, scale=0.5)
        bias[:, :, 3:5] = 0.0                                  # the caller zeroes the user's own candidates' columns
        up = rnd(rng, B, K, D)
        leaves = {"x": x, "lin_w": poly.linear.weight, "codes": poly.context_codes}
        out.update(poly_x=x.detach().numpy(), poly_mask=mask.numpy(), poly_bias=bias.numpy(), poly_up=up.numpy(),
                   poly_lin_w=poly.linear.weight.detach().numpy().copy(), poly_codes=poly.context_codes.detach().numpy().copy())
        for tag, bb in (("nobias", None), ("bias", bias)):
            y = poly(clicked_news_vector=x, attn_mask=mask, bias=None if bb is None else bb.clone())
            out[f"poly_{tag}_out"] = y.detach().numpy()
            for k, g in grads_of(y, up, leaves).items():
                out[f"poly_{tag}_d_{k}"] = g
        # ---- TargetAwareAttention, one zero-padded candidate row (to_dense_batch)
        tgt = TargetAwareAttention(input_embed_dim=D)
        keys["TargetAwareAttention"] = {k: list(v.shape) for k, v in tgt.state_dict().items()}
        query, key, value = rnd(rng, B, K, D, scale=0.5), rnd(rng, B, C, D, scale=0.5), rnd(rng, B, C, K)
        key[1, C - 1] = 0.0
        value[1, C - 1] = 0.0
        leaves = {"query": query.requires_grad_(True), "key": key.requires_grad_(True), "value": value.requires_grad_(True),
                  "lin_w": tgt.linear.weight}
        up = rnd(rng, B, C)
        y = tgt(query=query, key=key, value=value)
        out.update(target_query=query.detach().numpy(), target_key=key.detach().numpy(), target_value=value.detach().numpy(),
                   target_lin_w=tgt.linear.weight.detach().numpy().copy(), target_up=up.numpy(), target_out=y.detach().numpy())
        for k, g in grads_of(y, up, leaves).items():
            out[f"target_d_{k}"] = g
        # ---- DotProduct as MINERModule.forward calls it: [B, C, D] x permuted [B, K, D]
        cand, user = rnd(rng, B, C, D).requires_grad_(True), rnd(rng, B, K, D).requires_grad_(True)
        up = rnd(rng, B, C, K)
        y = DotProduct()(cand, user.permute(0, 2, 1))
        out.update(dot_cand=cand.detach().numpy(), dot_user=user.detach().numpy(), dot_up=up.numpy(), dot_out=y.detach().numpy())
        for k, g in grads_of(y, up, {"cand": cand, "user": user}).items():
            out[f"dot_d_{k}"] = g
        # ---- MINERNewsEncoder over tiny-bert
        cfg = PRESETS["tiny-bert"]
        w = make_plm_weights(cfg, seed=SEED, std=0.05)
        ids, amask = synth_news_tokens(ENC_N, cfg, seed=SEED, max_len=ENC_LP, lengths=np.array(ENC_LENGTHS))
        batch = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(amask)}
        R = rnd(rng, ENC_N, ENC_OUT)
        with tempfile.TemporaryDirectory() as tmp:
            plm_dir = hf_model_dir(cfg, w, tmp, no_dropout=True)
            enc = MINERNewsEncoder(plm_model=plm_dir, frozen_layers=[0], apply_reduce_dim=True, text_embedding_dim=cfg.hidden,
                                   news_embedding_dim=ENC_OUT, dropout_probability=0.0)
            plain = MINERNewsEncoder(plm_model=plm_dir, frozen_layers=[0], apply_reduce_dim=False, text_embedding_dim=cfg.hidden,
                                     news_embedding_dim=ENC_OUT, dropout_probability=0.0)
        keys["MINERNewsEncoder"] = {k: list(v.shape) for k, v in enc.state_dict().items()}
        keys["MINERNewsEncoder_no_reduce_dim"] = {k: list(v.shape) for k, v in plain.state_dict().items()}
        with torch.no_grad():
            out["enc_out_eval"] = enc.eval()(batch).numpy()
            out["enc_cls_eval"] = plain.eval()(batch).numpy()
        y = enc.train()(batch)
        (y * R).sum().backward()
        frozen = []
        out.update(enc_ids=ids, enc_mask=amask, enc_R=R.numpy(), enc_out=y.detach().numpy(),
                   enc_reduce_w=enc.reduce_dim.weight.detach().numpy().copy(), enc_reduce_b=enc.reduce_dim.bias.detach().numpy().copy(),
                   enc_d_reduce_w=enc.reduce_dim.weight.grad.numpy(), enc_d_reduce_b=enc.reduce_dim.bias.grad.numpy())
        for k, p in enc.plm_model.named_parameters():         # the layout of make_golden.gen_train
            if k.startswith("pooler."):
                continue
            if p.grad is None:
                frozen.append(k)
                continue
            g = p.grad.numpy()
            if k == "embeddings.word_embeddings.weight":
                rows = np.unique(ids[amask > 0])
                rest = np.ones(g.shape[0], bool)
                rest[rows] = False
                out["enc_word_rows"], out["enc_word_rest_abs_sum"] = rows, np.float64(np.abs(g[rest]).sum())
                g = g[rows]
            elif g.ndim == 2 and not k.startswith("embeddings."):
                g = g[:ENC_ROWS]
            out["enc_grad:" + k] = np.ascontiguousarray(g)
    meta = {"source": "reference PolyAttention / TargetAwareAttention (attention.py:32-116), DotProduct (click_predictors.py:5-12), "
                      "MINERNewsEncoder (news_encoder.py:297-328) over HF transformers " + __import__("transformers").__version__
                      + ", torch " + torch.__version__ + "; gradients of loss = sum(out * up), dropout probability 0",
            "seed": SEED, "shape": {"B": B, "S": S, "D": D, "Q": Q, "K": K, "C": C, "T": T}, "hist": list(HIST),
            "encoder": {"preset": "tiny-bert", "seed": SEED, "std": 0.05, "frozen_layers": [0], "frozen": frozen, "matrix_rows": ENC_ROWS,
                        "news_embedding_dim": ENC_OUT}}
    path = os.path.join(HERE, "miner.npz")
    np.savez_compressed(path, **out, meta=json.dumps(meta))
    with open(os.path.join(HERE, "miner_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays;", len(frozen), "frozen tensors")


if __name__ == "__main__":
    main()
