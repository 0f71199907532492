"""Golden vectors of the CAUM baseline's leaf classes -> tests/golden/caum.npz, tests/golden/caum_state_dict_keys.json.

Run in the build container only, like make_golden.py (it needs the reference checkout that make_golden.py puts on sys.path, and
transformers):

    python tests/golden/make_golden_caum.py

It imports the REFERENCE's own ``CAUMUserEncoder`` (manner/models/components/user_encoder.py:92-178), ``DenseAttention``
(attention.py:119-141), ``CAUMCategoryEncoder`` and ``CAUMNewsEncoder`` (news_encoder.py:331-434, over a tiny seeded HF BertModel
built from a config, with and without entities: entity dim 20 and 4 heads, head dim 5), runs them on seeded inputs a few units wide
and stores inputs, parameters, outputs and the autograd gradients of loss = sum(out * R) at dropout probability 0; the user encoder and
the dense attention are also run in float64 on the same values (``user64_*``, ``dense64_*``).  Only data goes
into the fixtures; no test reads the reference.
"""
import copy
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

from manner_amd.weights import make_mha_pool_weights  # noqa: E402

from manner.models.components.attention import DenseAttention  # noqa: E402
from manner.models.components.news_encoder import CAUMCategoryEncoder, CAUMNewsEncoder  # noqa: E402
from manner.models.components.user_encoder import CAUMUserEncoder  # noqa: E402

B, S, D, F, H1, H2, HEADS = 3, 7, 20, 24, 12, 8, 4
N_CATEG, CATEG_DIM = 9, 10
ENT_ROWS, ENT_DIM, ENT_HEADS, ENT_SLOTS, QUERY_DIM, TEXT_HEADS, NEWS_OUT = 13, 20, 4, 3, 16, 4, 20
ENC_N, ENC_LP, ENC_LENGTHS, ENC_ROWS = 5, 12, (2, 5, 9, 12, 7), 4
SEED = 67


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def reseed(module, rng, skip=()):
    """seeded values at scales that keep the tanh layers and the softmaxes in their curved range (the default init is near-linear)"""
    with torch.no_grad():
        for k, p in module.named_parameters():
            if any(k.startswith(s) for s in skip):
                continue
            p.copy_(rnd(rng, *p.shape, scale=0.1 if p.dim() == 1 else p.shape[-1] ** -0.5))


def main():
    torch.manual_seed(SEED)
    rng = np.random.default_rng(SEED)
    out, keys = {}, {}
    with torch.enable_grad():
        # ---- CAUMUserEncoder: one candidate per user
        ue = CAUMUserEncoder(news_vector_dim=D, num_filters=F, dense_att_hidden_dim1=H1, dense_att_hidden_dim2=H2, user_vector_dim=D,
                             num_attention_heads=HEADS, dropout_probability=0.0).train()
        reseed(ue, rng)
        keys["CAUMUserEncoder"] = {k: list(v.shape) for k, v in ue.state_dict().items()}
        x, c, up = rnd(rng, B, S, D).requires_grad_(True), rnd(rng, B, D).requires_grad_(True), rnd(rng, B)
        y = ue(x, c)
        (y * up).sum().backward()
        out.update(user_x=x.detach().numpy(), user_c=c.detach().numpy(), user_up=up.numpy(), user_out=y.detach().numpy(),
                   user_d_x=x.grad.numpy(), user_d_c=c.grad.numpy())
        for k, p in ue.named_parameters():
            out["user_sd:" + k], out["user_grad:" + k] = p.detach().numpy().copy(), p.grad.numpy().copy()
        # the same class in float64 on the same values: what the float64 restatement is held to at rel 1e-10
        ue64 = copy.deepcopy(ue).double()
        ue64.zero_grad()
        x64, c64 = x.detach().double().requires_grad_(True), c.detach().double().requires_grad_(True)
        y64 = ue64(x64, c64)
        (y64 * torch.from_numpy(out["user_up"]).double()).sum().backward()
        out.update(user64_out=y64.detach().numpy(), user64_d_x=x64.grad.numpy(), user64_d_c=c64.grad.numpy())
        for k, p in ue64.named_parameters():
            out["user64_grad:" + k] = p.grad.numpy().copy()
        # ---- DenseAttention alone: [.., 2U] -> [.., 1]
        da = DenseAttention(input_dim=2 * D, hidden_dim1=H1, hidden_dim2=H2)
        reseed(da, rng)
        keys["DenseAttention"] = {k: list(v.shape) for k, v in da.state_dict().items()}
        v, up = rnd(rng, B, S, 2 * D).requires_grad_(True), rnd(rng, B, S, 1)
        y = da(v)
        (y * up).sum().backward()
        out.update(dense_x=v.detach().numpy(), dense_up=up.numpy(), dense_out=y.detach().numpy(), dense_d_x=v.grad.numpy())
        for k, p in da.named_parameters():
            out["dense_sd:" + k], out["dense_grad:" + k] = p.detach().numpy().copy(), p.grad.numpy().copy()
        da64 = copy.deepcopy(da).double()
        da64.zero_grad()
        v64 = v.detach().double().requires_grad_(True)
        y64 = da64(v64)
        (y64 * up.double()).sum().backward()
        out.update(dense64_out=y64.detach().numpy(), dense64_d_x=v64.grad.numpy())
        for k, p in da64.named_parameters():
            out["dense64_grad:" + k] = p.grad.numpy().copy()
        # ---- CAUMCategoryEncoder
        ce = CAUMCategoryEncoder(num_categories=N_CATEG, category_embedding_dim=CATEG_DIM, category_output_dim=CATEG_DIM,
                                 dropout_probability=0.0).train()
        reseed(ce, rng)
        keys["CAUMCategoryEncoder"] = {k: list(v.shape) for k, v in ce.state_dict().items()}
        categ = torch.from_numpy(rng.integers(0, N_CATEG, (ENC_N,)))
        categ[0] = 0                                           # the padding row
        up = rnd(rng, ENC_N, CATEG_DIM)
        y = ce(categ)
        (y * up).sum().backward()
        out.update(categ_ids=categ.numpy(), categ_up=up.numpy(), categ_out=y.detach().numpy())
        for k, p in ce.named_parameters():
            out["categ_sd:" + k], out["categ_grad:" + k] = p.detach().numpy().copy(), p.grad.numpy().copy()
        # ---- CAUMNewsEncoder over tiny-bert, with and without entities
        cfg = PRESETS["tiny-bert"]
        w = make_plm_weights(cfg, seed=SEED, std=0.05)
        ids, amask = synth_news_tokens(ENC_N, cfg, seed=SEED, max_len=ENC_LP, lengths=np.array(ENC_LENGTHS))
        entities = rng.integers(0, ENT_ROWS, (ENC_N, ENT_SLOTS))
        entities[1, 1:] = 0                                    # padded entity slots
        table = (rng.standard_normal((ENT_ROWS, ENT_DIM)) * 0.5).astype(np.float32)
        R = rnd(rng, ENC_N, NEWS_OUT)
        out.update(news_ids=ids, news_mask=amask, news_categ=categ.numpy(), news_entities=entities, news_entity_table=table, news_R=R.numpy())
        frozen = None
        for tag, use_entities in (("ent", True), ("noent", False)):
            news = {"text": {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(amask)}, "category": categ,
                    "entities": torch.from_numpy(entities)}
            with tempfile.TemporaryDirectory() as tmp:
                ne = CAUMNewsEncoder(plm_model=hf_model_dir(cfg, w, tmp, no_dropout=True), frozen_layers=[0], text_embedding_dim=cfg.hidden,
                                     text_num_attention_heads=TEXT_HEADS, query_vector_dim=QUERY_DIM, dropout_probability=0.0,
                                     num_categories=N_CATEG, category_embedding_dim=CATEG_DIM, use_entities=use_entities,
                                     entity_embeddings=torch.from_numpy(table), entity_embedding_dim=ENT_DIM,
                                     entity_num_attention_heads=ENT_HEADS, news_out_embedding_dim=NEWS_OUT)
            reseed(ne, rng, skip=("text_encoder.", "entity_encoder.pretrained_embedding."))
            mw = make_mha_pool_weights(cfg.hidden, QUERY_DIM, seed=SEED, prefix="text_encoder.")     # regenerated by the tests, not stored
            missing, unexpected = ne.load_state_dict({k: torch.from_numpy(v) for k, v in mw.items()}, strict=False)
            assert not unexpected, unexpected
            keys["CAUMNewsEncoder" + ("" if use_entities else "_no_entities")] = {k: list(v.shape) for k, v in ne.state_dict().items()}
            with torch.no_grad():
                out[f"news_{tag}_out_eval"] = ne.eval()(news).numpy()
            y = ne.train()(news)
            (y * R).sum().backward()
            out[f"news_{tag}_out"] = y.detach().numpy()
            frozen = []
            for k, p in ne.named_parameters():
                if k.startswith("text_encoder.plm_model."):      # the layout of make_golden.gen_train
                    short = k[len("text_encoder.plm_model."):]
                    if short.startswith("pooler."):
                        continue
                    if not use_entities and p.grad is not None:  # the PLM's gradients are kept once, with entities
                        continue
                    if p.grad is None:
                        frozen.append(short)
                        continue
                    g = p.grad.numpy()
                    if short == "embeddings.word_embeddings.weight":
                        rows = np.unique(ids[amask > 0])
                        rest = np.ones(g.shape[0], bool)
                        rest[rows] = False
                        out[f"news_{tag}_word_rows"], out[f"news_{tag}_word_rest_abs_sum"] = rows, np.float64(np.abs(g[rest]).sum())
                        g = g[rows]
                    elif g.ndim == 2 and not short.startswith("embeddings."):
                        g = g[:ENC_ROWS]
                    out[f"news_{tag}_grad:" + short] = np.ascontiguousarray(g)
                else:
                    g = p.grad.numpy().copy()
                    if k.startswith("text_encoder."):          # seeded (make_mha_pool_weights): not stored; wide gradients by their first rows
                        g = g[:ENC_ROWS] if g.ndim == 2 and g.shape[0] > 32 else g
                    else:
                        out[f"news_{tag}_sd:" + k] = p.detach().numpy().copy()
                    out[f"news_{tag}_pgrad:" + k] = np.ascontiguousarray(g)
    meta = {"source": "reference CAUMUserEncoder (user_encoder.py:92-178), DenseAttention (attention.py:119-141), CAUMCategoryEncoder / "
                      "CAUMNewsEncoder (news_encoder.py:331-434) over HF transformers " + __import__("transformers").__version__
                      + ", torch " + torch.__version__ + "; gradients of loss = sum(out * up), dropout probability 0",
            "seed": SEED, "shape": {"B": B, "S": S, "D": D, "F": F, "H1": H1, "H2": H2, "heads": HEADS},
            "news": {"preset": "tiny-bert", "seed": SEED, "std": 0.05, "frozen_layers": [0], "frozen": frozen, "matrix_rows": ENC_ROWS,
                     "text_heads": TEXT_HEADS, "query_dim": QUERY_DIM, "num_categories": N_CATEG, "category_dim": CATEG_DIM,
                     "entity_dim": ENT_DIM, "entity_heads": ENT_HEADS, "news_out": NEWS_OUT}}
    path = os.path.join(HERE, "caum.npz")
    np.savez_compressed(path, **out, meta=json.dumps(meta))
    with open(os.path.join(HERE, "caum_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays;", len(frozen), "frozen tensors")


if __name__ == "__main__":
    main()
