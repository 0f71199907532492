"""Golden vectors of the LSTUR baseline's leaf classes -> tests/golden/lstur.npz, tests/golden/lstur_state_dict_keys.json.

Run in the build container only, like make_golden.py (it needs the reference checkout that make_golden.py puts on sys.path, and
transformers):

    python tests/golden/make_golden_lstur.py

It imports the REFERENCE's own ``LSTURUserEncoder`` (manner/models/components/user_encoder.py:45-89, both long_short_term_methods),
``LSTURCategoryEncoder`` and ``LSTURNewsEncoder`` (news_encoder.py:239-294, over a tiny seeded HF BertModel built from a config), runs
them on seeded inputs a few units wide — user ids [1, 0, 3, 3] (the padding row and a repeated user), history lengths [5, 1, 3, 2] of
5 slots — and stores inputs, parameters, outputs and the autograd gradients of loss = sum(out * R) at masking probability 0; the user
encoder is also run in float64 on the same values (``user64_*``).  Only data goes into the fixtures; no test reads the reference.
"""
import copy
import json
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import PRESETS, hf_model_dir, make_plm_weights, synth_news_tokens  # noqa: E402  (puts the reference on sys.path)

from manner_amd.weights import make_mha_pool_weights  # noqa: E402

from manner.models.components.news_encoder import LSTURCategoryEncoder, LSTURNewsEncoder  # noqa: E402
from manner.models.components.user_encoder import LSTURUserEncoder  # noqa: E402

B, S, I, N_USERS = 4, 5, 6, 7
USER, LENGTHS = [1, 0, 3, 3], [5, 1, 3, 2]
N_CATEG, CATEG_DIM, QUERY_DIM, TEXT_HEADS = 9, 10, 16, 4
ENC_N, ENC_LP, ENC_LENGTHS, ENC_ROWS = 5, 12, (2, 5, 9, 12, 7), 4
SEED = 71


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def reseed_user(ue, rng):
    """seeded values that put the gates in their curved range (the default init, uniform in +- 1 / sqrt(H), is near-linear); row 0 of
    the table stays the zero row of padding_idx"""
    with torch.no_grad():
        for k, p in ue.named_parameters():
            p.copy_(rnd(rng, *p.shape, scale=0.3 if p.dim() == 1 else 0.7 if k.startswith("long_term") else 2.0 * p.shape[-1] ** -0.5))
        ue.long_term_user_embedding.weight[0].zero_()


def main():
    torch.manual_seed(SEED)
    rng = np.random.default_rng(SEED)
    out, keys = {}, {}
    user, lengths = torch.tensor(USER), torch.tensor(LENGTHS)
    x0 = rnd(rng, B, S, I)
    out.update(user=user.numpy(), lengths=lengths.numpy(), user_x=x0.numpy())
    with torch.enable_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # nn.Dropout2d on a 3-D input
        for method in ("ini", "con"):
            ue = LSTURUserEncoder(num_users=N_USERS, input_dim=I, user_masking_probability=0.0, long_short_term_method=method).train()
            reseed_user(ue, rng)
            keys["LSTURUserEncoder_" + method] = {k: list(v.shape) for k, v in ue.state_dict().items()}
            x = x0.clone().requires_grad_(True)
            y = ue(user, x, lengths)
            up = rnd(rng, *y.shape)
            (y * up).sum().backward()
            out.update({f"user_{method}_up": up.numpy(), f"user_{method}_out": y.detach().numpy(), f"user_{method}_d_x": x.grad.numpy()})
            for k, p in ue.named_parameters():
                out[f"user_{method}_sd:" + k], out[f"user_{method}_grad:" + k] = p.detach().numpy().copy(), p.grad.numpy().copy()
            # the same class in float64 on the same values: what the float64 restatement is held to at rel 1e-10
            ue64 = copy.deepcopy(ue).double()
            ue64.zero_grad()
            x64 = x0.double().requires_grad_(True)
            y64 = ue64(user, x64, lengths)
            (y64 * up.double()).sum().backward()
            out.update({f"user64_{method}_out": y64.detach().numpy(), f"user64_{method}_d_x": x64.grad.numpy()})
            for k, p in ue64.named_parameters():
                out[f"user64_{method}_grad:" + k] = p.grad.numpy().copy()
        # ---- LSTURCategoryEncoder
        ce = LSTURCategoryEncoder(num_categories=N_CATEG, category_embedding_dim=CATEG_DIM)
        keys["LSTURCategoryEncoder"] = {k: list(v.shape) for k, v in ce.state_dict().items()}
        categ = torch.from_numpy(rng.integers(1, N_CATEG, (ENC_N,)))
        categ[0] = 0                                               # the padding row
        categ[2] = categ[1]                                        # a repeated category
        up = rnd(rng, ENC_N, CATEG_DIM)
        y = ce(categ)
        (y * up).sum().backward()
        out.update(categ_ids=categ.numpy(), categ_up=up.numpy(), categ_out=y.detach().numpy())
        for k, p in ce.named_parameters():
            out["categ_sd:" + k], out["categ_grad:" + k] = p.detach().numpy().copy(), p.grad.numpy().copy()
        # ---- LSTURNewsEncoder over tiny-bert
        cfg = PRESETS["tiny-bert"]
        w = make_plm_weights(cfg, seed=SEED, std=0.05)
        ids, amask = synth_news_tokens(ENC_N, cfg, seed=SEED, max_len=ENC_LP, lengths=np.array(ENC_LENGTHS))
        R = rnd(rng, ENC_N, cfg.hidden + CATEG_DIM)
        out.update(news_ids=ids, news_mask=amask, news_categ=categ.numpy(), news_R=R.numpy())
        news = {"text": {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(amask)}, "category": categ}
        with tempfile.TemporaryDirectory() as tmp:
            ne = LSTURNewsEncoder(plm_model=hf_model_dir(cfg, w, tmp, no_dropout=True), frozen_layers=[0], text_embedding_dim=cfg.hidden,
                                  num_attention_heads=TEXT_HEADS, query_vector_dim=QUERY_DIM, dropout_probability=0.0, num_categories=N_CATEG,
                                  category_embedding_dim=CATEG_DIM)
        mw = make_mha_pool_weights(cfg.hidden, QUERY_DIM, seed=SEED, prefix="text_encoder.")         # regenerated by the tests, not stored
        missing, unexpected = ne.load_state_dict({k: torch.from_numpy(v) for k, v in mw.items()}, strict=False)
        assert not unexpected, unexpected
        keys["LSTURNewsEncoder"] = {k: list(v.shape) for k, v in ne.state_dict().items()}
        with torch.no_grad():
            out["news_out_eval"] = ne.eval()(news).numpy()
        y = ne.train()(news)
        (y * R).sum().backward()
        out["news_out"] = y.detach().numpy()
        frozen = []
        for k, p in ne.named_parameters():
            if k.startswith("text_encoder.plm_model."):              # the layout of make_golden.gen_train
                short = k[len("text_encoder.plm_model."):]
                if short.startswith("pooler."):
                    continue
                if p.grad is None:
                    frozen.append(short)
                    continue
                g = p.grad.numpy()
                if short == "embeddings.word_embeddings.weight":
                    rows = np.unique(ids[amask > 0])
                    rest = np.ones(g.shape[0], bool)
                    rest[rows] = False
                    out["news_word_rows"], out["news_word_rest_abs_sum"] = rows, np.float64(np.abs(g[rest]).sum())
                    g = g[rows]
                elif g.ndim == 2 and not short.startswith("embeddings."):
                    g = g[:ENC_ROWS]
                out["news_grad:" + short] = np.ascontiguousarray(g)
            else:
                g = p.grad.numpy().copy()
                if k.startswith("text_encoder."):                    # seeded (make_mha_pool_weights): not stored; wide gradients by their first rows
                    g = g[:ENC_ROWS] if g.ndim == 2 and g.shape[0] > 32 else g
                else:
                    out["news_sd:" + k] = p.detach().numpy().copy()
                out["news_pgrad:" + k] = np.ascontiguousarray(g)
    meta = {"source": "reference LSTURUserEncoder (user_encoder.py:45-89), LSTURCategoryEncoder / LSTURNewsEncoder (news_encoder.py:239-294) "
                      "over HF transformers " + __import__("transformers").__version__ + ", torch " + torch.__version__
                      + "; gradients of loss = sum(out * up), masking probability 0",
            "seed": SEED, "shape": {"B": B, "S": S, "I": I, "num_users": N_USERS},
            "news": {"preset": "tiny-bert", "seed": SEED, "std": 0.05, "frozen_layers": [0], "frozen": frozen, "matrix_rows": ENC_ROWS,
                     "text_heads": TEXT_HEADS, "query_dim": QUERY_DIM, "num_categories": N_CATEG, "category_dim": CATEG_DIM}}
    path = os.path.join(HERE, "lstur.npz")
    np.savez_compressed(path, **out, meta=json.dumps(meta))
    with open(os.path.join(HERE, "lstur_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays;", len(frozen), "frozen tensors")


if __name__ == "__main__":
    main()
