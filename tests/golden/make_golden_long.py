#!/usr/bin/env python3
"""Generate the long-row golden fixtures (news of up to 512 tokens) from the REFERENCE itself.

Run in the build container only (needs the reference and transformers), like make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_long.py

The generators are those of make_golden.py (the reference's own MannerNewsEncoder in eval() over HF BertModel /
RobertaModel, and HF hidden_states of its PLM); this script only picks the shapes: rows on both sides of the short-row
attention tile (128 tokens), the 32-key tile edges beyond it, and rows up to the 512-token inference limit.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import gen_encoder, gen_hidden  # noqa: E402


def thin_hidden(name, every=16):
    """Keep the fixture small: of the packed real-token rows gen_hidden wrote, keep every `every`-th token of each news plus its
    first two, tokens 127..129 (the short tile's edge) and its last; their packed indices go into `rows`."""
    path = os.path.join(HERE, f"{name}.npz")
    z = dict(np.load(path))
    lens = z["mask"].sum(1)
    off = np.concatenate([[0], np.cumsum(lens)])
    rows = []
    for n, ln in enumerate(lens):
        t = set(range(0, ln, every)) | {0, 1, ln - 1} | {k for k in (127, 128, 129) if k < ln}
        rows += [off[n] + k for k in sorted(t)]
    rows = np.array(rows, dtype=np.int64)
    meta = json.loads(str(z["meta"]))
    meta["rows"] = f"packed real-token rows kept: every {every}th token, tokens 0, 1, 127-129 and the last of each news"
    out = {k: v[rows] for k, v in z.items() if k.startswith("h")}
    np.savez_compressed(path, ids=z["ids"], mask=z["mask"], rows=rows, **out, meta=json.dumps(meta))
    print(name, "kept", rows.shape[0], "of", int(off[-1]), "rows")


LONG_LENGTHS = np.array([2, 33, 96, 128, 129, 130, 160, 200, 255, 256, 257, 384, 480, 500, 511, 512])

if __name__ == "__main__":
    # bert-base shape, HF-init std, 16 news padded to 512 (the position table's size)
    gen_encoder("enc_long_bert_base", "bert-base-uncased", n=16, lp=512, seed=60, std=0.02, lengths=LONG_LENGTHS)
    # roberta-base: max_position_embeddings 514, positions start at pad_id + 1 = 2, so a 512-token row uses position 513
    gen_encoder("enc_long_roberta", "roberta-base", n=16, lp=512, seed=61, std=0.02, lengths=LONG_LENGTHS[::-1].copy())
    # HF hidden_states at layers 6 and 12 of long rows (what encode_hidden is judged against)
    gen_hidden("hidden_long_bert_base", "bert-base-uncased", n=4, lp=512, seed=62, std=0.02, lengths=np.array([129, 256, 300, 512]),
               layers_out=(6, 12))
    thin_hidden("hidden_long_bert_base")
