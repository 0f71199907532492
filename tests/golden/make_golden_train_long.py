#!/usr/bin/env python3
"""Generate the long-row TRAINING golden fixtures (news of up to 512 tokens) from the REFERENCE itself.

Run in the build container only (needs the reference and transformers), like make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_long.py

The generator is make_golden.py's gen_train: the gradients of the reference's own MannerTextEncoder.train() (HF model, "layer.N."
parameters of `frozen_layers` frozen) with every dropout probability 0, loss = sum(out * R).  This script only picks the shapes:
rows on both sides of the short-row attention tile (128 tokens), the 32-key tile edges and the 256-key edge of the short rows'
dropout index beyond it, and rows up to the 512-token training limit, on tiny architectures with a 512-position table.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import gen_train  # noqa: E402

TRAIN_LONG_LENGTHS = np.array([2, 128, 129, 160, 255, 256, 257, 384, 511, 512])

if __name__ == "__main__":
    # BERT: max_position_embeddings 512; layer 0 frozen, so the gradient reaches the embeddings through a frozen layer
    gen_train("train_long_tiny_bert", "tiny-bert-512", n=10, lp=512, seed=71, std=0.05, lengths=TRAIN_LONG_LENGTHS, frozen_layers=[0],
              matrix_rows=8)
    # RoBERTa: max_position_embeddings 514, positions start at pad_id + 1 = 2, so a 512-token row uses position 513
    gen_train("train_long_tiny_roberta", "tiny-roberta-514", n=10, lp=512, seed=72, std=0.05, lengths=TRAIN_LONG_LENGTHS[::-1].copy(),
              frozen_layers=[], matrix_rows=8)
