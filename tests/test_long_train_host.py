"""Long-row training (news of 129..512 tokens) on the CPU side: the oracle against the gradients of the reference's own
MannerTextEncoder.train() on long rows (tests/golden/make_golden_train_long.py), so that the GPU tests may also judge long rows
against the oracle on random inputs with replayed dropout masks; the header's training limit as the binding mirrors it; and the
argument checks of encode_train's opt-in."""
import os
import re

import numpy as np
import pytest
import torch

import manner_oracle as O
from manner_amd import _lib, train
from manner_amd.config import PRESETS
from test_oracle_golden import compare_train_grads, golden_train_case

GOLDEN_TRAIN_LONG = ["train_long_tiny_bert", "train_long_tiny_roberta"]
KEY_BIAS_ABS = 1e-5


def split_key_bias(expect):
    """The key-bias gradient is analytically zero (softmax is shift-invariant): what remains is rounding noise that grows with the
    row length (5e-7 at 512 tokens, above the relative bar's 1e-3 floor).  It is judged on its own, against an absolute bar."""
    kb = {k: v for k, v in expect.items() if k.endswith("attention.self.key.bias")}
    return {k: v for k, v in expect.items() if k not in kb}, kb


@pytest.mark.parametrize("name", GOLDEN_TRAIN_LONG)
def test_oracle_reproduces_the_long_training_goldens(golden_dir, name):
    cfg, w, z, meta, expect = golden_train_case(golden_dir, name)
    frozen = set(meta["frozen"])
    wt = {k: torch.from_numpy(v).requires_grad_(k not in frozen) for k, v in w.items()}
    out = O.encode_cls_train(z["ids"], z["mask"], wt, cfg)
    assert np.abs(out.detach().numpy() - z["out"]).max() < 2e-5          # the bars of tests/test_oracle_golden.py
    (out * torch.from_numpy(z["R"])).sum().backward()
    rest, kb = split_key_bias(expect)
    grads = {k: (None if v.grad is None else v.grad.numpy()) for k, v in wt.items()}
    compare_train_grads(grads, z, meta, rest, rel=2e-4)
    for k, ref in kb.items():
        assert np.abs(ref).max() < KEY_BIAS_ABS and np.abs(grads[k]).max() < KEY_BIAS_ABS, k


@pytest.mark.parametrize("name", GOLDEN_TRAIN_LONG)
def test_long_training_goldens_cover_the_tile_and_stream_edges(golden_dir, name):
    """129 (first long row), 256 / 257 (the short rows' 256-key dropout stride), 512 (the limit) — and a short row beside them."""
    _, _, z, meta, _ = golden_train_case(golden_dir, name)
    lens = set(z["mask"].sum(1).tolist())
    assert {2, 128, 129, 256, 257, 512} <= lens and z["ids"].shape[1] == 512
    cfg = PRESETS[meta["preset"]]
    pos0 = cfg.pad_id + 1 if cfg.arch == 1 else 0
    assert pos0 + 512 <= cfg.max_pos                                     # the longest row fits the position table


def test_long_training_golden_freezes_a_layer_below_trainable_embeddings(golden_dir):
    _, _, z, meta, expect = golden_train_case(golden_dir, "train_long_tiny_bert")
    assert any("layer.0." in k for k in meta["frozen"]) and "embeddings.position_embeddings.weight" in expect


def test_header_declares_the_training_limit():
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    defs = dict(re.findall(r"#define\s+(MANNER_HIP_MAX_LEN\w*)\s+(\d+)", text))
    assert int(defs["MANNER_HIP_MAX_LEN_TRAIN"]) == _lib.MAX_LEN_TRAIN == 512
    assert int(defs["MANNER_HIP_MAX_LEN"]) == _lib.MAX_LEN == 128
    assert int(re.search(r"#define\s+MANNER_HIP_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 8


@pytest.mark.parametrize("max_len", [0, 513])
def test_encode_train_rejects_a_limit_beyond_the_kernels(max_len):
    ids = torch.zeros((1, 8), dtype=torch.int64)
    with pytest.raises(ValueError, match="max_len"):
        train.encode_train(PRESETS["tiny-bert"], {}, ids, torch.ones_like(ids), precision="fp32", max_len=max_len)


def test_module_default_keeps_the_short_limit():
    from manner_amd.models.components.news_encoder import MannerTextEncoder
    want = int(os.environ.get("MANNER_HIP_TRAIN_MAX_LEN", "128"))
    assert MannerTextEncoder.train_max_length == want
