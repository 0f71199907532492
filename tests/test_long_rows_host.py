"""Long rows (129..512 tokens) on the CPU side: the oracle against the reference's own outputs beyond the 128-token attention tile
(tests/golden/make_golden_long.py), so that the GPU tests may also judge long rows against the oracle on random inputs; and the
header's per-row limits as the Python binding mirrors them."""
import json
import os
import re

import numpy as np
import pytest

import manner_oracle as O
from manner_amd import _lib
from manner_amd.config import PRESETS
from manner_amd.weights import make_plm_weights, tensor_sha256


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return z, json.loads(str(z["meta"]))


@pytest.mark.parametrize("name", ["enc_long_bert_base", "enc_long_roberta"])
def test_oracle_reproduces_the_long_row_goldens(golden_dir, name):
    z, meta = _load(golden_dir, name)
    cfg = PRESETS[meta["preset"]]
    w = make_plm_weights(cfg, seed=meta["seed"], std=meta["std"])
    for k, h in meta.get("sha256", {}).items():
        assert tensor_sha256(w[k]) == h, k
    lens = z["mask"].sum(1)
    assert z["ids"].shape[1] == 512 and lens.max() == 512 and lens.min() == 2 and (lens > 128).sum() >= 10
    out = O.encode_cls(z["ids"], z["mask"], w, cfg).numpy()
    assert np.abs(out - z["out"]).max() < 2e-5          # the bar of tests/test_oracle_golden.py


def test_long_roberta_golden_uses_the_last_position():
    """roberta-base's table has 514 positions and its positions start at pad_id + 1: a 512-token row reads position 513."""
    cfg = PRESETS["roberta-base"]
    assert cfg.max_pos == 514 and (cfg.pad_id + 1) + 512 - 1 == cfg.max_pos - 1


def test_hidden_long_golden_covers_the_tile_edges(golden_dir):
    z, meta = _load(golden_dir, "hidden_long_bert_base")
    lens = z["mask"].sum(1)
    assert sorted(lens.tolist()) == [129, 256, 300, 512] and meta["layers"] == [6, 12]
    off = np.concatenate([[0], np.cumsum(lens)])
    rows = z["rows"]
    assert z["h6"].shape == z["h12"].shape == (rows.shape[0], 768)
    for n in range(len(lens)):                            # token 128 (first of the fifth key tile) and the last token of every news
        assert off[n] + 128 in rows and off[n + 1] - 1 in rows


def test_header_declares_the_per_row_limits():
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    defs = dict(re.findall(r"#define\s+(MANNER_HIP_MAX_LEN\w*)\s+(\d+)", text))
    assert int(defs["MANNER_HIP_MAX_LEN"]) == _lib.MAX_LEN == 128
    assert int(defs["MANNER_HIP_MAX_LEN_INFER"]) == _lib.MAX_LEN_INFER == 512
    assert int(re.search(r"#define\s+MANNER_HIP_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 8
