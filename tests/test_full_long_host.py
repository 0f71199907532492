""""Full rows" on news of up to 512 tokens, CPU side: the header's limit as the binding mirrors it, the golden of the reference's
PLMTextEncoder on long padded batches (tests/golden/make_golden_full_long.py), the argument checks of encode_full_train's opt-in,
and the library's sources compiling for gfx950 without a warning."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from manner_amd import _lib, build, train
from manner_amd.config import PRESETS

CASES = {"p300": (300, [1, 32, 33, 128, 129, 300]), "p512": (512, [5, 257, 512])}


def test_header_declares_the_full_row_limit():
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    defs = dict(re.findall(r"#define\s+(MANNER_HIP_MAX_LEN\w*)\s+(\d+)", text))
    assert int(defs["MANNER_HIP_MAX_LEN_FULL"]) == _lib.MAX_LEN_FULL == 512
    assert int(defs["MANNER_HIP_MAX_LEN"]) == _lib.MAX_LEN == 128
    assert int(re.search(r"#define\s+MANNER_HIP_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 8


@pytest.mark.parametrize("tag", ["bert", "roberta"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_long_full_row_golden_holds_the_listed_key_counts(golden_dir, tag, case):
    z = np.load(os.path.join(golden_dir, "train_plm_long.npz"))
    meta = json.loads(str(z["meta"]))
    lp, keys = CASES[case]
    assert meta["cases"][case] == {"padded_len": lp, "real_tokens": keys}
    key = f"{tag}_{case}"
    ids, mask = z[f"{key}_ids"], z[f"{key}_mask"]
    cfg = PRESETS[meta["plm"][tag][0]]
    assert ids.shape == mask.shape == (len(keys), lp) and lp > _lib.MAX_LEN
    assert mask.sum(1).tolist() == keys
    assert ((np.arange(lp)[None, :] < mask.sum(1)[:, None]) == (mask == 1)).all()          # right-padded 0/1 prefixes
    assert (ids[mask == 0] == cfg.pad_id).all()
    pos0 = cfg.pad_id + 1 if cfg.arch == 1 else 0
    assert pos0 + lp <= cfg.max_pos                                                        # every position fits the table
    assert z[f"{key}_out"].shape == z[f"{key}_R"].shape == (len(keys), cfg.hidden)
    # the sampled last_hidden_state covers real and padded positions of every news that has both
    hs_n, hs_t = z[f"{key}_hs_news"], z[f"{key}_hs_pos"]
    assert z[f"{key}_hs"].shape == (len(hs_n), cfg.hidden) and np.isfinite(z[f"{key}_hs"]).all()
    for i, k in enumerate(keys):
        t = hs_t[hs_n == i]
        assert (t < k).any() and ((t >= k).any() or k == lp)
    # gradients: every trainable tensor, layer 0 frozen, the key bias analytically zero, the pad row of the word table zero
    grads = {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(f"{key}_grad:")}
    frozen = set(z[f"{key}_frozen"].tolist())
    assert len(grads) >= 25 and frozen and all("layer.0." in k for k in frozen)
    assert all(np.isfinite(g).all() for g in grads.values())
    assert np.abs(grads["plm_model.encoder.layer.1.attention.self.key.bias"]).max() < 1e-5
    assert np.abs(grads["plm_model.embeddings.word_embeddings.weight"][cfg.pad_id]).max() == 0.0      # rows 0..7 are stored whole


@pytest.mark.parametrize("max_len", [0, 513])
def test_encode_full_train_rejects_a_limit_beyond_the_kernels(max_len):
    ids = torch.zeros((1, 8), dtype=torch.int64)
    with pytest.raises(ValueError, match="max_len"):
        train.encode_full_train(PRESETS["tiny-bert"], {}, ids, torch.ones_like(ids), precision="fp32", max_len=max_len)


def test_plm_text_encoder_default_keeps_the_short_limit():
    from manner_amd.models.components.news_encoder import MannerTextEncoder, PLMTextEncoder
    want = int(os.environ.get("MANNER_HIP_TRAIN_MAX_LEN", "128"))
    assert PLMTextEncoder.train_max_length == MannerTextEncoder.train_max_length == want


def test_built_library_is_current_and_exports_every_header_symbol():
    """The check test_host.py applies to the build: the library loads under ABI 8 with every symbol of the header."""
    lib = _lib.load()
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES) and all(hasattr(lib, s) for s in _lib.SIGNATURES)
    assert lib.manner_hip_abi_version() == _lib.ABI_VERSION == 8


@pytest.mark.parametrize("source", ["train_attn.hip", "train.hip"])
def test_training_sources_cross_compile_for_gfx950_without_warnings(source):
    """The build's own flags (-Wall) with warnings as errors, front end only (host and gfx950 passes): the two files this path lives
    in, templates instantiated — the static_assert on the long-row LDS budget among them."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + build.FLAGS + ["-Werror", "-Wno-unused-command-line-argument", "-fsyntax-only", os.path.join(build.CSRC, source)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
