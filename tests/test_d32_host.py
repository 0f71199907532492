"""Head dimension 32 (the MiniLM family) on the host: the oracle against the reference's goldens at head_dim 32, the presets and the
precision rule, and the proof that the GPU tests' inputs can see the two mistakes a head_dim-32 attention kernel is most likely to
contain (tests/d32_common.py) — each moves the oracle past 10 x the fp32 bar on EVERY row of the fixtures."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import manner_oracle as O
from manner_amd.config import PRESETS, EncoderConfig, from_hf_dict, resolve
from manner_amd.weights import tensor_sha256

import d32_common as D


@pytest.mark.parametrize("name", D.GOLDEN_ENC + D.GOLDEN_ENC_16BIT)
def test_oracle_matches_reference_at_head_dim_32(golden_dir, name):
    z, meta = D.load(golden_dir, name)
    cfg, w = D.fixture_weights(meta)
    assert cfg.head_dim == 32 and meta["std"] == (0.1 if name in D.GOLDEN_ENC_16BIT else 0.05) and "std_note" in meta
    assert z["mask"].sum(1).tolist() == D.D32_LENGTHS
    for k, h in meta["sha256"].items():             # the seeded weights regenerate bit-identically
        assert tensor_sha256(w[k]) == h, k
    out = O.encode_cls(z["ids"], z["mask"], w, cfg).numpy()
    err = np.abs(out - z["out"]).max()
    print(f"{name}: oracle vs reference {err:.3e}")
    assert out.shape == z["out"].shape and err < D.ORACLE_TOL


def test_oracle_hidden_states_match_reference_at_head_dim_32(golden_dir):
    z, meta = D.load(golden_dir, "hidden_mini_minilm")
    cfg, w = D.fixture_weights(meta)
    assert cfg.head_dim == 32 and meta["layers"] == [1, 2] and z["mask"].sum(1).tolist() == [129, 256, 300, 512]
    keep = torch.from_numpy(z["mask"]).bool()
    for k in meta["layers"]:
        h = O.encode_tokens(z["ids"], z["mask"], w, cfg, layers=k)[keep].numpy()[z["rows"]]
        err = np.abs(h - z[f"h{k}"]).max()
        print(f"hidden_states[{k}]: oracle vs reference {err:.3e}")
        assert err < D.ORACLE_TOL, k


def test_presets():
    assert PRESETS["minilm-l12-h384"] == EncoderConfig(hidden=384, heads=12, layers=12, intermediate=1536, vocab=30522, max_pos=512)
    assert PRESETS["tiny-bert-d32"] == EncoderConfig(hidden=128, heads=4, layers=2, intermediate=512, vocab=2048, max_pos=512)
    assert PRESETS["mini-minilm"] == EncoderConfig(hidden=384, heads=12, layers=2, intermediate=1536, vocab=2048, max_pos=512)
    for name in ("minilm-l12-h384", "tiny-bert-d32", "mini-minilm"):
        cfg = resolve(name)
        assert cfg.head_dim == 32 and cfg.hidden % 128 == 0 and cfg.heads % 4 == 0
    # the twin of the tiny shape differs in the head count alone
    assert PRESETS[D.TWIN_PRESET] == EncoderConfig(**{**PRESETS["tiny-bert-d32"].to_dict(), "heads": 2})


# config.json of microsoft/MiniLM-L12-H384-uncased as shipped (its model card's files), written out: nothing is downloaded
MINILM_CONFIG_JSON = {
    "attention_probs_dropout_prob": 0.1,
    "hidden_act": "gelu",
    "hidden_dropout_prob": 0.1,
    "hidden_size": 384,
    "initializer_range": 0.02,
    "intermediate_size": 1536,
    "layer_norm_eps": 1e-12,
    "max_position_embeddings": 512,
    "model_type": "bert",
    "num_attention_heads": 12,
    "num_hidden_layers": 12,
    "type_vocab_size": 2,
    "vocab_size": 30522,
}


def test_the_shipped_minilm_config_resolves_to_the_preset():
    assert from_hf_dict(MINILM_CONFIG_JSON) == PRESETS["minilm-l12-h384"]
    # Multilingual-MiniLM-L12-H384: the same shape over its own vocabulary
    multi = from_hf_dict({**MINILM_CONFIG_JSON, "vocab_size": 250037, "tokenizer_class": "XLMRobertaTokenizer"})
    assert multi.head_dim == 32 and (multi.hidden, multi.heads, multi.layers, multi.intermediate) == (384, 12, 12, 1536)


@pytest.mark.parametrize("cfg,want", [
    (PRESETS["minilm-l12-h384"], "fp32"), (PRESETS["tiny-bert-d32"], "fp32"),
    # head_dim 32 at a width the split modes tile (H, I multiples of 256): still "fp32"
    (EncoderConfig(hidden=256, heads=8, layers=2, intermediate=1024, vocab=2048, max_pos=512), "fp32"),
    (EncoderConfig(hidden=512, heads=16, layers=2, intermediate=2048, vocab=2048, max_pos=512), "fp32"),
    # head_dim 64 keeps its rule
    (EncoderConfig(hidden=256, heads=4, layers=2, intermediate=1024, vocab=2048, max_pos=512), "f16x3"),
    (PRESETS["bert-base-uncased"], "f16x3"), (PRESETS["tiny-bert"], "fp32")])
def test_precision_rule_outside_autocast(cfg, want):
    from manner_amd.models.components.news_encoder import MannerTextEncoder
    stub = SimpleNamespace(precision=None, plm_model=SimpleNamespace(cfg=cfg))
    assert MannerTextEncoder.resolved_precision(stub) == want


@pytest.mark.parametrize("defect", sorted(D.DEFECTS))
@pytest.mark.parametrize("name", D.GOLDEN_ENC + D.GOLDEN_ENC_16BIT)
def test_planted_defects_are_visible_on_every_row(golden_dir, name, defect):
    """The inputs of the GPU tests, through the unchanged oracle with the defect planted in the weights: every row moves by more than
    10 x the fp32 bar, so a kernel that contained the mistake could not pass them."""
    z, meta = D.load(golden_dir, name)
    cfg, w = D.fixture_weights(meta)
    out = O.encode_cls(z["ids"], z["mask"], D.DEFECTS[defect](cfg, w), cfg).numpy()
    moved = np.abs(out - z["out"]).max(1)
    print(f"{name} {defect}: min over rows {moved.min():.3e}, max {moved.max():.3e}")
    assert moved.min() > 10 * D.FP32_TOL


def test_the_scale_defect_hides_at_hf_std(golden_dir):
    """Why the fixtures use std 0.05: at HF's 0.02 the head_dim-64 constant left in place moves some row of the tiny shape by less
    than 10 x the fp32 bar."""
    z, meta = D.load(golden_dir, "enc_tiny_bert_d32")
    cfg, w = D.fixture_weights(meta, std=0.02)
    ref = O.encode_cls(z["ids"], z["mask"], w, cfg).numpy()
    moved = np.abs(O.encode_cls(z["ids"], z["mask"], D.defect_scale(cfg, w), cfg).numpy() - ref).max(1)
    print(f"std 0.02: min over rows {moved.min():.3e}, max {moved.max():.3e}")
    assert moved.min() < 10 * D.FP32_TOL


def test_crossed_defect_is_a_permutation_of_whole_heads():
    cfg = PRESETS["tiny-bert-d32"]
    w = {f"encoder.layer.{l}.attention.self.value.{k}": (np.arange(128 * 128, dtype=np.float32).reshape(128, 128) if k == "weight"
                                                         else np.arange(128, dtype=np.float32)) for l in range(2) for k in ("weight", "bias")}
    x = D.defect_crossed(cfg, w)["encoder.layer.1.attention.self.value.bias"]
    assert x[:32].tolist() == list(range(32, 64)) and x[32:64].tolist() == list(range(32)) and x[64:96].tolist() == list(range(96, 128))
