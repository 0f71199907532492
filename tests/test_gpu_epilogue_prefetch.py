"""The epilogue constants of gemm_tn_w8_kernel staged in the wave's LDS slab under the K-loop (MANNER_HIP_EPI_PREFETCH, gemm.hip's
w8_prefetch_consts): the same values reach the same registers, so the outputs are the bits of the epilogue that fetches them itself
(MANNER_HIP_EPI_PREFETCH=0) and of the compiler-scheduled kernel (MANNER_HIP_GEMM_ASM=0), which never prefetches.  Held to
torch.equal on a two-layer bert-base-width encoder (H = 768, I = 3072), f16 and bf16, every launch forced onto a persistent kernel
(MANNER_HIP_GEMM_SMALL_TILES=0) with 256-row panels (MANNER_HIP_GEMM_PANEL=256: the panels the hand-scheduled kernel runs), at the
smallest token counts at which the prefetch can go wrong:

  ragged      22 450 tokens in one chunk: more tiles than workgroups in every launch, N = 768 included — every workgroup reuses its
              slab from tile to tile — and a partial last row panel (the clamp of the {mean, rstd} rows);
  panels29    7 313 tokens, 29 row panels: Q|K|V and FFN1 have two or more tiles per workgroup, the out-projection and FFN2 at most
              one, so some workgroups of those launches run no tile;
  whole       4 096 tokens, 16 whole panels: no clamp;
  no_fanin    `ragged` with MANNER_HIP_DLN_FANIN=0: the residual epilogue without the arrival behind it (the other cases have it);
  own_panels  `ragged` with the panel height left to the library (192-row launches keep the LDS-DMA kernel);
  two_chunks  `ragged` as one call of two chunks, which the engine runs on its two streams.

Run on the MI355X box: ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from manner_amd import hip  # noqa: E402
from manner_amd.synth import synth_news_tokens  # noqa: E402
from test_gpu_attention_slices import DEV, _case, _cuda, _engine  # noqa: E402

SWITCHES = ("MANNER_HIP_GEMM_SMALL_TILES", "MANNER_HIP_GEMM_ASM", "MANNER_HIP_GEMM_PANEL", "MANNER_HIP_DLN_FANIN", "MANNER_HIP_DEFER_LN",
            "MANNER_HIP_EPI_PREFETCH", "MANNER_HIP_XCD_RANGES", "MANNER_HIP_COL_GROUP", "MANNER_HIP_STREAMS")
PAD = 96
LENS = [2, 31, 33, 63, 64, 65, 95, 96]                    # 449 tokens per 8 news
# name: (lengths, switches on top of the forcing, max_chunk_tokens)
CASES = {
    "ragged": (np.resize(LENS, 400), {"GEMM_PANEL": "256"}, 65536),
    "panels29": (np.resize(LENS, 132), {"GEMM_PANEL": "256"}, 65536),
    "whole": (np.resize([32, 96], 64), {"GEMM_PANEL": "256"}, 65536),
    "no_fanin": (np.resize(LENS, 400), {"GEMM_PANEL": "256", "DLN_FANIN": "0"}, 65536),
    "own_panels": (np.resize(LENS, 400), {}, 65536),
    "two_chunks": (np.resize(LENS, 400), {"GEMM_PANEL": "256"}, 12000),
}
SETTINGS = {"on": {"EPI_PREFETCH": "1"}, "off": {"EPI_PREFETCH": "0"}, "default": {}, "compiler_scheduled": {"GEMM_ASM": "0"}}
_TOKENS = {}


def _tokens(name):
    lens = CASES[name][0]
    key = lens.tobytes()
    if key not in _TOKENS:
        cfg, _, _, _ = _case("bert-base", "hf", 512)
        ids, mask = synth_news_tokens(len(lens), cfg, seed=len(lens), lengths=lens, pad_to=PAD)
        _TOKENS[key] = _cuda(ids), _cuda(mask), mask.sum(1), torch.from_numpy(mask != 0).to(DEV)
    return _TOKENS[key]


def test_the_cases_are_the_shapes_they_claim():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cfg, _, _, _ = _case("bert-base", "hf", 512)
    assert cfg.hidden == 768 and cfg.intermediate == 3072 and cfg.layers == 2
    t = {name: int(c[0].sum()) for name, c in CASES.items()}
    assert t["ragged"] == 22450 and t["ragged"] % 256 and -(-t["ragged"] // 256) * (cfg.hidden // 256) > cus
    p29 = -(-t["panels29"] // 256)
    assert p29 == 29 and t["panels29"] % 256 and p29 * (cfg.hidden // 256) < cus < p29 * (3 * cfg.hidden // 256)
    assert t["whole"] % 256 == 0 and t["whole"] > 0
    assert t["two_chunks"] > CASES["two_chunks"][2] and t["two_chunks"] <= 2 * CASES["two_chunks"][2]


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_prefetched_constants_give_the_same_bits(name, mode, monkeypatch):
    """encode_cls under the four settings and, prefetch on against off, the hidden states behind both layers (every NORM / NRES
    output row of real tokens), bit for bit."""
    _, switches, chunk = CASES[name]
    ids, mask, lens, sel = _tokens(name)
    enc = _engine("bert-base", "hf")
    cls, hidden = {}, {}
    for setting, extra in SETTINGS.items():
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in {"GEMM_SMALL_TILES": "0", **switches, **extra}.items():
            monkeypatch.setenv("MANNER_HIP_" + k, v)
        cls[setting] = enc.encode_cls(ids, mask, precision=mode, host_lengths=lens, max_chunk_tokens=chunk).clone()
        if setting in ("on", "off"):
            hidden[setting] = [enc.encode_hidden(ids, mask, layer, precision=mode, host_lengths=lens, max_chunk_tokens=chunk)[sel].clone()
                               for layer in (1, 2)]
        hip.check_status(DEV)
    assert bool(torch.isfinite(cls["on"]).all()) and float(cls["on"].abs().max()) > 0
    for setting in ("off", "default", "compiler_scheduled"):
        assert torch.equal(cls["on"], cls[setting]), (setting, float((cls["on"].float() - cls[setting].float()).abs().max()))
    for layer in (0, 1):
        a, b = hidden["on"][layer], hidden["off"][layer]
        assert torch.equal(a, b), (layer + 1, int((a != b).any(1).sum()), "rows differ")
