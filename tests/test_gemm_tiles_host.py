"""The GEMM-aligned labellings of tests/slice_ref.py (packed_tile_labels, weight_tile_labels, vector_block_labels) and what the per-tile
error map sees through them, on the CPU: quiet on pure 16-bit operand rounding, and a defect confined to one 256 x 256 tile of a
persistent GEMM or of the weight-gradient kernel — one that the whole-tensor cosine bar of the 16-bit tests lets through — sends the
outlier ratio over FLAG and is named by ``worst``.  The GPU side is test_gpu_gemm_tiles.py, whose ratio bars stay at or below
FLAG / 2.

Synthetic operands at the shapes of the bert-base training batch of test_gpu_attention_slices (3 070 token rows = 95 full 32-row
stages + 30 rows, twelve news): "kernel" = the operands rounded to the 16-bit type, multiplied with f32 accumulation; reference = the
unrounded operands in float64."""
import numpy as np
import pytest
import torch

import slice_ref as S

LENS = np.array([31, 33, 128, 159, 161, 192, 255, 257, 384, 447, 511, 512])      # BATCHES[512] of test_gpu_attention_slices
M, H, I = int(LENS.sum()), 768, 3072
QUIET_RATIO = 2.0            # as in test_attention_slices_host.py
# a one-tile defect sends the map's outlier ratio over FLAG (measured here: bf16 43 / 63 / 36, f16 344 / 507 / 288 for the three
# defects below); every ratio bar of test_gpu_gemm_tiles.py is at most FLAG / 2
FLAG = 12.0
COS_BAR = 0.999              # the whole-tensor bar of the 16-bit training tests: the planted defects pass it
TILE = 256


def _mask():
    return (np.arange(512)[None, :] < LENS[:, None]).astype(np.int64)


def _cos(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def _r16(t, mode):
    return t.to(S.DT16[mode]).float()


def _padded(rows, mask):
    """[M, H] packed token rows -> [N, L, H] in the layout the encoder returns (zeros on padding)."""
    out = np.zeros(mask.shape + (rows.shape[1],), dtype=np.float64)
    out[mask != 0] = rows
    return out


# ------------------------------------------------------------------------------------------------ labelling identities
def test_packed_tile_labels_cover_every_real_element_once():
    mask = _mask()
    lab = S.packed_tile_labels(mask, H)
    assert lab.shape == (len(LENS), 512, H) and lab.dtype == np.int64
    assert (lab[mask == 0] == -1).all() and (lab[mask != 0] >= 0).all()
    packed = lab[mask != 0]                                              # [M, H] in news order: the GEMMs' rows
    n_row_blocks, n_col_blocks = (M + 63) // 64, H // 64
    uniq, cnt = np.unique(packed, return_counts=True)
    assert list(uniq) == list(range(n_row_blocks * n_col_blocks))          # every tile present, none invented
    full = np.full(n_row_blocks, 64)
    full[-1] = M - 64 * (n_row_blocks - 1)
    assert (cnt.reshape(n_row_blocks, n_col_blocks) == 64 * full[:, None]).all()      # each element in exactly one tile


def test_packed_tile_labels_are_constant_on_a_block_of_packed_rows():
    mask = _mask()
    packed = S.packed_tile_labels(mask, H)[mask != 0]
    for r0 in range(0, M, 64):
        for c0 in range(0, H, 64):
            blk = packed[r0:r0 + 64, c0:c0 + 64]
            assert (blk == blk[0, 0]).all() and blk[0, 0] == (r0 // 64) * (H // 64) + c0 // 64
    other = S.packed_tile_labels(mask, H, rows=192, cols=256)             # a 192-row panel x 256-column tile
    assert other[mask != 0][191, 255] == 0 and other[mask != 0][192, 0] == 3 and other[mask != 0][191, 256] == 1


def test_packed_tile_labels_change_inside_a_news_that_straddles_a_panel_boundary():
    """Rows 192..350 are the fourth news (159 tokens): packed row 256 is its token 64, and the label changes there, not at its start."""
    mask = _mask()
    lab = S.packed_tile_labels(mask, H, rows=256, cols=256)
    start = int(LENS[:3].sum())
    assert start == 192 and start + LENS[3] > 256
    news = lab[3, :LENS[3], 0]
    assert (news[:256 - start] == 0).all() and (news[256 - start:] == H // 256).all()
    assert lab[2, LENS[2] - 1, 0] == 0 and lab[3, 0, 0] == 0                 # the news boundary itself changes nothing


def test_weight_and_vector_labels():
    lab = S.weight_tile_labels((H, I))
    assert lab.shape == (H, I) and len(np.unique(lab)) == (H // 128) * (I // 64)
    assert lab[127, 63] == 0 and lab[127, 64] == 1 and lab[128, 0] == I // 64 and lab[H - 1, I - 1] == (H // 128) * (I // 64) - 1
    _, cnt = np.unique(lab, return_counts=True)
    assert (cnt == 128 * 64).all()
    odd = S.weight_tile_labels((130, 70))                                 # partial edge tiles keep labels of their own
    assert odd[129, 69] == 3 and odd[0, 69] == 1 and odd[129, 0] == 2
    v = S.vector_block_labels(H)
    assert v.shape == (H,) and v[63] == 0 and v[64] == 1 and v[-1] == H // 64 - 1


# ------------------------------------------------------------------------------------------------ the synthetic GEMMs
@pytest.fixture(scope="module")
def wgrad_case():
    """dW [N, K] = dY^T X over the 3 070 token rows, N = K = 768."""
    g = torch.Generator().manual_seed(11)
    dy, x = torch.randn((M, H), generator=g, dtype=torch.float64), torch.randn((M, H), generator=g, dtype=torch.float64)
    S.limit_threads()
    out = {"dy": dy, "x": x, "ref": (dy.T @ x).numpy()}
    for mode in S.DT16:
        out[mode] = (_r16(dy, mode).T @ _r16(x, mode)).numpy()
    return out


@pytest.fixture(scope="module")
def linear_case():
    """Y [M, N] = X W^T + b with N = 768, K = 3 072 (the FFN2 shape), laid out [news, position, N] as the encoder returns it."""
    g = torch.Generator().manual_seed(12)
    x = torch.randn((M, I), generator=g, dtype=torch.float64)
    w = 0.02 * torch.randn((H, I), generator=g, dtype=torch.float64)
    b = 0.02 * torch.randn((H,), generator=g, dtype=torch.float64)
    S.limit_threads()
    out = {"x": x, "w": w, "ref": (x @ w.T + b).numpy()}
    for mode in S.DT16:
        out[mode] = (_r16(x, mode) @ _r16(w, mode).T + b.float()).numpy()
    return out


@pytest.fixture(scope="module")
def layernorm_case():
    """LayerNorm (no affine) of [M, 768] rows of mean 1, deviation 1, the way the deferred algebra applies it: the row stored in the
    16-bit type, its statistics taken from the f32 values as 64-column partial sums."""
    g = torch.Generator().manual_seed(13)
    x = 1.0 + torch.randn((M, H), generator=g, dtype=torch.float64)
    ref = ((x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-12)).numpy()
    return {"x": x, "ref": ref}


def _layernorm16(x, mode, lost=None):
    """``lost`` = (first row, column group): that 256-row panel's partial sum of one 64-column group never reaches the row mean."""
    xf = x.float()
    part = xf.view(M, H // 64, 64).sum(2)                                  # [M, 12] partial sums
    var = xf.var(1, unbiased=False, keepdim=True)
    if lost is not None:
        part = part.clone()
        part[lost[0]:lost[0] + TILE, lost[1]] = 0.0
    mean = part.sum(1, keepdim=True) / H
    return ((_r16(xf, mode) - mean) / torch.sqrt(var + 1e-12)).numpy()


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_tile_maps_are_quiet_on_rounding_noise(wgrad_case, linear_case, mode):
    m = S.error_map(wgrad_case[mode], wgrad_case["ref"], S.weight_tile_labels((H, H)), per_slice=True)
    print(mode, m)
    assert len(m["rms"]) == (H // 128) * (H // 64) and m["ratio"] < QUIET_RATIO, m
    mask = _mask()
    y = S.error_map(_padded(linear_case[mode], mask), _padded(linear_case["ref"], mask), S.packed_tile_labels(mask, H))
    print(mode, y)
    assert len(y["rms"]) == ((M + 63) // 64) * (H // 64) and y["ratio"] < QUIET_RATIO, y


# ------------------------------------------------------------------------------------------------ planted defects
@pytest.mark.parametrize("tile", [(0, 0), (2, 1)])
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_a_dropped_partial_row_stage_in_one_weight_gradient_tile_is_flagged(wgrad_case, mode, tile):
    """(a) The last, partial 32-row stage (rows 3 040..3 069) never accumulated into one 256 x 256 tile of dW."""
    n0, k0 = TILE * tile[0], TILE * tile[1]
    last = (M // 32) * 32
    assert 0 < M - last < 32
    dy, x = _r16(wgrad_case["dy"], mode), _r16(wgrad_case["x"], mode)
    hip = wgrad_case[mode].copy()
    hip[n0:n0 + TILE, k0:k0 + TILE] -= (dy[last:, n0:n0 + TILE].T @ x[last:, k0:k0 + TILE]).numpy()
    print(mode, "cosine", _cos(hip, wgrad_case["ref"]))
    assert _cos(hip, wgrad_case["ref"]) > COS_BAR                            # the whole-tensor bar lets it through
    m = S.error_map(hip, wgrad_case["ref"], S.weight_tile_labels((H, H)), per_slice=True)
    print(mode, m)
    assert m["ratio"] > FLAG, m
    bn, bk = divmod(m["worst"], H // 64)
    assert n0 <= 128 * bn < n0 + TILE and k0 <= 64 * bk < k0 + TILE, m


@pytest.mark.parametrize("tile", [(0, 2), (11, 0)])           # (11, 0): the last, partial row panel (rows 2 816..3 069)
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_a_dropped_last_k_step_in_one_output_tile_is_flagged(linear_case, mode, tile):
    """(b) The last K-step (64 of 3 072) never accumulated into one 256 x 256 tile of Y."""
    r0, c0 = TILE * tile[0], TILE * tile[1]
    x, w = _r16(linear_case["x"], mode), _r16(linear_case["w"], mode)
    hip = linear_case[mode].copy()
    hip[r0:r0 + TILE, c0:c0 + TILE] -= (x[r0:r0 + TILE, I - 64:] @ w[c0:c0 + TILE, I - 64:].T).numpy()
    print(mode, "cosine", _cos(hip, linear_case["ref"]))
    assert _cos(hip, linear_case["ref"]) > COS_BAR
    mask = _mask()
    m = S.error_map(_padded(hip, mask), _padded(linear_case["ref"], mask), S.packed_tile_labels(mask, H))
    print(mode, m)
    assert m["ratio"] > FLAG, m
    br, bc = divmod(m["worst"], H // 64)
    assert r0 <= 64 * br < r0 + TILE and c0 <= 64 * bc < c0 + TILE, m


@pytest.mark.parametrize("where", [(1, 0), (4, 11)])          # (row panel, 64-column group)
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_a_lost_row_mean_partial_of_one_panel_is_flagged(layernorm_case, mode, where):
    """(c) One 256-row panel's partial sums of one 64-column group left out of the LayerNorm row mean (a lost fan-in partial): every
    column of those rows is off by the same amount."""
    r0 = TILE * where[0]
    ref = layernorm_case["ref"]
    mask = _mask()
    lab = S.packed_tile_labels(mask, H)
    quiet = S.error_map(_padded(_layernorm16(layernorm_case["x"], mode), mask), _padded(ref, mask), lab)
    assert quiet["ratio"] < QUIET_RATIO, quiet
    hip = _layernorm16(layernorm_case["x"], mode, lost=(r0, where[1]))
    print(mode, "cosine", _cos(hip, ref))
    assert _cos(hip, ref) > COS_BAR
    m = S.error_map(_padded(hip, mask), _padded(ref, mask), lab)
    print(mode, m)
    assert m["ratio"] > FLAG, m
    assert r0 <= 64 * (m["worst"] // (H // 64)) < r0 + TILE, m
