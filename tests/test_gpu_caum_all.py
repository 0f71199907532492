"""``manner_hip_caum_scores_all`` (csrc/caum.hip) — every candidate column of CAUMPLMModule.forward in one call on shared history
products — with ``CAUMUserEncoder.forward_all`` and ``hotpath.caum_forward`` above it, against the float64 loop over the columns
(``caum_ref.caum_module_forward``) under the MEASURED bar of tests/side_ops_ref.py (8 x the float32 CPU error of that loop, relative
to the largest score).  tests/caum_all_ref.py lists the shapes and says which row tile each is there for; tests/test_caum_all_host.py
holds the shared-product form and its planted defects on the CPU.  Every test prints its errors next to the bars and records them with
``measured`` (profiles/caum/measured_tolerances.json is that record from an MI355X)."""
import json
import os

import numpy as np
import pytest
import torch

import caum_all_ref as CA
import caum_ref as CR
import side_ops_ref as R
from manner_amd import hip, hotpath
from manner_amd.models.components.user_encoder import CAUMUserEncoder
from test_gpu_side_ops import _hold_measured

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(shape):
    return "B{}-S{}-D{}-F{}-H{}-{}-h{}-C{}".format(*shape)


def _operands(case):
    lv = {k: v.to(DEV) for k, v in case.leaves.items()}
    return lv["hist"], lv["cand"], [lv[n] for n in CR.PARAMS], case.consts["heads"]


def _bytes(shape, cols):
    b, s, d, f, h1, h2, heads, c = shape
    return int(hip._lib.load().manner_hip_caum_scores_all_workspace_bytes(b, s, c, d, f, d, h1, h2, heads, cols))


@pytest.mark.parametrize("shape", CA.SHAPES, ids=_ids)
def test_scores_all_against_the_float64_loop(shape, measured):
    case = CA.all_case(*shape)
    hist, cand, params, heads = _operands(case)
    got = hip.caum_scores_all(hist, cand, params, heads)
    _hold_measured(case, {"scores": got.cpu()}, measured)
    assert torch.equal(hip.caum_scores_all(hist, cand, params, heads), got)                    # fixed-order reductions: the same bits
    if shape[0] > 1:
        assert float(got[1, -1]) == 0.0                                                        # the zero-padded candidate row


def test_the_pass_width_does_not_change_a_bit():
    """C = 5 in a workspace that holds two columns (three passes, the last one partial) and in the least one (five passes) against
    the one-pass call"""
    shape = CA.SHAPES[0]
    hist, cand, params, heads = _operands(CA.all_case(*shape))
    whole = hip.caum_scores_all(hist, cand, params, heads)
    assert _bytes(shape, 1) < _bytes(shape, 2) < _bytes(shape, 3) <= _bytes(shape, 5) == _bytes(shape, 9)
    assert torch.equal(hip.caum_scores_all(hist, cand, params, heads, max_workspace_bytes=_bytes(shape, 2)), whole)
    assert torch.equal(hip.caum_scores_all(hist, cand, params, heads, max_workspace_bytes=0), whole)
    lib, out = hip._lib.load(), torch.empty_like(whole)
    tab = (hip.C.c_void_p * 16)(*[t.data_ptr() for t in params])
    small = torch.empty(_bytes(shape, 1) - 1, dtype=torch.uint8, device=DEV)
    b, s, d, f, h1, h2, _, c = shape
    with pytest.raises(RuntimeError, match="caum_scores_all: workspace too small"):
        hip._lib.check(lib.manner_hip_caum_scores_all(hip._ptr(hist), hip._ptr(cand), tab, b, s, c, d, f, d, h1, h2, heads, hip._ptr(out),
                                                      hip._ptr(small), small.numel(), hip._stream()))


def _shaped(b, s, d, f, h1, h2, c=2):
    x, cand = R.randn(1, b, s, d).to(DEV), R.randn(2, b, c, d).to(DEV)
    return x, cand, [R.randn(3 + i, *shp, scale=0.1).to(DEV) for i, shp in enumerate(CR.param_shapes(d, f, d, h1, h2).values())]


@pytest.mark.parametrize("shape,heads,limit", [((1, 257, 8, 8, 8, 8), 2, r"S=257 unsupported \(S <= 256\)"),
                                               ((1, 3, 1028, 8, 8, 8), 4, r"D=1028 unsupported \(D <= 1024\)"),
                                               ((1, 3, 8, 1028, 8, 8), 2, r"F=1028 unsupported \(F <= 1024\)"),
                                               ((1, 3, 8, 8, 1028, 8), 2, r"H1=1028 unsupported \(H1 <= 1024\)"),
                                               ((1, 3, 8, 8, 8, 1028), 2, r"H2=1028 unsupported \(H2 <= 1024\)"),
                                               ((1, 3, 130, 8, 8, 8), 2, r"head_dim 65 unsupported \(head_dim <= 64\)")],
                         ids=["S257", "D1028", "F1028", "H1-1028", "H2-1028", "dh65"])
def test_scores_all_refuses_shapes_past_the_bounds(shape, heads, limit):
    x, cand, params = _shaped(*shape)
    with pytest.raises(RuntimeError, match="caum_scores_all: " + limit):
        hip.caum_scores_all(x, cand, params, heads)


def test_scores_all_without_columns_or_users_and_a_negative_count():
    x, cand, params = _shaped(3, 4, 8, 8, 8, 8, c=0)
    out = hip.caum_scores_all(x, cand, params, 2)
    assert tuple(out.shape) == (3, 0) and out.dtype == torch.float32
    x0, cand0, _ = _shaped(0, 4, 8, 8, 8, 8, c=3)
    assert tuple(hip.caum_scores_all(x0, cand0, params, 2).shape) == (0, 3)
    tab = (hip.C.c_void_p * 16)(*[t.data_ptr() for t in params])
    buf = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r"caum_scores_all: bad shape C=-1"):
        hip._lib.check(hip._lib.load().manner_hip_caum_scores_all(hip._ptr(x), hip._ptr(buf), tab, 3, 4, -1, 8, 8, 8, 8, 8, 2, hip._ptr(buf), hip._ptr(buf),
                                                                  buf.numel(), hip._stream()))
    with pytest.raises(RuntimeError, match=r"news_vector_dim 24 != user_vector_dim 8"):
        hip.caum_scores_all(R.randn(1, 3, 4, 24).to(DEV), R.randn(2, 3, 2, 24).to(DEV), params, 2)
    x1, cand1, _ = _shaped(3, 4, 8, 8, 8, 8)                                                    # the library is still usable
    assert torch.isfinite(hip.caum_scores_all(x1, cand1, params, 2)).all()


# ------------------------------------------------------------------------------------------------ the mirror
def _mirror(case, p):
    (f, d4), h1, h2 = case.leaves["w1"].shape, case.leaves["wa"].shape[0], case.leaves["wb"].shape[0]
    d, heads = d4 // 4, case.consts["heads"]
    enc = CAUMUserEncoder(news_vector_dim=d, num_filters=f, dense_att_hidden_dim1=h1, dense_att_hidden_dim2=h2, user_vector_dim=d,
                          num_attention_heads=heads, dropout_probability=p)
    enc.load_state_dict({CR.STATE_KEYS[n]: case.leaves[n] for n in CR.PARAMS}, strict=True)
    return enc.to(DEV)


def test_forward_all_at_one_column_meets_the_golden_of_the_reference_class(golden_dir, measured):
    """C = 1 with the golden's state dict: the reference's own CAUMUserEncoder.forward on (user_x, user_c), within the 1e-4 of the
    largest entry that test_gpu_caum.py::test_user_encoder_mirror_matches_the_reference holds the per-column forward to"""
    z = np.load(os.path.join(golden_dir, "caum.npz"))
    _, _, d, f, h1, h2, heads = CR.GOLDEN_SHAPE
    enc = CAUMUserEncoder(news_vector_dim=d, num_filters=f, dense_att_hidden_dim1=h1, dense_att_hidden_dim2=h2, user_vector_dim=d,
                          num_attention_heads=heads, dropout_probability=0.0)
    enc.load_state_dict({k[len("user_sd:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("user_sd:")}, strict=True)
    enc = enc.to(DEV).eval()
    x, c = (torch.from_numpy(z[k]).to(DEV) for k in ("user_x", "user_c"))
    with torch.no_grad():
        got = enc.forward_all(x, c[:, None, :])[:, 0].cpu().numpy()
    want = z["user_out"]
    err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-3)
    print(f"forward_all at C = 1 against the golden: {err:.3e} (bar 1e-4)")
    measured(out_rel=err, bar=1e-4)
    assert got.shape == want.shape and err <= 1e-4


def test_forward_all_in_eval_is_the_library_entry_bit_for_bit():
    case = CA.all_case(*CA.SHAPES[0])
    hist, cand, params, heads = _operands(case)
    enc = _mirror(case, 0.2).eval()
    with torch.no_grad():
        assert torch.equal(enc.forward_all(hist, cand), hip.caum_scores_all(hist, cand, params, heads))
    with torch.inference_mode():
        assert torch.equal(enc.forward_all(hist, cand), hip.caum_scores_all(hist, cand, params, heads))
    for t in enc.parameters():
        t.requires_grad_(False)
    assert torch.equal(enc.forward_all(hist, cand), hip.caum_scores_all(hist, cand, params, heads))      # grad mode on, nothing to differentiate


def _loop_by_hand(enc, hist, cand):
    """CAUMPLMModule.forward's own lines (baselines/caum_plm_module.py:156-163)"""
    scores = torch.zeros(cand.shape[0], cand.shape[1], device=DEV)
    scores = scores.transpose(1, 0)
    for i in range(cand.shape[1]):
        cand_score = enc(hist, cand[:, i, :])
        scores[i, :] = cand_score
    return scores.transpose(1, 0)


def _with_gradients(enc, run, case, seed):
    hist, cand = (case.leaves[n].to(DEV).requires_grad_(True) for n in ("hist", "cand"))
    enc.zero_grad()
    torch.manual_seed(seed)
    scores = run(enc, hist, cand)
    (scores * R.randn(77, *scores.shape).to(DEV)).sum().backward()
    drawn = int(torch.randint(0, 2 ** 62, (1,)).item())                                        # where the CPU generator stands afterwards
    got = {"scores": scores.detach().clone(), "d_hist": hist.grad.clone(), "d_cand": cand.grad.clone(), "next_draw": torch.tensor(drawn)}
    got.update({"d_" + n: p.grad.detach().clone() for n, p in zip(CR.PARAMS, enc._params())})
    return got


@pytest.mark.parametrize("mode,p", [("train", 0.2), ("eval", 0.0)], ids=["train-p0.2", "requires-grad-p0"])
def test_forward_all_with_a_graph_or_dropout_is_the_loop_by_hand(mode, p):
    """train() at p = 0.2 under torch.manual_seed, and eval() with inputs and parameters that require grad: scores, every gradient and
    the seed draws are those of the loop over ``forward`` written by hand"""
    case = CA.all_case(*CA.SHAPES[0])
    enc = _mirror(case, p)
    enc = enc.train() if mode == "train" else enc.eval()
    hand = _with_gradients(enc, _loop_by_hand, case, 4321)
    got = _with_gradients(enc, lambda e, h, c: e.forward_all(h, c), case, 4321)
    assert set(got) == set(hand) and all(torch.equal(got[k], hand[k]) for k in hand), [k for k in hand if not torch.equal(got[k], hand[k])]
    assert float(hand["d_hist"].abs().max()) > 0 and float(hand["d_w1"].abs().max()) > 0
    if p > 0:
        with torch.no_grad():
            plain = hip.caum_scores_all(*_operands(case))
        assert R.rel_to_max(got["scores"].cpu(), plain.cpu()) > 1e-3                           # the dropouts were on


# ------------------------------------------------------------------------------------------------ hotpath.caum_forward
def test_caum_forward_on_a_ragged_batch(measured):
    """three impressions with 3 / 1 / 2 clicked news and 2 / 4 / 1 candidates, ``hist_max`` / ``cand_max`` carried by the batch, a stub
    news encoder that returns the rows it is given: scores [3, 4] against the float64 restatement on the zero-padded dense tensors,
    the padded slots (exact zeros) included"""
    _, _, d, f, h1, h2, heads, _ = CA.SHAPES[0]
    n_hist, n_cand = (3, 1, 2), (2, 4, 1)

    def build(salt):
        leaves, consts, _ = CR.caum_inputs(3, 3, d, f, h1, h2, heads, salt + 29)
        hist, cand = torch.zeros(3, 3, d), torch.zeros(3, 4, d)
        for i, (nh, nc) in enumerate(zip(n_hist, n_cand)):
            hist[i, :nh], cand[i, :nc] = R.randn(3400 + i + salt, nh, d), R.randn(3410 + i + salt, nc, d)
        leaves = dict({k: v for k, v in leaves.items() if k not in ("x", "c")}, hist=hist, cand=cand)
        return R.Case("caum-forward-ragged", CR.caum_module_forward, leaves, consts, None)
    case = R.settled(build)
    hist, cand = case.leaves["hist"], case.leaves["cand"]
    batch = {"x_hist": torch.cat([hist[i, :n] for i, n in enumerate(n_hist)]).to(DEV), "x_cand": torch.cat([cand[i, :n] for i, n in enumerate(n_cand)]).to(DEV),
             "batch_hist": torch.repeat_interleave(torch.arange(3), torch.tensor(n_hist)).to(DEV),
             "batch_cand": torch.repeat_interleave(torch.arange(3), torch.tensor(n_cand)).to(DEV),
             "users": torch.arange(3, device=DEV), "hist_max": 3, "cand_max": 4}
    enc = CAUMUserEncoder(news_vector_dim=d, num_filters=f, dense_att_hidden_dim1=h1, dense_att_hidden_dim2=h2, user_vector_dim=d,
                          num_attention_heads=heads, dropout_probability=0.2)
    enc.load_state_dict({CR.STATE_KEYS[n]: case.leaves[n] for n in CR.PARAMS}, strict=True)
    enc = enc.to(DEV).eval()
    with torch.no_grad():
        got = hotpath.caum_forward(lambda rows: rows, enc, batch)
        ragged = hotpath.caum_forward(lambda rows: rows, enc, batch, dense=False)
    assert tuple(got.shape) == (3, 4)
    want = R.evaluate(CA.caum_scores_all, case.leaves, case.consts, None, torch.float64)["scores"]
    assert R.rel_to_max(want, case.ref()["scores"]) <= 1e-12
    err, bar = R.rel_to_max(got.cpu(), want), case.bars()["scores"]
    print(f"{case}: error {err:.3e}  cpu f32 {bar['cpu_f32']:.3e}  bar {bar['bar']:.3e}")
    measured(scores_err=err, scores_cpu_f32=bar["cpu_f32"], scores_bar=bar["bar"])
    assert err <= bar["bar"]
    real = torch.tensor([[j < n for j in range(4)] for n in n_cand])
    assert float(want[~real].abs().max()) == 0.0 and float(got.cpu()[~real].abs().max()) == 0.0
    assert torch.equal(ragged.cpu(), got.cpu()[real])
