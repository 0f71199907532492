"""The MINER baseline's operators without a GPU: the float64 restatements of tests/miner_ref.py against the reference's own
outputs and gradients (tests/golden/miner.npz), the mirrors' state-dict keys and shapes against the reference's
(miner_state_dict_keys.json), ``install(baselines=("miner",))`` in a fresh interpreter over a reference-layout tree, and one planted
defect per loop and per quirk, each shown to exceed its bar at least 10-fold on the inputs tests/test_gpu_miner.py runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import miner_ref as M
import side_ops_ref as R
from test_host import _classes, _imports, _write_reference_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "miner.npz"))
    return z, json.loads(str(z["meta"]))


def _t(z, k):
    return torch.from_numpy(z[k])


def _against_golden(fn, leaves, consts, upstream, expect):
    """The float32 results of the reference against the float64 restatement: within 8 x the restatement's own float32 error, and
    no tighter than 8 half-ulps of the largest entry (the golden is another float32 evaluation, in torch's summation order)."""
    ref64 = R.evaluate(fn, leaves, consts, upstream, torch.float64)
    ref32 = R.evaluate(fn, leaves, consts, upstream, torch.float32)
    for k, want in expect.items():
        assert tuple(want.shape) == tuple(ref64[k].shape), k
        bar = R.MEASURED_FACTOR * max(R.rel_to_max(ref32[k], ref64[k]), R.U32)
        err = R.rel_to_max(torch.from_numpy(np.asarray(want)), ref64[k])
        assert err <= bar, (k, err, bar)


@pytest.mark.parametrize("tag", ["nobias", "bias"])
def test_poly_attention_restatement_matches_the_reference(golden, tag):
    z, meta = golden
    assert tuple(z["poly_x"].shape) == M.POLY_GOLDEN[:3] and z["poly_codes"].shape == (M.POLY_GOLDEN[4], M.POLY_GOLDEN[3])
    assert z["poly_mask"].sum(1).tolist() == meta["hist"] and len(set(meta["hist"])) > 1          # a ragged mask
    consts = {"mask": _t(z, "poly_mask"), "bias": _t(z, "poly_bias") if tag == "bias" else None}
    _against_golden(M.poly_attention, {"x": _t(z, "poly_x"), "lin_w": _t(z, "poly_lin_w"), "codes": _t(z, "poly_codes")}, consts,
                    {"out": _t(z, "poly_up")}, {"out": z[f"poly_{tag}_out"], "d_x": z[f"poly_{tag}_d_x"], "d_lin_w": z[f"poly_{tag}_d_lin_w"],
                                                "d_codes": z[f"poly_{tag}_d_codes"]})
    assert np.abs(z["poly_bias_out"] - z["poly_nobias_out"]).max() > 1e-3                         # the bias case is another case


def test_target_attention_restatement_matches_the_reference(golden):
    z, _ = golden
    leaves = {k: _t(z, "target_" + k) for k in ("query", "key", "value", "lin_w")}
    assert not z["target_key"][1, -1].any()                                                        # a zero-padded candidate row
    _against_golden(M.target_attention, leaves, {}, {"out": _t(z, "target_up")},
                    {"out": z["target_out"], **{"d_" + k: z["target_d_" + k] for k in leaves}})


def test_batched_dot_product_restatement_matches_the_reference(golden):
    z, _ = golden
    got = R.evaluate(M.bmm_rows, {"a": _t(z, "dot_cand"), "rows": _t(z, "dot_user")}, {}, {"out": _t(z, "dot_up")}, torch.float64)
    ref, absolute = (M.bmm_terms(z["dot_cand"], z["dot_user"], z["dot_up"], absolute=a) for a in (False, True))
    for k, want in (("out", z["dot_out"]), ("d_a", z["dot_d_cand"]), ("d_rows", z["dot_d_user"])):
        assert np.allclose(got[k].numpy(), ref[k][0], rtol=1e-12, atol=1e-12), k                 # autograd agrees with the written-out sums
        assert R.derived_ratio(want, ref[k][0], absolute[k][0], ref[k][1]) <= 1.0, k


def test_mirror_state_dict_keys_and_shapes_match_the_reference(golden, golden_dir):
    import warnings
    from manner_amd.models.components.attention import PolyAttention, TargetAwareAttention
    from manner_amd.models.components.news_encoder import MINERNewsEncoder
    with open(os.path.join(golden_dir, "miner_state_dict_keys.json")) as f:
        want = json.load(f)
    _, s, d, q, k = M.POLY_GOLDEN
    out_dim = golden[1]["encoder"]["news_embedding_dim"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mirrors = {"PolyAttention": PolyAttention(input_embed_dim=d, num_context_codes=k, context_code_dim=q),
                   "TargetAwareAttention": TargetAwareAttention(input_embed_dim=d),
                   "MINERNewsEncoder": MINERNewsEncoder(plm_model="tiny-bert", frozen_layers=[0], apply_reduce_dim=True, text_embedding_dim=128,
                                                        news_embedding_dim=out_dim, dropout_probability=0.2),
                   "MINERNewsEncoder_no_reduce_dim": MINERNewsEncoder(plm_model="tiny-bert", frozen_layers=[0], apply_reduce_dim=False,
                                                                      text_embedding_dim=128, news_embedding_dim=out_dim, dropout_probability=0.2)}
    for name, module in mirrors.items():
        assert {n: list(v.shape) for n, v in module.state_dict().items()} == want[name], name
    enc = mirrors["MINERNewsEncoder"]
    assert {n.split(".")[0] for n in want["MINERNewsEncoder"]} == {"plm_model", "reduce_dim"}
    assert not hasattr(mirrors["MINERNewsEncoder_no_reduce_dim"], "reduce_dim")
    frozen = {n for n, p in enc.named_parameters() if not p.requires_grad}
    assert frozen and all("layer.0." in n for n in frozen)
    codes = mirrors["PolyAttention"].context_codes                       # xavier_uniform_ at the tanh gain: |c| <= gain sqrt(6 / (K + Q))
    bound = torch.nn.init.calculate_gain("tanh") * (6.0 / (k + q)) ** 0.5
    assert 0.5 * bound < float(codes.detach().abs().max()) <= bound


_MINER_SCRIPT = r'''
import json, sys, types
import manner_amd, manner_amd.binding
ref = sys.argv[1]
sys.path.insert(0, ref)
cls = lambda c: c.__module__ + "." + c.__qualname__
import manner.models.components.news_encoder as NE, manner.models.components.attention as AT
from manner.models.components.attention import PolyAttention as UserEncoderEarly          # an alias taken BEFORE install()
fake = types.ModuleType("manner.models.fake_caller")
fake.UserEncoder = UserEncoderEarly
sys.modules["manner.models.fake_caller"] = fake
out = {}
out["plain_report"] = manner_amd.install(ref)
out["plain"] = {n: cls(getattr(m, n)) for m, n in ((NE, "MINERNewsEncoder"), (AT, "PolyAttention"), (AT, "TargetAwareAttention"))}
out["plain_alias"] = cls(fake.UserEncoder)
out["plain_installed"] = manner_amd.binding.installed()
manner_amd.uninstall()
try:
    manner_amd.install(ref, baselines=("caum",))
    out["unknown"] = "no error"
except ValueError as e:
    out["unknown"] = str(e)
out["after_unknown"] = manner_amd.binding.installed()
out["miner_report"] = manner_amd.install(ref, baselines=("miner",))
ns = {}
with open(ref + "/manner/models/baselines/miner_module.py") as f:
    for l in f:
        if l.startswith("from manner."):
            try:
                exec(l, ns)
            except ModuleNotFoundError as e:                     # a third-party package this image lacks
                assert (e.name or "").split(".")[0] != "manner", (l, e)
out["miner"] = {k: cls(v) for k, v in ns.items() if isinstance(v, type)}
out["miner_alias"] = cls(fake.UserEncoder)
out["kept"] = {n: cls(getattr(NE, n)) for n in ("NAMLNewsEncoder", "LSTURNewsEncoder", "CAUMNewsEncoder")}
out["kept"]["DenseAttention"] = cls(AT.DenseAttention)
out["again"] = manner_amd.install(ref, baselines=("miner",))      # idempotent
manner_amd.uninstall()
out["after_uninstall"] = {n: cls(getattr(m, n)) for m, n in ((NE, "MINERNewsEncoder"), (AT, "PolyAttention"), (AT, "TargetAwareAttention"))}
out["alias_after_uninstall"] = cls(fake.UserEncoder)
print("RESULT " + json.dumps(out))
'''


def test_install_rebinds_the_miner_classes_only_when_asked(tmp_path):
    """Fresh interpreter, reference-layout tree (class names only, nothing of the reference's code) with baselines/miner_module.py's
    import lines (miner_module.py:16-23).  A plain ``install()`` reports and binds what it always did and leaves the three MINER
    classes — and an alias of one taken earlier — the reference's own; ``install(baselines=("miner",))`` rebinds them, so that
    the import lines yield the mirrors under ``NewsEncoder``, ``UserEncoder``, ``TargetAwareAttention`` and ``DotProduct``;
    ``uninstall()`` restores them; an unknown baseline raises and binds nothing."""
    comp = "manner.models.components"
    reference = _write_reference_layout(str(tmp_path / "reference"))
    with open(os.path.join(reference, "manner/models/baselines/miner_module.py"), "w") as f:
        f.write(_imports(("manner.data.components.mind_batch", "MINDRecBatch", None), ("manner.metrics.diversity", "Diversity", None),
                         (f"{comp}.click_predictors", "DotProduct", None), (f"{comp}.news_encoder", "MINERNewsEncoder", "NewsEncoder"),
                         (f"{comp}.attention", "PolyAttention", "UserEncoder"), (f"{comp}.attention", "TargetAwareAttention", None))
                + _classes("MINERModule"))
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", _MINER_SCRIPT, reference], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    ref_ne, ref_at, mir = "manner.models.components.news_encoder.", "manner.models.components.attention.", "manner_amd.models.components."
    originals = {"MINERNewsEncoder": ref_ne + "MINERNewsEncoder", "PolyAttention": ref_at + "PolyAttention",
                 "TargetAwareAttention": ref_at + "TargetAwareAttention"}
    # default argument: exactly today's binding
    assert out["plain"] == originals and out["plain_alias"] == ref_at + "PolyAttention"
    assert {m: sorted(v) for m, v in out["plain_report"].items()} == {
        "manner.models.components.news_encoder": ["MannerEntityEncoder", "MannerNewsEncoder", "MannerTextEncoder", "PLMTextEncoder"],
        "manner.models.components.attention": ["AdditiveAttention"],
        "manner.models.components.user_encoder": ["NAMLUserEncoder", "NRMSUserEncoder"],
        "manner.models.components.click_predictors": ["DotProduct"]}
    assert out["plain_installed"] == {m: sorted(v) for m, v in out["plain_report"].items()}
    # an unknown name raises before anything is bound
    assert "unknown baseline 'caum'" in out["unknown"] and "miner" in out["unknown"] and out["after_unknown"] == {}
    # the opt-in
    assert sorted(out["miner_report"]["manner.models.components.news_encoder"]) == ["MINERNewsEncoder", "MannerEntityEncoder", "MannerNewsEncoder",
                                                                                      "MannerTextEncoder", "PLMTextEncoder"]
    assert sorted(out["miner_report"]["manner.models.components.attention"]) == ["AdditiveAttention", "PolyAttention", "TargetAwareAttention"]
    assert out["miner_report"]["manner.models.fake_caller"] == ["UserEncoder"]
    assert out["miner"]["NewsEncoder"] == mir + "news_encoder.MINERNewsEncoder"
    assert out["miner"]["UserEncoder"] == mir + "attention.PolyAttention" == out["miner_alias"]
    assert out["miner"]["TargetAwareAttention"] == mir + "attention.TargetAwareAttention"
    assert out["miner"]["DotProduct"] == mir + "click_predictors.DotProduct"
    assert out["miner"]["MINDRecBatch"].startswith("manner.data.components.mind_batch.")
    assert all(v.startswith("manner.models.components.") for v in out["kept"].values()), out["kept"]
    assert out["again"] == {}
    assert out["after_uninstall"] == originals and out["alias_after_uninstall"] == ref_at + "PolyAttention"


def test_run_takes_the_opt_in_as_a_flag_in_front_of_the_script(tmp_path):
    reference = _write_reference_layout(str(tmp_path / "reference"))
    script = tmp_path / "entry.py"
    script.write_text("import sys\nfrom manner.models.components.attention import PolyAttention, DenseAttention\n"
                      "print('ARGV', sys.argv[1:], PolyAttention.__module__, DenseAttention.__module__)\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + reference, PYTHONDONTWRITEBYTECODE="1")
    for flags, module in (([], "manner.models.components.attention"), (["--baselines", "miner"], "manner_amd.models.components.attention"),
                          (["--baselines=miner"], "manner_amd.models.components.attention")):
        r = subprocess.run([sys.executable, "-m", "manner_amd.run"] + flags + [str(script), "experiment=x", "--baselines", "y"], env=env,
                           capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        assert f"ARGV ['experiment=x', '--baselines', 'y'] {module} manner.models.components.attention" in r.stdout, r.stdout
    r = subprocess.run([sys.executable, "-m", "manner_amd.run", "--baselines", "lstur", str(script)], env=env, capture_output=True, text=True,
                       timeout=600, cwd=str(tmp_path))
    assert r.returncode != 0 and "unknown baseline 'lstur'" in r.stderr


def test_the_measured_cases_settle():
    for case in M.all_measured_cases():
        assert all(v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP for v in case.bars().values()), case
    b, s, d, q, k, t = M.POLY_SHAPES[3]
    mask = M.poly_case(b, s, d, q, k, t).consts["mask"]
    assert bool(mask[0].all()) and not bool(mask[1].all())                 # user 0 fills every slot past the first 64-slot trip; user 1 is ragged
    empty = M.poly_case(2, 9, 64, 24, 5, 0, empty_user=0)
    out = empty.ref()["out"]
    assert not bool(empty.consts["mask"][0].any()) and torch.isfinite(out).all()
    assert torch.allclose(out[0], empty.leaves["x"][0].double().mean(0).expand_as(out[0]), atol=1e-12)       # uniform weights


def _own_count(case):
    bias = case.consts["bias"]
    return (bias.abs().sum(1) == 0).sum(1)                                  # the columns the caller zeroed: the user's own candidates


# (planted defect, the case of tests/test_gpu_miner.py that must see it, keyword arguments of the restatement)
_PLANTED = [
    ("masked logit -inf instead of 1e-30", lambda: M.poly_case(*M.POLY_SHAPES[0]), lambda c: dict(masked_logit=float("-inf"))),
    ("bias mean over the user's own columns", lambda: M.poly_case(*M.POLY_SHAPES[1]), lambda c: dict(bias_count=_own_count(c))),
    ("history slots >= 64 dropped", lambda: M.poly_case(*M.POLY_SHAPES[3]), lambda c: dict(slot_limit=64)),
    ("history slots >= 64 dropped, second trip", lambda: M.poly_case(*M.POLY_SHAPES[5]), lambda c: dict(slot_limit=128)),
    ("context codes >= 32 dropped", lambda: M.poly_case(*M.POLY_SHAPES[3]), lambda c: dict(code_limit=32)),
    ("context codes >= 32 dropped, K = 64", lambda: M.poly_case(*M.POLY_SHAPES[5]), lambda c: dict(code_limit=32)),
    ("tanh derivative left out of the backward", lambda: M.poly_case(*M.POLY_SHAPES[2]), lambda c: dict(tanh_grad=False)),
    ("projection route of d x left out", lambda: M.poly_case(*M.POLY_SHAPES[2]), lambda c: dict(projection_route=False)),
    ("softmax over C instead of K", lambda: M.target_case(*M.TARGET_SHAPES[1]), lambda c: dict(softmax_dim=1)),
]


@pytest.mark.parametrize("what,case,kwargs", _PLANTED, ids=[p[0] for p in _PLANTED])
def test_a_planted_defect_exceeds_its_bar_tenfold(what, case, kwargs):
    case = case()
    bars, ref = case.bars(), case.ref()
    bad = R.evaluate(case.fn, case.leaves, dict(case.consts, **kwargs(case)), case.upstream, torch.float64)
    ratios = {k: (R.rel_to_max(bad[k], ref[k]) / bars[k]["bar"] if bars[k]["bar"] > 0 else float("inf") * (R.rel_to_max(bad[k], ref[k]) > 0))
              for k in ref if R.rel_to_max(bad[k], ref[k]) > 0}
    print(what, case, {k: f"{v:.3g}" for k, v in ratios.items()})
    assert ratios and max(ratios.values()) >= 10.0, (what, ratios)
    if "derivative" in what or "route" in what:                            # defects of the backward alone: the forward stays under its bar
        assert ratios.get("out", 0.0) < 1.0
    if "route" in what:
        assert {k for k, v in ratios.items() if v >= 1.0} == {"d_x"}


def test_the_dot_product_bar_sees_a_dropped_term():
    """derived bar: one product of the D = 256 sum left out is ~ 1 / 16 of the result's spread, far over (D + 4) 2^-24 sum|a b|"""
    case = M.bmm_case(*M.BMM_SHAPES[0])
    ref, absolute = case.terms(), case.terms(absolute=True)
    a, rows = case.leaves["a"].double().numpy(), case.leaves["rows"].double().numpy()
    short = np.einsum("bmd,bnd->bmn", a[:, :, :-1], rows[:, :, :-1])
    assert R.derived_ratio(short, ref["out"][0], absolute["out"][0], ref["out"][1]) >= 10.0
    f32 = R.evaluate(case.fn, case.leaves, case.consts, case.upstream, torch.float32)
    for k in ref:
        assert R.derived_ratio(f32[k].numpy(), ref[k][0], absolute[k][0], ref[k][1]) <= 1.0, k


def test_the_record_of_measured_figures_lists_every_gpu_case():
    with open(os.path.join(ROOT, "profiles", "miner", "measured_tolerances.json")) as f:
        rec = json.load(f)
    for prefix in ("test_poly_attention", "test_target_attention", "test_batched_dot_product", "test_miner_forward"):
        hits = [k for k in rec if k.startswith(prefix)]
        assert hits, prefix
        assert all(isinstance(v, float) for k in hits for v in rec[k].values())
