"""The LSTUR baseline's operators without a GPU: the float64 restatement of tests/lstur_ref.py against the reference's own outputs and
gradients (tests/golden/lstur.npz, float64 and float32), the mirrors' state-dict keys and shapes against the reference's
(lstur_state_dict_keys.json), ``install(baselines=("lstur_plm",))`` in a fresh interpreter over a reference-layout tree in both call
orders, and four planted defects, each shown to exceed the bar at least 10-fold on ``out`` at shapes tests/test_gpu_lstur.py runs."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import lstur_ref as LR
import side_ops_ref as R
from test_host import _classes, _imports, _write_reference_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("ini", "con")


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "lstur.npz"))
    return z, json.loads(str(z["meta"]))


def golden_case(z, method):
    """(leaves, consts, upstream) of the restatement on the golden's values"""
    leaves = {"x": torch.from_numpy(z["user_x"])}
    leaves.update({name: torch.from_numpy(z[f"user_{method}_sd:" + key]) for name, key in LR.STATE_KEYS.items()})
    consts = {"user": torch.from_numpy(z["user"]), "lengths": torch.from_numpy(z["lengths"]), "method": method}
    return leaves, consts, {"out": torch.from_numpy(z[f"user_{method}_up"])}


def golden_want(z, method, prefix):
    want = {"out": z[f"{prefix}_{method}_out"], "d_x": z[f"{prefix}_{method}_d_x"]}
    want.update({"d_" + name: z[f"{prefix}_{method}_grad:" + key] for name, key in LR.STATE_KEYS.items()})
    return want


@pytest.mark.parametrize("method", METHODS)
def test_restatement_matches_the_reference_in_float64(golden, method):
    """the reference's own LSTURUserEncoder run in float64 (``user64_*``: nn.GRU on the packed sequence) against the float64
    restatement on the same values: every output and gradient within 1e-10 of its tensor's largest entry"""
    z, meta = golden
    assert (meta["shape"]["B"], meta["shape"]["S"], meta["shape"]["I"]) == LR.GOLDEN_SHAPE[:3]
    assert z["user"].tolist() == [1, 0, 3, 3] == LR.users_of(4).tolist() and z["lengths"].tolist() == [5, 1, 3, 2]
    ref64 = R.evaluate(LR.lstur_user, *golden_case(z, method), torch.float64)
    for k, w in golden_want(z, method, "user64").items():
        assert w.dtype == np.float64 and tuple(w.shape) == tuple(ref64[k].shape), k
        err = R.rel_to_max(torch.from_numpy(w), ref64[k])
        assert err <= 1e-10, (k, err)
    assert float(ref64["d_table"][0].abs().max()) == 0.0 and not z[f"user64_{method}_grad:long_term_user_embedding.weight"][0].any()
    assert not ref64["d_x"][1, 1:].any() and not z[f"user64_{method}_d_x"][1, 1:].any() and ref64["d_x"][1, 0].any()      # d x past the length


@pytest.mark.parametrize("method", METHODS)
def test_restatement_matches_the_reference(golden, method):
    """float64 on the golden's float32 inputs against the reference's float32 results: every output and gradient within 8 x the
    restatement's own float32 error (and no tighter than 8 half-ulps)"""
    z, _ = golden
    case = golden_case(z, method)
    ref64, ref32 = R.evaluate(LR.lstur_user, *case, torch.float64), R.evaluate(LR.lstur_user, *case, torch.float32)
    for k, w in golden_want(z, method, "user").items():
        assert tuple(w.shape) == tuple(ref64[k].shape), k
        bar = R.MEASURED_FACTOR * max(R.rel_to_max(ref32[k], ref64[k]), R.U32)
        err = R.rel_to_max(torch.from_numpy(np.asarray(w)), ref64[k])
        assert err <= bar, (k, err, bar)


def test_mirror_state_dict_keys_and_shapes_match_the_reference(golden, golden_dir):
    from manner_amd.models.components.news_encoder import LSTURCategoryEncoder, LSTURNewsEncoder
    from manner_amd.models.components.user_encoder import LSTURUserEncoder
    with open(os.path.join(golden_dir, "lstur_state_dict_keys.json")) as f:
        want = json.load(f)
    n, shape = golden[1]["news"], golden[1]["shape"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mirrors = {"LSTURUserEncoder_" + m: LSTURUserEncoder(num_users=shape["num_users"], input_dim=shape["I"], user_masking_probability=0.5,
                                                             long_short_term_method=m) for m in METHODS}
        mirrors["LSTURCategoryEncoder"] = LSTURCategoryEncoder(num_categories=n["num_categories"], category_embedding_dim=n["category_dim"])
        mirrors["LSTURNewsEncoder"] = LSTURNewsEncoder(plm_model=n["preset"], frozen_layers=n["frozen_layers"], text_embedding_dim=128,
                                                       num_attention_heads=n["text_heads"], query_vector_dim=n["query_dim"], dropout_probability=0.2,
                                                       num_categories=n["num_categories"], category_embedding_dim=n["category_dim"])
    for name, module in mirrors.items():
        assert {k: list(v.shape) for k, v in module.state_dict().items()} == want[name], name
    assert set(want["LSTURUserEncoder_ini"]) == {"long_term_user_embedding.weight", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0",
                                                 "gru.bias_hh_l0"} == set(LR.STATE_KEYS.values())
    i = shape["I"]
    assert want["LSTURUserEncoder_ini"]["gru.weight_hh_l0"] == [3 * i, i] and want["LSTURUserEncoder_con"]["gru.weight_hh_l0"] == [3 * (i // 2), i // 2]
    assert want["LSTURUserEncoder_con"]["long_term_user_embedding.weight"] == [shape["num_users"], i // 2]
    assert not mirrors["LSTURUserEncoder_ini"].long_term_user_embedding.weight[0].any()                  # padding_idx = 0
    assert {k.split(".")[0] for k in want["LSTURNewsEncoder"]} == {"text_encoder", "category_encoder"}


_LSTUR_SCRIPT = r'''
import json, sys, types
import manner_amd, manner_amd.binding
ref = sys.argv[1]
early = "--early" in sys.argv
sys.path.insert(0, ref)
cls = lambda c: c.__module__ + "." + c.__qualname__
out = {}
if early:                                         # the reference's modules imported, and an alias taken, BEFORE install()
    import manner.models.components.news_encoder as NE, manner.models.components.user_encoder as UE
    from manner.models.components.user_encoder import LSTURUserEncoder as UserEncoderEarly
    fake = types.ModuleType("manner.models.fake_caller")
    fake.UserEncoder = UserEncoderEarly
    sys.modules["manner.models.fake_caller"] = fake
else:
    manner_amd.install(ref)
    import manner.models.components.news_encoder as NE, manner.models.components.user_encoder as UE
    manner_amd.uninstall()
three = ((NE, "LSTURCategoryEncoder"), (NE, "LSTURNewsEncoder"), (UE, "LSTURUserEncoder"))
state = lambda: {n: cls(getattr(m, n)) for m, n in three}
manner_amd.install(ref)
out["plain"], out["plain_installed"] = state(), manner_amd.binding.installed()
manner_amd.uninstall()
for other in ("miner", "caum_plm"):
    manner_amd.install(ref, baselines=(other,))
    out[other] = state()
    manner_amd.uninstall()
try:
    manner_amd.install(ref, baselines=("lstur",))
    out["unknown"] = "no error"
except ValueError as e:
    out["unknown"] = str(e)
out["after_unknown"], out["after_unknown_state"] = manner_amd.binding.installed(), state()
out["report"] = manner_amd.install(ref, baselines=("lstur_plm",))
ns = {}
with open(ref + "/manner/models/baselines/lstur_plm_module.py") as f:
    for l in f:
        if l.startswith("from manner."):
            try:
                exec(l, ns)
            except ModuleNotFoundError as e:                     # a third-party package this image lacks
                assert (e.name or "").split(".")[0] != "manner", (l, e)
out["module"] = {k: cls(v) for k, v in ns.items() if isinstance(v, type)}
out["bound"] = state()
if early:
    out["alias"] = cls(fake.UserEncoder)
out["kept"] = {n: cls(getattr(NE, n)) for n in ("NAMLNewsEncoder", "MINERNewsEncoder", "CAUMNewsEncoder")}
out["kept"].update({n: cls(getattr(UE, n)) for n in ("CAUMUserEncoder", "MINSUserEncoder")})
out["again"] = manner_amd.install(ref, baselines=("lstur_plm",))   # idempotent
manner_amd.uninstall()
out["after_uninstall"] = state()
if early:
    out["alias_after_uninstall"] = cls(fake.UserEncoder)
print("RESULT " + json.dumps(out))
'''


def _lstur_reference_layout(root):
    """test_host's reference-layout tree (class names only, nothing of the reference's code) plus the two category encoders and the
    import lines of baselines/lstur_plm_module.py"""
    comp = "manner.models.components"
    reference = _write_reference_layout(root)
    with open(os.path.join(reference, "manner/models/components/news_encoder.py"), "a") as f:
        f.write(_classes("LSTURCategoryEncoder", "CAUMCategoryEncoder"))
    with open(os.path.join(reference, "manner/models/baselines/lstur_plm_module.py"), "w") as f:
        f.write(_imports(("manner.data.components.mind_batch", "MINDRecBatch", None), ("manner.metrics.diversity", "Diversity", None),
                         (f"{comp}.click_predictors", "DotProduct", None), (f"{comp}.news_encoder", "LSTURNewsEncoder", "NewsEncoder"),
                         (f"{comp}.user_encoder", "LSTURUserEncoder", "UserEncoder")) + _classes("LSTURPLMModule"))
    return reference


@pytest.mark.parametrize("early", [False, True], ids=["install-first", "import-first"])
def test_install_rebinds_the_lstur_classes_only_when_asked(early, tmp_path):
    """``install()``, ``install(baselines=("miner",))`` and ``("caum_plm",)`` leave the three LSTUR classes the reference's own;
    ``"lstur"`` is an unknown name, raises and binds nothing; ``install(baselines=("lstur_plm",))`` rebinds the three, so that
    lstur_plm_module.py's import lines yield the mirrors under ``NewsEncoder`` and ``UserEncoder`` — whether the reference's modules
    were imported before ``install()`` (an alias taken earlier is rebound too) or after; ``uninstall()`` restores them."""
    reference = _lstur_reference_layout(str(tmp_path / "reference"))
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", _LSTUR_SCRIPT, reference] + (["--early"] if early else []), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    ref, mir = "manner.models.components.", "manner_amd.models.components."
    where = {"LSTURCategoryEncoder": "news_encoder.", "LSTURNewsEncoder": "news_encoder.", "LSTURUserEncoder": "user_encoder."}
    originals = {n: ref + m + n for n, m in where.items()}
    assert out["plain"] == originals == out["miner"] == out["caum_plm"]
    assert not any(n.startswith("LSTUR") for names in out["plain_installed"].values() for n in names)
    assert "unknown baseline 'lstur'" in out["unknown"] and "lstur_plm" in out["unknown"]
    assert out["after_unknown"] == {} and out["after_unknown_state"] == originals
    assert out["bound"] == {n: mir + m + n for n, m in where.items()}
    assert {"LSTURCategoryEncoder", "LSTURNewsEncoder"} <= set(out["report"][ref + "news_encoder"]) and "LSTURUserEncoder" in out["report"][ref + "user_encoder"]
    assert out["module"]["NewsEncoder"] == mir + "news_encoder.LSTURNewsEncoder" and out["module"]["UserEncoder"] == mir + "user_encoder.LSTURUserEncoder"
    assert all(v.startswith(ref) for v in out["kept"].values()), out["kept"]
    assert out["again"] == {}
    assert out["after_uninstall"] == originals
    if early:
        assert out["report"]["manner.models.fake_caller"] == ["UserEncoder"] and out["alias"] == mir + "user_encoder.LSTURUserEncoder"
        assert out["alias_after_uninstall"] == originals["LSTURUserEncoder"]


def test_run_takes_lstur_plm_as_a_baseline(tmp_path):
    reference = _lstur_reference_layout(str(tmp_path / "reference"))
    script = tmp_path / "entry.py"
    script.write_text("import sys\nfrom manner.models.components.news_encoder import LSTURNewsEncoder, CAUMNewsEncoder\n"
                      "from manner.models.components.user_encoder import LSTURUserEncoder\n"
                      "print('ARGV', sys.argv[1:], LSTURNewsEncoder.__module__, LSTURUserEncoder.__module__, CAUMNewsEncoder.__module__)\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + reference, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-m", "manner_amd.run", "--baselines", "lstur_plm", str(script), "experiment=x"], env=env, capture_output=True,
                       text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert ("ARGV ['experiment=x'] manner_amd.models.components.news_encoder manner_amd.models.components.user_encoder "
            "manner.models.components.news_encoder") in r.stdout, r.stdout


def _all_cases():
    return [LR.gru_case(*s) for s in LR.GRU_SHAPES] + [LR.strided_case()] + [LR.user_case(*s) for s in LR.USER_SHAPES]


def test_the_measured_cases_settle_and_cover_what_they_name():
    for case in _all_cases():
        assert all(v["cpu_f32"] == 0 or v["cpu_f32"] >= R.QUARTER_ULP for v in case.bars().values()), case
    shapes = [s[:4] for s in LR.GRU_SHAPES]
    assert any(s[0] == LR.ROW_TILE + 1 for s in shapes) and any(s[3] == LR.UNIT_SLICE + 1 for s in shapes) and any(s[3] == 1 for s in shapes)
    assert (2, 2, 1024, 1024) in shapes and (2, 256, 4, 4) in shapes and any(s[0] == 1 for s in shapes) and any(s[1] == 1 for s in shapes)
    assert (2, 3, 868, "ini") in LR.USER_SHAPES and (2, 3, 868, "con") in LR.USER_SHAPES
    ones, full = LR.gru_case(3, 3, 6, 6, "ones", True), LR.gru_case(3, 3, 6, 6, "full", False)
    assert ones.consts["lengths"].tolist() == [1, 1, 1] and full.consts["lengths"].tolist() == [3, 3, 3]
    mixed = LR.gru_case(*LR.GRU_SHAPES[0])
    assert mixed.consts["lengths"].max() == 5 and mixed.consts["lengths"].min() == 1
    assert not mixed.ref()["d_x"][-1, 1:].any() and mixed.ref()["d_x"][-1, 0].any()                    # d x is exactly 0 past the length
    strided = LR.strided_case()
    lo, hi = strided.consts["channels"]
    assert "h0" not in strided.leaves and strided.leaves["x"].shape[2] == 24 and hi - lo == 8 == strided.leaves["w_hh"].shape[1]
    assert not strided.ref()["d_x"][:, :, :lo].any() and not strided.ref()["d_x"][:, :, hi:].any()
    user = LR.user_case(4, 5, 6, "ini")
    assert user.consts["user"].tolist() == [1, 0, 3, 3] and not user.leaves["table"][0].any()
    d_table = user.ref()["d_table"]
    assert not d_table[0].any() and not d_table[2].any() and not d_table[4:].any() and d_table[1].any() and d_table[3].any()


def _per_user_keep(case, p=0.5, seed=5):
    keep = torch.from_numpy((np.random.default_rng(seed).random(case.leaves["x"].shape[0]) >= p).astype(np.uint8))
    keep[0], keep[-1] = 1, 0                                     # at least one user kept and one dropped
    return keep


def _per_element_keep(case, p=0.5, seed=5):
    """the per-user mask with one element of a kept user's row dropped: what per-element draws would do"""
    keep = _per_user_keep(case, p, seed)[:, None].repeat(1, case.leaves["table"].shape[1])
    keep[0, 0] = 0
    return keep


# (planted defect, keyword arguments of the restatement as a function of the case, the correct arguments to compare against)
_PLANTED = [
    ("gate order z | r | n", lambda c: dict(gate_order="zrn"), lambda c: {}),
    ("r applied before the hidden matmul", lambda c: dict(reset_before_matmul=True), lambda c: {}),
    ("last hidden taken at S instead of len", lambda c: dict(last_at_s=True), lambda c: {}),
    ("the mask applied per element instead of per user", lambda c: dict(p=0.5, keep=_per_element_keep(c)), lambda c: dict(p=0.5, keep=_per_user_keep(c))),
]


@pytest.mark.parametrize("shape", LR.DEFECT_SHAPES, ids=lambda s: "B{}-S{}-I{}-{}".format(*s))
@pytest.mark.parametrize("what,kwargs,good", _PLANTED, ids=[p[0] for p in _PLANTED])
def test_a_planted_defect_exceeds_the_bar_tenfold_on_out(what, kwargs, good, shape):
    case = LR.user_case(*shape)
    assert case.leaves["x"].shape[0] >= 2 and case.leaves["x"].shape[1] >= 3 and case.consts["lengths"].min() < case.leaves["x"].shape[1]
    right = good(case)
    if right:                                                    # the masking case: bar and reference with the per-user mask
        case = R.Case(str(case) + "-masked", case.fn, case.leaves, dict(case.consts, **right), case.upstream)
    bar, ref = case.bars()["out"]["bar"], case.ref()["out"]
    bad = R.evaluate(case.fn, case.leaves, dict(case.consts, **kwargs(case)), None, torch.float64)["out"]
    ratio = R.rel_to_max(bad, ref) / bar
    print(what, case, f"{ratio:.3g} x the bar")
    assert ratio >= 10.0, (what, ratio)


def test_the_record_of_measured_figures_lists_every_gpu_case():
    with open(os.path.join(ROOT, "profiles", "lstur", "measured_tolerances.json")) as f:
        rec = json.load(f)
    for prefix, count in (("test_gru_forward_and_backward", len(LR.GRU_SHAPES)), ("test_gru_reads_a_strided_channel_view", 1),
                          ("test_user_encoder_forward_and_backward", len(LR.USER_SHAPES)), ("test_user_encoder_mirror_matches_the_reference", 2)):
        hits = [k for k in rec if k.startswith(prefix)]
        assert len(hits) == count, (prefix, hits)
        assert all(isinstance(v, float) for k in hits for v in rec[k].values())
