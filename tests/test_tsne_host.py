"""t-SNE without a GPU: the float64 restatement (tests/tsne_ref.py) checked against the method's own identities, each planted defect
caught on the GPU tests' inputs at ten times the bar, the install keyword against stand-in reference modules, and the argument checks of
the five entry points (made before any launch)."""
import ctypes as C
import inspect
import sys
import types

import numpy as np
import pytest
import torch

import tsne_ref as R


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ---------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def small():
    X, labels = R.cluster_points(3, 4, 30, 8)
    idx, d2 = R.knn(R.normalise(X), 15)
    p, beta = R.affinities(d2, 5.0)
    return X, idx, d2, p, beta


def test_row_perplexities_meet_the_target(small):
    _, _, _, p, beta = small
    assert np.isfinite(p).all() and np.isfinite(beta).all()
    assert np.abs(p.sum(1) - 1).max() < 1e-12
    assert np.abs(R.perplexities(p) - 5.0).max() < 1e-4


def test_joint_p_is_symmetric_and_sums_to_one(small):
    _, idx, _, p, _ = small
    P = R.joint(idx, p)
    assert np.array_equal(P, P.T) and abs(P.sum() - 1) < 1e-12 and (np.diag(P) == 0).all()


def test_gradient_is_a_quarter_of_the_finite_difference_of_kl(small):
    _, idx, _, p, _ = small
    P = t64(R.joint(idx, p))
    Y = t64(np.random.default_rng(1).standard_normal((len(P), 2)))
    g = R.gradient(P, Y).numpy()
    h, worst = 1e-5, 0.0
    for i, c in [(0, 0), (7, 1), (55, 0), (119, 1)]:
        up, dn = Y.clone(), Y.clone()
        up[i, c] += h
        dn[i, c] -= h
        fd = float(R.kl_divergence(P, up) - R.kl_divergence(P, dn)) / (2 * h)
        worst = max(worst, abs(g[i, c] - fd / 4) / np.abs(g).max())
    assert worst < 1e-7, worst


def test_tiles_and_split_equal_the_package():
    from manner_amd import hip
    assert (hip.TSNE_TILE_I, hip.TSNE_TILE_J, hip.KNN_TILE_Q, hip.KNN_TILE_C) == (R.TILE_I, R.TILE_J, R.KNN_TILE_Q, R.KNN_TILE_C)
    for n in [0, 1, 2, 511, 512, 513, 1024, 1025, 4096, 16384, 65238, 2 ** 20]:
        assert hip.tsne_j_split(n) == R.j_split(n)
        assert 1 <= hip.tsne_j_split(n) <= max(1, -(-n // hip.TSNE_TILE_J))
    assert R.j_split(512) == 1 and R.j_split(513) == 2 and 513 in R.repulsion_sizes()
    assert hip.TSNE_STEP_ROWS == R.STEP_ROWS


def test_inputs_leave_no_row_out():
    for n, d, k in R.KNN_SHAPES:
        assert R.knn_continuous(n, d, k)[3] == 0


# ---------------------------------------------------------------- planted defects, on the GPU tests' own inputs
def moved(bad, good, bar):
    return R.rel_to_max(bad, good) / bar


@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
def test_defect_self_pair_left_in_z(scale):
    for n in [m for m in R.repulsion_sizes() if m > 1]:
        Y, _, z64, bars = R.repulsion_case(n, scale)
        _, zbad = R.repulsion(t64(Y), "self_in_z")
        assert moved(float(zbad), z64, bars["Z"]["bar"]) >= 10, (n, scale)


@pytest.mark.parametrize("defect,sizes", [("drop_last_tile", [R.TILE_J - 1, R.TILE_J + 1, 2 * R.TILE_J + 1]),
                                          ("drop_second_partial", [R.TILE_J + 1, 2 * R.TILE_J + 1])])
@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
def test_defect_dropped_j_rows(defect, sizes, scale):
    for n in sizes:
        Y, r64, _, bars = R.repulsion_case(n, scale)
        rbad, _ = R.repulsion(t64(Y), defect)
        assert moved(rbad[:, 2], r64[:, 2], bars["q"]["bar"]) >= 10, (n, scale)


@pytest.mark.parametrize("defect", ["drop_kth", "ties_high"])
def test_defect_in_the_neighbour_lists(defect):
    hit = 0
    for n, d, k in R.KNN_SHAPES:
        for kind in ("dup", "same", "runs"):
            X, idx, d2 = R.knn_integer(n, d, k, kind)
            bad = R.knn(X, k, defect)[0]
            hit += not np.array_equal(bad, idx)
        if defect == "drop_kth" and k > 1:
            X, idx, d2, _ = R.knn_continuous(n, d, k)
            bd2 = R.knn(X, k, defect)[1]
            assert (np.abs(bd2 - d2) / R.d2_bound(d2, d)).max() >= 10
    assert hit >= (3 * len(R.KNN_SHAPES)) // 2, hit                      # exact comparisons: any difference fails the GPU test


@pytest.mark.parametrize("defect,out", [("no_incoming", "Y"), ("incoming_first_k", "Y"), ("gains_eq", "gains"), ("no_centring", "Y")])
@pytest.mark.parametrize("kind", R.STEP_KINDS)
def test_defect_in_one_step(defect, out, kind):
    case, bars = R.step_case(kind)
    P = R.joint(case["idx"], case["p"], defect) if "incoming" in defect else case["P"]
    bad = R.step(t64(P), t64(case["Y"]), t64(case["u"]), t64(case["gains"]), case["ex"], case["mom"], case["lr"], defect)
    i = ("Y", "u", "gains").index(out)
    assert moved(bad[i], case["ref"][i], bars[out]["bar"]) >= 10


def test_star_list_has_a_hub_and_rows_without_incoming_edges():
    case, _ = R.step_case("star_early")
    indeg = np.bincount(case["idx"].reshape(-1), minlength=len(case["idx"]))
    assert indeg[0] > 1024 and (indeg[101:] == 0).all() and case["idx"].shape[1] < 1024
    assert (case["gains"] == np.float32(0.011)).mean() > 0.1 and (case["u"] == 0).mean() > 0.1
    flat, _ = R.step_case("flat")
    dY = flat["ref"][3]
    assert (dY[:, 1] == 0).all() and (flat["u"][:, 1] == 0).any() and (flat["u"][:, 1] != 0).any()


@pytest.mark.parametrize("defect", ["exaggeration_stays", "momentum_stays"])
def test_defect_in_the_schedule(defect):
    X, Y64, bars = R.ten_iterations_case(4)
    bad, _, _ = R.fit(X, 10.0, 10, 0, np.float64, n_iter_early_exag=4, defect=defect)
    assert moved(bad, Y64, bars["Y"]["bar"]) >= 10


def test_measured_bars_are_settled():
    for kind in R.AFFINITY_KINDS:
        for k in (1, 30, 90, 255):
            bars = R.affinity_case(kind, k)[4]
            assert all(b["bar"] >= R.FLOOR for b in bars.values())
            assert kind in ("constant", "zero") or not R.lucky(bars)
    for kind in R.STEP_KINDS:
        assert not R.lucky(R.step_case(kind)[1])


# ---------------------------------------------------------------- install(tsne=True)
@pytest.fixture
def fake_reference(monkeypatch):
    """a stand-in for the reference's packages, as far as install() looks: the four operator modules and a_module holding a TSNE"""
    from manner_amd import binding
    made = {}

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__file__ = "/nowhere/" + name.replace(".", "/") + ".py"
        for k, v in attrs.items():
            setattr(m, k, v)
        monkeypatch.setitem(sys.modules, name, m)
        made[name] = m
        return m

    for pkg in ("manner", "manner.models", "manner.models.components"):
        module(pkg).__path__ = []
    for leaf, names in binding.TARGETS.items():
        module("manner.models.components." + leaf, **{n: type(n, (), {}) for n in names})
    original = type("MulticoreTSNE", (), {})
    module("manner.models.a_module", TSNE=original)
    monkeypatch.delitem(sys.modules, "MulticoreTSNE", raising=False)
    yield made, original
    binding.uninstall()


def test_install_rebinds_tsne_only_on_request(fake_reference):
    import manner_amd
    from manner_amd import binding
    from manner_amd.manifold import TSNE as Own
    made, original = fake_reference
    a_module = made["manner.models.a_module"]
    report = manner_amd.install()
    assert "manner.models.a_module" not in report and a_module.TSNE is original and "MulticoreTSNE" not in sys.modules
    assert sorted(report) == sorted("manner.models.components." + leaf for leaf in binding.TARGETS)
    report = manner_amd.install(tsne=True)
    assert report["manner.models.a_module"] == ["TSNE"] and a_module.TSNE is Own
    assert sys.modules["MulticoreTSNE"].MulticoreTSNE is Own                     # the shim: `from MulticoreTSNE import MulticoreTSNE` gives the mirror
    assert binding.installed()["manner.models.a_module"] == ["TSNE"] and binding.installed()["MulticoreTSNE"] == ["MulticoreTSNE"]
    manner_amd.install(tsne=True)                                                # idempotent
    assert a_module.TSNE is Own
    manner_amd.uninstall()
    assert a_module.TSNE is original and "MulticoreTSNE" not in sys.modules and binding.installed() == {}


def test_install_patches_an_alias_of_the_real_package_by_identity(fake_reference, monkeypatch):
    import manner_amd
    from manner_amd.manifold import TSNE as Own
    made, original = fake_reference
    real = types.ModuleType("MulticoreTSNE")
    real.MulticoreTSNE = original
    monkeypatch.setitem(sys.modules, "MulticoreTSNE", real)
    made["manner.models.a_module"].Embedder = original                          # a second name for the same class
    manner_amd.install(tsne=True)
    assert made["manner.models.a_module"].TSNE is Own and made["manner.models.a_module"].Embedder is Own
    assert sys.modules["MulticoreTSNE"] is real and real.MulticoreTSNE is original          # the real package is left alone
    manner_amd.uninstall()
    assert made["manner.models.a_module"].TSNE is original and made["manner.models.a_module"].Embedder is original
    assert sys.modules["MulticoreTSNE"] is real


def test_constructor_carries_the_package_names_and_defaults():
    from manner_amd.manifold import TSNE
    sig = inspect.signature(TSNE.__init__).parameters
    expected = dict(n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate=200.0, n_iter=1000, n_iter_early_exag=250, angle=0.5,
                    init="random", random_state=None)
    for name, default in expected.items():
        assert sig[name].default == default and sig[name].kind == sig[name].POSITIONAL_OR_KEYWORD, name
    assert "n_jobs" in sig and "verbose" in sig
    TSNE(n_jobs=8)                                                               # a_module.py:150-173, 191-212: TSNE(n_jobs=8)
    with pytest.raises(ValueError, match="n_components"):
        TSNE(n_components=3)
    assert "IGNORED" in TSNE.__doc__ and "angle" in TSNE.__doc__


def test_there_is_no_cpu_fallback():
    from manner_amd.manifold import TSNE
    expected = (ValueError, "neighbours") if torch.cuda.is_available() else (RuntimeError, "no CPU fallback")
    with pytest.raises(expected[0], match=expected[1]):
        TSNE(perplexity=30).fit_transform(np.zeros((90, 4), np.float32))       # 90 rows have 89 others: fewer than 3 x 30


# ---------------------------------------------------------------- the entries' argument checks: before any launch, no device needed
def _lib():
    from manner_amd import _lib
    return _lib.load()


_BUF = (C.c_double * 64)()                                                       # never dereferenced: every case below fails a check first


def _p(null, name):
    return C.c_void_p(0 if name in null else C.addressof(_BUF))


def _call(entry, null=(), **o):
    lib = _lib()
    a = dict(N=100, D=16, k=30, split=R.j_split(o.get("N", 100)), n_in=3000, perp=10.0)
    a.update(o)
    p = lambda name: _p(null, name)
    if entry == "knn_rows_f32":
        rc = lib.manner_hip_knn_rows_f32(p("x"), a["N"], a["D"], a["k"], p("idx"), p("d2"), None)
    elif entry == "tsne_affinities":
        rc = lib.manner_hip_tsne_affinities(p("d2"), a["N"], a["k"], C.c_float(a["perp"]), p("p"), p("beta"), None)
    elif entry == "tsne_repulsion":
        rc = lib.manner_hip_tsne_repulsion(p("y"), a["N"], a["split"], p("part"), p("zpart"), None)
    elif entry == "tsne_step":
        rc = lib.manner_hip_tsne_step(p("y"), p("part"), p("zpart"), a["split"], p("out_idx"), p("out_p"), a["k"], p("in_off"), p("in_src"), p("in_p"),
                                      a["n_in"], a["N"], C.c_float(12.0), C.c_float(0.5), C.c_float(200.0), p("u"), p("gains"), p("y_out"), p("ypart"),
                                      None)
    else:
        rc = lib.manner_hip_tsne_kl(p("y"), p("zpart"), a["split"], p("out_idx"), p("out_p"), a["k"], a["N"], p("klpart"), p("kl"), None)
    return rc, lib.manner_hip_last_error().decode()


POINTERS = {"knn_rows_f32": ["x", "idx", "d2"], "tsne_affinities": ["d2", "p", "beta"], "tsne_repulsion": ["y", "part", "zpart"],
            "tsne_step": ["y", "part", "zpart", "out_idx", "out_p", "in_off", "in_src", "in_p", "u", "gains", "y_out", "ypart"],
            "tsne_kl": ["y", "zpart", "out_idx", "out_p", "klpart", "kl"]}
BAD = [("knn_rows_f32", dict(k=256), "k=256"), ("knn_rows_f32", dict(k=0), "k=0"), ("knn_rows_f32", dict(D=1025), "D=1025"),
       ("knn_rows_f32", dict(D=0), "D=0"), ("knn_rows_f32", dict(N=30), "N=30"), ("knn_rows_f32", dict(N=2 ** 20 + 1), "N=1048577"),
       ("knn_rows_f32", dict(N=-1), "N=-1"),
       ("tsne_affinities", dict(k=256), "k=256"), ("tsne_affinities", dict(N=2 ** 20 + 1), "N=1048577"),
       ("tsne_affinities", dict(perp=0.0), "perplexity"),
       ("tsne_repulsion", dict(N=2 ** 20 + 1), "N=1048577"), ("tsne_repulsion", dict(N=1025, split=1), "split=1"),
       ("tsne_step", dict(k=256), "k=256"), ("tsne_step", dict(N=30), "N=30"), ("tsne_step", dict(N=2 ** 20 + 1), "N=1048577"),
       ("tsne_step", dict(N=1025, split=2), "split=2"), ("tsne_step", dict(n_in=3001), "n_in=3001"),
       ("tsne_kl", dict(k=256), "k=256"), ("tsne_kl", dict(N=30), "N=30"), ("tsne_kl", dict(N=2 ** 20 + 1), "N=1048577"),
       ("tsne_kl", dict(N=1025, split=1), "split=1")]


@pytest.mark.parametrize("entry,over,word", BAD)
def test_entries_refuse_bad_shapes(entry, over, word):
    rc, msg = _call(entry, **over)
    assert rc == 1 and entry in msg and word in msg, (rc, msg)


@pytest.mark.parametrize("entry,null", [(e, n) for e, names in POINTERS.items() for n in names])
def test_entries_refuse_null_pointers(entry, null):
    rc, msg = _call(entry, null=(null,))
    assert rc == 1 and entry in msg and "null" in msg, (rc, msg)


def test_step_refuses_to_update_in_place():
    lib = _lib()
    b = lambda: C.c_void_p(C.addressof(_BUF))
    rc = lib.manner_hip_tsne_step(b(), b(), b(), 1, b(), b(), 30, b(), b(), b(), 3000, 100, C.c_float(1.0), C.c_float(0.5), C.c_float(200.0), b(), b(),
                                  b(), b(), None)
    assert rc == 1 and "y_out must not be y" in lib.manner_hip_last_error().decode()


@pytest.mark.parametrize("entry", list(POINTERS))
def test_entries_with_no_rows_launch_nothing(entry):
    rc, _ = _call(entry, null=tuple(POINTERS[entry]), N=0, n_in=0, split=1)
    assert rc == 0


def test_exports_are_declared_and_bound_under_abi_8():
    from manner_amd import _lib
    from manner_amd.build import SOURCES
    names = ["manner_hip_knn_rows_f32", "manner_hip_tsne_affinities", "manner_hip_tsne_repulsion", "manner_hip_tsne_step", "manner_hip_tsne_kl"]
    lib = _lib.load()
    for n in names:
        assert n in _lib.header_symbols() and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.manner_hip_abi_version() == 8 == _lib.ABI_VERSION and "tsne.hip" in SOURCES
