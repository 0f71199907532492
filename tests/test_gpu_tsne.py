"""The t-SNE kernels (csrc/tsne.hip) and manner_amd.manifold.TSNE against the float64 restatement of tests/tsne_ref.py, at the shapes
where the kernels can go wrong: one off either side of every tile, more than one workgroup, the first N whose j range is split, a hub
with more incoming edges than a wave walks in sixteen trips, and the searches' far ends.  Bars: module docstring of tsne_ref."""
import numpy as np
import pytest
import torch

import tsne_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def held(got, ref64, bar, what, measured=None):
    err = R.rel_to_max(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, ref64)
    print(f"{what}: error {err:.3e} of the largest entry, bar {bar['bar']:.3e} (float32 on the CPU {bar['cpu_f32']:.3e})")
    if measured is not None:
        measured(**{what + " gpu": err, what + " cpu_f32": bar["cpu_f32"], what + " bar": bar["bar"]})
    assert err <= bar["bar"], (what, err, bar)


# ---------------------------------------------------------------- neighbours
@pytest.mark.parametrize("n,d,k", R.KNN_SHAPES)
def test_knn_exact_on_integer_rows(n, d, k):
    from manner_amd import hip
    for kind in ("dup", "same", "runs"):
        X, idx, d2 = R.knn_integer(n, d, k, kind)
        gi, gd = hip.knn(dev(X), k)
        assert torch.equal(gi.cpu(), torch.from_numpy(idx)), kind
        assert torch.equal(gd.cpu(), torch.from_numpy(d2.astype(np.float32))), kind


@pytest.mark.parametrize("n,d,k", R.KNN_SHAPES)
def test_knn_on_continuous_rows(n, d, k):
    from manner_amd import hip
    X, idx, d2, left_out = R.knn_continuous(n, d, k)
    assert left_out == 0                                                   # every row's k-th gap exceeds twice the bar
    gi, gd = hip.knn(dev(X), k)
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.sort(gi, 1), np.sort(idx, 1))
    ref_of_got = np.take_along_axis(R.sqdist(X), gi.astype(np.int64), 1)   # the float64 distance of the neighbour the kernel names
    ratio = np.abs(gd - ref_of_got) / R.d2_bound(ref_of_got, d)
    print(f"d2: worst error / derived bar {ratio.max():.3f}")
    assert (ratio <= 1).all()
    assert (np.diff(gd, axis=1) >= 0).all() and (gi != np.arange(n)[:, None]).all()


def test_knn_refuses_too_few_rows():
    from manner_amd import hip
    with pytest.raises(RuntimeError, match="fewer than k"):
        hip.knn(torch.zeros(30, 4, device=DEV), 30)


# ---------------------------------------------------------------- affinities
@pytest.mark.parametrize("k", [1, 30, 90, 255])
@pytest.mark.parametrize("kind", R.AFFINITY_KINDS)
def test_affinities(kind, k, measured):
    from manner_amd import hip
    d2, p64, b64, perp, bars = R.affinity_case(kind, k)
    p, beta = hip.tsne_affinities(dev(d2), perp)
    assert torch.isfinite(p).all() and torch.isfinite(beta).all()
    held(p, p64, bars["p"], f"p[{kind}, k={k}]", measured)
    if k > 1 and kind == "doubling":
        assert float(beta.min()) > 2.0 ** 30
    if k > 1 and kind == "halving":
        assert float(beta.max()) < 2.0 ** -30


@pytest.mark.parametrize("n", [3, 4, 5, 9])
def test_affinities_at_the_workgroup_edge(n):
    from manner_amd import hip
    d2, p64, _, perp, bars = R.affinity_case("continuous", 90)
    p, _ = hip.tsne_affinities(dev(d2[:n]), perp)
    full, _ = hip.tsne_affinities(dev(d2), perp)
    assert torch.equal(p, full[:n])                                        # a row's bits do not depend on N


# ---------------------------------------------------------------- repulsion
@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
@pytest.mark.parametrize("n", R.repulsion_sizes())
def test_repulsion(n, scale, measured):
    from manner_amd import hip
    Y, r64, z64, bars = R.repulsion_case(n, scale)
    part, zpart = hip.tsne_repulsion(dev(Y))
    split = hip.tsne_j_split(n)
    assert part.shape == (split, n, 4) and (split > 1) == (n > hip.TSNE_TILE_J)
    rows = part[0].clone()
    for s in range(1, split):                                              # a row's partials in ascending order, as the consumer adds them
        rows += part[s]
    tag = f"[N={n}, scale={scale:g}]"
    held(rows[:, 0], r64[:, 0], bars["fx"], "sum q^2 dx" + tag, measured)
    held(rows[:, 1], r64[:, 1], bars["fy"], "sum q^2 dy" + tag, measured)
    held(rows[:, 2], r64[:, 2], bars["q"], "sum q" + tag, measured)
    assert (part[..., 3] == 0).all()
    z = float(zpart.sum().item()) - n
    if n > 1:
        held(np.float64(z), z64, bars["Z"], "Z" + tag, measured)
    else:
        assert z == 0.0


# ---------------------------------------------------------------- one step
@pytest.mark.parametrize("kind", R.STEP_KINDS)
def test_step(kind, measured):
    from manner_amd import hip
    from manner_amd.manifold import edge_transpose
    case, bars = R.step_case(kind)
    n = len(case["Y"])
    y, u, gains = dev(case["Y"]), dev(case["u"]), dev(case["gains"])
    idx, p = dev(case["idx"]), dev(case["p"])
    in_off, in_src, in_p = edge_transpose(idx, p)
    counts = (in_off[1:] - in_off[:-1]).cpu()
    assert int(counts[0]) == n - 1 > 1024 and int(counts[101:].max()) == 0 and int(in_off[-1]) == idx.numel()
    assert bool((in_src[: n - 1].cpu() == torch.arange(1, n)).all())        # the hub's incoming edges in ascending source order
    part, zpart = hip.tsne_repulsion(y)
    y_out = torch.empty_like(y)
    ypart = torch.empty(2 * -(-n // hip.TSNE_STEP_ROWS), dtype=torch.float64, device=DEV)
    hip.tsne_step(y, part, zpart, idx, p, in_off, in_src, in_p, u, gains, y_out, ypart, case["ex"], case["mom"], case["lr"])
    assert torch.equal(y.cpu(), torch.from_numpy(case["Y"]))               # the input coordinates are left alone
    held(y_out, case["ref"][0], bars["Y"], f"Y[{kind}]", measured)
    held(u, case["ref"][1], bars["u"], f"u[{kind}]", measured)
    held(gains, case["ref"][2], bars["gains"], f"gains[{kind}]", measured)
    assert float(gains.min()) == pytest.approx(0.01, rel=1e-6)             # some gains came to rest on the floor
    if kind == "flat":
        zero = torch.from_numpy(case["u"][:, 1] == 0)
        assert (u[:, 1].cpu()[zero] == 0).all()                            # dY = 0 and u = 0 stay 0


# ---------------------------------------------------------------- the fit
@pytest.mark.parametrize("early", [250, 4])
def test_ten_iterations(early, measured):
    from manner_amd.manifold import TSNE
    X, Y64, bars = R.ten_iterations_case(early)
    t = TSNE(perplexity=10.0, n_iter=10, n_iter_early_exag=early, random_state=0)
    Y = t.fit_transform(dev(X), as_tensor=True)
    assert Y.is_cuda and Y.dtype == torch.float32 and t.n_iter_ == 10
    held(Y, Y64, bars["Y"], f"Y after 10 iterations[early={early}]", measured)


@pytest.mark.parametrize("n", R.ROW_EDGE_SIZES)
def test_step_and_kl_at_the_row_tile_edges(n, measured):
    """three iterations and the KL at one off either side of the step / KL kernels' 64 rows per workgroup, and past two workgroups"""
    from manner_amd.manifold import TSNE
    X, Y64, kl64, bars = R.fit_case(n, 5.0, 3, 250)
    t = TSNE(perplexity=5.0, n_iter=3, random_state=0)
    Y = t.fit_transform(dev(X), as_tensor=True)
    held(Y, Y64, bars["Y"], f"Y after 3 iterations[N={n}]", measured)
    held(np.float64(t.kl_divergence_), np.float64(kl64), bars["kl"], f"KL after 3 iterations[N={n}]", measured)


@pytest.fixture(scope="module")
def end_to_end():
    from manner_amd.manifold import TSNE
    X, labels, P, kls, purities = R.end_to_end_case()
    t = TSNE(perplexity=10.0, random_state=0)
    Y = t.fit_transform(X)
    return t, Y, X, labels, P, kls, purities


def test_end_to_end_separates_the_clusters(end_to_end):
    t, Y, X, labels, P, kls, purities = end_to_end
    assert isinstance(Y, np.ndarray) and Y.dtype == np.float64 and Y.shape == (300, 2) and np.isfinite(Y).all()
    assert t.embedding_ is Y and t.n_iter_ == 1000
    assert (purities == 1.0).all()                                        # the restatement, from all eight initialisations
    assert R.purity(Y, labels) == 1.0
    spread = (kls.max() - kls.min()) / kls.mean()
    print(f"float64 restatement: KL {kls.min():.4f} .. {kls.max():.4f}, spread {spread:.4f}; this fit: {t.kl_divergence_:.4f}")
    assert t.kl_divergence_ <= kls.max() * (1 + spread)


def test_kl_is_the_kl_of_the_returned_embedding(end_to_end, measured):
    t, Y, X, labels, P, kls, purities = end_to_end
    Yt = torch.from_numpy(Y)
    kl64 = R.kl_divergence(P, Yt)
    # the float32 side of the bar: the same evaluation in float32 from the float32 pipeline's own P
    _, _, (idx32, p32) = R.fit(X, 10.0, 0, 0, np.float32)
    kl32 = R.kl_divergence(torch.from_numpy(R.joint(idx32, p32)).float(), Yt.float())
    bar = R.measured_bar(kl32, kl64)
    assert not R.lucky({"kl": bar})
    held(np.float64(t.kl_divergence_), kl64.numpy(), bar, "kl_divergence_", measured)


def test_same_bits_and_input_kinds():
    from manner_amd.manifold import TSNE
    X, _ = R.cluster_points(5, 6, 50, 16)
    a = TSNE(perplexity=10.0, n_iter=60, n_iter_early_exag=30, random_state=3).fit_transform(dev(X), as_tensor=True)
    b = TSNE(perplexity=10.0, n_iter=60, n_iter_early_exag=30, random_state=3).fit_transform(dev(X), as_tensor=True)
    assert torch.equal(a, b)
    c = TSNE(perplexity=10.0, n_iter=60, n_iter_early_exag=30, random_state=3).fit_transform(X)                 # numpy in, float64 numpy out
    assert c.dtype == np.float64 and np.array_equal(c, a.double().cpu().numpy())
    d = TSNE(perplexity=10.0, n_iter=60, n_iter_early_exag=30, random_state=4).fit_transform(dev(X), as_tensor=True)
    assert not torch.equal(a, d)
    e = TSNE(perplexity=10.0, n_iter=5, init=a.cpu().numpy()).fit_transform(torch.from_numpy(X).to(torch.bfloat16))
    assert np.isfinite(e).all()
    with pytest.raises(ValueError, match="neighbours"):
        TSNE(perplexity=30).fit_transform(X[:90])


def test_a_larger_fit_is_finite():
    from manner_amd.manifold import TSNE
    X = np.random.default_rng(2).standard_normal((4099, 256)).astype(np.float32)
    t = TSNE(n_iter=50, random_state=0)
    Y = t.fit_transform(dev(X), as_tensor=True)
    assert Y.shape == (4099, 2) and torch.isfinite(Y).all() and np.isfinite(t.kl_divergence_)
