"""``TSNE`` with MulticoreTSNE's call surface, on the HIP kernels of csrc/tsne.hip.

The reference's ``AModule.on_validation_epoch_end`` / ``on_test_epoch_end`` (manner/models/a_module.py:150-173, 191-212) embed all
validation or test embeddings with ``MulticoreTSNE(n_jobs=8).fit_transform`` on the CPU.  This class is the published method restated
(van der Maaten's implementation, whose update rule that package keeps): inputs centred and scaled by their largest entry,
``int(3 * perplexity)`` exact nearest neighbours, per-row binary search for the perplexity, the symmetrised P kept as a directed edge list
and its transpose, 1000 iterations of gains / momentum with early exaggeration, KL at the end.

What differs from the package, on purpose: the repulsive forces are EXACT (an all-pairs loop), so ``angle`` is accepted and ignored;
and the result is not the package's bits — nor is any run of the package reproducible from outside it, since it draws its own random
numbers.  ``random_state`` here seeds ``numpy.random.RandomState``; two fits with one seed return the same bits.

There is no CPU fallback: without the library or a GPU this raises, like everything else in ``manner_amd``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip

__all__ = ["TSNE"]


def edge_transpose(idx: torch.Tensor, p: torch.Tensor):
    """The directed edge list [N, k] grouped by destination, sources ascending: (in_off int64 [N + 1], in_src int32 [N k], in_p [N k]).
    A stable sort of the destinations and a scan — plumbing, torch."""
    n, k = idx.shape
    dst = idx.reshape(-1).long()
    valid = (dst >= 0) & (dst < n)                       # a row of NaN distances leaves -1: such an edge keeps its place and carries nothing
    dst = torch.where(valid, dst, torch.zeros_like(dst))
    order = torch.sort(dst, stable=True).indices
    in_src = torch.div(order, k, rounding_mode="floor").to(torch.int32)
    in_p = (p.reshape(-1) * valid)[order].contiguous()
    counts = torch.zeros(n, dtype=torch.int64, device=idx.device).scatter_add_(0, dst, torch.ones_like(dst))
    in_off = torch.zeros(n + 1, dtype=torch.int64, device=idx.device)
    in_off[1:] = torch.cumsum(counts, 0)
    return in_off, in_src.contiguous(), in_p


class TSNE:
    """t-SNE into two dimensions.  Parameters and defaults are MulticoreTSNE's; ``angle`` (the Barnes-Hut opening angle) is accepted and
    IGNORED — the forces are exact — and so are ``n_jobs``, ``verbose``, ``method``, ``cheat_metric``, ``n_iter_without_progress`` and
    ``min_grad_norm`` (all ``n_iter`` iterations run, as in the package).  ``init``: ``'random'`` (1e-4 x a standard normal drawn from
    ``RandomState(random_state)`` on the host) or an ``[N, 2]`` array.  Numpy and CPU inputs are taken to the current GPU; a GPU tensor
    stays where it is.

    Attributes after ``fit_transform``: ``embedding_`` (what it returned), ``kl_divergence_`` (sum P log(P / Q), float), ``n_iter_``."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate=200.0, n_iter=1000, n_iter_early_exag=250,
                 n_iter_without_progress=30, min_grad_norm=1e-07, metric="euclidean", init="random", verbose=0, random_state=None,
                 method="barnes_hut", angle=0.5, n_jobs=1, cheat_metric=True):
        if n_components != 2:
            raise ValueError("TSNE: n_components must be 2")
        if isinstance(init, str) and init != "random":
            raise ValueError("TSNE: init must be 'random' or an [N, 2] array")
        if metric != "euclidean":
            raise ValueError("TSNE: metric must be 'euclidean'")
        self.n_components, self.perplexity, self.early_exaggeration = n_components, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.n_iter, self.n_iter_early_exag = float(learning_rate), int(n_iter), int(n_iter_early_exag)
        self.n_iter_without_progress, self.min_grad_norm, self.metric, self.init = n_iter_without_progress, min_grad_norm, metric, init
        self.verbose, self.random_state, self.method, self.angle, self.n_jobs, self.cheat_metric = verbose, random_state, method, angle, n_jobs, cheat_metric
        self.embedding_, self.kl_divergence_, self.n_iter_ = None, None, None

    def _to_device(self, X) -> torch.Tensor:
        if isinstance(X, torch.Tensor):
            if not X.is_floating_point():
                raise TypeError("TSNE: X must be a float array")
            t = X.detach()
            if not t.is_cuda:
                t = t.to(self._device())
        else:
            a = np.asarray(X)
            if a.dtype.kind != "f":
                a = a.astype(np.float64)
            if a.dtype == np.float16:
                a = a.astype(np.float32)
            t = torch.from_numpy(np.ascontiguousarray(a)).to(self._device())
        if t.dim() != 2:
            raise ValueError("TSNE: X must be [N, D]")
        return t

    def _device(self) -> torch.device:
        if not torch.cuda.is_available():
            raise RuntimeError("manner_amd.manifold.TSNE runs on HIP kernels: there is no GPU and no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())

    def fit(self, X, _y=None):
        self.fit_transform(X)
        return self

    def fit_transform(self, X, _y=None, as_tensor: bool = False):
        """X [N, D]: a numpy array or a CPU / GPU torch tensor of any float dtype (a GPU tensor is not copied to the host).  Returns the
        embedding as float64 numpy [N, 2], as the package does; ``as_tensor=True`` returns the f32 device tensor."""
        x = self._to_device(X)
        n = x.shape[0]
        k = int(3 * self.perplexity)
        if n - 1 < k:
            raise ValueError(f"TSNE: perplexity {self.perplexity} needs {k} neighbours, {n} rows have {n - 1}")
        dev = x.device
        with torch.cuda.device(dev):
            # 1. centre per column, scale by the largest absolute entry (in the input's own precision, then f32 for the kernels)
            x = x.double() if x.dtype == torch.float64 else x.float()
            x = x - x.mean(0, keepdim=True)
            x = (x / x.abs().max()).float().contiguous()
            # 2.-4. neighbours, conditional affinities, the edge list's transpose
            out_idx, d2 = hip.knn(x, k)
            out_p, _beta = hip.tsne_affinities(d2, self.perplexity)
            in_off, in_src, in_p = edge_transpose(out_idx, out_p)
            # 5. iterations: nothing is read back inside the loop
            if isinstance(self.init, str):
                y0 = 1e-4 * np.random.RandomState(self.random_state).randn(n, 2)
            else:
                y0 = self.init.detach().cpu().numpy() if isinstance(self.init, torch.Tensor) else np.asarray(self.init)
                if y0.shape != (n, 2):
                    raise ValueError("TSNE: init must be [N, 2]")
            y = torch.from_numpy(np.ascontiguousarray(y0, dtype=np.float32)).to(dev)
            y_next = torch.empty_like(y)
            u, gains = torch.zeros_like(y), torch.ones_like(y)
            part, zpart = hip.tsne_repulsion(y)
            ypart = torch.empty((2 * -(-n // hip.TSNE_STEP_ROWS),), dtype=torch.float64, device=dev)
            for it in range(self.n_iter):
                early = it < self.n_iter_early_exag
                if it:
                    hip.tsne_repulsion(y, part, zpart)
                hip.tsne_step(y, part, zpart, out_idx, out_p, in_off, in_src, in_p, u, gains, y_next, ypart,
                              self.early_exaggeration if early else 1.0, 0.5 if early else 0.8, self.learning_rate)
                y, y_next = y_next, y
            # 6. KL of the final embedding; the one synchronising read
            kl = hip.tsne_kl(y, out_idx, out_p)
            self.kl_divergence_ = float(kl.item())
        self.n_iter_ = self.n_iter
        self.embedding_ = y if as_tensor else y.double().cpu().numpy()
        return self.embedding_
