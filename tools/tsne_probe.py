"""What a t-SNE plot of the A-Module's embeddings costs -> profiles/tsne/probe.json.

``manner_amd.manifold.TSNE`` (perplexity 30, 1000 iterations) on N seeded 256-dimensional embeddings — 18 Gaussian clusters, unit noise —
at N = 4096, 16 384 and 65 238 (a MIND-small news pool), timed per phase: neighbours, affinities, the edge list's transpose, the 1000
iterations, KL; and the repulsion kernel alone, as pairs per second and as a share of the 157 TF f32 vector peak (13 FLOP per pair: two
subtractions, two fmas for the squared distance, the reciprocal, a product, two fmas and an add for the sums).  Beside it scikit-learn's
``TSNE(method="barnes_hut", n_jobs=16)`` on the CPU at the first two sizes: the CPU comparison available where this was run.  It is NOT
MulticoreTSNE, the package the reference calls, which was not installed.

The tool itself never touches the GPU: every size is one child process under its own ``timeout``, one at a time, and the first child
that fails ends the run.

    python tools/tsne_probe.py [--sizes 4096,16384,65238] [--cpu-sizes 4096,16384] [--out profiles/tsne/probe.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
F32_PEAK, FLOP_PER_PAIR, D, PERPLEXITY, N_ITER, SEED = 157e12, 13, 256, 30.0, 1000, 12


def embeddings(n: int) -> np.ndarray:
    rng = np.random.default_rng(SEED)
    centres = 4.0 * rng.standard_normal((18, D))
    return (centres[rng.integers(0, 18, n)] + rng.standard_normal((n, D))).astype(np.float32)


def gpu_leg(n: int) -> dict:
    import torch
    from manner_amd import hip
    from manner_amd.manifold import TSNE, edge_transpose
    dev = "cuda:0"

    def timed(fn, reps=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) / reps

    x = torch.from_numpy(embeddings(n)).to(dev)
    TSNE(n_iter=3, random_state=0).fit_transform(x[:512], as_tensor=True)              # code objects loaded, allocator warm
    k = int(3 * PERPLEXITY)
    xn = x - x.mean(0, keepdim=True)
    xn = (xn / xn.abs().max()).contiguous()
    rec = {"N": n, "k": k}
    hip.knn(xn[:1024].contiguous(), k)
    (idx, d2), rec["neighbours_s"] = timed(lambda: hip.knn(xn, k))
    (p, _), rec["affinities_s"] = timed(lambda: hip.tsne_affinities(d2, PERPLEXITY))
    edge_transpose(idx, p)
    _, rec["transpose_s"] = timed(lambda: edge_transpose(idx, p))
    t = TSNE(perplexity=PERPLEXITY, n_iter=N_ITER, random_state=0)
    y, rec["fit_transform_s"] = timed(lambda: t.fit_transform(x, as_tensor=True))
    rec["kl_divergence"] = t.kl_divergence_
    _, rec["kl_s"] = timed(lambda: hip.tsne_kl(y, idx, p))
    rec["iterations_s"] = rec["fit_transform_s"] - rec["neighbours_s"] - rec["affinities_s"] - rec["transpose_s"] - rec["kl_s"]
    rec["iterations_note"] = f"fit_transform less the other phases: {N_ITER} iterations, normalisation and the upload of the start included"
    part, zpart = hip.tsne_repulsion(y)
    _, rep = timed(lambda: hip.tsne_repulsion(y, part, zpart), reps=50)
    rec["repulsion_us"] = rep * 1e6
    rec["repulsion_pairs_per_s"] = n * n / rep
    rec["repulsion_f32_vector_peak_fraction"] = n * n * FLOP_PER_PAIR / rep / F32_PEAK
    rec["j_split"] = hip.tsne_j_split(n)
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def cpu_leg(n: int) -> dict:
    import sklearn
    from sklearn.manifold import TSNE
    x = embeddings(n)
    t0 = time.perf_counter()
    t = TSNE(n_components=2, perplexity=PERPLEXITY, early_exaggeration=12.0, learning_rate=200.0, max_iter=N_ITER, init="random", random_state=0,
             method="barnes_hut", angle=0.5, n_jobs=16)
    t.fit_transform(x)
    return {"N": n, "fit_transform_s": time.perf_counter() - t0, "kl_divergence": float(t.kl_divergence_), "n_iter": int(t.n_iter_),
            "what": f"scikit-learn {sklearn.__version__} TSNE(method='barnes_hut', angle=0.5, n_jobs=16), not MulticoreTSNE", "cpu_threads": 16}


def child(kind: str, n: int, limit: int) -> dict:
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", kind, "--n", str(n)]
    print(f"[tsne_probe] {kind} leg, N={n}", flush=True)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    while True:
        try:
            stdout, stderr = proc.communicate(timeout=60)
            break
        except subprocess.TimeoutExpired:
            print("[tsne_probe] ... still running", flush=True)
    r = subprocess.CompletedProcess(cmd, proc.returncode, stdout, stderr)
    if r.returncode:
        raise SystemExit(f"{kind} leg at N={n} ended with status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65238")
    ap.add_argument("--cpu-sizes", default="4096,16384")
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne", "probe.json"))
    ap.add_argument("--leg")
    ap.add_argument("--n", type=int)
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(gpu_leg(args.n) if args.leg == "gpu" else cpu_leg(args.n)))
        return
    out = {"D": D, "perplexity": PERPLEXITY, "n_iter": N_ITER, "flop_per_pair": FLOP_PER_PAIR, "f32_vector_peak": F32_PEAK,
           "method": "one run per size, one child process at a time; wall time around a device synchronise; the repulsion kernel as the mean of 50 "
                     "calls on the final embedding",
           "gpu": {}, "cpu_scikit_learn": {}}
    for n in [int(v) for v in args.sizes.split(",") if v]:
        out["gpu"][f"N={n}"] = child("gpu", n, args.limit)
    for n in [int(v) for v in args.cpu_sizes.split(",") if v]:
        out["cpu_scikit_learn"][f"N={n}"] = child("cpu", n, args.limit)
        if f"N={n}" in out["gpu"]:
            out["cpu_scikit_learn"][f"N={n}"]["over_gpu_fit_transform"] = (out["cpu_scikit_learn"][f"N={n}"]["fit_transform_s"]
                                                                            / out["gpu"][f"N={n}"]["fit_transform_s"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
