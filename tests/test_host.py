"""CPU-side checks: the C-ABI library exports what the header declares, the module mirror keeps the
reference's surface, host logic (sharding, synthetic generators) is deterministic, and the
multi-rank plumbing works under gloo with world_size 2.  No GPU compute here."""
import ctypes
import inspect
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from manner_amd import _lib
from manner_amd.config import PRESETS
from manner_amd.synth import segment_ids, shard_range, synth_impressions, synth_lengths, synth_news_tokens


def test_library_exports_every_header_symbol():
    lib = _lib.load()
    syms = _lib.header_symbols()
    assert len(syms) >= 18 and set(syms) == set(_lib.SIGNATURES)
    for s in syms:
        assert isinstance(getattr(lib, s), ctypes._CFuncPtr)
    assert lib.manner_hip_abi_version() == _lib.ABI_VERSION == 8
    assert lib.manner_hip_encoder_workspace_bytes(None, 1, 1, 0) == 0          # null handle: no crash


def test_library_argument_errors_without_gpu():
    lib = _lib.load()
    assert lib.manner_hip_dot(None, None, 2, 2, 4, 8, 1, 4, None, None) == 1    # MANNER_HIP_E_INVALID
    assert b"dot" in lib.manner_hip_last_error()
    assert lib.manner_hip_encode_cls(None, None, None, None, 1, 8, 0, None, None, 0, None) == 1
    assert lib.manner_hip_zscore_fuse(None, 0, 1, None, None, 0, None, None, None) == 0   # B == 0: nothing to do
    assert lib.manner_hip_to_dense(None, None, 0, 4, 1, None, None, None, None) == 0         # no slots: nothing to do
    assert lib.manner_hip_to_dense(None, None, 2, 4, 1, None, None, None, None) == 1


def test_module_surface_matches_reference_signatures(golden_dir):
    """Constructor arguments / forward parameters as in reference news_encoder.py:76-87,115,
    user_encoder.py:10,17, click_predictors.py:6,9-11, attention.py:7,12."""
    from manner_amd.models.components.attention import AdditiveAttention
    from manner_amd.models.components.click_predictors import DotProduct
    from manner_amd.models.components.news_encoder import MannerNewsEncoder, MannerTextEncoder
    from manner_amd.models.components.user_encoder import NAMLUserEncoder

    def params(f):
        return list(inspect.signature(f).parameters)[1:]

    assert params(MannerNewsEncoder.__init__) == [
        "plm_model", "frozen_layers", "dropout_probability", "use_entities", "entity_embeddings",
        "entity_embedding_dim", "num_attention_heads", "query_vector_dim", "text_embedding_dim"]
    assert params(MannerNewsEncoder.forward) == ["news"]
    assert params(MannerTextEncoder.__init__) == ["plm_model", "frozen_layers", "dropout_probability"]
    assert params(NAMLUserEncoder.__init__) == ["news_embedding_dim", "query_vector_dim"]
    assert params(NAMLUserEncoder.forward) == ["clicked_news_vector"]
    assert params(DotProduct.forward) == ["clicked_news_vector", "candidate_news_vector"]
    assert params(AdditiveAttention.__init__) == ["input_dim", "query_dim"]
    with open(os.path.join(golden_dir, "state_dict_keys.json")) as f:
        ref_keys = json.load(f)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = MannerNewsEncoder("tiny-bert", [0, 1], 0.2, False, None, 100, 10, 200, 128)
        ent = MannerNewsEncoder("tiny-bert", [0], 0.2, True, np.zeros((7, 100), np.float32), 100, 10, 200, 128)
    assert sorted(enc.state_dict()) == ref_keys["tiny-bert"]
    frozen = [n for n, p in enc.named_parameters() if not p.requires_grad]
    assert frozen and all("layer.0." in n or "layer.1." in n for n in frozen)          # news_encoder.py:24-27
    extra = sorted(set(ent.state_dict()) - set(enc.state_dict()))
    assert extra == sorted(["entity_encoder.pretrained_embedding.weight", "entity_encoder.multihead_attention.in_proj_weight",
                            "entity_encoder.multihead_attention.in_proj_bias", "entity_encoder.multihead_attention.out_proj.weight",
                            "entity_encoder.multihead_attention.out_proj.bias", "entity_encoder.additive_attention.query",
                            "entity_encoder.additive_attention.linear.weight", "entity_encoder.additive_attention.linear.bias",
                            "linear.weight", "linear.bias"])
    assert tuple(ent.linear.weight.shape) == (128, 228)
    assert sorted(NAMLUserEncoder(768, 200).state_dict()) == ref_keys["user_encoder"]
    # no CPU fallback, no training path
    enc.eval()
    with pytest.raises(RuntimeError, match="GPU"):
        enc({"text": {"input_ids": torch.zeros(1, 4, dtype=torch.long), "attention_mask": torch.ones(1, 4, dtype=torch.long)}})
    with pytest.raises(RuntimeError, match="GPU"):
        DotProduct()(torch.zeros(1, 1, 4), torch.zeros(1, 4, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        ent.eval().entity_encoder(torch.zeros(1, 2, dtype=torch.long))
    assert sorted(ent.state_dict()) == ref_keys["tiny-bert-entities"]


def test_local_hf_directory_loading(tmp_path):
    from safetensors.torch import save_file
    from manner_amd.models.components.news_encoder import HipPLM
    from manner_amd.weights import make_plm_weights
    cfg = PRESETS["tiny-roberta"]
    w = make_plm_weights(cfg, seed=3)
    (tmp_path / "config.json").write_text(json.dumps({
        "model_type": "roberta", "hidden_size": cfg.hidden, "num_hidden_layers": cfg.layers,
        "num_attention_heads": cfg.heads, "intermediate_size": cfg.intermediate, "vocab_size": cfg.vocab,
        "max_position_embeddings": cfg.max_pos, "type_vocab_size": cfg.type_vocab, "layer_norm_eps": cfg.ln_eps,
        "pad_token_id": cfg.pad_id, "hidden_act": "gelu"}))
    save_file({"roberta." + k: torch.from_numpy(v) for k, v in w.items()}, str(tmp_path / "model.safetensors"))
    m = HipPLM.from_pretrained(str(tmp_path))
    assert m.cfg == cfg
    sd = m.state_dict()
    assert all(np.array_equal(sd[k].numpy(), v) for k, v in w.items())


def test_synthetic_inputs_are_deterministic_and_well_formed():
    cfg = PRESETS["bert-base-uncased"]
    ids, mask = synth_news_tokens(500, cfg, seed=42, profile="title_abstract")
    ids2, _ = synth_news_tokens(500, cfg, seed=42, profile="title_abstract")
    assert np.array_equal(ids, ids2) and ids.dtype == np.int64
    lens = mask.sum(1)
    assert lens.min() >= 5 and lens.max() <= 96 and (ids[:, 0] == 101).all()
    assert (ids[np.arange(500), lens - 1] == 102).all() and (ids[mask == 0] == cfg.pad_id).all()
    assert (np.diff(mask, axis=1) <= 0).all()                                  # right-padded prefix masks
    ta = synth_lengths(5000, 1, profile="title_abstract")        # SURVEY.md §8d formula: a third saturate at 96
    assert 0.25 < (ta == 96).mean() < 0.5 and 65 < ta.mean() < 85 and 12 < synth_lengths(5000, 1).mean() < 20
    imp = synth_impressions(2000, 65238, seed=42)
    h, c = np.diff(imp["hist_off"]), np.diff(imp["cand_off"])
    assert h.min() >= 1 and h.max() <= 50 and c.min() >= 2 and c.max() <= 300
    assert imp["cand_idx"].max() < 65238 and imp["hist_idx"].dtype == np.int32
    pos = np.add.reduceat(imp["labels"], imp["cand_off"][:-1])
    assert (pos >= 1).all()
    assert np.array_equal(segment_ids(np.array([0, 2, 2, 5])), [0, 0, 2, 2, 2])


def _classes(*names):
    return "".join(f"\n\nclass {n}:\n    pass\n" for n in names)


def _imports(*items):
    return "".join(f"from {mod} import {name}" + (f" as {alias}" if alias else "") + "\n" for mod, name, alias in items)


def _write_reference_layout(root):
    """A stand-in for a checkout of the reference: its package layout and the module / class names that manner_amd.install() binds
    into or must leave alone, with trivial class bodies written here.  The two caller modules import their operators
    by path, as the reference's LightningModules do (cr_module.py:12-16, baselines/naml_plm_module.py:11-16); a components module
    imports AdditiveAttention from the attention module, as the reference's news_encoder.py does.  One import line of each caller
    reaches a module built on a third-party package (the loss on pytorch_metric_learning, a metric on torchmetrics), as in the
    reference, so that a package this interpreter lacks is seen to be skipped as third-party rather than as a missing `manner`."""
    comp = "manner.models.components"
    files = {
        "manner/__init__.py": "",
        "manner/utils/__init__.py": "",
        "manner/data/__init__.py": "",
        "manner/data/components/__init__.py": "",
        "manner/data/components/mind_batch.py": _classes("MINDRecBatch"),
        "manner/models/__init__.py": "",
        "manner/models/components/__init__.py": "",
        "manner/models/components/attention.py": _classes("AdditiveAttention", "PolyAttention", "TargetAwareAttention", "DenseAttention"),
        "manner/models/components/click_predictors.py": _classes("DotProduct"),
        "manner/models/components/losses.py": "import pytorch_metric_learning\n" + _classes("SupConLoss"),
        "manner/metrics/__init__.py": "",
        "manner/metrics/diversity.py": "import torchmetrics\n" + _classes("Diversity"),
        "manner/models/components/news_encoder.py": _imports((f"{comp}.attention", "AdditiveAttention", None)) + _classes(
            "MannerTextEncoder", "MannerEntityEncoder", "MannerNewsEncoder", "PLMTextEncoder", "NAMLNewsEncoder", "LSTURNewsEncoder",
            "MINERNewsEncoder", "CAUMNewsEncoder"),
        "manner/models/components/user_encoder.py": _imports((f"{comp}.attention", "AdditiveAttention", None),
                                                             (f"{comp}.attention", "DenseAttention", None)) + _classes(
            "NAMLUserEncoder", "NRMSUserEncoder", "LSTURUserEncoder", "CAUMUserEncoder", "MINSUserEncoder"),
        "manner/models/cr_module.py": _imports(("manner.data.components.mind_batch", "MINDRecBatch", None),
                                               (f"{comp}.click_predictors", "DotProduct", None),
                                               (f"{comp}.losses", "SupConLoss", None),
                                               (f"{comp}.news_encoder", "MannerNewsEncoder", None),
                                               (f"{comp}.user_encoder", "NAMLUserEncoder", "UserEncoder")) + _classes("CRModule"),
        "manner/models/baselines/naml_plm_module.py": _imports(("manner.data.components.mind_batch", "MINDRecBatch", None),
                                                               ("manner.metrics.diversity", "Diversity", None),
                                                               (f"{comp}.click_predictors", "DotProduct", None),
                                                               (f"{comp}.news_encoder", "NAMLNewsEncoder", "NewsEncoder"),
                                                               (f"{comp}.user_encoder", "NAMLUserEncoder", "UserEncoder")) + _classes("NAMLPLMModule"),
    }
    for rel, text in files.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    return root


_INSTALL_SCRIPT = r'''
import importlib.util, json, re, sys
import manner_amd
ref = sys.argv[1]
early = "--early" in sys.argv
def lines(path):                                 # the caller module's own `from manner.… import …` lines, read where they lie
    with open(path) as f:
        return [l.rstrip("\n") for l in f if l.startswith("from manner.")]
if early:                                        # a reference module imported BEFORE install(): its aliases must be rebound too
    sys.path.insert(0, ref)
    import manner.models.components.user_encoder as UE0
    from manner.models.components.user_encoder import NAMLUserEncoder as UserEncoderEarly
    import types
    fake = types.ModuleType("manner.models.fake_caller")          # stands for cr_module, which needs lightning to import
    fake.UserEncoder = UserEncoderEarly
    sys.modules["manner.models.fake_caller"] = fake
report = manner_amd.install(ref)
out = {"report": report, "skipped_third_party": []}
ns_cr, ns_naml = {}, {}
for ns, path in ((ns_cr, ref + "/manner/models/cr_module.py"), (ns_naml, ref + "/manner/models/baselines/naml_plm_module.py")):
    src = lines(path)
    assert len(src) >= 4, (path, src)
    for l in src:
        assert re.match(r"from manner\.[\w.]+ import ", l), l
        try:
            exec(l, ns)
        except ModuleNotFoundError as e:         # a third-party package this image lacks (pytorch_metric_learning, torchmetrics): not ours to stub
            assert (e.name or "").split(".")[0] != "manner", (l, e)
            out["skipped_third_party"].append([l, e.name])
cls = lambda c: c.__module__ + "." + c.__qualname__
out["cr_module"] = {k: cls(v) for k, v in ns_cr.items() if isinstance(v, type)}
out["naml_plm_module"] = {k: cls(v) for k, v in ns_naml.items() if isinstance(v, type)}
import manner, manner.models.components.news_encoder as NE, manner.models.components.attention as AT
out["manner_file"] = manner.__file__
out["utils_origin"] = importlib.util.find_spec("manner.utils").origin
out["data_origin"] = importlib.util.find_spec("manner.data").origin
out["cr_module_origin"] = importlib.util.find_spec("manner.models.cr_module").origin
out["kept"] = {n: cls(getattr(NE, n)) for n in ("NAMLNewsEncoder", "LSTURNewsEncoder", "MINERNewsEncoder", "CAUMNewsEncoder")}
out["kept"].update({n: cls(getattr(AT, n)) for n in ("PolyAttention", "TargetAwareAttention", "DenseAttention")})
out["naml_inner_additive"] = cls(NE.AdditiveAttention)           # what the reference's NAMLNewsEncoder instantiates
if early:
    out["early_alias"] = cls(sys.modules["manner.models.fake_caller"].UserEncoder)
ue = ns_cr["UserEncoder"](news_embedding_dim=768, query_vector_dim=200)          # the reference's call, cr_module.py:65-68
out["ue_keys"] = sorted(ue.state_dict())
manner_amd.uninstall()
out["after_uninstall"] = cls(NE.MannerNewsEncoder)
print("RESULT " + json.dumps(out))
'''


@pytest.mark.parametrize("early", [False, True])
def test_install_binds_the_mirror_into_the_real_reference_tree(early, tmp_path):
    """VERDICT r3 item 2 — the binding must COEXIST with the reference tree.  In a fresh interpreter with this repository and a
    reference-layout tree importable (``_write_reference_layout``: the reference's packages, modules and class names, nothing of
    its code), after ``manner_amd.install()`` the import lines of manner/models/cr_module.py give the mirror classes, those of
    baselines/naml_plm_module.py give the mirror ``DotProduct`` / ``NAMLUserEncoder`` and the REFERENCE's own ``NAMLNewsEncoder``;
    ``manner``, ``manner.utils``, ``manner.data``, ``manner.models.cr_module`` still resolve to the reference tree's files; the
    untouched encoders / attentions stay the reference's classes, and the reference's ``NAMLNewsEncoder`` keeps using the reference's
    ``AdditiveAttention``.  ``early``: a reference module imported before ``install()`` has its aliases rebound."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    reference = _write_reference_layout(str(tmp_path / "reference"))
    env = dict(os.environ, PYTHONPATH=root, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", _INSTALL_SCRIPT, reference] + (["--early"] if early else []), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    mir = "manner_amd.models.components."
    assert out["cr_module"]["DotProduct"] == mir + "click_predictors.DotProduct"
    assert out["cr_module"]["MannerNewsEncoder"] == mir + "news_encoder.MannerNewsEncoder"
    assert out["cr_module"]["UserEncoder"] == mir + "user_encoder.NAMLUserEncoder"
    assert out["cr_module"]["MINDRecBatch"].startswith("manner.data.components.mind_batch.")
    assert out["naml_plm_module"]["NewsEncoder"] == "manner.models.components.news_encoder.NAMLNewsEncoder"      # the reference's own
    assert out["naml_plm_module"]["DotProduct"] == mir + "click_predictors.DotProduct"
    assert out["naml_plm_module"]["UserEncoder"] == mir + "user_encoder.NAMLUserEncoder"
    for k in ("manner_file", "utils_origin", "data_origin", "cr_module_origin"):
        assert out[k].startswith(reference + "/manner/"), (k, out[k])
    assert all(v.startswith("manner.models.components.") for v in out["kept"].values()), out["kept"]
    assert out["naml_inner_additive"] == "manner.models.components.attention.AdditiveAttention"
    assert all(e[1].split(".")[0] in ("pytorch_metric_learning", "torchmetrics", "lightning", "torch_geometric") for e in out["skipped_third_party"]), out["skipped_third_party"]
    import importlib.util
    missing = sorted(m for m in ("pytorch_metric_learning", "torchmetrics") if importlib.util.find_spec(m) is None)
    assert sorted(e[1] for e in out["skipped_third_party"]) == missing, (out["skipped_third_party"], missing)
    assert ("SupConLoss" in out["cr_module"]) == ("pytorch_metric_learning" not in missing)
    assert out["ue_keys"] == ["additive_attention.linear.bias", "additive_attention.linear.weight", "additive_attention.query"]
    assert out["after_uninstall"] == "manner.models.components.news_encoder.MannerNewsEncoder"
    assert sorted(out["report"]["manner.models.components.news_encoder"]) == ["MannerEntityEncoder", "MannerNewsEncoder", "MannerTextEncoder", "PLMTextEncoder"]
    if early:
        assert out["early_alias"] == mir + "user_encoder.NAMLUserEncoder"
        assert out["report"]["manner.models.fake_caller"] == ["UserEncoder"]


def test_install_without_a_reference_checkout_says_so():
    """No ``manner`` package importable (the GPU box): install() names the problem instead of binding nothing silently; this
    repository itself ships no ``manner`` package any more (rounds 1-3's shim shadowed the reference tree)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert not os.path.exists(os.path.join(root, "manner"))
    r = subprocess.run([sys.executable, "-c", "import manner_amd\ntry:\n    manner_amd.install()\nexcept ModuleNotFoundError as e:\n    print('OK', e)"],
                       env=dict(os.environ, PYTHONPATH=root, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=600, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.startswith("OK manner_amd.install(): the reference package `manner` is not importable"), r.stdout + r.stderr[-2000:]


def test_mirror_constructors_follow_the_reference_call_sites():
    """The PLM baselines' encoders (reference baselines/nrms_plm_module.py:15-16) and the CR-Module's user encoder, constructed as the
    reference constructs them, expose the reference's state_dict keys."""
    from manner_amd.models.components.user_encoder import NAMLUserEncoder, NRMSUserEncoder
    nrms = NRMSUserEncoder(news_embedding_dim=768, num_attention_heads=16, query_vector_dim=200)
    assert sorted(nrms.state_dict()) == ["additive_attention.linear.bias", "additive_attention.linear.weight", "additive_attention.query",
                                         "multihead_attention.in_proj_bias", "multihead_attention.in_proj_weight",
                                         "multihead_attention.out_proj.bias", "multihead_attention.out_proj.weight"]
    ue = NAMLUserEncoder(news_embedding_dim=768, query_vector_dim=200)          # the reference's call, cr_module.py:65-68
    assert sorted(ue.state_dict()) == ["additive_attention.linear.bias", "additive_attention.linear.weight", "additive_attention.query"]


def test_shard_range_partitions():
    for n in (0, 1, 7, 73152):
        for w in (1, 2, 3, 8):
            parts = [shard_range(n, r, w) for r in range(w)]
            assert parts[0][0] == 0 and parts[-1][1] == n
            assert all(parts[i][1] == parts[i + 1][0] for i in range(w - 1))
            assert max(b - a for a, b in parts) - min(b - a for a, b in parts) <= 1


def _gloo_worker(rank, world, port, tmp):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
        import manner_oracle as O
        from manner_amd import distributed as D
        from manner_amd.weights import make_plm_weights
        cfg = PRESETS["tiny-bert"]
        w = make_plm_weights(cfg, seed=5, std=0.05)
        ids, mask = synth_news_tokens(37, cfg, seed=5, max_len=24)
        shards = D.balanced_news_shards(mask.sum(1), world, cfg.flops_per_news)
        lo, hi = shards[rank]
        local = O.encode_cls(ids[lo:hi], mask[lo:hi], w, cfg)               # stand-in for the HIP encoder on CPU
        table = D.all_gather_table(local, shards)                           # ragged (FLOP-balanced) shards: one gather
        full = O.encode_cls(ids, mask, w, cfg)
        assert table.shape == full.shape and torch.allclose(table, full, atol=1e-5)
        eq = D.equal_news_shards(37, world)                                 # equal rows (19 + 18): blocks land in place
        assert eq[0] == (0, 19) and eq[-1][1] == 37
        elo, ehi = eq[rank]
        padded = torch.zeros((19, full.shape[1]))
        padded[: ehi - elo] = full[elo:ehi]
        assert torch.equal(D.all_gather_table(padded, eq), full) and torch.equal(D.all_gather_table(full[elo:ehi].clone(), eq), full)
        imp = synth_impressions(11, 37, seed=5, max_hist=6, max_cand=9)
        a, b = D.impression_shard(11)
        ho, co = imp["hist_off"], imp["cand_off"]
        bh = O.offsets_to_batch((ho[a:b + 1] - ho[a]).tolist())
        bc = O.offsets_to_batch((co[a:b + 1] - co[a]).tolist())
        sc = O.ragged(O.cr_scores(table[imp["hist_idx"][ho[a]:ho[b]].astype(np.int64)], bh,
                                  table[imp["cand_idx"][co[a]:co[b]].astype(np.int64)], bc), bc)
        nd, per = O.ndcg_at_k(sc, torch.from_numpy(imp["labels"][co[a]:co[b]]), (co[a:b + 1] - co[a]).tolist(), 10)
        sums = D.allreduce_metric_sums(torch.tensor([per.sum().item(), float(b - a)], dtype=torch.float64))
        torch.save({"sums": sums, "range": (a, b), "scores": sc}, os.path.join(tmp, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_bench_starts_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no launcher around it (what the driver's command line looks like): the parent starts
    two fresh rank processes before anything touches a GPU, the ranks rendezvous (gloo here, RCCL on the node), run the
    barrier / MAX-over-ranks protocol and rank 0's ONE JSON line is the command's stdout; a failing rank fails the command.
    MANNER_BENCH_DRY keeps the rank processes off the GPU (there is none in this container)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MANNER_BENCH_DRY="1", MANNER_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["world_size_seen"] == 2 and j["launcher"] == "self" and j["steps"] == 3 and j["dry_run"] is True
    assert j["impressions_all_ranks"] == 512.0 and abs(j["max_rank_time_s"] - 0.002) < 1e-12      # SUM and MAX over both ranks
    assert j["table_exchange"] == {"default_exchange": "collective", "mesh_equals_collective_on_every_rank": True, "n_news": 161013, "pieces": 4}
    # the target machine's world size: 8 ranks, the staggered 7-peer mesh with 4 pieces of a 161 013-row table, store agreement
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    j8 = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert j8["n_gpus"] == 8 and j8["world_size_seen"] == 8 and j8["impressions_all_ranks"] == 2048.0 and abs(j8["max_rank_time_s"] - 0.008) < 1e-12
    assert j8["table_exchange"]["mesh_equals_collective_on_every_rank"] is True
    # a rank that cannot start fails the whole command (non-zero exit), it does not hang the others
    env["MANNER_DIST_BACKEND"] = "no-such-backend"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and not [l for l in r.stdout.splitlines() if l.startswith("{")]


def _mesh_worker(rank, world, port, n_news, pieces, exchange):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("MANNER_TABLE_EXCHANGE", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from manner_amd import distributed as D
        full = torch.arange(n_news * 6, dtype=torch.float32).reshape(n_news, 6) * 0.5 + 1.0
        g = D.MeshTableGather(n_news, 6, "cpu", pieces=pieces, exchange=exchange, timeout_s=120)
        assert g.exchange == (exchange or "collective")              # the collective is the default (round 4)
        assert g.exchange_why == ("requested" if exchange else "default")
        g.table.fill_(-7.0)
        seen = []
        for c in range(pieces):                              # "encode" piece c of the own shard straight into the table, then post it
            a, b = g.piece_rows(rank, c)
            g.local_out(c).copy_(full[a:b])
            seen.append((a, b))
            g.post(c)
        lo, hi = g.shards[rank]
        assert seen[0][0] == lo and seen[-1][1] == hi and all(x[1] == y[0] for x, y in zip(seen, seen[1:]))
        ptr, padded = g.table.data_ptr(), g._padded
        table = g.wait()
        assert torch.equal(table, full), (rank, (table - full).abs().max())
        # round 5: the exchange works IN PLACE — the table is the first N rows of the [W * mx, D] gather buffer, rank r's rows start at
        # r * mx, and wait() hands back that very storage (no staging clone, no 495 MB copy back)
        assert table.data_ptr() == ptr == padded.data_ptr() and g._padded is padded and padded.shape[0] == world * g.block_rows >= n_news
        assert all(lo == min(r * g.block_rows, n_news) for r, (lo, hi) in enumerate(g.shards))
        assert torch.equal(g.wait(), full)                   # idempotent: a second exchange re-sends the same blocks
        # same bytes as the single collective
        eq = D.equal_news_shards(n_news, world)
        assert torch.equal(D.all_gather_table(full[eq[rank][0]:eq[rank][1]].clone(), eq), table)
    finally:
        dist.destroy_process_group()


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("world,n_news,pieces,exchange", [(2, 37, 4, "mesh"), (3, 41, 3, "mesh"), (4, 6, 4, "mesh"), (3, 41, 3, None),
                                                          # the target machine's world size at the MIND-large pool size, which 8 does not divide
                                                          (8, 161013, 4, "mesh"), (8, 161013, 4, "collective")])
def test_mesh_table_gather_overlapped_pieces_gloo(world, n_news, pieces, exchange):
    """the direct full-mesh exchange of the news-embedding table in pieces (each piece posted while the next
    is being encoded) assembles exactly the table the single all-gather does — uneven last shard, pieces that are empty on
    some ranks (6 news over 4 ranks x 4 pieces) included; world 8 x 4 pieces x 161 013 news is the shape of the first real run
    (staggered rank +- k peer order over 7 peers).  The default exchange is the collective; both give the same table."""
    import torch.multiprocessing as mp
    mp.spawn(_mesh_worker, args=(world, _free_port(), n_news, pieces, exchange), nprocs=world, join=True)


def _stuck_worker(rank, world, port, out_dir):
    import time
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from manner_amd import distributed as D
    g = D.MeshTableGather(10, 4, "cpu", pieces=1, exchange="mesh", timeout_s=2.0)
    g.table.zero_()
    t0 = time.monotonic()
    if rank == 0:
        g.post(0)                                            # rank 1 never posts: a mismatched point-to-point group
        try:
            g.wait()
            res = "returned"
        except TimeoutError as e:
            res = "TimeoutError: " + str(e)[:60]
    else:
        time.sleep(6.0)
        res = "idle"
    with open(os.path.join(out_dir, f"r{rank}.txt"), "w") as f:
        f.write(f"{res}|{time.monotonic() - t0:.1f}")
    os._exit(0)                                              # the group is broken on purpose: no orderly shutdown to wait for


def test_mesh_wait_is_bounded(tmp_path):
    """a peer that never posts its half of the exchange makes wait() raise TimeoutError after `timeout_s`
    instead of hanging the process until somebody kills it."""
    import torch.multiprocessing as mp
    mp.spawn(_stuck_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    res, secs = (tmp_path / "r0.txt").read_text().split("|")
    assert res.startswith("TimeoutError"), res
    assert 1.5 <= float(secs) < 6.0, secs


def test_two_rank_table_allgather_and_impression_sharding_gloo(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert r0["range"][0] == 0 and r0["range"][1] == r1["range"][0] and r1["range"][1] == 11
    assert torch.equal(r0["sums"], r1["sums"]) and r0["sums"][1] == 11
    # the two ranks' shards reproduce the single-process result
    import manner_oracle as O
    from manner_amd.weights import make_plm_weights
    cfg = PRESETS["tiny-bert"]
    w = make_plm_weights(cfg, seed=5, std=0.05)
    ids, mask = synth_news_tokens(37, cfg, seed=5, max_len=24)
    imp = synth_impressions(11, 37, seed=5, max_hist=6, max_cand=9)
    ref = O.reference_faithful_scores(ids, mask, imp["hist_idx"].astype(np.int64), imp["hist_off"].tolist(),
                                      imp["cand_idx"].astype(np.int64), imp["cand_off"].tolist(), w, cfg)
    both = torch.cat([r0["scores"], r1["scores"]])
    assert torch.allclose(both, ref, atol=1e-4)
    nd, per = O.ndcg_at_k(ref, torch.from_numpy(imp["labels"]), imp["cand_off"].tolist(), 10)
    assert abs(r0["sums"][0].item() / 11 - nd) < 1e-6


def _toy_news(g, n, vocab=2000, lmax=96):
    news = {}
    for i in range(n):
        length = int(g.integers(3, lmax + 1))
        news[f"N{i + 1}"] = {"tokens": [101] + g.integers(1000, vocab, length - 2).tolist() + [102],
                             "entities": g.integers(1, 500, int(g.integers(0, 7))).tolist(),
                             "category": int(g.integers(0, 19)), "sentiment": int(g.integers(0, 4)),
                             "sentiment_score": float(np.float32(g.uniform(-1, 1)))}
    return news


def _toy_behaviors(g, news, n_rows, tmp_path, empty_history_every=5):
    """Writes the SAME impressions in both wire formats of the reference: raw behaviors.tsv and the cached frame."""
    import pandas as pd
    nids = list(news)
    raw, rows = [], []
    for i in range(n_rows):
        h = [] if (i % empty_history_every == 3) else [nids[j] for j in g.integers(0, len(nids), int(g.integers(1, 70)))]
        c = [nids[j] for j in g.integers(0, len(nids), int(g.integers(1, 40)))]
        lab = (g.random(len(c)) < 0.2).astype(int).tolist()
        uid = f"U{int(g.integers(0, 9))}"
        raw.append("\t".join([str(i + 1), uid, "11/15/2019 8:55:22 AM", " ".join(h), " ".join(f"{n}-{l}" for n, l in zip(c, lab))]))
        if h:
            rows.append({"user": {"U1": 1, "U2": 2, "U5": 3}.get(uid, 0), "history": h, "candidates": c, "labels": lab})
    raw_path, parsed_path = str(tmp_path / "behaviors.tsv"), str(tmp_path / "parsed_behaviors.tsv")
    with open(raw_path, "w") as f:
        f.write("\n".join(raw) + "\n")
    pd.DataFrame(rows).to_csv(parsed_path, sep="\t", index=False)          # reference file_utils.to_tsv
    return raw_path, parsed_path, rows


def test_parse_behaviors_both_wire_formats(tmp_path):
    """CSR parse == the reference's pandas read paths (restated in the oracle), raw and cached formats."""
    from manner_amd.data.components.mind_rec_dataset import parse_behaviors
    import manner_oracle as O
    g = np.random.Generator(np.random.PCG64(3))
    news = _toy_news(g, 50)
    nid2row = {n: i for i, n in enumerate(news)}
    raw_path, parsed_path, rows = _toy_behaviors(g, news, 40, tmp_path)
    uid2index = {"U1": 1, "U2": 2, "U5": 3}
    for path in (raw_path, parsed_path):
        frame = O.load_behaviors_frame(path, uid2index)
        got = parse_behaviors(path, nid2row, 50, uid2index)
        assert len(got) == len(frame) == len(rows)
        assert got.users.tolist() == frame["user"].tolist()
        for i in range(len(frame)):
            h = [nid2row[n] for n in frame["history"][i][:50]]
            c = [nid2row[n] for n in frame["candidates"][i]]
            assert got.hist_rows[got.hist_off[i]:got.hist_off[i + 1]].tolist() == h
            assert got.cand_rows[got.cand_off[i]:got.cand_off[i + 1]].tolist() == c
            assert got.labels[got.cand_off[i]:got.cand_off[i + 1]].tolist() == [float(x) for x in frame["labels"][i]]
    with pytest.raises(KeyError):
        parse_behaviors(["user\thistory\tcandidates\tlabels", "1\t['N1']\t['N999999']\t[1]"], nid2row, 50)


def test_impression_blocks_are_prefix_stable():
    """bench.py draws one block per (rank, step): asking for more steps must not change the earlier batches."""
    from manner_amd.synth import synth_impression_blocks
    a = synth_impression_blocks([0, 1], 64, 5000, seed=42)
    b = synth_impression_blocks([0, 1, 2, 1_000_000], 64, 5000, seed=42)
    n_h, n_c = int(a["hist_off"][-1]), int(a["cand_off"][-1])
    assert np.array_equal(a["hist_idx"], b["hist_idx"][:n_h]) and np.array_equal(a["cand_idx"], b["cand_idx"][:n_c])
    assert np.array_equal(a["hist_off"], b["hist_off"][:129]) and np.array_equal(a["labels"], b["labels"][:n_c])
    assert b["hist_off"].shape == (257,) and b["cand_off"][-1] == b["cand_idx"].shape[0] == b["labels"].shape[0]
    for i in range(256):                                       # >= 1 positive per impression survives the concatenation
        assert b["labels"][b["cand_off"][i]:b["cand_off"][i + 1]].max() == 1.0


def test_distilbert_directory_loading_and_keys(tmp_path, golden_dir):
    """distilbert-base-multilingual-cased is the PLM of the reference's multilingual configs: a local
    DistilBertModel directory loads under its own parameter names, and those are the reference checkpoint's keys."""
    from safetensors.torch import save_file
    from manner_amd.models.components.news_encoder import HipPLM, MannerTextEncoder
    from manner_amd.weights import canonical_weights, make_plm_weights
    cfg = PRESETS["tiny-distilbert"]
    w = make_plm_weights(cfg, seed=45, std=0.05)
    (tmp_path / "config.json").write_text(json.dumps({
        "model_type": "distilbert", "dim": cfg.hidden, "n_layers": cfg.layers, "n_heads": cfg.heads,
        "hidden_dim": cfg.intermediate, "vocab_size": cfg.vocab, "max_position_embeddings": cfg.max_pos,
        "pad_token_id": 0, "activation": "gelu"}))
    save_file({"distilbert." + k: torch.from_numpy(v) for k, v in w.items()}, str(tmp_path / "model.safetensors"))
    m = HipPLM.from_pretrained(str(tmp_path))
    assert m.cfg == cfg
    sd = m.state_dict()
    assert set(sd) == set(w) and all(np.array_equal(sd[k].numpy(), v) for k, v in w.items())
    with open(os.path.join(golden_dir, "state_dict_keys.json")) as f:
        ref_keys = json.load(f)["tiny-distilbert"]
    enc = MannerTextEncoder(str(tmp_path), frozen_layers=[0], dropout_probability=0.2)
    assert sorted("text_encoder." + k for k in enc.state_dict()) == ref_keys
    frozen = [n for n, p in enc.plm_model.named_parameters() if not p.requires_grad]
    assert frozen and all("layer.0." in n for n in frozen)                      # news_encoder.py:24-27 name test
    c = canonical_weights(cfg, w)
    assert "encoder.layer.1.attention.self.query.weight" in c and c["embeddings.token_type_embeddings.weight"].shape == (1, cfg.hidden)


def test_training_buffer_sizes_follow_the_documented_rule():
    """manner_hip_train_workspace_bytes / _saved_bytes (host arithmetic, no GPU) against the sizing rule written out here —
    what each training kernel may touch (csrc/train.hip plan_work / plan_saved): a change of the rule has to be made twice."""
    import ctypes as C
    from manner_amd import _lib
    from manner_amd.train import _cfg_c
    lib = _lib.load()

    def up(v):
        return (v + 255) // 256 * 256

    for preset, n, mb in (("tiny-bert", 9, 256), ("tiny-bert", 300, 7424), ("bert-base-uncased", 928, 15616), ("roberta-large", 64, 2048)):
        cfg = PRESETS[preset]
        h, i, heads, layers = cfg.hidden, cfg.intermediate, cfg.heads, cfg.layers
        wide = max(i, 3 * h)
        rows = max(mb, wide) + 64 * 64
        work = [4 * wide * rows] * 2 + [4 * 3 * h * h, 4 * 3 * h, 4 * wide, 4 * mb * wide,                       # a16, b16, wcat, bcat, zero, tmp
                                        4 * mb * h, 4 * mb * h, 4 * mb * wide, 4 * mb * 3 * h, 4 * mb * heads,   # dx, dr, dbig, dqkv, dsum
                                        4 * wide * max(i, h), 4 * 2 * 1024 * wide,                               # dw, part (2 x LN_BWD_BLOCKS rows)
                                        2 * mb * h, 2 * mb * h, 2 * mb * wide,                                   # h16a, h16b, big16
                                        4 * (1024 * 65536 + wide * max(i, h)), 4 * 16]                           # dwp, dims
        want_w = 0
        for b in work:
            want_w = up(want_w) + b
        assert int(lib.manner_hip_train_workspace_bytes(C.byref(_cfg_c(cfg)), mb)) == want_w + 256, preset
        per_layer = [4 * mb * h, 4 * mb * 3 * h, 4 * mb * h, 4 * mb * h, 4 * mb * h, 4 * mb * i, 4 * mb * i, 4 * mb * h,   # x_in qkv ctx r1 h1 inter g r2
                     8 * mb, 8 * mb, 8 * mb * heads]                                                                         # st1 st2 ml
        parts = [4 * n, 4 * (n + 1), 16, 4 * mb * h, 8 * mb] + per_layer * layers                                          # lens cu m_total esum st0
        want_s = 0
        for b in parts:
            want_s = up(want_s) + b
        assert int(lib.manner_hip_train_saved_bytes(C.byref(_cfg_c(cfg)), n, mb, 0)) == want_s + 256, preset


def test_every_environment_switch_is_documented():
    """The library's A/B switches are read with getenv() in csrc/ and os.environ in the package: each one has a line in DESIGN.md
    (the table of switches, section 7) or INTEGRATION.md, so that a measured alternative cannot hide in the build."""
    import re
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = set()
    for root, _, files in os.walk(os.path.join(ROOT, "manner_amd")):
        if "lib" in root.split(os.sep) or "__pycache__" in root:
            continue
        for f in files:
            if f.endswith((".hip", ".h", ".py")):
                with open(os.path.join(root, f), encoding="utf-8") as fh:
                    txt = fh.read()
                names |= set(re.findall(r'getenv\("(MANNER_[A-Z0-9_]+)"', txt))
                names |= set(re.findall(r'environ(?:\.get)?[\(\[]\s*"(MANNER_[A-Z0-9_]+)"', txt))
    assert len(names) >= 10
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as fh:
        docs = fh.read()
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        docs += fh.read()
    missing = sorted(n for n in names if n not in docs)
    assert not missing, missing


def test_impression_blocks_are_balanced_by_occurrences():
    """SURVEY §8e phase C: ranks score contiguous impression blocks of equal sum(h_i + c_i).  Every impression lands in exactly one
    block, blocks are ordered, and the heaviest rank is within one impression's work of the mean; degenerate inputs (fewer
    impressions than ranks, none at all) give empty blocks, never an index outside the list."""
    from manner_amd.distributed import balanced_impression_shards
    from manner_amd.synth import synth_impressions
    imp = synth_impressions(5000, 3000, seed=4)
    ho, co = imp["hist_off"], imp["cand_off"]
    per = np.diff(ho) + np.diff(co)
    for w in (1, 2, 3, 8, 64):
        sh = balanced_impression_shards(ho, co, w)
        assert len(sh) == w and sh[0][0] == 0 and sh[-1][1] == 5000
        assert all(sh[r][1] == sh[r + 1][0] for r in range(w - 1)) and all(a <= b for a, b in sh)
        work = np.array([per[a:b].sum() for a, b in sh])
        assert work.sum() == per.sum() and work.max() <= per.sum() / w + per.max()
    one = balanced_impression_shards(np.array([0, 3]), np.array([0, 5]), 4)          # fewer impressions than ranks: empty blocks, no bad index
    assert len(one) == 4 and sum(b - a for a, b in one) == 1 and one[0][0] == 0 and one[-1][1] == 1 and all(x[1] == y[0] for x, y in zip(one, one[1:]))
    assert balanced_impression_shards(np.array([0]), np.array([0]), 2) == [(0, 0), (0, 0)]
    # the cut goes to the CLOSER side of the mark — cumulative work [3, 11, 23] at world 2 splits 11 / 12, not 23 / 0
    assert balanced_impression_shards(np.array([0, 1, 5, 10]), np.array([0, 2, 6, 13]), 2) == [(0, 2), (2, 3)]
    # one heavy impression among light ones: with at least as many impressions as ranks nobody is left without work
    for w in (2, 3, 4):
        sh = balanced_impression_shards(np.array([0, 1, 2, 3, 4]), np.array([0, 300, 302, 304, 306]), w)
        assert all(b > a for a, b in sh) and sh[0][0] == 0 and sh[-1][1] == 4 and all(x[1] == y[0] for x, y in zip(sh, sh[1:])), (w, sh)


def _load_bench():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("manner_bench", os.path.join(root, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_final_line_is_compact_strict_json(tmp_path, capsys):
    """The driver parses bench.py's LAST stdout line (round 4's 26 KB line left its record with `parsed: null`): with EVERY leg present
    and bloated — long prose, whole sweeps, NaN / Infinity — the line stays below 8 KB, is strict JSON, carries the contract keys and
    the three objects, and the complete record goes to the side file instead."""
    bench = _load_bench()
    prose = "a very long explanation of what this figure means and how it was obtained; " * 12
    sweep = [{"impression": i, "hip_top11": [[j, 1000 + j, 700.0 + j / 7, 700.0 + j / 9, 700.0 + j / 11] for j in range(11)],
              "oracle_top11": [[j, 1000 + j, 700.0 + j / 7, 700.0 + j / 9, 700.0 + j / 11] for j in range(11)]} for i in range(3)]
    modes = {m: {"score_max_abs_err": 1e-4 / 3, "top10_identical": 63, "top10_identical_frac": 63 / 64, "top10_valid_order_of_oracle_scores_frac": 1.0,
                 "ndcg10_delta": float("nan") if m == "bf16" else 6.4e-9, "differing_impressions": sweep} for m in ("fp32", "f16x3", "f16", "bf16")}
    agree = {"impressions": 73152, "top10_identical_frac": 0.7456, "ndcg10_delta": 6.5e-5, "score_max_abs_err": 0.0318, "what": prose}
    result = {
        "metric": "candidate news encoded+scored/sec", "value": 43848.81234567, "unit": "candidates/s", "n_gpus": 1, "steps": 20, "warmup": 5,
        "ms_per_step": 209.6031234, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
        "config": {"workload": prose, "baseline_config": 1, "modules": 1, "ensemble_weights": [], "impressions_per_step_per_gpu": 256,
                   "length_profile": "title_abstract", "seeded_weights_std": 0.02, "parallelism": "dp1 (impressions sharded, no collective)"},
        "news_encoded_per_s": 75341.2, "tokens_per_s": 5.6e6, "encoder_tflops": 912.2, "encoder_mfma_frac": 0.3649, "ndcg10_last_step": 0.26,
        "world_size_seen": 1, "dist_backend": None, "launcher": None,
        "bf16_mode": {"what": prose, "value": 45157.3, "ms_per_step": 203.5, "news_encoded_per_s": 77589.5, "encoder_mfma_frac": 0.3758},
        "parity_grade_mode": {"dtype": "f16x3", "value": 14391.0, "unit": "candidates/s", "ms_per_step": 638.7, "news_encoded_per_s": 24732.9, "steps": 20, "tag": prose},
        "pcie_inclusive_rank0": {"what": prose, "candidates_per_s": 43392.4, "ms_per_step": 211.8, "h2d_MB_per_step": 12.0},
        "kernels": {f"kernel_{i}": {"ms_total": 1.0 + i, "launches": 100, "avg_us": 10.0 + i, "flops_per_launch": 3e11, "tflops": 900.0} for i in range(12)},
        "roofline": {"kernel": "gemm_ffn1 (gemm_tn_x16_kernel)", "bound": "mfma", "achieved": 915.854, "peak": 2500.0, "unit": "TFLOP/s", "frac": 0.366342,
                     "traffic": 986080000.0, "traffic_source": prose, "mfma_only_ceiling_tflops": 2040.0, "avg_launch_us": 328.149, "flops_per_launch": 3.00536e11},
        "collate": {"ms_per_batch": 0.21, "note": prose, "large_batch": {"ms": 1.0}},
        "table_mode": {"what": prose, "candidates_per_s": 3.0e6, "news_encoded_per_s": 75813.7, "scorer_pairs_per_s": 2.2e9, "scorer_kernel_ms_rank0": 0.71,
                       "allgather_ms": 0.03, "allgather_exchange": "collective", "allgather_what": prose, "scorer_note": prose, "encode_ms": 860.5, "score_ms": 1.18,
                       "ndcg10": 0.2744, "allgather_GBps_per_rank": float("inf"), "allgather_frac_of_xgmi": 0.31, "scorer_f16_table": {"what": prose, "plain": agree, "centred": agree},
                       "mesh_exchange": {"exchange": "mesh", "tables_identical": True, "standalone_ms": 1.1, "standalone_frac_of_xgmi": 0.4, "what": prose}},
        "parity_at_scale": {"what": prose, "hf_init_weights_std0.02": {"f16": agree, "bf16": agree, "f16x3": agree}, "spread_weights_std0.05": {"f16": agree, "bf16": agree}},
        "parity_mode": {"dtype": "fp32", "news_encoded_per_s": 9898.9, "what": prose, "f16x3_news_encoded_per_s": 24732.9},
        "small_ops": {k: {"ms": 0.4, "GB/s": 1500.0, "frac_of_8TBps": 0.19, "bound": prose, "shape": {"B": 4096}} for k in ("additive_pool", "dot", "zscore_fuse", "to_dense")},
        "cpu_baseline": {"value": 28.51, "unit": "candidates/s", "cores": 16, "kind": "port", "cpu_model": "AMD EPYC 9575F 64-Core Processor",
                         "cores_how": prose, "runs_s": [7.75, 8.16, 8.58], "sample": prose},
        "parity": {**modes, "against_float64_oracle": {"impressions": 4, "oracle_f32_max_abs_err": 2.3e-4, "hip_fp32_max_abs_err": 1.3e-4, "hip_f16x3_max_abs_err": 1.2e-4, "what": prose},
                   "score_abs_scale": 776.8, "impressions": 64, "candidates": 2088, "repeated_candidates_in_sample": 0, "oracle_s": 63.6, "what": prose},
        "train_mode": {"what": prose, **{v: {"ms_per_step": 14.6, "peak_GB": 23.1, "frac_of_mfma_peak": 0.168, "step_ms_each": [14.6] * 5}
                                         for v in ("reference_default_embeddings_trainable", "embeddings_frozen_cached_prefix", "embeddings_frozen_prefix_cache_across_steps")}},
        "dropin": {"what": prose, **{f"B{b}_{m}": {"ms_per_step": 8.65, "enqueue_ms": 3.0} for b in (8, 64) for m in ("eval", "train")},
                   "B8_eval_embedding_cache": {"what": prose, "note": prose, "cold_whole_sweep": {"ms_per_step": 14.2, "hit_rate": 0.81}}},
    }

    class Args:
        precision = "f16"
        full_json = str(tmp_path / "bench_full.json")

    bench.emit(result, Args)
    out = capsys.readouterr().out.splitlines()
    line = out[-1]
    assert len(out) == 1 and len(line.encode()) < 8192, len(line)

    def reject(name):
        raise ValueError(name)

    j = json.loads(line, parse_constant=reject)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["value"] == pytest.approx(43848.8, rel=1e-5) and j["vs_baseline"] is None and j["config"]["baseline_config"] == 1
    assert set(j["roofline"]) >= {"kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "flops_per_launch", "encoder_mfma_frac"}
    assert j["roofline"]["frac"] == pytest.approx(0.366342) and j["roofline"]["encoder_mfma_frac"] == {"f16": 0.3649, "bf16": 0.3758}
    assert set(j["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "cpu_model", "runs_s", "sample"} and j["cpu_baseline"]["kind"] == "port"
    pg = j["config"]["parity_grade"]
    assert pg["dtype"] == "f16x3" and pg["candidates_per_s"] == 14391.0 and pg["top10_identical"] == 63 and pg["of_impressions"] == 64 and pg["timed_steps"] == 20
    assert j["config"]["parity_vs_oracle"]["bf16"].get("ndcg10_delta") is None            # NaN never reaches the line
    assert all(len(v) <= 120 for v in (j["config"]["workload"], j["cpu_baseline"]["sample"], j["roofline"]["traffic_source"]))
    assert j["legs"]["dropin_ms_per_step"]["B8_eval"] == 8.65 and j["legs"]["train_ms_per_step"]["reference_default_embeddings_trainable"] == 14.6
    # the complete record is in the side file, prose and sweeps included
    full = json.loads((tmp_path / "bench_full.json").read_text())
    assert full["parity"]["fp32"]["differing_impressions"][0]["hip_top11"][0][1] == 1000 and full["dropin"]["what"] == prose
    assert j["full_record"].endswith("bench_full.json")
    # a result that is far too large for the optional parts still yields a line below the limit with the three objects
    result["kernels"] = {f"kernel_with_a_long_name_{i:04d}": {"avg_us": float(i)} for i in range(600)}
    line2 = bench.compact_line(result)
    j2 = json.loads(line2, parse_constant=reject)
    assert len(line2.encode()) < 8192 and {"config", "roofline", "cpu_baseline"} <= set(j2) and "kernel_avg_us" not in j2.get("legs", {})


def test_bench_plain_run_and_output_dump(tmp_path, monkeypatch):
    """bench.py parses `--full` (the side legs) off by default, refuses `--full-json` without it, validates `--steps`, and
    `--dump-outputs` writes the last step's scores / top-10 / nDCG and a seeded [CLS]-table row sample as float32 /
    float64 .npy files below 64 MB — the same files for the same step."""
    bench = _load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path)])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == str(tmp_path) and a.full_json == os.path.join(bench.ROOT, "bench_full.json")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full-json", str(tmp_path / "r.json")])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    g = torch.Generator().manual_seed(5)
    n_news, n_cand, nb = 5000, 300, 12
    last = (torch.randn(n_cand, generator=g), torch.randint(-1, 40, (nb, 10), generator=g, dtype=torch.int32), torch.rand(nb, generator=g))
    tables = [torch.randn(n_news + 17, 16, generator=g) for _ in range(2)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), last, tables, n_news)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["ndcg10.npy", "scores.npy", "table_m0.npy", "table_m1.npy", "table_rows.npy", "top10.npy"]
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    rows = np.load(tmp_path / "a" / "table_rows.npy").astype(np.int64)
    assert len(rows) == bench.DUMP_TABLE_ROWS and (np.diff(rows) > 0).all() and rows.max() < n_news
    assert np.array_equal(np.load(tmp_path / "a" / "table_m1.npy"), tables[1][torch.from_numpy(rows)].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "top10.npy"), last[1].numpy().astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), last[0].numpy())


def test_segment_offsets_without_a_host_read():
    """hotpath.segment_offsets: sorted segment ids -> CSR offsets by a search over the sorted ids (round 5: torch.bincount, used before,
    reads the maximum back to the host — a full device wait in the middle of a training step).  Same offsets as the counting form,
    with empty segments in front, in the middle and at the end."""
    from manner_amd.hotpath import segment_offsets
    g = np.random.default_rng(3)
    for counts in ([3, 0, 2, 5, 0, 0], [0, 0, 4], [1], [7, 1, 1, 0], list(g.integers(0, 9, 40))):
        ids = torch.from_numpy(np.repeat(np.arange(len(counts)), counts).astype(np.int64))
        off = segment_offsets(ids, len(counts))
        assert off.dtype == torch.int64 and off.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert segment_offsets(torch.zeros(0, dtype=torch.int64), 3).tolist() == [0, 0, 0, 0]


def test_cached_parameter_view_equals_named_parameters():
    """MannerTextEncoder._plm_params (round 5): dict(named_parameters()) from a cached view of the module tree — 36 us instead of 250 us
    per forward for bert-base, paid with the GPU idle behind the reference's own host synchronisations.  The view re-checks the identity
    of every submodule and Parameter it remembers on every call: a Parameter replaced by assignment, a submodule added, replaced or
    removed all give exactly what named_parameters() gives (names, order, objects); it is not pickled."""
    import pickle
    from manner_amd.models.components.news_encoder import MannerTextEncoder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = MannerTextEncoder("tiny-bert", frozen_layers=[0], dropout_probability=0.2)

    def same():
        a, b = m._plm_params(), dict(m.plm_model.named_parameters())
        assert list(a) == list(b) and all(a[k] is b[k] for k in a)
        return a
    first_name, first_p = next(iter(same().items()))
    assert m._plm_params() is m._plm_params()                       # the cached dict itself while nothing changed
    holder = m.plm_model
    for q in first_name.split(".")[:-1]:
        holder = getattr(holder, q)
    setattr(holder, first_name.split(".")[-1], torch.nn.Parameter(torch.zeros_like(first_p)))
    assert same()[first_name] is not first_p
    holder.extra = torch.nn.Linear(2, 2)
    assert any(k.endswith("extra.weight") for k in same())
    old = holder.extra.weight
    holder.extra = torch.nn.Linear(2, 2)
    assert all(v is not old for v in same().values())
    del holder.extra
    assert not any("extra" in k for k in same())
    assert "_param_view" not in pickle.loads(pickle.dumps(m)).__dict__
    # state(): the (storage address, version counter) fingerprint _encoder() keys its packed weight copies on — in the order of the
    # view, equal to the per-parameter tuple it replaces, and changed by an in-place write as well as by a swap of .data
    params = m._plm_params()
    view = m.__dict__["_param_view"]
    ptrs, vers = view.state()
    assert ptrs == [p.data_ptr() for p in params.values()] and vers == [p._version for p in params.values()]
    assert view.state() == (ptrs, vers)
    some = list(params.values())[3]
    with torch.no_grad():
        some.add_(1.0)
    assert view.state()[1] != vers and view.state()[0] == ptrs
    vers = view.state()[1]
    some.data = some.data.clone()
    assert view.state()[0] != ptrs


def test_precision_resolution_follows_the_autocast_state(monkeypatch):
    """VERDICT r5 item 1 (host logic; the arithmetic itself is tests/test_gpu_boundary.py): the mirror's mode is the caller's
    autocast state — `trainer.precision` of the reference (configs/trainer/default.yaml:12) — unless a mode is pinned."""
    import warnings
    from manner_amd.models.components import news_encoder as ne
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tiny = ne.MannerTextEncoder("tiny-bert", [], 0.2)
        base = ne.MannerTextEncoder.__new__(ne.MannerTextEncoder)        # resolution needs the config only: no 110 M-parameter init
        torch.nn.Module.__init__(base)
        base.plm_model = type("P", (), {"cfg": PRESETS["bert-base-uncased"]})()
    assert ne.autocast_mode() is None                                     # no autocast region here
    for state, ev, tr in ((None, "f16x3", "fp32"), ("f16", "f16", "f16"), ("bf16", "bf16", "bf16")):
        monkeypatch.setattr(ne, "autocast_mode", lambda s=state: s)
        assert (base.resolved_precision(), base.resolved_train_precision()) == (ev, tr)
    monkeypatch.setattr(ne, "autocast_mode", lambda: None)
    assert tiny.resolved_precision() == "fp32"                            # hidden 128: the split-operand GEMMs tile K in 256s
    base.precision, base.train_precision = "bf16", "f16"                  # pinned modes win
    monkeypatch.setattr(ne, "autocast_mode", lambda: "f16")
    assert (base.resolved_precision(), base.resolved_train_precision()) == ("bf16", "f16")


def test_generated_gemm_asm_is_in_sync_with_its_generator(tmp_path):
    """manner_amd/csrc/gemm_w{8,4}_asm.inc are GENERATED (tools/gen_gemm_w.py: the hand-scheduled K-loops of the 16-bit GEMM) and committed:
    regenerating them must reproduce the committed files byte for byte, so that nobody edits the output instead of the schedule."""
    import importlib.util
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(ROOT, "manner_amd", "csrc")
    committed = {n: open(os.path.join(csrc, n), encoding="utf-8").read() for n in ("gemm_w8_asm.inc", "gemm_w4_asm.inc", "gemm_p4_asm.inc")}
    real_join = os.path.join

    def redirect(*parts):                                   # the generators write next to the sources: send their outputs to tmp_path
        path = real_join(*parts)
        return str(tmp_path / os.path.basename(path)) if path.endswith("_asm.inc") else path
    for script in ("gen_gemm_w.py", "gen_gemm_p4.py"):      # (gen_gemm_p4.py: the lab-only paired 4-wave form)
        spec = importlib.util.spec_from_file_location(script[:-3], os.path.join(ROOT, "tools", script))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        gen.os.path.join = redirect
        try:
            gen.main()
        finally:
            gen.os.path.join = real_join
    for n, text in committed.items():
        assert (tmp_path / n).read_text(encoding="utf-8") == text, f"{n} differs from what its generator in tools/ writes"
    # and the schedule's own invariants: every K-step body has 64 matrix instructions per wave (8-wave form), the LDS-queue simulation ran
    assert committed["gemm_w8_asm.inc"].count('MFMA "') == 2 * 4 * 64 and committed["gemm_w4_asm.inc"].count('MFMA "') == 4 * 128


def test_every_kernel_name_is_defined_in_one_file():
    """Kernel traces (rocprofv3, profiles/*/kernel_trace.json) identify a kernel by its name: two kernels under one name in different
    files of csrc/ make such a trace ambiguous, and are usually two copies of one kernel.  A shared kernel lives in one file (a header
    for a template that each caller instantiates)."""
    import glob
    import re
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(ROOT, "manner_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert len(files) >= 20
    where = {}
    for path in files:
        text = open(path, encoding="utf-8").read()
        for name in re.findall(r"__global__\b[^;{]*?\bvoid\s+(\w+)\s*\(", text, flags=re.S):
            where.setdefault(name, set()).add(os.path.basename(path))
    assert len(where) >= 100, "the pattern no longer finds the kernels"
    shared = {name: sorted(fs) for name, fs in where.items() if len(fs) > 1}
    assert not shared, f"kernel names defined in more than one file: {shared}"
