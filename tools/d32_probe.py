#!/usr/bin/env python3
"""What a head_dim-32 PLM (the MiniLM shape) costs in the inference engine -> profiles/d32/probe.json.

``"minilm-l12-h384"`` with seeded weights on 65 238 synthetic titles of bench.py's title-length distribution
(``synth_news_tokens(profile="title")``, the pool of tools/sentiment_probe.py).  Three legs, each a child process of its own under a
``timeout`` (the parent never opens the GPU; a leg that fails ends the run):

  encode     ``encode_cls`` in f16 / bf16 / fp32 over the whole pool: news/s, the median of ``--rounds`` alternating rounds (wall time
             around a device synchronise)
  attention  the short-row 16-bit attention kernel alone, head_dim 32 (``"minilm-l12-h384"``) beside head_dim 64
             (``"bert-base-uncased"``) in the same process: ``encode_hidden`` through every layer under the encoder's per-launch
             profiling (HIP events around each launch, one stream) on the first ``--attn-news`` titles; µs per launch and achieved
             TB/s over the bytes the kernel has to move (Q, K, V in, the context rows out: 4 H elements per token)
  hf         if ``transformers`` is importable: HF ``BertModel`` of the same config and dtype on the GPU under ``torch.no_grad()``, in
             batches of ``--hf-batch`` titles padded to the batch's longest — the comparison a user would otherwise run

    python tools/d32_probe.py [--rounds 5] [--news 65238] [--legs encode,attention,hf] [--out profiles/d32/probe.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
PRESET, PRESET_64 = "minilm-l12-h384", "bert-base-uncased"
LEG_TIMEOUT_S = {"encode": 300, "attention": 240, "hf": 300}


def _pool(news, cfg):
    import torch
    from manner_amd.synth import synth_news_tokens
    ids_np, mask_np = synth_news_tokens(news, cfg, seed=42, max_len=96, profile="title")
    return ids_np, mask_np, torch.from_numpy(ids_np).to(DEV), torch.from_numpy(mask_np).to(DEV)


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def encode_leg(a):
    from manner_amd import hip
    from manner_amd.config import PRESETS
    from manner_amd.weights import make_plm_weights
    cfg = PRESETS[PRESET]
    ids_np, mask_np, ids, mask = _pool(a.news, cfg)
    hl = mask_np.sum(1)
    modes = ("f16", "bf16", "fp32")
    enc = hip.HipEncoder(cfg, make_plm_weights(cfg, seed=7, std=0.02), precisions=modes, device=DEV)
    fns = {m: (lambda m=m: enc.encode_cls(ids, mask, precision=m, host_lengths=hl)) for m in modes}
    for f in fns.values():
        f()
    enc.status()
    got = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m, f in fns.items():
            got[m].append(_timed(f))
    enc.status()
    enc.close()
    import torch
    out = {"device": torch.cuda.get_device_name(0), "news": a.news, "tokens": int(mask_np.sum()), "padded_length": int(ids_np.shape[1])}
    for m, v in got.items():
        out[m] = {"call_s": round(statistics.median(v), 4), "call_min_max_s": [round(min(v), 4), round(max(v), 4)],
                  "news_per_s": round(a.news / statistics.median(v), 1)}
    return out


def attention_leg(a):
    import torch
    from manner_amd import hip
    from manner_amd.config import PRESETS
    from manner_amd.weights import make_plm_weights
    out = {"news": a.attn_news, "method": "encode_hidden through every layer under per-launch HIP events, one stream; bytes = 4 H x 2 per token and layer"}
    for preset in (PRESET, PRESET_64):
        cfg = PRESETS[preset]
        ids_np, mask_np, ids, mask = _pool(a.attn_news, cfg)
        hl, tokens = mask_np.sum(1), int(mask_np.sum())
        rec = {"head_dim": cfg.head_dim, "hidden": cfg.hidden, "tokens": tokens}
        for m in ("f16", "bf16"):
            enc = hip.HipEncoder(cfg, make_plm_weights(cfg, seed=7, std=0.02), precisions=(m,), device=DEV)
            run = lambda: enc.encode_hidden(ids, mask, cfg.layers, precision=m, out_dtype=torch.bfloat16, host_lengths=hl)   # noqa: E731
            run()
            enc.status()
            per = []
            for _ in range(a.rounds):
                enc.profile(True)
                enc.profile_read()
                run()
                ms, launches = enc.profile_read()["attention"]
                enc.profile(False)
                per.append((ms, launches))
            enc.close()
            ms, launches = statistics.median(p[0] for p in per), per[0][1]
            nbytes = tokens * 4 * cfg.hidden * 2 * cfg.layers
            rec[m] = {"launches": int(launches), "attention_ms": round(ms, 4), "us_per_launch": round(1e3 * ms / launches, 2),
                      "tokens_per_launch": round(tokens * cfg.layers / launches, 1), "tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3)}
            torch.cuda.empty_cache()
        out[preset] = rec
    return out


def hf_leg(a):
    try:
        import transformers
        from transformers import BertConfig, BertModel
    except ImportError as e:
        return {"skipped": str(e)}
    import torch
    from manner_amd.config import PRESETS
    cfg = PRESETS[PRESET]
    ids_np, mask_np, ids, mask = _pool(a.news, cfg)
    torch.manual_seed(7)
    model = BertModel(BertConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                                 intermediate_size=cfg.intermediate, max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab,
                                 layer_norm_eps=cfg.ln_eps, pad_token_id=cfg.pad_id, hidden_act="gelu"), add_pooling_layer=False).eval()
    lens = torch.from_numpy(mask_np.sum(1))
    out = {"transformers": transformers.__version__, "torch": torch.__version__, "batch": a.hf_batch, "news": a.news,
           "method": "BertModel(...).to(dtype) under torch.no_grad(), batches padded to their longest title, last_hidden_state[:, 0]"}
    for name, dt in (("f16", torch.float16), ("bf16", torch.bfloat16), ("fp32", torch.float32)):
        m = model.to(device=DEV, dtype=dt)

        def run():
            with torch.no_grad():
                for i in range(0, a.news, a.hf_batch):
                    lp = int(lens[i:i + a.hf_batch].max())
                    m(input_ids=ids[i:i + a.hf_batch, :lp], attention_mask=mask[i:i + a.hf_batch, :lp]).last_hidden_state[:, 0].float()
        run()
        v = [_timed(run) for _ in range(max(3, a.rounds // 2))]
        out[name] = {"call_s": round(statistics.median(v), 4), "call_min_max_s": [round(min(v), 4), round(max(v), 4)],
                     "news_per_s": round(a.news / statistics.median(v), 1)}
    return out


LEGS = {"encode": encode_leg, "attention": attention_leg, "hf": hf_leg}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--news", type=int, default=65238)
    ap.add_argument("--attn-news", type=int, default=16384)
    ap.add_argument("--hf-batch", type=int, default=1024)
    ap.add_argument("--legs", default="encode,attention,hf")
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process and print its JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "d32", "probe.json"))
    a = ap.parse_args()
    if a.leg:
        print("D32_PROBE_LEG " + json.dumps(LEGS[a.leg](a)), flush=True)
        return 0
    out = {"preset": PRESET, "rounds": a.rounds,
           "method": "every leg a child process under its own timeout; medians of alternating rounds, wall time around a device synchronise"}
    rc = 0
    for leg in a.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--rounds", str(a.rounds), "--news", str(a.news),
               "--attn-news", str(a.attn_news), "--hf-batch", str(a.hf_batch)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT_S[leg])
        except subprocess.TimeoutExpired:
            out[leg] = {"failed": f"no result within {LEG_TIMEOUT_S[leg]} s"}
            rc = 1
            break                                   # nothing more is started on the GPU after a leg that hung
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("D32_PROBE_LEG ")]
        if r.returncode or not line:
            out[leg] = {"failed": f"exit status {r.returncode}", "stderr_tail": r.stderr[-2000:]}
            rc = 1
            break                                   # ... or after one that failed
        out[leg] = json.loads(line[-1][len("D32_PROBE_LEG "):])
    if "encode" in out and "hf" in out and "f16" in out["encode"] and "f16" in out["hf"]:
        out["engine_over_hf"] = {m: round(out["encode"][m]["news_per_s"] / out["hf"][m]["news_per_s"], 3) for m in ("f16", "bf16", "fp32")}
    if "attention" in out and PRESET in out["attention"]:
        at = out["attention"]
        out["attention_d32_over_d64_tb_per_s"] = {m: round(at[PRESET][m]["tb_per_s"] / at[PRESET_64][m]["tb_per_s"], 3) for m in ("f16", "bf16")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))
    return rc


if __name__ == "__main__":
    sys.exit(main())
