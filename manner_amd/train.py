"""Training path of MannerTextEncoder as a ``torch.autograd.Function`` over ``manner_hip_train_*``.

The reference trains through ``MannerTextEncoder.forward`` in ``train()`` mode (news_encoder.py:29-37) and
``loss.backward()`` (Lightning drives ``CRModule.training_step``, cr_module.py:140-171).  ``encode_train`` is that
forward on the HIP engine — HF dropouts included — and registers a backward that fills ``.grad`` of exactly the
parameters with ``requires_grad=True``; optimiser, scheduler and Lightning stay the reference's.

Frozen prefix: the reference freezes the *parameters* of ``frozen_layers`` but leaves the embeddings trainable, so its
backward runs through all layers (news_encoder.py:24-27).  That is what happens here when an embedding tensor requires
grad.  When every tensor below the first trainable layer ``f`` is frozen, the prefix is run once by the inference
engine (``encode_hidden``, eval arithmetic: no dropout in the frozen layers — the one documented deviation from the
reference, which keeps dropout active there) and training starts from ``hidden_states[f]``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from manner_amd import _lib, hip
from manner_amd.config import EncoderConfig
from manner_amd.weights import canonical_weights

Tensor = torch.Tensor
_TRAIN_PRECISIONS = ("fp32", "f16", "bf16")


def _cfg_c(cfg: EncoderConfig) -> _lib.EncoderConfigC:
    return _lib.EncoderConfigC(cfg.arch, cfg.hidden, cfg.layers, cfg.heads, cfg.intermediate, cfg.vocab, cfg.max_pos,
                               cfg.type_vocab, cfg.pad_id, cfg.ln_eps)


def _table(tensors: Sequence[Optional[Tensor]]):
    return (C.c_void_p * len(tensors))(*[(t.data_ptr() if t is not None else None) for t in tensors])


def dropout_mask(seed: int, site: int, p: float, n: int, device) -> Tensor:
    """The keep-bits (uint8 [n]) the training kernels use at one dropout site — for tests that feed an oracle the same mask."""
    out = torch.empty(n, dtype=torch.uint8, device=device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().manner_hip_dropout_mask(C.c_uint64(seed), C.c_uint32(site), C.c_float(p), n, hip._ptr(out), hip._stream()))
    return out


class _WeightCopyCache:
    """16-bit copies of FROZEN PLM weights kept across training steps (manner_hip_train_weight_cache, round 4).

    The 16-bit training modes convert every weight matrix to the GEMM operand type — and transpose it for the data-gradient GEMMs —
    on every call; for the layers the reference freezes (``frozen_layers: [0..7]``, news_encoder.py:24-27) the result never changes:
    8 layers x (3 conversions + the Q|K|V pack + 4 transposes) = 0.5 ms of a 15.5 ms step.  An entry belongs to the parameter OBJECTS
    it was made from (round 5): it holds weak references to them, is used only while every reference still yields the very
    tensor passed in, and is dropped by a finalizer the moment one of them is collected — a new model whose fresh parameters land on
    the same allocator addresses with the same version counters can never see a stale copy, and the copies of a model that is gone do
    not stay pinned in HBM.  Within the owners' lifetime an entry is validated by storage (address, size) and the torch version
    counters (an optimizer step, ``load_state_dict`` or any in-place write through the parameter bumps them); a write through
    ``p.data`` bypasses the counter — call ``invalidate_weight_cache()`` after one.  A parameter that requires grad is never cached.
    The copies themselves are made by the library on first use — the same kernels as without the cache, so the cached path is
    bit-identical — this class only owns the buffers and the validity flags."""

    def __init__(self):
        self._entries = {}

    def clear(self):
        self._entries.clear()

    def __len__(self):
        return len(self._entries)

    def _drop(self, key):
        self._entries.pop(key, None)

    def arrays(self, cfg, params, needs_grad, prec, start, dev):
        import weakref
        n = len(params)
        h, i_ = cfg.hidden, cfg.intermediate
        esz = 2
        slots = (C.c_void_p * (2 * n))()
        valid = (C.c_int32 * (2 * n))()
        touched = []
        base0 = _lib.W_EMB_COUNT
        for l in range(start, cfg.layers):
            b = base0 + l * _lib.WL_COUNT
            groups = (("qkv", (0, 2, 4), 0, 3 * h * h * esz, True), ("qkv_bias", (1, 3, 5), 1, 3 * h * 4, False),
                      ("ao", (6,), 6, h * h * esz, True), ("ff1", (10,), 10, i_ * h * esz, True), ("ff2", (12,), 12, h * i_ * esz, True))
            for what, deps, at, nbytes, both in groups:
                if any(needs_grad[b + d] for d in deps):
                    continue
                owners = [params[b + d] for d in deps]
                key = (str(dev), prec, l, what) + tuple(id(o) for o in owners)
                ent = self._entries.get(key)
                vers = tuple(int(o._version) for o in owners)
                ptrs = tuple((o.data_ptr(), o.numel()) for o in owners)
                if ent is not None and not all(r() is o for r, o in zip(ent["owners"], owners)):
                    ent = None                       # an id() re-used by another object: never this entry's tensors
                if ent is None or ent["ptrs"] != ptrs:
                    ent = {"ptrs": ptrs, "vers": None, "owners": [weakref.ref(o) for o in owners],
                           "bufs": [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2 if both else 1)], "valid": [0, 0]}
                    self._entries[key] = ent
                    for o in owners:                 # the entry dies with the first of its owners
                        weakref.finalize(o, self._drop, key)
                if ent["vers"] != vers:
                    ent["valid"] = [0, 0]
                    ent["vers"] = vers
                for c in range(2 if both else 1):
                    slots[2 * (b + at) + c] = ent["bufs"][c].data_ptr()
                    valid[2 * (b + at) + c] = ent["valid"][c]
                touched.append((ent, 2 * (b + at), 2 if both else 1))
        return slots, valid, touched

    @staticmethod
    def commit(valid, touched):
        for ent, s0, cnt in touched:
            for c in range(cnt):
                ent["valid"][c] = int(valid[s0 + c])


_WCACHE = _WeightCopyCache()


def invalidate_weight_cache() -> None:
    """Forget every cached 16-bit copy of frozen weights (they are rebuilt on the next training call).  Needed only after a write that
    torch's version counter cannot see (``p.data.copy_(...)``, a raw pointer write); optimiser steps, ``load_state_dict`` and in-place
    ops through the parameter are detected by themselves."""
    _WCACHE.clear()


def _register_weight_cache(lib, cfg, params, needs_grad, opts, start, dev):
    """Hands the frozen weights' cached 16-bit copies to the next train_forward / _backward call (16-bit modes; MANNER_TRAIN_WEIGHT_CACHE=0
    switches it off for A/B).  Returns what ``_WeightCopyCache.commit`` needs after the call."""
    import os
    if opts["precision"] == "fp32" or os.environ.get("MANNER_TRAIN_WEIGHT_CACHE", "1") == "0":
        return None
    slots, valid, touched = _WCACHE.arrays(cfg, params, needs_grad, opts["precision"], start, dev)
    if not touched:
        return None
    _lib.check(lib.manner_hip_train_weight_cache(slots, valid, len(slots)))
    return slots, valid, touched


class _EncodeTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids: Tensor, mask: Tensor, prefix: Optional[Tensor], opts: dict, *params: Tensor):
        cfg: EncoderConfig = opts["cfg"]
        lib = _lib.load()
        n, lp = ids.shape
        m_bound = (n * lp + 255) // 256 * 256 if opts.get("m_bound") is None else int(opts["m_bound"])
        start = int(opts["start_layer"])
        prec = _lib.PRECISIONS[opts["precision"]]
        cc = _cfg_c(cfg)
        dev = ids.device
        with torch.cuda.device(dev):
            saved = torch.empty(int(lib.manner_hip_train_saved_bytes_for(C.byref(cc), n, m_bound, start, prec)), dtype=torch.uint8, device=dev)
            ws = torch.empty(int(lib.manner_hip_train_workspace_bytes(C.byref(cc), m_bound)), dtype=torch.uint8, device=dev)
            out = torch.empty((n, cfg.hidden), dtype=torch.float32, device=dev)
            weights = [p.detach() for p in params]
            status = hip.device_status(dev)
            status.poll()                     # flags of earlier calls (a token_bound below the mask's count, a bad id) raise here
            needs = [bool(p.requires_grad) for p in params]
            wc = _register_weight_cache(lib, cfg, params, needs, opts, start, dev)
            _lib.check(lib.manner_hip_train_forward(
                C.byref(cc), _table(weights), len(weights), hip._ptr(ids), hip._ptr(mask), n, lp, m_bound, prec, start,
                hip._ptr(prefix), C.c_float(opts["p_hidden"]), C.c_float(opts["p_attn"]), C.c_float(opts["p_out"]),
                C.c_uint64(opts["seed"]), hip._ptr(out), hip._ptr(saved), saved.numel(), hip._ptr(ws), ws.numel(),
                hip._ptr(status.word), hip._stream()))
            ctx.layout = int(lib.manner_hip_train_layout_last())    # ABI v8: the saved buffer's layout travels with the autograd ctx
            if wc is not None:
                _WeightCopyCache.commit(wc[1], wc[2])
            status.arm()                      # snapshot behind an event: examined, without blocking, by the next poll
        ctx.opts, ctx.m_bound, ctx.prec, ctx.start = opts, m_bound, prec, start
        ctx.needs = needs
        ctx.saved_buf, ctx.ws = saved, ws
        ctx.save_for_backward(ids, *params)
        ctx.prefix_grad = prefix is not None and prefix.requires_grad
        ctx.prefix_shape = None if prefix is None else tuple(prefix.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        ids, *params = ctx.saved_tensors
        opts, cfg = ctx.opts, ctx.opts["cfg"]
        lib = _lib.load()
        n, lp = ids.shape
        dev = ids.device
        need = ctx.needs_input_grad[4:]
        grads: List[Optional[Tensor]] = [torch.empty_like(p) if r else None for p, r in zip(params, need)]
        gprefix = torch.empty(ctx.prefix_shape, dtype=torch.float32, device=dev) if ctx.prefix_grad else None
        cc = _cfg_c(cfg)
        with torch.cuda.device(dev):
            g = grad_out.to(torch.float32).contiguous()
            wc = _register_weight_cache(lib, cfg, params, ctx.needs, opts, ctx.start, dev)
            _lib.check(lib.manner_hip_train_layout_next(ctx.layout))
            _lib.check(lib.manner_hip_train_backward(
                C.byref(cc), _table([p.detach() for p in params]), len(params), hip._ptr(ids), n, lp, ctx.m_bound, ctx.prec,
                ctx.start, C.c_float(opts["p_hidden"]), C.c_float(opts["p_attn"]), C.c_float(opts["p_out"]),
                C.c_uint64(opts["seed"]), hip._ptr(g), hip._ptr(ctx.saved_buf), ctx.saved_buf.numel(), _table(grads),
                hip._ptr(gprefix), hip._ptr(ctx.ws), ctx.ws.numel(), hip._stream()))
            if wc is not None:
                _WeightCopyCache.commit(wc[1], wc[2])
        return (None, None, gprefix, None, *grads)       # the activation buffer lives with ctx: backward(retain_graph=True) may run again


def first_trainable_layer(cfg: EncoderConfig, params: Dict[str, Tensor]) -> int:
    """Index of the layer training starts at when everything below it is frozen — 0 when an embedding table trains (the reference's
    default: the gradient then crosses every layer), else the first layer with a trainable tensor, capped at the last layer."""
    canon = canonical_weights(cfg, params)
    table = [canon[name] for name in hip.weight_table_order(cfg)]
    if any(t.requires_grad for t in table[:_lib.W_EMB_COUNT]):
        return 0
    for l in range(cfg.layers):
        if any(t.requires_grad for t in table[_lib.W_EMB_COUNT + l * _lib.WL_COUNT:_lib.W_EMB_COUNT + (l + 1) * _lib.WL_COUNT]):
            return min(l, cfg.layers - 1)
    return cfg.layers - 1


def encode_train(cfg: EncoderConfig, params: Dict[str, Tensor], ids: Tensor, mask: Tensor, *, precision: str = "f16",
                 p_hidden: float = 0.1, p_attn: float = 0.1, p_out: float = 0.2, seed: int = 0,
                 prefix_engine: Optional[hip.HipEncoder] = None, prefix_hidden: Optional[Tensor] = None,
                 start_layer: Optional[int] = None, token_bound: Optional[int] = None, max_len: int = _lib.MAX_LEN) -> Tensor:
    """[N, Lp] ids / mask -> [N, H] dropout([CLS]) with autograd into ``params`` (HF-named parameter dict).

    ``max_len``: the longest padded batch this call accepts (``Lp > max_len`` raises ``RuntimeError``).  The default is the
    128-token limit of the short-row kernels; up to ``_lib.MAX_LEN_TRAIN`` (512) opts in to news of 129..512 tokens, which run the
    long-row attention kernels (``saved`` grows per token, so such batches hold fewer news).  Every row must also fit the model's
    position table.

    ``start_layer`` / ``prefix_hidden``: explicit cached prefix; by default the prefix is used automatically when no
    tensor below the first trainable layer requires grad and a ``prefix_engine`` (inference HipEncoder over the same
    weights) is given.  ``token_bound``: a host-known upper bound of the real tokens (e.g. the collate's sum of lengths) —
    activation buffers are sized for it instead of N * Lp; a mask with more tokens is truncated at the bound (never indexed past
    it) and raises ``RuntimeError`` through the device status word: at the next training / scoring call (non-blocking poll) or
    at ``hip.check_status`` (blocking)."""
    if precision not in _TRAIN_PRECISIONS:
        raise ValueError(f"training precision {precision!r}: one of {_TRAIN_PRECISIONS}")
    if not 1 <= int(max_len) <= _lib.MAX_LEN_TRAIN:
        raise ValueError(f"max_len={max_len}: training takes padded batches of 1..{_lib.MAX_LEN_TRAIN} tokens")
    ids, mask = hip._dev(ids, torch.int64, "input_ids").contiguous(), hip._dev(mask, torch.int64, "attention_mask").contiguous()
    if ids.dim() != 2 or ids.shape != mask.shape:
        raise ValueError(f"input_ids {tuple(ids.shape)} / attention_mask {tuple(mask.shape)} must be equal 2-D")
    if ids.shape[1] > int(max_len):
        raise RuntimeError(f"train: padded_len={ids.shape[1]} beyond max_len={int(max_len)} (padded_len <= {int(max_len)}); news of up "
                           f"to {_lib.MAX_LEN_TRAIN} tokens train with max_len={_lib.MAX_LEN_TRAIN} "
                           f"(MannerTextEncoder.train_max_length, MANNER_HIP_TRAIN_MAX_LEN)")
    canon = canonical_weights(cfg, params)
    table = [canon[name] for name in hip.weight_table_order(cfg)]
    for name, t in zip(hip.weight_table_order(cfg), table):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise TypeError(f"{name}: training needs contiguous float32 GPU parameters")
    if start_layer is None:
        start_layer = 0
        emb_frozen = not any(t.requires_grad for t in table[:_lib.W_EMB_COUNT])
        if emb_frozen and prefix_engine is not None:
            first = cfg.layers
            for l in range(cfg.layers):
                if any(t.requires_grad for t in table[_lib.W_EMB_COUNT + l * _lib.WL_COUNT:_lib.W_EMB_COUNT + (l + 1) * _lib.WL_COUNT]):
                    first = l
                    break
            start_layer = min(first, cfg.layers - 1)
    if start_layer > 0 and prefix_hidden is None:
        if prefix_engine is None:
            raise ValueError("start_layer > 0 needs prefix_hidden or a prefix_engine")
        with torch.no_grad():
            prefix_hidden = prefix_engine.encode_hidden(ids, mask, start_layer, precision=precision if precision != "fp32" else "fp32")
    if prefix_hidden is not None:
        prefix_hidden = hip._dev(prefix_hidden, torch.float32, "prefix_hidden").contiguous()
        if tuple(prefix_hidden.shape) != (ids.shape[0], ids.shape[1], cfg.hidden):
            raise ValueError("prefix_hidden must be [N, Lp, H]")
    opts = dict(cfg=cfg, precision=precision, p_hidden=float(p_hidden), p_attn=float(p_attn), p_out=float(p_out),
                seed=int(seed) & (2 ** 64 - 1), start_layer=int(start_layer),
                m_bound=None if token_bound is None else (max(int(token_bound), 1) + 255) // 256 * 256)
    return _EncodeTrain.apply(ids, mask, prefix_hidden, opts, *table)


class _EncodeFullTrain(torch.autograd.Function):
    """HF last_hidden_state [N, Lp, H] INCLUDING the padded positions, with autograd into the PLM parameters (the PLM of
    PLMTextEncoder in train() mode, news_encoder.py:160-171)."""

    @staticmethod
    def forward(ctx, ids: Tensor, mask: Tensor, opts: dict, *params: Tensor):
        cfg: EncoderConfig = opts["cfg"]
        lib = _lib.load()
        n, lp = ids.shape
        m_bound = (n * lp + 255) // 256 * 256
        prec = _lib.PRECISIONS[opts["precision"]]
        cc = _cfg_c(cfg)
        dev = ids.device
        with torch.cuda.device(dev):
            saved = torch.empty(int(lib.manner_hip_train_saved_bytes(C.byref(cc), n, m_bound, 0)), dtype=torch.uint8, device=dev)
            ws = torch.empty(int(lib.manner_hip_train_workspace_bytes(C.byref(cc), m_bound)), dtype=torch.uint8, device=dev)
            out = torch.empty((n, lp, cfg.hidden), dtype=torch.float32, device=dev)
            weights = [p.detach() for p in params]
            status = hip.device_status(dev)
            status.poll()
            _lib.check(lib.manner_hip_train_full_forward(
                C.byref(cc), _table(weights), len(weights), hip._ptr(ids), hip._ptr(mask), n, lp, prec, C.c_float(opts["p_hidden"]),
                C.c_float(opts["p_attn"]), C.c_uint64(opts["seed"]), hip._ptr(out), hip._ptr(saved), saved.numel(), hip._ptr(ws), ws.numel(),
                hip._ptr(status.word), hip._stream()))
            ctx.layout = int(lib.manner_hip_train_layout_last())
            status.arm()
        ctx.opts, ctx.prec = opts, prec
        ctx.saved_buf, ctx.ws = saved, ws
        ctx.save_for_backward(ids, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        ids, *params = ctx.saved_tensors
        opts, cfg = ctx.opts, ctx.opts["cfg"]
        lib = _lib.load()
        n, lp = ids.shape
        need = ctx.needs_input_grad[3:]
        grads: List[Optional[Tensor]] = [torch.empty_like(p) if r else None for p, r in zip(params, need)]
        cc = _cfg_c(cfg)
        with torch.cuda.device(ids.device):
            g = grad_out.to(torch.float32).contiguous()
            _lib.check(lib.manner_hip_train_layout_next(ctx.layout))
            _lib.check(lib.manner_hip_train_full_backward(
                C.byref(cc), _table([p.detach() for p in params]), len(params), hip._ptr(ids), n, lp, ctx.prec, C.c_float(opts["p_hidden"]),
                C.c_float(opts["p_attn"]), C.c_uint64(opts["seed"]), hip._ptr(g), hip._ptr(ctx.saved_buf), ctx.saved_buf.numel(), _table(grads),
                hip._ptr(ctx.ws), ctx.ws.numel(), hip._stream()))
        return (None, None, None, *grads)


def encode_full_train(cfg: EncoderConfig, params: Dict[str, Tensor], ids: Tensor, mask: Tensor, *, precision: str = "fp32",
                      p_hidden: float = 0.1, p_attn: float = 0.1, seed: int = 0, max_len: int = _lib.MAX_LEN) -> Tensor:
    """[N, Lp] ids / mask -> HF ``last_hidden_state`` [N, Lp, H] including the padded positions (``hip.encode_full`` with
    autograd and HF's dropouts): what ``PLMTextEncoder`` feeds its un-masked attention in train() mode.

    ``max_len``: the longest padded batch this call accepts, as in ``encode_train`` (``Lp > max_len`` raises ``RuntimeError``); up to
    ``_lib.MAX_LEN_FULL`` (512) opts in to batches of 129..512 positions.  Every position is a row here, so ``saved`` grows with
    N * Lp; every position must also fit the model's position table."""
    if precision not in _TRAIN_PRECISIONS:
        raise ValueError(f"training precision {precision!r}: one of {_TRAIN_PRECISIONS}")
    if not 1 <= int(max_len) <= _lib.MAX_LEN_FULL:
        raise ValueError(f"max_len={max_len}: full-row training takes padded batches of 1..{_lib.MAX_LEN_FULL} tokens")
    ids, mask = hip._dev(ids, torch.int64, "input_ids").contiguous(), hip._dev(mask, torch.int64, "attention_mask").contiguous()
    if ids.dim() != 2 or ids.shape != mask.shape:
        raise ValueError(f"input_ids {tuple(ids.shape)} / attention_mask {tuple(mask.shape)} must be equal 2-D")
    if ids.shape[1] > int(max_len):
        raise RuntimeError(f"train (full rows): padded_len={ids.shape[1]} beyond max_len={int(max_len)} (padded_len <= {int(max_len)}); "
                           f"news of up to {_lib.MAX_LEN_FULL} tokens train with max_len={_lib.MAX_LEN_FULL} "
                           f"(PLMTextEncoder.train_max_length, MANNER_HIP_TRAIN_MAX_LEN)")
    canon = canonical_weights(cfg, params)
    table = [canon[name] for name in hip.weight_table_order(cfg)]
    for name, t in zip(hip.weight_table_order(cfg), table):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise TypeError(f"{name}: training needs contiguous float32 GPU parameters")
    opts = dict(cfg=cfg, precision=precision, p_hidden=float(p_hidden), p_attn=float(p_attn), seed=int(seed) & (2 ** 64 - 1))
    return _EncodeFullTrain.apply(ids, mask, opts, *table)


# ---------------------------------------------------------------------------------------------- scorer and loss
class _LateFusion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hist: Tensor, hist_off: Tensor, cand: Tensor, cand_off: Tensor):
        b, d = hist_off.numel() - 1, hist.shape[1]
        user = torch.empty((b, d), dtype=torch.float32, device=hist.device)
        scores = torch.empty(cand.shape[0], dtype=torch.float32, device=hist.device)
        with torch.cuda.device(hist.device):
            _lib.check(_lib.load().manner_hip_late_fusion_train_forward(hip._ptr(hist), hip._ptr(hist_off), hip._ptr(cand), hip._ptr(cand_off),
                                                                        b, d, hip._ptr(user), hip._ptr(scores), hip._stream()))
        ctx.save_for_backward(user, hist_off, cand, cand_off)
        ctx.n_hist = hist.shape[0]
        return scores

    @staticmethod
    def backward(ctx, g: Tensor):
        user, hist_off, cand, cand_off = ctx.saved_tensors
        b, d = user.shape
        dhist = torch.empty((ctx.n_hist, d), dtype=torch.float32, device=user.device)
        dcand = torch.empty_like(cand)
        with torch.cuda.device(user.device):
            g = g.to(torch.float32).contiguous()
            _lib.check(_lib.load().manner_hip_late_fusion_train_backward(hip._ptr(g), hip._ptr(user), hip._ptr(hist_off), hip._ptr(cand),
                                                                         hip._ptr(cand_off), b, d, hip._ptr(dhist), hip._ptr(dcand), hip._stream()))
        return dhist, None, dcand, None


def late_fusion_scores(hist: Tensor, hist_off: Tensor, cand: Tensor, cand_off: Tensor) -> Tensor:
    """Ragged scores of CRModule.forward(late_fusion=True) on per-occurrence vectors (cr_module.py:105-131), differentiable:
    hist [sum h_i, D], cand [sum c_i, D] f32, offsets int64 [B+1] on the GPU -> scores [sum c_i]."""
    hist, cand = hip._dev(hist, torch.float32, "hist").contiguous(), hip._dev(cand, torch.float32, "cand").contiguous()
    hist_off, cand_off = hip._dev(hist_off, torch.int64, "hist_off").contiguous(), hip._dev(cand_off, torch.int64, "cand_off").contiguous()
    if hist.shape[1] != cand.shape[1] or hist_off.numel() != cand_off.numel():
        raise ValueError("late_fusion_scores: mismatching shapes")
    return _LateFusion.apply(hist, hist_off, cand, cand_off)


class _Dot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user: Tensor, cand: Tensor):
        ctx.save_for_backward(user, cand)
        return hip.dot(user.detach(), cand.detach())

    @staticmethod
    def backward(ctx, g: Tensor):
        user, cand = ctx.saved_tensors
        b, _, d = user.shape
        c = cand.shape[2]
        du = torch.empty((b, 1, d), dtype=torch.float32, device=user.device)
        dc = torch.empty((b, d, c), dtype=torch.float32, device=user.device)
        with torch.cuda.device(user.device):
            g = g.to(torch.float32).contiguous()
            uc = user.contiguous()
            _lib.check(_lib.load().manner_hip_dot_backward(hip._ptr(g), hip._ptr(uc), hip._ptr(cand), b, c, d, cand.stride(0), cand.stride(1),
                                                           cand.stride(2), hip._ptr(du), hip._ptr(dc), hip._stream()))
        return du, dc


def dot(user: Tensor, cand: Tensor) -> Tensor:
    """DotProduct.forward (click_predictors.py:9-12) with autograd: user [B, 1, D], cand [B, D, C] (any strides)."""
    return _Dot.apply(hip._dev(user, torch.float32, "user_vector"), hip._dev(cand, torch.float32, "candidate_news_vector"))


class _Bmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor):
        ctx.save_for_backward(a, b)
        return hip.bmm(a.detach(), b.detach())

    @staticmethod
    def backward(ctx, g: Tensor):
        a, b = ctx.saved_tensors
        bsz, m, d = a.shape
        n = b.shape[2]
        da = torch.empty((bsz, m, d), dtype=torch.float32, device=a.device)
        db = torch.empty((bsz, d, n), dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            g, ac, bs = _f32(g, "grad"), a.contiguous(), hip._strided_operand(b)
            _lib.check(_lib.load().manner_hip_bmm_backward(hip._ptr(g), hip._ptr(ac), hip._ptr(bs), bsz, m, n, d, bs.stride(0), bs.stride(1),
                                                           bs.stride(2), hip._ptr(da), hip._ptr(db), hip._stream()))
        return da, db


def bmm(a: Tensor, b: Tensor) -> Tensor:
    """DotProduct.forward's ``torch.bmm`` for M > 1 rows (MINERModule.forward, baselines/miner_module.py:195-198) with autograd:
    a [B, M, D], b [B, D, N] (any strides) -> [B, M, N]."""
    return _Bmm.apply(hip._dev(a, torch.float32, "clicked_news_vector"), hip._dev(b, torch.float32, "candidate_news_vector"))


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores: Tensor, labels: Tensor, cand_off: Tensor, mode: int, temperature: float, c_max: int):
        b = cand_off.numel() - 1
        losses = torch.empty(b, dtype=torch.float32, device=scores.device)
        red = torch.empty(2, dtype=torch.float32, device=scores.device)
        grad = torch.empty_like(scores)
        with torch.cuda.device(scores.device):
            _lib.check(_lib.load().manner_hip_train_loss(hip._ptr(scores), hip._ptr(labels), hip._ptr(cand_off), b, mode, C.c_float(temperature),
                                                         c_max, hip._ptr(losses), hip._ptr(red), hip._ptr(grad), hip._stream()))
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(losses)
        return red[0], losses

    @staticmethod
    def backward(ctx, g: Tensor, _g_losses):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None, None


def model_step_loss(scores: Tensor, labels: Tensor, cand_off: Tensor, supcon: bool = True, temperature: float = 0.1,
                    c_max: Optional[int] = None):
    """The loss of CRModule.model_step (cr_module.py:140-171) on ragged scores, with autograd: SupConLoss on the score matrix
    (losses.py:12-40, mean over the non-zero per-impression losses) or nn.CrossEntropyLoss over the dense zero-padded rows
    (``c_max`` = the batch's largest candidate count, e.g. ``batch["cand_max"]`` from DeviceCollate).
    Returns (batch loss scalar, per-impression losses [B])."""
    scores = hip._dev(scores, torch.float32, "scores").contiguous()
    labels = hip._dev(labels, torch.float32, "labels").contiguous()
    cand_off = hip._dev(cand_off, torch.int64, "cand_off").contiguous()
    if not supcon and c_max is None:
        raise ValueError("cross-entropy mode needs c_max (the dense row width of the reference)")
    # nn.CrossEntropyLoss has no temperature (cr_module.py:169)
    return _Loss.apply(scores, labels, cand_off, 0 if supcon else 1, float(temperature) if supcon else 1.0, int(c_max or 1))


# ---------------------------------------------------------------------------------------------- small differentiable operators
# (train_small.hip) — what the reference's default `use_entities: True` and early fusion need around the text encoder
def _f32(t: Tensor, name: str) -> Tensor:
    return hip._dev(t, torch.float32, name).contiguous()


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor]):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        shape = x.shape
        y = hip.linear(x.reshape(-1, shape[-1]), weight, bias)
        return y.reshape(*shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, g: Tensor):
        x, weight = ctx.saved_tensors
        o, k = weight.shape
        x2, g2 = x.reshape(-1, k), _f32(g.reshape(-1, o), "grad")
        r = x2.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx = torch.empty_like(x2) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty(o, dtype=torch.float32, device=x.device) if need_b else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().manner_hip_linear_backward(hip._ptr(x2), hip._ptr(weight), hip._ptr(g2), r, k, o, hip._ptr(None),
                                                              hip._ptr(dx), hip._ptr(dw), hip._ptr(db), hip._stream()))
        return (dx.reshape(x.shape) if need_x else None), dw, db


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    """nn.Linear with autograd on the HIP kernels (f32): x [..., K], weight [O, K]."""
    return _Linear.apply(_f32(x, "x"), _f32(weight, "weight"), None if bias is None else _f32(bias, "bias"))


class _AdditivePool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, lin_w: Tensor, lin_b: Tensor, query: Tensor):
        ctx.save_for_backward(x, lin_w, lin_b, query)
        return hip.additive_pool(x, lin_w, lin_b, query, strict=True)      # the backward recomputes the exact-f32 pre-activations

    @staticmethod
    def backward(ctx, g: Tensor):
        x, lin_w, lin_b, query = ctx.saved_tensors
        b, s, d = x.shape
        q = lin_w.shape[0]
        lib = _lib.load()
        dx, dw, db, dq = torch.empty_like(x), torch.empty_like(lin_w), torch.empty_like(lin_b), torch.empty_like(query)
        with torch.cuda.device(x.device):
            need = int(lib.manner_hip_additive_pool_backward_workspace_bytes(b, s, d, q))
            ws = torch.empty(need, dtype=torch.uint8, device=x.device)
            g = _f32(g, "grad")
            _lib.check(lib.manner_hip_additive_pool_backward(hip._ptr(x), hip._ptr(lin_w), hip._ptr(lin_b), hip._ptr(query), hip._ptr(g), b, s, d,
                                                             q, hip._ptr(dx), hip._ptr(dw), hip._ptr(db), hip._ptr(dq), hip._ptr(ws), need,
                                                             hip._stream()))
        return dx, dw, db, dq


def additive_pool(x: Tensor, lin_w: Tensor, lin_b: Tensor, query: Tensor) -> Tensor:
    """AdditiveAttention.forward (attention.py:21-27) with autograd: x [B, S, D] -> [B, D]."""
    return _AdditivePool.apply(_f32(x, "input_vector"), _f32(lin_w, "linear.weight"), _f32(lin_b, "linear.bias"), _f32(query, "query"))


class _PolyAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, mask: Tensor, lin_w: Tensor, codes: Tensor, bias: Optional[Tensor]):
        ctx.save_for_backward(x, mask, lin_w, codes, bias)
        return hip.poly_attention(x, mask, lin_w, codes, bias)

    @staticmethod
    def backward(ctx, g: Tensor):
        x, mask, lin_w, codes, bias = ctx.saved_tensors      # the backward recomputes the weights from the pre-activations
        b, s, d = x.shape
        q, k = lin_w.shape[0], codes.shape[0]
        lib = _lib.load()
        dx, dw, dc = torch.empty_like(x), torch.empty_like(lin_w), torch.empty_like(codes)
        with torch.cuda.device(x.device):
            need = int(lib.manner_hip_poly_attention_backward_workspace_bytes(b, s, d, q, k))
            ws = hip._workspace(need, x.device)
            g = _f32(g, "grad")
            _lib.check(lib.manner_hip_poly_attention_backward(hip._ptr(x), hip._ptr(mask), hip._ptr(lin_w), hip._ptr(codes), hip._ptr(bias),
                                                              0 if bias is None else bias.shape[2], hip._ptr(g), b, s, d, q, k, hip._ptr(dx),
                                                              hip._ptr(dw), hip._ptr(dc), hip._ptr(ws), need, hip._stream()))
        return dx, None, dw, dc, None


def poly_attention(x: Tensor, mask: Tensor, lin_w: Tensor, codes: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """PolyAttention.forward (attention.py:60-84) with autograd for x, linear.weight and context_codes: x [B, S, D] -> [B, K, D].
    No gradient is built for ``bias`` (MINERModule feeds it from a frozen embedding): one that requires it is refused."""
    if bias is not None:
        if bias.requires_grad:
            raise RuntimeError("poly_attention: no gradient is built for `bias` (MINERModule's category bias comes from a frozen embedding)")
        bias = _f32(bias, "bias")
    x = _f32(x, "clicked_news_vector")
    mask = hip._mask_bytes(mask, x.shape[:2], "attn_mask")
    return _PolyAttention.apply(x, mask, _f32(lin_w, "linear.weight"), _f32(codes, "context_codes"), bias)


class _TargetAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query: Tensor, key: Tensor, value: Tensor, lin_w: Tensor):
        ctx.save_for_backward(query, key, value, lin_w)
        return hip.target_attention(query, key, value, lin_w)

    @staticmethod
    def backward(ctx, g: Tensor):
        query, key, value, lin_w = ctx.saved_tensors
        b, k, d = query.shape
        c = key.shape[1]
        lib = _lib.load()
        dq, dk, dv, dw = torch.empty_like(query), torch.empty_like(key), torch.empty_like(value), torch.empty_like(lin_w)
        with torch.cuda.device(query.device):
            need = int(lib.manner_hip_target_attention_backward_workspace_bytes(b, k, d))
            ws = hip._workspace(need, query.device)
            g = _f32(g, "grad")
            _lib.check(lib.manner_hip_target_attention_backward(hip._ptr(query), hip._ptr(key), hip._ptr(value), hip._ptr(lin_w), hip._ptr(g), b, c,
                                                                k, d, hip._ptr(dq), hip._ptr(dk), hip._ptr(dv), hip._ptr(dw), hip._ptr(ws), need,
                                                                hip._stream()))
        return dq, dk, dv, dw


def target_attention(query: Tensor, key: Tensor, value: Tensor, lin_w: Tensor) -> Tensor:
    """TargetAwareAttention.forward (attention.py:102-116) with autograd: query [B, K, D], key [B, C, D], value [B, C, K] -> [B, C]."""
    return _TargetAttention.apply(_f32(query, "query"), _f32(key, "key"), _f32(value, "value"), _f32(lin_w, "linear.weight"))


class _CodeScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cand: Tensor, cand_off: Tensor, user: Tensor, mode: int):
        arg = torch.empty(cand.shape[0], dtype=torch.int32, device=cand.device) if mode == 0 else None
        out = hip._code_scores_forward(cand, cand_off, user, mode, arg)
        ctx.save_for_backward(cand, cand_off, user, arg)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        cand, cand_off, user, arg = ctx.saved_tensors
        n, d = cand.shape
        b, k = user.shape[:2]
        dc, du = torch.empty_like(cand), torch.empty_like(user)
        with torch.cuda.device(cand.device):
            g = _f32(g, "grad")
            _lib.check(_lib.load().manner_hip_miner_code_scores_backward(hip._ptr(g), hip._ptr(cand), hip._ptr(cand_off), hip._ptr(user), hip._ptr(arg),
                                                                         n, b, k, d, ctx.mode, hip._ptr(dc), hip._ptr(du), hip._stream()))
        return dc, None, du, None


def miner_code_scores(cand: Tensor, cand_off: Tensor, user: Tensor, score_type: str) -> Tensor:
    """``hip.miner_code_scores`` with autograd into the candidate rows and the user vectors: 'max' sends a candidate's gradient to its
    argmax code (ties: the lowest index, as torch's CPU ``max(dim)``), 'mean' spreads it evenly over the K codes; d user is a
    fixed-order sum over the user's candidates."""
    cand, cand_off, user, mode = hip._code_scores_operands(cand, cand_off, user, score_type)
    return _CodeScores.apply(cand, cand_off, user, mode)


class _Disagreement(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user: Tensor):
        ctx.save_for_backward(user)
        return hip.disagreement_loss(user)

    @staticmethod
    def backward(ctx, g: Tensor):
        (user,) = ctx.saved_tensors
        b, k, d = user.shape
        du = torch.empty_like(user)
        with torch.cuda.device(user.device):
            g = _f32(g, "grad").reshape(1)                       # stays on the device: nothing is read back
            _lib.check(_lib.load().manner_hip_disagreement_loss_backward(hip._ptr(user), hip._ptr(g), b, k, d, hip._ptr(du), hip._stream()))
        return du


def disagreement_loss(user: Tensor) -> Tensor:
    """``hip.disagreement_loss`` with autograd into user [B, K, D]; a zero row receives the finite gradient through 1 / 1e-8 that torch
    autograd gives the reference's lines."""
    return _Disagreement.apply(hip._disagreement_operand(user))


def _head_backward(entry, ctx, g: Tensor, x: Tensor, weight: Tensor, saved: Tensor, dims):
    """The shared backward of the two row heads: the device-scalar upstream gradient goes to the library as it is; an input that needs
    no gradient (a frozen head, detached rows) passes NULL and its kernel is skipped."""
    need_x, need_w, need_b = ctx.needs_input_grad[:3]
    dx = torch.empty_like(x) if need_x else None
    dw = torch.empty_like(weight) if need_w else None
    db = torch.empty(weight.shape[0], dtype=torch.float32, device=x.device) if need_b else None
    lib = _lib.load()
    with torch.cuda.device(x.device):
        g = _f32(g, "grad").reshape(1)                           # stays on the device: nothing is read back
        need = int(lib.manner_hip_head_backward_workspace_bytes(x.shape[0], x.shape[1], weight.shape[0])) if (need_w or need_b) else 0
        ws = hip._workspace(need, x.device) if need else None
        _lib.check(entry(lib)(hip._ptr(g), hip._ptr(x), hip._ptr(weight), hip._ptr(saved), *dims, hip._ptr(dx), hip._ptr(dw), hip._ptr(db),
                              hip._ptr(ws), need, hip._stream()))
    return dx, dw, db, None


class _HeadCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Tensor, target: Tensor):
        saved = torch.empty((x.shape[0], weight.shape[0]), dtype=torch.float32, device=x.device)      # p - y
        loss = hip._head_ce_forward(x, weight, bias, target, saved, None)
        ctx.save_for_backward(x, weight, saved)
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        x, weight, saved = ctx.saved_tensors
        return _head_backward(lambda lib: lib.manner_hip_head_ce_backward, ctx, g, x, weight, saved, (x.shape[0], x.shape[1], weight.shape[0]))


def head_ce_loss(x: Tensor, weight: Tensor, bias: Tensor, target: Tensor) -> Tensor:
    """``hip.head_ce_loss`` with autograd into the rows, the weight and the bias: ``CrossEntropyLoss(Linear(x), one_hot(target))`` in one
    fused forward, gradients from the saved p - y with fixed-order sums over the rows."""
    return _HeadCE.apply(*hip._head_operands(x, weight, bias, target, torch.int64, "head_ce_loss"))


class _HeadL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Tensor, target: Tensor):
        saved = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)                           # sign(residual)
        loss = hip._head_l1_forward(x, weight, bias, target, saved)
        ctx.save_for_backward(x, weight, saved)
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        x, weight, saved = ctx.saved_tensors
        return _head_backward(lambda lib: lib.manner_hip_head_l1_backward, ctx, g, x, weight, saved, (x.shape[0], x.shape[1]))


def head_l1_loss(x: Tensor, weight: Tensor, bias: Tensor, target: Tensor) -> Tensor:
    """``hip.head_l1_loss`` with autograd: ``L1Loss(Linear(D, 1)(x).flatten(), target)``; a residual of exactly 0 sends no gradient
    (sign(0) = 0, as torch)."""
    return _HeadL1.apply(*hip._head_l1_operands(x, weight, bias, target))


class _SentiDiv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores: Tensor, cand_score: Tensor, hist_score: Tensor, hist_off: Tensor, cand_off: Tensor, c_max: int):
        ctx.save_for_backward(scores, cand_score, hist_score, hist_off, cand_off)
        ctx.c_max = c_max
        return hip._senti_div_forward(scores, cand_score, hist_score, hist_off, cand_off, c_max)

    @staticmethod
    def backward(ctx, g: Tensor):
        scores, cand_score, hist_score, hist_off, cand_off = ctx.saved_tensors
        ds = torch.zeros_like(scores)
        with torch.cuda.device(scores.device):
            g = _f32(g, "grad").reshape(1)                       # stays on the device: nothing is read back
            _lib.check(_lib.load().manner_hip_senti_div_backward(hip._ptr(g), hip._ptr(scores), hip._ptr(cand_score), hip._ptr(hist_score),
                                                                 hip._ptr(hist_off), hip._ptr(cand_off), scores.numel(), hist_score.numel(),
                                                                 cand_off.numel() - 1, ctx.c_max, hip._ptr(ds), hip._stream()))
        return ds, None, None, None, None, None


def senti_div_loss(scores: Tensor, cand_score: Tensor, hist_score: Tensor, hist_off: Tensor, cand_off: Tensor, c_max: int) -> Tensor:
    """``hip.senti_div_loss`` with autograd into the ragged scores: the gradient is 0 where the product u s score is <= 0."""
    return _SentiDiv.apply(*hip._senti_div_operands(scores, cand_score, hist_score, hist_off, cand_off, c_max))


class _MaskRowZero(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table: Tensor):
        return table.view_as(table)

    @staticmethod
    def backward(ctx, g: Tensor):
        g = g.clone()
        g[0].zero_()
        return g


def class_table(embedding_weight: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    """The C distinct outputs of SentiDebias's SentimentEncoder (reference baselines/senti_debias_plm_module.py:41-42),
    ``tanh(linear(embedding.weight))`` [C, D] by ``linear_tanh`` on the C rows.  Row 0 (``padding_idx = 0``) is read as it lies and receives
    no gradient into the embedding; its ``tanh(b)`` still sends gradient into the linear."""
    graph = torch.is_grad_enabled() and (embedding_weight.requires_grad or weight.requires_grad or bias.requires_grad)
    if not graph:
        return hip.linear_tanh(embedding_weight.detach(), weight.detach(), bias.detach())
    return linear_tanh(_MaskRowZero.apply(embedding_weight) if embedding_weight.requires_grad else embedding_weight, weight, bias)


class _OrthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows: Tensor, n_hist: int, table: Tensor, cls: Tensor, user_free: Tensor, user_aware: Tensor):
        means = torch.empty(2, dtype=torch.float32, device=rows.device)
        loss = hip._orth_forward(rows, n_hist, table, cls, user_free, user_aware, means)
        ctx.save_for_backward(rows, table, cls, user_free, user_aware, means)
        ctx.n_hist = n_hist
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        rows, table, cls, user_free, user_aware, means = ctx.saved_tensors
        need_rows, _, need_table, _, need_free, need_aware = ctx.needs_input_grad
        n, d = rows.shape
        c, b = table.shape[0], user_free.shape[0]
        d_rows = torch.empty_like(rows) if need_rows else None
        d_table = torch.empty_like(table) if need_table else None
        d_free = torch.empty_like(user_free) if need_free else None
        d_aware = torch.empty_like(user_aware) if need_aware else None
        lib = _lib.load()
        with torch.cuda.device(rows.device):
            g = _f32(g, "grad").reshape(1)                       # stays on the device: nothing is read back
            need = int(lib.manner_hip_orth_loss_backward_workspace_bytes(n, d, c)) if need_table else 0
            ws = hip._workspace(need, rows.device) if need else None
            _lib.check(lib.manner_hip_orth_loss_backward(hip._ptr(g), hip._ptr(means), hip._ptr(rows), n, ctx.n_hist, hip._ptr(table), hip._ptr(cls),
                                                         hip._ptr(user_free), hip._ptr(user_aware), b, d, c, hip._ptr(d_rows), hip._ptr(d_table),
                                                         hip._ptr(d_free), hip._ptr(d_aware), hip._ptr(ws), need, hip._stream()))
        return d_rows, None, d_table, None, d_free, d_aware


def orth_loss(rows: Tensor, n_hist: int, table: Tensor, cls: Tensor, user_free: Tensor, user_aware: Tensor) -> Tensor:
    """``hip.orth_loss`` with autograd into the rows, the class table and the two user vectors; the table's gradient is a per-class sum
    over chunks of ascending rows added in order.  A zero vector receives torch's zero gradient through its norm."""
    return _OrthLoss.apply(*hip._orth_operands(rows, n_hist, table, cls, user_free, user_aware))


class _ClassDense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table: Tensor, cls: Tensor, off: Tensor, width: int):
        ctx.save_for_backward(cls, off)
        ctx.dims = (width, table.shape[1], table.shape[0])
        return hip._class_dense_forward(table, cls, off, width)

    @staticmethod
    def backward(ctx, g: Tensor):
        cls, off = ctx.saved_tensors
        width, d, c = ctx.dims
        b = off.numel() - 1
        d_table = torch.empty((c, d), dtype=torch.float32, device=g.device)
        lib = _lib.load()
        with torch.cuda.device(g.device):
            g = _f32(g, "grad").contiguous()
            need = int(lib.manner_hip_class_dense_backward_workspace_bytes(b, width, d, c))
            ws = hip._workspace(need, g.device)
            _lib.check(lib.manner_hip_class_dense_backward(hip._ptr(g), hip._ptr(cls), hip._ptr(off), cls.numel(), b, width, d, c, hip._ptr(d_table),
                                                           hip._ptr(ws), need, hip._stream()))
        return d_table, None, None, None


def class_dense(table: Tensor, cls: Tensor, off: Tensor, width: int) -> Tensor:
    """``hip.class_dense`` with autograd into the class table."""
    return _ClassDense.apply(*hip._class_dense_operands(table, cls, off, width))


class _ClassScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user: Tensor, table: Tensor, cls: Tensor, off: Tensor):
        ctx.save_for_backward(user, table, cls, off)
        return hip._class_scores_forward(user, table, cls, off)

    @staticmethod
    def backward(ctx, g: Tensor):
        user, table, cls, off = ctx.saved_tensors
        need_user, need_table = ctx.needs_input_grad[:2]
        b, d = user.shape
        c = table.shape[0]
        d_user = torch.empty_like(user) if need_user else None
        d_table = torch.empty_like(table) if need_table else None
        lib = _lib.load()
        with torch.cuda.device(user.device):
            g = _f32(g, "grad").contiguous()
            need = int(lib.manner_hip_class_scores_workspace_bytes(b, c))
            ws = hip._workspace(need, user.device)
            _lib.check(lib.manner_hip_class_scores_backward(hip._ptr(g), hip._ptr(user), hip._ptr(table), hip._ptr(cls), hip._ptr(off), cls.numel(), b,
                                                            d, c, hip._ptr(d_user), hip._ptr(d_table), hip._ptr(ws), need, hip._stream()))
        return d_user, d_table, None, None


def class_scores(user: Tensor, table: Tensor, cls: Tensor, off: Tensor) -> Tensor:
    """``hip.class_scores`` with autograd into the user vectors and the class table, from the per-(user, class) sums of the upstream
    gradient."""
    return _ClassScores.apply(*hip._class_scores_operands(user, table, cls, off))


class _AdvLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows: Tensor, n_hist: int, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, cls: Tensor):
        hidden = torch.empty((rows.shape[0], w1.shape[0]), dtype=torch.float32, device=rows.device)
        saved = torch.empty((rows.shape[0], w2.shape[0]), dtype=torch.float32, device=rows.device)      # (p - y) / rows of the segment
        loss = hip._adv_forward(rows, n_hist, w1, b1, w2, b2, cls, hidden, saved)
        ctx.save_for_backward(rows, w1, w2, hidden, saved)
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        rows, w1, w2, hidden, saved = ctx.saved_tensors
        need_rows, _, need_w1, need_b1, need_w2, need_b2, _ = ctx.needs_input_grad
        n, d = rows.shape
        h, o = w1.shape[0], w2.shape[0]
        d_rows = torch.empty_like(rows) if need_rows else None
        d_w1 = torch.empty_like(w1) if need_w1 else None
        d_b1 = torch.empty(h, dtype=torch.float32, device=rows.device) if need_b1 else None
        d_w2 = torch.empty_like(w2) if need_w2 else None
        d_b2 = torch.empty(o, dtype=torch.float32, device=rows.device) if need_b2 else None
        lib = _lib.load()
        with torch.cuda.device(rows.device):
            g = _f32(g, "grad").reshape(1)                       # stays on the device: nothing is read back
            need = int(lib.manner_hip_adv_loss_backward_workspace_bytes(n, d, h, o))
            ws = hip._workspace(need, rows.device)
            _lib.check(lib.manner_hip_adv_loss_backward(hip._ptr(g), hip._ptr(rows), n, hip._ptr(w1), hip._ptr(w2), hip._ptr(hidden), hip._ptr(saved),
                                                        d, h, o, hip._ptr(d_rows), hip._ptr(d_w1), hip._ptr(d_b1), hip._ptr(d_w2), hip._ptr(d_b2),
                                                        hip._ptr(ws), need, hip._stream()))
        return d_rows, None, d_w1, d_b1, d_w2, d_b2, None


def adv_loss(rows: Tensor, n_hist: int, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, cls: Tensor) -> Tensor:
    """``hip.adv_loss`` with autograd into the rows and the discriminator's four parameters.  In the generator step the discriminator is
    frozen and only the rows' gradient is formed, in the discriminator step the rows are detached and only the four parameter gradients:
    both are the bits of the full backward."""
    return _AdvLoss.apply(*hip._adv_operands(rows, n_hist, w1, b1, w2, b2, cls))


class _Axis0Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv: Tensor, heads: int):
        l0, b1, e3 = qkv.shape
        out = torch.empty((l0, b1, e3 // 3), dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            _lib.check(_lib.load().manner_hip_axis0_attention(hip._ptr(qkv), l0, b1, e3 // 3, heads, hip._ptr(out), hip._stream()))
        ctx.save_for_backward(qkv)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        (qkv,) = ctx.saved_tensors
        l0, b1, e3 = qkv.shape
        dqkv = torch.empty_like(qkv)
        stats = torch.empty(l0 * b1 * ctx.heads * 3, dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            g = _f32(g, "grad")
            _lib.check(_lib.load().manner_hip_axis0_attention_backward(hip._ptr(qkv), hip._ptr(g), l0, b1, e3 // 3, ctx.heads, hip._ptr(dqkv),
                                                                       hip._ptr(stats), hip._stream()))
        return dqkv, None


def mha_axis0(x: Tensor, in_proj_w: Tensor, in_proj_b: Tensor, out_proj_w: Tensor, out_proj_b: Tensor, heads: int) -> Tensor:
    """nn.MultiheadAttention(batch_first=False) as the reference calls it on [batch, seq, E] without masks (quirk Q1), with
    autograd: in-projection, attention along axis 0, out-projection."""
    qkv = linear(x, in_proj_w, in_proj_b)
    return linear(_Axis0Attention.apply(qkv.contiguous(), int(heads)), out_proj_w, out_proj_b)


class _Axis0AttentionFamily(torch.autograd.Function):
    """The attention core of a run-time-head-dim family, ``hip.axis0_family``'s "any" or "wide": the forward keeps its output and the
    softmax statistics, the backward is the family's two entries."""

    @staticmethod
    def forward(ctx, qkv: Tensor, heads: int, family: str):
        l0, b1, _ = qkv.shape
        stats = torch.empty(l0 * b1 * heads * 3, dtype=torch.float32, device=qkv.device)
        out = hip._axis0_attention(family, qkv, heads, stats)
        ctx.save_for_backward(qkv, out, stats)
        ctx.heads, ctx.family = heads, family
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        qkv, out, stats = ctx.saved_tensors
        l0, b1, e3 = qkv.shape
        dqkv = torch.empty_like(qkv)
        lib = _lib.load()
        with torch.cuda.device(qkv.device):
            g = _f32(g, "grad")
            entry = "manner_hip_axis0_attention_" + ctx.family
            _lib.check(getattr(lib, entry + "_backward_q")(hip._ptr(qkv), hip._ptr(out), hip._ptr(g), l0, b1, e3 // 3, ctx.heads, hip._ptr(dqkv),
                                                           hip._ptr(stats), hip._stream()))
            _lib.check(getattr(lib, entry + "_backward_kv")(hip._ptr(qkv), hip._ptr(g), hip._ptr(stats), l0, b1, e3 // 3, ctx.heads, hip._ptr(dqkv),
                                                            hip._stream()))
        return dqkv, None, None


def _mha_axis0(family: str, x: Tensor, in_proj_w: Tensor, in_proj_b: Tensor, out_proj_w: Tensor, out_proj_b: Tensor, heads: int) -> Tensor:
    qkv = linear(x, in_proj_w, in_proj_b)
    return linear(_Axis0AttentionFamily.apply(qkv.contiguous(), int(heads), family), out_proj_w, out_proj_b)


def mha_axis0_any(x: Tensor, in_proj_w: Tensor, in_proj_b: Tensor, out_proj_w: Tensor, out_proj_b: Tensor, heads: int) -> Tensor:
    """``mha_axis0`` at ANY head dim 1..64, with autograd (CAUM's entity encoder: head dim 5)."""
    return _mha_axis0("any", x, in_proj_w, in_proj_b, out_proj_w, out_proj_b, heads)


class _CaumUser(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, c: Tensor, opts: dict, *params: Tensor):
        out, saved, need = hip._caum_forward(x, c, [t.detach() for t in params], opts["dims"], opts["p"], opts["seed"], opts["site0"])
        ctx.opts, ctx.saved_buf, ctx.saved_bytes = opts, saved, need
        ctx.save_for_backward(*params)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        params = ctx.saved_tensors
        opts = ctx.opts
        dims = opts["dims"]
        b, s, d = dims[:3]
        dev = ctx.saved_buf.device
        lib = _lib.load()
        dx = torch.empty((b, s, d), dtype=torch.float32, device=dev)
        dc = torch.empty((b, d), dtype=torch.float32, device=dev)
        grads = [torch.empty_like(t) for t in params]
        with torch.cuda.device(dev):
            g = _f32(g, "grad")
            need = int(lib.manner_hip_caum_user_backward_workspace_bytes(*dims))
            ws = hip._workspace(need, dev)
            _lib.check(lib.manner_hip_caum_user_backward(_table([t.detach() for t in params]), hip._ptr(g), *dims, C.c_float(opts["p"]),
                                                         C.c_uint64(opts["seed"]), C.c_uint32(opts["site0"]), hip._ptr(ctx.saved_buf),
                                                         ctx.saved_bytes, hip._ptr(dx), hip._ptr(dc), _table(grads), hip._ptr(ws), need,
                                                         hip._stream()))
        return (dx, dc, None, *grads)


def caum_user_scores(x: Tensor, c: Tensor, params: Sequence[Tensor], heads: int, p: float = 0.0, seed: int = 0,
                     site0: int = hip.CAUM_DROPOUT_SITE) -> Tensor:
    """CAUMUserEncoder.forward (user_encoder.py:121-178) with autograd into x, c and the 16 parameters (``hip.CAUM_PARAMS`` order):
    x [B, S, D], c [B, D] (any row stride) -> scores [B].  ``p`` > 0: dropout1 / 2 / 3 at the sites ``site0`` .. ``site0 + 2`` of the
    counter-based generator (``dropout_mask`` returns the same bits).  The backward is hand-written from the saved activations; the K
    third of d in_proj_bias and d dense_att.linear3.bias, zero in exact arithmetic, come back as exact zeros."""
    x, c, params, dims = hip._caum_operands(x, c, params, heads)
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"caum_user_scores: p={p} outside [0, 1)")
    opts = dict(dims=dims, p=float(p), seed=int(seed) & (2 ** 64 - 1), site0=int(site0))
    return _CaumUser.apply(x, c, opts, *params)


def dense_slots(off: Tensor, n: int, width: int) -> Tensor:
    """The flat slot b * width + j of each of the ``n`` ragged rows in the dense [B, width] layout of ``to_dense_batch`` — from the
    offsets on the device, nothing read back."""
    rows = torch.arange(n, dtype=torch.int64, device=off.device)
    seg = torch.searchsorted(off[1:].contiguous(), rows, right=True)
    return seg * int(width) + (rows - off[seg])


class _ToDense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, off: Tensor, width: int):
        ctx.save_for_backward(off)
        ctx.n, ctx.width = x.shape[0], int(width)
        return hip.to_dense(x, off, int(width))

    @staticmethod
    def backward(ctx, g: Tensor):
        (off,) = ctx.saved_tensors
        g = g.contiguous()
        return g.reshape((-1,) + tuple(g.shape[2:])).index_select(0, dense_slots(off, ctx.n, ctx.width)), None, None


def to_dense(x: Tensor, off: Tensor, width: int) -> Tensor:
    """``hip.to_dense`` (K9, ``to_dense_batch``) with autograd into the ragged rows: the gradient of a real slot, none for the padding."""
    return _ToDense.apply(_f32(x, "x"), hip._dev(off, torch.int64, "off").contiguous(), int(width))


class _CaumAll(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, cand: Tensor, opts: dict, seeds: Optional[Tensor], *params: Tensor):
        b, s, c = opts["dims"][:3]
        lib = _lib.load()
        scores = torch.empty((b, c), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            need = int(lib.manner_hip_caum_train_all_saved_bytes(*opts["dims"]))
            saved = hip._workspace(need, x.device)
            _lib.check(lib.manner_hip_caum_train_all_forward(hip._ptr(x), hip._ptr(cand), _table([t.detach() for t in params]), *opts["dims"],
                                                             C.c_float(opts["p"]), hip._ptr(seeds), C.c_uint32(opts["site0"]), hip._ptr(scores),
                                                             hip._ptr(saved), need, hip._stream()))
        ctx.opts, ctx.saved_buf, ctx.saved_bytes, ctx.seeds = opts, saved, need, seeds
        ctx.save_for_backward(*params)
        return scores

    @staticmethod
    def backward(ctx, g: Tensor):
        params = ctx.saved_tensors
        opts = ctx.opts
        dims = opts["dims"]
        b, s, c, d = dims[:4]
        dev = ctx.saved_buf.device
        lib = _lib.load()
        dx = torch.empty((b, s, d), dtype=torch.float32, device=dev)
        dc = torch.empty((b, c, d), dtype=torch.float32, device=dev)
        grads = [torch.empty_like(t) for t in params]
        with torch.cuda.device(dev):
            g = _f32(g, "grad")
            need = int(lib.manner_hip_caum_train_all_backward_workspace_bytes(*dims))
            ws = hip._workspace(need, dev)
            _lib.check(lib.manner_hip_caum_train_all_backward(_table([t.detach() for t in params]), hip._ptr(g), *dims, C.c_float(opts["p"]),
                                                              hip._ptr(ctx.seeds), C.c_uint32(opts["site0"]), hip._ptr(ctx.saved_buf),
                                                              ctx.saved_bytes, hip._ptr(dx), hip._ptr(dc), _table(grads), hip._ptr(ws), need,
                                                              hip._stream()))
        return (dx, dc, None, None, *grads)


def caum_scores_all(x: Tensor, cand: Tensor, params: Sequence[Tensor], heads: int, p: float = 0.0, seeds: Optional[Sequence[int]] = None,
                    site0: int = hip.CAUM_DROPOUT_SITE) -> Tensor:
    """The candidate loop of CAUMPLMModule.forward in train(): x [B, S, D], cand [B, C, D] -> scores [B, C] with autograd into x, cand
    and the 16 parameters, column c what ``caum_user_scores(x, cand[:, c, :], ..., p, seeds[c], site0)`` computes — the same dropout
    sites and element indices, so the same masks — in ONE library call forward and one backward over the B C S rows (f32 matrix-core
    linears, data and weight gradients).  ``seeds``: C integers (or an int64 tensor), needed when ``p`` > 0; they reach the device as one
    small tensor, nothing is read back.  d x is the sum of the columns' contributions in ascending c, each through its own dropout2
    mask; the two analytically zero gradients come back as exact zeros."""
    if not isinstance(cand, torch.Tensor) or cand.dim() != 3:
        raise ValueError(f"caum_scores_all: cand_news_vector {tuple(getattr(cand, 'shape', ()))} must be [B, C, D]")
    b, c = cand.shape[0], cand.shape[1]
    x, _, params, dims = hip._caum_operands(x, cand[:, 0, :] if c else cand.new_empty((b, cand.shape[2])), params, heads)
    cand = hip._dev(cand, torch.float32, "cand_news_vector").contiguous()
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"caum_scores_all: p={p} outside [0, 1)")
    dev_seeds = None
    if float(p) > 0.0:
        if seeds is None or len(seeds) != c:
            raise ValueError(f"caum_scores_all: p > 0 needs one seed per candidate column ({c})")
        if isinstance(seeds, torch.Tensor):
            dev_seeds = seeds.to(device=x.device, dtype=torch.int64).contiguous()
        else:                                                   # any 64 bits, carried as int64
            wrapped = [((int(v) & (2 ** 64 - 1)) ^ (1 << 63)) - (1 << 63) for v in seeds]
            dev_seeds = torch.tensor(wrapped, dtype=torch.int64).to(x.device, non_blocking=True)
    opts = dict(dims=(dims[0], dims[1], c) + dims[2:], p=float(p), site0=int(site0))
    return _CaumAll.apply(x, cand, opts, dev_seeds, *params)


def _gru_backward(ctx, g: Tensor, want_h0: bool):
    """manner_hip_gru_backward from the buffers ``ctx`` kept: g [B, >= H] (its first H columns are d last_hidden) ->
    (dx, dh0 or None, [dw_ih, dw_hh, db_ih, db_hh])."""
    lengths, w_ih, w_hh = ctx.saved_tensors[:3]
    b, s, i, h = dims = ctx.dims
    dev = ctx.saved_buf.device
    lib = _lib.load()
    dx = torch.empty((b, s, i), dtype=torch.float32, device=dev)
    dh0 = torch.empty((b, h), dtype=torch.float32, device=dev) if want_h0 else None
    grads = [torch.empty((3 * h, i), dtype=torch.float32, device=dev), torch.empty((3 * h, h), dtype=torch.float32, device=dev),
             torch.empty(3 * h, dtype=torch.float32, device=dev), torch.empty(3 * h, dtype=torch.float32, device=dev)]
    with torch.cuda.device(dev):
        need = int(lib.manner_hip_gru_workspace_bytes(*dims))
        ws = hip._workspace(need, dev)
        _lib.check(lib.manner_hip_gru_backward(hip._ptr(w_ih), hip._ptr(w_hh), hip._ptr(lengths), hip._ptr(g), g.stride(0) if b > 1 else g.shape[1],
                                               *dims, hip._ptr(ctx.saved_buf), ctx.saved_bytes, hip._ptr(dx), hip._ptr(dh0), *[hip._ptr(t) for t in grads],
                                               hip._ptr(ws), need, hip._stream()))
    return dx, dh0, grads


class _GruLastHidden(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, lengths: Tensor, dims, h0: Optional[Tensor], *params: Tensor):
        gru = [t.detach() for t in params]
        out = torch.empty((dims[0], dims[3]), dtype=torch.float32, device=x.device)
        ctx.saved_buf, ctx.saved_bytes = hip._gru_forward(x, lengths, gru, None if h0 is None else h0.detach(), dims, out, save=True)
        ctx.dims, ctx.has_h0 = dims, h0 is not None
        ctx.save_for_backward(lengths, params[0], params[1])
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        dx, dh0, grads = _gru_backward(ctx, _f32(g, "grad"), ctx.has_h0)
        return (dx, None, None, dh0, *grads)


def gru_last_hidden(x: Tensor, lengths: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, h0: Optional[Tensor] = None) -> Tensor:
    """``hip.gru_last_hidden`` with autograd into x, the four ``nn.GRU`` tensors and h0: the forward keeps the gates of every step, the
    backward is S plain launches in reverse and the stacked weight gradients.  d x is exactly 0 at the slots past a row's length."""
    x, lengths, params, h0, dims = hip._gru_operands(x, lengths, w_ih, w_hh, b_ih, b_hh, h0)
    return _GruLastHidden.apply(x, lengths, dims, h0, *params)


class _LsturUser(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user: Tensor, x: Tensor, lengths: Tensor, opts: dict, table: Tensor, *params: Tensor):
        out, ctx.saved_buf, ctx.saved_bytes = hip._lstur_forward(user, x, lengths, table.detach(), [t.detach() for t in params], opts["dims"],
                                                                 opts["method"], opts["p"], opts["seed"], save=True)
        ctx.dims, ctx.opts, ctx.rows = opts["dims"], opts, table.shape[0]
        ctx.save_for_backward(lengths, params[0], params[1], user)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        g = _f32(g, "grad")
        opts, user = ctx.opts, ctx.saved_tensors[3]
        b, h = ctx.dims[0], ctx.dims[3]
        ini = opts["method"] == "ini"
        dx, dh0, grads = _gru_backward(ctx, g, ini)
        if not ctx.needs_input_grad[4]:                # a frozen table: no [num_users, E] gradient is built
            return (None, dx, None, None, None, *grads)
        # the user rows' gradient (ini: d h0; con: the second half of g) through the mask, then into the rows of the table
        drows = hip.user_rows(None, dh0 if ini else g[:, h:], torch.empty((b, h), dtype=torch.float32, device=g.device), opts["p"], opts["seed"])
        dtable = torch.empty((ctx.rows, h), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.load().manner_hip_embedding_backward(hip._ptr(user), b, hip._ptr(drows), ctx.rows, h, 0, hip._ptr(dtable), hip._stream()))
        return (None, dx, None, None, dtable, *grads)


def lstur_user(user: Tensor, x: Tensor, lengths: Tensor, params: Sequence[Tensor], method: str, p: float = 0.0, seed: int = 0) -> Tensor:
    """LSTURUserEncoder.forward (user_encoder.py:70-89) with autograd into x and the five parameters (``hip.LSTUR_PARAMS`` order).
    ``p`` > 0: whole users are masked at (seed, row) (``nn.Dropout2d`` on [1, B, E]); the mask scale is applied to the incoming
    gradient before ``manner_hip_embedding_backward`` (row 0, the padding row, receives nothing; a repeated user's rows add up)."""
    user, x, lengths, table, gru, dims = hip._lstur_operands(user, x, lengths, params, method)
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"lstur_user: p={p} outside [0, 1)")
    opts = dict(dims=dims, method=method, p=float(p), seed=int(seed) & (2 ** 64 - 1))
    return _LsturUser.apply(user, x, lengths, opts, table, *gru)


class _ChannelGru(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, lengths: Tensor, dims, *params: Tensor):
        out, ctx.saved_buf, ctx.saved_bytes = hip._channel_gru_forward(x, lengths, [t.detach() for t in params], dims, save=True)
        ctx.dims = dims
        ctx.save_for_backward(lengths, params[0], params[1])
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        lengths, w_ih, w_hh = ctx.saved_tensors
        b, s, c, i, h = dims = ctx.dims
        dev = ctx.saved_buf.device
        lib = _lib.load()
        g = _f32(g, "grad")
        dx = torch.empty((b, s, c * i), dtype=torch.float32, device=dev)
        grads = [torch.empty((3 * h, i), dtype=torch.float32, device=dev), torch.empty((3 * h, h), dtype=torch.float32, device=dev),
                 torch.empty(3 * h, dtype=torch.float32, device=dev), torch.empty(3 * h, dtype=torch.float32, device=dev)]
        with torch.cuda.device(dev):
            need = int(lib.manner_hip_channel_gru_workspace_bytes(*dims))
            ws = hip._workspace(need, dev)
            _lib.check(lib.manner_hip_channel_gru_backward(hip._ptr(w_ih), hip._ptr(w_hh), hip._ptr(lengths), hip._ptr(g), c * h, *dims,
                                                           hip._ptr(ctx.saved_buf), ctx.saved_bytes, hip._ptr(dx), *[hip._ptr(t) for t in grads],
                                                           hip._ptr(ws), need, hip._stream()))
        return (dx, None, None, *grads)


def channel_gru_last_hidden(x: Tensor, lengths: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, channels: int) -> Tensor:
    """``hip.channel_gru_last_hidden`` with autograd into x and the four shared ``nn.GRU`` tensors: the forward keeps the gates of every
    step, the backward is one launch walking the steps in reverse and the weight gradients over the rows stacked in (b, t, c) order — one
    fixed-order sum over all channels.  d x is exactly 0 at the slots past a row's length."""
    x, lengths, params, dims = hip._channel_gru_operands(x, lengths, w_ih, w_hh, b_ih, b_hh, channels)
    return _ChannelGru.apply(x, lengths, dims, *params)


def mha_axis0_wide(x: Tensor, in_proj_w: Tensor, in_proj_b: Tensor, out_proj_w: Tensor, out_proj_b: Tensor, heads: int) -> Tensor:
    """``mha_axis0_any`` at head dims 65 .. 128, with autograd (MINS's user encoder: head dim 128)."""
    return _mha_axis0("wide", x, in_proj_w, in_proj_b, out_proj_w, out_proj_b, heads)


class _UnitPool(torch.autograd.Function):
    """AdditiveAttention over a sequence of ONE slot: the softmax over one logit is 1, so the output is the input bit for bit and the
    pooler's three parameters receive exact zeros — as tensors, not None, as the reference's autograd gives them."""

    @staticmethod
    def forward(ctx, x: Tensor, *pool: Tensor):
        ctx.save_for_backward(*pool)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g: Tensor):
        return (g, *[torch.zeros_like(t) if need else None for t, need in zip(ctx.saved_tensors, ctx.needs_input_grad[1:])])


def mins_user(x: Tensor, lengths: Tensor, params: Sequence[Tensor], channels: int, pool: Sequence[Tensor] = ()) -> Tensor:
    """MINSUserEncoder.forward (user_encoder.py:211-243) with autograd into x and the eight parameters (``hip.MINS_PARAMS`` order):
    x [B, S, D], lengths int64 [B] (never copied to the host) -> [B, D].  d x is NOT zero at the slots past a user's length: the
    attention reads them on behalf of the other users; only the GRU's own input gradient is zero there.  ``pool``: the parameters of
    the final AdditiveAttention, which runs over one slot and is the identity — they receive exact-zero gradients."""
    x, c = hip._mins_operands(x, params, channels)
    out = channel_gru_last_hidden(_mha_axis0(hip.axis0_family(x.shape[2] // c), x, *params[:4], c), lengths, *params[4:], c)
    return _UnitPool.apply(out, *pool) if pool else out


class _LinearTanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor]):
        shape = x.shape
        y = hip.linear_tanh(x.reshape(-1, shape[-1]), weight, bias)
        ctx.save_for_backward(x, weight, y)
        ctx.has_bias = bias is not None
        return y.reshape(*shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, g: Tensor):
        x, weight, y = ctx.saved_tensors
        o, k = weight.shape
        x2, g2 = x.reshape(-1, k), _f32(g.reshape(-1, o), "grad")
        r = x2.shape[0]
        lib = _lib.load()
        dpre, dx, dw = torch.empty_like(y), torch.empty_like(x2), torch.empty_like(weight)
        db = torch.empty(o, dtype=torch.float32, device=x.device) if ctx.has_bias else None
        with torch.cuda.device(x.device):
            _lib.check(lib.manner_hip_tanh_backward(hip._ptr(y), hip._ptr(g2), hip._ptr(dpre), y.numel(), hip._stream()))
            _lib.check(lib.manner_hip_linear_backward(hip._ptr(x2), hip._ptr(weight), hip._ptr(dpre), r, k, o, hip._ptr(None), hip._ptr(dx),
                                                      hip._ptr(dw), hip._ptr(db), hip._stream()))
        return dx.reshape(x.shape), dw, db


def linear_tanh(x: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    """tanh(nn.Linear(x)) with autograd (DenseAttention's first two layers, attention.py:135-138): x [..., K], weight [O, K]."""
    return _LinearTanh.apply(_f32(x, "x"), _f32(weight, "weight"), None if bias is None else _f32(bias, "bias"))


class _Relu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor):
        ctx.save_for_backward(x)
        return hip.relu(x)

    @staticmethod
    def backward(ctx, g: Tensor):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            g = _f32(g, "grad")
            _lib.check(_lib.load().manner_hip_relu_backward(hip._ptr(x), hip._ptr(g), hip._ptr(dx), x.numel(), hip._stream()))
        return dx


def relu(x: Tensor) -> Tensor:
    """F.relu with autograd (CAUMCategoryEncoder, news_encoder.py:353)."""
    return _Relu.apply(_f32(x, "x"))


class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids: Tensor, table: Tensor, padding_idx: int):
        out = torch.empty(tuple(ids.shape) + (table.shape[1],), dtype=torch.float32, device=table.device)
        with torch.cuda.device(table.device):
            _lib.check(_lib.load().manner_hip_embedding(hip._ptr(ids), ids.numel(), hip._ptr(table), table.shape[0], table.shape[1], hip._ptr(out),
                                                        hip._ptr(hip.device_status(table.device).word), hip._stream()))
        ctx.save_for_backward(ids)
        ctx.shape, ctx.padding_idx = tuple(table.shape), padding_idx
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        (ids,) = ctx.saved_tensors
        dt = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            g = _f32(g, "grad")
            _lib.check(_lib.load().manner_hip_embedding_backward(hip._ptr(ids), ids.numel(), hip._ptr(g), ctx.shape[0], ctx.shape[1],
                                                                 -1 if ctx.padding_idx is None else int(ctx.padding_idx), hip._ptr(dt), hip._stream()))
        return None, dt, None


def embedding(ids: Tensor, table: Tensor, padding_idx: Optional[int] = None) -> Tensor:
    """nn.Embedding lookup with autograd (row ``padding_idx`` receives no gradient)."""
    return _Embedding.apply(hip._dev(ids, torch.int64, "ids").contiguous(), _f32(table, "embedding.weight"), padding_idx)


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, p: float, seed: int, site: int):
        ctx.args = (p, seed, site)
        return _Dropout._run(x, p, seed, site)

    @staticmethod
    def _run(x, p, seed, site):
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().manner_hip_dropout(hip._ptr(x), hip._ptr(out), x.numel(), C.c_uint64(seed), C.c_uint32(site), C.c_float(p), hip._stream()))
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        return _Dropout._run(_f32(g, "grad"), *ctx.args), None, None, None


def dropout(x: Tensor, p: float, seed: int, site: int = 0) -> Tensor:
    """nn.Dropout in train() mode on the training path's counter-based generator (mask = f(seed, site, element index))."""
    if p <= 0.0:
        return x
    return _Dropout.apply(_f32(x, "x"), float(p), int(seed) & (2 ** 64 - 1), int(site))


class _SupConEmbeddings(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb: Tensor, labels: Tensor, temperature: float):
        n, d = emb.shape
        lib = _lib.load()
        losses = torch.empty(n, dtype=torch.float32, device=emb.device)
        red = torch.empty(2, dtype=torch.float32, device=emb.device)
        grad = torch.empty_like(emb)
        with torch.cuda.device(emb.device):
            need = int(lib.manner_hip_supcon_embeddings_workspace_bytes(n))
            ws = torch.empty(need, dtype=torch.uint8, device=emb.device)
            _lib.check(lib.manner_hip_supcon_embeddings(hip._ptr(emb), hip._ptr(labels), n, d, C.c_float(temperature), hip._ptr(losses), hip._ptr(red),
                                                        hip._ptr(grad), hip._ptr(ws), need, hip._stream()))
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(losses)
        return red[0], losses

    @staticmethod
    def backward(ctx, g: Tensor, _g_losses):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def supcon_embedding_loss(embeddings: Tensor, labels: Tensor, temperature: float = 0.1):
    """The A-Module's criterion (a_module.py:73-75,102-108: pytorch_metric_learning SupConLoss with an un-normalised dot-product
    similarity) on news embeddings [N, D] and aspect labels [N], with autograd.  Returns (batch loss, per-anchor losses)."""
    emb = hip._dev(embeddings, torch.float32, "embeddings").contiguous()
    lab = hip._dev(labels, torch.int64, "labels").contiguous()
    if emb.dim() != 2 or lab.shape != (emb.shape[0],):
        raise ValueError("supcon_embedding_loss: embeddings [N, D], labels [N]")
    return _SupConEmbeddings.apply(emb, lab, float(temperature))
