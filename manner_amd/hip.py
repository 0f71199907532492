"""Torch-tensor front end of the C ABI: pointer/stream plumbing only.

PyTorch-ROCm provides device memory and the current HIP stream; all arithmetic happens in
libmanner_hip.so.  Every function raises on non-GPU tensors — there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .config import EncoderConfig
from .weights import canonical_weights, plm_param_shapes

Tensor = torch.Tensor


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t: Tensor, dtype: torch.dtype, name: str) -> Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor — the MANNeR HIP hot path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


def _ptr(t: Optional[Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


# ------------------------------------------------------------------ device-side input validation
_STATUS_TEXT = {_lib.STATUS_MASK: "attention_mask is not a right-padded 0/1 prefix mask",
                _lib.STATUS_TOKEN: "input id / position outside the embedding tables",
                _lib.STATUS_INDEX: "news, entity, user or impression index outside the table (IndexError in the reference)",
                _lib.STATUS_LENGTHS: "host_lengths disagree with attention_mask, or a batch's offsets with the data set, or a history "
                                       "length outside [1, S] (pack_padded_sequence raises in the reference)"}


def _status_message(flag: int) -> str:
    return "; ".join(t for b, t in _STATUS_TEXT.items() if flag & b) or f"device status 0x{flag:x}"


class _FlagRing:
    """Snapshots of a device status word in a small ring of pinned host slots, each behind an event: ``completed()``
    returns the OR of the snapshots whose copy has finished, without ever blocking."""

    SLOTS = 32

    def __init__(self):
        self._host = torch.zeros(self.SLOTS, dtype=torch.int32).pin_memory()
        self._pending = []                     # (slot, event), oldest first
        self._next = 0

    def slot(self):
        """-> (flags carried over from a recycled slot, pinned one-element view to copy the word into)."""
        carried = 0
        i = self._next
        self._next = (i + 1) % self.SLOTS
        for j, (sl, ev) in enumerate(self._pending):
            if sl == i:                        # the slot comes round again before its snapshot was consumed: take it now
                ev.synchronize()
                carried = int(self._host[sl])
                del self._pending[j]
                break
        return carried, i, self._host[i:i + 1]

    def push(self, i: int) -> None:
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((i, ev))

    def completed(self, wait: bool = False) -> int:
        """OR of the finished snapshots.  ``wait``: block for all of them.  Otherwise every snapshot EXCEPT the newest is waited for
        (those copies were enqueued at least one call earlier — behind work the device has long finished or is about to —
        so a raised bit surfaces at the call after next at the latest instead of "whenever the event happens to have completed");
        the newest is taken only if it has already completed, so the host still runs one call ahead of the device."""
        flag, keep = 0, []
        last = len(self._pending) - 1
        for j, (i, ev) in enumerate(self._pending):
            if wait or j < last:
                ev.synchronize()
            if wait or j < last or ev.query():
                flag |= int(self._host[i])
            else:
                keep.append((i, ev))
        self._pending = keep
        return flag


class DeviceStatus:
    """The int32 status word the scoring kernels raise bits in (``MANNER_HIP_STATUS_*``) where the reference would
    raise an exception (an out-of-range table index).  ``check()`` is blocking; ``poll()`` never is: every ``arm()``
    enqueues a copy of the word into pinned host memory and an event, and ``poll()`` raises for the snapshots that have
    completed, waiting for every one but the newest — so a bad batch surfaces at the next call when the device has kept up,
    at the call after next at the latest, and the host never waits for the call it has just enqueued."""

    def __init__(self, device: torch.device):
        self.device = device
        self.word = torch.zeros(1, dtype=torch.int32, device=device)
        self._ring = _FlagRing()
        self._carry = 0

    def arm(self) -> None:
        with torch.cuda.device(self.device):
            carried, i, host = self._ring.slot()
            self._carry |= carried
            host.copy_(self.word, non_blocking=True)
            self.word.zero_()
            self._ring.push(i)

    def _raise(self, flag: int) -> None:
        flag |= self._carry
        self._carry = 0
        if flag:
            raise RuntimeError(f"manner_hip input error: {_status_message(flag)}")

    def poll(self) -> None:
        self._raise(self._ring.completed())

    def check(self) -> None:
        flag = int(self.word.item())           # synchronises with the kernels that may still raise bits
        self.word.zero_()
        self._raise(flag | self._ring.completed(wait=True))


_status: Dict[str, DeviceStatus] = {}


def device_status(device) -> DeviceStatus:
    key = str(torch.device(device))
    if key not in _status:
        _status[key] = DeviceStatus(torch.device(device))
    return _status[key]


def check_status(device=None) -> None:
    """Blocking: raise if any scoring / entity kernel on ``device`` (default: every device used so far) saw an
    out-of-range index since the last check."""
    for st in ([device_status(device)] if device is not None else list(_status.values())):
        st.check()


def status_poll(device) -> None:
    """Non-blocking: raise for every armed snapshot of ``device``'s status word whose copy has completed.  The composed
    entry points (hotpath.*, train.encode_train, the module mirrors) call this on the way in and ``status_arm`` on the
    way out, so an out-of-range index / a token_bound below the mask's token count surfaces at the next call when the device
    has kept up and at the call AFTER next at the latest (every snapshot but the newest is waited for) — the host still runs one
    call ahead of the device; ``check_status`` is the blocking form, to be called when a loop ends (epoch end)."""
    device_status(device).poll()


def status_arm(device) -> None:
    device_status(device).arm()


def weight_table_order(cfg: EncoderConfig) -> Sequence[str]:
    """HF parameter names in the order of the ``weights`` table of manner_hip_encoder_create."""
    names = ["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
             "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    per_layer = ["attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight",
                 "attention.self.key.bias", "attention.self.value.weight", "attention.self.value.bias",
                 "attention.output.dense.weight", "attention.output.dense.bias",
                 "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias",
                 "intermediate.dense.weight", "intermediate.dense.bias", "output.dense.weight",
                 "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias"]
    for l in range(cfg.layers):
        names += [f"encoder.layer.{l}.{n}" for n in per_layer]
    return names


class HipEncoder:
    """Owns a manner_hip_encoder handle (packed PLM weights) and a growable workspace."""

    def __init__(self, cfg: EncoderConfig, weights: Dict[str, Tensor], precisions: Sequence[str] = ("bf16", "fp32"),
                 device: Optional[torch.device] = None):
        lib = _lib.load()
        self.cfg = cfg
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("HipEncoder needs a GPU device — there is no CPU fallback")
        weights = canonical_weights(cfg, weights)           # DistilBERT names -> BERT names (+ zero token-type row)
        shapes = dict(plm_param_shapes(cfg if cfg.naming == "bert" else EncoderConfig(**{**cfg.to_dict(), "naming": "bert"})))
        names = weight_table_order(cfg)
        keep = []
        with torch.cuda.device(self.device):
            for n in names:
                w = weights[n]
                if isinstance(w, np.ndarray):
                    w = torch.from_numpy(w)
                w = w.detach().to(device=self.device, dtype=torch.float32).contiguous()
                if tuple(w.shape) != tuple(shapes[n]):
                    raise ValueError(f"{n}: shape {tuple(w.shape)} != {shapes[n]}")
                keep.append(w)
            table = (C.c_void_p * len(keep))(*[w.data_ptr() for w in keep])
            cc = _lib.EncoderConfigC(cfg.arch, cfg.hidden, cfg.layers, cfg.heads, cfg.intermediate, cfg.vocab,
                                     cfg.max_pos, cfg.type_vocab, cfg.pad_id, cfg.ln_eps)
            mask = 0
            for p in precisions:
                mask |= 1 << _lib.PRECISIONS[p]
            handle = C.c_void_p()
            _lib.check(lib.manner_hip_encoder_create(C.byref(cc), table, len(keep), mask, _stream(), C.byref(handle)))
        self._handle = handle
        self._ws: Optional[Tensor] = None
        self._ring: Optional[_FlagRing] = None
        self._carry = 0
        del keep                      # the handle owns private packed copies

    def close(self) -> None:
        if getattr(self, "_handle", None):
            _lib.load().manner_hip_encoder_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _workspace(self, n_news: int, tokens: int, prec: int) -> Tuple[Tensor, int]:
        """(buffer, bytes to hand to the library).  The library sizes its chunks from the BYTES it is given, so a buffer that an
        earlier call in a wider arithmetic left larger must not change this call's chunking (and with it the per-launch figures)."""
        need = int(_lib.load().manner_hip_encoder_workspace_bytes(self._handle, n_news, tokens, prec))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws, need

    def encode_cls(self, ids: Tensor, mask: Tensor, precision: str = "bf16",
                   host_lengths: Optional[np.ndarray] = None, max_chunk_tokens: int = 65536,
                   out: Optional[Tensor] = None) -> Tensor:
        """[N, Lp] int64 ids/mask -> [N, H] float32 CLS embeddings."""
        ids, mask = _dev(ids, torch.int64, "input_ids"), _dev(mask, torch.int64, "attention_mask")
        if ids.dim() != 2 or ids.shape != mask.shape:
            raise ValueError(f"input_ids {tuple(ids.shape)} / attention_mask {tuple(mask.shape)} must be equal 2-D")
        ids, mask = ids.contiguous(), mask.contiguous()
        n, lp = ids.shape
        prec = _lib.PRECISIONS[precision]
        if out is None:
            out = torch.empty((n, self.cfg.hidden), dtype=torch.float32, device=ids.device)
        else:
            _dev(out, torch.float32, "out")
            assert out.is_contiguous() and tuple(out.shape) == (n, self.cfg.hidden)
        if n == 0:
            return out
        hl = None
        if host_lengths is not None:
            hl = np.ascontiguousarray(host_lengths, dtype=np.int32)
            assert hl.shape == (n,)
            tokens = min(int(hl.sum()), max_chunk_tokens)
        else:
            tokens = min(n * lp, max_chunk_tokens)
        tokens = max(tokens, lp, 256)
        with torch.cuda.device(ids.device):
            ws, ws_bytes = self._workspace(min(n, tokens), tokens, prec)
            _lib.check(_lib.load().manner_hip_encode_cls(
                self._handle, _ptr(ids), _ptr(mask), C.c_void_p(hl.ctypes.data if hl is not None else 0), n, lp, prec,
                _ptr(out), _ptr(ws), ws_bytes, _stream()))
        return out

    def encode_hidden(self, ids: Tensor, mask: Tensor, n_layers: int, precision: str = "bf16",
                      out_dtype: torch.dtype = torch.float32, host_lengths: Optional[np.ndarray] = None,
                      max_chunk_tokens: int = 65536) -> Tensor:
        """HF ``hidden_states[n_layers]`` as [N, Lp, H] (zeros at padded positions): the cacheable output of the
        frozen layers (``frozen_layers: [0..7]`` -> ``n_layers=8``) for a training loop that only updates the rest."""
        ids, mask = _dev(ids, torch.int64, "input_ids"), _dev(mask, torch.int64, "attention_mask")
        if ids.dim() != 2 or ids.shape != mask.shape:
            raise ValueError(f"input_ids {tuple(ids.shape)} / attention_mask {tuple(mask.shape)} must be equal 2-D")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("out_dtype must be float32 or bfloat16")
        ids, mask = ids.contiguous(), mask.contiguous()
        n, lp = ids.shape
        prec = _lib.PRECISIONS[precision]
        out = torch.empty((n, lp, self.cfg.hidden), dtype=out_dtype, device=ids.device)
        if n == 0:
            return out
        hl = None
        if host_lengths is not None:
            hl = np.ascontiguousarray(host_lengths, dtype=np.int32)
            assert hl.shape == (n,)
            tokens = min(int(hl.sum()), max_chunk_tokens)
        else:
            tokens = min(n * lp, max_chunk_tokens)
        tokens = max(tokens, lp, 256)
        with torch.cuda.device(ids.device):
            ws, ws_bytes = self._workspace(min(n, tokens), tokens, prec)
            _lib.check(_lib.load().manner_hip_encode_hidden(
                self._handle, _ptr(ids), _ptr(mask), C.c_void_p(hl.ctypes.data if hl is not None else 0), n, lp, prec,
                int(n_layers), 0 if out_dtype == torch.float32 else 1, _ptr(out), _ptr(ws), ws_bytes, _stream()))
        return out

    def profile(self, enable: bool) -> None:
        """Bracket every launch of encode_cls with HIP events on the launch stream (opt-in)."""
        _lib.check(_lib.load().manner_hip_encoder_profile(self._handle, int(enable)))

    def profile_read(self) -> Dict[str, Tuple[float, int]]:
        """{kernel class: (total ms, launches)} accumulated since the last read; synchronises."""
        n = len(_lib.PROF_CLASSES)
        ms, cnt = (C.c_double * n)(), (C.c_int64 * n)()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().manner_hip_encoder_profile_read(self._handle, _stream(), ms, cnt))
        return {c: (ms[i], cnt[i]) for i, c in enumerate(_lib.PROF_CLASSES)}

    def status(self) -> None:
        """Blocking check of the device-side input validation flag (raises on bad masks/ids)."""
        carried = 0
        if self._ring is not None:
            carried = self._ring.completed(wait=True) | self._carry
            self._carry = 0
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().manner_hip_encoder_status(self._handle, _stream()))
        if carried:
            raise RuntimeError(f"manner_hip input error in an earlier encode call: {_status_message(carried)}")

    def status_arm(self) -> None:
        """Non-blocking: snapshot (and reset) the flag word into pinned host memory behind an event on the current
        stream; ``status_poll`` raises for completed snapshots.  The module mirror calls both around every forward."""
        if self._ring is None:
            self._ring = _FlagRing()
        with torch.cuda.device(self.device):
            carried, i, host = self._ring.slot()
            self._carry |= carried
            _lib.check(_lib.load().manner_hip_encoder_status_async(self._handle, C.c_void_p(host.data_ptr()), _stream()))
            self._ring.push(i)

    def status_poll(self) -> None:
        flag = self._carry | (self._ring.completed() if self._ring is not None else 0)
        self._carry = 0
        if flag:
            raise RuntimeError(f"manner_hip input error in an earlier encode call: {_status_message(flag)}")


class WeightFingerprint:
    """Tripwire for writes autograd's version counters cannot see (``p.data.mul_(2)``, ``p.data.copy_(ema)``: the ``.data`` alias has a
    version counter of its own) under a host that caches packed copies of the parameters — the module mirror's inference handle.

    One launch of ``manner_hip_fingerprint`` hashes up to ``SAMPLES`` evenly strided words of every tensor into one word per tensor.
    ``baseline`` is taken (blocking) when the packed copies are made; ``arm()`` enqueues a fresh fingerprint and its copy into a pinned
    slot behind an event, ``changed()`` compares the snapshots that have completed — every one but the newest is waited for, as
    ``_FlagRing`` does for the status word — so a bulk rewrite surfaces at the next call when the device has kept up and at the call
    after next at the latest, with no host synchronisation per forward; ``changed_now()`` is the blocking form.  A poke into single
    elements between the samples is not seen: documented limit, ``MannerTextEncoder.invalidate()`` is the exact tool."""

    SAMPLES = 1024
    SLOTS = 8

    def __init__(self, tensors: Sequence[Tensor], device: torch.device):
        self.device = torch.device(device)
        self._keep = [t for t in tensors]
        n = len(self._keep)
        # (normal tensors even when the first forward runs under inference_mode: they are updated in place by later no_grad calls)
        with torch.inference_mode(False), torch.cuda.device(self.device):
            self._ptrs = torch.tensor([t.data_ptr() for t in self._keep], dtype=torch.int64, device=self.device)
            self._counts = torch.tensor([t.numel() * t.element_size() // 4 for t in self._keep], dtype=torch.int64, device=self.device)
            self._out = torch.empty(n, dtype=torch.int32, device=self.device)
            self._host = torch.zeros((self.SLOTS, n), dtype=torch.int32).pin_memory()
        self._pending: list = []
        self._next = 0
        self.baseline = self._blocking()

    def _launch(self) -> None:
        _lib.check(_lib.load().manner_hip_fingerprint(_ptr(self._ptrs), _ptr(self._counts), len(self._keep), self.SAMPLES, _ptr(self._out), _stream()))

    def _blocking(self) -> Tensor:
        with torch.cuda.device(self.device):
            self._launch()
            return self._out.cpu()

    def changed_now(self) -> bool:
        return not torch.equal(self._blocking(), self.baseline)

    def arm(self) -> None:
        with torch.cuda.device(self.device):
            i = self._next
            self._next = (i + 1) % self.SLOTS
            stale = False
            for j, (sl, ev) in enumerate(self._pending):
                if sl == i:                    # the slot comes round before its snapshot was looked at: look now
                    ev.synchronize()
                    stale = not torch.equal(self._host[sl], self.baseline)
                    del self._pending[j]
                    break
            self._carry = getattr(self, "_carry", False) or stale
            self._launch()
            self._host[i].copy_(self._out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending.append((i, ev))

    def changed(self) -> bool:
        hit, keep = getattr(self, "_carry", False), []
        self._carry = False
        last = len(self._pending) - 1
        for j, (i, ev) in enumerate(self._pending):
            if j < last:
                ev.synchronize()
            if j < last or ev.query():
                hit = hit or not torch.equal(self._host[i], self.baseline)
            else:
                keep.append((i, ev))
        self._pending = keep
        return hit


class NewsEmbeddingCache:
    """Content-addressed table of text-encoder outputs (csrc/cache.hip; SURVEY.md §8d mode T behind the drop-in call pattern).

    ``lookup(ids, mask)`` keys every row by its real tokens and returns (rows int32 [N], state int32 [N]): state 0 — the embedding is
    (or, for a repeat of a key new in this call, will be) at ``table[rows]``; 1 — new, the caller encodes it and stores it at
    ``table[rows]``; 2 — encode, do not store (table full).  Everything lives in HBM: ``capacity`` rows of ``dim`` f32 plus
    2 x capacity hash slots of 20 bytes (161 013 news x 768 f32 = 495 MB — the whole MIND-large table fits 500 times over).
    The owner clears it whenever the weights or the arithmetic mode change."""

    def __init__(self, dim: int, capacity: int, device: torch.device, zero: bool = False):
        if capacity < 1:
            raise ValueError("NewsEmbeddingCache: capacity must be positive")
        self.dim, self.capacity, self.device = int(dim), int(capacity), torch.device(device)
        n_slots = 2
        while n_slots < 2 * self.capacity:
            n_slots *= 2
        self.n_slots = n_slots
        # ordinary tensors even when the first forward runs under torch.inference_mode() (Lightning's test loop): an inference
        # tensor could not be updated in place by a later call under no_grad
        with torch.inference_mode(False):
            self.table = (torch.zeros if zero else torch.empty)((self.capacity, self.dim), dtype=torch.float32, device=self.device)
            self.slot_keys = torch.zeros((2, n_slots), dtype=torch.int64, device=self.device)     # uint64 bit patterns
            self.slot_rows = torch.full((n_slots,), -1, dtype=torch.int32, device=self.device)
            self.row_count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.lookups = 0          # host-side counters (rows asked for / rows encoded), for the hit rate
        self.encoded = 0

    def clear(self) -> None:
        self.slot_keys.zero_()
        self.slot_rows.fill_(-1)
        self.row_count.zero_()
        self.lookups = self.encoded = 0

    def keys(self, ids: Tensor, mask: Tensor) -> Tensor:
        ids = _dev(ids, torch.int64, "input_ids").contiguous()
        mask = _dev(mask, torch.int64, "attention_mask").contiguous()
        if ids.dim() != 2 or ids.shape != mask.shape:
            raise ValueError("NewsEmbeddingCache: input_ids / attention_mask must be [n_news, padded_len]")
        out = torch.empty((ids.shape[0], 2), dtype=torch.int64, device=ids.device)
        with torch.cuda.device(ids.device):
            _lib.check(_lib.load().manner_hip_news_key128(_ptr(ids), _ptr(mask), ids.shape[0], ids.shape[1], _ptr(out), _stream()))
        return out

    def lookup(self, ids: Tensor, mask: Tensor) -> Tuple[Tensor, Tensor]:
        keys = self.keys(ids, mask)
        n = keys.shape[0]
        rows = torch.empty(n, dtype=torch.int32, device=keys.device)
        state = torch.empty(n, dtype=torch.int32, device=keys.device)
        scratch = torch.empty(2 * max(n, 1), dtype=torch.int32, device=keys.device)
        with torch.cuda.device(keys.device):
            _lib.check(_lib.load().manner_hip_news_cache_lookup(_ptr(keys), n, _ptr(self.slot_keys), _ptr(self.slot_rows), self.n_slots,
                                                                 _ptr(self.row_count), self.capacity, _ptr(rows), _ptr(state), _ptr(scratch),
                                                                 _stream()))
        return rows, state


class PrefixCache(NewsEmbeddingCache):
    """The same table with one row = the hidden states of a news after the frozen layers, [max_len, hidden] f32, zeros at padded
    positions ("activations after layer 7 are constant across epochs").  65 238 news x 96 tokens x 768 f32 =
    19.2 GB, 161 013 news = 47.5 GB: HBM the MI355X has to spare."""

    def __init__(self, hidden: int, max_len: int, capacity: int, device: torch.device):
        super().__init__(int(hidden) * int(max_len), capacity, device, zero=True)
        self.hidden, self.max_len = int(hidden), int(max_len)

    def clear(self) -> None:
        super().clear()
        self.table.zero_()                  # a row stored at a narrower padded width must read zeros beyond it

    def hidden_states(self, engine: "HipEncoder", ids: Tensor, mask: Tensor, n_layers: int, precision: str) -> Tensor:
        """``engine.encode_hidden(ids, mask, n_layers)`` [N, Lp, H] f32 with every row whose tokens were seen before taken from the table
        (bit-identical: a row's hidden states do not depend on the other rows of the call).  Wider batches than ``max_len`` bypass it."""
        n, lp = ids.shape
        if lp > self.max_len or n == 0:
            return engine.encode_hidden(ids, mask, n_layers, precision=precision)
        try:
            rows, state = self.lookup(ids, mask)
            todo = torch.nonzero(state != 0).squeeze(1)                          # one host read: how many rows are new
            self.lookups += int(n)
            self.encoded += int(todo.numel())
            tbl = self.table.view(self.capacity, self.max_len, self.hidden)
            fresh = None
            if todo.numel():
                fresh = engine.encode_hidden(ids.index_select(0, todo), mask.index_select(0, todo), n_layers, precision=precision)
                if todo.numel() == n and not bool((state == 1).any()):
                    return fresh
                keep = state.index_select(0, todo) == 1
                tbl[rows.index_select(0, todo)[keep].long(), :lp] = fresh[keep]
                if todo.numel() == n:
                    return fresh
            out = tbl[rows.clamp_min(0).long(), :lp]                             # gather: a new [N, Lp, H] tensor
            if fresh is not None:
                out.index_copy_(0, todo, fresh)                                  # rows that could not be stored
            return out
        except BaseException:                  # also KeyboardInterrupt / SystemExit: the table is torch.empty, a claimed key must not survive
            self.clear()
            raise


def _hash_slots(capacity_rows: int) -> int:
    n_slots = 2
    while n_slots < 2 * int(capacity_rows):
        n_slots *= 2
    return n_slots


def prefix_cache_bytes(hidden: int, capacity_rows: int, pool_tokens: Optional[int] = None, max_len: Optional[int] = None) -> Dict[str, int]:
    """Device bytes of a frozen-prefix cache, by part.  ``pool_tokens``: a ``PackedPrefixCache`` — payload pool_tokens x hidden f32,
    16 bytes of row metadata per row (token offset int64, token count and a scratch word int32) + the 8-byte token counter;
    ``max_len``: a ``PrefixCache`` — payload capacity_rows x max_len x hidden f32.  Both: hash slots of 20 bytes (128-bit key +
    row), twice the rows rounded up to a power of two, + the 4-byte row counter."""
    if (pool_tokens is None) == (max_len is None):
        raise ValueError("prefix_cache_bytes: give pool_tokens (packed) or max_len (padded)")
    slots = _hash_slots(capacity_rows) * 20 + 4
    if pool_tokens is not None:
        payload, rows = int(pool_tokens) * int(hidden) * 4, int(capacity_rows) * 16 + 8
    else:
        payload, rows = int(capacity_rows) * int(max_len) * int(hidden) * 4, 0
    return {"payload": payload, "rows": rows, "slots": slots, "total": payload + rows + slots}


class PackedPrefixCache(NewsEmbeddingCache):
    """``PrefixCache`` with the payload kept by REAL tokens (csrc/cache.hip, manner_hip_prefix_*): a news costs len x hidden f32 in a
    pool of ``pool_tokens`` token rows instead of a fixed max_len x hidden row, and a batch of any padded width up to
    ``_lib.MAX_LEN_INFER`` (512) is served — a payload stored at one width gathers into any other that holds the row.  With the
    title+abstract profile of ``synth.synth_lengths`` capped at 512 (65 238 news, seed 42) the pool needs 5 863 594 tokens, 89.9 per
    news (276 KB): ``prefix_cache_bytes(768, 65238, 5863594)`` is 18.02 GB against 102.61 GB for rows of 512 — 5.70x less
    (161 013 news: 44.4 GB against 253.3 GB).  When the pool is full a news keeps
    its key but gets no payload: it is encoded at every call, as with a full table.  Store and gather are HIP copies of the real
    tokens; the one host read is the count of rows to encode."""

    def __init__(self, hidden: int, capacity_rows: int, pool_tokens: int, device: torch.device, pool: Optional[Tensor] = None):
        if int(pool_tokens) < 1 or int(hidden) % 4:
            raise ValueError("PackedPrefixCache: pool_tokens must be positive and hidden a multiple of 4")
        super().__init__(0, capacity_rows, device)                 # keys, hash slots and row numbers; no fixed-width table
        self.hidden, self.pool_tokens, self.max_len = int(hidden), int(pool_tokens), _lib.MAX_LEN_INFER
        with torch.inference_mode(False):
            if pool is None:
                pool = torch.empty((self.pool_tokens, self.hidden), dtype=torch.float32, device=self.device)
            if pool.dtype != torch.float32 or tuple(pool.shape) != (self.pool_tokens, self.hidden) or not pool.is_contiguous() \
                    or pool.device != self.table.device or pool.data_ptr() % 16:
                raise ValueError("PackedPrefixCache: pool must be a contiguous, 16-byte aligned f32 [pool_tokens, hidden] on the device")
            self.pool = pool
            self.row_off = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
            self.row_len = torch.full((self.capacity,), -1, dtype=torch.int32, device=self.device)
            self.row_src = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
            self.tok_count = torch.zeros(1, dtype=torch.int64, device=self.device)                # uint64 bit pattern

    def clear(self) -> None:
        super().clear()
        self.row_len.fill_(-1)
        self.tok_count.zero_()

    def hidden_states(self, engine: "HipEncoder", ids: Tensor, mask: Tensor, n_layers: int, precision: str) -> Tensor:
        """``engine.encode_hidden(ids, mask, n_layers)`` [N, Lp, H] f32 with every row whose tokens were seen before (and fitted the
        pool) gathered from the pool — the same bits, zeros at padded positions.  Only batches wider than 512 bypass it."""
        n, lp = ids.shape
        if lp > self.max_len or n == 0:
            return engine.encode_hidden(ids, mask, n_layers, precision=precision)
        try:
            lib = _lib.load()
            rows, state = self.lookup(ids, mask)
            with torch.cuda.device(rows.device):
                _lib.check(lib.manner_hip_prefix_resolve(_ptr(rows), _ptr(state), n, _ptr(self.row_len), self.capacity, _stream()))
            todo = torch.nonzero(state != 0).squeeze(1)                          # one host read: how many rows are new
            self.lookups += int(n)
            self.encoded += int(todo.numel())
            fresh, n_fresh = None, int(todo.numel())
            src_of = torch.empty(n, dtype=torch.int32, device=rows.device)
            if n_fresh:
                whole = n_fresh == n
                fresh = engine.encode_hidden(ids if whole else ids.index_select(0, todo), mask if whole else mask.index_select(0, todo),
                                             n_layers, precision=precision)
                lens = mask.sum(1, dtype=torch.int32)
                with torch.cuda.device(rows.device):
                    _lib.check(lib.manner_hip_prefix_store(_ptr(fresh), n_fresh, _ptr(None if whole else todo), n, _ptr(rows), _ptr(state),
                                                           _ptr(lens), lp, self.hidden, _ptr(self.pool), self.pool_tokens, self.capacity,
                                                           _ptr(self.row_off), _ptr(self.row_len), _ptr(self.row_src),
                                                           _ptr(self.tok_count), _ptr(src_of), _stream()))
                if whole:
                    return fresh
            out = torch.empty((n, lp, self.hidden), dtype=torch.float32, device=rows.device)
            with torch.cuda.device(rows.device):
                _lib.check(lib.manner_hip_prefix_gather(_ptr(rows), _ptr(state), n, lp, self.hidden, _ptr(self.pool), self.pool_tokens,
                                                        self.capacity, _ptr(self.row_off), _ptr(self.row_len), _ptr(self.row_src),
                                                        _ptr(fresh), n_fresh, _ptr(src_of), _ptr(out), _stream()))
            return out
        except BaseException:                  # a claimed key without its payload must not survive
            self.clear()
            raise


def additive_pool(x: Tensor, lin_w: Tensor, lin_b: Tensor, query: Tensor, strict: bool = False) -> Tensor:
    """AdditiveAttention.forward (reference attention.py:21-27).  Default: the one-pass kernel where the shape allows it (D = 768,
    S <= 128, Q <= 320) — x read once and kept on the CU as power-of-two-scaled IEEE-half hi/lo pairs, logits as split (x3) products
    on the f16 matrix pipe, tanh by exp/rcp: pooled vectors within 1e-4 of the reference (measured 2e-7 on the goldens, 1.1e-5 on a
    peaked-softmax stress input; csrc/pool.hip).  ``strict=True`` (or MANNER_HIP_POOL_STRICT=1): the exact-f32 two-pass path (f32
    matrix pipe logits + apply), which train() mode always uses."""
    x = _dev(x, torch.float32, "input_vector").contiguous()
    b, s, d = x.shape
    lin_w = _dev(lin_w, torch.float32, "linear.weight").contiguous()
    lin_b = _dev(lin_b, torch.float32, "linear.bias").contiguous()
    query = _dev(query, torch.float32, "query").contiguous()
    q = lin_w.shape[0]
    assert lin_w.shape == (q, d) and lin_b.shape == (q,) and query.shape == (q,)
    out = torch.empty((b, d), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    nbytes = int(lib.manner_hip_additive_pool_workspace_bytes(b, s, d, q))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=x.device)
    off = (-ws.data_ptr()) % 256
    with torch.cuda.device(x.device):
        _lib.check(lib.manner_hip_additive_pool_fused(_ptr(x), _ptr(lin_w), _ptr(lin_b), _ptr(query), b, s, d, q, _ptr(out),
                                                      ws.data_ptr() + off, nbytes, 1 if strict else 0, _stream()))
    return out


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    """nn.Linear forward on f32 rows: x [R, K] -> [R, O]."""
    x = _dev(x, torch.float32, "input").contiguous()
    weight = _dev(weight, torch.float32, "weight").contiguous()
    r, k = x.shape
    o = weight.shape[0]
    assert weight.shape[1] == k
    if bias is not None:
        bias = _dev(bias, torch.float32, "bias").contiguous()
    y = torch.empty((r, o), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().manner_hip_linear(_ptr(x), _ptr(weight), _ptr(bias), r, k, o, _ptr(y), _stream()))
    return y


def entity_encode(entity_ids: Tensor, table: Tensor, in_proj_w: Tensor, in_proj_b: Tensor, out_proj_w: Tensor,
                  out_proj_b: Tensor, pool_w: Tensor, pool_b: Tensor, pool_q: Tensor, heads: int) -> Tensor:
    """MannerEntityEncoder.forward (eval), batch-faithful to the reference: [N, E] ids -> [N, D]."""
    ids = _dev(entity_ids, torch.int64, "entities").contiguous()
    n, e = ids.shape
    ts = [_dev(t, torch.float32, nm).contiguous() for t, nm in
          ((table, "pretrained_embedding.weight"), (in_proj_w, "in_proj_weight"), (in_proj_b, "in_proj_bias"),
           (out_proj_w, "out_proj.weight"), (out_proj_b, "out_proj.bias"), (pool_w, "linear.weight"),
           (pool_b, "linear.bias"), (pool_q, "query"))]
    d, q = ts[0].shape[1], ts[5].shape[0]
    out = torch.empty((n, d), dtype=torch.float32, device=ids.device)
    if n == 0:
        return out
    lib = _lib.load()
    need = int(lib.manner_hip_entity_workspace_bytes(n, e, d))
    ws = torch.empty(need, dtype=torch.uint8, device=ids.device)
    with torch.cuda.device(ids.device):
        _lib.check(lib.manner_hip_entity_encode(_ptr(ids), n, e, _ptr(ts[0]), ts[0].shape[0], d, heads, _ptr(ts[1]), _ptr(ts[2]),
                                                _ptr(ts[3]), _ptr(ts[4]), _ptr(ts[5]), _ptr(ts[6]), _ptr(ts[7]), q, _ptr(out),
                                                _ptr(ws), need, _ptr(device_status(ids.device).word), _stream()))
    return out


def mha_axis0(x: Tensor, in_proj_w: Tensor, in_proj_b: Tensor, out_proj_w: Tensor, out_proj_b: Tensor, heads: int) -> Tensor:
    """nn.MultiheadAttention(batch_first=False) exactly as the reference calls it on a [batch, seq, E] tensor without masks
    (PLMTextEncoder news_encoder.py:163-165, NRMSUserEncoder user_encoder.py:35-37): attention along AXIS 0 of x [L0, B1, E]."""
    x = _dev(x, torch.float32, "x").contiguous()
    l0, b1, e = x.shape
    ts = [_dev(t, torch.float32, nm).contiguous() for t, nm in ((in_proj_w, "in_proj_weight"), (in_proj_b, "in_proj_bias"),
                                                                (out_proj_w, "out_proj.weight"), (out_proj_b, "out_proj.bias"))]
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    lib = _lib.load()
    need = int(lib.manner_hip_mha_axis0_workspace_bytes(l0, b1, e))
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.manner_hip_mha_axis0(_ptr(x), l0, b1, e, heads, _ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), _ptr(ts[3]), _ptr(out),
                                            _ptr(ws), need, _stream()))
    return out


def encode_full(cfg: EncoderConfig, weights: Dict[str, Tensor], ids: Tensor, mask: Tensor, precision: str = "fp32") -> Tensor:
    """HF ``last_hidden_state`` [N, Lp, H] f32 INCLUDING the padded positions (what PLMTextEncoder consumes); ``weights`` is the
    HF-named dict of float32 GPU tensors, read in place.  ``Lp <= _lib.MAX_LEN_FULL`` (512), every position within the model's
    position table; in f16 / bf16 a batch of more than 128 positions runs the long-row matrix-pipe attention."""
    if precision not in ("fp32", "f16", "bf16"):
        raise ValueError("encode_full precision: fp32, f16 or bf16")
    ids, mask = _dev(ids, torch.int64, "input_ids").contiguous(), _dev(mask, torch.int64, "attention_mask").contiguous()
    if ids.dim() != 2 or ids.shape != mask.shape:
        raise ValueError(f"input_ids {tuple(ids.shape)} / attention_mask {tuple(mask.shape)} must be equal 2-D")
    if ids.shape[1] > _lib.MAX_LEN_FULL:
        raise RuntimeError(f"encode_full: padded_len={ids.shape[1]} (padded_len <= {_lib.MAX_LEN_FULL})")
    canon = canonical_weights(cfg, weights)
    table = [_dev(canon[n].detach(), torch.float32, n).contiguous() for n in weight_table_order(cfg)]
    n, lp = ids.shape
    out = torch.empty((n, lp, cfg.hidden), dtype=torch.float32, device=ids.device)
    if n == 0:
        return out
    lib = _lib.load()
    cc = _lib.EncoderConfigC(cfg.arch, cfg.hidden, cfg.layers, cfg.heads, cfg.intermediate, cfg.vocab, cfg.max_pos, cfg.type_vocab,
                             cfg.pad_id, cfg.ln_eps)
    with torch.cuda.device(ids.device):
        need = int(lib.manner_hip_encode_full_workspace_bytes(C.byref(cc), n, lp))
        ws = torch.empty(need, dtype=torch.uint8, device=ids.device)
        tab = (C.c_void_p * len(table))(*[t.data_ptr() for t in table])
        _lib.check(lib.manner_hip_encode_full(C.byref(cc), tab, len(table), _ptr(ids), _ptr(mask), n, lp, _lib.PRECISIONS[precision],
                                              _ptr(out), _ptr(ws), need, _ptr(device_status(ids.device).word), _stream()))
    return out


def dot(user: Tensor, cand: Tensor) -> Tensor:
    """DotProduct contract: user [B,1,D], cand [B,D,C] (any strides, e.g. a permuted [B,C,D]) -> [B,C]."""
    user, cand = _dev(user, torch.float32, "clicked_news_vector"), _dev(cand, torch.float32, "candidate_news_vector")
    b, one, d = user.shape
    assert one == 1 and cand.shape[0] == b and cand.shape[1] == d
    c = cand.shape[2]
    u = user.reshape(b, d).contiguous()
    if c == 0:
        return torch.empty((b, 0), dtype=torch.float32, device=user.device)
    if min(cand.stride()) < 0 or (cand.stride(1) != 1 and cand.stride(2) != 1):
        cand = cand.contiguous()
    out = torch.empty((b, c), dtype=torch.float32, device=user.device)
    with torch.cuda.device(user.device):
        _lib.check(_lib.load().manner_hip_dot(_ptr(u), _ptr(cand), b, c, d, cand.stride(0), cand.stride(1),
                                              cand.stride(2), _ptr(out), _stream()))
    return out


def _workspace(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def _mask_bytes(mask: Tensor, shape, name: str) -> Tensor:
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor — the MANNeR HIP hot path has no CPU fallback")
    if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != tuple(shape):
        raise TypeError(f"{name}: expected bool or uint8 {tuple(shape)}, got {mask.dtype} {tuple(mask.shape)}")
    return mask.contiguous()


def poly_attention(x: Tensor, mask: Tensor, lin_w: Tensor, codes: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """PolyAttention.forward (reference attention.py:60-84): x [B, S, D], mask bool [B, S], linear.weight [Q, D], context_codes
    [K, Q], bias [B, S, T] or None -> [B, K, D].  A masked slot keeps the logit 1e-30 and the bias mean runs over all T columns,
    as in the reference.  S <= 256, K <= 64, Q <= 512, D <= 1024 (the library refuses anything else)."""
    x = _dev(x, torch.float32, "clicked_news_vector").contiguous()
    b, s, d = x.shape
    mask = _mask_bytes(mask, (b, s), "attn_mask")
    lin_w = _dev(lin_w, torch.float32, "linear.weight").contiguous()
    codes = _dev(codes, torch.float32, "context_codes").contiguous()
    q, k = lin_w.shape[0], codes.shape[0]
    assert lin_w.shape == (q, d) and codes.shape == (k, q)
    t = 0
    if bias is not None:
        bias = _dev(bias, torch.float32, "bias").contiguous()
        assert bias.dim() == 3 and bias.shape[:2] == (b, s)
        t = bias.shape[2]
    out = torch.empty((b, k, d), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        need = int(lib.manner_hip_poly_attention_workspace_bytes(b, s, d, q, k))
        ws = _workspace(need, x.device)
        _lib.check(lib.manner_hip_poly_attention(_ptr(x), _ptr(mask), _ptr(lin_w), _ptr(codes), _ptr(bias), t, b, s, d, q, k, _ptr(out),
                                                 _ptr(ws), need, _stream()))
    return out


def target_attention(query: Tensor, key: Tensor, value: Tensor, lin_w: Tensor) -> Tensor:
    """TargetAwareAttention.forward (reference attention.py:102-116): query [B, K, D], key [B, C, D], value [B, C, K],
    linear.weight [D, D] -> [B, C].  K <= 64, D <= 1024."""
    query = _dev(query, torch.float32, "query").contiguous()
    key = _dev(key, torch.float32, "key").contiguous()
    value = _dev(value, torch.float32, "value").contiguous()
    lin_w = _dev(lin_w, torch.float32, "linear.weight").contiguous()
    b, k, d = query.shape
    c = key.shape[1]
    assert key.shape == (b, c, d) and value.shape == (b, c, k) and lin_w.shape == (d, d)
    out = torch.empty((b, c), dtype=torch.float32, device=query.device)
    lib = _lib.load()
    with torch.cuda.device(query.device):
        need = int(lib.manner_hip_target_attention_workspace_bytes(b, k, d))
        ws = _workspace(need, query.device)
        _lib.check(lib.manner_hip_target_attention(_ptr(query), _ptr(key), _ptr(value), _ptr(lin_w), b, c, k, d, _ptr(out), _ptr(ws), need,
                                                   _stream()))
    return out


def _strided_operand(t: Tensor) -> Tensor:
    """A [B, D, N] operand the kernels may read in place: non-negative strides, D or N contiguous."""
    if min(t.stride()) < 0 or (t.stride(1) != 1 and t.stride(2) != 1):
        return t.contiguous()
    return t


def bmm(a: Tensor, b: Tensor) -> Tensor:
    """DotProduct's ``torch.bmm`` for M > 1 rows, as MINERModule.forward calls it (reference baselines/miner_module.py:195-198):
    a [B, M, D], b [B, D, N] (any strides, e.g. a permuted [B, N, D], read in place) -> [B, M, N]."""
    a = _dev(a, torch.float32, "clicked_news_vector").contiguous()
    b = _strided_operand(_dev(b, torch.float32, "candidate_news_vector"))
    bsz, m, d = a.shape
    assert b.dim() == 3 and b.shape[0] == bsz and b.shape[1] == d
    n = b.shape[2]
    out = torch.empty((bsz, m, n), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().manner_hip_bmm(_ptr(a), _ptr(b), bsz, m, n, d, b.stride(0), b.stride(1), b.stride(2), _ptr(out), _stream()))
    return out


MINER_DROPOUT_SITE = 12   # category_dropout of MINERModule: history rows at site 12, candidate rows at 13 (11 is LSTUR's)
MINER_SCORE_MODES = {"max": 0, "mean": 1}


def miner_category_bias(hist_cat: Tensor, cand_cat: Tensor, table: Tensor, hist_off: Tensor, cand_off: Tensor, width: int, p: float = 0.0,
                        seeds: Sequence[int] = (0, 0), site0: int = MINER_DROPOUT_SITE) -> Tensor:
    """The category bias of MINERModule.forward (reference baselines/miner_module.py:162-181) reduced to what PolyAttention keeps of it
    (attention.py:75, the mean over its last axis): hist_cat int64 [N_hist], cand_cat int64 [T], the frozen ``category_embedding.weight``
    [V, Dc], hist_off / cand_off int64 [B + 1], ``width`` = S -> bias [B, S, 1], bias[b, s] = (1 / T) sum over the candidates of the
    batch that are not user b's own of cos(x_{b,s}, y_t) — the reference's value, quirks included: T counts every candidate, the cosine
    has no epsilon (a zero row gives NaN where it is summed), padded slots are exactly 0.  Hand it to ``poly_attention`` as ``bias``.
    ``p`` > 0: ``category_dropout`` in train(), history rows at (seeds[0], site0), candidate rows at (seeds[1], site0 + 1).
    Dc <= 1024, S <= 256; a category id outside the table raises at ``check_status``.  No gradient (the embedding is frozen)."""
    hist_cat = _dev(hist_cat, torch.int64, "x_hist.category").contiguous().reshape(-1)
    cand_cat = _dev(cand_cat, torch.int64, "x_cand.category").contiguous().reshape(-1)
    table = _dev(table, torch.float32, "category_embedding.weight").contiguous()
    hist_off = _dev(hist_off, torch.int64, "hist_off").contiguous()
    cand_off = _dev(cand_off, torch.int64, "cand_off").contiguous()
    assert table.dim() == 2 and hist_off.numel() == cand_off.numel() >= 1
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"miner_category_bias: p={p} outside [0, 1)")
    b, (v, dc) = hist_off.numel() - 1, table.shape
    nh, t = hist_cat.numel(), cand_cat.numel()
    bias = torch.empty((b, int(width), 1), dtype=torch.float32, device=table.device)
    lib = _lib.load()
    with torch.cuda.device(table.device):
        need = int(lib.manner_hip_miner_category_bias_workspace_bytes(nh, t, b, dc))
        ws = _workspace(need, table.device)
        _lib.check(lib.manner_hip_miner_category_bias(_ptr(hist_cat), _ptr(cand_cat), _ptr(table), v, dc, _ptr(hist_off), _ptr(cand_off), nh, t, b,
                                                      int(width), C.c_float(p), C.c_uint64(int(seeds[0]) & (2 ** 64 - 1)),
                                                      C.c_uint64(int(seeds[1]) & (2 ** 64 - 1)), C.c_uint32(site0), C.c_uint32(site0 + 1),
                                                      _ptr(bias), _ptr(ws), need, _ptr(device_status(table.device).word), _stream()))
    return bias


def _code_scores_operands(cand: Tensor, cand_off: Tensor, user: Tensor, score_type: str):
    if score_type not in MINER_SCORE_MODES:
        raise ValueError(f"miner_code_scores: score_type {score_type!r} ('max' or 'mean'; 'weighted' goes through target_attention)")
    cand = _dev(cand, torch.float32, "candidate_news_vector").contiguous()
    user = _dev(user, torch.float32, "user_vector").contiguous()
    cand_off = _dev(cand_off, torch.int64, "cand_off").contiguous()
    assert cand.dim() == 2 and user.dim() == 3 and user.shape[2] == cand.shape[1] and cand_off.numel() == user.shape[0] + 1
    return cand, cand_off, user, MINER_SCORE_MODES[score_type]


def _code_scores_forward(cand: Tensor, cand_off: Tensor, user: Tensor, mode: int, arg: Optional[Tensor]) -> Tensor:
    n, d = cand.shape
    b, k = user.shape[:2]
    out = torch.empty(n, dtype=torch.float32, device=cand.device)
    with torch.cuda.device(cand.device):
        _lib.check(_lib.load().manner_hip_miner_code_scores(_ptr(cand), _ptr(cand_off), _ptr(user), n, b, k, d, mode, _ptr(out), _ptr(arg),
                                                            _stream()))
    return out


def miner_code_scores(cand: Tensor, cand_off: Tensor, user: Tensor, score_type: str) -> Tensor:
    """The score lines of MINERModule.forward for ``score_type`` 'max' / 'mean' (reference baselines/miner_module.py:195-202) on the ragged
    candidate rows: cand [N, D], cand_off int64 [B + 1], user [B, K, D] -> [N], max_k or mean_k of cand[t] . user[b, k] — no [B, C, K]
    tensor and no dense candidates (a zero-padded row would score exactly 0).  K <= 64, D <= 1024."""
    cand, cand_off, user, mode = _code_scores_operands(cand, cand_off, user, score_type)
    return _code_scores_forward(cand, cand_off, user, mode, None)


def _disagreement_operand(user: Tensor) -> Tensor:
    user = _dev(user, torch.float32, "user_vector").contiguous()
    assert user.dim() == 3
    return user


def disagreement_loss(user: Tensor) -> Tensor:
    """MINER's disagreement loss (reference baselines/miner_module.py:237-241: ``pairwise_cosine_similarity(u, u, zero_diagonal=True)
    .mean()``, components/utils.py:4-31): user [B, K, D] -> scalar, the off-diagonal cosines with the reference's 1e-8 + norm,
    divided by B K K.  K <= 64, D <= 1024."""
    user = _disagreement_operand(user)
    b, k, d = user.shape
    loss = torch.empty(1, dtype=torch.float32, device=user.device)
    lib = _lib.load()
    with torch.cuda.device(user.device):
        need = int(lib.manner_hip_disagreement_loss_workspace_bytes(b))
        ws = _workspace(need, user.device)
        _lib.check(lib.manner_hip_disagreement_loss(_ptr(user), b, k, d, _ptr(loss), _ptr(ws), need, _stream()))
    return loss[0]


def _head_operands(x: Tensor, weight: Tensor, bias: Tensor, target: Tensor, target_dtype: torch.dtype, who: str):
    x = _dev(x, torch.float32, who + ": x").contiguous()
    weight = _dev(weight, torch.float32, who + ": weight").contiguous()
    bias = _dev(bias, torch.float32, who + ": bias").contiguous()
    target = _dev(target, target_dtype, who + ": target").contiguous().reshape(-1)
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1] or bias.numel() != weight.shape[0] or target.numel() != x.shape[0]:
        raise ValueError(f"{who}: x [N, D], weight [O, D], bias [O], target [N] expected, got {tuple(x.shape)}, {tuple(weight.shape)}, "
                         f"{tuple(bias.shape)}, {tuple(target.shape)}")
    return x, weight, bias, target


def _head_ce_forward(x: Tensor, weight: Tensor, bias: Tensor, target: Tensor, saved: Optional[Tensor], logits: Optional[Tensor]) -> Tensor:
    n, d = x.shape
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        need = int(lib.manner_hip_head_workspace_bytes(n))
        ws = _workspace(need, x.device)
        _lib.check(lib.manner_hip_head_ce(_ptr(x), _ptr(weight), _ptr(bias), _ptr(target), n, d, weight.shape[0], _ptr(loss), _ptr(saved),
                                          _ptr(logits), _ptr(ws), need, _ptr(device_status(x.device).word), _stream()))
    return loss[0]


def head_ce_loss(x: Tensor, weight: Tensor, bias: Tensor, target: Tensor, return_logits: bool = False):
    """TANR's topic head and its loss (reference baselines/tanr_plm_module.py:139-141,172-174) without gradients: x [N, D] news rows,
    the ``nn.Linear(D, O)``'s weight [O, D] and bias [O], target int64 [N] class indices -> the scalar
    ``CrossEntropyLoss(x W^T + b, one_hot(target))``, the mean over all N rows; the [N, O] logits reach memory only with
    ``return_logits`` (-> (loss, logits)).  O <= 64, D <= 1024; a class outside [0, O), where ``F.one_hot`` raises, raises at
    ``check_status``."""
    x, weight, bias, target = _head_operands(x, weight, bias, target, torch.int64, "head_ce_loss")
    logits = torch.empty((x.shape[0], weight.shape[0]), dtype=torch.float32, device=x.device) if return_logits else None
    loss = _head_ce_forward(x, weight, bias, target, None, logits)
    return (loss, logits) if return_logits else loss


def _head_l1_forward(x: Tensor, weight: Tensor, bias: Tensor, target: Tensor, saved: Optional[Tensor]) -> Tensor:
    n, d = x.shape
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        need = int(lib.manner_hip_head_workspace_bytes(n))
        ws = _workspace(need, x.device)
        _lib.check(lib.manner_hip_head_l1(_ptr(x), _ptr(weight), _ptr(bias), _ptr(target), n, d, _ptr(loss), _ptr(saved), _ptr(ws), need, _stream()))
    return loss[0]


def _head_l1_operands(x: Tensor, weight: Tensor, bias: Tensor, target: Tensor):
    x, weight, bias, target = _head_operands(x, weight, bias, target, torch.float32, "head_l1_loss")
    if weight.shape[0] != 1:
        raise ValueError(f"head_l1_loss: weight [1, D] expected (nn.Linear(D, 1)), got {tuple(weight.shape)}")
    return x, weight, bias, target


def head_l1_loss(x: Tensor, weight: Tensor, bias: Tensor, target: Tensor) -> Tensor:
    """SentiRec's sentiment head and its loss (reference baselines/sentirec_plm_module.py:141-143,174-177) without gradients: x [N, D],
    the ``nn.Linear(D, 1)``'s weight [1, D] and bias [1], target f32 [N] -> the scalar ``L1Loss((x w + b).flatten(), target)``.
    D <= 1024."""
    return _head_l1_forward(*_head_l1_operands(x, weight, bias, target), None)


def _senti_div_operands(scores: Tensor, cand_score: Tensor, hist_score: Tensor, hist_off: Tensor, cand_off: Tensor, c_max: int):
    scores = _dev(scores, torch.float32, "senti_div_loss: scores").contiguous().reshape(-1)
    cand_score = _dev(cand_score, torch.float32, "x_cand.sentiment_score").contiguous().reshape(-1)
    hist_score = _dev(hist_score, torch.float32, "x_hist.sentiment_score").contiguous().reshape(-1)
    hist_off = _dev(hist_off, torch.int64, "hist_off").contiguous()
    cand_off = _dev(cand_off, torch.int64, "cand_off").contiguous()
    if cand_score.numel() != scores.numel() or hist_off.numel() != cand_off.numel() or cand_off.numel() < 2:
        raise ValueError("senti_div_loss: ragged scores [T], candidate sentiment scores [T], hist_off / cand_off [B + 1] expected")
    return scores, cand_score, hist_score, hist_off, cand_off, int(c_max)


def _senti_div_forward(scores: Tensor, cand_score: Tensor, hist_score: Tensor, hist_off: Tensor, cand_off: Tensor, c_max: int) -> Tensor:
    b = cand_off.numel() - 1
    loss = torch.empty(1, dtype=torch.float32, device=scores.device)
    lib = _lib.load()
    with torch.cuda.device(scores.device):
        need = int(lib.manner_hip_senti_div_workspace_bytes(b))
        ws = _workspace(need, scores.device)
        _lib.check(lib.manner_hip_senti_div(_ptr(scores), _ptr(cand_score), _ptr(hist_score), _ptr(hist_off), _ptr(cand_off), scores.numel(),
                                            hist_score.numel(), b, c_max, _ptr(loss), _ptr(ws), need, _ptr(device_status(scores.device).word),
                                            _stream()))
    return loss[0]


def senti_div_loss(scores: Tensor, cand_score: Tensor, hist_score: Tensor, hist_off: Tensor, cand_off: Tensor, c_max: int) -> Tensor:
    """SentiRec's sentiment diversity regulariser (reference baselines/sentirec_plm_module.py:180-193) without gradients, on the RAGGED
    scores [sum c_i]: ``relu(u[b] * s_cand[b, c] * scores[b, c]).mean()`` over the dense [B, c_max] block, u[b] = the mean sentiment
    score of user b's history.  Padded slots add 0 and count in the divisor B * c_max; a user without history gives NaN, as the
    reference's 0 / 0 does.  ``c_max`` below the largest candidate count is refused — at ``check_status`` where only the device can
    know."""
    return _senti_div_forward(*_senti_div_operands(scores, cand_score, hist_score, hist_off, cand_off, c_max))


# ---- SentiDebias-PLM's generator and discriminator lines (csrc/debias.hip)
def _class_operands(table: Tensor, cls: Tensor, who: str):
    table = _dev(table, torch.float32, who + ": class table").contiguous()
    cls = _dev(cls, torch.int64, who + ": classes").contiguous().reshape(-1)
    if table.dim() != 2:
        raise ValueError(f"{who}: class table [C, D] expected, got {tuple(table.shape)}")
    return table, cls


def _orth_operands(rows: Tensor, n_hist: int, table: Tensor, cls: Tensor, user_free: Tensor, user_aware: Tensor):
    table, cls = _class_operands(table, cls, "orth_loss")
    rows = _dev(rows, torch.float32, "orth_loss: rows").contiguous()
    user_free = _dev(user_free, torch.float32, "orth_loss: user_free").contiguous()
    user_aware = _dev(user_aware, torch.float32, "orth_loss: user_aware").contiguous()
    d = table.shape[1]
    if rows.dim() != 2 or rows.shape[1] != d or cls.numel() != rows.shape[0] or user_free.dim() != 2 or user_free.shape[1] != d \
            or user_aware.shape != user_free.shape or not 0 <= int(n_hist) <= rows.shape[0]:
        raise ValueError(f"orth_loss: rows [N, D], 0 <= n_hist <= N, table [C, D], classes [N], user_free / user_aware [B, D] expected, got "
                         f"{tuple(rows.shape)}, {n_hist}, {tuple(table.shape)}, {tuple(cls.shape)}, {tuple(user_free.shape)}, {tuple(user_aware.shape)}")
    return rows, int(n_hist), table, cls, user_free, user_aware


def _orth_forward(rows: Tensor, n_hist: int, table: Tensor, cls: Tensor, user_free: Tensor, user_aware: Tensor, means: Optional[Tensor]) -> Tensor:
    n, b = rows.shape[0], user_free.shape[0]
    loss = torch.empty(1, dtype=torch.float32, device=rows.device)
    lib = _lib.load()
    with torch.cuda.device(rows.device):
        need = int(lib.manner_hip_orth_loss_workspace_bytes(n, b))
        ws = _workspace(need, rows.device)
        _lib.check(lib.manner_hip_orth_loss(_ptr(rows), n, n_hist, _ptr(table), _ptr(cls), _ptr(user_free), _ptr(user_aware), b, table.shape[1],
                                            table.shape[0], _ptr(loss), _ptr(means), _ptr(ws), need, _ptr(device_status(rows.device).word), _stream()))
    return loss[0]


def orth_loss(rows: Tensor, n_hist: int, table: Tensor, cls: Tensor, user_free: Tensor, user_aware: Tensor) -> Tensor:
    """SentiDebias's three orthogonality terms (reference baselines/senti_debias_plm_module.py:109-135) without gradients: rows [N, D]
    news vectors, the first ``n_hist`` the history's, ``table`` [C, D] the sentiment encoder's C distinct outputs, ``cls`` int64 [N] each
    row's sentiment class, user_free / user_aware [B, D] -> the scalar ``|mean_hist cos| + |mean_cand cos| + mean_b |cos_b|`` with
    ``cos(a, b) = a . b / (1e-8 + |a| |b|)``.  The [N, D] sentiment rows are never formed.  An empty segment gives NaN, as ``torch.mean``
    of nothing.  C <= 64, D <= 1024; a class outside [0, C) raises at ``check_status``."""
    return _orth_forward(*_orth_operands(rows, n_hist, table, cls, user_free, user_aware), None)


def _class_dense_operands(table: Tensor, cls: Tensor, off: Tensor, width: int):
    table, cls = _class_operands(table, cls, "class_dense")
    off = _dev(off, torch.int64, "class_dense: offsets").contiguous()
    if off.dim() != 1 or off.numel() < 1:
        raise ValueError("class_dense: offsets [B + 1] expected")
    return table, cls, off, int(width)


def _class_dense_forward(table: Tensor, cls: Tensor, off: Tensor, width: int) -> Tensor:
    b = off.numel() - 1
    out = torch.empty((b, width, table.shape[1]), dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        _lib.check(_lib.load().manner_hip_class_dense(_ptr(table), _ptr(cls), _ptr(off), cls.numel(), b, width, table.shape[1], table.shape[0],
                                                      _ptr(out), _ptr(device_status(table.device).word), _stream()))
    return out


def class_dense(table: Tensor, cls: Tensor, off: Tensor, width: int) -> Tensor:
    """``to_dense_batch`` of the sentiment rows ``table[cls]`` (reference baselines/senti_debias_plm_module.py:95-100) without forming
    them: table [C, D], cls int64 [N], off int64 [B + 1] -> [B, width, D], padded slots exactly 0.  ``B * width < N`` is refused; a
    single user with more than ``width`` rows raises at ``check_status``.  C <= 64."""
    return _class_dense_forward(*_class_dense_operands(table, cls, off, width))


def _class_scores_operands(user: Tensor, table: Tensor, cls: Tensor, off: Tensor):
    table, cls = _class_operands(table, cls, "class_scores")
    user = _dev(user, torch.float32, "class_scores: user").contiguous()
    off = _dev(off, torch.int64, "class_scores: offsets").contiguous()
    if user.dim() != 2 or user.shape[1] != table.shape[1] or off.numel() != user.shape[0] + 1:
        raise ValueError(f"class_scores: user [B, D], table [C, D], offsets [B + 1] expected, got {tuple(user.shape)}, {tuple(table.shape)}, "
                         f"{tuple(off.shape)}")
    return user, table, cls, off


def _class_scores_forward(user: Tensor, table: Tensor, cls: Tensor, off: Tensor) -> Tensor:
    b, c = user.shape[0], table.shape[0]
    out = torch.empty(cls.numel(), dtype=torch.float32, device=user.device)
    lib = _lib.load()
    with torch.cuda.device(user.device):
        need = int(lib.manner_hip_class_scores_workspace_bytes(b, c))
        ws = _workspace(need, user.device)
        _lib.check(lib.manner_hip_class_scores(_ptr(user), _ptr(table), _ptr(cls), _ptr(off), cls.numel(), b, table.shape[1], c, _ptr(out), _ptr(ws),
                                               need, _ptr(device_status(user.device).word), _stream()))
    return out


def class_scores(user: Tensor, table: Tensor, cls: Tensor, off: Tensor) -> Tensor:
    """SentiDebias's bias-aware scores (reference baselines/senti_debias_plm_module.py:142-145) on the ragged candidates: user [B, D] the
    bias-aware user vectors, table [C, D], cls int64 [sum c_i] the candidates' sentiment classes, off int64 [B + 1] -> [sum c_i],
    ``user_b . table[cls_t]`` read from the [B, C] products — no dense [B, Cmax, D] block, no permute, no bmm.  C <= 64."""
    return _class_scores_forward(*_class_scores_operands(user, table, cls, off))


def _adv_operands(rows: Tensor, n_hist: int, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, cls: Tensor):
    rows = _dev(rows, torch.float32, "adv_loss: rows").contiguous()
    w1, b1 = _dev(w1, torch.float32, "adv_loss: linear1.weight").contiguous(), _dev(b1, torch.float32, "adv_loss: linear1.bias").contiguous()
    w2, b2 = _dev(w2, torch.float32, "adv_loss: linear2.weight").contiguous(), _dev(b2, torch.float32, "adv_loss: linear2.bias").contiguous()
    cls = _dev(cls, torch.int64, "adv_loss: classes").contiguous().reshape(-1)
    if rows.dim() != 2 or w1.dim() != 2 or w2.dim() != 2 or w1.shape[1] != rows.shape[1] or w2.shape[1] != w1.shape[0] or b1.numel() != w1.shape[0] \
            or b2.numel() != w2.shape[0] or cls.numel() != rows.shape[0] or not 0 <= int(n_hist) <= rows.shape[0]:
        raise ValueError(f"adv_loss: rows [N, D], 0 <= n_hist <= N, linear1 [H, D] / [H], linear2 [O, H] / [O], classes [N] expected, got "
                         f"{tuple(rows.shape)}, {n_hist}, {tuple(w1.shape)}, {tuple(b1.shape)}, {tuple(w2.shape)}, {tuple(b2.shape)}, {tuple(cls.shape)}")
    return rows, int(n_hist), w1, b1, w2, b2, cls


def _adv_forward(rows: Tensor, n_hist: int, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, cls: Tensor, hidden: Tensor, saved: Optional[Tensor]) -> Tensor:
    n, d = rows.shape
    loss = torch.empty(1, dtype=torch.float32, device=rows.device)
    lib = _lib.load()
    with torch.cuda.device(rows.device):
        need = int(lib.manner_hip_adv_loss_workspace_bytes(n))
        ws = _workspace(need, rows.device)
        _lib.check(lib.manner_hip_adv_loss(_ptr(rows), n, n_hist, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(cls), d, w1.shape[0], w2.shape[0],
                                           _ptr(loss), _ptr(hidden), _ptr(saved), _ptr(ws), need, _ptr(device_status(rows.device).word), _stream()))
    return loss[0]


def adv_loss(rows: Tensor, n_hist: int, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, cls: Tensor) -> Tensor:
    """SentiDebias's discriminator and its loss (reference baselines/senti_debias_plm_module.py:163-167, 275-280) without gradients: rows
    [N, D], the first ``n_hist`` the history's, ``linear1`` [H, D] / [H], ``linear2`` [O, H] / [O], cls int64 [N] -> the scalar
    ``mean_hist CE_i + mean_cand CE_i`` with ``CE_i = -log softmax(W2 tanh(W1 x_i + b1) + b2)[(cls_i - 1) mod O]`` — the module writes
    ``y_true[i, t - 1] = 1``, so class 0 lands on the last column.  No [N, O] one-hot matrix, no loop over the rows.  O <= 64,
    H <= 1024, D <= 1024; a class outside [0, O) raises at ``check_status``."""
    rows, n_hist, w1, b1, w2, b2, cls = _adv_operands(rows, n_hist, w1, b1, w2, b2, cls)
    hidden = torch.empty((rows.shape[0], w1.shape[0]), dtype=torch.float32, device=rows.device)
    return _adv_forward(rows, n_hist, w1, b1, w2, b2, cls, hidden, None)


AXIS0_WIDE_MIN_DH = 65      # head dims 65 .. 128 are axis0_attention_wide's; 1 .. 64 are axis0_attention_any's


def axis0_family(dh: int) -> str:
    """The run-time-head-dim family that serves head dim ``dh``: "wide" (csrc/mins.hip) from ``AXIS0_WIDE_MIN_DH`` on, else "any"
    (csrc/caum.hip).  The seven fixed head dims of ``mha_axis0`` are a third family with entries of its own (csrc/axis0.hip)."""
    return "wide" if dh >= AXIS0_WIDE_MIN_DH else "any"


def _axis0_attention(family: str, qkv: Tensor, heads: int, stats: Optional[Tensor]) -> Tensor:
    """manner_hip_axis0_attention_<family> on projected rows: qkv [L0, B1, 3E] -> [L0, B1, E]."""
    qkv = _dev(qkv, torch.float32, "qkv").contiguous()
    l0, b1, e3 = qkv.shape
    out = torch.empty((l0, b1, e3 // 3), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        _lib.check(getattr(_lib.load(), "manner_hip_axis0_attention_" + family)(_ptr(qkv), l0, b1, e3 // 3, int(heads), _ptr(out), _ptr(stats),
                                                                               _stream()))
    return out


def _mha_axis0(family: str, x: Tensor, in_proj_w: Tensor, in_proj_b: Tensor, out_proj_w: Tensor, out_proj_b: Tensor, heads: int) -> Tensor:
    """in-projection, the attention core of ``family``, out-projection."""
    x = _dev(x, torch.float32, "x").contiguous()
    l0, b1, e = x.shape
    if x.numel() == 0:
        return torch.empty_like(x)
    qkv = linear(x.reshape(l0 * b1, e), in_proj_w, in_proj_b).reshape(l0, b1, 3 * e)
    att = _axis0_attention(family, qkv, heads, None)
    return linear(att.reshape(l0 * b1, e), out_proj_w, out_proj_b).reshape(l0, b1, e)


def axis0_attention_any(qkv: Tensor, heads: int, stats: Optional[Tensor] = None) -> Tensor:
    """The attention core of ``mha_axis0_any`` on projected rows: qkv [L0, B1, 3E] -> [L0, B1, E]; ``stats`` f32 [L0 * B1 * heads * 3]
    receives the softmax statistics the backward reads."""
    return _axis0_attention("any", qkv, heads, stats)


def mha_axis0_any(x: Tensor, in_proj_w: Tensor, in_proj_b: Tensor, out_proj_w: Tensor, out_proj_b: Tensor, heads: int) -> Tensor:
    """``mha_axis0`` at ANY head dim 1..64 (CAUM ships 25 in its user encoder and 5 in its entity encoder): attention along AXIS 0 of
    x [L0, B1, E], unmasked.  At L0 < 256 a workgroup takes several (slot, head) pairs, one thread per (pair, row)."""
    return _mha_axis0("any", x, in_proj_w, in_proj_b, out_proj_w, out_proj_b, heads)


CAUM_PARAMS = ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "multihead_attention.in_proj_weight",
               "multihead_attention.in_proj_bias", "multihead_attention.out_proj.weight", "multihead_attention.out_proj.bias",
               "linear3.weight", "linear3.bias", "dense_att.linear.weight", "dense_att.linear.bias", "dense_att.linear2.weight",
               "dense_att.linear2.bias", "dense_att.linear3.weight", "dense_att.linear3.bias")
CAUM_DROPOUT_SITE = 7     # dropout1 / 2 / 3 of CAUMUserEncoder draw at the sites 7, 8, 9 (2..6 are the news encoders')


def _caum_operands(x: Tensor, c: Tensor, params: Sequence[Tensor], heads: int):
    """Checked operands of the CAUM user-encoder entries: (x, c, params, dims); c keeps its row stride (the cand[:, i, :] view)."""
    x = _dev(x, torch.float32, "clicked_news_vector").contiguous()
    c = _dev(c, torch.float32, "cand_news_vector")
    if x.dim() != 3 or c.dim() != 2 or c.shape[0] != x.shape[0] or c.shape[1] != x.shape[2]:
        raise ValueError(f"caum_user_scores: clicked_news_vector {tuple(x.shape)} / cand_news_vector {tuple(c.shape)} must be [B, S, D] / [B, D]")
    if c.stride(1) != 1 or (c.shape[0] > 1 and c.stride(0) < c.shape[1]):
        c = c.contiguous()
    if len(params) != len(CAUM_PARAMS):
        raise ValueError(f"caum_user_scores: {len(CAUM_PARAMS)} parameters expected ({', '.join(CAUM_PARAMS)})")
    params = [_dev(t, torch.float32, n).contiguous() for t, n in zip(params, CAUM_PARAMS)]
    b, s, d = x.shape
    f, u, h1, h2 = params[0].shape[0], params[2].shape[0], params[10].shape[0], params[12].shape[0]
    if d != u:
        raise RuntimeError(f"CAUMUserEncoder: news_vector_dim {d} != user_vector_dim {u} — DenseAttention(input_dim=2 * {u}) is fed "
                           f"cat[all ({u}), candidate ({d})], which only the reference's D == U configuration can multiply")
    shapes = ((f, 4 * d), (f,), (u, 2 * d), (u,), (3 * u, u), (3 * u,), (u, u), (u,), (u, f + u), (u,), (h1, 2 * u), (h1,), (h2, h1), (h2,),
              (1, h2), (1,))
    for t, n, want in zip(params, CAUM_PARAMS, shapes):
        if tuple(t.shape) != want:
            raise ValueError(f"caum_user_scores: {n} is {tuple(t.shape)}, expected {want}")
    return x, c, params, (b, s, d, f, u, h1, h2, int(heads))


def _caum_forward(x: Tensor, c: Tensor, params: Sequence[Tensor], dims, p: float, seed: int, site0: int):
    b, s = dims[0], dims[1]
    lib = _lib.load()
    out = torch.empty(b, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        need = int(lib.manner_hip_caum_user_saved_bytes(*dims))
        saved = _workspace(need, x.device)
        tab = (C.c_void_p * len(params))(*[t.data_ptr() for t in params])
        _lib.check(lib.manner_hip_caum_user_forward(_ptr(x), _ptr(c), c.stride(0) if b > 1 else dims[2], tab, *dims, C.c_float(p),
                                                    C.c_uint64(seed), C.c_uint32(site0), _ptr(out), _ptr(saved), need, _stream()))
    return out, saved, need


def caum_user_scores(x: Tensor, c: Tensor, params: Sequence[Tensor], heads: int) -> Tensor:
    """CAUMUserEncoder.forward in eval() (reference user_encoder.py:121-178): x [B, S, D] clicked news, c [B, D] one candidate per user
    (any row stride), ``params`` the 16 tensors named by ``CAUM_PARAMS`` -> scores [B].  The attention runs across the B users at each
    history slot and the softmax over all S slots, unmasked, as in the reference.  S <= 256, widths <= 1024, head dim <= 64, D == U."""
    x, c, params, dims = _caum_operands(x, c, params, heads)
    return _caum_forward(x, c, params, dims, 0.0, 0, CAUM_DROPOUT_SITE)[0]


#: default cap of ``caum_scores_all``'s workspace: 256 MiB hold every column of a MIND dev batch at B = 8 (C = 300 at the shipped widths:
#: 0.7 MiB of wide rows per column and user) and 13 columns per pass at B = 64; what is taken once per call comes on top when it is more
CAUM_ALL_WORKSPACE_BYTES = 256 << 20


def caum_scores_all(x: Tensor, cand: Tensor, params: Sequence[Tensor], heads: int, max_workspace_bytes: Optional[int] = None) -> Tensor:
    """The candidate loop of CAUMPLMModule.forward (reference baselines/caum_plm_module.py:159-161) in one library call, eval() only:
    x [B, S, D] clicked news, cand [B, C, D] dense candidates, ``params`` as ``caum_user_scores`` -> scores [B, C] with column c what
    ``caum_user_scores(x, cand[:, c, :], ...)`` gives.  The products that depend on the history alone or on the candidate alone are
    taken once; only attention, linear3 and the dense attention's two tanh layers run over the B C S rows.  Those rows live in a
    workspace of at most ``max_workspace_bytes`` (default ``CAUM_ALL_WORKSPACE_BYTES``; never less than one column needs) and the
    library walks the columns in as many passes as that takes; a column's bits do not depend on the cap."""
    if not isinstance(cand, torch.Tensor) or cand.dim() != 3:
        raise ValueError(f"caum_scores_all: cand_news_vector {tuple(getattr(cand, 'shape', ()))} must be [B, C, D]")
    b, c = cand.shape[0], cand.shape[1]
    x, _, params, dims = _caum_operands(x, cand[:, 0, :] if c else cand.new_empty((b, cand.shape[2])), params, heads)
    cand = _dev(cand, torch.float32, "cand_news_vector").contiguous()
    out = torch.empty((b, c), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    args = (dims[0], dims[1], c) + dims[2:]
    with torch.cuda.device(x.device):
        least, full = (int(lib.manner_hip_caum_scores_all_workspace_bytes(*args, n)) for n in (1, max(c, 1)))
        cap = CAUM_ALL_WORKSPACE_BYTES if max_workspace_bytes is None else int(max_workspace_bytes)
        need = min(full, max(cap, least))
        work = _workspace(need, x.device)
        tab = (C.c_void_p * len(params))(*[t.data_ptr() for t in params])
        _lib.check(lib.manner_hip_caum_scores_all(_ptr(x), _ptr(cand), tab, *args, _ptr(out), _ptr(work), need, _stream()))
    return out


def linear_tanh(x: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    """tanh(nn.Linear(x)) in one kernel on f32 rows (DenseAttention, reference attention.py:135-138): x [R, K] -> [R, O]."""
    x = _dev(x, torch.float32, "input").contiguous()
    weight = _dev(weight, torch.float32, "weight").contiguous()
    r, k = x.shape
    o = weight.shape[0]
    assert weight.shape[1] == k
    if bias is not None:
        bias = _dev(bias, torch.float32, "bias").contiguous()
    y = torch.empty((r, o), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().manner_hip_linear_tanh(_ptr(x), _ptr(weight), _ptr(bias), r, k, o, _ptr(y), _stream()))
    return y


def seqcls_head(x: Tensor, dense_w: Tensor, dense_b: Tensor, out_w: Tensor, out_b: Tensor, pos_idx: int = -1, neg_idx: int = -1,
                with_probs: bool = True) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """The classifier of a ``*ForSequenceClassification`` checkpoint and the reference annotator's rule (sentiment_annotator.py:25-38) on
    [CLS] rows, one launch (csrc/seqcls.hip): x [N, H] f32 (a row-strided view is read in place) -> (label int32 [N], score f32 [N],
    probs f32 [N, L] or None).  tanh(dense) -> out -> softmax -> argmax (lowest index at a tie); score = p[a] / -p[a] for the ids
    ``pos_idx`` / ``neg_idx`` (-1: none), else (1 - p[a]) (p[L-1] - p[0]).  A row with a non-finite logit: label -1, score NaN."""
    x = _dev(x, torch.float32, "x")
    if x.dim() != 2:
        raise ValueError(f"seqcls_head: x {tuple(x.shape)} must be [N, H]")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    n, h = x.shape
    ldx = x.stride(0) if n > 1 else h
    dense_w, dense_b = _dev(dense_w, torch.float32, "dense_w").contiguous(), _dev(dense_b, torch.float32, "dense_b").contiguous()
    out_w, out_b = _dev(out_w, torch.float32, "out_w").contiguous(), _dev(out_b, torch.float32, "out_b").contiguous()
    nl = out_w.shape[0]
    if tuple(dense_w.shape) != (h, h) or tuple(dense_b.shape) != (h,) or tuple(out_w.shape) != (nl, h) or tuple(out_b.shape) != (nl,):
        raise ValueError(f"seqcls_head: dense {tuple(dense_w.shape)} / {tuple(dense_b.shape)}, out {tuple(out_w.shape)} / {tuple(out_b.shape)} "
                         f"do not fit x [N, {h}]")
    label = torch.empty((n,), dtype=torch.int32, device=x.device)
    score = torch.empty((n,), dtype=torch.float32, device=x.device)
    probs = torch.empty((n, nl), dtype=torch.float32, device=x.device) if with_probs else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().manner_hip_seqcls_head(_ptr(x), ldx, _ptr(dense_w), _ptr(dense_b), _ptr(out_w), _ptr(out_b), n, h, nl,
                                                      int(pos_idx), int(neg_idx), _ptr(probs), _ptr(label), _ptr(score), _stream()))
    return label, score, probs


def relu(x: Tensor) -> Tensor:
    x = _dev(x, torch.float32, "x").contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().manner_hip_relu(_ptr(x), _ptr(out), x.numel(), _stream()))
    return out


GRU_PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
LSTUR_PARAMS = ("long_term_user_embedding.weight",) + tuple("gru." + n for n in GRU_PARAMS)
LSTUR_DROPOUT_SITE = 11   # the user mask of LSTURUserEncoder (7 .. 10 are CAUM's)


def _gru_operands(x: Tensor, lengths: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, h0: Optional[Tensor]):
    """Checked operands of the GRU entries: (x, lengths, [w_ih, w_hh, b_ih, b_hh], h0, (B, S, I, H)).  x keeps its batch and slot
    strides when its features are contiguous (a channel view of a wider tensor is read in place); lengths stay on the device."""
    x = _dev(x, torch.float32, "x")
    if x.dim() != 3:
        raise ValueError(f"gru_last_hidden: x {tuple(x.shape)} must be [B, S, I]")
    if (x.shape[2] > 1 and x.stride(2) != 1) or min(x.stride()) < 0:
        x = x.contiguous()
    b, s, i = x.shape
    if not isinstance(lengths, torch.Tensor) or not lengths.is_cuda:
        raise RuntimeError("lengths: expected a GPU tensor — the MANNeR HIP hot path has no CPU fallback")
    if lengths.dtype not in (torch.int64, torch.int32) or tuple(lengths.shape) != (b,):
        raise TypeError(f"lengths: expected int64 [{b}], got {lengths.dtype} {tuple(lengths.shape)}")
    lengths = lengths.to(torch.int64).contiguous()
    params = [_dev(t, torch.float32, "gru." + n).contiguous() for t, n in zip((w_ih, w_hh, b_ih, b_hh), GRU_PARAMS)]
    h = params[1].shape[1]
    for t, n, want in zip(params, GRU_PARAMS, ((3 * h, i), (3 * h, h), (3 * h,), (3 * h,))):
        if tuple(t.shape) != want:
            raise ValueError(f"gru_last_hidden: gru.{n} is {tuple(t.shape)}, expected {want}")
    if h0 is not None:
        h0 = _dev(h0, torch.float32, "h0").contiguous()
        if tuple(h0.shape) != (b, h):
            raise ValueError(f"gru_last_hidden: h0 is {tuple(h0.shape)}, expected {(b, h)}")
    return x, lengths, params, h0, (b, s, i, h)


def _gru_forward(x: Tensor, lengths: Tensor, params: Sequence[Tensor], h0: Optional[Tensor], dims, out: Tensor, save: bool):
    """One manner_hip_gru_forward call into the first H columns of ``out`` [B, >= H]; -> (saved buffer or None, its size)."""
    b, s = dims[0], dims[1]
    lib = _lib.load()
    with torch.cuda.device(x.device):
        need = int(lib.manner_hip_gru_workspace_bytes(*dims))
        ws = _workspace(need, x.device)
        keep = int(lib.manner_hip_gru_saved_bytes(*dims)) if save else 0
        saved = _workspace(keep, x.device) if save else None
        _lib.check(lib.manner_hip_gru_forward(_ptr(x), x.stride(0) if b > 1 else 0, x.stride(1) if s > 1 else 0, _ptr(lengths), *[_ptr(t) for t in params],
                                              _ptr(h0), *dims, _ptr(out), out.stride(0) if b > 1 else out.shape[1], _ptr(saved), keep, _ptr(ws), need,
                                              _ptr(device_status(x.device).word), _stream()))
    return saved, keep


def gru_last_hidden(x: Tensor, lengths: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, h0: Optional[Tensor] = None) -> Tensor:
    """``nn.GRU`` on ``pack_padded_sequence(x, lengths, batch_first=True, enforce_sorted=False)``, ``last_hidden`` (reference
    user_encoder.py:78-88): x [B, S, I] (batch and slot strides are read in place), lengths int64 [B] on the device, the four
    ``nn.GRU`` tensors (gates r | z | n), h0 [B, H] or None -> [B, H], row b after its own ``lengths[b]`` steps.  Slots past a row's
    length are never read.  One launch per time step; nothing is read back to the host.  S <= 256, I, H <= 1024; a length outside
    [1, S] surfaces at ``check_status``."""
    x, lengths, params, h0, dims = _gru_operands(x, lengths, w_ih, w_hh, b_ih, b_hh, h0)
    out = torch.empty((dims[0], dims[3]), dtype=torch.float32, device=x.device)
    _gru_forward(x, lengths, params, h0, dims, out, save=False)
    return out


def user_rows(ids: Optional[Tensor], src: Tensor, out: Tensor, p: float, seed: int, site: int = LSTUR_DROPOUT_SITE) -> Tensor:
    """out[b, :E] = m(b) src[ids[b], :E] (``ids`` None: src[b, :E]), m(b) = 0 or 1 / (1 - p) per ROW b at (seed, site) —
    ``nn.Dropout2d`` on [1, B, E]: a whole user is masked.  ``src`` and ``out`` are 2-D with contiguous columns (row strides kept)."""
    b, e = out.shape
    n_rows = src.shape[0]
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().manner_hip_user_rows(_ptr(ids), _ptr(src), n_rows, src.stride(0) if n_rows > 1 else e, b, e, C.c_float(p),
                                                    C.c_uint64(seed), C.c_uint32(site), _ptr(out), out.stride(0) if b > 1 else e,
                                                    _ptr(device_status(out.device).word), _stream()))
    return out


def _lstur_operands(user: Tensor, x: Tensor, lengths: Tensor, params: Sequence[Tensor], method: str):
    if method not in ("ini", "con"):
        raise ValueError(f"lstur_user: long_short_term_method {method!r} (ini or con)")
    if len(params) != len(LSTUR_PARAMS):
        raise ValueError(f"lstur_user: {len(LSTUR_PARAMS)} parameters expected ({', '.join(LSTUR_PARAMS)})")
    table = _dev(params[0], torch.float32, LSTUR_PARAMS[0]).contiguous()
    x, lengths, gru, _, dims = _gru_operands(x, lengths, *params[1:], None)
    user = _dev(user, torch.int64, "user").contiguous()
    if tuple(user.shape) != (dims[0],) or table.dim() != 2 or table.shape[1] != dims[3]:
        raise ValueError(f"lstur_user: user {tuple(user.shape)} / {LSTUR_PARAMS[0]} {tuple(table.shape)} must be [{dims[0]}] / [num_users, {dims[3]}]")
    return user, x, lengths, table, gru, dims


def _lstur_forward(user, x, lengths, table, gru, dims, method: str, p: float, seed: int, save: bool):
    """-> (out, saved, saved bytes).  ``ini``: the masked user rows are h0; ``con``: they are the second half of the output buffer and
    the GRU writes its first half, so no concatenation runs."""
    b, h = dims[0], dims[3]
    if method == "ini":
        out = torch.empty((b, h), dtype=torch.float32, device=x.device)
        h0 = user_rows(user, table, torch.empty((b, h), dtype=torch.float32, device=x.device), p, seed)
    else:
        out = torch.empty((b, 2 * h), dtype=torch.float32, device=x.device)
        h0 = None
        if b:
            user_rows(user, table, out[:, h:], p, seed)
    saved, keep = _gru_forward(x, lengths, gru, h0, dims, out, save)
    return out, saved, keep


def lstur_user(user: Tensor, x: Tensor, lengths: Tensor, params: Sequence[Tensor], method: str, p: float = 0.0, seed: int = 0) -> Tensor:
    """LSTURUserEncoder.forward (reference user_encoder.py:70-89): user int64 [B], x [B, S, I] clicked news, lengths int64 [B],
    ``params`` the five tensors named by ``LSTUR_PARAMS``.  ``ini``: the GRU starts from the user's embedding row -> [B, H];
    ``con``: it starts from zero and the row is appended -> [B, 2 H].  ``p`` > 0 masks whole users (``nn.Dropout2d`` on [1, B, E]) at
    (seed, row).  A user id outside the table or a length outside [1, S] surfaces at ``check_status``."""
    user, x, lengths, table, gru, dims = _lstur_operands(user, x, lengths, params, method)
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"lstur_user: p={p} outside [0, 1)")
    return _lstur_forward(user, x, lengths, table, gru, dims, method, float(p), int(seed) & (2 ** 64 - 1), save=False)[0]


MINS_PARAMS = ("multihead_attention.in_proj_weight", "multihead_attention.in_proj_bias", "multihead_attention.out_proj.weight",
               "multihead_attention.out_proj.bias") + tuple("gru." + n for n in GRU_PARAMS)


def _channel_gru_operands(x: Tensor, lengths: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, channels: int):
    """Checked operands of the channel-GRU entries: (x, lengths, [w_ih, w_hh, b_ih, b_hh], (B, S, C, I, H)).  x [B, S, C I] keeps its
    batch and slot strides when its features are contiguous; lengths stay on the device."""
    x = _dev(x, torch.float32, "x")
    c = int(channels)
    if x.dim() != 3 or c < 1 or x.shape[2] % c:
        raise ValueError(f"channel_gru_last_hidden: x {tuple(x.shape)} must be [B, S, C I] with C = {channels} channels")
    if (x.shape[2] > 1 and x.stride(2) != 1) or min(x.stride()) < 0:
        x = x.contiguous()
    b, s, width = x.shape
    i = width // c
    if not isinstance(lengths, torch.Tensor) or not lengths.is_cuda:
        raise RuntimeError("lengths: expected a GPU tensor — the MANNeR HIP hot path has no CPU fallback")
    if lengths.dtype not in (torch.int64, torch.int32) or tuple(lengths.shape) != (b,):
        raise TypeError(f"lengths: expected int64 [{b}], got {lengths.dtype} {tuple(lengths.shape)}")
    lengths = lengths.to(torch.int64).contiguous()
    params = [_dev(t, torch.float32, "gru." + n).contiguous() for t, n in zip((w_ih, w_hh, b_ih, b_hh), GRU_PARAMS)]
    h = params[1].shape[1]
    for t, n, want in zip(params, GRU_PARAMS, ((3 * h, i), (3 * h, h), (3 * h,), (3 * h,))):
        if tuple(t.shape) != want:
            raise ValueError(f"channel_gru_last_hidden: gru.{n} is {tuple(t.shape)}, expected {want}")
    return x, lengths, params, (b, s, c, i, h)


def _channel_gru_forward(x: Tensor, lengths: Tensor, params: Sequence[Tensor], dims, save: bool):
    """One manner_hip_channel_gru_forward call -> (out [B, C H], saved buffer or None, its size)."""
    b, s, c, _, h = dims
    lib = _lib.load()
    out = torch.empty((b, c * h), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        need = int(lib.manner_hip_channel_gru_workspace_bytes(*dims))
        ws = _workspace(need, x.device)
        keep = int(lib.manner_hip_channel_gru_saved_bytes(*dims)) if save else 0
        saved = _workspace(keep, x.device) if save else None
        _lib.check(lib.manner_hip_channel_gru_forward(_ptr(x), x.stride(0) if b > 1 else 0, x.stride(1) if s > 1 else 0, _ptr(lengths),
                                                      *[_ptr(t) for t in params], *dims, _ptr(out), c * h, _ptr(saved), keep, _ptr(ws), need,
                                                      _ptr(device_status(x.device).word), _stream()))
    return out, saved, keep


def channel_gru_last_hidden(x: Tensor, lengths: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, channels: int) -> Tensor:
    """MINSUserEncoder's multi-channel GRU (reference user_encoder.py:217-238): x [B, S, C I] is C channels of width I (``torch.chunk``
    along the features, read in place), every channel through the SAME ``nn.GRU`` tensors (gates r | z | n) on
    ``pack_padded_sequence(lengths, enforce_sorted=False)``, ``last_hidden`` concatenated -> [B, C H].  lengths int64 [B] on the device;
    slots past a row's length are never read.  The whole recurrence is one launch (csrc/mins.hip); nothing is read back to the host.
    S <= 256, I <= 1024, H <= 128; a length outside [1, S] surfaces at ``check_status``."""
    x, lengths, params, dims = _channel_gru_operands(x, lengths, w_ih, w_hh, b_ih, b_hh, channels)
    return _channel_gru_forward(x, lengths, params, dims, save=False)[0]


def axis0_attention_wide(qkv: Tensor, heads: int, stats: Optional[Tensor] = None) -> Tensor:
    """``axis0_attention_any`` at head dims 65 .. 128 (MINS ships 768 / 6 = 128): qkv [L0, B1, 3E] -> [L0, B1, E]; a wave per query
    row, the lanes along the head dim.  ``stats`` f32 [L0 * B1 * heads * 3] receives the softmax statistics the backward reads."""
    return _axis0_attention("wide", qkv, heads, stats)


def mha_axis0_wide(x: Tensor, in_proj_w: Tensor, in_proj_b: Tensor, out_proj_w: Tensor, out_proj_b: Tensor, heads: int) -> Tensor:
    """``mha_axis0_any`` at head dims 65 .. 128: attention along AXIS 0 of x [L0, B1, E], unmasked."""
    return _mha_axis0("wide", x, in_proj_w, in_proj_b, out_proj_w, out_proj_b, heads)


def mins_check_widths(d: int, f: int, c: int) -> None:
    """As in the reference only num_filters == news_embedding_dim can run: its chunk width D / C is not the GRU's input width F / C."""
    if f != d:
        raise RuntimeError(f"MINSUserEncoder: num_filters {f} != news_embedding_dim {d} — the attention's output is chunked into "
                           f"{c} channels of width {d // c}, which the GRU of input width {f // c} cannot read; only the reference's "
                           f"num_filters == news_embedding_dim configuration can run")


def _mins_operands(x: Tensor, params: Sequence[Tensor], channels: int):
    """x [B, S, D] and the eight tensors named by ``MINS_PARAMS``; refuses num_filters != news_embedding_dim as the reference's
    forward does (its chunk of width D / C is not the GRU's input width F / C)."""
    if len(params) != len(MINS_PARAMS):
        raise ValueError(f"mins_user: {len(MINS_PARAMS)} parameters expected ({', '.join(MINS_PARAMS)})")
    x = _dev(x, torch.float32, "clicked_news_vector")
    c = int(channels)
    if x.dim() != 3 or c < 1 or x.shape[2] % c:
        raise ValueError(f"mins_user: clicked_news_vector {tuple(x.shape)} must be [B, S, D] with D a multiple of the {channels} channels")
    mins_check_widths(x.shape[2], c * params[4].shape[1], c)
    return x.contiguous(), c


def mins_user(x: Tensor, lengths: Tensor, params: Sequence[Tensor], channels: int) -> Tensor:
    """MINSUserEncoder.forward in eval() (reference user_encoder.py:211-243): x [B, S, D] clicked news, lengths int64 [B],
    ``params`` the eight tensors named by ``MINS_PARAMS`` -> [B, D].  The attention (heads = channels) runs ACROSS THE B USERS at each
    history slot, unmasked, as in the reference; head dims 65 .. 128 take ``mha_axis0_wide``, 1 .. 64 ``mha_axis0_any``.  The final
    additive pooler over a sequence of one slot is the identity and is not run."""
    x, c = _mins_operands(x, params, channels)
    mixed = _mha_axis0(axis0_family(x.shape[2] // c), x, *params[:4], c)
    return channel_gru_last_hidden(mixed, lengths, *params[4:], c)


class HalfTable:
    """IEEE-half copy of a news-embedding table for the scorer: ``rows`` float16 [n, D] and, when centred, ``mean`` float32 [D]
    (rows = half(T - mean)); see ``table_to_f16``."""

    def __init__(self, rows: Tensor, mean: Optional[Tensor]):
        self.rows, self.mean = rows, mean
        self.shape, self.device = rows.shape, rows.device


def score_late_fusion(table, hist_idx: Tensor, hist_off: Tensor, cand_idx: Tensor, cand_off: Tensor,
                      total_cand: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """Ragged scores [sum c_i] of impressions given as CSR index lists into ``table`` [n, D] — float32, or the float16
    copy made by ``table_to_f16`` (half the bytes per gathered row; Infinity-Cache resident at the MIND-large shape)."""
    mean = None
    half = isinstance(table, HalfTable) or (isinstance(table, torch.Tensor) and table.dtype == torch.float16)
    if half:
        if isinstance(table, HalfTable):
            table, mean = table.rows, table.mean
        table = _dev(table, torch.float16, "table").contiguous()
    else:
        table = _dev(table, torch.float32, "table").contiguous()
    hist_idx, cand_idx = _dev(hist_idx, torch.int32, "hist_idx"), _dev(cand_idx, torch.int32, "cand_idx")
    hist_off, cand_off = _dev(hist_off, torch.int64, "hist_off"), _dev(cand_off, torch.int64, "cand_off")
    nb = hist_off.numel() - 1
    assert cand_off.numel() == nb + 1
    total = int(cand_idx.numel()) if total_cand is None else total_cand
    if out is None:
        out = torch.empty((total,), dtype=torch.float32, device=table.device)
    else:
        _dev(out, torch.float32, "out")
        assert out.is_contiguous() and out.numel() == total
    # bind the contiguous copies to locals: a temporary's storage could be handed to the next temporary
    # before the kernel has read it
    hist_idx, hist_off, cand_idx, cand_off = (hist_idx.contiguous(), hist_off.contiguous(), cand_idx.contiguous(),
                                              cand_off.contiguous())
    with torch.cuda.device(table.device):
        if half:
            _lib.check(_lib.load().manner_hip_score_late_fusion_f16(
                _ptr(table), _ptr(mean), table.shape[0], table.shape[1], _ptr(hist_idx), _ptr(hist_off), _ptr(cand_idx), _ptr(cand_off),
                nb, _ptr(out), _ptr(device_status(table.device).word), _stream()))
        else:
            _lib.check(_lib.load().manner_hip_score_late_fusion(
                _ptr(table), table.shape[0], table.shape[1], _ptr(hist_idx), _ptr(hist_off), _ptr(cand_idx), _ptr(cand_off),
                nb, _ptr(out), _ptr(device_status(table.device).word), _stream()))
    return out


def table_to_f16(table: Tensor, centre: bool = False, out: Optional[Tensor] = None):
    """IEEE-half copy of a news-embedding table for ``score_late_fusion`` (rows rounded to 11 mantissa bits).
    ``centre=False`` -> the float16 tensor half(T).  ``centre=True`` -> ``HalfTable(half(T - mean), mean)``: the rows are
    centred on the table's column mean first, which is what keeps the rounding away from the scores when the rows are
    nearly collinear (the usual state of one encoder's [CLS] vectors)."""
    table = _dev(table, torch.float32, "table").contiguous()
    n, d = table.shape
    if out is None:
        out = torch.empty(table.shape, dtype=torch.float16, device=table.device)
    else:
        _dev(out, torch.float16, "out")
        assert out.is_contiguous() and out.shape == table.shape
    lib = _lib.load()
    with torch.cuda.device(table.device):
        if not centre:
            _lib.check(lib.manner_hip_table_to_f16(_ptr(table), n, d, None, _ptr(out), None, 0, _stream()))
            return out
        mean = torch.empty(d, dtype=torch.float32, device=table.device)
        need = int(lib.manner_hip_table_to_f16_workspace_bytes(d))
        ws = torch.empty(need, dtype=torch.uint8, device=table.device)
        _lib.check(lib.manner_hip_table_to_f16(_ptr(table), n, d, _ptr(mean), _ptr(out), _ptr(ws), need, _stream()))
    return HalfTable(out, mean)


def score_user(table: Tensor, user: Tensor, cand_idx: Tensor, cand_off: Tensor, total_cand: Optional[int] = None) -> Tensor:
    """Ragged scores [sum c_i] = <user[i], table[cand_idx[j]]> for the candidates j of impression i (the early-fusion
    tail of CRModule.forward, cr_module.py:125-129, without the dense candidate tensor)."""
    table = _dev(table, torch.float32, "table").contiguous()
    user = _dev(user, torch.float32, "user_vector").contiguous()
    cand_idx = _dev(cand_idx, torch.int32, "cand_idx").contiguous()
    cand_off = _dev(cand_off, torch.int64, "cand_off").contiguous()
    nb = cand_off.numel() - 1
    assert user.shape == (nb, table.shape[1])
    total = int(cand_idx.numel()) if total_cand is None else total_cand
    out = torch.empty((total,), dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        _lib.check(_lib.load().manner_hip_score_user(_ptr(table), table.shape[0], table.shape[1], _ptr(user), _ptr(cand_idx),
                                                     _ptr(cand_off), nb, _ptr(out), _ptr(device_status(table.device).word),
                                                     _stream()))
    return out


def to_dense(x: Tensor, off: Tensor, width: int, fill: Optional[Tensor] = None, with_mask: bool = False):
    """K9 (``to_dense_batch``): ragged rows x [sum n_i, *] + offsets int64 [B+1] -> dense [B, width, *]; padded slots
    hold 0 (or ``fill[b]``).  ``width`` is given by the caller — no device read-back.  With ``with_mask`` also the
    bool [B, width] mask of real slots."""
    x = _dev(x, torch.float32, "x").contiguous()
    off = _dev(off, torch.int64, "off").contiguous()
    nb = off.numel() - 1
    inner = tuple(x.shape[1:])
    d = 1
    for v in inner:
        d *= int(v)
    if fill is not None:
        fill = _dev(fill, torch.float32, "fill").contiguous()
        assert fill.numel() == nb
    dense = torch.empty((nb, width) + inner, dtype=torch.float32, device=x.device)
    mask = torch.empty((nb, width), dtype=torch.uint8, device=x.device) if with_mask else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().manner_hip_to_dense(_ptr(x), _ptr(off), nb, int(width), d, _ptr(fill), _ptr(dense), _ptr(mask),
                                                   _stream()))
    return (dense, mask.bool()) if with_mask else dense


def zscore_fuse(planes: Tensor, weights: Sequence[float], cand_off: Tensor, with_pad_value: bool = False):
    """planes [K, total] (module 0 = CR); weights of modules 1..K-1 -> fused ragged scores [total].  With
    ``with_pad_value`` also the per-impression value [B] that the reference's dense matrix holds in padded slots
    (its z-score runs over the zero-padded row, ensemble_module.py:145-149)."""
    planes = _dev(planes, torch.float32, "scores")
    if planes.dim() != 2 or planes.stride(1) != 1:
        planes = planes.contiguous()               # planes may be row views of a wider buffer (stride(0) > total)
    cand_off = _dev(cand_off, torch.int64, "cand_off").contiguous()
    k, total = planes.shape
    assert len(weights) == k - 1
    w = (C.c_float * max(1, k - 1))(*[float(v) for v in weights])
    out = torch.empty((total,), dtype=torch.float32, device=planes.device)
    pad = torch.empty((cand_off.numel() - 1,), dtype=torch.float32, device=planes.device) if with_pad_value else None
    with torch.cuda.device(planes.device):
        _lib.check(_lib.load().manner_hip_zscore_fuse(_ptr(planes), planes.stride(0) if k > 1 else total, k, w, _ptr(cand_off),
                                                      cand_off.numel() - 1, _ptr(out), _ptr(pad), _stream()))
    return (out, pad) if with_pad_value else out


def rank_ndcg(scores: Tensor, labels: Optional[Tensor], cand_off: Tensor, k: int = 10, with_mrr: bool = False):
    """Per impression: top-k candidate positions int32 [B,k] (-1 padded), nDCG@k float32 [B] and, with
    ``with_mrr``, the reciprocal rank of the best-ranked positive float32 [B]."""
    scores = _dev(scores, torch.float32, "scores").contiguous()
    cand_off = _dev(cand_off, torch.int64, "cand_off").contiguous()
    nb = cand_off.numel() - 1
    topk = torch.empty((nb, k), dtype=torch.int32, device=scores.device)
    ndcg = mrr = None
    if labels is not None:
        labels = _dev(labels, torch.float32, "labels").contiguous()
        ndcg = torch.empty((nb,), dtype=torch.float32, device=scores.device)
        if with_mrr:
            mrr = torch.empty((nb,), dtype=torch.float32, device=scores.device)
    with torch.cuda.device(scores.device):
        _lib.check(_lib.load().manner_hip_rank_ndcg(_ptr(scores), _ptr(labels), _ptr(cand_off), nb, k, _ptr(topk),
                                                    _ptr(ndcg), _ptr(mrr), _stream()))
    return (topk, ndcg, mrr) if with_mrr else (topk, ndcg)


def score_fuse_rank(tables: Sequence[Tensor], weights: Sequence[float], hist_idx: Tensor, hist_off: Tensor, cand_idx: Tensor, cand_off: Tensor,
                    labels: Optional[Tensor] = None, k: int = 10, with_pad_value: bool = False):
    """SURVEY §8e phase C in ONE launch (manner_hip_score_fuse_rank): K module tables [n, D] (D = 768 / 1024, float32) -> fused ragged
    scores [sum c_i] (K == 1: the raw late-fusion scores), top-k positions int32 [B, k], nDCG@k and MRR float32 [B] (with labels);
    bit-identical to score_late_fusion x K -> zscore_fuse -> rank_ndcg.  Returns a dict like hotpath.score_impressions."""
    tables = [_dev(t, torch.float32, "table").contiguous() for t in tables]
    kk = len(tables)
    assert kk >= 1 and len(weights) == kk - 1 and all(t.shape == tables[0].shape for t in tables)
    dev = tables[0].device
    hist_idx, cand_idx = _dev(hist_idx, torch.int32, "hist_idx").contiguous(), _dev(cand_idx, torch.int32, "cand_idx").contiguous()
    hist_off, cand_off = _dev(hist_off, torch.int64, "hist_off").contiguous(), _dev(cand_off, torch.int64, "cand_off").contiguous()
    nb, total = hist_off.numel() - 1, int(cand_idx.numel())
    scores = torch.empty((total,), dtype=torch.float32, device=dev)
    topk = torch.empty((nb, k), dtype=torch.int32, device=dev)
    pad = torch.empty((nb,), dtype=torch.float32, device=dev) if with_pad_value else None
    ndcg = mrr = None
    if labels is not None:
        labels = _dev(labels, torch.float32, "labels").contiguous()
        ndcg, mrr = torch.empty((nb,), dtype=torch.float32, device=dev), torch.empty((nb,), dtype=torch.float32, device=dev)
    lib = _lib.load()
    nbytes = int(lib.manner_hip_score_fuse_rank_workspace_bytes(kk, total))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tp = (C.c_void_p * kk)(*[t.data_ptr() for t in tables])
    w = (C.c_float * max(1, kk - 1))(*[float(v) for v in weights])
    with torch.cuda.device(dev):
        _lib.check(lib.manner_hip_score_fuse_rank(tp, kk, w, tables[0].shape[0], tables[0].shape[1], _ptr(hist_idx), _ptr(hist_off), _ptr(cand_idx),
                                                  _ptr(cand_off), nb, total, _ptr(labels), k, _ptr(scores), _ptr(pad), _ptr(topk), _ptr(ndcg),
                                                  _ptr(mrr), ws.data_ptr(), nbytes, _ptr(device_status(dev).word), _stream()))
    res = {"scores": scores, "topk": topk, "ndcg": ndcg, "mrr": mrr}
    if with_pad_value:
        res["pad"] = pad
    return res


def aspect_metrics(topk: Tensor, cand_aspect: Tensor, cand_off: Tensor, num_classes: int,
                   hist_aspect: Optional[Tensor] = None, hist_off: Optional[Tensor] = None):
    """Aspect Diversity@k (and, with the history aspects, Personalization@k) per impression from the
    top-k positions of ``rank_ndcg``: float32 [B] each."""
    topk = _dev(topk, torch.int32, "topk").contiguous()
    cand_aspect = _dev(cand_aspect, torch.int32, "cand_aspect").contiguous()
    cand_off = _dev(cand_off, torch.int64, "cand_off").contiguous()
    nb, k = topk.shape
    div = torch.empty((nb,), dtype=torch.float32, device=topk.device)
    pers = None
    if hist_aspect is not None:
        hist_aspect = _dev(hist_aspect, torch.int32, "hist_aspect").contiguous()
        hist_off = _dev(hist_off, torch.int64, "hist_off").contiguous()
        pers = torch.empty((nb,), dtype=torch.float32, device=topk.device)
    with torch.cuda.device(topk.device):
        _lib.check(_lib.load().manner_hip_aspect_metrics(_ptr(topk), _ptr(cand_aspect), _ptr(hist_aspect), _ptr(cand_off),
                                                         _ptr(hist_off), nb, k, num_classes, _ptr(div), _ptr(pers), _stream()))
    return div, pers


def auc(scores: Tensor, labels: Tensor, sigmoid_rule: bool = True, return_counts: bool = False):
    """Global binary AUC over every (score, label) pair — torchmetrics ``AUROC(task="binary")`` as the
    reference feeds it (cr_module.py:81, :267-273).  Returns a float64 scalar tensor on the device (and, with
    ``return_counts``, the exact int64 triple ``[2U, P, N]``).  -0 and +0 are one threshold, denormals are kept apart.
    Known divergence: NaN *scores*.  torchmetrics treats every NaN as a threshold of its own (NaN != NaN); here NaNs of equal bits
    tie and sort past +inf (negative-sign NaNs below -inf).  Scores are expected to be NaN-free."""
    scores = _dev(scores, torch.float32, "scores").contiguous().reshape(-1)
    labels = _dev(labels, torch.float32, "labels").contiguous().reshape(-1)
    n = scores.numel()
    if labels.numel() != n or n == 0:
        raise ValueError("auc: scores and labels must be non-empty and of equal size")
    lib = _lib.load()
    ws_bytes = lib.manner_hip_auc_workspace_bytes(n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=scores.device)
    out = torch.empty((1,), dtype=torch.float64, device=scores.device)
    counts = torch.empty((3,), dtype=torch.int64, device=scores.device)
    with torch.cuda.device(scores.device):
        _lib.check(lib.manner_hip_auc(_ptr(scores), _ptr(labels), n, int(bool(sigmoid_rule)), _ptr(ws), ws_bytes, _ptr(out),
                                      _ptr(counts), _stream()))
    return (out[0], counts) if return_counts else out[0]


# ---------------------------------------------------------------- device-side collate
def collate_segments(off: Tensor) -> Tensor:
    """``repeat_interleave(arange(B), sizes)`` from int64 offsets [B+1] (reference _make_batch_assignees,
    mind_rec_dataset.py:171-174).  ``off[-1]`` is read on the host once to size the output."""
    off = _dev(off, torch.int64, "off").contiguous()
    nb = off.numel() - 1
    total = int(off[-1]) if nb > 0 else 0
    seg = torch.empty((total,), dtype=torch.int64, device=off.device)
    with torch.cuda.device(off.device):
        _lib.check(_lib.load().manner_hip_collate_segments(_ptr(off), nb, total, _ptr(seg), _stream()))
    return seg


def collate_segments_sized(off: Tensor, total: int) -> Tensor:
    """As ``collate_segments`` when the host already knows ``off[-1]`` (no device read)."""
    off = _dev(off, torch.int64, "off").contiguous()
    seg = torch.empty((total,), dtype=torch.int64, device=off.device)
    with torch.cuda.device(off.device):
        _lib.check(_lib.load().manner_hip_collate_segments(_ptr(off), off.numel() - 1, total, _ptr(seg), _stream()))
    return seg


def collate_text(store_ids: Tensor, store_len: Tensor, rows: Tensor, padded_len: int, pad_id: int):
    """BatchEncoding tensors (ids, mask: int64 [M, padded_len]) of the store rows ``rows``."""
    store_ids = _dev(store_ids, torch.int32, "store_ids").contiguous()
    store_len = _dev(store_len, torch.int32, "store_len").contiguous()
    rows = _dev(rows, torch.int32, "rows").contiguous()
    m = rows.numel()
    ids = torch.empty((m, padded_len), dtype=torch.int64, device=rows.device)
    mask = torch.empty((m, padded_len), dtype=torch.int64, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(_lib.load().manner_hip_collate_text(_ptr(store_ids), _ptr(store_len), store_ids.shape[0], store_ids.shape[1],
                                                       _ptr(rows), m, padded_len, pad_id, _ptr(ids), _ptr(mask), _stream()))
    return ids, mask


def collate_entities(store_ent: Tensor, store_cnt: Tensor, rows: Tensor, width: int) -> Tensor:
    """Entity index matrix int64 [M, width], right-padded with 0 (reference _tokenize_entities)."""
    store_ent = _dev(store_ent, torch.int32, "store_ent").contiguous()
    store_cnt = _dev(store_cnt, torch.int32, "store_cnt").contiguous()
    rows = _dev(rows, torch.int32, "rows").contiguous()
    m = rows.numel()
    out = torch.empty((m, width), dtype=torch.int64, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(_lib.load().manner_hip_collate_entities(_ptr(store_ent), _ptr(store_cnt), store_ent.shape[0],
                                                           store_ent.shape[1], _ptr(rows), m, width, _ptr(out), _stream()))
    return out


def collate_aspects(category: Tensor, sentiment: Tensor, sentiment_score: Tensor, rows: Tensor):
    """category / sentiment int64 [M] and sentiment_score float32 [M] of the store rows ``rows``."""
    category = _dev(category, torch.int32, "category").contiguous()
    sentiment = _dev(sentiment, torch.int32, "sentiment").contiguous()
    sentiment_score = _dev(sentiment_score, torch.float32, "sentiment_score").contiguous()
    rows = _dev(rows, torch.int32, "rows").contiguous()
    m = rows.numel()
    ocat = torch.empty((m,), dtype=torch.int64, device=rows.device)
    osent = torch.empty((m,), dtype=torch.int64, device=rows.device)
    oscore = torch.empty((m,), dtype=torch.float32, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(_lib.load().manner_hip_collate_aspects(_ptr(category), _ptr(sentiment), _ptr(sentiment_score),
                                                          category.numel(), _ptr(rows), m, _ptr(ocat), _ptr(osent), _ptr(oscore),
                                                          _stream()))
    return ocat, osent, oscore


# ---------------------------------------------------------------- training batches: negative sampling on the device
def sample_candidates(cand_rows: Tensor, labels: Tensor, cand_off: Tensor, imp_idx: Tensor, out_off: Tensor, out_total: int,
                      ratio: int, seed: int, epoch: int, users: Optional[Tensor] = None, return_pos: bool = False):
    """The training candidates of the impressions ``imp_idx`` (int64 [B], any order, repeats allowed) of a data set held as CSR
    arrays (``cand_rows`` int32 / ``labels`` f32 [total], ``cand_off`` int64 [n_imp + 1]): every clicked candidate and ``ratio``
    non-clicked ones per click, in a random order — MINDRecDatasetTrain._sample_candidates (reference mind_rec_dataset.py:13-77) as the
    counter-based rule of include/manner_hip.h, a pure function of (seed, epoch, impression).  ``out_off`` int64 [B + 1] is the host's
    prefix sum of ``p * (1 + ratio)`` and ``out_total`` its last element, so nothing is read back.
    -> (rows int32 [out_total], labels f32 [out_total], users int64 [B] or None, positions int32 [out_total] or None).
    A bad index or an ``out_off`` that disagrees with the labels raises through the device status word (``check_status``)."""
    cand_rows = _dev(cand_rows, torch.int32, "cand_rows").contiguous()
    labels = _dev(labels, torch.float32, "labels").contiguous()
    cand_off = _dev(cand_off, torch.int64, "cand_off").contiguous()
    imp_idx = _dev(imp_idx, torch.int64, "imp_idx").contiguous()
    out_off = _dev(out_off, torch.int64, "out_off").contiguous()
    nb, total = imp_idx.numel(), cand_rows.numel()
    if labels.numel() != total or cand_off.numel() < 1 or out_off.numel() != nb + 1 or out_total < 0 or ratio < 0:
        raise ValueError("sample_candidates: labels / cand_off / out_off do not fit cand_rows and imp_idx")
    dev = cand_rows.device
    if users is not None:
        users = _dev(users, torch.int64, "users").contiguous()
        if users.numel() != cand_off.numel() - 1:
            raise ValueError("sample_candidates: users must hold one entry per impression")
    rows = torch.empty((out_total,), dtype=torch.int32, device=dev)
    lab = torch.empty((out_total,), dtype=torch.float32, device=dev)
    pos = torch.empty((out_total,), dtype=torch.int32, device=dev) if return_pos else None
    out_users = torch.empty((nb,), dtype=torch.int64, device=dev) if users is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().manner_hip_sample_candidates(
            _ptr(cand_rows), _ptr(labels), _ptr(cand_off), cand_off.numel() - 1, total, _ptr(users), _ptr(imp_idx), nb, _ptr(out_off),
            out_total, ratio, seed & (2 ** 64 - 1), epoch & (2 ** 64 - 1), _ptr(rows), _ptr(lab), _ptr(pos), _ptr(out_users),
            _ptr(device_status(dev).word), _stream()))
    return rows, lab, out_users, pos


def gather_segments(src: Tensor, src_off: Tensor, imp_idx: Tensor, out_off: Tensor, out_total: int, src_f: Optional[Tensor] = None):
    """Ragged gather: segment b of the result is segment ``imp_idx[b]`` of ``src`` (int32 [total], ``src_off`` int64 [n_seg + 1]);
    ``out_off`` int64 [B + 1] / ``out_total`` are the host's prefix sum of the segment lengths.  ``src_f``: an f32 array gathered
    alike.  -> out int32 [out_total] (, out_f f32 [out_total])."""
    src = _dev(src, torch.int32, "src").contiguous()
    src_off = _dev(src_off, torch.int64, "src_off").contiguous()
    imp_idx = _dev(imp_idx, torch.int64, "imp_idx").contiguous()
    out_off = _dev(out_off, torch.int64, "out_off").contiguous()
    nb = imp_idx.numel()
    if src_off.numel() < 1 or out_off.numel() != nb + 1 or out_total < 0:
        raise ValueError("gather_segments: src_off / out_off do not fit imp_idx")
    dev = src.device
    if src_f is not None:
        src_f = _dev(src_f, torch.float32, "src_f").contiguous()
        if src_f.numel() != src.numel():
            raise ValueError("gather_segments: src_f must have the size of src")
    out = torch.empty((out_total,), dtype=torch.int32, device=dev)
    out_f = torch.empty((out_total,), dtype=torch.float32, device=dev) if src_f is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().manner_hip_gather_segments(_ptr(src), _ptr(src_f), _ptr(src_off), src_off.numel() - 1, src.numel(),
                                                          _ptr(imp_idx), nb, _ptr(out_off), out_total, _ptr(out), _ptr(out_f),
                                                          _ptr(device_status(dev).word), _stream()))
    return out if src_f is None else (out, out_f)


def rows_max_len(store_len: Tensor, rows: Tensor, store_cnt: Optional[Tensor] = None) -> Tensor:
    """Device int32 [2]: the longest stored news and (``store_cnt`` given) the longest entity list among the store rows ``rows``."""
    store_len = _dev(store_len, torch.int32, "store_len").contiguous()
    rows = _dev(rows, torch.int32, "rows").contiguous()
    if store_cnt is not None:
        store_cnt = _dev(store_cnt, torch.int32, "store_cnt").contiguous()
    out = torch.empty((2,), dtype=torch.int32, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(_lib.load().manner_hip_rows_max_len(_ptr(store_len), _ptr(store_cnt), store_len.numel(), _ptr(rows), rows.numel(),
                                                       _ptr(out), _stream()))
    return out


# ---------------------------------------------------------------- A-Module batches: M-per-class sampling on the device
def sample_m_per_class(class_off: Tensor, class_members: Tensor, class_label: Tensor, rows: Tensor, store_len: Tensor,
                       store_cnt: Optional[Tensor], m: int, k: int, nb: int, seed: int, epoch: int):
    """A whole epoch of M-per-class batches in one call (include/manner_hip.h, "A-Module batches"): ``nb`` batches of ``k`` classes
    times ``m`` members over the class tables ``class_off`` int64 [L + 1] / ``class_members`` int32 [N] / ``class_label`` int64 [L];
    ``rows`` int32 [N] maps a data-set index to its store row.  A pure function of (seed, epoch) and the tables.
    -> (idx int32 [nb * k * m], store rows int32 [nb * k * m], labels int64 [nb * k * m], widths int32 [nb, 2]: per batch the longest
    token row and entity list, 0 for ``store_cnt`` None).  Nothing is read back; a bad ``rows`` entry raises through the device status
    word (``check_status``), sizes outside the kernel's bounds raise here, before any launch."""
    class_off = _dev(class_off, torch.int64, "class_off").contiguous()
    class_members = _dev(class_members, torch.int32, "class_members").contiguous()
    class_label = _dev(class_label, torch.int64, "class_label").contiguous()
    rows = _dev(rows, torch.int32, "rows").contiguous()
    store_len = _dev(store_len, torch.int32, "store_len").contiguous()
    if store_cnt is not None:
        store_cnt = _dev(store_cnt, torch.int32, "store_cnt").contiguous()
    n_cls, n = class_label.numel(), class_members.numel()
    if class_off.numel() != n_cls + 1 or rows.numel() != n or (store_cnt is not None and store_cnt.numel() != store_len.numel()):
        raise ValueError("sample_m_per_class: class_off / rows / store_cnt do not fit class_label, class_members and store_len")
    dev = rows.device
    total = max(int(nb), 0) * max(int(k), 0) * max(int(m), 0)
    if total >= 2 ** 31:
        raise ValueError("sample_m_per_class: nb * k * m overflows 2^31")
    idx = torch.empty((total,), dtype=torch.int32, device=dev)
    out_rows = torch.empty((total,), dtype=torch.int32, device=dev)
    labels = torch.empty((total,), dtype=torch.int64, device=dev)
    width = torch.empty((max(int(nb), 0), 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().manner_hip_sample_m_per_class(
            _ptr(class_off), _ptr(class_members), _ptr(class_label), n_cls, n, _ptr(rows), _ptr(store_len), _ptr(store_cnt),
            store_len.numel(), m, k, nb, seed & (2 ** 64 - 1), epoch & (2 ** 64 - 1), _ptr(idx), _ptr(out_rows), _ptr(labels),
            _ptr(width), _ptr(device_status(dev).word), _stream()))
    return idx, out_rows, labels, width


def eval_loss(scores: Tensor, labels: Tensor, cand_off: Tensor, supcon: bool = True, temperature: float = 0.1,
              c_max: Optional[int] = None, reduce: bool = True):
    """Loss of ``CRModule.model_step`` (cr_module.py:140-171) from the ragged scores: SupCon on the score matrix
    (``supcon=True``, losses.py:12-40; batch value = mean of the non-zero per-impression losses, the
    pytorch_metric_learning default reducer for SupConLoss) or CrossEntropyLoss with probability targets over the
    zero-padded row of width ``c_max`` (default: the batch maximum; batch value = mean)."""
    scores = _dev(scores, torch.float32, "scores").contiguous()
    labels = _dev(labels, torch.float32, "labels").contiguous()
    cand_off = _dev(cand_off, torch.int64, "cand_off").contiguous()
    nb = cand_off.numel() - 1
    if not supcon and c_max is None:
        c_max = int((cand_off[1:] - cand_off[:-1]).max())
    losses = torch.empty((nb,), dtype=torch.float32, device=scores.device)
    with torch.cuda.device(scores.device):
        _lib.check(_lib.load().manner_hip_eval_loss(_ptr(scores), _ptr(labels), _ptr(cand_off), nb, 0 if supcon else 1,
                                                    C.c_float(temperature if supcon else 1.0), int(c_max or 1), _ptr(losses), _stream()))
    if not reduce:
        return losses
    if not supcon:
        return losses.mean()
    if supcon and (not bool((labels > 0.5).any()) or not bool((labels <= 0.5).any())):
        return losses.sum() * 0                       # losses.py:24-25, 40: no positive or no negative pair in the batch
    nz = losses > 0
    return torch.where(nz.any(), (losses * nz).sum() / nz.sum().clamp(min=1), losses.sum() * 0)


# ---------------------------------------------------------------- t-SNE (csrc/tsne.hip)
# the launchers' tiles, for the tests: rows / j rows per workgroup of the repulsion kernel, query / candidate rows per tile of the
# neighbour search, rows per workgroup of the step and KL kernels
TSNE_TILE_I, TSNE_TILE_J, KNN_TILE_Q, KNN_TILE_C, TSNE_STEP_ROWS = 512, 512, 32, 64, 64
_TSNE_TARGET_WG = 1024


def tsne_j_split(n: int) -> int:
    """The number of j slices the repulsion launcher cuts N rows into — a function of N alone: enough slices for about 1024 workgroups,
    never more than there are j tiles.  The library refuses any other value."""
    if n <= 0:
        return 1
    nb, jt = -(-n // TSNE_TILE_I), -(-n // TSNE_TILE_J)
    return max(1, min(-(-_TSNE_TARGET_WG // nb), jt))


def knn(x: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """x f32 [N, D] -> (idx int32 [N, k], d2 f32 [N, k]): the k nearest other rows of every row by squared Euclidean distance, exact,
    ascending by (d2, idx).  D <= 1024, 1 <= k <= 255, k <= N - 1, N <= 2^20."""
    x = _dev(x, torch.float32, "x").contiguous()
    if x.dim() != 2:
        raise ValueError("knn: x must be [N, D]")
    n, d = x.shape
    idx = torch.empty((n, max(int(k), 0)), dtype=torch.int32, device=x.device)
    d2 = torch.empty((n, max(int(k), 0)), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().manner_hip_knn_rows_f32(_ptr(x), n, d, int(k), _ptr(idx), _ptr(d2), _stream()))
    return idx, d2


def tsne_affinities(d2: Tensor, perplexity: float) -> Tuple[Tensor, Tensor]:
    """d2 f32 [N, k] -> (p [N, k], beta [N]): per row the conditional distribution over its k neighbours whose entropy is
    log(perplexity) within 1e-5, and the beta the search ended on."""
    d2 = _dev(d2, torch.float32, "d2").contiguous()
    n, k = d2.shape
    p = torch.empty_like(d2)
    beta = torch.empty((n,), dtype=torch.float32, device=d2.device)
    with torch.cuda.device(d2.device):
        _lib.check(_lib.load().manner_hip_tsne_affinities(_ptr(d2), n, k, C.c_float(perplexity), _ptr(p), _ptr(beta), _stream()))
    return p, beta


def tsne_repulsion(y: Tensor, part: Optional[Tensor] = None, zpart: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """y f32 [N, 2] -> (part f32 [split, N, 4], zpart f64 [split * ceil(N / TSNE_TILE_I)]).  part[s, i] = (sum q^2 dx, sum q^2 dy, sum q, 0)
    of row i over the j rows of slice s, q = 1 / (1 + |y_i - y_j|^2), the self pair (q = 1, force 0) included; Z = zpart.sum() - N."""
    y = _dev(y, torch.float32, "y").contiguous()
    n = y.shape[0]
    s = tsne_j_split(n)
    if part is None:
        part = torch.empty((s, n, 4), dtype=torch.float32, device=y.device)
        zpart = torch.empty((s * -(-n // TSNE_TILE_I),), dtype=torch.float64, device=y.device)
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().manner_hip_tsne_repulsion(_ptr(y), n, s, _ptr(part), _ptr(zpart), _stream()))
    return part, zpart


def tsne_step(y: Tensor, part: Tensor, zpart: Tensor, out_idx: Tensor, out_p: Tensor, in_off: Tensor, in_src: Tensor, in_p: Tensor, u: Tensor,
              gains: Tensor, y_out: Tensor, ypart: Tensor, exaggeration: float, momentum: float, learning_rate: float) -> Tensor:
    """One iteration from the repulsion sums of ``y``: ``u`` and ``gains`` [N, 2] are updated in place, ``y_out`` (not ``y``) receives the
    new, centred coordinates; ``ypart`` f64 [2 * ceil(N / TSNE_STEP_ROWS)] is scratch.  Edges: ``out_idx`` int32 / ``out_p`` [N, k] and
    their transpose ``in_off`` int64 [N + 1] / ``in_src`` int32 / ``in_p``.  Every tensor as the library wants it (contiguous, its dtype):
    this is called a thousand times per fit and converts nothing."""
    n, k = out_idx.shape
    for t, dt, name in ((y, torch.float32, "y"), (part, torch.float32, "part"), (zpart, torch.float64, "zpart"), (out_idx, torch.int32, "out_idx"),
                        (out_p, torch.float32, "out_p"), (in_off, torch.int64, "in_off"), (in_src, torch.int32, "in_src"), (in_p, torch.float32, "in_p"),
                        (u, torch.float32, "u"), (gains, torch.float32, "gains"), (y_out, torch.float32, "y_out"), (ypart, torch.float64, "ypart")):
        if not _dev(t, dt, name).is_contiguous():
            raise ValueError(f"tsne_step: {name} must be contiguous")
    s = tsne_j_split(n)
    if (part.numel() != s * n * 4 or zpart.numel() != s * -(-n // TSNE_TILE_I) or ypart.numel() < 2 * -(-n // TSNE_STEP_ROWS) or in_off.numel() != n + 1
            or any(t.numel() != 2 * n for t in (y, u, gains, y_out)) or out_p.numel() != n * k or in_p.numel() != in_src.numel()):
        raise ValueError("tsne_step: buffer sizes do not fit N, k and the split")
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().manner_hip_tsne_step(_ptr(y), _ptr(part), _ptr(zpart), s, _ptr(out_idx), _ptr(out_p), k, _ptr(in_off), _ptr(in_src),
                                                    _ptr(in_p), in_src.numel(), n, C.c_float(exaggeration), C.c_float(momentum),
                                                    C.c_float(learning_rate), _ptr(u), _ptr(gains), _ptr(y_out), _ptr(ypart), _stream()))
    return y_out


def tsne_kl(y: Tensor, out_idx: Tensor, out_p: Tensor, zpart: Optional[Tensor] = None) -> Tensor:
    """Device f64 [1]: KL(P || Q) of the embedding ``y`` [N, 2] over the non-zero entries of the symmetrised P of the directed edges
    ``out_idx`` / ``out_p`` [N, k].  ``zpart``: that of a repulsion call on the same ``y`` (computed here when None)."""
    y = _dev(y, torch.float32, "y").contiguous()
    out_idx = _dev(out_idx, torch.int32, "out_idx").contiguous()
    out_p = _dev(out_p, torch.float32, "out_p").contiguous()
    n, k = out_idx.shape
    if y.numel() != 2 * n or out_p.numel() != n * k:
        raise ValueError("tsne_kl: y / out_p do not fit out_idx")
    if zpart is None:
        zpart = tsne_repulsion(y)[1]
    s = tsne_j_split(n)
    if _dev(zpart, torch.float64, "zpart").numel() != s * -(-n // TSNE_TILE_I) or not zpart.is_contiguous():
        raise ValueError("tsne_kl: zpart does not fit N and the split")
    klpart = torch.empty((max(-(-n // TSNE_STEP_ROWS), 1),), dtype=torch.float64, device=y.device)
    kl = torch.zeros((1,), dtype=torch.float64, device=y.device)
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().manner_hip_tsne_kl(_ptr(y), _ptr(zpart), s, _ptr(out_idx), _ptr(out_p), k, n, _ptr(klpart), _ptr(kl), _stream()))
    return kl
