"""numpy model of the token-packed frozen-prefix store (csrc/cache.hip manner_hip_prefix_*; hip.PackedPrefixCache), shared by
tests/test_prefix_packed_host.py (against a dictionary keyed by real tokens) and tests/test_gpu_prefix_packed.py (against the device).

The rules it restates: the lookup hands every new key a table row once (state 1 for one occurrence, state 0 for its repeats, state 2
when the table is full); `resolve` turns a state-0 occurrence of a key without payload into state 2; `reserve` adds a stored row's real
tokens to ONE counter and keeps the payload only if offset + length stays inside the pool (otherwise row_len = -2: key known, no
payload, for good); `store` copies the real tokens; `gather` pads a payload with zeros to the call's width and takes every other row
from the fresh encode — its own row, or the row of the state-1 occurrence of its key.  The order in which one call's rows reserve is
free on the device (one atomic add each); the model takes it as an argument so that a test can try several."""
import numpy as np


def check_layout(row_off, row_len, tok_count, pool_tokens, rows_handed_out):
    """Invariants of the per-row metadata, on the model's arrays or on copies of the device's: payloads lie inside the pool, do not
    overlap, and account for no more tokens than were handed out.  Returns (stored rows, rows without payload)."""
    row_off, row_len = np.asarray(row_off, np.int64), np.asarray(row_len, np.int64)
    used = min(int(rows_handed_out), len(row_len))
    assert set(np.unique(row_len[used:]).tolist()) <= {-1}                 # rows never handed out were never touched
    live = np.nonzero(row_len[:used] >= 1)[0]
    none = np.nonzero(row_len[:used] == -2)[0]
    assert len(live) + len(none) == used                                    # between calls no row is left "not attempted"
    start, end = row_off[live], row_off[live] + row_len[live]
    assert (start >= 0).all() and (end <= pool_tokens).all()
    order = np.argsort(start)
    assert (end[order][:-1] <= start[order][1:]).all()
    assert int(row_len[live].sum()) <= int(tok_count)
    return len(live), len(none)


class PackedStoreModel:
    def __init__(self, hidden, capacity_rows, pool_tokens):
        self.hidden, self.capacity, self.pool_tokens = hidden, capacity_rows, pool_tokens
        self.pool = np.full((pool_tokens, hidden), np.nan, np.float32)       # never-written tokens must never be returned
        self.row_of = {}                                                     # real tokens -> table row (-1: table full)
        self.row_count = 0
        self.row_off = np.zeros(capacity_rows, np.int64)
        self.row_len = np.full(capacity_rows, -1, np.int32)
        self.tok_count = 0
        self.lookups = self.encoded = 0

    def lookup(self, tokens):
        rows, state, new = [], [], set()
        for t in tokens:
            if t not in self.row_of:
                r = self.row_count if self.row_count < self.capacity else -1
                self.row_count += 1
                self.row_of[t] = r
                new.add(t)
                rows.append(r)
                state.append(1 if r >= 0 else 2)
            else:
                r = self.row_of[t]
                rows.append(r)
                state.append(0 if r >= 0 else 2)
        return np.array(rows, np.int64), np.array(state, np.int64)

    def hidden_states(self, tokens, lp, encode, reserve_order=None):
        """tokens: one tuple of real token ids per row; encode(list of tuples) -> list of [len, hidden] f32 (the rows' hidden states at
        their real positions).  Returns out [N, lp, hidden] and the indices of the rows that were encoded."""
        n = len(tokens)
        rows, state = self.lookup(tokens)
        for i in range(n):                                                   # resolve
            if state[i] == 0 and self.row_len[rows[i]] == -2:
                rows[i], state[i] = -1, 2
        todo = np.nonzero(state != 0)[0]
        self.lookups += n
        self.encoded += len(todo)
        fresh = np.zeros((len(todo), lp, self.hidden), np.float32)
        for j, h in enumerate(encode([tokens[i] for i in todo])):
            fresh[j, :len(h)] = h
        src_of, row_src = {}, {}
        for j in (range(len(todo)) if reserve_order is None else reserve_order(len(todo))):     # reserve + store
            i = int(todo[j])
            src_of[i] = j
            if state[i] != 1:
                continue
            r, ln = int(rows[i]), len(tokens[i])
            row_src[r] = j
            assert 1 <= ln <= lp
            got = -2
            if self.tok_count + ln <= self.pool_tokens:
                off = self.tok_count
                self.tok_count += ln
                self.row_off[r], got = off, ln
                self.pool[off:off + ln] = fresh[j, :ln]
            self.row_len[r] = got
        for i in todo:
            src_of.setdefault(int(i), int(np.nonzero(todo == i)[0][0]))
        out = np.full((n, lp, self.hidden), np.nan, np.float32)             # gather
        for i in range(n):
            r = int(rows[i])
            if r >= 0 and self.row_len[r] >= 1:
                off, ln = int(self.row_off[r]), int(self.row_len[r])
                assert off + ln <= self.pool_tokens and ln <= lp
                out[i, :ln], out[i, ln:] = self.pool[off:off + ln], 0.0
            else:
                out[i] = fresh[src_of[i] if state[i] != 0 else row_src[r]]
        return out, todo
