"""The reference of the constrained pick, in numpy on the CPU, shared by tests/test_constrain_cpu.py and tests/test_gpu_constrain.py, and the
synthetic vocabulary both use.

Row r carries an automaton over token classes: state[r] (-1 = unconstrained), cls[r][id], next[r] = its table, row-major [states][C] with
C = n_classes[r] in a row of ld_next entries.  advance: s >= 0 and the consumed token t in 0 .. V - 1 -> s2 = next[r][s * C + cls[r][t]], taken where
s2 >= 0.  mask: y[i] = x[i] where next[r][state * C + cls[r][i]] >= 0, else -inf.  Everything is exact: an output is the input's bits or -inf."""
import numpy as np


def constrain_ref(x, state, cls, nxt, n_classes, token=None):
    """x [n, V] fp32, state [n] int, cls [n, >= V] (values 0..65535), nxt [n, ld] int16, n_classes [n], token [n] or None
    -> (y [n, V] fp32, state after the advance [n] int32)."""
    x = np.asarray(x, dtype=np.float32)
    n, V = x.shape
    state = np.array(state, dtype=np.int32).copy()
    cls = np.asarray(cls).astype(np.int64) & 0xFFFF
    nxt = np.asarray(nxt).astype(np.int64)
    y = x.copy()
    for r in range(n):
        s, C = int(state[r]), int(n_classes[r])
        if s < 0:
            continue
        if token is not None and 0 <= int(token[r]) < V:
            s2 = int(nxt[r, s * C + cls[r, int(token[r])]])
            if s2 >= 0:
                s = s2
        state[r] = s
        ok = nxt[r, s * C + cls[r, :V]] >= 0
        y[r, ~ok] = -np.inf
    return y, state


def pairs_ref(y, n_slices):
    """The greedy pick's first stage: per (row, slice) the maximum of the processed row and the first index that holds it; a slice is a multiple of 4
    indices, an empty one reports (-inf, 0x7fffffff), an all -inf one its first index."""
    y = np.asarray(y, dtype=np.float32)
    n, V = y.shape
    per = (((V + n_slices - 1) // n_slices) + 3) & ~3
    pv = np.full((n, n_slices), -np.inf, dtype=np.float32)
    pi = np.full((n, n_slices), 0x7FFFFFFF, dtype=np.int32)
    for r in range(n):
        for sl in range(n_slices):
            lo, hi = min(sl * per, V), min(sl * per + per, V)
            if lo < hi:
                seg = y[r, lo:hi]
                pv[r, sl] = seg.max()
                pi[r, sl] = lo + int(np.flatnonzero(seg == seg.max())[0])
    return pv, pi


def merge_pairs(pv, pi):
    """(value, index) of a row's pairs merged as the pick merges them: the largest value, then the lower index."""
    best = pv.max()
    return float(best), int(pi[pv == best].min())


def first_argmax(y) -> int:
    y = np.asarray(y)
    return int(np.flatnonzero(y == y.max())[0])


def masked_first_argmax(x, allowed) -> int:
    """The greedy pick of raw logits x [V] under a bool mask."""
    y = np.where(np.asarray(allowed, dtype=bool), np.asarray(x, dtype=np.float32), -np.inf)
    return first_argmax(y)


# ---- the synthetic vocabulary: 1000 entries ----------------------------------------------------------------------------------------------------------
EOS_IDS = (998, 999)
SPLIT_ID = 256 + 12           # a token that ends inside a UTF-8 character: '"' + the first byte of 'é'


def synthetic_vocab(drop=()):
    """ids 0..255: the single bytes (those in `drop` are None); then multi-byte pieces, among them a token that splits a UTF-8 character and its
    completion; None entries; unrelated filler; two EOS ids (None: special tokens)."""
    tb = [None if i in set(drop) else bytes([i]) for i in range(256)]
    pieces = [b'{"', b'": ', b'true', b'12', b'false', b'", "', b'null', b'": "', b'"}', b'": [', b'], "', b', ',
              b'"' + "é".encode()[:1], "é".encode()[1:] + b'"', "é".encode(), b'ab', b'abc', b'bc', b'yes', b'no', b'no!', b'A', b'10', b'100',
              b'{\n  "', b'",\n  "', b'\n}', b'[\n    ', b',\n    ', b'\n  ]', b'":', b'  ', b'    ', b'\n', b'name', b'age', b'tags', b'"name": "', b'red', b'green',
              b'blue', b'-1', b'0.5', b'e+', b'[]', b'{}', b'1, 2', b'tr', b'ue', b'fal', b'se']
    assert pieces[SPLIT_ID - 256] == b'"\xc3'
    tb += [None if any(b in p for b in set(drop)) else p for p in pieces]       # (a piece that holds a dropped byte goes too)
    k = 0
    while len(tb) < 998:
        k += 1
        tb.append(None if k % 9 == 0 else b"~%d~" % k)            # filler no test language spells
    return tb + [None, None]


def brute_allowed(members, text: bytes, token_bytes):
    """The ids whose bytes keep `text` a prefix of some member (EOS excluded), and whether `text` is a member."""
    ok = [i for i, b in enumerate(token_bytes) if b and any(m.startswith(text + b) for m in members)]
    return set(ok), text in set(members)
