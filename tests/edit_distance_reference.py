"""The reference of the error counts and the MWER risk (include/nntoolkitcore_hip.h, "Error counts and MWER training"), in another form
than the kernel's: the kernel carries three counts forward with every cell; here the whole distance table is built first and the counts
are read off a backtrace from (m, n) that takes the first minimal predecessor in the stated order -- (1) the diagonal, a hit or
substitution, (2) (i, j-1), a deletion, (3) (i-1, j), an insertion.  Word mode splits in Python.  MWER in float64."""
import numpy as np


def split_words(seq, sep):
    """the words of seq between tokens equal to sep, as tuples; leading, trailing and repeated separators make no empty words"""
    words, cur = [], []
    for t in seq:
        if t == sep:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(int(t))
    if cur:
        words.append(tuple(cur))
    return words


def table(h, r):
    m, n = len(h), len(r)
    D = np.zeros((m + 1, n + 1), np.int64)
    D[0, :] = np.arange(n + 1)
    D[:, 0] = np.arange(m + 1)
    for i in range(1, m + 1):
        hi = h[i - 1]
        row, up = D[i], D[i - 1]
        for j in range(1, n + 1):
            row[j] = min(up[j - 1] + (hi != r[j - 1]), row[j - 1] + 1, up[j] + 1)
    return D


def counts(h, r):
    """(distance, substitutions, deletions, insertions) of hypothesis h against reference r (sequences of hashable units)"""
    h, r = list(h), list(r)
    D = table(h, r)
    i, j = len(h), len(r)
    S = Dl = I = 0
    while i > 0 or j > 0:
        if i == 0:
            Dl += 1; j -= 1
        elif j == 0:
            I += 1; i -= 1
        elif D[i, j] == D[i - 1, j - 1] + (h[i - 1] != r[j - 1]):
            S += int(h[i - 1] != r[j - 1]); i -= 1; j -= 1
        elif D[i, j] == D[i, j - 1] + 1:
            Dl += 1; j -= 1
        else:
            assert D[i, j] == D[i - 1, j] + 1
            I += 1; i -= 1
    assert S + Dl + I == D[len(h), len(r)]
    return int(D[len(h), len(r)]), S, Dl, I


def counts_fast(h, r):
    """the same four numbers for long pairs: the table by numpy rows (the deletion chain of a row is a running minimum), then the same
    backtrace.  Checked against counts() by the host tests."""
    h, r = list(h), list(r)
    m, n = len(h), len(r)
    req = {}
    D = np.zeros((m + 1, n + 1), np.int32)
    D[0, :] = np.arange(n + 1)
    D[:, 0] = np.arange(m + 1)
    idx = np.arange(n + 1, dtype=np.int64)
    for i in range(1, m + 1):
        hi = h[i - 1]
        if hi not in req:
            req[hi] = np.array([hi != x for x in r], dtype=np.int32) if n else np.zeros(0, np.int32)
        up = D[i - 1]
        c = np.empty(n + 1, np.int64)
        c[0] = i
        c[1:] = np.minimum(up[:-1] + req[hi], up[1:] + 1)
        # row[j] = min over k <= j of c[k] + (j - k)
        D[i] = np.minimum.accumulate(c - idx) + idx
    i, j = m, n
    S = Dl = I = 0
    while i > 0 or j > 0:
        if i == 0:
            Dl += 1; j -= 1
        elif j == 0:
            I += 1; i -= 1
        elif D[i, j] == D[i - 1, j - 1] + (h[i - 1] != r[j - 1]):
            S += int(h[i - 1] != r[j - 1]); i -= 1; j -= 1
        elif D[i, j] == D[i, j - 1] + 1:
            Dl += 1; j -= 1
        else:
            I += 1; i -= 1
    return int(D[m, n]), S, Dl, I


def batch_counts(hyp, hyp_lengths, refs, sep=-1, fast=False):
    """hyp [B][n_hyp][L] and hyp_lengths [B][n_hyp] as the decoders leave them, refs a list of B lists -> (counts [B][n_hyp][4],
    reference units [B]), with the call's rules: a length < 0 gives -1s, a length above L is read as L"""
    hyp = np.asarray(hyp)
    if hyp.ndim == 2:
        hyp = hyp[:, None, :]
    B, n_hyp, L = hyp.shape
    hl = np.asarray(hyp_lengths).reshape(B, n_hyp)
    out = np.zeros((B, n_hyp, 4), np.int32)
    units = np.zeros(B, np.int32)
    fn = counts_fast if fast else counts
    for b in range(B):
        r = [int(x) for x in refs[b]]
        r = split_words(r, sep) if sep >= 0 else r
        units[b] = len(r)
        for k in range(n_hyp):
            if hl[b, k] < 0:
                out[b, k] = -1
                continue
            h = [int(x) for x in hyp[b, k, :min(int(hl[b, k]), L)]]
            h = split_words(h, sep) if sep >= 0 else h
            out[b, k] = fn(h, r)
    return out, units


def mwer(logp, err):
    """float64 risk [B] and d risk / d logp [B][n_hyp] of the MWER definition; err < 0 marks an invalid slot"""
    logp = np.asarray(logp, np.float64)
    err = np.asarray(err, np.int64)
    B, N = logp.shape
    risk, grad = np.zeros(B), np.zeros((B, N))
    for b in range(B):
        v = err[b] >= 0
        if not v.any() or not np.isfinite(logp[b][v]).any():
            continue
        lp, e = logp[b][v], err[b][v].astype(np.float64)
        mx = lp.max()
        p = np.exp(lp - mx)
        p /= p.sum()
        c = e - e.mean()
        risk[b] = float((p * c).sum())
        grad[b][v] = p * (c - risk[b])
    return risk, grad
