"""numpy restatement of the sampled PLM decision (include/hsp.h "sampled PLM decoding"): the Philox4x32-10 stream of
the draws and the five steps penalty -> top-p -> temperature -> top-k -> race, for the host tests and for
tools/make_golden_sampling.py."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Random123) of counters ``ctr`` [..., 4] under ``key`` [..., 2] (uint32) -> [..., 4] uint32."""
    c = [np.asarray(ctr, np.uint64)[..., i] for i in range(4)]
    key = np.asarray(key, np.uint64)
    k0, k1 = key[..., 0].copy(), key[..., 1].copy()
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack(c, -1).astype(np.uint32)


def exp_draws(seed: int, j: int, n: int = 1024) -> np.ndarray:
    """q_i ~ Exp(1), i < n, of row seed ``seed`` at code column ``j`` (float64)."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    i = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([i, np.full_like(i, j), np.zeros_like(i), np.zeros_like(i)], -1)
    key = np.broadcast_to(np.array([s & 0xFFFFFFFF, s >> 32], np.uint64), (len(i), 2))
    w = philox4x32_10(ctr, key).reshape(-1)[:n]
    u = (w >> 8).astype(np.float64) * 2.0 ** -24 + 2.0 ** -25
    return -np.log(u)


def decide_probs(logits, prev, temperature=1.0, top_k=None, top_p=None, repetition_penalty=1.0):
    """logits_to_probs restated in float32 numpy: the kept, normalised distribution [V] and the filtered logits."""
    V = logits.shape[0]
    x = np.asarray(logits, np.float32).copy()
    rp = np.float32(repetition_penalty)
    if repetition_penalty != 1.0:
        toks = np.unique([int(t) for t in prev if 0 <= int(t) < V]).astype(np.int64)
        if len(toks):
            sc = x[toks]
            x[toks] = np.where(sc < 0, sc * rp, sc / rp)
    if top_p is not None and top_p < 1.0:
        order = np.argsort(-x, kind="stable")                  # descending, ties by lower index first
        e = np.exp((x[order] - x[order[0]]).astype(np.float64))
        cum = np.cumsum(e) / e.sum()
        remove = cum > np.float32(top_p)
        remove[0] = False
        x[order[remove]] = -np.inf
    x = x / np.float32(max(temperature, 1e-5))
    if top_k is not None:
        pivot = np.sort(x)[::-1][min(top_k, V) - 1]
        x = np.where(x < pivot, np.float32(-np.inf), x)
    m = x.max()
    e = np.exp((x - m).astype(np.float64))
    return (e / e.sum()).astype(np.float32), x


def race(x, seed, j):
    """argmax_i (x_i - ln q_i) over the kept tokens (lowest index on ties) and the relative gap between the best and
    the second-best race score p_i / q_i."""
    q = exp_draws(seed, j, x.shape[0])
    keep = np.isfinite(x)
    score = np.where(keep, (x.astype(np.float64) - x[keep].max()) - np.log(q), -np.inf)
    tok = int(np.argmax(score))
    rest = np.delete(score, tok)
    gap = 1.0 - np.exp(rest.max() - score[tok]) if np.isfinite(rest.max()) else 1.0
    return tok, gap


def decide(logits, prev, seed, j, **kw):
    """(token, probs) of one row: the whole decision."""
    probs, x = decide_probs(logits, prev, **kw)
    return race(x, seed, j)[0], probs
