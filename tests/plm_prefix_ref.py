"""Float64 restatement of prosody-LM decoding behind a given code prefix, for the tests of hsp_plm_prefill_attn_f32,
Megatts2PLM1.prefill / infer(prefix_codes=) and PlmDecodeSession.admit(prefix_codes=).  Built on tests/plm_causal_ref.py:

  * ``forced_decode``: the K/V-cached float64 decode with the first P codes of every row forced (R.greedy_decode's
    ``choose`` hook), and ``forced_decode_caches``: the same loop, also returning every layer's caches;
  * ``prefill_attn``: the contract of hsp_plm_prefill_attn_f32 (include/hsp.h "PLM prefill") for one row: the per-head
    causal softmax of R.layer_full, on a stacked q | k | v matrix.
"""
import numpy as np

import plm_causal_ref as R


def forced_decode(sd, tc, prefixes):
    """R.greedy_decode with codes[b, :P_b] = prefixes[b] forced: codes [B, T], logits [B, T, vq_bins], margin [B, T]
    (entries at t < P_b belong to forced positions: their logits are those of teacher forcing)."""
    choose = lambda lg, b, t, prev: int(prefixes[b][t]) if t < len(prefixes[b]) else int(np.argmax(lg))
    return R.greedy_decode(sd, tc, choose=choose)


def forced_decode_caches(sd, tc, prefixes):
    """The loop of R.greedy_decode (same steps, R.decode_layer) with forced prefixes -> codes, logits, margin and the
    per-layer caches [(k [B, D, T], v [B, D, T])]."""
    B, _, T = tc.shape
    ws = [R.layer_weights(sd, i) for i in range(R.N_LAYERS)]
    kv = [(np.full((B, R.D_MODEL, T), np.nan), np.full((B, R.D_MODEL, T), np.nan)) for _ in ws]
    pe = R.pos_table(T)
    codes = np.full((B, T + 1), R.GO_ID, np.int64)
    logits = np.empty((B, T, R.VQ_BINS))
    margin = np.empty((B, T))
    for t in range(T):
        x = np.concatenate([tc[:, :, t].astype(np.float64), sd["pc_embedding.weight"][codes[:, t]]], -1)
        x = x + sd["pos_emb.alpha"][0] * pe[t][None]
        for w, (kc, vc) in zip(ws, kv):
            x = R.decode_layer(w, x, kc, vc, t)
        lg = x @ sd["predict_layer.weight"].T
        logits[:, t] = lg
        top2 = np.sort(lg, -1)[:, -2:]
        margin[:, t] = top2[:, 1] - top2[:, 0]
        for b in range(B):
            codes[b, t + 1] = int(prefixes[b][t]) if t < len(prefixes[b]) else int(np.argmax(lg[b]))
    return codes[:, 1:], logits, margin, kv


def prefill_attn(qkv, n, D, H):
    """include/hsp.h "PLM prefill" for one row: qkv [3 D, >= n] (rows q | k | v) -> out [D, n] with
    out[h Dh + d, i] = sum_{j <= i} softmax_{j <= i}(q_h[:, i] . k_h[:, j] / sqrt(Dh)) v_h[d, j].  Columns >= n are not
    read.  The caches the entry point fills are qkv[D : 2 D, :n] and qkv[2 D :, :n] themselves."""
    Dh = D // H
    q, k, v = (np.asarray(qkv[i * D:(i + 1) * D, :n], np.float64) for i in range(3))
    hidden = np.triu(np.ones((n, n), bool), 1)                       # True = key above the diagonal
    out = np.empty((D, n))
    for h in range(H):
        sl = slice(h * Dh, (h + 1) * Dh)
        s = q[sl].T @ k[sl] / np.sqrt(Dh)                            # [i, j]
        out[sl] = (R.softmax(np.where(hidden, -np.inf, s)) @ v[sl].T).T
    return out


# Foreign prefixes: (P, T, seed of the latent).  The prefix is np.random.default_rng(100 + P).integers(0, 1024, P), codes the
# model would not have chosen itself.  Searched on the CPU against the float64 decode for a top-2 margin of at least 1e-3 of
# the logits' range at every decoded step and for a visible dependence of step P on the first half of the prefix;
# test_plm_prefix_host.py re-checks both.
FOREIGN_CASES = [(1, 6, 9007), (4, 9, 9028), (17, 24, 9119), (64, 70, 9448), (65, 72, 9456), (130, 140, 9910),
                 (257, 262, 10799)]


def foreign_prefix(P):
    return np.random.default_rng(100 + P).integers(0, 1024, P).astype(np.int64)


_FOREIGN = {}


def foreign(case):
    """(tc [1, 256, T], prefix [P], codes [1, T], logits [1, T, vq_bins], margin [1, T], caches) of a foreign-prefix case,
    computed once per process and shared (treat as read-only)."""
    if case not in _FOREIGN:
        P, T, seed = case
        tc = R.case_tc((1, T), [seed])
        prefix = foreign_prefix(P)
        _FOREIGN[case] = (tc, prefix) + forced_decode_caches(R.synth_state(), tc, [prefix])
    return _FOREIGN[case]


# Own prefixes: rows of R.decoded(shape) continued from their own first P_i float64 codes.  A causal decode behind its own
# codes reproduces the row, whose margins test_plm_causal_host.py checks at every step.
OWN_CASES = {(5, 13): [5, 1, 12, 4, 8], (2, 260): [256, 64]}
