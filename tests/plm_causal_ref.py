"""Float64 restatement of the causal prosody LM, for the tests of Megatts2PLM1.score / infer(causal=True) and of
hsp_plm_decode_layer_f32.

Three things, all numpy float64 on a state dict of the reference's key names:
  * ``forward_logits``: the logits of the reference's ``Megatts2PLM1.forward`` (ttv_v1/t2w2v_transformer.py:685-692) --
    codes shifted right behind the go token, embedding + sinusoid, the pre-LN encoder under ``make_attn_mask(lens,
    heads, causal=True)`` (ttv_v1/utils_mega.py:21-39: strictly upper triangle OR key padding -> -inf), the predict layer;
  * ``greedy_decode``: the same model decoded step by step through a K/V cache, one ``decode_layer`` per layer and step;
  * ``decode_layer``: one layer for one new position, exactly as include/hsp.h states it for the kernel.
"""
import numpy as np
import torch

GO_ID, D_MODEL, N_HEADS, N_LAYERS, VQ_BINS, TC_DIM = 1024, 276, 4, 4, 1024, 256


def synth_state(seed=7):
    """The synthetic PLM weights of the existing PLM tests (synth_tensor("plm." + key)), as float64 arrays."""
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import Megatts2PLM1
    return {k: synth.synth_tensor("plm." + k, tuple(v.shape), seed).astype(np.float64)
            for k, v in Megatts2PLM1().state_dict().items()}


def pos_table(n, dim=D_MODEL):
    """SinePositionalEmbedding's table (:482-490), built in float32 with torch's CPU ops as the reference builds it (the
    table is data of the model, not arithmetic under test), then widened."""
    pe = torch.zeros(n, dim)
    position = torch.arange(0, n, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * -(np.log(10000.0) / dim))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.numpy().astype(np.float64)


def embed(sd, tc, codes_in):
    """tc [B, 256, T], codes_in [B, T] (go token first) -> x [B, T, D]."""
    T = tc.shape[2]
    x = np.concatenate([tc.transpose(0, 2, 1).astype(np.float64), sd["pc_embedding.weight"][codes_in]], -1)
    return x + sd["pos_emb.alpha"][0] * pos_table(T)[None]


def layernorm(x, g, b, eps=1e-5):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


def layer_weights(sd, i):
    p = f"plm.layers.{i}."
    g = lambda k: sd[p + k]
    return dict(g1=g("norm1.weight"), b1=g("norm1.bias"), g2=g("norm2.weight"), b2=g("norm2.bias"),
                wq=g("attn.w_q.weight"), bq=g("attn.w_q.bias"), wk=g("attn.w_k.weight"), bk=g("attn.w_k.bias"),
                wv=g("attn.w_v.weight"), bv=g("attn.w_v.bias"), wo=g("attn.out_proj.0.weight"), bo=g("attn.out_proj.0.bias"),
                w1=g("ff.0.weight"), c1=g("ff.0.bias"), w2=g("ff.3.weight"), c2=g("ff.3.bias"))


def softmax(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def layer_full(w, x, hidden, H=N_HEADS):
    """One encoder layer on x [B, T, D]; ``hidden`` bool [B, T, T]: True = masked (-inf), as make_attn_mask."""
    B, T, D = x.shape
    Dh = D // H
    h = layernorm(x, w["g1"], w["b1"])
    split = lambda a: a.reshape(B, T, H, Dh).transpose(0, 2, 1, 3)
    q, k, v = split(h @ w["wq"].T + w["bq"]), split(h @ w["wk"].T + w["bk"]), split(h @ w["wv"].T + w["bv"])
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(Dh)
    s = np.where(hidden[:, None], -np.inf, s)
    a = (softmax(s) @ v).transpose(0, 2, 1, 3).reshape(B, T, D)
    x = x + a @ w["wo"].T + w["bo"]
    return x + np.maximum(layernorm(x, w["g2"], w["b2"]) @ w["w1"].T + w["c1"], 0.0) @ w["w2"].T + w["c2"]


def attn_hidden(lens, T, causal=True):
    """make_attn_mask: key padding, OR-ed with the strictly upper triangle when causal.  True = hidden."""
    lens = np.asarray(lens)
    assert not causal or lens.max() == T, "Causal mask requires all lengths to be equal to max_len"
    hid = np.broadcast_to((np.arange(T)[None, :] >= lens[:, None])[:, None, :], (len(lens), T, T))
    if causal:
        hid = hid | np.triu(np.ones((T, T), bool), 1)[None]
    return hid


def forward_logits(sd, tc, p_codes, lens):
    """Logits [B, T, vq_bins] of the reference's forward(tc_latent, p_codes, lens)."""
    B, T = p_codes.shape
    codes_in = np.concatenate([np.full((B, 1), GO_ID, np.int64), p_codes[:, :-1]], 1)      # pad_y_go
    x = embed(sd, tc, codes_in)
    hid = attn_hidden(lens, T)
    for i in range(N_LAYERS):
        x = layer_full(layer_weights(sd, i), x, hid)
    return x @ sd["predict_layer.weight"].T


def decode_layer(w, x, kc, vc, t, H=N_HEADS, eps=1e-5):
    """include/hsp.h "causal PLM decoding": x [B, D], caches [B, D, Tp] (column t is written in place) -> y [B, D].
    Only columns 0 .. t of the caches are read."""
    B, D = x.shape
    Dh = D // H
    h = layernorm(x, w["g1"], w["b1"], eps)
    q = h @ w["wq"].T + w["bq"]
    kc[:, :, t] = h @ w["wk"].T + w["bk"]
    vc[:, :, t] = h @ w["wv"].T + w["bv"]
    a = np.empty((B, D))
    for hd in range(H):
        sl = slice(hd * Dh, (hd + 1) * Dh)
        s = np.einsum("bd,bdj->bj", q[:, sl], kc[:, sl, :t + 1]) / np.sqrt(Dh)
        a[:, sl] = np.einsum("bj,bdj->bd", softmax(s), vc[:, sl, :t + 1])
    x1 = x + a @ w["wo"].T + w["bo"]
    return x1 + np.maximum(layernorm(x1, w["g2"], w["b2"], eps) @ w["w1"].T + w["c1"], 0.0) @ w["w2"].T + w["c2"]


def greedy_decode(sd, tc, choose=None):
    """K/V-cached decode of tc [B, 256, T]: codes [B, T], logits [B, T, vq_bins] and the per-step top-2 margin [B, T].
    ``choose(logits_row, b, t, prev_codes)`` replaces the argmax (first maximal index, as torch) when given."""
    B, _, T = tc.shape
    ws = [layer_weights(sd, i) for i in range(N_LAYERS)]
    kv = [(np.full((B, D_MODEL, T), np.nan), np.full((B, D_MODEL, T), np.nan)) for _ in ws]
    pe = pos_table(T)
    codes = np.full((B, T + 1), GO_ID, np.int64)
    logits = np.empty((B, T, VQ_BINS))
    margin = np.empty((B, T))
    for t in range(T):
        x = np.concatenate([tc[:, :, t].astype(np.float64), sd["pc_embedding.weight"][codes[:, t]]], -1)
        x = x + sd["pos_emb.alpha"][0] * pe[t][None]
        for w, (kc, vc) in zip(ws, kv):
            x = decode_layer(w, x, kc, vc, t)
        lg = x @ sd["predict_layer.weight"].T
        logits[:, t] = lg
        top2 = np.sort(lg, -1)[:, -2:]
        margin[:, t] = top2[:, 1] - top2[:, 0]
        for b in range(B):
            codes[b, t + 1] = int(np.argmax(lg[b])) if choose is None else choose(lg[b], b, t, codes[b, 1:t + 1])
    return codes[:, 1:], logits, margin


# The decode cases of tests/test_gpu_plm_causal.py: (B, T) -> one seed of the tc_latent draw PER ROW (rows are independent,
# so each was searched on its own).  test_plm_causal_host.py checks on the CPU that with these seeds the float64 top-2
# margin is at least 1e-3 * max|logits| at EVERY step, so a float32 error of 1e-4 of the range on two logits (2e-4
# between them) cannot flip a choice.
DECODE_CASES = {
    (1, 5): [1000],
    (3, 9): [2001, 2002, 2004],
    (5, 13): [3001, 3007, 3009, 3010, 3011],
    (16, 70): [4004, 4006, 4009, 4024, 4030, 4031, 4041, 4046, 4054, 4055, 4060, 4062, 4065, 4070, 4081, 4121],
    (2, 260): [5790, 5872],
}
GRAPH_CASE = ((4, 18), [61, 62, 63, 64])


def case_tc(shape, seeds):
    B, T = shape
    assert len(seeds) == B
    return np.concatenate([np.random.default_rng(s).standard_normal((1, TC_DIM, T)).astype(np.float32) for s in seeds], 0)


_DECODED = {}


def decoded(shape):
    """(tc, codes, logits, margin) of a decode case, computed once per process and shared (treat as read-only)."""
    if shape not in _DECODED:
        tc = case_tc(shape, DECODE_CASES[shape])
        _DECODED[shape] = (tc,) + greedy_decode(synth_state(), tc)
    return _DECODED[shape]
