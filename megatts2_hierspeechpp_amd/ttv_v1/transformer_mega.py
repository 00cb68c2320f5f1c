"""Pre-LN transformer encoder of the Mega-TTS2 PLM (reference ttv_v1/transformer_mega.py).

The reference works time-major ``[B, T, D]``; here a batch is ONE channel-major matrix
``[1, D, B*T]`` with the utterances side by side on the column axis (``batch=(B, T)`` tells the
attention where they are), so that every ``nn.Linear`` is a single GEMM over all B*T tokens on the
MFMA conv kernel; the three q/k/v projections run as one stacked GEMM, attention is ``hsp_mha_f32``
on strided views.  Inference only: dropout is the identity
(transformer_mega.py:78 passes ``dropout_p = 0`` outside training).

Two further forms serve the causal mode (Megatts2PLM1.score / infer(causal=True)): ``TransformerEncoder.forward`` with
``x_lens`` / ``causal`` is the reference's masked full pass (hsp_mha_f32 with a dense mask, then the projection), and
``TransformerEncoderLayer.decode_step`` is one new position against a K/V cache (hsp_plm_decode_layer_f32; with a
position tensor, one position PER ROW: hsp_plm_decode_layer_pos_f32); ``prefill`` is ONE row's first n positions in a single
full pass that leaves K and V in those caches (hsp_plm_prefill_attn_f32), so that a decode can start behind given codes."""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn

from .. import _lib as L
from .. import functional as Fh
from ..hip_layers import HipLayer, LinearCT, StackedLinearCT


class LayerNorm(HipLayer):
    """torch.nn.LayerNorm(dim) (parameter names ``weight`` / ``bias``) over the channel axis of [B, D, T]."""

    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.dim, self.eps = dim, eps
        self.weight = nn.Parameter(torch.ones(dim), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(dim), requires_grad=False)
        self._g = self._b = None

    def hsp_requests(self):
        return [("g", self.dim), ("b", self.dim)]

    def hsp_fill(self, arena, materialize):
        self._g, self._b = arena.view(self, "g"), arena.view(self, "b")
        if materialize:
            self._g.copy_(self.weight.data)
            self._b.copy_(self.bias.data)

    def forward(self, x):
        if self._g is None:
            raise L.HspError("LayerNorm used before finalize()")
        return Fh.layernorm_mod(x, self.eps, gamma=self._g, beta=self._b)


class DecodeWeights(HipLayer):
    """The weights of one encoder layer as hsp_plm_decode_layer_f32 reads them: every nn.Linear weight transposed to
    [in][out] (q / k / v stacked), the biases, and the two LayerNorms un-folded.  Owns no parameters: the copies are
    gathered from the layer's own modules at finalize, into the weight arena."""

    def __init__(self, layer):
        super().__init__()
        self.__dict__["_layer"] = layer      # not registered as a sub-module (no cycle, no duplicate state_dict keys)
        self._views = None

    def _spec(self):
        D, F = self._layer.dim, self._layer.ff_dim
        return [("wqkv_t", D * 3 * D), ("bqkv", 3 * D), ("wo_t", D * D), ("bo", D), ("w1_t", D * F), ("c1", F),
                ("w2_t", F * D), ("c2", D)]

    def hsp_requests(self):
        return self._spec()

    def hsp_fill(self, arena, materialize):
        v = {name: arena.view(self, name) for name, _ in self._spec()}
        self._views = v
        if materialize:
            ly = self._layer
            at, D, F = ly.attn, ly.dim, ly.ff_dim
            parts = (at.w_q, at.w_k, at.w_v)
            v["wqkv_t"].view(D, 3 * D).copy_(torch.cat([p.weight.data for p in parts], 0).t())
            v["bqkv"].copy_(torch.cat([p.bias.data for p in parts], 0))
            v["wo_t"].view(D, D).copy_(at.out_proj[0].weight.data.t())
            v["bo"].copy_(at.out_proj[0].bias.data)
            v["w1_t"].view(D, F).copy_(ly.ff["0"].weight.data.t())
            v["c1"].copy_(ly.ff["0"].bias.data)
            v["w2_t"].view(F, D).copy_(ly.ff["3"].weight.data.t())
            v["c2"].copy_(ly.ff["3"].bias.data)


class MultiHeadAttention(nn.Module):
    """transformer_mega.MultiHeadAttention (:44-87), self-attention; without a mask on the path Megatts2PLM1.infer uses
    (``self.plm(x_pos)`` passes no lengths, t2w2v_transformer.py:715), with a dense one in the masked full pass."""

    def __init__(self, qkv_dim, n_heads=8, dropout=0., pre_norm=None):
        """``pre_norm``: the LayerNorm the encoder layer applies to this module's input; it is folded into
        the stacked q/k/v GEMM (hsp_conv1d_args.ln_c1) and ``forward`` then takes the un-normalised x."""
        super().__init__()
        assert qkv_dim % n_heads == 0
        self.n_heads, self.head_dim, self.qkv_dim = n_heads, qkv_dim // n_heads, qkv_dim
        self.w_q = LinearCT(qkv_dim, qkv_dim, packed=False)
        self.w_k = LinearCT(qkv_dim, qkv_dim, packed=False)
        self.w_v = LinearCT(qkv_dim, qkv_dim, packed=False)
        self.qkv = StackedLinearCT([self.w_q, self.w_k, self.w_v])
        if pre_norm is not None:
            self.qkv.fuse_input_layernorm(pre_norm)
        self.out_proj = nn.ModuleList([LinearCT(qkv_dim, qkv_dim)])  # nn.Sequential(Linear, Dropout): key "out_proj.0"
        self.out_proj[0].keep_rowmajor_weight()   # A operand of the projection inside hsp_mha_proj_f32

    def forward_cached(self, cache, n, out_cols):
        """Layer 0 of the greedy loop with its q / k / v of OLD positions kept (round 6, VERDICT r05 item 3's small win): the
        layer's input is the embedding matrix, whose columns do not change once their code is chosen
        (t2w2v_transformer.py:708-716: position j of step t is position j of every later step), and q / k / v are
        per-column functions of it, so step t computes the ONE new column per utterance -- a [3D x B] LayerNorm-GEMM
        instead of [3D x B n] -- into ``cache.qkv`` [3D, B, Tp] beside the ``cache.emb`` [D, B, Tp] it was computed from.
        Attention reads the first n columns of every utterance through strided views; the output (+ residual = the
        embeddings) goes to the side-by-side layout [1, D, Np] the rest of the step works in."""
        D, B, Tp = self.qkv_dim, cache.emb.shape[1], cache.emb.shape[2]
        t = n - 1
        xin = cache.emb[:, :, t:t + 1].permute(1, 0, 2)            # [B, D, 1]: utterances as the batch, ONE column each
        self.qkv(xin, out=cache.qkv[:, :, t:t + 1].permute(1, 0, 2))
        per = lambda m: m[:, :, :n].permute(1, 0, 2)               # [B, C, n] view of a [C, B, Tp] matrix
        q, k, v = (per(cache.qkv[i * D:(i + 1) * D]) for i in range(3))
        Np = (B * n + 3) & ~3
        y = torch.empty(1, D, Np, dtype=torch.float32, device=cache.emb.device) if Np == B * n else \
            torch.zeros(1, D, Np, dtype=torch.float32, device=cache.emb.device)
        lin = self.out_proj[0]
        Fh.mha_proj(q, k, v, self.n_heads, 1.0 / math.sqrt(self.head_dim), lin._wt, bias=lin._b, res=per(cache.emb),
                    out=out_cols(y))
        return y

    def forward(self, x, kv=None, mask=None, res=None, batch=None, last_only=False):
        """x [1, D, B*T] -> out_proj(attention) [+ res]; ``last_only`` -> [1, D, B]: only the last
        position of every utterance (columns T-1, 2T-1, ...), ``res`` then being [1, D, B] already."""
        if kv is not None:
            raise NotImplementedError("cross-attention is not on the PLM inference path")
        if mask is not None and (batch is None or last_only):
            raise NotImplementedError("a mask goes with the side-by-side layout (batch=(B, T)), all positions")
        D = self.qkv_dim
        B, T = batch if batch is not None else (x.shape[0], x.shape[2])
        qkv = self.qkv(x)
        if mask is None and batch is not None and Fh.mha_proj_supported(self.n_heads, self.head_dim, D, T):
            # ONE launch: attention over all heads of a 16-query tile + out_proj + bias + residual (round 4)
            per = lambda m: m[:, :B * T].reshape(-1, B, T).permute(1, 0, 2)       # [B, C, T] view of a [C, Np] matrix
            q, k, v = (per(qkv[0, i * D:(i + 1) * D]) for i in range(3))
            lin = self.out_proj[0]
            if last_only:
                # only the last position of every utterance: y [1, D, B], res [1, D, B] (a strided view of x)
                y = torch.empty(1, D, B, dtype=torch.float32, device=x.device)
                as_b = lambda m: m[0].permute(1, 0).unsqueeze(2)                     # [B, D, 1] view of [1, D, B]
                Fh.mha_proj(q[:, :, T - 1:], k, v, self.n_heads, 1.0 / math.sqrt(self.head_dim), lin._wt, bias=lin._b,
                            res=None if res is None else as_b(res), out=as_b(y))
                return y
            y = torch.empty_like(x) if x.shape[2] == B * T else torch.zeros_like(x)
            Fh.mha_proj(q, k, v, self.n_heads, 1.0 / math.sqrt(self.head_dim), lin._wt, bias=lin._b,
                        res=None if res is None else per(res[0]), out=per(y[0]))
            return y
        # padding columns (odd batch sizes only) must stay finite: they flow through the following GEMMs
        o = torch.empty_like(x) if batch is None or x.shape[2] == B * T else torch.zeros_like(x)
        # [B, C, T] view of a [C, Np] matrix (Np >= B*T: rows may be padded to a multiple of 4 columns)
        per_utt = lambda m: m[:, :B * T].reshape(-1, B, T).permute(1, 0, 2) if batch is not None else m
        q, k, v = (per_utt(qkv[0, i * D:(i + 1) * D]) if batch is not None else qkv[:, i * D:(i + 1) * D]
                   for i in range(3))
        # mask [B, T, T] (1 = attend): the fused kernel has no mask inside its softmax (hsp.h), so a masked pass is
        # hsp_mha_f32 with mask_dense and the projection as two launches
        Fh.mha(q, k, v, self.n_heads, 1.0 / math.sqrt(self.head_dim), out=per_utt(o[0]) if batch is not None else o,
               mask_dense=mask)
        if last_only:
            o = o[0][:, :B * T].reshape(D, B, T)[:, :, T - 1].unsqueeze(0)  # [1, D, B] view, time stride T
        return self.out_proj[0](o, res=res)


class TransformerEncoderLayer(nn.Module):
    """transformer_mega.TransformerEncoderLayer (:89-132), ``conv_ff=False``."""

    def __init__(self, dim, ff_dim, conv_ff=False, n_heads=8, dropout=0.):
        super().__init__()
        if conv_ff:
            raise NotImplementedError("Megatts2PLM1 builds its layers with conv_ff=False")
        self.dim, self.ff_dim, self.conv_ff, self.n_heads = dim, ff_dim, conv_ff, n_heads
        self.norm1 = LayerNorm(dim)
        self.norm2 = LayerNorm(dim)
        # both LayerNorms run inside the GEMM that consumes them (statistics from the staged input tile)
        self.attn = MultiHeadAttention(dim, n_heads=n_heads, dropout=dropout, pre_norm=self.norm1)
        # nn.Sequential(Linear, ReLU, Dropout, Linear): keys "ff.0" and "ff.3"
        self.ff = nn.ModuleDict({"0": LinearCT(dim, ff_dim), "3": LinearCT(ff_dim, dim)})
        self.ff["0"].fuse_input_layernorm(self.norm2)
        self.decode = DecodeWeights(self)

    def decode_supported(self) -> bool:
        return bool(L.lib().hsp_plm_decode_supported(self.dim, self.n_heads, self.ff_dim))

    def decode_workspace(self, B: int, device) -> torch.Tensor:
        """The scratch buffer decode_step needs for B rows (the layers and steps of one stream may share it)."""
        n = L.lib().hsp_plm_decode_workspace_bytes(B, self.dim)
        return torch.empty((n + 3) // 4, dtype=torch.float32, device=device)

    def decode_step(self, x, y, k_cache, v_cache, t: int, workspace, pos=None):
        """One new position t of every row against this layer's K/V cache (hsp_plm_decode_layer_f32): x, y [D, B] views
        (any strides; y may be x), k_cache / v_cache [D, B, Tp], ``workspace`` from decode_workspace.  Writes column t
        of both caches.  With ``pos`` (int32 [B] on the device, read when the kernels run) row b is at ``pos[b]`` and
        ``t`` is the largest position a row may hold; a row whose position is outside [0, t] is idle and untouched
        (hsp_plm_decode_layer_pos_f32)."""
        w = self.decode._views
        if w is None or self.norm1._g is None:
            raise L.HspError("TransformerEncoderLayer used before finalize()")
        D, B = x.shape
        assert y.shape == (D, B) and k_cache.shape == v_cache.shape and k_cache.is_contiguous() and v_cache.is_contiguous()
        assert k_cache.shape[:2] == (D, B) and 0 <= t < k_cache.shape[2]
        a = L.PlmDecodeArgs()
        a.x, a.x_bs, a.x_cs = L.fptr(x), x.stride(1), x.stride(0)
        a.y, a.y_bs, a.y_cs = L.fptr(y), y.stride(1), y.stride(0)
        a.k_cache, a.v_cache, a.bs, a.cs = L.fptr(k_cache), L.fptr(v_cache), k_cache.stride(1), k_cache.stride(0)
        a.t, a.B, a.D, a.H, a.F, a.eps = t, B, D, self.n_heads, self.ff_dim, self.norm1.eps
        a.g1, a.b1, a.g2, a.b2 = (L.fptr(v) for v in (self.norm1._g, self.norm1._b, self.norm2._g, self.norm2._b))
        for name in ("wqkv_t", "bqkv", "wo_t", "bo", "w1_t", "c1", "w2_t", "c2"):
            setattr(a, name, L.fptr(w[name]))
        a.workspace, a.workspace_bytes = L.fptr(workspace), workspace.numel() * 4
        if pos is None:
            L.call("hsp_plm_decode_layer_f32", ctypes.byref(a))
            return
        if pos.dtype != torch.int32 or pos.shape != (B,) or pos.stride(0) != 1:
            raise L.HspError("pos must be a contiguous int32 [B] tensor")
        L.call("hsp_plm_decode_layer_pos_f32", ctypes.byref(a), L.ptr(pos))

    def prefill_supported(self) -> bool:
        return bool(L.lib().hsp_plm_prefill_attn_supported(self.dim, self.n_heads))

    def prefill(self, x, n: int, k_row, v_row, last: bool = False):
        """The first ``n`` positions of ONE row in a single pass: x [1, D, Np] (Np >= n, padding columns zero) ->
        this layer's output [1, D, Np] under the causal mask, with K / V of positions 0 .. n - 1 written to ``k_row`` /
        ``v_row`` -- the row's [D, >= n] slices of the layer's decode caches (unit time stride, one channel stride), where
        ``decode_step`` reads them from position n on.  The fused-LayerNorm stacked q/k/v GEMM over the Np columns, then
        hsp_plm_prefill_attn_f32 (no dense mask), then out_proj (+ residual), ff.0 (ReLU), ff.3 (+ residual) as in
        ``forward``.  ``last``: stop after K / V and return None -- nothing reads the last layer's outputs at prefix
        positions."""
        if self.norm1._g is None:
            raise L.HspError("TransformerEncoderLayer used before finalize()")
        D = self.dim
        assert x.dim() == 3 and x.shape[0] == 1 and x.shape[1] == D and 1 <= n <= x.shape[2]
        assert k_row.shape[0] == D and v_row.shape[0] == D and k_row.stride(1) == 1 and v_row.stride(1) == 1
        assert k_row.stride(0) == v_row.stride(0) and k_row.shape[1] >= n and v_row.shape[1] >= n
        qkv = self.attn.qkv(x)                                                    # norm1 fused: [1, 3 D, Np]
        # padding columns (n not a multiple of 4) must stay finite: they flow through the following GEMMs
        o = None if last else (torch.empty_like(x) if x.shape[2] == n else torch.zeros_like(x))
        a = L.PlmPrefillAttnArgs()
        a.qkv, a.q_rs = L.fptr(qkv), qkv.stride(1)
        a.out, a.o_rs = (L.fptr(o), o.stride(1)) if o is not None else (None, 0)
        a.k_cache, a.v_cache, a.cs = L.fptr(k_row), L.fptr(v_row), k_row.stride(0)
        a.n, a.D, a.H, a.debug = n, D, self.n_heads, 0
        L.call("hsp_plm_prefill_attn_f32", ctypes.byref(a))
        if last:
            return None
        x = self.attn.out_proj[0](o, res=x)
        h = self.ff["0"](x, act=L.ACT_RELU)                                       # norm2 fused into ff.0
        return self.ff["3"](h, res=x)

    def forward(self, x, mask=None, batch=None, last_only=False, cache=None):
        """``last_only`` returns just the last position of every utterance ``[1, D, B]`` (all the
        greedy loop reads from the final layer); attention still sees the whole prefix.  ``cache`` (layer 0 of the greedy
        loop): x is None, the layer input lives in ``cache.emb`` (MultiHeadAttention.forward_cached)."""
        if cache is not None:
            B, T = batch
            x = self.attn.forward_cached(cache, T, lambda y: y[0][:, :B * T].reshape(-1, B, T).permute(1, 0, 2))
            h = self.ff["0"](x, act=L.ACT_RELU)
            return self.ff["3"](h, res=x)
        res = x
        if last_only:
            B, T = batch
            # the last position of every utterance, read in place at column stride T (hsp_conv1d_args.res_ts)
            res = x[0][:, :B * T].reshape(-1, B, T)[:, :, T - 1].unsqueeze(0)
        x = self.attn(x, mask=mask, res=res, batch=batch, last_only=last_only)   # norm1 fused into q/k/v
        h = self.ff["0"](x, act=L.ACT_RELU)                                       # norm2 fused into ff.0
        return self.ff["3"](h, res=x)


class TransformerEncoder(nn.Module):
    """transformer_mega.TransformerEncoder (:135-163)."""

    def __init__(self, encoder_layer: TransformerEncoderLayer, num_layers: int, norm=None):
        super().__init__()
        e = encoder_layer
        self.layers = nn.ModuleList([e] + [TransformerEncoderLayer(e.dim, e.ff_dim, e.conv_ff, e.n_heads)
                                           for _ in range(num_layers - 1)])
        self.num_layers, self.norm = num_layers, norm

    @staticmethod
    def attn_mask(x_lens, T: int, causal: bool, device) -> torch.Tensor:
        """make_attn_mask (ttv_v1/utils_mega.py:21-39) as the [B, T, T] 0/1 matrix hsp_mha_f32 takes (1 = attend): key j of
        row b is visible when j < x_lens[b], and, when ``causal``, j <= i.  The reference asserts that the longest row
        fills the matrix when causal (:31); so does this.  Index comparisons only, no arithmetic on activations."""
        lens = torch.as_tensor(x_lens).to(torch.int64).reshape(-1)
        if causal and int(lens.max()) != T:
            raise L.HspError("Causal mask requires all lengths to be equal to max_len")
        if int(lens.max()) > T or int(lens.min()) < 1:
            raise L.HspError(f"x_lens must lie in [1, {T}]")
        j = torch.arange(T, device=device)
        vis = (j[None, :] < lens.to(device)[:, None])[:, None, :].expand(-1, T, -1)
        if causal:
            vis = vis & (j[None, :] <= j[:, None])[None]
        return vis.to(torch.float32).contiguous()

    def decode_state(self, B: int, T: int, device):
        """The device state of a K/V-cached decode of B rows of up to T positions -> ``(kv, workspace)``: per layer a
        (k_cache, v_cache) pair of [D, B, Tp] buffers, Tp = T rounded up to 4 columns (16-byte rows), and the workspace
        the layers' decode_step calls share.  Refuses a geometry hsp_plm_decode_layer_f32 has no kernel for."""
        e = self.layers[0]
        if not all(layer.decode_supported() for layer in self.layers):
            raise L.HspError(f"hsp_plm_decode_layer_f32 has no kernel for d_model {e.dim}, {e.n_heads} heads, ff {e.ff_dim}")
        new = lambda: torch.empty(e.dim, B, (T + 3) & ~3, dtype=torch.float32, device=device)
        kv = [(new(), new()) for _ in self.layers]
        return kv, e.decode_workspace(B, device)

    @staticmethod
    def kv_rows(kv, b: int):
        """Row b's [D, Tp] slices of every layer's caches: what ``prefill`` fills for that row."""
        return [(kc[:, b], vc[:, b]) for kc, vc in kv]

    def prefill(self, x, n: int, kv_rows):
        """ONE row's first ``n`` positions through every layer (TransformerEncoderLayer.prefill): x [1, D, Np],
        ``kv_rows`` one (k_row, v_row) pair of [D, >= n] cache slices per layer.  The last layer stops after its K / V."""
        assert len(kv_rows) == self.num_layers
        for i, (layer, (k_row, v_row)) in enumerate(zip(self.layers, kv_rows)):
            x = layer.prefill(x, n, k_row, v_row, last=i == self.num_layers - 1)

    def forward(self, x, x_lens=None, causal=False, batch=None, last_only=False, cache=None):
        """Without ``x_lens`` (the reference builds no mask then, whatever ``causal`` says: :155-158) the unmasked pass
        of the greedy loop.  With ``x_lens`` (int [B]; ``batch=(B, T)`` locates the rows in x [1, D, >= B*T]): every layer
        under the reference's mask -- key padding, plus the triangle when ``causal``."""
        if x_lens is not None:
            if batch is None or last_only or cache is not None:
                raise NotImplementedError("the masked pass is the full side-by-side form: batch=(B, T), all positions")
            mask = self.attn_mask(x_lens, batch[1], causal, x.device)
            for layer in self.layers:
                x = layer(x, mask=mask, batch=batch)
            return x if self.norm is None else self.norm(x)
        for i, layer in enumerate(self.layers):
            x = layer(x, batch=batch, last_only=last_only and i == self.num_layers - 1,
                      cache=cache if i == 0 and self.num_layers > 1 else None)
        if self.norm is not None:
            x = self.norm(x)
        return x
