"""HIP mirror of reference ttv_v1/t2w2v_transformer.py (inference members only)."""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os
import types
from typing import Optional

import torch
from torch import nn

from .. import _lib as L
from .. import attentions
from .. import functional as Fh
from ..hip_layers import Conv1d, ConvTranspose1d, HipLayer, LinearCT, entry as _entry, finalize as _finalize
from ..styleencoder import StyleEncoder
from . import modules
from .Gaussian import GaussianUpsampling, RangePredictor
from .modules import WN
from .quantize import ResidualVectorQuantizer
from .transformer_mega import TransformerEncoder, TransformerEncoderLayer
from .vits_models import DurationPredictor


class SinePositionalEmbedding(HipLayer):
    """t2w2v_transformer.SinePositionalEmbedding (:466-514).  The 4000-row table the reference
    precomputes on the host in its constructor (:482) is computed the same way (torch CPU fp32 ops)
    and kept transposed ``[dim][4000]`` in the weight arena; adding it is fused into
    ``hsp_plm_embed_f32``."""

    N_POS = 4000

    def __init__(self, dim_model: int, dropout: float = 0.0, scale: bool = False, alpha: bool = False):
        super().__init__()
        if scale:
            raise NotImplementedError("the PLM builds SinePositionalEmbedding with scale=False")
        self.dim_model = dim_model
        self.alpha = nn.Parameter(torch.ones(1), requires_grad=False)
        self._pe_t = self._alpha = None

    def table(self) -> torch.Tensor:
        pe = torch.zeros(self.N_POS, self.dim_model)
        position = torch.arange(0, self.N_POS, dtype=torch.float32).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, self.dim_model, 2, dtype=torch.float32)
                             * -(math.log(10000.0) / self.dim_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        return pe

    def hsp_requests(self):
        return [("pe_t", self.dim_model * self.N_POS), ("alpha", 1)]

    def hsp_fill(self, arena, materialize):
        self._pe_t, self._alpha = arena.view(self, "pe_t"), arena.view(self, "alpha")
        if materialize:
            self._pe_t.copy_(self.table().t().contiguous().reshape(-1))
            self._alpha.copy_(self.alpha.data)


class Embedding(HipLayer):
    """torch.nn.Embedding table kept in the weight arena (parameter name ``weight``)."""

    def __init__(self, num_embeddings, embedding_dim):
        super().__init__()
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.weight = nn.Parameter(torch.zeros(num_embeddings, embedding_dim), requires_grad=False)
        self._w = None

    def hsp_requests(self):
        return [("w", self.num_embeddings * self.embedding_dim)]

    def hsp_fill(self, arena, materialize):
        self._w = arena.view(self, "w")
        if materialize:
            self._w.copy_(self.weight.data.reshape(-1))


# (round 6)  Layer 0 of the greedy loop keeps its q / k / v of old positions: its input is the embedding
# matrix, whose columns are final once their code is chosen, so every step embeds and projects ONE new column per utterance
# instead of the whole prefix (transformer_mega.MultiHeadAttention.forward_cached).  HSP_PLM_CACHE_L0=0: the full re-projection.
PLM_CACHE_L0 = os.environ.get("HSP_PLM_CACHE_L0", "1") == "1"


@dataclasses.dataclass(frozen=True)
class PlmSampling:
    """Sampled decoding of the prosody LM: the GPT-SoVITS sampler (ttv_v1/utils_gptsovits.py logits_to_probs +
    multinomial_sample_one_no_sync) -- repetition penalty, then top-p on the penalised logits, then temperature
    (clamped to >= 1e-5), then top-k -- drawn on the GPU with a counter-based stream (include/hsp.h "sampled PLM
    decoding").  ``top_k`` / ``top_p`` None = off; ``top_k=1`` is greedy whatever the temperature."""

    temperature: float = 1.0
    top_k: Optional[int] = None
    top_p: Optional[float] = None
    repetition_penalty: float = 1.0

    def __post_init__(self):
        if not (isinstance(self.temperature, (int, float)) and math.isfinite(self.temperature) and self.temperature >= 0):
            raise ValueError(f"temperature must be a finite number >= 0, got {self.temperature!r}")
        if self.top_k is not None and (isinstance(self.top_k, bool) or not isinstance(self.top_k, int) or self.top_k < 1):
            raise ValueError(f"top_k must be None or an int >= 1, got {self.top_k!r}")
        if self.top_p is not None and not (isinstance(self.top_p, (int, float)) and 0 < self.top_p <= 1):
            raise ValueError(f"top_p must be None or in (0, 1], got {self.top_p!r}")
        if not (isinstance(self.repetition_penalty, (int, float)) and math.isfinite(self.repetition_penalty)
                and self.repetition_penalty > 0):
            raise ValueError(f"repetition_penalty must be a finite number > 0, got {self.repetition_penalty!r}")

    def c_args(self, seeds: torch.Tensor, probs: Optional[torch.Tensor] = None) -> L.SampleArgs:
        """The hsp_sample_args of this setting; ``seeds`` int64 [B] on the GPU (read when the kernels run).  The struct
        holds raw pointers: the caller keeps ``seeds`` and ``probs`` alive until the launches are enqueued."""
        if seeds.dtype != torch.int64 or seeds.dim() != 1 or seeds.stride(0) != 1:
            raise L.HspError("seeds must be a contiguous int64 [B] tensor")
        return L.SampleArgs(float(self.temperature), int(self.top_k or 0),
                            2.0 if self.top_p is None else float(self.top_p), float(self.repetition_penalty),
                            L.ptr(seeds), L.fptr(probs), probs.stride(0) if probs is not None else 0)


plm_seeds = Fh.row_seeds   # the seed rule of the prosody LM is the one of every seed argument (functional.row_seeds)


def session_plan(lengths, slots: int):
    """The schedule of a decode session, from the request lengths alone: requests are taken in order, each goes to the
    lowest free slot at the earliest step that has one, and a slot is free on the step after its row's last (a row of
    length n admitted at step s runs steps s .. s + n - 1).  Returns ``(admissions, steps)``: ``admissions[step]`` the
    ``(request, slot)`` pairs admitted before that step runs, ``steps`` the number of steps until every row is done."""
    lengths = [int(n) for n in lengths]
    if int(slots) < 1:
        raise L.HspError(f"a session needs at least one slot, got {slots}")
    if any(n < 1 for n in lengths):
        raise L.HspError(f"every request needs at least one frame, got lengths {lengths}")
    free_at = [0] * int(slots)
    admissions, step = {}, 0
    for i, n in enumerate(lengths):
        step = max(step, min(free_at))
        slot = next(k for k, f in enumerate(free_at) if f <= step)
        free_at[slot] = step + n
        admissions.setdefault(step, []).append((i, slot))
    return admissions, (max(free_at) if lengths else 0)


def check_prefix(prefix, T: int, vq_bins: int, dims: int = 1) -> int:
    """The argument checks of a given code prefix (``infer(prefix_codes=)``, ``PlmDecodeSession.admit(prefix_codes=)``),
    as a pure function of the tensor: int64, ``dims``-dimensional ([P], or [B, P] with ``dims`` = 2), 1 <= P < T -- at
    least one position is left to decode -- and every code in [0, vq_bins) (the go and pad ids are not codes).  Returns P.
    Reading the values of a device tensor is one read-back: callers run this outside any capture."""
    if not isinstance(prefix, torch.Tensor) or prefix.dtype != torch.int64:
        raise L.HspError(f"prefix codes must be an int64 tensor, got {getattr(prefix, 'dtype', type(prefix).__name__)}")
    if prefix.dim() != dims:
        raise L.HspError(f"prefix codes must be {'[P]' if dims == 1 else '[B, P]'}, got shape {tuple(prefix.shape)}")
    P = int(prefix.shape[-1])
    if not 1 <= P < int(T):
        raise L.HspError(f"a prefix needs 1 <= P < T = {int(T)} codes (one position at least is decoded), got P = {P}")
    if prefix.numel():
        lo, hi = int(prefix.min()), int(prefix.max())
        if lo < 0 or hi >= int(vq_bins):
            raise L.HspError(f"prefix codes must lie in [0, {int(vq_bins)}), got {lo} .. {hi}")
    return P


class PlmDecodeSession:
    """Causal decoding of ragged request streams from ONE step (Megatts2PLM1.decode_session): ``slots`` rows of fixed-shape
    device state, each row at its own position ``pos[slot]`` in device memory (include/hsp.h "per-row positions"), so the
    same chain of launches -- embed, one position-form layer call per layer, the predict layer over all slots, choose and
    advance -- serves every length, rows of different lengths run side by side, and a slot whose row has finished
    (pos = -1: idle, its workgroups return at once) takes the next request while the others keep going.  ``capture``
    turns the step into one graph that ``step`` replays.  The host keeps no device state: which slots are busy follows
    from the lengths it admitted and the steps it enqueued, so nothing here synchronises or reads back."""

    def __init__(self, plm, slots: int, max_len: int, sampling=None):
        if sampling is not None and not isinstance(sampling, PlmSampling):
            raise L.HspError("sampling must be a PlmSampling or None")
        if int(slots) < 1 or int(slots) > 65535:
            raise L.HspError(f"a session needs 1 .. 65535 slots, got {slots}")
        if int(max_len) < 1 or int(max_len) > plm.pos_emb.N_POS:
            raise L.HspError(f"max_len must lie in [1, {plm.pos_emb.N_POS}] (the position table), got {max_len}")
        self.plm, self.slots, self.max_len, self.sampling = plm, int(slots), int(max_len), sampling
        S, D, dev = self.slots, plm.d_model, plm.pos_emb._pe_t.device
        self.kv, self.ws = plm.plm.decode_state(S, self.max_len, dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.tc = torch.zeros(S, plm.tc_latent_dim, self.max_len, **f32)
        self.codes = torch.full((S, self.max_len + 1), plm.GO_ID, dtype=torch.int64, device=dev)
        self.pos = torch.full((S,), -1, dtype=torch.int32, device=dev)
        self.len = torch.zeros(S, dtype=torch.int32, device=dev)
        self.seeds = torch.zeros(S, dtype=torch.int64, device=dev)
        self.x = torch.zeros(1, D, S, **f32)            # zero: the predict GEMM reads idle columns too; they stay finite
        self.logits = torch.zeros(1, plm.vq_bins, S, **f32)
        self._sample = sampling.c_args(self.seeds) if sampling is not None else None
        self._left = [0] * S                            # steps a slot's row still needs; 0 = free
        self._len = [0] * S                             # the length last admitted to a slot
        self._graph = None
        self.steps = self.replays = self.captures = 0

    def busy(self, slot: int) -> bool:
        return self._left[slot] > 0

    def admit(self, slot: int, tc_latent: torch.Tensor, seed: int = 0, prefix_codes=None):
        """Start a request in a free slot: ``tc_latent`` [256, T] with 1 <= T <= max_len.  Stream-ordered copies only (the
        latent, the go token, len = T, pos = 0, the seed).  The slot's cache needs no clearing: columns above a row's
        position are never read.

        ``prefix_codes`` (int64 [P], 1 <= P < T; `check_prefix`, which reads a device tensor's values back once): the
        row's first P codes are given.  They are written to ``codes[slot, 1 : P + 1]``, the slot's K / V caches are
        prefilled for positions 0 .. P - 1 in one pass (Megatts2PLM1.prefill: eager launches on the current stream --
        admit stays outside any capture, so they are legal between replays), and the row starts at pos = P: it takes
        T - P steps, and ``codes_of`` returns all T codes, the prefix in front."""
        if not 0 <= slot < self.slots:
            raise L.HspError(f"slot {slot} is not one of the session's {self.slots}")
        if tc_latent.dim() != 2 or tc_latent.shape[0] != self.plm.tc_latent_dim:
            raise L.HspError(f"tc_latent must be [{self.plm.tc_latent_dim}, T], got {tuple(tc_latent.shape)}")
        T = tc_latent.shape[1]
        if T < 1 or T > self.max_len:
            raise L.HspError(f"a request needs 1 .. max_len = {self.max_len} frames, got {T}")
        if self.busy(slot):
            raise L.HspError(f"slot {slot} is busy for {self._left[slot]} more steps")
        P = 0 if prefix_codes is None else check_prefix(prefix_codes, T, self.plm.vq_bins)
        self.tc[slot, :, :T].copy_(tc_latent, non_blocking=True)
        self.codes[slot, :1].fill_(self.plm.GO_ID)
        self.seeds[slot:slot + 1].fill_(int(seed))
        self.len[slot:slot + 1].fill_(T)
        if P:
            self.codes[slot, 1:P + 1].copy_(prefix_codes, non_blocking=True)
            self.plm.prefill(self.tc[slot], self.codes[slot, 1:P + 1], self.plm.plm.kv_rows(self.kv, slot))
        self.pos[slot:slot + 1].fill_(P)
        self._left[slot], self._len[slot] = T - P, T

    def enqueue_step(self):
        """The launches of one step on the current stream, without the host's bookkeeping: what ``capture`` captures and
        what an uncaptured ``step`` runs."""
        m, S = self.plm, self.slots
        top = self.max_len - 1                          # the largest position a row may hold
        x = self.x[0]                                   # [D, S]: element (c, b) at c * S + b
        L.call("hsp_plm_embed_pos_f32", L.fptr(self.tc), self.tc.stride(0), self.tc.stride(1), m.tc_latent_dim,
               L.ptr(self.codes), self.codes.stride(0), L.fptr(m.pc_embedding._w), m.vq_dim,
               m.pc_embedding.num_embeddings, L.fptr(m.pos_emb._pe_t), m.pos_emb.N_POS, L.fptr(m.pos_emb._alpha),
               L.fptr(x), x.stride(1), x.stride(0), S, L.ptr(self.pos), top)
        for layer, (kc, vc) in zip(m.plm.layers, self.kv):
            layer.decode_step(x, x, kc, vc, top, self.ws, pos=self.pos)
        m.predict_layer(self.x if m.plm.norm is None else m.plm.norm(self.x), out=self.logits)
        lg = self.logits
        L.call("hsp_plm_choose_advance_f32", L.fptr(lg), 1, lg.stride(1), S, m.vq_bins, L.ptr(self.codes),
               self.codes.stride(0), L.ptr(self.pos), L.ptr(self.len), top,
               ctypes.byref(self._sample) if self._sample is not None else None)

    def step(self):
        """One position of every busy slot: a replay of the captured graph, else the same launches eagerly.  No host
        synchronisation, no allocation."""
        if self._graph is not None:
            self._graph.replay()
            self.replays += 1
        else:
            self.enqueue_step()
        self.steps += 1
        self._left = [max(n - 1, 0) for n in self._left]

    def capture(self):
        """Capture the step as one graph (a single chain of launches); ``step`` replays it from then on.  Every slot must
        be idle: one eager step runs first -- it changes nothing, and it is where the kernels' code objects are loaded and
        the attention kernel's LDS limit is raised, which is not legal inside a capture."""
        if self._graph is not None:
            raise L.HspError("the session's step is captured already")
        if any(self._left):
            raise L.HspError("capture() needs every slot idle")
        self.enqueue_step()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.enqueue_step()
        self._graph = graph
        self.captures += 1

    def run(self, tc_latents, seeds=None, prefixes=None):
        """Decode a sequence of requests ([256, T_i] each) through the session's slots -> a list of int64 [T_i] tensors.
        ``prefixes``: None, or one entry per request, each None or the request's first P_i codes (int64 [P_i], see
        ``admit``): such a request takes T_i - P_i steps -- the schedule is ``session_plan([T_i - P_i], slots)`` -- and its
        result holds all T_i codes.
        The lengths are known here, so the whole schedule is computed up front (session_plan) and enqueued as admit /
        step / copy-out of a finished row before its slot is admitted again: exactly the plan's number of steps, no
        read-back, nothing that could wait on device state.  ``seeds``: an int s gives request i the seed s + i (None =
        0), or one int per request.  Every slot must be idle."""
        tc_latents = list(tc_latents)
        n = len(tc_latents)
        if isinstance(seeds, torch.Tensor):
            seeds = seeds.tolist()
        seeds = [int(seeds or 0) + i for i in range(n)] if seeds is None or isinstance(seeds, int) else [int(v) for v in seeds]
        if len(seeds) != n:
            raise L.HspError(f"{n} requests need {n} seeds, got {len(seeds)}")
        if any(self._left):
            raise L.HspError("run() needs every slot idle")
        lengths = [t.shape[-1] for t in tc_latents]
        prefixes = [None] * n if prefixes is None else list(prefixes)
        if len(prefixes) != n:
            raise L.HspError(f"{n} requests need {n} prefixes (None for a request without one), got {len(prefixes)}")
        given = [0 if p is None else check_prefix(p, T, self.plm.vq_bins) for p, T in zip(prefixes, lengths)]
        plan, steps = session_plan([T - P for T, P in zip(lengths, given)], self.slots)
        out = [torch.empty(T, dtype=torch.int64, device=self.codes.device) for T in lengths]
        running = {}
        for step in range(steps):
            for req, slot in plan.get(step, ()):
                self.admit(slot, tc_latents[req], seeds[req], prefixes[req])
                running[slot] = req
            self.step()
            for slot in [k for k in running if not self.busy(k)]:
                out[running.pop(slot)].copy_(self.codes_of(slot))
        return out

    def codes_of(self, slot: int) -> torch.Tensor:
        """The codes of the slot's current (or last) request: a view ``codes[slot, 1 : len + 1]``."""
        return self.codes[slot, 1:self._len[slot] + 1]


class Megatts2PLM1(nn.Module):
    """t2w2v_transformer.Megatts2PLM1 (:627-718): greedy prosody-code generation.

    ``infer`` follows the reference loop exactly -- at step t the whole prefix of t+1 positions is
    re-encoded bidirectionally (no KV cache is possible in that mode) and the last position's logits pick the next
    code -- but it takes a batch: the reference's go token is ``[1, 1]`` so it runs one utterance per
    call; utterances are independent, so B rows run the same loop side by side (rows shorter than
    the longest simply produce codes past their length that the caller drops).  The code buffer
    lives in device memory and every step is a fixed chain of launches, so the loop has no host
    synchronisation and can be captured in a hipGraph.

    ``infer(causal=True)`` (opt-in) decodes the way the model is TRAINED instead: the reference's ``forward`` runs the
    encoder under a causal mask (:691), under which position j's activations never change after step j, so a step is one
    new column per row through a K/V cache in all layers (hsp_plm_decode_layer_f32).  Its step-t logits are the
    teacher-forced logits ``score(tc_latent, codes, lens)[:, t]`` of its own codes; they are not the logits of the
    bidirectional loop, and the codes differ.  ``infer_many`` / ``decode_session`` decode requests of different lengths
    that way from one captured step, each row at its own position in device memory (PlmDecodeSession).  In the causal
    mode a row may start behind given codes (``prefix_codes`` / ``prefixes``): ``prefill`` leaves the K / V of the prefix in
    the caches in one full pass and the loop decodes the rest."""

    GO_ID = 1024

    def __init__(self, n_layers: int = 4, n_heads: int = 4, vq_dim: int = 20, tc_latent_dim: int = 256,
                 vq_bins: int = 1024, kernel_size: int = 9, dropout: float = 0.1):
        super().__init__()
        d_model = vq_dim + tc_latent_dim
        self.d_model, self.vq_dim, self.tc_latent_dim, self.vq_bins = d_model, vq_dim, tc_latent_dim, vq_bins
        self.plm = TransformerEncoder(
            TransformerEncoderLayer(dim=d_model, ff_dim=d_model * 4, n_heads=n_heads, dropout=dropout, conv_ff=False),
            num_layers=n_layers)
        self.predict_layer = LinearCT(d_model, vq_bins, bias=False)
        self.pos_emb = SinePositionalEmbedding(d_model)
        self.pc_embedding = Embedding(vq_bins + 2, vq_dim)

    def finalize(self, device, materialize: bool = True):
        self.arena = _finalize(self, device, materialize)
        return self

    def _ready(self):
        if self.pos_emb._pe_t is None:
            raise L.HspError("Megatts2PLM1 used before finalize()")

    def _launch_embed(self, tc, codes, pe_t, x, x_bs, x_cs, B, n, prev_logits, sample, j):
        """THE embedding launch of positions 0 .. n - 1 of the operand views: ``tc`` [B, 256, >= n], ``codes`` [B, >= n],
        ``pe_t`` the flat [D][N_POS] table from the views' first position on, ``x`` with strides (x_bs, x_cs, 1).  Without
        ``prev_logits`` hsp_plm_embed_f32; with them ([1, vq_bins, B], the scores of the step before) the launch first
        takes ``codes[:, n - 1]`` -- code column ``j`` of the row -- as their argmax (hsp_plm_embed_step_f32) or, with
        ``sample`` (a SampleArgs), as the sampled choice (hsp_plm_embed_sample_f32)."""
        head = (L.fptr(tc), tc.stride(0), tc.stride(1), self.tc_latent_dim, L.ptr(codes), codes.stride(0),
                L.fptr(self.pc_embedding._w), self.vq_dim, self.pc_embedding.num_embeddings, L.fptr(pe_t),
                self.pos_emb.N_POS, L.fptr(self.pos_emb._alpha), L.fptr(x), x_bs, x_cs, B, n)
        if prev_logits is None:
            L.call("hsp_plm_embed_f32", *head)
            return
        lg = prev_logits
        assert lg.shape == (1, self.vq_bins, B) and lg.stride(2) == 1
        head += (L.fptr(lg), 1, lg.stride(1), self.vq_bins)
        if sample is None:
            L.call("hsp_plm_embed_step_f32", *head)
        else:
            L.call("hsp_plm_embed_sample_f32", *head, j, ctypes.byref(sample))

    def _embed(self, tc, codes, n, prev_logits=None, sample=None):
        """[1, d_model, Np]: utterance b occupies columns b*n .. b*n+n-1; Np = B*n rounded up to a multiple
        of 4 (16-B rows for the token GEMM's DMA), padding columns are zero.  ``prev_logits`` [1, vq_bins, B]: the
        scores of step n-1, whose argmax (with ``sample``, a SampleArgs: whose sampled choice) this launch takes (and
        stores to ``codes[:, n-1]``) before it embeds."""
        B = tc.shape[0]
        x = torch.empty(1, self.d_model, (B * n + 3) & ~3, dtype=torch.float32, device=tc.device)
        self._launch_embed(tc, codes, self.pos_emb._pe_t, x, n, x.shape[2], B, n, prev_logits, sample, n - 1)
        return x

    def _embed_one(self, tc, codes, t, cache, prev_logits, sample=None):
        """Position t of every utterance into ``cache.emb[:, :, t]`` ([D, B, Tp]: fixed pitch) -- the same launch as _embed
        with every per-position operand shifted to column t and n = 1 (the kernel then takes codes[:, t] = argmax of
        ``prev_logits`` first, as in the full form)."""
        emb = cache.emb                                              # column t: element (c, b) at c * B Tp + b Tp
        pe_t = self.pos_emb._pe_t[t:]                                # flat [D][N_POS] table: row c, position t at c * N_POS + t
        self._launch_embed(tc[:, :, t:], codes[:, t:], pe_t, emb[:, :, t], emb.stride(1), emb.stride(0), tc.shape[0], 1,
                           prev_logits, sample, t)

    @_entry
    def step_logits(self, tc_latent, codes, n, out=None, prev_logits=None, cache=None, sampling=None, seeds=None):
        """Logits of position n-1 given the first n columns of ``tc_latent`` [B, 256, T] and of
        ``codes`` [B, >= n] (go token first): one pass of the loop body (:710-716) -> [1, vq_bins, B].
        With ``prev_logits`` (the result of the call for n-1) ``codes[:, n-1]`` is not read but first set to their
        argmax, inside the embedding launch -- or, with ``sampling`` (a PlmSampling; ``seeds`` as for `infer`), to a
        sampled choice (hsp_plm_embed_sample_f32)."""
        B = tc_latent.shape[0]
        sample = None
        if sampling is not None and prev_logits is not None:
            seeds = plm_seeds(seeds, B, tc_latent.device)   # held until the launches below are enqueued
            sample = sampling.c_args(seeds)
        # the last layer only produces the last position of every utterance when those B columns form a
        # 16-B addressable matrix for the fused-LayerNorm GEMM; otherwise it runs in full
        last_only = B % 4 == 0
        att = self.plm.layers[0].attn
        if cache is not None:
            # layer 0 incrementally (PLM_CACHE_L0): only position n - 1 is embedded and projected, the older columns are kept
            self._embed_one(tc_latent, codes, n - 1, cache, prev_logits, sample)
        if cache is not None and Fh.mha_proj_supported(att.n_heads, att.head_dim, self.d_model, n):
            x = self.plm(None, batch=(B, n), last_only=last_only, cache=cache)
        else:
            if cache is not None:
                # the first three steps (fewer than four keys: no fused attention kernel): the new column still enters the
                # cache, the step itself runs in the full form (its embedding launch takes the same argmax -- or the same
                # draw, which depends on (seed, column, token) only -- again: idempotent)
                att.qkv(cache.emb[:, :, n - 1:n].permute(1, 0, 2), out=cache.qkv[:, :, n - 1:n].permute(1, 0, 2))
            x = self.plm(self._embed(tc_latent, codes, n, prev_logits, sample), batch=(B, n), last_only=last_only)
        if not last_only:
            x = Fh.copy_strided(x[0][:, :B * n].reshape(self.d_model, B, n)[:, :, n - 1].unsqueeze(0))
        return self.predict_layer(x, out=out)

    @_entry
    @torch.no_grad()
    def score(self, tc_latent: torch.Tensor, p_codes: torch.Tensor, lens) -> torch.Tensor:
        """Teacher-forced logits [B, T, vq_bins] of the code sequences ``p_codes`` int64 [B, T] given ``tc_latent``
        [B, 256, T]: the ``logits`` of the reference's ``forward`` (:685-692) -- the codes shifted right behind the go
        token, the encoder under ``causal=True`` with ``lens`` (int [B], max == T as the reference asserts), the predict
        layer.  Positions t >= lens[b] of a row hold what the reference computes there (nothing reads them); the loss and
        the accuracy of ``forward`` are training and are not mirrored."""
        self._ready()
        B, D, T = tc_latent.shape
        assert D == self.tc_latent_dim and tc_latent.stride(2) == 1 and 1 <= T <= self.pos_emb.N_POS
        assert p_codes.shape == (B, T) and p_codes.dtype == torch.int64
        codes = torch.empty(B, T, dtype=torch.int64, device=tc_latent.device)       # pad_y_go: F.pad(y, (1, 0), go)[:, :-1]
        codes[:, 0] = self.GO_ID
        codes[:, 1:] = p_codes[:, :T - 1]
        x = self.plm(self._embed(tc_latent, codes, T), x_lens=lens, causal=True, batch=(B, T))
        lg = self.predict_layer(x)                                                   # [1, vq_bins, Np]
        return lg[0][:, :B * T].reshape(self.vq_bins, B, T).permute(1, 2, 0)

    @_entry
    @torch.no_grad()
    def prefill(self, tc_latent: torch.Tensor, prefix_codes: torch.Tensor, kv_rows):
        """K / V of positions 0 .. P - 1 of ONE row into its cache slices, in one full pass instead of P decode steps:
        ``tc_latent`` [256, >= P] (unit time stride), ``prefix_codes`` int64 [P] on the device (checked by the caller:
        `check_prefix`), ``kv_rows`` one (k_row, v_row) pair of [D, >= P] slices per layer (``kv[l][*][:, b]`` of a
        [D, B, Tp] cache).  The inputs of positions 0 .. P - 1 are the go token followed by ``prefix_codes[:P - 1]``: the
        full-form embedding, then TransformerEncoder.prefill -- per layer the fused-LayerNorm q/k/v GEMM over the P
        columns, hsp_plm_prefill_attn_f32, and (but for the last layer) out_proj and the feed-forward on the token GEMMs.

        Prefill is always issued per row (B = 1, over that row's own P columns): a GEMM's kernel choice depends on its
        column count, so a row prefilled beside others could differ from the row alone.  Issued per row, a request's
        result does not depend on its neighbours -- the property the decode path has -- and a session admits rows one at a
        time anyway.  The price: a batch of B prefixes costs B x about 20 small launches."""
        self._ready()
        P = int(prefix_codes.shape[0])
        if tc_latent.dim() != 2 or tc_latent.shape[0] != self.tc_latent_dim or tc_latent.stride(1) != 1:
            raise L.HspError(f"tc_latent must be [{self.tc_latent_dim}, >= P] with unit time stride, got "
                             f"{tuple(tc_latent.shape)}")
        if not 1 <= P <= min(tc_latent.shape[1], self.pos_emb.N_POS):
            raise L.HspError(f"a prefix of {P} codes needs 1 <= P <= {min(tc_latent.shape[1], self.pos_emb.N_POS)}")
        if not all(layer.prefill_supported() for layer in self.plm.layers):
            raise L.HspError(f"hsp_plm_prefill_attn_f32 has no kernel for d_model {self.d_model}, "
                             f"{self.plm.layers[0].n_heads} heads")
        codes_in = torch.empty(1, P, dtype=torch.int64, device=tc_latent.device)
        codes_in[:, :1].fill_(self.GO_ID)
        codes_in[0, 1:].copy_(prefix_codes[:P - 1])
        self.plm.prefill(self._embed(tc_latent.unsqueeze(0), codes_in, P), P, kv_rows)

    def _infer_causal(self, tc_latent, return_logits, sampling, seeds, prefix=None):
        """The K/V-cached loop: per step one embedded column per row (_embed_one, which also takes the previous step's
        choice), ``num_layers`` calls of hsp_plm_decode_layer_f32 and the predict layer -- no host synchronisation.
        ``prefix`` int64 [B, P] on the device: the first P codes of every row are given; the caches are prefilled row by
        row (``prefill``) and the loop runs t = P .. T - 1, its first step reading the given ``codes[:, P]``."""
        B, _, T = tc_latent.shape
        P = 0 if prefix is None else prefix.shape[1]
        dev, D = tc_latent.device, self.d_model
        kv, ws = self.plm.decode_state(B, T, dev)
        codes = torch.empty(B, T + 1, dtype=torch.int64, device=dev)
        codes[:, 0] = self.GO_ID
        all_logits = torch.empty(T - P, self.vq_bins, B, dtype=torch.float32, device=dev) if return_logits else None
        cache = types.SimpleNamespace(emb=torch.empty_like(kv[0][0]))                # [D, B, Tp], the caches' pitch
        x = torch.empty(1, D, B, dtype=torch.float32, device=dev)
        if P:
            codes[:, 1:P + 1] = prefix
            for b in range(B):
                self.prefill(tc_latent[b], codes[b, 1:P + 1], self.plm.kv_rows(kv, b))
        lg = None
        for t in range(P, T):
            sample = sampling.c_args(seeds) if sampling is not None and lg is not None else None
            self._embed_one(tc_latent, codes, t, cache, lg, sample)
            src = cache.emb[:, :, t]
            for layer, (kc, vc) in zip(self.plm.layers, kv):
                layer.decode_step(src, x[0], kc, vc, t, ws)
                src = x[0]
            # the encoder's final norm (None in the PLM) reads x and leaves it in place for the next step's layers
            lg = self.predict_layer(x if self.plm.norm is None else self.plm.norm(x),
                                    out=all_logits[t - P:t - P + 1] if return_logits else None)
        return codes, lg, all_logits

    @_entry
    @torch.no_grad()
    def infer(self, tc_latent: torch.Tensor, return_logits: bool = False, sampling: Optional[PlmSampling] = None,
              seeds=None, causal: bool = False, prefix_codes: Optional[torch.Tensor] = None):
        """tc_latent (B, D, T) -> int64 codes (B, T)  [+ fp32 logits (B, T, vq_bins)].

        ``causal`` False: the reference's bidirectional loop.  True: K/V-cached decoding under the causal mask the model
        is trained with (class docstring); ``sampling`` / ``seeds`` / ``return_logits`` mean the same in both modes.

        ``sampling`` None: greedy (the reference).  A PlmSampling: every code is drawn instead (include/hsp.h "sampled
        PLM decoding"); ``seeds`` an int (row b gets seed + b; None = 0) or an int64 [B] tensor (a device tensor is read
        in place when the kernels run, so a captured loop replays with new seeds after ``seeds.copy_()``).  Row b
        depends on its own seed only, not on the rest of the batch.

        ``prefix_codes`` (``causal=True`` only; int64 [B, P], 1 <= P < T, codes in [0, vq_bins): `check_prefix`): the
        first P codes of every row are given -- the kept beginning of an earlier take, a row to resume, the codes of
        preceding speech -- and only positions P .. T - 1 are decoded, behind K / V caches prefilled in one pass per row
        (``prefill``).  The codes come back [B, T] with the prefix in front; ``return_logits`` gives [B, T - P, vq_bins],
        entry i belonging to position P + i.  The repetition penalty sees the prefix codes and draws stay keyed by
        (seed, column), so a tail drawn behind a prefix equals the tail of a full run that happened to draw that prefix.
        None is exactly the loop without a prefix (a tensor of P = 0 columns is refused, like every P outside 1 .. T - 1)."""
        self._ready()
        if sampling is not None and not isinstance(sampling, PlmSampling):
            raise L.HspError("sampling must be a PlmSampling or None")
        B, D, T = tc_latent.shape
        if prefix_codes is not None and not causal:
            raise L.HspError("prefix_codes needs causal=True: the bidirectional loop re-encodes every position at every "
                             "step, so nothing of a prefix can be kept")
        if prefix_codes is not None:
            check_prefix(prefix_codes, T, self.vq_bins, dims=2)
            if prefix_codes.shape[0] != B:
                raise L.HspError(f"prefix_codes must have one row per utterance ({B}), got {prefix_codes.shape[0]}")
            prefix_codes = prefix_codes.to(tc_latent.device)
        seeds = plm_seeds(seeds, B, tc_latent.device) if sampling is not None else None
        assert D == self.tc_latent_dim and tc_latent.stride(2) == 1 and T <= self.pos_emb.N_POS
        if causal:
            codes, lg, all_logits = self._infer_causal(tc_latent, return_logits, sampling, seeds, prefix_codes)
            return self._last_choice(codes, lg, all_logits, sampling, seeds)
        codes = torch.empty(B, T + 1, dtype=torch.int64, device=tc_latent.device)
        codes[:, 0] = self.GO_ID
        all_logits = torch.empty(T, self.vq_bins, B, dtype=torch.float32, device=tc_latent.device) if return_logits \
            else None
        lg = None
        cache = None
        if PLM_CACHE_L0 and self.plm.num_layers > 1 and \
                Fh.mha_proj_supported(self.plm.layers[0].attn.n_heads, self.plm.layers[0].attn.head_dim, self.d_model, T):
            Tp = (T + 3) & ~3
            cache = types.SimpleNamespace(
                emb=torch.empty(self.d_model, B, Tp, dtype=torch.float32, device=tc_latent.device),
                qkv=torch.empty(3 * self.d_model, B, Tp, dtype=torch.float32, device=tc_latent.device))
        for t in range(T):
            # the greedy choice of step t-1 is taken inside step t's embedding launch; only the last step's needs its own
            lg = self.step_logits(tc_latent, codes, t + 1, out=all_logits[t:t + 1] if return_logits else None,
                                  prev_logits=lg, cache=cache, sampling=sampling, seeds=seeds)
        return self._last_choice(codes, lg, all_logits, sampling, seeds)

    @_entry
    def decode_session(self, slots: int, max_len: int, sampling: Optional[PlmSampling] = None) -> PlmDecodeSession:
        """Fixed-shape state for decoding up to ``slots`` requests of up to ``max_len`` frames side by side, each at its
        own position (PlmDecodeSession): admit(slot, tc_latent [256, T], seed), step(), capture(), codes_of(slot)."""
        self._ready()
        return PlmDecodeSession(self, slots, max_len, sampling)

    @_entry
    @torch.no_grad()
    def infer_many(self, tc_latents, slots: int = 16, sampling: Optional[PlmSampling] = None, seeds=None,
                   capture: bool = True, prefixes=None):
        """Causal decoding of many requests of different lengths: ``tc_latents`` a sequence of [256, T_i] tensors ->
        a list of int64 [T_i] code tensors, request i's equal to ``infer(tc_i[None], causal=True, ...)[0]`` (with seed
        ``seeds[i]``; an int s means s + i, as in ``infer``) whatever the other requests are: one session of ``slots``
        rows, sized for the longest request, and PlmDecodeSession.run -- exactly session_plan's number of steps, no
        read-back, no polling.  ``capture``: the step is one captured graph, replayed (else launched eagerly).
        ``prefixes``: None, or per request None or its first P_i codes (int64 [P_i], 1 <= P_i < T_i): request i then equals
        ``infer(tc_i[None], causal=True, prefix_codes=prefixes[i][None], ...)[0]``, takes T_i - P_i steps, and comes back
        whole (PlmDecodeSession.run)."""
        tc_latents = list(tc_latents)
        if not tc_latents:
            session_plan([], slots)
            return []
        if any(t.dim() != 2 for t in tc_latents):
            raise L.HspError("every request is a [256, T] tensor")
        session_plan([t.shape[1] for t in tc_latents], slots)          # refuse before any state is allocated
        ses = self.decode_session(slots, max(t.shape[1] for t in tc_latents), sampling)
        if capture:
            ses.capture()
        return ses.run(tc_latents, seeds, prefixes)

    def _last_choice(self, codes, lg, all_logits, sampling, seeds):
        """The choice of the last step (every earlier one is taken inside the next step's embedding launch)."""
        B, T = codes.shape[0], codes.shape[1] - 1
        if sampling is None:
            L.call("hsp_argmax_f32", L.fptr(lg), 1, B, B, self.vq_bins, L.ptr(codes[:, T:]), codes.stride(0))
        else:
            L.call("hsp_sample_f32", L.fptr(lg), 1, B, B, self.vq_bins, L.ptr(codes[:, T:]), codes.stride(0), T,
                   ctypes.byref(sampling.c_args(seeds)))
        return (codes[:, 1:], all_logits.permute(2, 0, 1)) if all_logits is not None else codes[:, 1:]


# ======================================================================= front-end
class TextEncoder(nn.Module):
    """t2w2v_transformer.TextEncoder (:82-143).  ``cond`` / ``proj`` of the reference are dead code on
    every path (their uses are commented out) and are not mirrored."""

    def __init__(self, n_vocab, n_tone, n_language, out_channels, hidden_channels, filter_channels, n_heads, n_layers,
                 kernel_size, p_dropout):
        super().__init__()
        self.n_vocab, self.n_tone, self.n_language, self.hidden_channels = n_vocab, n_tone, n_language, hidden_channels
        self.emb = Embedding(n_vocab, hidden_channels)
        self.emb_tone = Embedding(n_tone, hidden_channels)
        self.emb_language = Embedding(n_language, hidden_channels)
        self.encoder = attentions.Encoder(hidden_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout)
        self.encoder2 = attentions.Encoder(hidden_channels, filter_channels, n_heads, 1, kernel_size, p_dropout)

    def forward(self, x, x_lengths, g, tone, language, out=None):
        h = Fh.embedding_sum([x, tone, language], [self.emb._w, self.emb_tone._w, self.emb_language._w],
                             [self.n_vocab, self.n_tone, self.n_language], math.sqrt(self.hidden_channels),
                             self.hidden_channels)
        x_mask = Fh.sequence_mask(x_lengths, h.shape[2])
        h = self.encoder(h, x_mask)
        h = self.encoder2(h, x_mask)
        return h, x_mask


class MelEncoder(nn.Module):
    """t2w2v_transformer.MelEncoder (:145-179)."""

    def __init__(self, out_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout):
        super().__init__()
        self.encoder = attentions.Encoder(hidden_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout)
        self.proj = Conv1d(hidden_channels, out_channels, 1)

    def forward(self, x, x_lengths):
        x_mask = Fh.sequence_mask(x_lengths, x.shape[2])
        return self.proj(self.encoder(x, x_mask), mask=x_mask, mask_mode=L.MASK_POST), x_mask


class W2VEncoder(nn.Module):
    """t2w2v_transformer.W2VEncoder (:182-226); ``project`` / ``proj`` are dead code there."""

    def __init__(self, out_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout):
        super().__init__()
        self.cond = Conv1d(256, hidden_channels, 1)
        self.encoder = attentions.Encoder(hidden_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout)
        self.encoder2 = attentions.Encoder(hidden_channels, filter_channels, n_heads, 1, kernel_size, p_dropout)

    def forward(self, x, x_lengths, g, x_mask=None, cond_added=False):
        """``cond_added``: the caller already fused ``+ cond(g)`` into the conv that produced x."""
        if x_mask is None:
            x_mask = Fh.sequence_mask(x_lengths, x.shape[2])
        if not cond_added:
            x = Fh.add_cbias(x, self.cond(g, force_direct=True))
        return self.encoder2(self.encoder(x, x_mask), x_mask), x_mask


class W2VDecoder(nn.Module):
    """t2w2v_transformer.W2VDecoder (:377-405)."""

    def __init__(self, in_channels, hidden_channels, kernel_size, dilation_rate, n_layers, output_size=1024,
                 gin_channels=0, p_dropout=0):
        super().__init__()
        self.pre = Conv1d(in_channels, hidden_channels, 1)
        self.enc = WN(hidden_channels, kernel_size, dilation_rate, n_layers, gin_channels=gin_channels, p_dropout=p_dropout)
        self.proj = Conv1d(hidden_channels, output_size, 1)

    def forward(self, x, x_mask, g=None):
        # pre(x * mask) * mask: x arrives masked from the encoder
        x = self.pre(x, mask=x_mask, mask_mode=L.MASK_POST)
        x = self.enc(x, x_mask, g=g)
        return self.proj(x, mask=x_mask, mask_mode=L.MASK_POST)


class PitchPredictor(nn.Module):
    """t2w2v_transformer.PitchPredictor (:408-463): HiFi-GAN style x4 upsampler, w2v -> log-f0."""

    def __init__(self):
        super().__init__()
        ks, ups, ch0 = [3, 5, 7], [(2, 4), (2, 4)], 256
        self.num_kernels, self.num_upsamples = len(ks), len(ups)
        self.conv_pre = Conv1d(1024, ch0, 7, padding=3)
        self.ups = nn.ModuleList([ConvTranspose1d(ch0 // 2 ** i, ch0 // 2 ** (i + 1), k, u, padding=(k - u) // 2,
                                                  weight_norm=True) for i, (u, k) in enumerate(ups)])
        self.resblocks = nn.ModuleList([modules.ResBlock1(ch0 // 2 ** (i + 1), k, (1, 3, 5))
                                        for i in range(len(ups)) for k in ks])
        self.conv_post = Conv1d(ch0 // 2 ** len(ups), 1, 7, padding=3, bias=False)
        self.cond = Conv1d(256, ch0, 1)

    def forward(self, x, g, lengths=None):
        """``lengths`` (int64 [B], 50 Hz frames): zero every intermediate past an utterance's end, so a
        short row of a batch sees the same zero padding as when it runs alone (the reference has no mask
        here and runs B = 1)."""
        B, _, T = x.shape
        mk = (lambda r: Fh.sequence_mask(lengths * r, T * r)) if lengths is not None else (lambda r: None)
        mm = lambda m: dict(mask=m, mask_mode=L.MASK_POST) if m is not None else {}
        x = self.conv_pre(x, cbias=self.cond(g, force_direct=True), **mm(mk(1)))
        for i in range(self.num_upsamples):
            m = mk(2 ** (i + 1))
            x = self.ups[i](x, lrelu=modules.LRELU_SLOPE)
            if m is not None:
                x = Fh.mask_mul(x, m)
            xs = torch.empty_like(x)
            for j in range(self.num_kernels):
                self.resblocks[i * self.num_kernels + j](x, x_mask=m, out=xs, accumulate=j > 0,
                                                         post_scale=1.0 / self.num_kernels if j == self.num_kernels - 1 else 1.0)
            x = xs
        return self.conv_post(x, lrelu=0.01)   # F.leaky_relu default slope (:458)


class PLMConv(nn.Module):
    """t2w2v_transformer.PLMConv (:517-528): x -> conv2(conv1(x * m) * m) * m on the 20-channel prosody track."""

    def __init__(self, hidden_channels=80):
        super().__init__()
        self.conv1 = Conv1d(hidden_channels, hidden_channels, 5, padding=2)
        self.conv2 = Conv1d(hidden_channels, hidden_channels, 5, padding=2)

    def forward(self, x, mask, premasked=False):
        if not premasked:
            x = Fh.mask_mul(x, mask)
        h = self.conv1(x, mask=mask, mask_mode=L.MASK_POST, force_direct=True)
        return self.conv2(h, mask=mask, mask_mode=L.MASK_POST, force_direct=True)


class SynthesizerTrn(nn.Module):
    """t2w2v_transformer.SynthesizerTrn (:721-1077), inference members only
    (``inf_extract_tc_latent``, ``inf_plm_gen`` and the older non-PLM ``infer``).  Same constructor signature;
    the ``lr`` sub-module, which only the training ``forward`` touches, is not built, so reference
    checkpoints load with ``strict=False``.

    The reference front-end is B = 1 only (RangePredictor's ``.squeeze()`` and the [B,1,N] x [B,N]
    broadcast at :961 break for B > 1).  Here a batch is B independent utterances: every stage honours
    the per-utterance lengths so that row b equals the reference run on utterance b alone, and frames
    past an utterance's length are zero."""

    def __init__(self, n_vocab, n_tone, n_language, spec_channels, hop_length, sampling_rate, segment_size,
                 inter_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout, resblock,
                 resblock_kernel_sizes, resblock_dilation_sizes, gin_channels=256, prosody_size=20, cfg=False,
                 freeze_quantizer=None, **kwargs):
        super().__init__()
        self.inter_channels, self.hidden_channels, self.stride = inter_channels, hidden_channels, 8
        ic = inter_channels
        self.enc_p = TextEncoder(n_vocab, n_tone, n_language, out_channels=ic, hidden_channels=ic, filter_channels=ic * 4,
                                 n_heads=4, n_layers=3, kernel_size=9, p_dropout=0.2)
        self.mel_encoder = MelEncoder(out_channels=256, hidden_channels=80, filter_channels=80 * 4, n_heads=4, n_layers=2,
                                      kernel_size=9, p_dropout=0.2)
        self.mha = attentions.MultiHeadAttention(ic, ic, n_heads=4, p_dropout=0.2)
        self.cond_g = Conv1d(256, ic, 1)
        self.w2v_encoder = W2VEncoder(out_channels=ic, hidden_channels=ic, filter_channels=ic * 4, n_heads=4, n_layers=3,
                                      kernel_size=9, p_dropout=0.2)
        self.w2v_decoder = W2VDecoder(ic, ic * 2, 5, 1, 8, output_size=1024, p_dropout=0.1, gin_channels=256)
        self.emb_g = StyleEncoder(in_dim=80, hidden_dim=256, out_dim=256)
        self.duration_predictor = DurationPredictor(hidden_channels, 256, 3, 0.5, gin_channels=gin_channels)
        self.RangePredictor = RangePredictor(257, 256)
        self.gaussian = GaussianUpsampling()
        self.dur_downsample = Conv1d(hidden_channels, hidden_channels, 1)   # stride 2: run on an x[..., ::2] view
        self.pp = PitchPredictor()
        self.quantizer = ResidualVectorQuantizer(dimension=20, n_q=1, bins=1024)
        self.ssl_proj = Conv1d(20, ic, 1)
        # legacy (non-PLM) prosody path of infer(): the prompt mel's first 20 bins -> PLMConv -> max-pool 8 -> PLMConv
        # -> nearest code (:794-797); nn.MaxPool1d has no parameters
        self.plm_conv1 = PLMConv(hidden_channels=20)
        self.plm_conv2 = PLMConv(hidden_channels=20)

    # keys of the reference checkpoint that no inference path reads
    UNUSED = ("lr.", "enc_p.cond.", "enc_p.proj.", "w2v_encoder.project.", "w2v_encoder.proj.")
    UNUSED_LEAVES = ("_codebook.inited", "_codebook.cluster_size", "_codebook.embed_avg")

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Accepts the reference's checkpoints: a bare state dict or utils.load_checkpoint's {'model': ...}
        (inference_plm.py:233); training-only / dead keys are skipped."""
        if "model" in state_dict and not any(k.startswith("enc_p.") for k in state_dict):
            state_dict = state_dict["model"]
        sd = {k: v for k, v in state_dict.items() if not k.startswith(self.UNUSED) and not k.endswith(self.UNUSED_LEAVES)}
        return super().load_state_dict(sd, strict=strict, **kw)

    def finalize(self, device, materialize: bool = True):
        self.arena = _finalize(self, device, materialize)
        return self

    def _tc_latent(self, x, x_lengths, ref_mel, ref_len, tone, language, length_scale, dur, scale=None):
        """The text -> frame-rate front part shared by ``inf_extract_tc_latent`` and ``extract_tc_latent_code``: style and
        MRTE from ``ref_mel``, predicted or given durations, range clamp, Gaussian upsampling, ``dur_downsample``.
        ``scale`` (fp32 [B, N] on the device, or None): a factor per phone on its duration before the ceil
        (hsp_duration_scaled_f32); None: hsp_duration_f32, the launch there has always been.
        -> x_frame [B, 256, T2], g [B, 256, 1], frame_lengths (float, host) [B], mask2 float [B, 1, T2]."""
        B, N = x.shape
        C = self.inter_channels
        x_lengths = x_lengths.to(torch.int64)
        g = self.emb_g(ref_mel, Fh.sequence_mask(ref_len, ref_mel.shape[2]), per_utterance=True).unsqueeze(-1)
        h, x_mask = self.enc_p(x, x_lengths, g, tone, language)
        mel_out, h_mask = self.mel_encoder(ref_mel, ref_len)
        # x = x + mha(x, mel) + cond_g(g), written into the first 256 channels of the RangePredictor input
        xd = torch.empty(B, C + 1, N, dtype=torch.float32, device=x.device)
        xs = xd[:, :C]
        self.mha(h, mel_out, mask_q=x_mask, mask_k=h_mask, res=h, cbias=self.cond_g(g, force_direct=True), out=xs)
        frames = torch.empty(B, dtype=torch.float32, device=x.device)
        dcol = xd[:, C]
        if dur is None:
            logw = self.duration_predictor(xs, x_mask, g=g, lengths=x_lengths)
            lw = (L.fptr(logw), logw.stride(0))
        else:
            dcol.copy_(dur.to(torch.float32))
            lw = (None, 0)
        if scale is None:
            L.call("hsp_duration_f32", lw[0], lw[1], L.ptr(x_lengths), float(length_scale), L.fptr(dcol), dcol.stride(0),
                   L.fptr(frames), B, N)
        else:
            if scale.shape != (B, N) or scale.dtype != torch.float32 or not scale.is_contiguous():
                raise L.HspError(f"the phone scales must be a contiguous fp32 [{B}, {N}] tensor, got "
                                 f"{scale.dtype} {tuple(scale.shape)}")
            L.call("hsp_duration_scaled_f32", lw[0], lw[1], L.ptr(x_lengths), float(length_scale), L.fptr(dcol),
                   dcol.stride(0), L.fptr(frames), B, N, L.fptr(scale), N)
        rng = self.RangePredictor(xd, x_lengths)
        frames_h = frames.cpu()                       # the reference's `.item()` (Gaussian.py:53): T is data dependent
        T = int(frames_h.max().item())
        x_frame = self.gaussian(xs, dcol, rng, x_lengths, frames, T)
        frame_lengths = frames_h / 2                   # (:976) float, may end in .5
        T2 = (T - 1) // 2 + 1
        len2 = torch.ceil(frame_lengths).to(torch.int64).to(x.device)
        mask2 = Fh.sequence_mask(len2, T2)
        x_frame = self.dur_downsample(x_frame[:, :, ::2], mask=mask2, mask_mode=L.MASK_POST)
        return x_frame, g, frame_lengths, mask2

    @_entry
    @torch.no_grad()
    def inf_extract_tc_latent(self, x, x_lengths, y_mel, y_length, tone, language, mrte_mel=None, mrte_mel_lengths=None,
                              length_scale=1, dur=None, host_lengths=False, phone_scale=None):
        """(:937-982) ids/tone/language int64 [B, N], x_lengths [B], y_mel [B, 80, Tm], y_length [B] ->
        x_frame [B, 256, T2], g [B, 256, 1], x_lengths (float, frames / 2) [B], x_mask BOOL [B, 1, T2] (the
        reference's dtypes, :979-982; ``inf_plm_gen`` takes that mask or a float one).
        ``dur`` [B, N] (optional) overrides the predicted durations (BASELINE config 3 pins them).
        ``host_lengths``: a fifth result, the same x_lengths as the CPU tensor the front-end read back (callers that
        slice rows by their frame counts need no second read-back).
        ``phone_scale`` (fp32 [B, N] on the device, or None): a factor per phone on its duration, predicted or given,
        before the ceil (include/hsp.h: hsp_duration_scaled_f32); entries past a row's length are not read."""
        ref_mel, ref_len = (mrte_mel, mrte_mel_lengths) if mrte_mel is not None else (y_mel, y_length)
        x_frame, g, frame_lengths, mask2 = self._tc_latent(x, x_lengths, ref_mel, ref_len, tone, language, length_scale, dur,
                                                           phone_scale)
        out = (x_frame, g, frame_lengths.to(x.device), mask2.to(torch.bool))   # a dtype cast, as the reference's (:982)
        return (*out, frame_lengths) if host_lengths else out

    @_entry
    @torch.no_grad()
    def inf_plm_gen(self, x_frame, g, codes, x_lengths, x_mask):
        """(:984-994) codes int64 [B, T2] (or the reference's [1, 1, T2]) -> w2v [B, 1024, T2], lf0 [B, 4 T2].
        ``x_mask`` (bool as returned by inf_extract_tc_latent, or float) is accepted for the reference's signature; the
        masks used here are rebuilt from ``x_lengths`` by the mask kernel (same values: :975-982)."""
        T2 = x_frame.shape[2]
        q = self.quantizer.decode(codes)
        # x_frame + ssl_proj(quantized) [+ w2v_encoder.cond(g), fused]
        x = self.ssl_proj(q, res=x_frame, cbias=self.w2v_encoder.cond(g, force_direct=True))
        len2 = torch.ceil(x_lengths.to(torch.float32)).to(torch.int64)
        mask = Fh.sequence_mask(len2, T2)
        x2v_enc, _ = self.w2v_encoder(x, x_lengths, g, x_mask=mask, cond_added=True)
        w2v_pred = self.w2v_decoder(x2v_enc, mask, g=g)
        lf0 = self.pp(w2v_pred, g, lengths=len2)
        mask4 = Fh.sequence_mask(4 * len2, 4 * T2)
        return w2v_pred, Fh.mask_mul(lf0, mask4).squeeze(1)

    @_entry
    @torch.no_grad()
    def prosody_codes(self, mel, mel_lengths, pooled=False):
        """Prosody codes of recorded speech (:912-929): mel [B, 80, T] fp32 (any T >= 1), mel_lengths [B] -> int64 [B, T],
        every code held for 8 frames and zeros from a row's length on (the reference's ``lr_codes``), or with ``pooled``
        int64 [B, ceil(T / 8)], one code per pooled frame.  One launch (hsp_prosody_encode_f32: first 20 bins ->
        PLMConv -> max-pool 8 -> PLMConv -> nearest code), nothing read back; rows are independent utterances and a row
        equals that row run alone.  A mel whose length is no multiple of 8 counts as zero-padded to the next one."""
        D, cb = self.quantizer.dimension, self.quantizer.vq.layers[0]._codebook
        if mel.dim() != 3 or mel.shape[1] < D or mel.shape[2] < 1:
            raise L.HspError(f"prosody_codes(): mel must be [B, >= {D}, T >= 1], got {tuple(mel.shape)}")
        B, _, T = mel.shape
        if mel_lengths.shape != (B,):
            raise L.HspError(f"prosody_codes(): mel_lengths must be [{B}], got {tuple(mel_lengths.shape)}")
        if mel.stride(2) != 1:
            mel = mel.contiguous()
        lens = mel_lengths.to(device=mel.device, dtype=torch.int64).contiguous()
        out = torch.empty(B, -(-T // self.stride) if pooled else T, dtype=torch.int64, device=mel.device)
        convs = (self.plm_conv1.conv1, self.plm_conv1.conv2, self.plm_conv2.conv1, self.plm_conv2.conv2)
        a = L.ProsodyArgs()
        a.x, a.x_bs, a.x_cs, a.lengths = L.fptr(mel), mel.stride(0), mel.stride(1), L.ptr(lens)
        a.B, a.D, a.T, a.k, a.w_ld, a.bins = B, D, T, convs[0].k, convs[0].M, self.quantizer.bins
        for name, c in zip(("1a", "1b", "2a", "2b"), convs):
            setattr(a, "w" + name, L.fptr(c._w))
            setattr(a, "b" + name, L.fptr(c._b))
        a.embed = L.fptr(cb._w)
        if pooled:
            a.pooled, a.p_bs = L.ptr(out), out.stride(0)
        else:
            a.codes, a.c_bs = L.ptr(out), out.stride(0)
        L.call("hsp_prosody_encode_f32", ctypes.byref(a))
        return out

    @_entry
    @torch.no_grad()
    def extract_tc_latent_code(self, x, x_lengths, mel_spk, mel_spk_lengths, tone, language, dur, mrte_mel, mrte_mel_lengths):
        """(:887-930) how the prosody LM's training pairs are made: -> (x_frame [B, 256, T2], lr_codes int64 [B, Tm]).
        ``x_frame`` is the text-derived track at the GIVEN durations ``dur`` [B, N], style and MRTE from ``mrte_mel`` (what
        ``inf_extract_tc_latent(..., dur=dur, mrte_mel=mrte_mel)`` returns); ``lr_codes`` are the prosody codes of
        ``mel_spk`` (``prosody_codes``).  Aligning a recording to its text is the caller's: ``dur`` is an input, as in the
        reference.  For B > 1 rows are independent utterances."""
        x_frame = self._tc_latent(x, x_lengths, mrte_mel, mrte_mel_lengths, tone, language, 1, dur)[0]
        return x_frame, self.prosody_codes(mel_spk, mel_spk_lengths)

    @_entry
    @torch.no_grad()
    def infer(self, x, x_lengths, mel_spk, mel_spk_lengths, tone, language, dur=None, mrte_mel=None, mrte_mel_lengths=None,
              noise_scale=1, noise_scale_w=1, length_scale=1, denoise_ratio=0, return_codes=False):
        """The older non-PLM text -> (w2v, lf0) path (:996-1077; call site inference.py:158): the prosody codes come
        from the PROMPT mel (first 20 bins -> PLMConv -> max-pool 8 -> PLMConv -> nearest code of the 1024-entry
        codebook, every code held for 8 frames) instead of from the prosody LM.

        The reference adds the projected codes, one per prompt-mel frame, to the text-derived frames (:1057), so it
        only runs when the caller passes ``dur`` [B, N] with sum(dur) / 2 == mel_spk.shape[2] (its RangePredictor call
        also needs ``dur`` 2-D) and the mel length is a multiple of 8 (:999); the same holds here, anything else raises.
        ``x_lengths`` of the encoder come from the PREDICTED durations (:1031-1035), as in the reference.  ``mrte_mel``
        is accepted and -- as in the reference, which overwrites g at :1009 -- does not change the style vector.
        B = 1 (the reference's RangePredictor .squeeze()); a batch here is B independent utterances.
        ``return_codes`` (not in the reference's signature) also returns the prompt's prosody codes, int64 [B, Tm]."""
        if dur is None:
            raise L.HspError("infer(): the reference path needs explicit durations (dur [B, N]); see the docstring")
        B, N = x.shape
        C = self.inter_channels
        Tm = mel_spk.shape[2]
        if Tm % self.stride:
            raise L.HspError("infer(): the prompt mel length must be a multiple of 8 (sequence_mask(len / 8, T / 8))")
        x_lengths = x_lengths.to(torch.int64)
        mel_mask = Fh.sequence_mask(mel_spk_lengths, Tm)
        g = self.emb_g(mel_spk, mel_mask, per_utterance=True).unsqueeze(-1)
        h, x_mask = self.enc_p(x, x_lengths, g, tone, language)
        ref_mel, ref_len = (mrte_mel, mrte_mel_lengths) if mrte_mel is not None else (mel_spk, mel_spk_lengths)
        mel_out, h_mask = self.mel_encoder(ref_mel, ref_len)
        xd = torch.empty(B, C + 1, N, dtype=torch.float32, device=x.device)
        xs = xd[:, :C]
        self.mha(h, mel_out, mask_q=x_mask, mask_k=h_mask, res=h, cbias=self.cond_g(g, force_direct=True), out=xs)
        # predicted durations: only their sum is used (the encoder's lengths); the frames follow the caller's `dur`
        logw = self.duration_predictor(xs, x_mask, g=g, lengths=x_lengths)
        dpred = torch.empty(B, N, dtype=torch.float32, device=x.device)
        frames_pred = torch.empty(B, dtype=torch.float32, device=x.device)
        L.call("hsp_duration_f32", L.fptr(logw), logw.stride(0), L.ptr(x_lengths), 1.0, L.fptr(dpred), dpred.stride(0),
               L.fptr(frames_pred), B, N)
        dcol = xd[:, C]
        dcol.copy_(dur.reshape(B, N).to(torch.float32))
        frames = torch.empty(B, dtype=torch.float32, device=x.device)
        L.call("hsp_duration_f32", None, 0, L.ptr(x_lengths), 1.0, L.fptr(dcol), dcol.stride(0), L.fptr(frames), B, N)
        rng = self.RangePredictor(xd, x_lengths)
        frames_h = frames.cpu()
        T = int(frames_h.max().item())
        T2 = (T - 1) // 2 + 1
        if T2 != Tm:
            raise L.HspError(f"infer(): sum(dur) / 2 = {T2} frames but the prompt mel has {Tm}: the reference adds the "
                             "two tensors frame by frame (t2w2v_transformer.py:1057)")
        x_frame = self.gaussian(xs, dcol, rng, x_lengths, frames, T)
        x_frame = self.dur_downsample(x_frame[:, :, ::2])
        # prosody codes of the prompt
        codes = self.prosody_codes(mel_spk, mel_spk_lengths)
        q = self.quantizer.decode(codes)
        # x_frame + ssl_proj(q * mel_mask) * mel_mask [+ w2v_encoder.cond(g), fused]
        xq = self.ssl_proj(Fh.mask_mul(q, mel_mask), mask=mel_mask, mask_mode=L.MASK_PRE, res=x_frame,
                           cbias=None)
        xq = Fh.add_cbias(xq, self.w2v_encoder.cond(g, force_direct=True))
        enc_len = frames_pred / 2                                     # (:1031-1035) float, from the predicted durations
        len2 = torch.clamp(torch.ceil(enc_len), max=T2).to(torch.int64)
        y_mask = Fh.sequence_mask(len2, T2)
        x2v_enc, _ = self.w2v_encoder(xq, enc_len, g, x_mask=y_mask, cond_added=True)
        w2v_pred = self.w2v_decoder(x2v_enc, y_mask, g=g)
        lf0 = self.pp(w2v_pred, g)
        if return_codes:
            return w2v_pred, lf0.squeeze(1), codes
        return w2v_pred, lf0.squeeze(1)
