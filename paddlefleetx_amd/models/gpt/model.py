"""GPT-2/3 decoder, MI355X-native.

One implementation covers the reference's single-card GPTModel
(ppfleetx/models/language_model/gpt/dygraph/single_model.py:608) and the
tensor-parallel GPTModelHybrid (hybrid_model.py:739): the parallel layers
degenerate at mp==1. Hot path: fused-QKV column-parallel GEMM ->
hand-written gfx950 flash attention -> row-parallel GEMM -> fused
bias-gelu FFN -> fused LayerNorm (all in paddlefleetx_amd.ops).

Sequence-parallel (hybrid_model.py:727-735, sequence_parallel_utils.py) is
handled by the sp variants of the linears when `sequence_parallel=True`
(activations [s/mp, b, h] between layers).
"""

from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from paddlefleetx_amd.ops import (FusedLayerNorm, bias_gelu,
                                  decode_attention, decode_linear,
                                  flash_attention,
                                  flash_attention_packed,
                                  fused_softmax_causal, kv_cache_store_fp8)
from paddlefleetx_amd.parallel.env import get_hcg
from paddlefleetx_amd.parallel.rng import (checkpoint_rng_context,
                                            model_parallel_rng)
from paddlefleetx_amd.parallel.tp import (ColumnParallelLinear,
                                          ParallelCrossEntropy,
                                          RowParallelLinear,
                                          VocabParallelEmbedding,
                                          parallel_matmul)
from paddlefleetx_amd.parallel import sp as sp_ops

__all__ = [
    "GPTModel", "GPTForPretraining", "GPTPretrainingCriterion",
    "MultiHeadAttention", "TransformerDecoderLayer", "GPTEmbeddings",
]

KVCache = Tuple[torch.Tensor, torch.Tensor]  # ([B,H,S,D] k, [B,H,S,D] v)


class StaticKVSlot:
    """One layer's view of a StaticKVCache: its k/v buffers (plus the
    per-row scales of an fp8 cache, else None) and the shared lengths.
    Layers read `lens`/`max_len`, never write them."""

    __slots__ = ("owner", "k", "v", "k_scale", "v_scale")

    def __init__(self, owner: "StaticKVCache", k: torch.Tensor,
                 v: torch.Tensor, k_scale: Optional[torch.Tensor] = None,
                 v_scale: Optional[torch.Tensor] = None):
        self.owner, self.k, self.v = owner, k, v
        self.k_scale, self.v_scale = k_scale, v_scale

    @property
    def fp8(self) -> bool:
        return self.k_scale is not None


class DecodeWeightCodes:
    """fp8 copies of decode-step weights (Generation.decode_weight_dtype:
    fp8): per weight, e4m3 codes [N, K] and one fp32 scale per output row
    (ref.quantize_weight_rows), N*K + 4*N bytes next to the bf16 parameter,
    which stays (prefill, the embedding lookup and training read it).

    A plain object, not a module: the codes are no parameters or buffers, so
    they stay out of state_dict and .float() / .to(dtype) on the model never
    casts them. Entries are keyed on the parameter and remember its
    data_ptr and _version: get() re-quantises a weight that was changed in
    place or re-pointed, INTO the same buffers, so a captured decode step
    that reads them stays valid. Quantisation never runs while a stream is
    capturing: refresh() before the capture (GPTForGeneration._start does).
    """

    def __init__(self):
        self._entries = {}

    def __len__(self) -> int:
        return len(self._entries)

    @property
    def nbytes(self) -> int:
        return sum(e[1].numel() + 4 * e[2].numel()
                   for e in self._entries.values())

    @staticmethod
    def _stamp(w):
        return (w.data_ptr(), w._version)

    def _quantize_into(self, w, codes, scale):
        from paddlefleetx_amd.ops import _reference as ref
        if w.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(
                "DecodeWeightCodes: a weight changed (or was first seen) "
                "while a stream is capturing; call refresh() before capture")
        with torch.no_grad():
            c, s = ref.quantize_weight_rows(w.detach())
            codes.view(torch.uint8).copy_(c.view(torch.uint8))
            scale.copy_(s)

    def get(self, w):
        """(codes, scale) of weight w [N, K], quantised on first use and
        again, in place, whenever w's data_ptr or _version moved."""
        e = self._entries.get(id(w))
        if e is None or e[0] is not w or e[1].device != w.device:
            codes = torch.empty(w.shape, dtype=torch.float8_e4m3fn,
                                device=w.device)
            scale = torch.empty(w.shape[0], dtype=torch.float32,
                                device=w.device)
            e = self._entries[id(w)] = [w, codes, scale, None]
        if e[3] != self._stamp(w):
            self._quantize_into(w, e[1], e[2])
            e[3] = self._stamp(w)
        return e[1], e[2]

    def refresh(self, weights) -> None:
        """Bring the codes of every given weight up to date."""
        for w in weights:
            self.get(w)


class StaticKVCache:
    """Preallocated, fixed-address KV cache appended to in place.

    Per-layer k/v buffers [B, h_local, Smax, D] (torch.empty: positions
    past the current length are uninitialised and never read), ONE shared
    device int32 lens[B] and a host-side max_len counter. Indexing gives
    layer i its slot; GPTModel.forward calls advance() once per forward,
    after the layer loop, so every layer of a step sees the same lengths.

    kv_dtype None/"bf16": the buffers have `dtype`. "fp8": they hold
    float8_e4m3fn codes and per-layer k_scale/v_scale [B, h_local, Smax]
    fp32 carry one scale per cached row, D + 4 bytes per row instead of
    2*D (`dtype` is then not used).

    max_seq_len (optional, in [1, max_len]): a FIXED bound that decode
    attention sizes its KV split for, in place of the host counter + 1. The
    kernel clamps per row, so this costs balance, not correctness; it makes
    the split choice independent of the step, which a captured decode step
    needs (and an eager run can share).

    fused_decode_linear (Generation.fused_decode_linear): decoder layers
    that decode one token against this cache run their linears through
    ops.decode_linear (TransformerDecoderLayer._forward_decode_fused).

    weight_codes (Generation.decode_weight_dtype: fp8): a DecodeWeightCodes
    those layers take fp8 codes and scales from instead of the bf16
    weights; None (the default) streams the parameters themselves.
    """

    def __init__(self, num_layers: int, batch_size: int, num_heads: int,
                 max_len: int, head_dim: int,
                 dtype: Optional[torch.dtype] = None, device=None,
                 kv_dtype: Optional[str] = None,
                 max_seq_len: Optional[int] = None,
                 fused_decode_linear: bool = False,
                 weight_codes: Optional[DecodeWeightCodes] = None):
        assert kv_dtype in (None, "bf16", "fp8"), \
            f"StaticKVCache: kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}"
        self.kv_dtype = "fp8" if kv_dtype == "fp8" else "bf16"
        self.capacity = int(max_len)
        assert max_seq_len is None or 1 <= int(max_seq_len) <= self.capacity, \
            f"StaticKVCache: max_seq_len {max_seq_len} not in [1, {max_len}]"
        self.max_seq_len = None if max_seq_len is None else int(max_seq_len)
        self.fused_decode_linear = bool(fused_decode_linear)
        assert weight_codes is None or self.fused_decode_linear, \
            "StaticKVCache: weight_codes needs fused_decode_linear"
        self.weight_codes = weight_codes
        shape = (batch_size, num_heads, self.capacity, head_dim)
        if self.kv_dtype == "fp8":
            dtype = torch.float8_e4m3fn
        self.k = [torch.empty(shape, dtype=dtype, device=device)
                  for _ in range(num_layers)]
        self.v = [torch.empty(shape, dtype=dtype, device=device)
                  for _ in range(num_layers)]
        self.k_scale = self.v_scale = None
        if self.kv_dtype == "fp8":
            self.k_scale = [torch.empty(shape[:3], dtype=torch.float32,
                                        device=device)
                            for _ in range(num_layers)]
            self.v_scale = [torch.empty(shape[:3], dtype=torch.float32,
                                        device=device)
                            for _ in range(num_layers)]
        self.lens = torch.zeros(batch_size, dtype=torch.int32, device=device)
        self.max_len = 0  # host mirror of max(lens)

    @property
    def nbytes(self) -> int:
        """Bytes of the K/V buffers (and scales) over all layers."""
        bufs = self.k + self.v + (self.k_scale or []) + (self.v_scale or [])
        return sum(t.numel() * t.element_size() for t in bufs)

    def __len__(self) -> int:
        return len(self.k)

    def __getitem__(self, i: int) -> StaticKVSlot:
        if self.kv_dtype == "fp8":
            return StaticKVSlot(self, self.k[i], self.v[i], self.k_scale[i],
                                self.v_scale[i])
        return StaticKVSlot(self, self.k[i], self.v[i])

    def advance(self, n: int) -> None:
        assert self.max_len + n <= self.capacity, \
            f"StaticKVCache overflow: {self.max_len}+{n} > {self.capacity}"
        self.lens += n
        self.max_len += n


class MultiHeadAttention(nn.Module):
    """Fused-QKV column-parallel attention (hybrid_model.py:96-392).

    fused_attn=True -> gfx950 flash-attention kernel (O(S) memory);
    otherwise explicit QK^T + fused causal softmax + PV (core_attn,
    hybrid_model.py:303-346) which supports attention dropout.
    """

    def __init__(self, hidden_size: int, num_heads: int,
                 attn_dropout: float = 0.0, fused_attn: bool = True,
                 dtype: Optional[torch.dtype] = None,
                 sequence_parallel: bool = False,
                 init_std: float = 0.02, output_layer_init_std: float = 0.02,
                 cp_backend: str = "ulysses", cp_zigzag: bool = False):
        super().__init__()
        assert cp_backend in ("ulysses", "ring")
        self.cp_backend = cp_backend
        self.cp_zigzag = cp_zigzag
        mp = get_hcg().get_model_parallel_world_size()
        assert num_heads % mp == 0, f"heads {num_heads} not divisible by mp {mp}"
        assert hidden_size % num_heads == 0
        self.num_heads = num_heads
        self.num_heads_local = num_heads // mp
        self.head_dim = hidden_size // num_heads
        self.hidden_size = hidden_size
        self.attn_dropout_p = attn_dropout
        self.fused_attn = fused_attn
        self.sequence_parallel = sequence_parallel
        if sequence_parallel:
            self.qkv = sp_ops.ColumnSequenceParallelLinear(
                hidden_size, 3 * hidden_size, bias=True, dtype=dtype,
                init_std=init_std)
            self.out_proj = sp_ops.RowSequenceParallelLinear(
                hidden_size, hidden_size, bias=True, dtype=dtype,
                init_std=output_layer_init_std)
        else:
            self.qkv = ColumnParallelLinear(hidden_size, 3 * hidden_size,
                                            bias=True, dtype=dtype,
                                            init_std=init_std)
            self.out_proj = RowParallelLinear(hidden_size, hidden_size,
                                              bias=True, dtype=dtype,
                                              init_std=output_layer_init_std)
        self.scale = 1.0 / math.sqrt(self.head_dim)

    def forward(self, x: torch.Tensor, cache: Optional[KVCache] = None,
                use_cache: bool = False
                ) -> Tuple[torch.Tensor, Optional[KVCache]]:
        qkv = self.qkv(x)
        cp = get_hcg().get_context_parallel_world_size()
        if isinstance(cache, StaticKVSlot):
            assert not self.sequence_parallel and cp == 1, \
                "StaticKVCache is not supported on sequence-parallel or " \
                "context-parallel attention layers"
            return self._forward_static(qkv, cache)
        if (cp > 1 and cache is None and not use_cache
                and not self.sequence_parallel):
            # Ulysses CP: x is the [B, S/cp, H] sequence shard; all-to-all
            # inside attention trades seq for heads (parallel/cp.py)
            assert self.attn_dropout_p == 0.0, \
                "attention dropout unsupported under context parallel"
            if self.cp_backend != "ring":
                # ring keeps all heads local; only the a2a path shards them
                assert self.num_heads_local % cp == 0, \
                    f"heads/mp {self.num_heads_local} not divisible by cp {cp}"
            B, Sl, _ = qkv.shape
            qkv = qkv.view(B, Sl, self.num_heads_local, 3 * self.head_dim)
            q, k, v = qkv.split(self.head_dim, dim=-1)  # [B, S/cp, h, D]
            if self.cp_backend == "ring":
                from paddlefleetx_amd.parallel.ring import RingAttention
                ca = RingAttention(scale=self.scale, causal=True,
                                   zigzag=self.cp_zigzag)
            else:
                from paddlefleetx_amd.parallel.cp import UlyssesAttention
                ca = UlyssesAttention(scale=self.scale, causal=True)
            o = ca(q, k, v).reshape(B, Sl, -1)
            return self.out_proj(o), None
        p_att = self.attn_dropout_p if self.training else 0.0
        if (self.fused_attn and cache is None and not use_cache
                and not self.sequence_parallel
                and (p_att == 0.0 or qkv.is_cuda)):
            # packed fast path: kernel reads the fused-QKV linear output
            # directly and writes [B, S, h*D] — zero layout copies.
            # Attention dropout runs IN the kernel (Philox mask keyed by
            # the per-rank local seed via model_parallel_rng — reference
            # hybrid_model.py:328 RNG-tracker dropout)
            B, S, _ = qkv.shape
            packed = qkv.view(B, S, self.num_heads_local, 3, self.head_dim)
            if p_att > 0.0:
                # mp-rank-local Philox seed for the in-kernel mask; the
                # context seeds the generator, so enter it ONLY when a
                # seed is drawn (hipGraph capture forbids reseeding)
                with model_parallel_rng():
                    o = flash_attention_packed(packed, self.num_heads_local,
                                               scale=self.scale,
                                               p_drop=p_att)
            else:
                o = flash_attention_packed(packed, self.num_heads_local,
                                           scale=self.scale)
            return self.out_proj(o), None
        if self.sequence_parallel:
            # x: [s/mp, B, H]; qkv allgathered the seq dim -> [S, B, 3H/mp]
            S, B = qkv.shape[0], qkv.shape[1]
            qkv = qkv.view(S, B, self.num_heads_local, 3 * self.head_dim)
            q, k, v = qkv.split(self.head_dim, dim=-1)
            q = q.permute(1, 2, 0, 3)  # [B, h, S, D]
            k = k.permute(1, 2, 0, 3)
            v = v.permute(1, 2, 0, 3)
        else:
            # x: [B, S, H]
            B, S, _ = x.shape
            qkv = qkv.view(B, S, self.num_heads_local, 3 * self.head_dim)
            q, k, v = qkv.split(self.head_dim, dim=-1)
            q = q.transpose(1, 2)  # [B, h, S, D]
            k = k.transpose(1, 2)
            v = v.transpose(1, 2)

        if cache is not None:
            k = torch.cat([cache[0], k], dim=2)
            v = torch.cat([cache[1], v], dim=2)
        new_cache = (k, v) if use_cache else None

        if self.fused_attn and not (cache is not None and S == 1) and (
                p_att == 0.0 or q.is_cuda):
            if p_att > 0.0:
                with model_parallel_rng():
                    o = flash_attention(q, k, v, causal=True,
                                        scale=self.scale, p_drop=p_att)
            else:
                o = flash_attention(q, k, v, causal=True, scale=self.scale)
        else:
            scores = torch.matmul(q, k.transpose(-1, -2))
            probs = fused_softmax_causal(scores, self.scale)
            if self.attn_dropout_p > 0.0 and self.training:
                with model_parallel_rng():
                    probs = F.dropout(probs, p=self.attn_dropout_p)
            o = torch.matmul(probs, v)
        if self.sequence_parallel:
            o = o.permute(2, 0, 1, 3).reshape(S, B, -1)  # [S, B, H/mp]
        else:
            o = o.transpose(1, 2).reshape(B, S, -1)  # [B, S, H/mp]
        out = self.out_proj(o)
        return out, new_cache

    def _decode_core(self, qkv: torch.Tensor, slot: StaticKVSlot
                     ) -> torch.Tensor:
        """Decode attention of one new token (qkv [B, 1, 3H/mp]) against a
        cache slot, before the output projection: [B, 1, H/mp]."""
        B, S, _ = qkv.shape
        assert S == 1
        packed = qkv.view(B, S, self.num_heads_local, 3, self.head_dim)
        n_cached = slot.owner.max_len
        assert n_cached + S <= slot.owner.capacity, \
            f"StaticKVCache overflow: {n_cached}+{S} > {slot.owner.capacity}"
        return decode_attention(packed, slot.k, slot.v, slot.owner.lens,
                                scale=self.scale,
                                max_seq_len=slot.owner.max_seq_len
                                or n_cached + 1,
                                k_scale=slot.k_scale, v_scale=slot.v_scale)

    def _forward_static(self, qkv: torch.Tensor, slot: StaticKVSlot
                        ) -> Tuple[torch.Tensor, StaticKVSlot]:
        """Inference against a preallocated cache slot. Decode (S == 1) is
        ONE fused kernel on the packed QKV view (in-place append + split-KV
        attention); prefill computes attention as the no-cache forward does
        and copies K/V into the slot (an fp8 slot: one quantising store;
        prefill attention still runs on the unquantised qkv)."""
        assert not (self.training and self.attn_dropout_p > 0.0), \
            "StaticKVCache is inference-only (attention dropout is on)"
        B, S, _ = qkv.shape
        packed = qkv.view(B, S, self.num_heads_local, 3, self.head_dim)
        n_cached = slot.owner.max_len
        assert n_cached + S <= slot.owner.capacity, \
            f"StaticKVCache overflow: {n_cached}+{S} > {slot.owner.capacity}"
        if S == 1:
            return self.out_proj(self._decode_core(qkv, slot)), slot
        assert n_cached == 0, \
            "StaticKVCache prefill (S > 1) needs an empty cache"
        if slot.fp8:
            # one quantising launch; attention below still runs on bf16 qkv
            kv_cache_store_fp8(packed, slot.k, slot.v, slot.k_scale,
                               slot.v_scale)
        else:
            slot.k[:, :, :S].copy_(packed[:, :, :, 1].transpose(1, 2))
            slot.v[:, :, :S].copy_(packed[:, :, :, 2].transpose(1, 2))
        if self.fused_attn:
            o = flash_attention_packed(packed, self.num_heads_local,
                                       scale=self.scale)
        else:
            q = packed[:, :, :, 0].transpose(1, 2)  # [B, h, S, D]
            k = packed[:, :, :, 1].transpose(1, 2)
            v = packed[:, :, :, 2].transpose(1, 2)
            scores = torch.matmul(q, k.transpose(-1, -2))
            probs = fused_softmax_causal(scores, self.scale)
            o = torch.matmul(probs, v).transpose(1, 2).reshape(B, S, -1)
        return self.out_proj(o), slot


class FFN(nn.Module):
    """Column-parallel up-proj -> fused bias-gelu -> row-parallel down-proj."""

    def __init__(self, hidden_size: int, ffn_hidden_size: int,
                 dtype: Optional[torch.dtype] = None, init_std: float = 0.02,
                 output_layer_init_std: float = 0.02,
                 sequence_parallel: bool = False):
        super().__init__()
        if sequence_parallel:
            self.up = sp_ops.ColumnSequenceParallelLinear(
                hidden_size, ffn_hidden_size, bias=False, dtype=dtype,
                init_std=init_std)
            self.down = sp_ops.RowSequenceParallelLinear(
                ffn_hidden_size, hidden_size, bias=True, dtype=dtype,
                init_std=output_layer_init_std)
        else:
            self.up = ColumnParallelLinear(hidden_size, ffn_hidden_size,
                                           bias=False, dtype=dtype,
                                           init_std=init_std)
            self.down = RowParallelLinear(ffn_hidden_size, hidden_size,
                                          bias=True, dtype=dtype,
                                          init_std=output_layer_init_std)
        # bias folded into the fused bias_gelu epilogue
        mp = get_hcg().get_model_parallel_world_size()
        self.up_bias = nn.Parameter(
            torch.zeros(ffn_hidden_size // mp, dtype=dtype))
        self.up_bias.is_mp = True
        self.up_bias.partition_dim = 0

    def forward(self, x):
        return self.down(bias_gelu(self.up(x), self.up_bias))


class TransformerDecoderLayer(nn.Module):
    """Pre-LN decoder layer (hybrid_model.py:489-674); MoE branch optional."""

    def __init__(self, hidden_size: int, num_heads: int, ffn_hidden_size: int,
                 hidden_dropout: float = 0.0, attn_dropout: float = 0.0,
                 fused_attn: bool = True, dtype: Optional[torch.dtype] = None,
                 sequence_parallel: bool = False, init_std: float = 0.02,
                 num_layers_for_scale: int = 1, expert_module: Optional[nn.Module] = None,
                 recompute_granularity: str = "full", use_recompute: bool = False,
                 cp_backend: str = "ulysses", cp_zigzag: bool = False):
        super().__init__()
        out_std = init_std / math.sqrt(2.0 * num_layers_for_scale)
        self.ln1 = FusedLayerNorm(hidden_size, dtype=dtype)
        self.ln2 = FusedLayerNorm(hidden_size, dtype=dtype)
        self.sequence_parallel = sequence_parallel
        self.hidden_dropout_p = hidden_dropout
        self.use_recompute = use_recompute
        self.recompute_granularity = recompute_granularity
        if sequence_parallel:
            sp_ops.mark_as_sp_param(self.ln1.weight)
            sp_ops.mark_as_sp_param(self.ln1.bias)
            sp_ops.mark_as_sp_param(self.ln2.weight)
            sp_ops.mark_as_sp_param(self.ln2.bias)
        self.attn = MultiHeadAttention(hidden_size, num_heads,
                                       attn_dropout=attn_dropout,
                                       fused_attn=fused_attn, dtype=dtype,
                                       sequence_parallel=sequence_parallel,
                                       init_std=init_std,
                                       output_layer_init_std=out_std,
                                       cp_backend=cp_backend,
                                       cp_zigzag=cp_zigzag)
        if expert_module is not None:
            self.ffn = expert_module
        else:
            self.ffn = FFN(hidden_size, ffn_hidden_size, dtype=dtype,
                           init_std=init_std, output_layer_init_std=out_std,
                           sequence_parallel=sequence_parallel)

    def _dropout(self, x):
        if self.hidden_dropout_p > 0.0 and self.training:
            return F.dropout(x, p=self.hidden_dropout_p)
        return x

    def _attn_branch(self, x, cache=None, use_cache=False):
        """dropout(attn(ln1(x))) — the branch WITHOUT the residual add
        (the add is fused into ln2, see forward)."""
        h = self.ln1(x)
        if self.use_recompute and self.recompute_granularity == "core_attn" \
                and self.training and cache is None and not use_cache \
                and torch.is_grad_enabled():
            # recompute only the attention core (QK^T/softmax/PV + projs);
            # reference granularity "core_attn" (hybrid_model.py:303-346)
            a = checkpoint(lambda t: self.attn(t)[0], h,
                           use_reentrant=False,
                           context_fn=checkpoint_rng_context)
            return self._dropout(a), None
        a, new_cache = self.attn(h, cache=cache, use_cache=use_cache)
        return self._dropout(a), new_cache

    def _attn_branch_nocache(self, x):
        return self._attn_branch(x)[0]

    def _forward_decode_fused(self, x, slot: StaticKVSlot):
        """One decode token with every linear as a decode_linear launch
        (bias, GELU and the residual adds ride in the epilogues): 7
        launches plus the attention merge."""
        attn, ffn = self.attn, self.ffn
        codes = slot.owner.weight_codes

        def wq(weight):
            # (weight, weight_scale): fp8 codes when the cache carries them
            return codes.get(weight) if codes is not None else (weight, None)

        h = self.ln1(x)
        w, s = wq(attn.qkv.weight)
        qkv = decode_linear(h, w, attn.qkv.bias, weight_scale=s)
        o = attn._decode_core(qkv, slot)
        w, s = wq(attn.out_proj.weight)
        y = decode_linear(o, w, attn.out_proj.bias, residual=x,
                          weight_scale=s)
        h2 = self.ln2(y)
        w, s = wq(ffn.up.weight)
        u = decode_linear(h2, w, ffn.up_bias, activation="gelu",
                          weight_scale=s)
        w, s = wq(ffn.down.weight)
        return decode_linear(u, w, ffn.down.bias, residual=y, weight_scale=s)

    def forward(self, x, cache: Optional[KVCache] = None, use_cache: bool = False):
        if (isinstance(cache, StaticKVSlot)
                and cache.owner.fused_decode_linear
                and x.shape[1] == 1 and not self.training
                and isinstance(self.ffn, FFN) and not self.sequence_parallel):
            z = self._forward_decode_fused(x, cache)
            return (z, cache) if use_cache else z
        if self.use_recompute and self.recompute_granularity == "full_attn" \
                and self.training and not use_cache and torch.is_grad_enabled():
            a = checkpoint(self._attn_branch_nocache, x,
                           use_reentrant=False,
                           context_fn=checkpoint_rng_context)
            new_cache = None
        else:
            a, new_cache = self._attn_branch(x, cache, use_cache)
        # fused: h2 = LN(x + a), y = x + a (one kernel; the backward joins
        # the residual gradient in the same pass)
        from paddlefleetx_amd.ops import layernorm_residual
        h2, y = layernorm_residual(a, x, self.ln2.weight, self.ln2.bias,
                                   self.ln2.eps)
        z = y + self._dropout(self.ffn(h2))
        if use_cache:
            return z, new_cache
        return z


class GPTEmbeddings(nn.Module):
    """Vocab-parallel word embedding + learned positions (hybrid_model.py:682-736)."""

    def __init__(self, vocab_size: int, hidden_size: int,
                 max_position_embeddings: int, dropout: float = 0.0,
                 dtype: Optional[torch.dtype] = None,
                 sequence_parallel: bool = False, init_std: float = 0.02):
        super().__init__()
        self.word_embeddings = VocabParallelEmbedding(vocab_size, hidden_size,
                                                      dtype=dtype,
                                                      init_std=init_std)
        self.position_embeddings = nn.Embedding(max_position_embeddings,
                                                hidden_size, dtype=dtype)
        # REPLICATED across mp ranks -> must init from the global stream,
        # not the per-mp-rank local_seed (else SP's seq allgather mixes
        # inconsistent copies; reference env.py:34-98 seed discipline)
        nn.init.normal_(self.position_embeddings.weight, std=init_std)
        self.dropout_p = dropout
        self.sequence_parallel = sequence_parallel

    def forward(self, input_ids, position_ids=None):
        B, S = input_ids.shape
        if position_ids is None:
            position_ids = torch.arange(S, device=input_ids.device).unsqueeze(0)
        x = self.word_embeddings(input_ids) + self.position_embeddings(position_ids)
        if self.dropout_p > 0.0 and self.training:
            x = F.dropout(x, p=self.dropout_p)
        if self.sequence_parallel:
            x = sp_ops.scatter_to_sp_region(x)
        return x


class GPTModel(nn.Module):
    """Decoder stack. Activations [B, S, H] ([s/mp, B, H] under SP)."""

    def __init__(self, vocab_size: int = 50304, hidden_size: int = 1024,
                 num_layers: int = 24, num_attention_heads: int = 16,
                 ffn_hidden_size: Optional[int] = None,
                 max_position_embeddings: int = 1024,
                 hidden_dropout_prob: float = 0.0,
                 attention_probs_dropout_prob: float = 0.0,
                 fused_attn: bool = True, use_recompute: bool = False,
                 recompute_granularity: str = "full",
                 sequence_parallel: bool = False,
                 initializer_range: float = 0.02,
                 moe_configs: Optional[Dict[str, Any]] = None,
                 cp_backend: str = "ulysses", cp_zigzag: bool = False,
                 dtype: Optional[torch.dtype] = None, **unused: Any):
        super().__init__()
        ffn_hidden_size = ffn_hidden_size or 4 * hidden_size

        def _make_expert_module():
            """MoE FFN when expert_mode (hybrid_model.py:535-587)."""
            if not (moe_configs and moe_configs.get("expert_mode", False)):
                return None
            from paddlefleetx_amd.models.moe import MoELayer
            return MoELayer(
                hidden_size, ffn_hidden_size,
                num_experts=moe_configs.get("num_experts", 1),
                gate=moe_configs.get("gate", "gshard"),
                top_k=moe_configs.get("top_k", 2),
                capacity_factor=moe_configs.get("capacity_factor"),
                dtype=dtype)
        self.use_recompute = use_recompute
        self.recompute_granularity = recompute_granularity
        self.sequence_parallel = sequence_parallel
        self.embeddings = GPTEmbeddings(vocab_size, hidden_size,
                                        max_position_embeddings,
                                        dropout=hidden_dropout_prob, dtype=dtype,
                                        sequence_parallel=sequence_parallel,
                                        init_std=initializer_range)
        self.layers = nn.ModuleList([
            TransformerDecoderLayer(hidden_size, num_attention_heads,
                                    ffn_hidden_size,
                                    hidden_dropout=hidden_dropout_prob,
                                    attn_dropout=attention_probs_dropout_prob,
                                    fused_attn=fused_attn, dtype=dtype,
                                    sequence_parallel=sequence_parallel,
                                    init_std=initializer_range,
                                    num_layers_for_scale=num_layers,
                                    use_recompute=use_recompute,
                                    recompute_granularity=recompute_granularity,
                                    expert_module=_make_expert_module(),
                                    cp_backend=cp_backend,
                                    cp_zigzag=cp_zigzag)
            for _ in range(num_layers)])
        self.final_ln = FusedLayerNorm(hidden_size, dtype=dtype)
        if sequence_parallel:
            sp_ops.mark_as_sp_param(self.final_ln.weight)
            sp_ops.mark_as_sp_param(self.final_ln.bias)

    def forward(self, input_ids, position_ids=None,
                caches: Optional[List[KVCache]] = None, use_cache: bool = False):
        x = self.embeddings(input_ids, position_ids)
        new_caches: List[KVCache] = []
        for i, layer in enumerate(self.layers):
            cache_i = caches[i] if caches is not None else None
            if (self.use_recompute and self.recompute_granularity == "full"
                    and self.training and not use_cache
                    and torch.is_grad_enabled()):
                x = checkpoint(layer, x, use_reentrant=False,
                               context_fn=checkpoint_rng_context)
            elif use_cache:
                x, c = layer(x, cache=cache_i, use_cache=True)
                new_caches.append(c)
            else:
                x = layer(x, cache=cache_i)
        if isinstance(caches, StaticKVCache):
            # every layer appended at the same lens; move them once
            caches.advance(input_ids.shape[1])
            new_caches = caches
        x = self.final_ln(x)
        if self.sequence_parallel:
            x = sp_ops.gather_from_sp_region(x)
        if use_cache:
            return x, new_caches
        return x


class GPTForPretraining(nn.Module):
    """Adds tied-embedding parallel logits (hybrid_model.py:897-941)."""

    def __init__(self, gpt: GPTModel):
        super().__init__()
        self.gpt = gpt

    def forward(self, input_ids, position_ids=None, caches=None,
                use_cache: bool = False):
        out = self.gpt(input_ids, position_ids, caches=caches,
                       use_cache=use_cache)
        if use_cache:
            hidden, new_caches = out
        else:
            hidden = out
        logits = parallel_matmul(hidden, self.gpt.embeddings.word_embeddings.weight,
                                 parallel_output=True)
        if use_cache:
            return logits, new_caches
        return logits


class GPTForSequenceClassification(nn.Module):
    """GPT + classification head on the last real token
    (single_model.py:856-897)."""

    def __init__(self, gpt: GPTModel, num_classes: int = 2):
        super().__init__()
        self.gpt = gpt
        hidden = gpt.final_ln.weight.shape[0]
        self.score = nn.Linear(hidden, num_classes, bias=False,
                               dtype=gpt.final_ln.weight.dtype)

    def forward(self, input_ids, attention_mask=None, position_ids=None):
        hidden = self.gpt(input_ids, position_ids)
        logits = self.score(hidden)  # [B, S, C]
        if attention_mask is not None:
            last = attention_mask.long().sum(dim=-1).clamp(min=1) - 1
        else:
            last = torch.full((input_ids.shape[0],), input_ids.shape[1] - 1,
                              device=input_ids.device, dtype=torch.long)
        return logits[torch.arange(logits.shape[0], device=logits.device),
                      last]


class GPTPretrainingCriterion(nn.Module):
    """(Parallel) softmax CE with loss mask (hybrid_model.py:943-996).
    Under context parallel each rank scores its sequence shard and the
    masked sum/count are all-reduced so every rank sees the global loss."""

    def __init__(self, sequence_parallel: bool = False):
        super().__init__()
        self.ce = ParallelCrossEntropy()

    def forward(self, logits, labels, loss_mask=None):
        losses = self.ce(logits, labels)  # [N] fp32
        cp = get_hcg().get_context_parallel_world_size()
        if loss_mask is not None:
            m = loss_mask.reshape(-1).float()
            num, den = (losses * m).sum(), m.sum()
        else:
            num = losses.sum()
            den = torch.tensor(float(losses.numel()), device=losses.device)
        if cp > 1:
            from paddlefleetx_amd.parallel.cp import cp_allreduce_sum
            num = cp_allreduce_sum(num)
            den = cp_allreduce_sum(den)
        return num / den.clamp(min=1.0)
