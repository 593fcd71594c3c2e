"""Megatron-style tensor parallelism on RCCL-over-xGMI.

Reference consumed these from paddle fleet (hybrid_model.py:139-140
ColumnParallelLinear/RowParallelLinear, :699 VocabParallelEmbedding,
:66-87 parallel_matmul, :951 ParallelCrossEntropy). Here they are built
natively: hipBLASLt GEMMs via torch.matmul + RCCL collectives, with the
vocab-parallel CE reduction done as local fused-kernel passes + small
allreduces (latency-bound one-shot messages on xGMI).
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from paddlefleetx_amd.ops.linear import fused_bias_add, fused_linear

from paddlefleetx_amd.parallel.env import get_hcg
from paddlefleetx_amd.parallel.rng import model_parallel_rng

__all__ = [
    "ColumnParallelLinear", "RowParallelLinear", "VocabParallelEmbedding",
    "ParallelCrossEntropy", "parallel_matmul",
    "copy_to_mp_region", "reduce_from_mp_region", "gather_from_mp_region",
]


def _mp_group():
    return get_hcg().get_model_parallel_group()


class _CopyToMP(torch.autograd.Function):
    """Identity fwd; allreduce grad bwd (input to a column-parallel linear)."""

    @staticmethod
    def forward(ctx, x):
        return x

    @staticmethod
    def backward(ctx, gy):
        g = _mp_group()
        if g.world_size > 1:
            gy = gy.contiguous()
            dist.all_reduce(gy, group=g.group)
        return gy


class _ReduceFromMP(torch.autograd.Function):
    """Allreduce fwd; identity bwd (output of a row-parallel linear)."""

    @staticmethod
    def forward(ctx, x):
        g = _mp_group()
        if g.world_size > 1:
            x = x.contiguous()
            dist.all_reduce(x, group=g.group)
        return x

    @staticmethod
    def backward(ctx, gy):
        return gy


class _GatherFromMP(torch.autograd.Function):
    """All-gather on last dim fwd; local slice bwd."""

    @staticmethod
    def forward(ctx, x):
        g = _mp_group()
        ctx.mp = g.world_size
        ctx.rank = g.rank
        if g.world_size == 1:
            return x
        x = x.contiguous()
        parts = [torch.empty_like(x) for _ in range(g.world_size)]
        dist.all_gather(parts, x, group=g.group)
        return torch.cat(parts, dim=-1)

    @staticmethod
    def backward(ctx, gy):
        if ctx.mp == 1:
            return gy
        chunk = gy.shape[-1] // ctx.mp
        return gy[..., ctx.rank * chunk:(ctx.rank + 1) * chunk].contiguous()


def copy_to_mp_region(x):
    return _CopyToMP.apply(x)


def reduce_from_mp_region(x):
    return _ReduceFromMP.apply(x)


def gather_from_mp_region(x):
    return _GatherFromMP.apply(x)


class ColumnParallelLinear(nn.Module):
    """y = x @ W^T + b with W sharded on output dim across mp ranks.

    Reference consumer: QKV / FFN-up projections (hybrid_model.py:139, 589-605).
    """

    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 gather_output: bool = False, dtype: Optional[torch.dtype] = None,
                 init_std: float = 0.02):
        super().__init__()
        g = _mp_group()
        assert out_features % g.world_size == 0, (
            f"out_features {out_features} not divisible by mp {g.world_size}")
        self.in_features = in_features
        self.out_features = out_features
        self.out_per_rank = out_features // g.world_size
        self.gather_output = gather_output
        self.weight = nn.Parameter(
            torch.empty(self.out_per_rank, in_features, dtype=dtype))
        # mark for checkpoint fuse/split + TP-aware init
        self.weight.is_mp = True
        self.weight.partition_dim = 0
        with model_parallel_rng():
            nn.init.normal_(self.weight, mean=0.0, std=init_std)
        if bias:
            self.bias = nn.Parameter(torch.zeros(self.out_per_rank, dtype=dtype))
            self.bias.is_mp = True
            self.bias.partition_dim = 0
        else:
            self.bias = None

    def forward(self, x):
        x = copy_to_mp_region(x)
        y = fused_linear(x, self.weight, self.bias)
        if self.gather_output:
            y = gather_from_mp_region(y)
        return y


class RowParallelLinear(nn.Module):
    """y = allreduce(x_local @ W_local^T) + b; W sharded on input dim.

    Reference consumer: attention-out / FFN-down projections
    (hybrid_model.py:140, 596).
    """

    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 input_is_parallel: bool = True, dtype: Optional[torch.dtype] = None,
                 init_std: float = 0.02):
        super().__init__()
        g = _mp_group()
        assert in_features % g.world_size == 0
        self.in_per_rank = in_features // g.world_size
        self.input_is_parallel = input_is_parallel
        self.weight = nn.Parameter(
            torch.empty(out_features, self.in_per_rank, dtype=dtype))
        self.weight.is_mp = True
        self.weight.partition_dim = 1
        with model_parallel_rng():
            nn.init.normal_(self.weight, mean=0.0, std=init_std)
        if bias:
            # bias applied after the reduce, replicated
            self.bias = nn.Parameter(torch.zeros(out_features, dtype=dtype))
        else:
            self.bias = None

    def forward(self, x):
        if not self.input_is_parallel:
            g = _mp_group()
            chunk = x.shape[-1] // g.world_size
            x = x[..., g.rank * chunk:(g.rank + 1) * chunk]
        y = fused_linear(x, self.weight, None)
        y = reduce_from_mp_region(y)
        if self.bias is not None:
            y = fused_bias_add(y, self.bias)
        return y


class VocabParallelEmbedding(nn.Module):
    """Embedding table sharded on vocab dim (hybrid_model.py:699-704)."""

    def __init__(self, num_embeddings: int, embedding_dim: int,
                 dtype: Optional[torch.dtype] = None, init_std: float = 0.02):
        super().__init__()
        g = _mp_group()
        assert num_embeddings % g.world_size == 0, (
            f"vocab {num_embeddings} not divisible by mp {g.world_size} "
            "(pad vocab to a multiple of 128*mp)")
        self.num_embeddings = num_embeddings
        self.per_rank = num_embeddings // g.world_size
        self.vocab_start = g.rank * self.per_rank
        self.vocab_end = self.vocab_start + self.per_rank
        self.weight = nn.Parameter(
            torch.empty(self.per_rank, embedding_dim, dtype=dtype))
        self.weight.is_mp = True
        self.weight.partition_dim = 0
        with model_parallel_rng():
            nn.init.normal_(self.weight, mean=0.0, std=init_std)

    def forward(self, ids):
        g = _mp_group()
        if g.world_size == 1:
            return F.embedding(ids, self.weight)
        mask = (ids < self.vocab_start) | (ids >= self.vocab_end)
        local_ids = (ids - self.vocab_start).masked_fill(mask, 0)
        out = F.embedding(local_ids, self.weight)
        out = out.masked_fill(mask.unsqueeze(-1), 0.0)
        return reduce_from_mp_region(out)


def parallel_matmul(x: torch.Tensor, word_embedding_weight: torch.Tensor,
                    parallel_output: bool = True) -> torch.Tensor:
    """Tied-embedding logits: x [.., H] @ W^T with W vocab-sharded.

    Reference: hybrid_model.py:66-87 (_c_identity + matmul + _c_concat).
    """
    g = _mp_group()
    if g.world_size == 1:
        return torch.matmul(x, word_embedding_weight.t())
    x = copy_to_mp_region(x)
    logits = torch.matmul(x, word_embedding_weight.t())
    if parallel_output:
        return logits  # [.., V/mp] fed to ParallelCrossEntropy
    return gather_from_mp_region(logits)


class _VocabParallelCE(torch.autograd.Function):
    """Vocab-parallel softmax cross-entropy (reference c_softmax_with_cross_entropy).

    Local fp32 max/sumexp passes + 3 small allreduces on the [N] vectors
    (one-shot latency-bound messages over xGMI).
    """

    @staticmethod
    def forward(ctx, logits, labels, vocab_start, vocab_end, group, ignore_index):
        if logits.is_cuda:
            from paddlefleetx_amd.ops import hip_ext
            ext = hip_ext()
            lc = logits.contiguous()
            labels = labels.contiguous()
            lmax = ext.row_max(lc)
            if group is not None:
                dist.all_reduce(lmax, op=dist.ReduceOp.MAX, group=group)
            sumexp = ext.row_sumexp(lc, lmax)
            if group is not None:
                dist.all_reduce(sumexp, group=group)
            lse = torch.log(sumexp) + lmax
            picked = ext.gather_label_logit(lc, labels, vocab_start,
                                            ignore_index)
            if group is not None:
                dist.all_reduce(picked, group=group)
            valid = labels != ignore_index
            loss = torch.where(valid, lse - picked, torch.zeros_like(lse))
            ctx.save_for_backward(lc, labels, lse)
        else:
            lf = logits.float()
            lmax = lf.max(dim=-1).values
            if group is not None:
                dist.all_reduce(lmax, op=dist.ReduceOp.MAX, group=group)
            sumexp = torch.exp(lf - lmax[:, None]).sum(dim=-1)
            if group is not None:
                dist.all_reduce(sumexp, group=group)
            lse = torch.log(sumexp) + lmax
            valid = labels != ignore_index
            in_part = (labels >= vocab_start) & (labels < vocab_end) & valid
            local_lab = (labels - vocab_start).masked_fill(~in_part, 0)
            picked = lf.gather(1, local_lab[:, None]).squeeze(1)
            picked = torch.where(in_part, picked, torch.zeros_like(picked))
            if group is not None:
                dist.all_reduce(picked, group=group)
            loss = torch.where(valid, lse - picked, torch.zeros_like(lse))
            ctx.save_for_backward(logits, labels, lse)
        ctx.vocab_start, ctx.vocab_end = vocab_start, vocab_end
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, labels, lse = ctx.saved_tensors
        if logits.is_cuda:
            from paddlefleetx_amd.ops import hip_ext
            g = hip_ext().vp_ce_bwd(dloss.float().contiguous(), logits,
                                    labels, lse, ctx.vocab_start,
                                    ctx.ignore_index)
            return g, None, None, None, None, None
        lf = logits.float()
        p = torch.exp(lf - lse[:, None])
        valid = labels != ctx.ignore_index
        in_part = (labels >= ctx.vocab_start) & (labels < ctx.vocab_end) & valid
        local_lab = (labels - ctx.vocab_start).masked_fill(~in_part, 0)
        p.scatter_add_(1, local_lab[:, None],
                       -in_part.to(p.dtype)[:, None])
        g = (p * dloss[:, None] * valid[:, None]).to(logits.dtype)
        return g, None, None, None, None, None


class ParallelCrossEntropy(nn.Module):
    """Loss over vocab-parallel logits [N, V/mp], labels [N] global ids."""

    def __init__(self, ignore_index: int = -100):
        super().__init__()
        self.ignore_index = ignore_index

    def forward(self, logits, labels):
        g = _mp_group()
        n = logits.shape[-1]
        vocab_start = g.rank * n
        return _VocabParallelCE.apply(
            logits.reshape(-1, n), labels.reshape(-1), vocab_start,
            vocab_start + n, g.group if g.world_size > 1 else None,
            self.ignore_index)
