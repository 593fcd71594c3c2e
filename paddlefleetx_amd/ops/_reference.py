"""Plain-PyTorch fp32 reference implementations of every HIP op.

These are the numerics twins the GPU kernels are tested against
(SURVEY.md §4 test strategy), and the CPU execution path for tests on
non-GPU hosts. They are NOT used on a GPU box — ops dispatch to the HIP
extension there and fail loudly if it is missing.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def layernorm_fwd(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                  eps: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Returns (y, mean, rstd); stats in fp32, y in x.dtype. x: [N, H]."""
    xf = x.float()
    mean = xf.mean(dim=-1)
    var = xf.var(dim=-1, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    y = (xf - mean[:, None]) * rstd[:, None] * weight.float() + bias.float()
    return y.to(x.dtype), mean, rstd


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor,
                  mean: torch.Tensor, rstd: torch.Tensor
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    xf, dyf, wf = x.float(), dy.float(), weight.float()
    H = x.shape[-1]
    xhat = (xf - mean[:, None]) * rstd[:, None]
    dyw = dyf * wf
    c1 = dyw.mean(dim=-1, keepdim=True)
    c2 = (dyw * xhat).mean(dim=-1, keepdim=True)
    dx = (dyw - c1 - xhat * c2) * rstd[:, None]
    dw = (dyf * xhat).sum(dim=0)
    db = dyf.sum(dim=0)
    return dx.to(x.dtype), dw, db


def layernorm_fwd_residual(x: torch.Tensor, res: torch.Tensor,
                           weight: torch.Tensor, bias: torch.Tensor,
                           eps: float):
    """LN(x + res); returns (y, mean, rstd, sum) with sum = x + res
    in x.dtype (the fused residual stream)."""
    s = (x.float() + res.float()).to(x.dtype)
    y, mean, rstd = layernorm_fwd(s, weight, bias, eps)
    return y, mean, rstd, s


def layernorm_bwd_residual(dy: torch.Tensor, s: torch.Tensor,
                           weight: torch.Tensor, mean: torch.Tensor,
                           rstd: torch.Tensor, dsum: torch.Tensor):
    """LN bwd with the residual-stream gradient fused into dx."""
    dx, dw, db = layernorm_bwd(dy, s, weight, mean, rstd)
    dx = (dx.float() + dsum.float()).to(dx.dtype)
    return dx, dw, db


def rmsnorm_fwd(x: torch.Tensor, weight: torch.Tensor, eps: float
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(dim=-1) + eps)
    y = xf * rstd[:, None] * weight.float()
    return y.to(x.dtype), rstd


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor,
                rstd: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    xf, dyf, wf = x.float(), dy.float(), weight.float()
    H = x.shape[-1]
    xhat = xf * rstd[:, None]
    dyw = dyf * wf
    c = (dyw * xhat).mean(dim=-1, keepdim=True)
    dx = (dyw - xhat * c) * rstd[:, None]
    dw = (dyf * xhat).sum(dim=0)
    return dx.to(x.dtype), dw


def bias_gelu_fwd(x: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    xf = x.float()
    if bias is not None:
        xf = xf + bias.float()
    # tanh approximation (matches the fused kernel)
    y = 0.5 * xf * (1.0 + torch.tanh(0.7978845608028654 * (xf + 0.044715 * xf ** 3)))
    return y.to(x.dtype)


def bias_gelu_bwd(dy: torch.Tensor, x: torch.Tensor, bias: Optional[torch.Tensor]
                  ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    xf = x.float()
    if bias is not None:
        xf = xf + bias.float()
    k = 0.7978845608028654
    t = torch.tanh(k * (xf + 0.044715 * xf ** 3))
    dgelu = 0.5 * (1.0 + t) + 0.5 * xf * (1.0 - t * t) * k * (1.0 + 3 * 0.044715 * xf * xf)
    dx = (dy.float() * dgelu)
    db = dx.reshape(-1, x.shape[-1]).sum(0) if bias is not None else None
    return dx.to(x.dtype), db


def decode_linear(x: torch.Tensor, weight: torch.Tensor,
                  bias: Optional[torch.Tensor] = None,
                  residual: Optional[torch.Tensor] = None,
                  activation: Optional[str] = None) -> torch.Tensor:
    """y = act(x @ weight^T + bias) + residual in fp32, one cast to x.dtype.

    x [..., K], weight [N, K], bias [N], residual [..., N]; activation None
    or "gelu" (the tanh form of bias_gelu_fwd).
    """
    assert activation in (None, "none", "gelu"), activation
    yf = torch.matmul(x.float(), weight.float().t())
    if bias is not None:
        yf = yf + bias.float()
    if activation == "gelu":
        yf = 0.5 * yf * (1.0 + torch.tanh(
            0.7978845608028654 * (yf + 0.044715 * yf ** 3)))
    if residual is not None:
        yf = yf + residual.float()
    return yf.to(x.dtype)


def attention_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                  causal: bool, scale: Optional[float] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """q,k,v: [B, H, S, D] -> (o [B,H,S,D], lse [B,H,S]) computed in fp32."""
    qf, kf, vf = q.float(), k.float(), v.float()
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        Sq, Sk = s.shape[-2], s.shape[-1]
        mask = torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).tril(Sk - Sq)
        s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = torch.matmul(p, vf)
    return o.to(q.dtype), lse


def attention_bwd(do: torch.Tensor, q: torch.Tensor, k: torch.Tensor,
                  v: torch.Tensor, o: torch.Tensor, lse: torch.Tensor,
                  causal: bool, scale: Optional[float] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    qf, kf, vf, dof, of = q.float(), k.float(), v.float(), do.float(), o.float()
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        Sq, Sk = s.shape[-2], s.shape[-1]
        mask = torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).tril(Sk - Sq)
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.exp(s - lse[..., None].float())
    dv = torch.matmul(p.transpose(-1, -2), dof)
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dof * of).sum(dim=-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = torch.matmul(ds, kf)
    dk = torch.matmul(ds.transpose(-1, -2), qf)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


def decode_attention(qkv: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, seq_lens: torch.Tensor,
                     scale: Optional[float] = None) -> torch.Tensor:
    """Single-token attention over a preallocated cache, fp32 math.

    qkv [B, 1, h, 3, D] (new token); k_cache/v_cache [B, h, Smax, D] are
    appended IN PLACE at position seq_lens[b]; positions past it are never
    read (they may be uninitialised). Returns [B, 1, h*D] in qkv.dtype.
    """
    B, _, h, _, D = qkv.shape
    Smax = k_cache.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    q, k_new, v_new = qkv[:, 0, :, 0], qkv[:, 0, :, 1], qkv[:, 0, :, 2]
    lens = seq_lens.long().clamp(0, Smax - 1)
    rows = torch.arange(B, device=qkv.device)
    k_cache[rows, :, lens] = k_new.to(k_cache.dtype)
    v_cache[rows, :, lens] = v_new.to(v_cache.dtype)
    valid = (torch.arange(Smax, device=qkv.device)[None, :]
             <= lens[:, None])[:, None, :]  # [B, 1, Smax]
    # select, never multiply: the tail may hold NaN/Inf
    kf = torch.where(valid[..., None], k_cache.float(), 0.0)
    vf = torch.where(valid[..., None], v_cache.float(), 0.0)
    s = torch.einsum("bhd,bhsd->bhs", q.float(), kf) * scale
    s = s.masked_fill(~valid, float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("bhs,bhsd->bhd", p, vf)
    return o.reshape(B, 1, h * D).to(qkv.dtype)


FP8_MAX = 448.0  # largest finite float8_e4m3fn


def quantize_kv_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row fp8 quantisation of the KV cache: x [..., D] -> (codes
    [..., D] float8_e4m3fn, scale [...] fp32). fp32 arithmetic:
    amax = max|x|; scale = amax / 448, inv = 448 / amax (both 1 for an
    all-zero row); code = e4m3_rne(clamp(x * inv, -448, 448)). The clamp
    comes before the cast, which would turn overflow into NaN."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    nz = amax > 0
    safe = torch.where(nz, amax, torch.ones_like(amax))
    scale = torch.where(nz, safe / FP8_MAX, torch.ones_like(amax))
    inv = torch.where(nz, FP8_MAX / safe, torch.ones_like(amax))
    codes = (xf * inv[..., None]).clamp(-FP8_MAX, FP8_MAX) \
        .to(torch.float8_e4m3fn)
    return codes, scale


def dequantize_kv_rows(codes: torch.Tensor, scale: torch.Tensor
                       ) -> torch.Tensor:
    """fp32 [..., D] = float(code) * scale of the row."""
    return codes.float() * scale.float()[..., None]


def quantize_weight_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-output-row fp8 quantisation of a linear's weight: w [N, K] ->
    (codes [N, K] float8_e4m3fn, scale [N] fp32), the arithmetic of
    quantize_kv_rows. One scale per row keeps the scale out of the k loop
    (one multiply per output element) and an outlier row costs no other."""
    assert w.dim() == 2, f"quantize_weight_rows: w must be [N, K], got {tuple(w.shape)}"
    return quantize_kv_rows(w)


def decode_linear_fp8(x: torch.Tensor, codes: torch.Tensor,
                      w_scale: torch.Tensor,
                      bias: Optional[torch.Tensor] = None,
                      residual: Optional[torch.Tensor] = None,
                      activation: Optional[str] = None) -> torch.Tensor:
    """decode_linear over quantize_weight_rows codes, fp32 math:
    y = act((x @ codes^T) * w_scale + bias) + residual, one cast to x.dtype.

    x [..., K], codes [N, K] float8_e4m3fn, w_scale [N] fp32, bias [N],
    residual [..., N]; activation None or "gelu". The scale multiplies the
    finished sum, as in the kernel's epilogue.
    """
    assert activation in (None, "none", "gelu"), activation
    yf = torch.matmul(x.float(), codes.float().t()) * w_scale.float()
    if bias is not None:
        yf = yf + bias.float()
    if activation == "gelu":
        yf = 0.5 * yf * (1.0 + torch.tanh(
            0.7978845608028654 * (yf + 0.044715 * yf ** 3)))
    if residual is not None:
        yf = yf + residual.float()
    return yf.to(x.dtype)


def decode_attention_fp8(qkv: torch.Tensor, k_cache: torch.Tensor,
                         v_cache: torch.Tensor, k_scale: torch.Tensor,
                         v_scale: torch.Tensor, seq_lens: torch.Tensor,
                         scale: Optional[float] = None) -> torch.Tensor:
    """decode_attention over an fp8 cache, fp32 math.

    k_cache/v_cache [B, h, Smax, D] float8_e4m3fn with k_scale/v_scale
    [B, h, Smax] fp32. The new token's K/V are quantised by
    quantize_kv_rows and appended IN PLACE (codes and scales) at position
    seq_lens[b], but enter the softmax unquantised; positions past it are
    never read (they may hold NaN codes and NaN scales).
    """
    B, _, h, _, D = qkv.shape
    Smax = k_cache.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    q, k_new, v_new = qkv[:, 0, :, 0], qkv[:, 0, :, 1], qkv[:, 0, :, 2]
    lens = seq_lens.long().clamp(0, Smax - 1)
    rows = torch.arange(B, device=qkv.device)
    for cache, scales, new in ((k_cache, k_scale, k_new),
                               (v_cache, v_scale, v_new)):
        codes, sc = quantize_kv_rows(new)
        cache[rows, :, lens] = codes
        scales[rows, :, lens] = sc
    pos = torch.arange(Smax, device=qkv.device)[None, :]
    cached = (pos < lens[:, None])[:, None, :]  # [B, 1, Smax]
    is_new = (pos == lens[:, None])[:, None, :]
    # select, never multiply: the tail may hold NaN codes and scales
    kf = torch.where(cached[..., None], dequantize_kv_rows(k_cache, k_scale),
                     0.0)
    vf = torch.where(cached[..., None], dequantize_kv_rows(v_cache, v_scale),
                     0.0)
    kf = torch.where(is_new[..., None], k_new.float()[:, :, None], kf)
    vf = torch.where(is_new[..., None], v_new.float()[:, :, None], vf)
    s = torch.einsum("bhd,bhsd->bhs", q.float(), kf) * scale
    s = s.masked_fill(~(cached | is_new), float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("bhs,bhsd->bhd", p, vf)
    return o.reshape(B, 1, h * D).to(qkv.dtype)


def kv_store_fp8(qkv: torch.Tensor, k_cache: torch.Tensor,
                 v_cache: torch.Tensor, k_scale: torch.Tensor,
                 v_scale: torch.Tensor) -> None:
    """Prefill store: quantise K and V of the packed qkv [B, S, h, 3, D]
    into positions [0, S) of the fp8 caches and their scales, in place."""
    S = qkv.shape[1]
    assert S <= k_cache.shape[2], "kv_store_fp8: S must be <= Smax"
    for cache, scales, which in ((k_cache, k_scale, 1), (v_cache, v_scale, 2)):
        codes, sc = quantize_kv_rows(qkv[:, :, :, which].transpose(1, 2))
        cache[:, :, :S].copy_(codes)
        scales[:, :, :S].copy_(sc)


def softmax_causal_fwd(scores: torch.Tensor, scale: float) -> torch.Tensor:
    """Fused scale + causal-mask + softmax on [B, H, Sq, Sk] scores (fp32 math)."""
    s = scores.float() * scale
    Sq, Sk = s.shape[-2], s.shape[-1]
    mask = torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).tril(Sk - Sq)
    s = s.masked_fill(~mask, float("-inf"))
    return torch.softmax(s, dim=-1).to(scores.dtype)


def softmax_causal_bwd(dy: torch.Tensor, y: torch.Tensor, scale: float) -> torch.Tensor:
    yf, dyf = y.float(), dy.float()
    ds = yf * (dyf - (dyf * yf).sum(dim=-1, keepdim=True)) * scale
    return ds.to(y.dtype)


def cross_entropy_fwd(logits: torch.Tensor, labels: torch.Tensor,
                      ignore_index: int = -100
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits [N, V] (any float dtype), labels [N] -> (loss [N] fp32, lse [N] fp32).

    loss = lse - logit[label]; 0 where ignored.
    """
    lf = logits.float()
    lse = torch.logsumexp(lf, dim=-1)
    valid = labels != ignore_index
    safe = labels.clamp(min=0)
    picked = lf.gather(1, safe[:, None]).squeeze(1)
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse))
    return loss, lse


def cross_entropy_bwd(dloss: torch.Tensor, logits: torch.Tensor,
                      labels: torch.Tensor, lse: torch.Tensor,
                      ignore_index: int = -100) -> torch.Tensor:
    lf = logits.float()
    p = torch.exp(lf - lse[:, None])
    valid = (labels != ignore_index)
    safe = labels.clamp(min=0)
    onehot = torch.zeros_like(lf)
    onehot.scatter_(1, safe[:, None], 1.0)
    g = (p - onehot) * dloss[:, None] * valid[:, None]
    return g.to(logits.dtype)


def adamw_step(master: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor,
               exp_avg_sq: torch.Tensor, model_out: Optional[torch.Tensor],
               lr: float, beta1: float, beta2: float, eps: float,
               weight_decay: float, step: int) -> None:
    """Flat-buffer AdamW, fp32 master + bf16 model copy. In-place."""
    gf = grad.float()
    exp_avg.mul_(beta1).add_(gf, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (exp_avg_sq / bc2).sqrt().add_(eps)
    master.mul_(1 - lr * weight_decay)
    master.addcdiv_(exp_avg / bc1, denom, value=-lr)
    if model_out is not None:
        model_out.copy_(master.to(model_out.dtype))


def rope_fwd(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x: [B, H, S, D]; cos/sin: [S, D/2] fp32. Interleaved-pair rotation."""
    xf = x.float()
    x1 = xf[..., 0::2]
    x2 = xf[..., 1::2]
    c = cos[None, None, :, :]
    s = sin[None, None, :, :]
    o1 = x1 * c - x2 * s
    o2 = x2 * c + x1 * s
    out = torch.stack((o1, o2), dim=-1).flatten(-2)
    return out.to(x.dtype)


def rope_bwd(dy: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    return rope_fwd(dy, cos, -sin)


def topp_sampling(probs: torch.Tensor, top_p: torch.Tensor,
                  seed: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Nucleus sampling. probs [B, V] (rows sum to 1), top_p [B].

    Returns (ids [B,1] int64, probs_of_ids [B,1]). Reference semantics of
    ppfleetx/ops/topp_sampling.cu:377 (smallest prefix of sorted probs with
    cumsum >= p, sampled proportionally).
    """
    if seed >= 0:
        g = torch.Generator(device=probs.device)
        g.manual_seed(seed)
    else:
        g = None
    sorted_p, sorted_idx = torch.sort(probs.float(), dim=-1, descending=True)
    cum = torch.cumsum(sorted_p, dim=-1)
    # keep tokens until cumulative prob reaches top_p (always keep first)
    keep = cum - sorted_p < top_p[:, None]
    keep[:, 0] = True
    filt = sorted_p * keep
    filt = filt / filt.sum(dim=-1, keepdim=True)
    pick = torch.multinomial(filt, 1, generator=g)
    ids = sorted_idx.gather(1, pick)
    pp = probs.gather(1, ids)
    return ids, pp


def sample_token_filter(logits: torch.Tensor, ids_buf: torch.Tensor,
                        lens: torch.Tensor, temperature: float = 1.0,
                        top_k: int = 0, top_p: float = 1.0,
                        repetition_penalty: float = 1.0, min_length: int = 0,
                        eos_token_id: int = -1
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Steps 1-6 of sample_token: (processed logits, probs, keep), all [B, V].

    processed: fp32 logits after the min-length mask and the repetition
    penalty (before temperature). probs: softmax(processed / temperature).
    keep: the tokens that survive top-k and top-p. Top-p is tie-inclusive:
    every token equal in probability to the last one of the sorted nucleus
    is kept, where the sort in TopPProcess keeps an arbitrary subset of a
    tie. A zero-probability token is never kept.
    """
    x = logits.float().clone()
    B, V = x.shape
    T = ids_buf.shape[1]
    L = lens.long().clamp(0, T)
    if 0 <= eos_token_id < V:
        x[:, eos_token_id] = torch.where(
            L < min_length, torch.full_like(x[:, eos_token_id], -math.inf),
            x[:, eos_token_id])
    if repetition_penalty != 1.0:
        valid = (torch.arange(T, device=x.device)[None] < L[:, None]) \
            & (ids_buf >= 0) & (ids_buf < V)
        seen = torch.zeros(B, V, dtype=torch.int32, device=x.device)
        seen.scatter_add_(1, ids_buf.clamp(0, V - 1), valid.to(torch.int32))
        x = torch.where(seen > 0,
                        torch.where(x < 0, x * repetition_penalty,
                                    x / repetition_penalty), x)
    probs = F.softmax(x / temperature if temperature != 1.0 else x, dim=-1)
    q = probs
    if 0 < top_k < V:
        kth = torch.topk(q, top_k, dim=-1).values[:, -1:]
        q = torch.where(q >= kth, q, torch.zeros_like(q))
    if top_p < 1.0:
        sorted_q, _ = torch.sort(q, dim=-1, descending=True)
        # shortest prefix whose mass exceeds top_p: sorted token j stays
        # while the mass ahead of it does not (cumsum is monotone, so the
        # kept positions are a prefix)
        ahead = torch.cumsum(sorted_q, dim=-1).roll(1, -1)
        ahead[:, 0] = 0.0
        ncut = (ahead <= max(top_p, 0.0)).sum(-1, keepdim=True)
        last = sorted_q.gather(1, ncut - 1)
        q = torch.where(q >= last, q, torch.zeros_like(q))
    return x, probs, q > 0


def sample_token(logits: torch.Tensor, ids_buf: torch.Tensor,
                 lens: torch.Tensor, unfinished: torch.Tensor,
                 u: torch.Tensor, next_tokens: torch.Tensor,
                 greedy: bool = False, temperature: float = 1.0,
                 top_k: int = 0, top_p: float = 1.0,
                 repetition_penalty: float = 1.0, min_length: int = 0,
                 eos_token_id: int = -1, pad_token_id: int = 0
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 twin of csrc/sample_token.hip; see ops.sample_token. Only tensor
    ops on the inputs' device, no host synchronisation."""
    B, V = logits.shape
    T = ids_buf.shape[1]
    L = lens.long().clamp(0, T)
    x, probs, keep = sample_token_filter(
        logits, ids_buf, lens, temperature, top_k, top_p, repetition_penalty,
        min_length, eos_token_id)
    if greedy:
        pick = x.argmax(dim=-1)
        count = torch.ones(B, dtype=torch.int32, device=x.device)
        mass = torch.zeros(B, dtype=torch.float32, device=x.device)
    else:
        kept = torch.where(keep, probs, torch.zeros_like(probs))
        cum = torch.cumsum(kept, dim=-1)  # inclusive, vocabulary order
        mass = cum[:, -1].clone()
        uu = u.gather(1, L.clamp(max=T - 1)[:, None])[:, 0]
        target = torch.minimum(uu * mass, mass)
        reach = (cum >= target[:, None]) & (cum > 0)
        pick = reach.to(torch.int8).argmax(dim=-1)  # first True
        count = keep.sum(-1).to(torch.int32)
    unf = unfinished.bool()
    tok = torch.where(unf, pick, torch.full_like(pick, pad_token_id))
    slot = L.clamp(max=T - 1)[:, None]
    ids_buf.scatter_(1, slot, torch.where(L < T, tok,
                                          ids_buf.gather(1, slot)[:, 0])[:, None])
    next_tokens.copy_(tok.view_as(next_tokens))
    unfinished.copy_((unf & (tok != eos_token_id)).to(unfinished.dtype))
    return count, mass
