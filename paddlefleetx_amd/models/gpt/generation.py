"""GPT text generation: KV-cache decode loop + top-k/top-p sampling.

Reference: ppfleetx/models/language_model/gpt/dygraph/single_model.py
  GPTForGeneration :898 (sample :1139, TopKProcess :1150, TopPProcess :1158,
  custom top-p op hook :1240-1252, greedy/sampling dispatch forward :1322-1418)
and the hybrid twin hybrid_model.py:1209.

MI355X-native notes: the decode loop runs the same GPTModel with per-layer
KV caches ([B, H, S, D] tensors grown by concat, or with `static_kv_cache`
one preallocated StaticKVCache appended in place by the fused decode
attention kernel, csrc/decode_attention.hip; `kv_cache_dtype: fp8` stores
that cache as e4m3 codes with a per-row scale, csrc/decode_attention_fp8.hip);
sampling post-processing
uses the hand-written gfx950 top-p kernel (csrc/topp.hip) when
`use_topp_sampling` is on, replacing the reference's CUB-based
ppfleetx/ops/topp_sampling.cu.

`fused_sampling: true` (needs the static cache) replaces the whole sampling
tail by ONE launch per token (csrc/sample_token.hip) that also keeps the
generation state on the device, so the loop has no host synchronisation
per token; `capture_decode: true` on top of it records one decode step
(forward + sampler) as a graph and replays it once per token.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from paddlefleetx_amd.models.gpt.model import (DecodeWeightCodes, GPTModel,
                                              StaticKVCache)
from paddlefleetx_amd.models.gpt.processor import get_logits_processor
from paddlefleetx_amd.ops import decode_linear, sample_token, topp_sampling
from paddlefleetx_amd.parallel.env import get_hcg
from paddlefleetx_amd.parallel.tp import parallel_matmul
from paddlefleetx_amd.utils.log import logger


def TopKProcess(probs: torch.Tensor, top_k: int, min_tokens_to_keep: int = 1
                ) -> torch.Tensor:
    """Zero all probability mass outside the top-k (single_model.py:1150-1156)."""
    top_k = min(max(top_k, min_tokens_to_keep), probs.shape[-1])
    topk_probs, _ = torch.topk(probs, k=top_k, dim=-1)
    kth = topk_probs[:, -1:].expand_as(probs)
    return torch.where(probs >= kth, probs, torch.zeros_like(probs))


def TopPProcess(probs: torch.Tensor, top_p: float, min_tokens_to_keep: int = 1
                ) -> torch.Tensor:
    """Nucleus filtering on the host graph (single_model.py:1158-1185)."""
    sorted_probs, sorted_indices = torch.sort(probs, descending=True, dim=-1)
    cumulative = torch.cumsum(sorted_probs, dim=-1)
    # remove tokens with cumulative prob above top_p, keeping at least one
    sorted_to_remove = cumulative > top_p
    sorted_to_remove[:, 0] = False
    if min_tokens_to_keep > 1:
        sorted_to_remove[:, :min_tokens_to_keep] = False
    # shift right: the first token crossing the threshold stays
    sorted_to_remove[:, 1:] = sorted_to_remove[:, :-1].clone()
    sorted_to_remove[:, 0] = False
    to_remove = sorted_to_remove.scatter(1, sorted_indices, sorted_to_remove)
    return probs.masked_fill(to_remove, 0.0)


class GPTForGeneration(nn.Module):
    """Decode-loop wrapper over GPTModel (single_model.py:898-1418)."""

    def __init__(self, gpt: GPTModel, configs: Optional[dict] = None):
        super().__init__()
        self.gpt = gpt
        cfg = configs or {}
        self.max_length = int(cfg.get("max_dec_len", 20))
        self.min_length = int(cfg.get("min_dec_len", 0))
        self.decode_strategy = cfg.get("decoding_strategy", "sampling")
        self.temperature = float(cfg.get("temperature", 1.0))
        self.top_k = int(cfg.get("top_k", 0))
        self.top_p = float(cfg.get("top_p", 1.0))
        self.repetition_penalty = float(cfg.get("repetition_penalty", 1.0))
        self.use_topp_sampling = bool(cfg.get("use_topp_sampling", False))
        self.eos_token_id = int(cfg.get("eos_token_id", 50256))
        self.pad_token_id = int(cfg.get("pad_token_id", 0))
        self.num_return_sequences = int(cfg.get("num_return_sequences", 1))
        self.static_kv_cache = bool(cfg.get("static_kv_cache", False))
        # storage of the static cache: "bf16" (the model dtype) or "fp8"
        # (e4m3 codes + one fp32 scale per cached row)
        self.kv_cache_dtype = str(cfg.get("kv_cache_dtype") or "bf16")
        if self.kv_cache_dtype not in ("bf16", "fp8"):
            raise ValueError(
                "Generation.kv_cache_dtype must be 'bf16' or 'fp8', got "
                f"{self.kv_cache_dtype!r}")
        if self.kv_cache_dtype == "fp8" and not self.static_kv_cache:
            raise ValueError(
                "Generation.kv_cache_dtype: fp8 needs static_kv_cache: true "
                "(the tuple cache has no fp8 mode)")
        # one sample_token launch per token, state on the device
        self.fused_sampling = bool(cfg.get("fused_sampling", False))
        if self.fused_sampling and not self.static_kv_cache:
            raise ValueError(
                "Generation.fused_sampling: true needs static_kv_cache: true "
                "(the sampler reads the static cache's device lens)")
        # the all-finished test (the loop's only host sync) runs every this
        # many tokens; the result is trimmed to what a per-token test gives
        self.finish_check_interval = int(cfg.get("finish_check_interval", 4))
        if self.finish_check_interval < 1:
            raise ValueError(
                "Generation.finish_check_interval must be >= 1, got "
                f"{self.finish_check_interval}")
        # optional fixed capacity of the static cache (default: prompt +
        # max_dec_len per call). When set, decode attention sizes its KV
        # split for this capacity at every step, so an eager and a captured
        # run make the same split choice.
        cap = cfg.get("kv_cache_capacity")
        self.kv_cache_capacity = int(cap) if cap else None
        # replay one captured decode step per token (see _sample_captured)
        self.capture_decode = bool(cfg.get("capture_decode", False))
        self._capture_warned = False
        if self.capture_decode and not self.fused_sampling:
            logger.warning("Generation.capture_decode needs fused_sampling: "
                           "true: staying eager")
            self.capture_decode = False
        self._graph_state = None
        # every linear of a static-cache decode step (and the logits of the
        # fused-sampling step) as one ops.decode_linear launch
        self.fused_decode_linear = bool(cfg.get("fused_decode_linear", False))
        if self.fused_decode_linear and not self.static_kv_cache:
            raise ValueError(
                "Generation.fused_decode_linear: true needs static_kv_cache: "
                "true (the fused layer runs against a static cache slot)")
        if self.fused_decode_linear and \
                get_hcg().get_model_parallel_world_size() != 1:
            logger.warning("Generation.fused_decode_linear needs "
                           "model-parallel size 1: staying on the existing "
                           "path")
            self.fused_decode_linear = False
        # storage of the weights a fused decode step streams: "bf16" (the
        # parameters) or "fp8" (e4m3 codes + one fp32 scale per output row,
        # quantised once, kept NEXT TO the bf16 parameters)
        self.decode_weight_dtype = str(cfg.get("decode_weight_dtype")
                                       or "bf16")
        if self.decode_weight_dtype not in ("bf16", "fp8"):
            raise ValueError(
                "Generation.decode_weight_dtype must be 'bf16' or 'fp8', got "
                f"{self.decode_weight_dtype!r}")
        if self.decode_weight_dtype == "fp8" and \
                not cfg.get("fused_decode_linear", False):
            raise ValueError(
                "Generation.decode_weight_dtype: fp8 needs "
                "fused_decode_linear: true (only ops.decode_linear reads "
                "fp8 weights)")
        if self.decode_weight_dtype == "fp8" and not self.fused_decode_linear:
            logger.warning("Generation.decode_weight_dtype: fp8 needs "
                           "model-parallel size 1: staying on bf16 weights")
            self.decode_weight_dtype = "bf16"
        # a plain attribute, not a submodule: no state_dict entry, no cast
        self._weight_codes = DecodeWeightCodes() \
            if self.decode_weight_dtype == "fp8" else None

    def _decode_weights(self):
        """The weights a fused decode step streams: four linears per decoder
        layer and the tied embedding."""
        ws = []
        for layer in self.gpt.layers:
            if not hasattr(layer.ffn, "up_bias"):
                continue  # an expert layer never takes the fused path
            ws += [layer.attn.qkv.weight, layer.attn.out_proj.weight,
                   layer.ffn.up.weight, layer.ffn.down.weight]
        ws.append(self.gpt.embeddings.word_embeddings.weight)
        return ws

    def _refresh_weight_codes(self) -> None:
        """Quantise what is new or was changed since the last call (a no-op
        otherwise); outside any captured region."""
        if self._weight_codes is not None:
            self._weight_codes.refresh(self._decode_weights())

    # -- one forward --------------------------------------------------------
    def _logits(self, input_ids, position_ids, caches):
        hidden, new_caches = self.gpt(input_ids, position_ids, caches=caches,
                                      use_cache=True)
        logits = parallel_matmul(
            hidden[:, -1, :], self.gpt.embeddings.word_embeddings.weight,
            parallel_output=False)
        return logits.float(), new_caches

    def _new_static_cache(self, batch_size: int, max_len: int, device,
                          max_seq_len: Optional[int] = None) -> StaticKVCache:
        attn = self.gpt.layers[0].attn
        return StaticKVCache(len(self.gpt.layers), batch_size,
                             attn.num_heads_local, max_len, attn.head_dim,
                             dtype=attn.qkv.weight.dtype, device=device,
                             kv_dtype=self.kv_cache_dtype,
                             max_seq_len=max_seq_len,
                             fused_decode_linear=self.fused_decode_linear,
                             weight_codes=self._weight_codes)

    # -- fused sampling -----------------------------------------------------
    def _capacity(self, prompt_len: int) -> int:
        need = prompt_len + self.max_length
        if self.kv_cache_capacity is None:
            return need
        if self.kv_cache_capacity < need:
            raise ValueError(
                f"Generation.kv_cache_capacity {self.kv_cache_capacity} < "
                f"prompt {prompt_len} + max_dec_len {self.max_length}")
        return self.kv_cache_capacity

    def _sampler_args(self, prompt_len: int) -> dict:
        return dict(greedy=self.decode_strategy == "greedy_search",
                    temperature=self.temperature, top_k=self.top_k,
                    top_p=self.top_p,
                    repetition_penalty=self.repetition_penalty,
                    min_length=(prompt_len + self.min_length
                                if self.min_length > 0 else 0),
                    eos_token_id=self.eos_token_id,
                    pad_token_id=self.pad_token_id)

    def _decode_step(self, st: dict, kw: dict) -> None:
        """One decode step on device state only: forward of next_tokens at
        position lens (which advances lens), logits, sample_token."""
        cache = st["cache"]
        pos = cache.lens.long().unsqueeze(1)
        hidden, _ = self.gpt(st["next_tokens"], pos, caches=cache,
                             use_cache=True)
        if self.fused_decode_linear:
            w, s = self.gpt.embeddings.word_embeddings.weight, None
            if self._weight_codes is not None:
                w, s = self._weight_codes.get(w)
            logits = decode_linear(hidden[:, -1, :], w, weight_scale=s)
        else:
            logits = parallel_matmul(
                hidden[:, -1, :], self.gpt.embeddings.word_embeddings.weight,
                parallel_output=False)
        sample_token(logits, st["ids_buf"], cache.lens, st["unfinished"],
                     st["u"], st["next_tokens"], **kw)

    def _new_state(self, B: int, capacity: int, device, fixed: bool) -> dict:
        return dict(
            cache=self._new_static_cache(
                B, capacity, device, max_seq_len=capacity if fixed else None),
            ids_buf=torch.empty(B, capacity, dtype=torch.long, device=device),
            unfinished=torch.empty(B, dtype=torch.bool, device=device),
            next_tokens=torch.empty(B, 1, dtype=torch.long, device=device),
            u=torch.zeros(B, capacity, dtype=torch.float32, device=device))

    def _start(self, st: dict, input_ids: torch.Tensor, kw: dict) -> None:
        """Reset the state, prefill eagerly and sample the first token."""
        B, prompt_len = input_ids.shape
        n = prompt_len + self.max_length
        self._refresh_weight_codes()
        cache = st["cache"]
        cache.lens.zero_()
        cache.max_len = 0
        st["ids_buf"].fill_(self.pad_token_id)
        st["ids_buf"][:, :prompt_len] = input_ids
        st["unfinished"].fill_(True)
        # the only RNG use of a call: seeding reproduces a run, and the draw
        # does not depend on the capacity of the buffers
        st["u"][:, :n] = torch.rand(B, n, device=input_ids.device)
        position_ids = torch.arange(prompt_len, device=input_ids.device) \
            .unsqueeze(0).expand(B, -1)
        hidden, _ = self.gpt(input_ids, position_ids, caches=cache,
                             use_cache=True)
        logits = parallel_matmul(
            hidden[:, -1, :], self.gpt.embeddings.word_embeddings.weight,
            parallel_output=False)
        sample_token(logits, st["ids_buf"], cache.lens, st["unfinished"],
                     st["u"], st["next_tokens"], **kw)

    def _trim(self, st: dict, prompt_len: int, n_done: int) -> torch.Tensor:
        """What the per-token loop returns: it stops at the step where the
        last row finishes; rows that finished earlier are padded."""
        out = st["ids_buf"][:, prompt_len:prompt_len + n_done]
        is_eos = out == self.eos_token_id
        # step at which each row finished (its first eos), n_done if never
        first = torch.where(is_eos.any(-1),
                            is_eos.to(torch.int8).argmax(-1) + 1,
                            torch.full((out.shape[0],), n_done,
                                       device=out.device))
        return out[:, :int(first.max())].clone()

    def _sample_fused(self, input_ids: torch.Tensor,
                      return_state: bool = False):
        """The loop of sample() with the tail fused into sample_token and no
        host synchronisation per token. return_state also hands back the
        device state (cache, ids_buf, ...) the call ended with."""
        B, prompt_len = input_ids.shape
        kw = self._sampler_args(prompt_len)
        if self._use_capture(input_ids):
            out = self._sample_captured(input_ids, kw)
            return (out, self._graph_state) if return_state else out
        st = self._new_state(B, self._capacity(prompt_len), input_ids.device,
                             fixed=self.kv_cache_capacity is not None)
        self._start(st, input_ids, kw)
        n_done = 1
        while n_done < self.max_length:
            if n_done % self.finish_check_interval == 0 and \
                    not st["unfinished"].any():
                break
            self._decode_step(st, kw)
            n_done += 1
        out = self._trim(st, prompt_len, n_done)
        return (out, st) if return_state else out

    # -- captured decode step -------------------------------------------------
    def _use_capture(self, input_ids: torch.Tensor) -> bool:
        if not self.capture_decode:
            return False
        why = None
        if input_ids.device.type != "cuda":
            why = "needs a CUDA device"
        elif get_hcg().get_model_parallel_world_size() != 1:
            why = "needs model-parallel size 1"
        if why is not None:
            if not self._capture_warned:
                logger.warning(
                    f"Generation.capture_decode {why}: staying eager")
                self._capture_warned = True
            return False
        return True

    def _build_graph(self, B: int, capacity: int, device, kw: dict) -> dict:
        """Allocate the fixed-address state and record ONE decode step on one
        stream (no parallel branches). The graph bakes in the sampler
        scalars, so they are part of the reuse key."""
        st = self._new_state(B, capacity, device, fixed=True)
        cache = st["cache"]
        self._refresh_weight_codes()  # never inside the captured region

        def reset():
            cache.lens.zero_()
            cache.max_len = 0
            st["ids_buf"].fill_(self.pad_token_id)
            st["unfinished"].fill_(True)
            st["next_tokens"].zero_()

        reset()
        # eager warm-up against the empty cache (L = 0 is a valid shape):
        # library handles, workspaces and the allocator settle before capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._decode_step(st, kw)
        torch.cuda.current_stream().wait_stream(side)
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._decode_step(st, kw)
        reset()
        st.update(graph=graph, key=(B, tuple(sorted(kw.items()))))
        logger.info(f"decode step captured (B={B}, capacity={capacity})")
        return st

    def _sample_captured(self, input_ids: torch.Tensor, kw: dict
                         ) -> torch.Tensor:
        B, prompt_len = input_ids.shape
        capacity = self._capacity(prompt_len)
        # min_length moves with the prompt length and is baked into the graph
        key = (B, tuple(sorted(kw.items())))
        st = self._graph_state
        if st is None or st["key"] != key or \
                st["cache"].capacity < capacity:
            self._graph_state = None  # free the old buffers first
            st = self._graph_state = self._build_graph(
                B, capacity, input_ids.device, kw)
        cache = st["cache"]
        self._start(st, input_ids, kw)
        n_done = 1
        while n_done < self.max_length:
            if n_done % self.finish_check_interval == 0 and \
                    not st["unfinished"].any():
                break
            # the recorded advance moves only the device lens
            assert cache.max_len + 1 <= cache.capacity, \
                f"StaticKVCache overflow: {cache.max_len}+1 > {cache.capacity}"
            st["graph"].replay()
            cache.max_len += 1
            n_done += 1
        return self._trim(st, prompt_len, n_done)

    def sample(self, input_ids: torch.Tensor,
               logits_processors=None) -> torch.Tensor:
        """Autoregressive sampling loop (single_model.py:1139-1320)."""
        if self.fused_sampling:
            if logits_processors is not None:
                raise ValueError(
                    "Generation.fused_sampling does not support user-supplied "
                    "logits_processors (the fused sampler applies min length "
                    "and the repetition penalty itself)")
            return self._sample_fused(input_ids)
        B, prompt_len = input_ids.shape
        device = input_ids.device
        processors = logits_processors if logits_processors is not None else \
            get_logits_processor(
                min_length=prompt_len + self.min_length,
                eos_token_id=self.eos_token_id,
                repetition_penalty=self.repetition_penalty)

        position_ids = torch.arange(prompt_len, device=device).unsqueeze(0) \
            .expand(B, -1)
        # prefill: full prompt builds the KV cache (single_model.py:1285)
        caches = None
        if self.static_kv_cache:
            # one fixed-address cache per call, filled in place
            caches = self._new_static_cache(
                B, prompt_len + self.max_length, device)
        logits, caches = self._logits(input_ids, position_ids, caches)

        unfinished = torch.ones(B, dtype=torch.bool, device=device)
        all_ids = input_ids
        cur_len = prompt_len
        while cur_len < prompt_len + self.max_length:
            logits = processors(all_ids, logits)
            if self.decode_strategy == "greedy_search":
                next_tokens = logits.argmax(dim=-1, keepdim=True)
            else:
                if self.temperature != 1.0:
                    logits = logits / self.temperature
                probs = F.softmax(logits, dim=-1)
                if self.top_k > 0:
                    probs = TopKProcess(probs, self.top_k)
                if self.use_topp_sampling and self.top_p < 1.0:
                    tp = torch.full((B,), self.top_p, device=device)
                    next_tokens, _ = topp_sampling(probs, tp)
                else:
                    if self.top_p < 1.0:
                        probs = TopPProcess(probs, self.top_p)
                    next_tokens = torch.multinomial(probs, num_samples=1)
            next_tokens = torch.where(
                unfinished.unsqueeze(1), next_tokens,
                torch.full_like(next_tokens, self.pad_token_id))
            all_ids = torch.cat([all_ids, next_tokens], dim=-1)
            unfinished = unfinished & (next_tokens.squeeze(1) != self.eos_token_id)
            cur_len += 1
            if not unfinished.any():
                break
            pos = torch.full((B, 1), cur_len - 1, device=device,
                             dtype=torch.long)
            logits, caches = self._logits(next_tokens, pos, caches)
        return all_ids[:, prompt_len:]

    def forward(self, input_ids: torch.Tensor) -> torch.Tensor:
        was_training = self.gpt.training
        self.gpt.eval()
        with torch.no_grad():
            if self.decode_strategy == "sampling" and \
                    self.num_return_sequences > 1:
                # expand_inputs_for_generation (single_model.py:1408-1412):
                # each prompt row is repeated n times, so the output is
                # [B*n, max_dec_len] grouped by prompt
                input_ids = input_ids.repeat_interleave(
                    self.num_return_sequences, dim=0)
            out = self.sample(input_ids)
        if was_training:
            self.gpt.train()
        return out
