#!/usr/bin/env python3
"""KV-cache decode + top-p sampling benchmark (ms/token over batch 1-16).

Counterpart of the reference's inference latency harness
(ppfleetx projects/gpt/benchmark.py:44-85: batch sweep, ms/batch print).

    python benchmarks/bench_generation.py [--model GPT-1.3B] \
        [--prompt-len 128] [--gen-len 64] \
        [--static-cache [--kv-dtype fp8] [--fused-sampling [--capture]] \
         [--fused-linear [--weight-dtype fp8|mxfp4] [--fused-ln] \
          [--no-wide-linear | --alternate-wide-linear]]]

--no-wide-linear keeps batches of 17 to 64 off csrc/decode_linear_wide.hip
(functional.DECODE_LINEAR_WIDE_MAX_M = 16: the library composition, or the
fp32 twin with fp8 weights); --alternate-wide-linear times both settings in
this process, generation by generation, on two generators over one model.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

SHAPES = {
    "GPT-345M": dict(hidden_size=1024, num_layers=24, num_attention_heads=16),
    "GPT-1.3B": dict(hidden_size=2048, num_layers=24, num_attention_heads=16),
    "GPT-6.7B": dict(hidden_size=4096, num_layers=32, num_attention_heads=32),
}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="GPT-1.3B", choices=sorted(SHAPES))
    p.add_argument("--prompt-len", type=int, default=128)
    p.add_argument("--gen-len", type=int, default=64)
    p.add_argument("--batches", type=str, default="1,2,4,8,16")
    p.add_argument("--top-p", type=float, default=0.9)
    p.add_argument("--static-cache", action="store_true",
                   help="preallocated KV cache + fused decode attention "
                        "(Generation.static_kv_cache)")
    p.add_argument("--kv-dtype", choices=("bf16", "fp8"), default="bf16",
                   help="storage of the static cache "
                        "(Generation.kv_cache_dtype); fp8 needs "
                        "--static-cache")
    p.add_argument("--fused-sampling", action="store_true",
                   help="one sample_token launch per token, no host sync per "
                        "token (Generation.fused_sampling); needs "
                        "--static-cache")
    p.add_argument("--capture", action="store_true",
                   help="replay a captured decode step per token "
                        "(Generation.capture_decode); needs --fused-sampling")
    p.add_argument("--fused-linear", action="store_true",
                   help="decode-step linears and logits through "
                        "ops.decode_linear (Generation.fused_decode_linear); "
                        "needs --static-cache")
    p.add_argument("--weight-dtype", choices=("bf16", "fp8", "mxfp4"),
                   default="bf16",
                   help="storage of the weights the fused decode linears "
                        "stream (Generation.decode_weight_dtype); fp8 and "
                        "mxfp4 need --fused-linear")
    p.add_argument("--fused-ln", action="store_true",
                   help="ln1 / ln2 / final_ln of the decode step inside the "
                        "qkv / ffn_up / logits launches "
                        "(Generation.fused_decode_ln); needs --fused-linear")
    p.add_argument("--no-wide-linear", action="store_true",
                   help="batches of 17 to 64 fall back as they did before "
                        "the wide decode_linear kernel")
    p.add_argument("--alternate-wide-linear", action="store_true",
                   help="time every batch with and without the wide kernel, "
                        "alternating")
    p.add_argument("--alternate-linear-codes", action="store_true",
                   help="time every batch with functional.LINEAR_CODES off "
                        "and on, alternating (batches of 65 and more with "
                        "fp8 or mxfp4 weights: csrc/linear_codes.hip)")
    p.add_argument("--num-return-sequences", type=int, default=1, metavar="G",
                   help="Generation.num_return_sequences: every batch row is "
                        "a prompt that is sampled G times (bs*G rows run)")
    p.add_argument("--shared-prompt", action="store_true",
                   help="time Generation.shared_prompt_cache off against on, "
                        "alternating in one process (needs --static-cache "
                        "--fused-sampling and G >= 2); also prints the time "
                        "of prefill + first token and the cache bytes")
    p.add_argument("--shared-prompt-fp8", action="store_true",
                   help="as --shared-prompt, but both sides share the prompt: "
                        "Generation.shared_prompt_dtype bf16 against fp8")
    p.add_argument("--finish-check-interval", type=int, default=None,
                   help="Generation.finish_check_interval (fused sampling)")
    p.add_argument("--fixed-capacity", action="store_true",
                   help="Generation.kv_cache_capacity = prompt + gen: decode "
                        "attention sizes its split for the capacity at every "
                        "step, as a captured step does")
    args = p.parse_args()
    if args.capture and not args.fused_sampling:
        p.error("--capture needs --fused-sampling")
    if args.fused_sampling and not args.static_cache:
        p.error("--fused-sampling needs --static-cache")
    if args.fused_linear and not args.static_cache:
        p.error("--fused-linear needs --static-cache")
    if args.fused_ln and not args.fused_linear:
        p.error("--fused-ln needs --fused-linear")
    if args.weight_dtype != "bf16" and not args.fused_linear:
        p.error(f"--weight-dtype {args.weight_dtype} needs --fused-linear")

    if args.shared_prompt_fp8:
        if args.shared_prompt:
            p.error("--shared-prompt-fp8 replaces --shared-prompt")
        args.shared_prompt = True
    if args.shared_prompt and (args.alternate_wide_linear
                               or args.alternate_linear_codes):
        p.error("--shared-prompt is an alternation of its own")

    from paddlefleetx_amd.parallel.env import set_hcg
    from paddlefleetx_amd.parallel.topology import HybridTopology
    import torch.distributed as dist
    if not dist.is_initialized():
        set_hcg(HybridTopology())
    from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
    from paddlefleetx_amd.models.gpt.model import GPTModel

    dev = "cuda" if torch.cuda.is_available() else "cpu"
    dtype = torch.bfloat16 if dev == "cuda" else torch.float32
    shape = SHAPES[args.model]
    vocab = 50304
    max_len = args.prompt_len + args.gen_len + 8
    from paddlefleetx_amd.ops import functional
    wide_max = functional.DECODE_LINEAR_WIDE_MAX_M
    # (label, DECODE_LINEAR_WIDE_MAX_M, LINEAR_CODES) of every generator
    # that is timed
    modes = [("", 16 if args.no_wide_linear else wide_max, True)]
    if args.alternate_wide_linear:
        modes = [("no wide ", 16, True), ("wide    ", wide_max, True)]
    if args.alternate_linear_codes:
        modes = [("no codes ", modes[0][1], False),
                 ("codes    ", modes[0][1], True)]
    modes = [m + (False,) for m in modes]
    if args.shared_prompt:
        modes = [("unshared ",) + modes[0][1:3] + (False,),
                 ("shared   ",) + modes[0][1:3] + (True,)]
    if args.shared_prompt_fp8:  # the last field: False, True or "fp8"
        modes = [("shared bf16 ",) + modes[0][1:3] + (True,),
                 ("shared fp8  ",) + modes[0][1:3] + ("fp8",)]
    torch.manual_seed(0)
    with torch.device(dev):
        gpt = GPTModel(vocab_size=vocab, max_position_embeddings=max_len,
                       dtype=dtype, **shape)
        models = [GPTForGeneration(gpt, {
            "max_dec_len": gen_len,
            "num_return_sequences": args.num_return_sequences,
            "shared_prompt_cache": bool(m[3]),
            "shared_prompt_dtype": "fp8" if m[3] == "fp8" else "bf16",
            "decoding_strategy": "sampling",
            "top_p": args.top_p,
            "use_topp_sampling": True,
            "eos_token_id": vocab - 1,
            "static_kv_cache": args.static_cache,
            "kv_cache_dtype": args.kv_dtype,
            "fused_sampling": args.fused_sampling,
            "capture_decode": args.capture,
            "fused_decode_linear": args.fused_linear,
            "decode_weight_dtype": args.weight_dtype,
            "fused_decode_ln": args.fused_ln,
            **({"finish_check_interval": args.finish_check_interval}
               if args.finish_check_interval else {}),
            **({"kv_cache_capacity": args.prompt_len + args.gen_len}
               if args.fixed_capacity else {}),
        }).eval() for m in modes
            for gen_len in ((args.gen_len, 1) if args.shared_prompt
                            else (args.gen_len,))]
    # with --shared-prompt every mode also has a max_dec_len = 1 twin: its
    # call is the prefill plus the first token
    stride = 2 if args.shared_prompt else 1

    print(f"# decode bench {args.model} prompt={args.prompt_len} "
          f"gen={args.gen_len} top_p={args.top_p} "
          f"static_cache={args.static_cache} kv_dtype={args.kv_dtype} "
          f"fused_sampling={args.fused_sampling} capture={args.capture} "
          f"fused_linear={args.fused_linear} "
          f"weight_dtype={args.weight_dtype} fused_ln={args.fused_ln} "
          f"wide_linear={[m[1] for m in modes]} "
          f"linear_codes={[m[2] for m in modes]} ({dev})")

    def generate(i, ids):
        # a captured step keeps the path of the call that captured it
        functional.DECODE_LINEAR_WIDE_MAX_M = modes[i][1]
        functional.LINEAR_CODES = modes[i][2]
        out = models[i * stride](ids)
        if dev == "cuda":
            torch.cuda.synchronize()
        return out

    def prefill_ms(i, ids):
        ts = []
        for _ in range(4):  # the first call warms up
            t0 = time.time()
            models[i * stride + 1](ids)
            if dev == "cuda":
                torch.cuda.synchronize()
            ts.append((time.time() - t0) * 1000.0)
        return statistics.median(ts[1:])

    for bs in [int(b) for b in args.batches.split(",")]:
        ids = torch.randint(0, vocab - 2, (bs, args.prompt_len), device=dev)
        reps = 3
        dts = [[] for _ in modes]
        with torch.no_grad():
            for i in range(len(modes)):
                generate(i, ids)  # warmup (compile caches, allocator)
            for _ in range(reps):
                for i in range(len(modes)):
                    t0 = time.time()
                    out = generate(i, ids)
                    dts[i].append(time.time() - t0)
        for i, ((label, _, _, _), t) in enumerate(zip(modes, dts)):
            dt = statistics.median(t) if len(modes) > 1 else sum(t) / reps
            # GPTForGeneration returns only the GENERATED ids
            ntok = out.shape[1] if out.shape[1] <= args.gen_len \
                else out.shape[1] - args.prompt_len
            ms_tok = dt * 1000.0 / max(1, ntok)
            rows = bs * out.shape[0] // ids.shape[0]
            extra = ""
            if args.shared_prompt:
                with torch.no_grad():
                    extra = f"  prefill+1 {prefill_ms(i, ids):.1f} ms"
                st = models[i * stride]._graph_state
                if st is not None:
                    extra += f"  cache {st['cache'].nbytes / 2**20:.1f} MiB"
            print(f"{label}bs={bs:3d}: {dt*1000:8.1f} ms/gen ({ntok} new "
                  f"tok) = {ms_tok:7.2f} ms/token, {rows*ntok/dt:8.0f} tok/s"
                  + (f"  (min/max {min(t)*1000:.1f}/{max(t)*1000:.1f} ms)"
                     if len(modes) > 1 else "") + extra, flush=True)


if __name__ == "__main__":
    main()
