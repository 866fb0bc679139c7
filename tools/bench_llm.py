"""Greedy generation of the language model: the stock path (`walkgptForCausalLM._generate` with the switch off: one transformers forward per
token) against the HIP LLaMA path (walkgpt_amd/llama_hip.py), eager and graphed, in one process on one GPU.

Default shape: a random-init bf16 LLaMA-7B (32 layers, 4096 hidden, 11008 intermediate, 32 heads; 13.5 GB), rows 1, L0 = 320 (64 text + 256 image
positions), 128 new tokens, no eos.  Per path the median of `--runs` runs of: the prefill alone, the whole generation, and from the two the decode
time per token, (generation - prefill) / (new - 1).  Also: the weight bytes a decode step streams / its time, as a share of the 6.29 TB/s copy rate
measured on an MI355X.  Prints one JSON line; results belong in profiles/llm_generate.md.

    python tools/bench_llm.py [--layers 32] [--rows 1] [--l0 320] [--new 128] [--runs 5] [--one-step] [--lora q_proj,v_proj --lora-r 8 --lora-alpha 16]
                              [--weights e4m3]
--one-step: no timing; after a warm generation, replay ONE graphed decode step (for `rocprofv3 --kernel-trace --stats -- python tools/bench_llm.py
--one-step`, whose per-kernel table then holds that step on top of the warm-up).
--lora: unmerged LoRA adapters.  The plain model is measured first (graphed HIP path), then stand-in adapters (tests/lora_reference.py's
LoraLinear, the attributes of PEFT's layer; random A and random non-zero B) go onto the named projections of every layer and the same process
measures the graphed HIP path and the stock path on the adapted model, and last the graphed HIP path with every adapter disabled (the plain
path again, as a control for drift inside the process).  "lora" in the JSON line: prefill ms and decode ms/token of the four, each with the
lowest and highest of its runs.  The stand-in layer comes from tests/lora_reference.py, so --lora needs the checkout's tests/ directory.  With --one-step the replayed step is the adapted model's.
--weights e4m3: the e4m3 weight-only decode (LlamaHipRunner(llm, weights="e4m3")) against the bf16 path in one process: the bf16 graphed path is
measured first, then the e4m3 graphed path on the same model (with --lora: on the same adapted model).  "weights" in the JSON line: prefill ms
and decode ms/token of the two (median, lowest, highest of the runs), the bytes a decode step streams in each mode and their rate, the time the
store took to build, and the share of the generated tokens on which the two modes agree.  With --one-step the replayed step is the e4m3 one."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12      # bytes / s, the measured device-to-device copy rate of an MI355X


def build(layers, dev):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=layers, num_attention_heads=32,
                      num_key_value_heads=32, max_position_embeddings=2048)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)      # as causal_lm._build_language_model: a 7B random init in fp32 would need 27 GB
    try:
        with torch.device(dev):
            llm = LlamaForCausalLM(cfg)
    finally:
        torch.set_default_dtype(prev)
    return llm.eval()


def timed_all(fn, runs):
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def timed(fn, runs):
    return statistics.median(timed_all(fn, runs))


def measure(prefill, generate, runs, new):
    """-> (tokens of the warm-up generation, {prefill_ms, decode_ms_per_token: median, lowest, highest of the runs}); a run's decode time per
    token is (its generation - the median prefill) / (new - 1)"""
    prefill()
    tokens = generate()[0]                         # warm-up (and, for the graphed path, the capture)
    p, t = timed_all(prefill, runs), timed_all(generate, runs)
    pm = statistics.median(p)
    d = [(x - pm) / max(1, new - 1) for x in t]
    stat = lambda v, nd: {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}
    return tokens, {"prefill_ms": stat(p, 3), "decode_ms_per_token": stat(d, 4)}


def add_adapters(llm, targets, r, alpha):
    """Stand-in adapters from the test suite's LoraLinear (peft is not needed): A and B ~ N(0, 0.02), seed 11."""
    try:
        from tests import lora_reference as lo
    except ImportError as e:
        raise SystemExit("--lora takes its stand-in LoRA layer from tests/lora_reference.py: run from a checkout that has tests/ (%s)" % e)
    return lo.inject_lora(llm, targets, r, alpha, 11, 0.02, 0.02)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rows", type=int, default=1)
    ap.add_argument("--l0", type=int, default=320)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--one-step", action="store_true")
    ap.add_argument("--lora", default="", help="comma-separated projections that get a stand-in adapter, e.g. q_proj,v_proj")
    ap.add_argument("--lora-r", type=int, default=8)
    ap.add_argument("--lora-alpha", type=float, default=16)
    ap.add_argument("--weights", default="bf16", choices=("bf16", "e4m3"), help="e4m3: measure the e4m3 weight-only decode against the bf16 path")
    a = ap.parse_args()
    targets = tuple(n for n in a.lora.split(",") if n)
    from walkgpt_amd.causal_lm import walkgptForCausalLM
    from walkgpt_amd.llama_hip import LlamaHipRunner
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    llm = build(a.layers, dev)
    g = torch.Generator().manual_seed(1)
    emb = llm.get_input_embeddings().weight[torch.randint(0, 32000, (a.rows, a.l0), generator=g).to(dev)]
    mask = torch.ones(a.rows, a.l0, dtype=torch.bool, device=dev)
    runner = LlamaHipRunner(llm)
    # _generate as the model runs it, without the grounding modules around it: `self` only has to carry what _generate reads
    stock = SimpleNamespace(llm=llm, eos_token_id=None, config=SimpleNamespace(pad_token_id=None), _hip_llm=None)
    with torch.no_grad():
        if a.weights == "e4m3":
            del runner
            if targets:
                add_adapters(llm, targets, a.lora_r, a.lora_alpha)
            if a.one_step:
                runner = LlamaHipRunner(llm, weights="e4m3")
                runner.generate(emb, mask, 4)
                torch.cuda.synchronize()
                runner._graph[0].replay()
                torch.cuda.synchronize()
                return
            res = {"layers": a.layers, "rows": a.rows, "l0": a.l0, "new": a.new, "runs": a.runs, "weights": {}}
            if targets:
                res["lora"] = {"targets": list(targets), "r": a.lora_r, "alpha": a.lora_alpha}
            hip = lambda r: (lambda: r.prefill(emb, mask), lambda: r.generate(emb, mask, a.new, graph=True))
            w = res["weights"]
            runner = LlamaHipRunner(llm)
            tok16, w["bf16"] = measure(*hip(runner), a.runs, a.new)
            proj = [t for lw in runner._layers() for t in lw[1:5] + lw[6:9]]
            head = llm.lm_head.weight.numel() * 2
            del runner                                 # its KV cache and graph go before the next runner's come
            runner = LlamaHipRunner(llm, weights="e4m3")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner._refresh_store()
            torch.cuda.synchronize()
            w["store_build_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            tok8, w["e4m3"] = measure(*hip(runner), a.runs, a.new)
            w["store_bytes"] = sum(q.numel() + s.numel() * 4 for q, s in (runner._store[t] for t in proj))
            med = lambda k, what: w[k][what]["median"]
            for k, b in (("bf16", sum(t.numel() * 2 for t in proj) + head), ("e4m3", w["store_bytes"] + head)):
                w[k]["weight_bytes_per_token"] = b
                w[k]["share_of_copy_rate"] = round(b / (med(k, "decode_ms_per_token") * 1e-3) / COPY_RATE, 4)
            w["e4m3_vs_bf16_decode"] = round(med("e4m3", "decode_ms_per_token") / med("bf16", "decode_ms_per_token"), 4)
            w["e4m3_vs_bf16_prefill"] = round(med("e4m3", "prefill_ms") / med("bf16", "prefill_ms"), 4)
            w["tokens_agreeing_with_bf16"] = round(float((tok8 == tok16).float().mean()), 3)
            print(json.dumps(res))
            return
        if a.one_step:
            if targets:
                runner = LlamaHipRunner(add_adapters(llm, targets, a.lora_r, a.lora_alpha))
            runner.generate(emb, mask, 4)
            torch.cuda.synchronize()
            runner._graph[0].replay()
            torch.cuda.synchronize()
            return
        if targets:
            res = {"layers": a.layers, "rows": a.rows, "l0": a.l0, "new": a.new, "runs": a.runs,
                   "lora": {"targets": list(targets), "r": a.lora_r, "alpha": a.lora_alpha}}
            hip = lambda r: (lambda: r.prefill(emb, mask), lambda: r.generate(emb, mask, a.new, graph=True))
            plain_tokens, res["lora"]["hip_graph_plain"] = measure(*hip(runner), a.runs, a.new)
            del runner
            add_adapters(llm, targets, a.lora_r, a.lora_alpha)
            runner = LlamaHipRunner(llm)
            tok, res["lora"]["hip_graph_adapted"] = measure(*hip(runner), a.runs, a.new)
            tok_s, res["lora"]["stock_adapted"] = measure(lambda: llm(inputs_embeds=emb, attention_mask=mask, use_cache=True, output_hidden_states=True),
                                                          lambda: walkgptForCausalLM._generate(stock, emb, mask, a.new), a.runs, a.new)
            for m in llm.modules():
                if hasattr(m, "lora_A"):
                    m.disable_adapters = True
            _, res["lora"]["hip_graph_disabled"] = measure(*hip(runner), a.runs, a.new)
            med = lambda k: res["lora"][k]["decode_ms_per_token"]["median"]
            res["lora"]["adapted_vs_plain_decode"] = round(med("hip_graph_adapted") / med("hip_graph_plain"), 4)
            res["lora"]["hip_graph_vs_stock_decode"] = round(med("stock_adapted") / med("hip_graph_adapted"), 3)
            res["lora"]["tokens_agreeing_with_stock"] = round(float((tok == tok_s).float().mean()), 3)
            res["lora"]["tokens_changed_by_the_adapters"] = round(float((tok != plain_tokens).float().mean()), 3)
            print(json.dumps(res))
            return
        paths = {
            "stock": (lambda: llm(inputs_embeds=emb, attention_mask=mask, use_cache=True, output_hidden_states=True),
                      lambda: walkgptForCausalLM._generate(stock, emb, mask, a.new)),
            "hip_eager": (lambda: runner.prefill(emb, mask), lambda: runner.generate(emb, mask, a.new, graph=False)),
            "hip_graph": (lambda: runner.prefill(emb, mask), lambda: runner.generate(emb, mask, a.new, graph=True)),
        }
        res = {"layers": a.layers, "rows": a.rows, "l0": a.l0, "new": a.new, "runs": a.runs}
        tokens = {}
        for name, (prefill, generate) in paths.items():
            prefill()
            tokens[name] = generate()[0]               # warm-up (and, for the graphed path, the capture)
            p, t = timed(prefill, a.runs), timed(generate, a.runs)
            res[name] = {"prefill_ms": round(p, 3), "generate_ms": round(t, 3), "decode_ms_per_token": round((t - p) / max(1, a.new - 1), 4)}
        w = sum(t.numel() * 2 for lw in runner._layers() for t in lw[:9] if t.dim() == 2) + llm.lm_head.weight.numel() * 2
        d = res["hip_graph"]["decode_ms_per_token"] * 1e-3
        res["weight_bytes_per_token"] = w
        res["hip_graph_share_of_copy_rate"] = round(w / d / COPY_RATE, 4)
        res["hip_graph_vs_stock_decode"] = round(res["stock"]["decode_ms_per_token"] / res["hip_graph"]["decode_ms_per_token"], 3)
        res["tokens_equal_eager_graph"] = bool(tokens["hip_eager"].equal(tokens["hip_graph"]))
        res["tokens_agreeing_with_stock"] = round(float((tokens["hip_graph"] == tokens["stock"]).float().mean()), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
