"""generate() wall time with the top rows of the image given: the stepwise form against the prefix fast path.
    python tools/given_bench.py [--reps 7] [--out given_bench.json]       forms (b) and (c), alternating in one process
    python tools/given_bench.py --plain [--reps 7] [--out ...]            form (a): a full generate() with nothing given

GPT-L shape (24 layers, d 1024), bf16, batch 32, cfg 4.0 (64 rows), N = 576 tokens (384 px), top-k 2000; the top 12 of the 24 token
rows are given (P = 288, random token ids: timing does not depend on them).  Each call is bracketed by HIP events on the launch
stream after `--warmup` calls of its form (graph captured, weights packed); medians, minima and maxima in ms.  --plain uses nothing
this feature added, so the same file measures a checkout without it (form (a) and its own spread: the yardstick for "(c) beats
(b)").  Writes JSON (committed under profiles/)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llamagen_amd import GPT_models, generate  # noqa: E402

B, N, P, V = 32, 576, 288, 16384
SKW = dict(cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=2000, top_p=1.0, sample_logits=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plain", action="store_true", help="form (a): nothing given")
    ap.add_argument("--out", type=str, default="given_bench.json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = GPT_models["GPT-L"](vocab_size=V, block_size=N, num_classes=1000, cls_token_num=1, model_type="c2i")
    torch.nn.init.normal_(m.output.weight, 0, 0.02)   # zero-initialised in the reference (gpt.py:305): constant rows are not the workload
    m = m.to(device=dev, dtype=torch.bfloat16).eval()
    g = torch.Generator().manual_seed(1)
    cond = torch.randint(0, 1000, (B,), generator=g).to(dev)
    given = torch.full((B, N), -1, dtype=torch.int32)
    given[:, :P] = torch.randint(0, V, (B, P), generator=g, dtype=torch.int32)
    forms = {"a_plain": {}} if a.plain else {"b_stepwise": dict(given=given, _given_stepwise=True), "c_fast_path": dict(given=given)}

    def timed(kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ids = generate(m, cond, N, **SKW, **kw)
        e1.record()
        torch.cuda.synchronize()
        assert tuple(ids.shape) == (B, N)
        return e0.elapsed_time(e1)
    for kw in forms.values():
        for _ in range(a.warmup):
            timed(kw)
    times = {k: [] for k in forms}
    for _ in range(a.reps):          # the forms alternate
        for k, kw in forms.items():
            times[k].append(timed(kw))
    res = dict(model="GPT-L", dtype="bf16", batch=B, cfg_scale=SKW["cfg_scale"], N=N, P=0 if a.plain else P, reps=a.reps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), ms={})
    for k, t in times.items():
        res["ms"][k] = dict(median=statistics.median(t), min=min(t), max=max(t), all=[round(x, 3) for x in t])
        print(f"{k}: median {statistics.median(t):.2f} ms  min {min(t):.2f}  max {max(t):.2f}  ({len(t)} calls)")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
