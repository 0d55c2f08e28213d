"""Workload for timing the sampler kernel of the continuous batcher (development aid): a 64-slot GPT-L bf16 ContinuousBatcher
(384 px class-conditional, cfg 4.0, top-k 2000) drains one warm-up round of 64 requests (kernels, graph capture) and then
2 x 64 requests of N tokens each, all through hipGraph replay.
    rocprofv3 --kernel-trace --stats -d OUT -o serve -- python tools/serve_sampler_trace.py [N]        (default N = 96)
and read the `sample_kernel` row of OUT/**/serve_kernel_stats.csv: its average time is the figure DESIGN.md quotes for the
per-slot sampling records against the batch-wide scalars.  Uses the constructor / submit / run interface only, so the same
file runs on a checkout from before the records existed."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llamagen_amd import GPT_models  # noqa: E402
from llamagen_amd.serve import ContinuousBatcher  # noqa: E402


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 96
    slots, dev = 64, torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    gpt = GPT_models["GPT-L"](vocab_size=16384, block_size=576, num_classes=1000, cls_token_num=1, model_type="c2i")
    torch.nn.init.normal_(gpt.output.weight, 0, 0.02)  # zero-initialised in the reference (gpt.py:305)
    gpt = gpt.to(device=dev, dtype=torch.bfloat16).eval()
    cb = ContinuousBatcher(gpt, slots, N, cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=2000, top_p=1.0, sample_logits=True)
    labels = torch.randint(0, 1000, (3 * slots,)).tolist()
    for l in labels[:slots]:
        cb.submit(l)
    cb.run()
    torch.cuda.synchronize()
    for l in labels[slots:]:
        cb.submit(l)
    t = time.perf_counter()
    out = cb.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    assert len(out) == 2 * slots
    print(f"{2 * slots} requests x {N} tokens on {slots} slots: {dt:.3f} s, {cb.steps_run} steps, "
          f"{dt / (2 * N) * 1e6:.1f} us per step", flush=True)


if __name__ == "__main__":
    main()
