"""Decode attention per launch, bf16 K/V against the fp8 (e4m3) KV cache, on the chip alone.
    python tools/attn_kv8_bench.py [--rows 640] [--launches 200] [--out kv8_attn.json]

GPT-L shape (16 heads, head_dim 64, S8 = 584), `rows` chain rows (640 = bench.py's chain: the library picks the persistent form for
both formats), positions 64 / 288 / 575.  lgen_attn_decode and lgen_attn_decode_kv8 launches ALTERNATE in one process; each is
timed with its own pair of HIP events, >= `launches` of each per position after a warm-up, and the median is reported (the mean
next to it).  Algorithmic bytes = K and V rows of the pos + 1 visible keys + q + the output; TB/s = bytes / median time.  Prints a
table and writes JSON (committed as profiles/kv8_attn.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llamagen_amd import _lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=640)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=str, default="kv8_attn.json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib, st = L.lib(), L.stream()
    H, hd, S8, B2 = 16, 64, 584, a.rows
    mts = (B2 + 15) // 16
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.zeros(mts * 16, H, 64, dtype=torch.bfloat16, device=dev)
    q[:B2] = torch.randn(B2, H, 64, generator=g, device=dev).to(torch.bfloat16)
    n = B2 * H * S8 * 64
    kv = {}
    for name, dt in (("bf16", torch.bfloat16), ("fp8_e4m3", torch.uint8)):
        flats = []
        for _ in range(2):
            if dt == torch.bfloat16:
                body = torch.randn(n, generator=g, device=dev).to(torch.bfloat16)
            else:   # random e4m3 codes of magnitude < 2 with a random sign (timing does not depend on the values; all finite)
                body = (torch.randint(0, 0x40, (n,), generator=g, device=dev, dtype=torch.uint8)
                        | (torch.randint(0, 2, (n,), generator=g, device=dev, dtype=torch.uint8) << 7))
            flats.append(torch.cat([body, torch.zeros(64, dtype=dt, device=dev)]))   # the slack both kernels may read
        kv[name] = flats
    out = torch.zeros(H * hd // 32, mts, 64, 8, dtype=torch.bfloat16, device=dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)

    def launch(name):
        k, v = kv[name]
        if name == "bf16":
            rc = lib.lgen_attn_decode(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(state), 0, 0, B2, mts, H, hd, 64, S8, 64, L.BF16, -1, st)
        else:
            rc = lib.lgen_attn_decode_kv8(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(state), 0, 0, B2, mts, H, hd, 64, S8, 64, L.BF16, -1,
                                          1.0, 1.0, st)
        L.check(rc, "attn " + name)

    rec = dict(shape=dict(rows=B2, heads=H, head_dim=hd, S8=S8), launches_per_format=a.launches, variant="library choice (-1)",
               device=torch.cuda.get_device_name(0), positions=[])
    print(f"{'pos':>4} {'format':>9} {'us median':>10} {'us mean':>9} {'MB':>8} {'TB/s':>6}")
    for pos in (64, 288, 575):
        state[0] = pos
        for _ in range(a.warmup):
            launch("bf16")
            launch("fp8_e4m3")
        torch.cuda.synchronize()
        ev = {"bf16": [], "fp8_e4m3": []}
        for _ in range(a.launches):
            for name in ("bf16", "fp8_e4m3"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(name)
                e1.record()
                ev[name].append((e0, e1))
        torch.cuda.synchronize()
        row = dict(pos=pos)
        for name, esz in (("bf16", 2), ("fp8_e4m3", 1)):
            us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[name]]
            nbytes = 2 * B2 * H * (pos + 1) * hd * esz + 2 * B2 * H * hd * 2
            med = statistics.median(us)
            row[name] = dict(us_median=round(med, 2), us_mean=round(statistics.fmean(us), 2), us_min=round(min(us), 2),
                             algorithmic_bytes=nbytes, tb_per_s=round(nbytes / med / 1e6, 3))
            print(f"{pos:>4} {name:>9} {med:>10.2f} {statistics.fmean(us):>9.2f} {nbytes / 1e6:>8.1f} {nbytes / med / 1e6:>6.2f}")
        row["fp8_over_bf16_time"] = round(row["fp8_e4m3"]["us_median"] / row["bf16"]["us_median"], 3)
        print(f"{pos:>4} fp8 / bf16 time ratio {row['fp8_over_bf16_time']:.3f}")
        rec["positions"].append(row)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
