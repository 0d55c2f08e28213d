"""Helpers of the FP8 (e4m3) KV-cache tests: the format restated on the CPU with torch's float8_e4m3fn cast, and a context
manager that makes the UNMODIFIED oracle see quantised K / V (tests/test_kv8_host.py, tests/test_gpu_kv8.py)."""
import torch

from oracle import llamagen_oracle as O

E4M3_MAX = 448.0
POISON = 0x7E   # the code of +448: finite, so a read of an invisible key shows as a wrong result, not as NaN


def quant(x, s):
    """include/lgen.h "FP8 KV cache": q = rne_e4m3(clamp(x * float32(1 / s), -448, 448)), x the bf16 value the default path stores."""
    return (x.float() * torch.tensor(1 / s, dtype=torch.float32)).clamp(-448, 448).to(torch.float8_e4m3fn)


def dequant(q, s):
    return q.float() * s


def qbytes(x, s):
    return quant(x, s).view(torch.uint8)


def all_codes():
    """The 256 byte values as float8_e4m3fn, and which of them are finite (0x7f and 0xff are the two NaNs)."""
    c = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn)
    return c, ~torch.isnan(c.float())


class KV8Sdpa:
    """Context: O.sdpa_math sees k, v as dequant(quant(.)) with the scales of the layer that calls it.  Quantising the whole cache
    on every call is idempotent and zeros stay zero, so this is exactly "quantise at append", the current key included.  `scales`:
    one (s_k, s_v) pair, or one per layer -- the oracle calls sdpa_math once per layer per forward, so a call counter modulo the
    layer count picks the pair."""

    def __init__(self, scales):
        self.scales = [scales] if isinstance(scales[0], (int, float)) else list(scales)
        self.calls = 0

    def __enter__(self):
        self.orig = O.sdpa_math

        def wrapped(q, k, v, mask, dt):
            sk, sv = self.scales[self.calls % len(self.scales)]
            self.calls += 1
            return self.orig(q, dequant(quant(k, sk), sk), dequant(quant(v, sv), sv), mask, dt)
        O.sdpa_math = wrapped
        return self

    def __exit__(self, *a):
        O.sdpa_math = self.orig
