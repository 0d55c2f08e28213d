"""CPU stand-in of liblgen_hip.so for the VQEngine host test: a recorder that takes the place of `_lib.lib`, `_lib.ptr` and
`_lib.stream`, runs no kernel and writes down every launch -- the function name and each argument typed from
`_lib.SIGNATURES[name]`: ints and floats verbatim, a pointer as None or `b<k>:dtype:numel` with k numbered by first appearance in
the trace.  That pins the kernel sequence, every scalar, every buffer size and the dataflow (which output feeds which input).

`python -m tests.vq_standin --write` records the six traces of TRACES x MODES into tests/vq_launch_trace.json;
`--engine FILE` records from that copy of vq_engine.py instead of the package's (how a parent commit's engine is recorded)."""
import contextlib
import functools
import importlib.util
import json
import os
import sys

import torch

from llamagen_amd import _lib as L

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vq_launch_trace.json")


class Recorder:
    def __init__(self):
        self.calls = []
        self._keep = []      # every tensor ptr() was handed: torch.empty on the CPU reuses freed blocks, an address must not recur
        self._by_addr = {}
        self._labels = {}

    def install(self, setattr_):
        """setattr_(obj, name, value): pytest's monkeypatch.setattr, or patched() below."""
        setattr_(L, "lib", lambda: self)
        setattr_(L, "ptr", self._ptr)
        setattr_(L, "stream", lambda: 0)

    def start(self):
        """A new trace: forget the calls so far (the constructor's) and number the buffers from b0 again."""
        self.calls, self._labels = [], {}

    def _ptr(self, t):
        if t is None:
            return 0
        self._keep.append(t)
        self._by_addr[t.data_ptr()] = t
        return t.data_ptr()

    def __getattr__(self, name):
        if name not in L.SIGNATURES:
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _call(self, name, *args):
        sig = L.SIGNATURES[name]
        assert len(args) == len(sig), (name, len(args), len(sig))
        rec = [name]
        for a, ty in zip(args, sig):
            if ty is L._P:
                if not a:
                    rec.append(None)
                    continue
                t = self._by_addr[a]  # KeyError: an address that never went through _lib.ptr
                label = self._labels.setdefault(a, f"b{len(self._labels)}")
                rec.append(f"{label}:{str(t.dtype).replace('torch.', '')}:{t.numel()}")
            elif ty is L._F:
                rec.append(float(a))
            else:
                assert isinstance(a, int) and not isinstance(a, bool), (name, a)
                rec.append(a)
        if name == "lgen_vq_argmin":  # the codebook gather after it needs indices in range
            self._by_addr[args[3]].zero_()
        self.calls.append(rec)
        return 0


# ---- the six traces of tests/test_vq_engine_host.py -----------------------------------------------------------------------------
def _decode_code(eng):
    codes = torch.randint(0, 16384, (1, 15), generator=torch.Generator().manual_seed(1))
    eng.decode_code(codes, [1, 8, 3, 5])      # 3x5, 6x10, 12x20 implicit-GEMM; 24x40, 48x80 fused


def _decode_quant(eng):
    eng.decode(torch.rand(2, 8, 8, 8, generator=torch.Generator().manual_seed(2)))  # every level fused


def _encode(eng):
    eng.encode(torch.rand(1, 3, 48, 32, generator=torch.Generator().manual_seed(3)) * 2 - 1)  # fused levels -> stride-2 -> small maps


TRACES = {"decode_code_3x5": _decode_code, "decode_quant_8x8": _decode_quant, "encode_48x32": _encode}
MODES = {"fused": None, "unfused": "0"}   # value of LGEN_VQ_FUSED

_MODEL = None


def model():
    global _MODEL
    if _MODEL is None:
        from tests.cases import VQ_CASES
        from tests.util import build_vq_holder
        _MODEL = build_vq_holder(VQ_CASES["vq16_4x4"])[0]
    return _MODEL


def record(engine_cls, call, setattr_):
    """The launches of call(engine) on a fresh engine_cls(model()) under a recorder installed with setattr_."""
    rec = Recorder()
    rec.install(setattr_)
    with torch.no_grad():
        eng = engine_cls(model())
        rec.start()
        call(eng)
    return rec.calls


@contextlib.contextmanager
def patched():
    undo = []

    def setattr_(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    try:
        yield setattr_
    finally:
        for obj, name, value in reversed(undo):
            setattr(obj, name, value)


def _main(argv):
    if "--write" not in argv:
        sys.exit(__doc__)
    if "--engine" in argv:
        spec = importlib.util.spec_from_file_location("llamagen_amd._vq_engine_recorded", argv[argv.index("--engine") + 1])
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    else:
        from llamagen_amd import vq_engine as mod
    out = {}
    for tname, call in TRACES.items():
        for mname, env in MODES.items():
            os.environ.pop("LGEN_VQ_FUSED", None)
            if env is not None:
                os.environ["LGEN_VQ_FUSED"] = env
            with patched() as setattr_:
                out[f"{tname}/{mname}"] = record(mod.VQEngine, call, setattr_)
            print(f"{tname}/{mname}: {len(out[f'{tname}/{mname}'])} launches")
    os.environ.pop("LGEN_VQ_FUSED", None)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    _main(sys.argv[1:])
