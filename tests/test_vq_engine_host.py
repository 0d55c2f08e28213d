"""VQEngine's launch sequence on the CPU: the engine drives tests/vq_standin.py's recorder in place of the HIP library, and every
launch -- kernel, order, each scalar, each buffer size, which buffer feeds which -- must equal tests/vq_launch_trace.json.

The fixture was recorded from commit cadb143 (the parent of the single-dispatch refactor of vq_engine.py), whose engine needed one
edit to be constructed on the CPU: its final stream synchronize guarded by `self.dev.type == "cuda"`.  With that file saved as F:
`python -m tests.vq_standin --write --engine F`.  It is not regenerated from a refactored engine -- if a trace differs, the engine
is wrong.  A later change that alters the launch sequence ON PURPOSE regenerates it from its own tree with
`python -m tests.vq_standin --write` and says so."""
import json

import pytest
import torch

from llamagen_amd.vq_engine import VQEngine
from tests import vq_standin as S

# launches per trace, counted from cadb143
COUNTS = {"decode_code_3x5/fused": 156, "decode_code_3x5/unfused": 172, "decode_quant_8x8/fused": 122,
          "decode_quant_8x8/unfused": 172, "encode_48x32/fused": 123, "encode_48x32/unfused": 131}
UPSAMPLE = {"lgen_conv_igemm": 15, "lgen_conv_fused": 16}  # position of the resample argument in a record


@pytest.fixture(scope="module")
def fixture():
    with open(S.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def traces():
    return {}


def _trace(traces, monkeypatch, key):
    """The engine's trace for `key`, recorded once per module and kept as JSON would hold it."""
    if key not in traces:
        tname, mname = key.split("/")
        if S.MODES[mname] is None:
            monkeypatch.delenv("LGEN_VQ_FUSED", raising=False)
        else:
            monkeypatch.setenv("LGEN_VQ_FUSED", S.MODES[mname])
        traces[key] = json.loads(json.dumps(S.record(VQEngine, S.TRACES[tname], monkeypatch.setattr)))
    return traces[key]


def test_fixture_is_the_parents(fixture):
    assert {k: len(v) for k, v in fixture.items()} == COUNTS


@pytest.mark.parametrize("key", list(COUNTS))
def test_launch_trace_matches_fixture(fixture, traces, monkeypatch, key):
    got, want = _trace(traces, monkeypatch, key), fixture[key]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{key}: launch {i} differs\n  engine:  {g}\n  fixture: {w}"
    assert len(got) == len(want), f"{key}: {len(got)} launches, the fixture has {len(want)}; first extra: {(got + want)[min(len(got), len(want))]}"


def test_trace_structure(traces, monkeypatch):
    names = lambda key: [c[0] for c in _trace(traces, monkeypatch, key)]
    mixed = names("decode_code_3x5/fused")       # 3x5 .. 12x20 implicit-GEMM, then an unfused producer feeds the fused 24x40 level
    assert "lgen_conv_fused" in mixed and "lgen_gn_stats" in mixed
    assert "lgen_conv_fused" in names("encode_48x32/fused")
    for key in COUNTS:
        tr = _trace(traces, monkeypatch, key)
        if key.endswith("/unfused"):
            assert not {"lgen_conv_fused", "lgen_gn_finalize"} & {c[0] for c in tr}, key
        # the stride-2 conv has no fused form; the fused kernel only ever sees resample 0 or 1
        assert all(c[UPSAMPLE[c[0]]] in (0, 1) for c in tr if c[0] == "lgen_conv_fused"), key
    for mname in S.MODES:
        tr = _trace(traces, monkeypatch, f"encode_48x32/{mname}")
        assert sum(c[0] == "lgen_conv_igemm" and c[UPSAMPLE[c[0]]] == 2 for c in tr) == 4, mname  # the four Downsample convs


def test_cpu_model_is_still_refused():
    with pytest.raises(RuntimeError, match=r"^llamagen_amd\.VQModel runs only on an AMD GPU through the HIP library \(no CPU fallback\)$"):
        S.model().decode_code(torch.zeros(1, 15, dtype=torch.int64), [1, 8, 3, 5])
