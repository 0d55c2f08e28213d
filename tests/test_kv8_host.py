"""FP8 (e4m3) KV cache, host side (no GPU): the three new C entry points, the format helpers the GPU tests use as their
reference, Transformer.set_kv_cache and the refusals of what the option does not cover."""
import os
import re
import types

import pytest
import torch

from tests.kv8_cases import KV8Sdpa, all_codes, dequant, qbytes, quant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KV8_SYMBOLS = ("lgen_gemm_qkv_rope_kv8", "lgen_gemm_qkv_rope_tile_kv8", "lgen_attn_decode_kv8")


def _tiny(**over):
    from llamagen_amd.gpt import ModelArgs, Transformer
    kw = dict(n_layer=2, n_head=4, dim=256, vocab_size=1024, block_size=16, num_classes=10)
    kw.update(over)
    return Transformer(ModelArgs(**kw))


def test_kv8_symbols_are_exported_declared_and_bound():
    from llamagen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lgen.h")).read()
    declared = dict(re.findall(r"^int\s+(lgen_\w+)\s*\(([^;]*?)\);", header, flags=re.M | re.S))
    for name, twin, extra in zip(KV8_SYMBOLS, ("lgen_gemm_qkv_rope", "lgen_gemm_qkv_rope_tile", "lgen_attn_decode"), (2, 2, 2)):
        assert hasattr(lib, name), name
        assert name in declared and name in _lib.SIGNATURES, name
        nargs = len([a for a in declared[name].split(",") if a.strip()])
        assert nargs == len(_lib.SIGNATURES[name]) == len(_lib.SIGNATURES[twin]) + extra, name   # the twin's arguments + two scales
        assert _lib.SIGNATURES[name][-3:-1] == [_lib._F, _lib._F], name
    assert lib.lgen_abi_version() == _lib.ABI_VERSION == 10   # additive: the version does not move
    assert "e4m3fn" in header and "fnuz" in header            # the header states the encoding


def test_kv8_entry_points_refuse_what_is_out_of_scope():
    """dtype != bf16 and hdp != 64 are LGEN_ERR_UNSUPPORTED, bad strides LGEN_ERR_BAD_ARG -- all decided before any launch (the
    pointers are dummies)."""
    from llamagen_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = L.lib()
    qkv = lambda dtype, hd, hdp, stride: lib.lgen_gemm_qkv_rope_kv8(8, 8, 8, 8, 8, 8, 8, 16, 1, 32 * hd, 32, hd, hdp, 40, stride, dtype,
                                                                    1, 1, 1, 0, 0, 0, 0.0, 1, 1.0, 1.0, 0)
    tile = lambda dtype, hd, hdp, stride: lib.lgen_gemm_qkv_rope_tile_kv8(8, 8, 8, 8, 8, 8, 8, 256, 16, 32 * hd, 32, hd, hdp, 40, stride,
                                                                          dtype, 4, 1, 1, 3, 4, 4, 4, 8, 8, 32 * hd // 16, 1e-5, 1.0, 1.0, 0)
    attn = lambda dtype, hd, hdp, stride, variant=-1: lib.lgen_attn_decode_kv8(8, 8, 8, 8, 8, 0, 0, 3, 1, 4, hd, hdp, 40, stride, dtype,
                                                                               variant, 1.0, 1.0, 0)
    for f in (qkv, tile, attn):
        assert f(L.F32, 64, 64, 64) == L.ERR_UNSUPPORTED
        assert f(L.F16, 64, 64, 64) == L.ERR_UNSUPPORTED
        assert f(L.BF16, 100, 128, 104) == L.ERR_UNSUPPORTED     # GPT-3B's head_dim
        assert f(L.BF16, 64, 64, 60) == L.ERR_BAD_ARG            # not a multiple of the 8-byte piece
        assert f(L.BF16, 64, 64, 56) == L.ERR_BAD_ARG            # shorter than the row
    for variant in (0, 1, 6, 8, 14, 99):
        assert attn(L.BF16, 64, 64, 64, variant) == L.ERR_UNSUPPORTED, variant


def test_quant_round_trips_the_254_finite_codes():
    codes, finite = all_codes()
    assert int(finite.sum()) == 254
    for s in (1.0, 0.5, 2.0, 0.25):
        back = qbytes(dequant(codes[finite], s), s)
        assert torch.equal(back, codes[finite].view(torch.uint8)), s
    assert float(codes.float()[finite].abs().max()) == 448.0


def test_quant_saturates_instead_of_producing_nan():
    x = torch.tensor([449.0, 464.0, 465.0, 1e4, 3e38, float("inf"), -449.0, -465.0, -1e4, float("-inf")])
    q = quant(x, 1.0)
    assert not torch.isnan(q.float()).any()
    assert q.float().tolist() == [448.0] * 6 + [-448.0] * 4
    assert qbytes(x, 1.0).tolist() == [0x7E] * 6 + [0xFE] * 4
    assert torch.isnan(torch.tensor(465.0).to(torch.float8_e4m3fn).float())   # the bare cast: why the clamp is explicit
    assert quant(torch.tensor([300.0]), 0.5).float().item() == 448.0 and dequant(quant(torch.tensor([300.0]), 0.5), 0.5).item() == 224.0


def test_quant_is_idempotent_and_keeps_zero():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(4096, generator=g) * torch.logspace(-4, 3, 4096)).to(torch.bfloat16)
    for s in (1.0, 0.5, 2.0):
        once = dequant(quant(x, s), s)
        assert torch.equal(qbytes(once, s), qbytes(x, s)), s
        assert torch.equal(dequant(quant(once, s), s), once), s
    assert qbytes(torch.zeros(3), 2.0).tolist() == [0, 0, 0]


def test_sdpa_wrapper_quantises_k_and_v_with_the_layers_scales():
    from oracle import llamagen_oracle as O
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(1, 2, 1, 8, generator=g), torch.randn(1, 2, 5, 8, generator=g) * 3, torch.randn(1, 2, 5, 8, generator=g) * 3)
    mask = torch.ones(1, 1, 1, 5, dtype=torch.bool)
    orig = O.sdpa_math
    with KV8Sdpa([(0.5, 2.0), (1.0, 0.25)]) as w:
        a = O.sdpa_math(q, k, v, mask, torch.float32)
        b = O.sdpa_math(q, k, v, mask, torch.float32)
        assert w.calls == 2
    assert O.sdpa_math is orig
    assert torch.equal(a, orig(q, dequant(quant(k, 0.5), 0.5), dequant(quant(v, 2.0), 2.0), mask, torch.float32))
    assert torch.equal(b, orig(q, dequant(quant(k, 1.0), 1.0), dequant(quant(v, 0.25), 0.25), mask, torch.float32))
    assert not torch.equal(a, orig(q, k, v, mask, torch.float32))


def test_set_kv_cache_validates_its_arguments(monkeypatch):
    from llamagen_amd.gpt import kv_cache_config
    monkeypatch.delenv("LGEN_KV_DTYPE", raising=False)
    m = _tiny()
    assert kv_cache_config(m) == (None, None, None)
    m.set_kv_cache("fp8_e4m3")
    assert kv_cache_config(m) == ("fp8_e4m3", (1.0, 1.0), (1.0, 1.0))
    m.set_kv_cache("fp8_e4m3", k_scales=0.5, v_scales=[2.0, 0.25])
    assert kv_cache_config(m) == ("fp8_e4m3", (0.5, 0.5), (2.0, 0.25))
    assert kv_cache_config(m.lane_view()) == kv_cache_config(m)   # lanes of one model share the setting
    early = m.lane_view()                                         # ... also lanes that exist before a later call (a pipeline's lanes)
    m.set_kv_cache("fp8_e4m3", 0.25, 4.0)
    assert kv_cache_config(early) == kv_cache_config(m) == ("fp8_e4m3", (0.25, 0.25), (4.0, 4.0))
    early.set_kv_cache(None)
    assert kv_cache_config(m) == (None, None, None)
    m.set_kv_cache(None)
    assert kv_cache_config(m) == (None, None, None)
    for bad in (dict(dtype="fp8"), dict(dtype="fp8_e5m2"), dict(dtype="fp8_e4m3", k_scales=[1.0]), dict(dtype="fp8_e4m3", v_scales=0.0),
                dict(dtype="fp8_e4m3", k_scales=-1.0), dict(dtype="fp8_e4m3", v_scales=[1.0, float("nan")]),
                dict(dtype="fp8_e4m3", k_scales=float("inf")), dict(dtype=None, k_scales=2.0)):
        with pytest.raises(ValueError):
            m.set_kv_cache(**bad)
    assert kv_cache_config(m) == (None, None, None)               # a refused call changes nothing
    with pytest.raises(NotImplementedError, match="head_dim 100"):
        _tiny(n_head=8, dim=800).set_kv_cache("fp8_e4m3")
    # nothing set on the model: the environment variable selects fp8 with unit scales; the model's own setting wins
    monkeypatch.setenv("LGEN_KV_DTYPE", "fp8_e4m3")
    assert kv_cache_config(m) == ("fp8_e4m3", (1.0, 1.0), (1.0, 1.0))
    m.set_kv_cache("fp8_e4m3", 4.0, 8.0)
    assert kv_cache_config(m) == ("fp8_e4m3", (4.0, 4.0), (8.0, 8.0))
    monkeypatch.setenv("LGEN_KV_DTYPE", "int4")
    with pytest.raises(ValueError):
        kv_cache_config(_tiny())


def _standin(kind="c2i", kv=("fp8_e4m3", (1.0,), (1.0,))):
    return types.SimpleNamespace(model_type=kind, num_classes=1000, n_layer=1, _kv_cache=kv, _engine=None,
                                 tok_embeddings=types.SimpleNamespace(weight=torch.zeros(1, dtype=torch.bfloat16)))


def test_batcher_and_score_refuse_a_model_with_an_fp8_kv_cache(monkeypatch):
    from llamagen_amd import score
    from llamagen_amd.serve import ContinuousBatcher
    monkeypatch.delenv("LGEN_KV_DTYPE", raising=False)
    for model in (_standin("c2i"), _standin("t2i")):
        with pytest.raises(NotImplementedError, match="set_kv_cache"):
            ContinuousBatcher(model, 4, 16)
        with pytest.raises(NotImplementedError, match="set_kv_cache"):
            score(model, torch.tensor([1, 2]), torch.zeros(2, 4, dtype=torch.long))
    real = _tiny()
    real.set_kv_cache("fp8_e4m3", 0.5, 2.0)
    with pytest.raises(NotImplementedError, match="set_kv_cache"):
        ContinuousBatcher(real, 4, 16)
    with pytest.raises(NotImplementedError, match="set_kv_cache"):
        score(real, torch.tensor([1]), torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="set_kv_cache"):
        real.eval()(torch.zeros(1, 4, dtype=torch.long), torch.tensor([1]))   # whole-sequence forward
    # selected through the environment only
    monkeypatch.setenv("LGEN_KV_DTYPE", "fp8_e4m3")
    with pytest.raises(NotImplementedError, match="LGEN_KV_DTYPE"):
        ContinuousBatcher(_standin("c2i", kv=None), 4, 16)
    # without the option the same calls get past the check (and fail later for want of a GPU / an engine, not with this error)
    monkeypatch.delenv("LGEN_KV_DTYPE")
    with pytest.raises(Exception) as ei:
        ContinuousBatcher(_standin("c2i", kv=None), 4, 16)
    assert not isinstance(ei.value, NotImplementedError)
