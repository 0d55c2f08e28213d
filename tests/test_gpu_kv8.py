"""FP8 (e4m3) KV cache on the GPU (include/lgen.h "FP8 KV cache").

Kernel level: the *_kv8 append entry points must write exactly quant(what the bf16 twin stores) -- byte for byte, q bit-identical,
nothing else touched -- and lgen_attn_decode_kv8 must meet the bar of the bf16 attention kernels (`_close` of
tests/test_gpu_gpt.py at its bf16 setting) against the oracle's sdpa_math on the dequantised slabs: a bf16 x e4m3 product is exact
in fp32, so the arithmetic differs by summation order only.  End to end: teacher-forced CFG-mixed logits against the UNMODIFIED
oracle whose sdpa_math sees dequant(quant(k)), dequant(quant(v)) (tests/kv8_cases.py), held to the project's bf16 rule
max(4 / 0.25 ulp, 2 x the oracle's own fp32-vs-fp64 distance); graph replay == eager; switching formats; refusals."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llamagen_oracle as O  # noqa: E402
from tests.cases import GPT_CASES, make_gpt_inputs  # noqa: E402
from tests.kv8_cases import POISON, KV8Sdpa, dequant, qbytes, quant  # noqa: E402
from tests.test_gpu_gpt import _close, _dev, _L, _rand  # noqa: E402
from tests.test_gpu_headline import _check, _Linear64  # noqa: E402
from tests.util import build_gpt_holder, oracle_cfg  # noqa: E402

BF = torch.bfloat16
SENTINEL = 0x55
SK, SV = 0.5, 2.0     # distinct, so that a swap shows


def _slab(rows, H, S8, fill, kvs=64):
    """A byte slab [rows][H][S8][kvs] + the 64 bytes of slack the attention may read, all `fill`."""
    n = rows * H * S8 * kvs
    flat = torch.full((n + 64,), fill, dtype=torch.uint8, device=_dev())
    return flat, flat[:n].view(rows, H, S8, kvs)


def _spread_weight(n_out, d, seed):
    """wqkv whose output features span six decades, so that K / V elements saturate (> 448 s) and fall below 2^-6 s."""
    w = _rand((n_out, d), torch.float32, seed, 0.05)
    f = torch.tensor([1.0, 1000.0, 1e-3, 30.0, 1e-2, 1.0])[torch.arange(n_out) % 6]
    return (w * f[:, None]).to(BF)


def _has_extremes(b):
    mag = b & 0x7F
    return bool((mag == 0x7E).any()) and bool((((b & 0x78) == 0) & ((b & 0x07) != 0)).any())


def _check_append(tag, rc, rc8, q, q8, kc, vc, kflat, vflat, k8, v8, pos, hd=64):
    """bf16 twin vs kv8: the same return code; q bit-identical; slot `pos` == quant(bf16 slot); every other byte the sentinel."""
    L = _L()
    assert rc8 == rc, (tag, rc, rc8)
    if rc == L.ERR_UNSUPPORTED:   # a refused shape writes nothing
        assert bool((kflat == SENTINEL).all()) and bool((vflat == SENTINEL).all()) and not bool(q8.any()), tag
        return False
    assert rc == 0, (tag, rc)
    assert torch.equal(q, q8), (tag, "q")
    for name, c, flat, s8, s in (("k", kc, kflat, k8, SK), ("v", vc, vflat, v8, SV)):
        want = qbytes(c[:, :, pos, :hd].cpu(), s)
        got = s8[:, :, pos, :hd].cpu()
        assert torch.equal(got, want), (tag, name, int((got != want).sum()), got[got != want][:4].tolist(), want[got != want][:4].tolist())
        if name == "v" or pos > 0:   # (the RoPE table's conditioning row, position 0, is all zeros: K there is +-0 whatever the input)
            assert _has_extremes(want), (tag, name, "the inputs must saturate and reach the subnormals")
        rest = flat.clone()
        rest[: s8.numel()].view_as(s8)[:, :, pos, :hd] = SENTINEL
        assert bool((rest == SENTINEL).all()), (tag, name, "bytes outside the slot were written")
    return True


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("B2", [5, 19])
def test_kv8_append_skinny_equals_quant_of_the_bf16_append(B2, norm):
    """lgen_gemm_qkv_rope_kv8 (generic ring kernel, the norm-prologue ring kernel and the register-resident fused-norm kernel
    at passes 1 and 3; MT 1 / 2 / 4) against lgen_gemm_qkv_rope on the same inputs."""
    from llamagen_amd.engine import pack_act, pack_weight, precompute_freqs_cis_2d
    L, dev = _L(), _dev()
    lib = L.lib()
    H, hd, d, grid, mts = 2, 64, 128, 6, 4
    S8 = O.find_multiple(1 + grid * grid, 8)
    assert S8 == 40
    x = _rand((B2, d), BF, 101, 1.3)
    w = _spread_weight(3 * d, d, 102)
    nw = (1 + 0.1 * _rand((d,), torch.float32, 103)).to(BF).to(dev)
    xp, wp = pack_act(x.to(dev), mts), pack_weight(w.to(dev))
    fr = precompute_freqs_cis_2d(grid + 1, hd, 10000.0, 1).to(dev)   # 50 rows: an angle row for every slot of S8 = 40
    ssq = torch.full((mts * 16, L.SSQ_STRIDE), float("nan"), device=dev)
    L.check(lib.lgen_ssq_pack(L.ptr(xp), L.ptr(ssq), mts, d, L.BF16, L.stream()), "ssq_pack")
    # (mt, nt, kw, passes): fused norm -> cpw = 4 chunks per wave at kw 1 (register-resident kernel; (2, 2, 2) has cpw 2 and takes the
    # ring kernel with the norm prologue); plain -> the generic ring kernel
    shapes = [(1, 4, 1, 1), (2, 4, 1, 3), (4, 2, 1, 1), (1, 1, 1, 3), (2, 2, 2, 1)] if norm else [(1, 1, 1, 1), (2, 2, 2, 1), (4, 1, 4, 1), (4, 4, 1, 1)]
    nargs = (L.ptr(nw), L.ptr(ssq), d // 16, 1e-5) if norm else (0, 0, 0, 0.0)
    ran = 0
    for pos in (0, 17, 39):
        state = torch.tensor([pos, 0], dtype=torch.int32, device=dev)
        for mt, nt, kw, passes in shapes:
            kc, vc = torch.zeros(B2, H, S8, 64, dtype=BF, device=dev), torch.zeros(B2, H, S8, 64, dtype=BF, device=dev)
            q, q8 = torch.zeros(mts * 16, H, 64, dtype=BF, device=dev), torch.zeros(mts * 16, H, 64, dtype=BF, device=dev)
            (kflat, k8), (vflat, v8) = _slab(B2, H, S8, SENTINEL), _slab(B2, H, S8, SENTINEL)
            rc = lib.lgen_gemm_qkv_rope(L.ptr(wp), L.ptr(xp), L.ptr(q), L.ptr(kc), L.ptr(vc), L.ptr(fr), L.ptr(state), B2, mts, d, H, hd,
                                        64, S8, 64, L.BF16, mt, nt, kw, *nargs, passes, L.stream())
            rc8 = lib.lgen_gemm_qkv_rope_kv8(L.ptr(wp), L.ptr(xp), L.ptr(q8), L.ptr(k8), L.ptr(v8), L.ptr(fr), L.ptr(state), B2, mts, d, H,
                                             hd, 64, S8, 64, L.BF16, mt, nt, kw, *nargs, passes, 1.0 / SK, 1.0 / SV, L.stream())
            torch.cuda.synchronize()
            ran += _check_append((B2, norm, pos, mt, nt, kw, passes), rc, rc8, q, q8, kc, vc, kflat, vflat, k8, v8, pos)
    assert ran == 3 * len(shapes)


def test_kv8_append_skinny_steady_state_kernel():
    """The steady-state ring kernel (K long and uniform: d = 512, 16 chunks in one wave) has its own EPI_QKV8 instantiation."""
    from llamagen_amd.engine import pack_act, pack_weight, precompute_freqs_cis_2d
    L, dev = _L(), _dev()
    lib = L.lib()
    B2, H, hd, d, grid, mts, pos = 19, 8, 64, 512, 6, 4, 17
    S8 = 40
    xp, wp = pack_act(_rand((B2, d), BF, 111, 1.0).to(dev), mts), pack_weight(_spread_weight(3 * d, d, 112).to(dev))
    fr = precompute_freqs_cis_2d(grid + 1, hd, 10000.0, 1).to(dev)   # 50 rows: an angle row for every slot of S8 = 40
    state = torch.tensor([pos, 0], dtype=torch.int32, device=dev)
    for mt, nt in ((4, 1), (2, 2)):
        kc, vc = torch.zeros(B2, H, S8, 64, dtype=BF, device=dev), torch.zeros(B2, H, S8, 64, dtype=BF, device=dev)
        q, q8 = torch.zeros(mts * 16, H, 64, dtype=BF, device=dev), torch.zeros(mts * 16, H, 64, dtype=BF, device=dev)
        (kflat, k8), (vflat, v8) = _slab(B2, H, S8, SENTINEL), _slab(B2, H, S8, SENTINEL)
        rc = lib.lgen_gemm_qkv_rope(L.ptr(wp), L.ptr(xp), L.ptr(q), L.ptr(kc), L.ptr(vc), L.ptr(fr), L.ptr(state), B2, mts, d, H, hd, 64,
                                    S8, 64, L.BF16, mt, nt, 1, 0, 0, 0, 0.0, 1, L.stream())
        rc8 = lib.lgen_gemm_qkv_rope_kv8(L.ptr(wp), L.ptr(xp), L.ptr(q8), L.ptr(k8), L.ptr(v8), L.ptr(fr), L.ptr(state), B2, mts, d, H, hd,
                                         64, S8, 64, L.BF16, mt, nt, 1, 0, 0, 0, 0.0, 1, 1.0 / SK, 1.0 / SV, L.stream())
        torch.cuda.synchronize()
        assert _check_append(("steady", mt, nt), rc, rc8, q, q8, kc, vc, kflat, vflat, k8, v8, pos)


def _tile_setup():
    from llamagen_amd.engine import pack_act, pack_weight, precompute_freqs_cis_2d
    L, dev = _L(), _dev()
    M, H, hd, d, grid, mts = 256, 16, 64, 1024, 6, 16
    xp, wp = pack_act(_rand((M, d), BF, 121, 1.3).to(dev), mts), pack_weight(_spread_weight(3 * d, d, 122).to(dev))
    nw = (1 + 0.1 * _rand((d,), torch.float32, 123)).to(BF).to(dev)
    fr = precompute_freqs_cis_2d(grid + 1, hd, 10000.0, 1).to(dev)   # 50 rows: an angle row for every slot of S8 = 40
    ssq = torch.full((mts * 16, L.SSQ_STRIDE), float("nan"), device=dev)
    L.check(L.lib().lgen_ssq_pack(L.ptr(xp), L.ptr(ssq), mts, d, L.BF16, L.stream()), "ssq_pack")
    return dict(M=M, H=H, hd=hd, d=d, mts=mts, S8=40, xp=xp, wp=wp, nw=nw, fr=fr, ssq=ssq)


def _tile_kv8(t, shape, state, q8, k8, v8):
    L = _L()
    return L.lib().lgen_gemm_qkv_rope_tile_kv8(L.ptr(t["wp"]), L.ptr(t["xp"]), L.ptr(q8), L.ptr(k8), L.ptr(v8), L.ptr(t["fr"]), L.ptr(state),
                                               t["M"], t["mts"], t["d"], t["H"], t["hd"], 64, t["S8"], 64, L.BF16, *shape, L.ptr(t["nw"]),
                                               L.ptr(t["ssq"]), t["d"] // 16, 1e-5, 1.0 / SK, 1.0 / SV, L.stream())


def test_kv8_append_tile_equals_quant_of_the_bf16_append():
    """lgen_gemm_qkv_rope_tile_kv8 at GPT-L width, 256 rows, with the shapes the schedule names for 256 and 640 rows; a shape the
    library refuses (no instantiation / one that would spill) returns LGEN_ERR_UNSUPPORTED and writes nothing."""
    from llamagen_amd.gemm_schedule import TILE_SCHEDULES
    L, dev = _L(), _dev()
    lib = L.lib()
    t = _tile_setup()
    M, H, S8, mts = t["M"], t["H"], t["S8"], t["mts"]
    shapes = [TILE_SCHEDULES[16]["qkv"], TILE_SCHEDULES[40]["qkv"], (8, 1, 1, 8, 2, 4, 4), (2, 2, 1, 1, 4, 4, 4)]
    ran = refused = 0
    for pos in (0, 17, 39):   # (position 0: K is +-0 through the zero RoPE row, codes 0x00 / 0x80)
        state = torch.tensor([pos, 0], dtype=torch.int32, device=dev)
        for shape in shapes:
            kc, vc = torch.zeros(M, H, S8, 64, dtype=BF, device=dev), torch.zeros(M, H, S8, 64, dtype=BF, device=dev)
            q, q8 = torch.zeros(mts * 16, H, 64, dtype=BF, device=dev), torch.zeros(mts * 16, H, 64, dtype=BF, device=dev)
            (kflat, k8), (vflat, v8) = _slab(M, H, S8, SENTINEL), _slab(M, H, S8, SENTINEL)
            rc = lib.lgen_gemm_qkv_rope_tile(L.ptr(t["wp"]), L.ptr(t["xp"]), L.ptr(q), L.ptr(kc), L.ptr(vc), L.ptr(t["fr"]), L.ptr(state), M,
                                             mts, t["d"], H, t["hd"], 64, S8, 64, L.BF16, *shape, L.ptr(t["nw"]), L.ptr(t["ssq"]),
                                             t["d"] // 16, 1e-5, L.stream())
            rc8 = _tile_kv8(t, shape, state, q8, k8, v8)
            torch.cuda.synchronize()
            ok = _check_append(("tile", pos, shape), rc, rc8, q, q8, kc, vc, kflat, vflat, k8, v8, pos)
            ran, refused = ran + ok, refused + (not ok)
    assert ran == 6 and refused == 6, (ran, refused)   # the two schedule shapes ran, the other two were refused, at every position


# ---- decode attention ---------------------------------------------------------------------------------------------------
ATTN_POSITIONS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 199)   # the boundaries of 32-, 64- and 128-key groups


def _attn_inputs(B2, H, S8, seed):
    g = torch.Generator().manual_seed(seed)
    mts = max(1, (B2 + 15) // 16)
    q = torch.zeros(mts * 16, H, 64, dtype=BF)
    q[:B2] = torch.randn(B2, H, 64, generator=g).to(BF)
    kq, vq = quant(torch.randn(B2, H, S8, 64, generator=g) * 3, SK), quant(torch.randn(B2, H, S8, 64, generator=g) * 3, SV)
    full = torch.tril(torch.ones(S8, S8, dtype=torch.bool)).unsqueeze(0).repeat(B2, 1, 1)
    rnd = full & (torch.rand(B2, 1, S8, generator=g) > 0.3) | torch.eye(S8, dtype=torch.bool)
    return mts, q, kq, vq, full, rnd


def _attn_kv8(q_d, k8, v8, out, state, mask_d, mask_len, B2, mts, H, S8, variant):
    L = _L()
    return L.lib().lgen_attn_decode_kv8(L.ptr(q_d), L.ptr(k8), L.ptr(v8), L.ptr(out), L.ptr(state), L.ptr(mask_d), mask_len, B2, mts, H, 64,
                                        64, S8, 64, L.BF16, variant, SK, SV, L.stream())


@pytest.mark.parametrize("mask_kind", ["causal", "random", "random_prefix100"])
@pytest.mark.parametrize("B2", [3, 32])
def test_kv8_decode_attention_vs_oracle_on_dequantised_slabs(B2, mask_kind):
    """Variants -1 / 2 (workgroup form) and 10 (persistent form, forced at these few rows) at every group boundary; the slots
    behind `pos` hold the code of +448, so a key that must not be seen changes the result."""
    from llamagen_amd.engine import unpack_act
    dev = _dev()
    H, S8 = 4, O.find_multiple(1 + 14 * 14, 8)
    assert S8 == 200
    mts, q, kq, vq, causal, rnd = _attn_inputs(B2, H, S8, 131 + B2)
    kd, vd = dequant(kq, SK), dequant(vq, SV)
    mask_len = 100 if mask_kind == "random_prefix100" else 0
    if mask_kind == "causal":
        mask_d, eff = None, causal
    else:
        mask_d = rnd.to(dev).contiguous()
        eff = rnd if mask_len == 0 else torch.where(torch.arange(S8) < mask_len, rnd, causal)   # keys >= mask_len: pure causal
    q_d = q.to(dev)
    (kflat, k8), (vflat, v8) = _slab(B2, H, S8, 0), _slab(B2, H, S8, 0)
    kb, vb = kq.view(torch.uint8).to(dev), vq.view(torch.uint8).to(dev)
    for pos in ATTN_POSITIONS:
        k8.copy_(kb)
        v8.copy_(vb)
        k8[:, :, pos + 1:] = POISON
        v8[:, :, pos + 1:] = POISON
        state = torch.tensor([pos, 0], dtype=torch.int32, device=dev)
        ref = O.sdpa_math(q[:B2].unsqueeze(2), kd, vd, eff[:, None, pos:pos + 1], BF).transpose(1, 2).reshape(B2, H * 64)
        for variant in (-1, 2, 10):
            out = torch.zeros(H * 64 // 32, mts, 64, 8, dtype=BF, device=dev)
            assert _attn_kv8(q_d, k8, v8, out, state, mask_d, mask_len, B2, mts, H, S8, variant) == 0
            _close(unpack_act(out, B2), ref, BF, f"attn kv8 B2={B2} {mask_kind} pos={pos} variant={variant}")


def test_kv8_decode_attention_256_rows_takes_the_persistent_form():
    """Variant -1 at 256 rows is the persistent kernel: the same bar, and the same bits as variant 10 asked for by name."""
    from llamagen_amd.engine import unpack_act
    dev = _dev()
    B2, H, S8, pos = 256, 4, 200, 129
    mts, q, kq, vq, causal, _ = _attn_inputs(B2, H, S8, 141)
    (kflat, k8), (vflat, v8) = _slab(B2, H, S8, 0), _slab(B2, H, S8, 0)
    k8.copy_(kq.view(torch.uint8).to(dev))
    v8.copy_(vq.view(torch.uint8).to(dev))
    k8[:, :, pos + 1:] = POISON
    v8[:, :, pos + 1:] = POISON
    state = torch.tensor([pos, 0], dtype=torch.int32, device=dev)
    ref = O.sdpa_math(q[:B2].unsqueeze(2), dequant(kq, SK), dequant(vq, SV), causal[:, None, pos:pos + 1], BF).transpose(1, 2).reshape(B2, H * 64)
    outs = {}
    for variant in (-1, 10, 2):
        out = torch.zeros(H * 64 // 32, mts, 64, 8, dtype=BF, device=dev)
        assert _attn_kv8(q.to(dev), k8, v8, out, state, None, 0, B2, mts, H, S8, variant) == 0
        outs[variant] = unpack_act(out, B2)
        _close(outs[variant], ref, BF, f"attn kv8 256 rows variant={variant}")
    assert torch.equal(outs[-1], outs[10])


def test_kv8_entry_points_are_deterministic():
    """20 launches of each *_kv8 entry point on one input: bit for bit the same outputs."""
    from llamagen_amd.engine import pack_act, pack_weight, precompute_freqs_cis_2d
    from llamagen_amd.gemm_schedule import TILE_SCHEDULES
    L, dev = _L(), _dev()
    lib = L.lib()
    # skinny, fused norm, three passes
    B2, H, hd, d, mts, S8, pos = 19, 2, 64, 128, 4, 40, 17
    xp, wp = pack_act(_rand((B2, d), BF, 101, 1.3).to(dev), mts), pack_weight(_spread_weight(3 * d, d, 102).to(dev))
    nw = (1 + 0.1 * _rand((d,), torch.float32, 103)).to(BF).to(dev)
    fr = precompute_freqs_cis_2d(7, hd, 10000.0, 1).to(dev)
    ssq = torch.full((mts * 16, L.SSQ_STRIDE), float("nan"), device=dev)
    L.check(lib.lgen_ssq_pack(L.ptr(xp), L.ptr(ssq), mts, d, L.BF16, L.stream()), "ssq_pack")
    state = torch.tensor([pos, 0], dtype=torch.int32, device=dev)

    def skinny():
        q8 = torch.zeros(mts * 16, H, 64, dtype=BF, device=dev)
        (kf, k8), (vf, v8) = _slab(B2, H, S8, SENTINEL), _slab(B2, H, S8, SENTINEL)
        assert lib.lgen_gemm_qkv_rope_kv8(L.ptr(wp), L.ptr(xp), L.ptr(q8), L.ptr(k8), L.ptr(v8), L.ptr(fr), L.ptr(state), B2, mts, d, H, hd, 64,
                                          S8, 64, L.BF16, 2, 4, 1, L.ptr(nw), L.ptr(ssq), d // 16, 1e-5, 3, 1.0 / SK, 1.0 / SV, L.stream()) == 0
        return q8, kf, vf

    t = _tile_setup()

    def tile():
        q8 = torch.zeros(t["mts"] * 16, t["H"], 64, dtype=BF, device=dev)
        (kf, k8), (vf, v8) = _slab(t["M"], t["H"], t["S8"], SENTINEL), _slab(t["M"], t["H"], t["S8"], SENTINEL)
        assert _tile_kv8(t, TILE_SCHEDULES[16]["qkv"], state, q8, k8, v8) == 0
        return q8, kf, vf

    aB2, aH, aS8, apos = 32, 4, 200, 199
    amts, q, kq, vq, _, rnd = _attn_inputs(aB2, aH, aS8, 151)
    q_d, mask_d = q.to(dev), rnd.to(dev).contiguous()
    (kflat, ak8), (vflat, av8) = _slab(aB2, aH, aS8, 0), _slab(aB2, aH, aS8, 0)
    ak8.copy_(kq.view(torch.uint8).to(dev))
    av8.copy_(vq.view(torch.uint8).to(dev))
    astate = torch.tensor([apos, 0], dtype=torch.int32, device=dev)

    def attn(variant):
        out = torch.zeros(aH * 64 // 32, amts, 64, 8, dtype=BF, device=dev)
        assert _attn_kv8(q_d, ak8, av8, out, astate, mask_d, 0, aB2, amts, aH, aS8, variant) == 0
        return (out,)

    for name, fn in (("skinny", skinny), ("tile", tile), ("attn 2", lambda: attn(2)), ("attn 10", lambda: attn(10))):
        first = fn()
        torch.cuda.synchronize()
        for i in range(19):
            again = fn()
            torch.cuda.synchronize()
            for a, b in zip(first, again):
                assert torch.equal(a, b), (name, i)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
LEG_A = dict(kwargs=dict(n_layer=2, n_head=4, dim=256, vocab_size=1024, block_size=64, num_classes=10, cls_token_num=1, model_type="c2i"),
             wseed=1, lin_std=0.05)
LEG_B = dict(kwargs=dict(n_layer=2, n_head=16, dim=1024, vocab_size=2048, block_size=64, num_classes=1000, cls_token_num=1,
                         model_type="c2i"), wseed=21, lin_std=0.02)
SCALES_2 = [(0.5, 2.0), (1.0, 0.25)]   # per layer (s_k, s_v)


def _set_fp8(m, scales):
    m.set_kv_cache("fp8_e4m3", [s[0] for s in scales], [s[1] for s in scales])


def _fill_caches8(oracles, eng, pos, hd, seed, scales):
    """Slots [0, pos) of every layer: quant bytes into the engine, the dequantised values into the oracles (one random draw, rolled
    per layer as tests/test_gpu_headline.py::_fill_caches does)."""
    g = torch.Generator().manual_seed(seed)
    B2, H, S8 = oracles[0].k_cache[0].shape[:3]
    kb = (torch.randn(B2, H, S8, hd, generator=g) * 0.6).to(BF)
    vb = (torch.randn(B2, H, S8, hd, generator=g) * 0.6).to(BF)
    for li in range(len(oracles[0].k_cache)):
        sk, sv = scales[li]
        sh = (li * 37) % S8
        kq, vq = quant(torch.roll(kb, sh, dims=2)[:, :, :pos], sk), quant(torch.roll(vb, sh, dims=2)[:, :, :pos], sv)
        for o in oracles:
            o.k_cache[li][:, :, :pos] = dequant(kq, sk)
            o.v_cache[li][:, :, :pos] = dequant(vq, sv)
        eng.k_cache[li][:, :, :pos, :hd] = kq.view(torch.uint8).to(eng.dev)
        eng.v_cache[li][:, :, :pos, :hd] = vq.view(torch.uint8).to(eng.dev)


def _teacher_forced8(case, B, cfg_scale, early, late, cond, scales, emb_masks=None, T=1):
    """tests/test_gpu_headline.py::_teacher_forced with an fp8 KV cache on the GPU side and both oracle evaluations (fp32 and fp64
    accumulation) under the sdpa_math wrapper; the self-distance comes from the two oracles, not from the code under test."""
    dev = _dev()
    m, sd = build_gpt_holder(case)
    m = m.to(device=dev, dtype=BF)
    _set_fp8(m, scales)
    cfgo = oracle_cfg(case)
    N, V, B2 = case["kwargs"]["block_size"], case["kwargs"]["vocab_size"], 2 * B
    if cfgo.model_type == "c2i":
        cond_c = torch.cat([cond, torch.ones_like(cond) * cfgo.num_classes])
        cond_dev = cond_c.to(dev)
    else:
        cond_c = torch.cat([cond, torch.zeros_like(cond) + sd["cls_embedding.uncond_embedding"]])
        cond_dev = cond_c.to(dev).to(BF)
    oracles = [O.GPTOracle(cfgo, sd, BF), O.GPTOracle(cfgo, sd, BF)]
    for o in oracles:
        o.setup_caches(B2, T + N)
    m.setup_caches(B2, T + N, BF)
    eng = m._engine
    assert eng.kv_dtype == "fp8_e4m3" and eng.k_cache.dtype == torch.uint8 and eng.kvs == 64
    assert m.layers[0].attention.kv_cache.k_cache.dtype == torch.uint8
    if emb_masks is not None:
        em = torch.cat([emb_masks, emb_masks])
        for o in oracles:
            cm = o.causal_mask
            cm[:, :, :T] = cm[:, :, :T] & (em.unsqueeze(1) != 0)
            o.causal_mask = cm | torch.eye(cm.size(1), dtype=torch.bool)
        cmd = m.causal_mask
        cmd[:, :, :T] = cmd[:, :, :T] & (em.to(dev).unsqueeze(1) != 0)
        cmd |= torch.eye(cmd.size(1), dtype=torch.bool, device=dev)
    g = torch.Generator().manual_seed(77)
    steps = [("prefill", None, True, torch.arange(0, T))]
    for i in range(early):
        steps.append((f"pos{T + i}", torch.randint(0, V, (B, 1), generator=g), None, torch.tensor([T + i])))
    for p in late:
        steps.append((f"late{p}", torch.randint(0, V, (B, 1), generator=g), None, torch.tensor([p])))
    out = []
    for label, tok, is_cond, ipos in steps:
        if label.startswith("late"):
            _fill_caches8(oracles, eng, int(ipos[0]), cfgo.head_dim, 1000 + int(ipos[0]), scales)
        refs = []
        x = None if tok is None else torch.cat([tok, tok])
        for k, o in enumerate(oracles):
            with KV8Sdpa(scales):
                if k == 1:
                    with _Linear64():
                        refs.append(o.forward(x, cond_c if is_cond else None, ipos)[:, -1])
                else:
                    refs.append(o.forward(x, cond_c if is_cond else None, ipos)[:, -1])
        if is_cond:
            lg, _ = m(None, cond_dev, ipos.to(dev))
        else:
            lg, _ = m(x.to(dev), None, ipos.to(dev).to(torch.int))
        got = O.cfg_mix(lg[:, -1].float().cpu(), cfg_scale)
        r0, r1 = O.cfg_mix(refs[0], cfg_scale), O.cfg_mix(refs[1], cfg_scale)
        ulp = r0.abs().max().item() * 2.0 ** -8
        e, s = (got - r0).abs(), (r1 - r0).abs()
        out.append(dict(step=label, ulp=ulp, err_max=e.max().item() / ulp, err_mean=e.mean().item() / ulp,
                        self_max=s.max().item() / ulp, self_mean=s.mean().item() / ulp,
                        argmax_agree=float((got.argmax(-1) == r0.argmax(-1)).float().mean())))
        print("kv8 parity", case["kwargs"]["dim"], out[-1])
    return out, m


def test_kv8_teacher_forced_logits_small_model_per_layer_scales():
    """Leg (a): depth 2, d 256, 4 heads, B = 3 (6 rows: skinny kernels, workgroup attention), per-layer scales: prefill,
    positions 1-3, position 60 on injected contents."""
    cond = torch.randint(0, 10, (3,), generator=torch.Generator().manual_seed(3))
    recs, m = _teacher_forced8(LEG_A, 3, 4.0, early=3, late=[60], cond=cond, scales=SCALES_2)
    assert m._engine.MTs == 1 and m._engine.S8 == 72
    _check("kv8_small_b3", recs)


def test_kv8_teacher_forced_logits_gptl_width_256_rows():
    """Leg (b): GPT-L width at depth 2, B = 128 -> 256 rows: wqkv on the tile family, persistent attention: prefill, positions
    1-2, position 60 on injected contents."""
    cond = torch.randint(0, 1000, (128,), generator=torch.Generator().manual_seed(5))
    recs, m = _teacher_forced8(LEG_B, 128, 4.0, early=2, late=[60], cond=cond, scales=SCALES_2)
    e = m._engine
    assert e.MTs == 16 and e.fuse_norm and e.gemm_schedule()["wqkv"]["family"] == "tile", e.gemm_schedule()
    _check("kv8_gptl_width_b256", recs)


def test_kv8_teacher_forced_logits_t2i_prefix_position_by_position():
    """Leg (c): the t2i case of the suite (T = 120 caption positions, emb_masks) through Transformer.__call__, which feeds the
    prefix one position at a time for every KV format: what this leg adds is the fp8 decode kernels with the caption mask consulted by
    the attention (`mask_len` = T) at T = 120.  The AUTOMATIC position-by-position prefix of generate() under fp8 is
    test_kv8_t2i_generate_takes_the_position_by_position_prefix below."""
    case = dict(GPT_CASES["t2i_cfg"])
    cond, masks = make_gpt_inputs(case)
    T = case["kwargs"]["cls_token_num"]
    recs, m = _teacher_forced8(case, case["batch"], case["cfg_scale"], early=2, late=[T + 12], cond=cond, scales=SCALES_2,
                               emb_masks=masks, T=T)
    _check("kv8_t2i_cfg", recs)


def _noise(N, B, V, seed):
    g = torch.Generator(device=_dev()).manual_seed(seed)
    noise = torch.empty(N, B, V, device=_dev())
    for j in range(N):
        noise[j].exponential_(1.0, generator=g)
    return noise


def test_kv8_t2i_generate_takes_the_position_by_position_prefix(monkeypatch):
    """generate() on a t2i model with fp8 selected, emb_masks given and LGEN_SEQ_PREFILL unset: engine.generate_iter must choose the
    position-by-position prefix by itself (the batched prefill runs the prefill kernels, which refuse fp8 slabs), fill the T prefix
    slots of every layer, and give identical tokens from the captured graph and from eager launches.  The first token (sampled
    from the prefix alone) must be the one the teacher-forced prefill logits of Transformer.__call__ give with the same noise."""
    from llamagen_amd import generate
    dev = _dev()
    monkeypatch.delenv("LGEN_SEQ_PREFILL", raising=False)
    monkeypatch.delenv("LGEN_KV_DTYPE", raising=False)
    case = dict(GPT_CASES["t2i_cfg"])
    cond, masks = make_gpt_inputs(case)
    T, V, N, B = case["kwargs"]["cls_token_num"], case["kwargs"]["vocab_size"], case["kwargs"]["block_size"], case["batch"]
    m, sd = build_gpt_holder(case)
    m = m.to(device=dev, dtype=BF)
    _set_fp8(m, SCALES_2)
    noise = _noise(N, B, V, 4321)
    kw = dict(cfg_scale=case["cfg_scale"], cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=True)
    cond_d, masks_d = cond.to(dev).to(BF), masks.to(dev)
    t_graph = generate(m, cond_d, N, emb_masks=masks_d, _noise_seq=noise, **kw).cpu()
    e = m._engine
    assert e.kv_dtype == "fp8_e4m3" and e.model_type == "t2i" and e.use_mask and len(e._graphs) == 1
    assert getattr(e, "_pf_ws", None) is None                      # the batched prefill workspace was never built
    for li in range(e.L):
        assert bool(e.k_cache[li][:, :, :T, :64].any()) and bool(e.v_cache[li][:, :, :T, :64].any()), li   # prefix slots were appended
    os.environ["LGEN_NO_GRAPH"] = "1"
    try:
        t_eager = generate(m, cond_d, N, emb_masks=masks_d, _noise_seq=noise, **kw).cpu()
    finally:
        del os.environ["LGEN_NO_GRAPH"]
    assert m._engine is e
    assert t_graph.shape == (B, N) and int(t_graph.min()) >= 0 and int(t_graph.max()) < V
    assert torch.equal(t_graph, t_eager), int((t_graph != t_eager).sum())
    # first token: from the teacher-forced prefill logits of __call__ (the path leg (c) holds to the oracle), same masks, same noise
    m.setup_caches(2 * B, T + N, BF)
    em = torch.cat([masks_d, masks_d])
    cm = m.causal_mask
    cm[:, :, :T] = cm[:, :, :T] & (em.unsqueeze(1) != 0)
    cm |= torch.eye(cm.size(1), dtype=torch.bool, device=dev)
    cond_c = torch.cat([cond_d, torch.zeros_like(cond_d) + sd["cls_embedding.uncond_embedding"].to(dev).to(BF)])
    lg, _ = m(None, cond_c, torch.arange(0, T, device=dev))
    first = O.sample(O.cfg_mix(lg[:, -1].float().cpu(), kw["cfg_scale"]), temperature=1.0, top_k=100, top_p=1.0, sample_logits=True,
                     noise=noise[0].cpu())[0].reshape(-1)
    assert torch.equal(first.to(torch.int32), t_graph[:, 0].to(torch.int32)), (first.tolist(), t_graph[:, 0].tolist())


@pytest.mark.parametrize("leg,B", [("a", 3), ("b", 128)])
def test_kv8_graph_replay_equals_eager(leg, B):
    """24 free-running tokens from injected noise: the captured decode graph and eager launches (LGEN_NO_GRAPH=1) must give
    identical tokens under fp8 too (6 rows; 256 rows = tile wqkv + persistent attention)."""
    from llamagen_amd import generate
    dev = _dev()
    case = LEG_A if leg == "a" else LEG_B
    m, _ = build_gpt_holder(case)
    m = m.to(device=dev, dtype=BF)
    _set_fp8(m, SCALES_2)
    N, V = 24, case["kwargs"]["vocab_size"]
    cond = torch.randint(0, case["kwargs"]["num_classes"], (B,), generator=torch.Generator().manual_seed(8)).to(dev)
    noise = _noise(N, B, V, 1234)
    kw = dict(cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=True)
    assert os.environ.get("LGEN_NO_GRAPH") is None
    t_graph = generate(m, cond, N, _noise_seq=noise, **kw).cpu()
    e = m._engine
    assert e.kv_dtype == "fp8_e4m3" and len(e._graphs) == 1 and e.MTs == (1 if leg == "a" else 16)
    os.environ["LGEN_NO_GRAPH"] = "1"
    try:
        t_eager = generate(m, cond, N, _noise_seq=noise, **kw).cpu()
    finally:
        del os.environ["LGEN_NO_GRAPH"]
    assert m._engine is e
    assert t_graph.shape == (B, N) and int(t_graph.min()) >= 0 and int(t_graph.max()) < V
    assert torch.equal(t_graph, t_eager), int((t_graph != t_eager).sum())
    assert len(torch.unique(t_graph)) > 20


def test_kv8_switching_formats_rebuilds_the_engine_and_scales_from_caches():
    """bf16 -> fp8 -> bf16 on one model: runs 1 and 3 give identical tokens, every switch (and a change of scales) builds a new
    engine -- no graph or slab is reused across formats; kv_scales_from_caches after the bf16 run returns powers of two
    >= headroom * amax / 448."""
    import math
    from llamagen_amd import generate, kv_scales_from_caches
    dev = _dev()
    m, _ = build_gpt_holder(LEG_A)
    m = m.to(device=dev, dtype=BF)
    B, N, V = 3, 24, 1024
    cond = torch.tensor([1, 7, 3], device=dev)
    noise = _noise(N, B, V, 99)
    kw = dict(cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=True)
    t1 = generate(m, cond, N, _noise_seq=noise, **kw).cpu()
    e1 = m._engine
    assert e1.kv_dtype is None and e1.k_cache.dtype == BF
    ks, vs = kv_scales_from_caches(m, headroom=2.0)
    assert len(ks) == len(vs) == 2
    n = N   # slots 0 .. N - 1 were written (the last token is sampled, not fed)
    for li in range(2):
        for s, slab in ((ks[li], e1.k_cache[li]), (vs[li], e1.v_cache[li])):
            amax = float(slab[:, :, :n, :64].float().abs().max())
            assert amax > 0 and math.log2(s) == int(math.log2(s)) and 2.0 * amax / 448 <= s < 4.0 * amax / 448, (li, s, amax)
    m.set_kv_cache("fp8_e4m3", ks, vs)
    with pytest.raises(RuntimeError):
        m.setup_caches(2 * B, 1 + N, BF) or kv_scales_from_caches(m)   # the helper reads storage-dtype caches only
    t2 = generate(m, cond, N, _noise_seq=noise, **kw).cpu()
    e2 = m._engine
    assert e2 is not e1 and e2.kv_dtype == "fp8_e4m3" and e2.k_cache.dtype == torch.uint8 and e2.k_scales == tuple(ks)
    assert m.layers[1].attention.kv_cache.v_cache.dtype == torch.uint8
    assert e2._k_flat.numel() * 2 < e1._k_flat.numel() * e1._k_flat.element_size() + 256   # half the KV bytes
    assert t2.shape == t1.shape and int(t2.min()) >= 0 and int(t2.max()) < V
    generate(m, cond, N, _noise_seq=noise, **kw)
    assert m._engine is e2 and len(e2._graphs) == 1                                       # same setting: engine and graph reused
    m.set_kv_cache("fp8_e4m3", [2 * k for k in ks], vs)                                   # the scales are launch constants
    generate(m, cond, N, _noise_seq=noise, **kw)
    assert m._engine is not e2
    m.set_kv_cache(None)
    t3 = generate(m, cond, N, _noise_seq=noise, **kw).cpu()
    assert m._engine.kv_dtype is None and m._engine.k_cache.dtype == BF
    assert torch.equal(t1, t3)


def test_kv8_refusals_on_the_device(monkeypatch):
    """head_dim 100, fp32 storage, score() and the continuous batcher each raise NotImplementedError before anything is launched
    (no engine is built)."""
    from llamagen_amd import generate, score
    from llamagen_amd.serve import ContinuousBatcher
    dev = _dev()
    monkeypatch.delenv("LGEN_KV_DTYPE", raising=False)
    hd100 = dict(kwargs=GPT_CASES["hd100_cfg4"]["kwargs"], wseed=1, lin_std=0.05)
    m, _ = build_gpt_holder(hd100)
    m = m.to(device=dev, dtype=BF)
    with pytest.raises(NotImplementedError, match="head_dim 100"):
        m.set_kv_cache("fp8_e4m3")
    monkeypatch.setenv("LGEN_KV_DTYPE", "fp8_e4m3")           # the environment route reaches the engine's own check
    with pytest.raises(NotImplementedError, match="head_dim 100"):
        generate(m, torch.tensor([1, 2], device=dev), 8, cfg_scale=4.0)
    assert m._engine is None
    monkeypatch.delenv("LGEN_KV_DTYPE")
    m32, _ = build_gpt_holder(LEG_A)
    m32 = m32.to(device=dev, dtype=torch.float32)
    m32.set_kv_cache("fp8_e4m3")
    with pytest.raises(NotImplementedError, match="bf16 storage only"):
        generate(m32, torch.tensor([1, 2], device=dev), 8, cfg_scale=4.0)
    assert m32._engine is None
    mb, _ = build_gpt_holder(LEG_A)
    mb = mb.to(device=dev, dtype=BF)
    mb.set_kv_cache("fp8_e4m3", 0.5, 2.0)
    with pytest.raises(NotImplementedError, match="set_kv_cache"):
        score(mb, torch.tensor([1, 2], device=dev), torch.zeros(2, 8, dtype=torch.long, device=dev), cfg_scale=4.0)
    with pytest.raises(NotImplementedError, match="set_kv_cache"):
        ContinuousBatcher(mb, 4, 16, cfg_scale=4.0)
    with pytest.raises(NotImplementedError, match="set_kv_cache"):
        mb(torch.zeros(2, 4, dtype=torch.long, device=dev), torch.tensor([1, 2], device=dev))
    assert mb._engine is None
    # and the option itself still works on that model afterwards
    toks = generate(mb, torch.tensor([1, 2], device=dev), 8, cfg_scale=4.0, top_k=100)
    assert toks.shape == (2, 8) and mb._engine.kv_dtype == "fp8_e4m3"
