"""Kernel-level parity tests of the per-row-position decode path the continuous batcher runs (llamagen_amd/serve.py):
lgen_embed_rows, lgen_gemm_qkv_rope_rows and lgen_attn_decode_rows through the C ABI, each against the CPU oracle and -- where the
arithmetic of a row cannot depend on its neighbours -- bit for bit against the one-position entry point.

Every buffer a kernel writes is allocated for MTs * 16 rows and prefilled with a known pattern, so that a wrong row or slot index
lands in memory the test owns and fails a comparison.  row_pos has MTs * 16 entries; the rows in [M, MTs * 16) hold S8 - 1, a
valid slot.  The inputs come from tests/rows_cases.py, whose properties tests/test_rows_cases_host.py asserts on the CPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llamagen_oracle as O  # noqa: E402
from tests import rows_cases as RC  # noqa: E402
from tests.test_gpu_gpt import DTYPES, _close, _code, _dev, _kc, _L, _rand  # noqa: E402

STORAGE = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SENTINEL = -7.0


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ints(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


def _dev_randn(shape, dt, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g, device=dev, dtype=torch.float32).to(dt)


# ------------------------------------------------------------------------------------------------ 1. lgen_embed_rows
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,d", [(37, 256), (40, 800)])
def test_embed_rows_vs_gather(dt, M, d):
    """Rows at position 0 take cls_table[cond], the others tok_table[cur_tok]; the index a row does NOT select is stale and out
    of the table (-1 / 10**6, what the batcher leaves behind) and must not be used: the kernel clamps indices, so a stale one
    would show as row 0 or the last row of a table, which no real index here names."""
    from llamagen_amd.engine import pack_act, unpack_act
    L, dev = _L(), _dev()
    lib, code = L.lib(), _code(dt)
    TOK, CLS = 50, 11
    mts = RC.mtiles(M)
    R = mts * 16
    tok, cls = _rand((TOK, d), dt, 71), _rand((CLS, d), dt, 72)
    row_pos = torch.tensor(RC.pad_positions(RC.embed_positions(M, 61), mts, RC.S8))
    g = torch.Generator().manual_seed(73)
    tok_idx = torch.randint(1, TOK - 1, (R,), generator=g)
    cls_idx = torch.randint(1, CLS - 1, (R,), generator=g)
    first = row_pos == 0
    stale = torch.where(torch.arange(R) % 2 == 0, -1, 10 ** 6)
    cur_tok, cond = torch.where(first, stale, tok_idx), torch.where(first, cls_idx, stale)
    tok_d, cls_d = tok.to(dev), cls.to(dev)
    cur_d, cond_d, pos_d = _ints(cur_tok.tolist(), dev), _ints(cond.tolist(), dev), _ints(row_pos.tolist(), dev)
    hp = pack_act(_rand((R, d), dt, 74).to(dev), mts)                       # every element is overwritten
    ssq = torch.full((R, L.SSQ_STRIDE), float("nan"), device=dev)
    L.check(lib.lgen_embed_rows(L.ptr(tok_d), L.ptr(cls_d), L.ptr(cur_d), L.ptr(cond_d), L.ptr(pos_d), L.ptr(hp), L.ptr(ssq),
                                M, mts, d, TOK, CLS, code, L.stream()), "embed_rows")
    ref = torch.where(first[:M, None], cls[cls_idx[:M]], tok[tok_idx[:M]])
    got = unpack_act(hp, R).cpu()
    assert _same_bits(got[:M], ref)
    assert not got[M:].float().any()
    parts = d // 16
    ss = ssq.cpu()
    ss_ref = (ref.double() ** 2).reshape(M, parts, 16).sum(-1)
    # one partial = 16 squares added in fp32: relative error <= 16 * 2^-24 ~ 1e-6; the row sum to the existing embed check's rtol
    np.testing.assert_allclose(ss[:M, :parts].numpy(), ss_ref.numpy(), rtol=1e-5, atol=1e-30)
    np.testing.assert_allclose(ss[:M, :parts].sum(1).numpy(), ss_ref.sum(1).float().numpy(), rtol=1e-5)
    assert not ss[M:, :parts].any() and bool(torch.isnan(ss[:, parts:]).all())
    # lgen_embed_pack on the rows that are not at position 0: the same bits (rows at position 0 get a real index there)
    idx2 = _ints(torch.where(first, 1, tok_idx).tolist(), dev)
    hp2 = pack_act(_rand((R, d), dt, 75).to(dev), mts)
    ssq2 = torch.full((R, L.SSQ_STRIDE), float("nan"), device=dev)
    L.check(lib.lgen_embed_pack(L.ptr(tok_d), L.ptr(idx2), L.ptr(hp2), L.ptr(ssq2), 0, M, mts, d, TOK, code, L.stream()), "embed_pack")
    keep = (~first[:M]).nonzero().flatten()
    assert len(keep) >= M // 3
    assert _same_bits(unpack_act(hp2, R).cpu()[keep], got[keep])
    assert torch.equal(ssq2.cpu()[keep, :parts], ss[keep, :parts])


# ------------------------------------------------------------------------------------------------ 2. lgen_gemm_qkv_rope_rows
def _kv_storage(layout, R, H, S8, hd, hdp, dt, dev, seed):
    """Seeded-random cache storage of R rows in one of the engine's layouts -> (list of storage tensors, kv_row_stride argument)."""
    epl = 4 if dt == torch.float32 else 8
    if layout == "packed":         # rows hd rounded up to one 16-byte piece apart, hdp readable elements behind the last row
        kvs = (hd + epl - 1) // epl * epl
        n = R * H * S8 * kvs
        return [_dev_randn((n + hdp,), dt, seed, dev), _dev_randn((n + hdp,), dt, seed + 1, dev)], kvs
    if layout == "interleaved":    # K and V row of a slot adjacent
        return [_dev_randn((R, H, S8, 2, hdp), dt, seed, dev)], 2 * hdp
    return [_dev_randn((R, H, S8, hdp), dt, seed, dev), _dev_randn((R, H, S8, hdp), dt, seed + 1, dev)], 0


def _kv_views(layout, store, R, H, S8, hd, hdp, dt):
    if layout == "packed":
        kvs = (store[0].numel() - hdp) // (R * H * S8)
        return tuple(s[:R * H * S8 * kvs].view(R, H, S8, kvs) for s in store)
    if layout == "interleaved":
        return store[0][..., 0, :], store[0][..., 1, :]
    return store[0], store[1]


QKV_CASES = [
    # a: no norm, 2 waves x 4 chunks (bf16 / fp16: KCH = 8) or x 8 chunks (fp32: KCH = 16): gemm_kernel<NORM = false> -- the
    #    steady-state form needs bf16 and >= 2 * DEPTH(MT 2, NT 2) = 12 chunks per wave (launch() in gemm_skinny.hip)
    *[pytest.param(dt, 40, 256, 4, 64, (2, 2, 2), False, (1,), lay, id=f"a-{STORAGE[dt]}-{lay}")
      for dt in DTYPES for lay in ("plain", "interleaved")],
    # b: bf16, KCH = 100, 5 waves x 20 chunks >= 2 * DEPTH(MT 4, NT 1) = 10, gemm_has_steady(4, 1, QKV): gemm_steady_kernel
    pytest.param(BF16, 64, 3200, 32, 100, (4, 1, 5), False, (1,), "packed", id="b-bf16-steady"),
    # c: bf16 + norm, KCH = 32 = 8 waves x CPW 4: lgen_gemm_normpre_try -> gemm_normpre_kernel MODE 0 (passes 1) and MODE 1
    #    (passes 3; (MT 2, NT 4, QKV) has a multi-pass instantiation up to CPW 4)
    pytest.param(BF16, 40, 1024, 16, 64, (2, 4, 8), True, (1, 3), "plain", id="c-bf16-normpre"),
    # d: norm with fp16 / fp32: lgen_gemm_normpre_try is bf16 only -> dispatch_dt<QKV, NORM = true>: the ring kernel; kw = None:
    #    lgen_gemm_max_kw(EPI_QKV, fused, 2, 2)
    *[pytest.param(dt, 40, 256, 4, 64, (2, 2, None), True, (1,), "plain", id=f"d-{STORAGE[dt]}-ring-norm") for dt in (F16, F32)],
    # e: fp32, MT = 4 (one workgroup tile holds all four m-tiles, one of them all padding): gemm_kernel<F32, 4, 1, QKV, false>
    pytest.param(F32, 33, 800, 8, 100, (4, 1, 5), False, (1,), "packed", id="e-fp32-mt4"),
]


@pytest.mark.parametrize("dt,M,d,H,hd,tiles,norm,passes_list,layout", QKV_CASES)
def test_qkv_rope_rows_vs_oracle_and_scalar_entry(dt, M, d, H, hd, tiles, norm, passes_list, layout):
    """Per-row RoPE angle and cache slot across m-tiles: q row m and K/V slot row_pos[m] of cache row m against the oracle chain
    ([rms_norm ->] linear -> apply_rotary_emb at freqs[row_pos[m]] -> append), nothing else written, and bit-equality with
    lgen_gemm_qkv_rope at every position (a row's GEMM does not depend on its position, its rotation only on its own angle)."""
    from llamagen_amd.engine import pack_act, pack_weight, precompute_freqs_cis_2d
    L, dev = _L(), _dev()
    lib, code = L.lib(), _code(dt)
    S8, hdp = RC.S8, 64 if hd <= 64 else 128
    mts = RC.mtiles(M)
    R = mts * 16
    mt, nt, kw = tiles
    if kw is None:
        kw = lib.lgen_gemm_max_kw(L.EPI_QKV, 1, mt, nt)
        assert kw >= 2
    assert mt >= 2 and mts % mt == 0
    live = RC.qkv_positions(M)
    assert all(RC.qkv_position_properties(live, M, mts, mt))
    row_pos = RC.pad_positions(live, mts, S8)
    pos_t = torch.tensor(live)
    # RoPE table: the model's 1 + 24 * 24 rows, extended to S8 rows (seeded angles) so that position S8 - 1 is inside it
    ang = torch.rand(S8 - 1 - RC.GRID ** 2, hd // 2, generator=torch.Generator().manual_seed(5)) * 6.0
    freqs = torch.cat([precompute_freqs_cis_2d(RC.GRID, hd, 10000.0, 1), torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)])
    assert tuple(freqs.shape) == (S8, hd // 2, 2)
    if norm:
        x, w = _rand((M, d), dt, 41, 1.3), _rand((3 * d, d), dt, 42, 0.03)
        nw = (1 + 0.1 * _rand((d,), torch.float32, 43)).to(dt)
    else:
        x, w, nw = _rand((M, d), dt, 9), _rand((3 * d, d), dt, 10, 0.05 if d <= 1024 else 0.02), None
    wp, xp, fr_d = pack_weight(w.to(dev)), pack_act(x.to(dev), mts), freqs.to(dev)
    nw_d = ssq = None
    if norm:
        nw_d = nw.to(dev)
        ssq = torch.full((R, L.SSQ_STRIDE), float("nan"), device=dev)
        L.check(lib.lgen_ssq_pack(L.ptr(xp), L.ptr(ssq), mts, d, code, L.stream()), "ssq_pack")
    pos_d = _ints(row_pos, dev)
    prefill, kvs = _kv_storage(layout, R, H, S8, hd, hdp, dt, dev, 11)
    stride = kvs or hdp

    def launch(fn, pos_arg, passes):
        store = [p.clone() for p in prefill]
        kc, vc = _kv_views(layout, store, R, H, S8, hd, hdp, dt)
        q = torch.zeros(R, H, hdp, dtype=dt, device=dev)
        L.check(fn(L.ptr(wp), L.ptr(xp), L.ptr(q), L.ptr(kc), L.ptr(vc), L.ptr(fr_d), L.ptr(pos_arg), M, mts, d, H, hd, hdp, S8, kvs,
                   code, mt, nt, kw, L.ptr(nw_d), L.ptr(ssq), d // 16 if norm else 0, 1e-5 if norm else 0.0, passes, L.stream()), "qkv")
        torch.cuda.synchronize()
        return q, kc, vc, store

    xin = O.rms_norm(x.float(), nw, 1e-5, dt) if norm else x.float()
    qkv = O.linear(xin, w.float(), dt)
    lq, lk, lv = (t.reshape(M, H, hd) for t in qkv.split([d, d, d], dim=-1))
    fr = freqs[pos_t]
    xq = O.apply_rotary_emb(lq.reshape(1, M, H, hd), fr, dt)[0]
    xk = O.apply_rotary_emb(lk.reshape(1, M, H, hd), fr, dt)[0]
    rows = torch.arange(M, device=dev)
    slot = pos_t.to(dev)
    outs = []
    for passes in passes_list:
        q, kc, vc, store = launch(lib.lgen_gemm_qkv_rope_rows, pos_d, passes)
        k_got, v_got = kc[rows, :, slot], vc[rows, :, slot]                # [M, H, stride]: slot row_pos[m] of cache row m
        if norm:   # the bars of test_qkv_fused_norm_rope_append_vs_oracle
            _close(q[:M, :, :hd], xq, dt, "q", frac_ulp1=0.05, mag=lq)
            _close(k_got[..., :hd], xk, dt, "k row", frac_ulp1=0.05, mag=lk)
            _close(v_got[..., :hd], lv, dt, "v row", frac_ulp1=0.05)
        else:      # the bars of test_qkv_rope_append_and_attention
            _close(q[:M, :, :hd], xq, dt, "q rope", mag=lq, ulps=2.0)
            _close(k_got[..., :hd], xk, dt, "k cache", mag=lk, ulps=2.0)
            _close(v_got[..., :hd], lv, dt, "v cache")
        # nothing else was written: the caches equal the prefill outside elements [0, hd) of slot row_pos[m] of rows m < M
        expect = [p.clone() for p in prefill]
        ek, ev = _kv_views(layout, expect, R, H, S8, hd, hdp, dt)
        ek[rows, :, slot, :hd] = k_got[..., :hd]
        ev[rows, :, slot, :hd] = v_got[..., :hd]
        for s, e in zip(store, expect):
            assert _same_bits(s, e), "a cache element outside the appended rows changed"
        assert not q[M:].any() and not q[:, :, hd:].any()
        # one position for all rows (lgen_gemm_qkv_rope), same operands / tiles / passes: the rows at that position, bit for bit
        for p in RC.QKV_POSITIONS:
            state = _ints([p, 0], dev)
            q1, kc1, vc1, _ = launch(lib.lgen_gemm_qkv_rope, state, passes)
            at = (pos_t == p).nonzero().flatten().to(dev)
            assert len(at) >= M // 5
            assert _same_bits(q1[at], q[at]), ("q", p)
            assert _same_bits(kc1[at, :, p], kc[at, :, p]) and _same_bits(vc1[at, :, p], vc[at, :, p]), ("k/v", p)
        outs.append((q, store))
    for q, store in outs[1:]:      # `passes` is a scheduling choice
        assert _same_bits(q, outs[0][0]) and all(_same_bits(a, b) for a, b in zip(store, outs[0][1]))
    assert stride >= hd


# ------------------------------------------------------------------------------------------------ 3. lgen_attn_decode_rows
class _Attn:
    """q / K / V of one attention problem on the device (caches hold exactly the values the oracle gets) and its launches."""

    def __init__(self, dt, q, k, v, layout):
        self.L, self.dev, self.dt = _L(), _dev(), dt
        dev = self.dev
        B2, H, S8, hd = k.shape
        self.B2, self.H, self.S8, self.hd = B2, H, S8, hd
        self.hdp = hdp = 64 if hd <= 64 else 128
        self.mts = RC.mtiles(B2)
        if layout == "packed":
            epl = 4 if dt == torch.float32 else 8
            self.kvs = kvs = (hd + epl - 1) // epl * epl
            n = B2 * H * S8 * kvs
            self.flat = [torch.zeros(n + hdp, dtype=dt, device=dev) for _ in range(2)]
            self.kc, self.vc = (f[:n].view(B2, H, S8, kvs) for f in self.flat)
        else:
            self.kvs = 0
            self.kc, self.vc = (torch.zeros(B2, H, S8, hdp, dtype=dt, device=dev) for _ in range(2))
        self.kc[..., :hd] = k.to(dev)
        self.vc[..., :hd] = v.to(dev)
        self.q = torch.zeros(self.mts * 16, H, hdp, dtype=dt, device=dev)      # elements [hd, hdp) exact zeros (lgen.h)
        self.q[:B2, :, :hd] = q.to(dev)

    def run(self, rows, pos_d, mask_d, mask_len, variant):
        """-> (return code, output rows [MTs * 16, d]); the output buffer starts filled with SENTINEL."""
        from llamagen_amd.engine import unpack_act
        L, kcd, d = self.L, _kc(self.dt), self.H * self.hd
        out = torch.full((d // kcd, self.mts, 64, kcd // 4), SENTINEL, dtype=self.dt, device=self.dev)
        fn = L.lib().lgen_attn_decode_rows if rows else L.lib().lgen_attn_decode
        rc = fn(L.ptr(self.q), L.ptr(self.kc), L.ptr(self.vc), L.ptr(out), L.ptr(pos_d), L.ptr(mask_d), mask_len, self.B2, self.mts,
                self.H, self.hd, self.hdp, self.S8, self.kvs, _code(self.dt), variant, L.stream())
        torch.cuda.synchronize()
        return rc, unpack_act(out, self.mts * 16)

    def ok(self, rows, pos_d, mask_d, mask_len, variant):
        rc, out = self.run(rows, pos_d, mask_d, mask_len, variant)
        self.L.check(rc, f"attn variant {variant}")
        assert bool((out[self.B2:] == SENTINEL).all()), ("rows >= B2 written", variant)
        return out[:self.B2]


def _ref(q, k, v, mrow, dt):
    """oracle attention of one query per row: q [B2, H, hd], mrow [B2, S8] bool -> [B2, H * hd]"""
    B2, H, hd = q.shape
    return O.sdpa_math(q[:, :, None], k, v, mrow[:, None, None, :], dt).transpose(1, 2).reshape(B2, H * hd)


def _workgroup_variants(H):
    return [v for v in range(8) if H % RC.WORKGROUP_VARIANTS[v][2] == 0] + [-1]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("H,hd,layout", [(4, 64, "plain"), (8, 100, "packed")])
def test_attn_rows_kv_length_boundaries(dt, H, hd, layout, use_mask):
    """3a: kv lengths just below, at and above every group size and waves x group size in ONE launch (rows of very different
    length, waves with no group next to waves with several), workgroup variants 0..7 and the library's choice, vs the oracle per
    row; rows at positions 0 / 129 / S8 - 1 bit-equal to the one-position entry point; persistent variants refused."""
    B2, S8 = 40, RC.S8
    dev = _dev()
    positions = RC.attn_positions(B2, 7)
    pos_t = torch.tensor(positions)
    q, k, v = _rand((B2, H, hd), dt, 21), _rand((B2, H, S8, hd), dt, 22), _rand((B2, H, S8, hd), dt, 23)
    A = _Attn(dt, q, k, v, layout)
    pos_d = _ints(RC.pad_positions(positions, A.mts, S8), dev)
    mrow = torch.arange(S8)[None, :] <= pos_t[:, None]
    mask_d = None
    if use_mask:
        mask = RC.random_key_mask(B2, S8)
        mrow = mask[torch.arange(B2), pos_t]
        assert bool(mrow[torch.arange(B2), pos_t].all()) and not mrow[0, positions[0] + 1:].any()
        mask_d = mask.to(dev).contiguous()
    ref = _ref(q, k, v, mrow, dt)
    for variant in _workgroup_variants(H):
        got = A.ok(True, pos_d, mask_d, 0, variant)
        _close(got, ref, dt, f"attn rows mask={use_mask} variant={variant}")
        for p in RC.ATTN_CROSS_POSITIONS:   # the same kernel, the result depends on the row's own kv length only
            one = A.ok(False, _ints([p, 0], dev), mask_d, 0, variant)
            at = (pos_t == p).nonzero().flatten().to(dev)
            assert len(at) >= 1 and _same_bits(one[at], got[at]), (variant, p)
    for variant in RC.PERSISTENT_VARIANTS:  # one kv length for all rows: refused with per-row positions, nothing written
        rc, out = A.run(True, pos_d, mask_d, 0, variant)
        assert rc == A.L.ERR_UNSUPPORTED and bool((out == SENTINEL).all()), variant


@pytest.mark.parametrize("H,chosen", [(4, 6), (3, 2)])
def test_attn_rows_library_choice_at_256_rows(H, chosen):
    """3b: from 256 rows variant -1 takes two heads per workgroup (variant 6), or variant 2 for an odd head count."""
    dt, B2, hd, S8 = BF16, 256, 64, O.find_multiple(1 + 16, 8)
    dev = _dev()
    positions = RC.cycle_positions(B2, 0, 16, 3)
    assert set(positions) == set(range(17))
    pos_t = torch.tensor(positions)
    q, k, v = _rand((B2, H, hd), dt, 24), _rand((B2, H, S8, hd), dt, 25), _rand((B2, H, S8, hd), dt, 26)
    A = _Attn(dt, q, k, v, "plain")
    pos_d = _ints(RC.pad_positions(positions, A.mts, S8), dev)
    ref = _ref(q, k, v, torch.arange(S8)[None, :] <= pos_t[:, None], dt)
    got = A.ok(True, pos_d, None, 0, -1)
    _close(got, ref, dt, f"attn rows 256 x {H} heads")
    assert _same_bits(A.ok(True, pos_d, None, 0, chosen), got)   # (two heads per workgroup do not divide 3 heads: variant 2)


@pytest.mark.parametrize("dt", [BF16, F32])
def test_attn_left_padded_caption_masks_and_mask_len(dt):
    """3c: the masks generate() builds from left-padded captions hide a long LEADING run of keys (whole key groups stay at the
    sentinel before the first visible one).  mask_len = T consults the mask for the prefix keys only: the bytes of keys >= T are
    poisoned in that launch's buffer, and mask_len = 0 with the true mask must give the same bits -- per row on the workgroup
    variants, and at one position on all 15 variants (the persistent ones never saw a masked prefix or mask_len > 0 before)."""
    T, S8, H, hd = RC.CAPTION_T, RC.CAPTION_S8, 4, 64
    B2 = len(RC.CAPTION_LENS)
    dev = _dev()
    mask = RC.caption_masks()
    positions = RC.caption_positions(B2)
    pos_t = torch.tensor(positions)
    q, k, v = _rand((B2, H, hd), dt, 27), _rand((B2, H, S8, hd), dt, 28), _rand((B2, H, S8, hd), dt, 29)
    A = _Attn(dt, q, k, v, "plain")
    true_d, poisoned_d = mask.to(dev).contiguous(), RC.poison_mask_tail(mask).to(dev).contiguous()
    pos_d = _ints(RC.pad_positions(positions, A.mts, S8), dev)
    ref = _ref(q, k, v, mask[torch.arange(B2), pos_t], dt)
    for variant in _workgroup_variants(H):
        got = A.ok(True, pos_d, poisoned_d, T, variant)
        _close(got, ref, dt, f"caption mask rows variant={variant}")
        assert _same_bits(A.ok(True, pos_d, true_d, 0, variant), got), variant
    p = RC.CAPTION_SCALAR_POS
    state = _ints([p, 0], dev)
    ref1 = _ref(q, k, v, mask[:, p], dt)
    for variant in list(range(15)) + [-1]:
        got = A.ok(False, state, poisoned_d, T, variant)
        _close(got, ref1, dt, f"caption mask pos {p} variant={variant}")
        assert _same_bits(A.ok(False, state, true_d, 0, variant), got), variant


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("plant", [True, False])
def test_attn_wide_score_range(dt, plant):
    """3d: scores with a standard deviation of WIDE_S units (exp(m_run - m_new) far outside [0.05, 1]) and, with plant, one key
    per row that leads the rest by more than 30 -- in the first group, in the last, or in a wave's second round -- so that
    everything folded before it underflows after the rescale.  Bars: _close defaults; rows_cases.WIDE_S says why they hold."""
    B2, H, hd, S8 = 40, 4, 64, RC.S8
    dev = _dev()
    s = RC.WIDE_S[STORAGE[dt]]
    positions = RC.attn_positions(B2, 7)
    q, k, v, keys = RC.wide_inputs(dt, STORAGE[dt], positions, H, hd, S8, s, plant=plant)
    A = _Attn(dt, q, k, v, "plain")
    pos_d = _ints(RC.pad_positions(positions, A.mts, S8), dev)
    ref = _ref(q, k, v, RC.visible_rows(positions, S8)[:, 0, 0], dt)
    for variant in (0, 2, 5, 6):
        _close(A.ok(True, pos_d, None, 0, variant), ref, dt, f"wide scores rows variant={variant} planted={plant}")
    same = [RC.WIDE_SCALAR_POS] * B2
    q, k, v, keys = RC.wide_inputs(dt, STORAGE[dt], same, H, hd, S8, s, plant=plant)
    A = _Attn(dt, q, k, v, "plain")
    ref = _ref(q, k, v, RC.visible_rows(same, S8)[:, 0, 0], dt)
    state = _ints([RC.WIDE_SCALAR_POS, 0], dev)
    for variant in (8, 10, 13):
        _close(A.ok(False, state, None, 0, variant), ref, dt, f"wide scores pos 300 variant={variant} planted={plant}")
