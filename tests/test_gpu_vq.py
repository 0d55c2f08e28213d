"""GPU parity tests of the VQ tokenizer path (decode_code, codebook argmin) against the CPU oracle
and the reference-made goldens.  Tolerance: decoded pixels within 1e-3 abs (BASELINE.json north_star);
argmin indices bit-exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import llamagen_oracle as O  # noqa: E402
from tests.cases import VQ_CASES, make_vq_inputs  # noqa: E402
from tests.util import build_vq_holder, load_golden  # noqa: E402


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _L():
    from llamagen_amd import _lib
    return _lib


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _planes(x, dev):
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi.to(dev).contiguous(), lo.to(dev).contiguous()


@pytest.mark.parametrize("B,H,W,C", [(2, 4, 4, 128), (3, 24, 24, 512), (1, 48, 40, 256)])
def test_gn_stats_and_split(B, H, W, C):
    L, dev = _L(), _dev()
    x = _rand((B, H, W, C), 1) * 2 + 0.5
    gamma, beta = 1 + 0.1 * _rand((C,), 2), 0.1 * _rand((C,), 3)
    xd = x.to(dev).contiguous()
    hw = H * W
    nchunk = 7
    ws = torch.empty(B * nchunk * 64, dtype=torch.float64, device=dev)
    st = torch.empty(B, 32, 2, device=dev)
    L.check(L.lib().lgen_gn_stats(L.ptr(xd), L.ptr(ws), L.ptr(st), B, hw, C, 1e-6, nchunk, L.stream()), "stats")
    xg = x.permute(0, 3, 1, 2).reshape(B, 32, -1).double()
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    np.testing.assert_allclose(st[..., 0].cpu().numpy(), mean.float().numpy(), atol=2e-6)
    np.testing.assert_allclose(st[..., 1].cpu().numpy(), (1 / torch.sqrt(var + 1e-6)).float().numpy(), rtol=2e-6)
    hi = torch.empty(B * hw * C, dtype=torch.bfloat16, device=dev)
    lo = torch.empty_like(hi)
    g_d, b_d = gamma.to(dev), beta.to(dev)
    L.check(L.lib().lgen_gn_swish_split(L.ptr(xd), L.ptr(st), L.ptr(g_d), L.ptr(b_d), L.ptr(hi), L.ptr(lo), B, hw, C, 3,
                                        L.stream()), "split")
    ref = O.swish(O.group_norm(x.permute(0, 3, 1, 2), gamma, beta)).permute(0, 2, 3, 1).reshape(-1)
    got = hi.float().cpu() + lo.float().cpu()
    assert (got - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,ups,res,nchw", [
    (2, 4, 4, 256, 512, 3, 0, 0, 0), (1, 24, 24, 512, 512, 3, 0, 1, 0), (2, 6, 10, 128, 128, 3, 1, 0, 0),
    (1, 3, 5, 512, 256, 1, 0, 0, 0), (2, 16, 16, 128, 3, 3, 0, 0, 1), (1, 9, 7, 64, 64, 3, 0, 1, 0),
])
def test_conv_igemm_vs_fp32_conv(B, H, W, Cin, Cout, k, ups, res, nchw):
    from llamagen_amd.vq_engine import _ConvW
    L, dev = _L(), _dev()

    class Cv:  # minimal holder
        pass
    cv = Cv()
    cv.weight = (_rand((Cout, Cin, k, k), 4) / (Cin * k * k) ** 0.5).to(dev)
    cv.bias = (0.1 * _rand((Cout,), 5)).to(dev)
    cw = _ConvW(cv)
    Hs, Ws = (H // 2, W // 2) if ups else (H, W)
    x = _rand((B, Hs, Ws, Cin), 6)
    r = _rand((B, H, W, Cout), 7) if res else None
    hi, lo = _planes(x.reshape(-1), dev)
    r_d = r.to(dev).contiguous() if res else None
    out = torch.empty(B * H * W * Cout, device=dev)
    L.check(L.lib().lgen_conv_igemm(L.ptr(hi), L.ptr(lo), L.ptr(cw.hi), L.ptr(cw.lo), L.ptr(cw.bias), L.ptr(r_d), L.ptr(out),
                                    B, H, W, Cin, Cout, cw.npad, k, ups, nchw, 0, 1.0, L.stream()), "conv")
    xin = x.permute(0, 3, 1, 2)
    if ups:
        xin = xin.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    ref = F.conv2d(xin.double(), cv.weight.cpu().double(), cv.bias.cpu().double(), padding=k // 2).float()
    if res:
        ref = ref + r.permute(0, 3, 1, 2)
    got = out.cpu().view(B, Cout, H, W) if nchw else out.cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
    err = (got - ref).abs().max().item()
    assert err < 5e-5 * max(1.0, ref.abs().max().item()), err


def test_lookup_pqconv_and_argmin_edges():
    L, dev = _L(), _dev()
    case = VQ_CASES["argmin_6x6"]
    m, sd = build_vq_holder(case)
    m = m.to(dev)
    eng = m._eng()
    cb = sd["quantize.embedding.weight"]
    np.testing.assert_allclose(eng.cbn.cpu().numpy(), O.l2_normalize(cb).numpy(), atol=1e-7)
    # exact codebook hits come back as themselves; empty batch works
    zhit = O.l2_normalize(cb)[[5, 9, 16383, 0]].t().reshape(1, 8, 2, 2)
    assert m.quantize_indices(zhit.to(dev)).cpu().tolist() == [5, 9, 16383, 0]
    assert m.quantize_indices(torch.zeros(0, 8, 2, 2, device=dev)).numel() == 0


@pytest.mark.parametrize("name", [k for k, c in VQ_CASES.items() if c["kind"] == "argmin"])
def test_argmin_matches_reference_golden(name):
    case = VQ_CASES[name]
    gold = load_golden("vq_" + name)
    m, sd = build_vq_holder(case)
    m = m.to(_dev())
    z = make_vq_inputs(case)["z"]
    idx = m.quantize_indices(z.to(_dev()))
    assert idx.dtype == torch.int64
    np.testing.assert_array_equal(idx.cpu().numpy(), gold["indices"])
    np.testing.assert_array_equal(idx.cpu().numpy(), O.codebook_argmin(sd["quantize.embedding.weight"], z).numpy())


@pytest.mark.parametrize("name", [k for k, c in VQ_CASES.items() if c["kind"] == "decode"])
def test_decode_code_matches_reference_golden(name):
    """decode_code pixels within 1e-3 abs of the reference's own output (golden) and of the oracle."""
    case = VQ_CASES[name]
    gold = load_golden("vq_" + name)
    m, sd = build_vq_holder(case)
    m = m.to(_dev())
    inp = make_vq_inputs(case)
    img = m.decode_code(inp["codes"].to(_dev()), inp["shape"])
    if "image" in gold:
        assert img.dtype == torch.float32 and tuple(img.shape) == gold["image"].shape
        err = np.abs(img.cpu().numpy() - gold["image"]).max()
    else:  # BASELINE configs[1] decode shape: every 8th pixel in fp32 + the whole image as the uint8 the reference would write
        assert img.dtype == torch.float32 and tuple(img.shape) == (case["batch"], 3, 16 * case["h"], 16 * case["w"])
        err = np.abs(img[:, :, ::8, ::8].cpu().numpy() - gold["image_s8"]).max()
        u8 = O.to_uint8_hwc(img.cpu()).numpy().astype(np.int32)
        assert (np.abs(u8 - gold["uint8"].astype(np.int32)) <= 1).all() and (u8 != gold["uint8"]).mean() < 2e-3
    assert err < 1e-3, err
    ref = O.vq_decode_code(sd, inp["codes"], inp["shape"], ch_mult=tuple(m.config.decoder_ch_mult))
    assert (img.cpu() - ref).abs().max().item() < 1e-3
    print(name, "max abs pixel err vs reference golden:", err)


def test_decode_quant_path_and_larger_grid():
    """decode(quant) == decode_code(codes) and a 24x24 latent (384 px) runs and matches the oracle."""
    case = VQ_CASES["vq16_4x4"]
    m, sd = build_vq_holder(case)
    dev = _dev()
    m = m.to(dev)
    g = torch.Generator().manual_seed(5)
    codes = torch.randint(0, 16384, (1, 576), generator=g)
    img = m.decode_code(codes.to(dev), [1, 8, 24, 24])
    quant = O.get_codebook_entry(sd["quantize.embedding.weight"], codes, [1, 8, 24, 24])
    img2 = m.decode(quant.to(dev))
    assert (img - img2).abs().max().item() < 1e-5
    ref = O.vq_decode_code(sd, codes, [1, 8, 24, 24])
    err = (img.cpu() - ref).abs().max().item()
    assert tuple(img.shape) == (1, 3, 384, 384) and err < 1e-3, err


@pytest.mark.parametrize("name", [k for k, c in VQ_CASES.items() if c["kind"] == "encode"])
def test_encode_matches_reference_golden(name):
    """VQModel.encode on the HIP path (vq_model.py:41-45, 215-232; caller extract_codes_c2i.py:92-111).
    Float part: latent (quant_conv output) within 1e-3 abs of the reference.  Integer part, by a MARGIN RULE: the
    argmin over 16384 entries can only legitimately differ from the reference's where the reference's own top-2
    distance margin is smaller than what the latent difference can move a distance by (|d - d'| <= 2 |n - n'| for unit
    codebook rows, n = normalised latent); wherever the margin exceeds twice that bound the index MUST be identical,
    and the indices are always exactly the argmin of OUR latent (oracle argmin)."""
    case = VQ_CASES[name]
    gold = load_golden("vq_" + name)
    m, sd = build_vq_holder(case)
    m = m.to(_dev())
    x = make_vq_inputs(case)["x"]
    quant, losses, (_, _, idx) = m.encode(x.to(_dev()))
    z = m._engine.last_latent.cpu()
    assert tuple(z.shape) == gold["latent"].shape and idx.dtype == torch.int64 and losses == (None, None, None, 0)
    zr = torch.from_numpy(gold["latent"])
    err = (z - zr).abs().max().item()
    assert err < 1e-3, err
    cb = sd["quantize.embedding.weight"]
    np.testing.assert_array_equal(idx.cpu().numpy(), O.codebook_argmin(cb, z).numpy())
    # margin rule against the reference's indices
    e = O.l2_normalize(cb).double()
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double()
    nr, no = torch.nn.functional.normalize(flat(zr), dim=-1), torch.nn.functional.normalize(flat(z), dim=-1)
    d = (nr ** 2).sum(-1, keepdim=True) + (e ** 2).sum(-1)[None] - 2 * nr @ e.t()
    top2 = torch.topk(d, 2, dim=-1, largest=False).values
    margin = top2[:, 1] - top2[:, 0]
    bound = 2 * (no - nr).norm(dim=-1)
    same = torch.from_numpy(gold["indices"]) == idx.cpu()
    decided = margin > 2 * bound
    assert bool(same[decided].all()), ("index differs where the reference margin decides it", int((~same[decided]).sum()))
    match = same.float().mean().item()
    # measured on MI355X: every golden vector (512 of them in enc16_256) is decided by its margin and reproduced exactly
    assert decided.float().mean().item() >= 0.98 and match == 1.0, (decided.float().mean().item(), match)
    zq_ref = O.get_codebook_entry(cb, idx.cpu(), list(z.shape))
    assert (quant.cpu() - zq_ref).abs().max().item() < 1e-6
    print(name, "latent max abs err", err, "index match vs reference", match, "of", same.numel(), "decided by margin", decided.float().mean().item())


def test_conv_stride2_downsample_vs_fp32_conv():
    from llamagen_amd.vq_engine import _ConvW
    L, dev = _L(), _dev()
    B, H, W, C = 2, 6, 10, 128  # output size; input 12 x 20

    class Cv:
        pass
    cv = Cv()
    cv.weight = (_rand((C, C, 3, 3), 4) / (C * 9) ** 0.5).to(dev)
    cv.bias = (0.1 * _rand((C,), 5)).to(dev)
    cw = _ConvW(cv)
    x = _rand((B, 2 * H, 2 * W, C), 6)
    hi, lo = _planes(x.reshape(-1), dev)
    out = torch.empty(B * H * W * C, device=dev)
    L.check(L.lib().lgen_conv_igemm(L.ptr(hi), L.ptr(lo), L.ptr(cw.hi), L.ptr(cw.lo), L.ptr(cw.bias), 0, L.ptr(out),
                                    B, H, W, C, C, cw.npad, 3, 2, 0, 0, 1.0, L.stream()), "conv s2")
    xin = F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1))
    ref = F.conv2d(xin.double(), cv.weight.cpu().double(), cv.bias.cpu().double(), stride=2).float()
    got = out.cpu().view(B, H, W, C).permute(0, 3, 1, 2)
    err = (got - ref).abs().max().item()
    assert err < 5e-5 * max(1.0, ref.abs().max().item()), err


def test_encode_decode_round_trip_256px():
    """Full-size property check (no oracle at this size): encode a 256 px batch -> ids -> decode_code gives
    finite images of the input shape, ids in range, and re-encoding the reconstruction is deterministic."""
    case = VQ_CASES["vq16_4x4"]
    m, _ = build_vq_holder(case)
    dev = _dev()
    m = m.to(dev)
    x = (torch.rand(4, 3, 256, 256, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(dev)
    quant, _, (_, _, idx) = m.encode(x)
    assert tuple(quant.shape) == (4, 8, 16, 16) and idx.numel() == 4 * 256 and int(idx.min()) >= 0 and int(idx.max()) < 16384
    img = m.decode_code(idx, [4, 8, 16, 16])
    assert tuple(img.shape) == (4, 3, 256, 256) and torch.isfinite(img).all()
    assert (m.decode(quant) - img).abs().max().item() < 1e-5
    _, _, (_, _, idx2) = m.encode(x)
    assert torch.equal(idx, idx2)
    rec, diff = m(x)  # VQModel.forward (vq_model.py:57-60, eval): encode -> decode
    assert torch.equal(rec, m.decode(quant)) and diff == (None, None, None, 0)


@pytest.mark.parametrize("B,Hi,Ho", [(2, 384, 256), (1, 24, 16), (3, 20, 32), (1, 7, 7)])
def test_postprocess_resize_and_uint8(B, Hi, Ho):
    """sample_c2i_ddp.py:141-143 on the HIP path vs torch's own CPU kernels (the reference's arithmetic):
    bicubic within fp32 rounding, uint8 identical except where the float lands within rounding of an integer."""
    from llamagen_amd.postprocess import resize_bicubic, to_uint8_hwc
    dev = _dev()
    x = _rand((B, 3, Hi, Hi), 11) * 0.6
    r = resize_bicubic(x.to(dev), Ho)
    ref = F.interpolate(x, size=(Ho, Ho), mode="bicubic")
    assert (r.cpu() - ref).abs().max().item() < 2e-6 * max(1.0, ref.abs().max().item())
    u = to_uint8_hwc(x.to(dev), Ho)
    uref = O.to_uint8_hwc(ref)
    assert u.dtype == torch.uint8 and tuple(u.shape) == (B, Ho, Ho, 3)
    d = (u.cpu().int() - uref.int()).abs()
    assert d.max().item() <= 1 and (d > 0).float().mean().item() < 1e-3
    assert torch.equal(to_uint8_hwc(ref.to(dev)).cpu(), uref)  # same float input -> identical bytes


def test_postprocess_uint8_matches_reference_golden():
    """The goldens hold the reference's own uint8 HWC conversion of its decoded image."""
    from llamagen_amd.postprocess import to_uint8_hwc
    gold = load_golden("vq_vq16_4x4")
    img = torch.from_numpy(gold["image"]).to(_dev())
    assert np.array_equal(to_uint8_hwc(img).cpu().numpy(), gold["uint8"])


def test_extract_codes_flip_augmentation():
    """extract_codes_c2i.py:92-103 on the HIP encoder: ids of the image and of its horizontal flip, [B, 2, h*w]."""
    from llamagen_amd.postprocess import extract_codes
    case = VQ_CASES["enc16_32x32"]
    m, sd = build_vq_holder(case)
    dev = _dev()
    m = m.to(dev)
    x = make_vq_inputs(case)["x"].to(dev)
    codes = extract_codes(m, x)
    assert tuple(codes.shape) == (2, 2, 4) and codes.dtype == torch.int64
    gold = load_golden("vq_enc16_32x32")
    np.testing.assert_array_equal(codes[:, 0].reshape(-1).cpu().numpy(), gold["indices"])
    _, idx_f, _ = O.vq_encode(sd, torch.flip(x.cpu(), dims=[-1]))
    np.testing.assert_array_equal(codes[:, 1].reshape(-1).cpu().numpy(), idx_f.numpy())


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,ups,res,nchw,gn", [
    (2, 8, 16, 128, 128, 3, 0, 1, 0, 1), (1, 16, 32, 256, 128, 3, 0, 0, 0, 1), (2, 16, 16, 128, 128, 3, 1, 0, 0, 0),
    (1, 8, 32, 256, 128, 1, 0, 0, 0, 0), (2, 16, 16, 128, 3, 3, 0, 0, 1, 1), (1, 48, 48, 512, 256, 3, 0, 1, 0, 1),
    (1, 24, 16, 64, 256, 3, 0, 0, 0, 0),
    # W not a multiple of the 16-pixel tile width (round 3): the 24 x 24 level of a 384 px decode, a 1x1 conv, an upsampled 48 -> 24
    (2, 24, 24, 128, 128, 3, 0, 1, 0, 1), (1, 8, 24, 256, 128, 1, 0, 1, 0, 1), (1, 16, 40, 64, 128, 3, 0, 0, 0, 0),
    (1, 24, 24, 128, 3, 3, 0, 0, 1, 1), (1, 48, 24, 64, 128, 3, 1, 0, 0, 0),
])
def test_conv_fused_vs_fp32_reference(B, H, W, Cin, Cout, k, ups, res, nchw, gn):
    """lgen_conv_fused (GroupNorm-apply + swish + split on the tile load, halo tile in LDS, bias / residual / next-norm
    statistics in the epilogue) against fp64 GroupNorm -> swish -> conv2d (vq_model.py:299-314, 354-378), plus the tile
    partials -> lgen_gn_finalize -> (scale, shift) against the statistics of the stored output."""
    from llamagen_amd.vq_engine import _ConvW
    L, dev = _L(), _dev()
    lib = L.lib()

    class Cv:
        pass
    cv = Cv()
    cv.weight = (_rand((Cout, Cin, k, k), 4) / (Cin * k * k) ** 0.5).to(dev)
    cv.bias = (0.1 * _rand((Cout,), 5)).to(dev)
    cw = _ConvW(cv)
    Hs, Ws = (H // 2, W // 2) if ups else (H, W)
    x = _rand((B, Hs, Ws, Cin), 6) * 1.5 + 0.3
    r = _rand((B, H, W, Cout), 7) if res else None
    xd = x.to(dev).contiguous()
    coef = None
    xin = x.permute(0, 3, 1, 2).double()
    if gn:
        gamma, beta = 1 + 0.1 * _rand((Cin,), 8), 0.1 * _rand((Cin,), 9)
        nchunk = 3
        ws = torch.empty(B * nchunk * 64, dtype=torch.float64, device=dev)
        st = torch.empty(B, 32, 2, device=dev)
        L.check(lib.lgen_gn_stats(L.ptr(xd), L.ptr(ws), L.ptr(st), B, Hs * Ws, Cin, 1e-6, nchunk, L.stream()), "stats")
        coef = torch.empty(B, Cin, 2, device=dev)
        g_d, b_d = gamma.to(dev), beta.to(dev)
        L.check(lib.lgen_gn_finalize(0, L.ptr(st), L.ptr(g_d), L.ptr(b_d), L.ptr(coef), B, Cin, 0, 0, Hs * Ws, 0, 1e-6, L.stream()), "fin")
        xin = F.group_norm(xin, 32, gamma.double(), beta.double(), eps=1e-6)
        xin = xin * torch.sigmoid(xin)
    if ups:
        xin = xin.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    ref = F.conv2d(xin, cv.weight.cpu().double(), cv.bias.cpu().double(), padding=k // 2).float()
    if res:
        ref = ref + r.permute(0, 3, 1, 2)
    r_d = r.to(dev).contiguous() if res else None
    out = torch.full((B * H * W * Cout,), float("nan"), device=dev)
    tiles_x = (W + 15) // 16
    ntiles = (H // 8) * tiles_x
    part = torch.full((B, ntiles, cw.fnpad // 4, 2), float("nan"), device=dev)
    L.check(lib.lgen_conv_fused(L.ptr(xd), L.ptr(coef), 1 if gn else 0, L.ptr(cw.frag), L.ptr(cw.bias), L.ptr(r_d), L.ptr(out),
                                L.ptr(part), B, H, W, Cin, Cout, cw.fnpad, k, ups, nchw, L.stream()), "conv_fused")
    got = out.cpu().view(B, Cout, H, W) if nchw else out.cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()   # every pixel of the map was written (masked tile columns included)
    if k == 3 and Cout >= 128:
        # round 6: the default weight / fragment staging (variant 3: LDS-DMA + fragment reads pipelined one tap ahead) and the older forms
        # (2: hi plane ahead only, 1: all reads in front of a tap's MFMAs, 0: staging registers) accumulate every output element in the
        # same order: bit-identical outputs and statistics partials
        try:
            for v in (2, 1, 0):
                lib.lgen_debug_set_conv_fused_variant(v)
                out_v = torch.full_like(out, float("nan"))
                part_v = torch.full_like(part, float("nan"))
                L.check(lib.lgen_conv_fused(L.ptr(xd), L.ptr(coef), 1 if gn else 0, L.ptr(cw.frag), L.ptr(cw.bias), L.ptr(r_d), L.ptr(out_v),
                                            L.ptr(part_v), B, H, W, Cin, Cout, cw.fnpad, k, ups, nchw, L.stream()), f"conv_fused variant {v}")
                assert torch.equal(out_v, out), ("variant", v)
                assert torch.equal(torch.nan_to_num(part_v, nan=-7.0), torch.nan_to_num(part, nan=-7.0)), ("variant partials", v)
        finally:
            lib.lgen_debug_set_conv_fused_variant(3)
    err = (got - ref).abs().max().item()
    assert err < 6e-5 * max(1.0, ref.abs().max().item()), err
    # statistics of what was stored, per (image, tile, 4-channel quad): (sum, M2 about the tile's own mean)
    nq = (Cout + 3) // 4
    gq = torch.zeros(B, nq * 4, H, W, dtype=torch.float64)
    gq[:, :Cout] = got.double()
    pc = part.cpu().double()
    for ty in range(H // 8):
        for tx in range(tiles_x):
            blk = gq[:, :, ty * 8:ty * 8 + 8, tx * 16:min(W, tx * 16 + 16)]
            blk = blk.reshape(B, nq, 4, -1).reshape(B, nq, -1)
            S = blk.sum(-1)
            M2 = ((blk - blk.mean(-1, keepdim=True)) ** 2).sum(-1)
            np.testing.assert_allclose(pc[:, ty * tiles_x + tx, :nq, 0].numpy(), S.numpy(), rtol=1e-5, atol=1e-3)
            np.testing.assert_allclose(pc[:, ty * tiles_x + tx, :nq, 1].numpy(), M2.numpy(), rtol=1e-4, atol=1e-3)
    if Cout % 128 == 0:
        g2, b2 = (1 + 0.1 * _rand((Cout,), 10)).to(dev), (0.1 * _rand((Cout,), 11)).to(dev)
        c2 = torch.empty(B, Cout, 2, device=dev)
        L.check(lib.lgen_gn_finalize(L.ptr(part), 0, L.ptr(g2), L.ptr(b2), L.ptr(c2), B, Cout, ntiles, cw.fnpad // 4, H * W, W, 1e-6,
                                     L.stream()), "fin2")
        gg = got.reshape(B, 32, -1).double()
        mean, var = gg.mean(-1), gg.var(-1, unbiased=False)
        rstd = 1 / torch.sqrt(var + 1e-6)
        gs = Cout // 32
        sc = rstd.repeat_interleave(gs, 1) * g2.cpu().double()
        sh = b2.cpu().double() - sc * mean.repeat_interleave(gs, 1)
        np.testing.assert_allclose(c2[..., 0].cpu().numpy(), sc.float().numpy(), rtol=2e-5)
        np.testing.assert_allclose(c2[..., 1].cpu().numpy(), sh.float().numpy(), rtol=2e-5, atol=2e-5)


def test_fused_groupnorm_statistics_survive_a_large_offset():
    """ADVICE (round 2): sum / sum-of-squares partials lose the variance to cancellation when |mean| >> std.  A 1x1 convolution with
    tiny weights and a large bias stores values 60 +- 0.02; the (sum, M2) partials + Chan combine must still give the fp64
    GroupNorm coefficients (the old E[x^2] - mean^2 form is off by orders of magnitude here)."""
    from llamagen_amd.vq_engine import _ConvW
    L, dev = _L(), _dev()
    lib = L.lib()
    B, H, W, C = 2, 16, 24, 128

    class Cv:
        pass
    cv = Cv()
    cv.weight = (2e-3 * _rand((C, C, 1, 1), 14)).to(dev)
    cv.bias = (60.0 + 0.01 * _rand((C,), 15)).to(dev)
    cw = _ConvW(cv)
    x = _rand((B, H, W, C), 16)
    xd = x.to(dev).contiguous()
    out = torch.empty(B * H * W * C, device=dev)
    ntiles = (H // 8) * ((W + 15) // 16)
    part = torch.empty(B, ntiles, cw.fnpad // 4, 2, device=dev)
    L.check(lib.lgen_conv_fused(L.ptr(xd), 0, 0, L.ptr(cw.frag), L.ptr(cw.bias), 0, L.ptr(out), L.ptr(part), B, H, W, C, C, cw.fnpad,
                                1, 0, 0, L.stream()), "conv_fused")
    g2, b2 = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    c2 = torch.empty(B, C, 2, device=dev)
    L.check(lib.lgen_gn_finalize(L.ptr(part), 0, L.ptr(g2), L.ptr(b2), L.ptr(c2), B, C, ntiles, cw.fnpad // 4, H * W, W, 1e-6,
                                 L.stream()), "fin")
    gg = out.cpu().view(B, H * W, 32, C // 32).permute(0, 2, 1, 3).reshape(B, 32, -1).double()
    mean, var = gg.mean(-1), gg.var(-1, unbiased=False)
    assert (mean.abs() / var.sqrt()).min() > 500          # the regime the advice is about
    rstd = (1 / torch.sqrt(var + 1e-6)).repeat_interleave(C // 32, 1)
    np.testing.assert_allclose(c2[..., 0].cpu().numpy(), rstd.float().numpy(), rtol=2e-3)
    np.testing.assert_allclose(c2[..., 1].cpu().numpy(), (-rstd * mean.repeat_interleave(C // 32, 1)).float().numpy(), rtol=2e-3)


def test_decode_code_fused_matches_unfused(monkeypatch):
    """The fused decoder path (default) and the round-1 path (LGEN_VQ_FUSED=0: gn_stats + gn_swish_split + conv_igemm) agree to
    fp32 rounding on a 128 px image.  At an 8x8 grid every level, 8x8 included, is fused in the default mode, and the un-fused run
    is all implicit-GEMM; sequences that mix the two are covered by the golden tests of vq16_3x5 and enc16_48x32 and by the launch
    traces of tests/test_vq_engine_host.py."""
    case = VQ_CASES["vq16_4x4"]
    m, sd = build_vq_holder(case)
    dev = _dev()
    m = m.to(dev)
    codes = torch.randint(0, 16384, (2, 64), generator=torch.Generator().manual_seed(5)).to(dev)
    img = m.decode_code(codes, [2, 8, 8, 8])
    assert m._engine.fused
    monkeypatch.setenv("LGEN_VQ_FUSED", "0")
    m._engine = None
    img0 = m.decode_code(codes, [2, 8, 8, 8])
    assert not m._engine.fused
    assert (img - img0).abs().max().item() < 2e-4
    ref = O.vq_decode_code(sd, codes.cpu(), [2, 8, 8, 8])
    assert (img.cpu() - ref).abs().max().item() < 1e-3
