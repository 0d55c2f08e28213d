"""VQEngine: launch sequence of the VQ-VAE decode path (and codebook argmin) on the HIP library.

Follows VQModel.decode_code -> decode -> Decoder.forward of the reference
(tokenizer/tokenizer_image/vq_model.py:47-55, 173-194): codebook gather + post_quant_conv, conv_in,
mid (Res, Attn, Res), the up-sampling levels, norm_out/swish/conv_out.  Activations are NHWC fp32 in
HBM; every convolution / bmm is `lgen_conv_igemm` (MFMA, hi/lo-split bf16 operands); GroupNorm is a
statistics pass + a fused apply/swish/split pass.  torch is used for buffers and the one-time weight
re-layout only.
"""
from __future__ import annotations

import os
from collections import namedtuple
from functools import partial

import torch

from . import _lib as L


def _split_planes(w: torch.Tensor):
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return hi.contiguous(), lo.contiguous()


class _ConvW:
    """[Cout, Cin, k, k] fp32 -> (hi, lo) bf16 planes [k*k][Npad][Cin] + fp32 bias."""

    def __init__(self, conv):
        w = conv.weight.detach().float()
        cout, cin, k, _ = w.shape
        blk = 128 if cout >= 128 else (64 if cout >= 64 else 16)
        npad = (cout + blk - 1) // blk * blk
        cpad = (cin + 31) // 32 * 32  # the igemm K-step is 32 input channels (RGB conv_in: 3 -> 32, zero weights)
        wt = torch.zeros(k * k, npad, cpad, device=w.device)
        wt[:, :cout, :cin] = w.permute(2, 3, 0, 1).reshape(k * k, cout, cin)
        self.hi, self.lo = _split_planes(wt)
        self.bias = conv.bias.detach().float().contiguous()
        self.cin, self.cout, self.npad, self.k = cpad, cout, npad, k
        # fragment-packed copy for lgen_conv_fused: [Npad/BN][Cin/32][taps][hi|lo][BN/16][4 g][16 r][8] -- one 1 KiB
        # block is one MFMA A fragment (lane = g*16 + r holds output channel r, input channels g*8..g*8+7)
        bn = 128 if cout >= 128 else (64 if cout > 16 else 16)
        self.fnpad = (cout + bn - 1) // bn * bn
        wf = torch.zeros(k * k, self.fnpad, cpad, device=w.device)
        wf[:, :cout, :cin] = wt[:, :cout, :cin]
        fh, fl = _split_planes(wf)
        pk = lambda q: q.view(k * k, self.fnpad // bn, bn // 16, 16, cpad // 32, 4, 8).permute(1, 4, 0, 2, 5, 3, 6)
        self.frag = torch.stack([pk(fh), pk(fl)], dim=3).contiguous()  # [nb][kc][tap][plane][j][g][r][8]
        self.bn = bn


class _GNW:
    def __init__(self, gn):
        self.gamma = gn.weight.detach().float().contiguous()
        self.beta = gn.bias.detach().float().contiguous()
        self.eps = gn.eps


class _Act:
    """An NHWC fp32 activation plus, when a fused conv produced it, the per-tile (sum, M2) partials of its values
    (the next GroupNorm's statistics without another pass over the tensor) and the width of the map they tile."""
    __slots__ = ("t", "part", "ntiles", "qstride", "width")

    def __init__(self, t, part=None, ntiles=0, qstride=0, width=0):
        self.t, self.part, self.ntiles, self.qstride, self.width = t, part, ntiles, qstride, width


# The input of the convs that produce one B x H x W map, prepared for the kernel family that will run them: for lgen_conv_fused
# the activation x with the GroupNorm (scale, shift) and the swish flag it applies on the tile load (planes is None), for
# lgen_conv_igemm the normalised / activated (hi, lo) bf16 planes.
_Prep = namedtuple("_Prep", "B H W resample x coef swish planes", defaults=(None, None, False, None))


def _res_w(r):
    return dict(n1=_GNW(r.norm1), c1=_ConvW(r.conv1), n2=_GNW(r.norm2), c2=_ConvW(r.conv2),
                nin=_ConvW(r.nin_shortcut) if hasattr(r, "nin_shortcut") else None)


def _att_w(a):
    return dict(n=_GNW(a.norm), q=_ConvW(a.q), k=_ConvW(a.k), v=_ConvW(a.v), p=_ConvW(a.proj_out))


def _level_w(res, attn, resample=None):
    """One resolution level: its ResBlocks, the AttnBlock that follows res[i] where there is one, its Upsample / Downsample conv.
    The mid block (Res, Attn, Res) is such a level too: two ResBlocks, an AttnBlock after the first, no resampling."""
    return dict(res=[_res_w(r) for r in res], attn=[_att_w(a) for a in attn],
                conv=_ConvW(resample.conv) if resample is not None else None)


class VQEngine:
    def __init__(self, model):
        self.lib = L.lib()
        if os.environ.get("LGEN_VQ_NT") is not None:  # tuning knob, see lgen_debug_set_vq_nt in lgen.h
            self.lib.lgen_debug_set_vq_nt(int(os.environ["LGEN_VQ_NT"]))
        self.dev = model.post_quant_conv.weight.device
        self.fused = os.environ.get("LGEN_VQ_FUSED", "1") != "0"  # lgen_conv_fused where the shape allows it
        if os.environ.get("LGEN_CF_VARIANT") is not None:  # tuning knob, see lgen_debug_set_conv_fused_variant in lgen.h
            self.lib.lgen_debug_set_conv_fused_variant(int(os.environ["LGEN_CF_VARIANT"]))
        cfg = model.config
        self.n_e, self.e_dim, self.l2, self.zc = cfg.codebook_size, cfg.codebook_embed_dim, cfg.codebook_l2_norm, cfg.z_channels
        self._sig_v = self._sig(model)
        dec = model.decoder
        self.conv_in = _ConvW(dec.conv_in)
        self.levels = [_level_w([dec.mid[0], dec.mid[2]], [dec.mid[1]])]
        self.levels += [_level_w(blk.res, blk.attn, getattr(blk, "upsample", None)) for blk in dec.conv_blocks]
        self.norm_out, self.conv_out = _GNW(dec.norm_out), _ConvW(dec.conv_out)
        # post_quant_conv 1x1 (Cin = e_dim): handled by the gather kernel
        self.pq_w = model.post_quant_conv.weight.detach().float().reshape(self.zc, self.e_dim).contiguous()
        self.pq_b = model.post_quant_conv.bias.detach().float().contiguous()
        cb = model.quantize.embedding.weight.detach().float().contiguous()
        self.cbn = torch.empty_like(cb)
        self.esq = torch.empty(self.n_e, device=self.dev)
        L.check(self.lib.lgen_vq_codebook_prep(L.ptr(cb), L.ptr(self.cbn), L.ptr(self.esq), self.n_e, self.e_dim,
                                               1 if self.l2 else 0, L.stream()), "codebook_prep")
        self._cb = cb
        self._enc = None
        self._model_ref = model
        # weight planes / codebook prep were enqueued on the constructing stream; lanes use this engine from their own
        # streams without an event dependency, so finish the one-time setup here
        if self.dev.type == "cuda":
            torch.cuda.current_stream(self.dev).synchronize()

    @staticmethod
    def _sig(model):
        return tuple((p.data_ptr(), p._version) for p in model.parameters())

    def compatible(self, model) -> bool:
        return self._sig_v == self._sig(model) and self.dev == model.post_quant_conv.weight.device

    # ---- primitive launches ----------------------------------------------------------------
    def _stats(self, x, B, hw, C, eps):
        nchunk = max(1, min((hw + 63) // 64, max(1, 2048 // max(B, 1))))
        ws = torch.empty(B * nchunk * 64, dtype=torch.float64, device=self.dev)
        st = torch.empty(B, 32, 2, dtype=torch.float32, device=self.dev)
        L.check(self.lib.lgen_gn_stats(L.ptr(x), L.ptr(ws), L.ptr(st), B, hw, C, eps, nchunk, L.stream()), "gn_stats")
        return st

    def _split(self, x, B, hw, C, gn=None, swish=False, slack_rows=0):
        n = B * hw * C + slack_rows * C
        hi = torch.empty(n, dtype=torch.bfloat16, device=self.dev)
        lo = torch.empty(n, dtype=torch.bfloat16, device=self.dev)
        mode = (1 if gn is not None else 0) | (2 if swish else 0)
        st = self._stats(x, B, hw, C, gn.eps) if gn is not None else None
        L.check(self.lib.lgen_gn_swish_split(L.ptr(x), L.ptr(st), L.ptr(gn.gamma) if gn else 0, L.ptr(gn.beta) if gn else 0,
                                             L.ptr(hi), L.ptr(lo), B, hw, C, mode, L.stream()), "gn_swish_split")
        return hi, lo

    @staticmethod
    def _fusable(H, W):
        return H % 8 == 0 and W >= 8   # tiles are 8 x 16 pixels; a last tile column may be partly outside the map (24-wide maps)

    def _coef(self, x: _Act, gn: _GNW, B, hw, C):
        """Per-channel (scale, shift) of GroupNorm `gn` on activation x: from the producer's tile partials when it has them,
        else from a statistics pass."""
        coef = torch.empty(B * C * 2, dtype=torch.float32, device=self.dev)
        st = self._stats(x.t, B, hw, C, gn.eps) if x.part is None else None  # then x.ntiles, x.qstride and x.width are 0
        L.check(self.lib.lgen_gn_finalize(L.ptr(x.part), L.ptr(st), L.ptr(gn.gamma), L.ptr(gn.beta), L.ptr(coef), B, C, x.ntiles,
                                          x.qstride, hw, x.width, gn.eps, L.stream()), "gn_finalize")
        return coef

    # ---- conv dispatch: lgen_conv_fused (GroupNorm-apply / swish / split on the tile load, statistics in the epilogue) where the
    # ---- shape allows it, else a split pass + lgen_conv_igemm; chosen in _prep and nowhere else ---------------------------------
    def _prep(self, x: _Act, C, B, H, W, gn=None, swish=False, resample=0) -> _Prep:
        """Prepare x (C channels, optionally through GroupNorm `gn` and swish) as the input of convs with OUTPUT size H x W.
        resample: 0 none / 1 nearest-2x input / 2 stride-2 Downsample conv, which the fused kernel does not have."""
        hw = H * W // 4 if resample == 1 else (H * W * 4 if resample == 2 else H * W)  # the INPUT map
        if self.fused and resample != 2 and self._fusable(H, W):
            return _Prep(B, H, W, resample, x=x, coef=self._coef(x, gn, B, hw, C) if gn is not None else None, swish=swish)
        return _Prep(B, H, W, resample, planes=self._split(x.t, B, hw, C, gn, swish))

    def _run(self, pre: _Prep, cw: _ConvW, res: _Act = None, out_nchw=False, want_part=True) -> _Act:
        """Conv `cw` (+ bias, + res) on a prepared input.  want_part: also write the tile partials of the result for the next
        GroupNorm -- the fused kernel only; the implicit-GEMM result never carries any."""
        B, H, W = pre.B, pre.H, pre.W
        out = torch.empty(B * H * W * cw.cout, dtype=torch.float32, device=self.dev)
        rp = L.ptr(res.t) if res is not None else 0
        if pre.planes is not None:
            L.check(self.lib.lgen_conv_igemm(L.ptr(pre.planes[0]), L.ptr(pre.planes[1]), L.ptr(cw.hi), L.ptr(cw.lo), L.ptr(cw.bias),
                                             rp, L.ptr(out), B, H, W, cw.cin, cw.cout, cw.npad, cw.k, pre.resample,
                                             1 if out_nchw else 0, 0, 1.0, L.stream()), "conv_igemm")
            return _Act(out)
        ntiles = (H // 8) * ((W + 15) // 16)
        part = torch.empty(B * ntiles * (cw.fnpad // 4) * 2, dtype=torch.float32, device=self.dev) if want_part else None
        L.check(self.lib.lgen_conv_fused(L.ptr(pre.x.t), L.ptr(pre.coef), 1 if pre.swish else 0, L.ptr(cw.frag), L.ptr(cw.bias), rp,
                                         L.ptr(out), L.ptr(part), B, H, W, cw.cin, cw.cout, cw.fnpad, cw.k, pre.resample,
                                         1 if out_nchw else 0, L.stream()), "conv_fused")
        return _Act(out, part, ntiles, cw.fnpad // 4, W) if want_part else _Act(out)

    def _conv(self, x: _Act, cw: _ConvW, B, H, W, gn=None, swish=False, resample=0, **kw) -> _Act:
        """_prep + _run for an input with one consumer; H, W = OUTPUT size."""
        return self._run(self._prep(x, cw.cin, B, H, W, gn, swish, resample), cw, **kw)

    def _gemm_nt(self, a_planes, b_planes, B, M, N, K, npad, alpha):
        """out[b] = alpha * A[b] (M x K) . Bm[b] (N x K)^T, batched, via the igemm kernel (1x1, W = 1)."""
        out = torch.empty(B * M * N, dtype=torch.float32, device=self.dev)
        L.check(self.lib.lgen_conv_igemm(L.ptr(a_planes[0]), L.ptr(a_planes[1]), L.ptr(b_planes[0]), L.ptr(b_planes[1]), 0, 0,
                                         L.ptr(out), B, M, 1, K, N, npad, 1, 0, 0, N * K, float(alpha), L.stream()), "gemm_nt")
        return out

    # ---- blocks (vq_model.py:299-314, 327-351) ----------------------------------------------
    def _res(self, x: _Act, p, B, H, W) -> _Act:
        h = self._conv(x, p["c1"], B, H, W, gn=p["n1"], swish=True)
        skip = x if p["nin"] is None else self._conv(x, p["nin"], B, H, W, want_part=False)
        return self._run(self._prep(h, p["c1"].cout, B, H, W, p["n2"], True), p["c2"], res=skip)

    def _attn(self, x: _Act, p, B, H, W) -> _Act:
        hw, c = H * W, p["q"].cin
        hn = self._prep(x, c, B, H, W, gn=p["n"])  # GroupNorm once for the three 1x1 convs (no activation, vq_model.py:330-334)
        q, k, v = [self._run(hn, p[n], want_part=False).t for n in "qkv"]
        blk = 128 if hw % 128 == 0 else (64 if hw % 64 == 0 else 16)
        npad = (hw + blk - 1) // blk * blk
        ld = (hw + 31) // 32 * 32
        qs = self._split(q, B, hw, c)
        ks = self._split(k, B, hw, c, slack_rows=npad)           # rows past hw of the last image are never stored
        s = self._gemm_nt(qs, ks, B, hw, hw, c, npad, float(int(c) ** (-0.5)))
        ph = torch.empty(B * hw * ld, dtype=torch.bfloat16, device=self.dev)
        pl = torch.empty_like(ph)
        L.check(self.lib.lgen_softmax_split(L.ptr(s), L.ptr(ph), L.ptr(pl), B * hw, hw, ld, L.stream()), "softmax_split")
        vh = torch.empty(B * c * ld, dtype=torch.bfloat16, device=self.dev)
        vl = torch.empty_like(vh)
        L.check(self.lib.lgen_split_t(L.ptr(v), L.ptr(vh), L.ptr(vl), B, hw, c, ld, L.stream()), "split_t")
        cblk = 128 if c % 128 == 0 else (64 if c % 64 == 0 else 16)
        o = self._gemm_nt((ph, pl), (vh, vl), B, hw, c, ld, (c + cblk - 1) // cblk * cblk, 1.0)
        return self._conv(_Act(o), p["p"], B, H, W, res=x)  # proj_out + skip (fused: with the statistics for the next norm1)

    def _blocks(self, levels, H, W, resample):
        """The level loop of the decoder (vq_model.py:180-191) and the encoder (:111-122): every block of `levels` in order as
        (method, weights, H, W of its output), each level's Upsample (resample 1) / Downsample (2) conv included.  The caller runs
        `x = method(x, weights, B, H, W)` itself: a frame here that held a level's input while its blocks run would keep one more
        full-resolution map alive at the last decoder level."""
        for lv in levels:
            for bi, rp in enumerate(lv["res"]):
                yield self._res, rp, H, W
                if bi < len(lv["attn"]):
                    yield self._attn, lv["attn"][bi], H, W
            if lv["conv"] is not None:  # Downsample is the stride-2 conv (vq_model.py:389-393): always the implicit-GEMM path
                H, W = (2 * H, 2 * W) if resample == 1 else (H // 2, W // 2)
                yield partial(self._conv, resample=resample), lv["conv"], H, W

    # ---- public ----------------------------------------------------------------------------------
    def decode_code(self, code_b, shape, channel_first=True):
        if shape is None:
            raise ValueError("decode_code needs shape=[B, C, h, w] (vq_model.py:52-55)")
        if channel_first:
            B, C, h, w = [int(v) for v in shape]
        else:
            B, h, w, C = [int(v) for v in shape]
        idx = code_b.reshape(-1).to(device=self.dev, dtype=torch.int64).contiguous()
        if idx.numel() != B * h * w or C != self.e_dim:
            raise ValueError(f"code_b has {idx.numel()} ids, shape {shape} expects {B * h * w} x {self.e_dim}")
        return self._decoder(self._pqconv(self.cbn, idx, self.n_e, self.e_dim, "lookup_pqconv"), B, h, w)

    def decode(self, quant):
        """quant: fp32 [B, e_dim, h, w] (already-quantised latents) -> post_quant_conv -> Decoder."""
        B, C, h, w = quant.shape
        zz = quant.to(self.dev, torch.float32).permute(0, 2, 3, 1).reshape(-1, C).contiguous()  # per-pixel "codebook"
        idx = torch.arange(B * h * w, dtype=torch.int64, device=self.dev)
        return self._decoder(self._pqconv(zz, idx, B * h * w, C, "pqconv"), B, h, w)

    def _pqconv(self, table, idx, n_e, e_dim, what) -> _Act:
        """post_quant_conv of rows idx of table [n_e][e_dim] -> NHWC [idx.numel() * z_channels]."""
        z = torch.empty(idx.numel() * self.zc, dtype=torch.float32, device=self.dev)
        L.check(self.lib.lgen_vq_lookup_pqconv(L.ptr(table), L.ptr(idx), L.ptr(self.pq_w), L.ptr(self.pq_b), L.ptr(z), idx.numel(),
                                               n_e, e_dim, self.zc, L.stream()), what)
        return _Act(z)

    def _decoder(self, z: _Act, B, H, W):
        """Decoder.forward, vq_model.py:173-194; z NHWC [B*H*W*z_channels]."""
        x = self._conv(z, self.conv_in, B, H, W)
        for block, p, H, W in self._blocks(self.levels, H, W, 1):  # mid, then the up-sampling levels
            x = block(x, p, B, H, W)
        out = self._conv(x, self.conv_out, B, H, W, gn=self.norm_out, swish=True, out_nchw=True, want_part=False)
        return out.t.view(B, self.conv_out.cout, H, W)

    def argmin(self, z):
        """Nearest codebook entry per latent vector (vq_model.py:215-232): z [B, e_dim, h, w] -> int64 [B*h*w]."""
        B, C, h, w = z.shape
        zc = z.to(self.dev, torch.float32).contiguous()
        out = torch.empty(B * h * w, dtype=torch.int64, device=self.dev)
        L.check(self.lib.lgen_vq_argmin(L.ptr(zc), L.ptr(self.cbn), L.ptr(self.esq), L.ptr(out), B * h * w, h * w, self.n_e, C,
                                        1 if self.l2 else 0, L.stream()), "vq_argmin")
        return out

    # ---- encoder (vq_model.py:64-124, 41-45) ----------------------------------------------------------
    def _encoder_weights(self):
        if self._enc is None:
            model, enc = self._model_ref, self._model_ref.encoder
            levels = [_level_w(blk.res, blk.attn, getattr(blk, "downsample", None)) for blk in enc.conv_blocks]
            self._enc = dict(conv_in=_ConvW(enc.conv_in), levels=levels + [_level_w([enc.mid[0], enc.mid[2]], [enc.mid[1]])],
                             norm_out=_GNW(enc.norm_out), conv_out=_ConvW(enc.conv_out), quant=_ConvW(model.quant_conv))
        return self._enc

    def encode(self, x):
        """VQModel.encode (eval): x fp32 [B, 3, H, W] -> (quant [B, e_dim, h, w], (None, None, None, 0),
        (None, None, indices int64 [B*h*w])) like vq_model.py:41-45 / 254-259 with self.training False."""
        E = self._encoder_weights()
        B, Cx, H, W = x.shape
        down = sum(lv["conv"] is not None for lv in E["levels"])
        if H % (1 << down) or W % (1 << down):
            raise ValueError(f"image size {H}x{W} must be a multiple of {1 << down}")
        xp = torch.zeros(B, H, W, E["conv_in"].cin, dtype=torch.float32, device=self.dev)  # NHWC, RGB padded to one 32-wide K-step
        xp[..., :Cx] = x.to(self.dev, torch.float32).permute(0, 2, 3, 1)
        h = self._conv(_Act(xp.reshape(-1)), E["conv_in"], B, H, W)
        for block, p, H, W in self._blocks(E["levels"], H, W, 2):  # the down-sampling levels, then mid
            h = block(h, p, B, H, W)
        h = self._conv(h, E["conv_out"], B, H, W, gn=E["norm_out"], swish=True, want_part=False)
        z = self._conv(h, E["quant"], B, H, W, out_nchw=True, want_part=False).t.view(B, self.e_dim, H, W)
        idx = self.argmin(z)
        emb = self.cbn if self.l2 else self._cb
        quant = emb[idx].view(B, H, W, self.e_dim).permute(0, 3, 1, 2).contiguous()  # gather of codebook rows (no arithmetic)
        self.last_latent = z
        return quant, (None, None, None, 0), (None, None, idx)
