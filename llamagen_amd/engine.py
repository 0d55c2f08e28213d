"""DecodeEngine: device state + launch sequence of the GPT decode loop on the HIP library.

Owns everything `Transformer.setup_caches` allocates in the reference (gpt.py:316-330) plus the
MI355X-specific state: fragment-packed weight copies, fragment-packed activation workspaces, KV
slabs [L][B2][H][S8][hd_pad], the device-side (pos, step) counters and the captured hipGraph of
one decode step (replayed N-2 times per generate()).  PyTorch is used for device memory, streams,
the Exp(1) noise draw and graph capture only -- every FLOP is a kernel of liblgen_hip.so.
"""
from __future__ import annotations

import math
import os
import weakref
from typing import Optional

import torch

from . import _lib as L
from . import gemm_schedule as S
from .given import given_prefix_length
from .gemm_schedule import MODEL_TILE_SCHEDULES, TESTED_TILE_SCHEDULES, TILE_SCHEDULES, tile_schedule_key  # noqa: F401  (the tests name them here)


def _ceil_div(a, b):
    return (a + b - 1) // b


def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """[N, K] row-major -> WP[N/16][K/KC][4 g][16 r][EPL] (one-time layout transform)."""
    N, K = w.shape
    epl = 4 if w.dtype == torch.float32 else 8
    kc = 4 * epl
    assert N % 16 == 0 and K % kc == 0, (N, K)
    return w.view(N // 16, 16, K // kc, 4, epl).permute(0, 2, 3, 1, 4).contiguous()


def pack_act(x: torch.Tensor, mts: int) -> torch.Tensor:
    """[M, K] row-major -> XP[K/KC][MTs][4 g][16 r][EPL] (rows padded with zeros)."""
    M, K = x.shape
    epl = 4 if x.dtype == torch.float32 else 8
    kc = 4 * epl
    assert K % kc == 0 and M <= mts * 16
    xp = torch.zeros(mts * 16, K, dtype=x.dtype, device=x.device)
    xp[:M] = x
    return xp.view(mts, 16, K // kc, 4, epl).permute(2, 0, 3, 1, 4).contiguous()


def unpack_act(xp: torch.Tensor, M: int) -> torch.Tensor:
    """Inverse of pack_act: XP[K/KC][MTs][4][16][EPL] -> [M, K]."""
    if xp.dim() == 4:  # [K/KC][MTs][64][EPL] workspace view
        xp = xp.view(xp.shape[0], xp.shape[1], 4, 16, xp.shape[3])
    kch, mts, g, r, epl = xp.shape
    return xp.permute(1, 3, 0, 2, 4).reshape(mts * 16, kch * g * epl)[:M].contiguous()


def precompute_freqs_cis_2d(grid_size: int, n_elem: int, base: float, cls_token_num: int) -> torch.Tensor:
    """2-D RoPE table of gpt.py:404-417 ([cls + grid^2, n_elem/2, 2] fp32, conditioning rows zero)."""
    half = n_elem // 2
    freqs = 1.0 / (base ** (torch.arange(0, half, 2)[: (half // 2)].float() / half))
    t = torch.arange(grid_size)
    freqs = torch.outer(t, freqs)
    fg = torch.concat([freqs[:, None, :].expand(-1, grid_size, -1), freqs[None, :, :].expand(grid_size, -1, -1)], dim=-1)
    cache = torch.stack([torch.cos(fg), torch.sin(fg)], dim=-1).flatten(0, 1)
    return torch.cat([torch.zeros(cls_token_num, n_elem // 2, 2), cache])


class PackedWeights:
    """MFMA-fragment-packed copies of a Transformer's parameters (see lgen.h for the layouts)."""

    def __init__(self, model, dtype, sig):
        cast = lambda p: p.detach().to(dtype)
        self.sig, self.dtype = sig, dtype
        self.layers = []
        for blk in model.layers:
            at, ff = blk.attention, blk.feed_forward
            w1p, w3p = pack_weight(cast(ff.w1.weight)), pack_weight(cast(ff.w3.weight))
            self.layers.append(dict(
                an=cast(blk.attention_norm.weight).contiguous(), fn=cast(blk.ffn_norm.weight).contiguous(),
                wqkv=pack_weight(cast(at.wqkv.weight)), wo=pack_weight(cast(at.wo.weight)),
                w13=torch.stack([w1p, w3p], dim=1).flatten(0, 1).contiguous(), w2=pack_weight(cast(ff.w2.weight))))
        self.norm_w = cast(model.norm.weight).contiguous()
        self.out_w = pack_weight(cast(model.output.weight))
        self.tok_emb = cast(model.tok_embeddings.weight).contiguous()
        if model.model_type == "c2i":
            self.cls_emb = cast(model.cls_embedding.embedding_table.weight).contiguous()
        else:
            self.fc1 = pack_weight(cast(model.cls_embedding.cap_proj.fc1.weight))
            self.fc2 = pack_weight(cast(model.cls_embedding.cap_proj.fc2.weight))
            self.cap_hidden = model.cls_embedding.cap_proj.fc1.weight.shape[0]
        # The packed copies are built by asynchronous kernels on the constructing stream and then shared by every lane
        # (other streams, no event dependency): finish them here, once, so that no lane can read a half-built copy.
        if self.tok_emb.is_cuda:
            torch.cuda.current_stream(self.tok_emb.device).synchronize()


_PACKED = weakref.WeakKeyDictionary()  # tok_embeddings module (shared by lane views) -> PackedWeights


class DecodeEngine:
    def __init__(self, model, max_batch: int, S8: int, dtype: torch.dtype, kv_dtype: Optional[str] = None, kv_scales=None):
        """kv_dtype None: K/V in the storage dtype.  "fp8_e4m3" (opt-in, Transformer.set_kv_cache): uint8 slabs of OCP e4m3fn codes,
        kv_scales = (k_scales, v_scales), one float per layer (default 1.0); bf16 storage and head_dim <= 64 only."""
        cfg = model.config
        if dtype not in (torch.bfloat16, torch.float32, torch.float16):
            raise NotImplementedError(f"the HIP engine implements --precision bf16, fp16 and none (fp32), not {dtype}")
        if kv_dtype is not None:
            if kv_dtype != "fp8_e4m3":
                raise ValueError(f"kv_dtype {kv_dtype!r}: expected None or 'fp8_e4m3'")
            if dtype != torch.bfloat16:
                raise NotImplementedError(f"fp8 KV cache: bf16 storage only, not {dtype} (the append and attention kernels read bf16 q)")
            if cfg.dim // cfg.n_head > 64:
                raise NotImplementedError(f"fp8 KV cache: head_dim {cfg.dim // cfg.n_head} > 64 has no kernels (64-byte key rows only)")
        self.kv_dtype = kv_dtype
        ks, vs = kv_scales if kv_scales is not None else (None, None)
        self.k_scales = tuple(float(x) for x in ks) if ks is not None else (1.0,) * cfg.n_layer
        self.v_scales = tuple(float(x) for x in vs) if vs is not None else (1.0,) * cfg.n_layer
        if len(self.k_scales) != cfg.n_layer or len(self.v_scales) != cfg.n_layer:
            raise ValueError("kv_scales: one (k, v) scale per layer")
        self.lib = L.lib()
        # decode-attention kernel variant: -1 = the library's choice by shape (lgen.h); LGEN_ATTN_VARIANT=n pins one (development)
        self.attn_variant = int(os.environ.get("LGEN_ATTN_VARIANT", "-1"))
        self.dev = model.tok_embeddings.weight.device
        self.dtype = dtype
        self.dt = {torch.bfloat16: L.BF16, torch.float32: L.F32, torch.float16: L.F16}[dtype]
        self.epl = 4 if dtype == torch.float32 else 8
        self.kc = 4 * self.epl
        self.B2, self.S8 = max_batch, S8
        self.L, self.H, self.d = cfg.n_layer, cfg.n_head, cfg.dim
        self.hd = cfg.dim // cfg.n_head
        self.hdp = 64 if self.hd <= 64 else 128
        if self.hd > 128 or self.hd % 4:
            raise NotImplementedError(f"head_dim {self.hd} unsupported")
        self.F = model.layers[0].feed_forward.hidden_dim
        self.V = cfg.vocab_size
        self.eps = cfg.norm_eps
        self.T = cfg.cls_token_num
        self.model_type = model.model_type
        for n in (self.d, self.F):
            if n % 32:
                raise NotImplementedError("model dims must be multiples of 32")
        if dtype != torch.float32 and self.d > 4096 and not (self.d // 32 % 8 == 0 and 3 <= self.d // 32 // 8 <= 6):
            # the stand-alone 16-bit RMSNorm kernel holds a row in registers up to 4096 columns (lgen_rmsnorm); every registry
            # model is <= 3200 wide -- say so here instead of failing in the middle of a decode chain
            raise NotImplementedError(f"dim {self.d} > 4096 with {dtype}: the stand-alone RMSNorm kernel covers 16-bit rows up to 4096 "
                                      "columns (use --precision none, or a model width the fused-norm GEMMs take)")
        if self.V % 16:
            raise NotImplementedError("vocab_size must be a multiple of 16")
        self.MTs = mts = S.round_mts(max_batch)
        dev, dt = self.dev, dtype
        z = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
        # KV slabs (gpt.py:170-185); hd padded to 64/128 so a key row is a power-of-two lane group.  Two separate
        # slabs by default; LGEN_KV_INTERLEAVE=1 puts the K and V row of a slot next to each other
        # ([.., S8, 2, hdp], row stride 2*hdp: one HBM stream per (b, h) instead of two) -- measured 1.4 % SLOWER
        # in the decode attention at kv_len 576 on MI355X, so it stays an option of the kernels' row-stride argument.
        if kv_dtype is not None:
            # fp8 slabs [L][B2][H][S8][kvs8] BYTES, kvs8 = hd rounded up to 16; zero-initialised (a zero byte is +0.0) and followed
            # by 64 readable zero bytes: the attention reads 64 bytes per key whatever the stride (the slack rule of the bf16 slabs)
            self.kvs = _ceil_div(self.hd, 16) * 16
            n = self.L * max_batch * self.H * S8 * self.kvs
            self._k_flat, self._v_flat = z(n + 64, dtype=torch.uint8), z(n + 64, dtype=torch.uint8)
            self.k_cache = self._k_flat[:n].view(self.L, max_batch, self.H, S8, self.kvs)
            self.v_cache = self._v_flat[:n].view(self.L, max_batch, self.H, S8, self.kvs)
        elif os.environ.get("LGEN_KV_INTERLEAVE") == "1":
            self.kv_slab = z(self.L, max_batch, self.H, S8, 2, self.hdp)
            self.k_cache, self.v_cache = self.kv_slab[..., 0, :], self.kv_slab[..., 1, :]
            self.kvs = 2 * self.hdp
        else:
            # Rows are packed at hd rounded up to 8 elements (one 16-byte piece), not at the lane group hdp (round 5): GPT-3B's
            # head_dim 100 -> 104 elements = 13 x 16 B per key instead of 128, i.e. 19 % fewer KV bytes for the HBM-bound decode
            # attention (the reference's own serving fork pads to 112, autoregressive/serve/gpt_model.py:208-220).  The kernels
            # still read hdp elements per key: the lanes past the row see the first bytes of the NEXT row, which meet q's zero
            # pad lanes (QK^T) or output elements >= hd that are never stored (PV); the slack behind the last row keeps those
            # reads inside the allocation (zeros: finite).  LGEN_KV_PACK=0 keeps rows of hdp elements.
            self.kvs = _ceil_div(self.hd, self.epl) * self.epl if os.environ.get("LGEN_KV_PACK", "1") != "0" else self.hdp
            n = self.L * max_batch * self.H * S8 * self.kvs
            self._k_flat, self._v_flat = z(n + self.hdp), z(n + self.hdp)
            self.k_cache = self._k_flat[:n].view(self.L, max_batch, self.H, S8, self.kvs)
            self.v_cache = self._v_flat[:n].view(self.L, max_batch, self.H, S8, self.kvs)
        self.causal_mask = torch.tril(torch.ones(S8, S8, dtype=torch.bool, device=dev)).unsqueeze(0).repeat(max_batch, 1, 1)
        grid = int(cfg.block_size ** 0.5)
        self.freqs_cis = precompute_freqs_cis_2d(grid, self.hd, cfg.rope_base, self.T).to(dev).contiguous()
        # activation workspaces (fragment-packed unless noted)
        self.hp = z(self.d // self.kc, mts, 64, self.epl)
        self.xnp = z(self.d // self.kc, mts, 64, self.epl)
        self.ap = z(self.d // self.kc, mts, 64, self.epl)
        self.gp = z(self.F // self.kc, mts, 64, self.epl)
        self.qbuf = z(mts * 16, self.H, self.hdp)            # row-major q (zero pad lanes stay zero)
        self.logits = z(mts * 16, self.V)                    # row-major, storage dtype (gpt.py:368)
        if self.d // 16 > L.SSQ_STRIDE:
            raise ValueError(f"dim {self.d} exceeds the fused-RMSNorm statistics row ({L.SSQ_STRIDE} x 16 columns)")
        self.ssq = z(mts * 16, L.SSQ_STRIDE, dtype=torch.float32)  # per row: d/16 partial sums of squares (fused RMSNorm)
        self.ssq_parts = 0
        # round 6: rows of `parts` partials that the consumers' fast path does not take (parts % 16 != 0 or > 128 -- GPT-3B: 200) are
        # grouped ONCE per consumer launch into their 4 lane-group sums (lgen_ssq_group4 -> ssq_g, parts 4: the same bits) instead
        # of once per consumer workgroup (profiles/r06_tile_ablations_3b.log: 25-38 us of a 99-140 us launch)
        self.ssq_g = z(mts * 16, L.SSQ_STRIDE, dtype=torch.float32)
        self.noise = None            # [N][B][V] fp32 Exp(1) draws of one generate() (allocated on demand)
        self.cur_tok = z(mts * 16, dtype=torch.int32)
        self.seq = z(max_batch, S8 + 8, dtype=torch.int32)
        self.logp = z(max_batch, S8 + 8, dtype=torch.float32)  # log-probability of seq's tokens (written only when asked for)
        self.given = None            # image completion: int32 shaped like seq, -1 = free (allocated by the first call that brings `given`)
        self.state = z(2, dtype=torch.int32)                 # [pos, step]
        # The decode / prefill attention consults `causal_mask` (the tensor Transformer.setup_caches exposes as
        # model.causal_mask, writable like the reference's, generate.py:154-163) whenever the model is t2i: a caller
        # that folds emb_masks into it by hand and then drives __call__ gets the reference's result.  c2i models
        # never edit the mask in the reference, so they keep the maskless (pure causal) kernels unless use_mask is set.
        self.use_mask = False
        self._force_causal = False  # whole-sequence `is_causal` forward (gpt.py:234) ignores causal_mask
        self._graphs = {}
        self._prof = None
        self.pos_rows = None         # continuous batching (llamagen_amd/serve.py): int32 [MTs*16] per-row positions
        self.use_tile = os.environ.get("LGEN_GEMM_TILE", "1") != "0"   # big-M tile family (round 4); 0 keeps the skinny kernels
        # tuning hooks (gemm_schedule.env_overrides): kind ("qkv" | "wo" | "w13" | "w2" | "head") -> (mt, nt, kw) / tile shape / passes
        self.tile_override, self.tile_shape_override, self.pass_override = S.env_overrides()
        self._tile_refused = set()   # GEMM kinds whose table shape the library refused (LGEN_ERR_UNSUPPORTED): served by the skinny kernels, reported as such
        self._plan = self._plan_facts = None
        # `fuse_norm` is DERIVED from these + pos_rows (property below); _fuse_base: what holds with per-row positions
        self._fuse_env, self._fuse_forced = os.environ.get("LGEN_FUSED_NORM"), None
        self._fuse_base, self._fuse_auto = (S.fuse_norm_auto(self._schedule_inputs(), rows) for rows in (True, False))
        self._pack(model)

    @property
    def pos_rows(self):
        return self._pos_rows

    @pos_rows.setter
    def pos_rows(self, value):
        """Per-row positions (llamagen_amd/serve.py) keep wqkv on the skinny kernels, so the RMSNorm is fused only where the
        register-resident fused-norm GEMMs apply (d / 32 = 8 x 3..6): a wide model (GPT-3B) that fused because its chain is >= 256
        rows would otherwise run the generic norm-prologue kernel, slower than stand-alone norm + the wide ring shapes.
        The fused / unfused choice is the `fuse_norm` property below -- nothing is flipped here (the flip used to stick
        after serving); only the captured graphs of the other mode are dropped, in BOTH directions."""
        if value is not None and self.kv_dtype is not None:
            raise NotImplementedError("per-row positions (continuous batching) have no fp8 KV cache form")
        before = self.fuse_norm if hasattr(self, "_fuse_auto") else None
        self._pos_rows = value
        if before is not None and self.fuse_norm != before:
            self._graphs = {}

    @property
    def fuse_norm(self) -> bool:
        """RMSNorm inside the consumer GEMMs?  LGEN_FUSED_NORM if set, else an explicit assignment (tests), else: with per-row
        positions only where the register-resident fused-norm kernels apply (`_fuse_base`), otherwise wherever the chain width
        / storage type allows (`_fuse_auto`).  gemm_schedule(), tile_schedule_tested() and the graph key read this."""
        if self._fuse_env is not None:
            return self._fuse_env == "1"
        if self._fuse_forced is not None:
            return self._fuse_forced
        return self._fuse_base if self._pos_rows is not None else self._fuse_auto

    @fuse_norm.setter
    def fuse_norm(self, value):
        self._fuse_forced = None if value is None else bool(value)
        self._graphs = {}

    # ---- weights --------------------------------------------------------------------------
    def _sig(self, model):
        return tuple((p.data_ptr(), p._version) for p in model.parameters())

    def _pack(self, model):
        """Fragment-packed weight copies: built once per parameter set and shared by every engine (lane)
        that serves the same parameters."""
        sig = self._sig(model)
        pw = _PACKED.get(model.tok_embeddings)
        if pw is None or pw.sig != sig or pw.dtype != self.dtype:
            pw = PackedWeights(model, self.dtype, sig)
            _PACKED[model.tok_embeddings] = pw
        self.pw = pw
        self.layers, self.norm_w, self.out_w, self.tok_emb = pw.layers, pw.norm_w, pw.out_w, pw.tok_emb
        if model.model_type == "c2i":
            self.cls_emb = pw.cls_emb
        else:
            self.fc1, self.fc2, self.cap_hidden = pw.fc1, pw.fc2, pw.cap_hidden
        self._wsig = sig
        self._graphs = {}

    def _kv_key(self):
        """KV format and scales: launch constants of the append / attention kernels (part of compatible() and of the graph key)."""
        return (self.kv_dtype, self.k_scales, self.v_scales) if self.kv_dtype is not None else (None,)

    def compatible(self, model, max_batch, S8, dtype, kv_dtype=None, kv_scales=None) -> bool:
        if kv_dtype is None:
            want = (None,)
        else:
            ks, vs = kv_scales if kv_scales is not None else ((1.0,) * self.L, (1.0,) * self.L)
            want = (kv_dtype, tuple(float(x) for x in ks), tuple(float(x) for x in vs))
        return (self.B2 == max_batch and self.S8 == S8 and self.dtype == dtype and self._kv_key() == want
                and self.dev == model.tok_embeddings.weight.device and self._wsig == self._sig(model))

    def reset(self, max_batch: int):
        """What re-running setup_caches means in the reference: fresh caches, position 0.  The KV slabs are
        NOT re-zeroed (3.5 GiB of stores per call at config 2): attention only ever reads slots < kv_len,
        all of which the current call has written (causal), so stale slots are unobservable."""
        self.state.zero_()
        self.use_mask = False
        self.causal_mask.copy_(torch.tril(torch.ones(self.S8, self.S8, dtype=torch.bool, device=self.dev)))

    # ---- GEMM schedule (llamagen_amd/gemm_schedule.py) --------------------------------------------
    def _schedule_inputs(self) -> S.ScheduleInputs:
        return S.ScheduleInputs(d=self.d, F=self.F, V=self.V, head_dim=self.hd, n_layer=self.L, MTs=self.MTs, dtype=self.dtype,
                                max_kw=self.lib.lgen_gemm_max_kw, use_tile=self.use_tile, tile_override=dict(self.tile_override),
                                tile_shape_override=dict(self.tile_shape_override), pass_override=dict(self.pass_override))

    @property
    def plan(self) -> S.Plan:
        """Kernel family, shape, passes and statistics grouping of every decode GEMM: what the launches below, gemm_schedule(),
        tile_schedule_tested() and launches_per_step() all read.  Recomputed only when one of the facts it depends on changed."""
        facts = (self.fuse_norm, self._pos_rows is not None, frozenset(self._tile_refused), self.use_tile,
                 *(tuple(sorted(o.items())) for o in (self.tile_override, self.tile_shape_override, self.pass_override)))
        if facts != self._plan_facts:
            self._plan = S.make_plan(self._schedule_inputs(), self.fuse_norm, self._pos_rows is not None, self._tile_refused)
            self._plan_facts = facts
        return self._plan

    def _tiles(self, kind: str, N: int, K: int):
        """(mt, nt, kw) of the skinny kernel for GEMM `kind` (N, K follow from the kind)."""
        return self.plan[kind].tiles

    def _passes(self, kind: str, N: int, tiles):
        return S.skinny_passes(self.plan.inputs, self.fuse_norm, kind, tiles)

    def gemm_schedule(self) -> dict:
        return S.gemm_schedule(self.plan)

    def tile_schedule_source(self) -> str:
        return S.tile_schedule_source(self.plan)

    def tile_schedule_tested(self) -> bool:
        return S.tile_schedule_tested(self.plan)

    def launches_per_step(self) -> int:
        return S.launches_per_step(self.plan)

    # ---- launches -----------------------------------------------------------------------------
    def _tile_stats(self, g: S.GemmPlan):
        """(statistics buffer, partials per row) for a fused-norm consumer of the TILE family: the producer's rows as they are where
        the consumers' fast path takes them, else (`g.group_stats`) their 4 lane-group sums, computed here by one small launch
        (bit-identical)."""
        if not g.group_stats:
            return self.ssq, self.ssq_parts
        L.check(self.lib.lgen_ssq_group4(L.ptr(self.ssq), L.ptr(self.ssq_g), self.MTs * 16, self.ssq_parts, L.stream()), "ssq_group4")
        return self.ssq_g, 4

    def _refuse_tile(self, kind) -> S.GemmPlan:
        """The library took no instantiation of `kind`'s tile shape (ERR_UNSUPPORTED): the skinny kernel from now on, and
        gemm_schedule() / tile_schedule_tested() say so."""
        self._tile_refused.add(kind)
        self._graphs = {}
        return self.plan[kind]

    def _norm_input(self, nw):
        """(input, norm weight) of a norm consumer on the decode workspace: fused -> the residual stream and the weight for the
        GEMM's prologue, else lgen_rmsnorm into `xnp` now and no weight."""
        if self.fuse_norm:
            return self.hp, nw
        L.check(self.lib.lgen_rmsnorm(L.ptr(self.hp), L.ptr(nw), L.ptr(self.xnp), self.MTs, self.d, self.eps, self.dt, L.stream()),
                "rmsnorm")
        return self.xnp, None

    def gemm(self, wp, xp, out, M, mts, N, K, epi, tiles, norm_w=None, ssq_out=None, sched=None):
        """One launch of the skinny GEMM kernels."""
        mt, nt, kw = tiles
        if mts % mt:
            mt = math.gcd(mts, mt)
        passes = int(sched[0]) if (sched is not None and norm_w is not None) else 1
        L.check(self.lib.lgen_gemm(L.ptr(wp), L.ptr(xp), L.ptr(out), M, mts, N, K, epi, self.dt, mt, nt, kw,
                                   L.ptr(norm_w), L.ptr(self.ssq) if norm_w is not None else 0, self.ssq_parts, self.eps,
                                   L.ptr(ssq_out), passes, L.stream()), "lgen_gemm")

    def qkv_gemm(self, i, w, x_in, nw):
        """[attention_norm +] wqkv + RoPE + KV append of layer i (gpt.py:214-226): the big-M tile form where the plan says so, else
        the skinny kernels (per-row positions, narrow chains, other storage types)."""
        lib, st, dt, M, mts = self.lib, L.stream(), self.dt, self.B2, self.MTs
        d, H, hd, hdp, S8 = self.d, self.H, self.hd, self.hdp, self.S8
        rows = self.pos_rows is not None
        pos_ptr = self.pos_rows.data_ptr() if rows else self.state.data_ptr()
        g = self.plan["qkv"]
        if self.kv_dtype is not None:   # fp8 slabs: the *_kv8 twins with layer i's inverse scales (fp32(1 / s), computed here)
            inv = (1.0 / self.k_scales[i], 1.0 / self.v_scales[i])
            if g.shape is not None and nw is not None:
                sq, parts = self._tile_stats(g)
                rc = lib.lgen_gemm_qkv_rope_tile_kv8(L.ptr(w["wqkv"]), L.ptr(x_in), L.ptr(self.qbuf), L.ptr(self.k_cache[i]),
                                                     L.ptr(self.v_cache[i]), L.ptr(self.freqs_cis), pos_ptr, M, mts, d, H, hd, hdp, S8,
                                                     self.kvs, dt, *g.shape, L.ptr(nw), L.ptr(sq), parts, self.eps, *inv, st)
                if rc != L.ERR_UNSUPPORTED:
                    L.check(rc, "gemm_qkv_rope_tile_kv8")
                    return
                g = self._refuse_tile("qkv")
            L.check(lib.lgen_gemm_qkv_rope_kv8(L.ptr(w["wqkv"]), L.ptr(x_in), L.ptr(self.qbuf), L.ptr(self.k_cache[i]),
                                               L.ptr(self.v_cache[i]), L.ptr(self.freqs_cis), pos_ptr, M, mts, d, H, hd, hdp, S8,
                                               self.kvs, dt, *g.tiles, L.ptr(nw), L.ptr(self.ssq if nw is not None else None),
                                               self.ssq_parts, self.eps, g.passes[0] if nw is not None else 1, *inv, st),
                    "gemm_qkv_rope_kv8")
            return
        if g.shape is not None and nw is not None:
            sq, parts = self._tile_stats(g)
            rc = lib.lgen_gemm_qkv_rope_tile(L.ptr(w["wqkv"]), L.ptr(x_in), L.ptr(self.qbuf), L.ptr(self.k_cache[i]),
                                             L.ptr(self.v_cache[i]), L.ptr(self.freqs_cis), pos_ptr, M, mts, d, H, hd, hdp, S8,
                                             self.kvs, dt, *g.shape, L.ptr(nw), L.ptr(sq), parts, self.eps, st)
            if rc != L.ERR_UNSUPPORTED:
                L.check(rc, "gemm_qkv_rope_tile")
                return
            g = self._refuse_tile("qkv")
        qkv_fn = lib.lgen_gemm_qkv_rope_rows if rows else lib.lgen_gemm_qkv_rope
        L.check(qkv_fn(L.ptr(w["wqkv"]), L.ptr(x_in), L.ptr(self.qbuf), L.ptr(self.k_cache[i]), L.ptr(self.v_cache[i]),
                       L.ptr(self.freqs_cis), pos_ptr, M, mts, d, H, hd, hdp, S8, self.kvs, dt, *g.tiles, L.ptr(nw),
                       L.ptr(self.ssq if nw is not None else None), self.ssq_parts, self.eps, g.passes[0] if nw is not None else 1, st),
                "gemm_qkv_rope")

    def gemm_kind(self, kind, w, x_in=None, nw=None, tile=True):
        """One decode GEMM of `kind` ("wo" | "w13" | "w2" | "head") on the decode workspaces with the shapes the decode graph uses
        (also what bench.py's roofline leg and the sweep tools time).  tile=False: the skinny kernel whatever the plan says."""
        d, F, M, mts = self.d, self.F, self.B2, self.MTs
        ssq = self.ssq if self.fuse_norm else None
        if x_in is None:
            x_in = self.hp
        if kind == "wo":
            wp, xp, out, epi, ssq_out = w["wo"], self.ap, self.hp, L.EPI_RES, ssq
        elif kind == "w13":
            wp, xp, out, epi, ssq_out = w["w13"], x_in, self.gp, L.EPI_SWIGLU, None
        elif kind == "w2":
            wp, xp, out, epi, ssq_out = w["w2"], self.gp, self.hp, L.EPI_RES, ssq
        elif kind == "head":
            wp, xp, out, epi, ssq_out = self.out_w, x_in, self.logits, L.EPI_ROWS, None
        else:
            raise ValueError(kind)
        N, K = self.plan.inputs.dims(kind)
        g = self.plan[kind]
        if tile and g.shape is not None and (nw is not None or kind in ("wo", "w2")):
            sq, parts = self._tile_stats(g) if nw is not None else (None, self.ssq_parts)
            rc = self.lib.lgen_gemm_tile(L.ptr(wp), L.ptr(xp), L.ptr(out), M, mts, N, K, epi, self.dt, *g.shape, L.ptr(nw),
                                         L.ptr(sq), parts, self.eps, L.ptr(ssq_out), L.stream())
            if rc != L.ERR_UNSUPPORTED:
                L.check(rc, "lgen_gemm_tile")
                return
            g = self._refuse_tile(kind)
        self.gemm(wp, xp, out, M, mts, N, K, epi, g.tiles, norm_w=nw, ssq_out=ssq_out, sched=g.passes)

    def _layers_and_logits(self, want_logits: bool = True):
        """L x [attention_norm+wqkv+rope+append | attention | wo+res | ffn_norm+w1,w3+swiglu | w2+res], then
        norm+output: 5 launches per layer (RMSNorm rides in the GEMM prologues, its statistics in the
        epilogues of the GEMMs that produce the residual stream)."""
        lib, st, dt, M, mts = self.lib, L.stream(), self.dt, self.B2, self.MTs
        H, hd, hdp, S8 = self.H, self.hd, self.hdp, self.S8
        # one device scalar (generate(): all rows at the same position) or one position per row (serve.py)
        rows = self.pos_rows is not None
        pos_ptr = self.pos_rows.data_ptr() if rows else self.state.data_ptr()
        attn_fn = lib.lgen_attn_decode_rows if rows else lib.lgen_attn_decode
        pm = self._mask()

        for i, w in enumerate(self.layers):
            self.qkv_gemm(i, w, *self._norm_input(w["an"]))
            if self._prof is not None:  # bench.py roofline leg: HIP events on the launch stream
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if self.kv_dtype is not None:
                L.check(lib.lgen_attn_decode_kv8(L.ptr(self.qbuf), L.ptr(self.k_cache[i]), L.ptr(self.v_cache[i]), L.ptr(self.ap),
                                                 pos_ptr, L.ptr(pm), self.T if pm is not None else 0, M, mts, H, hd, hdp, S8, self.kvs,
                                                 dt, self.attn_variant, self.k_scales[i], self.v_scales[i], st), "attn_decode_kv8")
            else:
                L.check(attn_fn(L.ptr(self.qbuf), L.ptr(self.k_cache[i]), L.ptr(self.v_cache[i]), L.ptr(self.ap),
                                pos_ptr, L.ptr(pm), self.T if pm is not None else 0, M, mts, H, hd, hdp, S8, self.kvs, dt, self.attn_variant, st),
                        "attn_decode")
            if self._prof is not None:
                e1.record()
                self._prof["events"].append((e0, e1))
            self.gemm_kind("wo", w)
            self.ssq_parts = self.d // 16
            self.gemm_kind("w13", w, *self._norm_input(w["fn"]))
            self.gemm_kind("w2", w)
        if want_logits:
            self.gemm_kind("head", None, *self._norm_input(self.norm_w))   # (not fused: xnp is also where the next decode step starts)

    def _mask(self):
        if self._force_causal:
            return None
        return self.causal_mask if (self.use_mask or self.model_type == "t2i") else None

    def _embed(self, table, idx, advance: bool = False):
        L.check(self.lib.lgen_embed_pack(L.ptr(table), L.ptr(idx), L.ptr(self.hp), L.ptr(self.ssq) if self.fuse_norm else 0,
                                         L.ptr(self.state) if advance else 0, self.B2, self.MTs, self.d, table.shape[0],
                                         self.dt, L.stream()), "embed_pack")
        self.ssq_parts = self.d // 16

    def _set_residual(self, rows: torch.Tensor):
        """Residual stream <- given rows [B2, d] (t2i prefix tokens from the CaptionEmbedder MLP)."""
        self.hp.copy_(pack_act(rows.contiguous(), self.MTs).view_as(self.hp))
        if self.fuse_norm:
            L.check(self.lib.lgen_ssq_pack(L.ptr(self.hp), L.ptr(self.ssq), self.MTs, self.d, self.dt, L.stream()), "ssq_pack")
        self.ssq_parts = self.d // 16

    def _sample(self, B, sp, logp=None, given=None):
        """CFG mix + top-k + softmax + argmax(p/q) for the token at step = state[1]; q = noise[step].  `logp` (fp32, shaped like
        `seq`): also the sampled token's log-probability, at the slot `seq` takes the token (serve/sampler.py:88-93,119-123).
        `given` (int32, shaped like `seq`): rows whose entry at this step is >= 0 take that token instead of drawing one."""
        greedy = 0 if sp["sample_logits"] else 1
        stride = B * self.V if not greedy else 0
        args = (L.ptr(self.logits), 0 if greedy else L.ptr(self.noise), stride, L.ptr(self.cur_tok),
                L.ptr(self.seq), L.ptr(self.state), B, self.V, self.seq.shape[1],
                1 if sp["use_cfg"] else 0, float(sp["cfg_scale"]), int(sp["cfg_interval"]),
                float(sp["temperature"]), int(sp["top_k"]), float(sp["top_p"]), greedy, self.dt)
        if logp is not None:
            assert logp.shape == self.seq.shape and logp.dtype == torch.float32
        if given is not None:
            assert given.shape == self.seq.shape and given.dtype == torch.int32
            L.check(self.lib.lgen_sample_given(*args, L.ptr(logp), L.ptr(given), L.stream()), "lgen_sample_given")
        elif logp is None:
            L.check(self.lib.lgen_sample(*args, L.stream()), "lgen_sample")
        else:
            L.check(self.lib.lgen_sample_logprob(*args, L.ptr(logp), L.stream()), "lgen_sample_logprob")

    def _logp_of(self, sp):
        return self.logp if sp.get("return_logprobs") else None

    def _given_of(self, sp):
        return self.given if sp.get("given") else None

    def decode_step(self, B, sp):
        """One KV-cached decode step: advance (pos, step); embed(cur_tok) -> L blocks -> logits -> sample."""
        self._embed(self.tok_emb, self.cur_tok, advance=True)
        self._layers_and_logits()
        self._sample(B, sp, self._logp_of(sp), self._given_of(sp))

    # ---- t2i prefix (CaptionEmbedder, gpt.py:110-131) ------------------------------------------
    def caption_embed(self, cond: torch.Tensor) -> torch.Tensor:
        """cond [B2, T, caption_dim] -> [B2, T, d] through the HIP GEMMs (fc1+gelu_tanh, fc2)."""
        B2, T, C = cond.shape
        x = cond.reshape(B2 * T, C).to(self.dtype)
        mts = S.round_mts(B2 * T)
        xp = pack_act(x, mts)
        hid = torch.zeros(self.cap_hidden // self.kc, mts, 64, self.epl, dtype=self.dtype, device=self.dev)
        out = torch.zeros(mts * 16, self.d, dtype=self.dtype, device=self.dev)
        mt = 8 if mts % 8 == 0 else mts
        self.gemm(self.fc1, xp, hid, B2 * T, mts, self.cap_hidden, C, L.EPI_GELU, (mt, 1, 1))
        self.gemm(self.fc2, hid, out, B2 * T, mts, self.d, self.cap_hidden, L.EPI_ROWS, (mt, 1, 1))
        return out[: B2 * T].view(B2, T, self.d)

    # ---- prefix prefill (t2i): all T caption positions through each layer at once -----------------------
    def _run_sequence(self, emb: torch.Tensor):
        """emb [B2, S, d] -> all S positions of all rows through every layer at once (causal, plus the folded
        `emb_masks` when a t2i mask is active): fills KV slots 0..S-1 of every layer and returns the workspace
        whose "hp" holds the final residual stream, rows r = t * B2 + b of a [B2*S]-row packed activation set.
        Same per-row math as feeding the positions one by one (rows are independent except through the
        attention); stand-alone RMSNorm kernels (the fused GEMMs are tuned for M <= 256)."""
        lib, st, dt = self.lib, L.stream(), self.dt
        B2, T, d = emb.shape
        F, H, hd, hdp, S8 = self.F, self.H, self.hd, self.hdp, self.S8
        if self.kv_dtype is not None:
            raise NotImplementedError("whole-sequence passes (score(), forward(idx, cond_idx), the batched t2i prefill) run the prefill "
                                      "kernels, which have no fp8 KV cache form: unset it with model.set_kv_cache(None) (and LGEN_KV_DTYPE)")
        if B2 != self.B2 or T > S8:
            raise ValueError(f"sequence forward of [{B2}, {T}] rows on caches set up for [{self.B2}, {S8}]")
        R = B2 * T
        mts = S.round_mts(R)
        key = (R, mts)
        ws = getattr(self, "_pf_ws", None)
        if ws is None or ws["key"] != key:
            z = lambda *s_: torch.zeros(*s_, dtype=self.dtype, device=self.dev)
            ws = dict(key=key, R=R, mts=mts, hp=z(d // self.kc, mts, 64, self.epl), xn=z(d // self.kc, mts, 64, self.epl),
                      ap=z(d // self.kc, mts, 64, self.epl), gp=z(F // self.kc, mts, 64, self.epl),
                      qkv=z(3 * d // self.kc, mts, 64, self.epl), q=z(mts * 16, H, hdp))
            self._pf_ws = ws
        rows = emb.transpose(0, 1).reshape(R, d).to(self.dtype)  # r = t * B2 + b
        ws["hp"].copy_(pack_act(rows.contiguous(), mts).view_as(ws["hp"]))
        tile = lambda K, nt=1: self._sequence_tiles(mts, K, nt)
        pm = self._mask()
        for i, w in enumerate(self.layers):
            L.check(lib.lgen_rmsnorm(L.ptr(ws["hp"]), L.ptr(w["an"]), L.ptr(ws["xn"]), mts, d, self.eps, dt, st), "rmsnorm")
            self.gemm(w["wqkv"], ws["xn"], ws["qkv"], R, mts, 3 * d, d, L.EPI_PACKED, tile(d))
            L.check(lib.lgen_rope_append_prefill(L.ptr(ws["qkv"]), L.ptr(ws["q"]), L.ptr(self.k_cache[i]), L.ptr(self.v_cache[i]),
                                                 L.ptr(self.freqs_cis), R, B2, mts, d, H, hd, hdp, S8, self.kvs, 0, dt, st),
                    "rope_append_prefill")
            L.check(lib.lgen_attn_prefill(L.ptr(ws["q"]), L.ptr(self.k_cache[i]), L.ptr(self.v_cache[i]), L.ptr(ws["ap"]), L.ptr(pm),
                                          T, B2, mts, H, hd, hdp, S8, self.kvs, dt, st), "attn_prefill")
            self.gemm(w["wo"], ws["ap"], ws["hp"], R, mts, d, d, L.EPI_RES, tile(d))
            L.check(lib.lgen_rmsnorm(L.ptr(ws["hp"]), L.ptr(w["fn"]), L.ptr(ws["xn"]), mts, d, self.eps, dt, st), "rmsnorm")
            self.gemm(w["w13"], ws["xn"], ws["gp"], R, mts, 2 * F, d, L.EPI_SWIGLU, tile(d, nt=2))
            self.gemm(w["w2"], ws["gp"], ws["hp"], R, mts, d, F, L.EPI_RES, tile(F))
        return ws

    def _sequence_tiles(self, mts, K, nt=1):
        """(mt, nt, kw) of the skinny kernel for a GEMM of the prefill / whole-sequence pass (many rows, reduction length K)."""
        return min(mts, 4), nt, max(1, min(8, (K // self.kc) // 2))

    def _prefill_prefix(self, emb: torch.Tensor):
        """emb [B2, T, d] (CaptionEmbedder output) -> KV slots 0..T-1 of every layer filled, residual stream of
        the LAST prefix position left in the decode workspace (self.hp)."""
        B2, T, _ = emb.shape
        ws = self._run_sequence(emb)
        last = unpack_act(ws["hp"], ws["R"])[(T - 1) * B2:]
        self._set_residual(last)

    def _given_begin(self, given, B, N):
        """`given` [B, N] (validated int32) -> the engine's buffer, shaped like `seq`; everything else in it is free (-1)."""
        if self.given is None:
            self.given = torch.full_like(self.seq, -1)
        self.given.fill_(-1)
        self.given[:B, :N].copy_(given)

    def _prefill_given(self, model, cond_combined, B, P):
        """Prefix fast path of image completion: the conditioning rows ++ tok_emb[given[:, :P]] (columns every row gives; the
        unconditional twins are fed the same tokens) through every layer in ONE whole-sequence pass instead of the prefill and P
        decode steps.  Leaves KV slots 0 .. T+P-1 filled, the last position's residual stream in the decode workspace, its logits
        in `logits`, state = (T - 1 + P, P) -- where the stepwise form stands when it samples token P -- and seq[:, :P] written."""
        cond = self._cond_rows(model, cond_combined)
        B2, T = cond.shape[0], cond.shape[1]
        fed = self.given[:B, :P].long().repeat(B2 // B, 1)
        ws = self._run_sequence(torch.cat([cond, self.tok_emb[fed]], dim=1))        # [B2, T + P, d]
        self._set_residual(unpack_act(ws["hp"], ws["R"])[(T + P - 1) * B2:])
        self.state[0] = T - 1 + P
        self.state[1] = P
        self._final_logits()
        self.seq[:B, :P].copy_(self.given[:B, :P])

    def _cond_rows(self, model, cond):
        """cls_embedding(cond)[:, :T] (gpt.py:341-346): rows of the class table (LabelEmbedder in eval mode, gpt.py:78-83) or the
        CaptionEmbedder MLP (gpt.py:110-131) -> [B2, T, d]."""
        if model.model_type == "c2i":
            return self.cls_emb[cond.reshape(-1).long()].unsqueeze(1)[:, : self.T]
        return self.caption_embed(cond)[:, : self.T]

    def _check_capacity(self, T, N):
        """T conditioning positions + N image tokens must fit the KV slots and (all but the last token) the RoPE table."""
        if T + N > self.S8 or T + N - 1 > self.freqs_cis.shape[0]:
            raise IndexError(f"{T} + {N} tokens exceed the caches ({self.S8} slots) / RoPE table ({self.freqs_cis.shape[0]} rows)")

    def fold_emb_masks(self, emb_masks, T):
        """generate.py:154-163: AND the validity of the T (left-padded) caption tokens, [B2, T] or [1, T] for every row alike, into
        the prefix columns of causal_mask, force the diagonal, and have the attention consult the mask.  None: nothing to fold."""
        if emb_masks is None:
            return
        cm = self.causal_mask
        cm[:, :, :T] = cm[:, :, :T] & emb_masks.to(self.dev).ne(0).unsqueeze(1)
        cm |= torch.eye(self.S8, dtype=torch.bool, device=self.dev)
        self.use_mask = True

    def forward_sequence(self, model, idx, cond_idx):
        """Teacher-forced forward over a whole sequence (gpt.py:341-346, 357-368 with `is_causal` attention):
        rows = cls_embedding(cond_idx)[:, :T] ++ tok_embeddings(idx) -> fp32 logits [B, T + n, V] (values carry
        the storage dtype's rounding, gpt.py:368).  The reference runs this shape without KV caches; here the
        K/V of every position land in the engine's slabs (slots 0..T+n-1) as a side effect."""
        emb = torch.cat([self._cond_rows(model, cond_idx), self.tok_emb[idx.long()]], dim=1)   # [B, T + n, d]
        B2, S, d = emb.shape
        self._force_causal = True  # this shape is `is_causal` in the reference (gpt.py:234), no emb_masks
        try:
            ws = self._run_sequence(emb)
        finally:
            self._force_causal = False
        return self._sequence_logit_rows(ws)[:ws["R"]].view(S, B2, self.V).transpose(0, 1).float().contiguous()

    def _sequence_logit_rows(self, ws):
        """norm + output (gpt.py:367-368) on the final residual stream of _run_sequence: storage-dtype logits [mts * 16, V],
        row r = t * B2 + b (rows >= R are padding)."""
        lib, st, dt, mts, R, d = self.lib, L.stream(), self.dt, ws["mts"], ws["R"], self.d
        L.check(lib.lgen_rmsnorm(L.ptr(ws["hp"]), L.ptr(self.norm_w), L.ptr(ws["xn"]), mts, d, self.eps, dt, st), "rmsnorm")
        lg = torch.empty(mts * 16, self.V, dtype=self.dtype, device=self.dev)
        self.gemm(self.out_w, ws["xn"], lg, R, mts, self.V, d, L.EPI_ROWS, self._sequence_tiles(mts, d))
        return lg

    def score_sequence(self, model, cond_combined, ids, B, emb_masks, cfg_scale, temperature):
        """log p(ids[b, j] | cond, ids[b, :j]) under the CFG-mixed, temperature-scaled model, fp32 [B, N]: ONE teacher-forced pass
        over cond ++ tok_emb[ids[:, :-1]] (the positions generate() visits one by one, with the same mask), lm_head in the storage
        dtype, then lgen_logprob_rows on its rows -- no fp32 [B, S, V] logits, no softmax of width V in memory (what
        gpt.py:373-380 does for the cross-entropy).  cond_combined: the B2 = B or 2B conditioning rows of generate() (conditional
        rows, then their unconditional twins); emb_masks: [B2, T] or None."""
        N = ids.shape[1]
        cond = self._cond_rows(model, cond_combined)
        T, B2 = cond.shape[1], cond.shape[0]
        self._check_capacity(T, N)
        ids = ids.to(device=self.dev, dtype=torch.int32)
        fed = ids[:, :-1].long().repeat(B2 // B, 1)                                 # the twins are fed the same tokens
        emb = torch.cat([cond, self.tok_emb[fed]], dim=1)                           # [B2, T + N - 1, d]
        self.fold_emb_masks(emb_masks, T)   # as generate_iter folds them
        ws = self._run_sequence(emb)
        lg = self._sequence_logit_rows(ws)
        S = T + N - 1
        tg = torch.full((lg.shape[0],), -1, dtype=torch.int32, device=self.dev)     # rows r = t * B2 + b; only (t >= T - 1, b < B) score
        tg[: S * B2].view(S, B2)[T - 1:, :B] = ids.t()
        out = torch.zeros(lg.shape[0], dtype=torch.float32, device=self.dev)
        L.check(self.lib.lgen_logprob_rows(L.ptr(lg), L.ptr(tg), L.ptr(out), S * B2, self.V, B if B2 > B else 0, float(cfg_scale),
                                           float(temperature), self.dt, L.stream()), "lgen_logprob_rows")
        return out[: S * B2].view(S, B2)[T - 1:, :B].t().contiguous()

    def _final_logits(self):
        """norm + output on the decode workspace (gpt.py:367-368) after the t2i prefill: on the SKINNY kernels at every chain width
        (tile and skinny differ in accumulation order; this is the form the t2i oracle tests hold)."""
        self.gemm_kind("head", None, *self._norm_input(self.norm_w), tile=False)

    # ---- Exp(1) noise: what torch.multinomial draws, one [B, V] fp32 exponential_ per sampled token ----
    def _noise_buffer(self, N, B):
        if self.noise is None or self.noise.shape[0] < N or self.noise.shape[1] != B:
            # ones, not empty: the slice of a filler batch (generate.PadBatch) is never drawn, and the sampler divides by it
            self.noise = torch.ones(N, B, self.V, dtype=torch.float32, device=self.dev)
        return self.noise

    def draw_noise(self, N, B, b0, n):
        """The N x [n, V] exponential_ draws of ONE batch of a chain (images b0 .. b0 + n - 1 of B): the same calls, in the same
        order, that this batch's own generate() would make (each [n, V] slice is one contiguous block of the chain's buffer)."""
        buf = self._noise_buffer(N, B)
        for j in range(N):
            buf[j, b0:b0 + n].exponential_(1.0)

    def _noise_begin(self, N, B, noise_seq):
        """noise[i] feeds the sampler of step i.  Injected (tests) or drawn from the device's default
        generator in the reference's order -- N separate [B, V] exponential_ calls -- up front on the
        calling stream (N x ~5 us, < 1 % of a generate()), so that no RNG launch sits inside the captured
        decode step.  (A side stream would overlap it, but HIP maps streams onto 4 hardware queues and a
        lane's side stream then queues behind another lane's whole decode loop.)"""
        self._noise_buffer(N, B)
        if noise_seq is not None:
            self.noise[:N].copy_(noise_seq[:N].to(self.dev))
            return
        for j in range(N):
            self.noise[j].exponential_(1.0)

    # ---- the generate() loop ---------------------------------------------------------------
    def generate(self, model, cond_combined, B, max_new_tokens, emb_masks, sp):
        """prefill + (N-1) decode steps; returns int32 [B, N] (with sp["return_logprobs"]: and fp32 [B, N] log-probabilities).
        sp: sampling parameter dict."""
        it = self.generate_iter(model, cond_combined, B, max_new_tokens, emb_masks, sp)
        while True:
            try:
                next(it)
            except StopIteration as stop:
                return stop.value

    def generate_iter(self, model, cond_combined, B, max_new_tokens, emb_masks, sp):
        """Generator form of generate(): yields after every enqueued decode step (nothing waits for the GPU),
        so that a scheduler can interleave the host-side submission of several in-flight batches
        (llamagen_amd/pipeline.py); the int32 [B, N] result is the generator's return value."""
        N = max_new_tokens
        T = 1 if model.model_type == "c2i" else cond_combined.shape[1]
        self._check_capacity(T, N)
        self._prof = getattr(model, "_prof", None)
        self.state.zero_()
        self.fold_emb_masks(emb_masks, T)
        noise_seq = sp.pop("_noise_seq", None)
        prefilled = sp.pop("_noise_prefilled", False)  # generate.py drew it batch by batch (chains of several batches)
        sampling = bool(sp["sample_logits"])
        if sampling and not prefilled:
            self._noise_begin(N, B, noise_seq)
        logp = self._logp_of(sp)
        # image completion (llamagen_amd/given.py): int32 [B, N], -1 = free.  Stepwise form: the sampler takes a given token
        # instead of drawing one, at any position, with any storage / KV dtype.  Prefix fast path: the P columns every row gives go
        # through every layer at once (not with the fp8 KV cache -- no whole-sequence kernels -- nor with log-probabilities)
        given = sp.pop("_given", None)
        stepwise = sp.pop("_given_stepwise", False)
        sp["given"] = given is not None
        P = 0
        if given is not None:
            self._given_begin(given, B, N)
            if not stepwise and self.kv_dtype is None and logp is None:
                P = given_prefix_length(given)
        # ---- prefill (generate.py:77-86): state = (pos, step) = (T-1, 0) when the first token is sampled
        if P >= 1:
            self._prefill_given(model, cond_combined if model.model_type == "t2i" else cond_combined.to(torch.int32), B, P)
        elif model.model_type == "c2i":
            self._embed(self.cls_emb, cond_combined.to(torch.int32).contiguous())
            self._layers_and_logits()
        else:
            emb = self.caption_embed(cond_combined)
            if os.environ.get("LGEN_SEQ_PREFILL") == "1" or T > 128 or self.kv_dtype is not None:   # (fp8 KV cache: decode kernels only)
                for t in range(T):  # causal prefix, one position at a time through the decode kernels
                    self.state[0] = t
                    self._set_residual(emb[:, t])
                    self._layers_and_logits(want_logits=(t == T - 1))
            else:  # all T positions per layer at once
                self._prefill_prefix(emb)
                self.state[0] = T - 1
                self._final_logits()
        self._sample(B, sp, logp, self._given_of(sp))
        yield P
        # ---- decode (generate.py:105-123): every step first advances (pos, step)
        key = (B, N, self._kv_key(), self._mask() is not None, self.fuse_norm, self.use_tile, tuple(sorted(self.tile_shape_override.items())),
               tuple(sorted(self.tile_override.items())),
               tuple(sorted(self.pass_override.items())), sp["use_cfg"], sp["cfg_scale"],
               sp["cfg_interval"], sp["temperature"], sp["top_k"], sp["top_p"], sp["sample_logits"],
               self.noise.data_ptr() if sampling else 0, logp is not None)
        if given is not None:   # the step samples through lgen_sample_given: a graph of its own (P is not part of it: the counters live on the device)
            key += ("given",)
        i = P + 1     # tokens 0 .. P are in `seq`
        use_graph = os.environ.get("LGEN_NO_GRAPH") is None and N > 3 and N - i >= 2   # (a capture needs its eager, warming step first)
        if use_graph:
            if i < N:  # first decode step eagerly (also warms every kernel before capture)
                self.decode_step(B, sp)
                i += 1
                yield i - 1
            g = self._graphs.get(key)
            if g is None:  # capture only records the step (on the current stream); nothing executes here
                g = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(g):
                    self.decode_step(B, sp)
                self._graphs[key] = g
            while i < N:
                g.replay()
                i += 1
                yield i - 1
        else:
            while i < N:
                self.decode_step(B, sp)
                i += 1
                yield i - 1
        if logp is not None:
            return self.seq[:B, :N].clone(), logp[:B, :N].clone()
        return self.seq[:B, :N].clone()

    # ---- Transformer.forward inference branches (gpt.py:347-368) ---------------------------------
    def forward(self, model, idx, cond_idx, input_pos):
        pos = [int(p) for p in input_pos.reshape(-1).tolist()]
        outs = []
        if cond_idx is not None:
            if model.model_type == "c2i":
                embs = None
                rows = cond_idx.reshape(-1).to(torch.int32).contiguous()
            else:
                embs = self.caption_embed(cond_idx)
            nb = cond_idx.shape[0]
        else:
            rows = idx.reshape(-1).to(torch.int32).contiguous()
            embs = None
            nb = idx.shape[0]
        if nb != self.B2:
            raise ValueError(f"batch {nb} != max_batch_size {self.B2} given to setup_caches")
        for p in pos:  # the reference's index_put / freqs_cis[input_pos] raise IndexError (gpt.py:177-185, 356)
            if not (0 <= p < self.S8 and p < self.freqs_cis.shape[0]):
                raise IndexError(f"input_pos {p} outside the caches set up for {self.S8} slots / {self.freqs_cis.shape[0]} RoPE rows")
        for j, p in enumerate(pos):
            self.state[0] = p
            if embs is not None:
                self._set_residual(embs[:, j])
            elif cond_idx is not None:
                self._embed(self.cls_emb, rows)
            else:
                self._embed(self.tok_emb, rows)
            self._layers_and_logits()
            outs.append(self.logits[:nb].float())
        return torch.stack(outs, dim=1)
