"""Which kernel serves each GEMM of a decode step, decided once: for GEMM `kind` of a model at a chain width, the kernel family
("tile" | "skinny"), its shape, the passes of a fused-norm GEMM and whether the statistics row is grouped first.

Pure arithmetic on a `ScheduleInputs` and three dynamic facts (RMSNorm fused?  per-row positions?  kinds the library refused): no
device, no engine object.  `DecodeEngine` launches from the `Plan`; gemm_schedule(), tile_schedule_source(), tile_schedule_tested()
and launches_per_step() report from the same `Plan`, so what is printed is what is launched.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Callable, Mapping, Optional

import torch

from . import _lib as L

KINDS = ("qkv", "wo", "w13", "w2", "head")
NORM_KINDS = ("qkv", "w13", "head")     # GEMMs whose input is an RMSNorm of the residual stream (the others add to it: EPI_RES)
REPORT_NAMES = {"wqkv": "qkv", "wo": "wo", "w13": "w13", "w2": "w2", "lm_head": "head"}   # gemm_schedule()'s spelling -> kind


def round_mts(rows: int) -> int:
    """m-tiles (16 rows each) of a packed activation set of `rows` rows: 1, 2, 4, 8 or a multiple of 8."""
    mts = -(-rows // 16)
    if mts > 4:
        return -(-mts // 8) * 8
    return 4 if mts == 3 else mts


# Big-M tile family (csrc/gemm_tile.hip): workgroup shapes (wm, wn, mtv, ntv, kb, stages, lw) per decode GEMM, keyed by the smallest
# MTs (rows / 16) they serve.  Per-CU tile area ~ rows x N / 256 CUs, as square as the wave arrangement allows (the feed per CU is the
# tile perimeter x K); measured on MI355X with tools/gemm_tile_sweep.py (gpurun_out/tile_sweep2/3.log, GPT-L, us per launch,
# skinny -> tile): 256 rows wqkv 10.2 -> 9.8, wo 4.85 -> 4.1, w1||w3 13.1 -> 10.6, w2 7.8 -> 7.7, lm_head 23.2 -> 20.9; 512 rows
# 16.3 -> 12.9, 7.7 -> 5.1, 20.3 -> 18.9, 9.5 -> 7.9, 39.0 -> 37.8; 1024 rows 51.6 -> 22.1, 13.0 -> 6.6, 34.1 -> 35.0, 16.9 -> 11.5,
# 71.1 -> 68.8.  The 256- and 640-row tables are what tests/test_gpu_headline.py holds to the oracle end to end and what bench.py
# accepts as a tested schedule; every shape of every table is held to the oracle at kernel level (and all shapes agree bit for bit).
TILE_SCHEDULES = {
    16: {"qkv": (4, 1, 1, 3, 4, 4, 4), "wo": (2, 2, 1, 1, 4, 4, 4), "w13": (4, 1, 1, 6, 4, 3, 4), "w2": (2, 2, 1, 1, 4, 4, 4),
         "head": (4, 1, 2, 8, 2, 4, 4)},
    32: {"qkv": (4, 1, 1, 6, 4, 3, 4), "wo": (2, 2, 2, 1, 4, 4, 4), "w13": (4, 1, 2, 8, 2, 4, 4), "w2": (2, 2, 2, 1, 4, 4, 4),
         "head": (4, 1, 2, 8, 2, 4, 4)},
    # 640 rows (`bench.py --steps 20`: two chains of ten batches), gpurun_out/tile_sweep4.log: a launch is whole ROUNDS of <= 256
    # workgroups, so the shapes are the ones that fill one round -- wqkv 240 workgroups 16.0 us (22.1 with the 512-row shape: 320
    # workgroups = two rounds), wo 160 / 6.3 (8.1), w1||w3 220 / 18.2, w2 160 / 10.9 (14.6), lm_head 640 / 50.3
    # (w1||w3 and lm_head: eight consumer waves x one m-tile -- two per SIMD, one's RMSNorm VALU work under the other's MFMAs:
    # 18.2 against 19.2 us and 50.3 against 52.0 for four waves x two m-tiles, gpurun_out/tile_sweep5.log)
    40: {"qkv": (4, 1, 1, 8, 2, 4, 4), "wo": (2, 2, 2, 2, 4, 4, 4), "w13": (8, 1, 1, 8, 2, 4, 4), "w2": (2, 2, 2, 2, 4, 4, 4),
         "head": (8, 1, 1, 8, 2, 4, 4)},
    64: {"qkv": (4, 1, 2, 8, 2, 4, 4), "wo": (2, 2, 2, 2, 4, 4, 4), "w13": (4, 1, 2, 8, 2, 4, 4), "w2": (2, 2, 2, 2, 4, 4, 4),
         "head": (4, 1, 2, 8, 2, 4, 4)},
}
TILE_SCHEDULE_EXACT = (40,)        # keys that serve exactly that MTs; the others serve every MTs from the key up to the next one
TESTED_TILE_SCHEDULES = (16, 40)   # keys of TILE_SCHEDULES with an end-to-end oracle test (tests/test_gpu_headline.py)
TABLE_MODEL = (1024, 2816, 16384)   # (dim, ffn hidden, vocab) of GPT-L: the model TILE_SCHEDULES was measured on

# The other registry models that bench.py runs with chains of >= 256 rows: the shapes the round-4 on-device search settled on
# (profiles/r04_bench_config{3,4}.json, `schedule`), now PINNED.  Round 4 timed every shape (and the skinny kernel) at first use in
# the user's process and kept whichever was faster at that moment: the tile shapes agree bit for bit, but tile and skinny differ in
# accumulation order and in the SwiGLU's exp / reciprocal, so the family -- and with it bf16 logits -- depended on timing noise
# (ADVICE round 4).  The family now depends on shapes only: tile wherever a table names a shape the library takes.
MODEL_TILE_SCHEDULES = {
    TABLE_MODEL: TILE_SCHEDULES,
    # Round 6: chains of >= 512 rows for the wide models (bench.py --config 3 / 4: two chains of eight batches of 32 / four batches of
    # 64) with shapes MEASURED per model and width (tools/gemm_tile_sweep.py, profiles/r06_tile_sweep_{xxl,3b,xl}.log, us per launch):
    # GPT-XXL 512 rows wqkv 24.0 (28.9 with the 256-row shape), w1||w3 26.1, wo 8.4, w2 19.6, lm_head 50.5; GPT-3B 512 rows wqkv 99.4,
    # w1||w3 140.7 (153.3), wo 23.7 (32.8), w2 53.6 (75.0), lm_head 109.3 (114.8); GPT-XL 256 rows (config 5: two chains of eight
    # batches of 16) wqkv 12.8 (skinny 15.4), wo 5.6 (7.3), w1||w3 14.8 (20.0), w2 13.3 (12.6), lm_head 24.5 (27.1).
    (1536, 4096, 16384): {   # GPT-XXL (config 3)
        16: {"qkv": (4, 1, 1, 8, 2, 4, 4), "wo": (2, 2, 2, 2, 4, 4, 4), "w13": (4, 1, 2, 8, 2, 4, 4), "w2": (2, 2, 2, 2, 4, 4, 4),
             "head": (4, 1, 2, 8, 2, 4, 4)},
        # wqkv: four consumer waves x two m-tiles instead of eight x one -- 25.5 against 24.0 us alone, 47.5 against 45.6 / 46.0 img/s in
        # the two-chain bench (same box, profiles/r06_c3_c5_shape_ab.log; the other candidates of that log lose or tie)
        32: {"qkv": (4, 1, 2, 6, 2, 4, 4), "wo": (2, 2, 2, 2, 4, 4, 4), "w13": (4, 1, 2, 8, 2, 4, 4), "w2": (2, 2, 2, 2, 4, 4, 4),
             "head": (4, 1, 2, 8, 2, 4, 4)}},
    (3200, 8704, 16384): {   # GPT-3B (config 4)
        16: {"qkv": (8, 1, 1, 6, 2, 4, 4), "wo": (2, 2, 2, 2, 4, 4, 4), "w13": (4, 1, 1, 6, 2, 4, 4), "w2": (2, 2, 2, 2, 4, 4, 4),
             "head": (8, 1, 1, 8, 2, 4, 4)},
        # 512 rows, statistics grouped (lgen_ssq_group4): wqkv 128 x 160 tiles = 240 workgroups, ONE round of the 256 CUs, 53.3 us
        # (75.3 with 128 x 96 = 400 workgroups = two rounds; 98.9 before the grouping: profiles/r06_tile_sweep2_3b.log).  w1||w3 keeps
        # 128 x 96: the 128 x 160 shape is faster alone (90.1 against 102.9 us) and SLOWER in the two-chain bench -- same box,
        # alternating (profiles/r06_c4_shape_ab.log): both new 31.4 / 31.4, both old 36.0 / 35.8, new wqkv only 37.2, new w1||w3 only 31.3 img/s
        32: {"qkv": (4, 1, 2, 10, 2, 4, 4), "wo": (2, 2, 4, 2, 2, 4, 4), "w13": (4, 1, 2, 6, 2, 4, 4), "w2": (2, 2, 4, 2, 2, 4, 4),
             "head": (4, 1, 2, 8, 2, 4, 4)}},
    (1280, 3584, 16384): {   # GPT-XL (config 5, t2i)
        16: {"qkv": (4, 1, 1, 4, 4, 4, 4), "wo": (2, 2, 2, 1, 4, 4, 4), "w13": (4, 1, 1, 8, 2, 4, 4), "w2": (2, 2, 2, 1, 4, 4, 4),
             "head": (8, 1, 1, 8, 2, 4, 4)},
        # 384 rows (two chains of twelve batches of 16, what bench.py --config 5 runs): 64 x 64 wqkv tiles would be 360 workgroups (two
        # rounds of the 256 CUs), 64 x 128 w1||w3 tiles 336; 64 x 96 (240) and 128 x 128 (168) fill one -- 21.6 / 21.45 against 21.16 /
        # 21.25 img/s in the two-chain bench, same box, alternating (profiles/r06_c5_shape_ab2.log)
        24: {"qkv": (4, 1, 1, 6, 4, 3, 4), "wo": (2, 2, 2, 1, 4, 4, 4), "w13": (4, 1, 2, 8, 2, 4, 4), "w2": (2, 2, 2, 1, 4, 4, 4),
             "head": (8, 1, 1, 8, 2, 4, 4)}},
}
# (dim, F, V) -> keys of its table that an end-to-end oracle test runs (tests/test_gpu_headline.py:
# test_config{3,4}_..._shapes_bf16_vs_oracle[128] / [192]: 256- / 384-row chains; test_config{3,4,5}_wide_chain_shapes_bf16_vs_oracle:
# the 512- / 512- / 256-row chains bench.py runs since round 6)
TESTED_MODEL_SCHEDULES = {TABLE_MODEL: TESTED_TILE_SCHEDULES, (1536, 4096, 16384): (16, 32), (3200, 8704, 16384): (16, 32),
                          (1280, 3584, 16384): (16, 24)}


def tile_schedule_key(mts: int, table=None):
    """Key of a tile table (default TILE_SCHEDULES) that serves a chain of `mts` m-tiles (None: below 256 rows, the skinny kernels)."""
    table = TILE_SCHEDULES if table is None else table
    exact = TILE_SCHEDULE_EXACT if table is TILE_SCHEDULES else ()
    if mts in exact:
        return mts
    keys = [k for k in table if k not in exact and k <= mts]
    return max(keys) if keys else None

def env_overrides(environ=os.environ):
    """(tile_override, tile_shape_override, pass_override) from the tuning switches:
    LGEN_TILES="qkv=2,4,8;wo=4,1,8;w2=4,1,8" -- (mt, nt, kw) of the skinny kernels (e.g. fewer, fatter workgroups per GEMM so that the
    kernels of several in-flight batches share the chip side by side instead of taking turns);
    LGEN_TILE_SHAPES="qkv=4,1,1,3,4,4,4;..." -- shapes of the big-M tile family instead of the measured tables;
    LGEN_PASSES="qkv=2,0;w13=3,0" -- (passes, double_buffer) of the fused-norm GEMMs (the `passes` argument of lgen_gemm)."""
    def parse(name, kinds, what, fields, ok=lambda t: True):
        out = {}
        for item in filter(None, environ.get(name, "").split(";")):
            kind, _, val = item.partition("=")
            if kind.strip() not in kinds:
                raise ValueError(f"{name}: unknown {what} '{kind}'")
            t = tuple(int(v) for v in val.split(","))
            if len(t) != len(fields.split(",")) or not ok(t):
                raise ValueError(f"{name}: '{item}' is not kind={fields}")
            out[kind.strip()] = t
        return out
    return (parse("LGEN_TILES", KINDS, "GEMM", "mt,nt,kw"), parse("LGEN_TILE_SHAPES", KINDS, "GEMM", "wm,wn,mtv,ntv,kb,stages,lw"),
            parse("LGEN_PASSES", NORM_KINDS, "fused-norm GEMM", "passes,double_buffer", lambda t: t[0] >= 1))


@dataclass(frozen=True)
class ScheduleInputs:
    """Everything static the decision depends on.  `max_kw(epi, fused, mt, nt)` is the library's lgen_gemm_max_kw (or a stub)."""
    d: int
    F: int
    V: int
    head_dim: int
    n_layer: int
    MTs: int
    dtype: torch.dtype
    max_kw: Callable[[int, int, int, int], int]
    use_tile: bool = True
    tile_override: Mapping = field(default_factory=dict)         # kind -> (mt, nt, kw)
    tile_shape_override: Mapping = field(default_factory=dict)   # kind -> (wm, wn, mtv, ntv, kb, stages, lw)
    pass_override: Mapping = field(default_factory=dict)         # kind -> (passes, double_buffer)

    @property
    def kc(self):      # elements of K per MFMA fragment chunk
        return 16 if self.dtype == torch.float32 else 32

    @property
    def mt(self):      # m-tiles per workgroup (1, 2 or 4; MTs is 1, 2, 4 or a multiple of 8)
        return min(self.MTs, 4)

    @property
    def model(self):   # key of MODEL_TILE_SCHEDULES
        return (self.d, self.F, self.V)

    def dims(self, kind):
        """(N, K) of GEMM `kind`."""
        d, F = self.d, self.F
        return {"qkv": (3 * d, d), "wo": (d, d), "w13": (2 * F, d), "w2": (d, F), "head": (self.V, d)}[kind]


def fuse_norm_auto(c: ScheduleInputs, per_row_positions: bool = False) -> bool:
    """RMSNorm folded into the consumer GEMMs (5 launches / layer instead of 7)?  Pays off (-12 % step time, GPT-L) only with
    gemm_normpre.hip, which normalises the activation panel in registers while the weight loads are in flight and needs a wave's K
    range to fit in registers: bf16, d/32 = 8 waves x 3..6 chunks (GPT-B .. GPT-XXL).  Elsewhere the stand-alone 3.4 us norm kernels
    are faster than the generic NORM prologue (+4 us of exposed VALU work per GEMM).
    (round 4) the big-M tile family normalises the B fragments between LDS and the MFMA, whatever the row length: chains of >= 256
    rows fuse for every width whose statistics row the kernels take (GPT-3B: d = 3200, 200 partials per row) -- unless the rows
    carry their own positions: the wqkv of a continuous batcher stays skinny, so only the register-resident rule holds."""
    kch = c.d // c.kc
    if c.dtype != torch.bfloat16:
        return False
    if kch % 8 == 0 and 3 <= kch // 8 <= 6:
        return True
    return not per_row_positions and c.MTs >= 16 and c.use_tile and (c.d // 16) % 4 == 0 and c.d // 16 <= L.SSQ_STRIDE


def skinny_tiles(c: ScheduleInputs, fuse_norm: bool, kind: str):
    """(mt, nt, kw) for one decode GEMM.  Measured on MI355X (tools/ubench_kernels.py, GPT-L, M = 64):
    every kernel of the chain is latency-bound (~4-6 us), so the shape that wins is the one that puts
    >= ~160 workgroups on the chip with the fewest dependent load rounds per wave: split the batch
    rows over workgroups (mt < MTs) when N alone gives too few tiles (wo / w2: N/16 = 64), group
    n-tiles (nt 2 / 4) only when there are >= 352 / 1024 of them (w1||w3, lm_head)."""
    if kind in c.tile_override:
        return c.tile_override[kind]
    N, K = c.dims(kind)
    ntiles = N // 16
    kch = K // c.kc
    bf16 = c.dtype == torch.bfloat16
    if c.MTs >= 8 and bf16 and not fuse_norm and kch >= 96:
        # wide models (GPT-3B: d 3200, F 8704) at 256 rows: every GEMM is the plain ring kernel and the work is MFMA-shaped
        # (64 GFLOP per layer), so big tiles and FEW K-splitting waves win -- measured (tools/gemm_sweep_wide.py,
        # profiles/r03_wide_sweep.log): qkv (4, 4, 4) 45.0 us against (4, 2, 8) 54.7, wo (4, 4, 4) 18.2 / 26.9, w1||w3 (8, 2, 4)
        # 64.4 / 84.1, w2 (4, 4, 8) 40.1 / 66.6, lm_head (8, 2, 4) 47.5 / 68.4: 4.07 ms of GEMMs per decode step instead of 5.64
        # at 128 rows: qkv (4, 4, 4) 29.5 us against (4, 2, 8) 34.5, wo (4, 2, 4) 12.9 / 16.3, w1||w3 (4, 4, 4) 43.4 / 51.0,
        # w2 (4, 2, 8) 28.8 / 37.1, lm_head (8, 2, 4) 26.3 / 36.9: 2.78 ms per step instead of 3.37
        if c.MTs >= 16:
            mt, nt = {"qkv": (4, 4), "wo": (4, 4), "w13": (8, 2), "w2": (4, 4), "head": (8, 2)}[kind]
        else:
            mt, nt = {"qkv": (4, 4), "wo": (4, 2), "w13": (4, 4), "w2": (4, 2), "head": (8, 2)}[kind]
        while ntiles % nt:
            nt //= 2
        while c.MTs % mt:
            mt //= 2
        if kind == "w13":
            nt = max(nt, 2)
        return mt, nt, (4 if kch <= 128 else 8)
    if c.MTs >= 16 and bf16 and fuse_norm and kch // 4 >= 12 and (kind == "w2" or (kind == "wo" and ntiles >= 96)) \
            and ntiles % 2 == 0:
        # RES GEMMs of the fused-norm models at 256 rows: 4 waves x >= 12 chunks run the steady-state ring kernel (counted waits);
        # measured: GPT-L w2 (2, 2, 4) 6.16 us against (4, 1, 8) 7.35 / (2, 2, 8) 6.90; GPT-XXL w2 13.2 / 17.1, wo 5.6 / 8.1
        # (GPT-L's wo, 8 chunks per wave at kw 4, stays (4, 1, 8): 4.64 us)
        return 2, 2, 4
    epi = {"qkv": L.EPI_QKV, "wo": L.EPI_RES, "w2": L.EPI_RES, "w13": L.EPI_SWIGLU, "head": L.EPI_ROWS}[kind]
    fused = fuse_norm and kind in NORM_KINDS
    if fused and kch % 8 == 0 and 3 <= kch // 8 <= 6:
        # normpre kernel (persistent along N since round 3): every workgroup normalises its own rows of the panel once and
        # walks `skinny_passes` n-groups, so few rows per workgroup and 4 n-tiles per group.  Measured best (tools/gemm_sweep.py,
        # GPT-L, profiles/r03_gemm_sweep.log): qkv (1, 4, 8) at every chain width (64 / 128 / 256 rows: 6.3 / 8.0 / 9.9 us with
        # 1 / 2 / 3 passes), w1||w3 and lm_head (2, 4, 8) (8.5 / 10.7 / 12.6 us and 11.1 / 14.8 / 22.0 us)
        mt = 1 if kind == "qkv" else max(1, c.mt // 2)
        nt = 4
        while ntiles % nt or (kind == "w13" and nt & 1 and nt > 1):
            nt //= 2
        return mt, max(nt, 2 if kind == "w13" else 1), 8
    nt = 4 if ntiles >= 1024 else (2 if (kind == "w13" or ntiles >= 352) else 1)
    while ntiles % nt:
        nt //= 2
    mt = c.mt
    while mt > 1 and (ntiles // nt) * (c.MTs // mt) < 160 and c.MTs % (mt // 2) == 0:
        mt //= 2
    kmax = c.max_kw(epi, 1 if fused else 0, mt, nt)
    kw = max(1, min(kmax, 16 if kch >= 64 else 8, kch // 2))
    return mt, nt, kw


def skinny_passes(c: ScheduleInputs, fuse_norm: bool, kind: str, tiles):
    """(passes, double_buffer) of a fused-norm GEMM: n-groups one workgroup walks with its normalised rows kept in registers
    (gemm_normpre.hip).  One workgroup of these kernels fills a CU, so the (n-group, m-group) units are dealt out as
    ~one workgroup per CU: ceil(units / 256) passes each."""
    if kind in c.pass_override:
        return c.pass_override[kind]
    if not (fuse_norm and kind in NORM_KINDS):
        return 1, 0
    mt, nt, _ = tiles
    units = (c.dims(kind)[0] // 16 // nt) * (c.MTs // max(1, math.gcd(c.MTs, mt)))
    passes = min(64, max(1, -(-units // 256)))   # (the library takes 1..64: a scheduling choice only, results are identical)
    # weights of the next n-group in a second register set: no faster than reloading after the MFMAs (10.74 vs 10.76 us,
    # w1||w3 at 128 rows) and bimodal inside the decode graph (73 / 63 img/s, tools/exp_r3c.py): off
    return passes, 0


def _tile_family_applies(c: ScheduleInputs, fuse_norm: bool) -> bool:
    return c.use_tile and c.MTs >= 16 and c.dtype == torch.bfloat16 and fuse_norm


def tile_shape(c: ScheduleInputs, fuse_norm: bool, per_row_positions: bool, refused, kind: str):
    """(wm, wn, mtv, ntv, kb, stages, lw) of the big-M tile family (csrc/gemm_tile.hip) for one decode GEMM, or None where the
    skinny kernels stay: chains of >= 256 rows, bf16, RMSNorm fused (the family's norm consumers read the producer's statistics),
    one position for all rows.  Measured on MI355X, GPT-L, 256 rows (tools/gemm_tile_sweep.py, us per launch, skinny -> tile):
    wqkv 10.2 -> 9.8, wo 4.85 -> 4.1, w1||w3 13.1 -> 10.6, w2 7.8 -> 7.7, lm_head 23.2 -> 20.9."""
    if kind in refused:
        return None
    if kind in c.tile_shape_override:
        return c.tile_shape_override[kind]
    if not _tile_family_applies(c, fuse_norm):
        return None
    if kind == "qkv" and (per_row_positions or c.head_dim < 16):
        return None
    table = MODEL_TILE_SCHEDULES.get(c.model, TILE_SCHEDULES)   # unknown widths: GPT-L's shapes by chain width
    key = tile_schedule_key(c.MTs, table)
    return None if key is None else table[key][kind]


@dataclass(frozen=True)
class GemmPlan:
    """One decode GEMM: `shape` of the tile family, or None for the skinny kernels.  `tiles` / `passes` are the skinny kernel's
    arguments (always there: what runs if the library refuses `shape`); `group_stats`: lgen_ssq_group4 in front of the launch."""
    shape: Optional[tuple]
    tiles: tuple
    passes: tuple
    group_stats: bool

    @property
    def family(self) -> str:
        return "skinny" if self.shape is None else "tile"


@dataclass(frozen=True)
class Plan:
    inputs: ScheduleInputs
    fuse_norm: bool
    gemms: Mapping[str, GemmPlan]

    def __getitem__(self, kind) -> GemmPlan:
        return self.gemms[kind]


def make_plan(c: ScheduleInputs, fuse_norm: bool, per_row_positions: bool = False, refused=()) -> Plan:
    parts = c.d // 16                                  # partial sums of squares per row of the fused-RMSNorm statistics
    fast_path = parts % 16 == 0 and parts <= 128       # the tile consumers stage such rows in LDS and sum contiguous quarters
    # rows the fast path does not take (GPT-3B: 200) are grouped once per consumer launch into their 4 lane-group sums
    # (parts % 4: lgen_ssq_group4 does not take the row; the consumer refuses it too)
    groupable = not (fast_path or parts % 4 or parts <= 4)
    gemms = {}
    for kind in KINDS:
        shape = tile_shape(c, fuse_norm, per_row_positions, refused, kind)
        if kind in NORM_KINDS and (not fuse_norm or (kind == "qkv" and per_row_positions)):
            shape = None                               # (an override cannot put a norm consumer without statistics on the family)
        tiles = skinny_tiles(c, fuse_norm, kind)
        gemms[kind] = GemmPlan(shape, tiles, skinny_passes(c, fuse_norm, kind, tiles),
                               shape is not None and kind in NORM_KINDS and groupable)
    return Plan(c, fuse_norm, gemms)


def gemm_schedule(plan: Plan) -> dict:
    """The kernel family and shapes the decode graph launches per GEMM kind (bench.py prints it; tests pin it)."""
    out = {}
    for name, kind in REPORT_NAMES.items():
        g = plan[kind]
        if g.shape is not None:
            out[name] = {"family": "tile", "shape(wm,wn,mtv,ntv,kb,stages,lw)": list(g.shape)}
        else:
            out[name] = {"family": "skinny", "tile(mt,nt,kw)": list(g.tiles), "passes": g.passes[0]}
    return out


def tile_schedule_source(plan: Plan) -> str:
    """Where the tile shapes of gemm_schedule() come from: "override" (LGEN_TILE_SHAPES), "table" (MODEL_TILE_SCHEDULES: measured
    and pinned per registry model), "table (GPT-L shapes by chain width)" (other widths), or "none" (chains below 256 rows / other
    storage types)."""
    c = plan.inputs
    if c.tile_shape_override:
        return "override"
    if not _tile_family_applies(c, plan.fuse_norm):
        return "none"
    return "table" if c.model in MODEL_TILE_SCHEDULES else "table (GPT-L shapes by chain width)"


def tile_schedule_tested(plan: Plan) -> bool:
    """True when every GEMM of the decode graph runs a schedule an end-to-end oracle test names (tests/test_gpu_headline.py):
    the skinny kernels (chains below 256 rows: the round-2/3 tests of every config) or a tested key of this model's tile table."""
    c = plan.inputs
    if all(plan[k].shape is None for k in KINDS):
        return not c.tile_shape_override and not c.tile_override and not c.pass_override
    table = MODEL_TILE_SCHEDULES.get(c.model)
    if table is None or tile_schedule_source(plan) != "table":
        return False
    return any(all((plan[k].shape or ()) == table[m][k] for k in KINDS) for m in TESTED_MODEL_SCHEDULES.get(c.model, ()))


def launches_per_step(plan: Plan) -> int:
    """Kernel launches of one captured decode step (embed + L layers + norm/lm_head + sampler): per GEMM one launch, plus a
    stand-alone RMSNorm in front of a norm consumer when the norm is not fused, plus lgen_ssq_group4 where the plan groups."""
    def consumer(kind):
        return 1 + (0 if plan.fuse_norm else 1) + (1 if plan[kind].group_stats else 0)
    per_layer = consumer("qkv") + 1 + 1 + consumer("w13") + 1      # wqkv, attention, wo, w1||w3, w2
    return 1 + plan.inputs.n_layer * per_layer + consumer("head") + 1
