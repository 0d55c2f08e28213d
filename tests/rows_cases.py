"""Input builders of the per-row-position kernel tests (tests/test_gpu_rows.py) and of their host checks
(tests/test_rows_cases_host.py): position lists, left-padded caption masks, wide-score q / k.  Plain torch on the CPU, no GPU and
no library import, so that the properties the GPU tests rely on are asserted without a device."""
import math

import torch

GRID = 24
S8 = 584                      # find_multiple(1 + GRID * GRID, 8): cache slots of a 24 x 24 class-conditional model


def find_multiple(n, k):
    return n if n % k == 0 else n + k - (n % k)


def mtiles(M):
    """m-tiles allocated for M rows (tests/test_gpu_gpt.py::test_gemm_rows_packed_res): 3 become 4, above 4 a multiple of 8."""
    mts = (M + 15) // 16
    mts = {3: 4}.get(mts, mts)
    if mts > 4:
        mts = (mts + 7) // 8 * 8
    return mts


def pad_positions(live, mts, s8):
    """row_pos of a launch: the live rows' positions, then S8 - 1 (a valid cache slot) for the rows in [M, MTs * 16)."""
    return list(live) + [s8 - 1] * (mts * 16 - len(live))


# ---- section 1: lgen_embed_rows ------------------------------------------------------------------------------------------
def embed_positions(M, seed):
    """Half of the rows at position 0 (fresh requests), the others mid-sequence; shuffled inside every m-tile so that each
    m-tile holds both kinds."""
    g = torch.Generator().manual_seed(seed)
    pos = []
    for m0 in range(0, M, 16):
        n = min(16, M - m0)
        tile = [0 if i % 2 == 0 else 1 + (7 * (m0 + i)) % 500 for i in range(n)]
        pos += [tile[i] for i in torch.randperm(n, generator=g).tolist()]
    return pos


# ---- section 2: lgen_gemm_qkv_rope_rows ----------------------------------------------------------------------------------
QKV_POSITIONS = (0, 1, 17, 301, S8 - 1)
# Seeds for which qkv_positions() has the two properties test_rows_cases_host.py asserts (found by trying 0, 1, 2, ...).
QKV_SEED = {33: 0, 40: 0, 64: 0}


def qkv_positions(M, seed=None):
    """Each live row's position from QKV_POSITIONS (cycled to M entries), assigned by a seeded permutation."""
    seed = QKV_SEED[M] if seed is None else seed
    g = torch.Generator().manual_seed(1000 + seed)
    vals = [QKV_POSITIONS[i % len(QKV_POSITIONS)] for i in range(M)]
    return [vals[i] for i in torch.randperm(M, generator=g).tolist()]


def qkv_position_properties(live, M, mts, mt, s8=S8):
    """(every m-tile with >= 3 live rows holds >= 3 distinct live positions,
        no two m-tiles of one workgroup tile (mt consecutive m-tiles) hold the same 16-entry sequence)."""
    rp = pad_positions(live, mts, s8)
    tiles = [rp[i * 16:(i + 1) * 16] for i in range(mts)]
    distinct = all(len(set(t[:max(0, min(16, M - i * 16))])) >= 3 for i, t in enumerate(tiles) if M - i * 16 >= 3)
    differ = all(len({tuple(t) for t in tiles[w:w + mt]}) == len(tiles[w:w + mt]) for w in range(0, mts, mt))
    return distinct, differ


# ---- section 3a: kv-length boundaries ------------------------------------------------------------------------------------
ATTN_POSITIONS = (0, 1, 2, 3, 4, 6, 7, 8, 14, 15, 16, 17, 30, 31, 32, 33, 62, 63, 64, 65, 126, 127, 128, 129, 255, 256, 257, 300,
                  383, 384, 385, S8 - 2, S8 - 1)
ATTN_CROSS_POSITIONS = (0, 129, S8 - 1)      # compared bit for bit with the one-position entry point


def attn_positions(B2, seed):
    """ATTN_POSITIONS, repeated from its start up to B2 rows, shuffled."""
    g = torch.Generator().manual_seed(seed)
    vals = [ATTN_POSITIONS[i % len(ATTN_POSITIONS)] for i in range(B2)]
    return [vals[i] for i in torch.randperm(B2, generator=g).tolist()]


def cycle_positions(B2, lo, hi, seed):
    """Positions lo..hi (inclusive) cycled over B2 rows from a seeded offset, shuffled (section 3b)."""
    g = torch.Generator().manual_seed(seed)
    off = int(torch.randint(0, hi - lo + 1, (1,), generator=g))
    vals = [lo + (off + i) % (hi - lo + 1) for i in range(B2)]
    return [vals[i] for i in torch.randperm(B2, generator=g).tolist()]


def random_key_mask(B2, s8, seed=13):
    """The mask of test_qkv_rope_append_and_attention: causal, a random 30 % of the keys of every row dropped, diagonal kept."""
    mask = torch.tril(torch.ones(s8, s8, dtype=torch.bool)).unsqueeze(0).repeat(B2, 1, 1)
    mask &= torch.rand(B2, 1, s8, generator=torch.Generator().manual_seed(seed)) > 0.3
    mask |= torch.eye(s8, dtype=torch.bool)
    return mask


# ---- section 3c: left-padded caption masks -------------------------------------------------------------------------------
CAPTION_T = 120
CAPTION_S8 = find_multiple(CAPTION_T + GRID * GRID, 8)           # 696
CAPTION_LENS = (1, 2, 7, 8, 9, 33, 64, 119, 120) * 2               # valid caption tokens per row, left-padded
CAPTION_SCALAR_POS = CAPTION_T + 200


def caption_emb_masks(T=CAPTION_T, lens=CAPTION_LENS):
    """emb_masks [B, T]: valid tokens at the END of the prefix."""
    mk = torch.zeros(len(lens), T, dtype=torch.int64)
    for b, n in enumerate(lens):
        mk[b, T - n:] = 1
    return mk


def caption_masks(T=CAPTION_T, lens=CAPTION_LENS, s8=CAPTION_S8):
    """[B, S8, S8] bool: causal AND (key >= T - len_b) for the prefix keys, with the diagonal kept."""
    key = torch.arange(s8)
    causal = key[None, :] <= key[:, None]
    rows = []
    for n in lens:
        vis = (key >= T - n) | (key >= T)
        rows.append((causal & vis[None, :]) | torch.eye(s8, dtype=torch.bool))
    return torch.stack(rows)


def caption_positions(B2, T=CAPTION_T, s8=CAPTION_S8):
    """Positions spread evenly over [T - 1, S8 - 1], both ends included; neighbours of the same caption length far apart."""
    return [T - 1 + round(i * (s8 - T) / (B2 - 1)) for i in range(B2)]


def poison_mask_tail(mask, T=CAPTION_T):
    """The buffer a mask_len = T launch gets: bytes of keys >= T cleared (only keys < mask_len may consult the mask)."""
    m = mask.clone()
    m[:, :, T:] = False
    return m


# ---- section 3d: wide score range ----------------------------------------------------------------------------------------
# q is multiplied by WIDE_S[storage] so that scores have a standard deviation of that many units, and one key per row is planted
# whose score exceeds every other visible key's by WIDE_MARGIN (> 30).  WIDE_S is the largest of (2, 4, 8) for which the fp32
# oracle sdpa_math, rounded to the storage type, stays within HALF of the _close default bars of a float64 softmax over the same
# stored operands (tests/test_rows_cases_host.py::test_wide_scale_leaves_the_kernel_half_of_the_bars asserts it for the chosen
# value and prints the distance).  With the planted key the softmax collapses onto one key and the condition is trivially met, so
# the same q, k, v WITHOUT the planted key (wide_inputs(plant=False)) must meet it too, and the GPU test runs both.  Every candidate
# passed for every storage type, so s = 8 everywhere.  Measured oracle-vs-float64 distance at s = 8 (max |err| / largest |ref|, and
# the share of elements that round differently; half bars: 1e-5 for fp32, about 2^-8 / 2^-11 of the value and a share of 1e-2):
#   fp32  planted 1.4e-15, not planted 9.1e-07
#   bf16  planted 1.8e-15, not planted 2.3e-03 (the rounding of the result itself), 2.0e-04 of the elements
#   fp16  planted 1.8e-15, not planted 2.9e-04 (the rounding of the result itself), 1.9e-03 of the elements
WIDE_CANDIDATES = (2, 4, 8)
WIDE_S = {"fp32": 8, "bf16": 8, "fp16": 8}
WIDE_MARGIN = 35.0
WIDE_SCALAR_POS = 300
# the planted key of a row, by row % 3: 0 -> in the first group (key 1), 1 -> the row's last key (its last group), 2 -> the middle of
# a wave's SECOND round: keys 40 / 144 (16-bit storage) or 20 / 72 (fp32), alternating -- 16-bit: variants 2, 5, 6 fold keys
# 32..63 and variant 0 keys 128..255 in round two; fp32 (groups half as long): 16..31 and 64..127.  Clamped to the row's position.
WIDE_SECOND_ROUND = {"fp32": (20, 72), "bf16": (40, 144), "fp16": (40, 144)}


def wide_planted_keys(positions, storage):
    keys = []
    for m, p in enumerate(positions):
        if m % 3 == 0:
            k = 1
        elif m % 3 == 1:
            k = p
        else:
            k = WIDE_SECOND_ROUND[storage][(m // 3) % 2]
        keys.append(min(k, p))
    return keys


def _rand(shape, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt)


def wide_inputs(dt, storage, positions, H, hd, s8, s, plant=True):
    """q [B2, H, hd] (scaled by s), k, v [B2, H, S8, hd] in the storage type, with the planted key of every (row, head): k at that
    slot is c * q with c chosen in float64, from the STORED operands, so that its score leads the row's other visible keys by
    WIDE_MARGIN.  plant = False: the same q, k, v without the planted key (the softmax then spreads over several keys instead of
    collapsing onto one, so the summation order of the kernel shows in the result).  Returns q, k, v, planted keys."""
    B2 = len(positions)
    q = (_rand((B2, H, hd), torch.float32, 51) * s).to(dt)
    k = _rand((B2, H, s8, hd), dt, 52)
    v = _rand((B2, H, s8, hd), dt, 53)
    keys = wide_planted_keys(positions, storage)
    if not plant:
        return q, k, v, keys
    sc = torch.einsum("bhd,bhsd->bhs", q.double(), k.double()) / math.sqrt(hd)
    for b, (p, kp) in enumerate(zip(positions, keys)):
        vis = torch.ones(s8, dtype=torch.bool)
        vis[p + 1:] = False
        vis[kp] = False
        for h in range(H):
            top = sc[b, h][vis].max().item() if vis.any() else 0.0
            qq = q[b, h].double()
            c = (top + WIDE_MARGIN) * math.sqrt(hd) / float(qq @ qq)
            k[b, h, kp] = (qq * c).to(dt)
    return q, k, v, keys


def wide_margin(q, k, positions, keys):
    """Smallest lead (float64, stored operands) of the planted key over the other visible keys of its (row, head)."""
    hd = q.shape[-1]
    sc = torch.einsum("bhd,bhsd->bhs", q.double(), k.double()) / math.sqrt(hd)
    lead = float("inf")
    for b, (p, kp) in enumerate(zip(positions, keys)):
        if p == 0:
            continue
        others = torch.ones(sc.shape[-1], dtype=torch.bool)
        others[p + 1:] = False
        others[kp] = False
        lead = min(lead, (sc[b, :, kp] - sc[b][:, others].max(-1).values).min().item())
    return lead


def visible_rows(positions, s8):
    """[B2, 1, 1, S8] bool: keys <= the row's own position."""
    return (torch.arange(s8)[None, :] <= torch.tensor(positions)[:, None])[:, None, None, :]


def sdpa_f64(q, k, v, mask):
    """The softmax attention of oracle.sdpa_math evaluated in float64 on the same stored operands (no rounding of the result)."""
    hd = q.shape[-1]
    att = (q.double() @ k.double().transpose(-2, -1)) / math.sqrt(hd)
    att = att.masked_fill(~mask, float("-inf"))
    return torch.softmax(att, dim=-1) @ v.double()


def half_bar_distance(got, ref64, dt):
    """`got` (storage-type values) against an unrounded float64 reference under HALF of the default bars of
    tests/test_gpu_gpt.py::_close.  Returns (ok, max |err| / largest |ref|, share of elements that round differently)."""
    got, ref64 = got.double(), ref64.double()
    err = (got - ref64).abs()
    scale = ref64.abs().max().item() + 1e-30
    if dt == torch.float32:
        return err.max().item() <= 0.5 * 2e-5 * max(1.0, scale), err.max().item() / scale, 0.0
    base = torch.maximum(ref64.abs(), got.abs())
    ulp = base * (2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10) + 2e-5 * scale
    if dt == torch.float16:
        ulp = ulp + 2.0 ** -11 * scale
    flips = (got != ref64.float().to(dt).double()).double().mean().item()
    ok = bool((err <= 0.5 * ulp * 1.01).all()) and flips <= 0.5 * 0.02
    return ok, err.max().item() / scale, flips


# ---- the workgroup variants of lgen_attn_decode (ATTN_VARIANTS of csrc/gpt_ops.hip, entries 0..7) as data ---------------
# (ch: K/V loads per buffer, nw: waves per (row, head), hpw: heads per workgroup); a group is ch * 64 / (hdp / EPL) keys with
# EPL = 8 elements per 16-byte piece for 16-bit storage, 4 for fp32.
WORKGROUP_VARIANTS = ((4, 4, 1), (2, 4, 1), (2, 2, 1), (4, 2, 1), (2, 1, 1), (4, 1, 1), (2, 2, 2), (2, 2, 4))
PERSISTENT_VARIANTS = (8, 9, 10, 11, 12, 13, 14)
STORAGE_EPL = {"fp32": 4, "bf16": 8, "fp16": 8}


def group_keys(storage, hdp, ch):
    return ch * 64 // (hdp // STORAGE_EPL[storage])
