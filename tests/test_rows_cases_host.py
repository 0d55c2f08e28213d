"""Host checks (no GPU) of the inputs tests/test_gpu_rows.py feeds the per-row-position kernels: the properties those tests rely
on are asserted here, on the CPU, from the same builders (tests/rows_cases.py)."""
import pytest
import torch

from oracle import llamagen_oracle as O
from tests import rows_cases as RC

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def test_shared_constants_match_the_oracle():
    assert RC.S8 == O.find_multiple(1 + RC.GRID * RC.GRID, 8)
    assert RC.CAPTION_S8 == O.find_multiple(RC.CAPTION_T + RC.GRID * RC.GRID, 8)
    assert [RC.mtiles(M) for M in (1, 16, 17, 33, 40, 64, 65, 256)] == [1, 1, 2, 4, 4, 4, 8, 16]


@pytest.mark.parametrize("M", [37, 40])
def test_embed_positions_mix_fresh_and_running_rows_in_every_m_tile(M):
    pos = RC.embed_positions(M, 61)
    assert len(pos) == M and max(pos) < RC.S8 - 1          # the padding rows' position S8 - 1 is no live row's
    for m0 in range(0, M, 16):
        tile = pos[m0:m0 + 16]
        assert 0 in tile and any(p != 0 for p in tile), m0


# (M, mt) of the five cases of test_qkv_rope_rows_vs_oracle_and_scalar_entry
@pytest.mark.parametrize("M,mt", [(40, 2), (64, 4), (33, 4)])
def test_qkv_positions_differ_inside_and_between_m_tiles(M, mt):
    live = RC.qkv_positions(M)
    mts = RC.mtiles(M)
    assert len(live) == M and set(live) == set(RC.QKV_POSITIONS) and mts % mt == 0
    assert all(0 <= p < RC.S8 for p in live)
    distinct, differ = RC.qkv_position_properties(live, M, mts, mt)
    assert distinct, "an m-tile holds fewer than 3 distinct positions"
    assert differ, "two m-tiles of one workgroup tile hold the same sequence of positions"
    # the same list is a permutation of the cycled position set: every position on about M / 5 rows
    assert all(live.count(p) >= M // len(RC.QKV_POSITIONS) for p in RC.QKV_POSITIONS)


@pytest.mark.parametrize("storage", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("hdp", [64, 128])
def test_attn_positions_straddle_every_group_boundary(storage, hdp):
    """kv length = position + 1: one below, at and above the group size and waves x group size of every workgroup variant."""
    lens = {p + 1 for p in RC.ATTN_POSITIONS}
    assert max(lens) == RC.S8 and all(1 <= n <= RC.S8 for n in lens)
    sizes = set()
    for ch, nw, hpw in RC.WORKGROUP_VARIANTS:
        gk = RC.group_keys(storage, hdp, ch)
        assert 4 <= gk <= 32 and nw * gk <= 128
        sizes |= {gk, nw * gk}
        assert max(lens) > 2 * 2 * nw * gk                  # beyond two rounds of the double buffer
    for n in sizes:
        assert {n - 1, n, n + 1} <= lens, (storage, hdp, n)
    for B2 in (40,):
        pos = RC.attn_positions(B2, 7)
        assert set(pos) == set(RC.ATTN_POSITIONS) and len(pos) == B2
        assert all(p in pos for p in RC.ATTN_CROSS_POSITIONS)


class _MaskOnly(O.GPTOracle):
    """The oracle with a stand-in forward: generate() still builds its causal_mask from emb_masks (generate.py:154-163)."""
    def forward(self, idx, cond, input_pos):
        return torch.zeros(idx.shape[0] if cond is None else cond.shape[0], len(input_pos), 8)


def test_caption_masks_are_what_generate_builds():
    T, S = RC.CAPTION_T, RC.CAPTION_S8
    em = RC.caption_emb_masks()
    mask = RC.caption_masks()
    B = em.shape[0]
    assert tuple(mask.shape) == (B, S, S) and em.sum(1).tolist() == list(RC.CAPTION_LENS)
    assert bool(torch.diagonal(mask, dim1=1, dim2=2).all())
    cfg = O.GPTConfig(dim=8, n_layer=1, n_head=1, vocab_size=8, block_size=RC.GRID * RC.GRID, cls_token_num=T, caption_dim=4,
                      model_type="t2i")
    model = _MaskOnly(cfg, {})
    O.generate(model, torch.zeros(B, T, 4), RC.GRID * RC.GRID, emb_masks=em, cfg_scale=1.0, sample_logits=False)
    assert torch.equal(model.causal_mask, mask)
    # a long hidden prefix: the row of a 1-token caption sees key T - 1 and the image tokens only
    assert mask[0, T + 5].nonzero().flatten().tolist() == list(range(T - 1, T + 6))
    pos = RC.caption_positions(B)
    assert pos[0] == T - 1 and pos[-1] == S - 1 and sorted(pos) == pos and len(set(pos)) == B
    poisoned = RC.poison_mask_tail(mask)
    assert not poisoned[:, :, T:].any() and torch.equal(poisoned[:, :, :T], mask[:, :, :T])


@pytest.mark.parametrize("storage", ["fp32", "bf16", "fp16"])
def test_wide_scale_leaves_the_kernel_half_of_the_bars(storage):
    """WIDE_S[storage] is the LARGEST candidate for which the fp32 oracle stays within half of the _close default bars of a
    float64 softmax on the same stored operands; the planted key leads by more than 30 for every candidate."""
    dt = DT[storage]
    sets = (RC.attn_positions(40, 7), [RC.WIDE_SCALAR_POS] * 40)     # the per-row launches, the one-position launches
    passing = []
    for s in RC.WIDE_CANDIDATES:
        oks = []
        for positions, plant in ((p, f) for p in sets for f in (True, False)):
            mask = RC.visible_rows(positions, RC.S8)
            q, k, v, keys = RC.wide_inputs(dt, storage, positions, 4, 64, RC.S8, s, plant=plant)
            sc = torch.einsum("bhd,bhsd->bhs", q.double(), k.double()) / 8.0
            if plant:
                assert RC.wide_margin(q, k, positions, keys) > 30.0, s
            else:
                assert sc.std().item() >= 0.9 * s
            ref = O.sdpa_math(q[:, :, None], k, v, mask, dt)
            ok, dist, flips = RC.half_bar_distance(ref, RC.sdpa_f64(q[:, :, None], k, v, mask), dt)
            print(f"{storage} s={s} rows={len(set(positions)) > 1} planted={plant}: oracle vs float64 max|err|/max|ref| = {dist:.3e}, "
                  f"elements rounding differently = {flips:.2e}, ok = {ok}")
            oks.append(ok)
        if all(oks):
            passing.append(s)
    assert passing and RC.WIDE_S[storage] == max(passing), (storage, passing)
    # the three kinds of planted key are all present, also among the rows long enough not to be clamped
    positions = sets[0]
    keys = RC.wide_planted_keys(positions, storage)
    a, b = RC.WIDE_SECOND_ROUND[storage]
    assert 1 in keys and a in keys and b in keys and any(k == p and p > b for k, p in zip(keys, positions))
