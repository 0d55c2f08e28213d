"""Host logic of llamagen_amd.serve.ContinuousBatcher (no GPU): the request queue, slot refill between steps and the
"a request that entered at step k is complete after step k + N - 1" accounting.  The device step is a stand-in that writes
token = label * 1000 + step into the slot's sequence, exactly where lgen_sample_rows would."""
import pytest
import torch

from llamagen_amd.gpt import find_multiple
from llamagen_amd.serve import RECORD_WORDS, ContinuousBatcher, SamplingParams, bucket_ladder, pick_bucket, plan_moves
from tests.serve_standin import CPU_MODEL, _Batcher  # greedy unless told otherwise; its step asserts every request's K/V history


def test_requests_outnumbering_slots_are_all_served_in_full():
    cb = _Batcher(slots=3, N=5)
    labels = [7, 1, 9, 4, 2, 8, 3]
    rids = [cb.submit(l) for l in labels]
    done = cb.run(use_graph=False)
    assert sorted(done) == rids
    for rid, l in zip(rids, labels):
        assert done[rid].tolist() == [l * 1000 + s for s in range(5)]
    # 7 requests x 5 steps on 3 slots: slots are refilled the step after they finish, none idles while the queue has work
    assert cb.steps_run == len(cb.active_per_step) == 15 and sum(cb.active_per_step) == 35
    assert cb.active_per_step[:10] == [3] * 10
    assert all(r is None for r in cb._slot_req) and not cb._queue


def test_late_submissions_join_a_running_batch_without_cfg_rows():
    cb = _Batcher(slots=2, N=4, cfg=False)
    a = cb.submit(5)
    first = cb.run(use_graph=False)
    b, c, d = cb.submit(6), cb.submit(7), cb.submit(8)
    second = cb.run(use_graph=False)
    assert first[a].tolist() == [5000, 5001, 5002, 5003]
    assert sorted(second) == [b, c, d] and second[d].tolist() == [8000, 8001, 8002, 8003]
    assert cb.steps_run == 4 + 8


def test_submit_validates_label_and_noise():
    cb = _Batcher(slots=2, N=4)
    with pytest.raises(IndexError):
        cb.submit(1001)            # the reference's embedding lookup raises for labels outside the table (gpt.py:78-83)
    with pytest.raises(IndexError):
        cb.submit(-1)
    cb.submit(1000)                # the null class is a valid table row
    with pytest.raises(ValueError):
        cb.submit(3, noise=torch.ones(4, 32))   # greedy batcher (no noise buffer)
    cb.noise = torch.zeros(2, 4, 32)
    with pytest.raises(ValueError):
        cb.submit(3, noise=torch.ones(5, 32))
    cb.submit(3, noise=torch.ones(4, 32))


def test_bucket_ladder_choice_and_move_plan():
    assert bucket_ladder(64, None) == [64] and bucket_ladder(64, (32, 16, 16, 64)) == [16, 32, 64]
    with pytest.raises(ValueError):
        bucket_ladder(64, (0, 16))
    with pytest.raises(ValueError):
        bucket_ladder(64, (128,))
    assert [pick_bucket([16, 32, 64], n) for n in (0, 1, 16, 17, 32, 33, 64, 500)] == [16, 16, 16, 32, 32, 64, 64, 64]
    # growing keeps every index; shrinking keeps the low ones and fills the lowest free slots with the rest
    assert plan_moves([True, False, True, True], 8) == [(0, 0), (2, 2), (3, 3)]
    assert plan_moves([False, True, False, False, True, False, True, False], 4) == [(1, 1), (4, 0), (6, 2)]
    with pytest.raises(ValueError):
        plan_moves([True, True, True], 2)


@pytest.mark.parametrize("cfg", [True, False])
def test_buckets_grow_and_shrink_with_load_and_requests_keep_their_state(cfg):
    """slots=8 with captured slot counts 2 / 4 / 8: one request alone runs in the 2-slot bucket, a burst grows the batch at once,
    the tail shrinks it again after `shrink_after` steps; every request's K/V history, token and counters follow it through every
    switch (the stand-in step asserts that before each token), so every sequence comes out complete."""
    cb = _Batcher(slots=8, N=6, cfg=cfg, buckets=(2, 4), shrink_after=2)
    first = cb.submit(5)
    out = {}
    cb._load(0, *cb._queue.popleft())
    for _ in range(2):           # two steps alone in the smallest bucket
        cb._step(); cb.steps_run += 1; cb._account(out)
    assert cb.bucket_per_step == [2, 2]
    labels = [11, 12, 13, 14, 15, 16, 17, 18, 19, 20]
    rids = [cb.submit(l) for l in labels[:6]]
    out.update(cb.run(use_graph=False))          # 7 live -> the 8-slot bucket at once
    rids += [cb.submit(l) for l in labels[6:9]]
    out.update(cb.run(use_graph=False))          # 3 live -> 4 slots after shrink_after steps (requests move mid-sequence)
    rids.append(cb.submit(labels[9]))
    out.update(cb.run(use_graph=False))          # 1 live -> 2 slots
    assert sorted(out) == [first] + rids
    for rid, l in zip([first] + rids, [5] + labels):
        assert out[rid].tolist() == [l * 1000 + s for s in range(6)]
    assert cb.bucket_per_step[2] == 8 and 4 in cb.bucket_per_step and cb.bucket_per_step[-1] == 2
    assert cb.switches >= 3 and all(r is None for r in cb._slot_req)
    # no step ran more slots than its bucket holds, and every switch down waited for shrink_after steps of lower load
    assert all(a <= b for a, b in zip(cb.active_per_step, cb.bucket_per_step))


def test_single_bucket_never_switches():
    cb = _Batcher(slots=3, N=4)
    for l in (1, 2, 3, 4):
        cb.submit(l)
    cb.run(use_graph=False)
    assert cb.switches == 0 and set(cb.bucket_per_step) == {3}


@pytest.mark.parametrize("cfg", [True, False])
def test_shrinking_relocates_requests_from_high_slots(cfg):
    """Two requests running in slots 5 and 6 of the 8-slot bucket: after `shrink_after` steps they continue in slots 0 and 1 of
    the 2-slot bucket with their K/V rows, tokens, positions, class ids and token rows moved (the step asserts the history)."""
    cb = _Batcher(slots=8, N=7, cfg=cfg, buckets=(2,), shrink_after=3)
    cb._switch(cb._bucket(8))
    a, b = cb.submit(41), cb.submit(42)
    cb._load(5, *cb._queue.popleft())
    cb._load(6, *cb._queue.popleft())
    out = cb.run(use_graph=False)
    assert out[a].tolist() == [41000 + s for s in range(7)] and out[b].tolist() == [42000 + s for s in range(7)]
    assert cb.bucket_per_step == [8, 8, 2, 2, 2, 2, 2] and cb.switches == 2
    assert cb.row_step.tolist()[2:] == [7] * 6        # the vacated slots read as empty


def test_constructor_state():
    """The real constructor, reachable on the CPU through the stand-in's `_bucket`: sequence capacity, bucket ladder, the
    slot-indexed tensors and the defaults record."""
    cb = _Batcher(slots=8, N=6, cfg=True, greedy=False, buckets=(2, 4))
    assert cb.S8 == find_multiple(cb.T + 6, 8) == 8 and cb.V == 32 and cb.num_classes == 1000
    assert cb.bucket_sizes == [2, 4, 8] and cb.cur.B == 2 and cb.use_cfg and cb.B2 == 4
    assert cb.row_step.tolist() == [6] * 8 and cb.row_step.dtype == torch.int32
    assert tuple(cb.seq.shape) == (8, 6) and tuple(cb.logp.shape) == (8, 6) and tuple(cb.noise.shape) == (8, 6, 32)
    assert tuple(cb.params.shape) == (8, RECORD_WORDS) and (cb.seq.dtype, cb.logp.dtype, cb.params.dtype) == (torch.int32, torch.float32, torch.int32)
    assert cb.defaults == SamplingParams(cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=True)
    assert cb._cand == {} and cb._group == {} and cb._req_sampling == {}
    greedy = _Batcher(slots=8, N=6, cfg=True, greedy=True, buckets=(2, 4))
    assert greedy.noise is None and greedy.defaults.sample_logits is False


def test_a_cpu_model_is_refused_where_the_first_engine_would_be_built():
    with pytest.raises(RuntimeError, match=r"^llamagen_amd\.serve runs only on an AMD GPU through the HIP library \(no CPU fallback\)$"):
        ContinuousBatcher(CPU_MODEL, slots=2, max_new_tokens=4)


def test_fold_emb_masks_per_row_and_shared():
    """DecodeEngine.fold_emb_masks on a bare state object: a [B2, T] mask (generate, score) clears each row's own invalid caption
    columns, the batcher's [1, T] view the same columns of every row; the diagonal stays set and the attention is told to look."""
    import types
    from llamagen_amd.engine import DecodeEngine
    S8, T = 8, 3
    fresh = lambda: types.SimpleNamespace(causal_mask=torch.tril(torch.ones(S8, S8, dtype=torch.bool)).repeat(2, 1, 1),
                                          dev=torch.device("cpu"), S8=S8, use_mask=False)
    masks = torch.tensor([[0, 1, 1], [0, 0, 1]])
    for m in (masks, masks[1][None]):
        e = fresh()
        DecodeEngine.fold_emb_masks(e, m, T)
        want = fresh().causal_mask
        for r in range(2):
            want[r, :, :T] &= m[r % m.shape[0]].bool()
            want[r] |= torch.eye(S8, dtype=torch.bool)
        assert torch.equal(e.causal_mask, want) and e.use_mask is True
    e = fresh()
    DecodeEngine.fold_emb_masks(e, None, T)
    assert torch.equal(e.causal_mask, fresh().causal_mask) and e.use_mask is False
