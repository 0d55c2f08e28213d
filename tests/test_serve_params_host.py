"""Per-request sampling parameters of llamagen_amd.serve (no GPU): SamplingParams validation, the 32-byte slot record, submit()'s
refusals, and the record's life in the slot table -- written at load, moved with a relocating shrink, replaced at refill.  The
device step is the stand-in of tests/test_serve_host.py (token = label * 1000 + step)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from llamagen_amd import _lib as L
from llamagen_amd.serve import RECORD_WORDS, RequestOutput, SamplingParams, pack_sampling, pick_best
from tests import serve_standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Mirror(ctypes.Structure):  # lgen_slot_sampling as include/lgen.h spells it
    _fields_ = [("cfg_scale", ctypes.c_float), ("temperature", ctypes.c_float), ("top_p", ctypes.c_float),
                ("cfg_interval", ctypes.c_int), ("top_k", ctypes.c_int), ("greedy", ctypes.c_int), ("reserved", ctypes.c_int * 2)]


def test_sampling_params_validation():
    sp = SamplingParams()
    assert (sp.cfg_scale, sp.cfg_interval, sp.temperature, sp.top_k, sp.top_p, sp.sample_logits, sp.seed) == (1.0, -1, 1.0, 0, 1.0, True, None)
    SamplingParams(cfg_scale=7.5, cfg_interval=3, temperature=1e-6, top_k=16384, top_p=1.0, sample_logits=False, seed=7)
    SamplingParams(top_p=1e-3)
    for bad in (dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.0001), dict(top_k=-1), dict(top_p=float("nan")),
                dict(temperature=float("inf")), dict(temperature=float("nan")), dict(cfg_scale=float("nan")),
                dict(cfg_scale=float("-inf")), dict(top_k=2.5)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)


def test_record_is_the_32_byte_struct_of_the_header():
    assert ctypes.sizeof(_Mirror) == 32 == ctypes.sizeof(L.SlotSampling) and RECORD_WORDS == 8
    assert [(n, t) for n, t, *_ in L.SlotSampling._fields_][:6] == [(n, t) for n, t, *_ in _Mirror._fields_][:6]
    # the header's typedef: same field order, floats first
    txt = open(os.path.join(ROOT, "include", "lgen.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} lgen_slot_sampling;", txt)
    assert m, "lgen_slot_sampling is not declared"
    names = [n.strip().split("[")[0] for part in m.group(1).split(";") if part.strip()
             for n in part.strip().split(None, 1)[1].split(",")]
    assert names == ["cfg_scale", "temperature", "top_p", "cfg_interval", "top_k", "greedy", "reserved"]
    assert names == [f[0] for f in _Mirror._fields_]
    w = pack_sampling(SamplingParams(cfg_scale=1.75, cfg_interval=5, temperature=0.7, top_k=50, top_p=0.9, sample_logits=False, seed=3))
    assert w.dtype == np.int32 and w.shape == (8,)
    rec = _Mirror.from_buffer_copy(w.tobytes())
    assert (rec.cfg_scale, rec.temperature, rec.top_p) == (np.float32(1.75), np.float32(0.7), np.float32(0.9))
    assert (rec.cfg_interval, rec.top_k, rec.greedy, list(rec.reserved)) == (5, 50, 1, [0, 0])
    assert w[:3].view(np.float32).tolist() == [np.float32(1.75), np.float32(0.7), np.float32(0.9)] and w[3:].tolist() == [5, 50, 1, 0, 0]
    assert _Mirror.from_buffer_copy(pack_sampling(SamplingParams()).tobytes()).greedy == 0


def test_new_symbol_is_declared_and_has_a_signature():
    txt = open(os.path.join(ROOT, "include", "lgen.h")).read()
    assert re.search(r"^int\s+lgen_sample_rows_params\s*\(", txt, flags=re.M)
    assert len(L.SIGNATURES["lgen_sample_rows_params"]) == 14
    assert "#define LGEN_ABI_VERSION 10" in txt and L.ABI_VERSION == 10      # additive: the version does not move


_Batcher = functools.partial(serve_standin._Batcher, greedy=False)   # sampled unless told otherwise; its step records `params`


def _words(sp):
    return pack_sampling(sp).tolist()


def test_submit_refusals():
    unguided = _Batcher(slots=2, N=4, cfg=False)
    with pytest.raises(ValueError):
        unguided.submit(3, sampling=SamplingParams(cfg_scale=4.0))      # no unconditional rows in this batcher
    unguided.submit(3, sampling=SamplingParams(cfg_scale=1.0, temperature=0.5))
    greedy = _Batcher(slots=2, N=4, greedy=True)
    with pytest.raises(ValueError):
        greedy.submit(3, sampling=SamplingParams(cfg_scale=4.0, sample_logits=True))   # no noise buffer in this batcher
    greedy.submit(3, sampling=SamplingParams(cfg_scale=4.0, sample_logits=False))
    with pytest.raises(TypeError):
        greedy.submit(3, sampling=dict(cfg_scale=4.0))
    assert len(unguided._queue) == 1 and len(greedy._queue) == 1
    assert all(len(entry) == 3 for entry in greedy._queue)             # the queue entries stay (rid, label, noise)


def test_records_sit_in_their_slots_and_are_replaced_at_refill():
    cb = _Batcher(slots=2, N=3)
    sps = [SamplingParams(cfg_scale=4.0, temperature=0.7), None, SamplingParams(cfg_scale=1.0, top_k=1, sample_logits=False),
           SamplingParams(cfg_scale=1.75, cfg_interval=1, top_p=0.5), None]
    rids = [cb.submit(10 + i, sampling=sp) for i, sp in enumerate(sps)]
    done = cb.run(use_graph=False)
    assert sorted(done) == rids
    for rid, sp in zip(rids, sps):
        want = _words(sp if sp is not None else cb.defaults)             # a request that brings none gets the constructor's values
        seen = cb.records_seen[rid]
        assert len(seen) == 3 and all(w == want for _, w in seen), rid
    # 5 requests on 2 slots: every slot was refilled, and each refill replaced the record
    assert {b for b, _ in cb.records_seen[rids[0]]} == {0} and {b for b, _ in cb.records_seen[rids[2]]} == {0}
    assert cb.records_seen[rids[0]][0][1] != cb.records_seen[rids[2]][0][1]
    assert not cb._req_sampling                                          # the side table is emptied as requests load


def test_record_follows_a_request_through_a_relocating_shrink():
    cb = _Batcher(slots=8, N=7, buckets=(2,), shrink_after=3)
    cb._switch(cb._bucket(8))
    spa, spb = SamplingParams(cfg_scale=1.0, temperature=0.7, top_p=0.9), SamplingParams(cfg_scale=3.0, top_k=5, sample_logits=False)
    a, b = cb.submit(41, sampling=spa), cb.submit(42, sampling=spb)
    cb._load(5, *cb._queue.popleft())
    cb._load(6, *cb._queue.popleft())
    assert cb.params[5].tolist() == _words(spa) and cb.params[6].tolist() == _words(spb)
    out = cb.run(use_graph=False)
    assert out[a].tolist() == [41000 + s for s in range(7)] and out[b].tolist() == [42000 + s for s in range(7)]
    assert cb.switches == 2
    assert [s for s, _ in cb.records_seen[a]] == [5, 5, 0, 0, 0, 0, 0] and [s for s, _ in cb.records_seen[b]] == [6, 6, 1, 1, 1, 1, 1]
    assert all(w == _words(spa) for _, w in cb.records_seen[a]) and all(w == _words(spb) for _, w in cb.records_seen[b])


def test_the_stand_in_without_new_attributes_still_takes_sampling():
    """The greedy stand-in of tests/test_serve_host.py (built by the real constructor like every other: it has defaults and a
    record table) serves one request that brings sampling values and one that brings none."""
    from tests.test_serve_host import _Batcher as Plain
    cb = Plain(slots=2, N=3)
    rid = cb.submit(7, sampling=SamplingParams(cfg_scale=2.0, sample_logits=False))
    plain = cb.submit(8)
    done = cb.run(use_graph=False)
    assert done[rid].tolist() == [7000, 7001, 7002] and done[plain].tolist() == [8000, 8001, 8002]


@pytest.mark.parametrize("plain_first", [False, True])
@pytest.mark.parametrize("full", [False, True])
def test_best_of_answers_with_the_likeliest_candidate(full, plain_first):
    """best_of=3 next to a plain request on 3 slots (the fewest check_best_of admits for three candidates; with the plain request
    ahead of them the last candidate waits for a refill and finishes after the others): the candidates run as requests of their
    own (the stand-in step gives candidate j tokens + 100 * (j + 1) and the per-token log-probability chosen here), the answer
    under the request's id is the one pick_best names, and nothing is left in the candidate tables."""
    per_token = [-1.0, -0.25, -0.5]
    cb = _Batcher(slots=3, N=4)
    with pytest.raises(ValueError):
        _Batcher(slots=2, N=4).submit(7, sampling=SamplingParams(best_of=3, seed=5))   # a candidate without a slot of its own
    if plain_first:
        plain = cb.submit(8)
    rid = cb.submit(7, sampling=SamplingParams(best_of=3, seed=5))
    if not plain_first:
        plain = cb.submit(8)
    assert sorted(cb._cand.values()) == [(rid, 0), (rid, 1), (rid, 2)] and len(cb._queue) == 4
    assert sorted(cb._req_sampling[c].seed for c in cb._cand) == [5, 6, 7] and all(cb._req_sampling[c].best_of == 1 for c in cb._cand)
    for cid, (_, j) in cb._cand.items():
        cb.marks[cid] = (100 * (j + 1), per_token[j])
    done = cb.run(use_graph=False, return_outputs=full)
    win = pick_best([4 * lp for lp in per_token])
    assert win == 1 and sorted(done) == sorted([rid, plain]) and cb.steps_run == 8
    want = [7000 + 100 * (win + 1) + s for s in range(4)]
    if full:
        assert isinstance(done[rid], RequestOutput) and done[rid].token_ids.tolist() == want
        assert done[rid].logprobs.tolist() == [per_token[win]] * 4 and done[rid].cumulative_logprob.item() == 4 * per_token[win]
        assert done[plain].token_ids.tolist() == [8000 + s for s in range(4)] and done[plain].cumulative_logprob.item() == 0.0
    else:
        assert done[rid].tolist() == want and done[plain].tolist() == [8000 + s for s in range(4)]
    assert not cb._cand and not cb._group and not cb._req_sampling and all(r is None for r in cb._slot_req)
