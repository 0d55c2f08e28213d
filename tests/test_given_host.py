"""CPU-only: image completion's host side -- the `given` argument's validation, the prefix-length function, the two new entry
points of the C ABI, the batcher's slot-indexed `given` rows through bucket switches (stand-in of tests/serve_standin.py), and the
MARGINS: every (case, pattern) tests/test_gpu_given.py holds token-exact through the prefix fast path is run through the oracle
loop of tests/given_cases.py here, and must decide every free step by more than 1e-3 (see that module's docstring)."""
import os
import re

import pytest
import torch

from tests import given_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lgen_sample_given", "lgen_sample_rows_params_given")


# ---- the argument ------------------------------------------------------------------------------------------------------------------
def test_check_given_shape_range_dtype():
    from llamagen_amd.given import check_given
    ok = torch.tensor([[-1, 0, 1023], [5, -1, -1]])
    for dt in (torch.int64, torch.int32, torch.int16):
        out = check_given(ok.to(dt), (2, 3), 1024)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.tolist() == ok.tolist()
    assert check_given(ok.t().contiguous().t(), (2, 3), 1024).is_contiguous()                # a strided view comes out packed
    for bad in (ok[:, :2], ok[0], ok.view(1, 2, 3)):                                          # shape
        with pytest.raises(ValueError):
            check_given(bad, (2, 3), 1024)
    for v in (-2, 1024, 1 << 20):                                                             # range: -1 or [0, vocab)
        g = ok.clone()
        g[1, 2] = v
        with pytest.raises(ValueError):
            check_given(g, (2, 3), 1024)
    for bad in (ok.float(), ok >= 0, ok.tolist(), None):                                      # dtype
        with pytest.raises(ValueError):
            check_given(bad, (2, 3), 1024)


def test_generate_validates_given_before_any_launch():
    """A CPU model: generate() would raise RuntimeError at setup_caches (no CPU fallback); a bad `given` is a ValueError before."""
    from llamagen_amd import generate
    from llamagen_amd.gpt import ModelArgs, Transformer
    m = Transformer(ModelArgs(n_layer=1, n_head=2, dim=64, vocab_size=64, block_size=4, num_classes=3))
    cond = torch.tensor([0, 1])
    for bad in (torch.full((2, 3), -1), torch.full((1, 4), -1), torch.full((2, 4), 64), torch.full((2, 4), -2), torch.zeros(2, 4)):
        with pytest.raises(ValueError):
            generate(m, cond, 4, given=bad)
    with pytest.raises(ValueError):       # chains of several batches take no given tokens
        generate(m, cond, 4, given=torch.full((2, 4), -1), _more_conds=[cond])
    with pytest.raises(RuntimeError):     # a valid one gets as far as the device
        generate(m, cond, 4, given=torch.full((2, 4), -1))
    with pytest.raises(TypeError):        # unknown keywords are still refused
        generate(m, cond, 4, givens=torch.full((2, 4), -1))


def test_given_prefix_length():
    from llamagen_amd.given import given_prefix_length as P
    F = -1
    assert P(torch.tensor([[F, F, F, F]])) == 0                                   # nothing given
    assert P(torch.tensor([[F, 3, 3, 3], [2, 2, 2, 2]])) == 0                     # no common prefix: one row starts free
    assert P(torch.tensor([[1, F, F, F], [1, 2, F, F]])) == 1                     # ragged rows: the shortest decides
    assert P(torch.tensor([[1, 2, 3, F], [1, 2, F, 9], [4, 4, 4, 4]])) == 2
    assert P(torch.tensor([[1, 2, F, 4], [1, 2, F, 4]])) == 2                     # given tokens behind a hole do not count
    assert P(torch.tensor([[1, 2, 3, 4], [5, 6, 7, 8]])) == 3                     # all given: capped at N - 1
    assert P(torch.tensor([[7]])) == 0 and P(torch.tensor([[F]])) == 0            # N = 1: the one token goes through the sampler
    assert P(torch.zeros(0, 4, dtype=torch.int32)) == 0
    for name, pat in G.PATTERNS.items():
        g = torch.where(pat, torch.tensor(7), torch.tensor(F)).expand(3, -1)
        assert P(g) == G.PATTERN_P[name], name


def test_keep_to_given_rows_and_mask():
    from llamagen_amd.given import keep_to_given
    idx = torch.arange(24).view(2, 12)
    top = keep_to_given(idx, 2, (3, 4))
    assert top.dtype == torch.int32 and top[:, :8].tolist() == idx[:, :8].tolist() and (top[:, 8:] == -1).all()
    assert (keep_to_given(idx, 0, (3, 4)) == -1).all() and keep_to_given(idx, 3, (3, 4)).tolist() == idx.tolist()
    mask = torch.zeros(3, 4, dtype=torch.bool)
    mask[:, 0] = True                                                            # a kept left strip
    strip = keep_to_given(idx, mask, (3, 4))
    assert strip[:, ::4].tolist() == idx[:, ::4].tolist() and int((strip >= 0).sum()) == 6
    for bad in (4, -1, 1.5, True, mask.t(), mask.int()):
        with pytest.raises(ValueError):
            keep_to_given(idx, bad, (3, 4))


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from llamagen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_new_entry_points_are_declared_exported_and_bound(lib):
    from llamagen_amd import _lib as L
    txt = open(os.path.join(ROOT, "include", "lgen.h")).read()
    assert re.search(r"#define LGEN_ABI_VERSION 10\b", txt) and lib.lgen_abi_version() == L.ABI_VERSION == 10   # additive
    for name in NEW:
        assert re.search(rf"^int\s+{name}\s*\(", txt, flags=re.M), name
        assert hasattr(lib, name) and name in L.SIGNATURES
    # each is its log-probability twin plus one pointer (`given`) in front of the stream
    for new, twin in zip(NEW, ("lgen_sample_logprob", "lgen_sample_rows_params_logprob")):
        assert L.SIGNATURES[new] == L.SIGNATURES[twin][:-1] + [L._P, L._P], new
        args = re.search(rf"^int\s+{new}\s*\(([^;]*?)\);", txt, flags=re.M | re.S).group(1)
        assert re.search(r"const int\*\s+given,\s*void\*\s+stream\s*$", args), new


def test_null_given_is_a_bad_argument_before_launch(lib):
    """Decided before any launch: these calls run without a GPU (the pointers are dummies and are never followed)."""
    from llamagen_amd import _lib as L
    p = 8
    assert lib.lgen_sample_given(p, p, 0, p, p, p, 1, 64, 4, 0, 1.0, -1, 1.0, 0, 1.0, 0, L.F32, p, 0, 0) == L.ERR_BAD_ARG
    assert lib.lgen_sample_given(p, p, 0, p, p, p, 1, 64, 4, 0, 1.0, -1, 1.0, 0, 1.0, 0, L.F32, 0, 0, 0) == L.ERR_BAD_ARG
    assert lib.lgen_sample_rows_params_given(p, p, p, p, p, p, 4, 1, 64, 4, 0, p, L.F32, p, 0, 0) == L.ERR_BAD_ARG
    assert lib.lgen_sample_rows_params_given(p, p, p, p, p, p, 4, 1, 64, 4, 0, p, L.F32, 0, p, 0) == L.ERR_BAD_ARG   # no log-probability buffer
    assert lib.lgen_sample_rows_params_given(p, p, p, p, p, p, 4, 1, 64, 4, 0, 0, L.F32, p, p, 0) == L.ERR_BAD_ARG   # no records
    assert lib.lgen_sample_given(p, p, 0, p, p, p, 1, 60, 4, 0, 1.0, -1, 1.0, 0, 1.0, 0, L.F32, 0, p, 0) == L.ERR_BAD_ARG  # V % 8


# ---- batcher host logic --------------------------------------------------------------------------------------------------------------
def _watching_batcher(**kw):
    from tests.serve_standin import _Batcher

    class Watch(_Batcher):
        """Before every stand-in step: the `given` row of each occupied slot, under the request that sits there."""
        def __init__(self, **kw2):
            self.given_seen = {}
            super().__init__(**kw2)

        def _step(self):
            for b in range(self.B):
                if int(self.row_step[b]) < self.N:
                    self.given_seen.setdefault(self._slot_req[b], []).append((b, self.B, self.given[b].tolist()))
            super()._step()
    return Watch(**kw)


@pytest.mark.parametrize("cfg", [True, False])
def test_given_rows_follow_their_request_through_grow_and_shrink(cfg):
    N = 6
    cb = _watching_batcher(slots=8, N=N, cfg=cfg, buckets=(2, 4), shrink_after=2)
    assert tuple(cb.given.shape) == (8, N) and cb.given.dtype == torch.int32 and (cb.given == -1).all()
    want, out = {}, {}

    def submit(label, given=None):
        rid = cb.submit(label, given=given)
        want[rid] = [-1] * N if given is None else [int(x) for x in given]
        return rid
    first = submit(5, torch.tensor([3, 1, -1, -1, 7, -1]))
    cb._load(0, *cb._queue.popleft())
    for _ in range(2):                       # two steps alone in the 2-slot bucket
        cb._step(); cb.steps_run += 1; cb._account(out)
    for i, l in enumerate((11, 12, 13, 14, 15, 16)):     # a burst: 7 live -> the 8-slot bucket (the first request moves mid-sequence)
        submit(l, None if i % 2 else torch.tensor([i, -1, 20 + i, -1, -1, 31]))
    out.update(cb.run(use_graph=False))
    for i, l in enumerate((17, 18, 19)):                 # 3 live -> 4 slots after shrink_after steps
        submit(l, torch.full((N,), i, dtype=torch.int16) if i != 1 else None)
    out.update(cb.run(use_graph=False))
    submit(20)                                           # a request without given tokens in a slot that held some
    out.update(cb.run(use_graph=False))
    assert sorted(out) == sorted(want) and cb.switches >= 3 and not cb._req_given
    for rid, rows in cb.given_seen.items():
        assert len(rows) == N and all(g == want[rid] for _, _, g in rows), (rid, rows)
    assert len({nb for _, nb, _ in cb.given_seen[first]}) > 1                  # it ran in more than one bucket
    # a shrink that RELOCATES: two requests in slots 5 and 6 of the 8-slot bucket continue in slots 0 and 1 of the 2-slot one
    cb = _watching_batcher(slots=8, N=7, cfg=cfg, buckets=(2,), shrink_after=3)
    cb._switch(cb._bucket(8))
    ga = torch.tensor([1, 2, 3, -1, -1, -1, 4])
    a, b = cb.submit(41, given=ga), cb.submit(42)
    cb._load(5, *cb._queue.popleft())
    cb._load(6, *cb._queue.popleft())
    cb.given[0].fill_(17)                                                       # stale contents where request a will land
    cb.run(use_graph=False)
    assert [x[:2] for x in cb.given_seen[a]] == [(5, 8)] * 2 + [(0, 2)] * 5 and [x[0] for x in cb.given_seen[b]] == [6] * 2 + [1] * 5
    assert all(g == ga.tolist() for _, _, g in cb.given_seen[a]) and all(g == [-1] * 7 for _, _, g in cb.given_seen[b])
    with pytest.raises(ValueError):
        cb.submit(1, given=torch.tensor([0, 0, 0, 0, 0, 32]))     # the stand-in's vocabulary is 32
    with pytest.raises(ValueError):
        cb.submit(1, given=torch.tensor([0, 0, 0]))


def test_best_of_candidates_share_the_given_row():
    from llamagen_amd.serve import SamplingParams
    N = 4
    cb = _watching_batcher(slots=4, N=N, cfg=True, greedy=False)
    g = torch.tensor([9, -1, -1, 2])
    rid = cb.submit(7, sampling=SamplingParams(cfg_scale=2.0, seed=3, best_of=3), given=g)
    plain = cb.submit(8)
    out = cb.run(use_graph=False)
    assert sorted(out) == [rid, plain]
    cands = [c for c in cb.given_seen if c not in (rid, plain)]
    assert len(cands) == 3 and all(all(row == g.tolist() for _, _, row in cb.given_seen[c]) for c in cands)
    assert all(row == [-1] * N for _, _, row in cb.given_seen[plain])


# ---- margins of the GPU tests' token-exact claims ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", list(G.PATTERNS))
def test_identity_patterns_have_margin(pattern):
    """tests/test_gpu_given.py::test_identity_fast_path: the free steps of every pattern, in the run the pattern's tokens come from."""
    run = G.oracle_run(G.IDENTITY_CASE, "identity")
    free = ~G.PATTERNS[pattern]
    worst = float(run["margins"][:, free].min()) if bool(free.any()) else float("inf")
    print(f"{pattern}: smallest gap over {int(free.sum()) * run['seq'].shape[0]} free steps = {worst:.3e}")
    assert worst > G.MARGIN, (pattern, worst)
    # the run itself (every step free) is held to the oracle token for token before its tokens are given back
    assert float(run["margins"].min()) > G.MARGIN


@pytest.mark.parametrize("name", G.ORACLE_CASES)
def test_oracle_cases_have_margin(name):
    """tests/test_gpu_given.py::test_given_matches_oracle (random given tokens, both forms): every free step is decided by more
    than MARGIN, the given tokens are really not the run's own, the common prefix is the one the fast path takes, and the
    reference log-probabilities exist (unambiguous nucleus boundary)."""
    from llamagen_amd.given import given_prefix_length
    run = G.oracle_run(name, "oracle")
    given, seq = run["given"], run["seq"]
    assert given_prefix_length(given) >= G.ORACLE_PREFIX and bool((given[:, G.ORACLE_PREFIX:] < 0).any())
    assert torch.equal(seq[given >= 0], given[given >= 0])
    free_run, _ = G.oracle_given(G.oracle_model(run["case"]), run["cond"], None, run["noise"], emb_masks=run["masks"], **run["skw"])
    assert not torch.equal(free_run[given >= 0], given[given >= 0])
    worst = float(run["margins"][given < 0].min())
    print(f"{name}: smallest gap over {int((given < 0).sum())} free steps = {worst:.3e}")
    assert worst > G.MARGIN, (name, worst)
    ref, mag = G.ref_logprobs(run["trace"], seq, given, **run["skw"])
    assert torch.isfinite(ref).all() and mag < 1e3
