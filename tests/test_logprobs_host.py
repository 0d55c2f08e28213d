"""CPU-only checks of the log-probability feature: the three new C-ABI entry points are exported, bound and refuse bad arguments
before any launch; SamplingParams.best_of validation; the best_of selection rule; the per-slot record keeps its layout."""
import os

import numpy as np
import pytest

NEW = ("lgen_sample_logprob", "lgen_sample_rows_params_logprob", "lgen_logprob_rows")


@pytest.fixture(scope="module")
def lib():
    from llamagen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from llamagen_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lgen.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert len(L.SIGNATURES["lgen_sample_logprob"]) == len(L.SIGNATURES["lgen_sample"]) + 1
    assert len(L.SIGNATURES["lgen_sample_rows_params_logprob"]) == len(L.SIGNATURES["lgen_sample_rows_params"]) + 1
    assert lib.lgen_abi_version() == L.ABI_VERSION == 10          # additive: the version stays


def test_launchers_refuse_bad_arguments_before_any_launch(lib):
    """Dummy non-null pointers: only refused shapes are called, so nothing is ever dereferenced."""
    from llamagen_amd import _lib as L
    p = 8
    assert lib.lgen_sample_logprob(p, p, 0, p, p, p, 1, 64, 16, 0, 1.0, -1, 1.0, 0, 1.0, 0, L.F32, 0, 0) == L.ERR_BAD_ARG
    assert lib.lgen_sample_rows_params_logprob(p, p, p, p, p, p, 4, 1, 64, 4, 0, p, L.F32, 0, 0) == L.ERR_BAD_ARG
    assert lib.lgen_sample_rows_params_logprob(p, p, p, p, p, p, 4, 1, 64, 4, 0, 0, L.F32, p, 0) == L.ERR_BAD_ARG   # no records
    for V in (12, 4, 0, 16392):
        assert lib.lgen_logprob_rows(p, p, p, 5, V, 0, 1.0, 1.0, L.F32, 0) == L.ERR_BAD_ARG, V
    assert lib.lgen_logprob_rows(p, p, p, 0, 64, 0, 1.0, 1.0, L.F32, 0) == L.ERR_BAD_ARG
    assert lib.lgen_logprob_rows(p, p, p, 5, 64, 0, 1.0, 1.0, 7, 0) == L.ERR_BAD_ARG             # unknown storage code
    for args in ((0, p, p), (p, 0, p), (p, p, 0)):
        assert lib.lgen_logprob_rows(*args, 5, 64, 0, 1.0, 1.0, L.F32, 0) == L.ERR_BAD_ARG


def test_best_of_validation():
    from llamagen_amd.serve import SamplingParams, check_best_of
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            SamplingParams(best_of=bad)
    with pytest.raises(ValueError):
        SamplingParams(best_of=2, sample_logits=False)           # greedy candidates are all the same
    sp = SamplingParams(best_of=3, seed=11, logprobs=True)
    assert sp.best_of == 3 and sp.logprobs is True and SamplingParams().best_of == 1 and SamplingParams().logprobs is False
    assert check_best_of(sp, 4) == 3 and check_best_of(sp, 3) == 3
    with pytest.raises(ValueError):
        check_best_of(sp, 2)                                     # more candidates than slots
    with pytest.raises(ValueError):
        check_best_of(sp, 4, has_noise=True)                     # one explicit noise block cannot serve three candidates
    assert check_best_of(SamplingParams(), 1, has_noise=True) == 1


def test_pick_best():
    from llamagen_amd.serve import pick_best
    assert pick_best([-3, -1, -1, -2]) == 1                      # ties go to the lowest index
    assert pick_best([-0.5]) == 0 and pick_best([-2.0, -3.0]) == 0 and pick_best([-9.0, -8.0, -7.5]) == 2


def test_record_layout_is_unchanged_by_the_new_fields():
    from llamagen_amd import _lib as L
    from llamagen_amd.serve import RECORD_WORDS, SamplingParams, pack_sampling
    old = dict(cfg_scale=3.5, cfg_interval=4, temperature=0.7, top_k=50, top_p=0.9, sample_logits=False)
    a = pack_sampling(SamplingParams(**old))
    b = pack_sampling(SamplingParams(logprobs=True, seed=5, **old))
    c = pack_sampling(SamplingParams(best_of=3, seed=5, **dict(old, sample_logits=True)))
    assert a.nbytes == 32 and RECORD_WORDS == 8 and np.array_equal(a, b)
    assert np.array_equal(a[:5], c[:5]) and c[5] == 0 and a[5] == 1 and not c[6:].any()
    want = np.frombuffer(bytes(L.SlotSampling(3.5, 0.7, 0.9, 4, 50, 1)), dtype=np.int32)
    assert np.array_equal(a, want)
