"""Image completion on the GPU: the sampler's given-token path (lgen_sample_given, lgen_sample_rows_params_given) and what is built
on it -- generate(given=...) in its stepwise form and through the prefix fast path, the batcher's submit(given=...), complete().

What is held exact and why:
  * kernel: a free entry (-1) is its log-probability twin bit for bit in every output; a given entry writes the given token, and
    its log-probability is within KERNEL_TOL (4.2e-5, the bound of tests/test_gpu_logprobs.py: same logits on both sides, expf /
    logf rounding and summation order over <= 16384 terms) of a float64 log-softmax of the whole scaled row;
  * identity (given = the run's own tokens): bit-equal on the stepwise form in every storage type and with the FP8 KV cache --
    the fed-back tokens are the same, so every launch sees the same bits;
  * prefix fast path and the oracle: token-equal in fp32 only for the seeds whose margins tests/test_given_host.py asserts on the
    CPU (tests/given_cases.py explains the 1e-3);
  * log-probabilities end to end: 2 * 2e-5 * max(1, max |logit / temperature|) + KERNEL_TOL (tests/test_gpu_logprobs.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llamagen_oracle as O  # noqa: E402
from tests import given_cases as G  # noqa: E402
from tests.cases import GPT_CASES  # noqa: E402
from tests.util import build_gpt_holder, build_vq_holder  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
KERNEL_TOL = 8 * 5.21e-6          # tests/test_gpu_logprobs.py: 8 x the largest kernel-level deviation measured on MI355X = 4.2e-5
SENT = -777.0
N = G.N


def _L():
    from llamagen_amd import _lib
    return _lib


def _code(dt):
    L = _L()
    return {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}[dt]


def _full_logprob(row_logits, uncond, cfg, mix, temp, tok):
    """float64 log-softmax of ONE scaled row at tok: the fp32 CFG mix and division of the oracle, then float64."""
    l = row_logits.float()
    if mix:
        l = O.cfg_mix(torch.stack([l, uncond.float()]), cfg, True)[0]
    l = l / max(temp, 1e-5)
    return float(torch.log_softmax(l.double(), dim=-1)[tok])


def _close(got, want, what):
    err = abs(float(got) - want)
    print(f"{what}: |got - float64 ref| = {err:.3e} (ref {want:.4f})")
    assert err <= KERNEL_TOL, (what, float(got), want, err)


# ---- kernel, scalar form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("V", [1024, 16384])
@pytest.mark.parametrize("cfg,interval,step", [(4.0, -1, 2), (3.0, 2, 4), (3.0, 5, 4), (1.0, -1, 3)],
                         ids=["cfg", "interval_passed", "interval_running", "nocfg"])
def test_sample_given_scalar_form(dt, V, cfg, interval, step):
    L, dt = _L(), DTYPES[dt]
    B, S, temp, topk, topp = 3, 16, 0.9, 100, 0.9
    use_cfg = cfg > 1.0
    B2 = 2 * B if use_cfg else B
    mix = use_cfg and not (step > 0 and interval > -1 and (step - 1) > interval)
    g = torch.Generator().manual_seed(1000 + V + step)
    logits = (torch.randn(B2, V, generator=g) * 2.0).to(dt)
    noise = torch.empty(B, V).exponential_(1, generator=g)
    # row 0 free; row 1 takes the LAST vocabulary entry; row 2 the least likely one (far outside top-k 100 / top-p 0.9)
    tok2 = int(torch.argmin(O.cfg_mix(logits.float(), cfg, mix)[2] if use_cfg else logits[2].float()))
    given = torch.full((B, S), 7, dtype=torch.int32)      # every other column holds a valid token: only (b, step) may be read
    given[:, step] = torch.tensor([-1, V - 1, tok2], dtype=torch.int32)
    lg_d, gv_d = logits.to(DEV), given.to(DEV)
    state = torch.tensor([10 + step, step], dtype=torch.int32, device=DEV)

    def launch(fn, nz, with_lp=True, with_given=True):
        nz_all = torch.ones(step + 1, B, V)
        nz_all[step] = nz
        nz_d = nz_all.to(DEV)
        cur = torch.full((B2,), -5, dtype=torch.int32, device=DEV)
        seq = torch.full((B, S), -1, dtype=torch.int32, device=DEV)
        lp = torch.full((B, S), SENT, dtype=torch.float32, device=DEV)
        args = (L.ptr(lg_d), L.ptr(nz_d), B * V, L.ptr(cur), L.ptr(seq), L.ptr(state), B, V, S, 1 if use_cfg else 0, cfg, interval,
                temp, topk, topp, 0, _code(dt), L.ptr(lp) if with_lp else 0)
        if with_given:
            args += (L.ptr(gv_d),)
        L.check(fn(*args, L.stream()), "sample")
        torch.cuda.synchronize()
        return seq.cpu(), cur.cpu(), lp.cpu()
    lib = L.lib()
    seq_t, cur_t, lp_t = launch(lib.lgen_sample_logprob, noise, with_given=False)
    seq_g, cur_g, lp_g = launch(lib.lgen_sample_given, noise)
    assert state.cpu().tolist() == [10 + step, step]                                 # read only
    # free row: the twin, bit for bit
    assert torch.equal(seq_g[0], seq_t[0]) and cur_g[0] == cur_t[0] and lp_g[0, step] == lp_t[0, step] and lp_g[0, step] != SENT
    if use_cfg:
        assert cur_g[B] == cur_t[B]
    # given rows: the token, fed to both halves; nothing else written
    for b, tok in ((1, V - 1), (2, tok2)):
        assert int(seq_g[b, step]) == tok and int(cur_g[b]) == tok and (not use_cfg or int(cur_g[B + b]) == tok)
        want = _full_logprob(logits[b], logits[B + b] if use_cfg else None, cfg, mix, temp, tok)
        _close(lp_g[b, step], want, f"scalar {dt} V={V} cfg={cfg} step={step} row {b}")
    keep = torch.ones(B, S, dtype=torch.bool)
    keep[:, step] = False
    assert (seq_g[keep] == -1).all() and (lp_g[keep] == SENT).all()
    # the noise of a given row is not read: NaN there changes nothing anywhere
    poisoned = noise.clone()
    poisoned[1:] = float("nan")
    seq_n, cur_n, lp_n = launch(lib.lgen_sample_given, poisoned)
    assert torch.equal(seq_n, seq_g) and torch.equal(cur_n, cur_g) and torch.equal(lp_n, lp_g)
    # without a log-probability buffer: the same tokens
    seq_0, cur_0, lp_0 = launch(lib.lgen_sample_given, noise, with_lp=False)
    assert torch.equal(seq_0, seq_g) and torch.equal(cur_0, cur_g) and (lp_0 == SENT).all()


# ---- kernel, per-slot form -----------------------------------------------------------------------------------------------------------
MAXS = 16


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("V", [1024, 16384])
def test_sample_given_rows_form(dt, V):
    from llamagen_amd.serve import SamplingParams as SP, pack_sampling
    L, dt = _L(), DTYPES[dt]
    B = 3
    recs_sp = [SP(cfg_scale=3.0, cfg_interval=2, temperature=1.0, top_k=50, top_p=1.0),        # slot 0 at step 4: interval passed
               SP(cfg_scale=4.0, cfg_interval=-1, temperature=0.9, top_k=100, top_p=0.9),      # slot 1: guided
               SP(cfg_scale=1.0, cfg_interval=-1, temperature=0.7, top_k=0, top_p=0.9)]        # slot 2: unguided in a guided batch
    g = torch.Generator().manual_seed(77 + V)
    logits = (torch.randn(2 * B, V, generator=g) * 2.0).to(dt)
    noise = torch.empty(B, MAXS, V).exponential_(1, generator=g)
    recs = torch.from_numpy(np.stack([pack_sampling(sp) for sp in recs_sp])).to(DEV)
    lg_d = logits.to(DEV)
    lib = L.lib()

    def launch(fn, steps, given, nz):
        st = dict(cur=torch.full((2 * B,), -7, dtype=torch.int32, device=DEV), seq=torch.full((B, MAXS), -1, dtype=torch.int32, device=DEV),
                  row_step=torch.tensor(steps, dtype=torch.int32, device=DEV),
                  row_pos=torch.tensor([20 + s for s in steps] * 2, dtype=torch.int32, device=DEV),
                  lp=torch.full((B, MAXS), SENT, dtype=torch.float32, device=DEV))
        nz_d = nz.to(DEV)
        args = (L.ptr(lg_d), L.ptr(nz_d), L.ptr(st["cur"]), L.ptr(st["seq"]), L.ptr(st["row_step"]), L.ptr(st["row_pos"]), MAXS, B, V,
                MAXS, 1, L.ptr(recs), _code(dt), L.ptr(st["lp"]))
        if given is not None:
            gv_d = given.to(DEV)
            args += (L.ptr(gv_d),)
        L.check(fn(*args, L.stream()), "sample_rows")
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in st.items()}
    # launch 1: slot 0 free at step 4, slot 1 given at step 3, slot 2 given at its LAST step
    steps = [4, 3, MAXS - 1]
    toks = [-1, V - 1, 5]
    given = torch.full((B, MAXS), 9, dtype=torch.int32)
    for b in range(B):
        given[b, steps[b]] = toks[b]
    twin = launch(lib.lgen_sample_rows_params_logprob, steps, None, noise)
    got = launch(lib.lgen_sample_rows_params_given, steps, given, noise)
    assert torch.equal(got["row_step"], twin["row_step"]) and got["row_step"].tolist() == [s + 1 for s in steps]     # counters advance alike
    assert torch.equal(got["row_pos"], twin["row_pos"]) and got["row_pos"].tolist() == [21 + s for s in steps] * 2
    assert torch.equal(got["seq"][0], twin["seq"][0]) and torch.equal(got["lp"][0], twin["lp"][0]) and got["lp"][0, 4] != SENT
    assert got["cur"][0] == twin["cur"][0] and got["cur"][B] == twin["cur"][B]
    for b in (1, 2):
        sp, s, tok = recs_sp[b], steps[b], toks[b]
        assert int(got["seq"][b, s]) == tok and int(got["cur"][b]) == tok and int(got["cur"][B + b]) == tok
        want = _full_logprob(logits[b], logits[B + b], sp.cfg_scale, sp.cfg_scale > 1.0, sp.temperature, tok)
        _close(got["lp"][b, s], want, f"rows {dt} V={V} slot {b}")
        keep = torch.ones(MAXS, dtype=torch.bool)
        keep[s] = False
        assert (got["seq"][b][keep] == -1).all() and (got["lp"][b][keep] == SENT).all()
    poisoned = noise.clone()
    poisoned[1:] = float("nan")
    again = launch(lib.lgen_sample_rows_params_given, steps, given, poisoned)
    for k in got:
        assert torch.equal(again[k], got[k]), k
    # launch 2: slots 0 and 2 finished (their given entries must not wake them), slot 1 free
    steps2 = [MAXS, 6, MAXS + 3]
    given2 = torch.full((B, MAXS), 9, dtype=torch.int32)
    given2[1, 6] = -1
    twin2 = launch(lib.lgen_sample_rows_params_logprob, steps2, None, noise)
    got2 = launch(lib.lgen_sample_rows_params_given, steps2, given2, noise)
    for k in got2:
        assert torch.equal(got2[k], twin2[k]), k
    assert (got2["seq"][[0, 2]] == -1).all() and (got2["lp"][[0, 2]] == SENT).all() and got2["cur"][[0, 2, 3, 5]].tolist() == [-7] * 4
    assert got2["row_step"].tolist() == [MAXS, 7, MAXS + 3] and int(got2["seq"][1, 6]) >= 0


# ---- models ----------------------------------------------------------------------------------------------------------------------
_models = {}


def _model(name, dt=torch.float32):
    """The case's synthetic-weight model on the GPU (one per case and storage type: its engine and graphs are reused)."""
    if (name, dt) not in _models:
        m, _ = build_gpt_holder(GPT_CASES[name])
        _models[(name, dt)] = m.to(device=DEV, dtype=dt).eval()
    return _models[(name, dt)]


def _gen(m, run, **kw):
    from llamagen_amd import generate
    masks = run["masks"]
    return generate(m, run["cond"].to(DEV), N, emb_masks=None if masks is None else masks.to(DEV), _noise_seq=run["noise"],
                    **run["skw"], **kw)


def _own(ids, pattern):
    return torch.where(G.PATTERNS[pattern][None, :], ids.cpu(), torch.full_like(ids.cpu(), -1))


# ---- identity: given = the run's own tokens ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("leg", ["fp32", "bf16", "fp16", "bf16_kv8"])
def test_identity_stepwise_is_bit_equal(leg):
    """A run given its own tokens is the same run: the whole sequence and the log-probabilities of the free positions, bit for
    bit, in every storage type and with the FP8 KV cache (whose whole-sequence passes are refused: the default form there IS the
    stepwise one).  N = 16 > 3: the captured graph is replayed."""
    run = G.oracle_run(G.IDENTITY_CASE, "identity")
    m = _model(G.IDENTITY_CASE, DTYPES[leg.split("_")[0]])
    if leg.endswith("kv8"):
        m.set_kv_cache("fp8_e4m3")
    try:
        base, base_lp = _gen(m, run, return_logprobs=True)
        assert torch.equal(_gen(m, run), base)
        if leg == "fp32":
            np.testing.assert_array_equal(base.cpu().numpy(), run["seq"].numpy())
        for pattern, pat in G.PATTERNS.items():
            given = _own(base, pattern)
            ids, lp = _gen(m, run, given=given, return_logprobs=True)           # log-probabilities: the stepwise form
            assert torch.equal(ids, base), pattern
            free = (~pat).to(DEV)
            assert torch.equal(lp[:, free], base_lp[:, free]), pattern
            assert torch.isfinite(lp).all()
            forced = _gen(m, run, given=given.to(DEV), _given_stepwise=not leg.endswith("kv8"))
            assert torch.equal(forced, base), pattern
        if leg.endswith("kv8"):
            assert m._engine.kv_dtype == "fp8_e4m3"
    finally:
        if leg.endswith("kv8"):
            m.set_kv_cache(None)


@pytest.mark.parametrize("pattern", list(G.PATTERNS))
def test_identity_fast_path_is_token_equal(pattern):
    """fp32, the seed whose margins tests/test_given_host.py::test_identity_patterns_have_margin asserts: the prefix goes through
    every layer in one pass (checked: the pass ran, with the pattern's P) and the tokens are the run's."""
    run = G.oracle_run(G.IDENTITY_CASE, "identity")
    m = _model(G.IDENTITY_CASE)
    base = _gen(m, run)
    np.testing.assert_array_equal(base.cpu().numpy(), run["seq"].numpy())
    e, seen = m._engine, []
    orig = e._prefill_given
    e._prefill_given = lambda model, cond, B, P: (seen.append(P), orig(model, cond, B, P))[1]
    try:
        ids = _gen(m, run, given=_own(base, pattern))
    finally:
        del e._prefill_given
    assert m._engine is e and seen == [G.PATTERN_P[pattern]]
    assert torch.equal(ids, base)


# ---- random given tokens against the oracle loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["stepwise", "fast"])
@pytest.mark.parametrize("name", G.ORACLE_CASES)
def test_given_matches_oracle(name, form):
    run = G.oracle_run(name, "oracle")
    m = _model(name)
    given = run["given"]
    ids = _gen(m, run, given=given, _given_stepwise=form == "stepwise")
    assert ids.dtype == torch.int32 and tuple(ids.shape) == tuple(given.shape)
    np.testing.assert_array_equal(ids.cpu().numpy(), run["seq"].numpy())
    if form == "fast":
        return
    ids2, lp = _gen(m, run, given=given, return_logprobs=True)
    assert torch.equal(ids2, ids)
    ref, mag = G.ref_logprobs(run["trace"], run["seq"], given, **run["skw"])
    tol = 2 * 2e-5 * max(1.0, mag) + KERNEL_TOL
    err = (lp.double().cpu() - ref).abs()
    print(f"{name}: log-probabilities max |got - ref| = {float(err.max()):.3e} (given {float(err[given >= 0].max()):.3e}), tol {tol:.3e}")
    assert float(err.max()) <= tol, (name, float(err.max()), tol)


# ---- fast path vs stepwise: the caches -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt", [("tiny_cfg4", "fp32"), ("t2i_cfg", "fp32"), ("tiny_cfg4", "bf16")])
def test_fast_path_fills_the_caches_like_the_steps(name, dt):
    """K/V slots 0 .. T+P-1 of every layer after the one-pass prefix against the same slots after P decode steps: 2e-5 relative in
    fp32; in bf16 the bar of tests/test_gpu_gpt.py::test_forward_whole_sequence_matches_stepwise (4 ulp of the largest value at
    most, 0.25 ulp on average)."""
    from llamagen_amd.given import given_prefix_length
    run = G.oracle_run(name, "oracle")
    m = _model(name, DTYPES[dt])
    given = run["given"]
    P, T = given_prefix_length(given), run["case"]["kwargs"]["cls_token_num"]
    assert P >= G.ORACLE_PREFIX
    caches = []
    for stepwise in (True, False):
        _gen(m, run, given=given, _given_stepwise=stepwise)
        e = m._engine
        caches.append([c[:, :, :, :T + P, :e.hd].float().cpu() for c in (e.k_cache, e.v_cache)])
    for a, b, what in zip(caches[0], caches[1], "kv"):
        err, top = (a - b).abs(), float(a.abs().max())
        print(f"{name} {dt} {what}: max |stepwise - fast| = {float(err.max()):.3e}, mean {float(err.mean()):.3e}, largest value {top:.3f}")
        if dt == "fp32":
            assert float(err.max()) <= 2e-5 * max(1.0, top), (what, float(err.max()))
        else:
            ulp = top * 2.0 ** -8
            assert float(err.max()) <= 4 * ulp and float(err.mean()) <= 0.25 * ulp, (what, float(err.max()), float(err.mean()), ulp)


# ---- batcher -----------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=True)


def _pattern_given(pattern, V, g):
    toks = torch.randint(0, V, (N,), generator=g, dtype=torch.int32)
    return torch.where(G.PATTERNS[pattern], toks, torch.full_like(toks, -1))


def test_batcher_mixed_traffic_through_bucket_switches():
    """Ten requests on buckets (4, 8): three start in the 4-slot bucket, a burst moves them into the 8-slot one mid-sequence, two
    late ones are relocated from slots 6 and 7 by the shrink.  With and without given tokens, different patterns, per-request
    sampling values, one best_of=2.  Every request equals generate(given=...) of a batch of one in its stepwise form (rows are
    independent through every kernel, as in tests/test_gpu_serve.py::test_staggered_arrivals_and_generate_agreement)."""
    from llamagen_amd import generate
    from llamagen_amd.serve import ContinuousBatcher, SamplingParams as SP, pick_best
    name = "tiny_cfg4"
    V = GPT_CASES[name]["kwargs"]["vocab_size"]
    m, m2 = _model(name), build_gpt_holder(GPT_CASES[name])[0].to(device=DEV, dtype=torch.float32).eval()
    g = torch.Generator().manual_seed(47)
    scattered = torch.where(torch.rand(N, generator=g) < 0.3, torch.randint(0, V, (N,), generator=g, dtype=torch.int32),
                            torch.full((N,), -1, dtype=torch.int32))
    reqs = [  # (label, sampling or None, given or None)
        (3, None, None),
        (7, None, _pattern_given("prefix5", V, g)),
        (1, SP(cfg_scale=1.0, temperature=0.8, top_k=0), _pattern_given("checker", V, g)),          # unguided in a guided batcher
        (9, SP(cfg_scale=3.0, cfg_interval=5, top_k=50), _pattern_given("left_half", V, g)),
        (0, None, _pattern_given("prefix16", V, g)),                                                # nothing left to sample
        (4, SP(cfg_scale=4.0, top_k=100, sample_logits=False), None),                               # greedy
        (6, SP(cfg_scale=3.0, temperature=0.9, top_k=50, seed=11, best_of=2), _pattern_given("left_half", V, g)),
        (2, None, scattered),
        (8, None, _pattern_given("prefix15", V, g)),
        (5, SP(cfg_scale=2.0, top_k=200, top_p=0.8), _pattern_given("prefix1", V, g)),
    ]
    noises = [torch.empty(N, V).exponential_(1, generator=g) for _ in reqs]
    cb = ContinuousBatcher(m, 8, N, slot_buckets=(4,), shrink_after=2, **DEFAULTS)
    assert cb.bucket_sizes == [4, 8] and cb.B == 4

    def sub(i):
        label, sp, given = reqs[i]
        nz = None if (sp is not None and (sp.best_of > 1 or not sp.sample_logits)) else noises[i]
        return cb.submit(label, nz, sampling=sp, given=given)
    ids, out = [sub(i) for i in range(3)], {}
    for b in range(3):
        cb._load(b, *cb._queue.popleft())
    for _ in range(3):                                  # three requests in the 4-slot bucket (eager steps)
        cb._step()
        cb.steps_run += 1
        cb._account(out)
    ids += [sub(i) for i in range(3, 8)]                # 3 running + 6 queued (best_of: two candidates): the 8-slot bucket
    out.update(cb.run())
    assert cb.switches >= 1
    ids += [sub(i) for i in range(8, 10)]
    if cb.B != 8:                                       # (the tail of the first run shrank the batch)
        cb._switch(cb._bucket(8))
    cb._load(6, *cb._queue.popleft())                   # HIGH slots of the 8-slot bucket: the shrink relocates them with their given rows
    cb._load(7, *cb._queue.popleft())
    out.update(cb.run())
    torch.cuda.synchronize()
    assert sorted(out) == ids and cb.B == 4 and cb.switches >= 3

    def solo(i, nz, sp, **kw):
        label, _, given = reqs[i]
        d = DEFAULTS if sp is None else dict(cfg_scale=sp.cfg_scale, cfg_interval=sp.cfg_interval, temperature=sp.temperature,
                                             top_k=sp.top_k, top_p=sp.top_p, sample_logits=sp.sample_logits)
        if given is not None:
            kw.update(given=given.view(1, N), _given_stepwise=True)
        return generate(m2, torch.tensor([label], device=DEV), N, _noise_seq=nz.view(N, 1, V), **d, **kw)
    for rid, i in zip(ids, range(len(reqs))):
        sp = reqs[i][1]
        if sp is not None and sp.best_of > 1:
            cands = []
            for j in range(sp.best_of):
                nz = torch.empty(N, V, device=DEV).exponential_(1.0, generator=torch.Generator(device=DEV).manual_seed(sp.seed + j))
                cands.append(solo(i, nz, sp, return_logprobs=True))
            cum = [float(lp.double().sum()) for _, lp in cands]
            assert abs(cum[0] - cum[1]) > 1e-3, cum       # an unambiguous winner
            want = cands[pick_best(cum)][0]
        else:
            want = solo(i, noises[i], sp)
        assert torch.equal(out[rid].cpu(), want[0].cpu()), (rid, i)
        given = reqs[i][2]
        if given is not None:
            assert torch.equal(out[rid].cpu()[given >= 0], given[given >= 0]), i


def test_batcher_text_conditional_first_token_given():
    """t2i: the first token is sampled on the private prefill engine, which honours column 0 of the request's given row."""
    from llamagen_amd import generate
    from llamagen_amd.serve import ContinuousBatcher
    case = GPT_CASES["t2i_cfg"]
    kw, V = case["kwargs"], case["kwargs"]["vocab_size"]
    T, C = kw["cls_token_num"], kw["caption_dim"]
    m, m2 = _model("t2i_cfg"), build_gpt_holder(case)[0].to(device=DEV, dtype=torch.float32).eval()
    g = torch.Generator().manual_seed(53)
    skw = dict(cfg_scale=7.5, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=True)
    caps, masks, givens = [], [], []
    for i in range(3):
        mk = torch.zeros(T, dtype=torch.int64)
        mk[T - int(torch.randint(1, T + 1, (1,), generator=g)):] = 1
        caps.append(torch.randn(T, C, generator=g) * mk[:, None])
        masks.append(mk)
    givens = [_pattern_given("checker", V, g), None, _pattern_given("prefix1", V, g)]      # 0 and 2: given at column 0
    noises = [torch.empty(N, V).exponential_(1, generator=g) for _ in range(3)]
    cb = ContinuousBatcher(m, 2, N, **skw)
    ids = [cb.submit(c, n, k, given=gv) for c, n, k, gv in zip(caps, noises, masks, givens)]
    out = cb.run()
    torch.cuda.synchronize()
    assert sorted(out) == ids
    for rid, c, n, k, gv in zip(ids, caps, noises, masks, givens):
        extra = {} if gv is None else dict(given=gv.view(1, N), _given_stepwise=True)
        want = generate(m2, c.unsqueeze(0).to(DEV), N, emb_masks=k.unsqueeze(0).to(DEV), _noise_seq=n.view(N, 1, V), **skw, **extra)
        assert torch.equal(out[rid].cpu(), want[0].cpu()), rid
        if gv is not None:
            assert int(out[rid][0]) == int(gv[0]) and torch.equal(out[rid].cpu()[gv >= 0], gv[gv >= 0])


# ---- complete() ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", ["rows", "mask"])
def test_complete_keeps_the_encoders_tokens_and_samples_the_rest(keep):
    """A VQ-16 tokenizer with a 1024-entry codebook on 64 x 64 inputs (a 4 x 4 token grid = the tiny GPT's 16 tokens): kept
    positions are the encoder's indices, free ones are generate(given=...)'s with the same noise, the image is decode_code(ids)."""
    from llamagen_amd import complete, generate
    case = GPT_CASES["tiny_cfg4"]
    B, V = case["batch"], case["kwargs"]["vocab_size"]
    vq, _ = build_vq_holder(dict(vq="VQ-16", codebook_size=V, embed_dim=8, wseed=3))
    vq = vq.to(DEV)
    gpt = _model("tiny_cfg4")
    g = torch.Generator().manual_seed(61)
    images = (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    cond = torch.randint(0, 10, (B,), generator=g).to(DEV)
    noise = torch.empty(N, B, V).exponential_(1, generator=g)
    if keep == "rows":
        k, kept = 2, torch.arange(N) < 8
    else:
        k = torch.zeros(4, 4, dtype=torch.bool)
        k[:, 0] = True                                   # outpaint a kept left strip
        k[3, 3] = True
        kept = k.reshape(-1)
    skw = G.sampling_of(case)
    out, ids = complete(gpt, vq, images, cond, k, _noise_seq=noise, **skw)
    _, _, (_, _, indices) = vq.encode(images)
    indices = indices.view(B, N).to(torch.int32)
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (B, N) and tuple(out.shape) == (B, 3, 64, 64) and out.dtype == torch.float32
    assert len(set(indices.view(-1).tolist())) > 1                     # the encoder's indices are not one constant
    assert torch.equal(ids[:, kept.to(DEV)], indices[:, kept.to(DEV)])
    given = torch.where(kept[None, :].to(DEV), indices, torch.full_like(indices, -1))
    assert torch.equal(ids, generate(gpt, cond, N, given=given, _noise_seq=noise, **skw))
    assert torch.equal(out, vq.decode_code(ids, [B, 8, 4, 4]))
