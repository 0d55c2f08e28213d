"""Per-token log-probabilities: the sampler's (lgen_sample_logprob, lgen_sample_rows_params_logprob), the scoring kernel
(lgen_logprob_rows), and what is built on them -- generate(return_logprobs=True), score(), the batcher's RequestOutputs and best_of.

Reference: the oracle's public functions give the final sampling distribution's support (O.cfg_mix, the fp32 division by
max(temperature, 1e-5) of O.sample, O.top_k_top_p_filtering); the log-softmax over that kept set is taken in float64 here.

Kernel-level tolerance.  Both sides get the same logits tensor, so what differs is expf / logf rounding and the summation order
over at most 16384 terms.  Measured on MI355X over every kernel-level case of this file (tests/test_gpu_logprobs.py -s prints the
figure of each case): largest |kernel - float64 reference| = MEASURED_MAX below; the assertion is 8 x that (headroom for other
seeds), and a bound above 1e-4 would be a defect of the kernel, not a tolerance.

End-to-end tolerance.  tests/test_gpu_gpt.py:_close allows fp32 logits 2e-5 * max(1, max|logit|); a log-softmax moves by at most
twice the largest perturbation of its inputs, so: 2 * 2e-5 * max(1, max|logits / temperature|) + the kernel-level bound.

Top-p rows: a reference whose nucleus boundary is a coin toss would measure the boundary, not the log-probability, so every top-p
row used here has the oracle's cumulative probability on both sides of the cut at least 1e-4 away from top_p (asserted on the CPU
before anything is launched; the seeds below were chosen for it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llamagen_oracle as O  # noqa: E402
from llamagen_amd.gpt import ModelArgs, Transformer  # noqa: E402
from llamagen_amd.testing import synth_for_module  # noqa: E402
from tests.cases import GPT_CASES, make_gpt_inputs  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DEV = torch.device("cuda:0")
MEASURED_MAX = 5.21e-6    # largest kernel-level deviation measured on MI355X (see the module docstring)
KERNEL_TOL = 8 * MEASURED_MAX    # 4.2e-5
assert KERNEL_TOL <= 1e-4
SENT = -777.0           # what an untouched log-probability slot holds
TOPP_MARGIN = 1e-4
_seen = {"max": 0.0}


def _L():
    from llamagen_amd import _lib
    return _lib


def _code(dt):
    L = _L()
    return {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}[dt]


def _scaled(mixed, temp):
    return mixed / max(temp, 1e-5)          # fp32, as O.sample divides


def topp_margin(l, top_k, top_p):
    """Smallest distance between top_p and the oracle's cumulative probability just below / just above the nucleus cut, over the
    rows of the scaled logits l (inf when top-p is off or a row keeps everything)."""
    if top_p >= 1.0:
        return float("inf")
    if top_k > 0:
        l = O.top_k_top_p_filtering(l, top_k=top_k, top_p=1.0)
    cp = torch.cumsum(torch.softmax(torch.sort(l, descending=True, stable=True)[0], dim=-1), dim=-1)
    worst = float("inf")
    for row in cp:
        n_le = int((row <= top_p).sum())
        if n_le > 0:
            worst = min(worst, top_p - float(row[n_le - 1]))
        if n_le < row.numel():
            worst = min(worst, float(row[n_le]) - top_p)
    return worst


def ref_logprob(mixed, temp, top_k, top_p, idx):
    """float64 log-softmax over the oracle's kept set, at idx [B]."""
    l = _scaled(mixed.float(), temp)
    assert topp_margin(l, top_k, top_p) >= TOPP_MARGIN, "ambiguous nucleus boundary: choose another seed"
    if top_k > 0 or top_p < 1.0:
        l = O.top_k_top_p_filtering(l, top_k=top_k, top_p=top_p)
    return torch.log_softmax(l.double(), dim=-1).gather(1, idx.view(-1, 1).long()).view(-1)


def _check(got, ref, what, tol=None):
    got, ref = got.detach().double().cpu().view(-1), ref.double().view(-1)
    err = float((got - ref).abs().max())
    if tol is None:
        _seen["max"] = max(_seen["max"], err)
        tol = KERNEL_TOL
    print(f"{what}: max |got - ref| = {err:.3e} (|ref| up to {float(ref.abs().max()):.2f}); running kernel-level max {_seen['max']:.3e}")
    assert err <= tol, (what, err, tol)


def _rand_logits(shape, dt, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g) * scale).to(dt)
    if dt != torch.float32:
        x[:, 7] = x[:, 3]  # exact ties around
    return x


# ---- sampler, scalar entry point ------------------------------------------------------------------------------------------
GRID = [  # the parameter grid of tests/test_gpu_gpt.py::test_sampler_index_exact
    (3, 1024, 4.0, -1, 0, 1.0, 100, 0, 1.0), (32, 16384, 4.0, -1, 5, 1.0, 2000, 0, 1.0), (5, 2048, 1.0, -1, 3, 0.8, 0, 0, 1.0),
    (4, 1024, 3.0, 2, 4, 1.0, 50, 0, 1.0), (4, 1024, 3.0, 2, 3, 1.0, 50, 0, 1.0), (2, 16384, 1.5, -1, 1, 1.0, 1, 0, 1.0),
    (3, 1024, 4.0, -1, 2, 1.0, 100, 1, 1.0), (2, 1024, 2.0, -1, 2, 1.0, 5000, 0, 1.0),
    (8, 16384, 4.0, -1, 2, 1.0, 2000, 0, 0.9), (6, 1024, 2.0, -1, 1, 1.0, 0, 0, 0.8), (4, 2048, 1.0, -1, 0, 0.7, 300, 0, 0.5),
    (4, 16384, 3.0, -1, 3, 1.0, 0, 0, 0.05), (3, 1024, 2.0, -1, 2, 1.0, 0, 1, 0.9),
    # V = 64: most threads own nothing; V = 8200: one thread of the second slice does
    (1, 64, 4.0, -1, 1, 0.9, 16, 0, 1.0), (3, 64, 4.0, -1, 1, 0.9, 16, 0, 1.0),
    (1, 8200, 4.0, -1, 1, 0.9, 2000, 0, 1.0), (3, 8200, 4.0, -1, 1, 0.9, 2000, 0, 1.0),
]


def _sample_both(lg_d, nz_all, stride, B, B2, V, S, state, use_cfg, cfg, interval, temp, topk, topp, greedy, code):
    """lgen_sample and lgen_sample_logprob on identical inputs -> ((seq, cur), (seq, cur, logp))."""
    L = _L()
    outs = []
    for with_lp in (False, True):
        cur = torch.full((B2,), -5, dtype=torch.int32, device=DEV)
        seq = torch.full((B, S), -1, dtype=torch.int32, device=DEV)
        lp = torch.full((B, S), SENT, dtype=torch.float32, device=DEV)
        args = (L.ptr(lg_d), L.ptr(nz_all), stride, L.ptr(cur), L.ptr(seq), L.ptr(state), B, V, S, 1 if use_cfg else 0, cfg,
                interval, temp, topk, topp, greedy, code)
        if with_lp:
            L.check(L.lib().lgen_sample_logprob(*args, L.ptr(lp), L.stream()), "sample_logprob")
        else:
            L.check(L.lib().lgen_sample(*args, L.stream()), "sample")
        outs.append((seq, cur, lp))
    return outs


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("gi", range(len(GRID)))
def test_sampler_logprob_matches_float64_reference(dt, gi):
    B, V, cfg, interval, step, temp, topk, greedy, topp = GRID[gi]
    use_cfg = cfg > 1.0
    B2 = 2 * B if use_cfg else B
    logits = _rand_logits((B2, V), dt, 20 + step)
    noise = torch.empty(B, V).exponential_(1, generator=torch.Generator().manual_seed(99))
    flag = not (step > 0 and interval > -1 and (step - 1) > interval)
    mixed = O.cfg_mix(logits.float(), cfg, flag)
    idx, _ = O.sample(mixed, temperature=temp, top_k=topk, top_p=topp, sample_logits=not greedy, noise=noise)
    ref = ref_logprob(mixed, temp, topk, topp, idx)     # (asserts the top-p precondition before anything runs on the GPU)
    state = torch.tensor([10 + step, step], dtype=torch.int32, device=DEV)
    nz_all = torch.ones(step + 1, B, V, device=DEV)
    nz_all[step] = noise.to(DEV)
    (seq_a, cur_a, lp_a), (seq_b, cur_b, lp_b) = _sample_both(logits.to(DEV), nz_all, B * V, B, B2, V, 16, state, use_cfg, cfg, interval,
                                                              temp, topk, topp, greedy, _code(dt))
    assert torch.equal(seq_a, seq_b) and torch.equal(cur_a, cur_b)           # bit for bit
    assert seq_b[:, step].cpu().tolist() == idx.view(-1).tolist()
    assert cur_b.cpu().tolist() == idx.view(-1).tolist() * (2 if use_cfg else 1)
    assert (lp_a == SENT).all()                                             # the plain entry point never touches a buffer
    keep = torch.ones(B, 16, dtype=torch.bool)
    keep[:, step] = False
    assert (lp_b.cpu()[keep] == SENT).all()
    _check(lp_b[:, step], ref, f"sampler grid {gi} {dt}")


@pytest.mark.parametrize("kind", ["constant", "plateau", "two_values", "huge_range"])
def test_sampler_logprob_degenerate_rows(kind):
    """The rows of tests/test_gpu_gpt.py::test_sampler_degenerate_rows (radix fallback).  huge_range: the outlier holds all the
    mass, so its log-probability is exactly 0."""
    B, V, topk = 4, 16384, 2000
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(B, V, generator=g)
    if kind == "constant":
        logits[:] = 0.25
    elif kind == "plateau":
        logits[:, :12000] = 0.5
    elif kind == "two_values":
        logits[:] = -1.0
        logits[:, ::3] = 2.0
    else:
        logits[:, 5] = 3.0e6
        logits[:, 9] = -3.0e6
    noise = torch.empty(B, V).exponential_(1, generator=g)
    idx, _ = O.sample(logits, temperature=1.0, top_k=topk, top_p=1.0, sample_logits=True, noise=noise)
    ref = ref_logprob(logits, 1.0, topk, 1.0, idx)
    state = torch.tensor([3, 1], dtype=torch.int32, device=DEV)
    nz_all = torch.ones(2, B, V, device=DEV)
    nz_all[1] = noise.to(DEV)
    (seq_a, cur_a, _), (seq_b, cur_b, lp) = _sample_both(logits.to(DEV), nz_all, B * V, B, B, V, 4, state, False, 1.0, -1, 1.0, topk, 1.0,
                                                         0, _L().F32)
    assert torch.equal(seq_a, seq_b) and torch.equal(cur_a, cur_b)
    assert seq_b[:, 1].cpu().tolist() == idx.view(-1).tolist()
    assert (lp.cpu()[:, [0, 2, 3]] == SENT).all()
    if kind == "huge_range":
        assert idx.view(-1).tolist() == [5] * B and (lp[:, 1] == 0.0).all(), lp[:, 1]
    _check(lp[:, 1], ref, f"sampler degenerate {kind}")


# ---- sampler, per-slot records ----------------------------------------------------------------------------------------------
MAXS = 16


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_rows_params_logprob_mixed_slots(dt):
    from llamagen_amd.serve import SamplingParams as SP, pack_sampling
    L, V = _L(), 1024
    slots = [  # (record, row_step)
        (SP(cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0), 0),
        (SP(cfg_scale=1.0, cfg_interval=-1, temperature=0.7, top_k=0, top_p=0.9), 3),            # unguided in a guided batch
        (SP(cfg_scale=3.0, cfg_interval=2, temperature=1.0, top_k=50, top_p=1.0), 4),            # interval passed: no mix
        (SP(cfg_scale=2.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=False), 2),   # greedy
        (SP(cfg_scale=4.0, cfg_interval=-1, temperature=0.7, top_k=50, top_p=0.9), MAXS),        # finished slot: left untouched
        (SP(cfg_scale=7.5, cfg_interval=10, temperature=0.7, top_k=50, top_p=0.5), 15),          # last step of a request
    ]
    B = len(slots)
    g = torch.Generator().manual_seed(41)
    logits = (torch.randn(2 * B, V, generator=g) * 2.0).to(dt)
    if dt != torch.float32:
        logits[:, 7] = logits[:, 3]
    noise = torch.empty(B, V).exponential_(1, generator=g)
    want, ref = {}, {}
    for b, (sp, step) in enumerate(slots):   # the oracle's token and log-probability of every live slot, before any launch
        if step >= MAXS:
            continue
        cond, uncond = logits[b:b + 1].float(), logits[B + b:B + b + 1].float()
        flag = not (step > 0 and sp.cfg_interval > -1 and (step - 1) > sp.cfg_interval)
        mixed = O.cfg_mix(torch.cat([cond, uncond]) if sp.cfg_scale > 1.0 else cond, sp.cfg_scale, flag)
        idx, _ = O.sample(mixed, temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p, sample_logits=sp.sample_logits,
                          noise=noise[b:b + 1])
        want[b], ref[b] = int(idx.view(())), ref_logprob(mixed, sp.temperature, sp.top_k, sp.top_p, idx)
    nz_all = torch.ones(B, MAXS, V)
    for b, (_, step) in enumerate(slots):
        if step < MAXS:
            nz_all[b, step] = noise[b]
    recs = torch.from_numpy(np.stack([pack_sampling(sp) for sp, _ in slots])).to(DEV)
    steps = [t for _, t in slots]
    res = []
    for with_lp in (False, True):
        st = dict(cur=torch.full((2 * B,), -7, dtype=torch.int32, device=DEV), seq=torch.full((B, MAXS), -1, dtype=torch.int32, device=DEV),
                  row_step=torch.tensor(steps, dtype=torch.int32, device=DEV),
                  row_pos=torch.tensor([20 + s for s in steps] * 2, dtype=torch.int32, device=DEV),
                  lp=torch.full((B, MAXS), SENT, dtype=torch.float32, device=DEV))
        lg_d, nz_d = logits.to(DEV), nz_all.to(DEV)
        args = (L.ptr(lg_d), L.ptr(nz_d), L.ptr(st["cur"]), L.ptr(st["seq"]), L.ptr(st["row_step"]), L.ptr(st["row_pos"]), MAXS, B, V,
                MAXS, 1, L.ptr(recs), _code(dt))
        if with_lp:
            L.check(L.lib().lgen_sample_rows_params_logprob(*args, L.ptr(st["lp"]), L.stream()), "sample_rows_params_logprob")
        else:
            L.check(L.lib().lgen_sample_rows_params(*args, L.stream()), "sample_rows_params")
        torch.cuda.synchronize()
        res.append(st)
    a, p = res
    for name in ("cur", "seq", "row_step", "row_pos"):
        assert torch.equal(a[name], p[name]), name
    lp, seq = p["lp"].cpu(), p["seq"].cpu()
    for b, (sp, step) in enumerate(slots):
        if step >= MAXS:
            assert (lp[b] == SENT).all() and (seq[b] == -1).all(), b
            continue
        assert int(seq[b, step]) == want[b], (b, sp)
        assert (lp[b, :step] == SENT).all() and (lp[b, step + 1:] == SENT).all(), b
        _check(lp[b, step:step + 1], ref[b], f"rows_params slot {b} {dt}")


# ---- scoring kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("V", [64, 8200, 16384])
@pytest.mark.parametrize("paired", [False, True])
def test_logprob_rows_matches_float64_reference(dt, V, paired):
    """R = 5 rows; targets 0, V - 1 and -1 (its row is not read, its output is 0 and the outputs around it are right), one row with
    a single huge outlier scored on it (exactly 0) and off it (about minus the outlier: there fp32 spacing, 2^-23 relative, is
    the bound).  The outlier is 3e6; fp16 storage cannot hold that, so there it is 6e4 -- still more than 104 above everything
    else, which is all the property needs."""
    L, R = _L(), 5
    big = 6.0e4 if dt == torch.float16 else 3.0e6
    pair_offset = R if paired else 0
    logits = _rand_logits((2 * R, V), dt, 300 + V)
    jo = V // 3
    logits[3, jo] = big
    lg_d = logits.to(DEV)
    g = torch.Generator().manual_seed(V)
    rnd = [int(t) for t in torch.randint(0, V, (2,), generator=g)]
    for cfg in (1.0, 4.0):
        for temp in (1.0, 0.7):
            mix = paired and cfg > 1.0
            mixed = O.cfg_mix(logits.float(), cfg) if mix else logits[:R].float()
            full = torch.log_softmax(_scaled(mixed, temp).double(), dim=-1)
            for targets in ([0, V - 1, -1, jo, rnd[0]], [rnd[1], 0, V - 1, (jo + 1) % V, -1]):
                tg = torch.tensor(targets, dtype=torch.int32, device=DEV)
                out = torch.full((R + 1,), SENT, dtype=torch.float32, device=DEV)
                L.check(L.lib().lgen_logprob_rows(L.ptr(lg_d), L.ptr(tg), L.ptr(out), R, V, pair_offset, cfg, temp, _code(dt), L.stream()),
                        "logprob_rows")
                out = out.cpu()
                assert out[R] == SENT
                what = f"logprob_rows {dt} V={V} pair={pair_offset} cfg={cfg} T={temp}"
                ordinary = [r for r in range(R) if targets[r] >= 0 and r != 3]
                for r in range(R):
                    if targets[r] < 0:
                        assert out[r] == 0.0, (what, r)
                refs = torch.stack([full[r, targets[r]] for r in ordinary])
                _check(out[ordinary], refs, what)
                if targets[3] == jo:
                    assert out[3] == 0.0, (what, out[3])
                else:
                    want = float(full[3, targets[3]])
                    assert np.isfinite(float(out[3])) and want < -0.9 * big / 1.0, (what, out[3], want)
                    assert abs(float(out[3]) - want) <= 2.0 ** -22 * abs(want), (what, float(out[3]), want)


# ---- end to end (fp32 tiny models) -------------------------------------------------------------------------------------------
def _model(kw, seed):
    m = Transformer(ModelArgs(**kw))
    sd = synth_for_module(m, seed=seed, lin_std=0.05)
    m.load_state_dict(sd, strict=False)
    return m.to(device=DEV, dtype=torch.float32).eval(), sd


def _oracle(kw, sd):
    return O.GPTOracle(O.GPTConfig(**kw), sd, torch.float32)


def _trace_logprobs(trace, ids, temp, top_k, top_p):
    """[B, N] float64 reference log-probabilities and the end-to-end tolerance from the oracle's pre-sampling logits."""
    ref = torch.stack([ref_logprob(tr, temp, top_k, top_p, ids[:, i]) for i, tr in enumerate(trace)], dim=1)
    mag = max(float(_scaled(tr, temp).abs().max()) for tr in trace)
    return ref, 2 * 2e-5 * max(1.0, mag) + KERNEL_TOL


TINY = GPT_CASES["tiny_cfg4"]["kwargs"]
T2I = GPT_CASES["t2i_cfg"]["kwargs"]
GEN_CASES = {  # name: (batch, N, labels seed, noise seed, sampling, order of the two calls); noise seed 62: the first from 8 up
    # whose 12 top-p rows all meet TOPP_MARGIN (the tiny model's distributions are flat: entries at the cut weigh about 1e-3)
    "cfg4_topk": (3, 16, 5, 6, dict(cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0), "plain_first"),
    "nocfg_topp": (2, 6, 7, 62, dict(cfg_scale=1.0, cfg_interval=-1, temperature=0.8, top_k=0, top_p=0.9), "logprobs_first"),
}


@pytest.mark.parametrize("name", list(GEN_CASES))
def test_generate_return_logprobs(name):
    """ids are generate()'s and the oracle's; logprobs are those of the oracle's trace.  Both calls run on the same engine (N > 3:
    the captured graph is replayed), in either order: a graph captured without the buffer must not serve a call that wants it."""
    from llamagen_amd import generate
    B, N, lseed, nseed, skw, order = GEN_CASES[name]
    V = TINY["vocab_size"]
    g = torch.Generator().manual_seed(lseed)
    cond = torch.randint(0, TINY["num_classes"], (B,), generator=g)
    noise = torch.empty(N, B, V).exponential_(1, generator=torch.Generator().manual_seed(nseed))
    m, sd = _model(TINY, 1)
    it, trace = iter(noise), []
    ref_ids = O.generate(_oracle(TINY, sd), cond, N, noise_fn=lambda shape: next(it), trace=trace, **skw)
    ref, tol = _trace_logprobs(trace, ref_ids, skw["temperature"], skw["top_k"], skw["top_p"])
    run = lambda **kw: generate(m, cond.to(DEV), N, _noise_seq=noise, **skw, **kw)
    if order == "plain_first":
        plain = run()
        ids, lp = run(return_logprobs=True)
    else:
        ids, lp = run(return_logprobs=True)
        plain = run()
    assert ids.dtype == torch.int32 and lp.dtype == torch.float32 and tuple(lp.shape) == (B, N)
    assert torch.equal(ids, plain)
    np.testing.assert_array_equal(ids.cpu().numpy(), ref_ids.numpy())
    _check(lp, ref, f"generate {name}", tol)


def test_score_class_conditional():
    from llamagen_amd import score
    B, N = 3, 16
    g = torch.Generator().manual_seed(17)
    cond = torch.randint(0, TINY["num_classes"], (B,), generator=g)
    ids = torch.randint(0, TINY["vocab_size"], (B, N), generator=g).to(torch.int32)
    m, sd = _model(TINY, 1)
    trace = []
    O.generate(_oracle(TINY, sd), cond, N, cfg_scale=4.0, sample_logits=False, trace=trace, teacher=ids)
    ref, tol = _trace_logprobs(trace, ids, 0.9, 0, 1.0)
    got = score(m, cond.to(DEV), ids.to(DEV), cfg_scale=4.0, temperature=0.9)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, N)
    _check(got, ref, "score c2i", tol)


def test_score_text_conditional_left_padded():
    from llamagen_amd import score
    case = dict(GPT_CASES["t2i_cfg"], batch=2)
    cond, masks = make_gpt_inputs(case)
    assert int(masks[:, 0].sum()) < masks.shape[0]              # left padding is really there
    N = 8
    ids = torch.randint(0, T2I["vocab_size"], (2, N), generator=torch.Generator().manual_seed(19)).to(torch.int32)
    m, sd = _model(T2I, 1)
    trace = []
    O.generate(_oracle(T2I, sd), cond, N, emb_masks=masks, cfg_scale=4.0, sample_logits=False, trace=trace, teacher=ids)
    ref, tol = _trace_logprobs(trace, ids, 0.9, 0, 1.0)
    got = score(m, cond.to(DEV), ids.to(DEV), emb_masks=masks.to(DEV), cfg_scale=4.0, temperature=0.9)
    _check(got, ref, "score t2i", tol)


DEFAULTS = dict(cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=True)


def _oracle_request(model, cond, nz, N, skw, mask=None):
    """(tokens [N], float64 logprobs [N], tolerance) of one request: the oracle's batch-of-one generate() on its noise."""
    it, trace = iter(nz), []
    kw = {} if mask is None else dict(emb_masks=mask.unsqueeze(0))
    toks = O.generate(model, cond, N, noise_fn=lambda shape: next(it).view(1, -1), trace=trace, **skw, **kw)
    ref, tol = _trace_logprobs(trace, toks, skw["temperature"], skw["top_k"], skw["top_p"])
    return toks[0], ref[0], tol


def test_batcher_request_outputs_through_a_bucket_switch():
    from llamagen_amd.serve import ContinuousBatcher, RequestOutput
    m, sd = _model(TINY, 1)
    N, V, nreq = 16, TINY["vocab_size"], 6
    g = torch.Generator().manual_seed(29)
    labels = torch.randint(0, 10, (nreq,), generator=g).tolist()
    noises = [torch.empty(N, V).exponential_(1, generator=g) for _ in range(nreq)]
    cb = ContinuousBatcher(m, 4, N, slot_buckets=(2,), **DEFAULTS)
    rids = [cb.submit(l, nz) for l, nz in zip(labels, noises)]
    out = cb.run(return_outputs=True)
    torch.cuda.synchronize()
    assert sorted(out) == rids and cb.switches >= 1
    model = _oracle(TINY, sd)
    for rid, l, nz in zip(rids, labels, noises):
        o = out[rid]
        assert isinstance(o, RequestOutput) and o.token_ids.dtype == torch.int32 and o.logprobs.dtype == torch.float32
        toks, ref, tol = _oracle_request(model, torch.tensor([l]), nz, N, DEFAULTS)
        np.testing.assert_array_equal(o.token_ids.cpu().numpy(), toks.numpy(), err_msg=f"request {rid}")
        _check(o.logprobs, ref, f"batcher request {rid}", tol)
        assert o.cumulative_logprob.dim() == 0 and o.cumulative_logprob.is_cuda
        assert float(o.cumulative_logprob) == float(o.logprobs.double().sum())


def test_batcher_text_conditional_first_logprob_comes_from_the_prefill():
    from llamagen_amd.serve import ContinuousBatcher
    m, sd = _model(T2I, 7)
    N, V, T, C = 8, T2I["vocab_size"], T2I["cls_token_num"], T2I["caption_dim"]
    g = torch.Generator().manual_seed(23)
    mk = torch.zeros(T, dtype=torch.int64)
    mk[T - 37:] = 1
    cap = torch.randn(T, C, generator=g) * mk[:, None]
    nz = torch.empty(N, V).exponential_(1, generator=g)
    skw = dict(cfg_scale=7.5, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=True)
    cb = ContinuousBatcher(m, 2, N, **skw)
    rid = cb.submit(cap, nz, mk)
    o = cb.run(return_outputs=True)[rid]
    toks, ref, tol = _oracle_request(_oracle(T2I, sd), cap.unsqueeze(0), nz, N, skw, mask=mk)
    np.testing.assert_array_equal(o.token_ids.cpu().numpy(), toks.numpy())
    _check(o.logprobs[:1], ref[:1], "t2i first token (prefill engine)", tol)
    _check(o.logprobs, ref, "t2i request", tol)


def test_best_of_returns_the_likeliest_candidate():
    from llamagen_amd.serve import ContinuousBatcher, SamplingParams as SP, pick_best
    m, sd = _model(TINY, 1)
    N, V, label, seed, k = 16, TINY["vocab_size"], 6, 11, 3
    base = dict(cfg_scale=3.0, cfg_interval=-1, temperature=0.9, top_k=50, top_p=1.0)
    cb = ContinuousBatcher(m, 4, N, **DEFAULTS)
    rid = cb.submit(label, sampling=SP(seed=seed, best_of=k, **base))
    best = cb.run(return_outputs=True)[rid]
    with pytest.raises(ValueError):
        cb.submit(label, noise=torch.ones(N, V), sampling=SP(best_of=2, **base))
    solo = []
    for j in range(k):
        r = cb.submit(label, sampling=SP(seed=seed + j, **base))
        solo.append(cb.run()[r])
    again = cb.submit(label, sampling=SP(seed=seed, best_of=k, **base))
    plain = cb.run()[again]                                      # run() without outputs: the winner's tokens
    model, cum, toks = _oracle(TINY, sd), [], []
    for j in range(k):
        nz = torch.empty(N, V, device=DEV).exponential_(1.0, generator=torch.Generator(device=DEV).manual_seed(seed + j)).cpu()
        t, ref, tol = _oracle_request(model, torch.tensor([label]), nz, N, dict(base, sample_logits=True))
        toks.append(t)
        cum.append(float(ref.sum()))
    ranked = sorted(cum, reverse=True)
    assert ranked[0] - ranked[1] > 1e-3, cum                     # an unambiguous winner
    j = pick_best(cum)
    np.testing.assert_array_equal(best.token_ids.cpu().numpy(), toks[j].numpy())
    assert torch.equal(best.token_ids, solo[j]) and torch.equal(plain, solo[j])
    assert abs(float(best.cumulative_logprob) - cum[j]) <= N * tol
    assert float(best.cumulative_logprob) == float(best.logprobs.double().sum())
