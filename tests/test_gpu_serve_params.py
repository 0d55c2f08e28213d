"""Per-request sampling parameters and seeds in the continuous batcher (llamagen_amd/serve.py, lgen_sample_rows_params): every
slot of one step batch samples with its own guidance scale / interval, temperature, top-k, top-p and greedy flag.  The property
held here: a request's tokens are those of the oracle's batch-of-one generate() with THAT request's values and noise, whatever its
neighbours ask for -- index-exact at the kernel (three storage types), token for token end to end (fp32 storage)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import llamagen_oracle as O  # noqa: E402
from llamagen_amd.gpt import ModelArgs, Transformer  # noqa: E402
from llamagen_amd.testing import synth_for_module  # noqa: E402

KW = dict(n_layer=2, n_head=4, dim=256, vocab_size=1024, block_size=16, num_classes=10, cls_token_num=1, model_type="c2i")
KW_T2I = dict(n_layer=2, n_head=4, dim=256, vocab_size=1024, block_size=16, cls_token_num=120, caption_dim=64, model_type="t2i")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DEV = torch.device("cuda:0")
MAXS = 16   # max_steps of the kernel-level tests


def _code(dt):
    from llamagen_amd import _lib
    return {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}[dt]


def _model(kw, seed):
    m = Transformer(ModelArgs(**kw))
    sd = synth_for_module(m, seed=seed, lin_std=0.05)
    m.load_state_dict(sd, strict=False)
    return m.to(device=DEV, dtype=torch.float32).eval(), sd


def _records(sps):
    from llamagen_amd.serve import pack_sampling
    return torch.from_numpy(np.stack([pack_sampling(sp) for sp in sps])).to(DEV)


def _kernel_inputs(dt, B, V, steps, seed):
    """Random conditional / unconditional logits in storage type `dt` (exact ties around for the 16-bit types, as
    test_sampler_index_exact prepares them), one Exp(1) block per slot at that slot's step, and the slot counters."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(2 * B, V, generator=g) * 2.0).to(dt)
    if dt != torch.float32:
        logits[:, 7] = logits[:, 3]
    noise = torch.empty(B, V).exponential_(1, generator=g)
    nz_all = torch.ones(B, MAXS, V)
    for b, st in enumerate(steps):
        if st < MAXS:
            nz_all[b, st] = noise[b]
    st = dict(logits=logits.to(DEV), noise=nz_all.to(DEV),
              cur=torch.full((2 * B,), -7, dtype=torch.int32, device=DEV), seq=torch.full((B, MAXS), -1, dtype=torch.int32, device=DEV),
              row_step=torch.tensor(steps, dtype=torch.int32, device=DEV),
              row_pos=torch.tensor([20 + s for s in steps] * 2, dtype=torch.int32, device=DEV))
    return logits, noise, st


def _expected(logits, noise, b, B, sp, step):
    """The oracle's token of slot b: its own rows, its own values (generate.py:79-99 CFG mix under the interval rule, :57-66 sample)."""
    cond, uncond = logits[b:b + 1].float(), logits[B + b:B + b + 1].float()
    flag = not (step > 0 and sp.cfg_interval > -1 and (step - 1) > sp.cfg_interval)
    rows = torch.cat([cond, uncond]) if sp.cfg_scale > 1.0 else cond
    mixed = O.cfg_mix(rows, sp.cfg_scale, flag)
    idx, _ = O.sample(mixed, temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p, sample_logits=sp.sample_logits,
                      noise=noise[b:b + 1])
    return int(idx.view(()))


@pytest.mark.parametrize("dt", DTYPES)
def test_heterogeneous_slots_in_one_launch_are_index_exact(dt):
    from llamagen_amd import _lib as L
    from llamagen_amd.serve import SamplingParams as SP
    V = 1024
    slots = [  # (record, row_step)
        (SP(cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0), 0),
        (SP(cfg_scale=1.0, cfg_interval=-1, temperature=0.7, top_k=0, top_p=0.9), 3),            # unguided in a guided batch
        (SP(cfg_scale=3.0, cfg_interval=2, temperature=1.0, top_k=50, top_p=1.0), 4),            # interval passed: no mix
        (SP(cfg_scale=3.0, cfg_interval=2, temperature=1.0, top_k=50, top_p=1.0), 3),            # interval still active: mix
        (SP(cfg_scale=2.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=False), 2),   # greedy, guided
        (SP(cfg_scale=1.5, cfg_interval=-1, temperature=1.0, top_k=1, top_p=1.0), 1),
        (SP(cfg_scale=0.5, cfg_interval=0, temperature=1.0, top_k=V, top_p=0.5), 5),             # unguided, top_k = V keeps all
        (SP(cfg_scale=4.0, cfg_interval=-1, temperature=0.7, top_k=50, top_p=0.9), MAXS),        # finished slot: left untouched
        (SP(cfg_scale=4.0, cfg_interval=-1, temperature=1e-6, top_k=0, top_p=1.0), 2),
        (SP(cfg_scale=1.0, cfg_interval=-1, temperature=0.7, top_k=0, top_p=0.9, sample_logits=False), 0),     # greedy, unguided
        (SP(cfg_scale=7.5, cfg_interval=10, temperature=0.7, top_k=50, top_p=0.5), 15),          # last step of a request
    ]
    B = len(slots)
    sps, steps = [s for s, _ in slots], [t for _, t in slots]
    logits, noise, st = _kernel_inputs(dt, B, V, steps, seed=41)
    recs = _records(sps)
    L.check(L.lib().lgen_sample_rows_params(L.ptr(st["logits"]), L.ptr(st["noise"]), L.ptr(st["cur"]), L.ptr(st["seq"]),
                                            L.ptr(st["row_step"]), L.ptr(st["row_pos"]), MAXS, B, V, MAXS, 1, L.ptr(recs), _code(dt),
                                            L.stream()), "sample_rows_params")
    torch.cuda.synchronize()
    cur, seq = st["cur"].cpu().tolist(), st["seq"].cpu()
    row_step, row_pos = st["row_step"].cpu().tolist(), st["row_pos"].cpu().tolist()
    for b, (sp, step) in enumerate(slots):
        if step >= MAXS:
            assert (seq[b] == -1).all() and cur[b] == -7 and cur[B + b] == -7, b
            assert row_step[b] == step and row_pos[b] == 20 + step and row_pos[B + b] == 20 + step, b
            continue
        want = _expected(logits, noise, b, B, sp, step)
        print(f"slot {b}: step {step} want {want} got {int(seq[b, step])}")
        assert int(seq[b, step]) == want, (b, sp)
        assert cur[b] == want and cur[B + b] == want, b               # the unconditional row of an unguided slot is fed too
        assert row_step[b] == step + 1 and row_pos[b] == 21 + step and row_pos[B + b] == 21 + step, b
        assert (seq[b, :step] == -1).all() and (seq[b, step + 1:] == -1).all(), b


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("use_cfg,cfg,interval,temp,topk,topp,greedy", [
    (1, 4.0, 2, 0.9, 50, 0.9, 0), (1, 3.0, -1, 1.0, 100, 1.0, 1), (0, 1.0, -1, 0.7, 0, 0.5, 0)])
def test_uniform_records_equal_the_scalar_entry_point(dt, use_cfg, cfg, interval, temp, topk, topp, greedy):
    from llamagen_amd import _lib as L
    from llamagen_amd.serve import SamplingParams as SP
    B, V = 8, 2048
    steps = [0, 1, 3, 4, 5, MAXS, 15, 2]
    _, _, a = _kernel_inputs(dt, B, V, steps, seed=17)
    _, _, p = _kernel_inputs(dt, B, V, steps, seed=17)
    recs = _records([SP(cfg_scale=cfg, cfg_interval=interval, temperature=temp, top_k=topk, top_p=topp, sample_logits=not greedy)] * B)
    lib = L.lib()
    L.check(lib.lgen_sample_rows(L.ptr(a["logits"]), L.ptr(a["noise"]), L.ptr(a["cur"]), L.ptr(a["seq"]), L.ptr(a["row_step"]),
                                 L.ptr(a["row_pos"]), MAXS, B, V, MAXS, use_cfg, cfg, interval, temp, topk, topp, greedy, _code(dt),
                                 L.stream()), "sample_rows")
    L.check(lib.lgen_sample_rows_params(L.ptr(p["logits"]), L.ptr(p["noise"]), L.ptr(p["cur"]), L.ptr(p["seq"]), L.ptr(p["row_step"]),
                                        L.ptr(p["row_pos"]), MAXS, B, V, MAXS, use_cfg, L.ptr(recs), _code(dt), L.stream()),
            "sample_rows_params")
    torch.cuda.synchronize()
    for name in ("cur", "seq", "row_step", "row_pos"):
        assert torch.equal(a[name], p[name]), name
    assert int((a["seq"] >= 0).sum()) == 7 and a["row_step"].cpu().tolist() == [1, 2, 4, 5, 6, MAXS, 16, 3]


def _mixed_requests(nreq, seed, N, V):
    """Labels, noise blocks and one SamplingParams per request: guided at several scales, unguided, greedy, top-p, an interval,
    and one request that brings none (the batcher's defaults)."""
    from llamagen_amd.serve import SamplingParams as SP
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, 10, (nreq,), generator=g).tolist()
    noises = [torch.empty(N, V).exponential_(1, generator=g) for _ in range(nreq)]
    base = [SP(cfg_scale=4.0, cfg_interval=3, temperature=0.9, top_k=50, top_p=1.0),
            SP(cfg_scale=1.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0),                       # unguided
            SP(cfg_scale=3.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=False),  # greedy
            SP(cfg_scale=1.75, cfg_interval=-1, temperature=0.7, top_k=0, top_p=0.9),
            None,                                                                                            # the constructor's values
            SP(cfg_scale=7.5, cfg_interval=0, temperature=1.0, top_k=0, top_p=0.5),
            SP(cfg_scale=1.0, cfg_interval=-1, temperature=0.7, top_k=1, top_p=1.0, sample_logits=False),    # greedy and unguided
            SP(cfg_scale=2.0, cfg_interval=8, temperature=1.0, top_k=1024, top_p=1.0),
            SP(cfg_scale=4.0, cfg_interval=-1, temperature=0.9, top_k=50, top_p=0.9)]
    return labels, noises, [base[i % len(base)] for i in range(nreq)]


DEFAULTS = dict(cfg_scale=4.0, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=True)


def _skw(sp):
    return dict(DEFAULTS) if sp is None else dict(cfg_scale=sp.cfg_scale, cfg_interval=sp.cfg_interval, temperature=sp.temperature,
                                                  top_k=sp.top_k, top_p=sp.top_p, sample_logits=sp.sample_logits)


def _submit(cb, label, nz, sp, mask=None):
    greedy = sp is not None and not sp.sample_logits
    return cb.submit(label, None if greedy else nz, mask, sampling=sp)


def _check_against_oracle(model, out, ids, conds, noises, sps, N, masks=None):
    for i, (rid, c, nz, sp) in enumerate(zip(ids, conds, noises, sps)):
        it = iter(nz)
        kw = _skw(sp)
        if masks is None:
            ref = O.generate(model, torch.tensor([c]), N, noise_fn=lambda shape: next(it).view(1, -1), **kw)
        else:
            ref = O.generate(model, c.unsqueeze(0), N, emb_masks=masks[i].unsqueeze(0), noise_fn=lambda shape: next(it).view(1, -1), **kw)
        np.testing.assert_array_equal(out[rid].cpu().numpy(), ref[0].numpy(), err_msg=f"request {rid} {kw}")


def test_mixed_traffic_end_to_end_matches_the_oracle_per_request():
    """3 slots, 8 requests with their own values, staggered arrivals (one request alone for 5 hand-driven steps, then the rest;
    hipGraph replay from there): each one equals a batch-of-one generate() with its values and noise."""
    from llamagen_amd.serve import ContinuousBatcher
    m, sd = _model(KW, 1)
    N, V, nreq = 16, KW["vocab_size"], 8
    labels, noises, sps = _mixed_requests(nreq, 13, N, V)
    cb = ContinuousBatcher(m, 3, N, **DEFAULTS)
    ids, out = [_submit(cb, labels[0], noises[0], sps[0])], {}
    cb._load(0, *cb._queue.popleft())
    for _ in range(5):
        cb._step()
        cb.steps_run += 1
        cb._account(out)
    ids += [_submit(cb, l, n, s) for l, n, s in zip(labels[1:], noises[1:], sps[1:])]
    out.update(cb.run())
    torch.cuda.synchronize()
    assert sorted(out) == ids
    _check_against_oracle(O.GPTOracle(O.GPTConfig(**KW), sd, torch.float32), out, ids, labels, noises, sps, N)


def test_mixed_traffic_through_slot_count_buckets():
    """The same kind of traffic through captured slot counts 1 / 2 / 6 with a grow and a relocating shrink: the record moves with
    the request (K/V rows, noise block, token row and sampling values), so the tokens stay the oracle's."""
    from llamagen_amd.serve import ContinuousBatcher
    m, sd = _model(KW, 3)
    N, V, nreq = 16, KW["vocab_size"], 9
    labels, noises, sps = _mixed_requests(nreq, 31, N, V)
    cb = ContinuousBatcher(m, 6, N, slot_buckets=(1, 2), shrink_after=2, **DEFAULTS)
    assert cb.bucket_sizes == [1, 2, 6] and cb.B == 1
    sub = lambda i: _submit(cb, labels[i], noises[i], sps[i])
    ids, out = [sub(0)], {}
    cb._load(0, *cb._queue.popleft())
    for _ in range(3):                                   # alone in the 1-slot bucket (eager steps)
        cb._step()
        cb.steps_run += 1
        cb._account(out)
    ids += [sub(i) for i in range(1, 6)]
    out.update(cb.run())                                 # 6 live: grows to the 6-slot bucket at once
    assert cb.B == 6
    ids += [sub(i) for i in range(6, 8)]
    cb._load(4, *cb._queue.popleft())                    # HIGH slots of the 6-slot bucket: the shrink to 2 slots relocates them
    cb._load(5, *cb._queue.popleft())
    out.update(cb.run())
    assert cb.B == 2
    ids.append(sub(8))
    out.update(cb.run())
    torch.cuda.synchronize()
    assert sorted(out) == ids and cb.B == 1 and cb.switches >= 3
    _check_against_oracle(O.GPTOracle(O.GPTConfig(**KW), sd, torch.float32), out, ids, labels, noises, sps, N)


def test_text_conditional_requests_with_their_own_guidance():
    """t2i: the first image token is sampled on the private prefill engine with the REQUEST's values (an unguided request in a
    guided batcher samples its conditional row alone); checked against generate() with emb_masks."""
    from llamagen_amd.serve import ContinuousBatcher, SamplingParams as SP
    m, sd = _model(KW_T2I, 7)
    N, V, T, C = 16, KW_T2I["vocab_size"], 120, 64
    sps = [SP(cfg_scale=7.5, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0),
           SP(cfg_scale=1.0, cfg_interval=-1, temperature=0.7, top_k=100, top_p=1.0),
           SP(cfg_scale=3.0, cfg_interval=4, temperature=0.9, top_k=0, top_p=0.9)]
    g = torch.Generator().manual_seed(23)
    caps, masks = [], []
    for _ in sps:
        n = int(torch.randint(1, T + 1, (1,), generator=g))
        mk = torch.zeros(T, dtype=torch.int64)
        mk[T - n:] = 1
        caps.append(torch.randn(T, C, generator=g) * mk[:, None])
        masks.append(mk)
    noises = [torch.empty(N, V).exponential_(1, generator=g) for _ in sps]
    cb = ContinuousBatcher(m, 2, N, cfg_scale=7.5, cfg_interval=-1, temperature=1.0, top_k=100, top_p=1.0, sample_logits=True)
    ids, out = [_submit(cb, caps[0], noises[0], sps[0], masks[0])], {}
    cb._load(0, *cb._queue.popleft())
    for _ in range(4):
        cb._step()
        cb.steps_run += 1
        cb._account(out)
    ids += [_submit(cb, c, n, s, k) for c, n, s, k in zip(caps[1:], noises[1:], sps[1:], masks[1:])]
    out.update(cb.run())
    torch.cuda.synchronize()
    assert sorted(out) == ids
    _check_against_oracle(O.GPTOracle(O.GPTConfig(**KW_T2I), sd, torch.float32), out, ids, caps, noises, sps, N, masks)


def test_same_seed_same_tokens_whatever_the_neighbours():
    from llamagen_amd.serve import ContinuousBatcher, SamplingParams as SP
    m, sd = _model(KW, 1)
    N, V, seed, label = 16, KW["vocab_size"], 1234, 6
    sp = SP(cfg_scale=3.0, cfg_interval=-1, temperature=0.9, top_k=50, top_p=1.0, seed=seed)
    cb = ContinuousBatcher(m, 3, N, **DEFAULTS)
    first = cb.submit(label, sampling=sp)                       # slot 0, at once
    for l in (1, 2):
        cb.submit(l, sampling=SP(cfg_scale=1.0, temperature=0.7))
    out = cb.run()
    for l in (3, 4, 5, 7):                                      # other neighbours (unseeded: the global generator), a later slot
        cb.submit(l)
    second = cb.submit(label, sampling=sp)
    out.update(cb.run())
    third = cb.submit(label, sampling=SP(cfg_scale=3.0, cfg_interval=-1, temperature=0.9, top_k=50, top_p=1.0, seed=seed + 1))
    out.update(cb.run())
    torch.cuda.synchronize()
    assert torch.equal(out[first], out[second])
    assert not torch.equal(out[first], out[third])              # another seed is another image
    nz = torch.empty(N, V, device=DEV).exponential_(1.0, generator=torch.Generator(device=DEV).manual_seed(seed)).cpu()
    _check_against_oracle(O.GPTOracle(O.GPTConfig(**KW), sd, torch.float32), out, [first], [label], [nz], [sp], N)


def test_launcher_refuses_missing_records_and_counters():
    from llamagen_amd import _lib as L
    from llamagen_amd.serve import SamplingParams as SP
    B, V = 2, 1024
    _, _, st = _kernel_inputs(torch.float32, B, V, [0, 0], seed=5)
    recs = _records([SP()] * B)
    before = {k: v.clone() for k, v in st.items()}
    fn = L.lib().lgen_sample_rows_params
    args = lambda **kw: [kw.get("logits", L.ptr(st["logits"])), L.ptr(st["noise"]), L.ptr(st["cur"]), L.ptr(st["seq"]),
                         kw.get("row_step", L.ptr(st["row_step"])), kw.get("row_pos", L.ptr(st["row_pos"])), kw.get("max_steps", MAXS),
                         B, V, MAXS, 1, kw.get("params", L.ptr(recs)), L.F32, L.stream()]
    assert fn(*args(params=0)) == L.ERR_BAD_ARG
    assert fn(*args(row_step=0)) == L.ERR_BAD_ARG
    assert fn(*args(row_pos=0)) == L.ERR_BAD_ARG
    assert fn(*args(max_steps=0)) == L.ERR_BAD_ARG
    torch.cuda.synchronize()
    for k in st:
        assert torch.equal(st[k], before[k]), k             # nothing was launched
