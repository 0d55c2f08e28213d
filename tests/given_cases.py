"""Image completion (`given` tokens): the cases, patterns, seeds and the CPU oracle loop shared by tests/test_given_host.py (which
checks on the CPU that every token-exact claim of the GPU tests has a margin) and tests/test_gpu_given.py.

The oracle for given tokens is the loop below, built from GPTOracle.forward, cfg_mix and sample: the reference's generate() with
the token fed back (to both CFG halves) replaced by the given one where there is one; noise[j] belongs to token j whether used or
not.  It records the CFG-mixed logits of every step.

Margins.  The whole-sequence pass of the prefix fast path and the decode steps differ by at most 2e-5 * max(1, |logit|) in fp32
(tests/test_gpu_gpt.py::test_forward_whole_sequence_matches_stepwise), so a token-exact claim through the fast path is made only
where, at every free step, the best and the second-best log(p / q) (the scaled logit when greedy) are more than MARGIN = 1e-3
= 50 x 2e-5 apart in the oracle.  The noise seeds below were chosen for that: the first seed from the case's own rseed upwards
that passes (and, for the top-p case, leaves the nucleus boundary of every free step unambiguous: 11 and 12 do not, 13 does);
tests/test_given_host.py asserts it."""
import torch

from oracle import llamagen_oracle as O
from tests.cases import GPT_CASES, make_gpt_inputs
from tests.util import build_gpt_holder, oracle_cfg

N, GRID = 16, (4, 4)
MARGIN = 1e-3
TOPP_MARGIN = 1e-4          # tests/test_gpu_logprobs.py: the reference log-probability needs an unambiguous nucleus boundary
SKW = ("cfg_scale", "cfg_interval", "temperature", "top_k", "top_p", "sample_logits")

# ---- patterns of the identity tests: bool [N] over the 4 x 4 token grid, the same in every row ---------------------------------
def _prefix(p):
    m = torch.zeros(N, dtype=torch.bool)
    m[:p] = True
    return m


_rc = torch.arange(N).view(*GRID)
PATTERNS = {
    "prefix1": _prefix(1), "prefix5": _prefix(5), "prefix15": _prefix(15), "prefix16": _prefix(16),
    "left_half": ((_rc % GRID[1]) < GRID[1] // 2).reshape(-1),                  # positions 0, 1, 4, 5, ...: P = 2
    "checker": (((_rc // GRID[1]) + (_rc % GRID[1])) % 2 == 0).reshape(-1),      # positions 0, 2, 5, 7, ...: P = 1
}
PATTERN_P = {"prefix1": 1, "prefix5": 5, "prefix15": 15, "prefix16": 15, "left_half": 2, "checker": 1}

# ---- seeds (noise seed per case; chosen on the CPU, see the module docstring) ---------------------------------------------------
IDENTITY_CASE = "tiny_cfg4"
IDENTITY_NOISE_SEED = 11
ORACLE_CASES = ("tiny_cfg4", "tiny_nocfg_temp", "tiny_interval", "tiny_topk_topp", "tiny_greedy", "t2i_cfg")
ORACLE_NOISE_SEED = {"tiny_cfg4": 11, "tiny_nocfg_temp": 11, "tiny_interval": 11, "tiny_topk_topp": 13, "tiny_greedy": 11,
                     "t2i_cfg": 11}
ORACLE_PREFIX = 5            # columns every row gives in the oracle tests; later entries are given with probability 0.3


def sampling_of(case):
    return {k: case[k] for k in SKW}


def noise_for(case, seed):
    """[N, B, V] fp32 Exp(1) draws."""
    V = case["kwargs"]["vocab_size"]
    return torch.empty(N, case["batch"], V).exponential_(1, generator=torch.Generator().manual_seed(seed))


def random_given(case, seed=None):
    """Random given tokens (NOT the ones the run would draw): columns < ORACLE_PREFIX in every row, each later entry with
    probability 0.3 -> int32 [B, N], -1 = free."""
    B, V = case["batch"], case["kwargs"]["vocab_size"]
    g = torch.Generator().manual_seed(case["rseed"] + 500 if seed is None else seed)
    toks = torch.randint(0, V, (B, N), generator=g, dtype=torch.int32)
    mask = torch.rand(B, N, generator=g) < 0.3
    mask[:, :ORACLE_PREFIX] = True
    return torch.where(mask, toks, torch.full_like(toks, -1))


def oracle_model(case):
    _, sd = build_gpt_holder(case)
    return O.GPTOracle(oracle_cfg(case), sd, torch.float32)


def oracle_given(model, cond, given, noise, emb_masks=None, cfg_scale=1.0, cfg_interval=-1, temperature=1.0, top_k=0, top_p=1.0,
                 sample_logits=True):
    """oracle.generate() (generate.py:126-176) with given tokens: returns (seq int32 [B, N], trace: the N CFG-mixed fp32 logits
    [B, V]).  given int [B, N] (-1 free) or None."""
    cfg = model.cfg
    B, n_new = cond.shape[0], noise.shape[0] if noise is not None else N
    guided = cfg_scale > 1.0
    if cfg.model_type == "c2i":
        cc, T = (torch.cat([cond, torch.ones_like(cond) * cfg.num_classes]) if guided else cond), 1
    else:
        null = torch.zeros_like(cond) + model.p["cls_embedding.uncond_embedding"].to(cond.dtype)
        cc, T = (torch.cat([cond, null]) if guided else cond), cond.shape[1]
    model.setup_caches(2 * B if guided else B, T + n_new)
    if emb_masks is not None:
        em = torch.cat([emb_masks, emb_masks]) if guided else emb_masks
        cm = model.causal_mask
        cm[:, :, :T] = cm[:, :, :T] & (em.unsqueeze(1) != 0)
        model.causal_mask = cm | torch.eye(cm.size(1), cm.size(2), dtype=torch.bool)
    skw = dict(temperature=temperature, top_k=top_k, top_p=top_p, sample_logits=sample_logits)
    seq = torch.empty(B, n_new, dtype=torch.int32)
    trace = []
    cur = None
    for j in range(n_new):
        if j == 0:
            logits = model.forward(None, cc, torch.arange(0, T))
        else:
            x = torch.cat([cur, cur]) if guided else cur
            logits = model.forward(x.view(-1, 1), None, torch.tensor([T + j - 1]))
        flag = not (j > 0 and cfg_interval > -1 and (j - 1) > cfg_interval)      # generate.py:113-114 at decode iteration j - 1
        mixed = O.cfg_mix(logits, cfg_scale, flag)[:, -1]
        trace.append(mixed.clone())
        nxt, _ = O.sample(mixed, noise=noise[j] if sample_logits else None, **skw)
        nxt = nxt.view(-1).to(torch.int32)
        if given is not None:
            nxt = torch.where(given[:, j] >= 0, given[:, j].to(torch.int32), nxt)
        seq[:, j] = nxt
        cur = nxt.long().view(-1, 1)
    return seq, trace


def step_margins(trace, noise, temperature=1.0, top_k=0, top_p=1.0, sample_logits=True, **_):
    """[B, N] float64: at step j of row b, the gap between the best and the second-best log(p / q) over the kept set (the scaled
    logit when greedy) -- how far the oracle's choice is from flipping."""
    out = []
    for j, mixed in enumerate(trace):
        l = mixed / max(temperature, 1e-5)
        if top_k > 0 or top_p < 1.0:
            l = O.top_k_top_p_filtering(l, top_k=top_k, top_p=top_p)
        s = l.double() if not sample_logits else torch.log_softmax(l.double(), dim=-1) - noise[j].double().log()
        top2 = torch.topk(s, 2, dim=-1)[0]
        out.append(top2[:, 0] - top2[:, 1])
    return torch.stack(out, dim=1)


def topp_margin(l, top_k, top_p):
    """tests/test_gpu_logprobs.py::topp_margin: distance between top_p and the oracle's cumulative probability on both sides of the
    nucleus cut, over the rows of the scaled logits l."""
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


def ref_logprobs(trace, seq, given, temperature=1.0, top_k=0, top_p=1.0, **_):
    """float64 [B, N] reference log-probabilities and the largest |scaled logit|: a free token under the oracle's kept set
    (tests/test_gpu_logprobs.py::ref_logprob), a given token under the log-softmax of the whole scaled row (what score() returns).
    Asserts the top-p precondition on the free rows."""
    cols, mag = [], 0.0
    for j, mixed in enumerate(trace):
        l = mixed.float() / max(temperature, 1e-5)
        mag = max(mag, float(l.abs().max()))
        free = torch.ones(l.shape[0], dtype=torch.bool) if given is None else given[:, j] < 0
        full = torch.log_softmax(l.double(), dim=-1)
        kept = full
        if (top_k > 0 or top_p < 1.0) and bool(free.any()):
            assert topp_margin(l[free], top_k, top_p) >= TOPP_MARGIN, "ambiguous nucleus boundary: choose another seed"
            kept = torch.log_softmax(O.top_k_top_p_filtering(l, top_k=top_k, top_p=top_p).double(), dim=-1)
        idx = seq[:, j].long().view(-1, 1)
        cols.append(torch.where(free, kept.gather(1, idx).view(-1), full.gather(1, idx).view(-1)))
    return torch.stack(cols, dim=1), mag


_cache = {}


def oracle_run(name, kind):
    """The CPU oracle's run of one test case, computed once per process and shared: kind "identity" (IDENTITY_CASE drawn freely:
    its own tokens are what the identity tests give back) or "oracle" (ORACLE_CASES with random_given()).
    -> dict(case, cond, masks, noise, given, seq, trace, margins)."""
    key = (name, kind)
    if key not in _cache:
        case = GPT_CASES[name]
        assert case["n_new"] == N and case["kwargs"]["block_size"] == N
        cond, masks = make_gpt_inputs(case)
        noise = noise_for(case, IDENTITY_NOISE_SEED if kind == "identity" else ORACLE_NOISE_SEED[name])
        given = None if kind == "identity" else random_given(case)
        skw = sampling_of(case)
        seq, trace = oracle_given(oracle_model(case), cond, given, noise, emb_masks=masks, **skw)
        _cache[key] = dict(case=case, cond=cond, masks=masks, noise=noise, given=given, seq=seq, trace=trace, skw=skw,
                           margins=step_margins(trace, noise, **skw))
    return _cache[key]
