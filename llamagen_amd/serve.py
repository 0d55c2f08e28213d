"""Token-level continuous batching of class-conditional sampling on the HIP engine.

What it stands in for: the reference's vLLM fork (autoregressive/serve/llm.py:22-267 request queue + engine loop,
serve/sampler.py:54-58,106-108 paired conditional / unconditional sequences with CFG applied at sampling time,
serve/model_runner.py:36-41,982-1076 graph replay over a fixed batch).  Same idea, MI355X-native form:

  * a fixed number of SLOTS; slot b owns rows b (conditional) and B + b (unconditional) of the step batch, its own KV-cache
    rows and its own Exp(1) noise block -- nothing of one request touches another's rows;
  * ONE captured hipGraph per step batch: embed (per-row source) -> L x [norm+wqkv+RoPE+append | attention | wo | norm+w1,w3 |
    w2] -> norm+lm_head -> sample, all with PER-ROW positions (`row_pos`, device ints): a row at position 0 is a fresh
    request and takes its class embedding, any other row continues with the token it sampled in the previous step;
  * the host refills finished slots between replays (a handful of scalar writes per new request, no device sync: a request
    that entered at replay k is complete after replay k + N - 1, which the host knows without asking the GPU).

Text-conditional requests (round 3) bring a [T, caption_dim] caption (left-padded, with its emb_mask, like generate()): the
T-token prefix of ONE request is prefilled on a private two-row engine (CaptionEmbedder MLP + all T positions per layer at once,
the first image token sampled there), its K/V slots 0..T-1 and its mask rows are copied into the slot's rows, and the slot joins
the step batch at position T -- the per-request prefill of the vLLM fork (serve/model_runner.py:982-1076) without stalling the
other slots' graph replays for longer than that one prefill.

Slot-count buckets (`slot_buckets=(16, 32)` next to `slots=64`; the captured-batch-size ladder of serve/model_runner.py:36-41):
one engine + one captured graph per bucket, built on first use.  Before a step the batcher picks the smallest bucket that holds
the live requests (running + queued); growing is immediate, shrinking waits `shrink_after` steps.  A switch moves every running
request -- its K/V rows, token, position, class id and mask rows, and (when its slot index changes) its noise block and token row
-- into the new bucket's rows with stream-ordered device copies, so a lightly loaded server replays a 32-row graph instead of a
128-row one and still never recomputes a prefix.

Per-request sampling (serve/llm.py:141-210 one SamplingParams per prompt, serve/sampler.py:65-83 per-sequence temperature /
top-k / top-p, serve/model_runner.py:620-645 per-request seeds): `submit(..., sampling=SamplingParams(...))` overrides the
constructor's values -- which are the DEFAULTS -- for that request.  The values travel as one 32-byte record per slot in a
slot-indexed device tensor that the sampler kernel reads (lgen_sample_rows_params).  Whether the step batch has unconditional rows
is fixed by the constructor (it fixes the row layout and the captured graphs): an unguided request in a guided batcher samples its
conditional logits unchanged and still pays for its unconditional row.

Log-probabilities and best-of-N (serve/sampler.py:88-93,119-123 the sampled token's log-probability under the final sampling
distribution, :357-365 `cumulative_logprob`, serve/llm.py `best_of`): every step also writes the token's log-probability into a
slot-indexed buffer (lgen_sample_rows_params_logprob: the same tokens, one more float per slot); `run(return_outputs=True)` returns
RequestOutput records.  `SamplingParams(best_of=k)` runs k candidates of one request in k slots (seed + j each) and answers with
the likeliest; the choice is an argmax on the device, nothing waits for it.

Image completion (`submit(..., given=ids)`, llamagen_amd/given.py): a request may fix any of its N tokens.  The tokens travel in a
slot-indexed `given` buffer next to `seq` (-1 = free; moved with the request on a bucket switch, shared by `best_of` candidates);
every step samples through lgen_sample_rows_params_given, so a slot at a given entry takes that token instead of drawing one, in the
same one graph per bucket.  A request still takes N steps (no start at step P from a private prefill).

Every request produces exactly the tokens a batch-of-one `generate()` would with the same noise and sampling values: rows are
independent through every kernel (tests/test_gpu_serve.py and tests/test_gpu_serve_params.py hold that to the oracle, token for
token, in fp32).
"""
from __future__ import annotations

import collections
import ctypes
import dataclasses
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .engine import DecodeEngine
from .given import check_given
from .gpt import find_multiple, kv_cache_refuse


def bucket_ladder(slots: int, slot_buckets: Optional[Sequence[int]]) -> List[int]:
    """Ascending captured slot counts; the full `slots` is always the last one."""
    if slots < 1:
        raise ValueError("slots must be >= 1")
    sizes = sorted({int(b) for b in (slot_buckets or ())})
    if sizes and (sizes[0] < 1 or sizes[-1] > slots):
        raise ValueError(f"slot_buckets must lie in [1, {slots}]")
    return [b for b in sizes if b < slots] + [slots]


def pick_bucket(sizes: Sequence[int], live: int) -> int:
    """Smallest captured slot count that holds `live` requests (the largest when none does)."""
    for b in sizes:
        if b >= live:
            return b
    return sizes[-1]


def pick_best(cumulative: Sequence[float]) -> int:
    """The `best_of` winner: the candidate with the largest cumulative log-probability, the lowest index among equals (what
    torch.argmax gives the device-side selection: the first maximum)."""
    best = 0
    for j in range(1, len(cumulative)):
        if cumulative[j] > cumulative[best]:
            best = j
    return best


def check_best_of(sampling: "SamplingParams", slots: int, has_noise: bool = False) -> int:
    """The number of slots a request's candidates take, or ValueError: every candidate needs a slot of its own, and k candidates
    cannot share one explicit noise block."""
    k = int(sampling.best_of)
    if k > int(slots):
        raise ValueError(f"best_of {k} exceeds the batcher's {slots} slots")
    if k > 1 and has_noise:
        raise ValueError("best_of > 1 draws one noise block per candidate: give a seed, not `noise`")
    return k


def plan_moves(active: Sequence[bool], new_slots: int):
    """(old slot, new slot) for every running request when the slot count becomes `new_slots`: a request keeps its index when
    that still exists, otherwise it takes the lowest free one."""
    run = [s for s, a in enumerate(active) if a]
    if len(run) > new_slots:
        raise ValueError(f"{len(run)} running requests do not fit {new_slots} slots")
    free = [t for t in range(new_slots) if not (t < len(active) and active[t])]
    return [(s, s) if s < new_slots else (s, free.pop(0)) for s in run]


@dataclasses.dataclass(frozen=True)
class SamplingParams:
    """Sampling values of one request (the fields of the vLLM fork's SamplingParams that serve/sampler.py:65-83 consumes, plus the
    guidance pair of serve/sampler.py:54-58 and the per-request seed of serve/model_runner.py:620-645)."""
    cfg_scale: float = 1.0
    cfg_interval: int = -1
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    sample_logits: bool = True
    seed: Optional[int] = None
    logprobs: bool = False      # informational (the batcher records every token's log-probability anyway): ask for RequestOutputs
    best_of: int = 1            # candidates drawn for this request; the likeliest (largest cumulative log-probability) is returned

    def __post_init__(self):
        for name in ("cfg_scale", "temperature", "top_p"):
            if not math.isfinite(float(getattr(self, name))):
                raise ValueError(f"{name} must be finite, got {getattr(self, name)}")
        if not 0.0 < float(self.top_p) <= 1.0:
            raise ValueError(f"top_p must lie in (0, 1], got {self.top_p}")
        if int(self.top_k) < 0:
            raise ValueError(f"top_k must be >= 0 (0 = off), got {self.top_k}")
        if int(self.top_k) != self.top_k or int(self.cfg_interval) != self.cfg_interval:
            raise ValueError("top_k and cfg_interval are integers")
        if isinstance(self.best_of, bool) or int(self.best_of) != self.best_of or int(self.best_of) < 1:
            raise ValueError(f"best_of must be an integer >= 1, got {self.best_of}")
        if int(self.best_of) > 1 and not self.sample_logits:
            raise ValueError("best_of > 1 needs sample_logits=True (greedy candidates are all the same)")


@dataclasses.dataclass
class RequestOutput:
    """What one request produced (the fields of the vLLM fork's CompletionOutput this project fills): device tensors, enqueued on
    the current stream."""
    token_ids: torch.Tensor            # int32 [N]
    logprobs: torch.Tensor             # fp32 [N]: log-probability of each token under the distribution it was drawn from
    cumulative_logprob: torch.Tensor   # 0-d float64: logprobs.double().sum() (serve/sampler.py:357-365)


def pack_sampling(sp: SamplingParams) -> np.ndarray:
    """The 32-byte device record of one slot (lgen_slot_sampling, include/lgen.h) as 8 int32 words: three floats (cfg_scale,
    temperature, top_p), three ints (cfg_interval, top_k, greedy), two reserved words.  `seed` is host-side only."""
    rec = L.SlotSampling(float(sp.cfg_scale), float(sp.temperature), float(sp.top_p), int(sp.cfg_interval), int(sp.top_k),
                         0 if sp.sample_logits else 1)
    return np.frombuffer(bytes(rec), dtype=np.int32).copy()


RECORD_WORDS = ctypes.sizeof(L.SlotSampling) // 4


class _Bucket:
    """One captured slot count: its engine (KV rows, activations), per-row positions / class ids and its step graph."""

    def __init__(self, model, slots: int, use_cfg: bool, S8: int, dtype, dev):
        self.B = slots
        self.B2 = 2 * slots if use_cfg else slots
        self.eng = e = DecodeEngine(model, self.B2, S8, dtype)
        R = e.MTs * 16
        # parked rows sit at position 1: a valid slot that is not 0 (= "fresh class-conditional request" for lgen_embed_rows) and
        # costs the attention two keys per idle row instead of a full sequence
        self.row_pos = torch.full((R,), 1, dtype=torch.int32, device=dev)
        self.cond = torch.full((R,), int(model.num_classes), dtype=torch.int32, device=dev)   # uncond rows: the null class
        e.pos_rows = self.row_pos  # switches the engine's layer chain to the per-row entry points
        self.graph = None


class ContinuousBatcher:
    def __init__(self, model, slots: int, max_new_tokens: int, cfg_scale: float = 1.0, cfg_interval: int = -1,
                 temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, sample_logits: bool = True,
                 slot_buckets: Optional[Sequence[int]] = None, shrink_after: int = 8):
        if model.model_type not in ("c2i", "t2i"):
            raise Exception("please check model type")
        kv_cache_refuse(model, "the continuous batcher (per-row positions)")
        dev = model.tok_embeddings.weight.device
        self.model, self.dev = model, dev
        self.num_classes, self.V = int(model.num_classes), int(model.config.vocab_size)
        self.t2i = model.model_type == "t2i"
        self.T = int(model.cls_token_num) if self.t2i else 1
        self.slots, self.N = int(slots), max_new_tokens
        self.use_cfg = cfg_scale > 1.0
        self._dtype = model.tok_embeddings.weight.dtype
        self.S8 = find_multiple(self.T + max_new_tokens, 8)
        if max_new_tokens > model.block_size:
            raise IndexError(f"{max_new_tokens} tokens exceed block_size {model.block_size}")
        self.bucket_sizes = bucket_ladder(self.slots, slot_buckets)
        self.shrink_after = max(1, int(shrink_after))
        self._buckets: Dict[int, _Bucket] = {}
        self._shrink_wait = 0
        self.switches = 0
        self.cur = self._bucket(self.bucket_sizes[0] if len(self.bucket_sizes) > 1 else self.slots)
        # slot-indexed state shared by every bucket (bucket k uses slots 0 .. k-1)
        self.row_step = torch.full((slots,), max_new_tokens, dtype=torch.int32, device=dev)  # >= N: empty slot
        self.noise = torch.empty(slots, max_new_tokens, self.V, dtype=torch.float32, device=dev) if sample_logits else None
        self.seq = torch.zeros(slots, max_new_tokens, dtype=torch.int32, device=dev)
        self.logp = torch.zeros(slots, max_new_tokens, dtype=torch.float32, device=dev)   # log-probability of seq's tokens
        # image completion: the tokens a request fixes (-1 = free), read by the sampler at (slot, step) like seq is written
        self.given = torch.full((slots, max_new_tokens), -1, dtype=torch.int32, device=dev)
        self._req_given: Dict[int, torch.Tensor] = {}   # queued requests (candidates) that brought given tokens: int32 [N], CPU
        self._cand: Dict[int, tuple] = {}      # candidate id -> (request id, j) of a best_of request
        self._group: Dict[int, list] = {}      # request id -> its candidates' RequestOutputs (None until finished)
        # the constructor's sampling values: what a request that brings no SamplingParams gets
        self.defaults = SamplingParams(cfg_scale=float(cfg_scale), cfg_interval=int(cfg_interval), temperature=float(temperature),
                                       top_k=int(top_k), top_p=float(top_p), sample_logits=bool(sample_logits))
        self.params = torch.zeros(slots, RECORD_WORDS, dtype=torch.int32, device=dev)  # lgen_slot_sampling per slot
        self._req_sampling: Dict[int, SamplingParams] = {}   # queued requests that brought their own values
        self._pe = None             # t2i: the private prefill engine (built on the first caption request)
        self._queue = collections.deque()
        self._slot_req: List[Optional[int]] = [None] * slots
        self._slot_left = [0] * slots
        self._next_id = 0
        self.steps_run = 0

    # the bucket in use: rows b and B + b pair up, so B is the CURRENT bucket's slot count
    B = property(lambda self: self.cur.B)
    B2 = property(lambda self: self.cur.B2)
    eng = property(lambda self: self.cur.eng)
    row_pos = property(lambda self: self.cur.row_pos)
    cond = property(lambda self: self.cur.cond)

    def _bucket(self, size: int) -> _Bucket:
        """The bucket of `size` slots, built on first use: the only place the constructor touches the device (the CPU tests of the
        host logic override it and `_step`)."""
        if size not in self._buckets:
            if self.dev.type != "cuda":
                raise RuntimeError("llamagen_amd.serve runs only on an AMD GPU through the HIP library (no CPU fallback)")
            self._buckets[size] = _Bucket(self.model, size, self.use_cfg, self.S8, self._dtype, self.dev)
        return self._buckets[size]

    # ---- bucket choice and migration --------------------------------------------------------------------------------------
    def _live(self) -> int:
        return sum(r is not None for r in self._slot_req) + len(self._queue)

    def _choose(self):
        """Grow at once when the live requests do not fit, shrink after `shrink_after` consecutive steps in which they would."""
        want = pick_bucket(self.bucket_sizes, self._live())
        if want > self.cur.B:
            self._switch(self._bucket(want))
        elif want < self.cur.B:
            self._shrink_wait += 1
            if self._shrink_wait >= self.shrink_after:
                self._switch(self._bucket(want))
        else:
            self._shrink_wait = 0

    def _switch(self, nb: _Bucket):
        """Move every running request from the current bucket's rows into `nb`'s (stream-ordered device copies)."""
        ob = self.cur
        moves = plan_moves([r is not None for r in self._slot_req], nb.B)
        oe, ne = ob.eng, nb.eng
        for s, t in moves:
            for src, dst in ((s, t),) + (((ob.B + s, nb.B + t),) if self.use_cfg else ()):
                ne.k_cache[:, dst].copy_(oe.k_cache[:, src])
                ne.v_cache[:, dst].copy_(oe.v_cache[:, src])
                ne.cur_tok[dst:dst + 1].copy_(oe.cur_tok[src:src + 1])
                nb.row_pos[dst:dst + 1].copy_(ob.row_pos[src:src + 1])
                nb.cond[dst:dst + 1].copy_(ob.cond[src:src + 1])
                if self.t2i:
                    ne.causal_mask[dst].copy_(oe.causal_mask[src])
            if t != s:
                if self.noise is not None:
                    self.noise[t].copy_(self.noise[s])
                self.seq[t].copy_(self.seq[s])
                self.given[t].copy_(self.given[s])
                self.logp[t].copy_(self.logp[s])
                self.params[t].copy_(self.params[s])
                self.row_step[t:t + 1].copy_(self.row_step[s:s + 1])
                self.row_step[s] = self.N
                self._slot_req[t], self._slot_left[t] = self._slot_req[s], self._slot_left[s]
                self._slot_req[s], self._slot_left[s] = None, 0
        ob.row_pos.fill_(1)  # the old bucket's rows idle until it is used again
        self.cur = nb
        self._shrink_wait = 0
        self.switches += 1

    # ---- requests ---------------------------------------------------------------------------------------------------
    def submit(self, class_label, noise: Optional[torch.Tensor] = None, emb_mask: Optional[torch.Tensor] = None,
               sampling: Optional[SamplingParams] = None, given: Optional[torch.Tensor] = None) -> int:
        """Queue one image request; `noise` (optional, [N, V] fp32 Exp(1) draws) replaces the default generator's draw.
        c2i: `class_label` is the class id.  t2i: `class_label` is the caption embedding [T, caption_dim] (left-padded and already
        multiplied by its mask, sample_t2i.py:95-108) and `emb_mask` its [T] validity mask.
        `sampling` (serve/llm.py:141-210) replaces the constructor's sampling values for this request; with a `seed` and no `noise`
        the request's Exp(1) block comes from a generator of its own, so its tokens do not depend on slot, arrival or neighbours.
        `given` (image completion): integer [N], -1 = free, a value in [0, vocab) fixes token j (generate()'s argument for one
        request); the candidates of a best_of request share it.  The request still takes N steps."""
        if sampling is not None:
            if not isinstance(sampling, SamplingParams):
                raise TypeError("sampling must be a llamagen_amd.serve.SamplingParams")
            if sampling.cfg_scale > 1.0 and not self.use_cfg:
                raise ValueError("cfg_scale > 1 needs a batcher built with cfg_scale > 1 (the step batch has no unconditional rows)")
            if sampling.sample_logits and self.noise is None:
                raise ValueError("sample_logits=True needs a batcher built with sample_logits=True (a greedy batcher has no noise buffer)")
            check_best_of(sampling, self.slots, noise is not None)
        if self.t2i:
            cap = class_label
            if not torch.is_tensor(cap) or cap.dim() != 2 or cap.shape[0] != self.T:
                raise ValueError(f"a text-conditional request is a [{self.T}, caption_dim] caption embedding")
            if emb_mask is not None and tuple(emb_mask.shape) != (self.T,):
                raise ValueError(f"emb_mask must be [{self.T}]")
            label = (cap, emb_mask)
        else:
            label = int(class_label)
            if not 0 <= label <= self.num_classes:  # num_classes itself is the null class (LabelEmbedder table row, gpt.py:66-72);
                raise IndexError(f"class label {label} outside [0, {self.num_classes}]")  # the reference's nn.Embedding raises too
        if noise is not None:
            if self.noise is None:
                raise ValueError("noise given but the batcher was built with sample_logits=False (greedy)")
            if tuple(noise.shape) != (self.N, self.V):
                raise ValueError(f"noise must be [{self.N}, {self.V}] fp32 Exp(1) draws, got {tuple(noise.shape)}")
        if given is not None:
            given = check_given(given, (self.N,), self.V)
        rid = self._next_id
        self._next_id += 1
        if sampling is not None and sampling.best_of > 1:
            # k candidates of ONE request: k queue entries with ids of their own (never handed out), the same conditioning and
            # seed + j; _output() answers under `rid` with the likeliest once the last one is through
            k = int(sampling.best_of)
            self._group[rid] = [None] * k
            for j in range(k):
                cid = self._next_id
                self._next_id += 1
                self._cand[cid] = (rid, j)
                self._req_sampling[cid] = dataclasses.replace(sampling, best_of=1,
                                                              seed=None if sampling.seed is None else int(sampling.seed) + j)
                if given is not None:
                    self._req_given[cid] = given
                self._queue.append((cid, label, None))
            return rid
        if sampling is not None:   # a side table, not a fourth queue field: the queue entries stay (rid, label, noise)
            self._req_sampling[rid] = sampling
        if given is not None:      # a side table like the sampling values
            self._req_given[rid] = given
        self._queue.append((rid, label, noise))
        return rid

    def _sampling_of(self, rid: int) -> SamplingParams:
        """The request's own values (taken out of the side table), else the constructor's."""
        return self._req_sampling.pop(rid, self.defaults)

    def _load(self, b: int, rid: int, label, noise):
        """Slot b <- a fresh request: position / step 0, its class label, its noise block and its sampling record (stream-ordered
        writes, no sync)."""
        sp = self._sampling_of(rid)
        rec = torch.from_numpy(pack_sampling(sp))
        if self.params.is_cuda:   # pinned staging: the copy is enqueued, the host does not wait for it
            rec = rec.pin_memory()
        self.params[b].copy_(rec, non_blocking=True)
        given = self._req_given.pop(rid, None)
        if given is None:
            self.given[b].fill_(-1)
        else:
            self.given[b].copy_(given)
        if self.noise is not None:
            if noise is not None:
                self.noise[b].copy_(noise.to(self.dev))
            elif not sp.sample_logits:
                pass  # a greedy request reads no noise: nothing drawn, the other requests' draws stay where they were
            elif sp.seed is not None:   # serve/model_runner.py:620-645: a generator per seeded request
                self.noise[b].exponential_(1.0, generator=torch.Generator(device=self.dev).manual_seed(int(sp.seed)))
            else:
                self.noise[b].exponential_(1.0)
        if self.t2i:
            self._load_caption(b, *label, sp)
            self._slot_req[b], self._slot_left[b] = rid, self.N - 1   # the first token was sampled by the prefill
            return
        self.row_pos[b] = 0
        self.row_step[b] = 0
        self.cond[b] = label
        if self.use_cfg:
            self.row_pos[self.B + b] = 0
        self._slot_req[b], self._slot_left[b] = rid, self.N

    def _load_caption(self, b: int, cap: torch.Tensor, emb_mask, sp: SamplingParams):
        """Per-request prefill of a text-conditional request (generate.py:128-170 for ONE image): caption (+ null caption with
        CFG) through the CaptionEmbedder and all T prefix positions of every layer on the private engine, first image token sampled
        from the slot's noise block with the REQUEST's sampling values (an unguided request of a guided batcher samples its
        conditional row alone), then K/V slots 0..T-1, mask rows, token and counters move into slot b of the step batch."""
        e, T, dev = self.eng, self.T, self.dev
        rows = 2 if self.use_cfg else 1
        if self._pe is None:
            self._pe = DecodeEngine(self.model, rows, self.S8, e.dtype)
        pe = self._pe
        pe.reset(rows)
        cond = cap.to(device=dev, dtype=e.dtype).unsqueeze(0)
        if self.use_cfg:
            cond = torch.cat([cond, self.model.cls_embedding.uncond_embedding.to(device=dev, dtype=e.dtype).unsqueeze(0)])
        pe.fold_emb_masks(None if emb_mask is None else emb_mask[None], T)   # [1, T]: both rows see the same pattern
        pe.use_mask = True   # also without a mask
        pe._prefill_prefix(pe.caption_embed(cond))
        pe.state[0] = T - 1
        pe.state[1] = 0
        pe._final_logits()
        first = dict(use_cfg=self.use_cfg and sp.cfg_scale > 1.0, cfg_scale=sp.cfg_scale, cfg_interval=sp.cfg_interval,
                     temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p, sample_logits=sp.sample_logits)
        pe.noise = self.noise[b].view(self.N, 1, self.V) if self.noise is not None else None
        if pe.given is None:
            pe.given = torch.full_like(pe.seq, -1)
        pe.given[0, 0:1].copy_(self.given[b, 0:1])   # column 0 of the request's given tokens: the prefill samples token 0
        pe._sample(1, first, pe.logp, pe.given)   # writes cur_tok[0]; both step-batch rows take it below
        for src, dst in ((0, b),) + (((1, self.B + b),) if self.use_cfg else ()):
            e.k_cache[:, dst, :, :T].copy_(pe.k_cache[:, src, :, :T])
            e.v_cache[:, dst, :, :T].copy_(pe.v_cache[:, src, :, :T])
            e.causal_mask[dst].copy_(pe.causal_mask[src])
            e.cur_tok[dst:dst + 1].copy_(pe.cur_tok[0:1])
            self.row_pos[dst] = T
        self.seq[b, 0:1].copy_(pe.seq[0, 0:1])
        self.logp[b, 0:1].copy_(pe.logp[0, 0:1])
        self.row_step[b] = 1

    # ---- one step of the whole slot batch -------------------------------------------------------------------------------
    def _step(self):
        e, lib = self.eng, self.eng.lib
        cls = e.tok_emb if self.t2i else e.cls_emb   # t2i rows never sit at position 0 (their prefix is prefilled): table unused
        L.check(lib.lgen_embed_rows(L.ptr(e.tok_emb), L.ptr(cls), L.ptr(e.cur_tok), L.ptr(self.cond), L.ptr(self.row_pos),
                                    L.ptr(e.hp), L.ptr(e.ssq) if e.fuse_norm else 0, self.B2, e.MTs, e.d, e.tok_emb.shape[0],
                                    cls.shape[0], e.dt, L.stream()), "embed_rows")
        e.ssq_parts = e.d // 16
        e._layers_and_logits()
        # noise is null only in a batcher built greedy, and submit() lets no sampled request into one (the kernel's contract)
        # always the `given` form (a slot without given tokens holds -1 throughout): one graph per bucket
        L.check(lib.lgen_sample_rows_params_given(L.ptr(e.logits), L.ptr(self.noise), L.ptr(e.cur_tok), L.ptr(self.seq),
                                                  L.ptr(self.row_step), L.ptr(self.row_pos), self.N, self.B, e.V, self.N,
                                                  1 if self.use_cfg else 0, L.ptr(self.params), e.dt, L.ptr(self.logp),
                                                  L.ptr(self.given), L.stream()), "sample_rows_params_given")

    def run(self, use_graph: bool = True, return_outputs: bool = False):
        """Drain the queue; returns {request id: int32 [N] token ids} (device tensors, enqueued on the current stream), with
        return_outputs=True {request id: RequestOutput} (tokens, per-token log-probabilities and their sum)."""
        done: Dict[int, object] = {}
        full = bool(return_outputs)
        with torch.no_grad():
            while self._queue or any(r is not None for r in self._slot_req):
                if len(self.bucket_sizes) > 1:
                    self._choose()
                for b in range(self.B):  # refill free slots (arrival order)
                    if self._slot_req[b] is None and self._queue:
                        self._load(b, *self._queue.popleft())
                if use_graph:
                    if self.cur.graph is None:
                        self._step()  # warm every kernel once, eagerly
                        self.steps_run += 1
                        self._account(done, full)
                        g = torch.cuda.CUDAGraph()
                        torch.cuda.synchronize()
                        with torch.cuda.graph(g):
                            self._step()
                        self.cur.graph = g
                        continue
                    self.cur.graph.replay()
                else:
                    self._step()
                self.steps_run += 1
                self._account(done, full)
        return done

    def _output(self, b: int, full: bool):
        """(request id, result) of slot b's finished request, called right after the step that wrote its last token was enqueued:
        the tokens, or with `full` a RequestOutput; (None, None) for a best_of candidate whose request still has others running."""
        cid = self._slot_req[b]
        cand = self._cand
        if cid not in cand and not full:
            return cid, self.seq[b].clone()
        lp = self.logp[b].clone()
        out = RequestOutput(self.seq[b].clone(), lp, lp.double().sum())
        if cid not in cand:
            return cid, out
        rid, j = cand.pop(cid)
        group = self._group[rid]
        group[j] = out
        if any(o is None for o in group):
            return None, None
        del self._group[rid]
        # pick_best() on the device: argmax returns the first maximum, index_select takes its row -- no host sync
        win = torch.stack([o.cumulative_logprob for o in group]).argmax().view(1)
        take = lambda name: torch.stack([getattr(o, name) for o in group]).index_select(0, win)[0]
        return rid, RequestOutput(take("token_ids"), take("logprobs"), take("cumulative_logprob")) if full else take("token_ids")

    def _account(self, done, full: bool = False):
        for b in range(self.B):
            if self._slot_req[b] is None:
                continue
            self._slot_left[b] -= 1
            if self._slot_left[b] == 0:  # the step just enqueued wrote this request's last token
                rid, out = self._output(b, full)
                if rid is not None:
                    done[rid] = out
                self._slot_req[b] = None
                self.row_pos[b] = 1          # park the rows again (after that step, stream-ordered): an idle row at its final
                if self.use_cfg:             # position would keep costing the attention a full sequence
                    self.row_pos[self.B + b] = 1
