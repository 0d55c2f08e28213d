"""CPU stand-in of llamagen_amd.serve.ContinuousBatcher for the host tests: the REAL constructor on a tiny CPU Transformer, with the
two device-bound methods replaced -- `_bucket` (no DecodeEngine, only the tensors _switch() moves) and `_step` (token =
label * 1000 + step, written into the slot's sequence exactly where the sampler kernel would)."""
import types

import torch

from llamagen_amd.gpt import ModelArgs, Transformer
from llamagen_amd.serve import ContinuousBatcher

# V == 32 and num_classes == 1000 are what the host tests count on; the weights are never read
CPU_MODEL = Transformer(ModelArgs(dim=32, n_layer=1, n_head=1, multiple_of=32, vocab_size=32, block_size=16, num_classes=1000))


class _Eng:  # the tensors _switch() moves between buckets
    def __init__(self, rows, S8):
        self.k_cache = torch.zeros(1, rows, 1, S8, 1)
        self.v_cache = torch.zeros(1, rows, 1, S8, 1)
        self.cur_tok = torch.zeros(rows, dtype=torch.int32)


class _Batcher(ContinuousBatcher):
    def __init__(self, slots, N, cfg=True, greedy=True, buckets=None, shrink_after=2):
        self.active_per_step, self.bucket_per_step = [], []
        self.records_seen = {}     # request id -> (slot, its sampling record) at every step it ran
        self.marks = {}            # request / candidate id -> (added to each of its tokens, log-probability of each): default (0, 0.0)
        super().__init__(CPU_MODEL, slots, N, cfg_scale=4.0 if cfg else 1.0, top_k=100, sample_logits=not greedy,
                         slot_buckets=buckets, shrink_after=shrink_after)

    def _bucket(self, size):
        if size not in self._buckets:
            rows = 2 * size if self.use_cfg else size
            self._buckets[size] = types.SimpleNamespace(B=size, B2=rows, eng=_Eng(rows, self.S8), graph=None,
                                                        row_pos=torch.full((rows,), 1, dtype=torch.int32),
                                                        cond=torch.full((rows,), 1000, dtype=torch.int32))
        return self._buckets[size]

    def _step(self):
        live, e = 0, self.eng
        for b in range(self.B):
            st = int(self.row_step[b])
            if st < self.N:  # an occupied slot: what the layer chain (K/V append) and the sampler kernel do for it
                label, rid = int(self.cond[b]), self._slot_req[b]
                rows = [b] + ([self.B + b] if self.use_cfg else [])
                for r in rows:
                    assert int(self.row_pos[r]) == st
                    # the request's earlier K/V entries are in ITS rows of the current bucket, whatever bucket wrote them
                    assert e.k_cache[0, r, 0, :st, 0].tolist() == [label * 1000 + p + (0.5 if r != b else 0) for p in range(st)], (b, st)
                    e.k_cache[0, r, 0, st, 0] = label * 1000 + st + (0.5 if r != b else 0)
                    assert st == 0 or int(e.cur_tok[r]) == label * 1000 + st - 1
                    e.cur_tok[r] = label * 1000 + st
                    self.row_pos[r] += 1
                extra, logp = self.marks.get(rid, (0, 0.0))
                self.seq[b, st] = label * 1000 + st + extra
                self.logp[b, st] = logp
                self.records_seen.setdefault(rid, []).append((b, self.params[b].tolist()))
                self.row_step[b] += 1
                live += 1
        self.active_per_step.append(live)
        self.bucket_per_step.append(self.B)
