"""Image completion, host side: the `given` argument of generate() / ContinuousBatcher.submit() -- "these tokens are fixed,
sample the rest" -- as pure functions (no device, no library), and complete(): encode -> given -> generate -> decode.

given: integer [B, N] (N = max_new_tokens; [N] for one batcher request).  -1: the position is free.  A value in [0, vocab): token j
of row b IS this.  At a given position the model still runs (K/V appended, position advanced); the token written to the sequence
and fed back to both CFG halves is the given one, and noise[j] stays token j's draw whether it is used or not -- so a seeded run
whose given tokens equal what it would have drawn is the same run."""
from __future__ import annotations

import torch

FREE = -1
# generate()'s default form for a prefix every row gives: one whole-sequence pass (True) or token by token through the sampler
# (DESIGN section 12 has the measurement that decides it)
PREFIX_FAST_PATH = True
_INT_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


def check_given(given, shape, vocab: int) -> torch.Tensor:
    """The caller's `given` as a contiguous int32 CPU tensor of `shape`, or ValueError: not an integer tensor, another shape, or an
    entry that is neither -1 nor a token id in [0, vocab).  Runs before anything is launched."""
    if not torch.is_tensor(given) or given.dtype not in _INT_DTYPES:
        raise ValueError("given must be an integer tensor (-1 = free, else a token id)")
    if tuple(given.shape) != tuple(shape):
        raise ValueError(f"given must be {list(shape)} (one entry per new token), got {list(given.shape)}")
    g = given.detach().to("cpu", torch.int64)
    if g.numel() and (int(g.min()) < FREE or int(g.max()) >= int(vocab)):
        raise ValueError(f"given entries must be -1 (free) or token ids in [0, {int(vocab)})")
    return g.to(torch.int32).contiguous()


def given_prefix_length(given: torch.Tensor) -> int:
    """P: the largest value <= N - 1 such that columns 0 .. P-1 of `given` [B, N] are given in EVERY row -- what one
    whole-sequence pass can feed instead of P decode steps.  Capped at N - 1: the pass leaves the logits of token P, so one token
    always goes through the sampler (as a given one when the rows are given throughout)."""
    B, N = given.shape
    if B == 0 or N == 0:
        return 0
    free = (given < 0).any(dim=0)
    first = int(torch.nonzero(free)[0]) if bool(free.any()) else N
    return min(first, N - 1)


def keep_to_given(indices: torch.Tensor, keep, grid) -> torch.Tensor:
    """given [B, h*w] from token ids `indices` [B, h*w]: kept positions carry their id, the rest is free.  keep: a row count (the
    top `keep` rows of the h x w token grid) or a bool [h, w] mask over it."""
    h, w = int(grid[0]), int(grid[1])
    if indices.dim() != 2 or indices.shape[1] != h * w:
        raise ValueError(f"indices must be [B, {h * w}] for a {h} x {w} token grid")
    if torch.is_tensor(keep):
        if keep.dtype != torch.bool or tuple(keep.shape) != (h, w):
            raise ValueError(f"keep must be a row count or a bool [{h}, {w}] mask over the token grid")
        mask = keep.reshape(-1)
    else:
        if isinstance(keep, bool) or int(keep) != keep or not 0 <= int(keep) <= h:
            raise ValueError(f"keep rows must be an integer in [0, {h}]")
        mask = torch.zeros(h, w, dtype=torch.bool)
        mask[: int(keep)] = True
        mask = mask.reshape(-1)
    mask = mask.to(indices.device)
    return torch.where(mask[None, :], indices.to(torch.int32), torch.full_like(indices, FREE, dtype=torch.int32))


@torch.no_grad()
def complete(gpt, vq, images, cond, keep, **generate_kwargs):
    """Continue pictures from a kept part: images fp32 [B, 3, H, W] in [-1, 1] -> vq.encode -> token ids [B, h*w] -> `given` (free
    where not kept) -> generate(gpt, cond, h*w, given=...) -> vq.decode_code.  keep: a row count of the token grid (the top rows
    stay) or a bool [h, w] mask.  Returns (images fp32 [B, 3, H, W], ids int32 [B, h*w]); generate_kwargs are generate()'s."""
    from .generate import generate
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError("images must be [B, 3, H, W]")
    B = images.shape[0]
    quant, _, (_, _, indices) = vq.encode(images)
    h, w = int(quant.shape[2]), int(quant.shape[3])
    given = keep_to_given(indices.view(B, h * w), keep, (h, w))
    out = generate(gpt, cond, h * w, given=given, **generate_kwargs)
    if isinstance(out, tuple):
        raise ValueError("complete() returns images and ids: ask generate() itself for log-probabilities")
    return vq.decode_code(out, [B, int(quant.shape[1]), h, w]), out
