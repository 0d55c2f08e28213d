#!/usr/bin/env python3
"""Class-conditional image completion on the MI355X-native engine: keep the top rows of given pictures, sample the rest.

    python examples/complete_c2i.py --vq-ckpt vq_ds16_c2i.pt --gpt-ckpt c2i_L_384.pt --gpt-model GPT-L --image-size 384 \
        --images photos.npz --labels 207,360 --keep-rows 12 --out completed.npz

Same checkpoint flags as examples/sample_c2i.py.  `--images` is an .npy / .npz file of uint8 [N, H, W, 3] (or one [H, W, 3]) images
of `--image-size` pixels; they are encoded to tokens by the VQ tokenizer, the top `--keep-rows` rows of the token grid are kept
(`llamagen_amd.complete`: given tokens, not drawn ones) and the rest is sampled.  The result is written as uint8 [N, H, W, 3]
`arr_0` (the layout of sample_c2i_ddp.py's .npz) next to the token ids `ids`; `main()` returns the tensors.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llamagen_amd import GPT_models, VQ_models, complete  # noqa: E402
from llamagen_amd.checkpoint import load_gpt_checkpoint, load_vq_checkpoint  # noqa: E402
from llamagen_amd.postprocess import to_uint8_hwc  # noqa: E402
from examples.sample_c2i import DEMO_LABELS, build_parser as _sample_parser  # noqa: E402


def build_parser():
    p = _sample_parser()
    p.description = "keep the top rows of given images, sample the rest"
    p.add_argument("--images", type=str, required=True, help=".npy / .npz of uint8 [N, H, W, 3] images (image-size pixels)")
    p.add_argument("--labels", type=str, default=None, help="comma-separated class ids, one per image (default: the demo's)")
    p.add_argument("--keep-rows", type=int, required=True, help="rows of the token grid (image-size / downsample-size of them) that stay")
    for act in p._actions:
        if act.dest == "out":
            act.help, act.default = "output .npz (uint8 images `arr_0`, token ids `ids`)", "completed.npz"
    return p


def load_images(path: str) -> torch.Tensor:
    """uint8 HWC file -> fp32 [N, 3, H, W] in [-1, 1] (the tokenizer's input range)."""
    arr = np.load(path)
    if not isinstance(arr, np.ndarray):   # .npz: the first array (`arr_0` of the sampling scripts)
        arr = arr[arr.files[0]]
    if arr.ndim == 3:
        arr = arr[None]
    if arr.ndim != 4 or arr.shape[-1] != 3 or arr.dtype != np.uint8:
        raise ValueError(f"{path}: expected uint8 [N, H, W, 3], got {arr.dtype} {arr.shape}")
    return torch.from_numpy(arr).permute(0, 3, 1, 2).float() / 127.5 - 1.0


def main(args):
    torch.manual_seed(args.seed)
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise RuntimeError("examples/complete_c2i.py needs an AMD GPU: llamagen_amd has no CPU path")
    device = "cuda"
    images = load_images(args.images)
    if images.shape[-1] != args.image_size or images.shape[-2] != args.image_size:
        raise ValueError(f"images are {images.shape[-2]} x {images.shape[-1]} pixels, --image-size is {args.image_size}")
    n = images.shape[0]
    labels = [int(x) for x in args.labels.split(",")] if args.labels else [DEMO_LABELS[i % len(DEMO_LABELS)] for i in range(n)]
    if len(labels) != n:
        raise ValueError(f"{n} images but {len(labels)} labels")

    vq_model = VQ_models[args.vq_model](codebook_size=args.codebook_size, codebook_embed_dim=args.codebook_embed_dim)
    vq_model.to(device).eval()
    load_vq_checkpoint(vq_model, args.vq_ckpt)
    precision = {"none": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[args.precision]
    latent_size = args.image_size // args.downsample_size
    gpt_model = GPT_models[args.gpt_model](vocab_size=args.codebook_size, block_size=latent_size ** 2, num_classes=args.num_classes,
                                           cls_token_num=args.cls_token_num, model_type=args.gpt_type).to(device=device, dtype=precision)
    load_gpt_checkpoint(gpt_model, args.gpt_ckpt, from_fsdp=args.from_fsdp)
    gpt_model.eval()
    if args.kv_cache_dtype != "auto":
        gpt_model.set_kv_cache(args.kv_cache_dtype)

    samples, ids = complete(gpt_model, vq_model, images.to(device), torch.tensor(labels, device=device), int(args.keep_rows),
                            cfg_scale=args.cfg_scale, cfg_interval=int(args.cfg_interval), temperature=args.temperature,
                            top_k=args.top_k, top_p=args.top_p, sample_logits=True)
    out = args.out if args.out.endswith(".npz") else args.out + ".npz"
    np.savez(out, arr_0=to_uint8_hwc(samples).cpu().numpy(), ids=ids.cpu().numpy())
    print(f"{n} images completed from their top {args.keep_rows} of {latent_size} token rows; saved to {out}")
    return dict(samples=samples, ids=ids, path=out)


if __name__ == "__main__":
    main(build_parser().parse_args())
