"""A float64 run of the CPU oracle (oracle/cpu_ref.py): the high-precision reference the shape-matrix tests compare the HIP kernels with.

cpu_ref is dtype-generic: given float64 weights and images every matmul, softmax and LayerNorm runs in float64 (token ids stay int64).
Nothing here changes cpu_ref's default (fp32) behaviour, which the golden-fixture tests pin bit for bit."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from oracle import cpu_ref


def sd64(sd_np) -> dict:
    """synth state dict (numpy fp32, aliased LN keys) -> torch float64 (aliases kept: one tensor per canonical array)"""
    seen, out = {}, {}
    for k, v in sd_np.items():
        if id(v) not in seen:
            t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
            seen[id(v)] = t.double()
        out[k] = seen[id(v)]
    return out


def img64(img: torch.Tensor) -> torch.Tensor:
    return img.detach().cpu().double()


@torch.no_grad()
def encode(sd, img: torch.Tensor, grid_w: Optional[int] = None, backbone_q=None) -> torch.Tensor:
    """backbone_q: a rounding applied wherever the hybrid backbone stores (cpu_ref.resnet_backbone); it has to keep the dtype it is given"""
    return cpu_ref.encode(sd, img64(img), grid_w=grid_w, backbone_q=backbone_q)


@torch.no_grad()
def decoder_net(sd, tokens: torch.Tensor, enc: torch.Tensor) -> torch.Tensor:
    return cpu_ref.decoder_net(sd, tokens.cpu(), enc.double())


@torch.no_grad()
def generate(sd, enc: torch.Tensor, bos: int, eos: Optional[int], max_len: int, stop: str = "global", pad: int = 0):
    """greedy: (tokens (B, n) int64, step logits (B, n, V) float64)"""
    return cpu_ref.generate_cached(sd, None, bos, eos, max_len, collect_logits=True, enc=enc.double(), stop=stop, pad=pad)


@torch.no_grad()
def beam_search(sd, enc: torch.Tensor, bos: int, eos: Optional[int], max_len: int, k: int):
    return cpu_ref.beam_search_cached(sd, enc.double(), bos, eos, max_len, k)


def margins(logits: torch.Tensor) -> torch.Tensor:
    """top-1 minus top-2 logit per (row, step): where the argmax is decided by less than a kernel's rounding, tokens may differ"""
    top2 = logits.topk(2, dim=-1).values
    return top2[..., 0] - top2[..., 1]
