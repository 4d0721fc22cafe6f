"""The container algorithm of the ragged hybrid front end (csrc/conv.h: the RAGGED forms), restated in torch on top of oracle/cpu_ref.py.
Dtype-generic like cpu_ref: float64 in, float64 throughout.  It holds no tests (tests/test_hybrid_ragged_cpu.py runs it against cpu_ref on
every image alone).

B images of different sizes sit in the top-left corners of the slots of ONE tensor [B][C][Hc/s][Wc/s] at every resolution s.  What the
engine's kernels do, and what is restated here:
- a convolution or pool tap outside image b's own extent (H_b/s x W_b/s) is zero (pool: absent), whatever the slot holds there;
- the low-side SAME offset of every layer is ONE number for the whole batch (LOW_PAD), because every image side is a multiple of 16;
- GroupNorm sums and counts over the extent only;
- the 1x1 projection runs over the container's token grid and image b's own h_b x w_b part of it is packed to rows 1 .. n_b-1 of its
  slot, with position ids from the canvas grid; rows n_b .. Ns-1 are zeros.
To show that nothing outside an extent reaches a kept value, every layer's output is overwritten with NaN outside the extents before the
next layer sees it."""
import math

import torch
import torch.nn.functional as F

from oracle import cpu_ref

# low-side SAME offset of (kernel, stride) on a side that is a multiple of 16 / 8 / 4 / 2 as it meets them in the backbone
LOW_PAD = {(7, 2): 2, (3, 2): 0, (3, 1): 1, (1, 2): 0, (1, 1): 0}
POOL_LOW_PAD = 0


def same_pad_low(side, k, stride):
    """Engine::same_pad (csrc/engine.hip), utils.py:97-99,112-123: the low-side pad of TF "SAME" """
    out = (side + stride - 1) // stride
    return max((out - 1) * stride + (k - 1) + 1 - side, 0) // 2


def _mask(x, ext, fill):
    """x [B][C][h][w] with everything outside image b's extent ext[b] = (h_b, w_b) replaced by `fill` (NaN there included)"""
    B, _, h, w = x.shape
    rows, cols = torch.arange(h)[None, :, None], torch.arange(w)[None, None, :]
    eh, ew = torch.tensor([e[0] for e in ext])[:, None, None], torch.tensor([e[1] for e in ext])[:, None, None]
    inside = ((rows < eh) & (cols < ew))[:, None]
    return torch.where(inside, x, torch.full((), fill, dtype=x.dtype))


def _poison(x, ext):
    return _mask(x, ext, float("nan"))


def _conv(x, w, stride, ext):
    """masked taps; out [B][OC][ceil(h/s)][ceil(w/s)] over the container grid"""
    k = w.shape[-1]
    ws = F.batch_norm(w.reshape(1, w.shape[0], -1), None, None, training=True, momentum=0.0, eps=1e-6).reshape_as(w)   # cpu_ref.std_conv
    lo = LOW_PAD[(k, stride)]
    h, wd = x.shape[-2:]
    oh, ow = -(-h // stride), -(-wd // stride)
    hi_h, hi_w = (oh - 1) * stride + k - lo - h, (ow - 1) * stride + k - lo - wd
    xp = F.pad(_mask(x, ext, 0.0), [lo, max(hi_w, 0), lo, max(hi_h, 0)])
    return F.conv2d(xp, ws, None, stride)[:, :, :oh, :ow]


def _group_norm(sd, p, x, ext, act, res=None):
    y = x.clone()
    for b, (eh, ew) in enumerate(ext):
        v = F.group_norm(x[b:b + 1, :, :eh, :ew], 32, sd[f"{p}.weight"], sd[f"{p}.bias"], 1e-5)
        if res is not None:
            v = v + res[b:b + 1, :, :eh, :ew]
        y[b:b + 1, :, :eh, :ew] = F.relu(v) if act else v
    return _poison(y, ext)


def _scaled(ext, num, den):
    return [(e[0] * num // den, e[1] * num // den) for e in ext]


def container_backbone(sd, box, sizes):
    """box [B][1][Hc][Wc] (anything outside the corners), sizes [(H_b, W_b)] -> features [B][1024][Hc/16][Wc/16], NaN outside the extents"""
    p = "encoder.patch_embed.backbone_net"
    e1 = list(sizes)
    x = _poison(_conv(box, sd[f"{p}.stem.0.weight"], 2, e1), _scaled(e1, 1, 2))
    e2 = _scaled(e1, 1, 2)
    x = _group_norm(sd, f"{p}.stem.1", x, e2, True)
    h, w = x.shape[-2:]
    oh, ow = -(-h // 2), -(-w // 2)
    xp = F.pad(_mask(x, e2, -float("inf")), [POOL_LOW_PAD, 2 * ow + 1 - w, POOL_LOW_PAD, 2 * oh + 1 - h], value=-float("inf"))
    ext = _scaled(e1, 1, 4)
    x = _poison(F.max_pool2d(xp, 3, 2)[:, :, :oh, :ow], ext)
    for st, depth in enumerate((2, 4, 6)):
        for i in range(depth):
            b = f"{p}.stages.{st}.stage_blocks.{i}"
            stride = 2 if (i == 0 and st > 0) else 1
            out = _scaled(ext, 1, stride)
            res = x
            if f"{b}.downsample.conv.weight" in sd:
                res = _group_norm(sd, f"{b}.downsample.norm", _conv(x, sd[f"{b}.downsample.conv.weight"], stride, ext), out, False)
            y = _group_norm(sd, f"{b}.block_list.1", _conv(x, sd[f"{b}.block_list.0.weight"], 1, ext), ext, True)
            y = _group_norm(sd, f"{b}.block_list.3", _conv(y, sd[f"{b}.block_list.2.weight"], stride, ext), out, True)
            x = _group_norm(sd, f"{b}.block_list.5", _conv(y, sd[f"{b}.block_list.4.weight"], 1, out), out, True, res=res)
            ext = out
    return x


def container_tokens(sd, box, sizes):
    """-> (tok [B][Ns-1][D] image b's h_b * w_b projected tokens packed to the front of slot b and zeros behind them, n_tokens [B])"""
    f = container_backbone(sd, box, sizes)
    f = F.conv2d(f, sd["encoder.patch_embed.proj.weight"], sd["encoder.patch_embed.proj.bias"])          # over the container's token grid
    grids = [(H // 16, W // 16) for H, W in sizes]
    ns = 1 + max(h * w for h, w in grids)
    tok = torch.zeros((len(sizes), ns - 1, f.shape[1]), dtype=f.dtype)
    for b, (h, w) in enumerate(grids):
        tok[b, :h * w] = f[b, :, :h, :w].flatten(1).t()
    return tok, [1 + h * w for h, w in grids]


def container_encode(sd, box, sizes, grid_w):
    """-> (enc [B][Ns][D] with zero rows behind n_b, n_tokens): the ViT behind the packed tokens runs on every image's own rows, with the
    position ids of grid[:h_b, :w_b] of the canvas grid grid_w wide (cpu_ref.encode's own tail)"""
    tok, ntok = container_tokens(sd, box, sizes)
    enc = torch.zeros((tok.shape[0], tok.shape[1] + 1, tok.shape[2]), dtype=tok.dtype)
    for b, (H, W) in enumerate(sizes):
        x = torch.cat([sd["encoder.cls_token"].expand(1, -1, -1), tok[b:b + 1, :ntok[b] - 1]], dim=1)
        x = x + sd["encoder.pos_embed"][:, cpu_ref.pos_ids(H // 16, W // 16, grid_w)]
        x = cpu_ref.stack(sd, "encoder.attn_layers", cpu_ref.kinds_of(sd, "encoder.attn_layers"), x, None, False, None)
        enc[b, :ntok[b]] = cpu_ref.layer_norm(x, sd["encoder.norm.weight"], sd["encoder.norm.bias"])[0]
    return enc, ntok


def pack(images, Hc, Wc, fill=float("nan")):
    """a list of (1, H_b, W_b) tensors -> ([B][1][Hc][Wc] with `fill` outside the corners, [(H_b, W_b)])"""
    box = torch.full((len(images), 1, Hc, Wc), fill, dtype=images[0].dtype)
    for b, im in enumerate(images):
        box[b, :, :im.shape[1], :im.shape[2]] = im
    return box, [(int(im.shape[1]), int(im.shape[2])) for im in images]
