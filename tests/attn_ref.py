"""Float64 restatement of the decoder stack (Transformer.forward, reference model/decoder.py:41-67) that returns every attention
block's probabilities (`post_softmax_attn`, model/attention.py:166-178) -- the checker of tests/test_attn_cpu.py and
tests/test_gpu_attn.py.  It holds no tests.  Built from oracle.cpu_ref's blocks (layer_norm, _split_heads, ffn, kinds_of) and its key
layout, which tests/test_oracle_golden.py pins against the reference; the attention itself is restated here because cpu_ref.mha does
not return its softmax."""
import numpy as np
import torch

from oracle.cpu_ref import SCALE, _split_heads, ffn, kinds_of, layer_norm

PREFIX = "decoder.net.attn_layers"


def sd64(sd):
    """a reference-layout state dict (numpy or torch) as float64 torch tensors"""
    return {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items()}


def attention(sd, p, xq, src, causal, q_mask=None, k_mask=None):
    """MultiHeadAttention.forward (attention.py:101-180) -> (block output, probabilities (B, heads, nq, nk)).  Masks as cpu_ref.mha:
    energy is filled with -FLT_MAX where not (q_mask (x) k_mask), then where j > i + (nk - nq) if causal."""
    q = _split_heads(xq @ sd[f"{p}.q.weight"].t())
    k = _split_heads(src @ sd[f"{p}.k.weight"].t())
    v = _split_heads(src @ sd[f"{p}.v.weight"].t())
    energy = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    fill = -torch.finfo(torch.float32).max                          # the reference's mask value (float32 arithmetic there)
    B, _, nq, nk = energy.shape
    if q_mask is not None or k_mask is not None:
        qm = q_mask if q_mask is not None else torch.ones((B, nq), dtype=torch.bool)
        km = k_mask if k_mask is not None else torch.ones((B, nk), dtype=torch.bool)
        energy = energy.masked_fill(~(qm[:, None, :, None] & km[:, None, None, :]), fill)
    if causal:
        i, j = torch.arange(nq).view(nq, 1), torch.arange(nk).view(1, nk)
        energy = energy.masked_fill(j > i + (nk - nq), fill)
    attn = torch.softmax(energy, dim=-1)
    out = torch.matmul(attn, v).permute(0, 2, 1, 3).reshape(B, nq, -1)
    a, g = (out @ sd[f"{p}.fc_out.0.weight"].t() + sd[f"{p}.fc_out.0.bias"]).chunk(2, dim=-1)
    return a * torch.sigmoid(g), attn


@torch.no_grad()
def decoder_attn(sd, tokens, enc, mask=None):
    """-> (logits (B, t, V), maps): maps is the reference's list -- self 0, cross 0, self 1, cross 1, ... -- each (B, heads, t, keys),
    float64.  sd: float64 state dict (sd64); tokens (B, t) int64; enc (B, N, D); mask (B, t) bool or None (all True)."""
    enc = torch.as_tensor(enc).double()
    t = tokens.shape[1]
    x = sd["decoder.net.token_embedding.weight"][tokens] + sd["decoder.net.pos_embedding.embedding.weight"][:t][None]
    g, b = sd[f"{PREFIX}.layers.0.0.weight"], sd[f"{PREFIX}.layers.0.0.bias"]
    kinds = kinds_of(sd, PREFIX)
    maps = []
    for s, kind in enumerate(kinds):
        p = f"{PREFIX}.layers.{s}.1"
        z = layer_norm(x, g, b)
        if kind == "self":
            o, a = attention(sd, p, z, z, True, q_mask=mask, k_mask=mask)
            maps.append(a)
        elif kind == "cross":
            o, a = attention(sd, p, z, enc, False, q_mask=mask)
            maps.append(a)
        else:
            o = ffn(sd, p, z)
        x = o + x
        if s != len(kinds) - 1:
            x = layer_norm(x, g, b)
    x = layer_norm(x, sd["decoder.net.norm.weight"], sd["decoder.net.norm.bias"])
    return x @ sd["decoder.net.to_logits.weight"].t() + sd["decoder.net.to_logits.bias"], maps


def stacked(maps):
    """the list of decoder_attn as the engine's two buffers: (self (Ld, B, heads, t, t), cross (Ld, B, heads, t, N))"""
    return torch.stack(maps[0::2]), torch.stack(maps[1::2])


# ---- the cases tests/test_attn_cpu.py and tests/test_gpu_attn.py share (synthetic weights, random encoder rows and tokens) -----------
class Case:
    """d, sd (numpy state dict), enc (B, N, D) float32, x (B, t) int64, mask (B, t) bool or None, and the float64 answer: logits and
    maps (the reference's list).  The answer is computed once per case and never changed."""

    def __init__(self, d, weight_seed, B, N, t, seed, lengths=None, sharpen=1.0):
        """sharpen: factor on the q projection of the first self attention -- its scores spread by that much (see future_excess)"""
        from texocr_amd import synth
        self.d, self.sd = d, synth.synth_state_dict(d, weight_seed)
        self.sd[f"{PREFIX}.layers.0.1.q.weight"] = self.sd[f"{PREFIX}.layers.0.1.q.weight"] * np.float32(sharpen)
        g = torch.Generator().manual_seed(seed)
        self.enc = torch.randn((B, N, d.embed_dim), generator=g)
        ordinary = torch.tensor([v for v in range(d.vocab) if v not in (d.bos, d.eos, d.pad)])
        self.x = ordinary[torch.randint(0, len(ordinary), (B, t), generator=g)]
        self.x[:, 0] = d.bos
        self.mask = None
        if lengths:
            self.mask = torch.arange(t)[None, :] < torch.tensor(lengths)[:, None]
            self.x[~self.mask] = d.pad
        self.logits, self.maps = decoder_attn(sd64(self.sd), self.x, self.enc, self.mask)
        self.self64, self.cross64 = stacked(self.maps)

    def valid(self):
        """(B, t) bool: the queries that are not padding"""
        return torch.ones(self.x.shape, dtype=torch.bool) if self.mask is None else self.mask


_CASES = {}


def case(name, *args, **kw):
    """Case(*args, **kw), built once per name"""
    if name not in _CASES:
        _CASES[name] = Case(*args, **kw)
    return _CASES[name]


def layer_distance(stack64, valid):
    """the smallest max |difference| between the float64 maps of two different layers (stack64 (Ld, B, heads, t, keys)), over the
    queries that are not padding: what a bound on |map - reference| must stay below to tell the layers apart"""
    sel = stack64.permute(0, 2, 4, 1, 3)[..., valid]              # (Ld, heads, keys, valid queries)
    Ld = stack64.shape[0]
    return min(float((sel[a] - sel[b]).abs().max()) for a in range(Ld) for b in range(Ld) if a != b)


def future_excess(c):
    """float64, first self attention of case c: the largest amount by which the score of a key BEHIND a query exceeds the best score
    among the keys the query may see.  Beyond ~104 (exp underflows in float32) a softmax whose maximum is taken over the future keys
    too loses every valid key of that row: the case then tells a causal limit missing from the maximum apart from a correct one,
    which plain arithmetic cannot (a softmax does not depend on its reference point)."""
    sd = sd64(c.sd)
    t = c.x.shape[1]
    x = sd["decoder.net.token_embedding.weight"][c.x] + sd["decoder.net.pos_embedding.embedding.weight"][:t][None]
    z = layer_norm(x, sd[f"{PREFIX}.layers.0.0.weight"], sd[f"{PREFIX}.layers.0.0.bias"])
    p = f"{PREFIX}.layers.0.1"
    S = torch.matmul(_split_heads(z @ sd[f"{p}.q.weight"].t()), _split_heads(z @ sd[f"{p}.k.weight"].t()).transpose(-1, -2)) * SCALE
    i, j = torch.arange(t).view(t, 1), torch.arange(t).view(1, t)
    return float((S.masked_fill(j <= i, -1e9).amax(-1) - S.masked_fill(j > i, -1e9).amax(-1))[..., :-1].max())


def small_dims(D, heads, max_len, canvas=128, canvas_w=0, vocab=200):
    from texocr_amd.config import Dims
    return Dims(canvas=canvas, canvas_w=canvas_w, in_channels=3, embed_dim=D, enc_heads=1, enc_layers=1, dec_heads=heads, dec_layers=2,
                enc_exp=1, dec_exp=1, vocab=vocab, max_len=max_len, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1)


WIDE = small_dims(64, 2, 130, canvas=224, canvas_w=672)              # 224 x 672: 589 encoder rows, one encoder layer
# (dims, weight seed, B, N, t, seed, lengths, sharpen): first-layer self scores spread over +-250, see future_excess
SHARP_CASE = (small_dims(64, 1, 130), 3, 2, 7, 130, 77, None, 60.0)


def _bf16_cases():
    from gpu_harness import SHAPE_CASES
    # name: (dims, weight seed, B, N, t, seed, lengths)
    return {"b_calib256": (SHAPE_CASES["calib256"][0], 11, 2, 65, 32, 51, None),
            "b_calib768": (SHAPE_CASES["calib768"][0], 12, 2, 65, 32, 52, None),
            "b_h20": (SHAPE_CASES["w768_h20"][0], 13, 2, 65, 32, 53, None),
            "b_n589": (WIDE, 14, 2, 589, 129, 54, [129, 70])}


BF16_CASES = _bf16_cases()
# bf16 engine against float64, max |p - reference| over the self, cross and head-mean maps of BF16_CASES, measured on MI355X, 2026-10-19
# (per case: calib256 0.00553, calib768 0.00492, 20 heads 0.00532, N = 589 0.00433); the tests assert twice the measured value
BF16_MEASURED = 0.00553
BF16_BOUND = 2 * BF16_MEASURED
