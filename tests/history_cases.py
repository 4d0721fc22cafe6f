"""The single-position decode where the SELF-attention history ends its slots and passes: the cases tests/test_gpu_self_history.py runs,
a pure-Python restatement of the arithmetic they are chosen for (tests/test_history_cases_cpu.py proves from it that the checkpoints
reach every seam they are listed for), and the float64 references (computed once, never modified; it holds no tests, imported like
gpu_harness and decode_cases).

The restatements follow the headers line by line and cite them; where a header and this file disagree the header is right and the
case has to move.

Forms of the self attention outside beam search (csrc/dec_attn.h, launch_dec_attn in csrc/engine.hip):
  plain       EPI_QKV appends key t, then dec_attn_tile<ATT_SELF, APRO_NONE> over L = t + 1 cached keys (the default);
  fused       TXO_SELF_FUSED=1: APRO_EMBED / APRO_LN2, L = t cached keys, key t scored apart (m_run starts at s_new);
  masked      KMASK: the plain form with a key mask, index min(key, lmax - 1);
  persistent  the persistent kernel's HIST_EARLY form: keys 0 .. t - 1 requested before the hand-off wait, key t spliced in by selects;
  latent      TXO_LATENT_SELF=1: lat_core_tile over the z history (csrc/lat_attn.h), L = t + 1.
Groups: A launch forms through TXO_NET_STEPWISE, B the persistent launch, C the latent self attention, D the multi-position pass and a
step behind it, E a compaction of two-pass histories (stop='row')."""
import dataclasses

import torch

import decode_cases as dc
import ref64
from gpu_harness import SHAPE_CASES, STOP_DIMS, first_eos, rgb_images
from texocr_amd import synth

T_HIST = 520                                      # positional table of the K/V cases: three passes and seven keys
T_LAT = 300                                       # table of the latent self attention (<= 512: eight waves) and of the compaction case
CHECKPOINTS = (0, 1, 15, 16, 17, 31, 32, 33, 254, 255, 256, 257, 258, 511, 512, 513, 519)
PROBE_P = (0, 15, 16, 31, 32, 255, 256, 257, 511, 512, 518)      # history positions whose token the one-key probe replaces
KV_FORMS = ("plain", "fused", "masked", "persistent")
FORMS = KV_FORMS + ("latent",)

# ---- csrc/dec_attn.h: dec_attn_tile, self attention ---------------------------------------------------------------------------------
NLS = {"fp32": 16, "bf16": 8}                     # engine.hip:1438 (launch_dec_attn), persist.h:360: wave instructions per pass


def kpb(dtype):
    """keys per block-instruction = keys per skipped slot (dec_attn.h:133-135)"""
    return dc.keys_per_pass(dtype) // dc.DA_NL_CROSS


def keys_per_pass(dtype):
    return NLS[dtype] * kpb(dtype)                # dec_attn.h:426: NL * KPB


def hist_len(form, t):
    """L: cached keys the passes run over (dec_attn.h:182: fused self handles the new key apart)"""
    return t if form == "fused" else t + 1


def new_key(form, t):
    """how key t reaches the softmax: from the cache like every other, scored apart (dec_attn.h:346, :356, :449), or spliced into the
    early history by selects (dec_attn.h:221-232, :373-377, :411-415; nothing is early at t = 0)"""
    return {"fused": "apart", "persistent": "spliced"}.get(form, "cache")


@dataclasses.dataclass(frozen=True)
class Pass:
    base: int
    slot: int                                     # LDS statistics slot (stat[slot * 4 + wave])
    nslot: int                                    # key slots not skipped
    last_fill: int                                # keys of the last slot that is not skipped


def passes(dtype, form, t):
    """do_pass(0, 0), then base = NL * KPB, .. < L with slot = 1, slot ^= 1 (dec_attn.h:423-429); nslot = (L - base + KPB - 1) / KPB
    (dec_attn.h:367), of which at most NL exist"""
    L, k, nl = hist_len(form, t), kpb(dtype), NLS[dtype]
    out, slot = [], 0
    for i, base in enumerate([0] + list(range(nl * k, L, nl * k))):
        slot = 0 if i == 0 else (1 if i == 1 else slot ^ 1)
        ns = min((L - base + k - 1) // k, nl)
        keys = min(L - base, nl * k)
        out.append(Pass(base, slot, ns, keys - (ns - 1) * k if ns else 0))
    return out


def idle_barriers(dtype, form, t):
    """dec_attn_idle (dec_attn.h:464-472) for APRO_NONE: first pass, one per later pass, partial outputs; the tile's own count is one per
    do_pass (dec_attn.h:397) and one before the reduction (:444)"""
    L, kpp = t + 1, keys_per_pass(dtype)
    return 1 + len(range(kpp, L, kpp)) + 1, len(passes(dtype, form, t)) + 1


# ---- csrc/persist.h: how the persistent launch deals the (row, head) pairs of an attention stage ----------------------------------------
PS_TEAMS, PS_TEAM_BLOCKS = 8, 32                  # persist.h:54


def persist_attn_rounds(rows, heads):
    """per team with rows: (rows of the team, 16-row tiles, [(pairs with a tile, idle groups) per round of the attention stage]).
    persist.h:209-214: rpt = ceil(B / 8) rows per team, nrt 16-row tiles; PS_ATTN (persist.h:311-332): np = nr * heads pairs over
    NSB = 64 groups (two per workgroup, sa = grp * 32 + rank) per round; a workgroup takes part in a round iff base + rank < np, and
    its group without a pair (base + sa >= np) runs dec_attn_idle"""
    rpt = -(-rows // PS_TEAMS)
    out = []
    for team in range(PS_TEAMS):
        nr = max(0, min(rows - team * rpt, rpt))
        if nr == 0:
            continue
        np_, rounds = nr * heads, []
        for base in range(0, np_, 2 * PS_TEAM_BLOCKS):
            busy = idle = 0
            for rank in range(PS_TEAM_BLOCKS):
                if base + rank < np_:
                    for grp in (0, 1):
                        if base + grp * PS_TEAM_BLOCKS + rank < np_:
                            busy += 1
                        else:
                            idle += 1
            rounds.append((busy, idle))
        out.append((nr, -(-nr // dc.DG_BM), rounds))
    return out


def lat_self_shape(t, width, dtype):
    """the latent self attention of position t: lat_core_tile over t + 1 rows of the z history (engine.hip:1566)"""
    return dc.lat_shape(t + 1, width, dtype)


LA_PATH_TILES = 4                                 # lat_attn.h:46


def lat_self_ok(d, dtype, table):
    """engine.hip:213-217 with TXO_LATENT_SELF=1 and TXO_LATENT=1: the fold exists (heads * 64 == 2 D, engine.hip:426, :1487) and the
    table fits 16 keys x waves x LA_PATH_TILES"""
    D = d.embed_dim
    return dc.latent_ok(D, dtype) and d.dec_heads * dc.DH == 2 * D and table <= 16 * dc.lat_waves(D, dtype) * LA_PATH_TILES


# ---- models: calib256 (the persistent launch is its default) and a 64-wide one with 2 heads, on the 64 x 64 canvas --------------------
def _dims(base, max_len, dec_layers=2, **over):
    return dataclasses.replace(SHAPE_CASES[base][0], canvas=64, max_len=max_len, dec_layers=dec_layers, **over)


DIMS = {}
for _n, _b, _o in (("calib256", "calib256", {}), ("w64_h2", "w64_h4", dict(enc_heads=2, dec_heads=2))):
    DIMS[_n] = _dims(_b, T_HIST, **_o)
    DIMS[_n + "_1l"] = _dims(_b, T_HIST, dec_layers=1, **_o)           # one decoder layer: the one-key probe
    DIMS[_n + "_t300"] = _dims(_b, T_LAT, **_o)
    DIMS[_n + "_own"] = DIMS[_n]                                       # the own-key model (weights() below)
WIDTHS = ("calib256", "w64_h2")
IMG = (64, 64)
IMAGE_SEED = 3520
FIVE = (0, 1, 0, 1, 1)                            # two distinct images over five slots
ROWS128 = tuple(i % 2 for i in range(128))        # the persistent launch at 128 bf16 rows: 16 rows per team, two full attention rounds per group
ROWS72 = tuple(i % 2 for i in range(72))          # ... at 72: 9 rows per team, a second attention round of 8 pairs beside 8 idle groups
ROWS136 = tuple(i % 2 for i in range(136))        # fp32 alone goes past 128 rows: 17 rows per team, TWO 16-row tiles, three attention rounds

_SD, _REF, _PROBE, _MASKED = {}, {}, {}, {}
SELF_PREFIX = "decoder.net.attn_layers.layers."    # layers 3 l: self attention, 3 l + 1: cross attention, 3 l + 2: feed-forward
OWN_T = (256, 512)                                # positions at which the last pass holds key t alone (plain / masked / persistent)
OWN_FLOOR = 0.15                                  # float64 max_v |dlogit| of dropping key t there: > 2 x the bf16 bound of 0.0557


def weights(name):
    """dims name -> (dims, synth state dict, float64 state dict)"""
    if name not in _SD:
        d = DIMS[name]
        sd = synth.synth_state_dict(d, 3)
        if name.endswith("_own"):
            # every self attention's k projection is its q projection: a query scores its OWN key |q|^2 / 8, at least a tenth of the
            # softmax at every position -- on the plain, masked and persistent forms key t is the one key of the last pass at t = 256 / 512
            for k in [k for k in sd if k.endswith(".1.k.weight") and k.startswith(SELF_PREFIX) and int(k.split(".")[4]) % 3 == 0]:
                sd[k] = sd[k.replace(".k.weight", ".q.weight")].copy()
        _SD[name] = (d, sd, ref64.sd64(sd))
    return _SD[name]


@dataclasses.dataclass(frozen=True)
class Ref:
    img: torch.Tensor                             # (2, 3, 64, 64)
    enc: torch.Tensor                             # float64 encoder rows
    toks: torch.Tensor                            # (2, table) the oracle's greedy tokens
    logits: torch.Tensor                          # (2, table, V) float64
    prefix: torch.Tensor                          # (2, table): bos, then the oracle's tokens: its own teacher-forced input

    @property
    def margin(self):
        return float(ref64.margins(self.logits).min())


def reference(name):
    """the two images and their float64 greedy decode over the whole table (eos never stops it); never modified"""
    if name not in _REF:
        d, _, s64 = weights(name)
        img = rgb_images(2, *IMG, IMAGE_SEED)
        enc = ref64.encode(s64, img, grid_w=d.grid)
        toks, lg = ref64.generate(s64, enc, d.bos, None, d.max_len)
        _REF[name] = Ref(img, enc, toks, lg, torch.cat([torch.full((2, 1), d.bos, dtype=torch.long), toks[:, :-1]], 1))
    return _REF[name]


def feedback(name, toks):
    """float64 logits of the given sequences (2, n) of the two images fed back: position i from bos and toks[:, :i]"""
    d, _, s64 = weights(name)
    x = torch.cat([torch.full((2, 1), d.bos, dtype=torch.long), toks.cpu()[:, :-1]], 1)
    return ref64.decoder_net(s64, x, reference(name).enc)


def without_own_key(sd, tokens, enc, drop):
    """float64 logits (B, t, V) of the decoder stack (tests/attn_ref.py: decoder_attn) in which the queries at the positions `drop` do
    not see their OWN key in any self attention: what a kernel computes that loses the single key of its last pass"""
    import attn_ref
    from oracle.cpu_ref import SCALE, _split_heads, ffn, kinds_of, layer_norm
    P = attn_ref.PREFIX
    t = tokens.shape[1]
    x = sd["decoder.net.token_embedding.weight"][tokens] + sd["decoder.net.pos_embedding.embedding.weight"][:t][None]
    g, b = sd[f"{P}.layers.0.0.weight"], sd[f"{P}.layers.0.0.bias"]
    kinds = kinds_of(sd, P)
    i, j = torch.arange(t).view(t, 1), torch.arange(t).view(1, t)
    for s, kind in enumerate(kinds):
        p = f"{P}.layers.{s}.1"
        z = layer_norm(x, g, b)
        if kind in ("self", "cross"):
            src = z if kind == "self" else enc
            q, k, v = (_split_heads(y @ sd[f"{p}.{w}.weight"].t()) for y, w in ((z, "q"), (src, "k"), (src, "v")))
            e = torch.matmul(q, k.transpose(-1, -2)) * SCALE
            if kind == "self":
                e = e.masked_fill(j > i, -3.0e38)
                for d in drop:
                    e[:, :, d, d] = -3.0e38
            out = torch.matmul(torch.softmax(e, -1), v).permute(0, 2, 1, 3).reshape(x.shape[0], t, -1)
            a, gate = (out @ sd[f"{p}.fc_out.0.weight"].t() + sd[f"{p}.fc_out.0.bias"]).chunk(2, dim=-1)
            o = a * torch.sigmoid(gate)
        else:
            o = ffn(sd, p, z)
        x = o + x
        if s != len(kinds) - 1:
            x = layer_norm(x, g, b)
    x = layer_norm(x, sd["decoder.net.norm.weight"], sd["decoder.net.norm.bias"])
    return x @ sd["decoder.net.to_logits.weight"].t() + sd["decoder.net.to_logits.bias"]


def own_key_effect(name, toks):
    """per position of OWN_T: the smallest (over the two images) max_v |dlogit| in float64 between the decoder on the sequences toks (2, n)
    and the decoder that drops key t at position t"""
    d, _, s64 = weights(name)
    x = torch.cat([torch.full((2, 1), d.bos, dtype=torch.long), toks.cpu()[:, :-1]], 1)
    enc = reference(name).enc
    diff = (without_own_key(s64, x, enc, ()) - without_own_key(s64, x, enc, OWN_T)).abs().amax(-1)
    return {t: float(diff[:, t].min()) for t in OWN_T}


# ---- the one-key probe (one decoder layer: the token at p reaches the logits of t > p through key / value p alone) ---------------------
# model -> replacement token per PROBE_P, chosen on the oracle (per image) so that max_v |dlogit| >= PROBE_FLOOR at every (image, t >= p)
# (tests/test_history_cases_cpu.py proves the floor)
PROBE_FLOOR = 1e-3
PROBE_TOKEN = {                                   # per p: the replacement in image 0's and in image 1's prefix
    "calib256_1l": {0: (275, 150), 15: (800, 475), 16: (925, 750), 31: (250, 250), 32: (175, 475), 255: (450, 400), 256: (525, 900),
                    257: (775, 175), 511: (675, 950), 512: (875, 125), 518: (50, 50)},           # floors 0.0030 (p = 256) .. 0.0119
    "w64_h2_1l": {0: (46, 149), 15: (24, 102), 16: (121, 77), 31: (184, 192), 32: (125, 162), 255: (2, 125), 256: (45, 93),
                  257: (125, 183), 511: (145, 49), 512: (23, 54), 518: (49, 115)},               # floors 0.00103 (p = 15) .. 0.0088
}


def probe(name):
    """-> (base float64 logits (2, T, V), {p: (prefix with the token at p replaced, float64 logits of it)})"""
    if name not in _PROBE:
        _, _, s64 = weights(name)
        ref = reference(name)
        base = ref64.decoder_net(s64, ref.prefix, ref.enc)
        out = {}
        for p in PROBE_P:
            x = ref.prefix.clone()
            new = torch.tensor(PROBE_TOKEN[name][p])
            assert not bool((x[:, p] == new).any())
            x[:, p] = new
            out[p] = (x, ref64.decoder_net(s64, x, ref.enc))
        _PROBE[name] = (base, out)
    return _PROBE[name]


# ---- key masks (tests/attn_ref.py is the float64 reference): False = never attended by a later query ---------------------------------
MASKED_P = (0, 255, 256, 511)
LEFT_PAD = 40


def key_masks():
    """name -> (T_HIST,) bool"""
    holes = torch.ones(T_HIST, dtype=torch.bool)
    holes[list(MASKED_P)] = False
    pad = torch.ones(T_HIST, dtype=torch.bool)
    pad[:LEFT_PAD] = False
    return {"holes": holes, "left_pad": pad}


def masked_reference(name, which):
    """float64 logits (2, T, V) of the oracle's prefix under the key mask (attn_ref.decoder_attn); positions that are masked themselves
    are unspecified in the engine and never compared"""
    if (name, which) not in _MASKED:
        import attn_ref
        _, _, s64 = weights(name)
        ref = reference(name)
        m = key_masks()[which][None].expand(2, -1)
        _MASKED[(name, which)] = attn_ref.decoder_attn(s64, ref.prefix, ref.enc, m)[0]
    return _MASKED[(name, which)]


# ---- E: stop='row' over a table of 300, rows finishing on both sides of position 256 -------------------------------------------------
STOP_ROWS = 40
STOP_BIAS = 0.6                                   # eos logit bias, tuned on the oracle (test_history_cases_cpu.py proves the schedule)
STOP_DIMS_LONG = dataclasses.replace(STOP_DIMS, max_len=T_LAT)
STOP_EVERY, STOP_GAIN, POLL_AHEAD = 2, 1, 4       # gpu_harness.STOP_ENV; lanes.h:171 (DonePoll::AHEAD)
_STOP = {}


def stop_case():
    """like gpu_harness.stop_case on the long table -> (dims, state dict, images, the oracle's stop='row' tokens, its float64 logits
    (every row decoded on to the end), every row's first eos or -1)"""
    if not _STOP:
        d = STOP_DIMS_LONG
        sd = synth.synth_state_dict(d, 7)
        b = sd["decoder.net.to_logits.bias"].copy()
        b[d.eos] += STOP_BIAS
        sd["decoder.net.to_logits.bias"] = b
        img = torch.from_numpy(synth.synth_images(STOP_ROWS, 3, 32, 48, seed=11)) * torch.linspace(0.2, 3.0, STOP_ROWS)[:, None, None, None]
        s64 = ref64.sd64(sd)
        want, lg = ref64.generate(s64, ref64.encode(s64, img, grid_w=d.grid), d.bos, d.eos, d.max_len, stop="row", pad=d.pad)
        _STOP["case"] = (d, sd, img, want, lg, first_eos(want.numpy(), d.eos))
    return _STOP["case"]


def compactions(first_eos, n_pos, rows=STOP_ROWS, every=STOP_EVERY, gain=STOP_GAIN, ahead=POLL_AHEAD):
    """engine.hip:2257-2281 with eager launches (TXO_STOP_GRAPH=0: any row count), one range: the finished-row count is requested behind
    position t where (t + 1) % every == 0 and t + 1 + AHEAD < n_pos, and read AHEAD positions later; the range then shrinks to its live
    rows if that frees `gain` rows.  -> [(positions decoded t1, rows before, rows after, live rows that sat behind a finished slot)]:
    compact_lane moves positions 0 .. t1 - 1 of every moved row's history."""
    slots = list(range(rows))                     # batch row of every slot (None: a filler); live rows keep their order (step.h:443)
    alive = lambda r, at: r is not None and not 0 <= first_eos[r] <= at
    out, pend, t = [], -1, 0
    while t < n_pos:
        if pend >= 0 and t == pend + ahead:
            live = [r for r in slots if alive(r, t)]                               # the scan runs behind position t
            bound = sum(alive(r, pend) for r in slots)                             # the host's bound: the count of the request
            if bound >= 1 and len(slots) - bound >= gain:
                moved = sum(1 for i, r in enumerate(slots) if alive(r, t) and any(not alive(s, t) for s in slots[:i]))
                out.append((t + 1, len(slots), bound, moved))
                slots = live + [None] * (bound - len(live))
            pend = -1
        if pend < 0 and (t + 1) % every == 0 and t + 1 + ahead < n_pos:
            pend = t
        t += 1
    return out
