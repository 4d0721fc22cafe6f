"""The single-position decode where its passes, tiles and forms switch: the cases tests/test_gpu_decode_edges.py runs, a pure-Python
restatement of the dispatch arithmetic they are chosen for (tests/test_decode_cases_cpu.py proves from it that every case reaches the
branch it is listed for), and the float64 reference of every distinct image (computed once, shared by both modules; it holds no tests,
imported like gpu_harness).

The restatements follow the headers line by line and cite them; where a header and this file disagree the header is right and the
case has to move.

A. cross attention on the projected K/V panels (csrc/dec_attn.h, ATT_CROSS): key counts on and beside the register-pass boundaries;
B. the same kernel with a key count per row (dec_attn_ragged_kernel): one ragged batch per storage type whose rows take 1, 1, 2 and 3 passes;
C. cross attention in latent form (csrc/lat_attn.h, lat_core_tile): key counts on and beside the rounds of 16-key tiles over the waves;
D. the row counts at which generate() changes the launch, the form, the range count and the projection blocks (csrc/engine.hip).
A-C: one encoder layer, two decoder layers on a 256 x 2032 canvas, engines with max_tokens = the largest N of the case.  A batch is a few
DISTINCT images placed at several slots (`slots`: the distinct image of each batch row)."""
import dataclasses

import torch

import ref64
from gpu_harness import SHAPE_CASES, rgb_images
from texocr_amd import synth

STEPS = 8                                         # decode positions: every position reads the whole cross panel

# ---- csrc/dec_attn.h: dec_attn_tile, cross attention -----------------------------------------------------------------------------
DA_NL_CROSS = 10                                  # dec_attn.h:112 (TXO_NL_CROSS)
DH = 64                                           # common.h:16
PER16 = {"fp32": 4, "bf16": 8}                    # common.h:27 / :33: elements per 16 bytes


def keys_per_pass(dtype):
    lpr = DH // PER16[dtype]                      # dec_attn.h:133: lanes per 64-element row
    kpi = 64 // lpr                               # dec_attn.h:134: keys per wave-instruction
    kpb = kpi * 4                                 # dec_attn.h:135: keys per block-instruction (four waves)
    return DA_NL_CROSS * kpb                      # dec_attn.h:211 / :426: NL * KPB keys are held per pass


def passes(n, dtype):
    """(pass count, keys of the last pass): do_pass(0, 0), then one pass per base = NL * KPB, 2 * NL * KPB, .. < L (dec_attn.h:423-429);
    a key is attended iff key < L (dec_attn.h:387)"""
    kpp = keys_per_pass(dtype)
    count = 1 + len(range(kpp, n, kpp))
    return count, n - (count - 1) * kpp


def ragged_len(lens, row, lmax):
    """the key count of a ragged session's row (dec_attn.h:183: L = min(max(lens[row], 1), lmax))"""
    return min(max(lens[row], 1), lmax)


# ---- csrc/lat_attn.h: lat_core_tile ----------------------------------------------------------------------------------------------
KCHUNK = {"fp32": 16, "bf16": 32}                 # common.h:28 / :34: elements per 64-byte k-chunk
SIZEOF = {"fp32": 4, "bf16": 2}


def lat_waves(width, dtype):
    """waves of a tile: la_waves (lat_attn.h:67: 8 up to width 256, 4 above); the bf16 engine runs width 256 on the 4-wave tile
    (engine.hip:223 lat_nw4, :1544)"""
    return 4 if (width > 256 or (width == 256 and dtype == "bf16")) else 8


def lat_lds_bytes(width, dtype):
    nw = 8 if width <= 256 else 4                 # la_supported asks for the default tile of the width (lat_attn.h:67, :76)
    return nw * 16 * 2 * 4 + 16 * width * SIZEOF[dtype] + nw * 16 * width * SIZEOF[dtype]     # lat_attn.h:73


def latent_ok(width, dtype):
    """engine.hip:660: the tile exists at widths 64 / 256 / 768 where its LDS image fits (lat_attn.h:76)"""
    return width in (64, 256, 768) and lat_lds_bytes(width, dtype) <= 160 * 1024 - 4096


@dataclasses.dataclass(frozen=True)
class LatShape:
    nw: int
    ntiles: int                                   # 16-key tiles
    nt_w: int                                     # rounds: tiles of the busiest wave
    idle: int                                     # waves without a tile in the last round
    nf: int                                       # tiles requested ahead
    last_tile_keys: int


def lat_shape(n, width, dtype):
    nw = lat_waves(width, dtype)
    ntiles = (n + 15) >> 4                        # lat_attn.h:129
    nt_w = (ntiles + nw - 1) // nw                # lat_attn.h:129
    kc = width // KCHUNK[dtype]                   # lat_attn.h:90
    nf = 2 if kc <= 8 else (1 if nw == 4 else 0)  # lat_attn.h:145
    # tile `it` of wave w holds keys 16 * (w + it * NW) .. (lat_attn.h:162, :210); a key counts iff key <= last_key = len - 1 (:130, :239)
    return LatShape(nw, ntiles, nt_w, nt_w * nw - ntiles, nf, n - 16 * (ntiles - 1))


# ---- csrc/engine.hip: which launch, which form, how many row ranges --------------------------------------------------------------
PERSIST_MAX_BF16_GREEDY = 128                     # engine.hip:1970
PS_MAXLD = 8                                      # persist.h:54
WIDE_MID_ROWS = 129                               # engine.hip:201
DG_BM = 16                                        # dec_gemm.h:116


def persist_usable(d, dtype, rows, persist=None, latent=None):
    """engine.hip:1971-1991 for a greedy fixed-shape generate() without profiling knobs; persist / latent: TXO_PERSIST / TXO_LATENT"""
    D = d.embed_dim
    if d.dec_exp != 4 or d.dec_layers > PS_MAXLD:                                            # :1979
        return False
    if not ((D == 256 and d.dec_heads == 8) or (D == 768 and d.dec_heads == 12 and dtype == "bf16")):   # :1980
        return False
    if latent_ok(D, dtype) and latent == 1:                                                  # :1982
        return False
    if persist is not None:                                                                  # :1983
        return persist != 0
    if D != 256:                                                                             # :1985
        return False
    if dtype == "bf16" and rows > PERSIST_MAX_BF16_GREEDY:                                   # :1989
        return False
    return rows <= 256                                                                       # :1990


def auto_latent(d, dtype, rows):
    return dtype == "bf16" and d.embed_dim == 256 and rows > PERSIST_MAX_BF16_GREEDY          # engine.hip:1488


def session_latent(d, dtype, rows, latent=None, ragged=False):
    """engine.hip:1274 (choose_form)"""
    return (not ragged) and latent_ok(d.embed_dim, dtype) and (latent == 1 or (latent is None and auto_latent(d, dtype, rows)))


def split(rows, want, unit=16):
    """lanes.h:56-63: contiguous ranges of whole 16-row units, as even as the units allow -> [(first row, rows)]"""
    units = (rows + unit - 1) // unit
    n = max(1, min(want, units))
    out, row = [], 0
    for i in range(n):
        nb = min(rows - row, (units // n + (1 if i < units % n else 0)) * unit)
        out.append((row, nb))
        row += nb
    return out


def row_ranges(d, dtype, rows, latent):
    """engine.hip:2211-2219 (plan_loop) without TXO_LANES"""
    D = d.embed_dim
    want = 2 if dtype == "bf16" and ((D >= 512 and rows >= 256) or (D < 512 and rows > PERSIST_MAX_BF16_GREEDY)) else 1   # :2211
    if want == 2 and latent and D < 512 and rows < 224:                                      # :2215
        want = 1
    if rows < 32:                                                                            # :2217
        want = 1
    return split(rows, want)


def expected_path(d, dtype, rows, persist=None, latent=None):
    """(Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES, Q_LAST_LATENT) of a generate() (engine.hip:2545-2546: a persistent launch reports one range
    and the K/V form), and the ranges' sizes"""
    if persist_usable(d, dtype, rows, persist, latent):
        return (1, 1, 0), [rows]
    lat = session_latent(d, dtype, rows, latent)
    rr = row_ranges(d, dtype, rows, lat)
    return (0, len(rr), int(lat)), [nb for _, nb in rr]


def out_proj_block(d, dtype, range_rows, latent):
    """rows x columns of the blocks of the cross attention's gated out-projection over one range (launch_dec_gemm_wide, engine.hip:1388-1415),
    (16, 32) = the 16-row kernel (dec_gemm.h:116)"""
    D = d.embed_dim
    if dtype != "bf16" or range_rows < 128:                                                  # :1389, :1391
        return (DG_BM, 32)
    folded = latent and d.dec_heads * DH == 2 * D                                            # engine.hip:1487 (latent_fold): K = heads * D
    K = d.dec_heads * D if folded else d.dec_heads * DH
    kw = K // (4 * KCHUNK[dtype]) if K % (4 * KCHUNK[dtype]) == 0 else 0                     # :1394
    if D < 512 and not (kw == 16 and range_rows >= WIDE_MID_ROWS):                           # :1401 (wide_min_rows is never reached)
        return (DG_BM, 32)
    if kw == 6:                                                                              # :1409: RT = 4, BN = 32
        return (DG_BM * 4, 32)
    if kw == 16:                                                                             # :1411: RT = 2, BN = 16
        return (DG_BM * 2, 16)
    return (DG_BM, 32)


# ---- image sizes: N = 1 + (H / 16)(W / 16) on the 256 x 2032 canvas ----------------------------------------------------------------
CANVAS = (256, 2032)
SIZE_OF = {
    2: (16, 16), 63: (16, 992), 64: (48, 336), 65: (64, 256), 127: (112, 288), 128: (16, 2032), 129: (128, 256), 159: (32, 1264),
    160: (48, 848), 161: (160, 256), 255: (32, 2032), 256: (240, 272), 257: (256, 256), 319: (96, 848), 320: (176, 464), 321: (256, 320),
    640: (144, 1136), 641: (256, 640),
}


def n_tokens(h, w):
    return 1 + (h // 16) * (w // 16)


def _on_canvas(name, **over):
    return dataclasses.replace(SHAPE_CASES[name][0], canvas=CANVAS[0], canvas_w=CANVAS[1], **over)


# name -> dims: width 64 with 2 (and 3) decoder heads; the config.yml widths (8 heads) and the ViT-Base widths (12 heads) for the latent tile
DIMS = {
    "w64_h2": _on_canvas("w64_h4", enc_heads=2, dec_heads=2),
    "w64_h3": _on_canvas("w64_h4", enc_heads=2, dec_heads=3),
    "w256_h8": _on_canvas("calib256"),
    "w768_h12": _on_canvas("calib768"),
    "calib256": SHAPE_CASES["calib256"][0],       # D: the 128 x 128 canvas of the shape matrix
    "calib768": SHAPE_CASES["calib768"][0],
}

NINE = (0, 1, 2, 0, 1, 2, 0, 0, 1)                # three distinct images over nine slots: every image at two slots or more


@dataclasses.dataclass(frozen=True)
class Case:
    group: str
    dims: str                                     # DIMS name
    dtype: str
    h: int
    w: int
    slots: tuple                                  # distinct image of every batch row
    why: tuple                                    # the branches the case is listed for (test_decode_cases_cpu.py: CLAIMS)
    latent: object = None                         # TXO_LATENT at engine creation (None: the engine's own choice)
    persist: object = None                        # TXO_PERSIST around generate() (None: the engine's own choice)
    expect: tuple = None                          # D: ((persistent, ranges, latent), range sizes)

    @property
    def n(self):
        return n_tokens(self.h, self.w)

    @property
    def rows(self):
        return len(self.slots)

    @property
    def distinct(self):
        return max(self.slots) + 1

    @property
    def id(self):
        return f"{self.group}-{self.dims}-N{self.n}-B{self.rows}-{self.dtype}"


# A. K/V form: N -> why, per storage type
A_WHY = {
    "fp32": {159: ("one pass", "last pass one short"), 160: ("one pass", "last pass full"), 161: ("two passes", "last pass one key"),
             320: ("two passes", "last pass full"), 321: ("three passes", "last pass one key")},
    "bf16": {319: ("one pass", "last pass one short"), 320: ("one pass", "last pass full"), 321: ("two passes", "last pass one key"),
             640: ("two passes", "last pass full"), 641: ("three passes", "last pass one key")},
}
A_CASES = [Case("A", dn, t, *SIZE_OF[n], NINE, why, latent=0, persist=0)
           for dn in ("w64_h2", "w64_h3") for t, tab in A_WHY.items() for n, why in tab.items()]

# B. ragged: the distinct images' N per storage type, interleaved over 20 slots: every 16-row tile holds rows of 1, 1, 2 and 3 passes
B_NS = {"fp32": (2, 160, 161, 321), "bf16": (2, 320, 321, 641)}
B_SLOTS = tuple(i % 4 for i in range(20))
B_DIMS = "w64_h2"

# C. latent form: (tile waves, N) -> why
C_WHY = {
    (8, 127): ("one round", "no idle wave", "last tile one short"), (8, 128): ("one round", "no idle wave", "last tile full"),
    (8, 129): ("two rounds", "idle waves", "last tile one key"), (8, 255): ("two rounds", "no idle wave", "last tile one short"),
    (8, 256): ("two rounds", "no idle wave", "last tile full"), (8, 257): ("three rounds", "idle waves", "last tile one key"),
    (4, 63): ("one round", "no idle wave", "last tile one short"), (4, 64): ("one round", "no idle wave", "last tile full"),
    (4, 65): ("two rounds", "idle waves", "last tile one key"), (4, 127): ("two rounds", "no idle wave", "last tile one short"),
    (4, 128): ("two rounds", "no idle wave", "last tile full"), (4, 129): ("three rounds", "idle waves", "last tile one key"),
    (4, 255): ("four rounds", "no idle wave", "last tile one short"), (4, 256): ("four rounds", "no idle wave", "last tile full"),
    (4, 257): ("five rounds", "idle waves", "last tile one key"),
}
C_NS8 = (127, 128, 129, 255, 256, 257)
# (dims, storage type) -> the key counts.  The bf16 engine runs width 256 on the FOUR-wave tile: its first seam is at 64 keys, so that
# engine also gets 63 / 64 / 65, and its 127 .. 257 are the two- to five-round boundaries
C_TABLE = {
    ("w64_h2", "fp32"): C_NS8, ("w64_h2", "bf16"): C_NS8, ("w256_h8", "fp32"): C_NS8, ("w256_h8", "bf16"): (63, 64, 65) + C_NS8,
    ("w768_h12", "bf16"): (63, 64, 65, 129),
}
C_CASES = [Case("C", dn, t, *SIZE_OF[n], NINE, C_WHY[(lat_waves(DIMS[dn].embed_dim, t), n)], latent=1)
           for (dn, t), ns in C_TABLE.items() for n in ns]

# D. row seams of generate() at N = 65 (128 x 128 images), default knobs: (dims, storage type, rows) -> ((persistent, ranges, latent), sizes)
D_TABLE = {
    ("calib256", "bf16", 128): ((1, 1, 0), [128]),
    ("calib256", "bf16", 129): ((0, 1, 1), [129]),
    ("calib256", "bf16", 223): ((0, 1, 1), [223]),
    ("calib256", "bf16", 224): ((0, 2, 1), [112, 112]),
    ("calib256", "bf16", 225): ((0, 2, 1), [128, 97]),
    ("calib256", "fp32", 256): ((1, 1, 0), [256]),
    ("calib256", "fp32", 257): ((0, 1, 0), [257]),
    ("calib768", "bf16", 127): ((0, 1, 0), [127]),
    ("calib768", "bf16", 128): ((0, 1, 0), [128]),
    ("calib768", "bf16", 255): ((0, 1, 0), [255]),
    ("calib768", "bf16", 256): ((0, 2, 0), [128, 128]),
}
D_CASES = [Case("D", dn, t, 128, 128, tuple(i % 3 for i in range(rows)), ("row seam",), expect=(path, tuple(sizes)))
           for (dn, t, rows), (path, sizes) in D_TABLE.items()]

ALL_CASES = A_CASES + C_CASES + D_CASES

# bf16 logits against float64.  The bound of every bf16 case is gpu_harness.BF16_BOUND["logits"] (0.0557: calib256 / calib768 at N <= 65,
# 24 positions).  A case that exceeds it although the fp32 engine passes it at 1e-4 and the two forms agree gets an entry here, derived
# as BF16_CALIB was: key count -> the error of calib256 dims on the K/V form at that key count against float64 (measured), bound = 1.5 x.
BF16_REBOUND = {}


def bf16_bound(n, base):
    return max(base, 1.5 * BF16_REBOUND[n]) if n in BF16_REBOUND else base


# ---- the float64 reference, once per distinct image ----------------------------------------------------------------------------------
IMAGE_SEED = {}                                   # (dims name, N) -> seed, where 3000 + N gave an fp32 margin below 2e-5
_SD, _REF = {}, {}


def weights(name):
    """dims name -> (dims, synth state dict, float64 state dict)"""
    if name not in _SD:
        d = DIMS[name]
        sd = synth.synth_state_dict(d, 3)
        _SD[name] = (d, sd, ref64.sd64(sd))
    return _SD[name]


@dataclasses.dataclass(frozen=True)
class Ref:
    img: torch.Tensor                             # (distinct, 3, h, w)
    enc: torch.Tensor                             # float64 encoder rows
    toks: torch.Tensor                            # (distinct, STEPS) the oracle's greedy tokens
    logits: torch.Tensor                          # (distinct, STEPS, V) float64

    @property
    def margin(self):
        return float(ref64.margins(self.logits).min())


def reference(name, h, w, distinct=3):
    """images and float64 greedy decode (eos never stops it) of the `distinct` images of a (dims, size); never modified"""
    key = (name, h, w, distinct)
    if key not in _REF:
        d, _, s64 = weights(name)
        img = rgb_images(distinct, h, w, IMAGE_SEED.get((name, n_tokens(h, w)), 3000 + n_tokens(h, w)))
        enc = ref64.encode(s64, img, grid_w=d.grid)
        toks, lg = ref64.generate(s64, enc, d.bos, None, STEPS)
        _REF[key] = Ref(img, enc, toks, lg)
    return _REF[key]


def case_reference(case):
    return reference(case.dims, case.h, case.w, case.distinct)


def ragged_reference(dtype):
    """group B: [Ref of ONE image] per distinct size (image 0 of the size's reference set)"""
    return [reference(B_DIMS, *SIZE_OF[n], 1) for n in B_NS[dtype]]
