"""The encoder's tile edges: the cases tests/test_gpu_encoder_edges.py runs, and a pure-Python restatement of the dispatch arithmetic
they are chosen for (tests/test_encoder_cases_cpu.py proves from it that every case reaches the branch it is listed for; it holds no
tests, imported like gpu_harness).

The restatements follow the headers line by line and cite them; where a header and this file disagree the header is right and the
case has to move.  The CU count is a launch-time device property (gemm_pp.h:404); the arithmetic below takes 256, the MI355X's.

Every case is two (B: four) distinct images placed at several batch slots (`slots`: the distinct image of each batch row).  Image b
starts at row b * N, so the copies of one image sit at different offsets inside GEMM row panels, attention query blocks and XCD slots."""
import dataclasses

from gpu_harness import SHAPE_CASES

CUS = 256

# ---- csrc/enc_attn.h -----------------------------------------------------------------------------------------------------------------
EA_QBLK, EA_KSTAGE = 128, 64                      # enc_attn.h:25


def attn_shape(n):
    """(nq, stages, tail) of a token count: nq query blocks (enc_attn.h:83 / :280 and engine.hip:1000: (N + EA_QBLK - 1) / EA_QBLK),
    key stages (enc_attn.h:137 / :345: (n + EA_KSTAGE - 1) / EA_KSTAGE) and the keys the last stage lacks to be full -- 0: the tail
    mask (enc_attn.h:164 / :385: kbase + EA_KSTAGE > n) is never taken"""
    nq, stages = (n + EA_QBLK - 1) // EA_QBLK, (n + EA_KSTAGE - 1) // EA_KSTAGE
    return nq, stages, stages * EA_KSTAGE - n


def last_stage_key_tiles(n):
    """16-key tiles the bf16 kernel's last stage runs (enc_attn.h:361: min(4, (n - kbase + 15) >> 4), kbase of the last stage)"""
    kbase = (attn_shape(n)[1] - 1) * EA_KSTAGE
    return min(4, (n - kbase + 15) >> 4)


def idle_query_waves(n):
    """waves of the last query block whose 32 queries all lie beyond n (enc_attn.h:349: active = q0 + wave * 32 < n)"""
    q0 = (attn_shape(n)[0] - 1) * EA_QBLK
    return sum(1 for wave in range(4) if q0 + wave * 32 >= n)


def ea_grid(nq, nbh):
    """workgroups of the attention launch (enc_attn.h:54: ((nbh + 7) / 8) * 8 * nq)"""
    return ((nbh + 7) // 8) * 8 * nq


def ea_block(block, nq, nbh, rev=0):
    """workgroup -> (bh, query block), or None for a retired one (enc_attn.h:47-53)"""
    xcd, slot = block & 7, block >> 3
    bh, qb = (slot // nq) * 8 + xcd, slot - (slot // nq) * nq
    if bh >= nbh:
        return None
    return (nbh - 1 - bh if rev else bh), qb


def retired_blocks(nq, nbh):
    return sum(1 for blk in range(ea_grid(nq, nbh)) if ea_block(blk, nq, nbh) is None)


# ---- csrc/gemm_pp.h ------------------------------------------------------------------------------------------------------------------
PP_BM, PP_BN, PP_BK, PP_SB_MB = 256, 256, 64, 64  # gemm_pp.h:35,41
GB_BM = 128                                       # gemm_big.h:20


def gemm_pp_fits(M, N, K):
    """gemm_pp.h:385-387; engine.hip:768-773 (gemm_plain) takes the LDS-DMA kernel for bf16 storage when this holds, else gemm_big"""
    return K % PP_BK == 0 and K >= 2 * PP_BK and N % PP_BN == 0 and M >= PP_BM and M * K < 2 ** 31 and N * K < 2 ** 31


@dataclasses.dataclass(frozen=True)
class Walk:
    tiles_m: int
    tiles_n: int
    n_tiles: int
    ct: int
    sbr: int
    grid: int

    @property
    def bands(self):
        """column tiles of each band (gemm_pp.h:92: the last band may be narrower)"""
        return [min(self.ct, self.tiles_n - b * self.ct) for b in range((self.tiles_n + self.ct - 1) // self.ct)]

    @property
    def super_blocks(self):
        """row panels of each super-block (gemm_pp.h:90: the last super-block may be shorter)"""
        return [min(self.sbr, self.tiles_m - s * self.sbr) for s in range((self.tiles_m + self.sbr - 1) // self.sbr)]


def pp_walk(M, N, K, sb_mb=PP_SB_MB, cus=CUS, ct_force=0):
    """the launch's tiles_m, tiles_n, ct, sbr and grid (gemm_pp.h:394-395, :414-422)"""
    tiles_m, tiles_n = (M + PP_BM - 1) // PP_BM, N // PP_BN
    n_tiles = tiles_m * tiles_n
    w_bytes, coltile_bytes = N * K * 2, PP_BN * K * 2
    ct = tiles_n
    if w_bytes > (5 << 19) and K < 2048:
        ct = max(1, min(tiles_n, (13 << 17) // coltile_bytes))
    if ct_force > 0 and ct < tiles_n:
        ct = max(1, min(tiles_n, ct_force))
    sbr = tiles_m
    if ct < tiles_n and sb_mb > 0:
        sbr = max(8, min(tiles_m, (sb_mb << 20) // (PP_BM * K * 2)))
    grid = ((min(n_tiles, cus) + 7) // 8) * 8
    return Walk(tiles_m, tiles_n, n_tiles, ct, sbr, grid)


def tile_origin(wk, block, seq, rev=0):
    """(row panel, column tile) of workgroup `block`'s seq-th output tile, or None behind its last (gemm_pp.h:77-80, :86-97)"""
    xcd, slot, chunks = block & 7, block >> 3, wk.grid >> 3
    L = (seq * 8 + xcd) * chunks + slot
    if L >= wk.n_tiles:
        return None
    sb_tiles = wk.sbr * wk.tiles_n
    sb = L // sb_tiles
    L -= sb * sb_tiles
    band_tiles = min(wk.sbr, wk.tiles_m - sb * wk.sbr) * wk.ct
    band = L // band_tiles
    k = L - band * band_tiles
    cols = min(wk.ct, wk.tiles_n - band * wk.ct)
    row, col = k // cols + sb * wk.sbr, k % cols
    if rev:
        row = wk.tiles_m - 1 - row
    return row, band * wk.ct + col


def walk_tiles(wk, rev=0):
    """every (row panel, column tile) the launch computes, workgroup by workgroup, with repeats if the walk had any"""
    out = []
    for block in range(wk.grid):
        seq = 0
        while (t := tile_origin(wk, block, seq, rev)) is not None:
            out.append(t)
            seq += 1
    return out


# ---- csrc/engine.hip: the GEMMs over the B * N encoder rows --------------------------------------------------------------------------
def row_gemms(d):
    """name -> (N, K) of every gemm_plain over M = B * N rows: the four of an encoder layer (engine.hip:1002-1012) and the cross K/V
    projection (engine.hip:1285)"""
    D, Ie, Fe, Id = d.embed_dim, d.enc_inner, d.enc_ffn, d.dec_inner
    return {"qkv": (3 * Ie, D), "attn_out": (2 * D, Ie), "ffn_in": (2 * Fe, D), "ffn_out": (D, Fe), "cross_kv": (d.dec_layers * 2 * Id, D)}


def pp_gemms(d, M):
    """the row GEMMs that take the LDS-DMA kernel in bf16 at M rows"""
    return sorted(k for k, (N, K) in row_gemms(d).items() if gemm_pp_fits(M, N, K))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
CANVAS = (256, 2032)                              # the position table holds a 16 x 127 grid: a 16 x 2032 strip is 128 tokens
MAX_TOKENS = 257


def dims(name, **over):
    """a SHAPE_CASES entry (one encoder layer) on the 256 x 2032 canvas"""
    return dataclasses.replace(SHAPE_CASES[name][0], canvas=CANVAS[0], canvas_w=CANVAS[1], **over)


def n_tokens(h, w):
    return 1 + (h // 16) * (w // 16)


FIVE = (0, 1, 0, 0, 1)                            # [a, b, a, a, b]

# the fp32 bounds of tests/test_gpu_shapes.py (set at N <= 65).  A case that exceeds its bound gets an entry in FP32_REBOUND:
# (float32 CPU oracle against float64 on the case's inputs, the engine's error); its bound is max(project bound, 4 x the oracle's error)
FP32_REBOUND = {}


def fp32_bound(case_id, d):
    base = 2e-4 if d.embed_dim >= 704 else 1e-4
    return max(base, 4 * FP32_REBOUND[case_id][0]) if case_id in FP32_REBOUND else base


@dataclasses.dataclass(frozen=True)
class Case:
    dims: str                                     # SHAPE_CASES name
    h: int
    w: int
    slots: tuple                                  # distinct image of every batch row
    why: tuple                                    # the branches the case is listed for (test_encoder_cases_cpu.py: CLAIMS)
    env: tuple = ()                               # knobs the engine reads at creation

    @property
    def n(self):
        return n_tokens(self.h, self.w)

    @property
    def rows(self):
        return len(self.slots) * self.n

    @property
    def distinct(self):
        return max(self.slots) + 1

    @property
    def id(self):
        return f"{self.dims}-N{self.n}-B{len(self.slots)}"


# A. token counts: N -> (image H x W, why)
TOKEN_COUNTS = {
    64: (112, 144, ("exact key stage",)),
    65: (128, 128, ("one past a key stage",)),
    127: (144, 224, ("one short of a query block",)),
    128: (16, 2032, ("exact query block", "exact key stage")),
    129: (128, 256, ("one past a query block", "one past a key stage", "idle query waves")),
    193: (192, 256, ("one past a key stage", "two query blocks")),
    256: (240, 272, ("exact query block", "exact key stage", "two query blocks")),
    257: (256, 256, ("one past a query block", "one past a key stage", "idle query waves")),
}
# what the dims add to a token-count case
A_DIMS = {"w192_h3": ("mostly gemm_big",), "w256_h3": (), "w512": ("pp every gemm",)}
A_RETIRED = ("w192_h3", "w256_h3")                # 3 and 5 encoder heads: retired attention workgroups from two query blocks on

A_CASES = []
for _dn, _dwhy in A_DIMS.items():
    _ret = lambda n: ("retired slots",) if _dn in A_RETIRED and n > EA_QBLK else ()
    for _n, (_h, _w, _why) in TOKEN_COUNTS.items():
        A_CASES.append(Case(_dn, _h, _w, FIVE, _why + _dwhy + _ret(_n)))
    A_CASES.append(Case(_dn, 256, 256, (0,), ("one past a query block", "one past a key stage", "one row in the last panel")
                        + _dwhy + _ret(257)))

# B. row counts across the GEMM seams: M = 128, 130, 254, 256, 258 (16 x 16 images, N = 2) and 255 (15 images of 64 x 64, N = 17)
B_DIMS = ("w128", "w384_h6", "w704_h11")
B_ROWS = {64: ("below pp",), 65: ("below pp",), 127: ("below pp", "one short of pp"), 128: ("pp split", "exact row panel"),
          129: ("pp split", "two rows in the last panel")}
B_CASES = []
for _dn in B_DIMS:
    for _b, _why in B_ROWS.items():
        B_CASES.append(Case(_dn, 16, 16, tuple(i % 4 for i in range(_b)), _why))
    B_CASES.append(Case(_dn, 64, 64, tuple(i % 4 for i in range(15)), ("below pp", "one short of pp")))

# C. the persistent walk at K = 512: 17 slots of 256 x 256 images, M = 4369
C_SLOTS = tuple(FIVE[i % 5] for i in range(17))
C_WHY = ("two tiles per workgroup", "narrower last band", "bands 6 6 4", "short last panel")
C_CASE = Case("w512", 256, 256, C_SLOTS, C_WHY + ("one super-block",))
C_CASE_SB = Case("w512", 256, 256, C_SLOTS, C_WHY + ("super-blocks 16 2",), env=(("TXO_PP_SB_MB", "4"),))

ALL_CASES = A_CASES + B_CASES + [C_CASE, C_CASE_SB]


def edge_rows(n):
    """name -> rows of an image whose error is printed apart: a failure then names the edge"""
    nq, stages, _ = attn_shape(n)
    qb0, ks0 = (nq - 1) * EA_QBLK, (stages - 1) * EA_KSTAGE
    first = ks0 if nq == 1 else min(qb0, ks0)     # (one query block: the rows in front of the last key stage)
    return {"interior": range(0, first), "last key stage": range(ks0, n), "last query block": range(qb0, n), "last row": range(n - 1, n)}
