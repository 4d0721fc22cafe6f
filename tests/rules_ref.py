"""Brute-force restatement of the LaTeX brace rule (texocr_amd/rules.py: brace_rules), independent of the table: the decoded BYTE STRING of
a token sequence is scanned byte by byte, tracking the parity of the current run of backslashes, the brace depth and, per token, whether it
dipped below zero.  Holds no tests."""
from typing import List, NamedTuple, Optional, Sequence


class Scan(NamedTuple):
    odd: bool                 # the text ends in an odd run of backslashes
    depth: int                # open groups at the end (clamped as the automaton clamps: never below 0, never above depth_max)
    disallowed: List[bool]    # per token: the rule would not have let a row pick it
    low: int                  # the deepest the raw (unclamped) depth ever dipped (0: never below zero)
    eos_depths: List[int]     # the depth in front of every eos token


def scan(vocab, tokens: Sequence[int], depth_max: int = 64, eos: Optional[int] = None, banned: Sequence[int] = ()) -> Scan:
    """vocab: id -> bytes.  One pass over the concatenated bytes; token boundaries only decide where the per-token verdicts are taken."""
    odd, depth, raw, low = False, 0, 0, 0
    verdicts, eos_depths = [], []
    for t in tokens:
        t = int(t)
        entry, dip = depth, 0
        bad = t in banned or t not in vocab
        if eos is not None and t == eos:
            eos_depths.append(depth)
            bad = bad or depth != 0
        rel = 0
        for c in vocab.get(t, b""):
            ch = bytes([c])
            if ch == b"\\":
                odd = not odd
                continue
            if not odd:
                if ch == b"{":
                    rel += 1
                elif ch == b"}":
                    rel -= 1
                    dip = min(dip, rel)
            odd = False
        bad = bad or entry + dip < 0 or entry + rel > depth_max
        raw += rel
        low = min(low, raw)
        depth = min(max(entry + rel, 0), depth_max)
        verdicts.append(bool(bad))
    return Scan(odd, depth, verdicts, low, eos_depths)
