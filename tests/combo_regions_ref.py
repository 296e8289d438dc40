"""kaori::CombinatorialBarcodesSingleEnd<max_size, V> (handlers/CombinatorialBarcodesSingleEnd.hpp:71-258) restated for any
number of variable regions V: what the seeded tests of the region-combination handler compare against.
tests/golden/kaori_combo_regions.json (the real handler's outputs for V = 1..8) pins the restatement, and at V = 2 the
oracle's count_combo does too: test_combo_regions_reference_cpu.py.

Every position and strand of every read is scanned: the constant mismatches are computed here, and the regions of the
windows within the budget are looked up through the oracle's match_barcodes, one call per region and strand over all such
windows of a case.  A look-up at the full budget gives the unique closest barcode and its distance; the handler's look-up
under the remaining budget b (:168) finds the same barcode when that distance is <= b and nothing otherwise.  Then
find_match's walk over the regions (:149-186), the first / best rule (:188-258) and the sort.
"""
import random

import numpy as np

from tests import gen

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i


def regions_of(template: str):
    """[(start, end)] of the runs of '-' in the forward template."""
    out, i = [], 0
    while i < len(template):
        if template[i] == "-":
            j = i
            while j < len(template) and template[j] == "-":
                j += 1
            out.append((i, j))
            i = j
        else:
            i += 1
    return out


def check_arguments(template: str, pools, mismatches: int):
    """The constructor's checks in its order (:79-93), then the engine's own on the budget; raises OracleError."""
    from oracle.pyoracle import OracleError
    regions = regions_of(template)
    if len(regions) != len(pools):
        raise OracleError(f"expected {len(pools)} variable regions in the constant template")
    for i, ((s, e), pool) in enumerate(zip(regions, pools)):
        vlen = len(pool[0]) if pool else 0
        if vlen != e - s:
            raise OracleError(f"length of variable region {i + 1} ({e - s}) should be the same as its sequences ({vlen})")
    if mismatches < 0:
        raise OracleError("negative number of mismatches")


def _strand_layout(template: str, reverse: bool):
    """(constant positions, their base codes, region starts and lengths in scan order) of the searched template."""
    t = gen.rc(template).replace("N", "-") if reverse else template      # (gen.rc gives 'N' for '-'; templates hold no N)
    pos = np.array([i for i, c in enumerate(t) if c != "-"], dtype=np.int64)
    codes = _CODE[np.frombuffer(t.encode(), dtype=np.uint8)][pos] if len(pos) else np.zeros(0, dtype=np.uint8)
    return pos, codes, regions_of(t)


def read_combinations(oracle, reads, template: str, strand: int, pools, mismatches: int, use_first: bool):
    """Per read the combination the handler collects (a tuple of pool indices), or None."""
    check_arguments(template, pools, mismatches)
    V, T = len(pools), len(template)
    strands = [s for s in (0, 1) if (s == 0 and strand in (0, 2)) or (s == 1 and strand in (1, 2))]
    layout = {s: _strand_layout(template, s == 1) for s in strands}
    for pool in pools:                                        # the libraries' own errors (duplicates, unknown bases)
        oracle.match_barcodes([], pool, max(mismatches, 0), False)
    # windows within the budget: (read, position, strand, constant mismatches), in the handler's order per read
    windows = []
    for i, read in enumerate(reads):
        raw = read.encode() if isinstance(read, str) else bytes(read)
        if len(raw) < T:
            continue
        codes = _CODE[np.frombuffer(raw, dtype=np.uint8)]
        view = np.lib.stride_tricks.sliding_window_view(codes, T)
        const = {}
        for s in strands:
            pos, want, _ = layout[s]
            const[s] = (view[:, pos] != want).sum(axis=1) if len(pos) else np.zeros(len(view), dtype=np.int64)
        for p in range(len(view)):
            for s in strands:
                if const[s][p] <= mismatches:
                    windows.append((i, p, s, int(const[s][p]), raw))
    # one look-up call per strand and region in scan order: region r of the reverse scan is pool V - 1 - r (:111-116)
    found = {}
    for s in strands:
        mine = [k for k, w in enumerate(windows) if w[2] == s]
        for r, (a, b) in enumerate(layout[s][2]):
            subs = [windows[k][4][windows[k][1] + a: windows[k][1] + b] for k in mine]
            slot = V - 1 - r if s else r
            idx, mm = oracle.match_barcodes(subs, pools[slot], mismatches, s == 1) if subs else ([], [])
            for k, x, d in zip(mine, idx, mm):
                found[(k, r)] = (int(x), int(d))
    out = [None] * len(reads)
    best = {}                                                 # read -> [best mismatches, combination, found]
    done = set()
    for k, (i, p, s, c, _) in enumerate(windows):
        if i in done:
            continue
        obs, combo, ok = c, [0] * V, True
        for r in range(V):                                    # find_match (:149-186)
            x, d = found[(k, r)]
            if x < 0 or d > mismatches - obs:
                ok = False
                break
            obs += d
            combo[V - 1 - r if s else r] = x
        if not ok:
            continue
        combo = tuple(combo)
        if use_first:                                         # :188-217
            out[i] = combo
            done.add(i)
            continue
        state = best.setdefault(i, [mismatches + 1, None, False])      # :219-258
        if obs == state[0]:
            if state[1] != combo:
                state[2] = False
        elif obs < state[0]:
            state[0], state[1], state[2] = obs, combo, True
    for i, state in best.items():
        if state[2]:
            out[i] = state[1]
    return out


def count_combo_regions(oracle, reads, template: str, strand: int, pools, mismatches: int, use_first: bool):
    """(indices int32[V, K] sorted by (first, ..., last), freq int32[K], total)."""
    per_read = read_combinations(oracle, reads, template, strand, pools, mismatches, use_first)
    tally = {}
    for combo in per_read:
        if combo is not None:
            tally[combo] = tally.get(combo, 0) + 1
    keys = sorted(tally)
    idx = np.array(keys, dtype=np.int32).reshape(len(keys), len(pools)).T.copy()
    return idx, np.array([tally[k] for k in keys], dtype=np.int32), len(reads)


# ---- seeded cases ---------------------------------------------------------------------------------------------------
def make_case(rng: random.Random, lens, sizes, n_reads: int, strand: int, mismatches: int, alphabet: str = gen.BASES, iupac: float = 0.0,
              flanks=(1, 6), begins: bool = False, ends: bool = False, p_sub: float = 0.03, p_n: float = 0.01, p_lower: float = 0.0,
              pad_hi: int = 12) -> dict:
    """A case over len(lens) regions: pools of `sizes` sequences of `lens` bases.  begins / ends: the template starts / stops
    with a variable region."""
    V = len(lens)
    pools = [gen.make_pool(rng, n, v, alphabet, min_dist=1, iupac_rate=iupac if v <= 64 else min(iupac, 0.01)) for n, v in zip(sizes, lens)]
    parts = ["" if begins else gen.rand_seq(rng, rng.randint(max(flanks[0], 1), flanks[1]))]
    for r, v in enumerate(lens):
        parts.append("-" * v)
        if r < V - 1:
            parts.append(gen.rand_seq(rng, rng.randint(max(flanks[0], 1), flanks[1])))
    parts.append("" if ends else gen.rand_seq(rng, rng.randint(max(flanks[0], 1), flanks[1])))
    template = "".join(parts)
    reads = gen.make_reads(rng, template, pools, n_reads, strand, p_sub, p_n, p_lower, 0.1, pad_hi)
    return dict(kind="combo_regions", template=template, strand=strand, pools=pools, mismatches=mismatches, reads=reads)


def indices_list(idx: np.ndarray, freq: np.ndarray):
    """(indices [V, K], freq [K]) as a plain list of [i_0, ..., i_last, count] rows, the goldens' form."""
    return [[int(x) for x in idx[:, j]] + [int(freq[j])] for j in range(idx.shape[1])]
