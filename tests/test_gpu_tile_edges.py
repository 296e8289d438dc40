"""The LDS-staged kernels at their tile and dispatch boundaries, cell by cell, against the oracle.

Each staged kernel is a template over the plane words per read (NW), per template window (NT), the candidate words
(NC), the key width (W) and its family's flags; the host picks one cell per batch (dispatch_shape and the Launch*
structs of scg_kernels.hip).  CELLS holds one entry per cell the host can select, with a template, key and max_len hint
that reach it.  Every cell gets deterministic, constructed inputs: constructs at the ends of reads and at the word
boundaries of the candidate mask, reads of T, T - 1, 0 and 32 * NW bases, two constructs per read, mismatches and
non-ACGT bases at the first and last constant and variable bases, a lone N in an otherwise-ACGT wavefront, constructs
split across neighbouring reads, workgroups and the ends of the batch, and every valid max_len hint.  Every result is
compared exactly with the oracle (oracle/liboracle.so).  Paired cells build these inputs on each mate in turn, with a
valid partner on the other mate, so that a wrong window shows up as a counted pair.  Placements use one barcode each,
so a failure names the placements whose counts differ.  tools/staged_variants.py checks, from a rocprofv3 run of this
module (profiles/tile_edges_kernel_stats.csv), that every instantiation was launched
(profiles/tile_edges_coverage.txt).
"""
import os
import random

import numpy as np
import pytest

from tests import gen

pytestmark = pytest.mark.gpu

U32, U64 = "unsigned int", "unsigned long"
SHAPES = [(5, 2, 3), (5, 2, 5), (10, 2, 10), (5, 4, 3), (5, 4, 5), (10, 4, 10), (5, 8, 3), (5, 8, 5), (10, 8, 10)]
C, V = "c", "v"

# Single-end templates with one variable region: (segments, max_len hint) per (NW, NT, NC, W).  NC = 3 needs
# compact_ok (both ends open with constant runs) and hint - T + 1 <= 96; NC = 5 with NT > 2 needs a seed past
# template block 1 (a template whose first 64 bases hold few constant runs, searched with 2 mismatches).
SE = {
    (5, 2, 3, U32): ([(C, 4), (V, 16), (C, 4)], 119),            # T = 24, hint T + 95
    (5, 2, 5, U32): ([(C, 16), (V, 32), (C, 16)], 160),          # T = 64, key 32, hint T + 96
    (10, 2, 10, U32): ([(C, 4), (V, 16), (C, 4)], 161),
    (5, 4, 3, U32): ([(C, 9), (V, 32), (C, 24)], 160),           # T = 65, hint T + 95
    (5, 4, 5, U32): ([(C, 16), (V, 32), (C, 80)], 160),          # T = 128
    (10, 4, 10, U32): ([(C, 48), (V, 32), (C, 48)], 319),
    (5, 8, 3, U32): ([(C, 48), (V, 32), (C, 49)], 160),          # T = 129
    (5, 8, 5, U32): ([(C, 16), (V, 32), (C, 102)], 160),
    (10, 8, 10, U32): ([(C, 112), (V, 32), (C, 112)], 320),      # T = 256
    (5, 2, 3, U64): ([(C, 15), (V, 33), (C, 16)], 159),          # key 33
    (5, 2, 5, U64): ([(C, 6), (V, 33), (C, 25)], 160),
    (10, 2, 10, U64): ([(C, 12), (V, 40), (C, 12)], 200),
    (5, 4, 3, U64): ([(C, 9), (V, 64), (C, 9)], 160),            # key 64
    (5, 4, 5, U64): ([(C, 2), (V, 64), (C, 34)], 160),
    (10, 4, 10, U64): ([(C, 16), (V, 33), (C, 16)], 161),        # T = 65
    (5, 8, 3, U64): ([(C, 32), (V, 64), (C, 33)], 160),
    (5, 8, 5, U64): ([(C, 2), (V, 64), (C, 74)], 160),
    (10, 8, 10, U64): ([(C, 96), (V, 64), (C, 96)], 320),
}
# Two variable regions (combo, dual_single_end): W is 64-bit when a region has 33..64 bases.
COMBO = {
    (5, 2, 3, U32): ([(C, 4), (V, 8), (C, 4), (V, 8), (C, 4)], 123),
    (5, 2, 5, U32): ([(C, 12), (V, 16), (C, 8), (V, 16), (C, 12)], 160),
    (10, 2, 10, U32): ([(C, 4), (V, 8), (C, 4), (V, 8), (C, 4)], 320),
    (5, 4, 3, U32): ([(C, 9), (V, 16), (C, 4), (V, 16), (C, 20)], 160),
    (5, 4, 5, U32): ([(C, 4), (V, 24), (C, 4), (V, 30), (C, 66)], 160),
    (10, 4, 10, U32): ([(C, 40), (V, 16), (C, 4), (V, 16), (C, 52)], 300),
    (5, 8, 3, U32): ([(C, 40), (V, 16), (C, 4), (V, 16), (C, 53)], 160),
    (5, 8, 5, U32): ([(C, 4), (V, 24), (C, 4), (V, 30), (C, 88)], 160),
    (10, 8, 10, U32): ([(C, 100), (V, 16), (C, 8), (V, 16), (C, 116)], 320),
    (5, 2, 3, U64): ([(C, 8), (V, 33), (C, 4), (V, 8), (C, 8)], 156),
    (5, 2, 5, U64): ([(C, 8), (V, 33), (C, 4), (V, 8), (C, 8)], 157),
    (10, 2, 10, U64): ([(C, 8), (V, 33), (C, 4), (V, 8), (C, 8)], 250),
    (5, 4, 3, U64): ([(C, 9), (V, 33), (C, 4), (V, 8), (C, 16)], 160),
    (5, 4, 5, U64): ([(C, 2), (V, 33), (C, 4), (V, 25), (C, 36)], 160),
    (10, 4, 10, U64): ([(C, 30), (V, 33), (C, 4), (V, 8), (C, 40)], 319),
    (5, 8, 3, U64): ([(C, 40), (V, 33), (C, 4), (V, 12), (C, 40)], 160),
    (5, 8, 5, U64): ([(C, 2), (V, 33), (C, 4), (V, 25), (C, 76)], 160),
    (10, 8, 10, U64): ([(C, 90), (V, 40), (C, 4), (V, 24), (C, 98)], 320),
}
# Eight variable regions (dual_single_end): always the 64-bit single kernel.
DSE8 = {
    (5, 2, 3): ([(C, 4)] + [(V, 3), (C, 2)] * 7 + [(V, 3), (C, 4)], 140),
    (10, 4, 10): ([(C, 30)] + [(V, 3), (C, 2)] * 7 + [(V, 3), (C, 40)], 319),
    (5, 8, 3): ([(C, 50)] + [(V, 3), (C, 2)] * 7 + [(V, 3), (C, 41)], 160),
}
# Paired templates: mate 2 carries the template that sets NT; mate 1 a short one that decides staged (two tiles: 10
# constant bases, 2 mismatches) or passes (24 constant bases, none).  (segments of mate 2, hint) per cell.
DUAL = {
    (5, 2, 3, U32): ([(C, 10), (V, 24), (C, 10)], 120),
    (5, 2, 5, U32): ([(C, 20), (V, 24), (C, 20)], 160),
    (10, 2, 10, U32): ([(C, 10), (V, 24), (C, 10)], 200),
    (5, 4, 3, U32): ([(C, 9), (V, 24), (C, 32)], 129),           # T2 = 65
    (5, 4, 5, U32): ([(C, 16), (V, 24), (C, 88)], 160),
    (10, 4, 10, U32): ([(C, 50), (V, 24), (C, 54)], 300),
    (5, 8, 3, U32): ([(C, 52), (V, 24), (C, 53)], 129),          # T2 = 129, hint - T1 + 1 = 96
    (5, 8, 5, U32): ([(C, 16), (V, 24), (C, 110)], 160),
    (10, 8, 10, U32): ([(C, 116), (V, 24), (C, 116)], 320),
    (5, 2, 3, U64): ([(C, 10), (V, 40), (C, 10)], 140),
    (5, 2, 5, U64): ([(C, 12), (V, 40), (C, 12)], 160),
    (10, 2, 10, U64): ([(C, 10), (V, 40), (C, 10)], 250),
    (5, 4, 3, U64): ([(C, 9), (V, 40), (C, 31)], 145),
    (5, 4, 5, U64): ([(C, 2), (V, 40), (C, 58)], 160),
    (10, 4, 10, U64): ([(C, 40), (V, 40), (C, 48)], 319),
    (5, 8, 3, U64): ([(C, 44), (V, 40), (C, 45)], 145),
    (5, 8, 5, U64): ([(C, 2), (V, 40), (C, 98)], 160),
    (10, 8, 10, U64): ([(C, 108), (V, 40), (C, 108)], 320),
}
PAIRED = ("dual_staged", "dual_passes", "dual_passes_rand", "dual_mates", "dual_mates_rand")
POOL = 72                   # barcodes per pool: one per placement


def _mate1(family, w):
    key = 24 if w == U32 else 40
    if family == "dual_staged":
        return [(C, 5), (V, key), (C, 5)], 2
    return [(C, 12), (V, key), (C, 12)], 0


def _pick_mm(t, nw, nc, nt, choices=(1, 0, 2)):
    """A mismatch budget that gives the template the compact form the cell needs."""
    for mm in choices:
        if nc == 3 and gen.compact_ok(t, mm):
            return mm
        if nw == 5 and nc == 5 and nt > 2 and not gen.compact_ok(t, mm):
            return mm
        if nc == nw and (nw == 10 or nt == 2):
            return mm
    raise AssertionError(f"no mismatch budget reaches NC={nc} for {t}")


def _build_cells():
    cells = []
    for w in (U32, U64):
        for nw, nt, nc in SHAPES:
            key = (nw, nt, nc, w)
            rng = random.Random(str(key))
            segs, hint = SE[key]
            t = gen.segments_template(rng, segs)
            cells.append(dict(family="single", nw=nw, nt=nt, nc=nc, w=w, t=t, hint=hint, mm=_pick_mm(t, nw, nc, nt)))
            if w == U32:
                cells.append(dict(family="random", nw=nw, nt=nt, nc=nc, w=None, t=t, hint=hint, mm=cells[-1]["mm"]))
            segs, hint = COMBO[key]
            t = gen.segments_template(rng, segs)
            mm = _pick_mm(t, nw, nc, nt)
            cells.append(dict(family="combo", nw=nw, nt=nt, nc=nc, w=w, t=t, hint=hint, mm=mm))
            cells.append(dict(family="combo_neg", nw=nw, nt=nt, nc=nc, w=w, t=t, hint=hint, mm=mm))
            if w == U32:
                cells.append(dict(family="dse2", nw=nw, nt=nt, nc=nc, w=U64, t=t, hint=hint, mm=mm))
            segs2, hint = DUAL[key]
            t2 = gen.segments_template(rng, segs2)
            for fam in PAIRED:
                segs1, mm1 = _mate1(fam, w)
                t1 = gen.segments_template(random.Random(len(fam) * 7 + nt), segs1)
                mm2 = _pick_mm(t2, nw, nc, nt, (0, 1, 2) if nc != 5 or nt == 2 else (2, 3))
                h = len(t1) + 96 if (nc, nt) == (5, 2) else hint        # compact off by one candidate position
                cells.append(dict(family=fam, nw=nw, nt=nt, nc=nc, w=w, t=t1, t2=t2, hint=h, mm=mm1, mm2=mm2))
    for (nw, nt, nc), (segs, hint) in DSE8.items():
        t = gen.segments_template(random.Random(nt * 31 + nw), segs)
        cells.append(dict(family="dse8", nw=nw, nt=nt, nc=nc, w=U64, t=t, hint=hint, mm=_pick_mm(t, nw, nc, nt)))
    for c in cells:
        w = {U32: "u32", U64: "u64", None: "any"}[c["w"]]
        tl = f"T{len(c['t'])}" + (f"+{len(c['t2'])}" if "t2" in c else "")
        c["id"] = f"{c['family']}-NW{c['nw']}-NT{c['nt']}-NC{c['nc']}-{w}-{tl}-h{c['hint']}"
    return cells


CELLS = _build_cells()


def _nt(T):
    return 2 if T <= 64 else 4 if T <= 128 else 8


def host_kernels(cell, hint=None):
    """The staged kernels the host launches for this cell (a mirror of launch_* and the Launch* structs)."""
    h = cell["hint"] if hint is None else hint
    nw = 5 if h <= 160 else 10
    fam = cell["family"]
    if fam in PAIRED:
        t1, t2 = cell["t"], cell["t2"]
        nt = _nt(max(len(t1), len(t2)))
        compact = nw == 5 and gen.compact_ok(t1, cell["mm"]) and gen.compact_ok(t2, cell["mm2"]) and h - min(len(t1), len(t2)) + 1 <= 96
        nc = 3 if compact else nw
        w = cell["w"]
        passes = gen.chance_hits(t1, cell["mm"], h) + gen.chance_hits(t2, cell["mm2"], h) < 0.01
        rand = "true" if fam.endswith("_rand") else "false"
        first = f"dual_passes_kernel<{nw}, {nt}, {nc}, false, {rand}, {w}>" if passes else f"dual_staged_kernel<{nw}, {nt}, {nc}, {w}>"
        if fam.startswith("dual_mates"):
            # include.invalid=TRUE: a plain pass (not randomized-specific for paired_combo) then the mates-only pass
            return {f"dual_passes_kernel<{nw}, {nt}, {nc}, true, {rand}, {w}>", first}
        return {first}
    t = cell["t"]
    nt = _nt(len(t))
    nc = 3 if nw == 5 and gen.compact_ok(t, cell["mm"]) and h - len(t) + 1 <= 96 else nw
    w = cell["w"]
    if fam == "single":
        return {f"single_staged_kernel<{nw}, {nt}, {nc}, {w}>"}
    if fam in ("dse2", "dse8"):
        return {f"single_staged_kernel<{nw}, {nt}, {nc}, {U64}>"}
    if fam == "random":
        return {f"random_staged_kernel<{nw}, {nt}, {nc}>"}
    if fam == "combo":
        return {f"combo_staged_kernel<{nw}, {nt}, {nc}, false, {w}>"}
    return {f"combo_staged_kernel<{nw}, {nt}, {nc}, true, {w}>", f"single_staged_kernel<{nw}, {nt}, {nc}, {U64}>"}


def test_cell_table_reaches_every_cell():
    """Each entry's template, budget and hint reach the cell its id names, and the table covers every combination."""
    seen = set()
    for c in CELLS:
        ks = host_kernels(c)
        named = {f"<{c['nw']}, {c['nt']}, {c['nc']}" in k for k in ks}
        assert named == {True}, (c["id"], ks)
        if c["family"] == "dual_staged":
            assert all(k.startswith("dual_staged_kernel") for k in ks), (c["id"], ks)
        if c["family"] in ("dual_passes", "dual_passes_rand"):
            assert all(k.startswith("dual_passes_kernel") for k in ks), (c["id"], ks)
        seen |= ks
    fams = {"single_staged_kernel": 18, "combo_staged_kernel": 36, "dual_staged_kernel": 18, "dual_passes_kernel": 72, "random_staged_kernel": 9}
    for f, n in fams.items():
        assert sum(k.startswith(f + "<") for k in seen) == n, (f, sorted(k for k in seen if k.startswith(f)))


# ---------------------------------------------------------------------------------------------
# Pools and constructs
# ---------------------------------------------------------------------------------------------
def _regions(t):
    out, i = [], 0
    while i < len(t):
        if t[i] == "-":
            j = i
            while j < len(t) and t[j] == "-":
                j += 1
            out.append((i, j))
            i = j
        else:
            i += 1
    return out


class Setup:
    """Pools and constructs of one cell: construct(j) spells barcode (or pair) j on the searched template(s)."""

    def __init__(self, cell):
        self.cell = cell
        self.fam = cell["family"]
        self.paired = self.fam in PAIRED
        rng = random.Random(cell["id"])
        self.fill = gen.Filler(len(cell["id"]) * 1009 + cell["nt"])
        regs = _regions(cell["t"])
        if len(regs) > 2:       # short regions: only the rows (combinations) need to differ
            self.pools = [[gen.rand_seq(rng, b - a) for _ in range(POOL)] for a, b in regs]
            assert len({"".join(row) for row in zip(*self.pools)}) == POOL, cell["id"]
        else:
            self.pools = [gen.make_pool(rng, POOL, b - a, gen.BASES, min_dist=min(3, b - a)) for a, b in regs]
        assert all(len(p) == POOL for p in self.pools), cell["id"]
        if self.paired:
            a, b = _regions(cell["t2"])[0]
            self.pool2 = gen.make_pool(rng, POOL, b - a, gen.BASES, min_dist=3)

    def construct(self, j, mate=1):
        if mate == 2:
            return gen.fill_template(self.cell["t2"], [self.pool2[j]])
        return gen.fill_template(self.cell["t"], [p[j] for p in self.pools])

    def tmpl(self, mate=1):
        return self.cell["t2"] if mate == 2 else self.cell["t"]

    def tlen(self, mate=1):
        return len(self.tmpl(mate))

    def mm(self, mate=1):
        return self.cell["mm2"] if mate == 2 else self.cell["mm"]


def _n_to_g(construct, t, count, where):
    """Replaces `count` G bases of the construct in its constant ('const') or variable ('var') positions with N.  N's
    2-bit code equals G's, so a scanner that lost the validity plane would see a match there."""
    idx = [i for i, ch in enumerate(t) if (ch != "-") == (where == "const") and construct[i] == "G"]
    if len(idx) < count:
        idx += [i for i, ch in enumerate(t) if construct[i] == "G" and i not in idx]
    s = construct
    for i in idx[:count]:
        s = gen.substitute(s, i, "N")
    return s


# ---------------------------------------------------------------------------------------------
# Batches.  A batch is a list of reads (single-end) or of (mate 1, mate 2) pairs, plus labels {barcode j: placement}.
# The builders construct one mate (`mate`) of a paired cell; the other mate of each read they give barcode j holds
# a valid construct of pair j, so that a wrong window on the constructed mate shows up as a counted pair.
# ---------------------------------------------------------------------------------------------
def _pairs(S, reads, mate):
    """Pairs of the constructed reads of `mate` with their partners: the matching construct of pair j (reverse-
    complemented when the entry says so: partners take the strand of their construct), or random bases beside
    fillers (j = None)."""
    other = 3 - mate
    out = []
    for r, j, *flip in reads:
        if j is None:
            partner = S.fill(min(S.cell["hint"], S.tlen(other) + 3))
        else:
            c = S.construct(j, other)
            c = gen.rc(c) if flip and flip[0] else c
            partner = c if len(c) + 3 > S.cell["hint"] else S.fill(3) + c
        out.append((r, partner) if mate == 1 else (partner, r))
    return out


def placement_batch(S, mate=1):
    cell, H, T, t = S.cell, S.cell["hint"], S.tlen(mate), S.tmpl(mate)
    construct = lambda j: S.construct(j, mate)         # noqa: E731
    reads, labels = [], {}
    j = 0

    def add(label, *rs):
        nonlocal j
        labels[j] = label
        for r in rs:
            reads.append((r, j, o == "rc"))
        j += 1

    o = "fwd"
    for o, f in (("fwd", lambda s: s), ("rc", gen.rc)):
        add(f"pos0-{o}", gen.place(S.fill, f(construct(j)), H, 0))
        add(f"last-{o}", gen.place(S.fill, f(construct(j)), H, H - T))
        add(f"exactT-{o}", f(construct(j)))
        add(f"Tminus1-{o}", f(construct(j))[:-1], f(construct(j))[1:])
        if 32 * cell["nw"] <= H:
            n = 32 * cell["nw"]
            add(f"len{n}-{o}", gen.place(S.fill, f(construct(j)), n, n - T), gen.place(S.fill, f(construct(j)), n, 0))
        for p in (31, 32, 63, 64, 95):
            if p + T <= H:
                add(f"cand{p}-{o}", gen.place(S.fill, f(construct(j)), H, p))
                add(f"cand{p}-last-{o}", gen.place(S.fill, f(construct(j)), p + T, p))
        if 2 * T <= H:
            c = f(construct(j))
            add(f"twice-{o}", c + c)
            c2 = f(construct(j + 1))
            add(f"two-barcodes-{o}", c + c2)
            labels[j] = f"two-barcodes-{o} (second)"
            j += 1
        ci = [i for i, ch in enumerate(t) if ch != "-"]
        vi = [i for i, ch in enumerate(t) if ch == "-"]
        for name, i in (("mm-const-first", ci[0]), ("mm-const-last", ci[-1]), ("mm-var-first", vi[0]), ("mm-var-last", vi[-1])):
            add(f"{name}-{o}", gen.place(S.fill, f(gen.substitute(construct(j), i)), min(H, T + 3), min(3, H - T)))
        for where in ("const", "var"):
            add(f"N-{where}-{o}", gen.place(S.fill, f(_n_to_g(construct(j), t, 1, where)), min(H, T + 2), 0))
            add(f"N{S.mm(mate) + 1}-{where}-{o}", f(_n_to_g(construct(j), t, S.mm(mate) + 1, where)))
            low = "".join(ch.lower() if (t[i] != "-") == (where == "const") else ch for i, ch in enumerate(construct(j)))
            add(f"lower-{where}-{o}", f(low))
    if 2 * T <= H:
        add("fwd+rc", construct(j) + gen.rc(construct(j)))
    add("empty", "")
    reads.append((S.fill(H), None))          # the batch's longest read has exactly `hint` bases
    assert j <= POOL, (cell["id"], j)
    return _finish(S, reads, mate), labels


def lone_n_batch(S, mate=1):
    """Three workgroups of clean constructs; the only non-ACGT read is lane 0 of the first, lane 63 of the second and
    lane 64 (the first lane of wave 1) of the third."""
    cell = S.cell
    reads, labels = [], {0: "lone-N-lane0", 1: "lone-N-lane63", 2: "lone-N-lane64"}
    for wg, lane in enumerate((0, 63, 64)):
        for i in range(256):
            if i == lane:
                c = _n_to_g(S.construct(wg, mate), S.tmpl(mate), S.mm(mate) + 1, "const")
                reads.append((c if wg != 1 else gen.rc(c), wg, wg == 1))
            else:
                j = 3 + (i % (POOL - 3))
                c = S.construct(j, mate)
                reads.append((S.fill(i % 3) + (c if i % 2 else gen.rc(c)), j, i % 2 == 0))
    reads.append((S.fill(cell["hint"]), None))
    for j in range(3, POOL):
        labels[j] = "clean"
    return _finish(S, reads, mate), labels


BLEED = 1        # the barcode of every split construct


def bleed_ks(T, regs):
    ks = {1, 2, 8, 15, 16, 17, 31, 32, 33, T // 2, T - 2, T - 1}
    for a, b in regs:
        ks |= {a, a + 1, b - 1, b}
    return sorted(k for k in ks if 1 <= k <= T - 1)


def bleed_batch(S, mate=1):
    """Constructs split across neighbouring reads, k = 1 .. T - 1 bases in the first, on both strands; and for a
    subset of k across workgroup boundaries (lanes 255 | 256).  Both reads of a split keep a valid partner."""
    cell, H, T = S.cell, S.cell["hint"], S.tlen(mate)
    c = S.construct(BLEED, mate)
    splits = [(k, cc) for cc in (c, gen.rc(c)) for k in range(1, T)]
    wg_splits = [(k, cc) for cc in (c, gen.rc(c)) for k in bleed_ks(T, _regions(S.tmpl(mate)))]
    n_wg = len(wg_splits) + 1 + (2 * len(splits)) // 250
    reads = [(S.fill(8), None) for _ in range(256 * n_wg)]

    def put(i, k, cc):
        a, b = gen.split_pair(S.fill, cc, k, min(H, k + 5), min(H, T - k + 5))
        reads[i], reads[i + 1] = (a, BLEED, cc != c), (b, BLEED, cc != c)

    for m, (k, cc) in enumerate(wg_splits):
        put(256 * (m + 1) - 1, k, cc)
    slot = [256 * g + l for g in range(n_wg) for l in range(2, 252, 2)]
    for (k, cc), i in zip(splits, slot):
        put(i, k, cc)
    reads.append((S.fill(H), None))
    return _finish(S, reads, mate), {BLEED: "split construct"}


def _finish(S, reads, mate=1):
    if S.paired:
        return _pairs(S, reads, mate)
    return [e[0] for e in reads]


def _strand_modes(S):
    """Two (use_first, strand) modes that count constructs of either orientation: both strands for single-end cells;
    for pairs, both mates forward and then both reverse (partners take the strand of their construct)."""
    return ((True, 0), (False, 1)) if S.paired else ((True, 2), (False, 2))


# ---------------------------------------------------------------------------------------------
# Running a cell on the GPU and in the oracle
# ---------------------------------------------------------------------------------------------
MODES = [(True, 0), (True, 1), (True, 2), (False, 0), (False, 1), (False, 2)]
REV = {0: (False, False), 1: (True, True), 2: (True, False)}


class Batch:
    """Reads as the kernels see them: optionally inside a larger buffer (bytes before and after the slice, offsets
    that start past the slice's first byte) or as one fixed-length block."""

    def __init__(self, reads, pre=b"", post=b"", lead=0, fixed=False, mate=1):
        self.reads, self.pre, self.post, self.lead, self.fixed = reads, pre, post, lead, fixed
        self.mate = mate            # paired batches: the mate whose buffer has this layout; the other is uploaded plainly

    def upload(self, reads, device, fixed):
        import torch
        body = "".join(reads).encode()
        big = self.pre + body + self.post
        buf = torch.from_numpy(np.frombuffer(big if big else b"\0", dtype=np.uint8).copy()).to(device)
        start = len(self.pre) - self.lead
        assert start >= 0
        seqs = buf[start:]
        if fixed:
            return seqs, None, len(reads[0]) if reads else 1
        offs = np.zeros(len(reads) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(r) for r in reads])
        offs += self.lead
        return seqs, torch.from_numpy(offs.astype(np.int32)).to(device), 0


def _all_reads(batches, paired):
    if paired:
        return [p for b in batches for p in b.reads]
    return [r for b in batches for r in b.reads]


def oracle_run(oracle, cell, batches, mode, tmp_path=None):
    fam, t, mm = cell["family"], cell["t"], cell["mm"]
    uf, strand = mode
    S = _setup(cell)
    reads = _all_reads(batches, fam in PAIRED)
    if fam == "single":
        c, tot = oracle.count_single(reads, t, strand, S.pools[0], mm, uf)
        return dict(counts=c, total=tot)
    if fam in ("dse2", "dse8"):
        c, tot = oracle.count_dual_single_end(reads, t, strand, S.pools, mm, uf)
        return dict(counts=c, total=tot)
    if fam == "combo":
        i, f, tot = oracle.count_combo(reads, t, strand, S.pools[0], S.pools[1], mm, uf)
        return dict(indices=i, freq=f, total=tot)
    if fam == "combo_neg":
        d = oracle.count_dual_single_end_diag(reads, t, strand, S.pools, mm, uf)
        return dict(counts=d["counts"], indices=d["indices"], freq=d["freq"], total=d["total"])
    if fam == "random":
        keys, tot = oracle.count_random(reads, t, strand, mm, uf)
        return dict(keys=dict(keys), total=tot)
    r1, r2 = [a for a, _ in reads], [b for _, b in reads]
    rev1, rev2 = REV[strand]
    args = (r1, r2, t, rev1, mm, S.pools[0], cell["t2"], rev2, cell["mm2"], S.pool2, fam.endswith("_rand"), uf)
    if fam.startswith("dual_mates"):
        d = oracle.count_dual_diag(*args)
        p = oracle.count_combo_paired(*args)
        return {**{"diag." + k: v for k, v in d.items()}, **{"pc." + k: v for k, v in p.items()}}
    c, tot = oracle.count_dual(*args)
    return dict(counts=c, total=tot)


def gpu_run(sc, gpu, cell, batches, mode, hint=None, tmp_path=None):
    """Counts every batch with one plan (hint: the max_len passed with each batch; None = the cell's)."""
    fam, t, mm = cell["family"], cell["t"], cell["mm"]
    uf, strand = mode
    S = _setup(cell)
    h = cell["hint"] if hint is None else hint
    if fam == "combo_neg":          # only the file entry runs include.invalid=TRUE; it passes the window's true maximum
        from oracle.pyoracle import write_fastq
        fq = os.path.join(str(tmp_path), "reads.fastq")
        write_fastq(fq, _all_reads(batches, False))
        c, (i, f), tot = sc.count_dual_barcodes_single_end(fq, t, S.pools, strand, mm, uf, True, 1)
        return dict(counts=c, indices=i, freq=f, total=tot)
    if fam in PAIRED:
        rev1, rev2 = REV[strand]
        args = (t, rev1, mm, S.pools[0], cell["t2"], rev2, cell["mm2"], S.pool2, fam.endswith("_rand"), uf)
        plans = [sc.Plan.dual(*args, diagnostics=True), sc.Plan.paired_combo(*args)] if fam.startswith("dual_mates") else [sc.Plan.dual(*args)]
        try:
            for b in batches:
                m1, m2 = [a for a, _ in b.reads], [x for _, x in b.reads]
                l1, l2 = (b, Batch(m2)) if b.mate == 1 else (Batch(m1), b)
                s1, o1, f1 = l1.upload(m1, gpu, l1.fixed)
                s2, o2, f2 = l2.upload(m2, gpu, l2.fixed)
                for p in plans:
                    p.count_paired(s1, s2, o1, o2, fixed_len1=f1, fixed_len2=f2, n_pairs=len(m1), max_len=h)
            if len(plans) == 2:
                d, pc = plans[0].read_diagnostics(), plans[1].read_diagnostics()
                return {**{"diag." + k: v for k, v in d.items()}, **{"pc." + k: v for k, v in pc.items()}}
            c, tot = plans[0].read()
            return dict(counts=c, total=tot)
        finally:
            for p in plans:
                p.close()
    if fam == "single":
        plan = sc.Plan.single(t, strand, S.pools[0], mm, uf)
    elif fam in ("dse2", "dse8"):
        plan = sc.Plan.dual_single_end(t, strand, S.pools, mm, uf)
    elif fam == "combo":
        plan = sc.Plan.combo(t, strand, S.pools[0], S.pools[1], mm, uf)
    else:
        plan = sc.Plan.random(t, strand, mm, uf)
    with plan:
        for b in batches:
            seqs, offs, fl = b.upload(b.reads, gpu, b.fixed)
            plan.count(seqs, offs, fixed_len=fl, n_reads=len(b.reads), max_len=h if offs is not None else 0)
        if fam == "combo":
            i, f, tot = plan.read_combo()
            return dict(indices=i, freq=f, total=tot)
        if fam == "random":
            (keys, freq), tot = plan.read_random()
            return dict(keys=dict(zip(keys, freq.tolist())), total=tot)
        c, tot = plan.read()
        return dict(counts=c, total=tot)


_SETUPS = {}


def _setup(cell):
    if cell["id"] not in _SETUPS:
        _SETUPS[cell["id"]] = Setup(cell)
    return _SETUPS[cell["id"]]


def _hits(cell, res, j):
    """Counts the result gives barcode (pair) j, for naming the placements that differ."""
    S = _setup(cell)
    fam = cell["family"]
    if fam == "random":
        return res["keys"].get(S.pools[0][j], 0)
    if "counts" in res:
        return int(res["counts"][j]) if j < len(res["counts"]) else 0
    if "indices" in res:
        return int(sum(f for a, b, f in zip(res["indices"][0], res["indices"][1], res["freq"]) if a == j and b == j))
    return int(res["diag.counts"][j]) + int(sum(f for a, b, f in zip(res["pc.indices"][0], res["pc.indices"][1], res["pc.freq"]) if a == j and b == j))


def assert_same(cell, got, exp, labels, what):
    bad = []
    for k in exp:
        a, b = exp[k], got[k]
        same = a == b if isinstance(a, (dict, int)) else np.array_equal(np.asarray(a), np.asarray(b))
        if not same:
            bad.append(k)
    if bad:
        diff = {lab: (_hits(cell, exp, j), _hits(cell, got, j)) for j, lab in labels.items() if _hits(cell, exp, j) != _hits(cell, got, j)}
        raise AssertionError(f"{cell['id']} {what}: {bad} differ; placements (oracle, gpu): {diff}; "
                             f"total {exp.get('total', exp.get('diag.total'))} vs {got.get('total', got.get('diag.total'))}")


IDS = [c["id"] for c in CELLS]
# (cell, mate): the placement, lone-N, bleed and hint tests build their constructs on each searched mate -- mate 2 of a
# paired cell carries the template that sets NT -- with a valid partner on the other mate.
SIDES = [(c, m) for c in CELLS for m in ((1, 2) if c["family"] in PAIRED else (1,))]
SIDE_IDS = [c["id"] + (f"-mate{m}" if c["family"] in PAIRED else "") for c, m in SIDES]


@pytest.mark.parametrize("cell,mate", SIDES, ids=SIDE_IDS)
def test_placement(sc, oracle, gpu, cell, mate, tmp_path):
    S = _setup(cell)
    reads, labels = placement_batch(S, mate)
    for mode in MODES:
        exp = oracle_run(oracle, cell, [Batch(reads)], mode)
        got = gpu_run(sc, gpu, cell, [Batch(reads)], mode, tmp_path=tmp_path)
        assert_same(cell, got, exp, labels, f"placement mate {mate} use_first={mode[0]} strand={mode[1]}")


@pytest.mark.parametrize("cell,mate", SIDES, ids=SIDE_IDS)
def test_lone_n_wavefront(sc, oracle, gpu, cell, mate, tmp_path):
    S = _setup(cell)
    reads, labels = lone_n_batch(S, mate)
    for mode in _strand_modes(S):
        exp = oracle_run(oracle, cell, [Batch(reads)], mode)
        if cell["family"] != "random":
            assert [_hits(cell, exp, j) for j in range(3)] == [0, 0, 0], cell["id"]     # mm + 1 N's: never a match
        got = gpu_run(sc, gpu, cell, [Batch(reads)], mode, tmp_path=tmp_path)
        assert_same(cell, got, exp, labels, f"lone N mate {mate} use_first={mode[0]} strand={mode[1]}")


@pytest.mark.parametrize("cell,mate", SIDES, ids=SIDE_IDS)
def test_bleed_across_reads(sc, oracle, gpu, cell, mate, tmp_path):
    S = _setup(cell)
    reads, labels = bleed_batch(S, mate)
    for mode in _strand_modes(S):
        exp = oracle_run(oracle, cell, [Batch(reads)], mode)
        assert _hits(cell, exp, BLEED) == 0, cell["id"]
        got = gpu_run(sc, gpu, cell, [Batch(reads)], mode, tmp_path=tmp_path)
        assert_same(cell, got, exp, labels, f"bleed mate {mate} use_first={mode[0]}")


def edge_batches(S, mate=1):
    """Batches sliced from a larger buffer whose bytes just before the slice hold a construct's head (the first read
    starts with its tail), or whose bytes after the last offset hold the tail (the last read ends with the head).  The
    split read keeps a valid partner."""
    H, T = S.cell["hint"], S.tlen(mate)
    c = S.construct(BLEED, mate)
    out = []
    for n, (k, cc) in enumerate((k, cc) for cc in (c, gen.rc(c)) for k in sorted({1, T // 2, T - 1})):
        fills = [(S.fill(10 + i), None) for i in range(5)] + [(S.fill(H), None)]
        head = [(cc[k:] + S.fill(3), BLEED, cc != c)] + fills
        tail = fills + [(S.fill(3) + cc[:k], BLEED, cc != c)]
        pre = S.fill(16 + n).encode() + cc[:k].encode()
        out.append(Batch(_finish(S, head, mate), pre=pre, post=S.fill(40).encode(), mate=mate))
        out.append(Batch(_finish(S, tail, mate), pre=S.fill(n + 1).encode(), post=cc[k:].encode() + S.fill(7).encode(), mate=mate))
    return out


EDGE_SIDES = [(c, m) for c, m in SIDES if c["family"] != "combo_neg"]        # (the file entry makes its own batches)


@pytest.mark.parametrize("cell,mate", EDGE_SIDES, ids=[i for (c, m), i in zip(SIDES, SIDE_IDS) if c["family"] != "combo_neg"])
def test_bleed_across_batch_ends(sc, oracle, gpu, cell, mate, tmp_path):
    S = _setup(cell)
    batches = edge_batches(S, mate)
    for mode in _strand_modes(S):
        exp = oracle_run(oracle, cell, batches, mode)
        assert _hits(cell, exp, BLEED) == 0, cell["id"]
        got = gpu_run(sc, gpu, cell, batches, mode, tmp_path=tmp_path)
        assert_same(cell, got, exp, {BLEED: "split construct"}, f"batch ends mate {mate} use_first={mode[0]}")


@pytest.mark.parametrize("cell,mate", SIDES, ids=SIDE_IDS)
def test_hint_invariance(sc, oracle, gpu, cell, mate, tmp_path, monkeypatch):
    """The same batch under every valid max_len hint (each selecting its own cell) and on the general engine."""
    S = _setup(cell)
    reads, labels = placement_batch(S, mate)
    hints = [0, cell["hint"]] + [h for h in (160, 320) if h > cell["hint"]]
    if cell["family"] == "combo_neg":
        # The only way to the only_if_negative combo kernel is the file entry, which passes each window's true maximum
        # itself: these cells run that one hint, and otherwise rest on the comparison with the general engine below.
        hints = [0]
    modes = ((False, 0), (False, 1)) if S.paired else ((False, 2),)
    for mode in modes:
        exp = oracle_run(oracle, cell, [Batch(reads)], mode)
        for h in hints:
            got = gpu_run(sc, gpu, cell, [Batch(reads)], mode, hint=h, tmp_path=tmp_path)
            assert_same(cell, got, exp, labels, f"mate {mate} strand {mode[1]} hint {h}")
    monkeypatch.setenv("SCG_FORCE_GENERAL", "1")
    for mode in modes:
        exp = oracle_run(oracle, cell, [Batch(reads)], mode)
        got = gpu_run(sc, gpu, cell, [Batch(reads)], mode, tmp_path=tmp_path)
        assert_same(cell, got, exp, labels, f"mate {mate} strand {mode[1]} general engine")


# ---------------------------------------------------------------------------------------------
# Batch geometry and counting modes, on one representative cell per family
# ---------------------------------------------------------------------------------------------
def _rep(family):
    want = {"single": "NW5-NT2-NC3-u32", "dse2": "NW10-NT4-NC10", "combo": "NW5-NT4-NC3-u32", "random": "NW10-NT2-NC10",
            "dual_staged": "NW5-NT2-NC3-u32", "dual_passes": "NW5-NT8-NC3-u64", "dual_mates": "NW10-NT4-NC10-u32"}[family]
    return next(c for c in CELLS if c["family"] == family and want in c["id"])


REPS = [_rep(f) for f in ("single", "dse2", "combo", "random", "dual_staged", "dual_passes", "dual_mates")]
REP_IDS = [c["id"] for c in REPS]


def _clean_reads(S, n, length=None):
    """n reads with one construct each (barcodes in turn, both strands), of `length` bases or ragged."""
    T, H = S.tlen(), S.cell["hint"]
    out = []
    for i in range(n):
        c = S.construct(i % POOL)
        c = c if i % 2 else gen.rc(c)
        L = length if length else min(H, T + (i * 7) % (H - T + 1))
        out.append((gen.place(S.fill, c, L, (i * 3) % (L - T + 1)), i % POOL, i % 2 == 0))
    return _finish(S, out)


@pytest.mark.parametrize("cell", REPS, ids=REP_IDS)
def test_batch_sizes(sc, oracle, gpu, cell):
    S = _setup(cell)
    for n in (1, 63, 64, 65, 255, 256, 257, 511, 513):
        reads = _clean_reads(S, n)
        for mode in _strand_modes(S):
            exp = oracle_run(oracle, cell, [Batch(reads)], mode)
            got = gpu_run(sc, gpu, cell, [Batch(reads)], mode)
            assert_same(cell, got, exp, {}, f"n={n} strand {mode[1]}")


@pytest.mark.parametrize("form", ["offsets", "fixed_len"])
@pytest.mark.parametrize("cell", REPS, ids=REP_IDS)
def test_misaligned_batches(sc, oracle, gpu, cell, form):
    """seqs sliced 1..15 bytes past an aligned allocation, the first offset past the slice's start (offsets form) or
    reads of one length (fixed_len form: mate 1 for pairs)."""
    S = _setup(cell)
    fixed = form == "fixed_len"
    batches = []
    for mis in range(1, 16):
        reads = _clean_reads(S, 300 + mis, length=cell["hint"] if fixed else None)
        lead = 0 if fixed else mis % 5
        batches.append(Batch(reads, pre=S.fill(mis + lead).encode(), post=S.fill(9).encode(), lead=lead, fixed=fixed))
    for mode in _strand_modes(S):
        exp = oracle_run(oracle, cell, batches, mode)
        got = gpu_run(sc, gpu, cell, batches, mode)
        assert_same(cell, got, exp, {}, f"{form} strand {mode[1]}")


@pytest.mark.parametrize("counting", ["tally", "lane-fold", "wave-fold", "direct"])
@pytest.mark.parametrize("cell", [c for c in REPS if c["family"] in ("single", "dse2", "combo", "dual_staged", "dual_passes")],
                         ids=[c["id"] for c in REPS if c["family"] in ("single", "dse2", "combo", "dual_staged", "dual_passes")])
def test_counting_modes(sc, oracle, gpu, cell, counting, monkeypatch):
    """The tally (SCG_TALLY=1), replicas folded one lane per counter (< 64 replicas) or one wave per counter, and direct
    atomics (no replicas); the replica count is fixed when the plan is created."""
    monkeypatch.setenv("SCG_TALLY", "1" if counting == "tally" else "0")
    # POOL counters (combo: POOL^2 cells): 2^(addr - 1) / counters replicas at most
    n_counters = POOL * POOL if cell["family"] == "combo" else POOL
    addr = {"tally": 20, "lane-fold": n_counters.bit_length() + 4, "wave-fold": n_counters.bit_length() + 8, "direct": 0}[counting]
    monkeypatch.setenv("SCG_REPLICA_ADDR_LOG2", str(addr))
    S = _setup(cell)
    reads, labels = placement_batch(S)
    reads = reads + _clean_reads(S, 700)
    # two launches accumulate: the oracle counts the reads twice over
    for mode in _strand_modes(S):
        exp = oracle_run(oracle, cell, [Batch(reads + reads)], mode)
        got = gpu_run(sc, gpu, cell, [Batch(reads), Batch(reads)], mode)
        assert_same(cell, got, exp, labels, f"{counting} strand {mode[1]}")


# ---------------------------------------------------------------------------------------------
# Paired batches whose mates take different shapes, and Big keys as a control
# ---------------------------------------------------------------------------------------------
def _dual_case(seed, l1, l2, t1_segs, t2_segs):
    rng = random.Random(seed)
    t1, t2 = gen.segments_template(rng, t1_segs), gen.segments_template(rng, t2_segs)
    p1 = gen.make_pool(rng, 30, l1, gen.BASES, min_dist=3)
    p2 = gen.make_pool(rng, 30, l2, gen.BASES, min_dist=3)
    return t1, t2, p1, p2, gen.Filler(seed)


MIXED = {
    "R1-short-R2-long": (20, 10, [(C, 4), (V, 20), (C, 4)], [(C, 6), (V, 10), (C, 6)], 150, 300),
    "T1-20-T2-200": (12, 24, [(C, 4), (V, 12), (C, 4)], [(C, 88), (V, 24), (C, 88)], 120, 260),
    "R1-fixed-R2-ragged": (16, 16, [(C, 8), (V, 16), (C, 8)], [(C, 8), (V, 16), (C, 8)], 64, 150),
    "R2-empty": (16, 16, [(C, 8), (V, 16), (C, 8)], [(C, 8), (V, 16), (C, 8)], 100, 0),
}


@pytest.mark.parametrize("randomized", [False, True])
@pytest.mark.parametrize("case", list(MIXED))
def test_mixed_mate_shapes(sc, oracle, gpu, case, randomized):
    l1, l2, s1, s2, n1, n2 = MIXED[case]
    t1, t2, p1, p2, fill = _dual_case(len(case), l1, l2, s1, s2)
    r1, r2 = [], []
    for i in range(400):
        j = i % 30
        a = gen.fill_template(t1, [p1[j]])
        b = gen.fill_template(t2, [p2[(j + (i % 7 == 0)) % 30]])
        a = gen.place(fill, a, n1, (i * 5) % (n1 - len(a) + 1)) if case == "R1-fixed-R2-ragged" else \
            gen.place(fill, a, min(n1, len(a) + i % 40), 0)
        b = "" if n2 == 0 else gen.place(fill, b, min(n2, len(b) + i % 90), i % (min(n2, len(b) + i % 90) - len(b) + 1))
        if randomized and i % 3 == 0:
            a, b = b, a
        r1.append(a)
        r2.append(b)
    for uf in (True, False):
        exp = oracle.count_dual(r1, r2, t1, False, 1, p1, t2, False, 1, p2, randomized, uf)
        s1_, o1 = sc.upload_reads(r1, gpu)
        s2_, o2 = sc.upload_reads(r2, gpu)
        with sc.Plan.dual(t1, False, 1, p1, t2, False, 1, p2, randomized, uf) as plan:
            if case == "R1-fixed-R2-ragged" and not randomized:
                plan.count_paired(s1_, s2_, None, o2, fixed_len1=n1, n_pairs=len(r1))
            else:
                plan.count_paired(s1_, s2_, o1, o2)
            got = plan.read()
        assert got[1] == exp[1] and np.array_equal(got[0], exp[0]), (case, uf)
        expd = oracle.count_dual_diag(r1, r2, t1, False, 1, p1, t2, False, 1, p2, randomized, uf)
        with sc.Plan.dual(t1, False, 1, p1, t2, False, 1, p2, randomized, uf, diagnostics=True) as plan:
            plan.count_paired(s1_, s2_, o1, o2)
            gotd = plan.read_diagnostics()
        for k in expd:
            assert np.array_equal(np.asarray(expd[k]), np.asarray(gotd[k])), (case, uf, k)


def test_big_keys_take_the_general_kernels(sc, oracle, gpu):
    """Keys of 65 bases (Big): the general kernels only, whatever the hint; a control beside the staged cells."""
    rng = random.Random(65)
    t = gen.segments_template(rng, [(C, 8), (V, 65), (C, 8)])
    pool = gen.make_pool(rng, 20, 65, gen.BASES, min_dist=3)
    fill = gen.Filler(65)
    reads = [gen.place(fill, gen.fill_template(t, [pool[i % 20]]), 81 + i % 60, i % (i % 60 + 1)) for i in range(300)]
    reads += [gen.rc(r) for r in reads[:50]]
    exp = oracle.count_single(reads, t, 2, pool, 1, False)
    seqs, offs = sc.upload_reads(reads, gpu)
    for h in (0, 160, 320):
        with sc.Plan.single(t, 2, pool, 1, False) as plan:
            plan.count(seqs, offs, max_len=h if h >= 141 else 0)
            got = plan.read()
        assert got[1] == exp[1] and np.array_equal(got[0], exp[0]), h
