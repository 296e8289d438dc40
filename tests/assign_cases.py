"""Constructed inputs for Plan.assign at the tile and dispatch boundaries of the staged kernels, with the match state
every read must get (a helper, not a test: tests/test_assign_abi.py and tests/test_gpu_assign.py use it).

One entry per (NW, NT, NC, W) cell of the single-end table of tests/test_gpu_tile_edges.py -- the same templates, budgets
and max_len hints, so that assign_staged_kernel is launched in each of the 18 shapes single_staged_kernel has.  A read is
built from placed constructs, and its expected state follows from the placements alone: a construct at position p on
strand s with c substitutions in its constant and d in its variable bases is a hit (barcode, p, c + d, d, s) when
c + d is within the budget; first mode takes the first hit in (position, forward before reverse) order, best mode the
fewest mismatches, none on a tie between two barcodes unless a strictly better hit follows (SimpleSingleMatch.hpp:200-306).
Filler bases could hide a chance match: tools/gen_assign_golden.py --check-edges runs every read through the reference
and compares field by field (profiles/assign_edges_vs_kaori.txt).

Each read of interest is the last read of workgroup 0 and the only read of workgroup 1 of a batch of STAGE_BLOCK + 1
reads; the other lanes of workgroup 0 hold the cell's other reads in turn.
"""
import numpy as np

from tests import gen
from tests.test_gpu_tile_edges import CELLS as _TILE_CELLS
from tests.test_gpu_tile_edges import POOL, Setup

STAGE_BLOCK = 256
FIELDS = ("index", "position", "mismatches", "variable_mismatches", "reverse")
NONE = (-1, -1, -1, -1, -1)
STRAND = 2                  # every cell searches both strands
CELLS = [c for c in _TILE_CELLS if c["family"] == "single"]
IDS = [c["id"] for c in CELLS]


def expected_state(hits, budget, use_first):
    """hits: (position, reverse, barcode, constant mismatches, variable mismatches) of every construct placed in a read."""
    best, state = budget + 1, NONE
    for p, rev, j, c, d in sorted(hits, key=lambda h: (h[0], h[1])):
        tot = c + d
        if tot > budget:
            continue
        if use_first:
            return (j, p, tot, d, int(rev))
        if tot == best:
            if state[0] != j:
                state = NONE
        elif tot < best:
            best, state = tot, (j, p, tot, d, int(rev))
    return state


class Case:
    """The reads of interest of one cell (`items`: label, read, expected state in first and in best mode) and the batches
    made of them (`batches`: lists of item numbers, STAGE_BLOCK + 1 each)."""

    def __init__(self, cell):
        self.cell = cell
        self.template, self.budget, self.hint = cell["t"], cell["mm"], cell["hint"]
        S = Setup(cell)
        self.pool = S.pools[0]
        self.items = []
        self._build(S)
        m = len(self.items)
        self.batches = [[(i + 1 + k) % m for k in range(STAGE_BLOCK - 1)] + [i, i] for i in range(m)]

    def _add(self, label, read, hits):
        assert len(read) <= self.hint, (self.cell["id"], label, len(read))
        self.items.append((label, read, expected_state(hits, self.budget, True), expected_state(hits, self.budget, False)))

    def _build(self, S):
        cell, H, t = self.cell, self.hint, self.template
        T = len(t)
        ci = [i for i, ch in enumerate(t) if ch != "-"]
        vi = [i for i, ch in enumerate(t) if ch == "-"]
        nxt = iter(range(10 ** 6))

        def barcode():
            return next(nxt) % POOL

        for o, f in (("fwd", lambda s: s), ("rc", gen.rc)):
            rev = o == "rc"

            def one(label, n, pos, c=0, d=0, edit=lambda s: s):
                j = barcode()
                self._add(f"{label}-{o}", gen.place(S.fill, f(edit(S.construct(j))), n, pos), [(pos, rev, j, c, d)])

            one("pos0", H, 0)
            one("last", H, H - T)
            one("exactT", T, 0)
            j = barcode()
            self._add(f"Tminus1-head-{o}", f(S.construct(j))[:-1], [])
            self._add(f"Tminus1-tail-{o}", f(S.construct(j))[1:], [])
            if 32 * cell["nw"] <= H:
                n = 32 * cell["nw"]
                one(f"len{n}-last", n, n - T)
                one(f"len{n}-pos0", n, 0)
            for p in (31, 32, 63, 64, 95, 96):
                if p + T <= H:
                    one(f"cand{p}", H, p)
                    one(f"cand{p}-last", p + T, p)
            n, pos = min(H, T + 3), min(3, H - T)
            one("mm-const-first", n, pos, c=1, edit=lambda s: gen.substitute(s, ci[0]))
            one("mm-const-last", n, pos, c=1, edit=lambda s: gen.substitute(s, ci[-1]))
            one("mm-var-first", n, pos, d=1, edit=lambda s: gen.substitute(s, vi[0]))
            one("mm-var-last", n, pos, d=1, edit=lambda s: gen.substitute(s, vi[-1]))
            one("mm-const+var", n, pos, c=1, d=1, edit=lambda s: gen.substitute(gen.substitute(s, ci[0]), vi[-1]))
            one("N-const", n, pos, c=1, edit=lambda s: gen.substitute(s, ci[len(ci) // 2], "N"))
        if 2 * T <= H:
            j, k = barcode(), barcode()
            a, b = S.construct(j), S.construct(k)
            worse = gen.substitute(a, ci[0])
            self._add("twice", a + a, [(0, False, j, 0, 0), (T, False, j, 0, 0)])
            self._add("second-better", worse + b, [(0, False, j, 1, 0), (T, False, k, 0, 0)])
            self._add("second-better-same-barcode", worse + a, [(0, False, j, 1, 0), (T, False, j, 0, 0)])
            self._add("two-barcodes", a + b, [(0, False, j, 0, 0), (T, False, k, 0, 0)])
            self._add("fwd+rc-two-barcodes", a + gen.rc(b), [(0, False, j, 0, 0), (T, True, k, 0, 0)])
            self._add("rc+fwd-two-barcodes", gen.rc(a) + b, [(0, True, j, 0, 0), (T, False, k, 0, 0)])
        if 3 * T <= H:
            j, k, m = barcode(), barcode(), barcode()
            tie = gen.substitute(S.construct(j), vi[0]) + gen.substitute(S.construct(k), ci[-1])
            self._add("tie-then-better", tie + S.construct(m), [(0, False, j, 0, 1), (T, False, k, 1, 0), (2 * T, False, m, 0, 0)])
        self._add("empty", "", [])

    def reads(self, batch):
        return [self.items[i][1] for i in batch]

    def expected(self, batch, use_first):
        """The five arrays of a batch, in FIELDS order."""
        rows = np.array([self.items[i][2 if use_first else 3] for i in batch], dtype=np.int64).reshape(len(batch), 5)
        return [rows[:, k].astype(np.int32 if k < 2 else np.int8) for k in range(5)]


_CASES = {}


def case(cell):
    if cell["id"] not in _CASES:
        _CASES[cell["id"]] = Case(cell)
    return _CASES[cell["id"]]
