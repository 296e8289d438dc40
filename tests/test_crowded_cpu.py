"""The crowded pools and queries of tests/gen.py (crowded_*): that the generators yield what they are meant to yield, checked
with a brute-force Hamming classifier in plain numpy, and that the oracle agrees with that brute force and with real kaori
(tests/golden/kaori_crowded.json) on them.  CPU only; tests/test_gpu_crowded.py runs the same inputs through the device."""
import random

import numpy as np
import pytest

from tests import gen
from tests import golden_util as G
from tests.test_oracle_golden import normalise, run_oracle

# what a library byte allows / what a query byte is, one bit per base; any other query byte is no base at all
_SETS = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}
ENTRY = np.zeros(256, dtype=np.uint8)
QUERY = np.zeros(256, dtype=np.uint8)
for _c, _v in _SETS.items():
    ENTRY[ord(_c)] = ENTRY[ord(_c.lower())] = _v
for _c in "ACGT":
    QUERY[ord(_c)] = QUERY[ord(_c.lower())] = _SETS[_c]
COMPLEMENT = np.array([(v & 1) << 3 | (v & 2) << 1 | (v & 4) >> 1 | (v & 8) >> 3 for v in range(16)], dtype=np.uint8)


def mismatch_table(choices, sequences, reverse=False):
    """bool[query, entry, position]: the query's byte is not one of the bases the entry allows there."""
    e = ENTRY[np.frombuffer("".join(choices).encode("latin1"), dtype=np.uint8)].reshape(len(choices), -1)
    q = QUERY[np.frombuffer("".join(sequences).encode("latin1"), dtype=np.uint8)].reshape(len(sequences), -1)
    if reverse:
        q = COMPLEMENT[q[:, ::-1]]
    return (e[None, :, :] & q[:, None, :]) == 0


def brute_match(choices, sequences, cap, reverse=False):
    """matchBarcodes by exhaustive comparison: (index, mismatches), -1 for nothing within cap and for a tie at the minimum."""
    dist = mismatch_table(choices, sequences, reverse).sum(axis=2)
    best = dist.min(axis=1)
    unique = (dist == best[:, None]).sum(axis=1) == 1
    ok = (best <= cap) & unique
    return np.where(ok, dist.argmin(axis=1), -1).astype(np.int32), np.where(ok, best, -1).astype(np.int32)


LENGTHS = sorted(set(gen.CROWDED_MATCH_LENGTHS) | {10, 12, 24, 36, 70, 100})       # every key length of a crowded case
MATCH_NAMES = [n for n in gen.crowded_golden_cases() if n.startswith("match-")]


def pool_and_queries(length, budget):
    if length in gen.CROWDED_MATCH_LENGTHS:
        case = G.crowded(f"match-{length}-{budget}-fwd")[0]
        return case["choices"], case["sequences"]
    rng = random.Random(f"cell {length} {budget}")
    pool = gen.crowded_pool(rng, length, budget, iupac=False)         # (as the paired and single-end cases build them)
    return list(pool), gen.crowded_queries(rng, pool, budget)


@pytest.mark.parametrize("budget", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("length", LENGTHS)
def test_queries_meet_their_conditions(length, budget):
    """Shares of ties, unique hits at a distance and misses; and for every position group of the index built for this
    budget, a unique hit and a tie that only that group can find (every other group holds a mismatch)."""
    pool, queries = pool_and_queries(length, budget)
    assert 50 <= len(pool) <= 150 and len(set(pool)) == len(pool)
    miss = mismatch_table(pool, queries)
    dist = miss.sum(axis=2)
    best = dist.min(axis=1)
    at_best = dist == best[:, None]
    within = best <= budget
    ties = within & (at_best.sum(axis=1) > 1)
    hits = within & (at_best.sum(axis=1) == 1) & (best >= 1)
    n = len(queries)
    assert ties.sum() >= 0.25 * n, ("ties", int(ties.sum()), n)
    assert hits.sum() >= 0.25 * n, ("unique hits at a distance", int(hits.sum()), n)
    assert (~within).sum() >= 0.10 * n, ("misses", int((~within).sum()), n)
    assert (best[~within] == budget + 1).sum() >= 0.10 * n, "misses one substitution beyond the cap"
    for d in range(1, budget + 1):
        assert (hits & (best == d)).any() and (ties & (best == d)).any(), d
    assert any(set(q.upper()) - set("ACGT") for q in queries) and any(q != q.upper() for q in queries)
    groups = gen.position_groups(length, budget)
    masks = np.zeros((len(groups), length), dtype=bool)
    for g, members in enumerate(groups):
        masks[g, sorted(members)] = True
    # intact[query, entry, group]: no mismatch of that entry inside the group
    intact = ~(miss[:, :, None, :] & masks[None, None, :, :]).any(axis=3)
    alone = intact.sum(axis=2) == 1
    for g in range(len(groups)):
        only_g = alone & intact[:, :, g] & at_best             # an entry at the minimum that only group g reaches
        assert (only_g.any(axis=1) & hits).any(), ("no unique hit for group", g)
        assert (only_g.any(axis=1) & ties).any(), ("no tie for group", g)


def test_short_pools_stay_in_three_bases():
    """(what makes a miss possible at 8 bases and a cap of 5: a T in a query mismatches every entry)"""
    pool, _ = pool_and_queries(8, 5)
    assert all(set(s) <= set("ACG" + "MSR") for s in pool)
    pool, _ = pool_and_queries(20, 5)
    assert any("T" in s for s in pool)


def test_iupac_entries_only_up_to_64_bases():
    for length in gen.CROWDED_MATCH_LENGTHS:
        pool, _ = pool_and_queries(length, 2)
        assert any(set(s) - set("ACGT") for s in pool) == (length <= 64), length


DUAL_CELLS = [((12, 10), (1, 1)), ((12, 10), (2, 3)), ((12, 10), (4, 4)), ((40, 36), (1, 1)), ((40, 36), (2, 3)), ((40, 36), (4, 4)),
              ((100, 70), (2, 2))]


@pytest.mark.parametrize("lens,budgets", DUAL_CELLS, ids=lambda v: "-".join(map(str, v)))
def test_dual_cases_hold_both_regimes_and_every_pair_outcome(lens, budgets):
    """Mate 1: five or more distinct barcodes within the cap for a good share of the pairs (pair_match's neighbour arrays
    overflow); mate 2: never more than four, so that pairs whose mate 1 stays within four run the crossed arrays.  The valid
    pairs are a strict subset of the cross product, and there are pairs with a unique best valid pair, with a tie between two
    valid pairs, and with nothing but invalid pairs within the caps."""
    case = gen.crowded_dual_case(gen.CROWDED_SEED, lens, budgets, False, True)
    u1, u2 = list(dict.fromkeys(case["pool1"])), list(dict.fromkeys(case["pool2"]))
    rows = list(zip(case["pool1"], case["pool2"]))
    assert len(set(rows)) == len(rows) < len(u1) * len(u2)
    assert len(u1) < len(rows) and len(u2) < len(rows)                       # barcodes recur over the rows
    d1 = mismatch_table(u1, [a for a, _ in case["probes"]]).sum(axis=2)
    d2 = mismatch_table(u2, [b for _, b in case["probes"]]).sum(axis=2)
    n1, n2 = (d1 <= budgets[0]).sum(axis=1), (d2 <= budgets[1]).sum(axis=1)
    n = len(case["probes"])
    assert n2.max() <= 4
    # (shares: a twentieth of 1 500 pairs is 75 pairs per regime, enough for every strand, swap and flank count to occur in each)
    assert ((n1 >= 5) & (n2 >= 1)).sum() >= 0.05 * n, "overflow into the nested search"
    assert ((n1 >= 1) & (n1 <= 4) & (n2 >= 1)).sum() >= 0.05 * n, "crossed arrays"
    r1 = np.array([u1.index(a) for a, _ in rows])
    r2 = np.array([u2.index(b) for _, b in rows])
    total = np.where((d1[:, r1] <= budgets[0]) & (d2[:, r2] <= budgets[1]), d1[:, r1] + d2[:, r2], 10 ** 6)
    best = total.min(axis=1)
    found = best < 10 ** 6
    tied = (total == best[:, None]).sum(axis=1) > 1
    assert (found & ~tied).sum() >= 0.05 * n, "a unique best valid pair"
    assert (found & tied).sum() >= 0.03 * n, "a tie between two valid pairs"
    assert (~found & (n1 >= 1) & (n2 >= 1)).sum() >= 0.03 * n, "only invalid pairs within the caps"


@pytest.mark.parametrize("lens", [(12, 12), (20, 20), (50, 50)], ids=lambda v: str(sum(v)))
def test_dual_single_end_rows_share_barcodes(lens):
    case = gen.crowded_dual_single_end_case(gen.CROWDED_SEED, lens, 3)
    rows = list(zip(*case["pools"]))
    assert len(set(rows)) == len(rows)
    assert all(len(set(col)) < len(rows) for col in case["pools"])


@pytest.mark.parametrize("name", MATCH_NAMES)
def test_oracle_equals_brute_force(oracle, name):
    case = G.crowded(name)[0]
    idx, mm = oracle.match_barcodes(case["sequences"], case["choices"], case["substitutions"], case["reverse"])
    exp = brute_match(case["choices"], case["sequences"], case["substitutions"], case["reverse"])
    assert np.array_equal(idx, exp[0]) and np.array_equal(mm, exp[1])


@pytest.mark.parametrize("name", list(gen.crowded_golden_cases()))
def test_oracle_equals_kaori(oracle, name):
    """match, single and combo: the outputs of real kaori on the same seeded inputs."""
    case, expect = G.crowded(name)
    assert normalise(run_oracle(oracle, case)) == normalise(expect)
