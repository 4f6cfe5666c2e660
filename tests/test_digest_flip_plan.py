"""CPU: the flip plan's expectations (tests/digest_flips.py) follow from
hashlib and bytes.__eq__ alone, not from the library under test.

For every object: hash each present shard with hashlib over its own length,
compare with the expected digest the plan hands to the library, drop the
mismatching shards from the input mask; fewer than k left is status -10 with
that mask, otherwise status 0 with every shard back (chunk_reader.rs:176-211).
The plan must state exactly that.  Also: the ALL bit set flips every digest
bit at least twice, BYTES touches every
digest byte, and no two shards of an object share a digest (else SWAP would
not be a mismatch).
"""
from __future__ import annotations

import hashlib
from collections import Counter

import numpy as np
import pytest

import digest_flips as df

SHAPES = {  # bits, S, last, stride, empty -- the shapes test_digest_compare_gpu.py uses, C at B's size
    "A": (df.ALL, 120, 55, 128, True),
    "B": (df.BYTES, 32 * 1024 + 64 + 17, 55, 33024, True),
}


@pytest.fixture(scope="module", params=list(SHAPES))
def plan(request):
    bits, S, last, stride, empty = SHAPES[request.param]
    return df.Plan(bits, S, last, stride, empty=empty)


def test_expectations_follow_from_hashlib(plan):
    for o, ob in enumerate(plan.objs):
        left = list(ob.present)
        for i in range(df.TOTAL):
            if not ob.present[i]:
                assert plan.expected[o, i].tobytes() == b"\xff" * 32
                assert (plan.given[o, i] == df.MISSING_FILL).all()
                continue
            got = hashlib.sha256(plan.given[o, i, :ob.lens[i]].tobytes()).digest()
            assert got == plan.digests[o, i].tobytes()
            if got != plan.expected[o, i].tobytes():
                left[i] = 0
        if sum(left) < df.K:
            assert ob.status == df.TOO_FEW, (o, ob)
            assert ob.mask == tuple(left), (o, ob)
        else:
            assert ob.status == df.OK, (o, ob)
            assert ob.mask == (1, 1, 1), (o, ob)
        assert plan.status[o] == ob.status and tuple(plan.mask[o]) == ob.mask
        assert tuple(plan.present[o]) == ob.present and tuple(plan.lens[o]) == ob.lens


def test_flipped_digests_differ_in_exactly_the_planned_bits(plan):
    for o, ob in enumerate(plan.objs):
        want = {i: 0 for i in range(df.TOTAL) if ob.present[i] and i not in ob.swap}
        for shard, bit in ob.flips:
            want[shard] ^= 1 << bit
        for i, x in want.items():
            a = int.from_bytes(plan.digests[o, i].tobytes(), "little")
            b = int.from_bytes(plan.expected[o, i].tobytes(), "little")
            assert a ^ b == x, (o, i, ob)  # bit b = bit b % 8 of byte b // 8
        if ob.swap:
            a, b = ob.swap
            assert plan.expected[o, a].tobytes() == plan.digests[o, b].tobytes()
            assert plan.expected[o, b].tobytes() == plan.digests[o, a].tobytes()


def test_digests_of_an_object_are_distinct_and_parity_is_the_oracles(plan):
    import oracle

    for o, ob in enumerate(plan.objs):
        assert len({plan.digests[o, i].tobytes() for i in range(df.TOTAL)}) == df.TOTAL, o
        if ob.lens[1] == 0:
            assert plan.digests[o, 1].tobytes() == hashlib.sha256(b"").digest()
    for o in (0, plan.n // 2, plan.n - 1):
        ob = plan.objs[o]
        data = [plan.orig[o, j, :ob.lens[j]] for j in range(df.K)]
        assert np.array_equal(oracle.encode(data, df.M, plan.S)[0], plan.orig[o, df.K, :plan.S])


def test_classes_and_shuffle(plan):
    n = Counter(ob.cls for ob in plan.objs)
    fails = 256 if plan.stride == 128 else 16
    assert n == {"FAIL": fails, "MISSING": 27, "SWAP": 6, "ONE": 16, "CLEAN": 16, "EMPTY": 2}
    assert sum(1 for ob in plan.objs if ob.cls == "MISSING" and ob.status == df.OK) == 3
    assert {ob.present.index(0) for ob in plan.objs if ob.cls == "MISSING"} == {0, 1, 2}
    bad = plan.status != df.OK
    assert bad.any() and not bad.all()
    runs = np.flatnonzero(np.diff(bad.astype(np.int8)))  # status changes along the batch: shuffled
    assert len(runs) >= 20
    assert [ob.cls for ob in df.layout(*SHAPES["A"][:3])] == [ob.cls for ob in df.layout(*SHAPES["A"][:3])]


def test_bit_sets_cover_the_digest():
    seen = Counter()
    where = {}
    for ob in df.layout(df.ALL, 120, 55):
        if ob.cls != "FAIL":
            continue
        assert len(ob.flips) == 2 and ob.flips[0][0] != ob.flips[1][0]
        for shard, bit in ob.flips:
            seen[bit] += 1
            where.setdefault(bit, set()).add(shard)
    assert set(seen) == set(range(256))
    assert all(c >= 2 for c in seen.values())
    # in different shard positions too, except b = 2 mod 3: (256 - b) % 3 == b % 3 there
    assert all(len(s) >= 2 for b, s in where.items() if b % 3 != 2)
    assert sorted(b // 8 for b in df.BYTES) == list(range(32))
    assert {b % 8 for b in df.BYTES} == set(range(8))
    flipped = sorted(bit // 8 for ob in df.layout(df.BYTES, 120, 55) if ob.cls == "FAIL" for _, bit in ob.flips)
    assert flipped == list(range(32))
    # MISSING: one bit from each quarter of the digest for every (absent, flipped) pair
    quarters = Counter()
    for ob in df.layout(df.ALL, 120, 55):
        if ob.cls == "MISSING" and ob.flips:
            (shard, bit), = ob.flips
            quarters[(ob.present.index(0), shard, bit // 64)] += 1
    assert len(quarters) == 24 and set(quarters.values()) == {1}
