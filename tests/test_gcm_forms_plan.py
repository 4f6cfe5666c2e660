"""CPU: the host-only model and plan of tests/gcm_forms.py, which
tests/test_gcm_form_edges_gpu.py runs on the device.  What the plan promises
is asserted here, from the plan alone: every boundary class meets every AAD
length and every GHASH length of gcm_cases.py for which it exists, every
geometry is one the library accepts, no two mapped bytes collide, and the
comparison reports a wrong byte on either side of every class's boundary and
in a guard.  No GPU, nothing from the library."""
from __future__ import annotations

import numpy as np
import pytest

import gcm_cases
import gcm_forms as F


def _rand(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def test_the_two_mappings_are_the_formulas():
    for off, c, stride, slots in ((0, 7, 7, 3), (5, 16, 53, 2), (2**33 * 40 + 11, 10, 10, 4), ((2**33 + 5) * 3003 + 2999, 1001, 1038, 3)):
        got = F.window_positions(50, off, c, stride, slots)
        assert got.tolist() == [((x // c) % slots) * stride + x % c for x in range(off, off + 50)]
    for off, n in ((0, 9), (8, 9), (5, 30)):
        assert F.ring_positions(n, off, 30).tolist() == [(off + o) % 30 for o in range(n)]


def test_lane_blocks_replays_the_kernel_loops():
    """Hand-worked frames.  300 whole blocks, no AAD: lanes 0 .. 43 take
    (l, l + 256) as a pair, lanes 44 .. 255 one block in the tail loop.  512
    whole blocks: every block in a pair, the tail loop takes the length block
    alone.  257 AAD blocks: lane 0 does AAD blocks 0 and 256 and then, in the
    tail loop (`i >= na` fails the pair loop's entry), payload block 255."""
    first, second, tail = F.lane_blocks(0, 300 * 16)
    assert first == tuple(range(44)) and second == tuple(range(256, 300)) and tail == tuple(range(44, 256))
    first, second, tail = F.lane_blocks(0, 512 * 16)
    assert first == tuple(range(256)) and second == tuple(range(256, 512)) and tail == ()
    first, second, tail = F.lane_blocks(0, 512 * 16 - 1)  # the partial block 511 is no pair's second block
    assert 255 in tail and 511 in tail and 255 not in first
    first, second, tail = F.lane_blocks(257, 16 * 511)  # m = 769
    assert 255 in tail and 255 not in first and 0 in first  # lane 1: AAD 1, then the pair (0, 256)
    assert "pair-to-tail" not in F.payload_cuts(0, 512 * 16, 0)
    assert F.payload_cuts(0, 300 * 16, 0)["pair-to-tail"] // 16 == 44
    assert F.payload_cuts(3, 300 * 16, 0)["second-pass"] // 16 == 253


def _exists(plan, classes_of):
    """{class: (the AAD lengths, the m) of the cases for which it exists}."""
    out = {}
    for p in plan:
        for cls in classes_of(p):
            a, m = out.setdefault(cls, (set(), set()))
            a.add(p.job.aad_len)
            if p.m in gcm_cases.SEQ_LENS:
                m.add(p.m)
    return out


def _coverage(plan):
    """The coverage conditions of a plan."""
    assert [p.i for p in plan] == list(range(len(gcm_cases.lane_cases())))
    for form, pick, classes_of, names in (
            ("window", lambda p: p.windows[0], lambda p: ["none"] + list(F.window_cuts(p.na, len(p.job.pt), p.i)),
             F.WINDOW_CLASSES),
            ("ring", lambda p: p.rings[0], lambda p: list(F.ring_cuts(p.na, len(p.job.pt), p.i)), F.RING_CLASSES)):
        exists = _exists(plan, classes_of)
        assert set(exists) == set(names), form
        met_a, met_m = {}, {}
        for p in plan:
            g = pick(p)
            assert g.cls in classes_of(p), (form, p.i, g.cls)
            met_a.setdefault(g.cls, set()).add(p.job.aad_len)
            met_m.setdefault(g.cls, set()).add(p.m)
        for cls in names:
            assert met_a[cls] >= exists[cls][0], (form, cls, "AAD lengths never met", sorted(exists[cls][0] - met_a[cls]))
            assert met_m[cls] >= exists[cls][1], (form, cls, "m never met", sorted(exists[cls][1] - met_m[cls]))
    # classes that exist for every case and every value
    ex = _exists(plan, lambda p: F.window_cuts(p.na, len(p.job.pt), p.i))
    for cls in ("nonce", "header-end", "last-block", "tag", "slot-wrap"):
        assert ex[cls] == (set(gcm_cases.AAD_LENS), set(gcm_cases.SEQ_LENS)), cls
    # second-pass needs sequence block 256 to be a payload block: m >= 258 and na <= 256
    assert ex["second-pass"][0] == set(gcm_cases.AAD_LENS) - {4101}
    assert ex["second-pass"][1] == {m for m in gcm_cases.SEQ_LENS if m >= 258}
    assert ex["pair-to-tail"][0] == set(gcm_cases.AAD_LENS) and ex["pair-to-tail"][1] == set(gcm_cases.SEQ_LENS)
    # `none` (ring) and `many` (window) for every case; thinning may drop a case's `many`, nothing else
    assert all(p.rings[1].cls == "none" and p.rings[1].cut == 0 for p in plan)
    assert all(p.windows[1] is None or p.windows[1].cls == "many" for p in plan)
    # the odd stride pad and the large period count meet every class
    for cls in F.WINDOW_CLASSES + ("many",):
        ws = [w for p in plan for w in p.windows if w is not None and w.cls == cls]
        assert {w.pad for w in ws} == set(F.PADS), cls
        assert {w.periods for w in ws} == set(F.PERIODS), cls
        assert any(w.pad % 2 and w.periods == F.PERIODS[2] for w in ws), cls


def test_plan_coverage():
    plan = F.lane_plan()
    _coverage(plan)
    assert all(p.windows[1] is not None for p in plan)  # `many` for every case
    assert {p.job.aad_len for p in plan} == set(gcm_cases.AAD_LENS)
    assert {p.m for p in plan} >= set(gcm_cases.SEQ_LENS)


@pytest.mark.parametrize("k", (2, 3, 5))
def test_a_thinned_plan_keeps_every_condition(k):
    """many_every = k drops the `many` window of the other cases and nothing else."""
    plan, full = F.lane_plan(k), F.lane_plan()
    _coverage(plan)
    assert [p.windows[0] for p in plan] == [p.windows[0] for p in full] and [p.rings for p in plan] == [p.rings for p in full]
    assert [p.windows[1] is not None for p in plan] == [p.i % k == 0 for p in plan]
    assert {p.job.aad_len for p in plan if p.windows[1]} == set(gcm_cases.AAD_LENS)


def _block_of(frame_off: int) -> int:
    return (frame_off - 12) // 16


def test_every_geometry_is_valid_and_cut_where_its_class_says():
    for p in F.lane_plan():
        n, fs = len(p.job.pt), p.job.frame_size
        span, nb = n + 28, (n + 15) // 16
        tail = F.lane_blocks(p.na, n)[2]
        for w in p.windows:
            assert F.window_valid(w, n, fs), (p.i, w)
            cuts = F.boundaries(w, span)
            at = F.window_positions(span, w.stream_off, w.chunk, w.stride, w.slots)
            assert np.unique(at).size == span and at.max() < w.slots * w.stride, (p.i, w)
            slot = at // w.stride
            if w.cls == "none":
                assert cuts == [] and w.cut == 0 and (np.diff(at) == 1).all()
                continue
            if w.cls == "many":
                assert 985 <= w.chunk <= 1016 and w.chunk % 16 and len(cuts) >= 1 and len(cuts) >= span // w.chunk
                if span > 3 * w.chunk:  # long enough to reach the last slot wherever it starts
                    assert (np.diff(slot) < 0).any(), "the frame never wraps to slot 0"
                continue
            assert cuts == [w.cut], (p.i, w, cuts)
            b, wraps = w.cut, bool((np.diff(slot) < 0).any())
            assert wraps == (w.cls == "slot-wrap"), (p.i, w)
            if w.cls == "slot-wrap":
                assert w.slots == 2 and slot[b - 1] == 1 and slot[b] == 0
            elif w.cls == "nonce":
                assert 1 <= b <= 11
            elif w.cls == "header-end":
                assert b == 12
            elif w.cls == "tag":
                assert 12 + n < b < span
            elif w.cls == "second-pass":
                assert _block_of(b) == _block_of(b - 1) == 256 - p.na and 0 <= 256 - p.na < nb
            elif w.cls == "pair-to-tail":
                assert _block_of(b) == _block_of(b - 1) == tail[0]
            elif w.cls == "last-block":
                assert _block_of(b) == nb - 1 and b < 12 + n
                assert _block_of(b - 1) == nb - 1 or n % 16 in (0, 1)  # on its start: a whole or a one-byte block
            else:
                raise AssertionError(w.cls)
        for r in p.rings:
            assert F.ring_valid(r, [n]), (p.i, r)
            at = F.ring_positions(n, r.ring_off, r.ring_bytes)
            assert np.unique(at).size == n
            wrapped = bool((np.diff(at) < 0).any())
            if r.cls in ("none", "end"):
                assert not wrapped
                assert r.cls == "none" or at[-1] == r.ring_bytes - 1
                continue
            assert wrapped and at[r.cut] == 0 and at[r.cut - 1] == r.ring_bytes - 1, (p.i, r)
            blk, inside = r.cut // 16, r.cut % 16 != 0
            if r.cls == "second-pass":
                assert inside and blk == 256 - p.na
            elif r.cls == "pair-to-tail":
                assert inside and blk == tail[0]
            elif r.cls == "last-block":
                assert blk == nb - 1 and (inside or n % 16 in (0, 1))
            elif r.cls == "block-boundary":
                assert not inside and 1 <= blk <= nb - 1
            else:
                raise AssertionError(r.cls)


def test_multi_frame_geometries():
    """The stream cases' windows: barely larger than the stream, 2^33 + 5
    periods in, every frame but the first in the second period; their rings
    wrap inside a middle frame.  The counter edge jobs are cut in a block
    that a lane takes second in a pair step."""
    for i, job in enumerate(gcm_cases.stream_cases()):
        w = F.late_window(job, i)
        assert F.window_valid(w, len(job.pt), job.frame_size)
        assert w.slots * w.chunk - job.frames_len < w.chunk and w.periods == 2**33 + 5
        assert F.second_period_frames(w, job) == job.n_frames - 1 >= 2
        r = F.middle_wrap(job, i)
        assert F.ring_valid(r, [len(job.pt)]) and 0 < r.cut // job.frame_size < job.n_frames - 1 and r.cut % 16
    assert {F.late_window(j, i).pad for i, j in enumerate(gcm_cases.stream_cases())} == set(F.PADS)
    for job in (gcm_cases.counter_edge_case(), gcm_cases.long_counter_case()):
        na, j = (job.aad_len + 15) // 16, F.counter_cut_block(job)
        first, second, _ = F.lane_blocks(na, job.frame_size)
        assert j in second and j - 256 in first and 30000 < j < job.frame_size // 16
        w = F.counter_window(job)
        assert F.window_valid(w, len(job.pt), job.frame_size) and F.boundaries(w, job.frames_len) == [w.cut]
        assert _block_of(w.cut) == _block_of(w.cut - 1) == j and w.pad % 2 and w.periods == 2**33 + 5
        w = F.counter_window(job, uncut=True)
        assert F.window_valid(w, len(job.pt), job.frame_size) and F.boundaries(w, job.frames_len) == []
        r = F.counter_ring(job)
        assert F.ring_valid(r, [len(job.pt)]) and r.cut // 16 == j and r.cut % 16
    assert gcm_cases.counter_edge_case().frame_size == 65534 * 16 and gcm_cases.long_counter_case().frame_size == 65535 * 16


@pytest.mark.parametrize("cus", (8, 256, 304))
def test_key_pass_cases_put_long_frames_under_new_keys_into_every_pass(cus):
    """One workgroup per CU takes four frames per pass: frames p * 4 * cus + t
    (t < 8) are what workgroups 0 and 1 meet in pass p.  Each is longer than
    256 GHASH blocks, so it multiplies by H^256, under another key than the
    frame the same group had one pass earlier; the rest are the tiny cases."""
    jobs, tiny = gcm_cases.key_pass_cases(cus), gcm_cases.tiny_cases(2 * 4 * cus + 37)
    assert len(jobs) == len(tiny) > 2 * 4 * cus and all(j.n_frames == 1 for j in jobs)
    heads = {4 * cus * p + t for p in range(3) for t in range(8)}
    for i, (j, t) in enumerate(zip(jobs, tiny)):
        if i in heads:
            assert (j.aad_len + 15) // 16 + (len(j.pt) + 15) // 16 + 1 >= 258 and j in gcm_cases.lane_cases()
            assert i < 4 * cus or j.key != jobs[i - 4 * cus].key
        else:
            assert j is t


def _bites(got, img, i, *names):
    """check() reports byte i of the buffer, and by one of the names."""
    got = got.copy()
    got[i] ^= 0x40
    with pytest.raises(AssertionError) as e:
        F.check(got, img, "bite")
    text = str(e.value)
    assert f"the first at {i}:" in text and any(n in text for n in names), (i, names, text)


def _field(n: int, o: int) -> str:
    return "nonce" if o < 12 else "ciphertext" if o < 12 + n else "tag"


@pytest.mark.parametrize("cls", F.WINDOW_CLASSES + ("many",))
def test_check_bites_on_either_side_of_a_window_boundary(cls):
    p = next(p for p in F.lane_plan() if cls in (p.windows[0].cls, "many"))
    w = p.windows[cls == "many"]
    n = len(p.job.pt)
    stream = _rand(n + 28, p.i)
    img = F.window_image(stream, w, p.job.frame_size, n, p.job.label)
    F.check(img.want, img)  # the image equals itself
    at = F.GUARD + F.window_positions(n + 28, w.stream_off, w.chunk, w.stride, w.slots)
    b = w.cut or (F.boundaries(w, n + 28) or [n + 27])[0]  # none: the frame's last byte and its first
    for o in (b - 1, b, 0, n + 27):
        _bites(img.want, img, int(at[o]), f"{_field(n, o)}, byte {o} of frame 0")
    for i in (0, F.GUARD - 1, img.size - F.GUARD, img.size - 1):
        _bites(img.want, img, i, "guard byte")
    mine = np.zeros(img.size, bool)
    mine[at] = True
    mine[:F.GUARD] = mine[-F.GUARD:] = True
    for i in np.flatnonzero(~mine)[[0, -1]]:
        _bites(img.want, img, int(i), "outside the job")
    if w.pad:  # between two slots
        _bites(img.want, img, F.GUARD + w.chunk, "outside the job")


@pytest.mark.parametrize("cls", F.RING_CLASSES + ("none",))
def test_check_bites_on_either_side_of_a_ring_wrap(cls):
    p = next(p for p in F.lane_plan() if cls in (p.rings[0].cls, "none"))
    r = p.rings[cls == "none"]
    n = len(p.job.pt)
    img = F.ring_image([(_rand(n, p.i), r.ring_off, p.job.frame_size, p.job.label)], r.ring_bytes)
    F.check(img.want, img)
    at = F.GUARD + F.ring_positions(n, r.ring_off, r.ring_bytes)
    for o in {max(r.cut - 1, 0), min(r.cut, n - 1), 0, n - 1}:
        _bites(img.want, img, int(at[o]), f"plaintext byte {o} (block {o // 16}) of frame 0")
    for i in (F.GUARD - 1, img.size - F.GUARD):
        _bites(img.want, img, i, "guard byte")
    free = np.setdiff1d(np.arange(F.GUARD, F.GUARD + r.ring_bytes), at)
    assert free.size  # every planned ring has slack
    _bites(img.want, img, int(free[0]), "ring byte", "outside the job")


def test_check_names_the_first_of_several_and_the_plaintext_buffer():
    img = F.plaintext_image(_rand(100, 1), 64, "a job")
    got = img.want.copy()
    got[F.GUARD + 70] ^= 1
    got[F.GUARD + 99] ^= 1
    with pytest.raises(AssertionError, match=r"2 bytes differ.*plaintext byte 6 \(block 0\) of frame 1"):
        F.check(got, img)
    assert (img.initial[F.GUARD:-F.GUARD] == 0x5A).all() and (img.initial[:F.GUARD] == F.GUARD_BYTE).all()
    with pytest.raises(AssertionError, match="collide"):
        img.place(b"x", np.array([5]), 64, 1, "another")
