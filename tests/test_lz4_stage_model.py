"""CPU: the Python statement of the bit-plane LZ4 coder's batching (tests/lz4_stage_model.py: windows of 64 ones, a batch when 65
entries are queued, 64 per batch, the staging area) against examples worked by hand, and against the parse it lays out
(tests/lz4_pk16_cases.gapenc_model, tools/sim/gapenc_ref.c in Python): the same bytes.  tests/test_gpu_lz4_stage_paths.py trusts
this statement for what a crafted plane is a case of; it is only as strong as the examples here.

The hand-worked planes are coded without candidates (depth 0), where the parse can be read off the plane: every one is coded,
and a one with at least 5 zeros behind it queues one entry — the literals since the last sequence up to and with the first of
those zeros (an offset-1 run copies the byte in front of it), then the other zeros, at least BP_TMIN = 4, as the run: 3 bytes +
the literals + one extension byte from 20 zeros on (a run of 19: match length 15 + 4)."""
import numpy as np
import pytest

from tests.lz4_pk16_cases import LAZY, MISSING, N, gapenc_model
from tests.lz4_stage_model import MATCHLIMIT, cases_of, expected_cases, len_ext, spec_plane, stage_constants, stage_model

K = stage_constants()


def ones_at(pos, missing=()):
    a = np.zeros(N, np.uint8)
    a[list(pos)] = 1
    a[list(missing)] = MISSING
    return a


def test_constants_are_the_kernels():
    assert (K["BP_QCAP"], K["BP_STAGE"], K["BP_QCAP_EXC"], K["BP_STAGE_EXC"]) == (80, 240, 80, 104)
    assert [len_ext(x) for x in (0, 14, 15, 269, 270, 4091)] == [0, 0, 1, 1, 2, 16]


def test_one_one_is_one_window_one_batch_of_two_entries():
    """a one at 100: the virtual one queues the run over bytes 1..99 (literal: byte 0; 99 zeros: 3 + 1 + 1 bytes), the one at 100
    the run from 102 to the match limit 4091 (literals: bytes 100 and 101; length 3989: 3 + 2 + 16 bytes)"""
    stream, windows, batches = stage_model(ones_at([100]), 0, K)
    assert len(windows) == 1 and windows[0]["valid"] == 2 and windows[0]["coded"] == [0, 1] and windows[0]["last"]
    assert (windows[0]["qn_before"], windows[0]["nw"], windows[0]["qn_queued"]) == (0, 2, 2)
    assert len(batches) == 1
    b = batches[0]
    assert (b["n"], b["qn"], b["sop"], b["total"], b["flushed"], b["direct"], b["make_room"]) == (2, 2, 0, 5 + 21, False, False, False)
    assert [e["ll1"] for e in b["entries"]] == [1, 2] and not any(e["on2"] for e in b["entries"])
    # token 0x1F, literal 0, offset 1, length 99 - 4 - 15 = 80; token 0x2F, literals 1 0, offset 1, 3989 - 4 - 15 = 15 x 255 + 145; last 5 literals
    want = [0x1F, 0, 1, 0, 80] + [0x2F, 1, 0, 1, 0] + [255] * 15 + [145] + [0x50, 0, 0, 0, 0, 0]
    assert stream.tolist() == want


def spaced(m, gap=9, start=0):
    return ones_at([start + k * (gap + 1) for k in range(m)])


@pytest.mark.parametrize("m,want", [
    # m ones 10 apart from byte 0 on: no entry of the virtual one (no zeros behind it), one of 5 bytes per one (the last: 19 or 20)
    (63, dict(windows=1, batches=[(63, 63, True)], queued=[63])),
    (64, dict(windows=2, batches=[(64, 64, True)], queued=[63, 64])),          # one 63 is the second window's only one; 64 entries leave at the end
    (65, dict(windows=2, batches=[(64, 65, True), (1, 1, False)], queued=[63, 65])),     # 65 queued: a batch of 64 leaves, the last entry alone behind it
    # 63 + 64 would not fit the queue of 80: 62 leave first (one stays: the batch's last entry needs its successor), then 1 + 64 queued
    (129, dict(windows=3, batches=[(62, 63, True), (64, 65, True), (3, 3, False)], queued=[63, 65, 3]))])
def test_evenly_spaced_ones(m, want):
    stream, windows, batches = stage_model(spaced(m), 0, K)
    assert len(windows) == want["windows"]
    assert [w["qn_queued"] for w in windows][:len(want["queued"])] == want["queued"][:len(windows)]
    assert [(b["n"], b["qn"], b["direct"]) for b in batches] == want["batches"]
    assert all(w["coded"] == list(range(w["valid"])) for w in windows)          # without candidates every one is coded
    last_run = MATCHLIMIT - (10 * (m - 1) + 2)
    for b in batches:
        assert b["total"] == 5 * b["n"] + (len_ext(last_run - 4) if b is batches[-1] else 0)   # (the plane's last run reaches the match limit)
    assert batches[0]["direct"] == (batches[0]["total"] > K["BP_STAGE"])


def test_window_two_makes_room_when_the_queue_would_overflow():
    """window 0: the virtual one and 16 ones 10 apart (16 entries), then 47 ones 2 apart, which queue nothing (one zero behind
    them) — but the last of them has 9: 17 entries.  Window 1: 64 ones 10 apart: 17 + 64 = 81 > 80, so a batch of 16 leaves first
    (80 bytes, staged at 0), the 65 queued send 64 off (flushed first, then direct), and the end takes the last one"""
    pos = [k * 10 for k in range(16)] + [160 + 2 * k for k in range(47)]
    pos += [pos[-1] + 10 * (k + 1) for k in range(64)]
    stream, windows, batches = stage_model(ones_at(pos), 0, K)
    assert [(w["qn_before"], w["nw"], w["qn_queued"]) for w in windows] == [(0, 17, 17), (17, 64, 65)]
    assert [(b["make_room"], b["n"], b["qn"]) for b in batches] == [(True, 16, 17), (False, 64, 65), (False, 1, 1)]
    assert (batches[0]["sop"], batches[0]["total"], batches[0]["direct"], batches[0]["flushed"]) == (0, 80, False, False)
    assert (batches[1]["sop"], batches[1]["direct"], batches[1]["flushed"]) == (80, True, True)
    # the entry behind the 47 close ones carries their literals: bytes 160 .. 253, since the run in front ended at byte 159
    assert batches[1]["entries"][0]["ll1"] == 94 and batches[1]["total"] == 3 + 1 + 94 + 63 * 5
    assert batches[2]["sop"] == 0 and not batches[2]["direct"]
    cs = cases_of(ones_at(pos), windows, batches, K)
    assert {"queue_over_by_one", "queue_65_at_window_end", "staged_at_0", "last_window_one_entry", "ones_127"} <= cs
    assert "queue_fits_exactly" not in cs and "staged_behind" not in cs


def test_a_batch_that_fills_the_staging_area_and_one_byte_more_goes_direct():
    """one batch: 45 ones 10 apart from byte 0 on are 45 x 5 bytes, and the last one's run, from 442 to the match limit, has 15
    extension bytes (length 3649 = 4 + 15 + 14 x 255 + 60): 240 — staged.  The last one 11 further: the run in front of it covers
    19 zeros, one extension byte more: 241 — direct"""
    pos = [10 * k for k in range(45)]
    a = ones_at(pos)
    stream, windows, batches = stage_model(a, 0, K)
    assert len(batches) == 1 and (batches[0]["n"], batches[0]["total"], batches[0]["direct"]) == (45, 240, False)
    assert "total_fills_stage" in cases_of(a, windows, batches, K)
    pos[-1] += 11
    b = ones_at(pos)
    stream, windows, batches = stage_model(b, 0, K)
    assert (batches[0]["total"], batches[0]["direct"]) == (241, True)
    assert "total_one_more_direct" in cases_of(b, windows, batches, K)


def test_missing_calls_take_the_smaller_area_and_show_in_the_literals():
    """ones at 10, 12, 14 (the last a missing call) and nothing else: the virtual one's run covers bytes 1..9, the three ones are
    coded alone and only the last has zeros behind it: its entry carries the literals 10..15 — 1 0 1 0 F7 0: a 0xF7 at position 4"""
    a = ones_at([10, 12], missing=[14])
    stream, windows, batches = stage_model(a, 0, K)
    e = batches[0]["entries"]
    assert [x["ll1"] for x in e] == [1, 6] and e[1]["lits"] == [1, 0, 1, 0, MISSING, 0]
    cs = cases_of(a, windows, batches, K)
    assert {"f7_at_4", "lit_run_1", "lit_run_6", "ones_3"} <= cs and not cs & {"f7_at_%d" % k for k in (0, 1, 2, 3, 5)}
    # 3 + 1 bytes, then 3 + 6 + the 16 extension bytes of a run of 4075
    assert batches[0]["total"] == 4 + 25 and not batches[0]["direct"]


@pytest.mark.parametrize("depth", [0, 2, 2 | LAZY, 12, 12 | LAZY])
def test_the_layout_gives_the_parses_bytes(depth):
    """random planes of the bench's kind and denser, with and without missing calls: the batches' bytes are gapenc_model's"""
    rng = np.random.default_rng(depth + 1)
    for i in range(10):
        a = (rng.random(N) < (0.03, 0.065, 0.1, 0.13)[i % 4]).astype(np.uint8)
        if i % 2:
            a[np.flatnonzero(a)[i % 5::5]] = MISSING
        want, _ = gapenc_model(a, depth, K)
        got = stage_model(a, depth, K)
        assert (want is None) == (got is None)
        if want is not None:
            assert np.array_equal(got[0], want)
            assert sum(b["n"] for b in got[2]) == sum(w["nw"] for w in got[1])


def test_expected_cases_name_what_a_depth_cannot_show():
    assert "window_all_coded" in expected_cases("plain", 0) and "reach_16" not in expected_cases("plain", 0)
    assert "f7_at_3" in expected_cases("missing", 12) and "f7_at_3" not in expected_cases("plain", 12)
    assert spec_plane(("r", 7, 65, 4096), "plain").sum() == 65
