"""CPU: the planner of GenotypeStore.read_windows (store.plan_windows) against brute force.  Every selection is expanded to
(chunk, chunk byte) -> output byte and compared with the direct formula of the chunk layout (sc, vc, 2) int8, sample-major:
byte h of variant v of sample s is byte (s % sc) * vc * 2 + 2 * (v % vc) + h of chunk (v // vc, s // sc); the output of
request q holds its variants end to end from out_off[q], with no gap and no overlap."""
import numpy as np
import pytest

from haplohyped_varawareml_amd.store import plan_windows


def brute(requests, sc, vc):
    """-> (vcol, scol, chunk byte) of every output byte, and the output size"""
    vcol, scol, cbyte = [], [], []
    for s, v_lo, v_hi in requests:
        v = np.repeat(np.arange(v_lo, v_hi, dtype=np.int64), 2)
        h = np.tile(np.arange(2, dtype=np.int64), max(v_hi - v_lo, 0))
        vcol.append(v // vc)
        scol.append(np.full(v.size, s // sc, np.int64))
        cbyte.append((s % sc) * vc * 2 + 2 * (v % vc) + h)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
    return cat(vcol), cat(scol), cat(cbyte)


def expand(sel, out_off, chunk_nbytes, bs, total):
    """selections -> the same three arrays indexed by output byte; -1 where no selection writes"""
    vcol = np.full(total, -1, np.int64)
    scol = np.full(total, -1, np.int64)
    cbyte = np.full(total, -1, np.int64)
    hits = np.zeros(total, np.int64)
    nblocks = -(-chunk_nbytes // bs)
    for r in sel:
        blk, lo, hi, dst = int(r["block"]), int(r["lo"]), int(r["hi"]), int(r["dst_off"])
        bsize = min(bs, chunk_nbytes - blk * bs)
        assert blk < nblocks and lo < hi <= bsize, r                         # what the kernel accepts
        q = int(r["req"])
        assert out_off[q] <= dst and dst + hi - lo <= out_off[q + 1], r        # inside its request's rows
        o = np.arange(dst, dst + hi - lo)
        hits[o] += 1
        vcol[o], scol[o] = r["vcol"], r["scol"]
        cbyte[o] = blk * bs + np.arange(lo, hi)
    return vcol, scol, cbyte, hits


def random_requests(rng, S, V, sc, vc, bs):
    reqs = [(int(rng.integers(S)), 0, 0), (int(rng.integers(S)), V, V), (S - 1, V - 1, V),        # empty, empty, last variant
            (S - 1, max(V - vc - 3, 0), V),                                  # last partial sample chunk, last partial column
            (0, 0, V), (int(rng.integers(S)), 0, 1)]                          # a whole row, a single variant
    for edge in (vc, 2 * vc, 4096, 8192, bs // 2, 3 * bs // 2):              # across chunk and block boundaries
        if 0 < edge < V:
            reqs.append((int(rng.integers(S)), max(edge - int(rng.integers(1, 40)), 0), min(edge + int(rng.integers(1, 40)), V)))
    for _ in range(12):
        a = int(rng.integers(V + 1))
        b = min(V, a + int(rng.integers(0, 3 * vc)))
        reqs.append((int(rng.integers(S)), a, b))
    return reqs


@pytest.mark.parametrize("sc", [1, 3, 64])
@pytest.mark.parametrize("vc", [4096, 8192, 12288])
@pytest.mark.parametrize("bs", [8192, 6144, 4000])
def test_plan_matches_brute_force(sc, vc, bs):
    rng = np.random.default_rng(sc * 100_003 + vc * 7 + bs)
    chunk_nbytes = sc * vc * 2
    bs = min(bs, chunk_nbytes)
    S = sc * int(rng.integers(1, 4)) + (int(rng.integers(1, sc)) if sc > 1 else 0)     # a partial last sample chunk
    V = vc * int(rng.integers(1, 3)) + int(rng.integers(1, vc))                        # a partial last chunk column
    reqs = random_requests(rng, S, V, sc, vc, bs)
    sel, out_off = plan_windows(reqs, sc, vc, bs)
    assert len(out_off) == len(reqs) + 1 and out_off[0] == 0
    assert np.array_equal(np.diff(out_off), [2 * (b - a) for _, a, b in reqs])
    total = int(out_off[-1])
    want = brute(reqs, sc, vc)
    got_vcol, got_scol, got_cbyte, hits = expand(sel, out_off, chunk_nbytes, bs, total)
    assert np.all(hits == 1), "gap or overlap in the output"
    assert np.array_equal(got_vcol, want[0]) and np.array_equal(got_scol, want[1]) and np.array_equal(got_cbyte, want[2])
    # empty requests give no selection; a chunk never goes past its column or sample chunk
    empty = {q for q, (_, a, b) in enumerate(reqs) if b <= a}
    assert not empty & set(sel["req"].tolist())
    assert np.all(sel["vcol"] <= (V - 1) // vc) and np.all(sel["scol"] <= (S - 1) // sc)


def test_plan_default_geometry_row():
    """the default chunk (64 x 8192 x 2, 8 KiB blocks): one sample's row of a column is two whole blocks, 16-byte aligned"""
    sel, out_off = plan_windows([(70, 0, 3 * 8192)], 64, 8192, 8192)
    assert out_off.tolist() == [0, 6 * 8192]
    assert sel["block"].tolist() == [12, 13] * 3 and sel["vcol"].tolist() == [0, 0, 1, 1, 2, 2]
    assert np.all(sel["scol"] == 1) and np.all(sel["lo"] == 0) and np.all(sel["hi"] == 8192)
    assert sel["dst_off"].tolist() == [i * 8192 for i in range(6)]


def test_plan_empty():
    sel, out_off = plan_windows([], 64, 8192, 8192)
    assert len(sel) == 0 and out_off.tolist() == [0]
    sel, out_off = plan_windows([(3, 5, 5), (1, 9, 2)], 64, 8192, 8192)
    assert len(sel) == 0 and out_off.tolist() == [0, 0, 0]
