"""No GPU: the 16-bit halves of the bit-plane LZ4 coder's packed pairs (csrc/lz4bits.hip, bp_extend_and_price) are exact.

The extension loop of the chosen candidate holds the one's side and the candidate's side of a position as the two halves of one
register, (pa, pb), takes both steps with one packed subtraction, d = (ga + 1, gb + 1), and reads what the loop used to add up
off its state afterwards: the steps taken telescope to pa - q1, the last step's gaps are the d the lane stopped at, the step
counter is the one's index.  Here (1) the bounds that make 16 bits enough are derived from the source's own constants, and
(2) that loop is run in numpy with uint16 wrap-around against the loop it replaced in int64 — the statement of
tools/sim/gapenc_ref.c — on 10^5 random (one, candidate) pairs and on every pair of the crafted planes of
tests/lz4_pk16_cases.py; every value that leaves the loop must agree everywhere."""
import numpy as np

from tests.lz4_pk16_cases import N, coder_constants, named_planes, one_list

K = coder_constants()
PICK, STEPS, TMIN = K["BP_PICK"], K["BP_STEPS"], K["BP_TMIN"]
WIDTH = K["BP_MAXONES"] + 8          # entries of P in LDS (BpLds::P)


def test_constants_are_the_ones_the_bounds_were_written_for():
    assert K["BP_N"] == N == 4096 and K["BP_MAXONES_EXC"] <= K["BP_MAXONES"]


def test_every_packed_quantity_fits_its_half():
    p_max = K["BP_N"] + 1                         # P[j + 1] = q_j + 1 <= n; the sentinels are n + 1
    # (pa, pb) and (P[a + 1], P[b + 1]): positions.  The compiler subtracts them with v_pk_sub_i16: below 32768, so that the
    # signed reading of a half is the unsigned one
    assert p_max < 32768
    # d = (P[a + 1] - P[a], P[b + 1] - P[b]): P ascends (strictly up to the first sentinel, which a + 1 and b + 1 do not pass:
    # a <= m, b < a), so 1 <= d <= n + 1 - P[0] = n + 1
    d_max = p_max - 0
    assert 1 <= d_max < 32768
    # "ga >= 255" is taken from the high byte of d's low half: exact for every d below 65536
    assert all((((d >> 8) & 0xFF) != 0) == (d - 1 >= 255) for d in range(0, d_max + 1))
    # the doubled index a2 = 2 a and its limit are 32-bit values; a + 1 <= m + 1 stays inside P, and so does the sentinel read
    assert 2 * (K["BP_MAXONES"] + 4) < 2 ** 32 and K["BP_MAXONES"] + 2 < WIDTH
    # min(d, BP_TMIN + 1) per step, at most BP_PICK agreed gaps + BP_STEPS + 1 steps: the literal cost stays far below 65536
    assert (PICK + STEPS + 1) * (TMIN + 1) < 65536
    # the pull-back min(gq, gc, BP_BACK) and clen <= n + 1 are 32-bit values in the kernel; both are below 65536 anyway
    assert K["BP_BACK"] < 65536 and p_max + d_max < 65536


def gap_bytes(P, m):
    """[planes][WIDTH]: zeros behind the one with P-index i, clipped to 255; 255 from the last one on"""
    g = np.minimum(P[:, 1:] - P[:, :-1] - 1, 255)
    g = np.concatenate([g, np.full((P.shape[0], 1), 255, np.int64)], axis=1)
    idx = np.arange(P.shape[1])[None, :]
    return np.where(idx < m[:, None], g, 255)


def make_cases(P, m, pi, jj, jq):
    """bk of every (plane pi, one jj, candidate jq): equal gap bytes from the two ones on, at most BP_PICK, a 255 agrees with nothing"""
    GB = gap_bytes(P, m)
    bk = np.zeros(len(pi), np.int64)
    go = np.ones(len(pi), bool)
    for k in range(PICK):
        ga, gb = GB[pi, np.minimum(jj + k, WIDTH - 1)], GB[pi, np.minimum(jq + k, WIDTH - 1)]
        go &= (ga == gb) & (ga != 255)
        bk += go
    return bk


def old_loop(P, m, pi, jj, jq, bk):
    """the extension as it was written before (csrc/lz4bits.hip at the parent commit; tools/sim/gapenc_ref.c), in int64"""
    a, b = jj + bk, jq + bk
    pa, pb = P[pi, a], P[pi, b]
    q1 = P[pi, jj]
    clen, cost = pa - q1, np.zeros_like(pa)
    tailz, zl = np.zeros_like(pa), np.zeros_like(pa)
    act = np.ones(len(pi), bool)
    s = bk.copy()
    for _ in range(STEPS + 3):
        na, nb = P[pi, a + 1], P[pi, b + 1]
        ga, gb = na - pa - 1, nb - pb - 1
        stop = (s < PICK) | (ga != gb) | (ga >= 255) | (a >= m[pi]) | (s >= STEPS)
        z = np.minimum(ga, gb)
        cost += np.where(act, 1 + np.where(ga >= TMIN + 1, 4, ga), 0)
        clen += np.where(act, 1 + np.where(stop, z, ga), 0)
        tailz = np.where(act & stop, ga - z, tailz)
        zl = np.where(act & stop, z, zl)
        act = act & ~stop
        a, b = a + act, b + act
        pa, pb = np.where(act, na, pa), np.where(act, nb, pb)
        s = s + 1
    assert not act.any()
    return a, clen, cost, tailz, zl


def new_loop(P, m, pi, jj, jq, bk):
    """the extension as csrc/lz4bits.hip has it now: halves in uint16 with wrap-around, everything else in uint32"""
    u16, u32 = np.uint16, np.uint32
    P16 = P.astype(u16)                                   # what a 16-bit LDS load returns
    back2 = (2 * (jj - jq)).astype(u32)
    a2 = (2 * (jj + bk)).astype(u32)
    lim = np.minimum(m[pi], jj + STEPS)
    lim2 = np.where(bk < PICK, 0, 2 * lim).astype(u32)
    pp_lo, pp_hi = P16[pi, a2 >> 1], P16[pi, (a2 - back2) >> 1]
    dl_lo, dl_hi = np.ones(len(pi), u16), np.ones(len(pi), u16)
    cost = np.zeros(len(pi), u32)
    st2 = np.full(len(pi), 2, u32)
    for _ in range(STEPS + 3):
        act = st2 != 0
        nn_lo, nn_hi = P16[pi, (a2 + u32(2)) >> 1], P16[pi, (a2 - back2 + u32(2)) >> 1]
        d_lo, d_hi = (nn_lo - pp_lo).astype(u16), (nn_hi - pp_hi).astype(u16)     # v_pk_sub: each half modulo 65536
        word = d_lo.astype(u32) | (d_hi.astype(u32) << u32(16))
        stop = (d_lo != d_hi) | (((word >> u32(8)) & u32(0xFF)) != 0) | (a2 >= lim2)
        cost += np.where(act, np.minimum(d_lo, u16(TMIN + 1)), 0).astype(u32)
        dl_lo, dl_hi = np.where(act, d_lo, dl_lo), np.where(act, d_hi, dl_hi)
        st2 = np.where(stop, u32(0), st2)
        a2 = a2 + st2
        pp_lo, pp_hi = np.where(st2 != 0, nn_lo, pp_lo), np.where(st2 != 0, nn_hi, pp_hi)
    assert not (st2 != 0).any()
    z1 = np.minimum(dl_lo, dl_hi).astype(u32)
    q1 = P[pi, jj].astype(u32)
    clen = pp_lo.astype(u32) - q1 + z1
    return (a2 >> 1).astype(np.int64), clen.astype(np.int64), cost.astype(np.int64), (dl_lo.astype(u32) - z1).astype(np.int64), (z1 - 1).astype(np.int64)


def compare(P, m, pi, jj, jq):
    bk = make_cases(P, m, pi, jj, jq)
    assert ((jj + bk) <= m[pi]).all()                     # the first open comparison starts at a real one (or the last)
    old, new = old_loop(P, m, pi, jj, jq, bk), new_loop(P, m, pi, jj, jq, bk)
    for name, o, n_ in zip(("a_last", "clen", "costR", "tailz", "z_last"), old, new):
        bad = np.flatnonzero(o != n_)
        assert bad.size == 0, f"{name}: {bad.size} of {len(pi)} pairs differ, first: plane {pi[bad[0]]}, one {jj[bad[0]]}, candidate {jq[bad[0]]}"
    return bk, old


def random_planes(rng, n):
    """sparse, dense, periodic with defects, long gaps (>= 255, thousands), ones at both ends: at most BP_MAXONES ones each"""
    out = []
    for k in range(n):
        kind = k % 5
        if kind == 0:
            a = rng.random(N) < rng.choice([0.002, 0.01, 0.05, 0.12])
        elif kind == 1:      # a period with a few defects
            per = int(rng.integers(2, 60))
            a = np.zeros(N, bool)
            start = int(rng.integers(0, N // 2))
            a[start:start + per * 300:per] = True
            a[rng.integers(0, N, 3)] ^= True
        elif kind == 2:      # motifs around gaps of 250-260 zeros
            a = np.zeros(N, bool)
            p = int(rng.integers(0, 5))
            while p < N:
                a[p] = True
                p += 1 + int(rng.choice([1, 2, 3, 254, 255, 256, 257])) if rng.random() < 0.5 else 1 + int(rng.integers(0, 6))
        elif kind == 3:      # a cluster at either end, nothing in between
            a = np.zeros(N, bool)
            a[:200] = rng.random(200) < 0.3
            a[N - 200:] = a[:200] if k % 2 else rng.random(200) < 0.3      # (the same cluster again: gaps of thousands between candidates)
            a[0] = a[N - 1] = True
        else:
            a = rng.random(N) < 0.08
            a[int(rng.integers(0, N)):] = False
        q = np.flatnonzero(a)
        if len(q) > K["BP_MAXONES"]:
            a[q[K["BP_MAXONES"]:]] = False
        out.append(a.astype(np.uint8))
    return out


def lists_of(planes):
    Pm = [one_list(pl, WIDTH) for pl in planes]
    return np.stack([p for p, _ in Pm]), np.array([m_ for _, m_ in Pm], np.int64)


def test_extension_in_halves_equals_the_extension_in_int64_on_random_pairs():
    rng = np.random.default_rng(13)
    P, m = lists_of(random_planes(rng, 500))
    ok = np.flatnonzero(m >= 2)
    pi = rng.choice(ok, 100_000)
    jj = (2 + rng.random(len(pi)) * (m[pi] - 1)).astype(np.int64)           # P-index of the one: 2 .. m
    near = rng.random(len(pi)) < 0.7                                        # most candidates are recent ones
    back = np.where(near, rng.integers(1, 8, len(pi)), (rng.random(len(pi)) * (jj - 1)).astype(np.int64) + 1)
    jq = np.maximum(jj - back, 1)
    assert len(pi) == 100_000 and (jq < jj).all() and (jq >= 1).all() and (jj <= m[pi]).all()
    bk, old = compare(P, m, pi, jj, jq)
    # the pairs really take the loop's paths: every bk, extensions past the third gap and to the step limit, stops at the last one
    assert all((bk == k).sum() > 100 for k in range(PICK + 1))
    a_last = old[0]
    assert (a_last - jj > PICK).sum() > 100 and (a_last - jj == STEPS).sum() > 10 and (a_last == m[pi]).sum() > 10


def test_extension_in_halves_equals_the_extension_in_int64_on_the_crafted_planes():
    named = named_planes()
    P, m = lists_of([named[k] for k in sorted(named)])
    pi, jj, jq = [], [], []
    for i in range(len(m)):
        for j in range(2, int(m[i]) + 1):
            for c in {j - 1, j - 2, j - 3, j - 4, j - 7, 1}:      # the nearest earlier ones, one further away, the first
                if 1 <= c < j:
                    pi.append(i), jj.append(j), jq.append(c)
    pi, jj, jq = (np.array(x, np.int64) for x in (pi, jj, jq))
    assert len(pi) > 30_000
    compare(P, m, pi, jj, jq)


def test_cost_of_the_agreed_gaps_masked_once():
    """bk + the sum of min(gap, BP_TMIN) over the gap bytes below bk (masked once) = the sum of 1 + (gap >= BP_TMIN + 1 ? 4 : gap)
    over s < bk (one select per gap), for every bk and every gap byte"""
    rng = np.random.default_rng(5)
    a4 = rng.integers(0, 2 ** 32, 200_000, dtype=np.uint64).astype(np.uint32)
    a4[:4096] = (np.arange(4096) % 16 * 0x01010101 + np.arange(4096) // 16).astype(np.uint32)    # small gaps, where the min bites
    for bk in range(PICK + 1):
        old = np.zeros(len(a4), np.int64)
        for s in range(PICK):
            g = ((a4 >> np.uint32(8 * s)) & np.uint32(0xFF)).astype(np.int64)
            old += np.where(s < bk, 1 + np.where(g >= TMIN + 1, 4, g), 0)
        am = a4 & np.uint32((1 << (8 * bk)) - 1)
        new = np.full(len(a4), bk, np.int64)
        for s in range(PICK):
            new += np.minimum(((am >> np.uint32(8 * s)) & np.uint32(0xFF)).astype(np.int64), TMIN)
        assert np.array_equal(old, new), bk
