"""Shared by tests/test_lz4_pk16_bounds.py (CPU) and tests/test_gpu_lz4_pk16.py (GPU): the planes on which a 16-bit half of the
bit-plane LZ4 coder's packed pairs (csrc/lz4bits.hip, bp_extend_and_price) could go wrong, and a Python statement of
tools/sim/gapenc_ref.c that also says WHY each one was coded as it was (which step stopped an extension, at what gain a match
was taken or left, ...).  The GPU test holds this statement to the C reference byte for byte before it trusts what it says
about a case.  Not a test module."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
MISSING = 0xF7
LAZY = 0x100


def coder_constants():
    """the #defines of csrc/lz4bits.hip the bounds hang on, parsed from the source"""
    src = open(os.path.join(ROOT, "haplohyped_varawareml_amd", "csrc", "lz4bits.hip")).read()
    out = {}
    for name in ("BP_N", "BP_MAXONES", "BP_MAXONES_EXC", "BP_BACK", "BP_STEPS", "BP_PICK", "BP_TMIN", "BP_MINM", "BP_GAPCLIP", "BP_LAZY_MIN"):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, re.M)
        assert m, name
        out[name] = int(m.group(1))
    return out


def one_list(plane, width):
    """P as the kernel holds it, padded to `width` entries: P[0] = 0, P[j + 1] = q_j + 1, then sentinels n + 1; and the count of ones"""
    q = np.flatnonzero(plane)
    P = np.full(width, N + 1, np.int64)
    P[0] = 0
    P[1:len(q) + 1] = q + 1
    return P, len(q)


def gapenc_model(plane, depth, K=None):
    """tools/sim/gapenc_ref.c in Python, statement for statement.  Returns (stream or None, records): one record per one that
    had a winner among its candidates, with what the extension and the pricing saw."""
    K = K or coder_constants()
    PICK, STEPS, TMIN, BACK, MINM, GAPCLIP = K["BP_PICK"], K["BP_STEPS"], K["BP_TMIN"], K["BP_BACK"], K["BP_MINM"], K["BP_GAPCLIP"]
    lazy = (depth >> 8) & 1
    depth &= 0xFF
    n = N
    inb = [int(b) for b in plane]
    if any(b > 1 and b != MISSING for b in inb):
        return None, []
    q_all = [i for i, b in enumerate(inb) if b]
    m = len(q_all)
    has_exc = any(inb[i] == MISSING for i in q_all)
    if m > K["BP_MAXONES"] or (has_exc and m > K["BP_MAXONES_EXC"]):
        return None, []
    P = [0] + [i + 1 for i in q_all] + [n + 1] * 8
    cls = [0] + [1 if inb[i] == MISSING else 0 for i in q_all] + [0] * 40
    GB = [min(P[i + 1] - P[i] - 1, 255) for i in range(m)] + [255] * 16
    tab = [0] * 64
    chain = [0] * (m + 4)
    mflimit, matchlimit = n - 12, n - 5
    E, nxt, ms, hv_, off_ = ([0] * (m + 2) for _ in range(5))
    recs = []
    for j in range(-1, m):
        q = P[j + 1] - 1
        hv = ln = nb = c = 0
        if depth > 0 and j >= 0 and q + 12 <= n:
            g1 = P[j + 2] - P[j + 1]
            idx = min(g1, GAPCLIP) ^ (63 if cls[j + 1] else 0)
            jc = tab[idx] - 1
            tab[idx] = j + 1
            chain[j] = jc
            best, bj, bk, tie = -1, -1, 0, False
            dpt = 0
            while dpt < depth and jc >= 0:
                if cls[jc + 1] == cls[j + 1]:
                    k = score = 0
                    while k < PICK and GB[j + 1 + k] == GB[jc + 1 + k] and GB[j + 1 + k] != 255 and cls[j + 2 + k] == cls[jc + 2 + k]:
                        score += GB[j + 1 + k] + 1
                        k += 1
                    score += 1 + min(GB[j + 1 + k], GB[jc + 1 + k])
                    score += min(GB[j], GB[jc], BACK)
                    if score > best:
                        best, bj, bk, tie = score, jc, k, False
                    elif score == best:
                        tie = True    # an equal candidate further away: the nearer one stays
                dpt += 1
                jc = chain[jc]
            if bj >= 0:
                jc = bj
                cc = P[jc + 1] - 1
                a, b = j + bk, jc + bk
                clen = P[a + 1] - P[j + 1]
                costR = tailz = 0
                for s in range(bk):
                    g = GB[j + 1 + s]
                    costR += 1 + (4 if g >= TMIN + 1 else g)
                s = bk
                steps = []      # (P[a + 1], P[a + 2], P[b + 1], P[b + 2]) of every step of the extension
                while True:
                    ga, gb = P[a + 2] - P[a + 1] - 1, P[b + 2] - P[b + 1] - 1
                    steps.append((P[a + 1], P[a + 2], P[b + 1], P[b + 2]))
                    costR += 1 + (4 if ga >= TMIN + 1 else ga)
                    why = ("pick" if s < PICK else "differ" if ga != gb else "ge255" if ga >= 255 else "last_one" if a + 1 >= m else
                           "steps" if s >= STEPS else "class" if cls[a + 2] != cls[b + 2] else "")
                    if why:
                        z = min(ga, gb)
                        clen += 1 + z
                        tailz = ga - z
                        break
                    clen += 1 + ga
                    a += 1
                    b += 1
                    s += 1
                gq, gc = q + 1 - P[j] - 1, cc + 1 - P[jc] - 1
                cnb = min(gq, gc, BACK)
                costH = 3 + (1 if clen + cnb >= 19 else 0) - cnb + (3 if tailz >= TMIN else tailz)
                end = min(q + clen, matchlimit)
                gain = costR - costH
                ok = end - q >= 4 and end - (q - cnb) >= MINM and q <= mflimit
                if gain > 0 and ok:
                    hv, ln, nb, c = 1, end - q, cnb, cc
                recs.append(dict(j=j, q=q, bk=bk, s_end=s, why=why, steps=steps, ga=ga, gb=gb, gq=gq, gc=gc, cnb=cnb, gain=gain, ok=ok, hv=hv,
                                 clamped=bool(hv and q + clen > matchlimit), tie=tie, clen=clen, costR=costR, tailz=tailz))
        e = q + ln if hv else q + 1
        E[j + 1], ms[j + 1], hv_[j + 1], off_[j + 1] = e, q - nb, hv, q - c
        t = j + 1
        while t < m and P[t + 1] - 1 < e:
            t += 1
        nxt[j + 1] = t
    if lazy:
        L = [0] * (m + 66)
        for i in range(m + 1):
            if (i & 63) == 63 or i + 1 > m or not hv_[i] or not hv_[i + 1] or P[i + 1] - 1 >= E[i]:
                continue
            nbi = (P[i] - 1) - ms[i]
            between = max(ms[i + 1] - P[i], 0)
            L[i] = 1 if E[i + 1] - E[i] >= K["BP_LAZY_MIN"] + nbi + between else 0
        for i in range(m + 1):
            if L[i]:
                t = 0
                while (i & 63) + t < 64 and i + t <= m and L[i + t]:
                    t += 1
                if t & 1:
                    hv_[i] = 2
        for i in range(m + 1):
            if hv_[i] == 2:
                qq = P[i] - 1
                hv_[i], E[i], ms[i], nxt[i] = 0, qq + 1, qq, i
    out = []

    def put_len(r):
        while r >= 255:
            out.append(255)
            r -= 255
        out.append(r)

    def put_seq(anchor, start, length, off):
        ll, ml = start - anchor, length - 4
        out.append((min(ll, 15) << 4) | min(ml, 15))
        if ll >= 15:
            put_len(ll - 15)
        out.extend(inb[anchor:start])
        out.extend((off & 0xFF, off >> 8))
        if ml >= 15:
            put_len(ml - 15)
    prev_end = 0
    j = -1
    while j < m:
        e = E[j + 1]
        if hv_[j + 1]:
            st = max(ms[j + 1], prev_end)
            put_seq(prev_end, st, e - st, off_[j + 1])
            prev_end = e
        rs = e + (1 if (e == 0 or inb[e - 1]) else 0)
        re_ = min(P[nxt[j + 1] + 1] - 1, matchlimit)
        zt, kn = re_ - rs, nxt[j + 1]
        nbk = 0
        if kn < m and hv_[kn + 1]:
            nbk = min((P[kn + 1] - 1) - ms[kn + 1], zt)
        if zt >= TMIN and zt - nbk >= TMIN and rs <= mflimit:
            put_seq(prev_end, rs, re_ - rs, 1)
            prev_end = re_
        j = nxt[j + 1]
    ll = n - prev_end
    out.append(min(ll, 15) << 4)
    if ll >= 15:
        put_len(ll - 15)
    out.extend(inb[prev_end:])
    return np.array(out, np.uint8), recs


# ---- the planes -------------------------------------------------------------------------------------------------------------
def _plane(pos):
    a = np.zeros(N, np.uint8)
    a[[p for p in pos if 0 <= p < N]] = 1
    return a


def _from_gaps(start, gaps):
    """ones at start, then one more behind every gap (zeros in between) while it fits"""
    pos, p = [start], start
    for g in gaps:
        p += g + 1
        if p >= N:
            break
        pos.append(p)
    return pos


def named_planes():
    """name -> plane (0/1).  What each is for stands in tests/test_gpu_lz4_pk16.py's table of cases."""
    out = {}
    # positions 0, 1, 4094, 4095: P holds 1, 2, 4095, 4096 and the sentinels 4097; the last one followed by nothing
    out["ends"] = _plane([0, 1, N - 2, N - 1])
    out["first"] = _plane([0])
    out["second"] = _plane([1])
    out["last"] = _plane([N - 1])
    out["single"] = _plane([2000])
    out["gap4094"] = _plane([0, N - 1])
    # a motif (2 zeros, G zeros, 2 zeros, ...) repeated: the extension meets a pair of EQUAL gaps of exactly G
    for G in (254, 255, 256):
        out["gap%d" % G] = _plane(_from_gaps(3, [2, G, 2, 7] * 8))
    out["gap4000"] = _plane([5, 9, 13, 4014, 4018, 4022, 4026])
    # periods: the extension runs past the third gap to BP_STEPS; at the end of the plane the match is cut at the match limit
    for per, cnt in ((2, 600), (3, 600), (7, 560), (13, 300), (40, 100)):
        out["period%d" % per] = _plane([N - 1 - k * per for k in range(cnt)])
        out["period%d_mid" % per] = _plane([100 + k * per for k in range(min(cnt, 300))])
    # a motif behind f1 zeros, and again behind f2 zeros: the pull-back is min(f1, f2, 64) — the candidate's front gap larger
    # than the one's and the reverse, pull-backs of 0, 63, 64 and 65 zeros
    for f1 in (0, 5, 63, 64, 65, 100):
        for f2 in (0, 63, 64, 65, 100):
            pos, p = [], 7
            for rep, f in enumerate((f1, f2, f1, f2)):
                if rep or f:
                    p += f
                for g in (3, 1 + rep % 2, 6, 2):
                    pos.append(p)
                    p += g + 1
                pos.append(p)
                p += 1
            out["front_%d_%d" % (f1, f2)] = _plane(pos)
    # two ones that share their first gap and little else: the gain of the match sweeps through -1, 0 and +1
    for g1 in (0, 1, 3, 9):
        for za in (0, 1, 3, 6):
            for zb in (0, 2, 5):
                for f in (None, 0, 2):
                    # (a one f zeros in front of the second motif bounds the pull-back; None: 39 zeros, those in front of the first)
                    a = [40, 41 + g1, 42 + g1 + zb]
                    b = [400, 401 + g1, 402 + g1 + za]
                    out["gain_%d_%d_%d_%s" % (g1, za, zb, f)] = _plane(a + ([] if f is None else [399 - f]) + b)
    # two equal candidates at different distances: ties go to the nearer
    out["tie"] = _plane(_from_gaps(10, [3, 5, 9, 20, 3, 5, 9, 30, 3, 5, 9, 40, 3, 5, 9]))
    # as many ones as the plain coder takes, and one more (the byte-wise coder gets that plane)
    out["ones636"] = _plane(_from_gaps(0, [5, 4, 6, 5, 7, 3] * 106)[:636])
    out["ones637"] = _plane(_from_gaps(0, [5, 4, 6, 5, 7, 3] * 107)[:637])
    out["ones540"] = _plane(_from_gaps(0, [6, 5, 7, 6, 8, 4] * 90)[:540])
    out["ones541"] = _plane(_from_gaps(0, [6, 5, 7, 6, 8, 4] * 91)[:541])
    return out


def with_missing(plane, every=5, shift=1):
    """every `every`-th nonzero byte becomes a missing call"""
    a = plane.copy()
    nz = np.flatnonzero(a)
    a[nz[shift::every]] = MISSING
    return a


def chunk_planes(kind, n_planes=256):
    """the chunk of a case set: the named planes in name order (kind "missing": with every fifth one a missing call, a plane's
    only one included — every fourth in the planes of the gaps around 255, whose motif has four ones: the classes repeat with the
    gaps), then the same planes shifted by 1, 2, ... positions towards the end until the chunk is full"""
    named = named_planes()
    planes, shift = [], 0
    while len(planes) < n_planes:
        for name in sorted(named):
            if len(planes) == n_planes:
                break
            a = b = named[name]
            if shift and not a[-shift:].any():      # (never drop ones: the counts at the limits must stay)
                b = np.zeros(N, np.uint8)
                b[shift:] = a[:-shift]
            every = 4 if name.startswith("gap25") else 5
            planes.append(with_missing(b, every, shift % every if np.count_nonzero(b) > shift % every else 0) if kind == "missing" else b)
        shift += 1
    return planes


# ---- the cases --------------------------------------------------------------------------------------------------------------
def cases_of(plane, recs):
    """the named cases a plane shows, from the plane itself and from what the model recorded of its candidates"""
    out = set()
    q = np.flatnonzero(plane)
    if len(q):
        for p, name in ((0, "one_at_0"), (1, "one_at_1"), (N - 2, "one_at_4094"), (N - 1, "one_at_4095")):
            if plane[p]:
                out.add(name)
        if len(q) == 1:
            out.add("single_one")
        gaps = np.diff(q) - 1
        for g in (254, 255, 256, 4000, 4094):
            if (gaps == g).any():
                out.add("gap_%d" % g)
        out.add("ones_%d" % len(q))
    for r in recs:
        if r["ga"] == r["gb"]:
            if r["ga"] == 254 and r["why"] != "ge255":
                out.add("equal_gaps_254_agree")
            if r["ga"] in (255, 256) and r["why"] == "ge255":
                out.add("equal_gaps_%d_stop" % r["ga"])
        if any(s[1] - s[0] - 1 == 254 and s[3] - s[2] - 1 == 254 for s in r["steps"][:-1]):
            out.add("equal_gaps_254_agree")
        if r["ga"] >= 3900 or r["gb"] >= 3900:
            out.add("gap_4000_in_extension")
        if r["s_end"] > 3:
            out.add("past_third_gap")
        if r["why"] == "steps":
            out.add("steps_limit")
        if r["why"] == "last_one":
            out.add("stopped_at_last_one")
        if r["why"] == "class":
            out.add("stopped_by_class")
        if r["clamped"]:
            out.add("clamped")
        if r["gq"] < r["gc"]:
            out.add("front_candidate_larger")
        if r["gq"] > r["gc"]:
            out.add("front_one_larger")
        for nbz in (0, 63, 64, 65):
            if min(r["gq"], r["gc"]) == nbz:
                out.add("pull_back_%d" % nbz)
        if r["ok"] and r["gain"] in (-1, 0, 1):
            out.add("gain_%+d" % r["gain"] if r["gain"] else "gain_0")
        if r["tie"]:
            out.add("tie_nearer_wins")
    return out
