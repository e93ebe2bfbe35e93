"""Shared by tests/test_lz4_stage_model.py (CPU) and tests/test_gpu_lz4_stage_paths.py (GPU): a Python statement of how the
bit-plane LZ4 coder (csrc/lz4bits.hip) gets a plane's parse into its stream — windows of 64 ones, the queue of coded ones,
batches of at most 64 entries, the staging area — and the crafted planes on which each of those paths is taken.  The parse
itself is tests/lz4_pk16_cases.gapenc_model's (tools/sim/gapenc_ref.c in Python); this module lays its sequences out the way
the kernel does, entry by entry, and must arrive at the same bytes.  Not a test module."""
import os
import re

import numpy as np

from tests.lz4_pk16_cases import LAZY, MISSING, N, coder_constants, gapenc_model, named_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCHLIMIT, MFLIMIT = N - 5, N - 12
WINDOW, BATCH = 64, 64      # ones per window (the first holds the virtual one at -1); entries per batch
SELF_STORED = 6             # literal bytes of a first sequence that the entry's lane stores itself


def stage_constants():
    """coder_constants() and the sizes of queue and staging area (BP_QCAP, BP_STAGE and their _EXC forms), from the source"""
    K = dict(coder_constants())
    src = open(os.path.join(ROOT, "haplohyped_varawareml_amd", "csrc", "lz4bits.hip")).read()
    for name in ("BP_QCAP", "BP_STAGE", "BP_QCAP_EXC", "BP_STAGE_EXC"):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, re.M)
        assert m, name
        K[name] = int(m.group(1))
    return K


def len_ext(x):
    """extension bytes of an LZ4 length field"""
    return (x + 240) // 255


def parse_of(plane, depth, K):
    """the reference's parse of a plane, per P-index t = j + 1 (t = 0: the virtual one at -1): (P, m, hv, E, ms, off, nxt), or
    None where the plane is not the bit-plane coder's.  From gapenc_model's records (every one with a winning candidate) and,
    with the lazy bit of depth, the lazy rule applied to them as gapenc_ref.c applies it."""
    stream, recs = gapenc_model(plane, depth, K)
    if stream is None:
        return None
    q_all = [int(i) for i in np.flatnonzero(plane)]
    m = len(q_all)
    P = [0] + [i + 1 for i in q_all] + [N + 1] * 8
    hv, E, ms, off = ([0] * (m + 2) for _ in range(4))
    for t in range(m + 1):
        E[t], ms[t] = P[t], P[t] - 1          # codes itself alone: E = q + 1
    for r in recs:
        if not r["hv"]:
            continue
        t, q = r["j"] + 1, r["q"]
        jc = P.index(r["steps"][0][2]) - 1 - r["bk"]      # the candidate: the one r["bk"] in front of the first step's b side
        hv[t], E[t], ms[t], off[t] = 1, min(q + r["clen"], MATCHLIMIT), q - r["cnb"], q - (P[jc + 1] - 1)
    nxt = [0] * (m + 2)
    for t in range(m + 1):
        k = t
        while k < m and P[k + 1] - 1 < E[t]:
            k += 1
        nxt[t] = k
    if depth & LAZY:
        L = [0] * (m + 66)
        for i in range(m + 1):
            if (i & 63) == 63 or i + 1 > m or not hv[i] or not hv[i + 1] or P[i + 1] - 1 >= E[i]:
                continue
            L[i] = 1 if E[i + 1] - E[i] >= K["BP_LAZY_MIN"] + (P[i] - 1) - ms[i] + max(ms[i + 1] - P[i], 0) else 0
        give = []
        for i in range(m + 1):
            if L[i]:
                t = 0
                while (i & 63) + t < 64 and i + t <= m and L[i + t]:
                    t += 1
                if t & 1:
                    give.append(i)
        for i in give:
            hv[i], E[i], ms[i], nxt[i] = 0, P[i], P[i] - 1, i
    return P, m, hv, E, ms, off, nxt


def stage_model(plane, depth, K=None):
    """The kernel's way from the parse to the stream.  Returns None where the plane is not the bit-plane coder's, else
    (stream, windows, batches):
      windows   per window of 64 ones: dict(jw, valid, coded (lanes), qn_before, nw, qn_queued (queue length behind the window's
                entries, in front of its batches), last, reach (for every coded one with a match: ones of the NEXT window it covers))
      batches   in stream order: dict(window, make_room, n, qn, sop (staged bytes in front, before a flush), total, flushed,
                direct, entries: per lane dict(on1, on2, lit2, ll1, lits (the first sequence's literal bytes)))"""
    K = K or stage_constants()
    inb = [int(b) for b in plane]
    has_exc = MISSING in inb
    QCAP, STAGE = (K["BP_QCAP_EXC"], K["BP_STAGE_EXC"]) if has_exc else (K["BP_QCAP"], K["BP_STAGE"])
    TMIN = K["BP_TMIN"]
    pr = parse_of(plane, depth, K)
    if pr is None:
        return None
    P, m, hv, E, ms, off, nxt = pr
    out, windows, batches = [], [], []
    state = dict(prev_end=0, sop=0)
    queue = []

    def entry(t):
        e = E[t]
        rs = e + (1 if (e == 0 or inb[e - 1]) else 0)
        re_ = min(P[min(nxt[t], m) + 1] - 1, MATCHLIMIT)
        onT = re_ - rs >= TMIN and rs <= MFLIMIT
        return dict(E=e, msr=ms[t], onM=bool(hv[t]), onT=onT, rs=rs, re=re_, off=off[t])

    def put_len(seq, r):
        while r >= 255:
            seq.append(255)
            r -= 255
        seq.append(r)

    def emit_batch(n, w, make_room):
        qn = len(queue)
        assert 1 <= n <= BATCH and (n < qn or not make_room)
        lanes, total, pe = [], 0, state["prev_end"]
        for lane in range(n):
            en = queue[lane]
            onT = en["onT"]
            zt = en["re"] - en["rs"]
            nbk = 0
            if lane + 1 < qn and queue[lane + 1]["onM"] and queue[lane + 1]["msr"] <= en["re"]:
                nbk = min(en["re"] - queue[lane + 1]["msr"], zt)
            onT = onT and zt - nbk >= TMIN
            onM = en["onM"]
            on1, on2 = onM or onT, onM and onT
            seq = []
            rec = dict(on1=on1, on2=on2, lit2=False, ll1=0, lits=[])
            if on1:
                s1 = max(en["msr"], pe) if onM else en["rs"]
                e1 = en["E"] if onM else en["re"]
                ll1, ml1, off1 = s1 - pe, e1 - s1 - 4, en["off"] if onM else 1
                seq.append((min(ll1, 15) << 4) | min(ml1, 15))
                if ll1 >= 15:
                    put_len(seq, ll1 - 15)
                seq.extend(inb[pe:s1])
                seq.extend((off1 & 0xFF, off1 >> 8))
                if ml1 >= 15:
                    put_len(seq, ml1 - 15)
                rec.update(ll1=ll1, lits=inb[pe:s1])
                assert len(seq) == 3 + len_ext(ll1) + ll1 + len_ext(ml1)
                pe = e1
            if on2:
                lit2, ml2 = en["rs"] != en["E"], en["re"] - en["rs"] - 4
                seq.append((16 if lit2 else 0) | min(ml2, 15))
                if lit2:
                    seq.append(inb[en["E"]])
                seq.extend((1, 0))
                if ml2 >= 15:
                    put_len(seq, ml2 - 15)
                rec["lit2"] = lit2
                pe = en["re"]
            out.extend(seq)
            total += len(seq)
            lanes.append(rec)
        sop = state["sop"]
        flushed = sop + total > STAGE
        if flushed:
            state["sop"] = 0
        direct = total > STAGE
        if not direct:
            state["sop"] += total
        state["prev_end"] = pe
        batches.append(dict(window=w, make_room=make_room, n=n, qn=qn, sop=sop, total=total, flushed=flushed, direct=direct, entries=lanes))
        del queue[:n]

    cur = 0        # P-index of the next coded one
    for w, jw in enumerate(range(-1, m, WINDOW)):
        t0 = jw + 1
        valid = min(WINDOW, m + 1 - t0)
        coded, reach = [], []
        while cur < t0 + WINDOW and cur <= m:
            coded.append(cur - t0)
            if hv[cur]:
                reach.append(max(nxt[cur] - (t0 + WINDOW - 1), 0))
            cur = nxt[cur] + 1
        ents = [entry(t0 + lane) for lane in coded]
        ents = [e for e in ents if e["onM"] or e["onT"]]
        last = jw + WINDOW >= m
        win = dict(jw=jw, valid=valid, coded=coded, qn_before=len(queue), nw=len(ents), last=last, reach=reach)
        while len(queue) + len(ents) > QCAP:
            emit_batch(min(len(queue) - 1, BATCH), w, True)
        queue.extend(ents)
        win["qn_queued"] = len(queue)
        windows.append(win)
        while len(queue) >= BATCH + 1 or (last and queue):
            emit_batch(min(len(queue) - (0 if last else 1), BATCH), w, False)
    ll = N - state["prev_end"]
    out.append(min(ll, 15) << 4)
    if ll >= 15:
        put_len(out, ll - 15)
    out.extend(inb[state["prev_end"]:])
    return np.array(out, np.uint8), windows, batches


# ---- the cases --------------------------------------------------------------------------------------------------------------
ONES = (1, 63, 64, 65, 127, 128, 129)
STAGING = ["staged_at_0", "staged_behind", "fits_exactly", "over_by_one_flushes", "total_fills_stage", "total_one_more_direct"]
LITERALS = ["lit_run_%d" % k for k in range(8)] + ["lane63_two_sequences", "lane63_one_sequence"]
F7 = ["f7_at_%d" % k for k in range(SELF_STORED)]
SELECTION = ["lane63_hands_over"] + ["ones_%d" % m for m in ONES]
OF_MATCHES = ["reach_1", "reach_2", "reach_16"]       # (a match needs candidates: not at depth 0)
QUEUE = ["queue_fits_exactly", "queue_over_by_one", "queue_64_at_window_end", "queue_65_at_window_end", "last_window_one_entry"]


# Without candidates every sequence is a run behind a one (or behind byte 0): its literals end with that one and the zero the run
# copies, so no literal run is empty and the last self-stored byte is never a missing call; no entry has two sequences; and every
# entry takes at least 4 bytes, so two batches — at least 65 entries — never share the staging area.
NOT_AT_DEPTH_0 = ["lit_run_0", "f7_at_5", "lane63_two_sequences", "staged_behind", "fits_exactly", "over_by_one_flushes"]


# With missing calls the area holds 104 bytes.  A second batch means 65 entries; an entry emits nothing only in front of an entry
# with a match, whose sequence then carries that one as a literal (4 bytes at least): 32 x 4 bytes > 104, so there too no two
# batches share the area.
NOT_AT_104_BYTES = ["staged_behind", "fits_exactly", "over_by_one_flushes"]


def expected_cases(kind, depth):
    out = STAGING + LITERALS + SELECTION + QUEUE + (F7 if kind == "missing" else [])
    if kind == "missing":
        out = [c for c in out if c not in NOT_AT_104_BYTES]
    if depth & 0xFF:
        return out + OF_MATCHES
    return [c for c in out if c not in NOT_AT_DEPTH_0] + ["window_all_coded"]      # (all 64 ones of a window coded: depth 0 gives it)


def cases_of(plane, windows, batches, K):
    """the named cases a plane shows, from stage_model's account of it"""
    has_exc = bool((plane == MISSING).any())
    QCAP, STAGE = (K["BP_QCAP_EXC"], K["BP_STAGE_EXC"]) if has_exc else (K["BP_QCAP"], K["BP_STAGE"])
    out = {"ones_%d" % int(np.count_nonzero(plane))}
    for b in batches:
        if not b["direct"]:
            out.add("staged_at_0" if (b["sop"] == 0 or b["flushed"]) else "staged_behind")
            if b["sop"] > 0 and b["sop"] + b["total"] == STAGE:
                out.add("fits_exactly")
            if b["sop"] > 0 and b["sop"] + b["total"] == STAGE + 1:
                assert b["flushed"]
                out.add("over_by_one_flushes")
            if b["total"] == STAGE:
                out.add("total_fills_stage")
        elif b["total"] == STAGE + 1:
            out.add("total_one_more_direct")
        for e in b["entries"]:
            if e["on1"] and e["ll1"] < 8:
                out.add("lit_run_%d" % e["ll1"])
            if e["on1"] and e["ll1"] <= SELF_STORED:
                out |= {"f7_at_%d" % k for k, v in enumerate(e["lits"]) if v == MISSING}
        if b["n"] == BATCH and b["entries"][63]["on1"]:
            out.add("lane63_two_sequences" if b["entries"][63]["on2"] else "lane63_one_sequence")
        if b["qn"] == 1 and windows[b["window"]]["last"] and not b["make_room"]:
            out.add("last_window_one_entry")
    for w in windows:
        if w["valid"] == WINDOW and len(w["coded"]) == WINDOW:
            out.add("window_all_coded")
        if not w["last"] and w["coded"] and w["coded"][-1] == WINDOW - 1:
            out.add("lane63_hands_over")
        if not w["last"]:
            out |= {"reach_%d" % r for r in w["reach"] if r in (1, 2, 16)}
        if w["nw"] and w["qn_before"] + w["nw"] == QCAP:
            out.add("queue_fits_exactly")
        if w["qn_before"] + w["nw"] == QCAP + 1:
            out.add("queue_over_by_one")
        if w["qn_queued"] in (64, 65):
            out.add("queue_%d_at_window_end" % w["qn_queued"])
    return out


# ---- the planes -------------------------------------------------------------------------------------------------------------
def spec_plane(spec, kind):
    """("r", seed, m, span): m ones at seeded random places among the first `span` bytes; ("n", name): a plane of
    tests/lz4_pk16_cases.named_planes (the periodic ones: matches of BP_STEPS ones); ("f", k, g): ones 0 - 3 zeros apart in runs
    of k, g zeros between the runs (literals pile up in front of a run's sequence).  kind "missing": every fourth nonzero byte,
    counted from a remainder the spec gives, is a missing call — in an "f" plane the last one of every run"""
    a = np.zeros(N, np.uint8)
    if spec[0] == "r":
        _, seed, m, span = spec
        a[np.random.default_rng(seed).choice(span, size=m, replace=False)] = 1
        shift = seed % 4
    elif spec[0] == "n":
        a, shift = named_planes()[spec[1]].copy(), 1
    else:
        _, k, g = spec
        p, last = 3, []
        while p + 4 * k + g < N - 16:
            for i in range(k):
                a[p] = 1
                p += 1 + (i + k) % 3 if i + 1 < k else 1
            last.append(p - 1)
            p += g
        if kind == "missing":
            a[last] = MISSING
        return a
    if kind == "missing":
        nz = np.flatnonzero(a)
        a[nz[shift % len(nz)::4]] = MISSING
    return a


# the planes of the two chunks: found by a search over a few thousand such specs for the first plane that shows each case of
# expected_cases(kind, depth) at each of the depths 0, 2, 2 | LAZY, 12, 12 | LAZY.  What they show is looked up again by the test.
SPECS = {
    "plain": [
    ('r', 101550, 520, 4096),
    ('n', 'period13'), ('n', 'period2'), ('n', 'period7'), ('f', 2, 9), ('f', 3, 30), ('r', 1, 1, 4096), ('r', 5, 63, 4096),
    ('r', 7, 63, 1500), ('r', 8, 63, 1500), ('r', 9, 64, 4096), ('r', 10, 64, 4096), ('r', 11, 64, 1500),
    ('r', 12, 64, 1500), ('r', 13, 65, 4096), ('r', 17, 127, 4096), ('r', 19, 127, 1500), ('r', 20, 127, 1500),
    ('r', 21, 128, 4096), ('r', 24, 128, 1500), ('r', 25, 129, 4096), ('r', 27, 129, 1500), ('r', 65, 56, 4096),
    ('r', 89, 80, 4096), ('r', 116, 107, 4096), ('r', 117, 107, 2048), ('r', 119, 110, 4096), ('r', 125, 116, 4096),
    ('r', 137, 128, 4096), ('r', 143, 134, 4096), ('r', 145, 134, 800), ('r', 152, 156, 4096), ('r', 156, 172, 2048),
    ('r', 158, 188, 4096), ('r', 170, 252, 4096), ('r', 177, 284, 2048), ('r', 185, 332, 4096), ('r', 192, 364, 2048),
    ('r', 197, 396, 4096), ('r', 296, 98, 800), ('r', 350, 204, 800), ('r', 653, 83, 4096), ('r', 738, 284, 2048),
    ('r', 1337, 524, 2048), ('r', 1693, 396, 4096), ('r', 1706, 492, 4096), ('r', 1838, 172, 4096), ('r', 6148, 220, 4096),
    ('r', 7133, 524, 4096), ('r', 8068, 524, 4096), ('r', 16109, 524, 4096), ('r', 28054, 364, 4096),
    ],
    "missing": [
    ('n', 'period13'), ('n', 'period2_mid'), ('n', 'period3_mid'), ('n', 'period40'), ('f', 2, 30), ('f', 3, 30),
    ('f', 4, 30), ('r', 1, 1, 4096), ('r', 5, 63, 4096), ('r', 6, 63, 4096), ('r', 7, 63, 1500), ('r', 8, 63, 1500),
    ('r', 9, 64, 4096), ('r', 10, 64, 4096), ('r', 11, 64, 1500), ('r', 12, 64, 1500), ('r', 13, 65, 4096),
    ('r', 15, 65, 1500), ('r', 16, 65, 1500), ('r', 17, 127, 4096), ('r', 19, 127, 1500), ('r', 20, 127, 1500),
    ('r', 21, 128, 4096), ('r', 23, 128, 1500), ('r', 25, 129, 4096), ('r', 27, 129, 1500), ('r', 29, 20, 4096),
    ('r', 86, 77, 4096), ('r', 93, 83, 2048), ('r', 101, 92, 4096), ('r', 102, 92, 2048), ('r', 104, 95, 4096),
    ('r', 105, 95, 2048), ('r', 107, 98, 4096), ('r', 113, 104, 4096), ('r', 123, 113, 2048), ('r', 129, 119, 2048),
    ('r', 138, 128, 2048), ('r', 139, 128, 800), ('r', 145, 134, 800), ('r', 188, 348, 4096), ('r', 197, 396, 4096),
    ('r', 204, 444, 4096), ('r', 218, 20, 800), ('r', 219, 23, 4096), ('r', 494, 110, 2048),
    ],
}


def chunk_planes(kind, n_planes=256):
    """the chunk of a kind: its planes in the order of SPECS, again and again until the chunk is full"""
    distinct = [spec_plane(tuple(s), kind) for s in SPECS[kind]]
    return [distinct[i % len(distinct)] for i in range(n_planes)]
