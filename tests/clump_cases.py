"""Case builders of the LD clumping tests (tests/test_clump_plan.py checks them on the CPU, tests/test_gpu_clump.py runs them
on the device): the windows that reach every lane-group width of csrc/clump.hip, strided paths whose links lie in one word
of the link bits, gadgets for the owners' minimum over a group's words, and a restatement of the rounds on the packed words
— sparse, so that it also runs where the dense np_rounds cannot, and with switches that break it on purpose: the CPU tests
prove with them that the cases notice a dropped word, a group mask or a minimum that is too wide, and the like.  Links are
carried as (k, d): variant k is linked with variant k - 1 - d, bit d % 64 of word d // 64 of row k."""
import numpy as np

# every lane-group width (LPV = 2 .. 32 lanes per variant); for 8, 16 and 32 a full group and one with idle lanes
CLUMP_WINDOWS = (64, 65, 128, 129, 192, 256, 257, 300, 448, 512, 513, 960, 1000, 1024)
# window: (nq words a side, LPV) — a literal table of what clump_words / clump_lanes of csrc/clump.hip select
CLUMP_SHAPES = {64: (1, 2), 65: (2, 4), 128: (2, 4), 129: (3, 8), 192: (3, 8), 256: (4, 8), 257: (5, 16), 300: (5, 16),
                448: (7, 16), 512: (8, 16), 513: (9, 32), 960: (15, 32), 1000: (16, 32), 1024: (16, 32)}
RANKINGS = ("identity", "reversed", "opposite")
CHAIN = 9                                # a strided case has 9 D + 1 variants: ten rounds, past the host's batch of eight


def n_words(window):
    return -(-window // 64)


def link_words(k, d, n, window):
    """the links (k, d) -> int64 [n, ceil(window / 64)], hhgt_ld_decisions' layout (d may lie past the window: a stray bit)"""
    words = np.zeros((n, n_words(window)), np.uint64)
    np.bitwise_or.at(words, (np.asarray(k, np.int64), np.asarray(d, np.int64) // 64),
                     np.uint64(1) << (np.asarray(d, np.int64) % 64).astype(np.uint64))
    return words.view(np.int64)


def link_matrix(k, d, n, window):
    """the links (k, d) -> bool [n, window]: what clump_reference and np_rounds take"""
    lb = np.zeros((n, window), bool)
    lb[np.asarray(k, np.int64), np.asarray(d, np.int64)] = True
    return lb


def links_of(words):
    """int64 [n, nq] -> (k, d) of every set bit, sorted by (k, d)"""
    u = np.ascontiguousarray(words).view(np.uint64)
    row, q = np.nonzero(u)
    vals = u[row, q]
    ks, ds = [], []
    for b in range(64):
        m = ((vals >> np.uint64(b)) & np.uint64(1)).astype(bool)
        ks.append(row[m])
        ds.append(q[m] * 64 + b)
    k, d = np.concatenate(ks).astype(np.int64), np.concatenate(ds).astype(np.int64)
    order = np.lexsort((d, k))
    return k[order], d[order]


# ---- strided paths -----------------------------------------------------------------------------------------------------------

def strided_distances(window):
    """[(q, D)]: per word q of the window the distances of its first and of its last usable bit"""
    return [(q, D) for q in range(n_words(window)) for D in sorted({64 * q + 1, min(64 * q + 64, window)})]


def strided(window, D, ranking, n=None):
    """n variants (9 D + 1 unless cut), the links exactly (k - D, k): chains of stride D, every link in word (D - 1) // 64.
    -> dict(n, window, k, d, rank, eligible, owner, rounds), owner and rounds in closed form:
    identity — rank k, all eligible: variant k = c D + r decides in round c + 1, an index where c is even;
    reversed — rank n - 1 - k: a chain resolves from its far end, c = cmax(r) is an index;
    opposite — identity, the heads k < D of odd k not eligible: an odd chain's c = 1 is an index at once and claims its head
    forward, so odd and even residues decide with opposite verdicts in every round."""
    assert 1 <= D <= window and ranking in RANKINGS
    n = CHAIN * D + 1 if n is None else n
    at = np.arange(n, dtype=np.int64)
    c, r = at // D, at % D
    k = at[D:]
    eligible = np.ones(n, np.uint8)
    if ranking == "identity":
        rank, owner = at.copy(), np.where(c % 2 == 0, at, at - D)
    elif ranking == "reversed":
        cmax = (n - 1 - r) // D
        rank, owner = n - 1 - at, np.where((cmax - c) % 2 == 0, at, at + D)
    else:
        odd = r % 2 == 1
        eligible[(at < D) & odd] = 0
        rank = at.copy()
        owner = np.where(odd, np.where(c % 2 == 1, at, at - D), np.where(c % 2 == 0, at, at - D))
        head = (at < D) & odd
        owner[head] = np.where(at[head] + D < n, at[head] + D, -1)
    return dict(n=n, window=window, k=k, d=np.full(len(k), D - 1, np.int64), rank=rank, eligible=eligible, owner=owner,
                rounds=(n - 1) // D + 1 if n else 0)


# ---- gadgets for the owners' minimum -----------------------------------------------------------------------------------------

def gadgets(window, turn):
    """per word j of the 2 nq of a variant (j < nq: back, else forward) two gadgets side by side: v, not eligible, linked
    with A in word j and with B in word j + 1 (the first gadget) or j - 1 (the second, its v one place on), modulo 2 nq; A
    and B are not linked, so both are indexes in round 1 and v's owner is the minimum over two words of its group.  Way
    (g + turn) % 3 of gadget g: 0 — rank(A) < rank(B), the owner is A; 1 — rank(A) > rank(B): B; 2 — equal ranks: the earlier
    of the two.  Over turn = 0, 1, 2 every gadget goes every way, and the two v side by side never go the same way.  Every
    other variant is eligible and linked with nothing.  No variant belongs to two gadgets.
    -> dict(n, window, k, d, rank, eligible, owner, rounds = 1, triples = [(v, A, B)])"""
    nq = n_words(window)
    span = 2 * window + 4
    n = 2 * nq * span
    usable = lambda j: min(64, window - 64 * (j % nq))                                                      # noqa: E731
    ks, ds, triples = [], [], []
    rank = np.arange(n, dtype=np.int64)                                  # (only the ranks of linked variants matter)
    eligible = np.ones(n, np.uint8)
    owner = np.arange(n, dtype=np.int64)

    def place(v, j, bit):
        d = 64 * (j % nq) + bit
        if j < nq:
            ks.append(v), ds.append(d)
            return v - 1 - d
        ks.append(v + 1 + d), ds.append(d)
        return v + 1 + d

    for j in range(2 * nq):
        for t in range(2):
            g = 2 * j + t
            v = window + 1 + j * span + t
            jb = (j + 1 - 2 * t) % (2 * nq)
            a = place(v, j, (11 * j + 5 * t + 2) % usable(j))
            b = place(v, jb, (7 * j + 3 * t + 1) % usable(jb))
            way = (g + turn) % 3
            rank[v], eligible[v] = 0, 0
            rank[a], rank[b] = 4 * g + 1 + (way == 1), 4 * g + 1 + (way == 0)
            owner[v] = (a, b, min(a, b))[way]
            triples.append((v, a, b))
    flat = [x for tr in triples for x in tr]
    assert len(set(flat)) == len(flat) and 0 <= min(flat) and max(flat) < n
    return dict(n=n, window=window, k=np.array(ks, np.int64), d=np.array(ds, np.int64), rank=rank, eligible=eligible,
                owner=owner, rounds=1, triples=triples)


# ---- the edges of the last word -----------------------------------------------------------------------------------------------

def edge_cases(window):
    """[case]: one link at exactly distance `window`, the last in reach, under the identity ranking (the earlier variant
    owns the later) and reversed; and, where the window is no multiple of 64, bits at or past `window` in the last word — d =
    window and d = 64 nq - 1 —, which count for nothing: on an eligible variant k1 (honoured, they would have it claimed), on
    one that is not eligible (k2: it would get an owner) and beside a real link at distance `window` (k3: the owner would be
    the variant one place before the real one)"""
    W = 64 * n_words(window)
    out = []
    for ranking in ("identity", "reversed"):
        n = window + 5
        at = np.arange(n, dtype=np.int64)
        owner = at.copy()
        owner[[2, window + 2]] = 2 if ranking == "identity" else window + 2
        out.append(dict(n=n, window=window, k=np.array([window + 2]), d=np.array([window - 1]), owner=owner, rounds=2,
                        rank=at if ranking == "identity" else n - 1 - at, eligible=np.ones(n, np.uint8)))
    if window % 64:
        k1 = W + 10
        k2 = k1 + W + 10
        k3 = k2 + W + 10
        n = k3 + 10
        at = np.arange(n, dtype=np.int64)
        eligible = np.ones(n, np.uint8)
        eligible[k2] = 0
        owner = at.copy()
        owner[k2], owner[k3] = -1, k3 - window
        out.append(dict(n=n, window=window, k=np.array([k1, k1, k2, k3, k3]), d=np.array([window, W - 1, window, window - 1, window]),
                        rank=at, eligible=eligible, owner=owner, rounds=2, stray=True))
    return out


# ---- the rounds on the packed words ------------------------------------------------------------------------------------------

MUTANTS = ("stray", "short", "wide_mask", "wide_min", "tie_later", "batch")


def word_rounds(words, window, rank, eligible, mutant=None):
    """hhgt_ld_clump restated on the packed words -> (owner int64 [n], rounds): a bit counts iff d < window and it points
    at a variant; word j of a variant's 2 nq (nq back, nq forward) holds its neighbours at distances 64 (j % nq) + 1 .. + 64;
    a blocker is a linked, eligible neighbour of lower rank; per round, on the state of the round before, an undecided
    variant is no index if a blocker is one, an index if no blocker is undecided; the owner of a variant that is no index
    is the linked index of lowest (rank, offset).  mutant breaks it on purpose (never the device): "stray" — bits at or past
    the window count; "short" — the last distance in reach does not; ("drop", j) — word j is never walked in the rounds,
    ("drop_owner", j) — nor by the owners; ("lanes", L) — only L lanes a variant, words j >= L are never walked;
    "wide_mask" — a verdict is taken over two neighbouring groups, "wide_min" — the owners' minimum likewise; "tie_later" —
    equal ranks go to the later variant; "batch" — rounds counted in whole batches of eight."""
    words = np.asarray(words)
    n, nq = words.shape
    rank, eligible = np.asarray(rank, np.int64), np.asarray(eligible).astype(bool)
    k, d = links_of(words)
    keep = k - 1 - d >= 0
    if mutant != "stray":
        keep &= d < (window - 1 if mutant == "short" else window)
    k, d = k[keep], d[keep]
    u = k - 1 - d
    a, b, j = np.concatenate([k, u]), np.concatenate([u, k]), np.concatenate([d // 64, nq + d // 64])        # a's word j: b
    walked = owned = np.ones(len(a), bool)
    if isinstance(mutant, tuple):
        if mutant[0] == "drop":
            walked = j != mutant[1]
        elif mutant[0] == "drop_owner":
            owned = j != mutant[1]
        else:
            walked = owned = j < mutant[1]
    blocks = walked & eligible[b] & (rank[b] < rank[a])
    pair = np.arange(n) ^ 1
    pair[pair >= n] = n - 1
    state = np.where(eligible, 0, 2)
    rounds = 0
    while True:
        has_index = np.bincount(a[blocks & (state[b] == 1)], minlength=n) > 0
        has_wait = np.bincount(a[blocks & (state[b] == 0)], minlength=n) > 0
        if mutant == "wide_mask":
            has_index, has_wait = has_index | has_index[pair], has_wait | has_wait[pair]
        new = np.where(state != 0, state, np.where(has_index, 2, np.where(has_wait, 0, 1)))
        if np.array_equal(new, state):
            break
        state, rounds = new, rounds + 1
    key = (rank << 32) | np.arange(n) if mutant != "tie_later" else (rank << 32) | (n - 1 - np.arange(n))
    best = np.full(n, np.iinfo(np.int64).max)
    m = owned & (state[b] == 1)
    np.minimum.at(best, a[m], key[b[m]])
    if mutant == "wide_min":
        best = np.minimum(best, best[pair])
    low = best & 0xFFFFFFFF
    claimed = np.where(best == np.iinfo(np.int64).max, -1, low if mutant != "tie_later" else n - 1 - low)
    owner = np.where(state == 1, np.arange(n), claimed).astype(np.int64)
    return owner, (-(-rounds // 8) * 8 if mutant == "batch" else rounds)
