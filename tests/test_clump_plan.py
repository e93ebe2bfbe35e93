"""CPU: the host side of LD clumping — store_stats.clump_rank / clump_reference / clump_summary and the clump command's
parser and options.  clump_reference, the contract the device route is held to, is checked against an independent brute
force (explicit set removal in sorted order) and against a numpy restatement of the round formulation that hhgt_ld_clump
runs; the conditions on the data that the GPU tests lean on are asserted here.  Also home of the helpers
tests/test_gpu_clump.py imports."""
import numpy as np
import pytest
import torch
from click.testing import CliRunner

from haplohyped_varawareml_amd import clump as clump_cli
from haplohyped_varawareml_amd import store_stats as SS
from tests.test_ld_plan import ld_genotypes, np_exceeds, np_ld_table, np_prune


# ---- helpers (imported by tests/test_gpu_clump.py) ---------------------------------------------------------------------------

def np_linked_back(table, r2, pos=None, max_dist=None):
    """LD table [n, W, 8] -> bool [n, W]: [k, d] = variant k is linked with variant k - 1 - d — np_exceeds of the pair and,
    with pos / max_dist, |pos[k] - pos[k - 1 - d]| <= max_dist; False where k - 1 - d < 0"""
    ex = np_exceeds(table, r2)
    n, window = ex.shape
    lb = np.zeros((n, window), bool)
    for d in range(window):
        k = np.arange(d + 1, n)
        lb[k, d] = ex[k - 1 - d, d]
        if pos is not None:
            lb[k, d] &= np.abs(pos[k] - pos[k - 1 - d]) <= max_dist
    return lb


def pack_bits(lb):
    """bool [n, W] -> int64 [n, ceil(W / 64)]: hhgt_ld_decisions' layout, bit d % 64 of word d // 64"""
    n, window = lb.shape
    nq = -(-window // 64)
    padded = np.zeros((n, nq * 64), np.uint64)
    padded[:, :window] = lb
    words = (padded.reshape(n, nq, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
    return words.view(np.int64)


def neighbours(lb):
    """bool [n, W] -> a list of n sets: the variants each one is linked with, on either side"""
    adj = [set() for _ in range(len(lb))]
    for k, d in zip(*np.nonzero(lb)):
        if k - 1 - d >= 0:
            adj[k].add(int(k - 1 - d))
            adj[k - 1 - d].add(int(k))
    return adj


def brute_clump(lb, p, p1):
    """the rule by explicit set removal: the variants in (p, offset) order; one that is still free and has p <= p1 becomes
    an index, leaves the free set and takes its free neighbours with it"""
    n, adj = len(p), neighbours(lb)
    free, owner = set(range(n)), [-1] * n
    for k in sorted(range(n), key=lambda k: (p[k], k)):
        if k in free and p[k] <= p1:
            for u in [k] + sorted(adj[k] & free):
                owner[u] = k
                free.discard(u)
    return np.array(owner, np.int64).reshape(n)


def np_rounds(lb, rank, eligible):
    """the round formulation of hhgt_ld_clump on dense matrices -> (owner, rounds): blockers = linked, eligible, of lower
    rank; per round, on the state of the round before, an undecided variant becomes not-index if a blocker is an index,
    index if every blocker is decided; rounds = those that decided something.  Equal ranks block neither way; among linked
    indexes the owner is the one of lowest (rank, offset)."""
    n = len(rank)
    A = np.zeros((n, n), bool)
    for k, nb in enumerate(neighbours(lb)):
        A[k, sorted(nb)] = True
    blockers = A & eligible[None, :].astype(bool) & (rank[None, :] < rank[:, None])
    state = np.where(eligible.astype(bool), 0, 2)
    rounds = 0
    while True:
        has_index = (blockers & (state == 1)[None, :]).any(1)
        has_wait = (blockers & (state == 0)[None, :]).any(1)
        new = np.where(state != 0, state, np.where(has_index, 2, np.where(has_wait, 0, 1)))
        if np.array_equal(new, state):
            break
        state, rounds = new, rounds + 1
    owner = np.full(n, -1, np.int64)
    key = rank.astype(np.int64) * (n + 1) + np.arange(n)
    for k in range(n):
        if state[k] == 1:
            owner[k] = k
        else:
            cand = np.flatnonzero(A[k] & (state == 1))
            if len(cand):
                owner[k] = cand[np.argmin(key[cand])]
    return owner, rounds


def random_p(seed, n, ties=12):
    """p in (0, 1) with planted ties: `ties` variants share the p of another one, some of them of a neighbour"""
    rng = np.random.default_rng(seed)
    p = rng.random(n)
    if n >= 4 * ties:
        src = rng.choice(n - 3, ties, replace=False)
        p[src + rng.integers(1, 4, ties)] = p[src]
    return p


S, V, SEED = 130, 600, 11
WINDOWS, R2S = (1, 7, 50, 65), (0.2, 0.5)


@pytest.fixture(scope="module")
def recipe():
    g = ld_genotypes(1, S, V)
    return {w: np_ld_table(g, w) for w in WINDOWS}


# ---- the reference against the brute force and the rounds ---------------------------------------------------------------------

@pytest.mark.parametrize("r2", R2S)
@pytest.mark.parametrize("window", WINDOWS)
def test_reference_against_brute_force_and_rounds(recipe, window, r2):
    lb = np_linked_back(recipe[window], r2)
    p = random_p(SEED, V)
    assert len(np.unique(p)) <= V - 10                                   # the ties are there
    for p1 in (1.0, 0.3):
        want = brute_clump(lb, p, p1)
        got = SS.clump_reference(lb, p, p1)
        assert got.dtype == np.int64 and np.array_equal(got, want), (window, r2, p1)
        owner, rounds = np_rounds(lb, SS.clump_rank(p), p <= p1)
        assert np.array_equal(owner, want), (window, r2, p1)
        s = SS.clump_summary(want, p)
        assert s["n_index"] + s["n_clumped_total"] + s["n_none"] == V and s["n_clumped"].sum() == s["n_clumped_total"]
        assert all(np.array_equal(want[m], np.full(len(m), i)) for i, m in zip(s["index"], s["members"]))
        assert sorted(s["best"].tolist()) == list(range(1, s["n_index"] + 1))
        assert s["index"][np.argmin(s["best"])] == min(s["index"], key=lambda k: (p[k], k))
        # the conditions on the data: a seed that fails them is the wrong seed
        largest = int(s["n_clumped"].max())
        print(f"window {window} r2 {r2} p1 {p1}: index {s['n_index']} clumped {s['n_clumped_total']} none {s['n_none']} "
              f"largest {largest} rounds {rounds}")
        if p1 == 1.0:
            assert s["n_none"] == 0
            if window >= 7:
                assert 0.3 * V <= s["n_index"] <= 0.5 * V and largest >= 5 and rounds >= 3, (window, r2)
        else:
            assert min(s["n_index"], s["n_clumped_total"], s["n_none"]) >= 0.15 * V, (window, r2)
        # no two index variants are linked; every claimed variant is linked to its owner, and to no index of lower rank
        adj, rank = neighbours(lb), SS.clump_rank(p)
        index = set(s["index"].tolist())
        for k in range(V):
            linked = adj[k] & index
            if want[k] == k:
                assert not linked and p[k] <= p1
            elif want[k] >= 0:
                assert want[k] == min(linked, key=lambda u: rank[u])
            else:
                assert not linked


# ---- the identities -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", WINDOWS)
def test_ascending_p_is_ld_prune(recipe, window):
    p = np.linspace(1e-9, 1.0, V)
    for r2 in R2S:
        owner = SS.clump_reference(np_linked_back(recipe[window], r2), p, 1.0)
        keep = np_prune(recipe[window], r2)
        assert np.array_equal(owner == np.arange(V), keep) and 0 < keep.sum() < V and (owner >= 0).all()


def test_distance_limit_is_a_narrower_window(recipe):
    pos = np.arange(V, dtype=np.int64) * 3 + 10
    p = random_p(SEED, V)
    free = np_linked_back(recipe[50], 0.2)
    for max_dist, w in ((60, 20), (6, 2), (8, 2), (0, 0)):              # 3 bp apart: 60 bp is 20 places, 6 and 8 bp are 2
        wide = np_linked_back(recipe[50], 0.2, pos, max_dist)
        narrow = np_linked_back(recipe[50][:, :max(w, 1)], 0.2) & (w > 0)
        assert np.array_equal(wide[:, :max(w, 1)], narrow) and not wide[:, w:].any()
        assert np.array_equal(SS.clump_reference(wide, p, 0.3), SS.clump_reference(narrow, p, 0.3))
    # (on this recipe nothing is linked more than 20 places apart; the limit of 2 places cuts, and changes the owners)
    cut = np_linked_back(recipe[50], 0.2, pos, 6)
    assert free[:, 2:].any() and not np.array_equal(SS.clump_reference(cut, p, 0.3), SS.clump_reference(free, p, 0.3))


# ---- special cases ------------------------------------------------------------------------------------------------------------

def test_rank_gives_ties_to_the_earlier_variant():
    p = np.array([0.5, 0.1, 0.5, 0.1, 0.0, 0.5])
    want = [3, 1, 4, 2, 0, 5]
    assert SS.clump_rank(p).tolist() == want and SS.clump_rank(p).dtype == np.int64
    t = SS.clump_rank(torch.from_numpy(p))
    assert t.dtype == torch.int64 and t.tolist() == want
    assert SS.clump_rank(np.zeros(0)).shape == (0,) and SS.clump_rank(torch.zeros(0, dtype=torch.float64)).shape == (0,)


def test_between_the_thresholds_is_never_an_index_but_is_claimed():
    # a path 0 - 1 - 2 - 3 and a loner 4; p1 = 0.01: 1 is the only index of the path, 3 and 4 lie between the thresholds
    lb = np.zeros((5, 2), bool)
    lb[1, 0] = lb[2, 0] = lb[3, 0] = True
    p = np.array([0.005, 0.001, 0.02, 0.03, 0.02])
    assert SS.clump_reference(lb, p, 0.01).tolist() == [1, 1, 1, -1, -1]
    # 0 is claimed by 1, so 0's p <= p1 makes no index of it; with 1 out of the way it is one, and claims nothing of 2's
    p[1] = 0.5
    assert SS.clump_reference(lb, p, 0.01).tolist() == [0, 0, -1, -1, -1]
    s = SS.clump_summary(np.array([1, 1, 1, -1, -1]), np.array([0.005, 0.001, 0.02, 0.03, 0.02]))
    assert s["role"].tolist() == [SS.CLUMP_CLUMPED, SS.CLUMP_INDEX, SS.CLUMP_CLUMPED, SS.CLUMP_NONE, SS.CLUMP_NONE]
    assert s["index"].tolist() == [1] and s["n_clumped"].tolist() == [2] and s["members"][0].tolist() == [0, 2]
    assert (s["n_index"], s["n_clumped_total"], s["n_none"]) == (1, 2, 2) and s["best"].tolist() == [1]


def test_empty_and_single():
    assert SS.clump_reference(np.zeros((0, 7), bool), np.zeros(0), 1.0).shape == (0,)
    assert SS.clump_reference(np.zeros((1, 7), bool), np.array([0.2]), 1.0).tolist() == [0]
    assert SS.clump_reference(np.ones((1, 7), bool), np.array([0.2]), 0.1).tolist() == [-1]
    s = SS.clump_summary(np.zeros(0, np.int64), np.zeros(0))
    assert s["n_index"] == 0 and s["members"] == [] and s["role"].shape == (0,)
    owner, rounds = np_rounds(np.zeros((1, 7), bool), np.zeros(1, np.int64), np.ones(1, bool))
    assert owner.tolist() == [0] and rounds == 1


# ---- the command line ---------------------------------------------------------------------------------------------------------

def test_cli_options():
    import click
    got = {o.name: (o.required, o.default, o.type) for o in clump_cli.main.params}
    assert list(got) == ["h5", "assoc", "out", "index_out", "pheno", "p_column", "p1", "p2", "r2", "kb", "window", "sample_list",
                         "chromosome"]
    assert [k for k, v in got.items() if v[0]] == ["h5", "assoc", "out"]
    assert {k: v[1] for k, v in got.items() if k in ("p_column", "p1", "p2", "r2", "kb", "window")} == dict(
        p_column="P", p1=1e-4, p2=1e-2, r2=0.5, kb=250.0, window=1024)
    assert got["index_out"][1] is None and got["pheno"][1] is None and got["sample_list"][1] is None
    w = got["window"][2]
    assert isinstance(w, click.IntRange) and (w.min, w.max) == (1, 1024)
    for k in ("p1", "p2", "r2"):
        t = got[k][2]
        assert isinstance(t, click.FloatRange) and (t.min, t.max) == (0.0, 1.0)
    assert next(o for o in clump_cli.main.params if o.name == "chromosome").multiple
    res = CliRunner().invoke(clump_cli.main, ["--help"])
    assert res.exit_code == 0 and "--index_out" in res.output and "--p_column" in res.output


@pytest.mark.parametrize("args", [["--window", "0"], ["--window", "1025"], ["--r2", "1.5"], ["--p1", "0.5", "--p2", "0.1"],
                                  ["--p1", "-0.1"], ["--p2", "2"]])
def test_cli_refuses_before_anything_is_opened(tmp_path, args):
    # neither file exists: a refusal that came after opening one would be another error
    res = CliRunner().invoke(clump_cli.main, ["--h5", str(tmp_path / "none.h5"), "--assoc", str(tmp_path / "none.tsv"),
                                              "--out", str(tmp_path / "o.tsv")] + args)
    assert res.exit_code == 2 and "Usage" in res.output and not (tmp_path / "o.tsv").exists()


LINEAR = "#CHROM\tPOS\tREF\tALT\tPHENO\tN\tAF\tBETA\tSE\tT\tP\n"
LOGISTIC = "#CHROM\tPOS\tREF\tALT\tPHENO\tN\tAF\tBETA\tSE\tZ\tP\tSCORE_CHI2\tSCORE_P\tSTEPS\tSTATUS\n"


def test_read_assoc(tmp_path):
    from haplohyped_varawareml_amd import assoc
    assert (LINEAR, LOGISTIC) == (assoc.HEADER, assoc.LOGISTIC_HEADER)
    f = tmp_path / "a.tsv"
    lin = ["chr7\t11\tA\tG\ty\t130\t0.25\t0.5\t0.1\t5\t1e-05", "chr7\t14\tA\tG\ty\t130\t0.25\tnan\tnan\tnan\tnan",
           "7\t17\tC\tT\ty\t130\t0.5\t-0.25\t0.1\t-2.5\t0.0125"]
    f.write_text(LINEAR + "\n".join(lin) + "\n")
    v, p, lines, head = clump_cli.read_assoc(str(f))
    assert v.tolist() == [("chr7", 11, "A", "G"), ("7", 17, "C", "T")] and p.tolist() == [1e-05, 0.0125]     # nan P: no part
    assert lines == [lin[0], lin[2]] and head == LINEAR.rstrip("\n")
    assert clump_cli.read_assoc(str(f), pheno="y")[2] == lines and clump_cli.read_assoc(str(f), p_column="AF")[1].tolist() == [0.25, 0.25, 0.5]
    # logistic, two phenotypes: --pheno is needed, and only its lines are read
    log = ["chr7\t11\tA\tG\ta\t130\t0.25\t0.5\t0.1\t5\t1e-05\t20\t1e-05\t4\ttested",
           "chr7\t11\tA\tG\tb\t130\t0.25\t0.5\t0.1\t5\t0.5\t20\t0.25\t4\ttested",
           "chr7\t14\tA\tG\ta\t130\t0\tnan\tnan\tnan\tnan\tnan\tnan\t0\tno_call",
           "chr7\t14\tA\tG\tb\t130\t0\t0.1\t0.1\t1\t0.75\t1\t0.125\t3\ttested"]
    f.write_text(LOGISTIC + "\n".join(log) + "\n")
    with pytest.raises(ValueError, match="--pheno"):
        clump_cli.read_assoc(str(f))
    v, p, lines, _ = clump_cli.read_assoc(str(f), pheno="b")
    assert v["pos"].tolist() == [11, 14] and p.tolist() == [0.5, 0.75] and lines == [log[1], log[3]]
    assert clump_cli.read_assoc(str(f), pheno="a")[1].tolist() == [1e-05]
    assert clump_cli.read_assoc(str(f), pheno="b", p_column="SCORE_P")[1].tolist() == [0.25, 0.125]
    with pytest.raises(ValueError, match="phenotype c"):
        clump_cli.read_assoc(str(f), pheno="c")
    # the errors: another width, no P column, not a number, outside [0, 1], no header
    for text, what in ((LINEAR + lin[0] + "\n" + lin[2] + "\textra\n", "line 3"), (LINEAR + lin[0].replace("1e-05", "x") + "\n", "line 2"),
                       (LINEAR + lin[0].replace("1e-05", "1.5") + "\n", "outside"), (LINEAR.replace("\tP\n", "\tQ\n") + lin[0] + "\n", "no column P"),
                       ("CHROM\tPOS\n", "first line"), ("", "first line")):
        f.write_text(text)
        with pytest.raises(ValueError, match=what):
            clump_cli.read_assoc(str(f))
    f.write_text(LINEAR)                                                 # a scan without a line is an empty one
    v, p, lines, _ = clump_cli.read_assoc(str(f))
    assert len(v) == 0 and len(p) == 0 and lines == []


# ---- the cases of tests/test_gpu_clump.py: every lane-group width, link word and round batch ---------------------------------

from tests import clump_cases as CC                                                                          # noqa: E402


def rank_reference(lb, rank, eligible):
    """clump_reference under a ranking: p = rank for the eligible, above p1 with the order kept for the others (as check_clump
    of tests/test_gpu_clump.py has it)"""
    rank, n = np.asarray(rank), len(rank)
    p = np.where(np.asarray(eligible, bool), rank, rank + 2.0 * n) / (4.0 * n + 1.0)
    return SS.clump_reference(lb, p, (n + 0.5) / (4.0 * n + 1.0))


def hold_case(case, dense=True):
    """a built case against the word model and, dense, against clump_reference and np_rounds"""
    n, window = case["n"], case["window"]
    words = CC.link_words(case["k"], case["d"], n, window)
    owner, rounds = CC.word_rounds(words, window, case["rank"], case["eligible"])
    assert np.array_equal(owner, case["owner"]) and rounds == case["rounds"], (window, np.flatnonzero(owner != case["owner"])[:5])
    if dense:
        inside = case["d"] < window                                       # (a stray bit has no place in the dense matrix)
        lb = CC.link_matrix(case["k"][inside], case["d"][inside], n, window)
        assert inside.all() == np.array_equal(pack_bits(lb), words)
        assert np.array_equal(rank_reference(lb, case["rank"], case["eligible"]), case["owner"])
        owner, rounds = np_rounds(lb, case["rank"], case["eligible"].astype(bool))
        assert np.array_equal(owner, case["owner"]) and rounds == case["rounds"]
    return words


def n_blockers(case):
    """per variant the linked, eligible variants of lower rank — and the links, read back from the packed words"""
    words = CC.link_words(case["k"], case["d"], case["n"], case["window"])
    k, d = CC.links_of(words)
    u, rank, el = k - 1 - d, case["rank"], case["eligible"].astype(bool)
    return (np.bincount(k[el[u] & (rank[u] < rank[k])], minlength=case["n"])
            + np.bincount(u[el[k] & (rank[k] < rank[u])], minlength=case["n"])), words, k, d


def test_clump_windows_reach_every_lane_group_width():
    want = [(1, 2), (2, 4), (2, 4), (3, 8), (3, 8), (4, 8), (5, 16), (5, 16), (7, 16), (8, 16), (9, 32), (15, 32), (16, 32), (16, 32)]
    assert CC.CLUMP_WINDOWS == (64, 65, 128, 129, 192, 256, 257, 300, 448, 512, 513, 960, 1000, 1024)
    assert [CC.CLUMP_SHAPES[w] for w in CC.CLUMP_WINDOWS] == want
    for w, (nq, lpv) in zip(CC.CLUMP_WINDOWS, want):                     # the table is what the rule says: the words of
        assert 64 * (nq - 1) < w <= 64 * nq                              # the window, the power of two >= 2 nq
        assert lpv & (lpv - 1) == 0 and 2 * nq <= lpv and (lpv == 2 or lpv < 4 * nq)
    assert {lpv for _, lpv in want} == {2, 4, 8, 16, 32}
    for lpv in (8, 16, 32):                                              # a full group, and one with idle lanes j >= 2 nq
        assert any(l == lpv == 2 * nq for nq, l in want) and any(l == lpv > 2 * nq for nq, l in want)
    assert {3, 7, 15} <= {nq for nq, _ in want}                          # one below a power of two


@pytest.mark.parametrize("window", CC.CLUMP_WINDOWS)
def test_strided_cases_lie_in_one_word_and_have_one_blocker(window):
    """what the GPU test leans on, for every case it runs: the links of a case lie in exactly one word, every variant that
    waits has exactly one blocker — so that word decides alone, back under the identity ranking, forward under the reversed
    one — and the closed forms are what the rounds on the packed words give (the dense references: below)"""
    nq = CC.n_words(window)
    pairs = CC.strided_distances(window)
    assert sorted({q for q, _ in pairs}) == list(range(nq)) and all(64 * q < D <= min(64 * q + 64, window) for q, D in pairs)
    assert {D for q, D in pairs if q == nq - 1} == {64 * (nq - 1) + 1, window}
    for q, D in pairs:
        for ranking in CC.RANKINGS:
            case = CC.strided(window, D, ranking)
            n = case["n"]
            assert n == 9 * D + 1 <= 9217 and case["rounds"] == 10
            blockers, words, k, d = n_blockers(case)
            assert words.nbytes < 1.2e6 and np.flatnonzero(words.any(axis=0)).tolist() == [q]
            assert np.array_equal(k, np.arange(D, n)) and (d == D - 1).all()
            at = np.arange(n)
            if ranking == "identity":
                assert np.array_equal(blockers, at >= D)
            elif ranking == "reversed":
                assert np.array_equal(blockers, at < n - D)
            else:                                                        # the second of an odd chain has none: its head is not eligible
                assert np.array_equal(blockers, (at >= D) & ~((at < 2 * D) & (at % D % 2 == 1)))
                assert (case["eligible"] == 0).sum() == D // 2
            hold_case(case, dense=False)


SMALL = tuple(w for w in CC.CLUMP_WINDOWS if w <= 300)


@pytest.mark.parametrize("window", SMALL)
def test_strided_closed_forms_small_windows(window):
    for q, D in CC.strided_distances(window):
        for ranking in CC.RANKINGS:
            hold_case(CC.strided(window, D, ranking))


@pytest.mark.parametrize("ranking", CC.RANKINGS)
@pytest.mark.parametrize("window", tuple(w for w in CC.CLUMP_WINDOWS if w > 300))
def test_strided_closed_forms_first_and_last_word(window, ranking):
    nq = CC.n_words(window)
    for q, D in CC.strided_distances(window):
        if q in (0, nq - 1):
            hold_case(CC.strided(window, D, ranking))


def test_strided_cases_cut_short():
    """the closed forms at any number of variants (the workgroup-boundary cases), chains of unequal length included"""
    for window, D in ((1, 1), (64, 3), (128, 5), (192, 7), (448, 2), (960, 3), (129, 129), (300, 257)):
        for n in (1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 65, 127, 128, 129, 257, 2 * D + 1, 3 * D - 1):
            for ranking in CC.RANKINGS:
                case = CC.strided(window, D, ranking, n=n)
                hold_case(case)
                assert case["rounds"] == (n - 1) // D + 1 and (D > 1 or case["rounds"] == n)


@pytest.mark.parametrize("window", CC.CLUMP_WINDOWS)
def test_gadgets_and_edges(window):
    """the builders against the word model at every window, against clump_reference and np_rounds at windows <= 129; every
    one of a variant's 2 nq words holds the owner of some gadget alone"""
    nq = CC.n_words(window)
    alone = set()
    for turn in range(3):
        case = CC.gadgets(window, turn)
        assert case["n"] < 150_000 and len(case["triples"]) == 4 * nq
        words = hold_case(case, dense=window <= 129)
        for g, (v, a, b) in enumerate(case["triples"]):
            assert not case["eligible"][v] and case["eligible"][a] and case["eligible"][b] and case["owner"][a] == a and case["owner"][b] == b
            assert case["owner"][v] == (a, b, min(a, b))[(g + turn) % 3]
        for j in range(2 * nq):
            got, _ = CC.word_rounds(words, window, case["rank"], case["eligible"], ("drop_owner", j))
            alone |= {(j, v) for v in np.flatnonzero(got != case["owner"])}
            assert any(v for jj, v in alone if jj == j)
    ways = {}
    for turn in range(3):                                                # every gadget goes every way; neighbours differ
        tr = CC.gadgets(window, turn)
        for g, (v, a, b) in enumerate(tr["triples"]):
            ways.setdefault(g, set()).add(int(np.sign(tr["rank"][a] - tr["rank"][b])))
            assert g % 2 or tr["triples"][g + 1][0] == v + 1
    assert all(w == {-1, 0, 1} for w in ways.values())
    for case in CC.edge_cases(window):
        hold_case(case, dense=window <= 300)
        assert (case["d"] >= window).any() == bool(case.get("stray")) and (case["d"] == window - 1).any()
    assert any(c.get("stray") for c in CC.edge_cases(window)) == (window % 64 != 0)


def test_word_model_is_the_round_model():
    """word_rounds against np_rounds on random links, variants that are not eligible among them, and with tied ranks"""
    rng = np.random.default_rng(0)
    for window in (1, 7, 65, 129, 300):
        for density in (min(0.5 / window, 0.4), min(1.5 / window, 0.6)):     # half a link a variant, and one and a half
            n = 400
            lb = rng.random((n, window)) < density
            rank = rng.permutation(n)
            eligible = rng.random(n) < 0.8
            want = np_rounds(lb, rank, eligible)
            got = CC.word_rounds(pack_bits(lb), window, rank, eligible)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] >= 2
            assert np.array_equal(want[0], rank_reference(lb, rank, eligible))
            rank[0:392:7] = rank[3:392:7]                                # equal ranks, linked ones among them, block neither
            want = np_rounds(lb, rank, eligible)                         # way (clump_rank never ties: the rounds only)
            got = CC.word_rounds(pack_bits(lb), window, rank, eligible)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] >= 2


def device_cases(window):
    """every crafted case tests/test_gpu_clump.py runs at a window (the paths and the cut cases apart)"""
    for _, D in CC.strided_distances(window):
        for ranking in CC.RANKINGS:
            yield CC.strided(window, D, ranking)
    for turn in range(3):
        yield CC.gadgets(window, turn)
    yield from CC.edge_cases(window)


def noticed(cases, mutant):
    """whether some case gives other owners or rounds under the mutant (the cases with links in the mutant's word first)"""
    first = lambda c: 0                                                                                     # noqa: E731
    if isinstance(mutant, tuple) and mutant[0] != "lanes":
        first = lambda c: not (c["d"] // 64 == mutant[1] % CC.n_words(c["window"])).any()                   # noqa: E731
    for case in sorted(cases, key=first):
        owner, rounds = CC.word_rounds(case["words"], case["window"], case["rank"], case["eligible"], mutant)
        if not np.array_equal(owner, case["owner"]) or rounds != case["rounds"]:
            return True
    return False


@pytest.mark.parametrize("window", CC.CLUMP_WINDOWS)
def test_the_cases_notice_a_broken_round_model(window):
    """mutations of the numpy model, never of the device: each one changes the owners or the rounds of some case"""
    nq, lpv = CC.CLUMP_SHAPES[window]
    cases = [dict(c, words=CC.link_words(c["k"], c["d"], c["n"], window)) for c in device_cases(window)]
    for mutant in CC.MUTANTS:
        assert noticed(cases, mutant) == (mutant != "stray" or window % 64 != 0), mutant
    for j in range(2 * nq):                                              # a word dropped in the rounds, or by the owners
        assert noticed(cases, ("drop", j)) and noticed(cases, ("drop_owner", j)), j
    for lanes in range(1, 2 * nq):                                       # the template of a narrower window: upper words idle
        assert noticed(cases, ("lanes", lanes)), lanes
    assert not noticed(cases, None) and not noticed(cases, ("lanes", 2 * nq)) and not noticed(cases, ("lanes", lpv))
