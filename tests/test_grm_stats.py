"""CPU: the statistics behind the genetic relationship matrix — store.standardized_dosages and grm_from_sums on numpy and on
CPU torch tensors (the same bits) and against a direct float64 restatement on a random genotype matrix with missing,
half-missing and allele-2 calls; the row sums of S on complete data; top_eigenpairs' order, sign rule and refusals; the
ctypes declaration of hhgt_grm and GRM_SPAN against include/hhgt.h; np_grm_chain, the float32 chain that include/hhgt.h
states for hhgt_grm, emulated in exact float64 steps — on weights that never round, on the span case that tells a missing
or misplaced restart apart (with both wrong restatements), and on the rounding case the GPU test holds the kernel to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd.store import (AC, AN, GRM_SPAN, grm_from_sums, standardized_dosages, top_eigenpairs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bound on an entry of S relative to T = sum |x_i x_j|: a chain of 32 * GRM_SPAN fused multiply-adds in float32
# (gamma_K ~ K 2^-24) and the two float32 roundings of z in every product; the float64 additions on top are 2^-29 of that
S_BOUND = (32 * GRM_SPAN + 4) * 2.0 ** -24


def np_counts(g):
    """int8 [S, V, 2] -> int64 [V, 4]: AN, AC (the other two columns are not read here)"""
    out = np.zeros((g.shape[1], 4), np.int64)
    out[:, AN] = (g >= 0).sum((0, 2))
    out[:, AC] = (g == 1).sum((0, 2))
    return out


def np_z(counts):
    """the contract, restated variant by variant -> (z float64 [3, V], not rounded; used bool [V])"""
    z, used = np.zeros((3, len(counts))), np.zeros(len(counts), bool)
    for v, (an, ac) in enumerate(zip(counts[:, AN].tolist(), counts[:, AC].tolist())):
        if an > 0 and 0 < ac < an:
            p = np.float64(ac) / np.float64(an)
            used[v] = True
            z[:, v] = [(d - 2.0 * p) / np.sqrt(2.0 * p * (1.0 - p)) for d in (0.0, 1.0, 2.0)]
    return z, used


def np_grm_sums(g, z, take):
    """int8 [n, V, 2], z float64 [3, V], take bool [V] -> (S, T, N): float64 sums of x_i x_j and of |x_i x_j|, int64 number
    of taken variants at which both calls are complete; x = z[dosage] of a complete call (both alleles 0 or 1) at a taken
    variant, else 0"""
    a, b = g[..., 0].astype(np.int64), g[..., 1].astype(np.int64)
    m = (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1) & take[None, :]
    x = np.where(m, z[np.where(m, a + b, 0), np.arange(g.shape[1])[None, :]], 0.0)
    mi = m.astype(np.int64)
    return x @ x.T, np.abs(x) @ np.abs(x).T, mi @ mi.T


def random_genotypes(rng, S, V):
    """every frequency from rare to common, 3 % missing alleles (so whole and half-missing calls), 1 % allele 2, then a
    monomorphic variant of each kind and one nobody is called at"""
    p = rng.random(V) * 0.9 + 0.02
    g = (rng.random((S, V, 2)) < p[None, :, None]).astype(np.int8)
    g[rng.random((S, V, 2)) < 0.03] = -9
    g[rng.random((S, V, 2)) < 0.01] = 2
    g[:, 0], g[:, 1], g[:, 2] = 0, 1, -9
    g[3, 1, 0] = -9
    return g


def test_numpy_and_torch_give_the_same_bits():
    rng = np.random.default_rng(1)
    c = np_counts(random_genotypes(rng, 40, 300)).astype(np.int32)
    z, used = standardized_dosages(c)
    zt, ut = standardized_dosages(torch.from_numpy(c))
    assert z.dtype == np.float32 and z.shape == (3, 300) and used.dtype == bool and used.shape == (300,)
    assert zt.dtype == torch.float32 and ut.dtype == torch.bool
    assert np.array_equal(z.view(np.uint32), zt.numpy().view(np.uint32)) and np.array_equal(used, ut.numpy())
    S = rng.standard_normal((7, 7)) * 1000
    N = rng.integers(0, 3, (7, 7)).astype(np.int32) * 500
    assert (N == 0).any()
    a, b = grm_from_sums(S, N), grm_from_sums(torch.from_numpy(S), torch.from_numpy(N))
    assert a.dtype == np.float64 and b.dtype == torch.float64
    assert np.array_equal(np.isnan(a), N == 0) and np.array_equal(a.view(np.uint64), b.numpy().view(np.uint64))


def test_against_direct_restatement():
    rng = np.random.default_rng(2)
    g = random_genotypes(rng, 40, 300)
    counts = np_counts(g)
    z, used = standardized_dosages(counts)
    want, want_used = np_z(counts)
    assert np.array_equal(used, want_used) and not used[:3].any() and used.sum() > 250
    assert not z[:, ~used].any() and not np.signbit(z[:, ~used]).any()
    assert np.array_equal(z, want.astype(np.float32))                    # float64, rounded once
    assert (z[0, used] < 0).all() and (z[2, used] > 0).all()
    # the matrix, pair by pair, from z as rounded (both sides float64)
    z64 = z.astype(np.float64)
    S, _, N = np_grm_sums(g, z64, used)
    got = grm_from_sums(S, N)
    for i in range(0, 40, 7):
        for j in range(40):
            tot, n = 0.0, 0
            for v in np.nonzero(used)[0]:
                ci, cj = g[i, v], g[j, v]
                if set(ci.tolist()) <= {0, 1} and set(cj.tolist()) <= {0, 1}:
                    tot += z64[int(ci.sum()), v] * z64[int(cj.sum()), v]
                    n += 1
            assert n == N[i, j] and n > 0
            assert abs(got[i, j] - tot / n) <= 1e-12 * abs(tot / n), (i, j)
    assert np.array_equal(got, got.T)


def test_row_sums_vanish_on_complete_data():
    rng = np.random.default_rng(3)
    p = rng.random(300) * 0.9 + 0.05
    g = (rng.random((40, 300, 2)) < p[None, :, None]).astype(np.int8)
    z, used = standardized_dosages(np_counts(g))
    S, T, N = np_grm_sums(g, z.astype(np.float64), used)
    assert (N == used.sum()).all()
    assert (np.abs(S.sum(1)) <= S_BOUND * T.sum(1)).all()
    assert np.abs(S).max() > 100 * np.abs(S.sum(1)).max()               # (the entries themselves are not small)


def test_top_eigenpairs():
    rng = np.random.default_rng(4)
    a = rng.standard_normal((12, 30))
    g = a @ a.T / 30
    w, v = np.linalg.eigh(g)
    vals, vecs = top_eigenpairs(g, 5)
    assert vals.dtype == np.float64 and vecs.shape == (12, 5)
    assert np.array_equal(vals, w[::-1][:5])
    for c in range(5):
        col = v[:, 11 - c]
        lead = int(np.argmax(np.abs(col)))
        assert np.array_equal(vecs[:, c], col if col[lead] > 0 else -col) and vecs[lead, c] > 0
    assert np.abs(vecs.T @ vecs - np.eye(5)).max() < 1e-12
    # a tie in magnitude: the first such component decides
    _, t = top_eigenpairs(np.array([[2.0, -1.0], [-1.0, 2.0]]), 1)
    assert t[0, 0] > 0 and t[1, 0] < 0
    assert top_eigenpairs(g, 12)[1].shape == (12, 12)
    for k in (0, 13, -1):
        with pytest.raises(ValueError):
            top_eigenpairs(g, k)
    g[2, 5] = g[5, 2] = np.nan
    with pytest.raises(ValueError, match="1 pair"):
        top_eigenpairs(g, 3)


# ---- the f32 chain of hhgt_grm, restated ---------------------------------------------------------------------------------
def np_plane_values(planes, z):
    """uint32 [3, n, W] (HET, HOM_REF, HOM_ALT; they may overlap), float32 [3, 32 W] (HOM_REF, HET, HOM_ALT) -> float32
    [n, 32 W]: a row's value at every position by the header's rule — z[1] where the HET bit is set, else z[0] where
    HOM_REF is set, else z[2] where HOM_ALT is set, else 0"""
    bits = np.unpackbits(np.ascontiguousarray(planes).view(np.uint8), axis=-1, bitorder="little").astype(bool)
    return np.where(bits[0], z[1], np.where(bits[1], z[0], np.where(bits[2], z[2], np.float32(0.0)))).astype(np.float32)


def span_restarts(w_lo, w_hi):
    """the words of [w_lo, w_hi) before which the chain of hhgt_grm restarts: every multiple of GRM_SPAN counted from w_lo"""
    return range(w_lo + GRM_SPAN, w_hi, GRM_SPAN)


def chain_walk(x, ranges, paired, restarts):
    """np_grm_chain with the restarts as an argument: restarts(w_lo, w_hi) -> the words before which the chain is converted
    to float64, added to the range's float64 sum, and set to 0.  The tests of the emulator hand it wrong rules too."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] % 32 == 0
    x64 = x.astype(np.float64)
    # multiples of 2^-6 of magnitude at most 64: a product is a multiple of 2^-12 below 2^12 (24 bits), a chain of up to
    # 4096 of them a multiple of 2^-12 of magnitude at most 2^24 (the cast to float32 keeps it one), so chain + product
    # (+ product) has at most 38 bits: the float64 arithmetic of a step is exact and the cast is its only rounding
    assert np.array_equal(x64 * 64.0, np.rint(x64 * 64.0)) and np.abs(x64).max(initial=0.0) <= 64.0
    n, W = x.shape[0], x.shape[1] // 32
    table = np.zeros((n, n), np.float64)
    for w_lo, w_hi in ranges:
        assert 0 <= w_lo <= w_hi <= W
        cuts = set(restarts(w_lo, w_hi))
        chain, total = np.zeros((n, n), np.float32), np.zeros((n, n), np.float64)
        for w in range(w_lo, w_hi):
            if w in cuts:
                total += chain.astype(np.float64)
                chain = np.zeros((n, n), np.float32)
            for p in range(32 * w, 32 * w + 32, 2 if paired else 1):
                prod = np.outer(x64[:, p], x64[:, p])
                if paired:                       # (a range starts at a word: 2k and 2k + 1 of the range are p and p + 1)
                    prod += np.outer(x64[:, p + 1], x64[:, p + 1])
                chain = (chain.astype(np.float64) + prod).astype(np.float32)
        total += chain.astype(np.float64)
        table += total
    return table


def np_grm_chain(x, ranges, paired):
    """the arithmetic include/hhgt.h states for hhgt_grm, on the CPU: x float32 [n, 32 W], the rows' values (0 without a
    bit), ranges a list of (w_lo, w_hi), one per call accumulating into one table -> float64 [n, n].  Per range and pair a
    float32 chain over the positions in ascending order; at every multiple of GRM_SPAN words counted from the range's w_lo,
    and at its end, the chain is converted to float64, added to a float64 sum and restarts from 0; at the end of the range
    the sum is added to the table.  paired=False: one rounding per position, c = f32(f64(c) + f64(x_i) f64(x_j)) — fmaf.
    paired=True: the two positions of one v_mfma_f32_32x32x2_f32 enter with one rounding, c = f32(f64(c) + (p0 + p1)).
    The values must be multiples of 2^-6 of magnitude at most 64 (asserted), which with spans of 32 * GRM_SPAN = 4096 =
    2^24 / 2^12 positions makes the float64 arithmetic inside a step exact."""
    assert 32 * GRM_SPAN <= 2 ** 24 // 2 ** 12
    return chain_walk(x, ranges, paired, span_restarts)


def np_exact_ranges(x, ranges):
    """the same sums in float64: exact for chain_walk's values (below 2^26 in multiples of 2^-12 for up to 2^14 positions)"""
    x64 = np.asarray(x).astype(np.float64)
    return sum(x64[:, 32 * a:32 * b] @ x64[:, 32 * a:32 * b].T for a, b in ranges)


def quarter_values(rng, n, W):
    """float32 [n, 32 W]: multiples of 1/4 in [-2, 2], half of them 0 — no float32 step rounds"""
    return (rng.integers(-8, 9, (n, 32 * W)) * (rng.random((n, 32 * W)) < 0.5) / 4.0).astype(np.float32)


def test_chain_emulator_is_exact_on_quarters():
    rng = np.random.default_rng(11)
    for n, W, ranges in ((7, 5, [(0, 5)]), (7, 5, [(1, 4), (0, 1), (2, 2)]), (3, 131, [(0, 131)]), (3, 300, [(5, 300), (7, 136)])):
        x = quarter_values(rng, n, W)
        want = np_exact_ranges(x, ranges)
        assert np.abs(want).max() > 8
        for paired in (False, True):
            assert np.array_equal(np_grm_chain(x, ranges, paired), want), (n, W, ranges, paired)
    for bad in (np.float32(1 / 128), np.float32(64.25), np.float32(0.1)):      # finer than 2^-6, beyond 64: refused
        x = quarter_values(rng, 2, 1)
        x[1, 7] = bad
        with pytest.raises(AssertionError):
            np_grm_chain(x, [(0, 1)], False)


SPAN_W = 300                    # row words of the span case
SPAN_SUM = 2.0 ** 24 + 1.0      # its exact sum: 4096 positions of 64 * 64, then 4096 of 2^-6 * 2^-6


def span_case(w_lo, n_rows=2, plus=(0, 1), minus=()):
    """the case that tells where a chain restarts -> (planes uint32 [3, n_rows, SPAN_W], z float32 [3, 32 SPAN_W]).  The rows
    `plus` have the value 64 over the words [w_lo, w_lo + GRM_SPAN), 2^-6 over the GRM_SPAN words after them and 0
    elsewhere; the rows `minus` the same with the other sign (through the HOM_REF plane); every other row has no bit.
    A pair of such rows sums to +-(2^24 + 1) exactly — if the chain of the first span is put aside before the second
    begins: 2^24 + 2^-12 is 2^24 in float32."""
    v = np.zeros(32 * SPAN_W, np.float32)
    v[32 * w_lo:32 * (w_lo + GRM_SPAN)] = 64.0
    v[32 * (w_lo + GRM_SPAN):32 * (w_lo + 2 * GRM_SPAN)] = 2.0 ** -6
    z = np.stack([np.where(v > 0, -v, np.float32(0.0)), v, np.zeros_like(v)]).astype(np.float32)
    planes = np.zeros((3, n_rows, SPAN_W), np.uint32)
    planes[0, list(plus)] = 0xffffffff
    planes[1, list(minus)] = 0xffffffff
    return planes, z


def span_signs(n_rows, plus, minus):
    s = np.zeros(n_rows)
    s[list(plus)], s[list(minus)] = 1.0, -1.0
    return s


@pytest.mark.parametrize("w_lo", [0, 5])
def test_span_case_tells_the_restarts_apart(w_lo):
    x = np_plane_values(*span_case(w_lo))
    assert x.shape == (2, 32 * SPAN_W) and np.array_equal(x[0], x[1]) and (x[0] == 64.0).sum() == (x[0] == 2.0 ** -6).sum() == 4096
    ranges = [(w_lo, SPAN_W)]
    assert np_exact_ranges(x, ranges)[0, 1] == SPAN_SUM == 16777217.0
    never = lambda a, b: ()
    absolute = lambda a, b: [w for w in range(a + 1, b) if w % GRM_SPAN == 0]
    for paired in (False, True):
        assert np.array_equal(np_grm_chain(x, ranges, paired), np.full((2, 2), SPAN_SUM))
        # a chain that never restarts loses the second span whole: 2^24 + 2^-12 (or 2^-11) rounds to 2^24
        assert np.array_equal(chain_walk(x, ranges, paired, never), np.full((2, 2), 16777216.0))
        # restarts at absolute multiples of GRM_SPAN: right at w_lo = 0; at 5 the 123 words of 2^-12 that follow 5 words
        # of 4096 in one chain are lost: 123 * 32 * 2^-12
        lost = 0.0 if w_lo % GRM_SPAN == 0 else 0.9609375
        assert np.array_equal(chain_walk(x, ranges, paired, absolute), np.full((2, 2), SPAN_SUM - lost))
    # several rows, both signs: every pair of carrying rows, and nothing else
    rows = dict(n_rows=7, plus=(0, 3), minus=(6,))
    x = np_plane_values(*span_case(w_lo, **rows))
    s = span_signs(**rows)
    assert np.array_equal(np_grm_chain(x, ranges, False), SPAN_SUM * np.outer(s, s))


def span_splits(w_lo):
    """the calls of the span case: whole; cut between the spans, inside the first at an even and at an odd word (the second
    call's spans count from ITS w_lo: 64 or 51 words of 64 and 2^-6 then share a chain); a range of odd length"""
    return [[(w_lo, SPAN_W)], [(w_lo, w_lo + GRM_SPAN), (w_lo + GRM_SPAN, SPAN_W)], [(w_lo, w_lo + 64), (w_lo + 64, SPAN_W)],
            [(w_lo, w_lo + 77), (w_lo + 77, SPAN_W)], [(w_lo, w_lo + GRM_SPAN + 33)]]


_SPLITS = {}


def span_split_sums(w_lo):
    """np_grm_chain of a pair of rows of the span case under each of span_splits, sequential and paired: computed once"""
    if w_lo not in _SPLITS:
        x = np_plane_values(*span_case(w_lo))
        tables = [[np_grm_chain(x, ranges, paired) for paired in (False, True)] for ranges in span_splits(w_lo)]
        assert all((t == t[0, 0]).all() for pair in tables for t in pair)
        _SPLITS[w_lo] = [[float(t[0, 1]) for t in pair] for pair in tables]
    return _SPLITS[w_lo]


def test_span_case_in_several_calls():
    """what the emulator says of the split calls, by hand: a condition on the reference the GPU test compares with"""
    for w_lo in (0, 5):
        got = span_split_sums(w_lo)
        # cut at 64: 64 words of 4096 (2^23, ulp 1) and then 64 of 2^-12 in one chain, lost; the other 64 kept: + 1/2
        # cut at 77: 51 words of 4096 (51 * 2^17, ulp 1/2), 77 words of 2^-12 lost, 51 kept
        # odd length: 33 words of the second span
        assert got == [[SPAN_SUM] * 2, [SPAN_SUM] * 2, [2.0 ** 24 + 0.5] * 2, [2.0 ** 24 + 51 * 32 * 2.0 ** -12] * 2,
                       [2.0 ** 24 + 33 * 32 * 2.0 ** -12] * 2]


CHAIN_SHAPES = [(66, 131), (130, 129), (33, 257)]       # (n_rows, row_words) of the rounding case


def chain_ranges(W):
    """whole rows; both ends odd; one span and a word from an odd word (cut to the row where it is shorter than 136 words)"""
    return [(0, W), (5, W - 2), (7, min(W, 7 + 129))]


def chain_case(n_rows, row_words):
    """the rounding case: rows from random_planes, weights that are multiples of 2^-6 in [-8, 8] -> (planes, z)"""
    from tests.test_gpu_pair_counts import random_planes
    rng = np.random.default_rng(n_rows * 1000 + row_words)
    planes = random_planes(rng, n_rows, row_words)
    return planes, (rng.integers(-512, 513, (3, 32 * row_words)) / 64.0).astype(np.float32)


_CHAINS = {}


def chain_reference(n_rows, row_words, words, paired):
    """np_grm_chain of the rounding case over one range: computed once, shared by the tests, never changed"""
    key = (n_rows, row_words, words, paired)
    if key not in _CHAINS:
        _CHAINS[key] = np_grm_chain(np_plane_values(*chain_case(n_rows, row_words)), [words], paired)
        _CHAINS[key].setflags(write=False)
    return _CHAINS[key]


@pytest.mark.parametrize("n_rows,row_words", CHAIN_SHAPES)
def test_rounding_case_rounds(n_rows, row_words):
    """a condition on the reference alone: on the inputs of the GPU test most entries of the sequential chain differ from
    the exact sum and from the paired chain, so a kernel cannot equal it by not rounding, or by rounding per instruction"""
    x = np_plane_values(*chain_case(n_rows, row_words))
    T = np.abs(x.astype(np.float64))
    for words in chain_ranges(row_words):
        a, b = words
        seq, two = chain_reference(n_rows, row_words, words, False), chain_reference(n_rows, row_words, words, True)
        exact = np_exact_ranges(x, [words])
        total = T[:, 32 * a:32 * b] @ T[:, 32 * a:32 * b].T
        print(f"chain {n_rows} x {row_words} {words}: differs from exact in {(seq != exact).mean():.3f}, from paired in "
              f"{(seq != two).mean():.3f}; largest error {(np.abs(seq - exact) / total).max():.3g} T")
        assert (seq != exact).mean() >= 0.5 and (seq != two).mean() >= 0.5
        assert (np.abs(seq - exact) <= S_BOUND * total).all() and (np.abs(two - exact) <= S_BOUND * total).all()
        for t in (seq, two):
            assert np.array_equal(t.view(np.uint64), t.T.copy().view(np.uint64))       # symmetric, bit for bit


def header_prototype(name):
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    args = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src).group(1)
    return [" ".join(a.split()) for a in args.split(",")]


def test_lib_declares_hhgt_grm_as_the_header_does():
    from haplohyped_varawareml_amd import _lib, build
    build.build()
    L = _lib.load()
    args = header_prototype("hhgt_grm")
    assert args == ["hhgt_ctx *ctx", "const uint32_t *d_planes", "uint64_t n_rows", "uint64_t row_words", "uint64_t w_lo",
                    "uint64_t w_hi", "const float *d_z", "double *d_table", "void *stream"]
    want = [ctypes.c_void_p if "*" in a else {"uint64_t": ctypes.c_uint64}[a.split()[0]] for a in args]
    assert list(L.hhgt_grm.argtypes) == want
    assert header_prototype("hhgt_pair_counts")[:6] == args[:6]          # the same plane arguments as its neighbour
    src = open(os.path.join(ROOT, "include", "hhgt.h")).read()
    assert int(re.search(r"#define\s+HHGT_GRM_SPAN\s+(\d+)", src).group(1)) == GRM_SPAN == 128
    assert _lib.STAGE_NAMES[int(re.search(r"#define\s+HHGT_STAGE_GRM\s+(\d+)", src).group(1))] == "grm"
    assert int(re.search(r"#define\s+HHGT_N_STAGES\s+(\d+)", src).group(1)) == _lib.N_STAGES == len(_lib.STAGE_NAMES)
