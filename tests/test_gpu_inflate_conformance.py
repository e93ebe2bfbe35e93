"""-m gpu: the device inflater (`k_inflate_members`, csrc/inflate.hip) on crafted DEFLATE streams (tests/deflate_craft.py)
and on BGZF files written by libdeflate, as htslib's bgzip writes them when it links it.

Bar: every valid member byte-exact with status 0 (CRC-32 checked); every invalid member with exactly the status the
corpus names (include/hhgt.h), zlib being the arbiter of what is invalid; no byte written outside a member's slice of the
destination, whose slices sit between 0xA5 guard gaps."""
import zlib

import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd import synth
from tests import deflate_craft as dc
from tests import extlibs

pytestmark = pytest.mark.gpu

CASES = dc.corpus()
GUARD = 0xA5


def interleaved(cases):
    good = [c for c in cases if c.status == dc.OK]
    bad = [c for c in cases if c.status != dc.OK]
    out = []
    for i in range(max(len(good), len(bad))):
        out += good[i:i + 1] + bad[i:i + 1]
    return out


def inflate_cases(ctx, cases, seed=0):
    """one `inflate_members` launch over `cases`: payloads at offsets of every alignment with junk between them, each
    member's output slice between guard gaps of 0xA5.  -> (status per case, dst as numpy, out_off, gaps)"""
    rng = np.random.default_rng(seed)
    src = bytearray()
    comp_off, comp_len, out_off, isize, crc = [], [], [], [], []
    gaps, pos = [], 0
    for k, c in enumerate(cases):
        src += bytes(rng.integers(0, 256, size=k % 4 + 4 * int(rng.integers(0, 3)), dtype=np.uint8))
        comp_off.append(len(src))
        comp_len.append(len(c.payload))
        src += c.payload
        g = 16 + int(rng.integers(0, 200))
        gaps.append((pos, pos + g))
        pos += g
        out_off.append(pos)
        isize.append(c.isize)
        crc.append(zlib.crc32(c.text) & 0xFFFFFFFF)
        pos += c.isize
    gaps.append((pos, pos + 64))
    total = pos + 64
    src += bytes(rng.integers(0, 256, size=(-len(src)) % 4 + 4, dtype=np.uint8))
    dv = ctx.device
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).to(dv)
    d_src = t(np.frombuffer(bytes(src), np.uint8), np.uint8)
    dst = torch.full((total,), GUARD, dtype=torch.uint8, device=dv)
    status = torch.full((len(cases),), 0x7777, dtype=torch.int32, device=dv)
    n_bad = ctx.inflate_members(d_src, len(src), t(comp_off, np.uint64), t(comp_len, np.uint32), t(out_off, np.uint64),
                                t(isize, np.uint32), len(cases), dst, total, status, d_crc32=t(crc, np.uint32))
    st = status.cpu().numpy()
    assert n_bad == int((st != 0).sum())
    return st, dst.cpu().numpy(), out_off, gaps


def verdicts(cases, st, out, out_off, gaps):
    """-> list of problems, one line per case that is wrong"""
    probs = []
    for (a, b) in gaps:
        if not (out[a:b] == GUARD).all():
            i = a + int(np.flatnonzero(out[a:b] != GUARD)[0])
            probs.append(f"guard byte {i} overwritten (gap {a}..{b})")
    for c, s, o in zip(cases, st.tolist(), out_off):
        if c.status == dc.OK:
            if s != 0:
                probs.append(f"{c.name}: status {s}, valid stream")
            elif out[o:o + c.isize].tobytes() != c.text:
                probs.append(f"{c.name}: wrong bytes")
        elif c.status == dc.ANY:
            if s == 0:
                probs.append(f"{c.name}: status 0, truncated stream")
        elif s != c.status:
            probs.append(f"{c.name}: status {s}, want {c.status}")
    return probs


def test_corpus_in_one_launch(ctx):
    cases = interleaved(CASES)
    st, out, off, gaps = inflate_cases(ctx, cases, seed=1)
    probs = verdicts(cases, st, out, off, gaps)
    assert not probs, "\n".join(probs)
    # and again in another order, at other offsets
    cases = cases[::-1]
    st, out, off, gaps = inflate_cases(ctx, cases, seed=2)
    probs = verdicts(cases, st, out, off, gaps)
    assert not probs, "\n".join(probs)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_alone(ctx, case):
    st, out, off, gaps = inflate_cases(ctx, [case], seed=3)
    probs = verdicts([case], st, out, off, gaps)
    assert not probs, "\n".join(probs)


# ---- BGZF written by libdeflate ----
needs_libdeflate = pytest.mark.skipif(not extlibs.have_libdeflate(), reason="libdeflate is not loadable on this box")


def _inputs():
    rng = np.random.default_rng(31)
    S = 120
    text, _ = synth.render_fixed_numpy("chr2", synth.variant_table(2, 700, S), S, seed=2)
    skew = rng.choice(np.frombuffer(b"0|1\t.\n", np.uint8), size=150_000, p=[0.7, 0.1, 0.1, 0.05, 0.03, 0.02])
    runs = b"".join(bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 3000)) for _ in range(120))
    return {"vcf": bytes(text), "random": bytes(rng.integers(0, 256, size=140_000, dtype=np.uint8)),
            "skewed": skew.astype(np.uint8).tobytes(), "runs": runs}


@needs_libdeflate
@pytest.mark.parametrize("level", list(range(13)))
def test_libdeflate_bgzf_every_level(ctx, level):
    for name, text in _inputs().items():
        for block in (0xFF00, 300):             # bgzip's members, and small ones (fixed-Huffman blocks)
            data = text if block == 0xFF00 else text[:60_000]
            raw = extlibs.bgzf_libdeflate(data, level, block_size=block)
            got, bad, status = ctx.inflate_bgzf(raw, return_status=True)
            st = status.cpu().numpy()
            assert bad == 0, (name, block, np.flatnonzero(st)[:8], st[st != 0][:8])
            assert got.cpu().numpy().tobytes() == data, (name, block)


@needs_libdeflate
def test_stream_file_of_a_libdeflate_file(ctx, tmp_path):
    """the converter's streaming path reads a libdeflate-written file the same with either inflater"""
    from haplohyped_varawareml_amd import pipeline
    S = 300
    tab = synth.variant_table(23, 9000, S)
    text_dev, _ = ctx.synth_fixed("chr1", tab, S, seed=23)
    path = tmp_path / "ld.vcf.gz"
    extlibs.write_bgzf_libdeflate(str(path), text_dev.cpu().numpy().tobytes(), level=6)
    res = {}
    for mode in (False, True):
        cols, tabs = [], []
        fs = pipeline.stream_file(ctx, str(path), sc=64, vc=512, block_bytes=6 << 20, compress=False, device_inflate=mode,
                                  on_columns=lambda G, n, framed: cols.append(G.cpu().numpy().copy()),
                                  on_variants=lambda st, r, a: tabs.append((st.copy(), r.copy(), a.copy())))
        res[mode] = (fs, np.concatenate(cols), [np.concatenate([t[i] for t in tabs]) for i in range(3)])
    (fh, Gh, vh), (fd, Gd, vd) = res[False], res[True]
    assert fd.is_bgzf and fd.n_kept == fh.n_kept == 9000 and fd.n_lines == fh.n_lines and fd.text_bytes == fh.text_bytes
    assert np.array_equal(Gh, Gd)
    for a, b in zip(vh, vd):
        assert np.array_equal(a, b)

