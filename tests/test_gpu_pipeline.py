"""-m gpu: files -> reader -> device pipeline -> store, through the reference's own surfaces
(parse_vcf.VCFLoader, VCFtoHDF5Converter, VCFH5Reader), against the oracle and the golden vectors."""
import gzip
import json
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import extlibs
from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd.reader import write_bgzf

pytestmark = pytest.mark.gpu


def test_facade_fixture_tuples(golden_dir, fixture_text, fixture_golden, capsys):
    import parse_vcf
    path = os.path.join(golden_dir, "chr22.filtered.vcf.gz")
    G = np.load(os.path.join(golden_dir, "fixture_G.npy"))
    for s, name in enumerate(fixture_golden["samples"]):
        rows = parse_vcf.load_vcf(path, name, "chr22")           # the spelling of vcf_to_h5.py:101
        assert len(rows) == 1000 and isinstance(rows[0], tuple) and len(rows[0]) == 7
        assert [r[5] for r in rows] == G[s, :, 0].tolist() and [r[6] for r in rows] == G[s, :, 1].tolist()
        assert all(type(v) is t for v, t in zip(rows[0], (str, int, int, str, str, int, int)))
    assert list(rows[0][:5]) == fixture_golden["first_tuple_sample0"][:5]
    assert f"Loaded 1000 SNPs for sample {name} and chromosome chr22" in capsys.readouterr().out
    sites = parse_vcf.VCFLoader().load_vcf_without_sample(path, "chr22")
    assert len(sites) == 1000 and sites[0] == tuple(fixture_golden["first_tuple_sample0"][:5])
    assert parse_vcf.VCFLoader().load_vcf(path, name) == rows                      # chrom defaults to ""
    with pytest.raises(RuntimeError, match="sample are not in the VCF"):
        parse_vcf.load_vcf(path, "nobody", "chr22")
    assert parse_vcf.load_vcf(path, name, "chr21") == []


@pytest.mark.parametrize("kind", ["gzip", "bgzf"])
def test_stream_file_small_blocks(ctx, tmp_path, kind):
    """many small text blocks: double-buffered H2D, appends across blocks and chunk columns"""
    from haplohyped_varawareml_amd.pipeline import encode_file_resident
    S, V = 500, 6000
    tab = synth.variant_table(8, V, S)
    text, _ = synth.render_fixed_numpy("chr8", tab, S, seed=8)
    p = str(tmp_path / "chr8.vcf.gz")
    if kind == "gzip":
        with gzip.open(p, "wb", compresslevel=1) as f:
            f.write(text)
    else:
        write_bgzf(p, text, level=1)
    G, start, ref, alt, fs = encode_file_resident(ctx, p, region="chr8", block_bytes=1 << 20)
    o = oracle.vcf_encode(text, S, region="chr8")
    assert fs.n_kept == V and fs.is_bgzf == (kind == "bgzf") and fs.text_bytes == len(text)
    assert np.array_equal(G.cpu().numpy(), o["G"])
    assert np.array_equal(start, o["start"]) and np.array_equal(ref, o["ref"]) and np.array_equal(alt, o["alt"])
    assert fs.chrom_runs == [(0, "chr8")]


def test_converter_end_to_end(ctx, tmp_path, golden_dir, fixture_golden):
    """vcf_to_h5 on the reference's own test inputs (tests/data/README.md 'Test VCF to HDF5 Conversion')
    plus a synthetic mixed chr4; read back through VCFH5Reader.fetch_genotypes"""
    from haplohyped_varawareml_amd.vcf_to_h5 import VCFtoHDF5Converter
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    from haplohyped_varawareml_amd.store import SNP_DTYPE
    vcf_dir = tmp_path / "vcf"
    vcf_dir.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr22.filtered.vcf.gz"), vcf_dir / "chr22.filtered.vcf.gz")
    names = fixture_golden["samples"]
    mixed = synth.render_mixed("chr4", 900, 3, seed=4, names=names)
    write_bgzf(str(vcf_dir / "chr4.filtered.vcf.gz"), mixed)
    conv = VCFtoHDF5Converter("test_cohort", str(vcf_dir), str(tmp_path / "out"),
                              os.path.join(golden_dir, "ipscs_samples_test.txt"), cores=2, cxx_threads=1, n_gpus=1,
                              keep_store=True)
    out = conv.run()
    assert out == str(tmp_path / "out" / "test_cohort.h5") == conv.h5_path      # the reference's artefact, vcf_to_h5.py:161
    store = conv.store_path
    assert os.path.isdir(store) and not os.path.exists(conv.tmp_dir)
    rd = VCFH5Reader(store, ctx=ctx)
    assert sorted(rd.store.groups()) == ["chr_22", "chr_4"]
    G22 = np.load(os.path.join(golden_dir, "fixture_G.npy"))
    o4 = oracle.vcf_encode(mixed, 3, region="chr4")
    for s, donor in enumerate(conv.donor_ids):
        rec = rd.fetch_genotypes(donor, 22)
        assert rec.dtype == SNP_DTYPE and rec.dtype.itemsize == 35 and len(rec) == 1000
        assert np.array_equal(rec["phase1"], G22[s, :, 0]) and np.array_equal(rec["phase2"], G22[s, :, 1])
        assert rec["chrom"][0] == b"chr22" and int(rec["start"][0]) == 10012121 and int(rec["stop"][0]) == 10012122
        r4 = rd.fetch_genotypes(donor, 4)
        assert len(r4) == o4["n_kept"]
        assert np.array_equal(r4["phase1"], o4["G"][s, :, 0]) and np.array_equal(r4["phase2"], o4["G"][s, :, 1])
        assert np.array_equal(r4["start"], o4["start"]) and b"".join(r4["ref"].tolist()) == bytes(o4["ref"])
    with pytest.raises(KeyError):
        rd.fetch_genotypes(conv.donor_ids[0], 5)
    # the exported HDF5 file alone serves the same records (read natively: h5file.H5Reader + GPU decode)
    rd5 = VCFH5Reader(conv.h5_path, ctx=ctx)
    assert sorted(rd5.store.groups()) == ["chr_22", "chr_4"] and rd5.store.samples == names
    for donor in conv.donor_ids:
        for chrom in (22, 4):
            a, b = rd.fetch_genotypes(donor, chrom), rd5.fetch_genotypes(donor, chrom)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # every stored chunk is a Blosc-1 frame (filter 32001) the oracle decodes to the chunk-tiled matrix bytes
    off = np.load(os.path.join(store, "chr_22", "offsets.npy"))
    raw = np.fromfile(os.path.join(store, "chr_22", "chunks.bin"), dtype=np.uint8)
    assert raw[0] == 2 and raw[3] == 2                      # Blosc-1 format version, typesize 2
    back = oracle.blosc_decompress(raw[off[0]:off[1]])
    assert back.size == 64 * 8192 * 2
    assert np.array_equal(back.view(np.int8).reshape(64, 8192, 2)[:3, :1000], G22)
    assert not back.view(np.int8).reshape(64, 8192, 2)[3:].any()
    if extlibs.have_blosc():
        assert np.array_equal(extlibs.blosc1_decompress(raw[off[0]:off[1]], back.size), back)
    # ... and OUT/{cohort}.h5 (the reference's output path, vcf_to_h5.py:161) is an HDF5 file that an independent
    # libhdf5 opens: same groups, tables, and the very same chunk bytes behind filter 32001
    assert conv.h5_path == str(tmp_path / "out" / "test_cohort.h5") and os.path.exists(conv.h5_path)
    from tests.test_h5file import h5check, have_h5py
    if have_h5py():
        got = h5check(conv.h5_path, tmp_path, "chr_22/genotype", "chr_4/genotype")
        assert [x.decode() for x in got["samples"]] == names
        meta = json.loads(str(got["chr_22/genotype|meta"]))
        assert meta["shape"] == [3, 1000, 2] and meta["chunks"] == [64, 8192, 2] and meta["filters"][0][0] == 32001
        assert meta["filters"][0][2][:4] == [2, 2, 2, 64 * 8192 * 2] and meta["n_chunks"] == 1
        assert np.array_equal(got["chr_22/genotype|chunk|0,0,0"], raw[off[0]:off[1]])
        assert int(got["chr_22/start"][0]) == 10012121 and np.array_equal(got["chr_22/stop"], got["chr_22/start"] + 1)
        assert np.array_equal(got["chr_4/start"], o4["start"]) and got["chr_4/ref"].tobytes() == bytes(o4["ref"])
        ck4 = oracle.blosc_decompress(got["chr_4/genotype|chunk|0,0,0"]).view(np.int8).reshape(64, 8192, 2)
        assert np.array_equal(ck4[:3, :o4["n_kept"]], o4["G"])
        assert [x.decode() for x in got["chr_4/chrom_run_name"]] == ["chr4"] and list(got["chr_4/chrom_run_first"]) == [0]
        # the reference's literal layout (3 donors: written by default): donor_{id}/chr_{N}/snp_data, 35-byte records
        d0 = f"donor_{conv.donor_ids[1]}/chr_22/snp_data"
        got = h5check(conv.h5_path, tmp_path, d0)
        meta = json.loads(str(got[d0 + "|meta"]))
        assert meta["shape"] == [1000] and meta["filters"][0][0] == 32001 and meta["filters"][0][2][2] == 35
        recs = oracle.blosc_decompress(got[d0 + "|chunk|0"]).view(SNP_DTYPE)[:1000]
        assert np.array_equal(recs["phase1"], G22[1, :, 0]) and np.array_equal(recs["phase2"], G22[1, :, 1])
        assert recs["chrom"][0] == b"chr22" and int(recs["start"][0]) == 10012121 and int(recs["stop"][999]) == int(recs["start"][999]) + 1
        if extlibs.have_blosc():
            assert np.array_equal(extlibs.blosc1_decompress(got[d0 + "|chunk|0"], 7488 * 35).view(SNP_DTYPE)[:1000], recs)
        # and the whole stock read path: libhdf5's filter pipeline with a c-blosc decoder registered for filter 32001
        from tests.test_h5file import build_blosc_plugin, h5read_filtered
        plugin = build_blosc_plugin(tmp_path)
        if plugin is not None:
            full = h5read_filtered(conv.h5_path, tmp_path, plugin, "chr_22/genotype", "chr_4/genotype", d0)
            assert np.array_equal(full["chr_22/genotype"], G22) and np.array_equal(full["chr_4/genotype"], o4["G"])
            assert np.array_equal(full[d0 + "|field|phase1"], G22[1, :, 0]) and np.array_equal(full[d0 + "|field|phase2"], G22[1, :, 1])
            assert full[d0 + "|field|chrom"][0] == b"chr22" and int(full[d0 + "|field|start"][0]) == 10012121


def _same_tree(a, b, skip=()):
    import filecmp
    cmp = filecmp.dircmp(a, b, ignore=list(skip))
    assert not cmp.left_only and not cmp.right_only, (cmp.left_only, cmp.right_only)
    for f in cmp.common_files:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f
    for d in cmp.common_dirs:
        _same_tree(os.path.join(a, d), os.path.join(b, d), skip)


def test_converter_two_workers_one_gpu(tmp_path, golden_dir, fixture_golden):
    """VCFtoHDF5Converter.run with two GPU worker processes (both on this box's one GPU) against the in-process
    run: identical store, identical OUT/{cohort}.h5; the default run removes the working store"""
    from haplohyped_varawareml_amd.vcf_to_h5 import VCFtoHDF5Converter
    vcf_dir = tmp_path / "vcf"
    vcf_dir.mkdir()
    shutil.copy(os.path.join(golden_dir, "chr22.filtered.vcf.gz"), vcf_dir / "chr22.filtered.vcf.gz")
    names = fixture_golden["samples"]
    write_bgzf(str(vcf_dir / "chr4.filtered.vcf.gz"), synth.render_mixed("chr4", 900, 3, seed=4, names=names))
    tab = synth.variant_table(7, 20000, 3)
    text, _ = synth.render_fixed_numpy("chr7", tab, 3, seed=7, names=names)
    write_bgzf(str(vcf_dir / "chr7.filtered.vcf.gz"), text)
    samples = os.path.join(golden_dir, "ipscs_samples_test.txt")
    one = VCFtoHDF5Converter("c", str(vcf_dir), str(tmp_path / "one"), samples, 2, 1, n_gpus=1, keep_store=True)
    two = VCFtoHDF5Converter("c", str(vcf_dir), str(tmp_path / "two"), samples, 2, 1, n_gpus=2, keep_store=True)
    assert one.run() == one.h5_path and two.run() == two.h5_path
    ranks = json.load(open(os.path.join(two.store_path, "ranks.json")))
    assert ranks["world"] == 2 and {g["rank"] for g in ranks["groups"].values()} == {0, 1}
    _same_tree(one.store_path, two.store_path, skip=["ranks.json"])
    assert open(one.h5_path, "rb").read() == open(two.h5_path, "rb").read()
    o7 = oracle.vcf_encode(text, 3, region="chr7")
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    rd = VCFH5Reader(two.h5_path)
    rec = rd.fetch_genotypes(names[2], 7)
    assert np.array_equal(rec["phase1"], o7["G"][2, :, 0]) and np.array_equal(rec["phase2"], o7["G"][2, :, 1])
    dflt = VCFtoHDF5Converter("c", str(vcf_dir), str(tmp_path / "dflt"), samples, 2, 1, n_gpus=1)
    assert dflt.run() == dflt.h5_path and not os.path.exists(dflt.store_path)
    assert open(dflt.h5_path, "rb").read() == open(one.h5_path, "rb").read()
    # without the per-donor datasets one GPU writes OUT/{cohort}.h5 directly (no store, no export): the same bytes as the
    # export of a kept store
    direct = VCFtoHDF5Converter("c", str(vcf_dir), str(tmp_path / "direct"), samples, 2, 1, n_gpus=1, donor_records=False)
    kept = VCFtoHDF5Converter("c", str(vcf_dir), str(tmp_path / "kept"), samples, 2, 1, n_gpus=1, donor_records=False, keep_store=True)
    assert direct.run() == direct.h5_path and not os.path.exists(direct.store_path)
    assert kept.run() == kept.h5_path and os.path.isdir(kept.store_path)
    assert open(direct.h5_path, "rb").read() == open(kept.h5_path, "rb").read()
    rec = VCFH5Reader(direct.h5_path).fetch_genotypes(names[2], 7)
    assert np.array_equal(rec["phase1"], o7["G"][2, :, 0]) and np.array_equal(rec["phase2"], o7["G"][2, :, 1])


def test_converter_on_gatk_shaped_cohort(ctx, tmp_path):
    """VCFtoHDF5Converter on a GATK-shaped file (GT:AD:DP:GQ:PL columns whose width varies by kilobytes) of 800 samples:
    the line index walks it in one pass per block, and the stored genotypes are the oracle's"""
    from haplohyped_varawareml_amd.store import GenotypeStore
    from haplohyped_varawareml_amd.vcf_to_h5 import VCFtoHDF5Converter
    from tests.gatk_text import gatk_text
    S = 800
    names = synth.sample_names(S)
    text, _ = gatk_text(np.random.default_rng(11), S, 12 << 20, contig="chr3", names=names)
    vcf_dir = tmp_path / "vcf"
    vcf_dir.mkdir()
    write_bgzf(str(vcf_dir / "chr3.filtered.vcf.gz"), text)
    sl = tmp_path / "samples.txt"
    sl.write_text("\n".join(names))
    conv = VCFtoHDF5Converter("c", str(vcf_dir), str(tmp_path / "out"), str(sl), 2, 1, n_gpus=1, donor_records=False,
                              keep_store=True)
    conv.run()
    o = oracle.vcf_encode(text, S, region="chr3")
    st = GenotypeStore(conv.store_path, ctx=ctx)
    assert st.meta["groups"]["chr_3"]["n_variants"] == o["n_kept"]
    for s in (0, 1, 399, 799):
        assert np.array_equal(st.sample_row("chr_3", names[s]), o["G"][s]), names[s]


def test_header_only_chromosome(ctx, tmp_path, fixture_golden):
    """a chromosome file with a header and no record: an empty group that neither the store nor the .h5 trips over"""
    from haplohyped_varawareml_amd.vcf_to_h5 import VCFtoHDF5Converter
    from haplohyped_varawareml_amd.h5_reader import VCFH5Reader
    vcf_dir = tmp_path / "vcf"
    vcf_dir.mkdir()
    names = ["A", "B"]
    write_bgzf(str(vcf_dir / "chr3.filtered.vcf.gz"), synth.header_text("chr3", names))
    tab = synth.variant_table(5, 500, 2)
    text, _ = synth.render_fixed_numpy("chr5", tab, 2, seed=5, names=names)
    write_bgzf(str(vcf_dir / "chr5.filtered.vcf.gz"), text)
    sl = tmp_path / "s.txt"
    sl.write_text("A\nB")
    conv = VCFtoHDF5Converter("c", str(vcf_dir), str(tmp_path / "out"), str(sl), 2, 1, n_gpus=1, keep_store=True)
    conv.run()
    o5 = oracle.vcf_encode(text, 2, region="chr5")
    for path in (conv.store_path, conv.h5_path):
        rd = VCFH5Reader(path, ctx=ctx)
        assert sorted(rd.store.groups()) == ["chr_3", "chr_5"]
        assert len(rd.fetch_genotypes("A", 3)) == 0
        rec = rd.fetch_genotypes("B", 5)
        assert np.array_equal(rec["phase1"], o5["G"][1, :, 0]) and np.array_equal(rec["start"], o5["start"])


def test_load_vcf_from_threads(golden_dir, fixture_golden):
    """the reference calls load_vcf from ThreadPoolExecutor workers (vcf_to_h5.py:191-192)"""
    from concurrent.futures import ThreadPoolExecutor
    import parse_vcf
    from haplohyped_varawareml_amd import parse_vcf as impl
    impl._CACHE.clear()
    path = os.path.join(golden_dir, "chr22.filtered.vcf.gz")
    G = np.load(os.path.join(golden_dir, "fixture_G.npy"))
    names = fixture_golden["samples"]
    jobs = [(s, r) for r in ("chr22", "chr22:10000000-15000000", "") for s in range(3)] * 2
    with ThreadPoolExecutor(6) as ex:
        got = list(ex.map(lambda j: parse_vcf.load_vcf(path, names[j[0]], j[1]), jobs))
    for (s, r), rows in zip(jobs, got):
        want = parse_vcf.load_vcf(path, names[s], r)
        assert rows == want
        if r in ("chr22", ""):
            assert [t[5] for t in rows] == G[s, :, 0].tolist() and [t[6] for t in rows] == G[s, :, 1].tolist()
