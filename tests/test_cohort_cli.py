"""CPU: the command-line surface of the six cohort tools — allele_freq, sample_stats, kinship, ld_prune, grm, assoc —,
option by option as it stood before they shared cohort_cli (name, required, default, multiple, type, in order), their
--help, the arguments they refuse before they open anything, and cohort_cli.variant_lines against literal text."""
import importlib

import click
import numpy as np
import pytest
from click.testing import CliRunner

from haplohyped_varawareml_amd import allele_freq, cohort_cli, ld_prune
from haplohyped_varawareml_amd.store import AC, AN, HET, HOM_ALT

NONE = "no default declared"            # (click's own placeholder for that differs from version to version)
STR, FLOAT, INT = click.STRING, click.FLOAT, click.INT
H5, OUT = ("h5", True, NONE, False, STR), ("out", True, NONE, False, STR)
SAMPLE_LIST, CHROMOSOME = ("sample_list", False, None, False, STR), ("chromosome", False, NONE, True, STR)
REGION, MIN_MAF = ("region", False, None, False, STR), ("min_maf", False, None, False, FLOAT)
LD_WINDOW, LD_R2 = ("ld_window", False, None, False, INT), ("ld_r2", False, 0.2, False, FLOAT)
# (name, required, default, multiple, type)
OPTIONS = dict(
    allele_freq=[H5, OUT, SAMPLE_LIST, CHROMOSOME, REGION],
    sample_stats=[H5, OUT, SAMPLE_LIST, CHROMOSOME, REGION, MIN_MAF, ("singletons", False, False, False, click.BOOL)],
    kinship=[H5, OUT, SAMPLE_LIST, CHROMOSOME, MIN_MAF, ("min_kinship", False, None, False, FLOAT)],
    ld_prune=[H5, OUT, SAMPLE_LIST, CHROMOSOME, MIN_MAF, ("window", False, 50, False, (click.IntRange, 1, 1024)),
              ("r2", False, 0.2, False, (click.FloatRange, 0.0, 1.0))],
    grm=[H5, OUT, SAMPLE_LIST, CHROMOSOME, MIN_MAF, LD_WINDOW, LD_R2, ("pcs", False, None, False, INT)],
    assoc=[H5, ("pheno", True, NONE, False, STR), OUT, ("covar", False, None, False, STR), ("pcs", False, 0, False, INT),
           LD_WINDOW, LD_R2, MIN_MAF, CHROMOSOME])


def main_of(name):
    return importlib.import_module("haplohyped_varawareml_amd." + name).main


@pytest.mark.parametrize("name", list(OPTIONS))
def test_options_are_those_of_before(name):
    params = main_of(name).params
    assert [p.name for p in params] == [o[0] for o in OPTIONS[name]]
    for p, (_, required, default, multiple, kind) in zip(params, OPTIONS[name]):
        assert isinstance(p, click.Option) and (p.required, p.multiple) == (required, multiple), p.name
        if default is NONE:
            assert p.default == click.Option(["--x"], required=required, multiple=multiple, type=str).default, p.name
        else:
            assert p.default == default and type(p.default) is type(default), p.name
        if isinstance(kind, tuple):
            assert type(p.type) is kind[0] and (p.type.min, p.type.max) == kind[1:], p.name
            assert not p.type.min_open and not p.type.max_open and not p.type.clamp
        else:
            assert type(p.type) is type(kind), p.name
    assert [p.name for p in params if p.is_flag] == [o[0] for o in OPTIONS[name] if o[0] == "singletons"]


@pytest.mark.parametrize("name", list(OPTIONS))
def test_help(name):
    res = CliRunner().invoke(main_of(name), ["--help"])
    assert res.exit_code == 0 and all("--" + o[0] in res.output for o in OPTIONS[name])


@pytest.mark.parametrize("name", ["allele_freq", "sample_stats"])
def test_region_excludes_chromosome_before_anything_is_opened(name, tmp_path):
    out = tmp_path / "out.tsv"
    res = CliRunner().invoke(main_of(name), ["--h5", str(tmp_path / "none.h5"), "--out", str(out), "--region", "x",
                                             "--chromosome", "1"])
    assert res.exit_code == 2 and "--region and --chromosome are exclusive" in res.output and not out.exists()


@pytest.mark.parametrize("bad", [["--window", "0"], ["--window", "1025"], ["--r2", "1.5"], ["--r2", "-0.1"]])
def test_ld_prune_refuses_window_and_r2_out_of_range(bad, tmp_path):
    res = CliRunner().invoke(main_of("ld_prune"), ["--h5", str(tmp_path / "none.h5"), "--out", str(tmp_path / "o")] + bad)
    assert res.exit_code == 2 and bad[0] in res.output


def test_variant_lines():
    assert cohort_cli.variant_lines([], [], [], []) == ""
    assert cohort_cli.variant_lines([], [], [], [], np.zeros(0, "U1")) == ""
    chrom, pos = np.array(["chr5", "chr5", "chrX"]), np.array([10177, 10235, 155270560])
    want = "chr5\t10177\tA\tG\nchr5\t10235\tC\tT\nchrX\t155270560\tG\tA\n"
    assert cohort_cli.variant_lines(chrom, pos, np.frombuffer(b"ACG", np.uint8), np.frombuffer(b"GTA", np.uint8)) == want
    assert cohort_cli.variant_lines(chrom, pos, np.array([b"A", b"C", b"G"]), np.array([b"G", b"T", b"A"])) == want
    assert cohort_cli.variant_lines(list(chrom), list(pos), np.frombuffer(b"ACG", np.uint8), np.array([b"G", b"T", b"A"]),
                                    np.array(["1", "22", "333"]), np.array(["NA", "0.5", "x"])) == (
        "chr5\t10177\tA\tG\t1\tNA\nchr5\t10235\tC\tT\t22\t0.5\nchrX\t155270560\tG\tA\t333\tx\n")


def test_both_format_rows_go_through_it():
    chrom, pos = np.array(["chr5", "chr5", "chr5", "chrX"]), np.array([10177, 10235, 10352, 155270560])
    ref, alt = np.frombuffer(b"ACGT", np.uint8), np.array([b"G", b"T", b"A", b"C"])
    counts = np.zeros((4, 4), np.int64)
    counts[:, AN], counts[:, AC], counts[:, HET] = [2000, 0, 3, 1998], [1, 0, 1, 1998], [1, 0, 1, 0]
    counts[:, HOM_ALT] = [0, 0, 0, 999]
    assert allele_freq.format_rows(chrom, pos, ref, alt, counts) == ("chr5\t10177\tA\tG\t1\t2000\t0.0005\t1\t0\n"
                                                                      "chr5\t10235\tC\tT\t0\t0\tNA\t0\t0\n"
                                                                      "chr5\t10352\tG\tA\t1\t3\t0.333333\t1\t0\n"
                                                                      "chrX\t155270560\tT\tC\t1998\t1998\t1\t0\t999\n")
    assert ld_prune.format_rows(chrom, pos, ref, alt) == ("chr5\t10177\tA\tG\nchr5\t10235\tC\tT\nchr5\t10352\tG\tA\n"
                                                          "chrX\t155270560\tT\tC\n")
    assert allele_freq.format_rows([], [], [], [], np.zeros((0, 4))) == "" == ld_prune.format_rows([], [], [], [])
    # the shared names stay importable from allele_freq
    assert allele_freq.parse_region is cohort_cli.parse_region and allele_freq.read_sample_list is cohort_cli.read_sample_list
    assert allele_freq.ordered_chromosomes is cohort_cli.ordered_chromosomes
