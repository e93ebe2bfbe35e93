"""CPU: the burden command line — its option list, --help, the BED reader, and the refusals that come before anything is
opened (the cohort file named in them does not exist)."""
import click
import pytest
from click.testing import CliRunner

from haplohyped_varawareml_amd import cohort_cli
from haplohyped_varawareml_amd.burden import check_options, main, read_bed

# name, required, default, kind
OPTIONS = [("h5", True, None, "text"), ("regions", True, None, "text"), ("out", True, None, "text"), ("max_maf", False, 0.01, "float"),
           ("min_ac", False, 1, "integer"), ("weights", False, "count", "choice"), ("coding", False, "additive", "choice"),
           ("impute", False, "mean", "choice"), ("sample_list", False, None, "text"), ("train_sample_list", False, None, "text"),
           ("pheno", False, None, "text"), ("covar", False, None, "text"), ("pcs", False, 0, "integer"),
           ("model", False, "linear", "choice")]


def test_options():
    assert [p.name for p in main.params] == [o[0] for o in OPTIONS]
    for p, (_, required, default, kind) in zip(main.params, OPTIONS):
        assert (p.required, p.type.name) == (required, kind), p.name
        # (a required option is given no default: whatever this click makes of that)
        assert p.default == (click.Option(["--x"], required=True, type=str).default if required else default), p.name
        assert not p.is_flag and not p.multiple
    choices = {p.name: list(p.type.choices) for p in main.params if p.type.name == "choice"}
    assert choices == dict(weights=["count", "beta"], coding=["additive", "carrier"], impute=["mean", "none"],
                           model=["linear", "logistic"])
    # built from the shared options: the same --h5, --out and --sample_list as the other cohort commands
    assert cohort_cli.h5_option(lambda: None).__click_params__[0].name == "h5"


def test_help():
    res = CliRunner().invoke(main, ["--help"])
    assert res.exit_code == 0
    for opt in ("--h5", "--regions", "--out", "--max_maf", "--min_ac", "--weights", "--coding", "--impute", "--sample_list",
                "--train_sample_list", "--pheno", "--covar", "--pcs", "--model"):
        assert opt in res.output, opt


def test_read_bed(tmp_path):
    bed = tmp_path / "genes.bed"
    bed.write_text("# a comment\n#another\nchr1\t100\t200\tGENE1\n1\t150\t400\tGENE2\t0\t+\n\nchrX\t0\t0\tEMPTY\n"
                   "chr_odd\t5\t6\tG 4 \r\n")
    assert read_bed(str(bed)) == [("1", 100, 200, "GENE1"), ("1", 150, 400, "GENE2"), ("X", 0, 0, "EMPTY"), ("_odd", 5, 6, "G 4")]
    for text, what in (("chr1\t100\t200\n", "line 1"), ("chr1 100 200 G\n", "columns"), ("#x\nchr1\ta\t200\tG\n", "line 2"),
                       ("chr1\t200\t100\tG\n", "start <= end"), ("chr1\t-1\t100\tG\n", "0 <= start"), ("# nothing\n\n", "no region")):
        bed.write_text(text)
        with pytest.raises(ValueError, match=what):
            read_bed(str(bed))


def test_check_options():
    ok = dict(max_maf=0.01, min_ac=1, coding="additive", weights="count", pheno=None, covar=None, pcs=0, model="linear")
    check_options(**ok)
    check_options(**{**ok, "pheno": "p.tsv", "covar": "c.tsv", "pcs": 3, "model": "logistic", "weights": "beta"})
    check_options(**{**ok, "coding": "carrier"})
    for bad, what in ((dict(max_maf=0.6), "max_maf"), (dict(max_maf=-0.1), "max_maf"), (dict(min_ac=-1), "min_ac"),
                      (dict(coding="carrier", weights="beta"), "carrier"), (dict(pcs=-1), "pcs"), (dict(covar="c.tsv"), "--pheno"),
                      (dict(pcs=2), "--pheno"), (dict(model="logistic"), "--pheno")):
        with pytest.raises(ValueError, match=what):
            check_options(**{**ok, **bad})


def test_refusals_come_before_anything_is_opened(tmp_path):
    bed = tmp_path / "genes.bed"
    bed.write_text("chr1\t100\t200\tGENE1\n")
    base = ["--h5", str(tmp_path / "none.h5"), "--out", str(tmp_path / "o")]
    run = lambda *more: CliRunner().invoke(main, base + list(more))                                          # noqa: E731
    for args, what in ((["--regions", str(bed), "--coding", "carrier", "--weights", "beta"], "carrier"),
                       (["--regions", str(bed), "--max_maf", "0.7"], "max_maf"),
                       (["--regions", str(bed), "--pcs", "2"], "--pheno"),
                       (["--regions", str(tmp_path / "missing.bed")], "missing.bed"),
                       (["--regions", str(bed), "--sample_list", str(tmp_path / "missing.txt")], "missing.txt")):
        res = run(*args)
        assert res.exit_code == 1 and what in res.output, (args, res.output)
    bed.write_text("chr1\t100\n")
    res = run("--regions", str(bed))
    assert res.exit_code == 1 and "line 1" in res.output
    assert run("--regions", str(bed), "--weights", "skat").exit_code == 2          # (click's own refusal of a choice)
    assert run().exit_code == 2                                                     # --regions is required
    assert not list(tmp_path.glob("o*"))
