"""Single-variant association scan of a cohort file (plink2 --glm style; linear regression, or logistic for case / control):

    python -m haplohyped_varawareml_amd.assoc --h5 OUT/C.h5 --pheno P.tsv --out O.tsv [--covar C.tsv]
        [--pcs K --ld_window W --ld_r2 T] [--min_maf X] [--chromosome N ...]
        [--model logistic [--test wald|score] [--case_control_12]]
        [--model mixed [--loco] [--grm_min_maf X] [--ld_window W --ld_r2 T]]

P.tsv and C.tsv: a header line `#IID<TAB>name...`, then one line per sample: its name and one number per column — the
format grm --pcs writes as PREFIX.eigenvec.tsv, which is therefore a valid --covar.  The samples of the scan are those of
the pheno file, in its order; a covar file lists the same set of samples, in any order.  A sample the cohort does not have,
a sample listed twice, a line of another width and a value that is not a finite number are errors.  --pcs K appends the K
largest principal components of the samples (over the same chromosomes, the variants that pass --min_maf and, with
--ld_window, the LD pruning) to the covariates; the scan itself runs over the variants that pass --min_maf.

O.tsv: the header #CHROM POS REF ALT PHENO N AF BETA SE T P, then one line per variant and phenotype, variants in
chromosome and file order: N the complete calls among the samples, AF the mean dosage of those / 2, BETA SE T P the dosage's
coefficient, its standard error, t statistic and two-sided p-value in the fit of the phenotype on [1 | covariates | dosage]
with a call that is not complete imputed to the variant's mean dosage (store.assoc_from_sums: those formulas are the
contract, not plink2's .glm.linear).  Floats are %.17g, nan where the variant is not tested.  The sums run on the device
(GenotypeStore.assoc_sums), the design and the principal components on the host.

--model logistic: every phenotype column holds 0 (control) and 1 (case) only — anything else is an error that names the
column; with --case_control_12 the columns hold 1 and 2, the coding of PLINK's .fam files, instead.  O.tsv: the header
#CHROM POS REF ALT PHENO N AF BETA SE Z P SCORE_CHI2 SCORE_P STEPS STATUS: BETA the log odds ratio per ALT allele in the
logistic regression of the phenotype on [1 | covariates | dosage], SE, Z and P its Wald test, SCORE_CHI2 and SCORE_P the score
test at the model without the variant, STEPS the Newton steps taken and STATUS one of tested, no_call, one_class, collinear,
not_converged — the six statistics are nan unless it is tested (store.logistic_fit_reference is the contract; a variant that
separates the classes is not_converged: no Firth correction is made).  --test score skips the fits and writes the score test
alone.  The fits run on the device (GenotypeStore.assoc_logistic).

--model mixed: the mixed model y = [1 | covariates] alpha + dosage beta + u + e with Var(u) = sg2 K, K the relationship matrix
of the samples over the chosen chromosomes — the variants that pass --grm_min_maf and, with --ld_window, the LD pruning —, the
variance components fixed at the null model (GCTA --mlma, EMMAX; store.mixed_null and store.mixed_from_forms are the contract).
--loco tests every chromosome against the K of the other chosen ones (GCTA --mlma-loco).  O.tsv: the header #CHROM POS REF
ALT PHENO N AF BETA SE Z P, Z^2 the chi-square on 1 df; it is a valid clump --assoc and score --weights input.  --pcs, --test
and --case_control_12 do not go with it.  The null fits run on the host, x^T M y and x^T M x of every variant on the device
(store_mixed.mixed_sums)."""
import click
import numpy as np

from . import cohort_cli as cli
from .store_stats import LOGIT_STATUS_NAMES

HEADER = "#CHROM\tPOS\tREF\tALT\tPHENO\tN\tAF\tBETA\tSE\tT\tP\n"
MIXED_HEADER = "#CHROM\tPOS\tREF\tALT\tPHENO\tN\tAF\tBETA\tSE\tZ\tP\n"
LOGISTIC_HEADER = "#CHROM\tPOS\tREF\tALT\tPHENO\tN\tAF\tBETA\tSE\tZ\tP\tSCORE_CHI2\tSCORE_P\tSTEPS\tSTATUS\n"


def read_table(path):
    """a `#IID<TAB>name...` file -> (samples, column names, float64 [n, columns]); ValueError for a bad file"""
    with open(path) as f:
        lines = [x.rstrip("\n") for x in f if x.strip()]
    if not lines or not lines[0].startswith("#IID\t"):
        raise ValueError(f"{path}: the first line must be #IID<TAB>name...")
    names = lines[0].split("\t")[1:]
    samples, rows = [], []
    for k, line in enumerate(lines[1:], 2):
        cells = line.split("\t")
        if len(cells) != 1 + len(names):
            raise ValueError(f"{path}: line {k} has {len(cells)} fields, the header {1 + len(names)}")
        try:
            row = [float(x) for x in cells[1:]]
        except ValueError:
            raise ValueError(f"{path}: line {k} holds a field that is not a number") from None
        if not np.isfinite(row).all():
            raise ValueError(f"{path}: line {k} holds a value that is not finite")
        samples.append(cells[0])
        rows.append(row)
    if len(set(samples)) != len(samples):
        raise ValueError(f"{path}: a sample is listed twice")
    return samples, names, np.array(rows, dtype=np.float64).reshape(len(samples), len(names))


def case_control(path, names, y, coded_12):
    """the phenotype table of a logistic scan as 0 / 1: its values must be 0 and 1 — or, coded_12, 1 and 2, which become 0
    and 1; ValueError that names the first column with another value"""
    lo = 1.0 if coded_12 else 0.0
    for c, name in enumerate(names):
        if not ((y[:, c] == lo) | (y[:, c] == lo + 1.0)).all():
            hint = "" if coded_12 or not ((y[:, c] == 1.0) | (y[:, c] == 2.0)).all() else " (1 / 2 coding: pass --case_control_12)"
            raise ValueError(f"{path}: column {name} holds a value other than {lo:g} and {lo + 1:g}: --model logistic takes a "
                             f"case / control phenotype{hint}")
    return y - lo


def write_tsv(reader, out, pheno, covar=None, chromosomes=None, min_maf=None, pcs=0, ld_window=None, ld_r2=0.2, model="linear",
              test="wald", case_control_12=False, loco=False, grm_min_maf=None):
    """the scan of a VCFH5Reader's cohort to the path `out`: pheno / covar the paths of the two tables"""
    samples, names, y = read_table(pheno)
    if model == "logistic":
        y = case_control(pheno, names, y, case_control_12)
    elif case_control_12 or test != "wald":
        raise ValueError("--test and --case_control_12 go with --model logistic")
    if model == "mixed" and pcs:
        raise ValueError("--pcs does not go with --model mixed: pass the components as --covar")
    if model != "mixed" and (loco or grm_min_maf is not None):
        raise ValueError("--loco and --grm_min_maf go with --model mixed")
    unknown = [s for s in samples if s not in reader.store.samples]
    if unknown:
        raise ValueError(f"{pheno}: {len(unknown)} sample(s) the cohort does not have, the first {unknown[0]}")
    cov = None
    if covar is not None:
        c_samples, _, c = read_table(covar)
        if set(c_samples) != set(samples):
            raise ValueError(f"{covar}: not the samples of {pheno}")
        at = {s: i for i, s in enumerate(c_samples)}
        cov = c[[at[s] for s in samples]]
    if model == "mixed":
        recs, _ = reader.mixed_association(y, cov, cli.ordered_chromosomes(reader, chromosomes), donor_ids=samples, min_maf=min_maf,
                                           grm_min_maf=grm_min_maf, ld_window=ld_window, ld_r2=ld_r2, loco=loco)
    else:
        recs = reader.association(y, cov, cli.ordered_chromosomes(reader, chromosomes), donor_ids=samples, min_maf=min_maf, pcs=pcs,
                                  ld_window=ld_window, ld_r2=ld_r2, model=model, test=test)
    floats = {"linear": ("af", "beta", "se", "t", "p"), "mixed": ("af", "beta", "se", "z", "p")}.get(
        model, ("af", "beta", "se", "z", "p", "score_chi2", "score_p"))
    with open(out, "w") as f:
        f.write({"linear": HEADER, "mixed": MIXED_HEADER}.get(model, LOGISTIC_HEADER))
        for v in range(len(recs[0]) if recs else 0):
            for name, rec in zip(names, recs):
                r = rec[v]
                tail = [] if model != "logistic" else [str(int(r["steps"])), LOGIT_STATUS_NAMES[int(r["status"])].replace(" ", "_")]
                f.write("\t".join([r["chrom"].decode(), str(int(r["pos"])), r["ref"].decode(), r["alt"].decode(), name,
                                   str(int(r["n"]))] + ["%.17g" % float(r[k]) for k in floats] + tail) + "\n")


def _scan_options(f):
    """the options of the scan, those of the linear model, in their order"""
    for option in reversed([cli.h5_option,
                            click.option("--pheno", required=True, type=str, help="Phenotypes: #IID<TAB>name..., one line per sample"),
                            cli.out_option("Output TSV"),
                            click.option("--covar", default=None, type=str, help="Covariates, same format (grm --pcs writes one)"),
                            click.option("--pcs", default=0, type=int, help="Append this many principal components to the covariates"),
                            cli.ld_options("LD-prune the variants of the components: counted variants back"),
                            cli.min_maf_option("Scan only variants with at least this minor allele frequency"),
                            cli.chromosome_option]):
        f = option(f)
    return f


def _scan(h5, pheno, out, covar, pcs, ld_window, ld_r2, min_maf, chromosome, model="linear", test="wald", case_control_12=False,
          loco=False, grm_min_maf=None):
    """what both commands below do with their options: write_tsv on the opened cohort, a ValueError as a usage error"""
    with cli.open_reader(h5) as r:
        try:
            write_tsv(r, out, pheno, covar, chromosomes=list(chromosome), min_maf=min_maf, pcs=pcs, ld_window=ld_window,
                      ld_r2=ld_r2, model=model, test=test, case_control_12=case_control_12, loco=loco, grm_min_maf=grm_min_maf)
        except ValueError as e:
            raise click.ClickException(str(e))


@click.command()
@_scan_options
def main(**options):
    """Regresses every phenotype of PHENO on every variant of the cohort in H5 and writes the table OUT."""
    _scan(**options)


# `main` is the linear scan with the options it has always had, for the callers that embed it (tests/test_cohort_cli.py holds
# its option list to that); the module run as a program is `scan`: the same options and the model's
@click.command(name="assoc")
@_scan_options
@click.option("--model", default="linear", type=click.Choice(["linear", "logistic", "mixed"]),
              help="linear: a quantitative phenotype; logistic: case / control, 0 / 1; mixed: quantitative, the relationship "
                   "matrix as the covariance of a random effect")
@click.option("--test", default="wald", type=click.Choice(["wald", "score"]),
              help="With --model logistic: wald fits every variant, score writes the score test alone")
@click.option("--case_control_12", is_flag=True, help="With --model logistic: the phenotypes are coded 1 / 2 (PLINK .fam), not 0 / 1")
@click.option("--loco", is_flag=True, help="With --model mixed: leave the scanned chromosome out of the relationship matrix")
@click.option("--grm_min_maf", default=None, type=float,
              help="With --model mixed: the relationship matrix runs over variants with at least this minor allele frequency")
def scan(**options):
    """Regresses every phenotype of PHENO on every variant of the cohort in H5 and writes the table OUT."""
    _scan(**options)


if __name__ == "__main__":
    scan()
